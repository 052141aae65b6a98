"""Characterisation of the grouped expert GEMM's host layer (csrc/moe_gemm.hip, moe_gemm_f16.hip, moe_gemm_bwd.hip): the status code of every
answer the four entry points dimsum_moe_gemm, dimsum_moe_gemm_f16s, dimsum_moe_gemm_dgrad and dimsum_moe_gemm_wgrad can give before a kernel is
launched. The codes were recorded from the library BEFORE the four entries were put on one shared set of host helpers and are kept verbatim: a
refactor of that layer has to reproduce them.

CPU-only. Every pointer is a made-up, suitably aligned host address that is never read, and nothing is launched: a case is either refused (a
status that is neither DIMSUM_OK nor DIMSUM_ERR_LAUNCH) or an empty call (tokens == 0), which returns DIMSUM_OK after the shape checks and before
any pointer is looked at. So an ACCEPTED width is shown by the empty call answering DIMSUM_OK, and by a call with rows getting past the shape
checks to the refusal of a missing pointer (DIMSUM_ERR_NULL where a refused width answers DIMSUM_ERR_SHAPE).

The order of the checks, which the cases with two faults pin: params pointer, struct_size, extension, shapes, (tokens == 0: done), required
pointers, ldc >= width, the per-expert pointer table (per expert: missing, then misaligned), the other alignments and ldc % 4.

The width ceilings differ between the entries and are kept as they are: the forward entries take k up to 2^31 - 32 (int32 indexing along a row)
and n up to 65535 * BN (n tiles ride on gridDim.y); the two gradients take k up to 65535 * BN and n up to 65535 * BM."""
import ctypes as C

import pytest

from dimsum_amd import _lib

OK, NULL, DTYPE, SHAPE, STRIDE, UNSUPPORTED, LAUNCH, ABI = range(8)
BM, BN, MAX_E = _lib.MOE_GEMM_BM, _lib.MOE_GEMM_BN, 64
E, T, K, N = 3, 100, 64, 96                          # the base call: three experts, rows, both widths multiples of 32 and different
TOKEN_CEILING = 2 ** 31 - BM * (MAX_E + 1)           # the first refused row count


def _addr(i):
    return 0x10000000 + 0x100000 * i                 # 1-MB aligned, distinct, never dereferenced


def _table(i):
    return [_addr(16 * i + e) for e in range(E)]


# entry -> (struct, C function, the base call's fields, its pointer tables, the field ldc bounds, (k, n) accepted ceilings,
#           the required pointers in the order the entry names them, {pointer: the alignment it must have})
ENTRIES = {
    "fwd": (_lib.MoeGemmParams, "dimsum_moe_gemm",
            dict(num_experts=E, tokens=T, k=K, n=N, ldc=N, x_ptr=_addr(0), offsets_ptr=_addr(1), bias_ptr=_addr(2), out_ptr=_addr(3)),
            {"w_ptrs": _table(1)}, "n", (2 ** 31 - 32, 65535 * BN),
            ("x_ptr", "offsets_ptr", "w_ptrs", "out_ptr"), {"x_ptr": 16, "out_ptr": 16, "bias_ptr": 16, "offsets_ptr": 4}),
    "f16s": (_lib.MoeGemmF16sParams, "dimsum_moe_gemm_f16s",
             dict(num_experts=E, tokens=T, k=K, n=N, ldc=N, x_ptr=_addr(0), x_inv_ptr=_addr(4), offsets_ptr=_addr(1), bias_ptr=_addr(2), out_ptr=_addr(3)),
             {"w_ptrs": _table(1), "w_inv_ptrs": _table(2)}, "n", (2 ** 31 - 32, 65535 * BN),
             ("x_ptr", "x_inv_ptr", "offsets_ptr", "w_ptrs", "w_inv_ptrs", "out_ptr"),
             {"x_ptr": 16, "x_inv_ptr": 4, "out_ptr": 16, "bias_ptr": 16, "offsets_ptr": 4}),
    "dgrad": (_lib.MoeGemmDgradParams, "dimsum_moe_gemm_dgrad",
              dict(num_experts=E, tokens=T, k=K, n=N, ldc=K, dy_ptr=_addr(0), offsets_ptr=_addr(1), dx_ptr=_addr(3)),
              {"w_ptrs": _table(1)}, "k", (65535 * BN, 65535 * BM),
              ("dy_ptr", "offsets_ptr", "w_ptrs", "dx_ptr"), {"dy_ptr": 16, "dx_ptr": 16, "offsets_ptr": 4}),
    "wgrad": (_lib.MoeGemmWgradParams, "dimsum_moe_gemm_wgrad",
              dict(num_experts=E, tokens=T, k=K, n=N, dy_ptr=_addr(0), x_ptr=_addr(5), offsets_ptr=_addr(1), db_ptr=_addr(2)),
              {"dw_ptrs": _table(1)}, None, (65535 * BN, 65535 * BM),
              ("dy_ptr", "x_ptr", "offsets_ptr", "dw_ptrs"), {"dy_ptr": 16, "x_ptr": 16, "db_ptr": 4, "offsets_ptr": 4}),
}
EXT_TOO_BIG = C.sizeof(_lib.MoeExt) + 8


def _status(entry, mut):
    """the status of the entry's base call changed by `mut`. Keys: a field of the struct; a table's name with None (no table) or with
    {expert: address}; "null" (no params at all); "ext_size" (the extension's struct_size); "no_ptrs" (every pointer and table NULL)"""
    struct, fn, base, tables, _, _, required, aligned = ENTRIES[entry]
    P = struct()
    X = _lib.attach_ext(P, _lib.MoeExt)
    fields = {**base, **{k: v for k, v in mut.items() if k not in tables and k not in ("null", "ext_size", "no_ptrs")}}
    keep = []
    for name, addrs in tables.items():
        change = mut.get(name, {})
        if change is None or mut.get("no_ptrs"):
            continue                                 # the field stays NULL
        addrs = list(addrs)
        for e, a in change.items():
            addrs[e] = a
        n = max(len(addrs), fields["num_experts"], 1)
        arr = (_lib.vp * n)(*(addrs + [_addr(200 + e) for e in range(n - len(addrs))]))
        keep.append(arr)
        setattr(P, name, arr)
    for key, val in fields.items():
        if mut.get("no_ptrs") and key.endswith("_ptr"):
            continue
        setattr(P, key, val)
    if "ext_size" in mut:
        X.struct_size = mut["ext_size"]
    return getattr(_lib.load(), fn)(None if mut.get("null") else P, None)


def _cases(entry):
    struct, _, base, tables, ldc_width, (k_top, n_top), required, aligned = ENTRIES[entry]
    first, table = required[0], next(iter(tables))
    miss = {first: None}                             # on top of accepted shapes: DIMSUM_ERR_NULL, the first answer after the shape checks
    t0, t1 = tables[table][0], tables[table][1]
    cases = [
        # ---- params, struct sizes, extension
        ({"null": 1}, NULL), ({"struct_size": 0}, ABI), ({"struct_size": C.sizeof(struct) + 8}, ABI), ({"struct_size": C.sizeof(struct) - 8}, ABI),
        ({"ext_size": EXT_TOO_BIG}, ABI), ({"ext_size": 2}, ABI),
        ({"struct_size": 0, "num_experts": 0}, ABI), ({"ext_size": 2, "num_experts": 0}, ABI), ({"ext_size": 2, "tokens": 0}, ABI),
        # ---- shapes
        ({"num_experts": 0}, SHAPE), ({"num_experts": MAX_E + 1}, SHAPE), ({"num_experts": -1}, SHAPE), ({"num_experts": MAX_E, **miss}, NULL),
        ({"tokens": -1}, SHAPE), ({"tokens": TOKEN_CEILING}, SHAPE), ({"tokens": TOKEN_CEILING - 1, **miss}, NULL),
        ({"k": 0}, SHAPE), ({"k": 48}, SHAPE), ({"k": -32}, SHAPE), ({"n": 0}, SHAPE), ({"n": 48}, SHAPE), ({"n": -32}, SHAPE),
        ({"k": k_top + 32}, SHAPE), ({"k": k_top + 32, **miss}, SHAPE), ({"k": k_top, **miss}, NULL), ({"k": k_top - 32, **miss}, NULL),
        ({"n": n_top + 32}, SHAPE), ({"n": n_top + 32, **miss}, SHAPE), ({"n": n_top, **miss}, NULL), ({"n": n_top - 32, **miss}, NULL),
        ({"k": k_top, "n": n_top, **miss}, NULL),
        ({"num_experts": 0, **miss}, SHAPE), ({"k": 48, **miss}, SHAPE), ({"n": 48, first: base[first] + 8}, SHAPE),
        # ---- the empty call: shapes are checked, pointers are not
        ({"tokens": 0}, OK), ({"tokens": 0, "no_ptrs": 1}, OK), ({"tokens": 0, first: base[first] + 2}, OK), ({"tokens": 0, table: {0: None, 1: t1 + 8}}, OK),
        ({"tokens": 0, "k": k_top}, OK), ({"tokens": 0, "k": k_top - 32}, OK), ({"tokens": 0, "n": n_top}, OK), ({"tokens": 0, "n": n_top - 32}, OK),
        ({"tokens": 0, "k": k_top, "n": n_top, "no_ptrs": 1}, OK), ({"tokens": 0, "num_experts": MAX_E}, OK),
        ({"tokens": 0, "k": k_top + 32}, SHAPE), ({"tokens": 0, "n": n_top + 32}, SHAPE), ({"tokens": 0, "k": 48}, SHAPE), ({"tokens": 0, "n": 0}, SHAPE),
        ({"tokens": 0, "k": 48, "no_ptrs": 1}, SHAPE), ({"tokens": 0, "n": n_top + 32, "no_ptrs": 1}, SHAPE), ({"tokens": 0, "num_experts": 0}, SHAPE),
        ({"tokens": 0, "num_experts": MAX_E + 1, "no_ptrs": 1}, SHAPE),
        # ---- pointers
        ({"no_ptrs": 1}, NULL),
    ]
    cases += [({name: None}, NULL) for name in required]
    cases += [({name: None, table: {0: t0 + 8}}, NULL) for name in required if name != table]          # required pointers before the table
    # ---- the per-expert tables: per expert missing, then misaligned; the earlier expert decides
    for name, addrs in tables.items():
        cases += [({name: {e: None}}, NULL) for e in range(E)] + [({name: {e: addrs[e] + 8}}, STRIDE) for e in range(E)]
        cases += [({name: {0: None, 1: addrs[1] + 8}}, NULL), ({name: {0: addrs[0] + 8, 1: None}}, STRIDE), ({name: {1: addrs[1] + 4, 2: None}}, STRIDE),
                  ({name: {1: None, 2: addrs[2] + 8}}, NULL)]
        cases += [({name: {2: None}, p: base[p] + a // 2}, NULL) for p, a in aligned.items()]          # the table before the other alignments
    if len(tables) == 2:                             # two tables are walked together, expert by expert
        (ta, aa), (tb, ab) = tables.items()
        cases += [({ta: {0: aa[0] + 8}, tb: {0: None}}, NULL), ({ta: {0: None}, tb: {0: ab[0] + 8}}, NULL),
                  ({tb: {0: ab[0] + 8}, ta: {1: None}}, STRIDE), ({ta: {0: aa[0] + 8}, tb: {1: None}}, STRIDE),
                  ({tb: {1: None}, ta: {2: aa[2] + 8}}, NULL), ({ta: {1: None}, tb: {0: None}}, NULL)]
    # ---- strides and alignment
    cases += [({p: base[p] + a // 2}, STRIDE) for p, a in aligned.items()]
    cases += [({p: base[p] + 1}, STRIDE) for p, a in aligned.items()]
    if ldc_width:
        w = base[ldc_width]
        cases += [({"ldc": w - 4}, STRIDE), ({"ldc": w - 32}, STRIDE), ({"ldc": 0}, STRIDE), ({"ldc": w + 2}, STRIDE), ({"ldc": w + 1}, STRIDE),
                  ({"ldc": w - 4, table: {0: None}}, STRIDE),        # ldc >= width before the table
                  ({"ldc": w + 2, table: {0: None}}, NULL),          # ldc % 4 after it
                  ({"ldc": w - 4, first: None}, NULL)]               # required pointers before both
    return [(entry, mut, want) for mut, want in cases]


CASES = [c for entry in ENTRIES for c in _cases(entry)]


def _case_id(case):
    entry, mut, _ = case
    return entry + ":" + ",".join(f"{k}={v}" for k, v in mut.items())


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_host_checks_keep_their_status(case):
    entry, mut, want = case
    assert want != LAUNCH and (want != OK or mut.get("tokens") == 0)      # nothing is launched: a refusal, or the empty call
    assert _status(entry, mut) == want


def test_the_entries_keep_their_own_width_ceilings():
    """the forward entries and the gradients accept different widths: k = 65535 * BN + 32 and n = 65535 * BM + 32 tell them apart"""
    for entry, k_ok, n_ok in (("fwd", OK, OK), ("f16s", OK, OK), ("dgrad", SHAPE, SHAPE), ("wgrad", SHAPE, SHAPE)):
        assert _status(entry, {"tokens": 0, "k": 65535 * BN + 32}) == k_ok, entry
        assert _status(entry, {"tokens": 0, "n": 65535 * BM + 32}) == n_ok, entry
    for entry in ("fwd", "f16s"):
        assert _status(entry, {"tokens": 0, "k": 2 ** 31 - 32}) == OK and _status(entry, {"tokens": 0, "k": 2 ** 31}) == SHAPE
        assert _status(entry, {"tokens": 0, "n": 65535 * BN}) == OK and _status(entry, {"tokens": 0, "n": 65535 * BN + 32}) == SHAPE
    for entry in ("dgrad", "wgrad"):
        assert _status(entry, {"tokens": 0, "k": 65535 * BN}) == OK and _status(entry, {"tokens": 0, "n": 65535 * BM}) == OK
