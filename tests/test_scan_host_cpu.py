"""Characterisation of the selective scan's host layer (csrc/ssm_scan_fwd.hip, ssm_scan_bwd.hip): the status code of every refusal the four
entry points can give before a kernel is launched, and the kernel the two dispatch queries pick over a grid of launch shapes. The numbers
were recorded from the library BEFORE the host layer was refactored and are kept verbatim: a refactor of that layer has to reproduce them.

CPU-only. Every pointer is a made-up, suitably aligned address that is never read: each case is refused (a status that is neither DIMSUM_OK
nor DIMSUM_ERR_LAUNCH), so nothing is launched.

`return DIMSUM_ERR_*` lines of the entry points that cannot be reached without a launch, and so have no case here:
  * launch_bwd<kRev>: `if (!p.z_ptr) return DIMSUM_ERR_NULL` -- dimsum_ssm_scan_bidir_bwd refuses a NULL z before it dispatches;
  * launch_bidir / launch_bwd / dimsum_ssm_scan_bidir_bwd: `return DIMSUM_ERR_LAUNCH` / the status of the second direction -- after the
    first kernel of the pair went out;
  * ssm_scan_fwd_run: `if (a.batch == 0) return DIMSUM_OK` -- the shape check before it refuses batch <= 0 (dead code, dropped by the
    refactor)."""
import ctypes as C

import pytest

from dimsum_amd import _lib

OK, NULL, DTYPE, SHAPE, STRIDE, UNSUPPORTED, LAUNCH, ABI = range(8)

B, D, L, N, G = 2, 64, 64, 16, 1                     # the base call: fp32, z given, contiguous (batch, dim, seqlen) operands
CKPT_BYTES = B * ((L + 7) // 8) * N * D * 4          # saved states (batch, ceil(L / 8), dstate, dim) fp32


def _addr(i):
    return 0x10000000 + 0x100000 * i                 # 1-MB aligned, distinct, never dereferenced


def _fill_fwd(F):
    """the base forward struct; its extension is attached and returned"""
    F.batch, F.dim, F.seqlen, F.dstate, F.n_groups, F.n_chunks, F.delta_softplus, F.dtype = B, D, L, N, G, 1, 1, _lib.F32
    F.A_d_stride, F.A_dstate_stride = N, 1
    for t in ("B", "C"):
        setattr(F, t + "_batch_stride", G * N * L), setattr(F, t + "_group_stride", N * L), setattr(F, t + "_dstate_stride", L)
    for t in ("u", "delta", "z", "out", "out_z"):
        setattr(F, t + "_batch_stride", D * L), setattr(F, t + "_d_stride", L)
    for i, t in enumerate(("A", "B", "C", "D", "u", "delta", "delta_bias", "z", "out", "out_z")):
        setattr(F, t + "_ptr", _addr(i))
    return _lib.attach_ext(F, _lib.SsmExt)


def _fill_bwd(Q, lib):
    """the base backward struct: saved states given, the workspace exactly the partial dB / dC sums"""
    E = _fill_fwd(Q.fwd)
    E.ckpt_ptr = _addr(30)
    Q.dA_d_stride, Q.dA_dstate_stride = N, 1
    for t in ("dB", "dC"):
        setattr(Q, t + "_batch_stride", G * N * L), setattr(Q, t + "_group_stride", N * L), setattr(Q, t + "_dstate_stride", L)
    for t in ("dout", "du", "dz", "ddelta"):
        setattr(Q, t + "_batch_stride", D * L), setattr(Q, t + "_d_stride", L)
    for i, t in enumerate(("dout", "dA", "dB", "dC", "dD", "du", "dz", "ddelta", "ddelta_bias", "workspace")):
        setattr(Q, t + "_ptr", _addr(10 + i))
    Q.workspace_bytes = lib.dimsum_ssm_scan_bwd_workspace_bytes(B, D, L, N, G) - CKPT_BYTES
    return E


def _fill_rev(P, bwd):
    P.A_b_ptr, P.A_b_d_stride, P.A_b_dstate_stride = _addr(20), N, 1
    P.out_b_ptr, P.out_b_batch_stride, P.out_b_d_stride = _addr(21), D * L, L
    P.ckpt_b_ptr = _addr(22)
    if bwd:
        P.dA_b_ptr, P.dA_b_d_stride, P.dA_b_dstate_stride = _addr(23), N, 1


def _make(entry, lib):
    """-> (C function, top struct, {prefix: struct}) of the base call of `entry`. Mutation keys are `prefix.field`: top = the struct the entry
    point takes, fwd = its dimsum_ssm_params_t, ext = that one's dimsum_ssm_ext_t, bwd = its dimsum_ssm_bwd_params_t"""
    if entry == "fwd":
        P = _lib.SsmParams()
        E = _fill_fwd(P)
        return lib.dimsum_ssm_scan_fwd, P, {"top": P, "fwd": P, "ext": E}
    if entry == "bwd":
        P = _lib.SsmBwdParams()
        E = _fill_bwd(P, lib)
        return lib.dimsum_ssm_scan_bwd, P, {"top": P, "fwd": P.fwd, "ext": E, "bwd": P}
    if entry == "bidir":
        P = _lib.SsmBidirParams()
        E = _fill_fwd(P.fwd)
        E.ckpt_ptr = _addr(30)
        _fill_rev(P, False)
        return lib.dimsum_ssm_scan_bidir_fwd, P, {"top": P, "fwd": P.fwd, "ext": E}
    P = _lib.SsmBidirBwdParams()
    E = _fill_bwd(P.bwd, lib)
    _fill_rev(P, True)
    return lib.dimsum_ssm_scan_bidir_bwd, P, {"top": P, "fwd": P.bwd.fwd, "ext": E, "bwd": P.bwd}


def _status(entry, mut):
    lib = _lib.load()
    fn, P, parts = _make(entry, lib)
    for key, val in mut.items():
        if key == "null":                            # the NULL struct itself
            return fn(None, None)
        if key == "no_ext":
            parts["fwd"].ext = None
            continue
        prefix, field = key.split(".")
        setattr(parts[prefix], field, val)
    return fn(P, None)


BIG = 1 << 30            # a row stride whose tile overflows the kernels' 32-bit byte offsets
EXT_TOO_BIG = C.sizeof(_lib.SsmExt) + 8
NO_Z = {"fwd.z_ptr": None, "fwd.out_z_ptr": None}
# the fused dt_proj of the forward: a served configuration apart from what a case breaks (the 64-channel kernel asked for by name)
DT = {"ext.kernel_variant": 1, "ext.ckpt_ptr": None, "ext.dt_w_ptr": _addr(40), "ext.dt_x_ptr": _addr(41), "ext.dt_rank": 8, "ext.dt_w_row_stride": 8,
      "ext.dt_x_row_stride": B * L}
Z16 = {"ext.kernel_variant": 1, "ext.ckpt_ptr": None, "ext.out_z_f16": 1, "ext.out_z_scale_ptr": _addr(42), "ext.out_z_scale_ld": 1}
PLANES = {"ext.out_z_lo_offset": B * D * L * 2}

# (entry, what the base call is changed in, status)
_SHARED_SHAPE = [({"fwd.batch": 0}, SHAPE), ({"fwd.batch": -1}, SHAPE), ({"fwd.dim": 0}, SHAPE), ({"fwd.seqlen": 0}, SHAPE), ({"fwd.n_groups": 0}, SHAPE),
                 ({"fwd.n_groups": 3}, SHAPE), ({"fwd.dstate": 257}, SHAPE), ({"fwd.n_chunks": 0}, SHAPE), ({"fwd.n_chunks": 2}, SHAPE),
                 ({"fwd.dstate": 0}, SHAPE), ({"fwd.dstate": 12}, SHAPE), ({"fwd.dstate": 64}, SHAPE), ({"fwd.dtype": 3}, DTYPE), ({"fwd.dtype": -1}, DTYPE)]
_SHARED_NULL = [({"fwd." + t + "_ptr": None}, NULL) for t in ("A", "B", "C", "u", "delta")]
_BWD_NULL = [({"bwd." + t + "_ptr": None}, NULL) for t in ("dout", "dA", "dB", "dC", "du", "ddelta", "workspace")]
_BWD_WS = [({"bwd.dz_ptr": None}, NULL), ({"fwd.out_ptr": None}, NULL), ({"bwd.workspace_ptr": _addr(19) + 8}, STRIDE),
           ({"bwd.workspace_ptr": _addr(19) + 4}, STRIDE), ({"bwd.workspace_bytes": 0}, SHAPE),
           ({"bwd.workspace_ptr": None, "bwd.workspace_bytes": 0}, NULL), ({"bwd.workspace_ptr": _addr(19) + 8, "bwd.workspace_bytes": 0}, STRIDE),
           ({"bwd.workspace_ptr": _addr(19) + 8, "bwd.dz_ptr": None}, NULL), ({"bwd.workspace_ptr": _addr(19) + 8, "fwd.dtype": 3}, STRIDE),
           ({"bwd.workspace_bytes": 0, "fwd.dtype": 3}, SHAPE), ({"bwd.dout_ptr": None, "fwd.batch": 0}, SHAPE), ({"fwd.A_ptr": None, "fwd.batch": 0}, NULL)]
_STRUCT = [({"null": 1}, NULL), ({"top.struct_size": 0}, ABI), ({"ext.struct_size": EXT_TOO_BIG}, ABI), ({"ext.struct_size": 2}, ABI)]

CASES = (
    [("fwd", m, s) for m, s in _STRUCT + _SHARED_NULL + _SHARED_SHAPE]
    + [("fwd", m, s) for m, s in [
        ({"top.struct_size": C.sizeof(_lib.SsmParams) + 8}, ABI),
        ({"fwd.out_z_ptr": None}, NULL),                                                  # z without out_z
        ({"fwd.dtype": 3, "fwd.dstate": 12}, DTYPE),                                      # dtype is looked at before dstate
        ({"fwd.dtype": 3, "fwd.batch": 0}, SHAPE),
        ({"fwd.u_d_stride": BIG}, STRIDE), ({"fwd.delta_d_stride": BIG}, STRIDE), ({"fwd.out_d_stride": BIG}, STRIDE), ({"fwd.z_d_stride": BIG}, STRIDE),
        ({"fwd.out_z_d_stride": BIG}, STRIDE), ({"fwd.B_dstate_stride": BIG}, STRIDE), ({"fwd.C_dstate_stride": BIG}, STRIDE), ({"fwd.u_d_stride": -L}, STRIDE),
        ({"fwd.x_ptr": _addr(50) + 8}, STRIDE), ({"fwd.x_ptr": _addr(50) + 4, "fwd.dtype": 1}, STRIDE),
        # out_z as a pair of bf16 planes
        ({**PLANES, "fwd.dtype": 1}, UNSUPPORTED), ({**PLANES, **NO_Z}, UNSUPPORTED), ({**PLANES, "fwd.seqlen": 60}, SHAPE),
        ({**PLANES, "fwd.u_ptr": _addr(4) + 4}, STRIDE), ({**PLANES, "fwd.out_z_ptr": _addr(9) + 8}, STRIDE), ({**PLANES, "ext.out_z_lo_offset": 12}, STRIDE),
        ({**PLANES, "fwd.out_z_batch_stride": D * L + 4}, STRIDE), ({**PLANES, "fwd.out_z_d_stride": L + 4}, STRIDE), ({**PLANES, "fwd.u_batch_stride": D * L + 2}, STRIDE),
        # fused dt_proj
        ({**DT, "ext.dt_x_ptr": None}, NULL), ({**DT, "ext.dt_rank": 0}, SHAPE), ({**DT, "ext.dt_rank": 36, "ext.dt_w_row_stride": 36}, SHAPE),
        ({**DT, "ext.dt_rank": 6}, SHAPE), ({**DT, "ext.dt_w_row_stride": 10}, STRIDE), ({**DT, "ext.dt_w_row_stride": 4}, STRIDE),
        ({**DT, "ext.dt_x_row_stride": B * L - 1}, STRIDE), ({**DT, "ext.dt_w_ptr": _addr(40) + 8}, STRIDE), ({**DT, "ext.dt_x_ptr": _addr(41) + 2}, STRIDE),
        ({**DT, "ext.dt_x_row_stride": 1 << 26}, STRIDE), ({**DT, "fwd.delta_ptr": None, "fwd.batch": 0}, SHAPE),
        ({**DT, "ext.kernel_variant": 2}, UNSUPPORTED), ({**DT, "ext.kernel_variant": 16}, UNSUPPORTED), ({**DT, "ext.kernel_variant": 0}, UNSUPPORTED),
        ({**DT, "fwd.dtype": 1}, UNSUPPORTED), ({**DT, "fwd.dstate": 8}, UNSUPPORTED), ({**DT, "ext.ckpt_ptr": _addr(30)}, UNSUPPORTED), ({**DT, **NO_Z}, UNSUPPORTED),
        ({**DT, "fwd.dim": 32}, UNSUPPORTED), ({**DT, "fwd.u_ptr": _addr(4) + 4}, UNSUPPORTED), ({**DT, "fwd.dstate": 12}, SHAPE), ({**DT, "fwd.dtype": 3}, DTYPE),
        # block-scaled fp16 out_z
        ({**Z16, "ext.kernel_variant": 4}, UNSUPPORTED), ({**Z16, "fwd.dtype": 2}, UNSUPPORTED), ({**Z16, "fwd.dstate": 32}, UNSUPPORTED),
        ({**Z16, "ext.ckpt_ptr": _addr(30)}, UNSUPPORTED), ({**Z16, **NO_Z}, UNSUPPORTED), ({**Z16, "ext.out_z_scale_ptr": None}, NULL),
        ({**Z16, "fwd.seqlen": 36}, UNSUPPORTED), ({**Z16, **PLANES}, UNSUPPORTED), ({**Z16, "fwd.out_z_batch_stride": D * L + 4}, STRIDE),
        ({**Z16, "fwd.out_z_d_stride": L + 4}, STRIDE), ({**Z16, "ext.out_z_scale_ld": 0}, STRIDE), ({**Z16, "fwd.out_z_ptr": _addr(9) + 8}, UNSUPPORTED),
        ({**Z16, "fwd.u_d_stride": BIG}, STRIDE), ({**Z16, "fwd.x_ptr": _addr(50) + 8}, STRIDE),
    ]]
    + [("bidir", m, s) for m, s in _STRUCT + _SHARED_NULL + _SHARED_SHAPE]
    + [("bidir", m, s) for m, s in [
        ({"top.struct_size": C.sizeof(_lib.SsmBidirParams) - 8}, ABI), ({"fwd.out_z_ptr": None}, NULL),
        ({"fwd.z_ptr": None}, NULL), (NO_Z, NULL), ({"top.A_b_ptr": None}, NULL),
        ({"ext.dt_w_ptr": _addr(40)}, UNSUPPORTED), ({**DT}, UNSUPPORTED), ({**PLANES}, UNSUPPORTED), ({"ext.out_z_f16": 1}, UNSUPPORTED), ({"fwd.x_ptr": _addr(50)}, UNSUPPORTED),
        ({"fwd.x_ptr": _addr(50), "fwd.A_ptr": None}, UNSUPPORTED), ({"fwd.x_ptr": _addr(50), "top.struct_size": 0}, ABI),
        ({"fwd.dtype": 3, "fwd.dstate": 12}, SHAPE),                                      # here dstate is looked at before dtype
        ({"fwd.dstate": 12, "top.A_b_ptr": None}, NULL),
        ({"fwd.u_d_stride": BIG}, STRIDE), ({"fwd.out_d_stride": BIG}, STRIDE), ({"top.out_b_d_stride": BIG}, STRIDE), ({"fwd.C_dstate_stride": BIG}, STRIDE),
        ({"fwd.u_d_stride": BIG, "fwd.dtype": 3}, DTYPE),
    ]]
    + [("bwd", m, s) for m, s in _STRUCT + _SHARED_NULL + _SHARED_SHAPE + _BWD_NULL + _BWD_WS]
    + [("bwd", m, s) for m, s in [
        ({"top.struct_size": C.sizeof(_lib.SsmBwdParams) + 8}, ABI),
        ({"ext.dt_w_ptr": _addr(40)}, UNSUPPORTED), ({**DT}, UNSUPPORTED), ({"ext.dt_w_ptr": _addr(40), "fwd.delta_ptr": None}, NULL),
        ({"fwd.dtype": 3, "fwd.dstate": 12}, DTYPE),
        ({"fwd.u_d_stride": BIG}, STRIDE), ({"bwd.dout_d_stride": BIG}, STRIDE), ({"bwd.du_d_stride": BIG}, STRIDE), ({"bwd.ddelta_d_stride": BIG}, STRIDE),
        ({"bwd.dz_d_stride": BIG}, STRIDE), ({"fwd.out_d_stride": BIG}, STRIDE), ({"fwd.out_z_d_stride": BIG}, STRIDE), ({"fwd.B_dstate_stride": BIG}, STRIDE),
        # no saved states: the workspace holds them too, and the state-rebuild sweep of the forward comes first
        ({"ext.ckpt_ptr": None}, SHAPE), ({"ext.ckpt_ptr": None, "bwd.workspace_bytes": 1 << 40, "fwd.dtype": 3}, DTYPE),
        ({"ext.ckpt_ptr": None, "bwd.workspace_bytes": 1 << 40, "fwd.dstate": 12}, SHAPE), ({"ext.ckpt_ptr": None, "bwd.workspace_bytes": 1 << 40, "fwd.u_d_stride": BIG}, STRIDE),
        ({"no_ext": 1}, SHAPE), ({"no_ext": 1, "bwd.workspace_bytes": 1 << 40, "fwd.delta_d_stride": BIG}, STRIDE),
    ]]
    + [("bidir_bwd", m, s) for m, s in _STRUCT + _SHARED_NULL + _SHARED_SHAPE + _BWD_NULL + _BWD_WS]
    + [("bidir_bwd", m, s) for m, s in [
        ({"top.struct_size": C.sizeof(_lib.SsmBidirBwdParams) - 8}, ABI),
        ({"ext.dt_w_ptr": _addr(40)}, UNSUPPORTED), ({**PLANES}, UNSUPPORTED), ({"ext.out_z_f16": 1}, UNSUPPORTED), ({"ext.out_z_f16": 1, "fwd.A_ptr": None}, UNSUPPORTED),
        ({"fwd.z_ptr": None}, NULL), ({"ext.ckpt_ptr": None}, NULL), ({"no_ext": 1}, NULL),
        ({"top.A_b_ptr": None}, NULL), ({"top.out_b_ptr": None}, NULL), ({"top.ckpt_b_ptr": None}, NULL), ({"top.dA_b_ptr": None}, NULL),
        ({"top.A_b_ptr": None, "bwd.workspace_ptr": _addr(19) + 8}, NULL), ({"ext.ckpt_ptr": None, "bwd.workspace_ptr": _addr(19) + 8}, NULL),
        ({"top.dA_b_ptr": None, "bwd.workspace_bytes": 0}, NULL), ({"top.dA_b_ptr": None, "fwd.dstate": 12}, NULL),
        ({"fwd.dtype": 3, "fwd.dstate": 12}, DTYPE),
        ({"fwd.u_d_stride": BIG}, STRIDE), ({"bwd.dout_d_stride": BIG}, STRIDE), ({"bwd.dz_d_stride": BIG}, STRIDE), ({"fwd.C_dstate_stride": BIG}, STRIDE),
    ]]
)


def _case_id(case):
    entry, mut, _ = case
    return entry + ":" + ",".join(f"{k}={v}" for k, v in mut.items())


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_refused_inputs_keep_their_status(case):
    entry, mut, want = case
    assert want not in (OK, LAUNCH)                  # a refusal: nothing is launched
    assert _status(entry, mut) == want


def test_base_calls_are_what_the_cases_break():
    """the base structs pass every check of the size / extension / pointer / shape layer (a refusal above is due to the one change made):
    the dispatch queries, which share those checks and launch nothing, accept them"""
    lib = _lib.load()
    _, P, _ = _make("fwd", lib)
    assert lib.dimsum_ssm_scan_fwd_variant(P) == 16
    _, P, parts = _make("bidir", lib)
    assert lib.dimsum_ssm_scan_bidir_fwd_variant(P) == 16


# ---- the dispatch queries over a grid of launch shapes ------------------------------------------------------------------------------------
BATCHES, DIMS, SEQLENS, DSTATES, GROUPS, VARIANTS = (1, 8, 16, 32, 64, 256), (64, 1024, 1152), (256, 1024, 4096), (4, 8, 16, 32), (1, 2), (0, 1, 2, 4, 16)
_CODE = {1: "1", 2: "2", 4: "4", 16: "L", -1: "-"}


def _query(bidir, batch, dim, seqlen, dstate, groups, variant, **extra):
    lib = _lib.load()
    P = _lib.SsmBidirParams() if bidir else _lib.SsmParams()
    F = P.fwd if bidir else P
    F.batch, F.dim, F.seqlen, F.dstate, F.n_groups, F.n_chunks = batch, dim, seqlen, dstate, groups, (seqlen + 2047) // 2048
    E = None
    if variant or any(k.startswith("ext.") for k in extra):
        E = _lib.attach_ext(F, _lib.SsmExt)
        E.kernel_variant = variant
    for key, val in extra.items():
        prefix, field = key.split(".")
        setattr({"top": P, "fwd": F, "ext": E}[prefix], field, val)
    return int((lib.dimsum_ssm_scan_bidir_fwd_variant if bidir else lib.dimsum_ssm_scan_fwd_variant)(P))


def _grid_rows(bidir):
    """one row per (batch, dim, seqlen): the picks over dstate x groups x kernel_variant, one character each (L = 16 lanes per channel)"""
    rows = []
    for batch in BATCHES:
        for dim in DIMS:
            for seqlen in SEQLENS:
                rows.append("".join(_CODE[_query(bidir, batch, dim, seqlen, n, g, v)] for n in DSTATES for g in GROUPS for v in VARIANTS))
    return rows


FWD_GRID = """
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
212112121141241412414124L4124L4124141241
212112121141241412414124L4124L4124141241
212112121141241412414124L4124L4124141241
212112121141241412414124L4124L4124141241
212112121141241412414124L4124L4124141241
212112121141241412414124L4124L4124141241
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
212112121141241412414124L4124L4124141241
212112121141241412414124L4124L4124141241
212112121141241412414124L4124L4124141241
212112121141241412414124L4124L4124141241
212112121141241412414124L4124L4124141241
212112121141241412414124L4124L4124141241
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
21211212114124141241L124LL124L4124141241
112111121111241112411124L1124L1124111241
112111121111241112411124L1124L1124111241
112111121111241112411124L1124L1124111241
112111121111241112411124L1124L1124111241
112111121111241112411124L1124L1124111241
112111121111241112411124L1124L1124111241
""".split()

BIDIR_GRID = """
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
111111111111111111111111L1111L1111111111
111111111111111111111111L1111L1111111111
111111111111111111111111L1111L1111111111
111111111111111111111111L1111L1111111111
111111111111111111111111L1111L1111111111
111111111111111111111111L1111L1111111111
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
111111111111111111111111L1111L1111111111
111111111111111111111111L1111L1111111111
111111111111111111111111L1111L1111111111
111111111111111111111111L1111L1111111111
111111111111111111111111L1111L1111111111
111111111111111111111111L1111L1111111111
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
11111111111111111111L111LL111L1111111111
111111111111111111111111L1111L1111111111
111111111111111111111111L1111L1111111111
111111111111111111111111L1111L1111111111
111111111111111111111111L1111L1111111111
111111111111111111111111L1111L1111111111
111111111111111111111111L1111L1111111111
""".split()


def test_fwd_variant_grid():
    assert _grid_rows(False) == FWD_GRID


def test_bidir_fwd_variant_grid():
    assert _grid_rows(True) == BIDIR_GRID


def test_variant_queries_refuse_with_minus_one():
    lib = _lib.load()
    shape = (16, 1152, 1024, 16, 1, 0)
    assert _query(False, *shape) == 16 and _query(True, *shape) == 16
    assert lib.dimsum_ssm_scan_fwd_variant(None) == -1 and lib.dimsum_ssm_scan_bidir_fwd_variant(None) == -1
    for bidir in (False, True):
        assert _query(bidir, *shape, **{"top.struct_size": 0}) == -1
        assert _query(bidir, *shape, **{"top.struct_size": C.sizeof(_lib.SsmBidirParams if bidir else _lib.SsmParams) + 8}) == -1
        assert _query(bidir, *shape, **{"ext.struct_size": EXT_TOO_BIG}) == -1
        assert _query(bidir, 16, 1152, 1024, 16, 0, 0) == -1
    # the forward's query looks at nothing but the sizes, the extension and n_groups
    assert _query(False, 0, 1152, 1024, 16, 1, 0) == 16 and _query(False, 16, 1152, 1024, 12, 1, 0) == 2 and _query(False, 16, 1152, 1024, 257, 1, 0) == 1
    assert _query(False, *shape, **{"fwd.x_ptr": _addr(50), "ext.dt_w_ptr": _addr(40), "ext.out_z_f16": 1, "ext.out_z_lo_offset": 8, "fwd.n_chunks": 7}) == 16
    # the bidirectional one refuses what the bidirectional forward refuses for the shape and the extension; the pointers are not looked at
    for extra in ({"fwd.x_ptr": _addr(50)}, {"ext.dt_w_ptr": _addr(40)}, {"ext.out_z_lo_offset": 8}, {"ext.out_z_f16": 1}, {"fwd.n_chunks": 0}, {"fwd.n_chunks": 2}):
        assert _query(True, *shape, **extra) == -1, extra
    for bad in ((0, 1152, 1024, 16, 1), (-1, 1152, 1024, 16, 1), (16, 0, 1024, 16, 1), (16, 1152, 0, 16, 1), (16, 1152, 1024, 16, 5), (16, 1152, 1024, 16, -1),
                (16, 1152, 1024, 0, 1), (16, 1152, 1024, 12, 1), (16, 1152, 1024, 64, 1), (16, 1152, 1024, 257, 1)):
        assert _query(True, *bad, 0) == -1, bad
    for extra in ({"fwd.A_ptr": _addr(0)}, {"fwd.z_ptr": _addr(7)}, {"top.A_b_ptr": _addr(20), "top.out_b_ptr": _addr(21), "ext.ckpt_ptr": _addr(30)}):
        assert _query(True, *shape, **extra) == 16, extra
