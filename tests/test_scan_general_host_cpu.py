"""Characterisation of the general selective scan's host layer, in two parts.

1. The C side (the host tail of csrc/ssm_scan_general.hip): the status code of every refusal the six entry points give before a kernel is
launched -- dimsum_ssm_scan_general_fwd / _general_bwd / _carry_fwd / _varlen_fwd / _varlen_bwd / _varlen_states_fwd -- what
dimsum_ssm_scan_general_bwd_workspace_bytes answers, and two-fault cases that pin the ORDER each entry checks in. The codes were recorded from
the library BEFORE the host layer was refactored and are kept verbatim: a refactor of that layer has to reproduce them. Every pointer is a
made-up, 4-KB aligned address that is never read: no case reaches a launch. (test_scan_general_cpu.py::test_refusals,
test_varlen_cpu.py::test_scan_refusals_in_order and the refusal tests of test_prefill_chunks_cpu.py / test_packed_prefill_cpu.py stay: this
file is the complete grid, not their replacement.)

`return DIMSUM_ERR_*` lines of the host tail that cannot be reached without a launch, and so have no case here:
  * gen_launch: `if (a.seq_idx) return DIMSUM_ERR_UNSUPPORTED` -- ids together with complex A or a constant B / C; every entry that takes ids
    goes through gen_varlen_check first, which refuses exactly those (the UNSUPPORTED cases below), so no call reaches the line at all: dead;
  * gen_dispatch: the `return DIMSUM_ERR_UNSUPPORTED` behind the eight (complex, varB, varC) cases -- the eight are all there are: dead;
  * launch_status()'s DIMSUM_ERR_LAUNCH (common.hpp), after a kernel went out.
What the carry entry does with h0_* / hT_* strides when NEITHER state pointer is given (it ignores them, like state_dtype) cannot be shown
without a launch either: nothing is checked behind them. That state_dtype is ignored then is pinned (a later refusal fires instead).

2. The Python side (dimsum_amd/native.py, general-scan section; dimsum_amd/ops/selective_scan_interface.py): each public function on CPU
tensors with awkward strides, through a stand-in for the library that records the entry reached and every field of the struct passed, nested
structs included; the sentences and the order of the Python refusals; and, for selective_scan_fn's four routes, which native function is
called with which operands and what the autograd classes hand back. Recorded before the refactor as well."""
import ctypes as C

import pytest
import torch

from dimsum_amd import _lib
from test_conv_host_cpu import _OnGpu, _snapshot, filled, routed  # noqa: F401  (filled, routed: fixtures)

OK, NULL, DTYPE, SHAPE, STRIDE, UNSUPPORTED, LAUNCH, ABI = range(8)

B, D, L, N, G = 2, 8, 5, 16, 1                       # the base call of part 1: fp32, real A, input-dependent B / C, z given
WS_REAL, WS_CPLX = 16384, 49152                      # batch * ceil(L / kT) * dstate * reals * (groups * 64-channel blocks * 64) * 4, kT = 4 / 2


def _addr(i):
    return 0x10000000 + 0x1000 * i                   # 4-KB aligned, distinct, never dereferenced


SCAN_STRIDES = [n for n, _ in _lib.SsmGeneralParams._fields_ if n.endswith("_stride")]
BWD_STRIDES = [n for n, _ in _lib.SsmGeneralBwdParams._fields_ if n.endswith("_stride")]
CARRY_STRIDES = [n for n, _ in _lib.SsmCarryParams._fields_ if n.endswith("_stride")]
STATE_STRIDES = ["state_slot_stride", "state_d_stride", "state_dstate_stride"]


def _fill_scan(F):
    F.batch, F.dim, F.seqlen, F.dstate, F.n_groups, F.n_chunks, F.delta_softplus, F.dtype = B, D, L, N, G, 1, 1, _lib.F32
    F.is_variable_B, F.is_variable_C, F.is_complex = 1, 1, 0
    F.A_d_stride, F.A_dstate_stride = N, 1
    for t in ("B", "C"):
        setattr(F, t + "_batch_stride", G * N * L), setattr(F, t + "_group_stride", N * L), setattr(F, t + "_dstate_stride", L)
    for t in ("u", "delta", "z", "out", "out_z"):
        setattr(F, t + "_batch_stride", D * L), setattr(F, t + "_d_stride", L)
    for i, t in enumerate(("A", "B", "C", "D", "u", "delta", "delta_bias", "z", "out", "x", "out_z")):
        setattr(F, t + "_ptr", _addr(i))


def _fill_bwd(Q):
    _fill_scan(Q.fwd)
    Q.dA_d_stride, Q.dA_dstate_stride = N, 1
    for t in ("dB", "dC"):
        setattr(Q, t + "_batch_stride", G * N * L), setattr(Q, t + "_group_stride", N * L), setattr(Q, t + "_dstate_stride", L)
    for t in ("dout", "du", "dz", "ddelta"):
        setattr(Q, t + "_batch_stride", D * L), setattr(Q, t + "_d_stride", L)
    for i, t in enumerate(("dout", "dA", "dB", "dC", "dD", "du", "dz", "ddelta", "ddelta_bias", "workspace")):
        setattr(Q, t + "_ptr", _addr(20 + i))
    Q.workspace_bytes = WS_REAL


def _fill_ids(V):
    V.seq_idx_ptr, V.seq_idx_batch_stride = _addr(40), L


def _make(entry, lib):
    """-> (C function, top struct, {prefix: struct}) of the base call of `entry`. Mutation keys are `prefix.field`: top = the struct the entry
    point takes, scan = its dimsum_ssm_general_params_t, bwd = its dimsum_ssm_general_bwd_params_t, ids = the struct that holds seq_idx"""
    if entry == "fwd":
        P = _lib.SsmGeneralParams()
        _fill_scan(P)
        return lib.dimsum_ssm_scan_general_fwd, P, {"top": P, "scan": P}
    if entry == "bwd":
        Q = _lib.SsmGeneralBwdParams()
        _fill_bwd(Q)
        return lib.dimsum_ssm_scan_general_bwd, Q, {"top": Q, "scan": Q.fwd, "bwd": Q}
    if entry == "carry":
        P = _lib.SsmCarryParams()
        _fill_scan(P.scan)
        P.state_dtype, P.h0_ptr, P.hT_ptr = _lib.F32, _addr(41), _addr(42)
        P.h0_batch_stride, P.h0_d_stride, P.h0_dstate_stride, P.hT_batch_stride, P.hT_d_stride, P.hT_dstate_stride = D * N, N, 1, D * N, N, 1
        return lib.dimsum_ssm_scan_carry_fwd, P, {"top": P, "scan": P.scan}
    if entry == "varlen_fwd":
        V = _lib.SsmVarlenParams()
        _fill_scan(V.scan), _fill_ids(V)
        return lib.dimsum_ssm_scan_varlen_fwd, V, {"top": V, "scan": V.scan, "ids": V}
    if entry == "varlen_bwd":
        V = _lib.SsmVarlenBwdParams()
        _fill_bwd(V.bwd), _fill_ids(V)
        return lib.dimsum_ssm_scan_varlen_bwd, V, {"top": V, "scan": V.bwd.fwd, "bwd": V.bwd, "ids": V}
    assert entry == "states"
    E = _lib.SsmVarlenStatesParams()
    _fill_scan(E.varlen.scan), _fill_ids(E.varlen)
    E.num_slots, E.end_slots_ptr, E.end_slots_batch_stride, E.state_ptr, E.state_f32 = 4, _addr(43), L, _addr(44), 1
    E.state_slot_stride, E.state_d_stride, E.state_dstate_stride = D * N, N, 1
    return lib.dimsum_ssm_scan_varlen_states_fwd, E, {"top": E, "scan": E.varlen.scan, "ids": E.varlen}


def _status(entry, mut):
    lib = _lib.load()
    fn, P, parts = _make(entry, lib)
    for key, val in mut.items():
        if key == "null":                            # the NULL struct itself
            return fn(None, None)
        prefix, field = key.split(".")
        if (field == "struct_size" and val) or field == "workspace_bytes":      # relative to the right one
            val += getattr(parts[prefix], field)
        setattr(parts[prefix], field, val)
    return fn(P, None)


_STRUCT = [({"null": 1}, NULL), ({"top.struct_size": 0}, ABI), ({"top.struct_size": 8}, ABI), ({"top.struct_size": -8}, ABI),
           ({"top.struct_size": 8, "scan.A_ptr": None}, ABI)]
_SCAN_NULL = [({"scan." + t + "_ptr": None}, NULL) for t in ("A", "B", "C", "u", "delta")]
_FWD_NULL = _SCAN_NULL + [({"scan.out_z_ptr": None}, NULL)]                          # z without out_z
_BWD_NULL = (_SCAN_NULL + [({"bwd." + t + "_ptr": None}, NULL) for t in ("dout", "dA", "dB", "dC", "du", "ddelta", "workspace")]
             + [({"bwd.dz_ptr": None}, NULL), ({"scan.out_ptr": None}, NULL)])        # z without dz / without the forward's out
_SHAPE = [({"scan.batch": 0}, SHAPE), ({"scan.batch": 65536}, SHAPE), ({"scan.dim": 0}, SHAPE), ({"scan.seqlen": 0}, SHAPE), ({"scan.dstate": 0}, SHAPE),
          ({"scan.dstate": 257}, SHAPE), ({"scan.n_groups": 0}, SHAPE), ({"scan.n_groups": 3}, SHAPE), ({"scan.n_chunks": 0}, SHAPE),
          ({"scan.n_chunks": 2}, SHAPE), ({"scan.is_variable_B": 0, "scan.is_variable_C": 0, "scan.n_groups": 2}, SHAPE)]
_DTYPE = [({"scan.dtype": -1}, DTYPE), ({"scan.dtype": 3}, DTYPE)]
_SCAN_STRIDE = [({"scan." + n: -1}, STRIDE) for n in SCAN_STRIDES] + [({"scan.x_ptr": _addr(9) + 4}, STRIDE)]
# the documented order of the shared check -- pointers, shape, dtype, strides -- and that more than four waves (dstate 80) change no refusal
_SCAN_ORDER = [({"scan.A_ptr": None, "scan.dstate": 0}, NULL), ({"scan.dstate": 257, "scan.dtype": 3}, SHAPE), ({"scan.dtype": 3, "scan.u_d_stride": -1}, DTYPE),
               ({"scan.n_chunks": 2, "scan.dtype": 3}, SHAPE), ({"scan.u_d_stride": -1, "scan.x_ptr": _addr(9) + 4}, STRIDE),
               ({"scan.dstate": 80, "scan.dtype": 3}, DTYPE), ({"scan.dstate": 80, "scan.u_d_stride": -1}, STRIDE), ({"scan.dstate": 80, "scan.n_groups": 3}, SHAPE)]
_SHARED_FWD = _STRUCT + _FWD_NULL + _SHAPE + _DTYPE + _SCAN_STRIDE + _SCAN_ORDER
_BWD_OWN = ([({"bwd." + n: -1}, STRIDE) for n in BWD_STRIDES]
            + [({"bwd.workspace_ptr": _addr(29) + 4}, STRIDE), ({"bwd.workspace_bytes": -1}, SHAPE), ({"scan.dstate": 80}, SHAPE),
               ({"scan.is_complex": 1}, SHAPE),                                      # a workspace sized for real weights is too small for complex ones
               # its own NULLs before the shared shape / dtype / strides, its strides behind those, the workspace last: alignment, then size
               ({"bwd.dout_ptr": None, "scan.dstate": 257}, NULL), ({"bwd.dz_ptr": None, "scan.dtype": 3}, NULL), ({"scan.out_ptr": None, "scan.u_d_stride": -1}, NULL),
               ({"bwd.workspace_ptr": None, "scan.n_groups": 3}, NULL), ({"scan.dstate": 257, "bwd.du_d_stride": -1}, SHAPE),
               ({"scan.dtype": 3, "bwd.du_d_stride": -1}, DTYPE), ({"scan.x_ptr": _addr(9) + 4, "bwd.workspace_bytes": -1}, STRIDE),
               ({"bwd.du_d_stride": -1, "bwd.workspace_bytes": -1}, STRIDE), ({"bwd.workspace_ptr": _addr(29) + 4, "bwd.workspace_bytes": -1}, STRIDE)])
_SHARED_BWD = _STRUCT + _BWD_NULL + _SHAPE + _DTYPE + _SCAN_STRIDE + _SCAN_ORDER + _BWD_OWN
_IDS = [({"ids.seq_idx_ptr": None}, NULL), ({"ids.seq_idx_batch_stride": -1}, STRIDE), ({"ids.seq_idx_batch_stride": L - 1}, STRIDE),
        ({"scan.is_variable_B": 0}, UNSUPPORTED), ({"scan.is_variable_C": 0}, UNSUPPORTED),
        # the shared checks before the ids; among the ids NULL, then the stride, then what is not built
        ({"scan.dstate": 257, "ids.seq_idx_ptr": None}, SHAPE), ({"scan.dtype": 3, "ids.seq_idx_ptr": None}, DTYPE),
        ({"scan.u_d_stride": -1, "ids.seq_idx_ptr": None}, STRIDE), ({"scan.A_ptr": None, "ids.seq_idx_batch_stride": -1}, NULL),
        ({"ids.seq_idx_ptr": None, "scan.is_variable_B": 0}, NULL), ({"ids.seq_idx_batch_stride": -1, "scan.is_variable_C": 0}, STRIDE)]
_IDS_FWD = _IDS + [({"scan.is_complex": 1}, UNSUPPORTED), ({"ids.seq_idx_ptr": None, "scan.is_complex": 1}, NULL),
                   ({"scan.dstate": 80, "scan.is_variable_B": 0}, UNSUPPORTED)]

# (entry, what the base call is changed in, status)
CASES = (
    [("fwd", m, s) for m, s in _SHARED_FWD]
    + [("bwd", m, s) for m, s in _SHARED_BWD]
    + [("carry", m, s) for m, s in _SHARED_FWD]
    + [("carry", {"top." + n: -1}, STRIDE) for n in CARRY_STRIDES]
    + [("carry", {"top." + n: -1, "top.hT_ptr": None}, STRIDE) for n in CARRY_STRIDES]         # one pointer is enough for all six to count
    + [("carry", {"top." + n: -1, "top.h0_ptr": None}, STRIDE) for n in CARRY_STRIDES]
    + [("carry", m, s) for m, s in [
        ({"top.state_dtype": _lib.F16}, DTYPE), ({"top.state_dtype": _lib.BF16, "top.h0_ptr": None}, DTYPE),
        ({"top.state_dtype": _lib.F16, "scan.dtype": _lib.F16, "scan.is_complex": 1}, DTYPE), ({"top.state_dtype": 7}, DTYPE),
        # the state's dtype: behind the scan's pointers, shape and dtype, before any stride; the state's strides behind the scan's
        ({"top.state_dtype": _lib.F16, "scan.u_d_stride": -1}, DTYPE), ({"top.state_dtype": _lib.F16, "scan.x_ptr": _addr(9) + 4}, DTYPE),
        ({"top.state_dtype": _lib.F16, "scan.dtype": 3}, DTYPE), ({"top.state_dtype": _lib.F16, "scan.dstate": 257}, SHAPE),
        ({"top.state_dtype": _lib.F16, "scan.A_ptr": None}, NULL), ({"top.state_dtype": _lib.F16, "top.h0_d_stride": -1}, DTYPE),
        ({"top.h0_d_stride": -1, "scan.dtype": 3}, DTYPE), ({"top.hT_batch_stride": -1, "scan.dstate": 0}, SHAPE),
        ({"top.hT_batch_stride": -1, "scan.out_z_ptr": None}, NULL),
        # without a state pointer state_dtype is not looked at: the scan's stride refusal fires
        ({"top.state_dtype": _lib.F16, "top.h0_ptr": None, "top.hT_ptr": None, "scan.u_d_stride": -1}, STRIDE),
    ]]
    + [("varlen_fwd", m, s) for m, s in _SHARED_FWD + _IDS_FWD]
    + [("varlen_bwd", m, s) for m, s in _SHARED_BWD + _IDS]
    + [("varlen_bwd", m, s) for m, s in [
        ({"scan.is_complex": 1, "bwd.workspace_bytes": WS_CPLX - WS_REAL}, UNSUPPORTED),
        ({"scan.dstate": 80, "scan.is_variable_B": 0, "bwd.workspace_bytes": 4 * WS_REAL}, UNSUPPORTED), ({"scan.dstate": 80, "scan.is_variable_B": 0}, SHAPE),
        # its own NULLs before the shared shape, the workspace before the ids
        ({"bwd.dout_ptr": None, "ids.seq_idx_ptr": None, "scan.dstate": 257}, NULL), ({"bwd.du_d_stride": -1, "ids.seq_idx_ptr": None}, STRIDE),
        ({"bwd.workspace_ptr": _addr(29) + 4, "ids.seq_idx_ptr": None}, STRIDE), ({"bwd.workspace_bytes": -1, "ids.seq_idx_ptr": None}, SHAPE),
        ({"bwd.workspace_bytes": -1, "scan.is_variable_B": 0}, SHAPE), ({"scan.is_complex": 1, "ids.seq_idx_ptr": None}, SHAPE),
    ]]
    + [("states", m, s) for m, s in _SHARED_FWD + _IDS_FWD]
    + [("states", {"top." + n: -1}, STRIDE) for n in STATE_STRIDES]
    + [("states", m, s) for m, s in [
        ({"top.num_slots": 0}, SHAPE), ({"top.num_slots": -1}, SHAPE), ({"top.end_slots_ptr": None}, NULL), ({"top.state_ptr": None}, NULL),
        ({"top.end_slots_batch_stride": -1}, STRIDE), ({"top.end_slots_batch_stride": L - 1}, STRIDE),
        # num_slots, then its NULLs, then its strides, then the shared checks, then the ids
        ({"top.num_slots": 0, "top.struct_size": 8}, ABI), ({"top.num_slots": 0, "top.end_slots_ptr": None}, SHAPE),
        ({"top.state_ptr": None, "top.state_slot_stride": -1}, NULL), ({"top.end_slots_ptr": None, "top.end_slots_batch_stride": -1}, NULL),
        ({"top.state_d_stride": -1, "scan.A_ptr": None}, STRIDE), ({"top.end_slots_batch_stride": -1, "scan.dtype": 3}, STRIDE),
        ({"top.state_dstate_stride": -1, "scan.dstate": 257}, STRIDE), ({"top.state_ptr": None, "scan.dstate": 257}, NULL),
        ({"top.num_slots": 0, "scan.A_ptr": None}, SHAPE), ({"top.end_slots_batch_stride": L - 1, "ids.seq_idx_ptr": None}, STRIDE),
        ({"scan.dtype": 3, "ids.seq_idx_ptr": None, "scan.is_complex": 1}, DTYPE),
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


def test_workspace_bytes():
    ws = _lib.load().dimsum_ssm_scan_general_bwd_workspace_bytes
    for bad in ((0, D, L, N, G), (65536, D, L, N, G), (B, 0, L, N, G), (B, D, 0, N, G), (B, D, L, 0, G), (B, D, L, 257, G), (B, D, L, N, 0), (B, D, L, N, 3)):
        assert ws(*bad, 0) == -1 and ws(*bad, 1) == -1, bad
    assert ws(B, D, L, N, G, 0) == WS_REAL == B * 2 * N * 64 * 4             # 2 tiles of 4 steps
    assert ws(B, D, L, N, G, 1) == WS_CPLX == B * 3 * N * 2 * 64 * 4         # 3 tiles of 2 steps, pairs
    assert ws(B, D, L, 80, G, 0) == B * 2 * 80 * 64 * 4                      # the tile does not depend on the number of waves
    assert ws(B, D, L, N, 2, 0) == 2 * WS_REAL                               # every group pads to its own 64-channel block
    assert ws(1, 130, 9, 3, 2, 1) == 1 * 5 * 3 * 2 * (2 * 2 * 64) * 4


# ---------------------------------------------------------------------------------------------------------------------
# part 2: what dimsum_amd.native hands the library, and what the ops layer hands dimsum_amd.native
# ---------------------------------------------------------------------------------------------------------------------
FG = 2                                               # groups of the input-dependent B / C of part 2 (shape otherwise as in part 1)
_CODE = {torch.float32: _lib.F32, torch.float16: _lib.F16, torch.bfloat16: _lib.BF16}
FWD_CASES = ["real", "bare", "const_B", "const_C", "const_BC", "complex", "complex_const_B", "half"]


@pytest.fixture
def scan_lib(filled):
    """`filled` + the one general-scan export that takes no struct: -> (the recording library, _Copies, the shapes the workspace was asked for)"""
    lib, rec = filled
    asked = []
    lib.dimsum_ssm_scan_general_bwd_workspace_bytes = lambda *shape: asked.append(shape) or 4 * 1000 + 2        # no multiple of 4
    return lib, rec, asked


def _operands(case):
    """-> dict of the nine operands of a forward: u and z halves of a wider buffer, B / C with group strides that are not dstate * seqlen,
    constant B / C transposed views"""
    dt = torch.float16 if case == "half" else torch.float32
    cplx = case.startswith("complex")
    k = 2 if cplx else 1
    wdt = torch.complex64 if cplx else torch.float32
    const_B, const_C = case in ("const_B", "const_BC", "complex_const_B"), case in ("const_C", "const_BC")
    o = {"u": torch.randn(B, 2 * D, L).to(dt)[:, D:], "delta": torch.rand(B, D, L).to(dt), "A": torch.randn(D, N, dtype=wdt)}
    o["B"] = torch.randn(N, D, dtype=wdt).t() if const_B else torch.randn(B, FG, N + 1, k * L).to(dt)[:, :, :N]
    o["C"] = torch.randn(N, D, dtype=wdt).t() if const_C else torch.randn(B, 2 * FG, N, k * L).to(dt)[:, ::2]
    bare = case == "bare"
    o["D"], o["delta_bias"] = (None, None) if bare else (torch.randn(D), torch.randn(D))
    o["z"] = None if bare else torch.randn(B, 2 * D, L).to(dt)[:, :D]
    return o


def _args(o):
    return [o[k] for k in ("u", "delta", "A", "B", "C", "D", "z", "delta_bias")]


def _p(t):
    return None if t is None else t.data_ptr()


def _bc_strides(name, t):
    """input-dependent: batch / group / dstate strides; constant: d / dstate strides; the others stay 0"""
    s = dict.fromkeys((f"{name}_batch_stride", f"{name}_d_stride", f"{name}_group_stride", f"{name}_dstate_stride"), 0)
    if t.dim() == 4:
        s[f"{name}_batch_stride"], s[f"{name}_group_stride"], s[f"{name}_dstate_stride"] = t.stride(0), t.stride(1), t.stride(2)
    else:
        s[f"{name}_d_stride"], s[f"{name}_dstate_stride"] = t.stride(0), t.stride(1)
    return s


def _pair(name, t):
    return {f"{name}_batch_stride": t.stride(0) if t is not None else 0, f"{name}_d_stride": t.stride(1) if t is not None else 0}


def _scan_fields(o, softplus, out, x, out_z, struct_size=0):
    """dimsum_ssm_general_params_t as _fill_ssm_general fills it"""
    var_B, var_C = o["B"].dim() == 4, o["C"].dim() == 4
    groups = o["B"].shape[1] if var_B else o["C"].shape[1] if var_C else 1
    return {"struct_size": struct_size, "batch": B, "dim": D, "seqlen": L, "dstate": N, "n_groups": groups, "n_chunks": 1, "delta_softplus": int(softplus),
            "dtype": _CODE[o["u"].dtype], "is_variable_B": int(var_B), "is_variable_C": int(var_C), "is_complex": int(o["A"].is_complex()), "reserved": 0,
            "A_d_stride": N, "A_dstate_stride": 1, **_bc_strides("B", o["B"]), **_bc_strides("C", o["C"]), **_pair("u", o["u"]), **_pair("delta", o["delta"]),
            **_pair("z", o["z"]), **_pair("out", out), **_pair("out_z", out_z),
            "A_ptr": _p(o["A"]), "B_ptr": _p(o["B"]), "C_ptr": _p(o["C"]), "D_ptr": _p(o["D"]), "u_ptr": _p(o["u"]), "delta_ptr": _p(o["delta"]),
            "delta_bias_ptr": _p(o["delta_bias"]), "z_ptr": _p(o["z"]), "out_ptr": _p(out), "x_ptr": _p(x), "out_z_ptr": _p(out_z)}


def _check_fwd_result(res, o, need_out=True, need_x=True):
    """-> (out, x, out_z) of a forward's return list"""
    out, x, *rest = res
    assert len(rest) == (o["z"] is not None)
    assert out is None if not need_out else (out.shape == o["u"].shape and out.dtype == o["u"].dtype and out.is_contiguous())
    assert x is None if not need_x else (tuple(x.shape) == (B, D, 1, 2 * N) and x.dtype == o["A"].dtype)
    if rest:
        assert rest[0].shape == o["z"].shape and rest[0].dtype == o["z"].dtype and rest[0].is_contiguous()
    return out, x, rest[0] if rest else None


def _no_copies(rec, o):
    for t in o.values():
        if t is not None:
            assert rec.of(t) == ([], t)


def _ids():
    return torch.tensor([[0, 0, 1, 1, 1], [0, 1, 1, 2, 2]], dtype=torch.int32)


def _ends():
    return torch.tensor([[-1, 3, -1, -1, 0], [1, -1, 4, -1, 2]], dtype=torch.int32)


def _pool(dtype, slots=5):
    """a non-contiguous (slots, dim, dstate) slice of a larger pool: strides (2 dim (dstate + 1), dstate + 1, 1)"""
    return torch.zeros(2 * slots, D, N + 1, dtype=dtype)[1::2, :, 1:]


@pytest.mark.parametrize("softplus", [True, False], ids=["softplus", "plain"])
@pytest.mark.parametrize("case", FWD_CASES)
def test_general_fwd_fill(scan_lib, case, softplus):
    from dimsum_amd import native
    lib, rec, _ = scan_lib
    o = _operands(case)
    out, x, out_z = _check_fwd_result(native.selective_scan_general_fwd(*_args(o), softplus), o)
    (name, P), = lib.calls
    assert name == "dimsum_ssm_scan_general_fwd"
    assert P == _scan_fields(o, softplus, out, x, out_z, C.sizeof(_lib.SsmGeneralParams))
    _no_copies(rec, o)


@pytest.mark.parametrize("need_out, need_x", [(False, True), (True, False), (False, False)])
@pytest.mark.parametrize("case", ["real", "bare"])
def test_general_fwd_fill_without_out_or_x(scan_lib, case, need_out, need_x):
    from dimsum_amd import native
    lib, _, _ = scan_lib
    o = _operands(case)
    out, x, out_z = _check_fwd_result(native.selective_scan_general_fwd(*_args(o), True, need_out=need_out, need_x=need_x), o, need_out, need_x)
    (name, P), = lib.calls
    assert name == "dimsum_ssm_scan_general_fwd" and P == _scan_fields(o, True, out, x, out_z, C.sizeof(_lib.SsmGeneralParams))
    assert (P["out_ptr"] is None) == (not need_out) and (P["x_ptr"] is None) == (not need_x)


@pytest.mark.parametrize("via", ["wrapper", "keyword"])
@pytest.mark.parametrize("case", ["real", "bare", "half"])
def test_varlen_fwd_fill(scan_lib, case, via):
    from dimsum_amd import native
    lib, rec, _ = scan_lib
    o, seq = _operands(case), _ids()
    res = (native.selective_scan_varlen_fwd(*_args(o), True, seq, need_x=False) if via == "wrapper"
           else native.selective_scan_general_fwd(*_args(o), True, need_x=False, seq_idx=seq))
    out, x, out_z = _check_fwd_result(res, o, True, False)
    (name, V), = lib.calls
    assert name == "dimsum_ssm_scan_varlen_fwd"
    assert V == {"struct_size": C.sizeof(_lib.SsmVarlenParams), "reserved": 0, "scan": _scan_fields(o, True, out, x, out_z), "seq_idx_ptr": seq.data_ptr(),
                 "seq_idx_batch_stride": L}
    _no_copies(rec, o)
    assert rec.of(seq) == ([], seq)


@pytest.mark.parametrize("pool_f32", [True, False], ids=["pool_f32", "pool_like_u"])
@pytest.mark.parametrize("case", ["real", "bare", "half"])
def test_varlen_states_fwd_fill(scan_lib, case, pool_f32):
    from dimsum_amd import native
    lib, rec, _ = scan_lib
    o, seq, ends = _operands(case), _ids(), _ends()
    pool = _pool(torch.float32 if pool_f32 else o["u"].dtype)
    out, x, out_z = _check_fwd_result(native.selective_scan_varlen_states_fwd(*_args(o), False, seq, ends, pool, need_out=case != "real"), o, case != "real")
    (name, E), = lib.calls
    assert name == "dimsum_ssm_scan_varlen_states_fwd"
    assert E == {"struct_size": C.sizeof(_lib.SsmVarlenStatesParams), "num_slots": 5,
                 "varlen": {"struct_size": 0, "reserved": 0, "scan": _scan_fields(o, False, out, x, out_z), "seq_idx_ptr": seq.data_ptr(), "seq_idx_batch_stride": L},
                 "end_slots_ptr": ends.data_ptr(), "end_slots_batch_stride": L, "state_ptr": pool.data_ptr(), "state_slot_stride": 2 * D * (N + 1),
                 "state_d_stride": N + 1, "state_dstate_stride": 1, "state_f32": int(pool.dtype == torch.float32), "reserved": 0}
    _no_copies(rec, o)
    assert rec.of(pool) == ([], pool) and rec.of(ends) == ([], ends)


def _carried(dtype, batch_major=True):
    """a (batch, dim, dstate) state inside a wider cache: strides (dim (dstate + 3), dstate + 3, 1), or a d-major one"""
    t = torch.zeros(B, D, N + 3, dtype=dtype)[:, :, 3:]
    return t if batch_major else torch.zeros(D, B, N, dtype=dtype).transpose(0, 1)


@pytest.mark.parametrize("states", ["initial", "final", "same", "both", "none"])
@pytest.mark.parametrize("case", ["real", "bare", "const_BC", "complex", "half", "half_state"])
def test_carry_fwd_fill(scan_lib, case, states):
    from dimsum_amd import native
    lib, rec, _ = scan_lib
    o = _operands("half" if case == "half_state" else case)
    sdt = torch.complex64 if case == "complex" else torch.float16 if case == "half_state" else torch.float32
    h0 = _carried(sdt) if states in ("initial", "same", "both") else None
    hT = h0 if states == "same" else _carried(sdt, batch_major=False) if states in ("final", "both") else None
    res = native.selective_scan_carry_fwd(*_args(o), True, h0, hT)
    gated = o["z"] is not None
    assert torch.is_tensor(res) and res.shape == o["u"].shape and res.dtype == o["u"].dtype
    assert res.is_contiguous()
    (name, P), = lib.calls
    stride3 = lambda t: dict(zip(("batch", "d", "dstate"), t.stride() if t is not None else (0, 0, 0)))      # noqa: E731
    assert name == "dimsum_ssm_scan_carry_fwd"
    assert P == {"struct_size": C.sizeof(_lib.SsmCarryParams), "state_dtype": 0 if states == "none" else _lib.F16 if case == "half_state" else _lib.F32,
                 "scan": _scan_fields(o, True, None if gated else res, None, res if gated else None),         # with z only the gated output is stored
                 **{f"h0_{k}_stride": v for k, v in stride3(h0).items()}, **{f"hT_{k}_stride": v for k, v in stride3(hT).items()},
                 "h0_ptr": _p(h0), "hT_ptr": _p(hT)}
    _no_copies(rec, o)


BWD_CASES = ["real", "bare", "const_B", "const_C", "const_BC", "complex", "half"]


def _bwd_call(native, o, buffers, seq=None, dz_given=False):
    """-> (the result list, dout, out, the dz handed in, the dB / dC handed in)"""
    dt = o["u"].dtype
    dout = torch.randn(B, 3 * D, L).to(dt)[:, D:2 * D]
    out = torch.randn(B, D, L).to(dt) if o["z"] is not None else None
    dz = torch.empty(B, 2 * D, L, dtype=dt)[:, D:] if dz_given and o["z"] is not None else None
    dB = torch.ones(o["B"].shape).as_subclass(_OnGpu) if buffers and o["B"].dim() == 4 else None
    dC = torch.ones(B, FG, N + 2, o["C"].shape[-1])[:, :, 2:].as_subclass(_OnGpu) if buffers and o["C"].dim() == 4 else None
    args = (*_args(o), dout, out, dz, True)
    res = native.selective_scan_general_bwd(*args, dB=dB, dC=dC) if seq is None else native.selective_scan_varlen_bwd(*args, seq, dB=dB, dC=dC)
    return res, dout, out, dz, dB, dC


def _check_bwd(Q, res, o, dout, out, dz_in, dB_in, dC_in, asked):
    """the backward struct against the result list; the workspace: the size the library named, passed down as it is"""
    du, ddelta, dA, dB, dC, dD, dbias, *rest = res
    gated = o["z"] is not None
    assert len(rest) == gated and (not gated or dz_in is None or rest[0] is dz_in)
    dz = rest[0] if gated else None
    assert du.shape == o["u"].shape and du.dtype == o["u"].dtype and du.is_contiguous() and ddelta.stride() == (D * L, L, 1)
    assert dA.shape == o["A"].shape and dA.dtype == o["A"].dtype
    for g, like, given in ((dB, o["B"], dB_in), (dC, o["C"], dC_in)):
        assert g.shape == like.shape
        if given is not None:                        # the caller's fp32 buffer: zeroed, then returned as it is
            assert g is given and g.dtype == torch.float32 and not g.any()
        else:                                        # its own: in the operand's dtype
            assert g.dtype == like.dtype
    assert (dD is None) == (o["D"] is None) and (dbias is None) == (o["delta_bias"] is None)
    assert dz is None or (dz.shape == o["z"].shape and dz.dtype == o["z"].dtype)
    assert asked == [(B, D, L, N, Q["fwd"]["n_groups"], int(o["A"].is_complex()))]
    assert Q["fwd"] == _scan_fields(o, True, out, None, None)                      # out: only with z
    assert Q["workspace_ptr"] and Q["workspace_bytes"] == 4002
    accum = lambda g, given, like: given if given is not None else g if like.dim() != 4 or like.dtype == torch.float32 else None      # noqa: E731
    want = {"reserved": 0, **_pair("dout", dout), "dA_d_stride": N, "dA_dstate_stride": 1, **_pair("du", du), **_pair("dz", dz), **_pair("ddelta", ddelta),
            "dout_ptr": _p(dout), "dA_ptr": _p(dA), "dD_ptr": _p(dD), "du_ptr": _p(du), "dz_ptr": _p(dz), "ddelta_ptr": _p(ddelta), "ddelta_bias_ptr": _p(dbias)}
    for name, g, given, like in (("dB", dB, dB_in, o["B"]), ("dC", dC, dC_in, o["C"])):
        acc = accum(g, given, like)                  # fp32 accumulators: the returned tensor itself unless it was cast to a 16-bit operand's dtype
        if acc is not None:
            want.update(_bc_strides(name, acc), **{name + "_ptr": acc.data_ptr()})
        else:
            want.update(_bc_strides(name, torch.empty(like.shape)))
            assert Q[name + "_ptr"] and Q[name + "_ptr"] != g.data_ptr()
    assert {k: v for k, v in Q.items() if k in want} == want
    assert set(Q) == set(want) | {"struct_size", "fwd", "dB_ptr", "dC_ptr", "workspace_ptr", "workspace_bytes"}


@pytest.mark.parametrize("buffers", [False, True], ids=["own_dBdC", "caller_dBdC"])
@pytest.mark.parametrize("case", BWD_CASES)
def test_general_bwd_fill(scan_lib, case, buffers):
    from dimsum_amd import native
    lib, rec, asked = scan_lib
    o = _operands(case)
    res, dout, out, dz, dB, dC = _bwd_call(native, o, buffers, dz_given=buffers)
    (name, Q), = lib.calls
    assert name == "dimsum_ssm_scan_general_bwd" and Q["struct_size"] == C.sizeof(_lib.SsmGeneralBwdParams)
    _check_bwd(Q, res, o, dout, out, dz, dB, dC, asked)
    _no_copies(rec, o)
    assert rec.of(dout) == ([], dout)


@pytest.mark.parametrize("buffers", [False, True], ids=["own_dBdC", "caller_dBdC"])
@pytest.mark.parametrize("case", ["real", "bare", "half"])
def test_varlen_bwd_fill(scan_lib, case, buffers):
    from dimsum_amd import native
    lib, rec, asked = scan_lib
    o, seq = _operands(case), _ids()
    res, dout, out, dz, dB, dC = _bwd_call(native, o, buffers, seq=seq)
    (name, V), = lib.calls
    assert name == "dimsum_ssm_scan_varlen_bwd"
    assert {k: v for k, v in V.items() if k != "bwd"} == {"struct_size": C.sizeof(_lib.SsmVarlenBwdParams), "reserved": 0, "seq_idx_ptr": seq.data_ptr(),
                                                         "seq_idx_batch_stride": L}
    assert V["bwd"]["struct_size"] == 0
    _check_bwd(V["bwd"], res, o, dout, out, dz, dB, dC, asked)
    _no_copies(rec, o)


def test_empty_inputs_launch_nothing(scan_lib):
    """u.numel() == 0: the same lists, nothing launched and no workspace asked for"""
    from dimsum_amd import native
    lib, _, asked = scan_lib
    for empty in ("batch", "seqlen"):
        b, l = (0, L) if empty == "batch" else (B, 0)
        u, z, A, Bm, Dv = torch.randn(b, D, l), torch.randn(b, D, l), torch.randn(D, N), torch.randn(b, FG, N, l), torch.randn(D)
        seq, pool = torch.zeros(b, l, dtype=torch.int32), _pool(torch.float32)
        for res in (native.selective_scan_general_fwd(u, u, A, Bm, Bm, Dv, z, Dv, True),
                    native.selective_scan_varlen_fwd(u, u, A, Bm, Bm, Dv, z, Dv, True, seq),
                    native.selective_scan_varlen_states_fwd(u, u, A, Bm, Bm, Dv, z, Dv, True, seq, seq, pool)):
            assert [tuple(t.shape) for t in res] == [(b, D, l), (b, D, (l + 2047) // 2048, 2 * N), (b, D, l)]
        assert [None if t is None else tuple(t.shape) for t in native.selective_scan_general_fwd(u, u, A, Bm, Bm, None, None, None, True, need_out=False)] == [
            None, (b, D, (l + 2047) // 2048, 2 * N)]
        for res in (native.selective_scan_general_bwd(u, u, A, Bm, Bm, Dv, z, Dv, u, u, None, True),
                    native.selective_scan_varlen_bwd(u, u, A, Bm, Bm, Dv, z, Dv, u, u, None, True, seq)):
            assert [tuple(t.shape) for t in res] == [(b, D, l), (b, D, l), (D, N), (b, FG, N, l), (b, FG, N, l), (D,), (D,), (b, D, l)]
            assert not res[2].any() and not res[5].any() and not res[6].any()
        with pytest.raises(RuntimeError, match="selective_scan_carry: u must not be empty"):
            native.selective_scan_carry_fwd(u, u, A, Bm, Bm, Dv, z, Dv, True, None, None)
    assert not lib.calls and not asked


def _refused(msg, fn, *a, **k):
    with pytest.raises(RuntimeError) as e:
        fn(*a, **k)
    assert msg in str(e.value), str(e.value)


def test_refusals_fire_in_their_order():
    """on plain CPU tensors, nothing replaced: every shape, dtype and stride refusal of the shared check comes before the device is looked at,
    in this order; the wrappers' own refusals come before the shared check"""
    from dimsum_amd import native
    o = _operands("real")
    u, delta, A, Bm, Cm, Dv, z, bias = _args(o)
    g = "selective_scan_general: "
    cpu = "no CPU fallback"
    fwd = native.selective_scan_general_fwd
    # each call holds the fault named and the one behind it
    _refused(g + "u must be (batch, dim, seqlen) float32, float16 or bfloat16", fwd, u[0], delta, A.double(), Bm, Cm, Dv, z, bias, True)
    _refused(g + "u must be (batch, dim, seqlen) float32, float16 or bfloat16", fwd, u.double(), delta, A, Bm, Cm, Dv, z, bias, True)
    _refused(g + "A must be a float32 or complex64 (dim, dstate) matrix", fwd, u, delta, torch.randn(D, 257).double(), Bm, Cm, Dv, z, bias, True)
    _refused("selective_scan only supports state dimension <= 256", fwd, u, delta, torch.randn(D + 1, 257), Bm, Cm, Dv, z, bias, True)
    _refused("selective_scan only supports state dimension <= 256", fwd, u, delta, torch.randn(D, 0), Bm, Cm, Dv, z, bias, True)
    _refused(g + "A must have shape (dim, dstate)", fwd, u, delta.half(), A[:4], Bm, Cm, Dv, z, bias, True)
    _refused(g + "delta must be like u", fwd, u, delta[:, :4], A, Bm[:1], Cm, Dv, z, bias, True)
    _refused(g + "input-dependent B must be (batch, groups, dstate, seqlen) of u's dtype (2 * seqlen with complex A)", fwd, u, delta, A, Bm[:, 0], Cm[:1], Dv, z, bias, True)
    _refused(g + "input-dependent B must be (batch, groups, dstate, seqlen)", fwd, u, delta, A, Bm.half(), Cm.transpose(2, 3), Dv, z, bias, True)
    _refused(g + "B.stride(-1) must be 1", fwd, u, delta, A, torch.randn(B, FG, L, N).transpose(2, 3), Cm[:, :, :4], Dv, z, bias, True)
    _refused(g + "input-dependent C must be (batch, groups, dstate, seqlen)", fwd, u, delta, A, Bm, Cm[:, :, :4], Dv, z[0], bias, True)
    _refused(g + "constant B must be (dim, dstate) of A's dtype", fwd, u, delta, A, A[:4], torch.randn(B, FG, L, N).transpose(2, 3), Dv, z, bias, True)
    _refused(g + "constant C must be (dim, dstate) of A's dtype", fwd, u, delta, A, A, A.to(torch.complex64), Dv, z, bias, True)
    _refused(g + "B and C must have the same number of groups", fwd, u, delta, A, Bm, Cm[:, :1], Dv, z.transpose(1, 2), bias, True)
    _refused(g + "dim must be a multiple of the number of groups", fwd, u, delta, A, torch.randn(B, 3, N, L), A, Dv, z.half(), bias, True)
    _refused(g + "u.stride(-1) must be 1", fwd, torch.randn(B, D, 2 * L)[..., ::2], torch.randn(B, D, 2 * L)[..., ::2], A, Bm, Cm, Dv, z.half(), bias, True)
    _refused(g + "delta.stride(-1) must be 1", fwd, u, torch.randn(B, D, 2 * L)[..., ::2], A, Bm, Cm, Dv, torch.randn(B, D, 2 * L)[..., ::2], bias, True)
    _refused(g + "z.stride(-1) must be 1", fwd, u, delta, A, Bm, Cm, Dv, torch.randn(B, D, 2 * L).half()[..., ::2], bias, True)
    _refused(g + "bad z", fwd, u, delta, A, Bm, Cm, Dv[:4], z.half(), bias, True)
    _refused(g + "bad z", fwd, u, delta, A, Bm, Cm, Dv, z[:, :4], bias, True)
    _refused(g + "bad D", fwd, u, delta, A, Bm, Cm, Dv[:4], z, bias.double(), True)
    _refused(g + "bad D", fwd, u, delta, A, Bm, Cm, torch.randn(2 * D)[::2], z, bias, True)
    _refused(g + "bad delta_bias", fwd, u, delta, A, Bm, Cm, Dv, z, bias.double(), True)
    big = torch.zeros(65536, 1, 1)
    _refused(g + "batch <= 65535", fwd, big, big, torch.zeros(1, 1), torch.zeros(65536, 1, 1, 1), torch.zeros(65536, 1, 1, 1), None, None, None, True)
    _refused(cpu, fwd, u, delta, A, Bm, Cm, Dv, z, bias, True)
    # every other entry runs the same check: its sentences keep the shared prefix
    seq, ends, pool = _ids(), _ends(), _pool(torch.float32)
    _refused(g + "delta must be like u", native.selective_scan_varlen_fwd, u, delta[:, :4], A, Bm, Cm, Dv, z, bias, True, seq.long())
    _refused(g + "delta must be like u", native.selective_scan_general_bwd, u, delta[:, :4], A, Bm, Cm, Dv, z, bias, u[:1], None, None, True)
    _refused(g + "delta must be like u", native.selective_scan_varlen_bwd, u, delta[:, :4], A, Bm, Cm, Dv, z, bias, u[:1], None, None, True, seq.long())
    for fn, extra in ((native.selective_scan_varlen_fwd, (seq,)), (native.selective_scan_varlen_states_fwd, (seq, ends, pool)),
                      (native.selective_scan_carry_fwd, (None, None))):
        _refused(cpu, fn, u, delta, A, Bm, Cm, Dv, z, bias, True, *extra)
    for fn, extra in ((native.selective_scan_general_bwd, ()), (native.selective_scan_varlen_bwd, (seq,))):
        _refused(cpu, fn, u, delta, A, Bm, Cm, Dv, z, bias, u[:1], None, None, True, *extra)
    # the wrappers' own: before the shared check
    _refused("selective_scan_varlen_fwd: seq_idx is required", native.selective_scan_varlen_fwd, u[0], delta, A, Bm, Cm, Dv, z, bias, True, None)
    _refused("selective_scan_varlen_bwd: seq_idx is required", native.selective_scan_varlen_bwd, u[0], delta, A, Bm, Cm, Dv, z, bias, u, None, None, True, None)
    who = "selective_scan_varlen_states_fwd"
    st = native.selective_scan_varlen_states_fwd
    _refused(f"{who}: seq_idx is required", st, u[0], delta, A, Bm, Cm, Dv, z, bias, True, None, ends.long(), pool[0])
    _refused(g + "u must be (batch, dim, seqlen) float32, float16 or bfloat16", st, u[0], delta, A, Bm, Cm, Dv, z, bias, True, seq, ends.long(), pool[0])
    _refused(f"{who}: end_slots must be a contiguous int32 (batch, seqlen) = ({B}, {L}) tensor", st, u, delta, A, Bm, Cm, Dv, z, bias, True, seq, ends.long(), pool[0])
    _refused(f"{who}: end_slots must be a contiguous int32", st, u.double(), delta, A, Bm, Cm, Dv, z, bias, True, seq, ends[:, :4], pool)
    _refused(f"{who}: ssm_state must be a pool (num_slots >= 1, dim, dstate)", st, u, delta, A, Bm, Cm, Dv, z, bias, True, seq, ends, pool.double()[:, :, :4])
    _refused(f"{who}: ssm_state must be a pool (num_slots >= 1, dim, dstate)", st, u, delta, A, Bm, Cm, Dv, z, bias, True, seq, ends, pool[:0])
    _refused(f"{who}: ssm_state must be float32 or of u's dtype torch.float32, got torch.float64", st, u, delta[:, :4], A, Bm, Cm, Dv, z, bias, True, seq, ends, pool.double())
    _refused(g + "delta must be like u", st, u, delta[:, :4], A, Bm, Cm, Dv, z, bias, True, seq.long(), ends, pool)
    # the carried state: its own checks before the shared one
    c = "selective_scan_carry: "
    h = torch.zeros(B, D, N)
    carry = native.selective_scan_carry_fwd
    _refused(c + "initial_state must be (batch, dim, dstate)", carry, u, delta[:, :4], A, Bm, Cm, Dv, z, bias, True, h[0], h.double())
    _refused(c + "initial_state must be float32 or of u's dtype (complex64 with complex A)", carry, u, delta, A, Bm, Cm, Dv, z, bias, True, h.half(), h[0])
    _refused(c + "final_state must be (batch, dim, dstate)", carry, u, delta, A, Bm, Cm, Dv, z, bias, True, h, h[:, :4])
    _refused(c + "final_state must be float32 or of u's dtype (complex64 with complex A)", carry, u, delta, A, Bm, Cm, Dv, z, bias, True, None, h.to(torch.complex64))
    oc = _operands("complex")
    _refused(c + "initial_state must be float32 or of u's dtype (complex64 with complex A)", carry, *_args(oc), True, h, None)
    _refused(c + "initial_state and final_state must share one dtype", carry, u.half(), delta[:, :4], A, Bm, Cm, Dv, z, bias, True, h, h.half())
    _refused(c + "an in-place update needs final_state to be initial_state (same strides)", carry, u, delta[:, :4], A, Bm, Cm, Dv, z, bias, True, h,
             torch.as_strided(h, h.shape, (0, N, 1)))
    _refused(g + "delta must be like u", carry, u, delta[:, :4], A, Bm, Cm, Dv, z, bias, True, h, h)


def test_routed_refusals_keep_their_sentences(scan_lib):
    """past the device: the packed rows' ids (under the name of the forward / backward wrapper, whichever function was entered), what the
    packed kernels are not built for, and the backward's own operands"""
    from dimsum_amd import native
    lib, _, asked = scan_lib
    o, oc, ob = _operands("real"), _operands("complex"), _operands("const_B")
    u, delta, A, Bm, Cm, Dv, z, bias = _args(o)
    seq, ends, pool = _ids(), _ends(), _pool(torch.float32)
    not_built = "(the packed-row kernels are instantiated for real A with input-dependent B and C)"
    for who, fn, more in (("selective_scan_varlen_fwd", native.selective_scan_varlen_fwd, lambda s: (True, s)),
                          ("selective_scan_varlen_fwd", native.selective_scan_varlen_states_fwd, lambda s: (True, s, ends, pool)),
                          ("selective_scan_varlen_bwd", native.selective_scan_varlen_bwd, lambda s: (u[:1], None, None, True, s))):
        for bad in (seq.long(), seq[:, :4].contiguous(), torch.zeros(L, B, dtype=torch.int32).t(), seq[0]):
            _refused(f"{who}: seq_idx must be a contiguous int32 (batch, seqlen) = ({B}, {L}) tensor", fn, *_args(o), *more(bad))
        _refused(f"{who}: seq_idx must be a contiguous int32", fn, *_args(oc), *more(seq.long()))
        if fn is not native.selective_scan_varlen_states_fwd:       # (whose own pool check wants a real state of A's width first; same sentences)
            _refused(f"{who}: seq_idx with a complex A is not built {not_built}", fn, *_args(oc), *more(seq))
        _refused(f"{who}: seq_idx with a constant B or C is not built {not_built}", fn, *_args(ob), *more(seq))
        _refused(f"{who}: seq_idx with a constant B or C is not built {not_built}", fn, *_args(_operands("const_C")), *more(seq))
    _refused("selective_scan_general_fwd: end_slots belong to packed rows (seq_idx)", native.selective_scan_general_fwd, *_args(o), True, end_slots=ends, ssm_state=pool)
    _refused("selective_scan_carry: u must not be empty", native.selective_scan_carry_fwd, u[:0], delta[:0], A, Bm[:0], Cm[:0], Dv, z[:0], bias, True, None, None)
    dout = torch.randn(B, D, L)
    for fn, extra in ((native.selective_scan_general_bwd, ()), (native.selective_scan_varlen_bwd, (seq,))):
        bwd = lambda *a, **k: fn(*_args(o), *a, True, *extra, **k)      # noqa: E731  (dout, out, dz)
        g = "selective_scan_general_bwd: "
        _refused(g + "bad dout", bwd, dout[:1], None, None)
        _refused(g + "bad dout", bwd, dout.half(), None, None)
        _refused(g + "bad dout", bwd, torch.randn(B, D, 2 * L)[..., ::2], None, None)
        _refused(g + "`out` of the forward is required with z", bwd, dout, None, dout[:1])
        _refused(g + "`out` of the forward is required with z", bwd, dout, torch.randn(B, D, 2 * L)[..., ::2], None)
        _refused(g + "bad dz", bwd, dout, dout, dout[:1])
        _refused(g + "bad dz", bwd, dout, dout, dout.half())
        good = torch.zeros(Bm.shape).as_subclass(_OnGpu)
        _refused(g + "bad dB / dC buffer", bwd, dout, dout, None, dB=torch.zeros(Bm.shape))                  # not on the GPU
        _refused(g + "bad dB / dC buffer", bwd, dout, dout, None, dB=good.half())
        _refused(g + "bad dB / dC buffer", bwd, dout, dout, None, dB=good, dC=good[:1])
    _refused("selective_scan_general_bwd: bad dB / dC buffer", native.selective_scan_general_bwd, *_args(ob), dout, dout, None, True,
             dB=torch.zeros(D, N).as_subclass(_OnGpu))                                                       # a constant B takes no buffer
    assert not lib.calls and not asked


# ---- the ops layer: what selective_scan_fn hands native on each of its four routes ---------------------------------------------------------------
def _described(t):
    return None if t is None else (tuple(t.shape), t.stride(), t.data_ptr()) if torch.is_tensor(t) else t


@pytest.fixture
def native_standins(monkeypatch):
    """every native scan function selective_scan_fn can reach replaced by a stand-in that records (name, what each argument looks like, the
    keywords) and returns lists of the right shapes; gone again, with the recorded calls left, when the test ends"""
    from dimsum_amd import native
    calls = []

    def fwd(name):
        def run(u, delta, A, Bm, Cm, Dv, z, bias, softplus, *more, **kw):
            calls.append((name, [_described(t) for t in (u, delta, A, Bm, Cm, Dv, z, bias, softplus, *more)], kw))
            if name == "selective_scan_carry_fwd":
                if more[1] is not None:
                    more[1].fill_(7.0)
                return torch.full_like(delta, 2.0)
            res = [torch.full_like(delta, 1.0), torch.full((u.shape[0], u.shape[1], 1, 2 * A.shape[1]), 3.0) if kw.get("need_x", True) else None]
            return res + ([torch.full_like(delta, 2.0)] if z is not None else []) + ([torch.zeros(1)] if kw.get("need_ckpt") else [])
        return run

    def bwd(name):
        def run(u, delta, A, Bm, Cm, Dv, z, bias, dout, *more, **kw):
            calls.append((name, [_described(t) for t in (u, delta, A, Bm, Cm, Dv, z, bias, dout, *more)], {k: _described(v) for k, v in kw.items()}))
            # dD, ddelta_bias (and below dz) come back even where the operand is absent: the autograd classes must drop them
            res = [torch.full_like(u, 1.0), torch.full_like(delta, 2.0), torch.full_like(A, 3.0), torch.full_like(Bm, 4.0), torch.full_like(Cm, 5.0),
                   torch.full((u.shape[1],), 6.0), torch.full((u.shape[1],), 7.0)]
            return res + [torch.full_like(u, 8.0)]
        return run

    with monkeypatch.context() as m:
        for name in ("selective_scan_fwd", "selective_scan_general_fwd", "selective_scan_varlen_fwd", "selective_scan_varlen_states_fwd", "selective_scan_carry_fwd"):
            m.setattr(native, name, fwd(name))
        for name in ("selective_scan_bwd", "selective_scan_general_bwd", "selective_scan_varlen_bwd"):
            m.setattr(native, name, bwd(name))
        yield calls


def _ops_operands(on_gpu, rank3=True, extras=True):
    """u unit-stride inside a wider buffer, delta strided along the sequence, three-dim B, a strided D"""
    mk = (lambda t: t.as_subclass(_OnGpu)) if on_gpu else (lambda t: t)
    u = mk(torch.randn(B, 2 * D, L)[:, D:])
    delta = mk(torch.rand(B, D, 2 * L)[..., ::2])
    A = mk(-torch.rand(D, 12))
    Bm = mk(torch.randn(B, 12, L)) if rank3 else mk(torch.randn(B, FG, 12, L))
    Cm = mk(torch.randn(B, 12, 2 * L)[..., ::2]) if rank3 else mk(torch.randn(B, FG, 12, L))
    Dv, z, bias = (mk(torch.randn(2 * D)[::2]), mk(torch.randn(B, D, L)), mk(torch.rand(D))) if extras else (None, None, None)
    return u, delta, A, Bm, Cm, Dv, z, bias


def _check_normalised(got, ops, rank3):
    """the eight operands as a native function must receive them from the ops layer"""
    u, delta, A, Bm, Cm, Dv, z, bias = ops
    assert got[0] == _described(u)                                                   # unit stride: passed as it is, not copied
    assert got[1][:2] == (tuple(delta.shape), (D * L, L, 1)) and got[1][2] != delta.data_ptr()      # strided along the sequence: copied
    assert got[2] == _described(A)
    if rank3:
        assert got[3] == ((B, 1, 12, L), (12 * L, 12 * L, L, 1), Bm.data_ptr())      # three-dim -> four-dim, a view
        assert got[4][:2] == ((B, 1, 12, L), (12 * L, 12 * L, L, 1)) and got[4][2] != Cm.data_ptr()
    else:
        assert got[3] == _described(Bm) and got[4] == _described(Cm)
    if Dv is None:
        assert got[5:8] == [None, None, None]
    else:
        assert got[5][:2] == ((D,), (1,)) and got[5][2] != Dv.data_ptr()             # D.contiguous()
        assert got[6] == _described(z) and got[7] == _described(bias)


@pytest.mark.parametrize("extras", [True, False], ids=["D_z_bias", "bare"])
@pytest.mark.parametrize("rank3", [True, False], ids=["BC_3d", "BC_4d"])
@pytest.mark.parametrize("route", ["tuned", "general", "seq_idx"])
def test_selective_scan_fn_autograd_routes(native_standins, route, rank3, extras):
    """forward and backward of the two autograd classes: the native pair reached, the operands it gets, and the gradients that come back --
    dB / dC in the caller's rank, nothing for an absent D / z / delta_bias although native returned something"""
    from dimsum_amd.ops import selective_scan_fn
    calls = native_standins
    ops = _ops_operands(on_gpu=route == "general", rank3=rank3, extras=extras)
    leaves = [t.requires_grad_() if t is not None else None for t in ops]
    kw = {"seq_idx": _ids()} if route == "seq_idx" else {}
    out, last = selective_scan_fn(*leaves, delta_softplus=True, return_last_state=True, **kw)
    assert out.eq(2.0 if extras else 1.0).all() and tuple(last.shape) == (B, D, 12) and last.eq(3.0).all()
    out.sum().backward()
    (f_name, f_args, f_kw), (b_name, b_args, b_kw) = calls
    assert (f_name, b_name) == {"tuned": ("selective_scan_fwd", "selective_scan_bwd"), "general": ("selective_scan_general_fwd", "selective_scan_general_bwd"),
                                "seq_idx": ("selective_scan_varlen_fwd", "selective_scan_varlen_bwd")}[route]
    _check_normalised(f_args, ops, rank3)
    assert f_args[8] is True and f_kw == ({"need_ckpt": True} if route == "tuned" else {})
    assert f_args[9:] == ([_described(kw["seq_idx"])] if route == "seq_idx" else [])
    assert b_args[:8] == f_args[:8] and b_args[8][:2] == ((B, D, L), (D * L, L, 1))
    if route == "tuned":          # dout, x, out, dz, delta_softplus, recompute_out_z
        assert b_args[9][0] == (B, D, 1, 24) and (b_args[10] is None) == (not extras) and b_args[11:] == [None, True, False] and b_kw == {"ckpt": ((1,), (1,), b_kw["ckpt"][2])}
    else:                         # dout, out, dz, delta_softplus(, seq_idx)
        assert (b_args[9] is None) == (not extras) and b_args[10:12] == [None, True] and b_kw == {}
        assert b_args[12:] == ([_described(kw["seq_idx"])] if route == "seq_idx" else [])
    for t, val in zip(leaves, (1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 8.0, 7.0)):
        assert t is None or (t.grad.shape == t.shape and t.grad.eq(val).all())


@pytest.mark.parametrize("extras", [True, False], ids=["D_z_bias", "bare"])
@pytest.mark.parametrize("rank3", [True, False], ids=["BC_3d", "BC_4d"])
@pytest.mark.parametrize("route", ["end_slots", "initial_state"])
def test_selective_scan_fn_inference_routes(native_standins, route, rank3, extras):
    from dimsum_amd.ops import selective_scan_fn
    calls = native_standins
    ops = _ops_operands(on_gpu=False, rank3=rank3, extras=extras)
    if route == "end_slots":
        seq, ends, pool = _ids(), _ends(), torch.zeros(5, D, 12)
        for last_state in (True, False):
            res = selective_scan_fn(*ops, delta_softplus=True, return_last_state=last_state, seq_idx=seq, end_slots=ends, ssm_state=pool)
            out = res[0] if last_state else res
            assert out.eq(2.0 if extras else 1.0).all() and (not last_state or (tuple(res[1].shape) == (B, D, 12) and res[1].eq(3.0).all()))
            name, args, kw = calls[-1]
            assert name == "selective_scan_varlen_states_fwd" and kw == {"need_x": last_state}
            _check_normalised(args, ops, rank3)
            assert args[8:] == [True, _described(seq), _described(ends), _described(pool)]
        assert len(calls) == 2
    else:
        h0 = torch.zeros(B, D, 12 + 1, dtype=torch.float32)[:, :, 1:]
        out, last = selective_scan_fn(*ops, delta_softplus=True, return_last_state=True, initial_state=h0)
        assert out.eq(2.0).all() and last.eq(7.0).all() and last.shape == h0.shape and last.dtype == h0.dtype and last.data_ptr() != h0.data_ptr()
        assert selective_scan_fn(*ops, delta_softplus=False, initial_state=h0).eq(2.0).all()
        (name, args, kw), (name2, args2, _) = calls
        assert name == name2 == "selective_scan_carry_fwd" and kw == {}
        _check_normalised(args, ops, rank3)
        assert args[8:] == [True, _described(h0), _described(last)] and args2[8:] == [False, _described(h0), None]


def test_standins_are_gone():
    """nothing of the fixtures above outlives its test"""
    from dimsum_amd import native
    for name in ("selective_scan_fwd", "selective_scan_bwd", "selective_scan_general_fwd", "selective_scan_general_bwd", "selective_scan_varlen_fwd",
                 "selective_scan_varlen_bwd", "selective_scan_varlen_states_fwd", "selective_scan_carry_fwd"):
        assert getattr(native, name).__module__ == "dimsum_amd.native" and getattr(native, name).__name__ == name
    assert _lib.load().__class__.__name__ != "_RecordingLib"
