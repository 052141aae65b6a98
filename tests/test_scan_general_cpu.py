"""The general selective scan (csrc/ssm_scan_general.hip) without a GPU: the C ABI's symbols, struct layouts and refusals (every case is
refused before a launch; the pointers are made-up addresses that are never read), the routing rule of selective_scan_fn, and the plain-torch
restatement of the operator (scan_general_ref.py) against fixtures of the reference's selective_scan_ref in float64 / complex128
(tools/gen_golden.py --only scan_general)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import golden
from dimsum_amd import _lib
from scan_general_ref import scan_restated
from test_host_logic import _header_layout

OK, NULL, DTYPE, SHAPE, STRIDE, UNSUPPORTED, LAUNCH, ABI = range(8)
B, D, L, N, G = 2, 72, 37, 64, 1


def _addr(i):
    return 0x10000000 + 0x100000 * i


def _fill_fwd(F):
    F.batch, F.dim, F.seqlen, F.dstate, F.n_groups, F.n_chunks, F.delta_softplus, F.dtype = B, D, L, N, G, 1, 1, _lib.F32
    F.is_variable_B, F.is_variable_C, F.is_complex = 1, 1, 0
    F.A_d_stride, F.A_dstate_stride = N, 1
    for t in ("B", "C"):
        setattr(F, t + "_batch_stride", G * N * L), setattr(F, t + "_group_stride", N * L), setattr(F, t + "_dstate_stride", L)
    for t in ("u", "delta", "z", "out", "out_z"):
        setattr(F, t + "_batch_stride", D * L), setattr(F, t + "_d_stride", L)
    for i, t in enumerate(("A", "B", "C", "D", "u", "delta", "delta_bias", "z", "out", "x", "out_z")):
        setattr(F, t + "_ptr", _addr(i))


def _make(entry, lib):
    if entry == "fwd":
        P = _lib.SsmGeneralParams()
        _fill_fwd(P)
        return lib.dimsum_ssm_scan_general_fwd, P, {"top": P, "fwd": P}
    Q = _lib.SsmGeneralBwdParams()
    _fill_fwd(Q.fwd)
    Q.dA_d_stride, Q.dA_dstate_stride = N, 1
    for t in ("dB", "dC"):
        setattr(Q, t + "_batch_stride", G * N * L), setattr(Q, t + "_group_stride", N * L), setattr(Q, t + "_dstate_stride", L)
    for t in ("dout", "du", "dz", "ddelta"):
        setattr(Q, t + "_batch_stride", D * L), setattr(Q, t + "_d_stride", L)
    for i, t in enumerate(("dout", "dA", "dB", "dC", "dD", "du", "dz", "ddelta", "ddelta_bias", "workspace")):
        setattr(Q, t + "_ptr", _addr(20 + i))
    Q.workspace_bytes = lib.dimsum_ssm_scan_general_bwd_workspace_bytes(B, D, L, N, G, 0)
    return lib.dimsum_ssm_scan_general_bwd, Q, {"top": Q, "fwd": Q.fwd, "bwd": Q}


def _status(entry, mut):
    lib = _lib.load()
    fn, P, parts = _make(entry, lib)
    for key, val in mut.items():
        if key == "null":
            return fn(None, None)
        prefix, field = key.split(".")
        setattr(parts[prefix], field, val)
    return fn(P, None)


_SHARED = ([({"null": 1}, NULL), ({"top.struct_size": 0}, ABI)]
           + [({"fwd." + t + "_ptr": None}, NULL) for t in ("A", "B", "C", "u", "delta")]
           + [({"fwd.dstate": 0}, SHAPE), ({"fwd.dstate": 257}, SHAPE), ({"fwd.batch": 0}, SHAPE), ({"fwd.dim": 0}, SHAPE), ({"fwd.seqlen": 0}, SHAPE),
              ({"fwd.n_groups": 5}, SHAPE), ({"fwd.n_chunks": 2}, SHAPE), ({"fwd.is_variable_B": 0, "fwd.is_variable_C": 0, "fwd.n_groups": 2}, SHAPE),
              ({"fwd.dtype": 3}, DTYPE), ({"fwd.dtype": -1}, DTYPE), ({"fwd.u_d_stride": -L}, STRIDE), ({"fwd.B_dstate_stride": -1}, STRIDE),
              # the documented order: pointers, then shape, then dtype, then strides
              ({"fwd.A_ptr": None, "fwd.dstate": 0}, NULL), ({"fwd.dstate": 257, "fwd.dtype": 3}, SHAPE), ({"fwd.dtype": 3, "fwd.u_d_stride": -L}, DTYPE),
              ({"top.struct_size": 0, "fwd.A_ptr": None}, ABI)])
CASES = ([("fwd", m, s) for m, s in _SHARED]
         + [("fwd", m, s) for m, s in [({"top.struct_size": C.sizeof(_lib.SsmGeneralParams) + 8}, ABI), ({"fwd.out_z_ptr": None}, NULL),
                                       ({"fwd.x_ptr": _addr(9) + 4}, STRIDE)]]
         + [("bwd", m, s) for m, s in _SHARED]
         + [("bwd", m, s) for m, s in [({"top.struct_size": C.sizeof(_lib.SsmGeneralBwdParams) - 8}, ABI)]
            + [({"bwd." + t + "_ptr": None}, NULL) for t in ("dout", "dA", "dB", "dC", "du", "ddelta", "workspace", "dz")]
            + [({"fwd.out_ptr": None}, NULL), ({"bwd.du_d_stride": -1}, STRIDE), ({"bwd.workspace_ptr": _addr(29) + 4}, STRIDE),
               ({"bwd.workspace_bytes": 0}, SHAPE), ({"bwd.workspace_ptr": _addr(29) + 4, "bwd.workspace_bytes": 0}, STRIDE),
               # a workspace sized for real weights is too small for complex ones
               ({"fwd.is_complex": 1}, SHAPE)]])


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0] + ":" + ",".join(f"{k}={v}" for k, v in c[1].items()))
def test_refusals(case):
    entry, mut, want = case
    assert want not in (OK, LAUNCH)
    assert _status(entry, mut) == want


def test_symbols_and_struct_layouts():
    lib = _lib.load()
    header = open(_lib._HERE + "/../include/dimsum_hip.h").read()
    for name in ("dimsum_ssm_scan_general_fwd", "dimsum_ssm_scan_general_bwd", "dimsum_ssm_scan_general_bwd_workspace_bytes"):
        assert name in _lib.EXPORTS and hasattr(lib, name) and f"{name}(" in header, name
    assert lib.dimsum_abi_version() == 18
    pairs = [("dimsum_ssm_general_params_t", _lib.SsmGeneralParams), ("dimsum_ssm_general_bwd_params_t", _lib.SsmGeneralBwdParams),
             ("dimsum_ssm_params_t", _lib.SsmParams), ("dimsum_ssm_bwd_params_t", _lib.SsmBwdParams)]
    layout = _header_layout(pairs)
    for cname, mirror in pairs:
        size, offs = layout[cname]
        assert size == C.sizeof(mirror), cname
        for f, _ in mirror._fields_:
            assert offs[f] == getattr(mirror, f).offset, (cname, f)


def test_workspace_query():
    lib = _lib.load()
    q = lib.dimsum_ssm_scan_general_bwd_workspace_bytes
    # the state before every tile of 64 / (16 states per wave x reals per state) = 4 (complex: 2) steps, channels padded to 64 per group
    assert q(2, 72, 37, 64, 1, 0) == 2 * ((37 + 3) // 4) * 64 * 128 * 4
    assert q(2, 72, 37, 256, 1, 0) == 2 * ((37 + 3) // 4) * 256 * 128 * 4
    assert q(2, 72, 37, 64, 1, 1) == 2 * ((37 + 1) // 2) * 64 * 2 * 128 * 4
    assert q(2, 128, 64, 12, 2, 0) == 2 * 16 * 12 * 128 * 4
    for bad in ((0, 72, 37, 64, 1, 0), (2, 72, 37, 0, 1, 0), (2, 72, 37, 257, 1, 0), (2, 72, 37, 64, 5, 0)):
        assert q(*bad) == -1


def test_routing_rule():
    from dimsum_amd.native import scan_takes_general_path as route
    for n in (4, 8, 16, 32):
        assert not route(n) and not route(n, False, True, True, force=False)
        assert route(n, is_variable_B=False) and route(n, is_variable_C=False) and route(n, is_complex=True) and route(n, force=True)
    for n in (1, 3, 12, 64, 256):
        assert route(n)
    # the host-side switch of tests and measurements is an argument, not something the rule reads
    from dimsum_amd import native
    assert not native.scan_general_forced()
    with native.scan_force_general():
        assert native.scan_general_forced() and not route(16) and route(16, force=native.scan_general_forced())
    assert not native.scan_general_forced()


def test_native_checks_are_loud_without_a_gpu():
    from dimsum_amd import native
    u = torch.randn(1, 4, 8)
    A = -torch.rand(4, 12)
    Bm = torch.randn(1, 1, 12, 8)
    with pytest.raises(RuntimeError, match="stride"):
        native.selective_scan_general_fwd(u.transpose(1, 2).contiguous().transpose(1, 2), u, A, Bm, Bm, None, None, None, True)
    with pytest.raises(RuntimeError, match="stride"):
        native.selective_scan_general_fwd(u, u, A, torch.randn(1, 1, 8, 12).transpose(2, 3), Bm, None, None, None, True)
    with pytest.raises(RuntimeError, match="<= 256"):
        native.selective_scan_general_fwd(u, u, -torch.rand(4, 257), torch.randn(1, 1, 257, 8), torch.randn(1, 1, 257, 8), None, None, None, True)
    with pytest.raises(RuntimeError, match="constant B"):
        native.selective_scan_general_fwd(u, u, A, torch.randn(4, 12, dtype=torch.complex64), Bm, None, None, None, True)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        native.selective_scan_general_fwd(u, u, A, Bm, Bm, None, None, None, True)


GOLDENS = ["scang_real_vv_n12", "scang_real_cv_n3", "scang_real_cc_n20", "scang_cplx_vv_n5", "scang_cplx_vc_n12", "scang_cplx_cc_n3"]


@pytest.mark.parametrize("name", GOLDENS)
def test_restatement_matches_the_reference(name):
    """float64 against float64: 1e-10 relative to each tensor's largest element"""
    g = golden(name)
    leaf = lambda k: torch.from_numpy(g[k]).requires_grad_() if k in g.files else None
    t = {k: leaf(k) for k in ("u", "delta", "A", "B", "C", "D", "z", "delta_bias")}
    out, _, last, _ = scan_restated(t["u"], t["delta"], t["A"], t["B"], t["C"], t["D"], t["z"], t["delta_bias"], bool(g["softplus"]))
    out.backward(torch.from_numpy(g["dout"]))

    def close(got, want, what):
        got, want = got.detach().numpy(), np.asarray(want)
        assert got.shape == want.shape and got.dtype == want.dtype, what
        assert np.abs(got - want).max() <= 1e-10 * max(np.abs(want).max(), 1.0), what

    close(out, g["out"], "out")
    close(last, g["last_state"], "last_state")
    for k in ("u", "delta", "A", "B", "C", "D", "z", "delta_bias"):
        if t[k] is not None:
            close(t[k].grad, g["d" + k], "d" + k)
