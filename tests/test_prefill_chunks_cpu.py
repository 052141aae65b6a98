"""Continuing a cached sequence by any number of tokens, without a GPU: the C ABI of the two entry points (dimsum_ssm_scan_carry_fwd,
dimsum_causal_conv1d_chunk) and the refusals of their wrappers; the two plain-torch restatements (ops: causal_conv1d_chunk_torch,
selective_scan_carry_torch); Mamba / CondMamba.extend and utils.chunked_prefill on the CPU oracle backend with the two native calls replaced
by the restatements. The reference is always ONE pass over the whole sequence from zero states: the restatement's own, or the reference
module's recorded rows in mixer_step.npz (*_y_full, *_conv_state, *_ssm_state). Bound: test_mixer_step_cpu.py's fp32 one (rtol 3e-4,
atol 1e-3); conv states are compared exactly; float64 splits of the restatements to 1e-12."""
import ctypes

import pytest
import torch

from conftest import golden
from oracle.torch_backend import cpu_oracle_backend
from test_host_logic import _header_layout
from test_mixer_step_cpu import CONV_CASES, L, close, conv_case, mixer

T = torch.from_numpy
STRUCTS = [("dimsum_ssm_carry_params_t", "SsmCarryParams"), ("dimsum_conv_chunk_params_t", "ConvChunkParams")]
SYMBOLS = (("dimsum_ssm_scan_carry_fwd", "SsmCarryParams"), ("dimsum_causal_conv1d_chunk", "ConvChunkParams"))


# ---- plain-torch stand-ins of native.causal_conv1d_chunk / native.selective_scan_carry_fwd (same signatures and results) -------------------------
def native_conv_chunk(x, conv_state, weight, bias, silu_activation):
    from dimsum_amd.ops import causal_conv1d_chunk_torch
    return causal_conv1d_chunk_torch(x, conv_state, weight, bias, "silu" if silu_activation else None)


def native_scan_carry(u, delta, A, B, C, D, z, delta_bias, delta_softplus, initial_state, final_state):
    from dimsum_amd.ops import selective_scan_carry_torch
    out, h = selective_scan_carry_torch(u, delta, A, B, C, D, z, delta_bias, delta_softplus, initial_state)
    if final_state is not None:
        final_state.copy_(h)
    return out


@pytest.fixture
def chunk_backend(monkeypatch):
    from dimsum_amd import native
    from test_mixer_step_cpu import native_conv_update, native_state_update
    monkeypatch.setattr(native, "causal_conv1d_update", native_conv_update)
    monkeypatch.setattr(native, "selective_state_update", native_state_update)
    monkeypatch.setattr(native, "causal_conv1d_chunk", native_conv_chunk)
    monkeypatch.setattr(native, "selective_scan_carry_fwd", native_scan_carry)
    with cpu_oracle_backend():
        yield


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------------------------
def test_struct_layouts_exports_and_stale_structs():
    from dimsum_amd import _lib
    pairs = [(c, getattr(_lib, m)) for c, m in STRUCTS]
    layout = _header_layout(pairs)
    for cname, mirror in pairs:
        size, offs = layout[cname]
        assert size == ctypes.sizeof(mirror), cname
        assert offs == {f: getattr(mirror, f).offset for f, _ in mirror._fields_}, cname
        assert mirror._fields_[0][0] == "struct_size" and mirror().struct_size == size
    scan = _header_layout([("dimsum_ssm_general_params_t", _lib.SsmGeneralParams)])["dimsum_ssm_general_params_t"]
    assert scan[0] == ctypes.sizeof(_lib.SsmGeneralParams) == _lib.SsmCarryParams.scan.size      # nested whole: the existing struct is untouched
    lib = _lib.load()
    assert lib.dimsum_abi_version() == 18
    header = open(_lib.os.path.join(_lib._HERE, "..", "include", "dimsum_hip.h")).read()
    assert "#define DIMSUM_ABI_VERSION 18" in header
    for name, m in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(lib, name) and f"int {name}(" in header, name
        fn, p = getattr(lib, name), getattr(_lib, m)()
        assert fn(p, None) == 1                                   # a zeroed struct of the right size: the first NULL pointer, nothing launched
        p.struct_size -= 8
        assert fn(p, None) == 7                                   # a stale struct is refused before anything is read
        assert fn(None, None) == 1


def _carry_params(addr):
    """a dimsum_ssm_carry_params_t whose every check passes up to the LAST one this test trips (host memory, never dereferenced)"""
    from dimsum_amd import _lib
    P = _lib.SsmCarryParams()
    s = P.scan
    for f in ("A_ptr", "B_ptr", "C_ptr", "u_ptr", "delta_ptr"):
        setattr(s, f, addr)
    s.batch, s.dim, s.seqlen, s.dstate, s.n_groups, s.n_chunks = 2, 8, 5, 16, 1, 1
    s.is_variable_B = s.is_variable_C = 1
    return P


def test_library_refuses_bad_calls_before_any_launch():
    """every call below fails a host-side check: no launch is ever reached (there is no GPU here)"""
    from dimsum_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    addr = ctypes.addressof(buf)
    fn = lib.dimsum_ssm_scan_carry_fwd
    P = _carry_params(addr)
    for field, bad in (("dstate", 0), ("dstate", 257), ("seqlen", 0), ("batch", 0), ("n_chunks", 2), ("n_groups", 3)):
        P = _carry_params(addr)
        setattr(P.scan, field, bad)
        assert fn(P, None) == 3, (field, bad)                     # DIMSUM_ERR_SHAPE
    P = _carry_params(addr)
    P.scan.dtype = 3
    assert fn(P, None) == 2                                       # DIMSUM_ERR_DTYPE: the scan's
    for dtype, cplx, sdt in ((1, 0, 2), (0, 0, 1), (2, 0, 3), (1, 1, 1), (0, 0, -1)):
        for which in ("h0_ptr", "hT_ptr"):
            P = _carry_params(addr)
            P.scan.dtype, P.scan.is_complex, P.state_dtype = dtype, cplx, sdt
            P.scan.u_d_stride = -1                                # the dtype is checked before any stride
            setattr(P, which, addr)
            assert fn(P, None) == 2, (dtype, cplx, sdt, which)    # DIMSUM_ERR_DTYPE: the state's
    for field in ("h0_batch_stride", "h0_d_stride", "h0_dstate_stride", "hT_batch_stride", "hT_d_stride", "hT_dstate_stride"):
        P = _carry_params(addr)
        P.h0_ptr = P.hT_ptr = addr
        setattr(P, field, -1)
        assert fn(P, None) == 4, field                            # DIMSUM_ERR_STRIDE
    P = _carry_params(addr)
    P.scan.u_d_stride = -1
    assert fn(P, None) == 4
    P = _carry_params(addr)
    P.scan.z_ptr = addr                                           # z without out_z
    assert fn(P, None) == 1

    fn = lib.dimsum_causal_conv1d_chunk
    Q = _lib.ConvChunkParams()
    Q.x_ptr = Q.weight_ptr = Q.out_ptr = addr
    assert fn(Q, None) == 1                                       # no conv_state
    Q.conv_state_ptr = addr
    for B, D, S, W in ((1, 4, 3, 1), (1, 4, 3, 5), (0, 4, 3, 4), (1, 0, 3, 4), (1, 4, 0, 4), (-1, 4, 3, 4)):
        Q.batch, Q.dim, Q.seqlen, Q.width = B, D, S, W
        assert fn(Q, None) == 3, (B, D, S, W)
    Q.batch, Q.dim, Q.seqlen, Q.width, Q.dtype = 1, 4, 3, 4, 3
    assert fn(Q, None) == 2
    Q.dtype = 0
    for field in ("x_batch_stride", "x_c_stride", "state_batch_stride", "state_c_stride", "state_w_stride", "out_batch_stride", "out_c_stride"):
        setattr(Q, field, -1)
        assert fn(Q, None) == 4, field
        setattr(Q, field, 0)


def test_wrappers_refuse_shapes_dtypes_and_strides_before_the_device():
    from dimsum_amd import native, ops
    x, st, w = torch.zeros(2, 8, 5), torch.zeros(2, 8, 4), torch.zeros(8, 4)
    for args, why in (((x[0], st, w, None, True), "batch, dim, seqlen"), ((x.double(), st.double(), w, None, True), "float32, float16"),
                      ((x, st, torch.zeros(8, 5), None, True), "between 2 and 4"), ((x, st[:, :, :3], w, None, True), "conv_state must be"),
                      ((x, st.half(), w, None, True), "conv_state must be"), ((x, st, w, torch.zeros(7), True), "bias must be"),
                      ((x.transpose(1, 2).contiguous().transpose(1, 2), st, w, None, True), r"stride\(-1\)"), ((x, st, w, None, True), "GPU tensor")):
        with pytest.raises(RuntimeError, match=why):
            native.causal_conv1d_chunk(*args)
    with pytest.raises(NotImplementedError, match="silu"):
        ops.causal_conv1d_chunk(x, st, w, None, "gelu")
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.causal_conv1d_chunk(x, st, w, None, "silu")
    u, A, Bm, h = torch.zeros(2, 8, 5), -torch.ones(8, 16), torch.zeros(2, 1, 16, 5), torch.zeros(2, 8, 16)
    call = lambda **kw: native.selective_scan_carry_fwd(*[kw.get(k, v) for k, v in (("u", u), ("delta", u), ("A", A), ("B", Bm), ("C", Bm), ("D", None), ("z", None),  # noqa: E731
                                                                                    ("delta_bias", None), ("sp", True), ("h0", h), ("hT", h))])
    for kw, why in ((dict(h0=h[:, :, :8]), "initial_state must be"), (dict(hT=h[0]), "final_state must be"), (dict(h0=h.double()), "float32 or of u's dtype"),
                    (dict(h0=h.half(), hT=h.half()), "float32 or of u's dtype"), (dict(hT=h.to(torch.complex64)), "float32 or of u's dtype"),
                    (dict(h0=h, hT=torch.zeros(2, 8, 32)[:, :, ::2]), None), (dict(A=-torch.ones(8, 300), h0=None, hT=None), "<= 256"),
                    (dict(u=u.transpose(1, 2).contiguous().transpose(1, 2)), r"stride\(-1\)"), (dict(), "GPU tensor")):
        with pytest.raises(RuntimeError, match=why or "GPU tensor"):
            call(**kw)
    with pytest.raises(RuntimeError, match="same strides"):
        native.selective_scan_carry_fwd(u, u, A, Bm, Bm, None, None, None, True, h, torch.as_strided(h, h.shape, (0, 16, 1)))
    with pytest.raises(RuntimeError, match="one dtype"):
        native.selective_scan_carry_fwd(u.half(), u.half(), A, Bm.half(), Bm.half(), None, None, None, True, h, h.half())


# ---- the restatements ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "B%dD%dW%d_b%ds%d" % c)
def test_conv_chunk_restatement_with_one_token_is_the_update(case):
    from dimsum_amd.ops import causal_conv1d_chunk_torch, causal_conv1d_update_torch
    c = conv_case(golden("mixer_step"), *case)
    act = "silu" if case[4] else None
    s_chunk, s_update = c["state_in"].clone(), c["state_in"].clone()
    out = causal_conv1d_chunk_torch(c["x"].unsqueeze(-1), s_chunk, c["weight"], c["bias"], act)
    want = causal_conv1d_update_torch(c["x"], s_update, c["weight"], c["bias"], act)
    assert out.shape == (*c["x"].shape, 1)
    assert torch.equal(s_chunk, s_update) and torch.equal(s_chunk, c["state_out"])
    close(out.squeeze(-1), want, "out vs the update restatement")
    close(out.squeeze(-1), c["out"], "out vs the fixture")
    with pytest.raises(NotImplementedError):
        causal_conv1d_chunk_torch(c["x"].unsqueeze(-1), s_chunk, c["weight"], c["bias"], "gelu")


@pytest.mark.parametrize("W", [2, 3, 4])
def test_conv_chunk_restatement_split_anywhere_is_one_pass(W):
    """(2, 5, 12) in float64: one pass from a zero state is torch's own causal conv; the two pieces of every split, the second entered with the
    state the first left, give the same outputs and the same final state -- the last W inputs, the very values"""
    from dimsum_amd.ops import causal_conv1d_chunk_torch
    g = torch.Generator().manual_seed(W)
    x, w, b = (torch.randn(*s, generator=g, dtype=torch.float64) for s in ((2, 5, L), (5, W), (5,)))
    s_full = torch.zeros(2, 5, W, dtype=torch.float64)
    full = causal_conv1d_chunk_torch(x, s_full, w, b, "silu")
    want = torch.nn.functional.silu(torch.nn.functional.conv1d(torch.nn.functional.pad(x, (W - 1, 0)), w.unsqueeze(1), b, groups=5))
    assert (full - want).abs().max() < 1e-12 and torch.equal(s_full, x[:, :, -W:])
    for s in range(1, L):
        st = torch.zeros(2, 5, W, dtype=torch.float64)
        a = causal_conv1d_chunk_torch(x[:, :, :s], st, w, b, "silu")
        mid = st.clone()
        bb = causal_conv1d_chunk_torch(x[:, :, s:], st, w, b, "silu")
        assert torch.equal(mid, torch.nn.functional.pad(x[:, :, :s], (W, 0))[:, :, -W:]), s      # a piece shorter than W keeps old (zero) values
        assert (torch.cat([a, bb], -1) - full).abs().max() < 1e-12 and torch.equal(st, s_full), s


@pytest.mark.parametrize("cplx,var", [(False, True), (False, False), (True, True), (True, False)])
def test_scan_carry_restatement_split_anywhere_is_one_pass(cplx, var):
    """(2, 6, 9), 5 states, 2 groups, float64 / complex128: from a zero state the restatement is scan_general_ref's one pass; the pieces of
    every split, the second entered with the state the first left, reproduce its outputs and its final state"""
    from dimsum_amd.ops import selective_scan_carry_torch
    from scan_general_ref import make_case, scan_restated
    n = 9
    c = {k: (v.detach() if v is not None else None) for k, v in make_case(2, 6, n, 5, cplx, var, var, groups=2 if var else 1, seed=3).items()}
    want, _, want_h, _ = scan_restated(c["u"], c["delta"], c["A"], c["B"], c["C"], c["D"], c["z"], c["delta_bias"], True)
    args = lambda lo, hi: [c["u"][..., lo:hi], c["delta"][..., lo:hi], c["A"]] + [  # noqa: E731
        (m[..., lo * (2 if cplx else 1):hi * (2 if cplx else 1)] if var else m) for m in (c["B"], c["C"])] + [c["D"], c["z"][..., lo:hi], c["delta_bias"], True]
    full, h = selective_scan_carry_torch(*args(0, n))
    assert full.dtype == torch.float64 and (full - want).abs().max() < 1e-12 and (h - want_h).abs().max() < 1e-12
    for s in range(1, n):
        a, h1 = selective_scan_carry_torch(*args(0, s))
        keep = h1.clone()
        b, h2 = selective_scan_carry_torch(*args(s, n), initial_state=h1)
        assert torch.equal(h1, keep)                                           # the state handed in is left as it is
        assert (torch.cat([a, b], -1) - want).abs().max() < 1e-12 and (h2 - want_h).abs().max() < 1e-12, s


# ---- the modules -----------------------------------------------------------------------------------------------------------------------------------
def _inputs(cls):
    g = golden("mixer_step")
    return g, T(g[f"{cls}_x"]), ((T(g[f"{cls}_c"]),) if cls == "CondMamba" else ())


def _check_against_fixture(g, cls, ys, states, what):
    close(ys, g[f"{cls}_y_full"], what + ": outputs vs one forward of the reference module")
    close(states[0], g[f"{cls}_conv_state"], what + ": conv_state")
    close(states[1], g[f"{cls}_ssm_state"], what + ": ssm_state")


@pytest.mark.parametrize("c", [1, 2, 3, 7])
@pytest.mark.parametrize("p", [1, 3, 5])
@pytest.mark.parametrize("cls", ["Mamba", "CondMamba"])
def test_prompt_then_extend_in_chunks_matches_the_reference_module(cls, p, c, chunk_backend):
    """a prompt of p tokens through forward(inference_params=...), then extend in chunks of c to the end (a ragged last chunk where c does
    not divide 12 - p): the reference module's one forward and the states it leaves"""
    from dimsum_amd.utils import InferenceParams
    g, x, args = _inputs(cls)
    m = mixer(cls)
    params = InferenceParams(max_seqlen=L, max_batch_size=2)
    with torch.no_grad():
        ys = [m(x[:, :p], *args, inference_params=params)]
        conv_state, ssm_state = params.key_value_memory_dict[3]
        for t in range(p, L, c):
            out, cs, ss = m.extend(x[:, t:t + c], conv_state, ssm_state)
            assert cs is conv_state and ss is ssm_state and out.shape == (2, min(c, L - t), 32)      # the very tensors, updated in place
            ys.append(out)
    _check_against_fixture(g, cls, torch.cat(ys, 1), (conv_state, ssm_state), f"p{p} c{c}")
    if p == c or (p, c) == (5, 7):
        # chunked_prefill: the same walk (first chunk = the prompt path) for chunk sizes that divide 12 or not
        m2, p2 = mixer(cls), InferenceParams(max_seqlen=L, max_batch_size=2)
        from dimsum_amd.utils import chunked_prefill
        got = chunked_prefill(m2, x, p2, c, *args)
        assert p2.seqlen_offset == L and got.shape == (2, L, 32)
        _check_against_fixture(g, cls, got, p2.key_value_memory_dict[3], f"chunked_prefill {c}")


@pytest.mark.parametrize("cls", ["Mamba", "CondMamba"])
def test_two_extends_from_zero_states_split_anywhere(cls, chunk_backend):
    """no prompt path at all: extend over [0, s) and [s, 12) from freshly allocated (zero) states, for every s, and one extend over all 12"""
    g, x, _ = _inputs(cls)
    m = mixer(cls)
    for s in range(1, L + 1):
        states = m.allocate_inference_cache(2, L)
        ys = [m.extend(x[:, :s], *states)[0]] + ([m.extend(x[:, s:], *states)[0]] if s < L else [])
        _check_against_fixture(g, cls, torch.cat(ys, 1), states, f"split {s}")


def test_extend_records_no_graph_and_keeps_the_refusals(chunk_backend):
    from test_model_cpu import build_mixer
    from dimsum_amd.utils import InferenceParams, chunked_prefill
    _, x, _ = _inputs("Mamba")
    m = mixer("Mamba").train()
    states = m.allocate_inference_cache(2, L)
    out = m.extend(x[:, :3].clone().requires_grad_(), *states)[0]
    assert not out.requires_grad and out.grad_fn is None and not states[1].requires_grad
    for bad, why in ((build_mixer("condmamba_v2"), "no causal recurrence"), (build_mixer("condmamba_zigma8"), "no token-by-token order")):
        with pytest.raises(NotImplementedError, match=why):
            bad.extend(torch.zeros(2, 3, 32), *bad.allocate_inference_cache(2, 64))
    with pytest.raises(AssertionError, match="seqlen_offset"):
        chunked_prefill(m, x, InferenceParams(max_seqlen=L, max_batch_size=2, seqlen_offset=2), 4)
    # what must stay: step and forward at an offset > 0 take one token (test_mixer_step_cpu.py pins it too)
    with pytest.raises(AssertionError, match="1 token"):
        m.step(x[:, :2], *states)
    with pytest.raises(AssertionError, match="1 token"):
        m(x[:, :2], inference_params=InferenceParams(max_seqlen=L, max_batch_size=2, seqlen_offset=3))


# ---- the operator ----------------------------------------------------------------------------------------------------------------------------------
def test_selective_scan_fn_takes_a_carried_state_for_inference_only(monkeypatch):
    from dimsum_amd import native
    from dimsum_amd.ops import selective_scan_carry_torch, selective_scan_fn
    g = torch.Generator().manual_seed(0)
    u, delta = torch.rand(2, 4, 6, generator=g), torch.rand(2, 4, 6, generator=g)
    A, Bm, Cm, h0 = -torch.rand(4, 16, generator=g), torch.randn(2, 16, 6, generator=g), torch.randn(2, 16, 6, generator=g), torch.randn(2, 4, 16, generator=g)
    for leaf in ("u", "A", "h0"):
        kw = dict(u=u, A=A, h0=h0)
        kw[leaf] = kw[leaf].clone().requires_grad_()
        with pytest.raises(NotImplementedError, match="inference argument"):
            selective_scan_fn(kw["u"], delta, kw["A"], Bm, Cm, initial_state=kw["h0"])
        with torch.no_grad(), pytest.raises(RuntimeError, match="GPU tensor"):       # grad mode off: not refused for the leaf, only for the device
            selective_scan_fn(kw["u"], delta, kw["A"], Bm, Cm, initial_state=kw["h0"])
    # the routing: with a carried state the call goes to native.selective_scan_carry_fwd whatever the dstate (16: a tuned one), 3-dim B / C
    # as one group; without one, not to it
    seen = []

    def carry(*a):
        seen.append(a)
        return native_scan_carry(*a)

    monkeypatch.setattr(native, "selective_scan_carry_fwd", carry)
    out, last = selective_scan_fn(u, delta, A, Bm, Cm, delta_softplus=True, return_last_state=True, initial_state=h0)
    want, want_h = selective_scan_carry_torch(u, delta, A, Bm, Cm, delta_softplus=True, initial_state=h0)
    assert len(seen) == 1 and seen[0][3].shape == (2, 1, 16, 6) and seen[0][9] is h0 and seen[0][10] is last
    assert torch.equal(out, want) and torch.equal(last, want_h) and out.grad_fn is None
    assert selective_scan_fn(u, delta, A, Bm, Cm, initial_state=h0).shape == u.shape and seen[1][10] is None
    with cpu_oracle_backend():
        selective_scan_fn(u, delta, A, Bm, Cm)
    assert len(seen) == 2
