"""Continuing a cached sequence by any number of tokens, on the GPU: dimsum_causal_conv1d_chunk (csrc/causal_conv1d.hip) and the carried
state of the general scan forward (csrc/ssm_scan_general.hip, dimsum_ssm_scan_carry_fwd) against ONE float64 pass over the whole sequence
from zero states (ops: causal_conv1d_chunk_torch, selective_scan_carry_torch; never a chunked reference); Mamba / CondMamba prompt + extend
against the reference module's recorded rows (mixer_step.npz) and one fused forward; an extend replayed from a captured graph.
Tolerances are the project's own, unchanged: CONV_TOL / SSU_TOL of test_mixer_step_gpu.py for the conv, the carried state and the mixers,
test_scan_general_gpu.py's per-dtype ones for scan outputs (tol(L) in fp32; rtol / atol 3e-3 / 5e-3 in fp16, 3e-2 / 5e-2 in bf16).
Conv states are compared exactly: the kernel moves them."""
import ctypes
import itertools

import pytest
import torch

from conftest import assert_close, golden
from scan_general_ref import make_case
from test_mixer_step_cpu import L as SEQ
from test_mixer_step_gpu import CONV_TOL, DEV, DTYPES, SSU_TOL, close, exact_fp32, gpu_mixer, rnd  # noqa: F401  (exact_fp32: a fixture)
from test_scan_gpu import tol

pytestmark = pytest.mark.gpu
T = torch.from_numpy
SCAN_TOL = {torch.float16: dict(rtol=3e-3, atol=5e-3), torch.bfloat16: dict(rtol=3e-2, atol=5e-2)}      # test_scan_general_gpu.py:131


# ---- conv chunk ------------------------------------------------------------------------------------------------------------------------------------
CONV_LENGTHS = (1, 2, 3, 4, 5, 255, 256, 257, 260)      # shorter than the width, one step, the 256-element step boundary, a vector tail


def conv_takes_vector_path(x, out_like):
    """the launcher's own predicate (csrc/causal_conv1d.hip, launch_conv_chunk): seqlen, both outer strides and the base of x and of out
    multiples of 4 elements"""
    ok = lambda t: t.shape[2] % 4 == 0 and t.stride(0) % 4 == 0 and t.stride(1) % 4 == 0 and t.data_ptr() % (4 * t.element_size()) == 0  # noqa: E731
    return ok(x) and ok(out_like)


def conv_check(x, state, w, b, silu, dtype, what):
    """one launch on `state` (in place) against the float64 restatement -> out"""
    from dimsum_amd.ops import causal_conv1d_chunk, causal_conv1d_chunk_torch
    W = w.shape[1]
    s64 = state.double().clone()
    want = causal_conv1d_chunk_torch(x.double(), s64, w.double(), b.double() if b is not None else None, "silu" if silu else None)
    want_state = torch.cat([state, x], dim=-1)[..., -W:].clone()
    out = causal_conv1d_chunk(x, state, w, b, "silu" if silu else None)
    assert out.dtype == dtype and out.shape == x.shape, what
    assert torch.equal(state, want_state) and torch.equal(state.double(), s64), what + ": state"
    close(out, want, CONV_TOL[dtype], what + ": out")
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("B,D", [(2, 5), (3, 65)])
@pytest.mark.parametrize("W", [2, 3, 4])
def test_conv_chunk_against_float64(W, B, D, dtype):
    """every length with and without bias and SiLU, from a random state. Contiguous x: lengths 4, 256 and 260 take the 16-byte path, the
    others the element path. One token leaves exactly the state dimsum_causal_conv1d_update leaves."""
    from dimsum_amd.ops import causal_conv1d_update
    w, bias = rnd(D, W, seed=3), rnd(D, seed=4)
    paths = set()
    for n, (has_bias, silu) in itertools.product(CONV_LENGTHS, itertools.product((False, True), repeat=2)):
        x, state = rnd(B, D, n, dtype=dtype, seed=10 + n), rnd(B, D, W, dtype=dtype, seed=2)
        paths.add(conv_takes_vector_path(x, x))
        state0 = state.clone()
        conv_check(x, state, w, bias if has_bias else None, silu, dtype, f"L{n} bias={has_bias} silu={silu}")
        if n == 1:
            s_update = state0.clone()
            causal_conv1d_update(x[:, :, 0], s_update, w, bias if has_bias else None, "silu" if silu else None)
            assert torch.equal(state, s_update)
    assert paths == {False, True}


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("W", [2, 3, 4])
def test_conv_chunk_layouts_and_split_anywhere(W, dtype):
    """(3, 65, 260) once as a contiguous x, once as the mixer's view -- the first half of a (B, 2D, L) xz, batch stride 2 D L --, both on the
    16-byte path, and once as a view one element off alignment, which must take the element path: one float64 pass each, xz untouched.
    Then the same sequence in two pieces split at 1, 3, 255, 256 and 257, the second entered with the state the first left: the float64
    pass's outputs and its final state, the very values."""
    B, D, n = 3, 65, 260
    w, bias = rnd(D, W, seed=5), rnd(D, seed=6)
    xz = rnd(B, 2 * D, n, dtype=dtype, seed=7)
    xz0 = xz.clone()
    state0 = rnd(B, D, W, dtype=dtype, seed=8)
    buf = torch.empty(B * D * n + 8, dtype=dtype, device=DEV)
    lead = 1 if buf.data_ptr() % (4 * buf.element_size()) == 0 else 0
    shifted = buf[lead:lead + B * D * n].view(B, D, n)
    shifted.copy_(xz[:, :D])
    from dimsum_amd.ops import causal_conv1d_chunk, causal_conv1d_chunk_torch
    for x, vec in ((xz[:, :D].contiguous(), True), (xz[:, :D], True), (shifted, False)):
        assert conv_takes_vector_path(x, torch.empty_like(x)) == vec
        conv_check(x, state0.clone(), w, bias, True, dtype, f"stride {x.stride()}")
    assert torch.equal(xz, xz0)
    final = torch.cat([state0, xz[:, :D]], dim=-1)[..., -W:]
    want = causal_conv1d_chunk_torch(xz[:, :D].double(), state0.double(), w.double(), bias.double(), "silu")
    for s in (1, 3, 255, 256, 257):
        state = state0.clone()
        a = causal_conv1d_chunk(xz[:, :D, :s], state, w, bias, "silu")
        b = causal_conv1d_chunk(xz[:, :D, s:], state, w, bias, "silu")
        close(torch.cat([a, b], -1), want, CONV_TOL[dtype], f"split {s}")
        assert torch.equal(state, final), s


def test_conv_chunk_on_a_strided_state():
    """conv_state as the first batch rows of a larger cache and as a transposed window of a (batch, width, dim) buffer: nothing outside moves"""
    from dimsum_amd.ops import causal_conv1d_chunk
    B, D, W = 3, 65, 4
    w, bias = rnd(D, W, seed=6), rnd(D, seed=7)
    cache, window = rnd(B + 2, D, W, seed=8), rnd(B, W + 2, D + 3, seed=9)
    for n in (2, 5):
        x = rnd(B, D, n, seed=n)
        for make in (lambda: cache[:B], lambda: window[:, 1:W + 1, 2:D + 2].transpose(1, 2)):
            cache0, window0 = cache.clone(), window.clone()
            state = make()
            old = state.clone()
            conv_check(x, state, w, bias, True, torch.float32, f"L{n} state stride {state.stride()}")
            state.copy_(old)
            assert torch.equal(cache, cache0) and torch.equal(window, window0)
    x, st = rnd(2, 8, 3), rnd(2, 8, 5)
    with pytest.raises(RuntimeError, match="width between 2 and 4"):
        causal_conv1d_chunk(x, st, rnd(8, 5), None, "silu")


# ---- scan carry ------------------------------------------------------------------------------------------------------------------------------------
_REF = {}


def scan_case(N, dim, n, cplx, dtype, opts, var=True, seed=0):
    """-> (operands on the GPU in the kernels' dtypes, float64 reference: ONE pass over the n steps from a zero state -> (out, last state))"""
    from dimsum_amd.ops import selective_scan_carry_torch
    key = (N, dim, n, cplx, dtype, opts, var, seed)
    if key not in _REF:
        c = make_case(2, dim, n, N, cplx, var, var, has_D=opts, has_z=opts, has_bias=opts, seed=seed + N + n, dtype=dtype)
        c = {k: (v.detach() if v is not None else None) for k, v in c.items()}
        with torch.no_grad():
            want = selective_scan_carry_torch(c["u"], c["delta"], c["A"], c["B"], c["C"], c["D"], c["z"], c["delta_bias"], True)
        g = {}
        for k, v in c.items():
            weight = k in ("A", "D", "delta_bias") or (k in ("B", "C") and v is not None and v.dim() == 2)
            g[k] = None if v is None else v.to(torch.complex64 if v.is_complex() else (torch.float32 if weight else dtype)).to(DEV)
        g["float64"] = c
        _REF[key] = (g, want)
    return _REF[key]


def piece(g, lo, hi, cplx):
    k = 2 if cplx else 1
    cut = lambda m: m if m.dim() == 2 else m[..., lo * k:hi * k]      # noqa: E731
    return (g["u"][..., lo:hi], g["delta"][..., lo:hi], g["A"], cut(g["B"]), cut(g["C"]), g["D"], None if g["z"] is None else g["z"][..., lo:hi],
            g["delta_bias"], True)


def np64(t):
    t = t.detach().cpu()
    return torch.view_as_real(t.to(torch.complex128)).numpy() if t.is_complex() else t.double().numpy()


def state_rounding_bound(g, s, state_dtype):
    """What a 16-bit carried state costs the outputs after a split at s, from the number format alone: the store rounds each h_n once, by at
    most u |h_n| (u = 2^-11 in fp16, 2^-8 in bf16); A < 0, so the error only decays, and step t adds sum_n |C_t,n| of it to y_t:
    |dy| <= u max|C| max_(b,d) sum_n |h_n| at the split (times max |silu(z)| <= max(|z|, 1) behind the gate). h at the split comes from
    the float64 restatement over [0, s)."""
    from dimsum_amd.ops import selective_scan_carry_torch
    if s == 0 or state_dtype in (torch.float32, torch.complex64):
        return 0.0
    c = g["float64"]
    key = ("h", s)
    if key not in g:
        with torch.no_grad():
            g[key] = selective_scan_carry_torch(c["u"][..., :s], c["delta"][..., :s], c["A"], c["B"][..., :s], c["C"][..., :s], None, None,
                                                c["delta_bias"], True)[1]
    u = 2.0 ** (-11 if state_dtype == torch.float16 else -8)
    gate = 1.0 if c["z"] is None else max(1.0, c["z"].abs().max().item())
    return u * c["C"].abs().max().item() * g[key].abs().sum(-1).max().item() * gate


def check_split(g, want, n, s, cplx, dtype, state_dtype, what):
    """[0, s) from an explicit zero state, then [s, n) from the state that left, both through native.selective_scan_carry_fwd with the state
    updated in place, against the one float64 pass. A state of a 16-bit I/O dtype is rounded at the split, which the float64 pass is not:
    those cases alone get state_rounding_bound on top of the per-dtype atol. Measured without it on the fp32 plain-torch restatement with the
    same single rounding of the state (so a property of the format, not of the kernel): fp16 I/O and state, 17 states, 5 channels, 9 steps
    split at 4: |err| 6.6e-3 against the unwidened 6.0e-3 at an output of 0.32. Every other case runs on the unwidened tolerances."""
    from dimsum_amd import native
    want_out, want_h = want
    h = torch.zeros(want_h.shape, dtype=state_dtype, device=DEV)
    outs = [native.selective_scan_carry_fwd(*piece(g, lo, hi, cplx), h, h) for lo, hi in ((0, s), (s, n)) if hi > lo]
    out = torch.cat(outs, -1)
    assert out.dtype == dtype and h.dtype == state_dtype
    bound = dict(tol(n)) if dtype == torch.float32 else dict(SCAN_TOL[dtype])
    bound["atol"] += state_rounding_bound(g, s, state_dtype)
    assert_close(np64(out), np64(want_out), what=what + " out", **bound)
    rtol, atol = SSU_TOL[dtype]
    assert_close(np64(h), np64(want_h), rtol, atol, what + " state")


@pytest.mark.parametrize("dim", [5, 65])
@pytest.mark.parametrize("N", [1, 16, 17, 64])
def test_scan_carry_real_split_anywhere(N, dim):
    """dstate 1 and 16: one wave; 17: two, the second with one live state; 64: four. Lengths below, at and past the 4-step tile, every split
    (s = 0: the whole sequence entered with an explicit zero state), fp32 and 16-bit I/O, the state float32 or of the I/O dtype, with and
    without z / D / delta_bias."""
    for n, opts in itertools.product((1, 3, 4, 5, 9), (True, False)):
        for dtype, state_dtype in ((torch.float32, torch.float32), (torch.float16, torch.float32), (torch.float16, torch.float16),
                                   (torch.bfloat16, torch.float32), (torch.bfloat16, torch.bfloat16)):
            g, want = scan_case(N, dim, n, False, dtype, opts)
            for s in range(n):
                check_split(g, want, n, s, False, dtype, state_dtype, f"N{N} D{dim} L{n} s{s} {dtype} state {state_dtype} opts={opts}")


@pytest.mark.parametrize("dim", [5, 65])
@pytest.mark.parametrize("N", [1, 16, 17, 64])
def test_scan_carry_complex_split_anywhere(N, dim):
    """complex A (a 2-step tile): lengths 1, 2, 3, 5, every split, fp32 and fp16 I/O on a complex64 state"""
    for n, opts, dtype in itertools.product((1, 2, 3, 5), (True, False), (torch.float32, torch.float16)):
        g, want = scan_case(N, dim, n, True, dtype, opts)
        for s in range(n):
            check_split(g, want, n, s, True, dtype, torch.complex64, f"complex N{N} D{dim} L{n} s{s} {dtype} opts={opts}")


@pytest.mark.parametrize("cplx", [False, True])
def test_scan_carry_constant_B_and_C(cplx):
    n, N, dim = 5, 17, 65
    g, want = scan_case(N, dim, n, cplx, torch.float32, True, var=False)
    for s in range(n):
        check_split(g, want, n, s, cplx, torch.float32, torch.complex64 if cplx else torch.float32, f"constant B / C s{s}")


@pytest.mark.parametrize("state_dtype", [torch.float32, torch.bfloat16], ids=str)
def test_scan_carry_updates_a_strided_slice_in_place(state_dtype):
    """the state as a slice [1:3, 2:67, 3:20] of a (4, 70, 24) buffer filled with a sentinel: after the two pieces the slice holds the final state
    and every element around it the sentinel; h0 and hT as two different tensors give the same bits and leave h0 as it was"""
    from dimsum_amd import native
    n, N, dim, s = 9, 17, 65, 4
    dtype = torch.float32 if state_dtype == torch.float32 else state_dtype
    g, want = scan_case(N, dim, n, False, dtype, True)
    big = torch.full((4, 70, 24), 7.0, dtype=state_dtype, device=DEV)
    h = big[1:3, 2:67, 3:20]
    h.zero_()
    outs = [native.selective_scan_carry_fwd(*piece(g, lo, hi, False), h, h) for lo, hi in ((0, s), (s, n))]
    rtol, atol = SSU_TOL[dtype]
    assert_close(np64(h), np64(want[1]), rtol, atol, "state in the slice")
    assert_close(np64(torch.cat(outs, -1)), np64(want[0]), what="out", **(tol(n) if dtype == torch.float32 else SCAN_TOL[dtype]))
    mask = torch.ones_like(big, dtype=torch.bool)
    mask[1:3, 2:67, 3:20] = False
    assert bool((big[mask] == 7.0).all())
    # out of place
    h0 = torch.zeros(2, dim, N, dtype=state_dtype, device=DEV)
    h1, h2 = torch.empty_like(h0), torch.empty_like(h0)
    a = native.selective_scan_carry_fwd(*piece(g, 0, s, False), h0, h1)
    keep = h1.clone()
    b = native.selective_scan_carry_fwd(*piece(g, s, n, False), h1, h2)
    assert not h0.any() and torch.equal(h1, keep) and torch.equal(h2, h) and torch.equal(torch.cat([a, b], -1), torch.cat(outs, -1))
    # h0 = None is a zero state; hT = None stores none
    c = native.selective_scan_carry_fwd(*piece(g, 0, s, False), None, None)
    assert torch.equal(c, a)


def _general_params(g, softplus, out, x, out_z):
    """(dimsum_ssm_general_params_t, dimsum_ssm_carry_params_t with NULL states) filled from the same operands by native's own fill"""
    from dimsum_amd import _lib, native
    flags = native._check_ssm_general(g["u"], g["delta"], g["A"], g["B"], g["C"], g["D"], g["z"], g["delta_bias"])
    P, Q = _lib.SsmGeneralParams(), _lib.SsmCarryParams()
    for target, (o, xx, oz) in ((P, (out[0], x[0], out_z[0])), (Q.scan, (out[1], x[1], out_z[1]))):
        native._fill_ssm_general(target, g["u"], g["delta"], g["A"], g["B"], g["C"], g["D"], g["z"], g["delta_bias"], softplus, o, xx, oz, flags)
    return P, Q


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
@pytest.mark.parametrize("cplx,N,var", [(False, 16, True), (False, 17, True), (False, 64, False), (True, 17, True), (True, 64, True)])
def test_null_states_are_the_general_forward_bit_for_bit(cplx, N, var, dtype):
    """dimsum_ssm_scan_carry_fwd with h0 == hT == NULL against dimsum_ssm_scan_general_fwd on the same operands: out, out_z and x (running
    products and chunk-end states) bit-equal"""
    from dimsum_amd import _lib
    n, dim = 37, 72
    g, _ = scan_case(N, dim, n, cplx, dtype, True, var=var, seed=1)
    out = [torch.full_like(g["u"], 3.0) for _ in range(2)]
    out_z = [torch.full_like(g["u"], 3.0) for _ in range(2)]
    x = [torch.full((2, dim, 1, 2 * N), 3.0, dtype=g["A"].dtype, device=DEV) for _ in range(2)]
    P, Q = _general_params(g, True, out, x, out_z)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib = _lib.load()
    assert lib.dimsum_ssm_scan_general_fwd(P, stream) == 0 and lib.dimsum_ssm_scan_carry_fwd(Q, stream) == 0
    torch.cuda.synchronize()
    for a, b, what in ((*out, "out"), (*out_z, "out_z")):
        assert torch.equal(a, b) and not bool((a == 3.0).all()), what
    assert torch.equal(torch.view_as_real(x[0]) if cplx else x[0], torch.view_as_real(x[1]) if cplx else x[1])


def test_x_under_a_carried_state():
    """x keeps its meaning: the running product counts from THIS call's first step, the state entries include what was carried in"""
    from dimsum_amd import _lib
    n, N, dim, s = 9, 17, 65, 4
    g, want = scan_case(N, dim, n, False, torch.float32, True)
    second = dict({k: v for k, v in g.items() if isinstance(k, str) and k != "float64"}, **dict(zip(("u", "delta", "A", "B", "C", "D", "z", "delta_bias"), piece(g, s, n, False)[:8])))
    from dimsum_amd import native
    h = torch.zeros(2, dim, N, device=DEV)
    native.selective_scan_carry_fwd(*piece(g, 0, s, False), h, h)
    out, out_z, x = torch.empty_like(second["u"]), torch.empty_like(second["u"]), torch.empty(2, dim, 1, 2 * N, device=DEV)
    _, Q = _general_params(second, True, [None, out], [None, x], [None, out_z])
    Q.h0_ptr = Q.hT_ptr = h.data_ptr()
    Q.h0_batch_stride, Q.h0_d_stride, Q.h0_dstate_stride = Q.hT_batch_stride, Q.hT_d_stride, Q.hT_dstate_stride = h.stride()
    assert _lib.load().dimsum_ssm_scan_carry_fwd(Q, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    assert torch.equal(x[:, :, 0, 1::2], h)
    rtol, atol = SSU_TOL[torch.float32]
    assert_close(np64(h), np64(want[1]), rtol, atol, "state")
    dt = torch.nn.functional.softplus(second["delta"].double() + second["delta_bias"].double()[None, :, None])
    prod = torch.exp(dt.sum(-1)[..., None] * second["A"].double())
    assert_close(np64(x[:, :, 0, 0::2]), np64(prod), 2e-3, 1e-30, "x.prod_a")      # test_scan_gpu.py's bound for the same quantity


def test_selective_scan_fn_with_an_initial_state():
    """the public operator: dstate 16 (a tuned size: the carried call takes the general kernel all the same), 3-dim B / C, last state back"""
    from dimsum_amd.ops import selective_scan_fn
    n, N, dim, s = 9, 16, 65, 5
    g, want = scan_case(N, dim, n, False, torch.float32, True)
    a = piece(g, 0, s, False)
    b = piece(g, s, n, False)
    fn = lambda p, h: selective_scan_fn(p[0], p[1], p[2], p[3].squeeze(1), p[4].squeeze(1), p[5], p[6], p[7], delta_softplus=True,  # noqa: E731
                                        return_last_state=True, initial_state=h)
    out_a, h1 = fn(a, torch.zeros(2, dim, N, device=DEV))
    out_b, h2 = fn(b, h1)
    assert_close(np64(torch.cat([out_a, out_b], -1)), np64(want[0]), what="out", **tol(n))
    assert_close(np64(h2), np64(want[1]), *SSU_TOL[torch.float32], "last state")
    with pytest.raises(NotImplementedError, match="inference argument"):
        selective_scan_fn(a[0].clone().requires_grad_(), a[1], a[2], a[3], a[4], initial_state=h1)


# ---- the modules -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 2, 3, 7])
@pytest.mark.parametrize("p", [1, 3, 5])
@pytest.mark.parametrize("cls", ["Mamba", "CondMamba"])
def test_prompt_then_extend_in_chunks_equals_one_forward(cls, p, c, exact_fp32):
    from dimsum_amd.utils import InferenceParams, chunked_prefill
    g = golden("mixer_step")
    tolerance = SSU_TOL[torch.float32]
    m = gpu_mixer(cls)
    x = T(g[f"{cls}_x"]).to(DEV)
    args = (T(g[f"{cls}_c"]).to(DEV),) if cls == "CondMamba" else ()
    params = InferenceParams(max_seqlen=SEQ, max_batch_size=2)
    with torch.no_grad():
        full = m(x, *args)
        ys = [m(x[:, :p], *args, inference_params=params)]
        conv_state, ssm_state = params.key_value_memory_dict[3]
        for t in range(p, SEQ, c):
            out, cs, ss = m.extend(x[:, t:t + c], conv_state, ssm_state)
            assert cs is conv_state and ss is ssm_state
            ys.append(out)
    ys = torch.cat(ys, 1)
    close(ys, full, tolerance, "prompt + extends vs one fused forward")
    close(ys, T(g[f"{cls}_y_full"]), tolerance, "prompt + extends vs the fixture")
    close(conv_state, T(g[f"{cls}_conv_state"]), tolerance, "conv_state")
    close(ssm_state, T(g[f"{cls}_ssm_state"]), tolerance, "ssm_state")
    if p == c or (p, c) == (5, 7):
        p2 = InferenceParams(max_seqlen=SEQ, max_batch_size=2)
        got = chunked_prefill(m, x, p2, c, *args)
        assert p2.seqlen_offset == SEQ
        close(got, T(g[f"{cls}_y_full"]), tolerance, "chunked_prefill vs the fixture")
        close(p2.key_value_memory_dict[3][0], T(g[f"{cls}_conv_state"]), tolerance, "chunked_prefill conv_state")
        close(p2.key_value_memory_dict[3][1], T(g[f"{cls}_ssm_state"]), tolerance, "chunked_prefill ssm_state")


def test_an_extend_replayed_from_a_captured_graph(exact_fp32):
    """one extend of 5 tokens captured on static buffers (a single stream: no parallel branches), replayed twice == two eager calls, bit for bit"""
    m = gpu_mixer("Mamba")
    x = T(golden("mixer_step")["Mamba_x"]).to(DEV)
    with torch.no_grad():
        eager_states = m.allocate_inference_cache(2, SEQ)
        eager = [m.extend(x[:, t:t + 5], *eager_states)[0].clone() for t in (0, 5)]
        conv_state, ssm_state = m.allocate_inference_cache(2, SEQ)
        tokens = x[:, :5].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m.extend(tokens, conv_state, ssm_state)                 # warm-up outside the capture (library handles, workspaces)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = m.extend(tokens, conv_state, ssm_state)[0]
        conv_state.zero_()
        ssm_state.zero_()
        replayed = []
        for t in (0, 5):
            tokens.copy_(x[:, t:t + 5])
            graph.replay()
            replayed.append(out.clone())
    torch.cuda.synchronize()
    for i in range(2):
        assert torch.equal(replayed[i], eager[i]), i
    assert torch.equal(conv_state, eager_states[0]) and torch.equal(ssm_state, eager_states[1])
