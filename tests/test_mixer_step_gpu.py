"""The recurrent form of the mixer on the GPU: the two kernels of csrc/mixer_step.hip against the float64 restatements
(ops: causal_conv1d_update_torch, selective_state_update_torch) and the reference fixture mixer_step.npz, on every path the launcher takes
(aligned rows / element strides / scalar tails, each dtype pairing, every optional operand, strided views of larger buffers); the modules'
prefill + step recurrence against one fused forward and the fixture; a step replayed from a captured graph; the refusals of the library.
Tolerances are the reference tests' own, per dtype (causal-conv1d/tests/test_causal_conv1d.py:93-95,
mamba/tests/ops/triton/test_selective_state_update.py:18-20); the conv state is compared exactly."""
import ctypes
import itertools

import pytest
import torch
import torch.nn.functional as F

from conftest import golden
from procedural import procedural_fill
from test_mixer_step_cpu import CONV_CASES, L, MIXER, SSU_CASES, conv_case, run_recurrent, ssu_case

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = "cuda"
CONV_TOL = {torch.float32: (3e-4, 1e-3), torch.float16: (3e-3, 5e-3), torch.bfloat16: (1e-2, 5e-2)}
SSU_TOL = {torch.float32: (3e-4, 1e-3), torch.float16: (5e-3, 1e-2), torch.bfloat16: (1e-2, 5e-2)}
DTYPES = [torch.float32, torch.float16, torch.bfloat16]


def close(a, b, tol, what):
    rtol, atol = tol
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, what
    err = (a - b).abs()
    assert bool((err <= atol + rtol * b.abs()).all()), f"{what}: max |err| {err.max().item():.3e} (rtol {rtol}, atol {atol})"


def rnd(*shape, dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype).to(DEV)


def urnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g).to(DEV)


# ---- conv update -----------------------------------------------------------------------------------------------------------------------------------
def conv_reference(x, state, w, b, silu):
    """-> (out in float64, the shifted state in the input dtype: a move of the input values)"""
    from dimsum_amd.ops import causal_conv1d_update_torch
    s64 = state.double().clone()
    out = causal_conv1d_update_torch(x.double(), s64, w.double(), b.double() if b is not None else None, "silu" if silu else None)
    return out, torch.cat([state[:, :, 1:], x[:, :, None]], dim=2)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", [(2, 5, 2), (2, 5, 3), (3, 65, 4), (1, 1, 2), (2, 129, 4)], ids=lambda s: "B%dD%dW%d" % s)
def test_conv_update_against_float64(shape, dtype):
    from dimsum_amd.ops import causal_conv1d_update
    B, D, W = shape
    for has_bias, silu in itertools.product((False, True), repeat=2):
        x, state = rnd(B, D, dtype=dtype, seed=1), rnd(B, D, W, dtype=dtype, seed=2)
        w, b = rnd(D, W, seed=3), rnd(D, seed=4) if has_bias else None
        want_out, want_state = conv_reference(x, state, w, b, silu)
        out = causal_conv1d_update(x, state, w, b, "silu" if silu else None)
        assert out.dtype == dtype and out.shape == (B, D)
        assert torch.equal(state, want_state), (has_bias, silu)
        close(out, want_out, CONV_TOL[dtype], f"out bias={has_bias} silu={silu}")


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "B%dD%dW%d_b%ds%d" % c)
def test_conv_update_against_the_fixture(case):
    from dimsum_amd.ops import causal_conv1d_update
    c = {k: v.to(DEV) if v is not None else None for k, v in conv_case(golden("mixer_step"), *case).items()}
    state = c["state_in"].clone()
    out = causal_conv1d_update(c["x"], state, c["weight"], c["bias"], "silu" if case[4] else None)
    assert torch.equal(state, c["state_out"])
    close(out, c["out"], CONV_TOL[torch.float32], "out")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("W", [2, 3, 4])
def test_conv_update_on_strided_views(W, dtype):
    """x as the first half of the (B, 2D) in_proj output, conv_state as the first rows of a larger cache and as a transposed window of a
    (batch, width, dim) buffer: results as on contiguous copies, nothing outside the views written"""
    from dimsum_amd.ops import causal_conv1d_update
    B, D = 3, 65
    xz = rnd(B, 2 * D, dtype=dtype, seed=5)
    w, b = rnd(D, W, seed=6), rnd(D, seed=7)
    x = xz[:, :D]
    cache = rnd(B + 2, D, W, dtype=dtype, seed=8)
    window = rnd(B, W + 2, D + 3, dtype=dtype, seed=9)
    for make in (lambda: cache[:B], lambda: window[:, 1:W + 1, 2:D + 2].transpose(1, 2)):
        xz0, cache0, window0 = xz.clone(), cache.clone(), window.clone()
        state = make()
        assert state.shape == (B, D, W)
        want_out, want_state = conv_reference(x, state.clone(), w, b, True)
        out = causal_conv1d_update(x, state, w, b, "silu")
        assert torch.equal(state, want_state)
        close(out, want_out, CONV_TOL[dtype], "out")
        assert torch.equal(xz, xz0)
        # outside the views nothing moved: undo the views' own update and compare whole buffers
        state.copy_(cache0[:B] if state.data_ptr() == cache.data_ptr() else window0[:, 1:W + 1, 2:D + 2].transpose(1, 2))
        assert torch.equal(cache, cache0) and torch.equal(window, window0)


# ---- state update ----------------------------------------------------------------------------------------------------------------------------------
def ssu_inputs(B, D, N, dtype, state_dtype=None, bc_dtype=None, seed=0):
    """the reference test's distributions (test_selective_state_update.py:24-36)"""
    return dict(state=rnd(B, D, N, dtype=state_dtype or dtype, seed=seed), x=rnd(B, D, dtype=dtype, seed=seed + 1),
                dt=rnd(B, D, dtype=dtype, seed=seed + 2), dt_bias=urnd(D, seed=seed + 3) - 4.0, A=-urnd(D, N, seed=seed + 4) - 1.0,
                B=rnd(B, N, dtype=bc_dtype or dtype, seed=seed + 5), C=rnd(B, N, dtype=bc_dtype or dtype, seed=seed + 6), D=rnd(D, seed=seed + 7),
                z=rnd(B, D, dtype=dtype, seed=seed + 8))


OPTIONS = [dict(), dict(D=1, z=1, dt_bias=1, softplus=1), dict(D=1, softplus=1), dict(z=1, dt_bias=1)]


def ssu_check(i, opt, tol, what, dt_proj=None, dt64=None):
    """one launch on a clone of i["state"] against the float64 restatement -> (out, the new state)"""
    from dimsum_amd import native
    from dimsum_amd.ops import selective_state_update, selective_state_update_torch
    if not opt.get("softplus") and dt64 is None:
        # without softplus the caller hands over the step size itself, a positive number (the reference test's dt and dt_bias, randn and
        # rand - 4, are inputs of softplus): a negative one makes the state grow by exp(|dt A|) in one step and leave float16's range
        i = dict(i, dt=i["dt"].abs(), dt_bias=(i["dt_bias"] + 4.0) * 0.1)
    D, z, bias = (i[k] if opt.get(k) else None for k in ("D", "z", "dt_bias"))
    s64 = i["state"].double().clone()
    d = lambda t: t.double() if t is not None else None      # noqa: E731
    want = selective_state_update_torch(s64, i["x"].double(), i["dt"].double() if dt64 is None else dt64, i["A"].double(), i["B"].double(),
                                        i["C"].double(), d(D), d(z), d(bias), bool(opt.get("softplus")))
    state = i["state"].clone()
    if dt_proj is None:
        out = selective_state_update(state, i["x"], i["dt"], i["A"], i["B"], i["C"], D=D, z=z, dt_bias=bias, dt_softplus=bool(opt.get("softplus")))
    else:
        out = native.selective_state_update(state, i["x"], None, i["A"], i["B"], i["C"], D, z, bias, bool(opt.get("softplus")), dt_proj=dt_proj)
    assert out.dtype == i["x"].dtype and out.shape == i["x"].shape and state.dtype == i["state"].dtype
    close(state, s64, tol, what + " state")
    close(out, want, tol, what + " out")
    return out, state


@pytest.mark.parametrize("N", [1, 16, 17, 64, 256])
def test_state_update_against_float64(N):
    for D, B, opt in itertools.product((1, 5, 65), (1, 3), OPTIONS):
        ssu_check(ssu_inputs(B, D, N, torch.float32, seed=N), opt, SSU_TOL[torch.float32], f"B{B} D{D} N{N} {sorted(opt)}")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=str)
@pytest.mark.parametrize("f32_state", [False, True])
@pytest.mark.parametrize("f32_bc", [False, True])
def test_state_update_dtype_pairings(dtype, f32_state, f32_bc):
    """16-bit x next to a float32 state and / or float32 B and C (the reference's own test feeds float32 B / C, :29-30)"""
    for (B, D, N), opt in itertools.product(((3, 65, 16), (3, 65, 17), (1, 5, 64), (1, 1, 1)), OPTIONS):
        i = ssu_inputs(B, D, N, dtype, torch.float32 if f32_state else dtype, torch.float32 if f32_bc else dtype, seed=3)
        ssu_check(i, opt, SSU_TOL[dtype], f"B{B} D{D} N{N} {sorted(opt)}")


@pytest.mark.parametrize("case", SSU_CASES, ids=lambda c: "B%dD%dN%d_z%dd%d" % c)
def test_state_update_against_the_fixture(case):
    from dimsum_amd.ops import selective_state_update
    c = {k: v.to(DEV) if v is not None else None for k, v in ssu_case(golden("mixer_step"), *case).items()}
    state = c["state_in"].clone()
    out = selective_state_update(state, c["x"], c["dt"], c["A"], c["B"], c["C"], D=c["D"], z=c["z"], dt_bias=c["dt_bias"], dt_softplus=True)
    close(state, c["state_out"], SSU_TOL[torch.float32], "state")
    close(out, c["out"], SSU_TOL[torch.float32], "out")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_state_update_around_the_softplus_threshold(dtype):
    """dt + dt_bias on both sides of torch's threshold of 20: softplus below and at it, the identity above"""
    B, D, N = 3, 65, 16
    i = ssu_inputs(B, D, N, dtype, torch.float32, torch.float32, seed=11)
    i["dt_bias"] = torch.full((D,), 4.0, device=DEV)
    i["dt"] = torch.tensor([15.5, 16.0, 16.5, -3.0], device=DEV).repeat(B * D // 4 + 1)[:B * D].view(B, D).to(dtype)     # sums 19.5, 20, 20.5, 1
    assert sorted(set((i["dt"].float() + 4.0).flatten().tolist())) == [1.0, 19.5, 20.0, 20.5]
    ssu_check(i, dict(D=1, z=1, dt_bias=1, softplus=1), SSU_TOL[dtype], "threshold")


def takes_vector_path(state, A, Bm, Cm):
    """the launcher's own predicate (csrc/mixer_step.hip, launch_state_update): dstate >= 4 and, for each of state, A, B, C, unit stride
    along the row, every outer stride a multiple of 4 elements and a base aligned to 4 elements"""
    ok = lambda t: t.stride(-1) == 1 and all(st % 4 == 0 for st in t.stride()[:-1]) and t.data_ptr() % (4 * t.element_size()) == 0  # noqa: E731
    return state.shape[-1] >= 4 and all(ok(t) for t in (state, A, Bm, Cm))


def off_by_one(t):
    """a contiguous copy of t whose base is one element past an aligned address: the launcher must take the element path for it"""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    lead = 1 if buf.data_ptr() % (4 * t.element_size()) == 0 else 0
    out = buf[lead:lead + t.numel()].view(t.shape)
    out.copy_(t)
    return out


@pytest.mark.parametrize("state_dtype", [torch.float32, torch.float16, torch.bfloat16], ids=str)
@pytest.mark.parametrize("N,row", [(16, 16), (16, 20), (17, 20), (5, 8), (7, 8)])
def test_state_update_on_a_strided_cache_slice(N, row, state_dtype):
    """The operands as the views a step really has: state = the first batch rows and the first N of `row` columns of a larger cache, A the
    first N columns of a padded table, x and z the halves of a (B, 2D) tensor, B and C column ranges of an x_proj output whose ranges start
    4-element aligned. These rows are aligned, so the launch walks them in 4-element pieces, with a scalar tail where N % 4 != 0 (17: four
    pieces + one element, 5 and 7: one piece + a tail). The same values as misaligned contiguous copies take the element path. Both are
    held to the float64 restatement, must agree bit for bit (same expressions, same order), and nothing outside the views is written."""
    from dimsum_amd.ops import selective_state_update
    B, D, R = 3, 65, 4
    dtype = torch.float32 if state_dtype == torch.float32 else state_dtype
    tol = SSU_TOL[dtype]
    cache = rnd(B + 2, D, row, dtype=state_dtype, seed=21)
    cache0 = cache.clone()
    xz, x_db = rnd(B, 2 * D + 6, dtype=dtype, seed=22), rnd(B, R + 2 * row, dtype=dtype, seed=23)
    A_buf = -urnd(D, row, seed=25) - 1.0
    i = ssu_inputs(B, D, N, dtype, seed=24)
    i.update(state=cache[:B, :, :N], A=A_buf[:, :N], x=xz[:, :D], z=xz[:, D:2 * D], B=x_db[:, R:R + N], C=x_db[:, R + row:R + row + N])
    assert takes_vector_path(i["state"], i["A"], i["B"], i["C"])
    opt = dict(D=1, z=1, dt_bias=1, softplus=1)
    ssu_check(i, opt, tol, "aligned views (on a clone of the state)")
    # the element path: the same values, contiguous, each base one element off alignment
    e = dict(i, state=off_by_one(i["state"]), A=off_by_one(i["A"]), B=off_by_one(i["B"]), C=off_by_one(i["C"]))
    assert not takes_vector_path(e["state"], e["A"], e["B"], e["C"])
    want_out, want_state = ssu_check(e, opt, tol, "misaligned copies")
    # the launch on the views themselves
    state = i["state"]
    out = selective_state_update(state, i["x"], i["dt"], i["A"], i["B"], i["C"], D=i["D"], z=i["z"], dt_bias=i["dt_bias"], dt_softplus=True)
    assert torch.equal(out, want_out) and torch.equal(state, want_state)          # the vector (+ tail) path gives the element path's bits
    state.copy_(cache0[:B, :, :N])
    assert torch.equal(cache, cache0)                                              # nothing outside the view was written


@pytest.mark.parametrize("R", [1, 2, 36])
def test_state_update_forms_dt_proj_itself(R, exact_fp32):
    B, D, N = 3, 65, 16
    i = ssu_inputs(B, D, N, torch.float32, seed=31)
    x_db = rnd(B, R + 2 * N, seed=32)
    dt_w, dt_x = rnd(D, R, seed=33) * R ** -0.5, x_db[:, :R]
    dt64 = dt_x.double() @ dt_w.double().t()
    for opt in OPTIONS:
        fused, s_fused = ssu_check(i, opt, SSU_TOL[torch.float32], f"R{R} fused", dt_proj=(dt_w, dt_x), dt64=dt64)
        plain, s_plain = ssu_check(dict(i, dt=F.linear(dt_x, dt_w)), opt, SSU_TOL[torch.float32], f"R{R} F.linear", dt64=dt64)
        close(fused, plain, SSU_TOL[torch.float32], "fused vs F.linear")
        close(s_fused, s_plain, SSU_TOL[torch.float32], "fused vs F.linear state")
    from dimsum_amd import native
    with pytest.raises(RuntimeError, match="replaces dt"):
        native.selective_state_update(i["state"].clone(), i["x"], i["dt"], i["A"], i["B"], i["C"], dt_proj=(dt_w, dt_x))


def test_two_launches_from_equal_inputs_are_bit_identical():
    from dimsum_amd.ops import causal_conv1d_update, selective_state_update
    for dtype in DTYPES:
        x, st, w, b = rnd(3, 129, dtype=dtype), rnd(3, 129, 4, dtype=dtype, seed=1), rnd(129, 4, seed=2), rnd(129, seed=3)
        s1, s2 = st.clone(), st.clone()
        assert torch.equal(causal_conv1d_update(x, s1, w, b, "silu"), causal_conv1d_update(x, s2, w, b, "silu")) and torch.equal(s1, s2)
        for N in (16, 17):
            i = ssu_inputs(3, 129, N, dtype, seed=5)
            outs = []
            for _ in range(2):
                s = i["state"].clone()
                outs.append((selective_state_update(s, i["x"], i["dt"], i["A"], i["B"], i["C"], D=i["D"], z=i["z"], dt_bias=i["dt_bias"],
                                                    dt_softplus=True), s))
            assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ---- the modules -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def exact_fp32():
    old = torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = torch.backends.cudnn.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32 = old


def gpu_mixer(cls):
    from dimsum_amd.modules import mamba_simple
    m = getattr(mamba_simple, cls)(**MIXER, layer_idx=3, scan_type="none", **({"d_cond": 48} if cls == "CondMamba" else {})).eval()
    procedural_fill(m, seed=7)
    return m.to(DEV)


@pytest.mark.parametrize("prefill", [1, 3, 5])
@pytest.mark.parametrize("cls", ["Mamba", "CondMamba"])
def test_prefill_then_steps_equal_one_forward(cls, prefill, exact_fp32):
    g = golden("mixer_step")
    tol = SSU_TOL[torch.float32]
    m = gpu_mixer(cls)
    x = T(g[f"{cls}_x"]).to(DEV)
    args = (T(g[f"{cls}_c"]).to(DEV),) if cls == "CondMamba" else ()
    with torch.no_grad():
        full = m(x, *args)
    ys, p = run_recurrent(m, x, args, prefill)
    conv_state, ssm_state = p.key_value_memory_dict[3]
    close(ys, full, tol, "prefill + steps vs one fused forward")
    close(ys, T(g[f"{cls}_y_steps"]), tol, "prefill + steps vs the fixture")
    close(full, T(g[f"{cls}_y_full"]), tol, "one forward vs the fixture")
    close(conv_state, T(g[f"{cls}_conv_state"]), tol, "conv_state")
    close(ssm_state, T(g[f"{cls}_ssm_state"]), tol, "ssm_state")


def test_a_step_replayed_from_a_captured_graph(exact_fp32):
    """one step captured on static buffers (a single stream: no parallel branches), replayed 4 times == 4 eager steps, bit for bit"""
    m = gpu_mixer("Mamba")
    x = T(golden("mixer_step")["Mamba_x"]).to(DEV)
    with torch.no_grad():
        eager_states = m.allocate_inference_cache(2, L)
        eager = [m.step(x[:, t:t + 1], *eager_states)[0].clone() for t in range(4)]
        conv_state, ssm_state = m.allocate_inference_cache(2, L)
        token = x[:, :1].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m.step(token, conv_state, ssm_state)                   # warm-up outside the capture (library handles, workspaces)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = m.step(token, conv_state, ssm_state)[0]
        conv_state.zero_()
        ssm_state.zero_()
        replayed = []
        for t in range(4):
            token.copy_(x[:, t:t + 1])
            graph.replay()
            replayed.append(out.clone())
    torch.cuda.synchronize()
    for t in range(4):
        assert torch.equal(replayed[t], eager[t]), t
    assert torch.equal(conv_state, eager_states[0]) and torch.equal(ssm_state, eager_states[1])


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------
def test_library_refuses_bad_shapes_before_any_launch():
    from dimsum_amd import _lib, native
    lib = _lib.load()
    x, st, w = rnd(2, 8), rnd(2, 8, 5, seed=1), rnd(8, 5, seed=2)
    out, st0 = torch.full_like(x, 7.0), st.clone()
    P = _lib.ConvUpdateParams()
    P.batch, P.dim, P.width = 2, 8, 5
    P.x_batch_stride, P.x_c_stride = x.stride()
    P.state_batch_stride, P.state_c_stride, P.state_w_stride = st.stride()
    P.weight_c_stride, P.weight_width_stride = w.stride()
    P.out_batch_stride, P.out_c_stride = out.stride()
    P.x_ptr, P.weight_ptr, P.conv_state_ptr, P.out_ptr = x.data_ptr(), w.data_ptr(), st.data_ptr(), out.data_ptr()
    assert lib.dimsum_causal_conv1d_update(P, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 3      # DIMSUM_ERR_SHAPE
    with pytest.raises(RuntimeError, match="width between 2 and 4"):
        native.causal_conv1d_update(x, st, w, None, True)
    s, A, Bm = rnd(2, 8, 257, seed=3), -urnd(8, 257) - 1.0, rnd(2, 257, seed=4)
    s0 = s.clone()
    Q = _lib.StateUpdateParams()
    Q.batch, Q.dim, Q.dstate = 2, 8, 257
    Q.state_batch_stride, Q.state_d_stride, Q.state_n_stride = s.stride()
    Q.x_batch_stride, Q.x_d_stride = Q.dt_batch_stride, Q.dt_d_stride = Q.out_batch_stride, Q.out_d_stride = x.stride()
    Q.A_d_stride, Q.A_n_stride = A.stride()
    Q.B_batch_stride, Q.B_n_stride = Q.C_batch_stride, Q.C_n_stride = Bm.stride()
    Q.state_ptr, Q.x_ptr, Q.dt_ptr, Q.A_ptr, Q.B_ptr, Q.C_ptr, Q.out_ptr = (t.data_ptr() for t in (s, x, x, A, Bm, Bm, out))
    assert lib.dimsum_selective_state_update(Q, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 3    # DIMSUM_ERR_SHAPE
    with pytest.raises(RuntimeError, match="between 1 and 256"):
        native.selective_state_update(s, x, x, A, Bm, Bm)
    torch.cuda.synchronize()
    assert torch.equal(st, st0) and torch.equal(s, s0) and bool((out == 7.0).all())       # nothing ran
