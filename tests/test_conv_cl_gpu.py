"""GPU parity of csrc/causal_conv1d_cl.hip, the causal conv1d on channel-last operands ((batch, seqlen, dim) memory, seen as (batch, dim, seqlen)
views with channel stride 1), through dimsum_amd.native and causal_conv1d_fn: every width, SiLU and bias on and off, lengths around the
taps and around the kernel's token chunk, dims on the 16-byte vector path and on the element path of each dtype, channel slices of wider
buffers, misaligned and batch-strided views, out / dx written into views, both dout layouts, autograd, saturated SiLU, a batch stride past
2^31 elements, the backward's batch fold, and agreement with the seqlen-contiguous kernel.

Reference: the C oracle (oracle/c_ops.py, float64 inside) on a contiguous (B, D, L) fp32 copy, or float64 torch.nn.functional.conv1d (+ SiLU)
under autograd on the CPU. fp32 tolerances are the ones tests/test_norm_conv_paths_gpu.py holds for the seqlen-contiguous kernel (out, dx:
rtol 1e-5, atol 2e-6, scale_atol 1e-6; dweight, dbias: rtol 1e-4, scale_atol 1e-5); a half-precision output adds the half-ulp of its type
(2^-8 bfloat16, 2^-11 float16) because it is the rounding of an fp32 value. Every comparison prints `measured ...` (largest |error| and
largest error / bound) before it asserts (pytest -s); the docstrings quote the largest error / bound seen on an MI355X."""
import numpy as np
import pytest
import torch

from conftest import assert_close

pytestmark = pytest.mark.gpu

HALF_ULP = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
OUT_TOL = dict(rtol=1e-5, atol=2e-6, scale_atol=1e-6)
SUM_TOL = dict(rtol=1e-4, scale_atol=1e-5)


def _chunk():
    from dimsum_amd import native
    return native.CONV_CL_CHUNK


C = 64     # native.CONV_CL_CHUNK, asserted below: parametrize needs it at import time, before the package is imported


def test_chunk_constant():
    assert _chunk() == C


def _np(t):
    return None if t is None else np.ascontiguousarray(t.detach().float().cpu().numpy())


def _close(what, got, ref, rtol, atol=0.0, scale_atol=0.0):
    """conftest.assert_close, after printing the measured error next to its bound"""
    a, b = (t.detach().cpu().double().numpy() if torch.is_tensor(t) else np.asarray(t, np.float64) for t in (got, ref))
    if a.shape == b.shape and b.size:
        err = np.abs(a - b)
        tol = atol + scale_atol * np.abs(b).max() + rtol * np.abs(b)
        ratio = np.divide(err, tol, out=np.where(err > 0, np.inf, 0.0), where=tol > 0)
        print(f"measured {what}: max |err| {np.nanmax(err):.3e}, worst err / bound {np.nanmax(ratio):.3f}")
    assert_close(a, b, rtol, atol, what, scale_atol=scale_atol)


def _cl(t):
    """the same (B, D, L) values in (B, L, D) memory"""
    return t.transpose(1, 2).contiguous().transpose(1, 2)


def _is_cl(t):
    return t.stride(1) == 1 or t.shape[1] == 1


def _inputs(B, D, L, W, seed, dt=torch.float32, bias=True):
    """x, weight, bias, dout on the GPU; x and dout channel-last"""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    return _cl(rn(B, D, L).to(dt).cuda()), rn(D, W).cuda(), (rn(D).cuda() if bias else None), _cl(rn(B, D, L).to(dt).cuda())


def _check(tag, x, w, b, dout, silu, out=None, dx=None, relative=False):
    """forward + backward of channel-last GPU tensors against the oracle on contiguous fp32 copies; out and dx must be channel-last"""
    from dimsum_amd import native
    from oracle import c_ops
    assert _is_cl(x) and (x.stride(2) != 1 or x.shape[2] == 1 or x.shape[1] == 1), "the test must feed the channel-last kernels"
    out_g = native.causal_conv1d_fwd(x, w, b, silu, out=out)
    dx_g, dw_g, db_g = native.causal_conv1d_bwd(x, w, b, dout, dx, silu)
    assert out_g.dtype == x.dtype and dx_g.dtype == x.dtype and out_g.shape == x.shape and dx_g.shape == x.shape
    assert _is_cl(out_g) and _is_cl(dx_g), (out_g.stride(), dx_g.stride())
    if out is not None:
        assert out_g.data_ptr() == out.data_ptr()
    if dx is not None:
        assert dx_g.data_ptr() == dx.data_ptr()
    ref_out = c_ops.causal_conv1d_fwd(_np(x), _np(w), _np(b), silu)
    rdx, rdw, rdb = c_ops.causal_conv1d_bwd(_np(x), _np(w), _np(b), _np(dout), silu)
    rtol = 1e-5 + HALF_ULP[x.dtype]
    tol = dict(atol=0.0, scale_atol=2e-6) if relative else dict(atol=2e-6, scale_atol=1e-6)
    _close(f"{tag} out", out_g, ref_out, rtol, **tol)
    _close(f"{tag} dx", dx_g, rdx, rtol, **tol)
    _close(f"{tag} dweight", dw_g, rdw, **SUM_TOL)
    if b is not None:
        _close(f"{tag} dbias", db_g, rdb, **SUM_TOL)
    else:
        assert db_g is None
    return dict(out=out_g, dx=dx_g, dw=dw_g, db=db_g)


# (batch, dim, SiLU, bias, dtype): dim 4 = one fp32 vector, 7 = the element path, 8 = one 16-bit vector, 12 = fp32 vectors but 16-bit elements,
# 264 = 66 fp32 vectors (a second channel block with two lanes) / 33 16-bit vectors
CASES = [(3, 4, True, True, torch.float32), (1, 7, True, False, torch.float32), (3, 7, False, True, torch.bfloat16),
         (1, 8, True, True, torch.bfloat16), (3, 8, False, False, torch.float16), (1, 12, False, True, torch.float32),
         (3, 12, True, True, torch.float16), (3, 264, True, True, torch.float32), (1, 264, True, False, torch.bfloat16)]


@pytest.mark.parametrize("W", [2, 3, 4])
@pytest.mark.parametrize("L", [1, 2, 3, C - 1, C, C + 1, 2 * C + 3])
def test_cl_lengths_dims_dtypes(L, W):
    """rows shorter than the taps, one token short of a chunk, a full chunk, one token into the second chunk (its halo rows re-read, the
    gradient halo rebuilt from the tokens after the first), two chunks and a 3-token tail (the one-token loops).
    measured: worst error / bound half precision out 0.99, dx 0.99 (the half-ulp is attained), fp32 out 0.03, dx 0.12; dweight 0.03, dbias 0.02"""
    for B, D, silu, bias, dt in CASES:
        x, w, b, dout = _inputs(B, D, L, W, seed=B + D + L + W, dt=dt, bias=bias)
        _check(f"B{B} D{D} {dt} silu={silu} bias={bias}", x, w, b, dout, silu)


def _wide(B, L, Dw, dt, gen):
    return torch.randn(B, L, Dw, generator=gen).to(dt).cuda()


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("D", [8, 12])
@pytest.mark.parametrize("view", ["first_half", "second_half", "one_channel_in", "batch_strided"])
def test_cl_views_of_wider_buffers(view, D, dt):
    """x and dout as views, never copied: the two halves of a (B, L, 2 D) buffer (the second starts D elements in: 16-byte aligned for
    D = 8 and for fp32 at D = 12, the element path for bfloat16 at D = 12), a slice one channel in (misaligned: the element path) and
    every second batch row of a taller buffer. measured: worst error / bound out 0.99, dx 0.99 (bfloat16: the half-ulp), dweight 0.02, dbias 0.01"""
    B, L, W = 3, C + 5, 4
    gen = torch.Generator().manual_seed(D + len(view))
    w, b = torch.randn(D, W, generator=gen).cuda(), torch.randn(D, generator=gen).cuda()
    if view == "batch_strided":
        xb, gb = _wide(2 * B, L, D, dt, gen), _wide(2 * B, L, D, dt, gen)
        x, dout = xb[::2].transpose(1, 2), gb[::2].transpose(1, 2)
        assert x.stride() == (2 * L * D, 1, D)
    else:
        lo = {"first_half": 0, "second_half": D, "one_channel_in": 1}[view]
        xb, gb = _wide(B, L, 2 * D, dt, gen), _wide(B, L, 2 * D, dt, gen)
        x, dout = xb[..., lo:lo + D].transpose(1, 2), gb[..., lo:lo + D].transpose(1, 2)
        assert x.stride() == (2 * L * D, 1, 2 * D) and x.data_ptr() == xb.data_ptr() + lo * xb.element_size()
    _check(view, x, w, b, dout, True)


@pytest.mark.parametrize("dt", [torch.float32, torch.float16])
@pytest.mark.parametrize("D", [8, 7])
def test_cl_out_and_dx_into_views(D, dt):
    """out= and dx= as channel slices of NaN-filled (B, L, 2 D + 1) buffers, one on the vector path (D = 8, slice at 0) and one on the
    element path: every column outside the slice keeps its NaN. measured: worst error / bound out 0.95, dx 0.95 (float16: the half-ulp), dweight 0.02, dbias 0.02"""
    B, L, W = 3, C + 1, 3
    x, w, b, dout = _inputs(B, D, L, W, seed=D, dt=dt)
    lo = 0 if D == 8 else 3
    bufs = []
    for _ in range(2):
        buf = torch.full((B, L, 2 * D + 1), float("nan"), device="cuda", dtype=dt)
        outside = torch.ones_like(buf, dtype=torch.bool)
        outside[..., lo:lo + D] = False
        bufs.append((buf, buf[..., lo:lo + D].transpose(1, 2), outside))
    _check("views", x, w, b, dout, True, out=bufs[0][1], dx=bufs[1][1])
    for buf, view, outside in bufs:
        assert torch.isnan(buf[outside]).all(), "the kernel wrote outside the view it was given"
        assert torch.isfinite(view).all()


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_cl_dout_seqlen_contiguous_is_converted_once(dt):
    """a dout in (B, D, L) memory against a channel-last x: native brings it to x's layout (one transposing copy) and dx is still
    channel-last. measured: worst error / bound out 0.97, dx 0.96 (bfloat16: the half-ulp), dweight 0.02, dbias 0.01"""
    x, w, b, dout = _inputs(3, 12, C + 2, 4, seed=5, dt=dt)
    dout = dout.contiguous()
    assert dout.stride(2) == 1 and dout.stride(1) != 1
    _check("dout (B, D, L)", x, w, b, dout, True)


@pytest.mark.parametrize("sliced", [False, True])
def test_cl_causal_conv1d_fn_under_autograd(sliced):
    """causal_conv1d_fn on the transpose of a (B, L, D) activation, or of the first half of a (B, L, 2 D) xz: the output is channel-last,
    x.grad (re-strided by autograd to the leaf) and the gradients of weight and bias match float64 conv1d + SiLU under autograd on the CPU.
    measured: worst error / bound out 0.02, dx 0.09, dweight 0.01, dbias 0.01"""
    from dimsum_amd.ops.causal_conv1d_interface import causal_conv1d_fn
    B, D, L, W = 2, 24, C + 7, 4
    gen = torch.Generator().manual_seed(L + sliced)
    xz0, w0, b0, dout0 = (torch.randn(*s, generator=gen) for s in ((B, L, 2 * D if sliced else D), (D, W), (D,), (B, D, L)))
    seen = {}

    def run(to, fn, tag):
        xz, w, b = (to(t).requires_grad_() for t in (xz0, w0, b0))
        x = (xz[..., :D] if sliced else xz).transpose(1, 2)
        out = fn(x, w, b)
        seen[tag] = (x.stride(), out.stride())
        out.backward(to(dout0))
        return out, xz.grad, w.grad, b.grad

    ref_fn = lambda x, w, b: torch.nn.functional.silu(torch.nn.functional.conv1d(x, w.unsqueeze(1), b, padding=W - 1, groups=D)[..., :L])
    got = run(lambda t: t.cuda(), lambda x, w, b: causal_conv1d_fn(x, w, b, activation="silu"), "gpu")
    ref = run(lambda t: t.double(), ref_fn, "ref")
    x_stride, out_stride = seen["gpu"]
    assert x_stride[1] == 1 and out_stride[1] == 1 and out_stride == (L * D, 1, D), (x_stride, out_stride)
    for name, a, r, tol in zip(("out", "dx", "dweight", "dbias"), got, ref, (OUT_TOL,) * 2 + (SUM_TOL,) * 2):
        assert a.dtype == torch.float32
        _close(name, a, r, **tol)


def test_cl_saturated_silu():
    """x * 30: pre-activations of magnitude 20 .. 100 and beyond in both signs through sigmoidf_fast / SiLU' (exp overflows to inf on the
    negative side). Everything stays finite and within the fp32 tolerances taken relative to max|ref|.
    measured: worst error / bound out 0.01, dx 0.15, dweight 0.01, dbias 0.02"""
    from oracle import c_ops
    x, w, b, dout = _inputs(2, 16, 300, 4, seed=30)
    x = x * 30
    pre = c_ops.causal_conv1d_fwd(_np(x), _np(w), _np(b), False)
    assert (pre > 20).sum() > 100 and (pre < -20).sum() > 100 and (pre > 100).any() and (pre < -100).any()
    got = _check("saturated", x, w, b, dout, True, relative=True)
    for k in ("out", "dx", "dw", "db"):
        assert torch.isfinite(got[k]).all(), k


@pytest.mark.parametrize("W,silu", [(4, True), (2, False)])
def test_cl_agrees_with_the_seqlen_contiguous_kernel(W, silu):
    """the same values through both kernels: each is a rounding of the same fp32 expression, so they agree within twice the fp32 bound
    (not bit for bit: the FMA order differs). measured: worst error / (2 x bound) at most 0.09 for every quantity"""
    from dimsum_amd import native
    x, w, b, dout = _inputs(3, 40, 2 * C + 9, W, seed=W)
    xc, dc = x.contiguous(), dout.contiguous()
    assert xc.stride(2) == 1 and x.stride(1) == 1
    out, (dx, dw, db) = native.causal_conv1d_fwd(x, w, b, silu), native.causal_conv1d_bwd(x, w, b, dout, None, silu)
    out_c, (dx_c, dw_c, db_c) = native.causal_conv1d_fwd(xc, w, b, silu), native.causal_conv1d_bwd(xc, w, b, dc, None, silu)
    assert out.stride(1) == 1 and dx.stride(1) == 1 and out_c.stride(2) == 1 and dx_c.stride(2) == 1
    twice = lambda t: {k: 2 * v for k, v in t.items()}
    _close("out", out, out_c, **twice(OUT_TOL))
    _close("dx", dx, dx_c, **twice(OUT_TOL))
    _close("dweight", dw, dw_c, **twice(SUM_TOL))
    _close("dbias", db, db_c, **twice(SUM_TOL))


def test_cl_backward_batch_fold():
    """131072 channels = 512 channel blocks of fp32 vectors: the backward launches two grid rows for three batch rows, so one wave sums
    rows 0 and 2 in its registers before its atomics. measured: worst error / bound out 0.02, dx 0.14, dweight 0.02, dbias 0.01"""
    x, w, b, dout = _inputs(3, 131072, 5, 4, seed=11)
    _check("fold", x, w, b, dout, True)


def test_cl_batch_stride_past_2_31_elements():
    """two batch rows 2^31 + 64 elements apart in one bfloat16 buffer (x and out), dx likewise: the row offsets need 64-bit arithmetic.
    Only the two small rows are touched. measured: worst error / bound out 0.99, dx 0.99 (the half-ulp), dweight 0.01, dbias 0.01"""
    B, D, L, W = 2, 16, C + 3, 4
    stride = 2 ** 31 + 64
    x0, w, b, dout = _inputs(B, D, L, W, seed=31, dt=torch.bfloat16)
    views = []
    for _ in range(3):
        buf = torch.empty(stride + L * D, device="cuda", dtype=torch.bfloat16)
        views.append(buf.as_strided((B, D, L), (stride, 1, D)))
    x, out, dx = views
    x.copy_(x0)
    _check("far rows", x, w, b, dout, True, out=out, dx=dx)


def test_cl_empty_batch_and_refused_layouts():
    from dimsum_amd import native
    w, b = torch.randn(8, 4, device="cuda"), torch.randn(8, device="cuda")
    x0 = torch.empty(0, 5, 8, device="cuda").transpose(1, 2)
    out = native.causal_conv1d_fwd(x0, w, b, True)
    assert tuple(out.shape) == (0, 8, 5)
    dx, dw, db = native.causal_conv1d_bwd(x0, w, b, x0, None, True)
    assert tuple(dx.shape) == (0, 8, 5) and not dw.any() and not db.any()
    neither = torch.randn(2, 16, 10, device="cuda")[:, ::2, ::2]
    with pytest.raises(RuntimeError, match="only seqlen-contiguous"):
        native.causal_conv1d_fwd(neither, w, b, True)
    x = torch.randn(2, 5, 8, device="cuda").transpose(1, 2)
    with pytest.raises(RuntimeError, match="channel-last"):
        native.causal_conv1d_fwd(x, w, b, True, out=torch.empty(2, 8, 5, device="cuda"))
    with pytest.raises(RuntimeError, match="bad dx"):
        native.causal_conv1d_bwd(x, w, b, x, torch.empty(2, 8, 5, device="cuda"), True)
