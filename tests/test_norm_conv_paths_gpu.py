"""GPU parity of csrc/norm.hip and csrc/causal_conv1d.hip on the paths the other suites leave out: LayerNorm (mean, the c2 term, dbias,
the masked variance of the element-wise path), folded modulation as _ln_modulate calls it, half-precision I/O, the second row per trip and the
8-piece kernel of the norm backward over many rows, the forward grid-stride loop, row-strided and misaligned views, LayerNormFn and
causal_conv1d_fn under autograd, the width limit; for the conv the half-precision backward, very short rows, misaligned rows, layouts of
out / dout that differ from x, a strided weight, the backward batch split and saturated SiLU.

References: the C oracle (oracle/c_ops.py, float64 inside) or a float64 numpy / torch expression on the CPU. fp32 tolerances are the ones
tests/test_conv_norm_gpu.py holds; a half-precision output adds the half-ulp of its type (rtol 2^-8 bfloat16, 2^-11 float16) because it is the
rounding of an fp32 value. Every comparison prints `measured ...` (largest |error| and largest error / bound) before it asserts (pytest -s);
the docstrings quote the largest error / bound seen on an MI355X."""
import numpy as np
import pytest
import torch

from conftest import assert_close

pytestmark = pytest.mark.gpu

HALF_ULP = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


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


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---------------------------------------------------------------------------------------------------------------------
# norm
# ---------------------------------------------------------------------------------------------------------------------
EPS = 1e-5


def _norm_inputs(M, N, seed, bias=True, residual=True, dres=True):
    """weight 1 + 0.1 randn, bias randn, x = randn + 3 (a row mean LayerNorm has to remove), residual, dy, dresidual -- CPU fp32"""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    return dict(x=rn(M, N) + 3, w=1 + 0.1 * rn(N), b=rn(N) if bias else None, res=rn(M, N) if residual else None, dy=rn(M, N),
                dro=rn(M, N) if dres else None)


def _norm_oracle(c, is_rms, eps=EPS):
    from oracle import c_ops
    y, ro, mean, rstd = c_ops.norm_fwd(_np(c["x"]), _np(c["w"]), _np(c["b"]), _np(c["res"]), eps, is_rms)
    dx, dw, db = c_ops.norm_bwd(ro, _np(c["w"]), _np(c["dy"]), _np(c["dro"]), eps, is_rms)
    return dict(y=y, ro=ro, mean=mean, rstd=rstd, dx=dx, dw=dw, db=db)


def _norm_gpu(c, is_rms, eps=EPS, place=None):
    """forward + backward through dimsum_amd.native; `place` puts each (M, N) operand on the GPU (contiguous, or as a view of a wider buffer).
    The backward reads the saved stream through `place` too, so r_row_stride follows the layout under test."""
    from dimsum_amd import native
    dev = lambda t: None if t is None else t.cuda()
    put = place or dev
    x, res, dy, dro = (None if c[k] is None else put(c[k]) for k in ("x", "res", "dy", "dro"))
    w, b = dev(c["w"]), dev(c["b"])
    y, mean, rstd, ro = native.layer_norm_fwd(x, w, b, eps, residual=res, is_rms_norm=is_rms)
    r = ro if res is None or place is None else place(ro)
    dx, dw, db, dres_in = native.layer_norm_bwd(dy, r, w, b, eps, mean, rstd, dresidual=dro, has_residual=res is not None, is_rms_norm=is_rms)
    return dict(x=x, y=y, mean=mean, rstd=rstd, ro=ro, dx=dx, dw=dw, db=db, dres_in=dres_in)


def _check_norm(tag, got, ref, c, is_rms):
    """the tolerances of test_norm_vs_golden / test_norm_vs_oracle"""
    _close(f"{tag} y", got["y"], ref["y"], 1e-5, 1e-5)
    _close(f"{tag} rstd", got["rstd"], ref["rstd"], 1e-6)
    if is_rms:
        assert got["mean"] is None
    else:
        _close(f"{tag} mean", got["mean"], ref["mean"], 1e-6, scale_atol=1e-6)
    if c["res"] is not None:
        assert np.array_equal(_np(got["ro"]), ref["ro"]), f"{tag}: residual_out is the fp32 sum, bit for bit"
        assert got["dres_in"] is not None
        _close(f"{tag} dresidual_in", got["dres_in"], ref["dx"], 1e-4, 1e-5)
    _close(f"{tag} dx", got["dx"], ref["dx"], 1e-4, 1e-5)
    _close(f"{tag} dweight", got["dw"], ref["dw"], 1e-4, scale_atol=1e-5)
    if c["b"] is not None:
        _close(f"{tag} dbias", got["db"], ref["db"], 1e-4, scale_atol=1e-5)
    else:
        assert got["db"] is None


# one shape per launcher branch (1 / 2 / 4 / 5 / 8 register pieces) and memory path (16-byte vectors when N % 4 == 0, else element-wise);
# 3100 rows: the backward's grid is capped at 384 workgroups = 1536 rows per trip, so its second row per trip is live for every wave in the
# first trip and missing (re-reading the first) in the second; 3100 x 2048: the one-row-per-trip kernel over three trips;
# 16500 rows: more than the forward's 4096 workgroups x 4 rows
LN_SHAPES = [(37, 100), (64, 384), (300, 1000), (257, 1152), (21, 1150), (9, 2048), (6, 2047), (3100, 1024), (3100, 1022), (3100, 2048),
             (16500, 100)]
RMS_SHAPES = [(21, 1150), (6, 2047), (3100, 1024), (3100, 1022), (3100, 2048), (16500, 100)]      # (the rest: test_norm_vs_oracle)


@pytest.mark.parametrize("M,N", LN_SHAPES)
def test_layernorm_fwd_bwd_vs_oracle(M, N):
    """y, mean, rstd, residual_out (bit for bit), dx, dresidual_in, dweight, dbias with bias, residual and dresidual.
    measured: worst error / bound y 0.07, rstd 0.20, mean 0.08, dx 0.03, dweight 0.03, dbias 0.03"""
    c = _norm_inputs(M, N, seed=M + N)
    _check_norm(f"LN {M}x{N}", _norm_gpu(c, False), _norm_oracle(c, False), c, False)


@pytest.mark.parametrize("M,N", RMS_SHAPES)
def test_rmsnorm_fwd_bwd_vs_oracle_rows_and_paths(M, N):
    """the same for RMSNorm (with a bias) at the shapes test_norm_vs_oracle leaves out.
    measured: worst error / bound y 0.04, rstd 0.20, dx 0.01, dweight 0.03, dbias 0.03"""
    c = _norm_inputs(M, N, seed=M + N + 1)
    _check_norm(f"RMS {M}x{N}", _norm_gpu(c, True), _norm_oracle(c, True), c, True)


@pytest.mark.parametrize("is_rms", [False, True])
@pytest.mark.parametrize("M,N", [(64, 384), (21, 1150), (300, 1000), (3100, 1022)])
def test_norm_without_residual_and_without_dresidual(M, N, is_rms):
    """the non-prenorm call: no residual is added (residual_out IS x), the backward gets no dresidual (dres_ptr null) and returns no
    dresidual_in. measured: worst error / bound y 0.07, rstd 0.19, mean 0.08, dx 0.01, dweight 0.03, dbias 0.03"""
    c = _norm_inputs(M, N, seed=7 * M + N, residual=False, dres=False)
    got = _norm_gpu(c, is_rms)
    assert got["ro"] is got["x"], "nothing is added and no dtype changes: residual_out is x itself"
    assert got["dres_in"] is None
    _check_norm(f"{'RMS' if is_rms else 'LN'} {M}x{N} no residual", got, _norm_oracle(c, is_rms), c, is_rms)


def _wide_view(t, shift):
    """t (M, N) as columns [shift, shift + N) of a NaN-filled (M, 2N) GPU buffer: row stride 2N; shift = 1 moves the base pointer off 16 bytes"""
    M, N = t.shape
    buf = torch.full((M, 2 * N), float("nan"), device="cuda", dtype=t.dtype)
    v = buf[:, shift:shift + N]
    v.copy_(t)                                                  # (from the CPU or from the GPU)
    return v


@pytest.mark.parametrize("is_rms", [False, True])
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("M,N", [(4, 1024), (37, 384), (130, 1152), (1600, 100)])
def test_norm_row_strided_and_misaligned_views(M, N, shift, is_rms):
    """x, residual, dy, dresidual and the saved stream as column ranges of wider buffers (what _as_rows hands over for a channel slice):
    against the oracle, and bit for bit against the contiguous call -- both memory paths fill the same registers and do the same arithmetic.
    dweight / dbias are sums of one float atomic per workgroup and column, so their bits depend on the order the workgroups finish in:
    they are compared bit for bit where a single workgroup runs (M <= 4) and against the oracle everywhere.
    measured: worst error / bound y 0.06, rstd 0.18, mean 0.08, dx 0.03, dweight 0.02, dbias 0.03; every bit comparison holds"""
    c = _norm_inputs(M, N, seed=M + N + shift)
    ref = _norm_oracle(c, is_rms)
    got = _norm_gpu(c, is_rms, place=lambda t: _wide_view(t, shift))
    assert got["x"].stride(0) == 2 * N and (got["x"].data_ptr() % 16 == 0) == (shift == 0)
    _check_norm(f"{'RMS' if is_rms else 'LN'} {M}x{N} shift {shift}", got, ref, c, is_rms)
    flat = _norm_gpu(c, is_rms)
    for k in ("y", "rstd", "ro", "dx", "dres_in") + (() if is_rms else ("mean",)) + (("dw", "db") if M <= 4 else ()):
        assert _bits_equal(got[k], flat[k]), f"{k}: the strided call differs from the contiguous call"


@pytest.mark.parametrize("B,L,N", [(3, 16, 384), (2, 64, 1152), (2, 8, 1150)])
def test_layernorm_with_folded_modulation_like_ln_modulate(B, L, N):
    """_ln_modulate's call: weight = ones, no bias, eps 1e-6, scale / shift slices of one (B, 6N) adaLN row, rows_per_batch = L, against the
    float64 expression LN(x) * (1 + scale) + shift (rtol 1e-5 + 1e-5 max|ref|: the y tolerance with its absolute part made relative,
    modulated rows are not unit scale); where N % 4 == 0 the three operand images are the images of that fp32 y, bit for bit.
    measured: worst error / bound y 0.01, mean 0.07, rstd 0.12; the three images are bit-identical"""
    from dimsum_amd import native
    gen = torch.Generator().manual_seed(B + L + N)
    x = (torch.randn(B * L, N, generator=gen) + 3).cuda()
    mods = torch.randn(B, 6 * N, generator=gen).cuda()
    shift, scale = mods[:, 3 * N:4 * N], mods[:, 4 * N:5 * N]                      # shift_mlp, scale_mlp of adaLN_modulation(c).chunk(6, dim=1)
    assert shift.stride(0) == 6 * N
    ones = torch.ones(N, device="cuda")
    kw = dict(is_rms_norm=False, mod_scale=scale, mod_shift=shift, rows_per_batch=L)
    y, mean, rstd, ro = native.layer_norm_fwd(x, ones, None, 1e-6, **kw)
    assert ro is x
    xd = x.double().cpu().view(B, L, N)
    mu, var = xd.mean(-1, keepdim=True), xd.var(-1, unbiased=False, keepdim=True)
    ref = ((xd - mu) / torch.sqrt(var + 1e-6) * (1 + scale.double().cpu()[:, None]) + shift.double().cpu()[:, None]).view(B * L, N)
    _close("modulated LN y", y, ref, 1e-5, scale_atol=1e-5)
    _close("modulated LN mean", mean, mu.view(-1), 1e-6, scale_atol=1e-6)
    _close("modulated LN rstd", rstd, 1 / torch.sqrt(var + 1e-6).view(-1), 1e-6)
    if N % 4:
        return
    y3 = native.layer_norm_fwd(x, ones, None, 1e-6, split3=True, **kw)[0]
    assert y3.dtype == torch.bfloat16 and tuple(y3.shape) == (B * L, 3 * N)
    assert _bits_equal(y3, native.split3_rows(y, left=True))
    pair = native.layer_norm_fwd(x, ones, None, 1e-6, split3="pair", **kw)[0]
    assert isinstance(pair, native.PairImage) and tuple(pair.data.shape) == (B * L, 2 * N)
    assert _bits_equal(pair.data[:, :N], y3[:, :N]) and _bits_equal(pair.data[:, N:], y3[:, 2 * N:]) and _bits_equal(pair.image3(), y3)
    img, want = native.layer_norm_fwd(x, ones, None, 1e-6, split3="f16s", **kw)[0], native.rows_f16s(y)
    assert isinstance(img, native.F16Image) and _bits_equal(img.data, want.data) and _bits_equal(img.inv, want.inv)


def _norm_bwd_f64(r, w, dy, dro, mean, rstd, is_rms):
    """float64 backward from the SAVED statistics (what the kernel does); r, dy, dro, mean, rstd: numpy"""
    r, w, dy, rstd = (np.asarray(a, np.float64) for a in (r, w, dy, rstd))
    xhat = (r - (0.0 if is_rms else np.asarray(mean, np.float64)[:, None])) * rstd[:, None]
    wdy = w * dy
    c1 = (xhat * wdy).mean(1, keepdims=True)
    c2 = 0.0 if is_rms else wdy.mean(1, keepdims=True)
    dx = (wdy - (xhat * c1 + c2)) * rstd[:, None] + (0.0 if dro is None else np.asarray(dro, np.float64))
    return dx, (dy * xhat).sum(0), dy.sum(0)


@pytest.mark.parametrize("is_rms", [False, True])
@pytest.mark.parametrize("N", [384, 1150, 2048])
@pytest.mark.parametrize("fp32_stream", [True, False])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_norm_half_precision_io(dt, fp32_stream, N, is_rms):
    """x (and y) in half precision, the residual stream in fp32 or in x's type, against the oracle on the exactly upcast inputs.
    residual_out is the fp32 sum bit for bit, or its round-to-nearest in a half stream; y is the rounding of an fp32 value: the half-ulp of
    its type on top of the fp32 tolerance. Backward with x_dtype half: dx is the rounding of the fp32 call's dx; the fp32 dx against the
    oracle (fp32 stream) or against the float64 backward from the saved statistics (half stream: the saved stream is rounded, the saved
    statistics are those of the unrounded sum). measured: worst error / bound y 0.99 (bfloat16) / 0.96 (float16): the half-ulp is attained; rstd 0.10, mean 0.08, dx 0.02, dweight 0.01, dbias 0.01"""
    from dimsum_amd import native
    M = 33
    c = _norm_inputs(M, N, seed=N + 2 * is_rms + fp32_stream)
    rdt = torch.float32 if fp32_stream else dt
    c["x"], c["res"], c["dy"], c["dro"] = c["x"].to(dt), c["res"].to(rdt), c["dy"].to(dt), c["dro"].to(rdt)
    ref = _norm_oracle(c, is_rms)
    x, res, dy, dro, w, b = (c[k].cuda() for k in ("x", "res", "dy", "dro", "w", "b"))
    y, mean, rstd, ro = native.layer_norm_fwd(x, w, b, EPS, residual=res, is_rms_norm=is_rms)
    assert y.dtype == dt and ro.dtype == rdt and rstd.dtype == torch.float32
    sum32 = c["x"].float() + c["res"].float()
    assert np.array_equal(_np(sum32), ref["ro"])
    assert _bits_equal(ro.cpu(), sum32.to(rdt)), "residual_out: the fp32 sum, rounded to nearest in a half stream"
    _close(f"y {dt}", y, ref["y"], 1e-5 + HALF_ULP[dt], 1e-5)
    _close("rstd", rstd, ref["rstd"], 1e-6)
    if not is_rms:
        _close("mean", mean, ref["mean"], 1e-6, scale_atol=1e-6)
    kw = dict(dresidual=dro, has_residual=True, is_rms_norm=is_rms)
    dxh, dwh, dbh, dres_h = native.layer_norm_bwd(dy, ro, w, b, EPS, mean, rstd, x_dtype=dt, **kw)
    dxf, dwf, dbf, dres_f = native.layer_norm_bwd(dy, ro, w, b, EPS, mean, rstd, x_dtype=torch.float32, **kw)
    assert dxh.dtype == dt and dxf.dtype == torch.float32 and dres_h.dtype == rdt and dres_f.dtype == rdt
    assert _bits_equal(dxh, dxf.to(dt)), "dx in half precision is the rounding of the fp32 dx"
    assert _bits_equal(dres_h, dxf.to(rdt)) and _bits_equal(dres_f, dxf.to(rdt))
    if fp32_stream:
        rdx, rdw, rdb = ref["dx"], ref["dw"], ref["db"]
    else:
        rdx, rdw, rdb = _norm_bwd_f64(_np(ro), _np(w), _np(dy), _np(dro), None if is_rms else _np(mean), _np(rstd), is_rms)
    _close("dx (fp32 call)", dxf, rdx, 1e-4, 1e-5)
    for got_w, got_b in ((dwh, dbh), (dwf, dbf)):
        _close("dweight", got_w, rdw, 1e-4, scale_atol=1e-5)
        _close("dbias", got_b, rdb, 1e-4, scale_atol=1e-5)


def _norm_f64(x, w, b, res, eps, is_rms):
    r = x if res is None else x + res
    if is_rms:
        y = r * torch.rsqrt(r.pow(2).mean(-1, keepdim=True) + eps) * w
    else:
        y = (r - r.mean(-1, keepdim=True)) * torch.rsqrt(r.var(-1, unbiased=False, keepdim=True) + eps) * w
    return (y if b is None else y + b), r


# name, N, x dtype, channel slice, residual, prenorm, residual_in_fp32, the stream output gets a gradient
_F32, _BF16 = torch.float32, torch.bfloat16
AUTOGRAD_CASES = [
    ("plain", 384, _F32, False, False, False, False, False),
    ("residual", 1150, _F32, False, True, False, False, False),
    ("prenorm_residual", 384, _F32, False, True, True, False, True),
    ("prenorm_no_residual_fp32_stream", 1152, _F32, False, False, True, True, True),
    ("prenorm_stream_without_gradient", 384, _F32, False, True, True, False, False),
    ("channel_slice_prenorm_residual", 384, _F32, True, True, True, True, True),
    ("channel_slice_odd_width", 1150, _F32, True, False, False, False, False),
    ("bf16_x_fp32_residual", 384, _BF16, False, True, True, True, True),
    ("bf16_x_residual_in_fp32_no_residual", 1152, _BF16, False, False, True, True, True),
]


@pytest.mark.parametrize("is_rms", [False, True])
@pytest.mark.parametrize("name,N,dt,sliced,with_res,prenorm,res_fp32,stream_grad", AUTOGRAD_CASES, ids=[c[0] for c in AUTOGRAD_CASES])
def test_layernorm_fn_under_autograd(name, N, dt, sliced, with_res, prenorm, res_fp32, stream_grad, is_rms):
    """ops/layernorm.py: layer_norm_fn / rms_norm_fn forward and the gradients of x, weight, bias and the residual against torch's float64
    autograd on the CPU, for a (B, L, N) input: prenorm or not, with and without residual, residual_in_fp32, x a channel slice of a
    (B, L, 2N) tensor (a strided view out of _as_rows), a prenorm stream that gets no gradient, bfloat16 x (y and dx then carry the
    half-ulp of bfloat16). measured: worst error / bound y 0.99 and dx 0.97 (bfloat16 rounding), stream 0.05, dresidual 0.03, dweight 0.02, dbias 0.01"""
    from dimsum_amd.ops.layernorm import layer_norm_fn, rms_norm_fn
    B, L = 3, 50
    gen = torch.Generator().manual_seed(N + len(name))
    rn = lambda *s: torch.randn(*s, generator=gen)
    width = 2 * N if sliced else N
    x0 = (rn(B, L, width) + 3).to(dt)
    r0 = rn(B, L, width) if with_res else None
    w0, b0 = 1 + 0.1 * rn(N), rn(N)
    dy0, ds0 = rn(B, L, N).to(dt), rn(B, L, N)
    sl = (lambda t: t[..., N // 2:N // 2 + N]) if sliced else (lambda t: t)

    def run(to, fn):
        leaves = [None if t is None else to(t).requires_grad_() for t in (x0, w0, b0, r0)]
        x, w, b, r = leaves
        out = fn(sl(x), w, b, None if r is None else sl(r))
        y, stream = out if prenorm else (out[0] if isinstance(out, tuple) else out, None)
        outs, grads = [y], [to(dy0).to(y.dtype)]
        if prenorm and stream_grad:
            outs.append(stream)
            grads.append(to(ds0).to(stream.dtype))
        torch.autograd.backward(outs, grads)
        return y, stream, [None if t is None else t.grad for t in leaves]

    if is_rms:
        gpu_fn = lambda x, w, b, r: rms_norm_fn(x, w, b, residual=r, prenorm=prenorm, residual_in_fp32=res_fp32, eps=EPS)
    else:
        gpu_fn = lambda x, w, b, r: layer_norm_fn(x, w, b, residual=r, eps=EPS, prenorm=prenorm, residual_in_fp32=res_fp32)
    y, stream, (dx, dw, db, dr) = run(lambda t: t.cuda(), gpu_fn)
    y_ref, s_ref, (dx_ref, dw_ref, db_ref, dr_ref) = run(lambda t: t.double(), lambda x, w, b, r: _norm_f64(x, w, b, r, EPS, is_rms)[:2 if prenorm else 1])
    assert y.dtype == dt and tuple(y.shape) == (B, L, N) and dx.dtype == dt and dx.shape == x0.shape
    _close("y", y, y_ref, 1e-5 + HALF_ULP[dt], 1e-5)
    if prenorm:
        want = torch.float32 if (res_fp32 or dt == torch.float32) else dt
        assert stream.dtype == want and tuple(stream.shape) == (B, L, N)
        _close("stream", stream, s_ref, 1e-6, 1e-6)                                # (one fp32 addition)
    _close("dx", dx, dx_ref, 1e-4 + HALF_ULP[dt], 1e-5)
    _close("dweight", dw, dw_ref, 1e-4, scale_atol=1e-5)
    _close("dbias", db, db_ref, 1e-4, scale_atol=1e-5)
    if with_res:
        assert dr.dtype == torch.float32 and dr.shape == r0.shape
        _close("dresidual", dr, dr_ref, 1e-4, 1e-5)


def test_norm_limits():
    """rows wider than the 8 register pieces (2048 columns) are refused with an error from both entry points, before any launch; M = 0
    returns empty tensors of the right shapes and dtypes"""
    from dimsum_amd import native
    N = 2052
    x, w, b = torch.randn(8, N, device="cuda"), torch.ones(N, device="cuda"), torch.zeros(N, device="cuda")
    for is_rms in (False, True):
        with pytest.raises(RuntimeError):
            native.layer_norm_fwd(x, w, b, EPS, is_rms_norm=is_rms)
        with pytest.raises(RuntimeError):
            native.layer_norm_fwd(x, w, b, EPS, residual=x, is_rms_norm=is_rms)
        with pytest.raises(RuntimeError):
            native.layer_norm_bwd(x, x, w, b, EPS, None if is_rms else torch.zeros(8, device="cuda"), torch.ones(8, device="cuda"),
                                  dresidual=x, has_residual=True, is_rms_norm=is_rms)
    y, mean, rstd, ro = native.layer_norm_fwd(x[:, :2048].contiguous(), w[:2048], b[:2048], EPS)       # the widest row that is served
    assert torch.isfinite(y).all()
    for N in (384, 1150):
        for dt in (torch.float32, torch.bfloat16):
            x0, res0 = torch.empty(0, N, device="cuda", dtype=dt), torch.empty(0, N, device="cuda")
            w, b = torch.ones(N, device="cuda"), torch.zeros(N, device="cuda")
            for is_rms in (False, True):
                y, mean, rstd, ro = native.layer_norm_fwd(x0, w, b, EPS, residual=res0, is_rms_norm=is_rms)
                assert tuple(y.shape) == (0, N) and y.dtype == dt and tuple(ro.shape) == (0, N) and ro.dtype == torch.float32
                assert tuple(rstd.shape) == (0,) and rstd.dtype == torch.float32
                assert mean is None if is_rms else (tuple(mean.shape) == (0,) and mean.dtype == torch.float32)
                dx, dw, db, dres = native.layer_norm_bwd(x0, ro, w, b, EPS, mean, rstd, dresidual=res0, has_residual=True, is_rms_norm=is_rms,
                                                         x_dtype=dt)
                assert tuple(dx.shape) == (0, N) and dx.dtype == dt and tuple(dres.shape) == (0, N) and dres.dtype == torch.float32
                assert tuple(dw.shape) == (N,) and tuple(db.shape) == (N,) and dw.dtype == torch.float32
                assert not dw.any() and not db.any()


# ---------------------------------------------------------------------------------------------------------------------
# causal conv1d
# ---------------------------------------------------------------------------------------------------------------------
def _conv_check(tag, x, w, b, dout, silu, out=None, dx=None, relative=False):
    """forward + backward of GPU tensors in whatever layout they come, against the oracle on contiguous fp32 copies.
    fp32: the tolerances of test_conv_vs_golden; half precision: out and dx carry the half-ulp of their type on top (dweight / dbias are
    accumulated and returned in fp32 and keep the fp32 bound); relative: the absolute parts are taken relative to max|ref|."""
    from dimsum_amd import native
    from oracle import c_ops
    out_g = native.causal_conv1d_fwd(x, w, b, silu, out=out)
    dx_g, dw_g, db_g = native.causal_conv1d_bwd(x, w, b, dout, dx, silu)
    assert out_g.dtype == x.dtype and dx_g.dtype == x.dtype and out_g.shape == x.shape and dx_g.shape == x.shape
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
    _close(f"{tag} dweight", dw_g, rdw, 1e-4, scale_atol=1e-5)
    if b is not None:
        _close(f"{tag} dbias", db_g, rdb, 1e-4, scale_atol=1e-5)
    else:
        assert db_g is None
    return dict(out=out_g, dx=dx_g, dw=dw_g, db=db_g, ref_out=ref_out, ref_dx=rdx, ref_dw=rdw, ref_db=rdb)


def _conv_inputs(B, D, L, W, seed, dt=torch.float32, bias=True):
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    return rn(B, D, L).to(dt).cuda(), rn(D, W).cuda(), (rn(D).cuda() if bias else None), rn(B, D, L).to(dt).cuda()


@pytest.mark.parametrize("B,D,L,W", [(2, 64, 512, 4), (2, 33, 301, 3), (3, 7, 1030, 2)])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_conv_half_precision_fwd_bwd(dt, B, D, L, W):
    """bfloat16 / float16 x, dout -> out, dx (fp32 weights), vector path and element-wise multi-step path, against the oracle on the
    upcast inputs: out and dx are roundings of fp32 values (half-ulp + the fp32 tolerance), dweight / dbias keep the fp32 bound, which
    an accumulation of gradients rounded to the I/O type would miss. measured: worst error / bound out 0.99, dx 0.99 (the half-ulp is attained), dweight 0.01, dbias 0.01"""
    x, w, b, dout = _conv_inputs(B, D, L, W, seed=L + W, dt=dt)
    _conv_check(f"{dt}", x, w, b, dout, True)


@pytest.mark.parametrize("W", [2, 3, 4])
@pytest.mark.parametrize("L", [1, 2, 3, 5, 257, 260, 513])
def test_conv_length_edges(L, W):
    """rows shorter than the filter, one element past a 256-element step (the x halo loads and the gradient carry of the backward), the
    vector path at 260; SiLU without bias and bias without SiLU; B * D = 21 and 37: a ragged four-row tail across workgroups in the
    forward, waves without a batch row in the backward. measured: worst error / bound out 0.02, dx 0.09, dweight 0.13, dbias 0.01"""
    for B, D, silu, bias in ((3, 7, True, False), (1, 37, False, True), (37, 1, True, True)):
        x, w, b, dout = _conv_inputs(B, D, L, W, seed=B + L + W, bias=bias)
        _conv_check(f"B{B} D{D} silu={silu} bias={bias}", x, w, b, dout, silu)


def _d_major(t):
    """the same (B, D, L) values stored (D, B, L): Mamba's layout after rearrange(.., "d (b l) -> b d l")"""
    return t.permute(1, 0, 2).contiguous().permute(1, 0, 2)


def _nan_view(shape, kind):
    """a (B, D, L) view of a NaN-filled wider buffer and the mask of the elements outside it"""
    B, D, L = shape
    if kind == "channels":
        buf = torch.full((B, 2 * D, L), float("nan"), device="cuda")
        idx = (slice(None), slice(0, D), slice(None))
    else:                                                       # "shifted": the base pointer one element off
        buf = torch.full((B, D, L + 8), float("nan"), device="cuda")
        idx = (slice(None), slice(None), slice(1, 1 + L))
    outside = torch.ones_like(buf, dtype=torch.bool)
    outside[idx] = False
    return buf, buf[idx], outside


LAYOUTS = ["x_shifted", "out_d_major", "x_d_major", "dout_d_major", "weight_strided", "nan_channels", "nan_shifted"]


@pytest.mark.parametrize("silu,bias", [(True, False), (False, True)])
@pytest.mark.parametrize("L,W", [(260, 4), (512, 3), (301, 2)])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_conv_layouts(layout, L, W, silu, bias):
    """x one element off a 16-byte boundary (L % 4 == 0 lands on the element-wise path with its x[t0 - 1 .. t0 - 3] halo loads);
    out d-major from a batch-major x (selective_scan_interface's conv call) and the reverse; dout d-major against a batch-major x;
    weight as every second column of a wider tensor (weight_width_stride 2); out and dx as views of NaN-filled wider buffers, whose
    elements outside the view must stay NaN. measured: worst error / bound out 0.02, dx 0.11, dweight 0.01, dbias 0.01"""
    B, D = 3, 7
    x, w, b, dout = _conv_inputs(B, D, L, W, seed=L + W + len(layout), bias=bias)
    out = dx = None
    bufs = []
    if layout == "x_shifted":
        wide = torch.full((B, D, L + 8), float("nan"), device="cuda")
        wide[:, :, 1:1 + L] = x
        x = wide[:, :, 1:1 + L]
        assert x.data_ptr() % 16 == 4
    elif layout == "out_d_major":
        out = _d_major(torch.empty_like(x))
    elif layout == "x_d_major":
        x, out = _d_major(x), torch.empty(B, D, L, device="cuda")
        assert x.stride() == (L, B * L, 1) and out.stride() == (D * L, L, 1)
    elif layout == "dout_d_major":
        dout = _d_major(dout)
    elif layout == "weight_strided":
        w_wide = torch.full((D, 2 * W), float("nan"), device="cuda")
        w_wide[:, ::2] = w
        w = w_wide[:, ::2]
        assert w.stride() == (2 * W, 2)
    else:
        kind = layout[4:]
        (obuf, out, o_outside), (dbuf, dx, d_outside) = _nan_view((B, D, L), kind), _nan_view((B, D, L), kind)
        bufs = [(obuf, o_outside), (dbuf, d_outside)]
    _conv_check(layout, x, w, b, dout, silu, out=out, dx=dx)
    for buf, outside in bufs:
        assert torch.isnan(buf[outside]).all(), "the kernel wrote outside the view it was given"


@pytest.mark.parametrize("B,D,L", [(9, 2048, 64), (33, 8, 300)])
def test_conv_backward_work_split(B, D, L):
    """(9, 2048, 64): one split, the four waves of a workgroup own 3 / 2 / 2 / 2 batch rows; (33, 8, 300): split = 16, 64 wave slots
    for 33 rows, so waves without a row still take part in the reduction. Tolerances of test_conv_strided_views_like_mamba.
    measured: worst error / bound out 0.02, dx 0.14, dweight 0.01, dbias 0.01"""
    x, w, b, dout = _conv_inputs(B, D, L, 4, seed=B + D + L)
    _conv_check(f"split B{B} D{D}", x, w, b, dout, True)


def test_conv_saturated_silu():
    """x * 30: pre-activations of magnitude 20 .. 100 and beyond in both signs through sigmoidf_fast / silu_grad (exp overflows to inf on
    the negative side). Everything stays finite and within the fp32 tolerances taken relative to max|ref|.
    measured: worst error / bound out 0.01, dx 0.15, dweight 0.01, dbias 0.01"""
    from oracle import c_ops
    x, w, b, dout = _conv_inputs(2, 16, 300, 4, seed=30)
    x = x * 30
    pre = c_ops.causal_conv1d_fwd(_np(x), _np(w), _np(b), False)
    assert (pre > 20).sum() > 100 and (pre < -20).sum() > 100 and (pre > 100).any() and (pre < -100).any()
    got = _conv_check("saturated", x, w, b, dout, True, relative=True)
    for k in ("out", "dx", "dw", "db"):
        assert torch.isfinite(got[k]).all(), k


@pytest.mark.parametrize("strided", [False, True])
def test_causal_conv1d_fn_under_autograd(strided):
    """ops/causal_conv1d_interface.py: out and the gradients of x, weight, bias against torch.nn.functional.conv1d + SiLU in float64 on the
    CPU; x contiguous, or the first half of xz's channels (Mamba's xz.chunk(2, dim=1)) with an odd length.
    measured: worst error / bound out 0.02, dx 0.08, dweight 0.01, dbias 0.01"""
    from dimsum_amd.ops.causal_conv1d_interface import causal_conv1d_fn
    B, D, L, W = (2, 24, 301, 4) if strided else (2, 24, 256, 4)
    gen = torch.Generator().manual_seed(L)
    xz0, w0, b0, dout0 = (torch.randn(*s, generator=gen) for s in ((B, 2 * D if strided else D, L), (D, W), (D,), (B, D, L)))

    def run(to, fn):
        xz, w, b = (to(t).requires_grad_() for t in (xz0, w0, b0))
        out = fn(xz.chunk(2, dim=1)[0] if strided else xz, w, b)
        out.backward(to(dout0))
        return out, xz.grad, w.grad, b.grad

    ref_fn = lambda x, w, b: torch.nn.functional.silu(torch.nn.functional.conv1d(x, w.unsqueeze(1), b, padding=W - 1, groups=D)[..., :L])
    got = run(lambda t: t.cuda(), lambda x, w, b: causal_conv1d_fn(x, w, b, activation="silu"))
    ref = run(lambda t: t.double(), ref_fn)
    for name, a, r, tol in zip(("out", "dx", "dweight", "dbias"), got, ref,
                               (dict(rtol=1e-5, atol=2e-6, scale_atol=1e-6),) * 2 + (dict(rtol=1e-4, scale_atol=1e-5),) * 2):
        assert a.dtype == torch.float32
        _close(name, a, r, **tol)
