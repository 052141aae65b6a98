"""The plain MLP's HIP path (csrc/act_rows.hip, DIMSUM_GEMM_EPI_GELU_F16, dimsum_amd.mlp.Mlp) and the DiT family on it (models_dit.py).

Row pass: against float64 F.gelu(approximate="tanh") (and its float64 autograd) on the CPU, with the bound MEASURED per case -- the max error
of the CPU's own fp32 evaluation against float64 on the same input, times 4 (the margin covers tanhf / expf implementation differences and
FMA contraction), the convention of tests/test_einfft_gpu.py. d bias: against the float64 column sum of the kernel's OWN dx (dx has its bound
above; this one is the accumulation's) to rows * 2^-23 * max|dx|, whatever H. Scaled-fp16 images: decoded, equal to the fp32 output to one fp16
ulp of the row maximum, the scales being that maximum's exact power of two.

GEMM epilogue: against the F32_BIAS GEMM followed by the row pass writing the "f16s" image with the SAME bound-derived row scale (the row pass's
`scales` argument: the epilogue cannot know a row's maximum, it spans column tiles): equal scales, images within one fp16 ulp elementwise.

Mlp / DiT: against the plain-torch composition in fp32-highest on the same device with Y_TOL / G_TOL / SUM_TOL of
tests/test_blocks_linear_window_gpu.py; the f16s inference policy against the exact-fp32 output of the same model with the as-run DiM bound
1e-3 |ref| + 5e-4 max|ref| (tests/test_model_gpu.py). The DiT tests run 16 latents of 8 x 8 (256 token rows: one 256-row GEMM panel).

Observed on an MI355X (error / bound): row pass forward (1, 4) 1.3e-7 / 5.0e-7 and 1.8e-7 / 7.2e-7 (without / with bias), (3, 36) 2.0e-7 / 7.5e-7
and 2.5e-7 / 7.2e-7, (65, 1028) 4.8e-7 / 1.6e-6 and 6.7e-7 / 2.3e-6, (256, 4096) 5.2e-7 / 1.7e-6 and 7.0e-7 / 2.6e-6; backward dx (1, 4) 7.4e-8 / 2.9e-7
and 1.1e-7 / 3.2e-7, (3, 36) 5.1e-7 / 1.0e-6 and 4.0e-7 / 8.6e-7, (65, 1028) 3.3e-6 / 7.2e-6 and 4.5e-6 / 5.4e-6, (256, 4096) 4.1e-6 / 1.3e-5 and
4.4e-6 / 1.2e-5; d bias 0 / 1.8e-7, 2.0e-7 / 8.0e-7, 7.2e-6 / 3.1e-5, 9.5e-6 / 1.6e-4; scaled-fp16 images at most 0.500 ulp of the row maximum;
the epilogue's images bit-identical to GEMM + row pass at both shapes (0 elements differ)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close
from procedural import procedural_fill, seeded
from test_blocks_linear_window_gpu import G_TOL, SUM_TOL, Y_TOL, _AtenLog
from test_model_gpu import f16s_policy  # noqa: F401  (fixture)
from test_train_gpu import _fixed_transport

pytestmark = pytest.mark.gpu
T = torch.from_numpy
n = lambda t: t.detach().cpu().numpy()      # noqa: E731
ROW_SHAPES = [(1, 4), (3, 36), (65, 1028), (256, 4096)]
EPI_SHAPES = [(256, 128, 256), (512, 192, 1024)]


@pytest.fixture(autouse=True)
def _fp32_matmul():
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.set_float32_matmul_precision("highest")


_ROW_REF = {}


def _row_ref(shape, with_bias):
    """x, bias, dh, the float64 h / dx and the errors of the CPU's fp32 evaluation of both: once per case, never modified"""
    key = (shape, with_bias)
    if key not in _ROW_REF:
        rows, H = shape
        x, dh = T(seeded(shape, 301, scale=1.5)), T(seeded(shape, 303))
        bias = T(seeded((H,), 302, scale=0.5)) if with_bias else None

        def run(dt):
            a = (x.to(dt) if bias is None else x.to(dt) + bias.to(dt)).requires_grad_()
            h = F.gelu(a, approximate="tanh")
            h.backward(dh.to(dt))
            return h.detach(), a.grad
        h64, dx64 = run(torch.float64)
        h32, dx32 = run(torch.float32)
        _ROW_REF[key] = (x, bias, dh, h64, dx64, (h32.double() - h64).abs().max().item(), (dx32.double() - dx64).abs().max().item())
    return _ROW_REF[key]


def _cu(t):
    return None if t is None else t.cuda()


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("shape", ROW_SHAPES)
def test_row_pass_forward_against_float64(shape, with_bias):
    from dimsum_amd import native
    x, bias, _, h64, _, cpu_err, _ = _row_ref(shape, with_bias)
    h = native.gelu_fwd(x.cuda(), _cu(bias))
    assert h.shape == x.shape and h.dtype == torch.float32
    err = (h.cpu().double() - h64).abs().max().item()
    print(f"gelu_fwd {shape} bias={with_bias}: err {err:.3e}, cpu fp32 err {cpu_err:.3e}, bound {4 * cpu_err:.3e}")
    assert err <= 4 * cpu_err


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("shape", ROW_SHAPES)
def test_row_pass_backward_against_float64(shape, with_bias):
    from dimsum_amd import native
    x, bias, dh, _, dx64, _, cpu_err = _row_ref(shape, with_bias)
    dx, db = native.gelu_bwd(x.cuda(), _cu(bias), dh.cuda())
    err = (dx.cpu().double() - dx64).abs().max().item()
    print(f"gelu_bwd {shape} bias={with_bias}: dx err {err:.3e}, cpu fp32 err {cpu_err:.3e}, bound {4 * cpu_err:.3e}")
    assert err <= 4 * cpu_err
    assert (db is None) == (bias is None)
    if db is not None:
        want = dx.cpu().double().sum(0)
        berr, bound = (db.cpu().double() - want).abs().max().item(), shape[0] * 2.0 ** -23 * dx.abs().max().item()
        print(f"    dbias err {berr:.3e}, bound {bound:.3e}")
        assert db.shape == (shape[1],) and berr <= bound
        assert native.gelu_bwd(x.cuda(), bias.cuda(), dh.cuda(), need_dbias=False)[1] is None


def _pow2_floor_exp(v):
    """floor(log2 |v|), exactly (frexp: |v| = m 2^e with m in [0.5, 1))"""
    return torch.frexp(v.abs())[1].to(torch.float32) - 1


def _ulp16(v):
    """one fp16 ulp at magnitude |v|: 2^(floor(log2 |v|) - 10), the subnormal spacing 2^-24 below 2^-14"""
    return torch.exp2(_pow2_floor_exp(v.abs().clamp_min(2.0 ** -14)) - 10)


@pytest.mark.parametrize("shape", ROW_SHAPES)
def test_row_pass_images_decode_to_the_fp32_output(shape):
    from dimsum_amd import native
    x, bias, dh, *_ = _row_ref(shape, True)
    x, bias, dh = x.cuda(), bias.cuda(), dh.cuda()
    rows, H = shape
    for name, ref, img, img3, pair in (("fwd", native.gelu_fwd(x, bias), native.gelu_fwd(x, bias, split3="f16s"), native.gelu_fwd(x, bias, split3=True),
                                        native.gelu_fwd(x, bias, split3="pair")),
                                       ("bwd", native.gelu_bwd(x, bias, dh)[0], native.gelu_bwd(x, bias, dh, split3="f16s")[0],
                                        native.gelu_bwd(x, bias, dh, split3=True)[0], native.gelu_bwd(x, bias, dh, split3="pair")[0])):
        rmax = ref.abs().amax(1)
        assert img.data.dtype == torch.float16 and img.data.shape == shape and img.inv.shape == (rows,)
        # the scale is the row maximum's exact power of two: max * 2^s in [2^14, 2^15)
        assert torch.equal(img.inv, torch.exp2(_pow2_floor_exp(rmax) - 14)), name
        err = (img.float() - ref).abs().amax(1)
        print(f"{name} f16s image {shape}: max err / ulp(row max) {(err / _ulp16(rmax)).max().item():.3f}")
        assert (err <= _ulp16(rmax)).all(), name
        # the split-bf16 images: hi + lo = the fp32 value to 2^-16 relative; forward in left order [hi | hi | lo], backward in weight order [hi | lo | hi]
        p3 = img3.float()
        hi, lo = p3[:, :H], (p3[:, 2 * H:] if name == "fwd" else p3[:, H:2 * H])
        assert torch.equal(hi, p3[:, H:2 * H] if name == "fwd" else p3[:, 2 * H:])
        assert ((hi + lo - ref).abs() <= 2.0 ** -16 * ref.abs()).all(), name
        assert torch.equal(pair.data.float(), torch.cat([hi, lo], 1)), name
    # the backward's d bias rides with every image form
    want = native.gelu_bwd(x, bias, dh)[1]
    for mode in (True, "pair", "f16s"):
        assert_close(n(native.gelu_bwd(x, bias, dh, split3=mode)[1]), n(want), 0, 0, f"dbias ({mode})", scale_atol=shape[0] * 2.0 ** -23)


@pytest.mark.parametrize("shape", [(9, 2052), (130, 2052), (9, 4100), (130, 4100)])
def test_row_pass_f16s_images_against_float64(shape):
    """The three- and five-strip instantiations of the scaled-fp16 row pass (H in (2048, 3072] and (4096, 5120]; ROW_SHAPES stops at one, two and
    four strips), forward and backward, decoded against the float64 expression: one fp16 ulp of the row maximum (the image tolerance of
    test_row_pass_images_decode_to_the_fp32_output) plus the fp32 pass's own bound, 4 x the CPU's fp32 error (the tests above). 9 rows = one full
    workgroup of 8 rows and a ragged one, 130 = 17 workgroups. d bias against the float64 column sum: every one of the `rows` summands carries the
    dx bound, and the fp32 accumulation rows * 2^-23 * max|dx| as above."""
    from dimsum_amd import native
    x, bias, dh, h64, dx64, ferr, berr = _row_ref(shape, True)
    rows, H = shape
    img = native.gelu_fwd(x.cuda(), bias.cuda(), split3="f16s")
    dimg, db = native.gelu_bwd(x.cuda(), bias.cuda(), dh.cuda(), split3="f16s")
    for name, im, ref, cpu_err in (("fwd", img, h64, ferr), ("bwd", dimg, dx64, berr)):
        assert im.data.dtype == torch.float16 and im.data.shape == shape and im.inv.shape == (rows,)
        top = im.data.float().abs().amax(1)
        assert torch.all(torch.frexp(im.inv)[0] == 0.5) and torch.all(top >= 2.0 ** 14) and torch.all(top < 2.0 ** 15), name
        rmax = ref.abs().amax(1)
        err = (im.float().cpu().double() - ref).abs().amax(1)
        bound = _ulp16(rmax.float()).double() + 4 * cpu_err
        print(f"{name} f16s image {shape} vs float64: max err / bound {(err / bound).max().item():.3f}")
        assert (err <= bound).all(), name
    berr_got = (db.cpu().double() - dx64.sum(0)).abs().max().item()
    bbound = rows * (2.0 ** -23 * dx64.abs().max().item() + 4 * berr)
    print(f"    dbias err {berr_got:.3e}, bound {bbound:.3e}")
    assert db.shape == (H,) and berr_got <= bbound


def _epi_case(M, K, N):
    from dimsum_amd import gemm, native
    x16 = native.rows_f16s(T(seeded((M, K), 311, scale=2.0)).cuda())
    w = T(seeded((N, K), 312, scale=K ** -0.5)).cuda()
    b = T(seeded((N,), 313, scale=0.3)).cuda()
    w16, l1 = native.rows_f16s(w, want_l1=True)
    bound = torch.cat([l1 * gemm._K10, b.abs().max().reshape(1)]).contiguous()
    return x16, w16, b, bound


@pytest.mark.parametrize("M,K,N", EPI_SHAPES)
def test_gelu_epilogue_equals_gemm_plus_row_pass(M, K, N):
    from dimsum_amd import native
    x16, w16, b, bound = _epi_case(M, K, N)
    with native.gemm_kernel_log() as log:
        fused = native.gemm_nt(x16.data, w16.data, bias=b, epilogue="gelu_f16", scales=(x16.inv, w16.inv), gate_bound=bound)
    assert log == [("gelu_f16", 0)]                                   # the 256-row tiles
    x1 = native.gemm_nt(x16.data, w16.data, bias=b, scales=(x16.inv, w16.inv))                 # DIMSUM_GEMM_EPI_F32_BIAS
    ref = native.gelu_fwd(x1, None, split3="f16s", scales=(x16.inv, bound))
    assert fused.data.shape == (M, N) and fused.data.dtype == torch.float16
    assert torch.equal(fused.inv, ref.inv)
    a, r = fused.data.float(), ref.data.float()
    d = (a - r).abs()
    print(f"gelu_f16 epilogue {(M, K, N)}: {int((d > 0).sum())} of {d.numel()} elements differ, max {(d / torch.maximum(_ulp16(a), _ulp16(r))).max().item():.2f} ulp")
    assert (d <= torch.maximum(_ulp16(a), _ulp16(r))).all()
    # and the image means what it says: decoded, gelu(x W^T + b) in float64 to the fp16 rounding under the bound-derived scale (scaled values
    # stay below 2^15: half an ulp there is 8 inv) plus the fp32 accumulation and activation (1e-5 of the largest value)
    want = F.gelu((x16.float().double() @ w16.float().double().t() + b.double()), approximate="tanh")
    assert ((fused.float().double() - want).abs() <= 8 * fused.inv.double()[:, None] + 1e-5 * want.abs().max()).all()
    assert (fused.data.float().abs() < 2.0 ** 15).all()
    # the 128-row tiles (tune_variant 512): the same scales, the same values to one ulp
    with native.gemm_kernel_log() as log:
        m128 = native.gemm_nt(x16.data, w16.data, bias=b, epilogue="gelu_f16", scales=(x16.inv, w16.inv), gate_bound=bound, tune=(512, 0))
    assert log == [("gelu_f16", 1)] and torch.equal(m128.inv, fused.inv)
    assert ((m128.data.float() - a).abs() <= torch.maximum(_ulp16(a), _ulp16(m128.data.float()))).all()


def test_gelu_epilogue_refuses_bf16_and_the_mlp_falls_back(monkeypatch):
    from dimsum_amd import native
    from dimsum_amd.mlp import Mlp
    M, K = 256, 128
    x = T(seeded((M, K), 321)).cuda()
    x3, w3 = native.split3_rows(x, left=True), native.split3_rows(T(seeded((256, K), 322, scale=K ** -0.5)).cuda(), left=False)
    ones = torch.ones(256, device="cuda")
    with pytest.raises(RuntimeError, match=r"status 5"):               # DIMSUM_ERR_UNSUPPORTED
        native.gemm_nt(x3, w3, epilogue="gelu_f16", scales=(ones[:M], ones), gate_bound=torch.ones(2, device="cuda"))
    mlp = procedural_fill(Mlp(K, 4 * K, act_layer=lambda: torch.nn.GELU(approximate="tanh")), seed=5).cuda()
    calls = []
    real = native.gelu_fwd
    monkeypatch.setattr(native, "gelu_fwd", lambda *a, **k: calls.append(k.get("split3")) or real(*a, **k))
    with torch.no_grad():
        y, yb = mlp.forward_deferred(x.view(1, M, K), x3=x3)
        want = F.linear(F.gelu(F.linear(x, mlp.fc1.weight, mlp.fc1.bias), approximate="tanh"), mlp.fc2.weight)
    assert len(calls) == 1 and calls[0] in (True, "pair") and yb is mlp.fc2.bias
    assert_close(n(y.view(M, K)), n(want), what="Mlp on split-bf16 images (GEMM + row pass)", **Y_TOL)


@pytest.mark.parametrize("hidden", [64, 96])
def test_mlp_forward_and_gradients_vs_torch(hidden):
    from dimsum_amd.mlp import Mlp
    mlp = procedural_fill(Mlp(hidden, 4 * hidden, act_layer=lambda: torch.nn.GELU(approximate="tanh")), seed=6).cuda()
    x = T(seeded((2, 32, hidden), 331)).cuda().requires_grad_()
    w = T(seeded((2, 32, hidden), 332)).cuda()
    names = ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"]
    params = [dict(mlp.named_parameters())[k] for k in names]

    def grads(fn):
        y = fn(x)
        return y, torch.autograd.grad((y * w).sum(), [x] + params)
    y, g = grads(mlp)
    y_ref, g_ref = grads(lambda v: F.linear(F.gelu(F.linear(v, mlp.fc1.weight, mlp.fc1.bias), approximate="tanh"), mlp.fc2.weight, mlp.fc2.bias))
    assert_close(n(y), n(y_ref), what="y", **Y_TOL)
    for k, a, b in zip(["x"] + names, g, g_ref):
        assert_close(n(a), n(b), what="d " + k, **G_TOL)


# ---- the model --------------------------------------------------------------------------------------------------------------------------
def _dit():
    from dimsum_amd.models_dit import DiT
    m = DiT(input_size=8, patch_size=2, hidden_size=128, depth=2, num_heads=2, num_classes=10, class_dropout_prob=0.1)
    return procedural_fill(m, seed=7).cuda().eval()


def _dit_inputs(B=16):
    return T(seeded((B, 4, 8, 8), 341)).cuda(), T(seeded((B,), 342, kind="uniform")).cuda(), (torch.arange(B, device="cuda") * 3) % 10


def _torch_dit(m, x, t, y):
    """models_dit.py:252-272 with torch ops only: LayerNorm, modulate, SDPA, the plain MLP"""
    H = m.pos_embed.shape[-1]
    mod = lambda v, shift, scale: F.layer_norm(v, (H,), eps=1e-6) * (1 + scale[:, None]) + shift[:, None]      # noqa: E731
    c = m.t_embedder(t) + m.y_embedder(y, False)
    h = F.conv2d(x, m.x_embedder.proj.weight, m.x_embedder.proj.bias, stride=m.patch_size).flatten(2).transpose(1, 2) + m.pos_embed
    for b in m.blocks:
        sa, ca, ga, sm, cm, gm = b.adaLN_modulation(c).chunk(6, dim=1)
        B, N, C = h.shape
        qkv = F.linear(mod(h, sa, ca), b.attn.qkv.weight, b.attn.qkv.bias).reshape(B, N, 3, b.attn.num_heads, C // b.attn.num_heads).permute(2, 0, 3, 1, 4)
        with torch.nn.attention.sdpa_kernel(torch.nn.attention.SDPBackend.MATH):
            o = F.scaled_dot_product_attention(*qkv.unbind(0)).transpose(1, 2).reshape(B, N, C)
        h = h + ga[:, None] * F.linear(o, b.attn.proj.weight, b.attn.proj.bias)
        u = F.gelu(F.linear(mod(h, sm, cm), b.mlp.fc1.weight, b.mlp.fc1.bias), approximate="tanh")
        h = h + gm[:, None] * F.linear(u, b.mlp.fc2.weight, b.mlp.fc2.bias)
    shift, scale = m.final_layer.adaLN_modulation(c).chunk(2, dim=1)
    return m.unpatchify(m.final_layer.linear(mod(h, shift, scale)))


_DIT_REF = {}


def _dit_exact():
    """the model, its inputs and its exact-fp32 inference output on the HIP path: once, never modified"""
    if not _DIT_REF:
        m, args = _dit(), _dit_inputs()
        with torch.no_grad():
            _DIT_REF["v"] = (m, args, m(*args))
    return _DIT_REF["v"]


def test_dit_forward_and_backward_vs_torch_composition():
    from dimsum_amd import utils
    m, (x, t, y), y_inf = _dit_exact()
    before = utils.torch_path_counts()
    xg = x.clone().requires_grad_()
    w = T(seeded(tuple(y_inf.shape), 343)).cuda()
    params = {k: p for k, p in m.named_parameters() if p.requires_grad}
    out = m(xg, t, y)
    g = torch.autograd.grad((out * w).sum(), [xg] + list(params.values()))
    ref = _torch_dit(m, xg, t, y)
    g_ref = torch.autograd.grad((ref * w).sum(), [xg] + list(params.values()))
    assert utils.torch_path_counts() == before                         # head_dim 64: the MFMA attention kernels
    assert_close(n(y_inf), n(ref), what="y (inference)", **Y_TOL)
    assert_close(n(out), n(ref), what="y (autograd)", **Y_TOL)
    assert_close(n(g[0]), n(g_ref[0]), what="dx", **G_TOL)
    for k, a, b in zip(params, g[1:], g_ref[1:]):
        assert_close(n(a), n(b), what="d " + k, **SUM_TOL)


def test_dit_under_the_f16s_policy(f16s_policy, monkeypatch):  # noqa: F811
    """the single-product inference policy: fc1 with the GELU epilogue, fc2 on the image it wrote; no gelu / tanh / addmm aten op inside the MLPs"""
    from dimsum_amd import native
    m, args, ref = _dit_exact()
    epis, log = [], _AtenLog()
    real = native.gemm_nt
    monkeypatch.setattr(native, "gemm_nt", lambda a, b, **kw: epis.append(kw.get("epilogue", "f32")) or real(a, b, **kw))
    for blk in m.blocks:
        def logged(*a, _f=blk.mlp.forward_deferred, **k):
            with log:
                return _f(*a, **k)
        monkeypatch.setattr(blk.mlp, "forward_deferred", logged)
    with torch.no_grad():
        got = m(*args)
    assert epis.count("gelu_f16") == len(m.blocks), epis
    bad = [op for op in log.ops if any(s in op for s in ("gelu", "tanh", "addmm"))]
    assert log.ops and not bad, bad
    assert not torch.equal(got, ref)
    assert_close(n(got), n(ref), 1e-3, 0, "y (f16s policy)", scale_atol=5e-4)


def test_dit_one_train_step():
    from dimsum_amd.train import build_training, train_step
    model, ema, opt = build_training(_dit(), "cuda", lr=1e-4)
    x, _, y = _dit_inputs()
    tr = _fixed_transport(T(seeded((16,), 351, kind="uniform")), T(seeded((16, 4, 8, 8), 352)))
    loss = train_step(model.train(), ema, opt, tr, x, y, max_grad_norm=2.0)
    assert math.isfinite(loss.item())
    missing = [k for k, p in model.named_parameters() if p.requires_grad and (p.grad is None or not torch.isfinite(p.grad).all())]
    assert not missing, missing
    assert [k for k, p in model.named_parameters() if not p.requires_grad] == ["pos_embed"]
