"""Block type "combined_einfft" on the HIP passes (csrc/einfft.hip).
Transform passes: against float64 torch.fft on the CPU, with the bound MEASURED per shape -- the max error of the CPU's own fp32 torch.fft
against float64 on the same input, times 4 (both are O(log N)-stage fp32 butterflies; the margin covers another radix and FMA contraction).
Adjointness: the two float64-accumulated inner products agree to 8 * 2^-24 |x|_2 |G|_2; the round trip to twice the transform bound. One-hot
input: every bin's magnitude is (4 N)^-1/2 to (3 log2 N + 4) * 2^-24 relative (per butterfly stage one twiddle of modulus 1 +- 1.5 * 2^-24
and one rounded complex product; the 4-point part and the scale add four roundings). MLP, operator, block, model: Y_TOL / G_TOL / SUM_TOL of
tests/test_blocks_linear_window_gpu.py. Gradients are discontinuous where a pre-ReLU value is 0 or a pre-shrink value has magnitude lambda:
the gradient tests first REQUIRE, in float64, that no element of their inputs lies closer to its kink than 2^-20 of its tensor's rms (a
condition on the chosen seeds, not a tolerance)."""
from collections import Counter

import numpy as np
import pytest
import torch

from conftest import assert_close, golden
from procedural import procedural_fill, seeded
from test_blocks_linear_window_gpu import G_TOL, SUM_TOL, Y_TOL, _AtenLog
from test_einfft_cpu import PARAMS, check_block_against_fixture, check_einfft_against_fixture
from test_model_cpu import _published
from test_train_gpu import KW, _fixed_transport

pytestmark = pytest.mark.gpu
T = torch.from_numpy
n = lambda t: t.detach().cpu().numpy()      # noqa: E731
LAM = 0.01
DFT_SHAPES = [(2, 16, 32), (1, 64, 192), (2, 256, 64), (1, 1024, 576), (3, 32, 96)]
KINK_MARGIN = 2.0 ** -20
OP_SEED = 200           # x = seeded(shape, 200), parameters from torch.Generator().manual_seed(1200): chosen on the CPU so that the float64
                        # reference keeps every element of (1, 16, 192) and (1, 16, 576) outside KINK_MARGIN (the smallest distances / rms
                        # found there: 1.3e-4 and 4.9e-5; 8.5e-5 and 5.5e-5)


@pytest.fixture(autouse=True)
def _fp32_matmul():
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.set_float32_matmul_precision("highest")


def _unit_params(C, seed):
    """weights randn * bs^-0.5, biases randn * 0.1: unit gain, about half of the ReLUs on, nearly everything outside the shrink zone"""
    bs, gen = C // 4, torch.Generator().manual_seed(seed)
    w = lambda: torch.randn(2, 4, bs, bs, generator=gen) * bs ** -0.5        # noqa: E731
    b = lambda: torch.randn(2, 4, bs, generator=gen) * 0.1                   # noqa: E731
    return w(), b(), w(), b()


def _module_params(C, seed):
    """the module's own regime: everything randn * 0.02 (about half of layer 2 inside the shrink zone)"""
    bs, gen = C // 4, torch.Generator().manual_seed(seed)
    return tuple(torch.randn(*s, generator=gen) * 0.02 for s in ((2, 4, bs, bs), (2, 4, bs), (2, 4, bs, bs), (2, 4, bs)))


_DFT_REF = {}


def _dft_ref(shape):
    """x, its float64 spectrum and the error of the CPU's fp32 torch.fft on it: computed once per shape, never modified"""
    if shape not in _DFT_REF:
        from dimsum_amd.ops.einfft import dft_torch
        x = T(seeded(shape, 161))
        ref = torch.stack(dft_torch(x.double()))
        cpu_err = (torch.stack(dft_torch(x)).double() - ref).abs().max().item()
        _DFT_REF[shape] = (x, ref, cpu_err)
    return _DFT_REF[shape]


@pytest.mark.parametrize("shape", DFT_SHAPES)
def test_dft_against_float64(shape):
    from dimsum_amd import native
    x, ref, cpu_err = _dft_ref(shape)
    B, N, C = shape
    wide = torch.empty(B, N, 2 * C, device="cuda")
    wide[..., C:] = x.cuda()
    wide[..., :C] = 7.0
    re, im = native.einfft_dft(wide[..., C:])
    re2, im2 = native.einfft_dft(x.cuda())
    assert torch.equal(re, re2) and torch.equal(im, im2)                       # the channel-half view is read in place, same arithmetic
    assert re.is_contiguous() and im.is_contiguous() and re.shape == x.shape
    err = (torch.stack((re, im)).cpu().double() - ref).abs().max().item()
    print(f"dft {shape}: max err {err:.3e}, CPU fp32 torch.fft {cpu_err:.3e}, ratio {err / cpu_err:.2f} (output rms {ref.pow(2).mean().sqrt() * 2 ** 0.5:.3f})")
    assert err <= 4 * cpu_err


@pytest.mark.parametrize("shape", DFT_SHAPES)
def test_idft_adjointness_and_round_trip(shape):
    from dimsum_amd import native
    from dimsum_amd.ops.einfft import idft_real_torch
    x, ref, cpu_err = _dft_ref(shape)
    B, N, C = shape
    gr, gi = T(seeded(shape, 162)), T(seeded(shape, 163))
    re, im = native.einfft_dft(x.cuda())
    wide = torch.full((B, N, 2 * C), 7.0, device="cuda")
    y = native.einfft_idft_real(gr.cuda(), gi.cuda(), out=wide[..., :C])        # a strided destination
    assert y.data_ptr() == wide.data_ptr() and bool((wide[..., C:] == 7.0).all())
    assert torch.equal(y, native.einfft_idft_real(gr.cuda(), gi.cuda()))
    yref = idft_real_torch(gr.double(), gi.double())
    cpu_err_inv = (idft_real_torch(gr, gi).double() - yref).abs().max().item()
    err = (y.cpu().double() - yref).abs().max().item()
    print(f"idft_real {shape}: max err {err:.3e}, CPU fp32 torch.fft {cpu_err_inv:.3e}, ratio {err / cpu_err_inv:.2f}")
    assert err <= 4 * cpu_err_inv
    lhs = (re.cpu().double() * gr.double()).sum() + (im.cpu().double() * gi.double()).sum()
    rhs = (x.double() * y.cpu().double()).sum()
    bound = 8 * 2.0 ** -24 * x.double().norm() * torch.sqrt(gr.double().norm() ** 2 + gi.double().norm() ** 2)
    print(f"adjointness {shape}: |<dft x, G> - <x, idft G>| / bound = {abs(lhs - rhs) / bound:.3f}")
    assert abs(lhs - rhs) <= bound
    back = native.einfft_idft_real(re, im)
    assert (back.cpu().double() - x.double()).abs().max().item() <= 2 * 4 * cpu_err


@pytest.mark.parametrize("N,C", [(16, 32), (32, 96), (1024, 64)])
def test_dc_and_one_hot_pins(N, C):
    from dimsum_amd import native
    bs = C // 4
    vals = T(seeded((2, 1, bs), 164)).repeat(1, 1, 4)                          # constant over tokens and over the 4 blocks, per column j
    re, im = native.einfft_dft(vals.expand(2, N, C).contiguous().cuda())
    want = np.sqrt(4.0 * N) * vals[:, 0, :bs].double().numpy()
    got = n(re)[:, 0, :bs].astype(np.float64)
    assert (np.abs(got - want) <= 2 * np.spacing(np.abs(want).astype(np.float32))).all()      # bin (0, 0): sqrt(4 N) x to 2 ulp
    rest = re.clone()
    rest[:, 0, :bs] = 0
    assert not rest.any() and not im.any()                                       # every other bin: exactly zero
    x = torch.zeros(1, N, C)
    x[0, N // 3, 2 * bs + 3] = 1.0                                               # one token, block 2, column 3
    re, im = native.einfft_dft(x.cuda())
    mag = torch.sqrt(re.double() ** 2 + im.double() ** 2).cpu().view(N, 4, bs)
    assert (mag[:, :, 3] - (4.0 * N) ** -0.5).abs().max().item() <= (3 * np.log2(N) + 4) * 2.0 ** -24 * (4.0 * N) ** -0.5
    mag[:, :, 3] = 0
    assert not mag.any()


@pytest.mark.parametrize("regime", ["unit", "module"])
@pytest.mark.parametrize("rows", [32, 67])
@pytest.mark.parametrize("bs", [8, 48, 144])
def test_mlp_forward_against_float64(bs, rows, regime):
    from dimsum_amd import native
    from dimsum_amd.ops.einfft import mlp_torch
    C = 4 * bs
    params = (_unit_params if regime == "unit" else _module_params)(C, 170 + bs)
    re, im = T(seeded((1, rows, C), 171)), T(seeded((1, rows, C), 172))
    if regime == "module":          # the spectrum of a unit-variance input: the DC row is sqrt(4 N) times the typical one
        re[:, 0] *= 8.0
    zr, zi = native.einfft_mlp_fwd(re.cuda(), im.cuda(), *(p.cuda() for p in params), LAM)
    rr, ri, _ = mlp_torch(re.double(), im.double(), *(p.double() for p in params), LAM)
    passed = ((rr != 0).double().mean().item() + (ri != 0).double().mean().item()) / 2
    print(f"mlp bs {bs} rows {rows} {regime}: shrink pass {passed:.3f}")
    assert 0.05 < passed <= 1.0
    assert_close(n(zr), rr.numpy(), what="zr", **Y_TOL)                         # continuous across both kinks: no element excluded
    assert_close(n(zi), ri.numpy(), what="zi", **Y_TOL)


def _kink_margins(x, w1, b1, w2, b2):
    """float64: the smallest distance of a pre-ReLU element to 0 and of a pre-shrink element's magnitude to lambda, over each tensor's rms"""
    from dimsum_amd.ops.einfft import _cmul_torch, dft_torch
    B, N, C = x.shape
    re, im = dft_torch(x)
    sh = (B, N, 4, C // 4)
    p = torch.stack(_cmul_torch(re.reshape(sh), im.reshape(sh), w1, b1))
    q = torch.stack(_cmul_torch(p[0].relu(), p[1].relu(), w2, b2))
    return (p.abs().min() / p.pow(2).mean().sqrt()).item(), ((q.abs() - LAM).abs().min() / q.pow(2).mean().sqrt()).item()


def test_operator_against_the_reference_fixture():
    from dimsum_amd.ops.einfft import einfft
    g = golden("einfft")
    m = _kink_margins(T(g["small_x"]).double(), *(T(g["small_" + k]).double() for k in PARAMS))
    assert min(m) >= KINK_MARGIN, m
    check_einfft_against_fixture(einfft, "small", "cuda", Y_TOL, G_TOL, SUM_TOL)


@pytest.mark.parametrize("shape", [(1, 16, 192), (1, 16, 576)])
def test_operator_forward_and_backward_against_float64(shape):
    from dimsum_amd.ops.einfft import einfft, einfft_torch
    B, N, C = shape
    x, dy, params = T(seeded(shape, OP_SEED)), T(seeded(shape, OP_SEED + 1)), _unit_params(C, OP_SEED + 1000)
    m = _kink_margins(x.double(), *(p.double() for p in params))
    print(f"operator {shape}: kink margins / rms {m[0]:.2e} (ReLU) {m[1]:.2e} (shrink)")
    assert min(m) >= KINK_MARGIN, m
    xr = x.double().requires_grad_()
    pr = [p.double().requires_grad_() for p in params]
    yr = einfft_torch(xr, *pr, LAM)
    yr.backward(dy.double())
    wide = torch.zeros(B, N, 2 * C, device="cuda")
    wide[..., C:] = x.cuda()
    wide.requires_grad_()
    pg = [p.cuda().requires_grad_() for p in params]
    y = einfft(wide[..., C:], *pg, LAM)
    y.backward(dy.cuda())
    assert_close(n(y), n(yr), what="y", **Y_TOL)
    assert_close(n(wide.grad[..., C:]), n(xr.grad), what="dx", **G_TOL)
    assert not wide.grad[..., :C].any()
    for k, a, b in zip(PARAMS, pg, pr):
        assert_close(n(a.grad), n(b.grad), what="g " + k, **SUM_TOL)


@pytest.mark.usefixtures("allow_torch_sdpa")        # (the fusion of a hidden-64 block has head_dim 4: conftest)
def test_block_against_the_reference_fixture():
    check_block_against_fixture("cuda", Y_TOL, G_TOL, SUM_TOL)


def _tiny():
    from dimsum_amd.models_dim import DiM
    m = DiM(depth=4, hidden_size=64, patch_size=2, **_published(block_type="combined_einfft"))
    procedural_fill(m, seed=3)
    return m.cuda().eval()


_SPECTRAL_OPS = ("fft", "einsum", "relu", "softshrink", "view_as_complex", "stack", "complex")


@pytest.mark.usefixtures("allow_torch_sdpa")        # (the shared DiTBlock of a hidden-64 model has head_dim 4: conftest)
def test_tiny_model_forward_all_hip():
    g = golden("model_tiny_einfft")
    m = _tiny()
    args = tuple(T(g[k]).cuda() for k in ("x", "t", "y"))
    with torch.no_grad():
        m(*args)                                    # (lazy tables)
        with _AtenLog() as log:
            out = m(*args)
    assert_close(out.cpu().numpy(), g["out"], 2e-4, 0, "out", scale_atol=2e-5)
    assert len(log.ops) > 0
    assert not [op for op in log.ops if any(s in op for s in ("fft", "softshrink", "view_as_complex", "complex"))], Counter(log.ops)
    # and nothing of the torch composition among the ops this block type adds to the "combined" forward's
    from dimsum_amd.models_dim import DiM
    base_m = DiM(depth=4, hidden_size=64, patch_size=2, **_published())
    procedural_fill(base_m, seed=3)
    base_m = base_m.cuda().eval()
    with torch.no_grad():
        base_m(*args)
        with _AtenLog() as base:
            base_m(*args)
    extra = Counter(log.ops) - Counter(base.ops)
    assert not [op for op in extra if any(s in op for s in _SPECTRAL_OPS)], extra
    x = args[0].clone().requires_grad_()
    out = m(x, *args[1:])
    out.backward(T(g["dout"]).cuda())
    assert_close(out.detach().cpu().numpy(), g["out"], 2e-4, 0, "out (grad mode)", scale_atol=2e-5)
    assert_close(x.grad.cpu().numpy(), g["dx"], 5e-4, 0, "dx", scale_atol=5e-5)


@pytest.mark.usefixtures("allow_torch_sdpa")
@pytest.mark.parametrize("fused_step", [False, True])
def test_two_training_steps(fused_step):
    from dimsum_amd.models_dim import DiM
    from dimsum_amd.train import build_training, train_step
    m = DiM(depth=4, hidden_size=64, patch_size=2, **dict(KW, block_type="combined_einfft"))
    procedural_fill(m, seed=3)
    model, ema, opt = build_training(m.cuda(), "cuda", lr=1e-3, fused_step=fused_step)
    start = {k: v.detach().clone() for k, v in model.named_parameters()}
    x, y = T(seeded((4, 4, 32, 32), 81)).cuda(), torch.tensor([1, 22, 333, 999], device="cuda")
    tr = _fixed_transport(T(seeded((4,), 82, kind="uniform")), T(seeded((4, 4, 32, 32), 83)))
    for _ in range(2):
        loss = train_step(model.train(), ema, opt, tr, x, y, max_grad_norm=2.0, ema_decay=0.5)
        assert torch.isfinite(loss).item()
    now = dict(model.named_parameters())
    moved = [k for k in start if ".freq_mamba.complex_" in k]
    assert len(moved) == 4 * 4
    for k in moved:
        assert not torch.equal(now[k], start[k]), k
    assert not torch.equal(now["x_embedder.proj.weight"], start["x_embedder.proj.weight"])


@pytest.mark.usefixtures("allow_torch_sdpa")
def test_hip_graph_replay_and_two_streams_are_bit_identical():
    from dimsum_amd.hip_graph import GraphedForward
    from dimsum_amd.models_dim import branch_streams
    m = _tiny()
    graphed = GraphedForward(m)
    gen = torch.Generator(device="cuda").manual_seed(0)
    for _ in range(2):
        x, t = torch.randn(4, 4, 32, 32, device="cuda", generator=gen), torch.rand(4, device="cuda", generator=gen)
        y = torch.randint(0, 1000, (4,), device="cuda", generator=gen)
        with torch.no_grad():
            with branch_streams(False):
                ref = m(x, t, y)
            with branch_streams(True):
                two = m(x, t, y)
        assert any("_side_stream" in blk.__dict__ for blk in m.blocks)
        assert torch.equal(two, ref)
        assert torch.equal(graphed(x, t, y), ref)
    assert len(graphed.graphs) == 1


def test_wrappers_refuse_before_any_launch():
    from dimsum_amd import native
    z = lambda *s, dt=torch.float32: torch.zeros(*s, device="cuda", dtype=dt)        # noqa: E731
    for N in (48, 2048):
        with pytest.raises(RuntimeError, match="power of two"):
            native.einfft_dft(z(1, N, 32))
        with pytest.raises(RuntimeError, match="power of two"):
            native.einfft_idft_real(z(1, N, 32), z(1, N, 32))
    with pytest.raises(RuntimeError, match="multiple of 32"):
        native.einfft_dft(z(1, 16, 40))
    with pytest.raises(RuntimeError, match="multiple of 32"):
        native.einfft_mlp_fwd(z(1, 16, 40), z(1, 16, 40), z(2, 4, 10, 10), z(2, 4, 10), z(2, 4, 10, 10), z(2, 4, 10), LAM)
    with pytest.raises(RuntimeError, match="float32"):
        native.einfft_dft(z(1, 16, 32, dt=torch.float16))
    with pytest.raises(RuntimeError, match="float32"):
        native.einfft_mlp_fwd(z(1, 16, 32, dt=torch.float16), z(1, 16, 32), z(2, 4, 8, 8), z(2, 4, 8), z(2, 4, 8, 8), z(2, 4, 8), LAM)
