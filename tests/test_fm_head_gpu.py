"""The fused head on the GPU: dimsum_fm_plan against the reference's fixture (tests/golden/transport_blur.npz) and against the matrix-form
torch expression evaluated in float64 on the CPU; the loss kernels against the torch expression in float64; training_losses end to end with
blurring and with fused_head, forward and backward. Shapes are the smallest at which the kernels can go wrong: one lane, a partial wave,
several workgroups, a batch-strided x1, tails that are no multiple of 4, rows that start at unaligned addresses.
Tolerances are the transport's own (tests/test_transport_golden.py): rtol 2e-5 + 2e-6 max|ref| for tensors, rtol 1e-4 + 1e-5 max|ref| for
the reduced losses (an fp32 sum of 4096 squares carries ~64 ulp = 4e-6 in the worst case, a pairwise one far less)."""
import math

import pytest
import torch

from conftest import assert_close, golden
from procedural import seeded, toy_denoiser
from test_fm_head_cpu import LOSS_TOL, TOL, blur_case, check_blur_losses

from dimsum_amd.transport import create_transport
from dimsum_amd.transport.blurring import blur_times, dct_blur, dct_blur_torch

pytestmark = pytest.mark.gpu
EPS = dict(train_eps=1e-3, sample_eps=2e-3)


def _coef(B, sigmas, seed):
    """(5, B) table: arbitrary alpha, sigma, d_alpha, d_sigma (the kernel knows nothing of the path) and blur_t = blur_sigma^2 / 2"""
    c = torch.from_numpy(seeded((5, B), seed))
    c[4] = sigmas ** 2 / 2
    return c


def _plan_ref(x1, x0, coef, p):
    """float64 on the CPU: xt from the blurred x1, ut from the unblurred one"""
    x1, x0, coef = x1.double(), x0.double(), coef.double()
    k = [coef[i].view(-1, 1, 1, 1) for i in range(4)]
    xb = dct_blur_torch(x1, p, coef[4]) if p else x1
    return k[0] * xb + k[1] * x0, k[2] * x1 + k[3] * x0


@pytest.mark.parametrize("shape,p", [((5, 3, 8, 8), 4), ((1, 1, 8, 8), 8), ((3, 2, 8, 8), 8), ((3, 2, 8, 8), 2), ((2, 4, 32, 32), 4),
                                     ((3, 4, 32, 32), 4), ((3, 2, 16, 16), 8)])
def test_fm_plan_blur_matches_cpu_expression(shape, p):
    from dimsum_amd import native
    B = shape[0]
    x1, x0 = torch.from_numpy(seeded(shape, 31)), torch.from_numpy(seeded(shape, 32))
    sigmas = torch.linspace(0, 3, B) if B > 1 else torch.tensor([1.7])
    coef = _coef(B, sigmas, 33)
    xt, ut = native.fm_plan(x1.cuda(), x0.cuda(), coef.cuda(), p)
    want_xt, want_ut = _plan_ref(x1, x0, coef, p)
    assert_close(xt.cpu(), want_xt, what="xt", **TOL)
    assert_close(ut.cpu(), want_ut, what="ut", **TOL)
    assert torch.equal(ut, (coef[2].view(-1, 1, 1, 1) * x1 + coef[3].view(-1, 1, 1, 1) * x0).cuda())     # the unblurred x1, product by product


def test_dct_blur_on_gpu_matches_every_reference_fixture():
    g = golden("transport_blur")
    for tag in g["blur_cases"]:
        x, p, sigmas, want = blur_case(g, tag)
        assert_close(dct_blur(x.cuda(), p, sigmas.cuda()).cpu(), want, what=f"dct_blur {tag}", **TOL)
        assert_close(dct_blur(x.cuda(), p, torch.zeros(x.shape[0])).cpu(), x.numpy(), what=f"dct_blur {tag}, no blur", **TOL)


@pytest.mark.parametrize("p", [0, 2, 4, 8])
def test_fm_plan_reads_a_batch_strided_x1_in_place(p):
    from dimsum_amd import native
    big = torch.from_numpy(seeded((7, 3, 16, 16), 41)).cuda()
    x1 = big[1::2]                                                           # 3 samples, batch stride twice the sample
    assert not x1.is_contiguous() and x1.stride(0) == 2 * 3 * 16 * 16
    x0 = torch.from_numpy(seeded((3, 3, 16, 16), 42))
    coef = _coef(3, torch.tensor([0.0, 1.1, 3.0]), 43)
    before = big.clone()
    xt, ut = native.fm_plan(x1, x0.cuda(), coef.cuda(), p)
    want_xt, want_ut = _plan_ref(x1.cpu(), x0, coef, p)
    assert_close(xt.cpu(), want_xt, what="xt", **TOL)
    assert_close(ut.cpu(), want_ut, what="ut", **TOL)
    assert torch.equal(big, before)


@pytest.mark.parametrize("shape", [(5, 3, 8, 8), (3, 3, 5, 5), (2, 1, 1, 1), (2, 4, 32, 32)])
def test_fm_plan_without_blur_is_the_plain_expression_bitwise(shape):
    """every product is rounded before the sum, like the expression evaluated as separate passes; 75 elements per sample: rows that start at
    unaligned addresses and a tail of 3"""
    from dimsum_amd import native
    B = shape[0]
    x1, x0, coef = torch.from_numpy(seeded(shape, 51)).cuda(), torch.from_numpy(seeded(shape, 52)).cuda(), _coef(B, torch.zeros(B), 53).cuda()
    xt, ut = native.fm_plan(x1, x0, coef, 0)
    k = [coef[i].view(-1, 1, 1, 1) for i in range(4)]
    assert torch.equal(xt, k[0] * x1 + k[1] * x0) and torch.equal(ut, k[2] * x1 + k[3] * x0)
    want_xt, want_ut = _plan_ref(x1.cpu(), x0.cpu(), coef.cpu(), 0)
    assert_close(xt.cpu(), want_xt, what="xt", **TOL)
    assert_close(ut.cpu(), want_ut, what="ut", **TOL)


def test_unsupported_patch_size_raises_on_cuda():
    x = torch.zeros(2, 3, 16, 16, device="cuda")
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        dct_blur(x, 16, torch.zeros(2))
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        dct_blur(x.double(), 4, torch.zeros(2))
    tr = create_transport("GVP", "velocity", path_args=dict(use_blurring=True, blur_upscale=16))
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        tr.training_losses(toy_denoiser, x)
    with pytest.raises(ValueError):
        dct_blur(torch.zeros(2, 3, 8, 12, device="cuda"), 4, torch.zeros(2))
    assert_close(dct_blur(x.cpu(), 16, torch.zeros(2)), x.cpu().numpy(), what="the CPU expression has no such limit", **TOL)


# ---- the loss kernels --------------------------------------------------------------------------------------------------------------------
PARAMETRISATIONS = ("velocity", "noise", "score")


@pytest.mark.parametrize("n", [48, 75, 192, 4096])
@pytest.mark.parametrize("kind", PARAMETRISATIONS)
def test_loss_kernels_match_float64_expression(n, kind):
    from dimsum_amd import native
    B = 3
    out, tgt = torch.from_numpy(seeded((B, n), 61)), torch.from_numpy(seeded((B, n), 62))
    w = None if kind == "velocity" else torch.tensor([0.3, 2.5, 11.0])
    c = torch.tensor([0.9, 0.05, 0.4]) if kind == "score" else None
    sign = 1 if kind == "score" else -1
    gloss = torch.tensor([1.0 / B, -0.7, 2.0])                               # an upstream gradient that differs per sample
    o64 = out.double().requires_grad_(True)
    d = (o64 if c is None else c.double().view(B, 1) * o64) + sign * tgt.double()
    want = (1.0 if w is None else w.double()) * (d ** 2).mean(1)
    want.backward(gloss.double())
    dev = lambda v: None if v is None else v.cuda()  # noqa: E731
    loss = native.fm_loss_fwd(out.cuda(), tgt.cuda(), dev(w), dev(c), sign)
    again = native.fm_loss_fwd(out.cuda(), tgt.cuda(), dev(w), dev(c), sign)
    assert torch.equal(loss, again)                                          # one summation order
    assert_close(loss.cpu(), want.detach(), what="loss", **LOSS_TOL)
    dout = native.fm_loss_bwd(gloss.cuda(), out.cuda(), tgt.cuda(), dev(w), dev(c), sign)
    assert_close(dout.cpu(), o64.grad, what="dout", **TOL)


def test_loss_is_independent_of_alignment():
    """the same 75 values at a 16-byte aligned address and 4 bytes further: lane l owns the same elements either way"""
    from dimsum_amd import native
    out, tgt = torch.from_numpy(seeded((1, 75), 63)).cuda(), torch.from_numpy(seeded((1, 75), 64)).cuda()
    buf = torch.zeros(2, 80, device="cuda")
    buf[0, 1:76], buf[1, 1:76] = out[0], tgt[0]
    shifted = native.fm_loss_fwd(buf[0, 1:76].view(1, 75), buf[1, 1:76].view(1, 75))
    assert buf[0, 1:76].data_ptr() % 16 == 4 and torch.equal(shifted, native.fm_loss_fwd(out, tgt))


# ---- the whole path ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def cpu_draws(monkeypatch):
    # Transport.sample draws x0 = randn_like(x1) on x1's device and then t on the CPU; the fixtures were made on the CPU, where both come
    # from one stream -- here x0 is drawn there too and moved over (like tests/test_transport_golden.py)
    monkeypatch.setattr(torch, "randn_like", lambda x, **k: torch.randn(x.shape).to(x))


@pytest.mark.parametrize("fused_head", [False, True])
def test_training_losses_with_blurring_match_reference_fixture_on_gpu(cpu_draws, fused_head):
    check_blur_losses("cuda", fused_head)


def test_fused_head_matches_the_unblurred_reference_fixture(cpu_draws):
    """the existing transport.npz: every velocity case, and the weighted noise / score ones, through fm_plan without blur and the loss kernels"""
    g = golden("transport")
    x1, y = torch.from_numpy(g["loss_x1"]).cuda(), torch.from_numpy(g["y"]).cuda()
    cases = [(pt, "velocity", None) for pt in ("GVP", "Linear", "VP")] + [("GVP", "noise", "velocity"), ("VP", "noise", None),
                                                                           ("GVP", "score", "likelihood"), ("Linear", "score", "velocity")]
    for pt, pred, lw in cases:
        tag = f"loss_{pt}_{pred}_{lw}"
        tr = create_transport(pt, pred, lw, **EPS, fused_head=True)
        seen = {}

        def model(xt, t, y=None):
            seen["xt"] = xt
            return toy_denoiser(xt, t, y)

        torch.manual_seed(int(g[tag + "_seed"]))
        terms = tr.training_losses(model, x1, dict(y=y))
        assert_close(seen["xt"].cpu(), g[tag + "_xt"], what=tag + " xt", **TOL)
        assert_close(terms["pred"].cpu(), g[tag + "_pred"], what=tag + " pred", **TOL)
        assert_close(terms["loss"].cpu(), g[tag + "_loss"], what=tag + " loss", **LOSS_TOL)


@pytest.mark.parametrize("pred,lw,blur", [("velocity", None, True), ("velocity", None, False), ("noise", "velocity", True),
                                          ("score", "likelihood", False)])
def test_backward_through_the_fused_head_matches_the_unfused_run(pred, lw, blur):
    """loss.backward() through a small convolution standing in for the denoiser: parameter gradients of the fused run against the
    unfused run on the same draws"""
    torch.manual_seed(5)
    net = torch.nn.Conv2d(4, 4, 3, padding=1).cuda()
    x1 = torch.from_numpy(seeded((3, 4, 16, 16), 71)).cuda()
    grads, losses = [], []
    for fused in (False, True):
        tr = create_transport("GVP", pred, lw, **EPS, path_args=dict(use_blurring=blur), fused_head=fused)
        net.zero_grad(set_to_none=True)
        torch.manual_seed(123)
        terms = tr.training_losses(lambda xt, t: net(xt) * (1 + t.view(-1, 1, 1, 1)), x1)
        terms["loss"].mean().backward()
        losses.append(terms["loss"].detach().cpu())
        grads.append([q.grad.detach().cpu() for q in net.parameters()])
        assert all(math.isfinite(float(v.abs().sum())) and float(v.abs().sum()) > 0 for v in grads[-1])
    assert_close(losses[1], losses[0], what="loss", **LOSS_TOL)
    for got, want, name in zip(grads[1], grads[0], ("weight", "bias")):
        assert_close(got, want, what=f"d {name}", **TOL)


def test_blur_times_follow_the_path():
    """blur_sigma_max at the noise end, none at the data end, on the device of the data"""
    ps = create_transport("Linear", "velocity", path_args=dict(use_blurring=True, blur_sigma_max=3)).path_sampler
    t = torch.tensor([0.0, 1.0], device="cuda")
    table = ps.coef_table(t).cpu()
    assert table.shape == (5, 2) and table[4].tolist() == [4.5, 0.0] and table[:4].tolist() == [[0, 1], [1, 0], [1, 1], [-1, -1]]
    assert blur_times(torch.zeros(2, 1, 4, 4, device="cuda"), 3.0).tolist() == [4.5, 4.5]
