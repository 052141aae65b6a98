"""The LM loss on the GPU: dimsum_cross_entropy_fwd / _bwd (csrc/cross_entropy.hip) against float64 on both of their mappings (one wave per
row, one workgroup per row), on whole pieces, tails and misaligned rows, as views of NaN-padded buffers; the chunked head + loss; training
the tiny fixture model through MambaLMHeadModel.loss.

Kernel bound, per element: 2 x (the error of torch's own fp32 path -- F.cross_entropy / torch.logsumexp and autograd on logits.float(), same
device, same inputs -- against the same float64 values) + 4 * 2^-24 * max(1, |want|), plus half an ulp of T at |want| for a gradient stored in
16 bits. The factor 2 is for the different summation order; the floor is the one test_lm_gpu.py uses where the yardstick happens to be exact.
The worst err / bound of each case is printed."""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import golden
from test_cross_entropy_cpu import ARGS
from test_lm_cpu import LM_TINY, T, tiny_model
from test_mixer_step_gpu import SSU_TOL, exact_fp32  # noqa: F401  (exact_fp32: a fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
TH = 4096                      # _lib.CROSS_ENTROPY_WAVE_ROW_MAX: rows up to it are one wave's, longer ones a workgroup's
MS = (1, 3, 37)
IGNORE = -100
NAN = float("nan")


def piece(dtype):
    return 16 // torch.empty((), dtype=dtype).element_size()


def vocab_sizes(dtype):
    return [1, 3, piece(dtype), 260, TH - 1, TH, TH + 1, 4099, 50280]


def padded_view(M, V, dtype, seed):
    """-> (buf, view): view = buf[1 : M + 1, :V] of a NaN-filled (M + 2, Vp) buffer, Vp the next multiple of 8 above V (50288 for 50280):
    padding columns and a guard row on either side"""
    Vp = (V + 8) // 8 * 8
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((M + 2, Vp), NAN, dtype=dtype, device=DEV)
    buf[1:M + 1, :V] = (3 * torch.randn(M, V, generator=g)).to(dtype).to(DEV)
    return buf, buf[1:M + 1, :V]


def labels_for(M, V, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, V, (M,), generator=g)
    y[0] = V - 1                                   # the last column
    if M > 1:
        y[1] = 0                                   # the first
        y[2] = IGNORE
    return y.to(DEV)


def half_ulp(want, dtype):
    if dtype == torch.float32:
        return torch.zeros_like(want)
    mant, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    e = torch.floor(torch.log2(want.abs().clamp(min=2.0 ** emin)))
    return torch.pow(2.0, e - mant - 1)


def worst(got, want, yard, extra=None):
    """max over the elements of err / bound"""
    err = (got.double() - want).abs()
    bound = 2 * (yard.double() - want).abs() + 4 * 2.0 ** -24 * want.abs().clamp(min=1.0)
    if extra is not None:
        bound = bound + extra
    assert bool(torch.isfinite(got).all()), "a NaN or inf reached an output"
    return (err / bound).max().item()


def references(view, y, dloss, eps, scale, zscale):
    """-> (want, yard): each (loss, lse, dlogits); want in float64 from cross_entropy_torch, yard from torch's fp32 path"""
    from dimsum_amd.ops import cross_entropy_torch
    x64 = view.double().requires_grad_()
    loss, _, lse = cross_entropy_torch(x64, y, eps, scale, zscale, IGNORE, return_lse=True)
    (g64,) = torch.autograd.grad((loss * dloss.double()).sum(), x64)
    xf = view.float().requires_grad_()
    s = xf * scale
    lse32 = torch.logsumexp(s, -1)
    loss32 = F.cross_entropy(s, y, label_smoothing=eps, reduction="none", ignore_index=IGNORE) + torch.where(y == IGNORE, 0.0, zscale * lse32 * lse32)
    (g32,) = torch.autograd.grad((loss32 * dloss).sum(), xf)
    return (loss.detach(), lse, g64), (loss32.detach(), lse32.detach(), g32)


def run_kernels(view, y, dloss, eps, scale, zscale, inplace=False):
    from dimsum_amd import native
    loss, lse, z = native.cross_entropy_fwd(view, y, eps, scale, zscale, IGNORE)
    d = native.cross_entropy_bwd(dloss, view, lse, y, eps, scale, zscale, IGNORE, inplace=inplace)
    return loss, lse, z, d


def check_case(view, y, dloss, args, dtype, what, buf=None):
    """the kernels on `view` (in place when its buffer is given: guards and padding must come back bit-unchanged) -> worst err / bound"""
    want, yard = references(view, y, dloss, *args)
    before = None if buf is None else buf.clone()
    loss, lse, z, d = run_kernels(view, y, dloss, *args, inplace=buf is not None)
    assert d.dtype == dtype and d.shape == view.shape and loss.dtype == z.dtype == torch.float32 and lse.dtype == torch.float64
    if buf is not None:
        M, V = view.shape
        assert d.data_ptr() == view.data_ptr()
        raw = lambda t: t.view(torch.int16 if t.element_size() == 2 else torch.int32)
        assert torch.equal(raw(buf[0]), raw(before[0])) and torch.equal(raw(buf[M + 1]), raw(before[M + 1])), f"{what}: a guard row changed"
        assert torch.equal(raw(buf[1:M + 1, V:]), raw(before[1:M + 1, V:])), f"{what}: the padding changed"
    ws = (worst(loss, want[0], yard[0]), worst(lse, want[1], yard[1]), worst(d, want[2], yard[2], half_ulp(want[2], dtype)))
    w = max(ws)
    ign = y == IGNORE
    assert bool((loss[ign] == 0).all()) and bool((z[ign] == 0).all()) and bool((d[ign] == 0).all()), f"{what}: ignored rows"
    zwant = torch.where(ign, 0.0, args[2] * want[1] * want[1])
    assert worst(z, zwant, torch.where(ign, 0.0, args[2] * yard[1] * yard[1])) <= 1.0, f"{what}: z_loss"
    assert w <= 1.0, f"{what}: err / bound of loss, lse, dlogits {ws[0]:.3f} {ws[1]:.3f} {ws[2]:.3f}"
    return w


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("V", range(9), ids=lambda i: "V%d" % i)
def test_kernels_against_float64(V, dtype):
    V = vocab_sizes(dtype)[V]
    w = 0.0
    for M in MS:
        for i, args in enumerate(ARGS):
            buf, view = padded_view(M, V, dtype, seed=V + M)
            y = labels_for(M, V, seed=i)
            dloss = (0.5 + torch.rand(M, generator=torch.Generator().manual_seed(7))).to(DEV)
            # out of place on the view, then in place inside its NaN-padded buffer: the same bits
            _, _, _, d = run_kernels(view, y, dloss, *args)
            w = max(w, check_case(view, y, dloss, args, dtype, f"M{M} V{V} {args}", buf=buf))
            assert torch.equal(view, d), "the in-place backward differs from the out-of-place one"
    # every row ignored
    buf, view = padded_view(3, V, dtype, seed=1)
    y = torch.full((3,), IGNORE, device=DEV)
    w = max(w, check_case(view, y, torch.ones(3, device=DEV), ARGS[3], dtype, f"V{V} all ignored", buf=buf))
    print(f"cross_entropy {dtype} V={V}: worst err / bound {w:.3f}")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_a_misaligned_base_gives_the_bits_of_its_aligned_copy(dtype):
    """rows that start 4 bytes off a 16-byte boundary are walked element by element; same pieces, same lanes, same bits"""
    off = 4 // torch.empty((), dtype=dtype).element_size()
    for M, V in ((3, 264), (2, TH + 8), (1, 261), (1, TH + 3)):           # rows of M > 1 keep 16-byte strides: only the base is off
        flat = torch.full((M * V + off + 8,), NAN, dtype=dtype, device=DEV)
        g = torch.Generator().manual_seed(V)
        x = (3 * torch.randn(M, V, generator=g)).to(dtype).to(DEV)
        view = flat[off:off + M * V].view(M, V)
        view.copy_(x)
        assert view.data_ptr() % 16 == 4 and x.data_ptr() % 16 == 0
        y = labels_for(M, V, seed=3) if M > 2 else torch.tensor([V - 1, 0], device=DEV)[:M]
        dloss = torch.tensor(0.25, device=DEV).expand(M)                       # an expanded scalar: stride 0
        a, b = run_kernels(view, y, dloss, *ARGS[3]), run_kernels(x, y, dloss, *ARGS[3])
        for ta, tb in zip(a, b):
            assert torch.equal(ta, tb), (M, V)
        check_case(x, y, dloss.contiguous(), ARGS[3], dtype, f"misaligned M{M} V{V}")


def test_range():
    """a running sum that is not rescaled overflows here"""
    V = 300
    x = torch.zeros(5, V, device=DEV)
    x[0, 7], x[0, 200] = 80.0, -80.0
    x[1, 290], x[1, 3] = 80.0, -80.0                # the large one late in the row
    x[2] = 11.5                                     # equal values
    x[3] = torch.randn(V, generator=torch.Generator().manual_seed(0)).to(DEV)
    x[3, 10:40] = -math.inf
    x[3, 299] = -math.inf
    x[4] = torch.linspace(-80, 80, V).to(DEV)
    y = torch.tensor([7, 3, 5, 100, 299], device=DEV)
    dloss = torch.ones(5, device=DEV)
    for scale in (1.0, 2.0):
        w = check_case(x, y, dloss, (0.0, scale, 0.0), torch.float32, f"range scale {scale}")
        print(f"cross_entropy range, logit_scale {scale}: worst err / bound {w:.3f}")
    long = torch.zeros(2, TH + 5, device=DEV)       # the workgroup-per-row kernel: the waves' pairs differ by 160
    long[0, 1], long[0, TH], long[1, TH + 4], long[1, 0] = 80.0, -80.0, 80.0, -80.0
    check_case(long, torch.tensor([1, 0], device=DEV), dloss[:2], (0.0, 2.0, 1e-4), torch.float32, "range, long rows")
    h = torch.zeros(2, 72, device=DEV, dtype=torch.float16)
    h[0, 33], h[1, 71], h[1, 0] = 65504.0, 65504.0, -65504.0
    w = check_case(h, torch.tensor([33, 2], device=DEV), dloss[:2], (0.0, 1.0, 0.0), torch.float16, "range f16")
    print(f"cross_entropy range, float16 max: worst err / bound {w:.3f}")


def test_out_of_range_label_is_nan_for_its_row_alone():
    buf, view = padded_view(4, 260, torch.float32, seed=2)
    y = torch.tensor([3, 260, -1, 259], device=DEV)
    before = buf.clone()
    loss, lse, z, d = run_kernels(view, y, torch.ones(4, device=DEV), 0.1, 1.0, 1e-4, inplace=True)
    torch.cuda.synchronize()
    assert torch.isnan(loss).tolist() == [False, True, True, False] and bool(torch.isfinite(lse).all())
    assert torch.isnan(d).all(1).tolist() == [False, True, True, False] and torch.isnan(d).any(1).tolist() == [False, True, True, False]
    assert torch.equal(buf[0].view(torch.int32), before[0].view(torch.int32)) and torch.equal(buf[5].view(torch.int32), before[5].view(torch.int32))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
@pytest.mark.parametrize("V", [TH, TH + 1, 50280])
def test_reproducible_and_independent_of_the_other_rows(V, dtype):
    M = 37
    _, view = padded_view(M, V, dtype, seed=5)
    y = labels_for(M, V, seed=5)
    dloss = (0.5 + torch.rand(M, generator=torch.Generator().manual_seed(1))).to(DEV)
    a, b = run_kernels(view, y, dloss, *ARGS[3]), run_kernels(view, y, dloss, *ARGS[3])
    for ta, tb in zip(a, b):
        assert torch.equal(ta, tb)
    for r in (0, 5, 36):
        one = run_kernels(view[r:r + 1], y[r:r + 1], dloss[r:r + 1], *ARGS[3])
        for ta, tb in zip(a, one):
            assert torch.equal(ta[r:r + 1], tb), (r, V)


# ---- the chunked head + loss -----------------------------------------------------------------------------------------------------------------------
def test_chunked_head_against_float64(exact_fp32):  # noqa: F811
    from dimsum_amd.ops import cross_entropy_torch, linear_cross_entropy
    M, d, V, Vp = 37, 64, 1001, 1008
    g = torch.Generator().manual_seed(0)
    h = torch.randn(M, d, generator=g).to(DEV)
    w = (torch.randn(Vp, d, generator=g) * d ** -0.5).to(DEV)
    y = torch.randint(0, V, (M,), generator=g).to(DEV)
    y[16:32] = IGNORE                                                      # the second chunk entirely
    y[0], y[1] = 0, V - 1
    kw = dict(label_smoothing=0.1, lse_square_scale=1e-4)
    h64, w64 = h.double().requires_grad_(), w.double().requires_grad_()
    want = cross_entropy_torch(F.linear(h64, w64)[:, :V], y, **kw)[0].sum() / 21
    want.backward()
    hf, wf = h.clone().requires_grad_(), w.clone().requires_grad_()
    logits = F.linear(hf, wf)[:, :V]
    lse = torch.logsumexp(logits, -1)
    yard = (F.cross_entropy(logits, y, label_smoothing=0.1, reduction="none") + torch.where(y == IGNORE, 0.0, 1e-4 * lse * lse)).sum() / 21
    yard.backward()
    hg, wg = h.clone().requires_grad_(), w.clone().requires_grad_()
    got = linear_cross_entropy(hg, wg, y, chunk_rows=16, vocab_size=V, **kw)
    got.backward()
    ws = [worst(got.detach(), want.detach(), yard.detach()), worst(hg.grad, h64.grad, hf.grad), worst(wg.grad, w64.grad, wf.grad)]
    print(f"linear_cross_entropy: worst err / bound loss {ws[0]:.3f} dh {ws[1]:.3f} dW {ws[2]:.3f}")
    assert max(ws) <= 1.0, ws
    assert bool((wg.grad[V:] == 0).all()) and bool((hg.grad[16:32] == 0).all())


def test_chunked_head_never_holds_the_logits():
    from dimsum_amd.ops import linear_cross_entropy
    M, d, V, Vp = 4096, 64, 50280, 50288
    g = torch.Generator(device=DEV).manual_seed(0)
    h = torch.randn(M, d, device=DEV, generator=g).requires_grad_()
    w = (torch.randn(Vp, d, device=DEV, generator=g) * d ** -0.5).requires_grad_()
    y = torch.randint(0, V, (M,), device=DEV, generator=g)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = linear_cross_entropy(h, w, y, chunk_rows=512, vocab_size=V)
    loss.backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"linear_cross_entropy M={M} V={V} chunk_rows=512: peak rise {rise / 1e6:.0f} MB (the logits alone: {M * V * 4 / 1e6:.0f} MB)")
    assert bool(torch.isfinite(loss)) and rise < M * V * 4 // 2
    assert abs(loss.item() - math.log(V)) < 1.0                             # random logits of unit scale: about ln V + 1/2


# ---- the model -------------------------------------------------------------------------------------------------------------------------------------
def gpu_model(dtype=torch.float32):
    g = golden("lm_tiny_rms1_fp32res1")
    return tiny_model(1, 1, g).to(DEV).to(dtype), T(g["prompt"]).to(DEV)


def test_model_loss_and_gradients_equal_the_materialised_path(exact_fp32):  # noqa: F811
    V = LM_TINY["vocab_size"]
    m, ids = gpu_model()
    loss = m.loss(ids, chunk_rows=5)
    loss.backward()
    got = {k: p.grad.clone() for k, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    logits = m(ids).logits[..., :V]
    ref = F.cross_entropy(logits[:, :-1].reshape(-1, V), ids[:, 1:].reshape(-1))
    ref.backward()
    want64 = F.cross_entropy(logits.detach().double()[:, :-1].reshape(-1, V), ids[:, 1:].reshape(-1))
    w = worst(loss.detach(), want64, ref.detach())
    print(f"model.loss: err / bound {w:.3f}")
    assert w <= 1.0
    assert set(got) == {k for k, _ in m.named_parameters()} and "backbone.embedding.weight" in got
    for k, p in m.named_parameters():
        err, scale = (got[k] - p.grad).abs().max().item(), p.grad.abs().max().item()
        assert err <= 3e-4 * scale, f"{k}: max |err| {err:.3e} against max |grad| {scale:.3e}"
    assert bool((got["backbone.embedding.weight"][V:] == 0).all())        # the vocabulary padding: no gradient from the head


def test_three_sgd_steps_lower_the_loss(exact_fp32):  # noqa: F811
    m, ids = gpu_model()
    opt = torch.optim.SGD(m.parameters(), lr=0.02)
    losses = []
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        loss = m.loss(ids)
        loss.backward()
        opt.step()
        losses.append(loss)
    with torch.no_grad():
        losses.append(m.loss(ids))
    losses = [v.item() for v in losses]
    print("model.loss over three SGD steps:", " ".join(f"{v:.4f}" for v in losses))
    assert all(math.isfinite(v) for v in losses) and losses[0] > losses[1] > losses[2] > losses[3]


def test_bf16_model_loss_is_close_to_fp32():
    m, ids = gpu_model()
    with torch.no_grad():
        want = m.loss(ids)
    m16, _ = gpu_model(torch.bfloat16)
    got = m16.loss(ids, chunk_rows=8)                                       # with the head's gradients formed in the forward
    rtol, atol = SSU_TOL[torch.bfloat16]
    assert got.dtype == torch.float32 and math.isfinite(got.item())
    assert abs(got.item() - want.item()) <= atol + rtol * abs(want.item()), (got.item(), want.item())
