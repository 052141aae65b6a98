"""The LM loss without a GPU: `cross_entropy_torch` (the definition the GPU tests compare the kernels with) against F.cross_entropy and
hand-computed rows; the autograd Functions of ops/cross_entropy.py with native.cross_entropy_fwd / _bwd replaced by plain-torch restatements
(`native_ce_fwd` / `native_ce_bwd` below, as test_lm_cpu.py does for decode_linear) in float64, where the chunked head-plus-loss path must
equal the unchunked autograd result to roundoff; MambaLMHeadModel.loss on the tiny fixture model; the C ABI checks of
dimsum_cross_entropy_fwd / _bwd in their documented order with host pointers that are never dereferenced, nothing launched."""
import ctypes
import math
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import golden
from oracle.torch_backend import cpu_oracle_backend
from test_host_logic import _header_layout
from test_lm_cpu import LM_TINY, T, tiny_model
from test_mixer_step_cpu import close

ARGS = [(0.0, 1.0, 0.0), (0.1, 1.0, 0.0), (0.0, 0.5, 1e-4), (0.1, 2.0, 1e-4)]          # (label_smoothing, logit_scale, lse_square_scale)


def native_ce_fwd(logits, labels, label_smoothing=0.0, logit_scale=1.0, lse_square_scale=0.0, ignore_index=-100):
    """native.cross_entropy_fwd restated in torch in the precision of the logits: -> (loss, lse, z_loss)"""
    from dimsum_amd.ops import cross_entropy_torch
    loss, z, lse = cross_entropy_torch(logits.detach(), labels, label_smoothing, logit_scale, lse_square_scale, ignore_index, return_lse=True)
    return loss, lse, z


def native_ce_bwd(dloss, logits, lse, labels, label_smoothing=0.0, logit_scale=1.0, lse_square_scale=0.0, ignore_index=-100, inplace=False):
    """native.cross_entropy_bwd restated in torch: the closed form of include/dimsum_hip.h from the saved lse, optionally over the logits"""
    V = logits.shape[-1]
    ignored = labels == ignore_index
    bad = ~ignored & ((labels < 0) | (labels >= V))
    onehot = F.one_hot(labels.clamp(0, V - 1), V).to(logits.dtype)
    p = torch.exp(logits * logit_scale - lse[:, None])
    d = dloss[:, None] * logit_scale * ((1 + 2 * lse_square_scale * lse)[:, None] * p - (1 - label_smoothing) * onehot - label_smoothing / V)
    d = torch.where(ignored[:, None], torch.zeros_like(d), torch.where(bad[:, None], torch.full_like(d, float("nan")), d)).to(logits.dtype)
    if inplace:
        logits.copy_(d)
        return logits
    return d


@pytest.fixture
def ce_backend(monkeypatch):
    from dimsum_amd import native
    monkeypatch.setattr(native, "cross_entropy_fwd", native_ce_fwd)
    monkeypatch.setattr(native, "cross_entropy_bwd", native_ce_bwd)


def rows(M, V, seed=0, ignore=()):
    g = torch.Generator().manual_seed(seed)
    x = 3 * torch.randn(M, V, generator=g, dtype=torch.float64)
    y = torch.randint(0, V, (M,), generator=g)
    y[list(ignore)] = -100
    return x, y


# ---- the definition --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_definition_equals_torch_cross_entropy(eps):
    from dimsum_amd.ops import cross_entropy_torch
    x, y = rows(13, 29, ignore=(0, 5, 12))
    loss, z = cross_entropy_torch(x, y, label_smoothing=eps)
    want = F.cross_entropy(x, y, label_smoothing=eps, reduction="none")
    assert loss.dtype == torch.float64 and torch.allclose(loss, want, rtol=1e-13, atol=1e-13)
    assert bool((loss[[0, 5, 12]] == 0).all()) and bool((z == 0).all())
    # another ignore_index, a leading shape of two dims
    y2 = y.clone()
    y2[y2 == -100] = 7
    loss2, _ = cross_entropy_torch(x.view(1, 13, 29), y2.view(1, 13), label_smoothing=eps, ignore_index=7)
    assert torch.allclose(loss2[0], F.cross_entropy(x, y2, label_smoothing=eps, reduction="none", ignore_index=7), rtol=1e-13, atol=1e-13)


def test_z_loss_and_logit_scale_against_a_hand_computed_case():
    from dimsum_amd.ops import cross_entropy_torch
    x = torch.tensor([[0.0, math.log(2.0), math.log(3.0)], [2.0, 2.0, 2.0]], dtype=torch.float64)
    y = torch.tensor([2, 0])
    # row 0: sum exp = 1 + 2 + 3, lse = ln 6; row 1: lse = 2 + ln 3
    lse = torch.tensor([math.log(6.0), 2.0 + math.log(3.0)], dtype=torch.float64)
    loss, z, got_lse = cross_entropy_torch(x, y, lse_square_scale=0.01, return_lse=True)
    assert torch.allclose(got_lse, lse, rtol=1e-14)
    assert torch.allclose(z, 0.01 * lse ** 2, rtol=1e-14)
    assert torch.allclose(loss, torch.tensor([math.log(6.0) - math.log(3.0), math.log(3.0)], dtype=torch.float64) + 0.01 * lse ** 2, rtol=1e-14)
    # logit_scale 2: row 0 is ln(1, 4, 9), lse = ln 14, s[label] = ln 9; row 1: lse = 4 + ln 3. Smoothing 0.3: minus 0.3 * (mean(s) - s[label])
    lse2 = torch.tensor([math.log(14.0), 4.0 + math.log(3.0)], dtype=torch.float64)
    loss, z, got_lse = cross_entropy_torch(x, y, logit_scale=2.0, lse_square_scale=0.5, label_smoothing=0.3, return_lse=True)
    mean_s = torch.tensor([(math.log(4.0) + math.log(9.0)) / 3, 4.0], dtype=torch.float64)
    picked = torch.tensor([math.log(9.0), 4.0], dtype=torch.float64)
    assert torch.allclose(got_lse, lse2, rtol=1e-14) and torch.allclose(z, 0.5 * lse2 ** 2, rtol=1e-14)
    assert torch.allclose(loss, lse2 - 0.7 * picked - 0.3 * mean_s + 0.5 * lse2 ** 2, rtol=1e-14)


def test_out_of_range_label_gives_nan_for_its_row_alone():
    from dimsum_amd.ops import cross_entropy_torch
    x, y = rows(4, 6)
    y[1], y[3] = 6, -1
    x.requires_grad_()
    loss, z, lse = cross_entropy_torch(x, y, lse_square_scale=0.1, return_lse=True)
    assert torch.isnan(loss).tolist() == [False, True, False, True] and bool(torch.isfinite(lse).all())
    loss[[0, 2]].sum().backward()
    assert bool(torch.isfinite(x.grad[[0, 2]]).all())
    dl = native_ce_bwd(torch.ones(4, dtype=torch.float64), x.detach(), lse, y, lse_square_scale=0.1)
    assert torch.isnan(dl).all(1).tolist() == [False, True, False, True] and torch.isnan(dl).any(1).tolist() == [False, True, False, True]


# ---- the autograd Function on the restatements -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps,scale,zscale", ARGS)
def test_function_gradients_equal_autograd_through_the_definition(eps, scale, zscale, ce_backend):
    from dimsum_amd.ops import cross_entropy_loss, cross_entropy_torch
    x, y = rows(11, 17, seed=1, ignore=(2, 10))
    w = torch.randn(11, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    a, b = x.clone().requires_grad_(), x.clone().requires_grad_()
    loss, z = cross_entropy_loss(a.view(1, 11, 17), y.view(1, 11), eps, scale, zscale)
    want, want_z = cross_entropy_torch(b, y, eps, scale, zscale)
    assert loss.shape == z.shape == (1, 11) and not z.requires_grad
    assert torch.allclose(loss[0], want, rtol=1e-13, atol=1e-13) and torch.allclose(z[0], want_z, rtol=1e-13, atol=1e-13)
    (loss[0] * w).sum().backward()
    (want * w).sum().backward()
    assert torch.allclose(a.grad, b.grad, rtol=1e-12, atol=1e-13)
    assert bool((a.grad[[2, 10]] == 0).all())


def test_inplace_backward_returns_the_logits_storage(ce_backend):
    from dimsum_amd.ops import cross_entropy_loss
    x, y = rows(5, 12, seed=3)
    buf = torch.full((7, 16), float("nan"), dtype=torch.float64)           # a padded buffer with a guard row on either side
    buf[1:6, :12] = x
    view = buf[1:6, :12].requires_grad_()
    loss, _ = cross_entropy_loss(view, y, inplace_backward=True)
    (grad,) = torch.autograd.grad(loss.sum(), view)
    assert grad.data_ptr() == view.data_ptr() and grad.stride() == view.stride()
    plain = x.clone().requires_grad_()
    (want,) = torch.autograd.grad(cross_entropy_loss(plain, y)[0].sum(), plain)
    assert want.data_ptr() != plain.data_ptr() and torch.equal(grad, want)
    assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[6]).all()) and bool(torch.isnan(buf[1:6, 12:]).all())


def test_module_reductions(ce_backend):
    from dimsum_amd.ops import CrossEntropyLoss, cross_entropy_torch
    x, y = rows(9, 14, seed=4, ignore=(1, 2, 8))
    per_row, per_z = cross_entropy_torch(x, y, 0.1, 1.0, 1e-2)
    kw = dict(label_smoothing=0.1, lse_square_scale=1e-2)
    assert torch.allclose(CrossEntropyLoss(reduction="mean", **kw)(x, y), per_row.sum() / 6, rtol=1e-13)
    assert torch.allclose(CrossEntropyLoss(reduction="sum", **kw)(x, y), per_row.sum(), rtol=1e-13)
    assert torch.allclose(CrossEntropyLoss(reduction="none", **kw)(x, y), per_row, rtol=1e-13)
    loss, z = CrossEntropyLoss(return_z_loss=True, **kw)(x, y)
    assert torch.allclose(z, per_z.sum() / 6, rtol=1e-13) and torch.allclose(loss, per_row.sum() / 6, rtol=1e-13)
    assert torch.allclose(CrossEntropyLoss()(x, y), F.cross_entropy(x, y), rtol=1e-13)
    # every row ignored: 0, not 0 / 0
    a = x.clone().requires_grad_()
    none = CrossEntropyLoss()(a, torch.full((9,), -100))
    none.backward()
    assert none.item() == 0.0 and bool((a.grad == 0).all())
    with pytest.raises(NotImplementedError, match="reduction"):
        CrossEntropyLoss(reduction="batchmean")


# ---- the chunked head + loss -----------------------------------------------------------------------------------------------------------------------
def head_case():
    g = torch.Generator().manual_seed(5)
    M, d, V, Vp = 37, 8, 21, 24
    h, w, b = (torch.randn(*s, generator=g, dtype=torch.float64) for s in ((M, d), (Vp, d), (Vp,)))
    y = torch.randint(0, V, (M,), generator=g)
    y[5:10] = -100                      # chunk_rows 5: the second chunk is ignored entirely
    y[36] = -100
    return h, w, b, y, V


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("chunk_rows", [5, 16, 37, 64])
def test_chunked_head_equals_the_unchunked_autograd_result(chunk_rows, reduction, ce_backend):
    from dimsum_amd.ops import cross_entropy_torch, linear_cross_entropy
    h, w, b, y, V = head_case()
    args = dict(label_smoothing=0.1, lse_square_scale=1e-3)
    leaves = [t.clone().requires_grad_() for t in (h, w, b)]
    per_row, _ = cross_entropy_torch(F.linear(leaves[0], leaves[1], leaves[2])[:, :V], y, **args)
    want = per_row.sum() / 31 if reduction == "mean" else per_row.sum()
    (3.0 * want).backward()
    got_leaves = [t.clone().requires_grad_() for t in (h, w, b)]
    got = linear_cross_entropy(got_leaves[0].view(1, 37, 8), got_leaves[1], y.view(1, 37), got_leaves[2], chunk_rows=chunk_rows,
                               reduction=reduction, vocab_size=V, **args)
    (3.0 * got).backward()                                                  # the incoming gradient scales the stored ones
    assert got.dim() == 0 and abs(got.item() - want.item()) <= 1e-12 * abs(want.item())
    for name, a, r in zip(("dh", "dW", "db"), got_leaves, leaves):
        assert a.grad.shape == r.grad.shape, name
        assert (a.grad - r.grad).abs().max().item() <= 1e-12 * r.grad.abs().max().item(), name
    assert bool((got_leaves[1].grad[V:] == 0).all()) and bool((got_leaves[2].grad[V:] == 0).all())      # the vocabulary padding
    assert bool((got_leaves[0].grad[5:10] == 0).all())


def test_chunked_head_without_bias_grads_and_refusals(ce_backend):
    from dimsum_amd.ops import cross_entropy_torch, linear_cross_entropy
    h, w, _, y, V = head_case()
    want = cross_entropy_torch(F.linear(h, w), y)[0].sum() / 31               # vocab_size None: every row of the weight is a class
    got = linear_cross_entropy(h, w, y, chunk_rows=16)
    assert not got.requires_grad and abs(got.item() - want.item()) <= 1e-12 * abs(want.item())
    hw = h.clone().requires_grad_()
    linear_cross_entropy(hw, w, y, chunk_rows=16).backward()                  # only the hidden states want a gradient
    assert hw.grad is not None and w.grad is None
    assert linear_cross_entropy(h, w, torch.full((37,), -100), chunk_rows=16).item() == 0.0
    with pytest.raises(NotImplementedError, match="would need the\\s+logits again"):
        linear_cross_entropy(h, w, y, reduction="none")
    with pytest.raises(ValueError, match="leading shape"):
        linear_cross_entropy(h, w, y[:-1])
    with pytest.raises(ValueError, match="vocab_size"):
        linear_cross_entropy(h, w, y, vocab_size=25)


# ---- the model -------------------------------------------------------------------------------------------------------------------------------------
def test_model_loss_equals_cross_entropy_on_its_logits(ce_backend):
    g = golden("lm_tiny_rms1_fp32res1")
    m = tiny_model(1, 1, g)
    ids = T(g["prompt"])
    with cpu_oracle_backend(), torch.no_grad():
        logits = m(ids).logits[..., :LM_TINY["vocab_size"]]
        loss = m.loss(ids, chunk_rows=5)
        shifted = torch.cat([ids[:, 1:], torch.full((2, 1), -100)], 1)
        explicit = m.loss(ids, shifted, chunk_rows=64)
        smoothed = m.loss(ids, label_smoothing=0.1, lse_square_scale=1e-4, reduction="sum")
    want = F.cross_entropy(logits[:, :-1].reshape(-1, 90), ids[:, 1:].reshape(-1))
    close(loss, want, "loss")
    close(explicit, loss, "labels=None is next-token prediction")
    per_row = F.cross_entropy(logits[:, :-1].reshape(-1, 90), ids[:, 1:].reshape(-1), label_smoothing=0.1, reduction="none")
    zterm = 1e-4 * torch.logsumexp(logits[:, :-1].reshape(-1, 90), -1) ** 2
    assert torch.allclose(smoothed, (per_row + zterm).sum(), rtol=3e-4)


# ---- the wrappers ----------------------------------------------------------------------------------------------------------------------------------
def test_native_wrappers_refuse_clearly():
    from dimsum_amd import native
    x, y = torch.zeros(4, 8), torch.zeros(4, dtype=torch.int64)
    lse, dl = torch.zeros(4, dtype=torch.float64), torch.ones(4)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        native.cross_entropy_fwd(x, y)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        native.cross_entropy_bwd(dl, x, lse, y)
    with pytest.raises(RuntimeError, match="labels must be \\(rows,\\) int64"):
        native.cross_entropy_fwd(x, y.int())
    with pytest.raises(RuntimeError, match="unit column stride"):
        native.cross_entropy_fwd(torch.zeros(8, 4).t(), y)
    with pytest.raises(RuntimeError, match="float32, float16 or bfloat16"):
        native.cross_entropy_fwd(x.double(), y)
    with pytest.raises(RuntimeError, match="row stride >= vocab"):
        native.cross_entropy_fwd(torch.zeros(1, 8).expand(4, 8), y)
    with pytest.raises(RuntimeError, match="label_smoothing"):
        native.cross_entropy_fwd(x, y, label_smoothing=1.0)
    with pytest.raises(RuntimeError, match="dloss must be \\(rows,\\) float32"):
        native.cross_entropy_bwd(dl.double(), x, lse, y)
    with pytest.raises(RuntimeError, match="lse must be"):
        native.cross_entropy_bwd(dl, x, lse[:3], y)


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------------------------
def test_struct_layout_and_exports():
    from dimsum_amd import _lib
    layout = _header_layout([("dimsum_cross_entropy_params_t", _lib.CrossEntropyParams)])
    size, offs = layout["dimsum_cross_entropy_params_t"]
    assert size == ctypes.sizeof(_lib.CrossEntropyParams) == _lib.CrossEntropyParams().struct_size
    assert offs == {f: getattr(_lib.CrossEntropyParams, f).offset for f, _ in _lib.CrossEntropyParams._fields_}
    assert _lib.CrossEntropyParams._fields_[0][0] == "struct_size"
    lib = _lib.load()
    assert lib.dimsum_abi_version() == 18                                      # new symbols only: the ABI number stands
    header = open(os.path.join(_lib._HERE, "..", "include", "dimsum_hip.h")).read()
    for name in ("dimsum_cross_entropy_fwd", "dimsum_cross_entropy_bwd"):
        assert name in _lib.EXPORTS and hasattr(lib, name) and f"int {name}(" in header


def test_library_checks_in_their_documented_order():
    """every pointer set to host memory that is never dereferenced: the checks run on the host and return before a launch. Each call breaks
    one rule AND every later one's, so the code that comes back names the first check that fails"""
    from dimsum_amd import _lib
    lib = _lib.load()
    fwd, bwd = lib.dimsum_cross_entropy_fwd, lib.dimsum_cross_entropy_bwd
    NULL, DTYPE, SHAPE, STRIDE, UNSUPPORTED, ABI, ALIAS = 1, 2, 3, 4, 5, 7, 8
    buf = (ctypes.c_float * 8192)()
    addr = ctypes.addressof(buf)
    for fn in (fwd, bwd):
        assert fn(None, None) == NULL
        P = _lib.CrossEntropyParams()
        P.struct_size += 8
        assert fn(P, None) == ABI                                              # before anything else is read
    # wrong in every later way: rows 0, dtype 3, a row stride below vocab, label_smoothing 1, dlogits half over logits
    P = _lib.CrossEntropyParams()
    P.rows, P.vocab, P.dtype, P.logits_row_stride, P.dlogits_row_stride, P.dloss_stride, P.label_smoothing = 0, 8, 3, 4, 4, -1, 1.0
    for fn, ptrs in ((fwd, ("logits_ptr", "labels_ptr", "lse_ptr", "loss_ptr")), (bwd, ("logits_ptr", "labels_ptr", "lse_ptr", "dloss_ptr", "dlogits_ptr"))):
        for f in ("logits_ptr", "labels_ptr", "lse_ptr", "loss_ptr", "dloss_ptr", "dlogits_ptr", "z_loss_ptr"):
            setattr(P, f, None)
        for f in ptrs:
            assert fn(P, None) == NULL, f                                      # while one required pointer is missing (z_loss is optional)
            setattr(P, f, addr + 16384 if f != "dlogits_ptr" else addr + 64)
        P.logits_ptr = addr
        for r, v in ((0, 8), (-1, 8), (4, 0), (1 << 31, 8), (4, (1 << 31) - 16)):
            P.rows, P.vocab = r, v
            assert fn(P, None) == SHAPE, (r, v)
        P.rows, P.vocab = 4, 8
        for dt in (3, -1):
            P.dtype = dt
            assert fn(P, None) == DTYPE
        P.dtype = 0
        assert fn(P, None) == STRIDE                                           # logits_row_stride 4 < vocab 8
        P.logits_row_stride = 8
        if fn is bwd:
            assert fn(P, None) == STRIDE                                       # dlogits_row_stride 4
            P.dlogits_row_stride = 8
            assert fn(P, None) == STRIDE                                       # dloss_stride -1
            P.dloss_stride = 0
            # logits: 4 rows of 8 floats (128 bytes) from addr + 1024. dlogits over part of them is refused at either end, and so is the same
            # base under another row stride; the in-place backward (same base, same stride) is the one overlap allowed, and it and a
            # disjoint dlogits go on to the next check (label_smoothing is still 1)
            P.logits_ptr = addr + 1024
            for off in (64, 124, -124):
                P.dlogits_ptr = addr + 1024 + off
                assert fn(P, None) == ALIAS, off
            P.dlogits_ptr, P.dlogits_row_stride = addr + 1024, 16
            assert fn(P, None) == ALIAS
            P.dlogits_row_stride = 8
            assert fn(P, None) == UNSUPPORTED                                  # in place
            P.dlogits_ptr = addr + 1024 + 128
            assert fn(P, None) == UNSUPPORTED                                  # the first byte after the logits
        for eps in (1.0, -0.1, float("nan")):
            P.label_smoothing = eps
            assert fn(P, None) == UNSUPPORTED, eps
        P.label_smoothing, P.logit_scale = 0.1, float("inf")
        assert fn(P, None) == UNSUPPORTED
        P.logit_scale, P.lse_square_scale = 1.0, float("nan")
        assert fn(P, None) == UNSUPPORTED                                      # (a call that passed every check would launch: none does)
        # break again what the next entry's pass repairs
        P.rows, P.dtype, P.logits_row_stride, P.dlogits_row_stride, P.dloss_stride, P.label_smoothing = 0, 3, 4, 4, -1, 1.0
        P.logit_scale, P.lse_square_scale = 1.0, 0.0
