"""The LM training loss on the HIP kernels of csrc/cross_entropy.hip (the place of the fused cross-entropy in the reference's training
recipes): `cross_entropy_loss` / `CrossEntropyLoss` over materialised logits, and `linear_cross_entropy`, the head product and the loss
chunk by chunk, which never holds more than `chunk_rows` rows of logits. `cross_entropy_torch` is the same definition in plain torch.

Per row, with s = logit_scale * logits[m, :], eps = label_smoothing and V the number of columns:
    lse = logsumexp(s)    z = lse_square_scale * lse^2    loss = lse - (1 - eps) s[label] - (eps / V) sum(s) + z
A row whose label is ignore_index has loss = z = 0 and a zero gradient; another label outside [0, V) gives loss = NaN and a NaN gradient row."""
import torch
import torch.nn as nn

from .. import gemm, native

_REDUCTIONS = ("mean", "sum", "none")


class _CrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, label_smoothing, logit_scale, lse_square_scale, ignore_index, inplace_backward):
        V = logits.shape[-1]
        x2 = logits.reshape(-1, V)                      # a view wherever the leading dims share one row stride ([..., :vocab] of a padded buffer)
        if x2.stride(-1) != 1:
            x2 = x2.contiguous()
        lab = labels.reshape(-1)
        loss, lse, z_loss = native.cross_entropy_fwd(x2, lab, label_smoothing, logit_scale, lse_square_scale, ignore_index)
        ctx.save_for_backward(x2, lse, lab)
        ctx.args = (label_smoothing, logit_scale, lse_square_scale, ignore_index)
        ctx.inplace, ctx.shape = inplace_backward, logits.shape
        lead = logits.shape[:-1]
        z_loss = z_loss.view(lead)
        ctx.mark_non_differentiable(z_loss)
        return loss.view(lead), z_loss

    @staticmethod
    def backward(ctx, dloss, _dz):
        x2, lse, lab = ctx.saved_tensors
        dloss = dloss.to(torch.float64 if x2.dtype == torch.float64 else torch.float32)      # float32: the kernels' dtype of row values
        dloss = dloss.reshape(-1) if dloss.dim() != 1 else dloss        # a 1-D expanded scalar keeps its stride 0
        dlogits = native.cross_entropy_bwd(dloss, x2, lse, lab, *ctx.args, inplace=ctx.inplace)
        return (dlogits.view(ctx.shape) if dlogits.shape != ctx.shape else dlogits), None, None, None, None, None, None


def cross_entropy_loss(logits, labels, label_smoothing=0.0, logit_scale=1.0, lse_square_scale=0.0, ignore_index=-100, inplace_backward=False):
    """-> (losses, z_losses), both float32 of the leading shape of `logits` (..., V); labels int64 of that leading shape.
    losses include the z term lse_square_scale * lse^2; z_losses return it alone, for logging, and carry no gradient.
    inplace_backward: the gradient is written into the logits' own storage (the logits are gone after backward) -- for logits that nothing
    else reads, as those of an LM head."""
    if tuple(labels.shape) != tuple(logits.shape[:-1]):
        raise ValueError(f"cross_entropy_loss: labels {tuple(labels.shape)} must have the leading shape of logits {tuple(logits.shape)}")
    return _CrossEntropyFn.apply(logits, labels, float(label_smoothing), float(logit_scale), float(lse_square_scale), int(ignore_index),
                                 bool(inplace_backward))


def _n_valid(labels, ignore_index):
    """the number of rows that count, on the device, at least 1 (every row ignored: the mean is 0 / 1 = 0, not NaN)"""
    return (labels != ignore_index).sum().clamp(min=1)


class CrossEntropyLoss(nn.Module):
    """cross_entropy_loss with a reduction: "mean" divides the sum by the number of rows whose label is not ignore_index (counted on the
    device, at least 1), "sum", or "none". return_z_loss: -> (loss, z_loss), the z term reduced the same way (no gradient)."""

    def __init__(self, ignore_index=-100, reduction="mean", label_smoothing=0.0, logit_scale=1.0, lse_square_scale=0.0, inplace_backward=False,
                 return_z_loss=False):
        super().__init__()
        if reduction not in _REDUCTIONS:
            raise NotImplementedError(f"CrossEntropyLoss: reduction {reduction!r} (one of {_REDUCTIONS})")
        self.ignore_index, self.reduction, self.label_smoothing, self.logit_scale = ignore_index, reduction, label_smoothing, logit_scale
        self.lse_square_scale, self.inplace_backward, self.return_z_loss = lse_square_scale, inplace_backward, return_z_loss

    def forward(self, input, target):
        loss, z_loss = cross_entropy_loss(input, target, self.label_smoothing, self.logit_scale, self.lse_square_scale, self.ignore_index,
                                          self.inplace_backward)
        if self.reduction == "mean":
            n = _n_valid(target, self.ignore_index)
            loss, z_loss = loss.sum() / n, z_loss.sum() / n
        elif self.reduction == "sum":
            loss, z_loss = loss.sum(), z_loss.sum()
        return (loss, z_loss) if self.return_z_loss else loss


class _LinearCrossEntropyFn(torch.autograd.Function):
    """The reduced loss of (hidden @ weight[:V]^T + bias[:V]) against labels, chunk_rows rows at a time. The forward already knows every row's
    share of the reduction, so it runs the loss backward on each chunk of logits IN PLACE while they are there and turns them into dh, dW and
    db; the autograd backward only scales those by the incoming scalar. Nothing is read back to the host."""

    @staticmethod
    def forward(ctx, hidden, weight, bias, labels, V, chunk_rows, mean, label_smoothing, logit_scale, lse_square_scale, ignore_index):
        d = hidden.shape[-1]
        h2, lab = hidden.reshape(-1, d), labels.reshape(-1)
        M = h2.shape[0]
        w = weight[:V]
        b = None if bias is None else bias[:V]
        args = (label_smoothing, logit_scale, lse_square_scale, ignore_index)
        need_h, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], bias is not None and ctx.needs_input_grad[2]
        acc = torch.float32 if hidden.dtype in (torch.float16, torch.bfloat16) else hidden.dtype      # row values; dW / db add up over the chunks in it
        valid = (lab != ignore_index).to(acc)
        share = valid / valid.sum().clamp(min=1) if mean else valid                 # d(loss) / d(row loss), on the device
        dh = torch.empty_like(h2) if need_h else None
        dw = torch.zeros(weight.shape, device=weight.device, dtype=acc) if need_w else None           # rows >= V: the padding, zero
        db = torch.zeros(bias.shape, device=bias.device, dtype=acc) if need_b else None
        total = torch.zeros((), device=hidden.device, dtype=acc)
        for r0 in range(0, M, chunk_rows):
            r1 = min(r0 + chunk_rows, M)
            hc = h2[r0:r1]
            logits = gemm.linear(hc, w)
            if b is not None:
                logits += b
            loss, lse, _ = native.cross_entropy_fwd(logits, lab[r0:r1], *args)
            total += (loss * share[r0:r1]).sum()
            if not (need_h or need_w or need_b):
                del logits
                continue
            dlogits = native.cross_entropy_bwd(share[r0:r1], logits, lse, lab[r0:r1], *args, inplace=True)
            if need_h:
                torch.mm(dlogits, w, out=dh[r0:r1])
            if need_w:
                if acc == hidden.dtype:
                    dw[:V].addmm_(dlogits.t(), hc)
                else:
                    dw[:V] += gemm.mm_tn(dlogits, hc, out_dtype=acc)
            if need_b:
                db[:V] += dlogits.sum(0, dtype=acc)
            del logits, dlogits                         # before the next chunk's product allocates: one chunk of logits at a time
        ctx.save_for_backward(dh, None if dw is None else dw.to(weight.dtype), None if db is None else db.to(bias.dtype))
        ctx.hidden_shape = hidden.shape
        return total

    @staticmethod
    def backward(ctx, g):
        dh, dw, db = ctx.saved_tensors
        return (None if dh is None else (dh * g.to(dh.dtype)).view(ctx.hidden_shape), None if dw is None else dw * g.to(dw.dtype),
                None if db is None else db * g.to(db.dtype), None, None, None, None, None, None, None, None)


def linear_cross_entropy(hidden, weight, labels, bias=None, *, chunk_rows=4096, reduction="mean", vocab_size=None, label_smoothing=0.0,
                         logit_scale=1.0, lse_square_scale=0.0, ignore_index=-100):
    """-> the scalar loss (float32) of an LM head: cross_entropy_loss of hidden @ weight[:vocab_size]^T (+ bias[:vocab_size]) against labels,
    reduced by "mean" (over the rows whose label is not ignore_index) or "sum", WITHOUT materialising more than chunk_rows rows of logits.
    hidden (..., d), weight (V_padded, d), bias (V_padded,) or None, labels int64 of hidden's leading shape. vocab_size=None: every row of
    weight is a class; otherwise rows >= vocab_size (vocabulary padding) take no part and get a zero gradient.
    The gradients of hidden, weight and bias are formed during the forward (one in-place loss backward per chunk) and scaled in backward."""
    if reduction not in ("mean", "sum"):
        raise NotImplementedError(f"linear_cross_entropy: reduction {reduction!r}: only 'mean' and 'sum'. The gradients are formed in the "
                                  f"forward from each row's share of the reduction; per-row upstream gradients ('none') would need the "
                                  f"logits again -- use cross_entropy_loss on materialised logits for that")
    V = weight.shape[0] if vocab_size is None else int(vocab_size)
    if not (weight.dim() == 2 and weight.shape[1] == hidden.shape[-1] and 1 <= V <= weight.shape[0]):
        raise ValueError(f"linear_cross_entropy: weight {tuple(weight.shape)} must be (V_padded >= vocab_size = {V}, d = {hidden.shape[-1]})")
    if tuple(labels.shape) != tuple(hidden.shape[:-1]):
        raise ValueError(f"linear_cross_entropy: labels {tuple(labels.shape)} must have the leading shape of hidden {tuple(hidden.shape)}")
    if int(chunk_rows) < 1:
        raise ValueError("linear_cross_entropy: chunk_rows must be >= 1")
    return _LinearCrossEntropyFn.apply(hidden, weight, bias, labels, V, int(chunk_rows), reduction == "mean", float(label_smoothing),
                                       float(logit_scale), float(lse_square_scale), int(ignore_index))


def cross_entropy_torch(logits, labels, label_smoothing=0.0, logit_scale=1.0, lse_square_scale=0.0, ignore_index=-100, return_lse=False):
    """cross_entropy_loss written out in plain torch, in the precision of its inputs (float64 logits give the float64 answer) and
    differentiable by autograd: -> (losses, z_losses), or (losses, z_losses, lse) with return_lse. What the tests compare the kernels with;
    never a fallback: nothing in the package calls it."""
    V = logits.shape[-1]
    s = logits * logit_scale
    lse = torch.logsumexp(s, dim=-1)
    z = lse_square_scale * lse * lse
    ignored = labels == ignore_index
    bad = ~ignored & ((labels < 0) | (labels >= V))
    picked = s.gather(-1, labels.clamp(0, V - 1).unsqueeze(-1)).squeeze(-1)
    loss = lse - (1.0 - label_smoothing) * picked + z
    if label_smoothing > 0.0:
        loss = loss - (label_smoothing / V) * s.sum(-1)
    zero = torch.zeros_like(lse)
    loss = loss * torch.where(bad, torch.full_like(lse, float("nan")), torch.ones_like(lse))       # NaN, and a NaN gradient, for that row alone
    loss = torch.where(ignored, zero, loss)
    z = torch.where(ignored, zero, z).detach()
    return (loss, z, lse.detach()) if return_lse else (loss, z)
