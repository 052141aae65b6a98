"""The rope and cpe positional encodings of the embed pass as autograd operators on (batch, L = grid * grid tokens, channels) float32 tensors:

  rotary(x, sin, cos)          x cos + rotate_half(x) sin                               (dimsum/pe/my_rotary.py:63-72)
  cpe(x, weight, bias, gamma, beta, mod, grid, eps)
                               modulate(LayerNorm(conv3x3_depthwise(x) + x), shift, scale), (shift | scale) = mod
                                                                                         (dimsum/pe/cpe.py:37-48)

Each forward is ONE HIP launch (csrc/pos_embed.hip through dimsum_amd.native). The rotary map is a rotation of every channel pair, so its
backward is the same kernel with the sign of sin flipped. The cpe backward is two launches; it keeps x, the row statistics (mean, rstd) and
the operands, and rebuilds v = conv(x) + x from x instead of keeping it ("Positional encodings").
The torch expressions at the end document the math and serve the tests; the model never calls them."""
import torch
import torch.nn.functional as F

from .. import native


class _RotaryFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, sin, cos):
        ctx.save_for_backward(sin, cos)
        return native.pos_rope(x, sin, cos)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        sin, cos = ctx.saved_tensors
        return native.pos_rope(dy, sin, cos, inverse=True), None, None


def rotary(x, sin, cos):
    """x: (B, L, C); sin, cos: (L, C) tables (constants: no gradient)"""
    return _RotaryFn.apply(x, sin, cos)


class _CpeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, mod, grid, eps):
        C = x.shape[-1]
        shift, scale = mod[:, :C], mod[:, C:]
        need = any(ctx.needs_input_grad)
        y, mean, rstd, _ = native.pos_cpe_fwd(x, weight, bias, gamma, beta, shift, scale, grid, eps, need_stats=need)
        if need:
            ctx.save_for_backward(x, weight, bias, gamma, beta, mod, mean, rstd)
            ctx.grid, ctx.eps = grid, eps
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, weight, bias, gamma, beta, mod, mean, rstd = ctx.saved_tensors
        C = x.shape[-1]
        dx, dweight, dbias, dgamma, dbeta, dmod = native.pos_cpe_bwd(dy, x, weight, bias, gamma, beta, mod[:, :C], mod[:, C:], mean, rstd,
                                                                     ctx.grid, ctx.eps)
        return dx, dweight, dbias, dgamma, dbeta, dmod, None, None


def cpe(x, weight, bias, gamma, beta, mod, grid, eps=1e-5):
    """x: (B, grid^2, C); weight (C, 1, 3, 3), bias (C,): the depthwise convolution; gamma, beta (C,): the LayerNorm's affine;
    mod (B, 2 C): the adaLN head's output [shift | scale]"""
    return _CpeFn.apply(x, weight, bias, gamma, beta, mod, grid, eps)


# ---- the same maps as torch expressions (documentation, tests) ---------------------------------------------------------------------------------
def rotate_half(x):
    pairs = x.reshape(*x.shape[:-1], -1, 2)
    return torch.stack((-pairs[..., 1], pairs[..., 0]), dim=-1).reshape(x.shape)


def rotary_torch(x, sin, cos, inverse=False):
    """inverse: the transpose of the forward map, g cos - rotate_half(g sin)"""
    if inverse:
        return x * cos - rotate_half(x * sin)
    return x * cos + rotate_half(x) * sin


def cpe_v_torch(x, weight, bias, grid):
    B, L, C = x.shape
    img = x.transpose(1, 2).reshape(B, C, grid, grid)
    return (F.conv2d(img, weight.reshape(C, 1, 3, 3), bias, padding=1, groups=C) + img).flatten(2).transpose(1, 2)


def cpe_torch(x, weight, bias, gamma, beta, mod, grid, eps=1e-5):
    C = x.shape[-1]
    n = F.layer_norm(cpe_v_torch(x, weight, bias, grid), (C,), gamma, beta, eps)
    return n * (1 + mod[:, None, C:]) + mod[:, None, :C]
