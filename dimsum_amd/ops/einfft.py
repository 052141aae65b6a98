"""The spectral branch of block type "combined_einfft" as ONE autograd operator on (batch, N tokens, C channels) float32 tensors:

  einfft(x, w1, b1, w2, b2, lam)    Re ifft2( softshrink( relu(fft2(x) W1 + b1) W2 + b2, lam ) )      (dimsum/models_dim.py:739-775)

fft2 / ifft2 run over (the N tokens, the 4 channel blocks of bs = C / 4 columns), ortho-normalised; W1, W2 are block-diagonal complex
(bs, bs) matrices per channel block, ReLU and softshrink act on the real and the imaginary part separately.

The forward is THREE HIP launches (csrc/einfft.hip through dimsum_amd.native): dft -> mlp -> idft_real. The transform matrix is symmetric and
unitary, so each transform pass is the other's transpose and the backward is dft(dy) -> mlp_bwd -> idft_real, three launches again (plus the
transposes of the two weight tensors); the parameter gradients are torch.bmm products of the plane pairs the mlp backward writes, the bias
gradients their column sums. Kept for the backward: the spectrum planes (re, im) and the MLP's output planes (zr, zi) -- 4 x B N C x 4 bytes
 -- and the four parameters.
The torch expression at the end documents the math and serves the tests; the model never calls it."""
import torch
import torch.nn.functional as F

from .. import native


def _planes_t(p, bs):
    """(B, N, C) plane -> (4, bs, B N): block k's columns as the rows of a matrix (a view)"""
    return p.view(-1, 4, bs).permute(1, 2, 0)


def _planes(p, bs):
    """(B, N, C) plane -> (4, B N, bs) (a view)"""
    return p.view(-1, 4, bs).permute(1, 0, 2)


def _complex_weight_grad(a, g, bs):
    """d (2, 4, bs, bs) of out = a W in complex arithmetic, from the plane pairs a = (ar, ai), g = (gr, gi):
    dWr = ar^T gr + ai^T gi, dWi = ar^T gi - ai^T gr, per block"""
    (ar, ai), (gr, gi) = a, g
    art, ait, grp, gip = _planes_t(ar, bs), _planes_t(ai, bs), _planes(gr, bs), _planes(gi, bs)
    return torch.stack((torch.baddbmm(torch.bmm(art, grp), ait, gip), torch.baddbmm(torch.bmm(art, gip), ait, grp, alpha=-1.0)))


def _complex_bias_grad(g, bs):
    return torch.stack((g[0].view(-1, 4, bs).sum(0), g[1].view(-1, 4, bs).sum(0)))


class _EinFFTFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, lam):
        re, im = native.einfft_dft(x)
        zr, zi = native.einfft_mlp_fwd(re, im, w1, b1, w2, b2, lam)
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(re, im, zr, zi, w1, b1, w2, b2)
            ctx.lam = lam
        return native.einfft_idft_real(zr, zi)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        re, im, zr, zi, w1, b1, w2, b2 = ctx.saved_tensors
        bs = re.shape[-1] // 4
        dzr, dzi = native.einfft_dft(dy)
        dxr, dxi, h1, dz2, dp1 = native.einfft_mlp_bwd(dzr, dzi, re, im, zr, zi, w1, b1, w2, b2, ctx.lam)
        dx = native.einfft_idft_real(dxr, dxi) if ctx.needs_input_grad[0] else None
        dw1 = _complex_weight_grad((re, im), dp1, bs) if ctx.needs_input_grad[1] else None
        db1 = _complex_bias_grad(dp1, bs) if ctx.needs_input_grad[2] else None
        dw2 = _complex_weight_grad(h1, dz2, bs) if ctx.needs_input_grad[3] else None
        db2 = _complex_bias_grad(dz2, bs) if ctx.needs_input_grad[4] else None
        return dx, dw1, db1, dw2, db2, None


def einfft(x, w1, b1, w2, b2, lam=0.01):
    """x: (B, N, C) float32 (a channel-half view is read in place); w1, w2: (2, 4, C/4, C/4) = [re | im][block][in][out]; b1, b2: (2, 4, C/4)"""
    return _EinFFTFn.apply(x, w1, b1, w2, b2, float(lam))


# ---- the same maps as torch expressions (documentation, tests) ---------------------------------------------------------------------------------
def dft_torch(x):
    """-> (re, im) of fft2 over (tokens, the 4 channel blocks), ortho-normalised"""
    B, N, C = x.shape
    s = torch.fft.fft2(x.reshape(B, N, 4, C // 4), dim=(1, 2), norm="ortho")
    return s.real.reshape(B, N, C), s.imag.reshape(B, N, C)


def idft_real_torch(re, im):
    B, N, C = re.shape
    return torch.fft.ifft2(torch.complex(re, im).reshape(B, N, 4, C // 4), dim=(1, 2), norm="ortho").real.reshape(B, N, C)


def _cmul_torch(xr, xi, w, b):
    mul = lambda t, m: torch.einsum("...bd,bdk->...bk", t, m)
    return mul(xr, w[0]) - mul(xi, w[1]) + b[0], mul(xr, w[1]) + mul(xi, w[0]) + b[1]


def mlp_torch(re, im, w1, b1, w2, b2, lam):
    """-> (zr, zi, (h1r, h1i)): the block-diagonal complex MLP on (B, N, C) planes"""
    B, N, C = re.shape
    xr, xi = re.reshape(B, N, 4, C // 4), im.reshape(B, N, 4, C // 4)
    pr, pi = _cmul_torch(xr, xi, w1, b1)
    hr, hi = F.relu(pr), F.relu(pi)
    qr, qi = _cmul_torch(hr, hi, w2, b2)
    zr, zi = (F.softshrink(q, lam) if lam else q for q in (qr, qi))
    return zr.reshape(B, N, C), zi.reshape(B, N, C), (hr.reshape(B, N, C), hi.reshape(B, N, C))


def einfft_torch(x, w1, b1, w2, b2, lam=0.01):
    re, im = dft_torch(x)
    zr, zi, _ = mlp_torch(re, im, w1, b1, w2, b2, lam)
    return idft_real_torch(zr, zi)
