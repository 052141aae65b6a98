"""DCT blur of the data end of the path (DCTBlur, dimsum/transport/path.py:249-259): every p x p tile X of every channel becomes
C^T (G_b o (C X C^T)) C, with C the orthonormal p-point DCT-II matrix and the per-sample gain
G_b[i, j] = exp(-(f_i^2 + f_j^2) blur_sigma_b^2 / 2) (1 - min_scale) + min_scale, f_k = pi k / p.
The reference reaches the same numbers through an FFT-based DCT; this is the matrix form, written out: on CUDA fp32 tensors one HIP launch
(dimsum_fm_plan, one tile per lane), everywhere else the torch expression below."""
import math

import torch as th


def dct_matrix(p, dtype=th.float32, device=None):
    """C[k, n] = s_k cos(pi (2 n + 1) k / (2 p)), s_0 = sqrt(1 / p), s_k = sqrt(2 / p): C C^T = I. Built in float64, then rounded."""
    k = th.arange(p, dtype=th.float64).view(p, 1)
    n = th.arange(p, dtype=th.float64).view(1, p)
    c = math.sqrt(2.0 / p) * th.cos(math.pi * (2 * n + 1) * k / (2 * p))
    c[0] = math.sqrt(1.0 / p)
    return c.to(dtype=dtype, device=device)


def check_blur_shape(x, patch_size):
    """the reference breaks on these with a broadcasting error somewhere inside its rearrange"""
    if x.dim() != 4:
        raise ValueError(f"dct_blur: x is (B, C, H, W), got {tuple(x.shape)}")
    H, W = x.shape[-2:]
    if patch_size < 1 or H != W or H < patch_size or H % patch_size != 0:
        raise ValueError(f"dct_blur: square images whose side is a multiple of the patch size {patch_size} are required, got {H} x {W}")


def blur_times(x, blur_sigmas):
    """per-sample blur_sigma^2 / 2 as a (B,) tensor of x's dtype and device; blur_sigmas: a number, or B values in any shape"""
    s = th.as_tensor(blur_sigmas).to(device=x.device, dtype=x.dtype).reshape(-1)
    if s.numel() not in (1, x.shape[0]):
        raise ValueError(f"dct_blur: one blur sigma, or one per sample, got {s.numel()} for a batch of {x.shape[0]}")
    return (s ** 2 / 2).expand(x.shape[0])


def dct_blur_torch(x, patch_size, blur_t, min_scale=1e-3):
    """the matrix form as torch operations in x's dtype; blur_t: (B,) = blur_sigma^2 / 2"""
    B, C, H, W = x.shape
    p = patch_size
    cm = dct_matrix(p, x.dtype, x.device)
    f = math.pi * th.arange(p, dtype=x.dtype, device=x.device) / p
    f2 = f[:, None] ** 2 + f[None, :] ** 2
    gain = th.exp(-f2 * blur_t.view(B, 1, 1, 1, 1, 1)) * (1 - min_scale) + min_scale               # (B, 1, 1, 1, p, p)
    tiles = x.reshape(B, C, H // p, p, W // p, p).permute(0, 1, 2, 4, 3, 5)                         # (B, C, H/p, W/p, p, p)
    coefs = (cm @ tiles @ cm.t()) * gain
    return (cm.t() @ coefs @ cm).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H, W)


def dct_blur(x, patch_size, blur_sigmas, min_scale=1e-3):
    """x: (B, C, H, H) with H a multiple of patch_size; blur_sigmas: per-sample standard deviations of the blur (0 returns x up to rounding).
    CUDA: the HIP kernel, float32 and patch_size in {2, 4, 8}; anything else raises RuntimeError (there is no torch path behind it).
    CPU: the torch expression."""
    check_blur_shape(x, patch_size)
    blur_t = blur_times(x, blur_sigmas)
    if x.is_cuda:
        from .. import native
        if patch_size not in native.FM_PATCHES or x.dtype != th.float32:
            raise RuntimeError(f"dct_blur: no HIP kernel for patch size {patch_size} / {x.dtype} (instantiated for float32 and patch sizes "
                               f"{native.FM_PATCHES}) and no torch path on CUDA")
        zero, one = th.zeros_like(blur_t), th.ones_like(blur_t)
        return native.fm_plan(x, None, th.stack([one, zero, zero, zero, blur_t]), patch_size, min_scale, need_ut=False)[0]
    return dct_blur_torch(x, patch_size, blur_t, min_scale)
