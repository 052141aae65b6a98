"""2-D rotary positional encoding, DiM(pe_type="rope") (dimsum/pe/my_rotary.py:11-72): the (L, H) sin / cos tables and their application."""
import numpy as np

from ..ops import pos_embed


def get_1d_sincos_rotary_embed_from_grid(embed_dim, pos):
    """pos (M,) -> sin, cos (M, embed_dim / 2) of pos * omega_d, omega_d = 10000^(-d / (embed_dim / 2)), in float64"""
    assert embed_dim % 2 == 0
    omega = 1.0 / 10000 ** (np.arange(embed_dim // 2, dtype=np.float64) / (embed_dim / 2.0))
    out = np.einsum("m,d->md", pos.reshape(-1), omega)
    return np.sin(out), np.cos(out)


def get_2d_sincos_rotary_embed(embed_dim, grid_size, cls_token=False, extra_tokens=0):
    """-> (sin, cos), each (grid_size^2, embed_dim) float64: the first half of the channels encodes the first axis of the w-first meshgrid, the
    second half the other, and every frequency covers the channel pair (2i, 2i + 1) it rotates"""
    assert embed_dim % 2 == 0
    g = np.arange(grid_size, dtype=np.float32)
    grid = np.stack(np.meshgrid(g, g), axis=0).reshape(2, 1, grid_size, grid_size)          # w first
    halves = [get_1d_sincos_rotary_embed_from_grid(embed_dim // 2, grid[a]) for a in (0, 1)]
    sin, cos = (np.concatenate([halves[0][k], halves[1][k]], axis=1).repeat(2, axis=1) for k in (0, 1))
    return sin, cos


def apply_rotary(x, emb_sin, emb_cos):
    """x cos + rotate_half(x) sin on (B, L, C) tokens: one HIP launch, forward and backward"""
    return pos_embed.rotary(x, emb_sin, emb_cos)
