"""Conditional positional encoding, DiM(pe_type="cpe") (dimsum/pe/cpe.py:8-51): a depthwise 3x3 convolution over the token grid with a
skip connection, in AdaInPosCNN followed by a LayerNorm and an adaLN modulation -- same module tree and state_dict keys, one HIP pass."""
import torch
import torch.nn as nn

from ..ops import pos_embed


def _conv(in_chans, embed_dim, s):
    if s != 1 or in_chans != embed_dim:
        raise NotImplementedError("the positional convolution is implemented for stride 1 and in_chans == embed_dim (all the reference builds)")
    return nn.Sequential(nn.Conv2d(in_chans, embed_dim, 3, s, 1, bias=True, groups=embed_dim))


class PosCNN(nn.Module):
    """conv3x3_depthwise(x) + x on the token grid, no norm (dimsum/pe/cpe.py:8-26). The reference's DiM never builds it; it is here for its
    module tree and state_dict keys, and its forward raises: the HIP pass is AdaInPosCNN's, which does not stop before the LayerNorm."""

    def __init__(self, in_chans, embed_dim=768, s=1):
        super().__init__()
        self.proj = _conv(in_chans, embed_dim, s)
        self.s = s

    def forward(self, x, H, W):
        raise NotImplementedError("PosCNN without the LayerNorm has no HIP pass (DiM only builds AdaInPosCNN)")

    def no_weight_decay(self):
        return ["proj.%d.weight" % i for i in range(4)]


class AdaInPosCNN(nn.Module):
    def __init__(self, in_chans, embed_dim=768, s=1):
        super().__init__()
        self.proj = _conv(in_chans, embed_dim, s)
        self.adaLN_modulation = nn.Sequential(nn.SiLU(), nn.Linear(embed_dim, 2 * embed_dim, bias=True))
        self.norm = nn.LayerNorm(embed_dim)
        self.s = s

    def forward(self, x, c, H, W):
        from ..models_dim import _modulation
        if H != W:
            raise NotImplementedError("non-square token grids are out of scope")
        conv = self.proj[0]
        return pos_embed.cpe(x, conv.weight, conv.bias, self.norm.weight, self.norm.bias, _modulation(self.adaLN_modulation, c), H, self.norm.eps)

    def no_weight_decay(self):
        return ["proj.%d.weight" % i for i in range(4)]
