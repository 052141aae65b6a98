"""DiT baseline -- same module tree, constructor flags and state_dict keys as dimsum/models_dit.py (DiT :152-297, DiTBlock :112-131, zoo
:354-415), composed from the pieces models_dim.py already runs on the HIP operators: the embedders, FinalLayer, the fixed sin-cos table and
DiTBlock (the block DiM shares every k layers), here with the plain Mlp (mlp.py: bias + tanh-GELU as one HIP pass / GEMM epilogue) and the
model's own head count. The block's key names equal the reference's (norm1 / norm2 carry no parameters; attn.qkv, attn.proj, mlp.fc1, mlp.fc2,
adaLN_modulation.1), so there is no subclass.

What is structured differently (results equal to fp32 roundoff): the forward goes through gemm.forward_scope (one weight-image launch per
inference forward under the scaled-fp16 policy) and shares SiLU(c) among the adaLN heads, like DiM.forward. Gradient checkpointing
(`set_gradient_checkpointing`) wraps each block in torch.utils.checkpoint as the reference does.

The constructor takes the upstream DiT names (`input_size`, `class_dropout_prob`) and, as aliases, the ones the reference's create_model.py
passes (`img_resolution`, `label_dropout`)."""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import gemm
from .models_dim import DiTBlock, FinalLayer, LabelEmbedder, PatchEmbed, TimestepEmbedder, get_2d_sincos_pos_embed


class DiT(nn.Module):
    def __init__(self, input_size=32, patch_size=2, in_channels=4, hidden_size=1152, depth=28, num_heads=16, mlp_ratio=4.0,
                 class_dropout_prob=0.1, num_classes=1000, learn_sigma=False, img_resolution=None, label_dropout=None):
        super().__init__()
        input_size = input_size if img_resolution is None else img_resolution
        class_dropout_prob = class_dropout_prob if label_dropout is None else label_dropout
        self.learn_sigma, self.in_channels = learn_sigma, in_channels
        self.out_channels = in_channels * 2 if learn_sigma else in_channels
        self.patch_size, self.num_heads, self.num_classes = patch_size, num_heads, num_classes
        self.enable_gradient_checkpointing = False
        self.x_embedder = PatchEmbed(input_size, patch_size, in_channels, hidden_size, bias=True)
        self.t_embedder = TimestepEmbedder(hidden_size)
        self.y_embedder = LabelEmbedder(num_classes, hidden_size, class_dropout_prob)
        self.pos_embed = nn.Parameter(torch.zeros(1, self.x_embedder.num_patches, hidden_size), requires_grad=False)     # fixed sin-cos table
        self.blocks = nn.ModuleList([DiTBlock(hidden_size, num_heads, mlp_ratio=mlp_ratio, use_gated_mlp=False) for _ in range(depth)])
        self.final_layer = FinalLayer(hidden_size, patch_size, self.out_channels)
        self.initialize_weights()

    def set_gradient_checkpointing(self):
        self.enable_gradient_checkpointing = True

    def initialize_weights(self):
        """models_dit.py:193-228 (adaLN-zero: a freshly initialised model outputs exactly 0). Order matters: the Xavier pass over every Linear
        first, the special cases after it."""
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.xavier_uniform_(m.weight)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
        pe = get_2d_sincos_pos_embed(self.pos_embed.shape[-1], int(self.x_embedder.num_patches ** 0.5))
        self.pos_embed.data.copy_(torch.from_numpy(pe).float().unsqueeze(0))
        w = self.x_embedder.proj.weight.data            # the patch Conv2d like the Linear it is
        nn.init.xavier_uniform_(w.view([w.shape[0], -1]))
        nn.init.zeros_(self.x_embedder.proj.bias)
        nn.init.normal_(self.y_embedder.embedding_table.weight, std=0.02)
        for lin in (self.t_embedder.mlp[0], self.t_embedder.mlp[2]):
            nn.init.normal_(lin.weight, std=0.02)
        zeroed = [blk.adaLN_modulation[-1] for blk in self.blocks] + [self.final_layer.adaLN_modulation[-1], self.final_layer.linear]
        for lin in zeroed:
            nn.init.zeros_(lin.weight)
            nn.init.zeros_(lin.bias)

    def unpatchify(self, x):
        c, p = self.out_channels, self.x_embedder.patch_size[0]
        h = w = int(x.shape[1] ** 0.5)
        assert h * w == x.shape[1]
        x = x.reshape(x.shape[0], h, w, p, p, c)
        return torch.einsum("nhwpqc->nchpwq", x).reshape(x.shape[0], c, h * p, h * p)

    def forward(self, x, t, y=None, **kwargs):
        """x: (N, C, H, W) latents, t: (N,) times, y: (N,) labels (None: the null class) -> (N, out_channels, H, W)."""
        if y is None:
            y = torch.ones(x.size(0), dtype=torch.long, device=x.device) * (self.y_embedder.get_in_channels() - 1)
        with gemm.forward_scope(self, x.shape[0] * self.x_embedder.num_patches):     # (inference under the scaled-fp16 policy: one weight-image launch)
            c = self.t_embedder(t) + self.y_embedder(y, self.training)
            gemm._tls.cond = (c, F.silu(c)) if os.environ.get("DIMSUM_FORWARD_MEMO", "1") != "0" else None      # (the adaLN heads' shared SiLU(c))
            try:
                return self._forward_blocks(x, c)
            finally:
                gemm._tls.cond = None

    def _forward_blocks(self, x, c):
        x = self.x_embedder(x) + self.pos_embed
        for block in self.blocks:
            if self.enable_gradient_checkpointing and torch.is_grad_enabled():
                x = torch.utils.checkpoint.checkpoint(block, x, c, use_reentrant=False)
            else:
                x = block(x, c)
        return self.unpatchify(self.final_layer(x, c))

    def forward_with_cfg(self, x, t, y=None, cfg_scale=1.0, **kwargs):
        """classifier-free guidance on a [cond | uncond] batch (models_dit.py:274-290), guidance on the first in_channels channels."""
        half = x[: len(x) // 2]
        out = self.forward(torch.cat([half, half], dim=0), t, y)
        eps, rest = out[:, : self.in_channels], out[:, self.in_channels:]
        cond, uncond = torch.split(eps, len(eps) // 2, dim=0)
        g = uncond + cfg_scale * (cond - uncond)
        return torch.cat([torch.cat([g, g], dim=0), rest], dim=1)


def _zoo(depth, hidden_size, patch_size, num_heads):
    def make(**kwargs):
        return DiT(depth=depth, hidden_size=hidden_size, patch_size=patch_size, num_heads=num_heads, **kwargs)
    return make


_SIZES = {"XL": (28, 1152, 16), "L": (24, 1024, 16), "B": (12, 768, 12), "S": (12, 384, 6)}        # depth, width, heads (head_dim 72 / 64 / 64 / 64)
DiT_models = {f"DiT-{size}/{patch}": _zoo(depth, width, patch, heads) for size, (depth, width, heads) in _SIZES.items() for patch in (2, 4, 8)}
