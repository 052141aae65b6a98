"""SwitchMLP: the top-1 mixture-of-experts layer, with the reference's constructor, parameter names and semantics (dimsum/switch_mlp.py):
`router` (Linear(dim, E), with bias) and `local_experts.{i}.linear_fc1 / linear_fc2` (mlp.MLP). Per token: route = sigmoid(logits) for
routing_mode == "sinkhorn", softmax(logits, 1) for every other value; (p, e) = max(route, 1) (the first maximum on ties);
out = p * expert_e(x). The forward is ONE autograd function over fused HIP routing passes and per-expert GEMMs on contiguous row slices
(ops/moe.py, csrc/moe.hip) with one host read of E + 1 ints, where the reference runs E nonzero() synchronisations, E gathers and E scatters.
With `grouped=True` (or DIMSUM_MOE_GROUPED=1 at construction; `set_grouped(model, True)` on a built model) a call that does not train runs the
experts as ONE grouped GEMM launch per projection that reads the offsets on the device (csrc/moe_gemm.hip): no host read at all, which is what lets
hip_graph.GraphedForward capture an is_moe model. Off by default; a call that trains always takes the autograd function above.
With `grouped_train=True` (or DIMSUM_MOE_GROUPED_TRAIN=1 at construction; `set_grouped_train(model, True)` on a built model) a call that TRAINS
runs on the grouped GEMM too, with its data and weight gradients in the backward (csrc/moe_gemm_bwd.hip): a training step then has no host read in
any SwitchMLP. Off by default and independent of `grouped`.
`sinkhorn` is ported for API parity: the reference's forward never calls it."""
import os

import torch
import torch.nn as nn

from . import native
from .mlp import MLP
from .ops.moe import switch_mlp_fn


def sinkhorn(cost, tol=0.0001):
    """Sinkhorn normalisation of exp(2 cost) towards uniform row and column sums: alternate row / column scalings until the column scaling moves
    by less than `tol` on average (switch_mlp.py:6-21, the same arithmetic in the same order) -> cols * exp(2 cost) * rows"""
    k = torch.exp(2.0 * cost)
    n_rows, n_cols = k.size(0), k.size(1)
    rows = torch.ones(n_rows, device=k.device, dtype=k.dtype)
    cols = 1 / (n_cols * torch.sum(k, 0))
    err = 1e9
    while err > tol:
        rows = (1 / n_rows) * 1 / (torch.sum(cols * k, 1) + 1e-8)
        moved = (1 / n_cols) * 1 / (torch.sum(rows.unsqueeze(1) * k, 0) + 1e-8)
        err = torch.mean(torch.abs(cols - moved))
        cols = moved
    return cols * k * rows.unsqueeze(1)


class SwitchMLP(nn.Module):
    """Top-1 mixture of experts: routes every token to one of E MLP experts"""

    def __init__(self, dim, layer_idx=None, mamba_moe_layers=None, num_moe_experts=None, add_bias_linear=False, gated_linear_unit=True,
                 routing_mode="top1", grouped=None, grouped_train=None):
        super().__init__()
        self.layer = layer_idx
        if mamba_moe_layers:            # (the last character of the layer's entry: switch_mlp.py:43-44)
            self.num_moe_experts = int(mamba_moe_layers[layer_idx - 1][-1])
        else:
            self.num_moe_experts = num_moe_experts
        if not 1 <= int(self.num_moe_experts) <= 64:
            raise NotImplementedError(f"SwitchMLP: 1 <= experts <= 64 (got {self.num_moe_experts})")
        if dim % 4 != 0:
            raise NotImplementedError(f"SwitchMLP: dim must be a multiple of 4 (got {dim})")
        self.router = nn.Linear(dim, self.num_moe_experts)
        self.routing = routing_mode
        self.route_algo = sinkhorn
        self.router_activation = torch.sigmoid
        self.gated_linear_unit = gated_linear_unit
        self.num_local_experts = self.num_moe_experts
        self.local_expert_indices = list(range(self.num_local_experts))
        self.local_experts = nn.ModuleList(
            MLP(dim, add_bias_linear=add_bias_linear, gated_linear_unit=gated_linear_unit, is_expert=True, layer_idx=layer_idx)
            for _ in range(self.num_local_experts))
        self.grouped = False
        self.set_grouped(os.environ.get("DIMSUM_MOE_GROUPED") == "1" if grouped is None else grouped)
        self.grouped_train = False
        self.set_grouped_train(os.environ.get("DIMSUM_MOE_GROUPED_TRAIN") == "1" if grouped_train is None else grouped_train)

    def check_grouped(self):
        """raises when the grouped expert GEMM does not serve this layer's widths (refused, not emulated)"""
        for w in (self.local_experts[0].linear_fc1.weight, self.local_experts[0].linear_fc2.weight):
            if not native.moe_gemm_serves(w.shape[1], w.shape[0], self.num_local_experts):
                raise NotImplementedError(f"SwitchMLP(grouped=True): the grouped GEMM serves widths that are multiples of 32 (an expert projection "
                                          f"is {w.shape[1]} -> {w.shape[0]}); there is no fallback")

    def set_grouped_train(self, on):
        """serve the calls that train from the grouped expert GEMM and its two gradients (no host read forward or backward)"""
        if on:                              # the backward's four products run over the forward's two width pairs: what check_grouped passes they serve
            self.check_grouped()
        self.grouped_train = bool(on)

    def set_grouped(self, on):
        """serve the calls that do not train from the grouped expert GEMM (no host read of the expert offsets)"""
        if on:
            self.check_grouped()
        self.grouped = bool(on)

    def gather_indices(self, local_indices):
        return local_indices

    def forward(self, hidden_states, inference_params=None):
        ex = self.local_experts
        biased = ex[0].linear_fc1.bias is not None
        return switch_mlp_fn(hidden_states, self.router.weight, self.router.bias, [m.linear_fc1.weight for m in ex], [m.linear_fc2.weight for m in ex],
                             [m.linear_fc1.bias for m in ex] if biased else None, [m.linear_fc2.bias for m in ex] if biased else None,
                             routing_mode=self.routing, gated=self.gated_linear_unit, grouped=self.grouped, grouped_train=self.grouped_train)


def set_grouped(model, on=True):
    """flips `grouped` on every SwitchMLP of a built model -> the number of layers touched"""
    layers = [m for m in model.modules() if isinstance(m, SwitchMLP)]
    if on:                                  # every layer is checked before any is flipped: a refusal leaves the model as it was
        for m in layers:
            m.check_grouped()
    for m in layers:
        m.set_grouped(on)
    return len(layers)


def set_grouped_train(model, on=True):
    """flips `grouped_train` on every SwitchMLP of a built model -> the number of layers touched"""
    layers = [m for m in model.modules() if isinstance(m, SwitchMLP)]
    if on:                                  # every layer is checked before any is flipped: a refusal leaves the model as it was
        for m in layers:
            m.check_grouped()
    for m in layers:
        m.set_grouped_train(on)
    return len(layers)
