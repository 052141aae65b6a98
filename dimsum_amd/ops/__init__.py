"""Operator API of the hot path (same names as the reference's Python op modules)."""
from .causal_conv1d_interface import (  # noqa: F401
    causal_conv1d_chunk,
    causal_conv1d_chunk_torch,
    causal_conv1d_fn,
    causal_conv1d_update,
    causal_conv1d_update_torch,
    causal_conv1d_varlen_torch,
)
from .cross_entropy import CrossEntropyLoss, cross_entropy_loss, cross_entropy_torch, linear_cross_entropy  # noqa: F401
from .layernorm import RMSNorm, layer_norm_fn, rms_norm_fn  # noqa: F401
from .moe import moe_act, moe_act_torch, switch_mlp_fn, switch_mlp_torch  # noqa: F401
from .selective_scan_interface import (  # noqa: F401
    bimamba_inner_fn,
    mamba_inner_fn,
    mamba_inner_fn_cond,
    mamba_inner_fn_no_out_proj,
    mamba_inner_fn_no_out_proj_cond,
    selective_scan_fn,
    selective_scan_varlen_torch,
)
from .selective_state_update import selective_scan_carry_torch, selective_state_update, selective_state_update_torch  # noqa: F401
from .state_copy import state_copy_slots_torch, state_pool_table_torch  # noqa: F401
