"""Mamba / CondMamba mixers -- same constructor arguments, parameter names (state_dict keys) and forward contract as
mamba/mamba_ssm/modules/mamba_simple.py (Mamba :42-297, CondMamba :438-701), running on the HIP operators of
dimsum_amd.ops, including the recurrent form (`allocate_inference_cache`, `forward(inference_params=...)`, `step`: :299-380, :703-784).

The recurrent form: `forward(x, inference_params=p)` at `p.seqlen_offset == 0` processes a prompt on the fused path and leaves the layer's
(conv_state, ssm_state) in `p.key_value_memory_dict[layer_idx]`; at `seqlen_offset > 0` it is one `step` (one token) on those states, which
the two kernels of csrc/mixer_step.hip update in place. The caller advances `seqlen_offset`, as with the reference. One deliberate difference:
a prompt shorter than d_conv leaves its tokens zero-padded on the left in conv_state (what a causal conv sees before the first token; upstream
Mamba pads the same way) where the reference's `conv_state.copy_(x[:, :, -d_conv:])` (:258) raises a shape error. Refused, with the reason in
the message: scan_type "v2" (the backward-direction twin has no causal recurrence), the zigzag scan types (a permuted sequence has no
token-by-token order) and the operand-image input `x3` (inference images and a cache do not combine). A cached sequence is continued by
more than one token per call through `extend` (a causal conv and a scan that enter with the cache's states and leave the new ones behind;
`dimsum_amd.utils.chunked_prefill` walks a long prompt with it); `step` and `forward` at `seqlen_offset > 0` keep taking one token. The
recurrent form is for inference: the cache is filled without autograd edges and the step and extend kernels have no backward.
Packed rows: `Mamba.forward(..., seq_idx=ids)` with ids (B, L) int32 keeps the sequences of one row apart (ops/selective_scan_interface.py: the
packed-row route of mamba_inner_fn). With a cache at `seqlen_offset == 0` the states left behind are those of every row's LAST segment: ssm_state
its final state, conv_state its last inputs with whatever belongs to an earlier segment zeroed -- so a prompt left-padded with its padding as a
segment of its own prefills as if it stood alone. Refused with seq_idx: scan types other than "none", `x3`, CondMamba's cond, `seqlen_offset > 0`.
`Block` (mamba_simple.py:383-436) wraps a mixer with its add + norm; for one token of a cached sequence it runs the mixer's `step_fused`: the
same step on the weight-streaming kernel of csrc/decode_step.hip, four launches per layer.

Differences that do not change results:
  * `cond_proj(c)` is numerically dead in the reference (its output only donates a buffer to the conv kernel,
    causal_conv1d.cpp:326-329). The parameter is kept (checkpoint compatibility); under grad mode its (batch, d_inner)
    output is threaded through the autograd Function so the graph has the same edges (and the same `None` gradient),
    but the (batch, d_inner, seqlen) expand+copy of mamba_simple.py:589 -- 268 MB per call at DiM-L/2, batch 256 --
    is never materialised.
  * the zigzag gather / inverse gather (mamba_simple.py:627-657) are index_selects on the token axis.
"""
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import gemm, native
from ..ops.causal_conv1d_interface import causal_conv1d_update
from ..ops.layernorm import RMSNorm, layer_norm_fn
from ..ops.selective_scan_interface import (mamba_inner_fn_cond, mamba_inner_fn_no_out_proj_cond)
from ..ops.selective_state_update import selective_state_update

_ZIGZAG = ("zigma", "sweep", "jpeg")


def fused_decode_enabled(batch, dtype):
    """DIMSUM_FUSED_DECODE, read at call time: 0 sends every decode step through the unfused `step`, 1 takes the fused step wherever it serves
    (tests and tools/bench_decode.py run both); unset: where it measured faster than the unfused step eager AND replayed from a graph
    (DESIGN.md section 3.16): float32 at batch <= 4"""
    v = os.environ.get("DIMSUM_FUSED_DECODE", "")
    if v in ("0", "1"):
        return v == "1"
    return dtype == torch.float32 and batch <= 4


class _MambaBase(nn.Module):
    def __init__(self, d_model, d_state=16, d_conv=4, expand=2, dt_rank="auto", dt_min=0.001, dt_max=0.1,
                 dt_init="random", dt_scale=1.0, dt_init_floor=1e-4, conv_bias=True, bias=False, use_fast_path=True,
                 layer_idx=None, device=None, dtype=None, scan_type="none", d_cond=None, **kwargs):
        fk = {"device": device, "dtype": dtype}
        super().__init__()
        self.d_model, self.d_state, self.d_conv, self.expand = d_model, d_state, d_conv, expand
        self.d_inner = int(expand * d_model)
        self.dt_rank = math.ceil(d_model / 16) if dt_rank == "auto" else dt_rank
        self.use_fast_path, self.layer_idx, self.scan_type, self.d_cond = use_fast_path, layer_idx, scan_type, d_cond

        self.in_proj = nn.Linear(d_model, self.d_inner * 2, bias=bias, **fk)
        self.conv1d = nn.Conv1d(self.d_inner, self.d_inner, bias=conv_bias, kernel_size=d_conv, groups=self.d_inner,
                                padding=d_conv - 1, **fk)
        self.activation = "silu"
        self.act = nn.SiLU()
        self.x_proj = nn.Linear(self.d_inner, self.dt_rank + d_state * 2, bias=False, **fk)
        self.dt_proj = nn.Linear(self.dt_rank, self.d_inner, bias=True, **fk)
        if d_cond is not None:
            self.cond_proj = nn.Linear(d_cond, self.d_inner, bias=True, **fk)
        self._init_dt(self.dt_proj, dt_init, dt_scale, dt_min, dt_max, dt_init_floor, fk)
        self.A_log = self._s4d_real(device)
        self.D = nn.Parameter(torch.ones(self.d_inner, device=device))
        self.D._no_weight_decay = True
        if scan_type == "v2":       # bidirectional twin (mamba_simple.py:529-553)
            self.A_b_log = self._s4d_real(device)
            self.conv1d_b = nn.Conv1d(self.d_inner, self.d_inner, bias=conv_bias, kernel_size=d_conv, groups=self.d_inner,
                                      padding=d_conv - 1, **fk)
            self.x_proj_b = nn.Linear(self.d_inner, self.dt_rank + d_state * 2, bias=False, **fk)
            self.dt_proj_b = nn.Linear(self.dt_rank, self.d_inner, bias=True, **fk)
            self._init_dt(self.dt_proj_b, dt_init, dt_scale, dt_min, dt_max, dt_init_floor, fk)
            self.D_b = nn.Parameter(torch.ones(self.d_inner, device=device))
            self.D_b._no_weight_decay = True
        else:
            self.A_b_log = self.conv1d_b = self.x_proj_b = self.dt_proj_b = self.D_b = None
        self.out_proj = nn.Linear(self.d_inner, d_model, bias=bias, **fk)
        self.register_buffer("zigzag_paths", kwargs.get("zigzag_paths", None))
        self.register_buffer("zigzag_paths_reverse", kwargs.get("zigzag_paths_reverse", None))

    def _s4d_real(self, device):
        A = torch.arange(1, self.d_state + 1, dtype=torch.float32, device=device).repeat(self.d_inner, 1).contiguous()
        p = nn.Parameter(torch.log(A))      # kept in fp32
        p._no_weight_decay = True
        return p

    def _init_dt(self, proj, dt_init, dt_scale, dt_min, dt_max, dt_init_floor, fk):
        """dt_proj initialised so that softplus(bias) is log-uniform in [dt_min, dt_max] (mamba_simple.py:494-512)."""
        std = self.dt_rank ** -0.5 * dt_scale
        if dt_init == "constant":
            nn.init.constant_(proj.weight, std)
        elif dt_init == "random":
            nn.init.uniform_(proj.weight, -std, std)
        else:
            raise NotImplementedError
        dt = torch.exp(torch.rand(self.d_inner, **fk) * (math.log(dt_max) - math.log(dt_min)) + math.log(dt_min))
        dt = dt.clamp(min=dt_init_floor)
        with torch.no_grad():
            proj.bias.copy_(dt + torch.log(-torch.expm1(-dt)))      # inverse softplus
        proj.bias._no_reinit = True

    def _is_zigzag(self):
        return self.scan_type.startswith(_ZIGZAG)

    def takes_image(self):
        """whether `x3` (the input as a split-bf16 operand image, gemm.py) can replace hidden_states: not when this mixer
        gathers its tokens itself"""
        return not (self._is_zigzag() and not getattr(self, "_zigzag_folded", False))

    def _refuse_seq_idx(self, seq_idx, hidden_states, cond, x3):
        if self.scan_type != "none":
            raise NotImplementedError(f'seq_idx with scan_type "{self.scan_type}" is not built: only the plain causal mixer ("none") has a '
                                      "packed-row form (the backward twin and the zigzag orders read a row in another order)")
        if x3 is not None:
            raise NotImplementedError("seq_idx with an operand-image input (x3) is not built: the in_proj + conv epilogue takes no sequence ids; "
                                      "pass hidden_states")
        if cond is not None:
            raise NotImplementedError("seq_idx with a conditional conv entry (cond) is not built")
        if not (torch.is_tensor(seq_idx) and seq_idx.dtype == torch.int32 and tuple(seq_idx.shape) == tuple(hidden_states.shape[:2])):
            raise ValueError(f"seq_idx must be an int32 (batch, seqlen) = {tuple(hidden_states.shape[:2])} tensor")

    def _mix(self, hidden_states, cond, x3=None, states=None, seq_idx=None, prefill_slots=None, prefill_starts=None):
        """states: the (conv_state, ssm_state) of an inference cache, filled from this call's sequence (forward(inference_params=...));
        seq_idx: packed rows (module docstring); prefill_slots (B, L) int32 with both: `states` are POOLS and the conv and scan kernels store
        every segment's states into the slot named at its last position (InferenceParams.prefill_slots) -- no torch op touches the states;
        prefill_starts (InferenceParams.prefill_starts) with those: segments that continue their slot's states -- one index_select takes the
        conv's carried inputs out of the pool (a snapshot: the conv may not read a slot it stores), the scan reads the SSM pool in place"""
        if prefill_starts is not None:
            self._refuse_prefill_starts(prefill_starts, prefill_slots, hidden_states)
        if prefill_slots is not None:
            self._refuse_prefill_slots(prefill_slots, hidden_states, cond, x3, states, seq_idx)
            prefill_slots = prefill_slots.contiguous()
        if seq_idx is not None:
            self._refuse_seq_idx(seq_idx, hidden_states, cond, x3)
            seq_idx = seq_idx.contiguous()
        bsz, L, _ = (hidden_states if x3 is None else x3).shape
        own_gather = self._is_zigzag() and not getattr(self, "_zigzag_folded", False)   # folded: the enclosing block's token
        if own_gather:                                                                  # tables already include the path
            assert x3 is None
            # xz[..., j] = xz[..., perm[j]]: permuting the columns of xz == permuting the tokens before in_proj
            hidden_states = hidden_states.index_select(1, self.zigzag_paths[self.layer_idx])
        # in_proj with the transpose fused: (2D, d_model) @ (d_model, B*L) viewed as (B, 2D, L) -- d-major, no copy
        conv_done = False
        if x3 is not None:
            # inference on operand images: where a 256-token tile of the GEMM holds whole sequences, the mixer's causal conv1d + SiLU runs in
            # in_proj's epilogue (csrc/gemm_nt_kernel.hpp, kEpiF32Conv): xz[:, :d_inner] then already IS the conv output and
            # mamba_inner_fn skips the conv kernel (one launch and a read + write of (b, d_inner, l) fp32 less per mixer)
            cw = self.conv1d.weight
            if (self.scan_type != "v2" and self.in_proj.bias is None and not torch.is_grad_enabled() and cond is None and cw.dtype == torch.float32
                    and self.d_inner % 256 == 0 and 256 % L == 0 and L % 4 == 0):
                xz, conv_done = gemm.matmul_wx_split3(self.in_proj.weight, x3.reshape(bsz * L, -1),
                                                      conv=(cw.reshape(cw.shape[0], cw.shape[-1]), self.conv1d.bias, L))
            else:
                xz = gemm.matmul_wx_split3(self.in_proj.weight, x3.reshape(bsz * L, -1))
            xz = xz.view(2 * self.d_inner, bsz, L).permute(1, 0, 2)
        else:
            xz = gemm.matmul_wx(self.in_proj.weight, hidden_states.reshape(bsz * L, -1).t()).view(2 * self.d_inner, bsz, L).permute(1, 0, 2)
        if self.in_proj.bias is not None:
            xz = xz + self.in_proj.bias.to(xz.dtype).view(1, -1, 1)
        if prefill_slots is not None and states[0].dtype != xz.dtype:
            raise NotImplementedError(f"prefill_slots: the conv pool is {states[0].dtype} but the activations are {xz.dtype}: the conv kernel moves "
                                      "x's elements into the pool, it does not convert them (allocate the pool in the activations' dtype)")
        if states is not None and prefill_slots is None:
            # the last d_conv inputs of the conv (mamba_simple.py:258), zero-padded on the left when the prompt is shorter (module docstring)
            xin = xz[:, :self.d_inner]
            with torch.no_grad():       # the cache is data for the next calls, never an autograd edge
                tail = xin[:, :, -self.d_conv:]
                if seq_idx is not None and L > 1:
                    # only the last segment's inputs: position p of the tail stays iff no boundary lies in (p, L - 1] (on the device: no host read)
                    ids = seq_idx[:, -self.d_conv:]
                    same = (ids[:, 1:] == ids[:, :-1]).flip(1).cumprod(1).flip(1).bool()
                    keep = torch.cat([same, same.new_ones(bsz, 1)], dim=1)
                    tail = torch.where(keep[:, None, :], tail, torch.zeros_like(tail))
                states[0].copy_(tail if L >= self.d_conv else F.pad(tail, (self.d_conv - L, 0)))
        # recomputed on every call (two tiny launches): a cached copy could not see in-place parameter updates made through
        # `.data` (EMA, load_state_dict), which do not bump the version counter, and would be frozen into a captured hipGraph
        A = gemm.neg_exp(self.A_log)
        if self.scan_type == "v2":
            A_b = gemm.neg_exp(self.A_b_log)
            out = mamba_inner_fn_no_out_proj_cond(xz, self.conv1d.weight, self.conv1d.bias, self.x_proj.weight,
                                                  self.dt_proj.weight, A, None, None, self.D.float(),
                                                  delta_bias=self.dt_proj.bias.float(), delta_softplus=True, init_states=cond)
            out_b = mamba_inner_fn_no_out_proj_cond(xz.flip([-1]), self.conv1d_b.weight, self.conv1d_b.bias,
                                                    self.x_proj_b.weight, self.dt_proj_b.weight, A_b, None, None,
                                                    self.D_b.float(), delta_bias=self.dt_proj_b.bias.float(),
                                                    delta_softplus=True, init_states=cond)
            y = (out + out_b.flip([-1])).transpose(1, 2)
            return nn.functional.linear(y, self.out_proj.weight, self.out_proj.bias)
        if prefill_slots is not None:
            starts = {}
            if prefill_starts is not None:
                with torch.no_grad():
                    snapshot = states[0].index_select(0, prefill_starts["start_list"])      # (S_in, d_inner, d_conv): start_rows index it by ordinal
                starts = dict(start_slots=prefill_starts["start_slots"].contiguous(), start_rows=prefill_starts["start_rows"].contiguous(),
                              conv_initial_states=snapshot)
            out = mamba_inner_fn_cond(xz, self.conv1d.weight, self.conv1d.bias, self.x_proj.weight, self.dt_proj.weight,
                                      self.out_proj.weight, self.out_proj.bias, A, None, None, self.D.float(),
                                      delta_bias=self.dt_proj.bias.float(), delta_softplus=True, seq_idx=seq_idx, end_slots=prefill_slots,
                                      conv_state=states[0], ssm_state=states[1], **starts)
            return out
        out = mamba_inner_fn_cond(xz, self.conv1d.weight, self.conv1d.bias, self.x_proj.weight, self.dt_proj.weight,
                                  self.out_proj.weight, self.out_proj.bias, A, None, None, self.D.float(),
                                  delta_bias=self.dt_proj.bias.float(), delta_softplus=True, init_states=cond, conv_done=conv_done,
                                  last_state=None if states is None else states[1], **({"seq_idx": seq_idx} if seq_idx is not None else {}))
        if own_gather:
            out = out.index_select(1, self.zigzag_paths_reverse[self.layer_idx])
        return out

    def _refuse_prefill_slots(self, prefill_slots, hidden_states, cond, x3, states, seq_idx):
        """what a packed prompt pass into slots is not built for, each with its reason; the VALUES of prefill_slots are never read"""
        if seq_idx is None:
            raise ValueError("prefill_slots without seq_idx: per-segment states belong to packed rows (pass seq_idx; one request alone is an "
                             "all-equal id row)")
        if self.scan_type == "v2" or self._is_zigzag():
            raise NotImplementedError(f'prefill_slots with scan_type "{self.scan_type}" is not built: only the plain causal mixer ("none") has '
                                      "states to leave behind")
        if cond is not None:
            raise NotImplementedError("prefill_slots with a conditional conv entry (cond) is not built")
        if x3 is not None:
            raise NotImplementedError("prefill_slots with an operand-image input (x3) is not built: pass hidden_states")
        if states is None:
            raise ValueError("prefill_slots need the pools of an inference cache (forward(inference_params=...))")
        if not (torch.is_tensor(prefill_slots) and prefill_slots.dtype == torch.int32 and tuple(prefill_slots.shape) == tuple(hidden_states.shape[:2])):
            raise ValueError(f"prefill_slots must be an int32 (batch, seqlen) = {tuple(hidden_states.shape[:2])} tensor")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError("prefill_slots is an inference argument: the pass that stores states has no backward; call it under "
                                      "torch.no_grad()")

    def _refuse_prefill_starts(self, prefill_starts, prefill_slots, hidden_states):
        """prefill_starts ride on prefill_slots (whose refusals -- v2 / zigzag, cond, x3, grad mode -- then apply as they are); the VALUES are
        never read"""
        if prefill_slots is None:
            raise ValueError("prefill_starts without prefill_slots: resumed segments belong to the packed prompt pass into slots (set "
                             "inference_params.prefill_slots and pass seq_idx)")
        shape = tuple(hidden_states.shape[:2])
        ok = isinstance(prefill_starts, dict) and all(torch.is_tensor(prefill_starts.get(k)) for k in ("start_slots", "start_rows", "start_list"))
        if not (ok and all(prefill_starts[k].dtype == torch.int32 and tuple(prefill_starts[k].shape) == shape for k in ("start_slots", "start_rows"))
                and prefill_starts["start_list"].dtype == torch.int64 and prefill_starts["start_list"].dim() == 1
                and prefill_starts["start_list"].numel() >= 1):
            raise ValueError(f"prefill_starts must hold start_slots and start_rows, int32 (batch, seqlen) = {shape}, and start_list, int64 with at "
                             "least one slot (plan_packed_prefill(resume=...))")

    # ---- the recurrent form (mamba_simple.py:299-380) ------------------------------------------------------------------------------------------
    def _refuse_recurrent(self, x3=None):
        if self.scan_type == "v2":
            raise NotImplementedError('scan_type "v2" cannot run token by token: its backward-direction twin reads the sequence from its end, '
                                      "which has no causal recurrence")
        if self._is_zigzag():
            raise NotImplementedError(f'scan_type "{self.scan_type}" cannot run token by token: the mixer scans a permuted sequence, which has '
                                      "no token-by-token order")
        if x3 is not None:
            raise NotImplementedError("inference_params with an operand-image input (x3): inference images and a state cache do not combine; "
                                      "pass hidden_states")

    def allocate_inference_cache(self, batch_size, max_seqlen, dtype=None, **kwargs):
        """-> zeroed (conv_state (batch, d_inner, d_conv), ssm_state (batch, d_inner, d_state)), as mamba_simple.py:346-353"""
        device = self.out_proj.weight.device
        conv_dtype = self.conv1d.weight.dtype if dtype is None else dtype
        ssm_dtype = self.dt_proj.weight.dtype if dtype is None else dtype
        return (torch.zeros(batch_size, self.d_inner, self.d_conv, device=device, dtype=conv_dtype),
                torch.zeros(batch_size, self.d_inner, self.d_state, device=device, dtype=ssm_dtype))

    def _get_states_from_cache(self, inference_params, batch_size, initialize_states=False):
        """this layer's (conv_state, ssm_state) in inference_params.key_value_memory_dict, created on first use (mamba_simple.py:355-380)"""
        assert self.layer_idx is not None
        if self.layer_idx not in inference_params.key_value_memory_dict:
            if getattr(inference_params, "state_indices", None) is not None:
                raise ValueError("state_indices need a pool of states in key_value_memory_dict (allocate_inference_cache(num_slots, ...)): a "
                                 "cache created on first use has one row per batch row, not one per slot")
            conv_state = torch.zeros(batch_size, self.d_inner, self.d_conv, device=self.conv1d.weight.device, dtype=self.conv1d.weight.dtype)
            ssm_state = torch.zeros(batch_size, self.d_inner, self.d_state, device=self.dt_proj.weight.device, dtype=self.dt_proj.weight.dtype)
            inference_params.key_value_memory_dict[self.layer_idx] = (conv_state, ssm_state)
        else:
            conv_state, ssm_state = inference_params.key_value_memory_dict[self.layer_idx]
            if initialize_states:
                conv_state.zero_()
                ssm_state.zero_()
        return conv_state, ssm_state

    def step(self, hidden_states, conv_state, ssm_state, state_indices=None):
        """one token: hidden_states (B, 1, d_model) -> (out (B, 1, d_model), conv_state, ssm_state), both states updated in place
        (mamba_simple.py:299-344): in_proj -> causal_conv1d_update -> x_proj -> selective_state_update -> out_proj.
        state_indices (B,) int32: the states are pools (num_slots, ...) and row b works on slot state_indices[b] (InferenceParams)"""
        self._refuse_recurrent()
        assert hidden_states.shape[1] == 1, "Only support decoding with 1 token at a time for now"
        slots = {} if state_indices is None else {"state_indices": state_indices}
        xz = F.linear(hidden_states.squeeze(1), self.in_proj.weight, self.in_proj.bias)     # (B, 2 d_inner)
        x, z = xz.chunk(2, dim=-1)                                                            # views: the kernels take the strides
        cw = self.conv1d.weight
        x = causal_conv1d_update(x, conv_state, cw.reshape(cw.shape[0], cw.shape[-1]), self.conv1d.bias, self.activation, **slots)
        x_db = F.linear(x, self.x_proj.weight)                                                # (B, dt_rank + 2 d_state)
        dt, B, C = torch.split(x_db, [self.dt_rank, self.d_state, self.d_state], dim=-1)
        A = gemm.neg_exp(self.A_log)
        if x.dtype == torch.float32 and self.dt_proj.weight.dtype == torch.float32:
            # dt_proj inside the state update (csrc/mixer_step.hip): one GEMV launch less per step, which is bound by its launches
            y = native.selective_state_update(ssm_state, x, None, A, B, C, self.D, z, self.dt_proj.bias, True, dt_proj=(self.dt_proj.weight, dt),
                                              **slots)
        else:
            dt = F.linear(dt, self.dt_proj.weight)                                            # without the bias: the kernel adds it (:324-325)
            y = selective_state_update(ssm_state, x, dt, A, B, C, self.D, z=z, dt_bias=self.dt_proj.bias, dt_softplus=True, **slots)
        out = F.linear(y, self.out_proj.weight, self.out_proj.bias)
        return out.unsqueeze(1), conv_state, ssm_state

    def fused_step_serves(self, hidden, norm, conv_state, ssm_state):
        """whether `step_fused` takes this token: hidden (B <= 16, d_model), every parameter of the mixer and of `norm` of hidden's dtype T, a
        conv state of T and an SSM state the state-update kernel pairs with T (float32 or T), a conv width the epilogue has"""
        if self.scan_type == "v2" or self._is_zigzag() or not 2 <= self.d_conv <= 4 or self.d_state > 256:
            return False
        T = hidden.dtype
        params = [self.in_proj.weight, self.in_proj.bias, self.conv1d.weight, self.conv1d.bias, self.x_proj.weight, self.dt_proj.weight,
                  self.dt_proj.bias, self.A_log, self.D, self.out_proj.weight, self.out_proj.bias, norm.weight, norm.bias]
        return (native.decode_linear_serves(hidden, self.in_proj.weight, *params) and conv_state.dtype == T
                and ssm_state.dtype in (torch.float32, T))

    def step_fused(self, hidden, residual, norm, residual_dtype, conv_state, ssm_state, state_indices=None):
        """one token through "add -> norm -> mixer" as four dependent launches of the library (csrc/decode_step.hip, csrc/mixer_step.hip) plus
        neg_exp: hidden (B, d_model), the previous layer's mixer output (or the embedding); residual (B, d_model) or None; norm: the block's
        LayerNorm / RMSNorm module; residual_dtype: of the residual stream this call returns (the incoming one's when there is one)
        -> (out (B, d_model) WITHOUT the residual add: it lives in the next caller's prologue, residual_out (B, d_model)).
          1. in_proj with the add + norm prologue and the conv-update epilogue  2. x_proj  3. the state update, dt_proj inside it where the
          kernel takes it (float32; a 16-bit dt_proj is one more decode_linear)  4. out_proj with its bias
        state_indices (B,) int32: the states are pools and launches 1 and 3 address slot state_indices[b] for row b (same launch count)"""
        D, R, N = self.d_inner, self.dt_rank, self.d_state
        cw = self.conv1d.weight
        slots = {} if state_indices is None else {"state_indices": state_indices}
        xz, residual_out = native.decode_linear(hidden, self.in_proj.weight, self.in_proj.bias,
                                                norm=(norm.weight, norm.bias, norm.eps, isinstance(norm, RMSNorm)), residual=residual,
                                                residual_out=residual_dtype,
                                                conv=(conv_state, cw.reshape(cw.shape[0], cw.shape[-1]), self.conv1d.bias, True), **slots)
        x, z = xz[:, :D], xz[:, D:]                                                          # views: the kernels take the strides
        x_db = native.decode_linear(x, self.x_proj.weight)
        dt, B, C = x_db[:, :R], x_db[:, R:R + N], x_db[:, R + N:]
        A = gemm.neg_exp(self.A_log)
        if hidden.dtype == torch.float32:
            y = native.selective_state_update(ssm_state, x, None, A, B, C, self.D, z, self.dt_proj.bias, True, dt_proj=(self.dt_proj.weight, dt),
                                              **slots)
        else:
            y = native.selective_state_update(ssm_state, x, native.decode_linear(dt, self.dt_proj.weight), A, B, C, self.D, z, self.dt_proj.bias, True,
                                              **slots)
        return native.decode_linear(y, self.out_proj.weight, self.out_proj.bias), residual_out

    @torch.no_grad()
    def extend(self, hidden_states, conv_state, ssm_state, state_indices=None, prefill_slots=None):
        """any number of tokens on carried states, the sibling of `step`: hidden_states (B, T, d_model), T >= 1 -> (out (B, T, d_model),
        conv_state, ssm_state), both states updated in place: in_proj (d-major, as _mix forms xz) -> causal_conv1d_chunk -> x_proj / dt_proj
        (the general path of mamba_inner_fn) -> the scan entered with ssm_state and leaving it (csrc/ssm_scan_general.hip) with the z gate ->
        out_proj. No host read and no allocation depends on data: one call can be captured on a single stream.
        state_indices is refused: the chunk kernels address a batch's own states; a slot of a pool is extended through a view pool[s:s+1]."""
        self._refuse_recurrent()
        if prefill_slots is not None:
            raise NotImplementedError("extend with prefill_slots is not built: continuing a slot's state from a packed pass would need a carried "
                                      "state per segment; a packed prompt is one pass at seqlen_offset == 0")
        if state_indices is not None:
            raise NotImplementedError("extend with state_indices is not built: causal_conv1d_chunk and the carried scan take no slot index (only "
                                      "the one-token step kernels do); extend slot s of a pool through the views pool[s:s+1]")
        bsz, T, _ = hidden_states.shape
        assert T >= 1, "extend needs at least one token"
        D, R, N = self.d_inner, self.dt_rank, self.d_state
        xz = gemm.matmul_wx(self.in_proj.weight, hidden_states.reshape(bsz * T, -1).t()).view(2 * D, bsz, T).permute(1, 0, 2)
        if self.in_proj.bias is not None:
            xz = xz + self.in_proj.bias.to(xz.dtype).view(1, -1, 1)
        x, z = xz[:, :D], xz[:, D:]
        cw = self.conv1d.weight
        conv_out = native.causal_conv1d_chunk(x, conv_state, cw.reshape(cw.shape[0], cw.shape[-1]), self.conv1d.bias, True)
        conv_rows = conv_out.permute(1, 0, 2).reshape(D, bsz * T)                           # "b d l -> d (b l)": a view of a d-major conv_out
        x_dbl_t = self.x_proj.weight @ conv_rows                                            # (R + 2N, b l)
        delta = (self.dt_proj.weight @ x_dbl_t[:R]).view(D, bsz, T).permute(1, 0, 2)        # without the bias: the scan adds it
        Bm = x_dbl_t[R:R + N].view(N, bsz, T).permute(1, 0, 2).unsqueeze(1)                 # (b, 1, N, l) views, unit stride along l
        Cm = x_dbl_t[R + N:].view(N, bsz, T).permute(1, 0, 2).unsqueeze(1)
        A = gemm.neg_exp(self.A_log)
        y = native.selective_scan_carry_fwd(conv_out, delta, A, Bm, Cm, self.D.float(), z, self.dt_proj.bias.float(), True, ssm_state, ssm_state)
        if self.out_proj.bias is None:
            out = gemm.linear(y.transpose(1, 2), self.out_proj.weight)
        else:
            out = F.linear(y.transpose(1, 2), self.out_proj.weight, self.out_proj.bias)
        return out, conv_state, ssm_state

    def _forward_cached(self, hidden_states, cond, inference_params, x3, seq_idx=None):
        """forward(inference_params=...): a prompt at seqlen_offset 0 (fused path + the states it leaves behind), one step after it"""
        state_indices = getattr(inference_params, "state_indices", None)
        if state_indices is not None and (self.scan_type == "v2" or self._is_zigzag()):
            raise NotImplementedError(f'state_indices with scan_type "{self.scan_type}" is not built: only the plain causal mixer ("none") runs '
                                      "token by token, so only it has states to index")
        self._refuse_recurrent(x3)
        prefill_slots = getattr(inference_params, "prefill_slots", None)
        prefill_starts = getattr(inference_params, "prefill_starts", None)
        if prefill_starts is not None and prefill_slots is None:
            self._refuse_prefill_starts(prefill_starts, None, hidden_states)
        if prefill_slots is not None:
            if seq_idx is None:
                raise ValueError("prefill_slots without seq_idx: per-segment states belong to packed rows (pass seq_idx; one request alone is "
                                 "an all-equal id row)")
            if inference_params.seqlen_offset > 0:
                raise ValueError("prefill_slots at seqlen_offset > 0: they belong to the packed prompt pass (seqlen_offset == 0); clear "
                                 "inference_params.prefill_slots before the decode steps")
            if state_indices is not None:
                raise ValueError("prefill_slots together with state_indices: the first belong to a packed prompt pass, the second to the decode "
                                 "steps; set one of them")
            if self.layer_idx not in inference_params.key_value_memory_dict:
                raise ValueError("prefill_slots need a pool of states in key_value_memory_dict (allocate_inference_cache(num_slots, ...))")
            states = inference_params.key_value_memory_dict[self.layer_idx]
            return self._mix(hidden_states, cond, states=states, seq_idx=seq_idx, prefill_slots=prefill_slots, prefill_starts=prefill_starts)
        if state_indices is not None and inference_params.seqlen_offset == 0:
            raise ValueError("state_indices at seqlen_offset == 0: a prompt is prefilled into slot s of a pool through the views pool[s:s+1] "
                             "with state_indices=None; the slot index belongs to the decode steps (seqlen_offset > 0)")
        conv_state, ssm_state = self._get_states_from_cache(inference_params, hidden_states.shape[0])
        if inference_params.seqlen_offset > 0:
            if seq_idx is not None:
                raise ValueError("seq_idx at seqlen_offset > 0: sequence ids belong to the prompt pass (seqlen_offset == 0); a decode step "
                                 "continues every row's last segment")
            if state_indices is not None:
                return self.step(hidden_states, conv_state, ssm_state, state_indices=state_indices)[0]
            return self.step(hidden_states, conv_state, ssm_state)[0]       # the states are updated in place
        if seq_idx is None:
            return self._mix(hidden_states, cond, states=(conv_state, ssm_state))
        return self._mix(hidden_states, cond, states=(conv_state, ssm_state), seq_idx=seq_idx)


class Mamba(_MambaBase):
    def forward(self, hidden_states, cond_emb=None, inference_params=None, x3=None, seq_idx=None):
        """hidden_states: (B, L, D) -> (B, L, D).  cond_emb: accepted and unused, as in the reference (mamba_simple.py:162): the DiM blocks
        call every mixer as mixer(x, c).  x3: the input as a split-bf16 operand image instead (inference, gemm.py).
        inference_params: a dimsum_amd.utils.InferenceParams -- the recurrent form, see the module docstring.
        seq_idx: (B, L) int32 sequence ids of packed rows, see the module docstring; None: the call it always was."""
        if seq_idx is not None:
            if inference_params is not None:
                return self._forward_cached(hidden_states, None, inference_params, x3, seq_idx=seq_idx)
            return self._mix(hidden_states, None, x3=x3, seq_idx=seq_idx)
        if inference_params is not None:
            return self._forward_cached(hidden_states, None, inference_params, x3)
        return self._mix(hidden_states, None, x3=x3)


class CondMamba(_MambaBase):
    def forward(self, hidden_states, cond_emb=None, inference_params=None, x3=None):
        """hidden_states: (B, L, D), cond_emb: (B, d_cond) -> (B, L, D). See the module docstring about cond_proj.
        x3: the input as a split-bf16 operand image instead (inference, gemm.py).
        inference_params: a dimsum_amd.utils.InferenceParams -- the recurrent form, see the module docstring."""
        cond = None
        if cond_emb is not None and torch.is_grad_enabled() and self.d_cond is not None:
            cond = self.cond_proj(cond_emb)       # (B, d_inner): graph edge only, never read by a kernel
        if inference_params is not None:
            return self._forward_cached(hidden_states, cond, inference_params, x3)
        return self._mix(hidden_states, cond, x3=x3)


class Block(nn.Module):
    """Add -> LayerNorm / RMSNorm -> mixer, returning (hidden_states, residual): the block of mamba_simple.py:383-436, same constructor,
    forward contract and state-dict keys (`mixer.*`, `norm.*`). One token of a cached sequence (seqlen 1 at seqlen_offset > 0) goes through
    the mixer's `step_fused` when `fused_add_norm` is set, `fused_decode_enabled` (DIMSUM_FUSED_DECODE) and `fused_step_serves` say so: the add + norm is then
    the prologue of in_proj's launch. Everything else -- prompts, training, larger batches, mixed parameter dtypes -- runs the fused add + norm
    kernel (or, without fused_add_norm, the modules) and the mixer's forward, with the same results."""

    def __init__(self, dim, mixer_cls, norm_cls=nn.LayerNorm, fused_add_norm=False, residual_in_fp32=False):
        super().__init__()
        self.residual_in_fp32 = residual_in_fp32
        self.fused_add_norm = fused_add_norm
        self.mixer = mixer_cls(dim)
        self.norm = norm_cls(dim)
        if self.fused_add_norm:
            assert isinstance(self.norm, (nn.LayerNorm, RMSNorm)), "Only LayerNorm and RMSNorm are supported for fused_add_norm"

    def _fused_decode_states(self, hidden_states, residual, inference_params):
        """the layer's (conv_state, ssm_state) when this call is one token that the fused decode step serves, else None"""
        if not (self.fused_add_norm and inference_params is not None and inference_params.seqlen_offset > 0 and hidden_states.dim() == 3
                and hidden_states.shape[1] == 1 and hasattr(self.mixer, "step_fused") and fused_decode_enabled(hidden_states.shape[0], hidden_states.dtype)
                and not torch.is_grad_enabled()):
            return None
        if residual is not None and residual.dtype not in (torch.float32, hidden_states.dtype):
            return None
        states = self.mixer._get_states_from_cache(inference_params, hidden_states.shape[0])       # with state_indices: the pools (num_slots, ...)
        return states if self.mixer.fused_step_serves(hidden_states[:, 0], self.norm, *states) else None

    def forward(self, hidden_states, residual=None, inference_params=None, seq_idx=None):
        """seq_idx: handed to the mixer (packed rows; a prompt or training pass, never a decode step)"""
        if seq_idx is not None and inference_params is not None and inference_params.seqlen_offset > 0:
            raise ValueError("seq_idx at seqlen_offset > 0: sequence ids belong to the prompt pass (seqlen_offset == 0)")
        states = self._fused_decode_states(hidden_states, residual, inference_params)
        if states is not None:
            res_dtype = residual.dtype if residual is not None else (torch.float32 if self.residual_in_fp32 else hidden_states.dtype)
            slots = getattr(inference_params, "state_indices", None)
            out, residual = self.mixer.step_fused(hidden_states[:, 0], None if residual is None else residual[:, 0], self.norm, res_dtype, *states,
                                                  **({} if slots is None else {"state_indices": slots}))
            return out.unsqueeze(1), residual.unsqueeze(1)
        if not self.fused_add_norm:
            residual = (hidden_states + residual) if residual is not None else hidden_states
            hidden_states = self.norm(residual.to(dtype=self.norm.weight.dtype))
            if self.residual_in_fp32:
                residual = residual.to(torch.float32)
        else:
            hidden_states, residual = layer_norm_fn(hidden_states, self.norm.weight, self.norm.bias, residual=residual, eps=self.norm.eps, prenorm=True,
                                                    residual_in_fp32=self.residual_in_fp32, is_rms_norm=isinstance(self.norm, RMSNorm))
        hidden_states = self.mixer(hidden_states, inference_params=inference_params, **({"seq_idx": seq_idx} if seq_idx is not None else {}))
        return hidden_states, residual

    def allocate_inference_cache(self, batch_size, max_seqlen, dtype=None, **kwargs):
        return self.mixer.allocate_inference_cache(batch_size, max_seqlen, dtype=dtype, **kwargs)
