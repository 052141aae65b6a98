"""Autograd front-ends of the selective scan and of the fused Mamba inner block -- same names, argument order and
return conventions as mamba/mamba_ssm/ops/selective_scan_interface.py, implemented on dimsum_amd.native (HIP, gfx950).

  selective_scan_fn                      <- :94-101   (SelectiveScanFn :12-91)
  mamba_inner_fn[_cond]                  <- :1277-1348 (MambaInnerFn :579-790, MambaInnerFnCond :793-1007)
  mamba_inner_fn_no_out_proj[_cond]      <- :1389-1452 (MambaInnerFnNoOutProj[Cond] :174-576)
  bimamba_inner_fn                       <- :1351-1388 (BiMambaInnerFn :1010-1274), on the bidirectional scan (native.selective_scan_bidir_*)

The four fused variants of the reference are four near-identical 200-line classes; here they are ONE Function with two
switches (out-projection, conditional conv entry). Semantics kept: checkpoint_lvl=1 recomputation of conv1d_out and
delta in the backward, dx/dz written side by side into one `dxz`, `dcond = None` (SURVEY finding 1), fp32 dB/dC
accumulation cast back to the input dtype, autocast-aware weight casts.
One deliberate difference in what is SAVED (not in what is computed): the reference drops `out_z` after the forward and has
the backward kernel recompute and re-write it (selective_scan_interface.py:952, `recompute_out_z=True`) to save one
activation tensor on 40-80 GB GPUs. With 288 GB of HBM the forward's `out_z` is simply kept for `d out_proj.weight`, and the
backward kernel skips that store (0.27 GB less traffic per call at DiM-L/2, batch 256). DIMSUM_RECOMPUTE_OUT_Z=1 restores
the reference's trade.

selective_scan_fn takes everything the reference's does: any dstate in 1..256, constant (dim, dstate) B / C, complex A (B / C then complex, or
real with a last axis of 2 seqlen). What the tuned kernels are not built for -- native.scan_takes_general_path -- runs on the general kernels
(csrc/ssm_scan_general.hip); every other call takes the path it always took. mamba_inner_fn and its _cond / _no_out_proj forms run any dstate
in 1..256 the same way, without the fused extras (dt_proj inside the scan, out_z operand images, f16s training).
selective_scan_fn(..., initial_state=h) starts from a carried (batch, dim, dstate) state instead of zeros (inference only, no graph): the general
kernel's carried-state entry point for every dstate; without it the routing is what it was.
seq_idx (batch, seqlen) int32 -- packed rows, upstream Mamba's per-token sequence id: the sequences of one row do not see each other (the conv
drops the taps that cross a change of the id, the scan restarts its state there). selective_scan_fn(seq_idx=...) runs the packed-row
instantiations of the general kernels whatever the dstate; mamba_inner_fn / mamba_inner_fn_no_out_proj(seq_idx=...) run the plain sequence
conv -> x_proj / dt_proj -> scan -> out_proj on them under autograd, none of the fused extras. seq_idx=None is the call it always was.
Not implemented (raise): seq_idx with complex A, constant B / C, a carried initial_state, conv_done, the _cond forms' init_states (bimamba_inner_fn has no such argument);
complex A and constant B / C inside mamba_inner_fn* and bimamba_inner_fn; a dstate outside {4, 8, 16, 32} inside
bimamba_inner_fn.
"""
import os
from collections import namedtuple

import torch
import torch.nn.functional as F
from torch.amp import custom_bwd, custom_fwd

from .. import gemm, native
from .causal_conv1d_interface import causal_conv1d_fn


def _last_contig(t):
    return t if t is None or t.stride(-1) == 1 else t.contiguous()


def _scan_operands(u, delta, B, C, D, z):
    """the operands as every route of selective_scan_fn hands them to native: unit stride along the sequence, four-dim B / C, a dense D
    -> (u, delta, B, C, D, z, B was three-dim, C was three-dim)"""
    u, delta, B, C, z = (_last_contig(t) for t in (u, delta, B, C, z))
    squeeze_B, squeeze_C = B.dim() == 3, C.dim() == 3
    return (u, delta, B.unsqueeze(1) if squeeze_B else B, C.unsqueeze(1) if squeeze_C else C, D.contiguous() if D is not None else None, z,
            squeeze_B, squeeze_C)


def _scan_grads(ctx, du, ddelta, dA, dB, dC, dD, ddelta_bias, *rest):
    """native's backward list -> the gradients of forward's eleven arguments: dB / dC in the caller's rank, nothing for an absent D / z /
    delta_bias nor for the three arguments that are no tensors"""
    return (du, ddelta, dA, dB.squeeze(1) if ctx.squeeze_B else dB, dC.squeeze(1) if ctx.squeeze_C else dC, dD if ctx.has_D else None,
            rest[0] if ctx.has_z else None, ddelta_bias if ctx.has_bias else None, None, None, None)


class SelectiveScanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False, return_last_state=False,
                need_ckpt=False):
        u, delta, B, C, D, z, ctx.squeeze_B, ctx.squeeze_C = _scan_operands(u, delta, B, C, D, z)
        ctx.delta_softplus, ctx.has_z, ctx.has_D, ctx.has_bias = delta_softplus, z is not None, D is not None, delta_bias is not None
        # the general kernels (csrc/ssm_scan_general.hip) serve what the tuned ones are not built for: constant B / C, complex A, other dstates
        # (GPU tensors only: anything else keeps going to native.selective_scan_fwd, which refuses it -- or to what stands in for it in tests)
        ctx.general = u.is_cuda and native.scan_takes_general_path(A.shape[-1], A.is_complex(), B.dim() >= 3, C.dim() >= 3, force=native.scan_general_forced())
        if ctx.general:
            out, x, *rest = native.selective_scan_general_fwd(u, delta, A, B, C, D, z, delta_bias, delta_softplus)
            ckpt = None
        else:
            # training extra: saved states for the backward kernel (`need_ckpt` is decided by the caller: inside forward()
            # grad mode is off and ctx.needs_input_grad ignores torch.no_grad())
            out, x, *rest = native.selective_scan_fwd(u, delta, A, B, C, D, z, delta_bias, delta_softplus, need_ckpt=need_ckpt)
            ckpt = rest.pop() if need_ckpt else None
        last_state = x[:, :, -1, 1::2]                     # (batch, dim, dstate)   (:39)
        ctx.save_for_backward(u, delta, A, B, C, D, z, delta_bias, x, out if ctx.has_z else None, ckpt)
        res = rest[0] if ctx.has_z else out
        return res if not return_last_state else (res, last_state)

    @staticmethod
    def backward(ctx, dout, *args):
        u, delta, A, B, C, D, z, delta_bias, x, out, ckpt = ctx.saved_tensors
        dout = _last_contig(dout)
        if ctx.general:
            return _scan_grads(ctx, *native.selective_scan_general_bwd(u, delta, A, B, C, D, z, delta_bias, dout, out, None, ctx.delta_softplus))
        return _scan_grads(ctx, *native.selective_scan_bwd(u, delta, A, B, C, D, z, delta_bias, dout, x, out, None, ctx.delta_softplus, False, ckpt=ckpt))


class SelectiveScanVarlenFn(torch.autograd.Function):
    """selective_scan_fn(seq_idx=...): packed rows on the kVarlen instantiations of csrc/ssm_scan_general.hip, whatever the dstate"""

    @staticmethod
    def forward(ctx, u, delta, A, B, C, D, z, delta_bias, delta_softplus, return_last_state, seq_idx):
        u, delta, B, C, D, z, ctx.squeeze_B, ctx.squeeze_C = _scan_operands(u, delta, B, C, D, z)
        ctx.delta_softplus, ctx.has_z, ctx.has_D, ctx.has_bias = delta_softplus, z is not None, D is not None, delta_bias is not None
        out, x, *rest = native.selective_scan_varlen_fwd(u, delta, A, B, C, D, z, delta_bias, delta_softplus, seq_idx)
        ctx.save_for_backward(u, delta, A, B, C, D, z, delta_bias, out if ctx.has_z else None, seq_idx)
        res = rest[0] if ctx.has_z else out
        return res if not return_last_state else (res, x[:, :, -1, 1::2])      # the state of the row's last segment

    @staticmethod
    def backward(ctx, dout, *args):
        u, delta, A, B, C, D, z, delta_bias, out, seq_idx = ctx.saved_tensors
        return _scan_grads(ctx, *native.selective_scan_varlen_bwd(u, delta, A, B, C, D, z, delta_bias, _last_contig(dout), out, None, ctx.delta_softplus,
                                                                  seq_idx))


def _refuse_varlen_scan(who, A, B, C):
    """what the packed-row scan kernels are not instantiated for (nothing asks for these combinations)"""
    if A.is_complex():
        raise NotImplementedError(f"{who}: seq_idx with a complex A is not built: the packed-row scan kernels are instantiated for real A with "
                                  "input-dependent B and C")
    if (B is not None and B.dim() < 3) or (C is not None and C.dim() < 3):
        raise NotImplementedError(f"{who}: seq_idx with a constant (dim, dstate) B or C is not built: the packed-row scan kernels are "
                                  "instantiated for real A with input-dependent B and C")


def _selective_scan_varlen_states(u, delta, A, B, C, D, z, delta_bias, delta_softplus, return_last_state, seq_idx, end_slots, ssm_state):
    """selective_scan_fn(seq_idx=, end_slots=, ssm_state=): the kEmit instantiations of csrc/ssm_scan_general.hip, no graph"""
    if end_slots is None or ssm_state is None:
        raise ValueError("selective_scan_fn: end_slots and ssm_state go together (where to store, and the pool to store into)")
    if seq_idx is None:
        raise ValueError("selective_scan_fn: end_slots without seq_idx: per-segment states belong to packed rows (pass seq_idx; one segment is an "
                         "all-equal id row)")
    _refuse_varlen_scan("selective_scan_fn", A, B, C)
    if _will_backprop(u, delta, A, B, C, D, z, delta_bias, ssm_state):
        raise NotImplementedError("selective_scan_fn: end_slots / ssm_state are inference arguments -- the scan that stores per-segment states "
                                  "has no backward; call it under torch.no_grad() or on inputs that do not require grad")
    with torch.no_grad():
        u, delta, B, C, D, z, _, _ = _scan_operands(u, delta, B, C, D, z)
        out, x, *rest = native.selective_scan_varlen_states_fwd(u, delta, A, B, C, D, z, delta_bias, delta_softplus, seq_idx, end_slots, ssm_state,
                                                                need_x=return_last_state)
    res = rest[0] if z is not None else out
    return res if not return_last_state else (res, x[:, :, -1, 1::2])


def _selective_scan_varlen_resume(u, delta, A, B, C, D, z, delta_bias, delta_softplus, return_last_state, seq_idx, end_slots, ssm_state, start_slots,
                                  initial_states):
    """selective_scan_fn(seq_idx=, start_slots=, initial_states=[, end_slots=, ssm_state=]): the kStart instantiations of
    csrc/ssm_scan_general.hip, no graph"""
    if start_slots is None or initial_states is None:
        raise ValueError("selective_scan_fn: start_slots and initial_states go together (which segments continue, and the states they continue)")
    if seq_idx is None:
        raise ValueError("selective_scan_fn: start_slots without seq_idx: resumed segments belong to packed rows (pass seq_idx; one segment is an "
                         "all-equal id row)")
    if (end_slots is None) != (ssm_state is None):
        raise ValueError("selective_scan_fn: end_slots and ssm_state go together (where to store, and the pool to store into)")
    _refuse_varlen_scan("selective_scan_fn", A, B, C)
    if _will_backprop(u, delta, A, B, C, D, z, delta_bias, ssm_state, initial_states):
        raise NotImplementedError("selective_scan_fn: start_slots / initial_states are inference arguments -- the scan that continues states "
                                  "has no backward; call it under torch.no_grad() or on inputs that do not require grad")
    with torch.no_grad():
        u, delta, B, C, D, z, _, _ = _scan_operands(u, delta, B, C, D, z)
        if end_slots is None:
            # a continuation that stores nothing: an all-negative row, and a pool nobody writes (initial_states itself serves)
            end_slots, ssm_state = torch.full_like(start_slots, -1), initial_states
        out, x, *rest = native.selective_scan_varlen_resume_fwd(u, delta, A, B, C, D, z, delta_bias, delta_softplus, seq_idx, end_slots, ssm_state,
                                                                start_slots, initial_states, need_x=return_last_state)
    res = rest[0] if z is not None else out
    return res if not return_last_state else (res, x[:, :, -1, 1::2])


def selective_scan_varlen_torch(u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False, return_last_state=False, seq_idx=None,
                                end_slots=None, ssm_state=None, start_slots=None, initial_states=None):
    """selective_scan_fn(seq_idx=...) written out in plain torch, in the precision of its inputs (float64 inputs give the float64 answer): a
    loop over the positions, h_t = (1 - r_t) exp(dt_t A) h_{t-1} + dt_t B_t u_t with r_t = 1 where seq_idx changes; real A, B / C
    (batch, dstate, seqlen) or (batch, groups, dstate, seqlen). Differentiable. What the tests compare the kernels with and what CPU tests put
    in their place; never a fallback: nothing in the package calls it.
    end_slots / ssm_state: selective_scan_fn's -- where end_slots[b, t] = s >= 0, ssm_state[s] receives h_t of row b (a host read of
    end_slots: test infrastructure).
    start_slots / initial_states: selective_scan_fn's -- where start_slots[b, t] = s >= 0 (a segment's first position) the state entering
    position t is initial_states[s] instead of zeros. initial_states may be ssm_state: a slot is read at its segment's first step and
    stored at its segment's end, in that order."""
    batch, dim, seqlen = u.shape
    N = A.shape[-1]
    assert (end_slots is None) == (ssm_state is None) and (end_slots is None or seq_idx is not None)
    assert (start_slots is None) == (initial_states is None) and (start_slots is None or seq_idx is not None)
    starts = None
    if start_slots is not None:
        assert start_slots.dtype == torch.int32 and tuple(start_slots.shape) == (batch, seqlen) and tuple(initial_states.shape[1:]) == (dim, N)
        starts = start_slots.tolist()
    ends = None
    if end_slots is not None:
        assert end_slots.dtype == torch.int32 and tuple(end_slots.shape) == (batch, seqlen) and tuple(ssm_state.shape[1:]) == (dim, N)
        ends = end_slots.tolist()
    B4 = B.unsqueeze(1) if B.dim() == 3 else B
    C4 = C.unsqueeze(1) if C.dim() == 3 else C
    rep = dim // B4.shape[1]
    dt = delta if delta_bias is None else delta + delta_bias[None, :, None]
    if delta_softplus:
        dt = torch.where(dt <= 20.0, F.softplus(dt), dt)
    h = u.new_zeros(batch, dim, N)
    ys = []
    for t in range(seqlen):
        if seq_idx is not None and t > 0:
            h = torch.where((seq_idx[:, t] != seq_idx[:, t - 1])[:, None, None], torch.zeros_like(h), h)
        if starts is not None and any(starts[b][t] >= 0 for b in range(batch)):
            h = torch.stack([initial_states[starts[b][t]].detach().to(h.dtype) if starts[b][t] >= 0 else h[b] for b in range(batch)])
        Bt = B4[:, :, :, t].repeat_interleave(rep, dim=1)                         # (batch, dim, dstate)
        Ct = C4[:, :, :, t].repeat_interleave(rep, dim=1)
        h = torch.exp(dt[:, :, t, None] * A[None]) * h + (dt[:, :, t] * u[:, :, t])[:, :, None] * Bt
        ys.append((h * Ct).sum(-1))
        if ends is not None:
            for b in range(batch):
                if ends[b][t] >= 0:
                    with torch.no_grad():
                        ssm_state[ends[b][t]] = h[b].to(ssm_state.dtype)
    y = torch.stack(ys, dim=-1)
    if D is not None:
        y = y + D[None, :, None] * u
    if z is not None:
        y = y * (z * torch.sigmoid(z))
    y = y.to(u.dtype)
    return y if not return_last_state else (y, h)


def _selective_scan_carry(u, delta, A, B, C, D, z, delta_bias, delta_softplus, return_last_state, initial_state):
    """selective_scan_fn(initial_state=...): the general kernel for every dstate (csrc/ssm_scan_general.hip, dimsum_ssm_scan_carry_fwd), no graph"""
    if _will_backprop(u, delta, A, B, C, D, z, delta_bias, initial_state):
        raise NotImplementedError("selective_scan_fn: a carried state (initial_state) is an inference argument -- the scan that starts from it has "
                                  "no backward; call it under torch.no_grad() or on inputs that do not require grad")
    with torch.no_grad():
        u, delta, B, C, D, z, _, _ = _scan_operands(u, delta, B, C, D, z)
        last = torch.empty_like(initial_state) if return_last_state else None
        out = native.selective_scan_carry_fwd(u, delta, A, B, C, D, z, delta_bias, delta_softplus, initial_state, last)
    return out if not return_last_state else (out, last)


def selective_scan_fn(u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False, return_last_state=False, initial_state=None,
                      seq_idx=None, end_slots=None, ssm_state=None, start_slots=None, initial_states=None):
    """out (or (out, last_state)); the gradient of last_state is not propagated (as in the reference).
    initial_state (batch, dim, dstate), float32 or of u's dtype (complex64 with complex A): the scan starts from it instead of from zeros --
    a cached sequence continued by seqlen tokens; last_state then comes back in its dtype. An inference argument: no graph is recorded, and
    inputs that require grad under grad mode are refused. Such a call runs on the general kernel whatever the dstate.
    seq_idx (batch, seqlen) int32, contiguous: packed rows -- position t >= 1 is a boundary iff seq_idx[b, t] != seq_idx[b, t - 1] (the values
    are only compared), and the state restarts there: every segment gets what it gets as a row of its own, last_state is the last
    segment's. With autograd. Runs the packed-row general kernels whatever the dstate; real A and input-dependent B / C only.
    end_slots (batch, seqlen) int32, contiguous, with seq_idx and ssm_state (num_slots, dim, dstate), float32 or of u's dtype: where
    end_slots[b, t] = s >= 0 the state after position t is stored into ssm_state[s], IN PLACE; negative entries store nothing and unnamed
    slots are not touched. Entries must be < num_slots and none may appear twice: neither is checked (it would take a device read).
    Inference arguments: no graph is recorded.
    start_slots (batch, seqlen) int32, contiguous, with seq_idx and initial_states (n_init, dim, dstate), float32 or of u's dtype:
    start_slots[b, t] = s >= 0 is allowed only at a segment's first position and makes that segment CONTINUE initial_states[s] instead of
    starting from zeros; negative entries start from zeros. end_slots / ssm_state may be absent (nothing is stored). initial_states MAY BE
    ssm_state: one lane owns each (channel, state), loads it at the segment's first step and stores it at the segment's end -- provided a
    slot stored in this call is read only by the segment that stores it (not checked). Inference arguments."""
    if start_slots is not None or initial_states is not None:
        if initial_state is not None:
            raise NotImplementedError("selective_scan_fn: start_slots together with a carried initial_state: a packed row takes its carried "
                                      "states per segment, through start_slots / initial_states")
        return _selective_scan_varlen_resume(u, delta, A, B, C, D, z, delta_bias, delta_softplus, return_last_state, seq_idx, end_slots, ssm_state,
                                             start_slots, initial_states)
    if end_slots is not None or ssm_state is not None:
        if initial_state is not None:
            raise NotImplementedError("selective_scan_fn: end_slots together with a carried initial_state is not built: a packed row starts "
                                      "from zero state")
        return _selective_scan_varlen_states(u, delta, A, B, C, D, z, delta_bias, delta_softplus, return_last_state, seq_idx, end_slots, ssm_state)
    if seq_idx is not None:
        if initial_state is not None:
            raise NotImplementedError("selective_scan_fn: seq_idx together with a carried initial_state is not built: a packed row starts from "
                                      "zero state (there is no packed-row form of the carried-state kernel)")
        _refuse_varlen_scan("selective_scan_fn", A, B, C)
        return SelectiveScanVarlenFn.apply(u, delta, A, B, C, D, z, delta_bias, delta_softplus, return_last_state, seq_idx)
    if initial_state is not None:
        return _selective_scan_carry(u, delta, A, B, C, D, z, delta_bias, delta_softplus, return_last_state, initial_state)
    return SelectiveScanFn.apply(u, delta, A, B, C, D, z, delta_bias, delta_softplus, return_last_state,
                                 _will_backprop(u, delta, A, B, C, D, z, delta_bias))


def _f16s_train(xz, out_proj_weight, will_backprop):
    """whether this training call's out_proj GEMMs run on the single-product carrier (gemm.split3_train_enabled == "f16s" and shapes the kernels take)"""
    if not will_backprop or out_proj_weight is None or not xz.is_cuda or xz.dtype != torch.float32:
        return False
    bsz, d2, L = xz.shape
    return (gemm.split3_train_enabled(_Rows(bsz * L, d2, xz), out_proj_weight) == "f16s"
            and gemm.mamba_f16s_train_ok(bsz * L, out_proj_weight.shape[0], d2 // 2))


class _Rows:
    """a shape-only stand-in for the (tokens, features) view of a d-major tensor: what gemm.split3_train_enabled looks at"""

    def __init__(self, rows, cols, like):
        self.shape, self.is_cuda, self.dtype, self._n = (rows, cols), like.is_cuda, like.dtype, rows * cols

    def numel(self):
        return self._n


def _will_backprop(*tensors):
    """True when autograd will record this call: only then is it worth storing the scan's saved states"""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _checkpoint_lvl():
    """The reference hard-codes checkpoint_lvl = 1 (selective_scan_interface.py:588: conv_out and delta are dropped after the forward and recomputed in
    the backward -- a conv1d launch and a dt_proj GEMM per mixer, to save 2 b d l 4 bytes of activations on 40 / 80-GB parts). With 288 GB per GPU the
    default here is 0: both tensors stay (4.4 GB at DiM-L/2, 64 latents) and the backward starts from them; the gradients are bit-identical
    (the recomputation is deterministic). DIMSUM_MAMBA_CHECKPOINT_LVL=1 restores the reference's trade."""
    return 1 if os.environ.get("DIMSUM_MAMBA_CHECKPOINT_LVL", "0") == "1" else 0


def _rows(t):   # "b d l -> d (b l)" as a view-friendly reshape
    b, d, l = t.shape
    return t.permute(1, 0, 2).reshape(d, b * l)


def _delta(delta_proj_weight, dt_rows, bsz, L):   # dt_proj over the (R, b l) rows, written d-major: (b, d, l) with strides (L, bL, 1), no transpose
    return (delta_proj_weight @ dt_rows).view(delta_proj_weight.shape[0], bsz, L).permute(1, 0, 2)


def _prologue(xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, out_proj_weight, out_proj_bias):
    """shared by both mixers -> xz (unit last stride), conv weight (d, w), conv bias, x, z, the four projection operands (cast under autocast)"""
    if torch.is_autocast_enabled("cuda"):
        adt = torch.get_autocast_dtype("cuda")
        x_proj_weight, delta_proj_weight = x_proj_weight.to(adt), delta_proj_weight.to(adt)
        out_proj_weight = out_proj_weight.to(adt) if out_proj_weight is not None else None
        out_proj_bias = out_proj_bias.to(adt) if out_proj_bias is not None else None
    xz = _last_contig(xz)
    conv_w = conv1d_weight.reshape(conv1d_weight.shape[0], conv1d_weight.shape[-1])     # "d 1 w -> d w"
    x, z = xz.chunk(2, dim=1)
    return xz, conv_w, conv1d_bias.contiguous() if conv1d_bias is not None else None, x, z, x_proj_weight, delta_proj_weight, out_proj_weight, out_proj_bias


def _conv(x, conv_w, conv_b, conv_done=False, init_states=None, d_major=False):
    """causal conv1d + SiLU of the x half. conv_done: x already holds it. d_major (the bidirectional mixer): written d-major, so that x_proj reads its
    (d, b l) rows without a transposing copy. `init_states` is numerically dead in the reference (its buffer is overwritten with the plain conv
    result, causal_conv1d.cpp:326-329). A full-size buffer is honoured as the output buffer; anything else (e.g. the (batch, d_inner) cond_proj
    output CondMamba passes) only keeps the autograd edge."""
    if conv_done:
        return x
    if d_major:
        return native.causal_conv1d_fwd(x, conv_w, conv_b, True, out=x.new_empty(x.shape[1], x.shape[0], x.shape[2]).permute(1, 0, 2))
    if init_states is not None and init_states.shape == x.shape and init_states.dtype == x.dtype and init_states.stride(-1) == 1:
        return native.causal_conv1d_fwd_cond(x, conv_w, conv_b, True, init_states)
    return native.causal_conv1d_fwd(x, conv_w, conv_b, True)


_Proj = namedtuple("_Proj", "x_dbl x_dbl_t delta Bm Cm")     # x_dbl: what the backward gets (None: inference), x_dbl_t: (R + 2N, b l) or None, delta: None = fused


def _project(conv_out, x_proj_weight, delta_proj_weight, N, B_proj_bias, C_proj_bias, training, dt_fusion=None, transposed=None):
    """conv_out -> x_proj -> delta, B, C. Layouts chosen like the reference (:622-626): the GEMM writes delta d-major so that it needs no transpose.
    THE layout rule (transposed=None; the bidirectional mixer asks for True): x_dbl transposed where no projection bias is added and conv_out's (d, b l)
    rows are contiguous; in training only on the GPU outside autocast (DIMSUM_XDBL_T_TRAIN=0: the reference's row-major layout).
    dt_fusion = (z, A) where the caller's launch lets the scan form delta itself (inference without the `out` / `x` stores)."""
    bsz, d_inner, L = conv_out.shape
    R = delta_proj_weight.shape[1]
    conv_rows = _rows(conv_out)
    if transposed is None:
        transposed = (B_proj_bias is None and C_proj_bias is None and conv_rows.stride(1) == 1 and (not training or (
            conv_out.is_cuda and not torch.is_autocast_enabled("cuda") and os.environ.get("DIMSUM_XDBL_T_TRAIN", "1") != "0")))
    if transposed:
        # x_proj written transposed, (R + 2N, b l): its rows are the d-major delta input, B and C as the scan reads them -- (b, 1, N, l) views with strides
        # (l, ., b l, 1) -- without the two transposing copies per mixer. Training keeps it as x_dbl: B and C are read in place by both scan kernels, and the
        # backward writes dB / dC straight into the rows of d x_dbl^T -- 7 transposing / slicing copies per mixer less than the (b l, R + 2N) layout of the
        # reference (:840-860)
        x_dbl_t = x_proj_weight @ (conv_rows if conv_rows.stride(1) == 1 else conv_rows.contiguous())
        # dt_proj inside the scan (csrc/ssm_scan_fwd_kernel.hpp, kDt): where the 64-channel kernel serves the launch, delta = W_dt x_dbl[:R] is formed tile by
        # tile on the matrix cores and the (b, d, l) tensor never exists: one GEMM launch and 2 b d l 4 bytes less per mixer. The launch keeps no `out` / `x`
        # stores then (DIMSUM_SCAN_INFER_STORES=1, the reference interface's launch, takes the GEMM). Only under allow_tf32 (the reference's own setting,
        # train.py:20-21): the in-scan product is three bf16 products per fp32 product (2e-5 relative, what the library's TF32-policy GEMM spends) -- with the
        # flag off the reference multiplies in exact fp32 and so does this path (the library's fp32 GEMM), which also keeps bench.py's exact-fp32 leg exact.
        fused = (dt_fusion is not None and not torch.is_autocast_enabled("cuda") and os.environ.get("DIMSUM_SCAN_DT_PROJ", "1") != "0"
                 and torch.backends.cuda.matmul.allow_tf32 and native.scan_dt_proj_supported(conv_out, dt_fusion[0], dt_fusion[1], delta_proj_weight, x_dbl_t[:R]))
        delta = None if fused else _delta(delta_proj_weight, x_dbl_t[:R], bsz, L)
        Bm = x_dbl_t[R:R + N] if B_proj_bias is None else x_dbl_t[R:R + N] + B_proj_bias.to(x_dbl_t.dtype)[:, None]
        Cm = x_dbl_t[R + N:] if C_proj_bias is None else x_dbl_t[R + N:] + C_proj_bias.to(x_dbl_t.dtype)[:, None]
        return _Proj(x_dbl_t if training else None, x_dbl_t, delta, Bm.view(N, bsz, L).permute(1, 0, 2).unsqueeze(1), Cm.view(N, bsz, L).permute(1, 0, 2).unsqueeze(1))
    x_dbl = F.linear(conv_out.transpose(1, 2).reshape(bsz * L, d_inner), x_proj_weight)        # (b l, R + 2N)
    delta = _delta(delta_proj_weight, x_dbl[:, :R].t(), bsz, L)
    Bm = x_dbl[:, R:R + N] if B_proj_bias is None else x_dbl[:, R:R + N] + B_proj_bias.to(x_dbl.dtype)
    Cm = x_dbl[:, -N:] if C_proj_bias is None else x_dbl[:, -N:] + C_proj_bias.to(x_dbl.dtype)
    Bm = Bm.reshape(bsz, L, N).permute(0, 2, 1).unsqueeze(1).contiguous()                       # (b, 1, N, l)
    Cm = Cm.reshape(bsz, L, N).permute(0, 2, 1).unsqueeze(1).contiguous()
    return _Proj(x_dbl, None, delta, Bm, Cm)


def _out_proj_route(xz, conv_out, z, A, groups, out_proj_weight, out_proj_bias, general, training, keep):
    """gemm.out_proj_route for this launch: the planes unless training (only: a prompt pass that keeps the stores may take them), the two fp16 routes
    unless the scan keeps its `out` / `x` stores (training, last_state, DIMSUM_SCAN_INFER_STORES=1) or autocast is on"""
    bsz, d_inner, L = conv_out.shape
    planes, f16 = not training and L % 8 == 0 and d_inner % 64 == 0, not keep and not torch.is_autocast_enabled("cuda")
    if general or out_proj_weight is None or out_proj_bias is not None or not xz.is_cuda or not (planes or f16):
        return "none"
    route = gemm.out_proj_route(xz, out_proj_weight, bsz * L, L, native.scan_fwd_kernel_for(bsz, d_inner, L, A.shape[-1], groups), planes, f16)
    return "none" if route == "f16_scan" and not native.scan_out_z_f16_supported(conv_out, z, A, groups) else route


def _dbc_into(dx_dbl, R, N, bsz, L):   # dB / dC land in rows R .. R + 2N of d x_dbl^T (R + 2N, b l): the (b, 1, N, l) views the scan backward writes through
    return {"dB": dx_dbl[R:R + N].view(N, bsz, L).permute(1, 0, 2).unsqueeze(1), "dC": dx_dbl[R + N:].view(N, bsz, L).permute(1, 0, 2).unsqueeze(1)}


def _bwd_tail_t(s, x, conv_out, ddelta, dx_dbl, du, dx):
    """the backward behind the scan on the transposed x_dbl (R + 2N, b l) of the saved record s, rows R.. of dx_dbl already written: d dt_proj.weight,
    dx_dbl[:R], d x_proj.weight, d conv_out = du + W_x^T dx_dbl, the conv backward (dx in place) -> (dx_proj_weight, ddelta_proj_weight, dconv_w, dconv_b)"""
    bsz, d_inner, L = x.shape
    R = s.delta_proj_weight.shape[1]
    ddelta2, conv_rows = _rows(ddelta), _rows(conv_out)                                         # (d, b l) views
    conv_rows = conv_rows if conv_rows.stride(1) == 1 else conv_rows.contiguous()
    ddelta_proj_weight = gemm.mm_nt_rows(ddelta2, s.x_dbl[:R])                                  # "dB,rB->dr", sliced reduction
    torch.mm(s.delta_proj_weight.t(), ddelta2, out=dx_dbl[:R])                                  # "dr,dB->rB"
    dx_proj_weight = gemm.mm_nt_rows(dx_dbl, conv_rows)                                         # "rB,dB->rd", sliced reduction
    dconv2 = _rows(du)                         # (d, b l) view of the scan's own du: the product is added in place (no copy of the addend)
    dconv2 = dconv2.addmm_(s.x_proj_weight.t(), dx_dbl) if dconv2.stride(1) == 1 else torch.addmm(dconv2, s.x_proj_weight.t(), dx_dbl)
    _, dconv_w, dconv_b = native.causal_conv1d_bwd(x, s.conv_w, s.conv_b, dconv2.view(d_inner, bsz, L).permute(1, 0, 2), dx, True)
    return dx_proj_weight, ddelta_proj_weight, dconv_w, dconv_b


def _bwd_tail_rows(s, x, conv_out, ddelta, dx_dbl, du, dx, dB, dC, has_Bb, has_Cb):
    """the same on the row-major x_dbl (b l, R + 2N) of the reference, dB / dC copied into its columns -> (.., dB_proj_bias, dC_proj_bias)"""
    bsz, d_inner, L = x.shape
    R, N = s.delta_proj_weight.shape[1], dB.shape[2]
    dBf = dB.squeeze(1).permute(0, 2, 1).reshape(bsz * L, N)                                        # "b 1 n l -> (b l) n"
    dCf = dC.squeeze(1).permute(0, 2, 1).reshape(bsz * L, N)
    dB_proj_bias, dC_proj_bias = dBf.sum(0) if has_Bb else None, dCf.sum(0) if has_Cb else None
    dx_dbl[:, R:R + N] = dBf
    dx_dbl[:, -N:] = dCf
    ddelta2 = _rows(ddelta)                                                                         # (d, b l)
    ddelta_proj_weight = gemm.mm_nn_rows(ddelta2, s.x_dbl[:, :R])                                   # "dB,Br->dr", sliced reduction
    dx_dbl[:, :R] = ddelta2.t() @ s.delta_proj_weight                                               # "dB,dr->Br"
    dconv2 = _rows(du)                                                                              # (d, b l)
    dx_proj_weight = gemm.mm_nn_rows(_rows(conv_out), dx_dbl).t()                                   # "Br,Bd->rd", sliced reduction
    dconv2 = torch.addmm(dconv2, s.x_proj_weight.t(), dx_dbl.t())
    _, dconv_w, dconv_b = native.causal_conv1d_bwd(x, s.conv_w, s.conv_b, dconv2.view(d_inner, bsz, L).permute(1, 0, 2), dx, True)
    return dx_proj_weight, ddelta_proj_weight, dconv_w, dconv_b, dB_proj_bias, dC_proj_bias


# what _MambaInner saves, in ctx.save_for_backward's order; the last five: the fp32 out_z (kept for d out_proj.weight) or, on the scaled-fp16 training
# carrier, the images of out_z and W_out^T
_MambaSaved = namedtuple("_MambaSaved", "xz conv_w conv_b x_dbl x_proj_weight delta_proj_weight out_proj_weight conv_out delta A Bm Cm D delta_bias "
                                        "scan_x out ckpt kept_out_z oz16_data oz16_inv wt16_data wt16_inv", defaults=(None,) * 5)


class _MambaInner(torch.autograd.Function):
    """conv1d(silu) -> x_proj -> dt_proj -> selective scan (+ silu(z) gate) [-> out_proj]."""

    @staticmethod
    @custom_fwd(device_type="cuda")
    def forward(ctx, xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, out_proj_weight, out_proj_bias,
                A, B, C, D, delta_bias, B_proj_bias, C_proj_bias, delta_softplus, init_states, has_out_proj, checkpoint_lvl,
                need_ckpt=False, conv_done=False, f16s_train=False, last_state=None):
        # complex A and constant B / C are refused here (selective_scan_fn takes them); any dstate in 1..256 runs
        # need_ckpt (= training: autograd will record this call; decided by the caller: grad mode is off in here): the tile-boundary states ride along to
        # the backward (one activation tensor): it then needs no sweep of its own to rebuild them. They depend on (conv_out, delta, A, B) only, which
        # the backward recomputes identically.
        # conv_done (inference extra, not in the reference's signature): xz[:, :d_inner] already holds the causal conv1d + SiLU of the in_proj
        # output (the GEMM's epilogue formed it, modules/mamba_simple.py) -- the conv kernel is skipped
        # f16s_train (training extra, decided by the caller like need_ckpt): out_proj's forward, input-gradient and
        # weight-gradient GEMMs as ONE fp16 product per element over scaled-fp16 images (gemm.py, policy "f16s")
        # last_state (recurrent-form extra): a (batch, d_inner, dstate) buffer that receives the scan's state after the last step, as
        # selective_scan_fn(return_last_state=True) returns it (:39) -- the ssm_state a prompt leaves in an inference cache. The launch keeps the
        # reference interface's `x` store then.
        assert checkpoint_lvl in (0, 1)
        assert not (conv_done and need_ckpt), "conv_done is an inference extra"
        if A.is_complex():
            raise NotImplementedError("mamba_inner_fn: complex A is outside this build's scope")
        if B is not None or C is not None:
            raise NotImplementedError("mamba_inner_fn: constant B/C is outside this build's scope")
        L, N, training = xz.shape[-1], A.shape[-1], need_ckpt
        # a dstate the tuned kernels are not built for: the plain sequence on the general kernels (csrc/ssm_scan_general.hip), none of the fused
        # extras below. conv_done is honoured: it says what xz already holds.
        general = xz.is_cuda and native.scan_takes_general_path(N, force=native.scan_general_forced())
        xz, conv_w, conv_b, x, z, x_proj_weight, delta_proj_weight, out_proj_weight, out_proj_bias = _prologue(
            xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, out_proj_weight if has_out_proj else None, out_proj_bias if has_out_proj else None)
        conv_out = _conv(x, conv_w, conv_b, conv_done, init_states)
        bsz = conv_out.shape[0]
        # `out` (ungated) and the chunk states `x` only serve the backward. The reference's kernel always stores them
        # (selective_scan_fwd_kernel.cuh:239-254); here an inference call (nothing to differentiate) passes NULL out_ptr / x_ptr and the
        # kernel skips both stores: 1.082 instead of 1.384 GB per launch at DiM-L/2, batch 256 (SURVEY 8(d)'s "inference-only lower bound"),
        # same arithmetic, bit-identical out_z. DIMSUM_SCAN_INFER_STORES=1 restores the reference interface's stores (bench.py prices
        # that launch too, as `roofline_full_interface`).
        keep = training or last_state is not None or os.environ.get("DIMSUM_SCAN_INFER_STORES", "0") == "1"
        proj = _project(conv_out, x_proj_weight, delta_proj_weight, N, B_proj_bias, C_proj_bias, training, None if general or keep else (z, A))
        x_dbl, delta, Bm, Cm = proj.x_dbl, proj.delta, proj.Bm, proj.Cm
        D = D.contiguous() if D is not None else None
        route = _out_proj_route(xz, conv_out, z, A, Bm.shape[1], out_proj_weight, out_proj_bias, general, training, keep)
        if general:
            out, scan_x, out_z = native.selective_scan_general_fwd(conv_out, delta, A.contiguous(), Bm, Cm, D, z, delta_bias, delta_softplus, need_out=keep, need_x=keep)
            rest = [None]
        else:
            out, scan_x, out_z, *rest = native.selective_scan_fwd(conv_out, delta, A, Bm, Cm, D, z, delta_bias, delta_softplus,
                                                                  need_out=keep, need_x=keep, need_ckpt=training, **({"out_z_planes": True} if route == "planes" else {}),
                                                                  **({"out_z_f16": True} if route == "f16_scan" else {}),
                                                                  **({"dt_proj": (delta_proj_weight, proj.x_dbl_t[:delta_proj_weight.shape[1]])} if delta is None else {}))
        if last_state is not None:
            last_state.copy_(scan_x[:, :, -1, 1::2])
        # the routed product. The conversion route on an out_z whose (d, b l) rows the conversion pass does not take goes on with the fp32 out_z below.
        y = None
        if route == "f16_scan":
            y = gemm.out_proj_f16(out_z[0], out_z[1], out_proj_weight)
        elif route == "planes":
            y = gemm.out_proj_planes(out_z, out_proj_weight)
        elif route == "f16_convert":
            oz_rows = _rows(out_z)
            if oz_rows.stride(1) == 1 and oz_rows.stride(0) % 4 == 0:
                y = gemm.out_proj_f16(*native.rows_block_f16s(oz_rows), out_proj_weight)
        if y is not None:
            return y.view(bsz, L, out_proj_weight.shape[0])
        ckpt = rest[0] if training else None
        ctx.general, ctx.delta_softplus, ctx.has_out_proj, ctx.checkpoint_lvl = general, delta_softplus, has_out_proj, checkpoint_lvl
        ctx.xdbl_t = x_dbl is not None and x_dbl is proj.x_dbl_t       # (training: x_dbl is saved as its transpose)
        ctx.flags = (conv1d_bias is not None, D is not None, delta_bias is not None, B_proj_bias is not None,
                     C_proj_bias is not None, has_out_proj and out_proj_bias is not None)
        if checkpoint_lvl >= 1:
            conv_out, delta = None, None            # recomputed in the backward (:663-664)
        keep_out_z = has_out_proj and training and (general or os.environ.get("DIMSUM_RECOMPUTE_OUT_Z", "0") != "1")     # (the general backward does not recompute it)
        ctx.f16s = bool(f16s_train) and not general and out_proj_bias is None and keep_out_z
        saved = _MambaSaved(xz, conv_w, conv_b, x_dbl, x_proj_weight, delta_proj_weight, out_proj_weight, conv_out, delta, A, Bm, Cm, D, delta_bias,
                            scan_x, out, ckpt, out_z if keep_out_z and not ctx.f16s else None)
        if ctx.f16s:
            # out = out_z^T W_out^T as the TN product of two images whose rows are the reduction index (channels): out_z (d, b l) with one scale per
            # channel, W_out^T (d, e) with one per channel -> per-reduction-row factors. The image replaces the fp32 out_z among the saved tensors
            # (d out_proj.weight reads it again): half the bytes kept per mixer.
            oz16 = native.rows_f16s(_rows(out_z))
            wt16 = gemm.weight_t_f16s_train(out_proj_weight)
            y = native.gemm_tn(oz16.data, wt16.data, row_invs=(oz16.inv, wt16.inv))
            ctx.save_for_backward(*saved[:18], oz16.data, oz16.inv, wt16.data, wt16.inv)
            return y.view(bsz, L, out_proj_weight.shape[0])
        ctx.save_for_backward(*saved)
        if not has_out_proj:
            return out_z                                                                                # (b, d, l)
        oz_t = out_z.transpose(1, 2)
        return gemm.linear(oz_t, out_proj_weight) if out_proj_bias is None else F.linear(oz_t, out_proj_weight, out_proj_bias)    # (b, l, d_model)

    @staticmethod
    @custom_bwd(device_type="cuda")
    def backward(ctx, dout):
        s = _MambaSaved._make(ctx.saved_tensors)
        xz, x_dbl, conv_out, delta, A = s.xz, s.x_dbl, s.conv_out, s.delta, s.A
        has_conv_b, has_D, has_dbias, has_Bb, has_Cb, has_ob = ctx.flags
        L, R, N = xz.shape[-1], s.delta_proj_weight.shape[1], A.shape[-1]
        x, z = xz.chunk(2, dim=1)
        bsz, d_inner = x.shape[0], x.shape[1]
        dout = _last_contig(dout)
        if ctx.checkpoint_lvl == 1:
            conv_out = native.causal_conv1d_fwd(x, s.conv_w, s.conv_b, True)         # the NON-cond entry, as in :929
            delta = _delta(s.delta_proj_weight, x_dbl[:R] if ctx.xdbl_t else x_dbl[:, :R].t(), bsz, L)
        dxz = torch.empty_like(xz)
        dx, dz = dxz.chunk(2, dim=1)
        dout16 = None
        if ctx.f16s:
            # dout_y (d, b l) = W_out^T dout^T as an NT product of the images of W_out^T (one scale per channel = output row) and dout (one per token)
            dout16 = native.rows_f16s(dout.reshape(bsz * L, -1))
            dout_y = native.gemm_nt(s.wt16_data, dout16.data, scales=(s.wt16_inv, dout16.inv)).view(d_inner, bsz, L).permute(1, 0, 2)
        elif ctx.has_out_proj:
            dout2 = dout.reshape(bsz * L, -1).t()                                                       # "b l e -> e (b l)"
            dout_y = (s.out_proj_weight.t() @ dout2).view(d_inner, bsz, L).permute(1, 0, 2)             # d-major like delta
        else:
            dout_y = dout
        recompute = ctx.has_out_proj and s.kept_out_z is None and not ctx.f16s     # only d out_proj.weight needs out_z
        dx_dbl = torch.empty_like(x_dbl)
        into = _dbc_into(dx_dbl, R, N, bsz, L) if ctx.xdbl_t else {}
        if ctx.general:
            dconv_out, ddelta, dA, dB, dC, dD, ddelta_bias, dz = native.selective_scan_general_bwd(
                conv_out, delta, A.contiguous(), s.Bm, s.Cm, s.D, z, s.delta_bias, dout_y, s.out, dz, ctx.delta_softplus, **into)
            rest = []
        else:
            dconv_out, ddelta, dA, dB, dC, dD, ddelta_bias, dz, *rest = native.selective_scan_bwd(
                conv_out, delta, A, s.Bm, s.Cm, s.D, z, s.delta_bias, dout_y, s.scan_x, s.out, dz, ctx.delta_softplus, recompute, ckpt=s.ckpt, **into)
        out_z = rest[0] if recompute else s.kept_out_z
        dout_proj_weight = dout_proj_bias = dB_proj_bias = dC_proj_bias = None
        if ctx.f16s:
            # "eB,dB->ed" as the mixed-layout product out_z (d, B) dout (B, e): the saved image's rows run along the reduction, dout's over it
            dout_proj_weight = native.gemm_nn(s.oz16_data, s.oz16_inv, dout16.data, dout16.inv).t()
        elif ctx.has_out_proj:
            # "eB,dB->ed": a (d_model, d_inner) output over a b*l-long reduction -- sliced, it would fill 8 of 256 CUs otherwise
            dout_proj_weight = gemm.mm_nn_rows(_rows(out_z), dout.reshape(bsz * L, -1)).t()
        if ctx.has_out_proj:
            dout_proj_bias = dout.sum(dim=(0, 1)) if has_ob else None
        if ctx.xdbl_t:
            dx_proj_weight, ddelta_proj_weight, dconv_w, dconv_b = _bwd_tail_t(s, x, conv_out, ddelta, dx_dbl, dconv_out, dx)
        else:
            dx_proj_weight, ddelta_proj_weight, dconv_w, dconv_b, dB_proj_bias, dC_proj_bias = _bwd_tail_rows(
                s, x, conv_out, ddelta, dx_dbl, dconv_out, dx, dB, dC, has_Bb, has_Cb)
        return (dxz, dconv_w.unsqueeze(1), dconv_b if has_conv_b else None, dx_proj_weight, ddelta_proj_weight,
                dout_proj_weight, dout_proj_bias, dA, None, None, dD if has_D else None,
                ddelta_bias if has_dbias else None, dB_proj_bias, dC_proj_bias, None, None, None, None, None, None, None, None)


def _mamba_inner_varlen(has_out_proj, xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, out_proj_weight, out_proj_bias, A, B, C, D,
                        delta_bias, B_proj_bias, C_proj_bias, delta_softplus, seq_idx, last_state=None, end_slots=None, conv_state=None, ssm_state=None,
                        start_slots=None, start_rows=None, conv_initial_states=None):
    """mamba_inner_fn(seq_idx=...): the general route's plain sequence on packed rows, conv -> x_proj / dt_proj -> scan -> out_proj, each piece
    under its own autograd node (causal_conv1d_fn and selective_scan_fn with seq_idx; the projections are GEMMs): no dt_proj in the scan, no
    operand images, no f16s training, no saved-state extras. last_state receives the state of every row's last segment.
    end_slots with the pools conv_state and ssm_state (inference): the conv and the scan store every segment's states into its slot
    themselves (causal_conv1d_fn / selective_scan_fn); last_state is then not taken.
    start_slots / start_rows / conv_initial_states on top of those: resumed segments. The scan reads ssm_state IN PLACE by start_slots (pool
    ids); the conv reads conv_initial_states, a snapshot, by start_rows (ordinals into the snapshot): its carried inputs may not alias the
    pool it stores into."""
    emit = end_slots is not None or conv_state is not None or ssm_state is not None
    resume = start_slots is not None or start_rows is not None or conv_initial_states is not None
    if resume and (start_slots is None or start_rows is None or conv_initial_states is None):
        raise ValueError("mamba_inner_fn_cond: start_slots, start_rows and conv_initial_states go together")
    if resume and not emit:
        raise ValueError("mamba_inner_fn_cond: start_slots without end_slots / conv_state / ssm_state: the scan continues the states of the pool")
    if emit and (end_slots is None or conv_state is None or ssm_state is None):
        raise ValueError("mamba_inner_fn_cond: end_slots, conv_state and ssm_state go together")
    if emit and last_state is not None:
        raise ValueError("mamba_inner_fn_cond: last_state together with end_slots: the per-segment states go to the pools, there is no row state to return")
    if A.is_complex():
        raise NotImplementedError("mamba_inner_fn: complex A is outside this build's scope")
    if B is not None or C is not None:
        raise NotImplementedError("mamba_inner_fn: constant B/C is outside this build's scope")
    xz, conv_w, conv_b, x, z, x_proj_weight, delta_proj_weight, out_proj_weight, out_proj_bias = _prologue(
        xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, out_proj_weight if has_out_proj else None, out_proj_bias if has_out_proj else None)
    bsz, d_inner, L = x.shape
    N, R = A.shape[-1], delta_proj_weight.shape[1]
    conv_out = causal_conv1d_fn(x, conv_w, conv_b, "silu", seq_idx, **({"end_slots": end_slots, "conv_state": conv_state} if emit else {}),
                                **({"start_slots": start_rows, "initial_states": conv_initial_states} if resume else {}))
    x_dbl = F.linear(conv_out.transpose(1, 2).reshape(bsz * L, d_inner), x_proj_weight)            # (b l, R + 2N)
    delta = _delta(delta_proj_weight, x_dbl[:, :R].t(), bsz, L)
    Bm = x_dbl[:, R:R + N] if B_proj_bias is None else x_dbl[:, R:R + N] + B_proj_bias.to(x_dbl.dtype)
    Cm = x_dbl[:, -N:] if C_proj_bias is None else x_dbl[:, -N:] + C_proj_bias.to(x_dbl.dtype)
    Bm = Bm.reshape(bsz, L, N).permute(0, 2, 1).unsqueeze(1).contiguous()                           # (b, 1, N, l)
    Cm = Cm.reshape(bsz, L, N).permute(0, 2, 1).unsqueeze(1).contiguous()
    out_z = selective_scan_fn(conv_out, delta, A, Bm, Cm, D, z, delta_bias, delta_softplus, return_last_state=last_state is not None, seq_idx=seq_idx,
                              **({"end_slots": end_slots, "ssm_state": ssm_state} if emit else {}),
                              **({"start_slots": start_slots, "initial_states": ssm_state} if resume else {}))
    if last_state is not None:
        out_z, last = out_z
        with torch.no_grad():
            last_state.copy_(last)
    if not has_out_proj:
        return out_z
    oz_t = out_z.transpose(1, 2)
    return gemm.linear(oz_t, out_proj_weight) if out_proj_bias is None else F.linear(oz_t, out_proj_weight, out_proj_bias)


def _mamba_inner(has_out_proj, xz, *a, init_states=None, conv_done=False, last_state=None, seq_idx=None, **emit):
    """a: conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, out_proj_weight, out_proj_bias, A, B, C, D, delta_bias, B_proj_bias, C_proj_bias,
    delta_softplus -- _MambaInner.apply's order"""
    if seq_idx is not None:
        if conv_done:
            raise NotImplementedError("mamba_inner_fn: conv_done with seq_idx is not built: the in_proj + conv epilogue takes no sequence ids, so "
                                      "xz cannot already hold the packed-row conv")
        if init_states is not None:
            raise NotImplementedError("mamba_inner_fn_cond: init_states with seq_idx is not built: the conditional entry has no packed-row form")
        return _mamba_inner_varlen(has_out_proj, xz, *a, seq_idx, last_state=last_state, **emit)
    if emit:
        raise ValueError("mamba_inner_fn_cond: end_slots without seq_idx: per-segment states belong to packed rows")
    wb = _will_backprop(xz, *a[:-1], init_states)
    return _MambaInner.apply(xz, *a, init_states, has_out_proj, _checkpoint_lvl(), wb, conv_done, _f16s_train(xz, a[4], wb), last_state)


def mamba_inner_fn(xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, out_proj_weight, out_proj_bias, A,
                   B=None, C=None, D=None, delta_bias=None, B_proj_bias=None, C_proj_bias=None, delta_softplus=True, seq_idx=None):
    return _mamba_inner(True, xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, out_proj_weight, out_proj_bias, A, B, C, D, delta_bias,
                        B_proj_bias, C_proj_bias, delta_softplus, **({"seq_idx": seq_idx} if seq_idx is not None else {}))


def mamba_inner_fn_cond(xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, out_proj_weight, out_proj_bias,
                        A, B=None, C=None, D=None, delta_bias=None, B_proj_bias=None, C_proj_bias=None,
                        delta_softplus=True, init_states=None, conv_done=False, last_state=None, seq_idx=None, end_slots=None, conv_state=None,
                        ssm_state=None, start_slots=None, start_rows=None, conv_initial_states=None):
    """seq_idx: the packed-row route of mamba_inner_fn (last_state is honoured); init_states or conv_done with it raise NotImplementedError.
    end_slots (batch, seqlen) int32 with the pools conv_state (num_slots, d_inner, d_conv) and ssm_state (num_slots, d_inner, d_state), and
    seq_idx: the packed PROMPT pass -- every segment's states are stored into its slot by the conv and scan kernels (inference only).
    start_slots / start_rows (batch, seqlen) int32 and conv_initial_states (n, d_inner, d_conv) with those: segments that CONTINUE a slot --
    the scan reads ssm_state in place by start_slots, the conv reads the snapshot conv_initial_states by start_rows"""
    emit = {k: v for k, v in (("end_slots", end_slots), ("conv_state", conv_state), ("ssm_state", ssm_state), ("start_slots", start_slots),
                              ("start_rows", start_rows), ("conv_initial_states", conv_initial_states)) if v is not None}
    return _mamba_inner(True, xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, out_proj_weight, out_proj_bias, A, B, C, D, delta_bias,
                        B_proj_bias, C_proj_bias, delta_softplus, init_states=init_states, conv_done=conv_done, last_state=last_state,
                        **({"seq_idx": seq_idx} if seq_idx is not None else {}), **emit)


def mamba_inner_fn_no_out_proj(xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, A, B=None, C=None,
                               D=None, delta_bias=None, B_proj_bias=None, C_proj_bias=None, delta_softplus=True, seq_idx=None):
    return _mamba_inner(False, xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, None, None, A, B, C, D, delta_bias,
                        B_proj_bias, C_proj_bias, delta_softplus, **({"seq_idx": seq_idx} if seq_idx is not None else {}))


def mamba_inner_fn_no_out_proj_cond(xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, A, B=None, C=None,
                                    D=None, delta_bias=None, B_proj_bias=None, C_proj_bias=None, delta_softplus=True,
                                    init_states=None, seq_idx=None):
    if seq_idx is not None:
        raise NotImplementedError("mamba_inner_fn_no_out_proj_cond: seq_idx is not built for the conditional form; call mamba_inner_fn_no_out_proj")
    return _mamba_inner(False, xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, None, None, A, B, C, D, delta_bias,
                        B_proj_bias, C_proj_bias, delta_softplus, init_states=init_states)


# what _BiMambaInner saves, in ctx.save_for_backward's order
_BiSaved = namedtuple("_BiSaved", "xz conv_w conv_b x_dbl x_proj_weight delta_proj_weight out_proj_weight conv_out delta A A_b Bm Cm D delta_bias "
                                  "out out_b ckpt ckpt_b kept_out_z")


class _BiMambaInner(torch.autograd.Function):
    """conv1d(silu) -> x_proj -> dt_proj -> forward scan (A) + time-reversed scan (A_b) over the same operands, each gated by silu(z), summed ->
    out_proj (BiMambaInnerFn, mamba/mamba_ssm/ops/selective_scan_interface.py:1010-1388). The reference runs the second scan on .flip(-1)
    copies of u, delta, B, C, z and flips its output back; here both directions are one bidirectional launch pair that reads the forward
    layouts backwards (native.selective_scan_bidir_fwd / _bwd). x_proj is written transposed, (R + 2N, b l), as in _MambaInner's training
    layout: B and C are read in place and the backward writes dB / dC straight into the rows of d x_dbl^T.
    Gradients are those of bimamba_inner_ref (:1503-1561): the reference's backward drops the reversed direction's part of dz (it returns a
    dxz whose z half holds only the forward direction's dz, :1171-1190 / :1218 / :1257); this one does not."""

    @staticmethod
    @custom_fwd(device_type="cuda")
    def forward(ctx, xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, out_proj_weight, out_proj_bias,
                A, A_b, B, C, D, delta_bias, B_proj_bias, C_proj_bias, delta_softplus, checkpoint_lvl, need_ckpt):
        assert checkpoint_lvl in (0, 1)
        if A.is_complex() or A_b.is_complex():
            raise NotImplementedError("bimamba_inner_fn: complex A is outside this build's scope")
        if B is not None or C is not None:
            raise NotImplementedError("bimamba_inner_fn: constant B/C is outside this build's scope")
        native._gpu(xz, conv1d_weight, x_proj_weight, delta_proj_weight, out_proj_weight, A, A_b)
        xz, conv_w, conv_b, x, z, x_proj_weight, delta_proj_weight, out_proj_weight, out_proj_bias = _prologue(
            xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, out_proj_weight, out_proj_bias)
        conv_out = _conv(x, conv_w, conv_b, d_major=True)                                              # shared by both directions (the reference's too)
        x_dbl, _, delta, Bm, Cm = _project(conv_out, x_proj_weight, delta_proj_weight, A.shape[-1], B_proj_bias, C_proj_bias, need_ckpt, transposed=True)
        D = D.contiguous() if D is not None else None
        A, A_b = A.contiguous(), A_b.contiguous()
        out, out_b, out_z, *ck = native.selective_scan_bidir_fwd(conv_out, delta, A, A_b, Bm, Cm, D, z, delta_bias, delta_softplus,
                                                                need_out=need_ckpt, need_ckpt=need_ckpt)
        oz_t = out_z.transpose(1, 2)
        y = gemm.linear(oz_t, out_proj_weight) if out_proj_bias is None else F.linear(oz_t, out_proj_weight, out_proj_bias)       # (b, l, d_model)
        if not need_ckpt:
            return y
        ctx.delta_softplus, ctx.checkpoint_lvl = delta_softplus, checkpoint_lvl
        ctx.flags = (conv1d_bias is not None, D is not None, delta_bias is not None, B_proj_bias is not None,
                     C_proj_bias is not None, out_proj_bias is not None)
        if checkpoint_lvl >= 1:
            conv_out, delta = None, None            # recomputed in the backward (:1095-1096)
        keep_out_z = os.environ.get("DIMSUM_RECOMPUTE_OUT_Z", "0") != "1"
        ctx.save_for_backward(*_BiSaved(xz, conv_w, conv_b, x_dbl, x_proj_weight, delta_proj_weight, out_proj_weight, conv_out, delta, A, A_b, Bm, Cm,
                                        D, delta_bias, out, out_b, ck[0], ck[1], out_z if keep_out_z else None))
        return y

    @staticmethod
    @custom_bwd(device_type="cuda")
    def backward(ctx, dout):
        s = _BiSaved._make(ctx.saved_tensors)
        xz, x_dbl, conv_out, delta = s.xz, s.x_dbl, s.conv_out, s.delta
        has_conv_b, has_D, has_dbias, has_Bb, has_Cb, has_ob = ctx.flags
        L, R, N = xz.shape[-1], s.delta_proj_weight.shape[1], s.A.shape[-1]
        x, z = xz.chunk(2, dim=1)
        bsz, d_inner = x.shape[0], x.shape[1]
        dout = _last_contig(dout)
        if ctx.checkpoint_lvl == 1:
            conv_out = native.causal_conv1d_fwd(x, s.conv_w, s.conv_b, True)
            delta = _delta(s.delta_proj_weight, x_dbl[:R], bsz, L)
        dxz = torch.empty_like(xz)
        dx, dz = dxz.chunk(2, dim=1)
        dout2 = dout.reshape(bsz * L, -1).t()                                                          # "b l e -> e (b l)"
        dout_y = (s.out_proj_weight.t() @ dout2).view(d_inner, bsz, L).permute(1, 0, 2)               # d-major like delta
        recompute = s.kept_out_z is None
        dx_dbl = torch.empty_like(x_dbl)                                                               # (R + 2N, b l)
        into = _dbc_into(dx_dbl, R, N, bsz, L) if x_dbl.dtype == torch.float32 else {}                 # (the kernel's dB / dC are fp32)
        # dz: both directions' parts, written into dxz's z half (the reference keeps only the forward direction's there)
        du, ddelta, dA, dA_b, dB, dC, dD, ddelta_bias, dz, *rest = native.selective_scan_bidir_bwd(
            conv_out, delta, s.A, s.A_b, s.Bm, s.Cm, s.D, z, s.delta_bias, dout_y, s.out, s.out_b, s.ckpt, s.ckpt_b, ctx.delta_softplus, recompute,
            dz=dz, **into)
        if not into:
            dx_dbl[R:R + N] = dB.squeeze(1).permute(1, 0, 2).reshape(N, bsz * L)
            dx_dbl[R + N:] = dC.squeeze(1).permute(1, 0, 2).reshape(N, bsz * L)
        out_z = rest[0] if recompute else s.kept_out_z
        dB_proj_bias = dx_dbl[R:R + N].float().sum(1) if has_Bb else None
        dC_proj_bias = dx_dbl[R + N:].float().sum(1) if has_Cb else None
        # "eB,dB->ed": a (d_model, d_inner) output over a b*l-long reduction
        dout_proj_weight = gemm.mm_nn_rows(_rows(out_z), dout.reshape(bsz * L, -1)).t()
        dout_proj_bias = dout.sum(dim=(0, 1)) if has_ob else None
        dx_proj_weight, ddelta_proj_weight, dconv_w, dconv_b = _bwd_tail_t(s, x, conv_out, ddelta, dx_dbl, du, dx)
        return (dxz, dconv_w.unsqueeze(1), dconv_b if has_conv_b else None, dx_proj_weight, ddelta_proj_weight,
                dout_proj_weight, dout_proj_bias, dA, dA_b, None, None, dD if has_D else None,
                ddelta_bias if has_dbias else None,
                dB_proj_bias.to(s.Bm.dtype) if has_Bb else None, dC_proj_bias.to(s.Cm.dtype) if has_Cb else None, None, None, None)


def bimamba_inner_fn(xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, out_proj_weight, out_proj_bias, A, A_b,
                     B=None, C=None, D=None, delta_bias=None, B_proj_bias=None, C_proj_bias=None, delta_softplus=True):
    """the fused bidirectional Mamba mixer (selective_scan_interface.py:1351-1388): real A / A_b, input-dependent B / C, -> (b, l, d_model).
    It takes no seq_idx (its signature is the reference's): the bidirectional scan kernels have no packed-row form."""
    wb = _will_backprop(xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, out_proj_weight, out_proj_bias, A, A_b, B, C, D,
                        delta_bias, B_proj_bias, C_proj_bias)
    return _BiMambaInner.apply(xz, conv1d_weight, conv1d_bias, x_proj_weight, delta_proj_weight, out_proj_weight, out_proj_bias,
                               A, A_b, B, C, D, delta_bias, B_proj_bias, C_proj_bias, delta_softplus, _checkpoint_lvl(), wb)
