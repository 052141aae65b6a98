"""causal_conv1d_fn / causal_conv1d_update -- same API as causal-conv1d/causal_conv1d/causal_conv1d_interface.py:8-45, :64-76, on the HIP kernels."""
import torch

from .. import native


def _silu_flag(activation, who=None):
    """activation None | "silu" | "swish" -> whether SiLU is applied; anything else is refused (who: a plain-torch restatement names itself)"""
    if activation not in (None, "silu", "swish"):
        raise NotImplementedError("activation must be None, silu, or swish" if who is None else f"{who}: activation {activation!r} (None, 'silu' or 'swish')")
    return activation is not None


class CausalConv1dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias=None, activation=None):
        ctx.activation = _silu_flag(activation)
        if x.stride(2) != 1 and x.stride(1) != 1:
            x = x.contiguous()          # neither seqlen-contiguous nor channel-last (causal_conv1d_interface.py:15-16)
        bias = bias.contiguous() if bias is not None else None
        ctx.save_for_backward(x, weight, bias)
        return native.causal_conv1d_fwd(x, weight, bias, ctx.activation)

    @staticmethod
    def backward(ctx, dout):
        x, weight, bias = ctx.saved_tensors
        channel_last = not (x.stride(2) == 1 or x.shape[2] == 1)
        if not channel_last and dout.stride(2) != 1:
            dout = dout.contiguous()    # a channel-last x takes dout as it comes: native brings it to x's layout once if need be (causal_conv1d.cpp:378-379)
        dx, dweight, dbias = native.causal_conv1d_bwd(x, weight, bias, dout, None, ctx.activation)
        return dx, dweight, dbias if bias is not None else None, None


class CausalConv1dVarlenFn(torch.autograd.Function):
    """causal_conv1d_fn(seq_idx=...): packed rows on the kVarlen kernels of csrc/causal_conv1d.hip"""

    @staticmethod
    def forward(ctx, x, weight, bias, activation, seq_idx):
        ctx.activation = _silu_flag(activation)
        if x.stride(2) != 1:
            x = x.contiguous()          # the packed-row kernels read seqlen-contiguous rows (free batch and channel strides)
        bias = bias.contiguous() if bias is not None else None
        ctx.save_for_backward(x, weight, bias, seq_idx)
        return native.causal_conv1d_varlen_fwd(x, weight, bias, ctx.activation, seq_idx)

    @staticmethod
    def backward(ctx, dout):
        x, weight, bias, seq_idx = ctx.saved_tensors
        if dout.stride(2) != 1:
            dout = dout.contiguous()
        dx, dweight, dbias = native.causal_conv1d_varlen_bwd(x, weight, bias, dout, None, ctx.activation, seq_idx)
        return dx, dweight, dbias if bias is not None else None, None, None


def _conv_varlen_states(x, weight, bias, activation, seq_idx, end_slots, conv_state):
    """causal_conv1d_fn(seq_idx=, end_slots=, conv_state=): the kEmit kernels of csrc/causal_conv1d.hip, no graph"""
    silu = _silu_flag(activation)
    if end_slots is None or conv_state is None:
        raise ValueError("causal_conv1d_fn: end_slots and conv_state go together (where to store, and the pool to store into)")
    if seq_idx is None:
        raise ValueError("causal_conv1d_fn: end_slots without seq_idx: per-segment states belong to packed rows (pass seq_idx; one segment is an "
                         "all-equal id row)")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, weight, bias, conv_state)):
        raise NotImplementedError("causal_conv1d_fn: end_slots / conv_state are inference arguments -- the pass that stores states has no "
                                  "backward; call it under torch.no_grad() or on inputs that do not require grad")
    with torch.no_grad():
        if x.stride(2) != 1:
            x = x.contiguous()
        return native.causal_conv1d_varlen_states_fwd(x, weight, bias.contiguous() if bias is not None else None, silu, seq_idx, end_slots, conv_state)


def _storage_range(t):
    """[first, last + 1) byte addresses a strided tensor can touch (positive strides); an empty tensor touches nothing"""
    if t.numel() == 0:
        return 0, 0
    lo = t.data_ptr()
    return lo, lo + (sum((n - 1) * st for n, st in zip(t.shape, t.stride())) + 1) * t.element_size()


def _conv_varlen_resume(x, weight, bias, activation, seq_idx, end_slots, conv_state, start_slots, initial_states):
    """causal_conv1d_fn(seq_idx=, start_slots=, initial_states=[, end_slots=, conv_state=]): the kStart kernels of csrc/causal_conv1d.hip, no graph"""
    silu = _silu_flag(activation)
    if start_slots is None or initial_states is None:
        raise ValueError("causal_conv1d_fn: start_slots and initial_states go together (which segments continue, and the carried inputs they "
                         "continue)")
    if seq_idx is None:
        raise ValueError("causal_conv1d_fn: start_slots without seq_idx: resumed segments belong to packed rows (pass seq_idx; one segment is an "
                         "all-equal id row)")
    if (end_slots is None) != (conv_state is None):
        raise ValueError("causal_conv1d_fn: end_slots and conv_state go together (where to store, and the pool to store into)")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, weight, bias, conv_state, initial_states)):
        raise NotImplementedError("causal_conv1d_fn: start_slots / initial_states are inference arguments -- the pass that continues states has "
                                  "no backward; call it under torch.no_grad() or on inputs that do not require grad")
    if end_slots is not None and torch.is_tensor(initial_states) and torch.is_tensor(conv_state):
        (a0, a1), (b0, b1) = _storage_range(initial_states), _storage_range(conv_state)
        if initial_states.device == conv_state.device and a0 < b1 and b0 < a1:
            raise ValueError("causal_conv1d_fn: initial_states overlaps conv_state: the lanes that read a slot's carried inputs are not the lane "
                             "that stores the slot's new state, so a slot stored in this launch must not be read in it -- pass a snapshot "
                             "(conv_state.index_select(0, slots)); the scan's initial_states may alias its pool, the conv's may not")
    with torch.no_grad():
        if x.stride(2) != 1:
            x = x.contiguous()
        if end_slots is None:
            # a continuation that stores nothing: an all-negative row, and a pool nobody writes (initial_states itself serves)
            end_slots, conv_state = torch.full_like(start_slots, -1), initial_states
        return native.causal_conv1d_varlen_resume_fwd(x, weight, bias.contiguous() if bias is not None else None, silu, seq_idx, end_slots, conv_state,
                                                      start_slots, initial_states)


def causal_conv1d_fn(x, weight, bias=None, activation=None, seq_idx=None, end_slots=None, conv_state=None, start_slots=None, initial_states=None):
    """x: (batch, dim, seqlen), weight: (dim, width), bias: (dim,), activation: None | "silu" | "swish".
    seq_idx (batch, seqlen) int32, contiguous: packed rows -- a tap that would reach across a change of the id is dropped (position t >= 1 is
    a boundary iff seq_idx[b, t] != seq_idx[b, t - 1]; the values are only compared). None: the call it always was.
    end_slots (batch, seqlen) int32, contiguous, with seq_idx and conv_state (num_slots, dim, width) of x's dtype: where end_slots[b, t] =
    s >= 0 the conv state of the segment ending at t -- its last `width` inputs, zero-padded on the left, x[b, :, t] last -- is stored into
    conv_state[s], IN PLACE; negative entries store nothing and unnamed slots are not touched. Entries must be < num_slots and none may
    appear twice: neither is checked (it would take a device read). Inference arguments: no graph is recorded.
    start_slots (batch, seqlen) int32, contiguous, with seq_idx and initial_states (n_init, dim, width) of x's dtype: start_slots[b, t] = s >= 0
    is allowed only at a segment's first position and makes that segment CONTINUE initial_states[s] -- the last `width` inputs of the
    earlier piece, newest last: the taps that reach before t read them instead of zeros, and a state stored through end_slots is the last
    `width` values of concat(initial_states[s], the segment). Negative entries: zero state, as without the argument. end_slots / conv_state
    may be absent (nothing is stored). initial_states must not overlap conv_state (ValueError): pass a snapshot of the slots. Inference
    arguments."""
    if start_slots is not None or initial_states is not None:
        return _conv_varlen_resume(x, weight, bias, activation, seq_idx, end_slots, conv_state, start_slots, initial_states)
    if end_slots is not None or conv_state is not None:
        return _conv_varlen_states(x, weight, bias, activation, seq_idx, end_slots, conv_state)
    if seq_idx is not None:
        return CausalConv1dVarlenFn.apply(x, weight, bias, activation, seq_idx)
    return CausalConv1dFn.apply(x, weight, bias, activation)


def causal_conv1d_varlen_torch(x, weight, bias=None, activation=None, seq_idx=None, end_slots=None, conv_state=None, start_slots=None,
                               initial_states=None):
    """causal_conv1d_fn(seq_idx=...) written out in plain torch, in the precision of its inputs (float64 inputs give the float64 answer): a
    loop over the positions, tap j of position t counted iff t - j >= 0 and no boundary lies in (t - j, t]. Differentiable. What the tests
    compare the kernels with and what CPU tests put in their place; never a fallback: nothing in the package calls it.
    end_slots / conv_state: causal_conv1d_fn's -- where end_slots[b, t] = s >= 0, conv_state[s, :, width - 1 - j] receives the masked tap j of
    position t (a host read of end_slots: test infrastructure).
    start_slots / initial_states: causal_conv1d_fn's -- a segment whose first position t carries start_slots[b, t] = s >= 0 sees
    initial_states[s, :, width - m] as x[b, :, t - m], m = 1 .. width - 1, and its stored state is the last `width` values of
    concat(initial_states[s], the segment). initial_states is read before anything is stored: it may be conv_state here."""
    silu = _silu_flag(activation, "causal_conv1d_varlen_torch")
    batch, dim, seqlen = x.shape
    width = weight.shape[-1]
    assert weight.shape == (dim, width) and (seq_idx is None or tuple(seq_idx.shape) == (batch, seqlen))
    assert (end_slots is None) == (conv_state is None) and (end_slots is None or seq_idx is not None)
    ends = None
    if end_slots is not None:
        assert end_slots.dtype == torch.int32 and tuple(end_slots.shape) == (batch, seqlen) and tuple(conv_state.shape[1:]) == (dim, width)
        ends = end_slots.tolist()
    assert (start_slots is None) == (initial_states is None) and (start_slots is None or seq_idx is not None)
    zero = x.new_zeros(batch, dim)
    carried = None                                                                 # [b][t] -> {j: the (dim,) value tap j of position t takes from initial_states}
    if start_slots is not None:
        assert start_slots.dtype == torch.int32 and tuple(start_slots.shape) == (batch, seqlen) and tuple(initial_states.shape[1:]) == (dim, width)
        starts, ids, init = start_slots.tolist(), seq_idx.tolist(), initial_states.detach().clone()
        carried = [[{} for _ in range(seqlen)] for _ in range(batch)]
        for b in range(batch):
            for f in range(seqlen):
                if starts[b][f] < 0:
                    continue
                assert f == 0 or ids[b][f] != ids[b][f - 1], "start_slots: a non-negative entry is allowed only at a segment's first position"
                for t in range(f, min(f + width - 1, seqlen)):
                    if ids[b][t] != ids[b][f]:
                        break
                    for j in range(t - f + 1, width):
                        carried[b][t][j] = init[starts[b][f], :, width - (j - (t - f))].to(x.dtype)
    cols = []
    for t in range(seqlen):
        pre = x[:, :, t] * weight[:, width - 1]
        same = torch.ones(batch, dtype=torch.bool, device=x.device)               # no boundary in (t - j, t] so far
        taps = [x[:, :, t]]                                                        # the masked taps j = 0 .. width - 1 of position t
        for j in range(1, min(width, t + 1) if carried is None else width):
            if t - j >= 0:
                if seq_idx is not None:
                    same = same & (seq_idx[:, t - j + 1] == seq_idx[:, t - j])
                tap = torch.where(same[:, None], x[:, :, t - j], zero)
            else:
                tap = zero
            if carried is not None and any(j in carried[b][t] for b in range(batch)):
                tap = torch.stack([carried[b][t].get(j, tap[b]) for b in range(batch)])
            taps.append(tap)
            pre = pre + taps[j] * weight[:, width - 1 - j]
        cols.append(pre if bias is None else pre + bias)
        if ends is not None:
            for b in range(batch):
                if ends[b][t] >= 0:
                    with torch.no_grad():
                        for j in range(width):
                            conv_state[ends[b][t], :, width - 1 - j] = (taps[j][b] if j < len(taps) else zero[b]).to(conv_state.dtype)
    pre = torch.stack(cols, dim=-1)
    return (pre * torch.sigmoid(pre) if silu else pre).to(x.dtype)


def causal_conv1d_update(x, conv_state, weight, bias=None, activation=None, state_indices=None):
    """one token of the causal conv1d on a carried state (causal_conv1d_interface.py:64-76), on the HIP kernel.
    x: (batch, dim), conv_state: (batch, dim, width) -- shifted left by one and x appended, IN PLACE --, weight: (dim, width), bias: (dim,)
    -> out (batch, dim). Every operand may be a strided view.
    state_indices (batch,) int32 (upstream Mamba's conv_state_indices): conv_state is a pool (num_slots, dim, width), row b works on
    conv_state[state_indices[b]], a negative entry is a padding row (no state touched, zero output). Entries must be < num_slots and no slot
    may be named twice: neither is checked (it would take a device read)."""
    silu = _silu_flag(activation)
    if state_indices is None:
        return native.causal_conv1d_update(x, conv_state, weight, bias, silu)
    return native.causal_conv1d_update(x, conv_state, weight, bias, silu, state_indices=state_indices)


def causal_conv1d_chunk(x, conv_state, weight, bias=None, activation=None):
    """any number of tokens of the causal conv1d on a carried state, on the HIP kernel (csrc/causal_conv1d.hip): causal_conv1d_update for a
    block of tokens. x: (batch, dim, seqlen) with stride(-1) == 1, conv_state: (batch, dim, width) -- the conv sees its last width - 1 columns
    to the left of x, and it becomes the last `width` values of concat(conv_state, x), IN PLACE --, weight: (dim, width), bias: (dim,)
    -> out (batch, dim, seqlen). Inference only."""
    return native.causal_conv1d_chunk(x, conv_state, weight, bias, _silu_flag(activation))


def causal_conv1d_chunk_torch(x, conv_state, weight, bias=None, activation=None):
    """causal_conv1d_chunk written out in plain torch, in the precision of its inputs (float64 inputs give the float64 answer): with
    v = concat(conv_state[.., 1:], x) along the sequence, out[.., t] = act(bias + sum_k weight[:, k] v[.., t + k]); conv_state receives the
    last `width` values of concat(conv_state, x). What the tests compare the kernel with; never a fallback: nothing in the package calls it."""
    silu = _silu_flag(activation, "causal_conv1d_chunk_torch")
    width, seqlen = weight.shape[-1], x.shape[-1]
    assert conv_state.shape == (*x.shape[:2], width) and weight.shape == (x.shape[1], width)
    both = torch.cat([conv_state, x], dim=-1)                                           # (batch, dim, width + seqlen)
    windows = both[..., 1:].unfold(-1, width, 1)                                        # (batch, dim, seqlen, width)
    pre = (windows * weight[None, :, None, :]).sum(-1)
    if bias is not None:
        pre = pre + bias[None, :, None]
    conv_state.copy_(both[..., -width:])
    return (pre * torch.sigmoid(pre) if silu else pre).to(x.dtype)


def _slot_rows(state_indices, batch):
    """the restatements' view of state_indices: ([rows b with a slot], [their slots]) as Python lists (a host read: test infrastructure)"""
    assert state_indices.dim() == 1 and state_indices.shape[0] == batch and state_indices.dtype == torch.int32
    slots = state_indices.tolist()
    live = [b for b, s in enumerate(slots) if s >= 0]
    return live, [slots[b] for b in live]


def causal_conv1d_update_torch(x, conv_state, weight, bias=None, activation=None, state_indices=None):
    """The step of the causal conv1d written out in plain torch, in the precision of its inputs (float64 inputs give the float64 answer):
    the window a causal conv of width W sees at the new token is the last W - 1 columns of the state followed by x; the output is the dot
    product of that window with the taps, plus bias, through SiLU if asked. conv_state receives the window. What the tests compare the
    kernel with; never a fallback: nothing in the package calls it.
    state_indices (batch,) int32: conv_state is a pool and row b works on conv_state[state_indices[b]]; rows with a negative entry are
    skipped -- no slot is read or written -- and give zeros."""
    if state_indices is not None:
        live, slots = _slot_rows(state_indices, x.shape[0])
        out = torch.zeros_like(x)
        if live:
            rows = conv_state[slots]                                                    # a gathered copy
            out[live] = causal_conv1d_update_torch(x[live], rows, weight, bias, activation)
            conv_state[slots] = rows
        return out
    silu = _silu_flag(activation, "causal_conv1d_update_torch")
    width = weight.shape[-1]
    window = torch.cat([conv_state[..., 1:], x.unsqueeze(-1)], dim=-1)                  # (batch, dim, width)
    assert window.shape == conv_state.shape and weight.shape == (x.shape[1], width)
    pre = (window * weight.unsqueeze(0)).sum(-1)
    if bias is not None:
        pre = pre + bias.unsqueeze(0)
    conv_state.copy_(window)
    return (pre * torch.sigmoid(pre) if silu else pre).to(x.dtype)
