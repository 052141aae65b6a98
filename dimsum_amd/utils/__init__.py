"""small host utilities"""
import dataclasses
from typing import Optional

import torch


@dataclasses.dataclass
class InferenceParams:
    """what a caller hands to Mamba / CondMamba.forward(inference_params=...) to run a sequence token by token: the per-layer
    (conv_state, ssm_state) caches keyed by layer_idx and how many tokens they have seen. Same fields and `reset` as the reference's
    (mamba/mamba_ssm/utils/generation.py:12-28), minus what only its generation loop reads.
    state_indices (no reference counterpart; upstream Mamba's state_batch_indices): None, or an int32 (batch,) device tensor that makes the
    cached states a POOL (num_slots, ...) -- row b of a decode step (seqlen_offset > 0) works on slot state_indices[b], a negative entry is
    a padding row. A prompt (seqlen_offset == 0) takes no indices: it is prefilled into slot s through a view pool[s:s+1]. `reset` leaves it
    alone (the tensor is a static buffer of whoever schedules the batch: dimsum_amd.utils.serving.DecodeEngine).
    prefill_slots (no reference counterpart): None, or an int32 (batch, seqlen) device tensor for a PACKED prompt pass (seqlen_offset == 0
    with seq_idx): the cached states are the pools, and where prefill_slots[b, t] = s >= 0 the conv and SSM states after position t of row b
    are stored into slot s by the conv and scan kernels themselves; negative entries store nothing (plan_packed_prefill builds it). The
    non-negative entries must be < num_slots and pairwise different: not checked (it would take a device read). `reset` leaves it alone.
    prefill_starts (no reference counterpart): None, or what a packed prompt pass with prefill_slots needs to RESUME segments from the
    states their slots already hold -- a dict of plan_packed_prefill(resume=...)'s start_slots and start_rows, (batch, seqlen) int32 on the
    device, and start_list, (S_in,) int64 on the device, the resumed slots in ordinal order. Every mixer snapshots its conv pool over
    start_list (one index_select) and hands the conv the snapshot with start_rows; the scan reads the SSM pool in place with start_slots.
    Needs prefill_slots and seq_idx. `reset` leaves it alone."""
    max_seqlen: int
    max_batch_size: int
    seqlen_offset: int = 0
    key_value_memory_dict: dict = dataclasses.field(default_factory=dict)
    state_indices: Optional[torch.Tensor] = None
    prefill_slots: Optional[torch.Tensor] = None
    prefill_starts: Optional[dict] = None

    def reset(self, max_seqlen, max_batch_size):
        self.max_seqlen, self.max_batch_size, self.seqlen_offset = max_seqlen, max_batch_size, 0


@torch.no_grad()
def chunked_prefill(mixer, hidden_states, inference_params, chunk, *cond):
    """a prompt (B, L, d_model) through a Mamba / CondMamba in pieces of `chunk` tokens, in memory bounded by the piece: the first piece goes
    through forward(inference_params=...) at offset 0 (the fused prompt path, which fills the cache), the rest through `extend` on the cached
    states. *cond: what the mixer's forward takes after hidden_states (CondMamba's cond_emb). Advances inference_params.seqlen_offset by L
    -> the concatenated output (B, L, d_model)."""
    assert chunk >= 1 and inference_params.seqlen_offset == 0, "chunked_prefill starts a sequence: seqlen_offset must be 0"
    if getattr(inference_params, "state_indices", None) is not None:
        raise NotImplementedError("chunked_prefill with state_indices is not built: `extend` works on a batch's own states; prefill a slot of "
                                  "a pool through a view, pool[s:s+1], with state_indices=None")
    if getattr(inference_params, "prefill_slots", None) is not None:
        raise NotImplementedError("chunked_prefill with prefill_slots is not built: `extend` continues a batch's own states and takes no "
                                  "sequence ids; a packed prompt is one pass (forward(seq_idx=..., inference_params=...))")
    L = hidden_states.shape[1]
    outs = [mixer(hidden_states[:, :chunk], *cond, inference_params=inference_params)]
    states = inference_params.key_value_memory_dict[mixer.layer_idx]
    for t in range(chunk, L, chunk):
        outs.append(mixer.extend(hidden_states[:, t:t + chunk], *states)[0])
    inference_params.seqlen_offset += L
    return torch.cat(outs, dim=1)


def seq_idx_from_lengths(lengths, seqlen=None, device=None):
    """one row's sequence ids from its segment lengths -> (seqlen,) int32: 0 for the first `lengths[0]` positions, 1 for the next
    `lengths[1]`, ... seqlen defaults to sum(lengths); a trailing remainder becomes a segment of its own (the next id). Stack the rows of a
    batch with torch.stack. E.g. a prompt of 3 tokens left-padded to 9: seq_idx_from_lengths([6, 3])."""
    lengths = [int(n) for n in lengths]
    if any(n < 0 for n in lengths):
        raise ValueError(f"seq_idx_from_lengths: negative length in {lengths}")
    total = sum(lengths)
    seqlen = total if seqlen is None else int(seqlen)
    if total > seqlen:
        raise ValueError(f"seq_idx_from_lengths: the lengths sum to {total}, more than seqlen = {seqlen}")
    if total < seqlen:
        lengths = lengths + [seqlen - total]
    return torch.repeat_interleave(torch.arange(len(lengths), dtype=torch.int32), torch.tensor(lengths, dtype=torch.long)).to(device)


def plan_packed_prefill(lengths, slots, rows=1, pad_multiple=1, resume=None):
    """the layout of one packed prompt pass over several new requests, on the host (nothing is read from a device): segment i has
    lengths[i] >= 1 tokens and its states go to slot slots[i]. The segments are placed in order, each onto the currently shortest of `rows`
    rows (the lowest such row on a tie); the rows are then padded to one length, a multiple of pad_multiple, and a row's padding is a segment
    of its own that stores nothing.
    -> dict(seq_idx (rows, seqlen) int32, end_slots (rows, seqlen) int32: slots[i] at segment i's last position and -1 everywhere else,
            segments [(row, start)] per segment, logits_positions (n,) int64: row * seqlen + start + length - 1 per segment, seqlen)
    CPU tensors; rows that got no segment are all padding. What MambaLMHeadModel.forward(seq_idx=, logits_positions=) and
    InferenceParams.prefill_slots take.
    resume: None, or one truth value per segment -- resume[i]: segment i CONTINUES the state already in slots[i] (a later piece of a prompt
    fed in pieces) instead of starting from zeros. The dict then also holds start_slots (rows, seqlen) int32: slots[i] at a resumed
    segment's first position and -1 everywhere else; start_rows, the same positions holding the segment's ordinal among the resumed ones;
    start_list (n_resumed,) int64: the resumed slots in ordinal order -- what InferenceParams.prefill_starts takes. resume=None returns
    exactly the dict above."""
    lengths, slots = [int(n) for n in lengths], [int(s) for s in slots]
    rows, pad_multiple = int(rows), int(pad_multiple)
    if len(lengths) != len(slots) or not lengths:
        raise ValueError(f"plan_packed_prefill: one slot per segment and at least one segment, got {len(lengths)} lengths and {len(slots)} slots")
    if min(lengths) < 1 or min(slots) < 0 or len(set(slots)) != len(slots):
        raise ValueError(f"plan_packed_prefill: lengths must be >= 1 and slots non-negative and pairwise different, got {lengths} and {slots}")
    if rows < 1 or pad_multiple < 1:
        raise ValueError(f"plan_packed_prefill: rows and pad_multiple must be >= 1, got {rows} and {pad_multiple}")
    if resume is not None:
        resume = [bool(f) for f in resume]
        if len(resume) != len(lengths):
            raise ValueError(f"plan_packed_prefill: one resume flag per segment, got {len(resume)} flags for {len(lengths)} segments")
    fill, segments = [0] * rows, []
    for n in lengths:
        r = min(range(rows), key=lambda i: (fill[i], i))
        segments.append((r, fill[r]))
        fill[r] += n
    seqlen = -(-max(fill) // pad_multiple) * pad_multiple
    seq_idx = torch.zeros(rows, seqlen, dtype=torch.int32)
    end_slots = torch.full((rows, seqlen), -1, dtype=torch.int32)
    count = [0] * rows
    for (r, start), n, s in zip(segments, lengths, slots):
        seq_idx[r, start:start + n] = count[r]
        end_slots[r, start + n - 1] = s
        count[r] += 1
    for r in range(rows):
        seq_idx[r, fill[r]:] = count[r]          # the padding: a segment of its own
    pos = torch.tensor([r * seqlen + start + n - 1 for (r, start), n in zip(segments, lengths)], dtype=torch.int64)
    plan = {"seq_idx": seq_idx, "end_slots": end_slots, "segments": segments, "logits_positions": pos, "seqlen": seqlen}
    if resume is not None:
        start_slots, start_rows, start_list = torch.full((rows, seqlen), -1, dtype=torch.int32), torch.full((rows, seqlen), -1, dtype=torch.int32), []
        for (r, start), s, f in zip(segments, slots, resume):
            if f:
                start_slots[r, start], start_rows[r, start] = s, len(start_list)
                start_list.append(s)
        plan.update(start_slots=start_slots, start_rows=start_rows, start_list=torch.tensor(start_list, dtype=torch.int64))
    return plan


def packed_labels(input_ids, seq_idx, ignore_index=-100):
    """next-token labels of packed rows -> (batch, seqlen) int64: labels[b, t] = input_ids[b, t + 1] where t + 1 belongs to the segment of
    t, else ignore_index -- the first token of every segment is nobody's target, and the row's last position has none. What
    MambaLMHeadModel.loss(input_ids, labels, seq_idx=seq_idx) wants."""
    assert input_ids.shape == seq_idx.shape and input_ids.dim() == 2
    labels = torch.full_like(input_ids, ignore_index, dtype=torch.long)
    same = seq_idx[:, 1:] == seq_idx[:, :-1]
    labels[:, :-1] = torch.where(same, input_ids[:, 1:].long(), labels[:, :-1])
    return labels


@torch.no_grad()
def rerandomize_zeros(model, std=0.02, seed=0):
    """The reference initialisation is adaLN-zero + zero final layer, so a freshly initialised DiM outputs exactly 0
    (dimsum/models_dim.py:1762-1770; SURVEY finding 5). Benchmarks with random-init weights re-draw every all-zero
    parameter from N(0, std^2) so that no block degenerates to the identity."""
    g = torch.Generator().manual_seed(seed)
    for _, p in sorted(model.named_parameters(), key=lambda kv: kv[0]):
        if p.numel() > 0 and torch.count_nonzero(p) == 0:
            p.copy_((torch.randn(p.shape, generator=g) * std).to(p.device, p.dtype))
    return model


# ---- explicit accounting of torch-library paths ---------------------------------------------------------------------------
# The hot path runs on libdimsum_hip.so. A few module VARIANTS that no published config enables (qk_norm / swap_k /
# attention dropout in CrossAttentionFusion) have no HIP kernel and run on torch's SDPA; shapes the MFMA attention
# kernels are not instantiated for (head_dim outside {24, 32, 48, 64, 72}, non-fp32 activations) are an ERROR unless
# DIMSUM_ALLOW_TORCH_SDPA=1. Every such call is counted here and announced once, so that "no silent fallback" is checkable:
# tests assert torch_path_counts() stays empty on the published configs.
_torch_paths = {}


def note_torch_path(what, required_opt_in=False):
    import os
    import warnings
    if required_opt_in and os.environ.get("DIMSUM_ALLOW_TORCH_SDPA", "0") != "1":
        raise RuntimeError(f"dimsum_amd: {what} has no HIP kernel in this build (the MFMA attention kernels cover fp32 activations with "
                           "head_dim in {24, 32, 48, 64, 72}). Set DIMSUM_ALLOW_TORCH_SDPA=1 to run it on torch's "
                           "scaled_dot_product_attention instead (counted in dimsum_amd.utils.torch_path_counts()).")
    if what not in _torch_paths:
        warnings.warn(f"dimsum_amd: {what} runs on torch's scaled_dot_product_attention, not on libdimsum_hip.so", stacklevel=3)
    _torch_paths[what] = _torch_paths.get(what, 0) + 1


def torch_path_counts():
    """{description: calls} of everything that ran on a torch-library path instead of a HIP kernel of this build"""
    return dict(_torch_paths)
