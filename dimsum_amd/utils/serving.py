"""Continuous batching on the recurrent form: `DecodeEngine`, a host-side scheduler that keeps requests of different lengths in ONE decode
batch of a fixed size and reuses a finished request's place at once (no reference counterpart: mamba/mamba_ssm/utils/generation.py decodes a
batch that lives and dies together).

A Mamba layer's state per request is a fixed (d_inner, d_conv) + (d_inner, d_state), with no position-dependent cache, so membership is one
indirection: the engine owns a POOL of `num_slots` states per layer (allocate_inference_cache(num_slots, ...)) and a per-row slot index, an
int32 device tensor that rides in InferenceParams.state_indices and is read by the step kernels themselves (csrc/mixer_step.hip,
csrc/decode_step.hip). Idle rows carry slot -1: they touch no state and stay finite. With cg=True the step -- the
model's forward at the fixed batch `max_batch` plus, with fused sampling, the sampler writing into the step's own token buffer -- is captured
into ONE hipGraph per engine (`n_captures == 1`) that serves every membership: between replays the host only rewrites static buffers (the
slots, the token of a newly admitted row, the step's uniforms).

Scheduling, chosen for simplicity: `submit` only queues. `step` first admits queued requests while a row and a slot are free -- each is
prefilled ALONE, eagerly, at batch 1, through the existing prompt path on the views pool[s:s+1] (which overwrites both states of the slot
completely: `_mix` copies the conv tail into conv_state and the scan's last state into ssm_state, so slots are not zeroed on release), and its
first token is sampled ON THE DEVICE from the prompt's logits into the row's place in the token buffer -- then runs one decode step of every
live row. So a prefill stalls the decode batch, and an admitted request always takes a row for at least one step: a request that its first
token already ends (max_new_tokens 1, or eos) is retired after that step and the step's token of its row is dropped.

Host reads: exactly one per step -- the batch's tokens after the decode step (the step's (max_batch,) tokens together with the first tokens
of the rows admitted in this step, ONE small device-to-host copy), which the host needs to see eos_token_id and to report the tokens. It is
the engine's only host read: an admission reads nothing, and the slots are never read back.

Packed prefill (`packed_prefill=True`, or DIMSUM_PACKED_PREFILL=1; off by default): an admission takes EVERY queued request that fits -- a row
and a slot free, and the prompt tokens within `max_prefill_tokens` if given (one request always fits) -- packs the prompts into
`prefill_rows` rows (utils.plan_packed_prefill) and runs ONE model pass with seq_idx and InferenceParams.prefill_slots on the pool itself:
the conv and scan kernels store every request's states into its slot (csrc/causal_conv1d.hip, csrc/ssm_scan_general.hip; DESIGN.md section
3.20). The head runs on the requests' last tokens only (logits_positions), ONE sampler launch draws all first tokens, and device index ops
scatter them and the slots into the step's buffers. An admission still reads nothing back. The packed pass runs the general scan kernels
whatever the d_state, so a request's first logits agree with its alone prefill to rounding, not bit for bit.

Chunked prefill (`chunked_prefill=True` on top of packed_prefill and max_prefill_tokens; off by default): an admission NEVER exceeds
max_prefill_tokens prompt tokens. A prompt that does not fit in what is left of the budget is cut: its first piece claims a row and a slot and
stores its states there; the request stays "prefilling" -- its row is reserved but its slot is not in the step's slot buffer, so the decode
step does not touch it, and it gets no logits and no sample. Every following step admits the next pieces of the prefilling requests first, in
queue order before new requests, as segments that RESUME their slot (plan_packed_prefill(resume=...), InferenceParams.prefill_starts; the
kStart kernels). The piece that ends the prompt is in logits_positions, is sampled with uniforms[0] and joins the
decode batch exactly as a packed admission does. So a long prompt delays the live rows by bounded passes instead of one long one.

Held states (chunked_prefill=True only): a held state is a slot the engine does not free -- (slot, tokens consumed,
pending token or None) under a handle from the request-id counter. `hold(prefix)` queues a prefill-only entry in the same FIFO: admitted in
pieces like a chunked request, it claims a slot and no row, nothing is sampled, and when its last piece is in the handle is ready.
`submit(..., start=h)` continues a held state: a fork (move=False) claims a new slot, all forks of one admission are copied by ONE
native.state_copy_slots launch before the prompt pass, and the request enters it as a resumed piece over [pending] + prompt_ids; a session
turn (move=True) takes over the handle's slot, no copy, the handle is consumed. A request whose handle is not ready waits at the queue's head.
`keep=True` turns a finished request's slot into a ready handle under its rid: its last generated token was sampled but never fed, so the
state covers the prompt and tokens[:-1] and that token is `pending` (a request ended by its first token has fed it in the step of its
admission: nothing is pending). `submit_n` draws n samples from one prefill; `release(h)` frees a handle; `held` lists the ready ones.

Documented limits: prefill stalls the batch (by at most max_prefill_tokens tokens per step with chunked_prefill); without chunked_prefill a
packed admission starts every slot from zero state; max_batch above 16 runs the unfused step (with slots); no automatic (hash-keyed) prefix
matching: the caller names the handle; no preemption.
Sampling: `fused_sampling=True` draws token i of a request with uniforms[i] of THAT request (given to `submit`, or drawn there from the
engine's generator) whichever row and step it lands on, so a request's output does not depend on its neighbours or on the schedule;
`fused_sampling=False` runs generation.sample() per step on the batch's logits, whose multinomial draws (top_k != 1) come from one shared
generator and do depend on the schedule."""
import collections
import dataclasses
import os
from typing import Optional

import torch

from . import InferenceParams, plan_packed_prefill
from .. import native
from .generation import sample


@dataclasses.dataclass
class _Request:
    rid: int
    prompt: torch.Tensor                      # (L,) int64 on the model's device
    max_new_tokens: int
    uniforms: Optional[torch.Tensor]          # (max_new_tokens,) float32 on the host, or None (unfused sampling)
    tokens: list = dataclasses.field(default_factory=list)
    scores: list = dataclasses.field(default_factory=list)
    slot: int = -1
    row: int = -1
    finished: bool = False
    done: int = 0                             # chunked prefill: tokens of `feed` already prefilled into the slot
    feed: Optional[torch.Tensor] = None       # what the prompt passes consume: the prompt, behind the pending token of the state it starts from
    history: Optional[torch.Tensor] = None    # the tokens of the held state it starts from (its pending token included), or None
    start: Optional["_Held"] = None           # the held state it starts from
    move: bool = False                        # it takes over start's slot (a session turn); else start's slot is copied (a fork)
    keep: bool = False                        # when it finishes its slot becomes a held state
    handle: Optional["_Held"] = None          # a prefill-only entry (`hold`): the held state it fills; it takes a slot and no row


@dataclasses.dataclass
class _Held:
    hid: int
    tokens: torch.Tensor                      # (consumed,) int64 on the model's device: every token the slot's state covers once it is ready
    slot: int = -1
    pending: Optional[int] = None             # a token that was sampled but never fed to the model: whoever continues feeds it first
    ready: bool = False
    users: int = 0                            # queued forks that have not been admitted yet
    auto_release: bool = False                # submit_n: released when its last fork is admitted


class DecodeEngine:
    """eng = DecodeEngine(model, max_batch, num_slots=None, max_seqlen=..., top_k=1, top_p=0.0, temperature=1.0, eos_token_id=None,
                          vocab_size=None, cg=True, fused_sampling=True, packed_prefill=False, prefill_rows=1, max_prefill_tokens=None)
    rid = eng.submit(prompt_ids, max_new_tokens, uniforms=None)    1-D prompt; uniforms (max_new_tokens,) float32 pins the draws
    h = eng.hold(prefix_ids); eng.submit(..., start=h, move=False, keep=False); eng.submit_n(prompt_ids, max_new_tokens, n); eng.release(h);
    eng.held; eng.context(rid)                                     held states: shared prefixes, forks, kept sessions (module docstring)
    events = eng.step()                                            [(rid, token, finished)]: admissions' first tokens, then one decode step
    results = eng.run()                                            until idle -> {rid: LongTensor prompt + generated}
    model: a MambaLMHeadModel (anything with allocate_inference_cache and forward(ids, inference_params=, num_last_tokens=) -> .logits).
    num_slots (default max_batch) >= max_batch states per layer. max_seqlen: what allocate_inference_cache is told (Mamba states do not
    depend on it). vocab_size: the classes of a padded head, as in generate(). output_scores=True keeps every token's logits row
    (`scores(rid)`). generator: with fused sampling a CPU generator from which `submit` draws a request's uniforms on the host; without it
    the device generator handed to sample(). packed_prefill / prefill_rows / max_prefill_tokens: one packed prompt pass per admission (module
    docstring; None = DIMSUM_PACKED_PREFILL=1). chunked_prefill: cut prompts to the budget (module docstring). `n_prefill_passes` counts the
    model's prompt passes, `n_prefill_pieces` the prompt segments in them, `prefill_pass_tokens` the prompt tokens of each chunked pass. Bookkeeping the tests read: `n_captures`, `free_slots`, `rows`, `slot_history` [(rid, slot)] in admission order.
    See the module docstring for the schedule, the host reads and the limits."""

    def __init__(self, model, max_batch, num_slots=None, *, max_seqlen, top_k=1, top_p=0.0, temperature=1.0, eos_token_id=None, vocab_size=None,
                 cg=True, fused_sampling=True, output_scores=False, generator=None, packed_prefill=None, prefill_rows=1, max_prefill_tokens=None,
                 chunked_prefill=False):
        num_slots = max_batch if num_slots is None else int(num_slots)
        if max_batch < 1 or num_slots < max_batch:
            raise ValueError(f"DecodeEngine: need max_batch >= 1 and num_slots >= max_batch, got {max_batch} and {num_slots}")
        self.model, self.max_batch, self.num_slots, self.max_seqlen = model, int(max_batch), num_slots, int(max_seqlen)
        self.top_k, self.top_p, self.temperature = int(top_k), float(top_p), float(temperature)
        self.eos_token_id, self.vocab_size = eos_token_id, vocab_size
        self.cg, self.fused_sampling, self.output_scores, self.generator = bool(cg), bool(fused_sampling), bool(output_scores), generator
        self.packed_prefill = os.environ.get("DIMSUM_PACKED_PREFILL", "0") == "1" if packed_prefill is None else bool(packed_prefill)
        self.prefill_rows = int(prefill_rows)
        self.max_prefill_tokens = None if max_prefill_tokens is None else int(max_prefill_tokens)
        if self.prefill_rows < 1 or (self.max_prefill_tokens is not None and self.max_prefill_tokens < 1):
            raise ValueError(f"DecodeEngine: prefill_rows and max_prefill_tokens must be >= 1, got {prefill_rows} and {max_prefill_tokens}")
        self.chunked_prefill = bool(chunked_prefill)
        if self.chunked_prefill and not (self.packed_prefill and self.max_prefill_tokens is not None):
            raise ValueError("DecodeEngine: chunked_prefill cuts prompts to the budget of a packed admission: it needs packed_prefill=True and "
                             "max_prefill_tokens")
        self.n_prefill_passes = self.n_prefill_pieces = 0
        self.prefill_pass_tokens = []                       # chunked prefill: prompt tokens of every pass, in order
        self._prefilling = []                               # chunked prefill: requests whose prompt is partly in their slot, in queue order
        param = next(iter(model.parameters()))
        self.device = param.device
        with torch.no_grad():
            self.pool = model.allocate_inference_cache(num_slots, self.max_seqlen, param.dtype)
        # the static buffers of the step: every row's slot (-1 = idle), its newest token, its uniform; and the first tokens of the rows
        # admitted since the last step, waiting for the step's host read
        self.slots = torch.full((self.max_batch,), -1, dtype=torch.int32, device=self.device)
        self.input_ids = torch.zeros((self.max_batch, 1), dtype=torch.long, device=self.device)
        self.u = torch.zeros(self.max_batch, dtype=torch.float32, device=self.device)
        self.first = torch.zeros(self.max_batch, dtype=torch.long, device=self.device)
        self._fresh = set()                                 # rows admitted since the last step
        self.params = InferenceParams(max_seqlen=self.max_seqlen, max_batch_size=self.max_batch, seqlen_offset=1, key_value_memory_dict=self.pool,
                                      state_indices=self.slots)
        self.free_slots = list(range(num_slots))
        self.rows = [None] * self.max_batch                 # row -> rid
        self.queue = collections.deque()
        self.requests = {}
        self.slot_history = []
        self.n_captures = 0
        self._next_rid = 0
        self._graph = self._logits = None
        self._handles = {}                                  # held states by handle id, ready or still prefilling
        self._hold_reqs = {}                                # the prefill-only entries of `hold` until their state is ready
        self._keeping = set()                               # unfinished requests whose slot will become a held state
        self._pool_table = None                             # native.state_pool_table(self.pool), built at the first fork

    # ---- the request side --------------------------------------------------------------------------------------------------------------------
    def _need_chunked(self, what):
        if not self.chunked_prefill:
            raise ValueError(f"DecodeEngine: {what} rides on chunked admission and the resume kernels: it needs an engine with chunked_prefill=True")

    def _handle(self, h):
        if h not in self._handles:
            raise KeyError(f"DecodeEngine: {h!r} is not a held state (never held, released, or consumed by a move=True request)")
        return self._handles[h]

    def _room_to_hold(self, what):
        if len(self._handles) + len(self._keeping) + 1 >= self.num_slots:
            raise ValueError(f"DecodeEngine.{what}: every one of the {self.num_slots} slots would then be held and no request could be admitted")

    def _id(self):
        self._next_rid += 1
        return self._next_rid - 1

    def hold(self, prefix_ids):
        """queues a prefill-only entry -> a handle. Admitted like a chunked request, it claims a slot and no row; nothing is sampled. Once all
        of prefix_ids is in the slot the handle is ready (`held`): submit(..., start=handle) continues from it."""
        self._need_chunked("hold")
        prefix = torch.as_tensor(prefix_ids, dtype=torch.long)
        if prefix.dim() != 1 or prefix.numel() < 1:
            raise ValueError("DecodeEngine.hold: prefix_ids must be 1-D with at least one token")
        self._room_to_hold("hold")
        hid = self._id()
        prefix = prefix.to(self.device)
        self._handles[hid] = h = _Held(hid, prefix)
        self._hold_reqs[hid] = _Request(hid, prefix, 0, None, feed=prefix, handle=h)
        self.queue.append(hid)
        return hid

    def release(self, h):
        """frees a ready held state's slot; the handle is gone"""
        held = self._handle(h)
        if not held.ready or held.users:
            raise ValueError(f"DecodeEngine.release: held state {h} is {'still prefilling' if not held.ready else 'awaited by queued forks'}")
        del self._handles[h]
        self.free_slots.append(held.slot)

    @property
    def held(self):
        """{handle: (slot, tokens consumed, pending token or None)} of the ready held states"""
        return {hid: (h.slot, h.tokens.numel(), h.pending) for hid, h in self._handles.items() if h.ready}

    def submit_n(self, prompt_ids, max_new_tokens, n, uniforms=None):
        """n samples of one prompt -> their ids: the prompt but its last token is prefilled ONCE into a held state, n forks continue it with
        the last token, and the hold is released when the last fork is admitted. uniforms: (n, max_new_tokens), row i pins sample i."""
        prompt = torch.as_tensor(prompt_ids, dtype=torch.long)
        if prompt.dim() != 1 or prompt.numel() < 1 or int(n) < 1:
            raise ValueError("DecodeEngine.submit_n: prompt_ids must be 1-D with at least one token, n >= 1")
        if uniforms is not None and len(uniforms) != int(n):
            raise ValueError(f"DecodeEngine.submit_n: uniforms must be (n, max_new_tokens) = ({int(n)}, {int(max_new_tokens)})")
        rows = [None] * int(n) if uniforms is None else list(uniforms)
        if prompt.numel() == 1:
            return [self.submit(prompt, max_new_tokens, u) for u in rows]
        self._need_chunked("submit_n")
        h = self.hold(prompt[:-1])
        try:
            rids = [self.submit(prompt[-1:], max_new_tokens, u, start=h) for u in rows]
        except Exception:
            held = self._handles[h]                          # nothing of a refused call stays queued
            for rid in [i for i in self.queue if i in self.requests and self.requests[i].start is held]:
                self.queue.remove(rid)
                del self.requests[rid]
            self.queue.remove(h)
            del self._handles[h], self._hold_reqs[h]
            raise
        self._handles[h].auto_release = True
        return rids

    def submit(self, prompt_ids, max_new_tokens, uniforms=None, start=None, move=False, keep=False):
        """queues a request -> its id. prompt_ids: 1-D, at least one token. uniforms (max_new_tokens,) float32 in [0, 1): draw i of this
        request (fused sampling); None: drawn here from the engine's generator.
        start: a handle (`hold`, or the id of a finished keep=True request) -- the request's context is the held state, then prompt_ids, which
        may be empty when the state has a pending token. move=False: a fork, the state is copied into a new slot and the handle stays;
        move=True: a session turn, the request takes over the handle's slot and the handle is consumed. keep=True: when the request
        finishes its slot is not freed and its id becomes a ready handle (module docstring)."""
        prompt = torch.as_tensor(prompt_ids, dtype=torch.long)
        if start is not None or keep or move:
            self._need_chunked("start= / move= / keep=")
        if move and start is None:
            raise ValueError("DecodeEngine.submit: move=True takes over the slot of a held state: it needs start=")
        held = None if start is None else self._handle(start)
        fewest = 0 if held is not None and held.pending is not None else 1
        if prompt.dim() != 1 or prompt.numel() < fewest or int(max_new_tokens) < 1:
            raise ValueError("DecodeEngine.submit: prompt_ids must be 1-D with at least one token (none is needed behind a held state's pending "
                             "token), max_new_tokens >= 1")
        max_new_tokens = int(max_new_tokens)
        if self.fused_sampling:
            if uniforms is None:
                uniforms = torch.rand(max_new_tokens, dtype=torch.float32, generator=self.generator)       # on the host: a CPU generator
            uniforms = torch.as_tensor(uniforms).detach().to("cpu")
            if tuple(uniforms.shape) != (max_new_tokens,) or uniforms.dtype != torch.float32:
                raise ValueError(f"DecodeEngine.submit: uniforms must be (max_new_tokens,) = ({max_new_tokens},) float32, got {tuple(uniforms.shape)} {uniforms.dtype}")
        elif uniforms is not None:
            raise ValueError("DecodeEngine.submit: uniforms pin the draws of the fused sampler; this engine runs sample() (fused_sampling=False)")
        if keep and not (move and held is not None):          # a kept session turn holds what its handle held
            self._room_to_hold("submit(keep=True)")
        rid = self._id()
        prompt = prompt.to(self.device)
        self.requests[rid] = r = _Request(rid, prompt, max_new_tokens, uniforms, feed=prompt, start=held, move=bool(move), keep=bool(keep))
        if held is not None:
            pending = [] if held.pending is None else [torch.tensor([held.pending], dtype=torch.long, device=self.device)]
            r.history, r.feed = torch.cat([held.tokens] + pending), torch.cat(pending + [prompt])
            if move:
                del self._handles[start]
            else:
                held.users += 1
        if keep:
            self._keeping.add(rid)
        self.queue.append(rid)
        return rid

    def context(self, rid):
        """-> LongTensor: the full token history of a request -- the held state's tokens it started from, its prompt, what it generated"""
        r = self.requests[rid]
        return self.sequence(rid) if r.history is None else torch.cat([r.history.cpu(), self.sequence(rid)])

    def idle(self):
        return not self.queue and not self._prefilling and all(r is None for r in self.rows)

    def sequence(self, rid):
        """-> LongTensor (prompt + generated so far) on the host"""
        r = self.requests[rid]
        return torch.cat([r.prompt.cpu(), torch.tensor(r.tokens, dtype=torch.long)])

    def scores(self, rid):
        """-> the (vocab,) logits rows the request's tokens were chosen from, in order (output_scores=True)"""
        return list(self.requests[rid].scores)

    def run(self):
        """steps until the queue and the batch are empty -> {rid: LongTensor prompt + generated} of every request submitted so far"""
        while not self.idle():
            self.step()
        return {rid: self.sequence(rid) for rid in self.requests}

    # ---- sampling ----------------------------------------------------------------------------------------------------------------------------
    def _view(self, logits):
        return logits[..., :self.vocab_size] if self.vocab_size is not None else logits

    def _sample_into(self, logits, u, out):
        """one token per row of logits -> out (rows,) / (rows, 1) int64, by the fused sampler (u (rows,)) or sample()"""
        if self.fused_sampling:
            native.sample_logits(self._view(logits), u, top_k=self.top_k, top_p=self.top_p, temperature=self.temperature, out=out)
        else:
            out.copy_(sample(self._view(logits), top_k=self.top_k, top_p=self.top_p, temperature=self.temperature,
                             generator=self.generator).view(out.shape))

    # ---- admission ---------------------------------------------------------------------------------------------------------------------------
    def _done(self, r, token):
        return len(r.tokens) >= r.max_new_tokens or (self.eos_token_id is not None and token == self.eos_token_id)

    def _admit_packed(self):
        """every queued request that fits, in ONE packed prompt pass (module docstring)"""
        batch, budget = [], self.max_prefill_tokens
        free_rows = [row for row, rid in enumerate(self.rows) if rid is None]
        while self.queue and len(batch) < min(len(self.free_slots), len(free_rows)):
            r = self.requests[self.queue[0]]
            if batch and budget is not None and sum(b.prompt.numel() for b in batch) + r.prompt.numel() > budget:
                break
            batch.append(self.requests[self.queue.popleft()])
        if not batch:
            return
        slots, rows = [self.free_slots.pop(0) for _ in batch], free_rows[:len(batch)]
        plan = plan_packed_prefill([r.prompt.numel() for r in batch], slots, rows=self.prefill_rows)
        ids = torch.zeros((self.prefill_rows, plan["seqlen"]), dtype=torch.long)
        dev = lambda t: t.to(self.device, non_blocking=True)
        ids = dev(ids)
        for r, (prow, start) in zip(batch, plan["segments"]):
            ids[prow, start:start + r.prompt.numel()].copy_(r.prompt)
        prefill = InferenceParams(max_seqlen=self.max_seqlen, max_batch_size=self.prefill_rows, key_value_memory_dict=self.pool,
                                  prefill_slots=dev(plan["end_slots"]))
        logits = self.model(ids, inference_params=prefill, seq_idx=dev(plan["seq_idx"]), logits_positions=dev(plan["logits_positions"])).logits
        self.n_prefill_passes += 1
        self.n_prefill_pieces += len(batch)
        u = None if not self.fused_sampling else dev(torch.stack([r.uniforms[0] for r in batch]))
        first = torch.empty(len(batch), dtype=torch.long, device=self.device)
        self._sample_into(logits, u, first)                                      # (S, V) -> (S,): stays on the device
        row_idx = dev(torch.tensor(rows, dtype=torch.long))
        self.first.index_copy_(0, row_idx, first)
        self.input_ids.index_copy_(0, row_idx, first.view(-1, 1))
        self.slots.index_copy_(0, row_idx, dev(torch.tensor(slots, dtype=torch.int32)))
        for i, (r, slot, row) in enumerate(zip(batch, slots, rows)):
            self.slot_history.append((r.rid, slot))
            if self.output_scores:
                r.scores.append(self._view(logits)[i].clone())
            r.slot, r.row, self.rows[row] = slot, row, r.rid
            self._fresh.add(row)

    def _admit_chunked(self):
        """_admit_packed under a hard budget: the next pieces of the prefilling requests first, then queued requests, cut where the budget ends
        (module docstring). Pieces that end their prompt are sampled and join the decode batch; the others only store their states."""
        budget, batch = self.max_prefill_tokens, []                              # batch: (request, piece length, resumed)
        for r in self._prefilling:
            if budget == 0:
                break
            n = min(budget, r.feed.numel() - r.done)
            batch.append((r, n, True))
            budget -= n
        free_rows = [row for row, rid in enumerate(self.rows) if rid is None]
        new, copies, spent = [], [], []                 # admitted here; (src, dst) of the forks; submit_n holds whose last fork was admitted
        while self.queue and budget > 0:
            r = self.requests[self.queue[0]] if self.queue[0] in self.requests else self._hold_reqs[self.queue[0]]
            held, own_slot = r.start, r.start is None or not r.move
            if held is not None and not held.ready:                              # its state is still being prefilled: the queue keeps its order
                break
            if (own_slot and not self.free_slots) or (r.handle is None and not free_rows):
                break
            self.queue.popleft()
            r.slot = self.free_slots.pop(0) if own_slot else held.slot
            if held is not None and own_slot:
                copies.append((held.slot, r.slot))
                held.users -= 1
                if held.auto_release and held.users == 0:
                    spent.append(held)
            if r.handle is None:
                r.row = free_rows.pop(0)
                self.rows[r.row] = r.rid                                         # the row is reserved; its entry in self.slots stays -1
            else:
                r.handle.slot = r.slot                                           # a hold takes no row
            self.slot_history.append((r.rid, r.slot))
            n = min(budget, r.feed.numel())
            batch.append((r, n, held is not None))                               # a request behind a held state resumes its slot at once
            new.append(r)
            budget -= n
        if not batch:
            return
        if copies:                                                               # every fork of this admission: ONE launch, before the pass
            if self._pool_table is None:
                self._pool_table = native.state_pool_table(self.pool)
            native.state_copy_slots(self._pool_table, copies)
        plan = plan_packed_prefill([n for _, n, _ in batch], [r.slot for r, _, _ in batch], rows=self.prefill_rows, resume=[f for _, _, f in batch])
        dev = lambda t: t.to(self.device, non_blocking=True)
        ids = dev(torch.zeros((self.prefill_rows, plan["seqlen"]), dtype=torch.long))
        for (r, n, _), (prow, start) in zip(batch, plan["segments"]):
            ids[prow, start:start + n].copy_(r.feed[r.done:r.done + n])
        last = [i for i, (r, n, _) in enumerate(batch) if r.done + n == r.feed.numel() and r.handle is None]
        starts = None
        if plan["start_list"].numel():
            starts = {k: dev(plan[k]) for k in ("start_slots", "start_rows", "start_list")}
        prefill = InferenceParams(max_seqlen=self.max_seqlen, max_batch_size=self.prefill_rows, key_value_memory_dict=self.pool,
                                  prefill_slots=dev(plan["end_slots"]), prefill_starts=starts)
        # the head runs on the pieces that end their prompt; a pass of inner pieces alone still needs one position: its logits are dropped
        pos = plan["logits_positions"][last] if last else plan["logits_positions"][:1]
        logits = self.model(ids, inference_params=prefill, seq_idx=dev(plan["seq_idx"]), logits_positions=dev(pos)).logits
        self.n_prefill_passes += 1
        self.n_prefill_pieces += len(batch)
        self.prefill_pass_tokens.append(sum(n for _, n, _ in batch))
        for r, n, _ in batch:
            r.done += n
            if r.handle is not None and r.done == r.feed.numel():               # a hold's last piece: nothing is sampled, the state is ready
                r.handle.ready = True
                del self._hold_reqs[r.rid]
        for held in spent:                                                       # stream order: the copies above read the slot before it is reused
            if self._handles.get(held.hid) is held:
                self.release(held.hid)
        self._prefilling = [r for r in self._prefilling + new if r.done < r.feed.numel()]
        if not last:
            return
        ready = [batch[i][0] for i in last]
        u = None if not self.fused_sampling else dev(torch.stack([r.uniforms[0] for r in ready]))
        first = torch.empty(len(ready), dtype=torch.long, device=self.device)
        self._sample_into(logits, u, first)
        row_idx = dev(torch.tensor([r.row for r in ready], dtype=torch.long))
        self.first.index_copy_(0, row_idx, first)
        self.input_ids.index_copy_(0, row_idx, first.view(-1, 1))
        self.slots.index_copy_(0, row_idx, dev(torch.tensor([r.slot for r in ready], dtype=torch.int32)))
        for i, r in enumerate(ready):
            if self.output_scores:
                r.scores.append(self._view(logits)[i].clone())
            self._fresh.add(r.row)

    def _admit(self):
        if self.chunked_prefill:
            return self._admit_chunked()
        if self.packed_prefill:
            return self._admit_packed()
        while self.queue and self.free_slots and None in self.rows:
            r = self.requests[self.queue.popleft()]
            slot, row = self.free_slots.pop(0), self.rows.index(None)
            self.slot_history.append((r.rid, slot))
            views = {k: tuple(t[slot:slot + 1] for t in states) for k, states in self.pool.items()}
            prefill = InferenceParams(max_seqlen=self.max_seqlen, max_batch_size=1, key_value_memory_dict=views)
            logits = self.model(r.prompt.unsqueeze(0), inference_params=prefill, num_last_tokens=1).logits[:, -1]
            self.n_prefill_passes += 1
            if self.output_scores:
                r.scores.append(self._view(logits)[0].clone())
            first = self.first[row:row + 1]
            self._sample_into(logits, None if r.uniforms is None else r.uniforms[:1].to(self.device), first)      # stays on the device
            self.input_ids[row:row + 1].copy_(first.view(1, 1))
            self.slots[row:row + 1].fill_(slot)
            r.slot, r.row, self.rows[row] = slot, row, r.rid
            self._fresh.add(row)

    # ---- the step ----------------------------------------------------------------------------------------------------------------------------
    def _forward(self):
        logits = self.model(self.input_ids, inference_params=self.params, num_last_tokens=1).logits[:, -1]
        if self.fused_sampling:
            self._sample_into(logits, self.u, self.input_ids)       # the step feeds itself: the token lands in its own input buffer
        return logits

    def _capture(self, n_warmups=2):
        """the one graph of this engine. Warm-up runs on a side stream with every row idle (slot -1: no state of the pool is touched); the
        live membership is put back before the capture, which records but does not run."""
        live = self.slots.clone()
        tokens = self.input_ids.clone()
        self.slots.fill_(-1)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(n_warmups):
                self._forward()
            s.synchronize()
        torch.cuda.current_stream().wait_stream(s)
        self.slots.copy_(live)
        self.input_ids.copy_(tokens)
        self._graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._graph):
            self._logits = self._forward()
        self.n_captures += 1

    def _book(self, r, token, events):
        r.tokens.append(token)
        r.finished = self._done(r, token)
        events.append((r.rid, token, r.finished))

    def _retire(self, row, r, fed_last=False):
        if r.keep:
            # the state covers every token that was FED: the last generated token was sampled and never fed -- unless the request's first
            # token ended it, which the step of its admission consumed (module docstring, "Scheduling")
            fed = r.tokens if fed_last else r.tokens[:-1]
            parts = ([] if r.history is None else [r.history]) + [r.prompt, torch.tensor(fed, dtype=torch.long, device=self.device)]
            self._handles[r.rid] = _Held(r.rid, torch.cat(parts), r.slot, None if fed_last else r.tokens[-1], ready=True)
            self._keeping.discard(r.rid)
        else:
            self.free_slots.append(r.slot)
        self.rows[row] = None
        self.slots[row:row + 1].fill_(-1)
        r.slot = r.row = -1

    @torch.no_grad()
    def step(self):
        """admits what fits, then one decode step of every live request -> [(rid, token, finished)]: per row, the first token of a request
        admitted in this step, then the step's token"""
        self._admit()
        live = [(row, self.requests[rid]) for row, rid in enumerate(self.rows) if rid is not None]
        live = [(row, r) for row, r in live if r.done == 0 or r.done == r.feed.numel()]          # a prefilling request only holds its row
        if not live:
            return []
        fresh, self._fresh = self._fresh, set()
        if self.fused_sampling:
            u = torch.zeros(self.max_batch, dtype=torch.float32)
            for row, r in live:
                i = len(r.tokens) + (row in fresh)           # a fresh row's first token is not in the book yet
                u[row] = r.uniforms[i] if i < r.max_new_tokens else 0.0
            self.u.copy_(u)
        if self.cg:
            if self._graph is None:
                self._capture()
            self._graph.replay()
            logits = self._logits
        else:
            logits = self._forward()
        if not self.fused_sampling:
            self._sample_into(logits, None, self.input_ids)
        tokens = torch.cat([self.first, self.input_ids[:, 0]]).tolist()      # the engine's only host read: 2 max_batch tokens, one copy
        events = []
        for row, r in live:
            if row in fresh:
                self._book(r, tokens[row], events)
            fed_last = r.finished                            # ended by its first token, which this step has fed to the model
            if not r.finished:                               # else ended by its first token: the step's token of this row is dropped
                if self.output_scores:
                    r.scores.append(self._view(logits)[row].clone())
                self._book(r, tokens[self.max_batch + row], events)
            if r.finished:
                self._retire(row, r, fed_last)
        return events
