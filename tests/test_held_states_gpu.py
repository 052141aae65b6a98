"""Held states on the GPU: dimsum_state_copy_slots bit for bit -- the 16-byte path and every element-wise path, the
skips and the bounds, surroundings included, under graph replay with a rewritten pairs buffer -- and DecodeEngine's forks, session turns and
submit_n on the real kernels against the same contexts run alone, by the rule of test_resume_prefill_gpu.py where routes differ (a fork resumes a
state where the alone run is one pass): max |logit - alone logit| < min_gap / 4 first, token ids second."""
import pytest
import torch

from test_lm_cpu import tiny_model
from test_mixer_step_gpu import exact_fp32  # noqa: F401  (a fixture)
from test_slots_gpu import VOCAB, alone

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAIRS = [(0, 1), (0, 2), (-1, 3), (4, -1), (9, 3), (5, 4)]
SLOTS = 6
_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32}


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------------------------
def _carved(seed=0):
    """-> (pool, bases): three "layers" and a byte tensor, each a view into a larger 1-D base filled with 7. Row bytes / path:
    conv (6, 5, 3) bf16: 30-byte rows, 2-byte pieces | ssm (6, 5, 16) f32: 16-byte pieces | conv (6, 8, 4) f16 and ssm (6, 8, 1) bf16: 16-byte
    pieces | conv (6, 4, 4) f32 whose base is 4 bytes off a 16-byte boundary: 4-byte pieces | ssm (6, 5, 16) f32 whose slots are 400 bytes apart:
    16-byte pieces, sentinels between the rows | (6, 7) uint8 one byte off: 1-byte pieces"""
    g = torch.Generator().manual_seed(seed)

    def carve(shape, dtype, offset, slot_elems=None):
        row = 1
        for s in shape[1:]:
            row *= s
        slot_elems = row if slot_elems is None else slot_elems
        base = torch.full((offset + SLOTS * slot_elems + 24,), 7, dtype=dtype, device=DEV)
        view = base[offset:offset + SLOTS * slot_elems].view(SLOTS, slot_elems)[:, :row].view(shape)
        data = torch.randint(100, 200, shape, generator=g).to(dtype) if dtype == torch.uint8 else torch.randn(shape, generator=g).to(dtype)
        view.copy_(data.to(DEV))
        assert base.data_ptr() % 256 == 0                                   # the allocator's alignment: `offset` alone decides the path
        return view, base
    specs = [((SLOTS, 5, 3), torch.bfloat16, 8), ((SLOTS, 5, 16), torch.float32, 4), ((SLOTS, 8, 4), torch.float16, 8), ((SLOTS, 8, 1), torch.bfloat16, 8),
             ((SLOTS, 4, 4), torch.float32, 1), ((SLOTS, 5, 16), torch.float32, 4, 100), ((SLOTS, 7), torch.uint8, 1)]
    views, bases = zip(*(carve(*s) for s in specs))
    assert views[4].data_ptr() % 16 == 4 and views[5].stride(0) * 4 == 400 and views[0][0].numel() * 2 == 30
    return {0: views[0:2], 1: views[2:4], 2: views[4:6], 3: views[6:7]}, bases


def _bits(t):
    return t.view(_BITS[t.element_size()])


def _expect(pool, bases, pairs):
    """the bases after the copy, worked out on clones: rows move, nothing else changes"""
    want = [b.clone() for b in bases]
    tensors = [t for k in sorted(pool) for t in pool[k]]
    for t, b, w in zip(tensors, bases, want):
        off = (t.data_ptr() - b.data_ptr()) // t.element_size()
        view = w.as_strided(t.shape, t.stride(), off)
        rows = {d: t[s].clone() for s, d in pairs if 0 <= s < SLOTS and 0 <= d < SLOTS}
        for d, row in rows.items():
            view[d].copy_(row)
    return want


def _same(bases, want):
    return all(torch.equal(_bits(b), _bits(w)) for b, w in zip(bases, want))


def test_state_copy_slots_bit_for_bit():
    from dimsum_amd import native
    pool, bases = _carved()
    table = native.state_pool_table(pool)
    assert table.num_slots == SLOTS and tuple(table.table.shape) == (7, 3) and table.max_row_bytes == 320
    assert table.table.tolist() == [[t.data_ptr(), t.stride(0) * t.element_size(), t[0].numel() * t.element_size()] for t in table.tensors]
    old = [b.clone() for b in bases]
    want = _expect(pool, bases, PAIRS)
    pairs = torch.tensor(PAIRS, dtype=torch.int32, device=DEV)
    native.state_copy_slots(table, pairs)
    for t in table.tensors:                                                     # every dst row is its src, bit for bit
        assert torch.equal(_bits(t[1]), _bits(t[0])) and torch.equal(_bits(t[2]), _bits(t[0])) and torch.equal(_bits(t[4]), _bits(t[5]))
    assert _same(bases, want)                                                   # ... and slots 0, 3, 5 and all surroundings keep their bits
    for b, o in zip(bases, old):
        assert bool((b[-24:] == 7).all()) and bool((b[0] == 7).all()) and int((b == 7).sum()) >= int((o == 7).sum())     # the sentinels stand
    assert not _same(bases, old)
    native.state_copy_slots(table, pairs)                                       # again: 1, 2 <- 0 and 4 <- 5 once more, the same bits
    assert _same(bases, want)
    native.state_copy_slots(table, pairs[:0])                                   # n_pairs == 0
    native.state_copy_slots(table, [])
    assert _same(bases, want)
    # a host list goes through the checks and the same launch; the pairs' row stride is free
    want = _expect(pool, bases, [(3, 0), (3, 5)])
    native.state_copy_slots(table, [(3, 0), (-1, 2), (3, 5)])
    assert _same(bases, want)
    wide = torch.tensor([[1, 3, 99, 99], [-1, -1, 99, 99]], dtype=torch.int32, device=DEV)
    want = _expect(pool, bases, [(1, 3)])
    native.state_copy_slots(table, wide[:, :2])
    assert _same(bases, want)
    with pytest.raises(RuntimeError, match="a dst slot is also a src"):
        native.state_copy_slots(table, [(0, 1), (1, 2)])
    with pytest.raises(RuntimeError, match="pairs must be a GPU tensor"):
        native.state_copy_slots(table, torch.tensor(PAIRS, dtype=torch.int32))
    assert _same(bases, want)


def test_state_copy_slots_replays_with_rewritten_pairs():
    from dimsum_amd import native
    pool, bases = _carved(seed=1)
    table = native.state_pool_table(pool)
    pairs = torch.full((6, 2), -1, dtype=torch.int32, device=DEV)               # all padding: warm-up and capture copy nothing
    start = [b.clone() for b in bases]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        native.state_copy_slots(table, pairs)
        s.synchronize()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        native.state_copy_slots(table, pairs)
    assert _same(bases, start)                                                  # recorded, not run
    for new in (PAIRS, [(1, 0), (-1, -1), (3, 5), (2, 9), (-1, 4), (-1, -1)]):
        want = _expect(pool, bases, new)
        pairs.copy_(torch.tensor(new, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        assert _same(bases, want), new                                          # the pairs of THIS replay, nothing else touched


# ---- the engine ------------------------------------------------------------------------------------------------------------------------------------------
SEED = 5                                       # test_slots_gpu's model
GAP = 1e-3                                     # what the alone runs' smallest top-1 / top-2 gap must reach
# the token seeds were picked on the CPU stand-ins (fp32): the alone runs' gaps are 0.14, 0.19 (forks), 0.18, 0.22, 0.24, 0.39 (turns), 0.06 (samples)
PREFIX, PREFIX_SEED = 19, 0                    # the hold is cut 8 + 8 + 3 by max_prefill_tokens = 8
TAILS, TAIL_SEEDS, FORK_NEW = (3, 5), (43, 41), (4, 5)
TURNS = ((7, 71, 4, 5, 81, 3), (6, 69, 5, 0, 0, 4))       # (prompt tokens, seed, new tokens, the next turn's tokens -- one is empty --, seed, new tokens)
N_PROMPT, N_SEED, N_SAMPLES, N_NEW = 13, 30, 3, 4


def _ids(seed, n):
    return torch.randint(0, VOCAB, (n,), generator=torch.Generator().manual_seed(400 + seed))


def _engine(m, **over):
    from dimsum_amd.utils.serving import DecodeEngine
    return DecodeEngine(m, **dict(dict(max_batch=4, num_slots=6, max_seqlen=96, vocab_size=VOCAB, cg=True, output_scores=True, packed_prefill=True,
                                       prefill_rows=1, max_prefill_tokens=8, chunked_prefill=True), **over))


def _watch_copies(monkeypatch):
    """native.state_copy_slots as it is, plus a look at the pool directly after each launch -> [(pairs, every dst row equals its src)]"""
    from dimsum_amd import native
    real, seen = native.state_copy_slots, []

    def copy(table, pairs):
        real(table, pairs)
        seen.append((list(pairs), all(torch.equal(_bits(t[d]), _bits(t[s])) for t in table.tensors for s, d in pairs)))
    monkeypatch.setattr(native, "state_copy_slots", copy)
    return seen


def _check(label, eng, runs, min_gap):
    """runs: [(rid, the context alone: (sequence, scores))]. Logits first, by the gap rule; then the token ids, exactly."""
    err = max(float((torch.stack(eng.scores(rid)).float() - scores.float()).abs().max()) for rid, (_, scores) in runs)
    print(f"{label}: max |logit - alone logit| {err:.3e}, alone min_gap {min_gap:.3e}, passes {eng.prefill_pass_tokens}")
    assert err < min_gap / 4
    for rid, (seq, _) in runs:
        assert torch.equal(eng.context(rid), seq), rid


def _min_gap(runs):
    top = torch.cat([s for _, s in runs]).float().topk(2, dim=-1).values
    return float((top[:, 0] - top[:, 1]).min())


@pytest.mark.parametrize("prefill_rows", [1, 2])
def test_engine_forks_sessions_and_samples_reproduce_their_contexts_alone(prefill_rows, exact_fp32, monkeypatch):  # noqa: F811
    monkeypatch.setenv("DIMSUM_FUSED_DECODE", "1")
    torch.manual_seed(SEED)
    m = tiny_model(1, 1, vocab_size=VOCAB).to(DEV)
    seen = _watch_copies(monkeypatch)
    prefix, tails = _ids(PREFIX_SEED, PREFIX), [_ids(s, n) for s, n in zip(TAIL_SEEDS, TAILS)]
    # every reference is the full context in one plain run, alone
    fork_want = [alone(m, torch.cat([prefix, t]).to(DEV), n) for t, n in zip(tails, FORK_NEW)]
    turn_want = []
    for n_prompt, seed, new, n_turn, seed2, new2 in TURNS:
        prompt, turn = _ids(seed, n_prompt), _ids(seed2, n_turn)
        first = alone(m, prompt.to(DEV), new)
        turn_want.append((prompt, turn, new, new2, first, alone(m, torch.cat([first[0], turn]).to(DEV), new2)))
    n_prompt = _ids(N_SEED, N_PROMPT)
    n_want = alone(m, n_prompt.to(DEV), N_NEW)
    min_gap = _min_gap(fork_want + [w for *_, a, b in turn_want for w in (a, b)] + [n_want])
    assert min_gap >= GAP, min_gap                                              # a tie cannot hide a failure

    eng = _engine(m, prefill_rows=prefill_rows)
    # forks: one hold, two tails in one admission
    h = eng.hold(prefix)
    rids = [eng.submit(t, n, start=h) for t, n in zip(tails, FORK_NEW)]
    eng.run()
    slot = eng.held[h][0]
    assert eng.held[h] == (slot, PREFIX, None) and eng.prefill_pass_tokens == [8, 8, 3, sum(TAILS)]
    assert len(seen) == 1 and seen[0][1] and [s for s, _ in seen[0][0]] == [slot, slot] and len(seen[0][0]) == 2      # ONE launch, exact copies
    held_bits = [_bits(t[slot]).clone() for t in eng._pool_table.tensors]
    _check(f"forks, prefill_rows={prefill_rows}", eng, list(zip(rids, fork_want)), min_gap)
    assert sum(eng.prefill_pass_tokens) == PREFIX + sum(TAILS) != 2 * PREFIX + sum(TAILS)         # the prefix went through the model once
    # sessions: a kept request, then a turn in its slot behind the pending token
    spent = sum(eng.prefill_pass_tokens)
    for prompt, turn, new, new2, first, second in turn_want:
        r1 = eng.submit(prompt, new, keep=True)
        eng.run()
        # the last token was sampled and never fed: the state covers the prompt and new - 1 tokens
        assert eng.held[r1] == (eng.slot_history[-1][1], prompt.numel() + new - 1, int(first[0][-1]))
        r2 = eng.submit(turn, new2, start=r1, move=True)
        eng.run()
        assert eng.slot_history[-1][1] == eng.slot_history[-2][1] and r1 not in eng.held
        _check(f"session turn of {turn.numel()} tokens, prefill_rows={prefill_rows}", eng, [(r1, first), (r2, second)], min_gap)
        spent += prompt.numel() + 1 + turn.numel()                              # the prompt, the pending token, the turn: never the history
        assert sum(eng.prefill_pass_tokens) == spent
    assert len(seen) == 1                                                       # a turn copies nothing
    # submit_n: greedy samples are the alone run, three times, from one prefill
    rids = eng.submit_n(n_prompt, N_NEW, N_SAMPLES)
    eng.run()
    _check(f"submit_n, prefill_rows={prefill_rows}", eng, [(rid, n_want) for rid in rids], min_gap)
    assert sum(eng.prefill_pass_tokens) == spent + (N_PROMPT - 1) + N_SAMPLES != spent + N_SAMPLES * N_PROMPT
    assert len(seen) == 2 and seen[1][1] and len(seen[1][0]) == N_SAMPLES
    assert eng.n_captures == 1 and list(eng.held) == [h] and sorted(eng.free_slots + [slot]) == list(range(6))
    assert all(torch.equal(_bits(t[slot]), b) for t, b in zip(eng._pool_table.tensors, held_bits))   # the held slot was never written
    eng.release(h)
    assert sorted(eng.free_slots) == list(range(6))


def test_engine_forks_on_a_bf16_model(monkeypatch):
    """the fork scenario on a bfloat16 model, against the alone runs' own bf16 logits under the same gap rule"""
    monkeypatch.setenv("DIMSUM_FUSED_DECODE", "1")
    torch.manual_seed(SEED)
    m = tiny_model(1, 1, vocab_size=VOCAB).to(DEV).to(torch.bfloat16)
    seen = _watch_copies(monkeypatch)
    prefix, tails = _ids(PREFIX_SEED, PREFIX), [_ids(s, n) for s, n in zip(TAIL_SEEDS, TAILS)]
    want = [alone(m, torch.cat([prefix, t]).to(DEV), n) for t, n in zip(tails, FORK_NEW)]
    min_gap = _min_gap(want)
    assert min_gap >= GAP, min_gap
    eng = _engine(m)
    h = eng.hold(prefix)
    rids = [eng.submit(t, n, start=h) for t, n in zip(tails, FORK_NEW)]
    eng.run()
    assert len(seen) == 1 and seen[0][1] and eng.n_captures == 1 and sum(eng.prefill_pass_tokens) == PREFIX + sum(TAILS)
    assert {t.dtype for t in eng._pool_table.tensors} >= {torch.bfloat16}
    _check("forks, bf16", eng, list(zip(rids, want)), min_gap)
