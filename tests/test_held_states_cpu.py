"""CPU tests of held states: the torch stand-in of native.state_copy_slots and the wrapper's refusals, the C entry
point's host checks in their documented order (host memory that is never dereferenced: every call fails a check or has nothing to launch), and
DecodeEngine's hold / start= / move= / keep= / submit_n on the torch stand-ins, where token equality with a plain request over the full context
is exact."""
import ctypes

import pytest
import torch

from test_host_logic import _header_layout
from test_lm_cpu import tiny_model
from test_packed_prefill_cpu import packed_backend  # noqa: F401  (a fixture)
from test_sampling_cpu import sample_logits_torch

OK, NULL, SHAPE, STRIDE, ABI = 0, 1, 3, 4, 7
PAIRS = [(0, 1), (0, 2), (-1, 3), (4, -1), (9, 3), (5, 4)]
BUDGET = 8


@pytest.fixture
def held_backend(packed_backend, monkeypatch):  # noqa: F811
    """packed_backend + the two state-copy entries replaced by their torch stand-ins; `.calls` lists the pairs of every copy launch"""
    from dimsum_amd import native
    from dimsum_amd.ops import state_copy_slots_torch, state_pool_table_torch
    calls = []

    def copy(table, pairs):
        calls.append(list(pairs))
        state_copy_slots_torch(table, pairs)
    monkeypatch.setattr(native, "state_pool_table", state_pool_table_torch)
    monkeypatch.setattr(native, "state_copy_slots", copy)
    monkeypatch.setenv("DIMSUM_FUSED_DECODE", "1")
    copy.calls = calls
    return copy


def _pool(slots=6):
    g = torch.Generator().manual_seed(3)
    mk = lambda *s, dtype=torch.float32: torch.randn(slots, *s, generator=g).to(dtype)
    wide = torch.randn(slots, 4, 9, generator=g)
    return {0: (mk(5, 3, dtype=torch.bfloat16), mk(5, 16)), 1: (mk(8, 4, dtype=torch.float16), mk(8, 1, dtype=torch.bfloat16)),
            2: (wide.view(slots, 36)[:, :20].view(slots, 5, 4), wide.view(slots, 36)[:, 20:])}      # slot stride 36 over rows of 20 and 16


# ---- the stand-in and the wrapper --------------------------------------------------------------------------------------------------------------------
def test_stand_in_copies_rows_and_skips():
    from dimsum_amd.ops import state_copy_slots_torch, state_pool_table_torch
    pool = _pool()
    table = state_pool_table_torch(pool)
    assert table.num_slots == 6 and len(table.tensors) == 6 and table.table is None and table.max_row_bytes == 5 * 16 * 4
    assert [t.data_ptr() for t in table.tensors] == [t.data_ptr() for k in sorted(pool) for t in pool[k]]           # the pool itself, in layer order
    old = [t.clone() for t in table.tensors]
    state_copy_slots_torch(table, torch.tensor(PAIRS, dtype=torch.int32))           # a tensor is taken as is: skips instead of refusals
    for t, o in zip(table.tensors, old):
        assert torch.equal(t[1], o[0]) and torch.equal(t[2], o[0]) and torch.equal(t[4], o[5])                       # one src feeds many dst
        assert torch.equal(t[[0, 3, 5]], o[[0, 3, 5]])                              # (-1, 3), (4, -1) and the out-of-range (9, 3) copy nothing
    state_copy_slots_torch(table, [])
    state_copy_slots_torch(table, [(3, 0), (-1, 2), (1, -7)])                        # a host list: padding is fine
    assert all(torch.equal(t[0], o[3]) and torch.equal(t[2], o[0]) for t, o in zip(table.tensors, old))


def test_wrapper_refusals_carry_their_reason():
    from dimsum_amd import native
    pool = _pool()
    fake = native.StatePoolTable(*native.state_pool_tensors(pool), table=torch.zeros(6, 3, dtype=torch.int64))
    for pairs, reason in (([(0, 1), (2, 1)], "a dst slot is named twice"), ([(0, 1), (1, 2)], "a dst slot is also a src"),
                          ([(3, 3)], "a dst slot is also a src"), ([(0, 6)], "out of range for num_slots = 6"), ([(9, -1)], "out of range")):
        with pytest.raises(RuntimeError, match=reason):
            native.state_copy_slots(fake, pairs)
    native.state_copy_slots(fake, [])                                                # nothing to copy: no launch, no GPU asked for
    with pytest.raises(RuntimeError, match="pairs must be a GPU tensor"):            # a clean list passes the host checks: the device comes last
        native.state_copy_slots(fake, torch.tensor([(0, 1)], dtype=torch.int32))
    for bad in (torch.zeros(2, 2), torch.zeros(4, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32)[:, ::2]):
        with pytest.raises(RuntimeError, match=r"pairs must be an int32 \(n_pairs, 2\)"):
            native.state_copy_slots(fake, bad)
    with pytest.raises(RuntimeError, match="table must come from state_pool_table"):
        native.state_copy_slots(native.StatePoolTable(*native.state_pool_tensors(pool)), [(0, 1)])
    with pytest.raises(RuntimeError, match="must live on one device"):
        native.state_pool_table({0: (torch.zeros(6, 4, 3), torch.zeros(6, 4, 2, device="meta"))})
    with pytest.raises(RuntimeError, match=r"same num_slots, got \[5, 6\]"):
        native.state_pool_table({0: (torch.zeros(6, 4, 3), torch.zeros(5, 4, 2))})
    with pytest.raises(RuntimeError, match="row must be contiguous"):
        native.state_pool_table({0: (torch.zeros(6, 4, 3).transpose(1, 2), torch.zeros(6, 4, 2))})
    with pytest.raises(RuntimeError, match="non-empty dict"):
        native.state_pool_table({})
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):                  # the device last; there is no CPU path
        native.state_pool_table(pool)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------------------------
def test_struct_symbol_and_abi_version():
    from dimsum_amd import _lib
    mirror = _lib.StateCopyParams
    size, offsets = _header_layout([("dimsum_state_copy_params_t", mirror)])["dimsum_state_copy_params_t"]
    assert size == ctypes.sizeof(mirror) == mirror().struct_size == 64
    assert offsets == {n: getattr(mirror, n).offset for n, _ in mirror._fields_}
    lib = _lib.load()
    header = open(_lib.os.path.join(_lib._HERE, "..", "include", "dimsum_hip.h")).read()
    assert lib.dimsum_abi_version() == 18 and "#define DIMSUM_ABI_VERSION 18" in header           # a new symbol only
    name = "dimsum_state_copy_slots"
    assert name in _lib.EXPORTS and hasattr(lib, name) and f"int {name}(const dimsum_state_copy_params_t *p, void *stream);" in header
    assert getattr(lib, name).argtypes[0]._type_ is mirror
    assert f"#define DIMSUM_STATE_COPY_CHUNK_BYTES {_lib.STATE_COPY_CHUNK_BYTES}" in header


def test_library_checks_in_their_documented_order():
    """each call breaks one rule AND every later one's, so the code names the first failing check; nothing is ever launched"""
    from dimsum_amd import _lib
    fn, mirror = _lib.load().dimsum_state_copy_slots, _lib.StateCopyParams
    buf = (ctypes.c_int64 * 8)()
    addr = ctypes.addressof(buf)
    assert fn(None, None) == NULL
    for delta in (-8, 8, -ctypes.sizeof(mirror) + 4):
        P = mirror()
        P.struct_size += delta
        assert fn(P, None) == ABI, delta
    P = mirror()                                                                                  # zeroed: every later rule is broken too
    assert fn(P, None) == NULL                                                                    # table_ptr
    P.table_ptr = addr
    assert fn(P, None) == NULL                                                                    # pairs_ptr
    P.pairs_ptr = addr
    assert fn(P, None) == SHAPE                                                                   # num_slots
    P.num_slots = -3
    assert fn(P, None) == SHAPE
    P.num_slots = 6
    for field in ("n_tensors", "n_pairs", "max_row_bytes"):
        setattr(P, field, -1)
        assert fn(P, None) == SHAPE, field
        setattr(P, field, 0)
    P.n_tensors, P.n_pairs, P.max_row_bytes = 2 ** 20, 2 ** 20, 2 * _lib.STATE_COPY_CHUNK_BYTES       # 2^41 workgroups
    assert fn(P, None) == SHAPE
    P.n_tensors, P.n_pairs, P.max_row_bytes = 2 ** 15, 2 ** 15, _lib.STATE_COPY_CHUNK_BYTES + 1        # 2^31
    assert fn(P, None) == SHAPE
    P.n_tensors = P.n_pairs = 0
    for stride in (-2, 0, 1):
        P.pairs_stride = stride
        assert fn(P, None) == STRIDE, stride                                                      # before "nothing to do"
    P.pairs_stride = 2
    for n_tensors, n_pairs, row in ((0, 0, 0), (0, 4, 64), (3, 0, 64), (3, 4, 0)):
        P.n_tensors, P.n_pairs, P.max_row_bytes = n_tensors, n_pairs, row
        assert fn(P, None) == OK                                                                  # nothing to do, nothing launched


# ---- the engine ------------------------------------------------------------------------------------------------------------------------------------------
def _kw(prefill_rows, **over):
    return dict(dict(max_batch=3, num_slots=5, max_seqlen=96, vocab_size=90, cg=False, fused_sampling=False, packed_prefill=True,
                     prefill_rows=prefill_rows, max_prefill_tokens=BUDGET, chunked_prefill=True), **over)


def _tokens(seed, n):
    return torch.randint(0, 90, (n,), generator=torch.Generator().manual_seed(seed))


def _plain(m, context, new, kw, uniforms=None):
    """the parent's route: a fresh engine, one plain request over the whole context -> (context + generated, the engine)"""
    from dimsum_amd.utils.serving import DecodeEngine
    eng = DecodeEngine(m, **kw)
    rid = eng.submit(context, new, uniforms)
    return eng.run()[rid], eng


def _slot_bits(eng, slot):
    return [t[slot].clone() for k in sorted(eng.pool) for t in eng.pool[k]]


@pytest.mark.parametrize("prefill_rows", [1, 2])
def test_forks_equal_plain_requests_over_the_full_context(prefill_rows, held_backend):
    from dimsum_amd.utils.serving import DecodeEngine
    m, kw = tiny_model(1, 1), _kw(prefill_rows)
    prefix, tails = _tokens(1, 19), [_tokens(2, 3), _tokens(3, 5)]                    # 19 > BUDGET: the hold itself is cut into 8 + 8 + 3
    eng = DecodeEngine(m, **kw)
    h = eng.hold(prefix)
    rids = [eng.submit(t, 4, start=h) for t in tails]
    assert eng.held == {} and not eng.idle()
    bits = None
    while not eng.idle():
        eng.step()
        if bits is None and h in eng.held:
            bits = _slot_bits(eng, eng.held[h][0])                                                # ready: from here on its slot is never written
            assert eng.held[h] == (0, 19, None) and eng.prefill_pass_tokens == [8, 8, 3] and not held_backend.calls
    assert held_backend.calls == [[(0, 1), (0, 2)]]                                               # both forks of the admission: ONE copy launch
    assert eng.prefill_pass_tokens == [8, 8, 3, 8] and eng.slot_history == [(h, 0), (rids[0], 1), (rids[1], 2)]
    assert all(torch.equal(a, b) for a, b in zip(bits, _slot_bits(eng, 0))) and h in eng.held
    for rid, t in zip(rids, tails):
        want, _ = _plain(m, torch.cat([prefix, t]), 4, kw)
        assert torch.equal(eng.context(rid), want), rid
        assert torch.equal(eng.sequence(rid), torch.cat([t, want[-4:]])), rid                     # its own prompt + what it generated
    # the handle stays valid: a third fork, alone in its admission, whose tail is cut by the budget (a resumed first piece, then another)
    t3 = _tokens(4, 11)
    r3 = eng.submit(t3, 3, start=h)
    eng.run()
    assert torch.equal(eng.context(r3), _plain(m, torch.cat([prefix, t3]), 3, kw)[0])
    assert held_backend.calls[1:] == [[(0, eng.slot_history[-1][1])]] and eng.prefill_pass_tokens[4:] == [8, 3]
    assert all(torch.equal(a, b) for a, b in zip(bits, _slot_bits(eng, 0)))
    eng.release(h)
    assert sorted(eng.free_slots) == list(range(5)) and eng.held == {}


@pytest.mark.parametrize("prefill_rows", [1, 2])
@pytest.mark.parametrize("turn", [5, 0, 12], ids=["tail5", "empty", "cut"])
def test_session_turn_equals_one_request_over_the_history(turn, prefill_rows, held_backend):
    from dimsum_amd.utils.serving import DecodeEngine
    m, kw = tiny_model(1, 1), _kw(prefill_rows)
    prompt, t2 = _tokens(5, 7), _tokens(6, turn)
    eng = DecodeEngine(m, **kw)
    r1 = eng.submit(prompt, 4, keep=True)
    first = eng.run()[r1]
    slot = eng.slot_history[0][1]
    # the last generated token was sampled but never fed: the state covers the prompt and tokens[:-1], the token itself is pending
    assert eng.held == {r1: (slot, 7 + 3, int(first[-1]))} and slot not in eng.free_slots and eng.idle()
    r2 = eng.submit(t2, 3, start=r1, move=True)
    with pytest.raises(KeyError, match="not a held state"):                                       # consumed at once
        eng.submit(t2, 3, start=r1)
    eng.run()
    want, _ = _plain(m, torch.cat([first, t2]), 3, kw)
    assert torch.equal(eng.context(r2), want) and torch.equal(eng.sequence(r2), torch.cat([t2, want[-3:]]))
    assert eng.slot_history == [(r1, slot), (r2, slot)] and not held_backend.calls                # the same slot, no copy
    assert sum(eng.prefill_pass_tokens) == 7 + 1 + turn                                           # the prompt, the pending token, the turn
    assert sorted(eng.free_slots) == list(range(5)) and eng.held == {}                            # keep=False: released as ever


def test_kept_request_ended_by_its_first_token_has_nothing_pending(held_backend):
    """max_new_tokens=1: the step of the admission has fed the only token to the model, so the state covers it and nothing is pending"""
    from dimsum_amd.utils.serving import DecodeEngine
    m, kw = tiny_model(1, 1), _kw(1)
    prompt, t2 = _tokens(7, 6), _tokens(8, 4)
    eng = DecodeEngine(m, **kw)
    r1 = eng.submit(prompt, 1, keep=True)
    first = eng.run()[r1]
    assert eng.held == {r1: (0, 7, None)}
    with pytest.raises(ValueError, match="at least one token"):
        eng.submit([], 2, start=r1, move=True)
    assert r1 in eng.held                                                                         # a refused submit consumes nothing
    r2 = eng.submit(t2, 3, start=r1, move=True, keep=True)                                        # a kept turn: the session goes on
    eng.run()
    want, _ = _plain(m, torch.cat([first, t2]), 3, kw)
    assert torch.equal(eng.context(r2), want) and eng.held == {r2: (0, 7 + 4 + 2, int(want[-1]))}


@pytest.mark.parametrize("prefill_rows", [1, 2])
def test_submit_n_draws_every_sample_from_one_prefill(prefill_rows, held_backend, monkeypatch):
    from dimsum_amd import native
    from dimsum_amd.utils.serving import DecodeEngine
    monkeypatch.setattr(native, "sample_logits", sample_logits_torch)
    m, kw = tiny_model(1, 1), _kw(prefill_rows, fused_sampling=True, top_k=0, max_batch=4, num_slots=6)
    prompt = _tokens(9, 13)
    u = torch.rand(2, 5, generator=torch.Generator().manual_seed(10))
    uniforms = torch.stack([u[0], u[1], u[0]])
    eng = DecodeEngine(m, **kw)
    rids = eng.submit_n(prompt, 5, 3, uniforms)
    out = eng.run()
    assert torch.equal(out[rids[0]], out[rids[2]]) and not torch.equal(out[rids[0]], out[rids[1]])    # equal draws, equal samples
    assert sum(eng.prefill_pass_tokens) == 12 + 3 and len(held_backend.calls) == 1 and len(held_backend.calls[0]) == 3
    assert sorted(eng.free_slots) == list(range(6)) and eng.held == {}                            # the hold went when its last fork was admitted
    for rid, row in zip(rids, uniforms):
        assert torch.equal(eng.context(rid), _plain(m, prompt, 5, kw, row)[0]) and eng.sequence(rid)[0] == prompt[-1]
    # more samples than rows: the hold outlives the first admission and goes with the last fork; a one-token prompt is n plain requests
    eng = DecodeEngine(m, **kw)
    rids = eng.submit_n(prompt, 2, 6)
    eng.step()
    eng.step()
    assert len(eng.held) == 1
    eng.run()
    assert sorted(eng.free_slots) == list(range(6)) and eng.held == {} and len(eng.requests) == 6
    assert sum(eng.prefill_pass_tokens) == 12 + 6
    rids = eng.submit_n(prompt[:1], 2, 2)
    assert [eng.requests[r].start for r in rids] == [None, None] and eng.held == {}
    eng.run()
    with pytest.raises(ValueError, match=r"uniforms must be \(n, max_new_tokens\)"):
        eng.submit_n(prompt, 2, 3, uniforms[:2])
    with pytest.raises(ValueError, match="uniforms must be"):                                     # refused by the second fork: nothing stays queued
        eng.submit_n(prompt, 2, 2, [torch.rand(2), torch.rand(3)])
    assert eng.idle() and not eng._handles and not eng._hold_reqs


def test_bookkeeping_and_refusals(held_backend):
    from dimsum_amd.utils.serving import DecodeEngine
    m, kw = tiny_model(1, 1), _kw(1, max_batch=2, num_slots=3)
    plain = DecodeEngine(m, **dict(kw, chunked_prefill=False))
    for call in (lambda: plain.hold([1, 2]), lambda: plain.submit([1], 2, keep=True), lambda: plain.submit([1], 2, start=0),
                 lambda: plain.submit([1], 2, move=True), lambda: plain.submit_n([1, 2], 2, 2)):
        with pytest.raises(ValueError, match="needs an engine with chunked_prefill=True"):
            call()
    assert plain.submit_n([1], 2, 2) == [0, 1] and plain.held == {}                               # n plain submits need nothing new
    eng = DecodeEngine(m, **kw)
    with pytest.raises(KeyError, match="not a held state"):
        eng.submit([1], 2, start=0)
    with pytest.raises(ValueError, match="needs start="):
        eng.submit([1], 2, move=True)
    with pytest.raises(ValueError, match="at least one token"):
        eng.hold([])
    h = eng.hold(_tokens(11, 12))                                                                 # two passes
    assert h == 0 and eng.held == {} and not eng.idle()                                           # handles and requests share one counter
    with pytest.raises(ValueError, match="still prefilling"):
        eng.release(h)
    with pytest.raises(ValueError, match="at least one token"):                                   # a hold has no pending token
        eng.submit([], 2, start=h)
    r1, r2 = eng.submit([3, 4], 3, start=h), eng.submit([5], 3)                                   # the plain request queues behind the fork
    assert (r1, r2) == (1, 2)
    assert eng.step() == [] and eng.rows == [None, None] and eng.free_slots == [1, 2]             # a hold takes a slot and no row
    assert list(eng.queue) == [r1, r2] and eng.held == {} and eng.slot_history == [(h, 0)]        # the unready handle blocks the queue's head
    events = eng.step()                                                                           # the hold's last piece; 4 tokens of budget are left
    assert events == [] and list(eng.queue) == [r1, r2] and eng.held == {h: (0, 12, None)} and not eng.idle()
    with pytest.raises(ValueError, match="awaited by queued forks"):
        eng.release(h)
    events = eng.step()
    assert {rid for rid, _, _ in events} == {r1, r2} and eng.rows == [r1, r2] and held_backend.calls == [[(0, 1)]]
    assert eng.slot_history == [(h, 0), (r1, 1), (r2, 2)]
    eng.run()
    assert eng.idle() and eng.held == {h: (0, 12, None)} and sorted(eng.free_slots) == [1, 2]     # idle ignores a ready hold
    with pytest.raises(ValueError, match="every one of the 3 slots would then be held"):
        eng.hold([1]), eng.hold([2])                                                              # the second one
    assert len(eng._handles) == 2
    with pytest.raises(ValueError, match="every one of the 3 slots would then be held"):
        eng.submit([1], 2, keep=True)
    eng.run()
    eng.release(1 + r2)                                                                           # the hold made above
    eng.release(h)
    assert sorted(eng.free_slots) == [0, 1, 2] and eng.held == {}
    for call in (lambda: eng.release(h), lambda: eng.submit([1], 2, start=h)):
        with pytest.raises(KeyError, match="not a held state"):
            call()
    assert set(eng.run()) == {r1, r2}                                                             # holds are no requests
