"""Slot-indexed decode states on the GPU: the slot forms of causal_conv1d_update, selective_state_update (with and without dt_proj) and the
conv epilogue of decode_linear, bit for bit against the un-indexed kernels on a gathered contiguous copy of the same state rows -- the two
forms evaluate the same expressions in the same order, only the address of the state row differs, so equality is the bar and no tolerance
is used (the un-indexed kernels are pinned to float64 and to the reference fixtures by test_mixer_step_gpu.py / test_lm_gpu.py) -- on
contiguous pools, slices of wider pools, transposed and misaligned pools; one captured step replayed under changing membership against eager
steps; DecodeEngine on a tiny language model against generate() of every request alone.
Shapes: dim 130 (two waves and a partial one), batch 4 on a pool of 7 with slots [5, -1, 0, 3]. No test passes an out-of-range or a
duplicated slot: that is undefined by contract (include/dimsum_hip.h)."""
import pytest
import torch

from test_lm_cpu import tiny_model
from test_mixer_step_gpu import exact_fp32, rnd  # noqa: F401  (exact_fp32: a fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
D, POOL = 130, 7
SLOTS = {4: [5, -1, 0, 3], 8: [5, -1, 0, 3, 6, -1, 1, 2]}


def split(slots):
    """-> (live rows, their slots, padding rows, the slots nobody names)"""
    live = [b for b, s in enumerate(slots) if s >= 0]
    named = [slots[b] for b in live]
    return live, named, [b for b, s in enumerate(slots) if s < 0], sorted(set(range(POOL)) - set(named))


def make_pool(layout, inner, dtype, seed):
    """a (POOL, D, inner) pool: contiguous; a [:, :, :inner] slice of a pool 3 wider; transposed (stored (POOL, inner, D)); contiguous from
    a base one element off 16-byte alignment"""
    if layout == "contig":
        return rnd(POOL, D, inner, dtype=dtype, seed=seed)
    if layout == "slice":
        return rnd(POOL, D, inner + 3, dtype=dtype, seed=seed)[:, :, :inner]
    if layout == "transposed":
        return rnd(POOL, inner, D, dtype=dtype, seed=seed).transpose(1, 2)
    assert layout == "misaligned"
    return rnd(POOL * D * inner + 1, dtype=dtype, seed=seed)[1:].view(POOL, D, inner)


def check_against_gathered(call, pool, batch=4):
    """call(state, state_indices or None, rows or None) -> out. Runs the slot form on `pool` and the un-indexed kernel on a gathered
    contiguous copy of the live rows; everything is compared bitwise; then once more from equal inputs (reproducibility)"""
    slots = SLOTS[batch]
    live, named, pads, others = split(slots)
    idx = torch.tensor(slots, dtype=torch.int32, device=DEV)
    before = pool.clone()
    rows = before[named].contiguous()
    want = call(rows, None, live)
    out = call(pool, idx, None)
    assert torch.equal(out[live], want), "outputs of the live rows"
    assert torch.equal(pool[named], rows) and not torch.equal(rows, before[named]), "the live slots hold the un-indexed kernel's updated states"
    assert torch.equal(pool[others], before[others]), "every other slot is untouched"
    assert not out[pads].any(), "a padding row's output is exactly zero"
    after = pool.clone()
    pool.copy_(before)
    assert torch.equal(call(pool, idx, None), out) and torch.equal(pool, after), "two launches from equal inputs are bit-identical"
    return out


# ---- conv update -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("width", [2, 3, 4])
@pytest.mark.parametrize("layout", ["contig", "slice", "transposed"])
def test_conv_update_with_slots(layout, width, dtype):
    from dimsum_amd import native
    x, w, b = rnd(4, D, dtype=dtype, seed=1), rnd(D, width, seed=2), rnd(D, seed=3)
    pool = make_pool(layout, width, dtype, seed=4)

    def call(state, idx, rows):
        if idx is None:
            return native.causal_conv1d_update(x[rows], state, w, b, True)
        return native.causal_conv1d_update(x, state, w, b, True, state_indices=idx)

    check_against_gathered(call, pool)


def test_conv_update_takes_a_strided_index_and_x():
    """the index has its own element stride; x a half of a wider row (what Mamba.step hands over)"""
    from dimsum_amd import native
    xz, w = rnd(4, 2 * D, seed=5), rnd(D, 4, seed=6)
    x = xz[:, :D]
    pool = make_pool("contig", 4, torch.float32, seed=7)
    wide = torch.tensor([[s, 99] for s in SLOTS[4]], dtype=torch.int32, device=DEV)

    def call(state, idx, rows):
        if idx is None:
            return native.causal_conv1d_update(x[rows], state, w, None, False)
        return native.causal_conv1d_update(x, state, w, None, False, state_indices=wide[:, 0])

    check_against_gathered(call, pool)


# ---- state update ----------------------------------------------------------------------------------------------------------------------------------
# dstate 16: whole vector pieces; 17 in a 20-wide pool row: pieces plus a scalar tail; 5 on a misaligned contiguous pool: the element path
SSU_POOLS = [(16, "contig"), (17, "slice"), (5, "misaligned"), (16, "slice")]


# activations with a float32 state and with a state of their own dtype (for float32 the two are one case)
SSU_DTYPES = [(torch.float32, True), (torch.float16, True), (torch.float16, False), (torch.bfloat16, True), (torch.bfloat16, False)]


@pytest.mark.parametrize("dtype,state32", SSU_DTYPES, ids=lambda v: str(v))
@pytest.mark.parametrize("dt_proj", [False, True], ids=["dt", "dt_proj"])
@pytest.mark.parametrize("N,layout", SSU_POOLS, ids=["N16", "N17in20", "N5misaligned", "N16in19"])
def test_state_update_with_slots(N, layout, dt_proj, dtype, state32):
    from dimsum_amd import native
    R = 9
    x, z, dt = rnd(4, D, dtype=dtype, seed=1), rnd(4, D, dtype=dtype, seed=2), (0.5 * rnd(4, D, seed=3)).to(dtype)
    A = -0.5 * torch.rand(D, N, generator=torch.Generator().manual_seed(4)).to(DEV) - 0.1
    B, C = rnd(4, N, dtype=dtype, seed=5), rnd(4, N, dtype=dtype, seed=6)
    Dv, db = rnd(D, seed=7), 0.3 * rnd(D, seed=8)
    dt_w, dt_x = 0.3 * rnd(D, R, seed=9), rnd(4, R, dtype=dtype, seed=10)
    pool = make_pool(layout, N, torch.float32 if state32 else dtype, seed=11)

    def call(state, idx, rows):
        r = slice(None) if rows is None else rows
        kw = {} if idx is None else {"state_indices": idx}
        if dt_proj:
            return native.selective_state_update(state, x[r], None, A, B[r], C[r], Dv, z[r], db, True, dt_proj=(dt_w, dt_x[r]), **kw)
        return native.selective_state_update(state, x[r], dt[r], A, B[r], C[r], Dv, z[r], db, True, **kw)

    check_against_gathered(call, pool)


def test_ops_wrappers_take_the_index_and_match_the_restatements():
    """the public ops against their plain-torch restatements in float64 on the same pool: an independent statement of the semantics"""
    from dimsum_amd.ops import causal_conv1d_update, causal_conv1d_update_torch, selective_state_update, selective_state_update_torch
    idx = torch.tensor(SLOTS[4], dtype=torch.int32, device=DEV)
    x, w, b = rnd(4, D, seed=1), rnd(D, 4, seed=2), rnd(D, seed=3)
    pool = make_pool("contig", 4, torch.float32, seed=4)
    p64 = pool.double()
    out = causal_conv1d_update(x, pool, w, b, "silu", state_indices=idx)
    want = causal_conv1d_update_torch(x.double(), p64, w.double(), b.double(), "silu", state_indices=idx)
    assert torch.equal(pool.double(), p64) and torch.allclose(out.double(), want, rtol=3e-4, atol=1e-3)
    N = 16
    A = -0.5 * torch.rand(D, N, generator=torch.Generator().manual_seed(4)).to(DEV) - 0.1
    dt, B, C, z = 0.5 * rnd(4, D, seed=5), rnd(4, N, seed=6), rnd(4, N, seed=7), rnd(4, D, seed=8)
    pool = make_pool("contig", N, torch.float32, seed=9)
    p64 = pool.double()
    out = selective_state_update(pool, x, dt, A, B, C, b, z=z, dt_bias=None, dt_softplus=True, state_indices=idx)
    want = selective_state_update_torch(p64, x.double(), dt.double(), A.double(), B.double(), C.double(), b.double(), z.double(), None, True,
                                        state_indices=idx)
    assert torch.allclose(out.double(), want, rtol=3e-4, atol=1e-3) and torch.allclose(pool.double(), p64, rtol=3e-4, atol=1e-3)
    assert not out[1].any() and not want[1].any()


# ---- the conv epilogue of decode_linear ------------------------------------------------------------------------------------------------------------
# conv_dim 517 of N 1034 at K 40; and N >= 16384 (a wave owns four rows) with a conv_dim that is no multiple of 4: the boundary between the
# epilogue's columns and the plain ones falls inside one wave's rows
EPILOGUES = [(517, 1034, 2), (517, 1034, 3), (517, 1034, 4), (8193, 16390, 4)]


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("batch", [4, 8])
@pytest.mark.parametrize("cd,N,width", EPILOGUES, ids=lambda v: str(v))
def test_decode_linear_epilogue_with_slots(cd, N, width, batch, dtype):
    from dimsum_amd import native
    K = 40
    slots = SLOTS[batch]
    live, named, pads, others = split(slots)
    idx = torch.tensor(slots, dtype=torch.int32, device=DEV)
    x, w, b = rnd(batch, K, dtype=dtype, seed=1), rnd(N, K, dtype=dtype, seed=2) * K ** -0.5, rnd(N, dtype=dtype, seed=3)
    cw, cb = rnd(cd, width, dtype=dtype, seed=4), rnd(cd, dtype=dtype, seed=5)
    for layout in ("contig", "slice", "transposed"):
        if layout == "contig":
            pool = rnd(POOL, cd, width, dtype=dtype, seed=6)
        elif layout == "slice":
            pool = rnd(POOL, cd, width + 3, dtype=dtype, seed=6)[:, :, :width]
        else:
            pool = rnd(POOL, width, cd, dtype=dtype, seed=6).transpose(1, 2)
        before = pool.clone()
        rows = torch.zeros(batch, cd, width, dtype=dtype, device=DEV)          # the un-indexed call's states: the gathered rows, zeros for padding
        rows[live] = before[named]
        want = native.decode_linear(x, w, b, conv=(rows, cw, cb, True))
        y = native.decode_linear(x, w, b, conv=(pool, cw, cb, True), state_indices=idx)
        assert torch.equal(y[live], want[live]), layout
        assert torch.equal(y[:, cd:], want[:, cd:]) and not y[pads, :cd].any(), layout         # plain columns as ever, zeros where the conv output goes
        assert torch.equal(pool[named], rows[live]) and torch.equal(pool[others], before[others]), layout
        after = pool.clone()
        pool.copy_(before)
        assert torch.equal(native.decode_linear(x, w, b, conv=(pool, cw, cb, True), state_indices=idx), y) and torch.equal(pool, after)


def test_index_refusals_that_need_a_gpu_tensor():
    from dimsum_amd import native
    x, w, pool = rnd(4, 8), rnd(12, 8), rnd(POOL, 6, 4)
    idx = torch.tensor(SLOTS[4], dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="need `conv`"):
        native.decode_linear(x, w, state_indices=idx)
    with pytest.raises(RuntimeError, match="state_indices must be a GPU tensor"):
        native.causal_conv1d_update(rnd(4, 6), pool, rnd(6, 4), None, True, state_indices=idx.cpu())
    with pytest.raises(RuntimeError, match="pool"):
        native.causal_conv1d_update(rnd(4, 6), rnd(POOL, 5, 4), rnd(6, 4), None, True, state_indices=idx)


# ---- a tiny language model -----------------------------------------------------------------------------------------------------------------------------
SEED = 5                                                    # picked on the CPU stand-ins: the alone runs' smallest top-1 / top-2 gap is 3.7e-2
REQUESTS = [(3, 12), (9, 2), (5, 7), (7, 4), (4, 9), (6, 5)]  # (prompt tokens, new tokens)
VOCAB = 257


def lm():
    torch.manual_seed(SEED)
    m = tiny_model(1, 1, vocab_size=VOCAB).to(DEV)          # d_model 64, 2 layers, vocabulary 257 padded to 264, fused_add_norm, fp32
    g = torch.Generator().manual_seed(100 + SEED)
    return m, [torch.randint(0, VOCAB, (n,), generator=g).to(DEV) for n, _ in REQUESTS]


def alone(m, prompt, new, **kw):
    out = m.generate(prompt.unsqueeze(0), max_length=prompt.numel() + new, vocab_size=VOCAB, return_dict_in_generate=True, output_scores=True,
                     cg=False, **kw)
    return out.sequences[0].cpu(), torch.stack(out.scores)[:, 0]


def assert_a_released_slot_was_reused(eng):
    """from the engine's bookkeeping: some request was admitted into a slot that an earlier request had held"""
    seen, reused = set(), False
    for rid, slot in eng.slot_history:
        reused |= slot in seen
        seen.add(slot)
    assert reused and len(eng.slot_history) == len(REQUESTS), eng.slot_history


def test_engine_on_the_fused_step_is_bitwise_every_request_alone(exact_fp32, monkeypatch):  # noqa: F811
    from dimsum_amd.utils.serving import DecodeEngine
    monkeypatch.setenv("DIMSUM_FUSED_DECODE", "1")
    m, prompts = lm()
    want = [alone(m, p, n) for p, (_, n) in zip(prompts, REQUESTS)]
    eng = DecodeEngine(m, max_batch=4, num_slots=5, max_seqlen=32, vocab_size=VOCAB, cg=True, output_scores=True)
    rids = [eng.submit(p, n) for p, (_, n) in zip(prompts, REQUESTS)]
    out = eng.run()
    assert eng.n_captures == 1                               # one graph, however membership changed
    assert_a_released_slot_was_reused(eng)
    for rid, (seq, scores) in zip(rids, want):
        assert torch.equal(out[rid], seq), rid               # token for token
        got = torch.stack(eng.scores(rid))
        assert got.shape == scores.shape and torch.equal(got, scores), rid       # every launch of the fused step is a pure per-row function
    assert sorted(eng.free_slots) == list(range(5)) and eng.slots.tolist() == [-1] * 4


def test_engine_samples_each_request_with_its_own_uniforms(exact_fp32, monkeypatch):  # noqa: F811
    from dimsum_amd.utils.serving import DecodeEngine
    monkeypatch.setenv("DIMSUM_FUSED_DECODE", "1")
    m, prompts = lm()
    kw = dict(top_k=8, top_p=0.9, temperature=0.8)
    g = torch.Generator().manual_seed(9)
    us = [torch.rand(n, generator=g) for _, n in REQUESTS]
    want = []
    for p, (_, n), u in zip(prompts, REQUESTS, us):
        table = torch.zeros(p.numel() + n, 1)
        table[:n, 0] = u                                     # row i draws the i-th new token
        want.append(alone(m, p, n, fused_sampling=True, uniforms=table.to(DEV), **kw)[0])
    eng = DecodeEngine(m, max_batch=4, num_slots=5, max_seqlen=32, vocab_size=VOCAB, cg=True, **kw)
    rids = [eng.submit(p, n, uniforms=u) for p, (_, n), u in zip(prompts, REQUESTS, us)]
    out = eng.run()
    assert eng.n_captures == 1
    for rid, seq in zip(rids, want):
        assert torch.equal(out[rid], seq), rid
    greedy = [alone(m, p, n)[0] for p, (_, n) in zip(prompts, REQUESTS)]
    assert any(not torch.equal(a, b) for a, b in zip(want, greedy))              # the draws did something


@pytest.mark.parametrize("cg", [True, False], ids=["cg", "eager"])
def test_engine_on_the_unfused_step(cg, exact_fp32, monkeypatch):  # noqa: F811
    """the GEMVs are BLAS calls whose rows may depend on the batch: the logits within a quarter of the alone runs' smallest top-1 / top-2
    gap (the rule of test_lm_gpu.py), then equal tokens"""
    from dimsum_amd.utils.serving import DecodeEngine
    monkeypatch.setenv("DIMSUM_FUSED_DECODE", "0")
    m, prompts = lm()
    want = [alone(m, p, n) for p, (_, n) in zip(prompts, REQUESTS)]
    top = torch.cat([s for _, s in want]).topk(2, dim=-1).values
    min_gap = float((top[:, 0] - top[:, 1]).min())
    assert min_gap >= 1e-3, min_gap                          # a tie cannot hide a failure
    eng = DecodeEngine(m, max_batch=4, num_slots=5, max_seqlen=32, vocab_size=VOCAB, cg=cg, fused_sampling=cg, output_scores=True)
    rids = [eng.submit(p, n) for p, (_, n) in zip(prompts, REQUESTS)]
    out = eng.run()
    assert eng.n_captures == (1 if cg else 0)
    assert_a_released_slot_was_reused(eng)
    err = max(float((torch.stack(eng.scores(rid)) - scores).abs().max()) for rid, (_, scores) in zip(rids, want))
    print(f"unfused step, cg={cg}: max |logit - alone logit| {err:.3e}, min_gap {min_gap:.3e}")
    assert err < min_gap / 4
    for rid, (seq, _) in zip(rids, want):
        assert torch.equal(out[rid], seq), rid


@pytest.mark.parametrize("fused", ["1", "0"], ids=["fused", "unfused"])
def test_one_captured_step_serves_changing_membership(fused, exact_fp32, monkeypatch):  # noqa: F811
    """the slots buffer goes [0, 1, 2, 3] -> [4, 1, -1, 3] -> [4, 0, 2, -1] between replays of ONE graph; eager steps of the same schedule on a
    copy of the pool give the same logits and leave the same states, bit for bit"""
    from dimsum_amd.utils import InferenceParams
    monkeypatch.setenv("DIMSUM_FUSED_DECODE", fused)
    m, _ = lm()
    with torch.no_grad():
        pool_g = m.allocate_inference_cache(5, 16)
        for i, (conv, ssm) in pool_g.items():
            conv.copy_(0.5 * rnd(*conv.shape, seed=20 + i))
            ssm.copy_(0.5 * rnd(*ssm.shape, seed=30 + i))
        pool_e = {i: (c.clone(), s.clone()) for i, (c, s) in pool_g.items()}
        slots = torch.full((4,), -1, dtype=torch.int32, device=DEV)
        ids = torch.zeros(4, 1, dtype=torch.long, device=DEV)
        p_g = InferenceParams(max_seqlen=16, max_batch_size=4, seqlen_offset=1, key_value_memory_dict=pool_g, state_indices=slots)
        p_e = InferenceParams(max_seqlen=16, max_batch_size=4, seqlen_offset=1, key_value_memory_dict=pool_e, state_indices=slots)
        step = lambda p: m(ids, inference_params=p, num_last_tokens=1).logits[:, -1]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                step(p_g)                                    # warm-up with every row idle: no state is touched
            side.synchronize()
        torch.cuda.current_stream().wait_stream(side)
        for i in pool_g:
            assert all(torch.equal(a, b) for a, b in zip(pool_g[i], pool_e[i]))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            logits = step(p_g)
        g = torch.Generator().manual_seed(3)
        for member in ([0, 1, 2, 3], [4, 1, -1, 3], [4, 0, 2, -1]):
            slots.copy_(torch.tensor(member, dtype=torch.int32))
            ids.copy_(torch.randint(0, VOCAB, (4, 1), generator=g))
            graph.replay()
            want = step(p_e)
            assert torch.equal(logits, want) and bool(torch.isfinite(want).all()), member
            for i in pool_g:
                assert all(torch.equal(a, b) for a, b in zip(pool_g[i], pool_e[i])), (member, i)
