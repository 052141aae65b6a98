"""Packed prefill into slots on the GPU: the kEmit instantiations of csrc/causal_conv1d.hip and
csrc/ssm_scan_general.hip, the Mamba module's packed prompt pass and DecodeEngine(packed_prefill=True).

Kernels: EQUALITY, no tolerance. The state a launch stores for an entry end_slots[b, t] = s is held against the plain kernels on the piece
[segment start, t] of the row alone -- the plain general scan's last state (x[:, :, -1, 1::2], rounded once with .to() for a 16-bit pool),
a plain slice of x for the conv -- and out / out_z / x against dimsum_*_varlen_fwd on the same inputs, bit for bit. Slots nobody names keep
their 7.0 bit for bit, and two launches give the same bits. Entries sit at segment ends AND inside segments: the contract does not depend on
where the boundaries lie.
Module and engine: see the tests' docstrings for the rule used where two routes differ."""
import math

import pytest
import torch

from test_mixer_step_gpu import exact_fp32  # noqa: F401  (a fixture)
from test_slots_gpu import REQUESTS, VOCAB, alone, assert_a_released_slot_was_reused, lm

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def layout(ends_rows, L):
    """ends_rows: per row [(t, boundary_after)] in ascending t -> (seq_idx, end_slots, [(row, segment start, t, slot)], num_slots): an entry
    stores the state after position t; boundary_after says whether the next position starts a new segment (an entry need not end one).
    Slots are handed out in a scrambled order and three of the pool belong to nobody."""
    n = sum(len(r) for r in ends_rows)
    num_slots = n + 3
    order = [(7 * i + 2) % num_slots for i in range(num_slots)]             # a permutation when 7 does not divide num_slots
    if len(set(order)) != num_slots:
        order = list(range(num_slots))[::-1]
    seq = torch.zeros(len(ends_rows), L, dtype=torch.int32)
    ends = torch.full((len(ends_rows), L), -1, dtype=torch.int32)
    entries, k = [], 0
    for r, row in enumerate(ends_rows):
        start, sid = 0, 0
        for t, cut in row:
            ends[r, t] = order[k]
            entries.append((r, start, t, order[k]))
            k += 1
            if cut and t + 1 < L:
                seq[r, t + 1:] = sid + 1
                sid, start = sid + 1, t + 1
    return seq, ends, entries, num_slots


def make_pool(kind, num_slots, dim, n, dtype):
    """a 7.0-filled pool (num_slots, dim, n) in one of the layouts, with the buffer it lives in"""
    if kind == "contig":
        base = torch.full((num_slots, dim, n), 7.0, dtype=dtype, device=DEV)
        return base, base
    if kind == "slice":
        base = torch.full((num_slots, dim, n + 5), 7.0, dtype=dtype, device=DEV)
        return base[:, :, :n], base
    if kind == "transposed":
        base = torch.full((num_slots, n, dim), 7.0, dtype=dtype, device=DEV)
        return base.transpose(1, 2), base
    base = torch.full((num_slots * dim * n + 1,), 7.0, dtype=dtype, device=DEV)               # one element off 16-byte alignment
    pool = base[1:].view(num_slots, dim, n)
    assert pool.data_ptr() % 16 != 0
    return pool, base


POOLS = ["contig", "slice", "transposed", "offset"]


# ---- the scan ------------------------------------------------------------------------------------------------------------------------------------------
# L = 23 (L % 4 = 3; a tile is 4 steps): entries at t % 4 = 0, 1, 2, 3, at consecutive positions (segments of length 1), two in one tile
# (5 and 6), one inside a segment (9), one at L - 1
SCAN_ROWS = [[(0, True), (1, True), (2, True), (3, True), (5, True), (6, True), (9, False), (12, True), (22, True)],
             [(22, True)],                                                 # one segment, its end at L - 1
             [(3, True), (7, False), (11, True)]]                           # the rest of the row is a padding segment that stores nothing


def scan_inputs(batch, dim, N, L, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    t = dict(u=r(batch, dim, L).to(dtype), delta=(0.5 * torch.rand(batch, dim, L, generator=g)).to(dtype), A=-torch.rand(dim, N, generator=g) - 0.05,
             B=r(batch, 1, N, L).to(dtype), C=r(batch, 1, N, L).to(dtype), D=r(dim), z=r(batch, dim, L).to(dtype), bias=0.5 * torch.rand(dim, generator=g))
    return {k: v.to(DEV) for k, v in t.items()}


def run_scan(ends_rows, dim, N, L, dtype, pool_dtype, pool_kind, seed):
    from dimsum_amd import native
    seq, ends, entries, num_slots = layout(ends_rows, L)
    g = scan_inputs(len(ends_rows), dim, N, L, dtype, seed)
    args = lambda sl=slice(None), rows=slice(None): (g["u"][rows, :, sl], g["delta"][rows, :, sl], g["A"], g["B"][rows, :, :, sl], g["C"][rows, :, :, sl],
                                                    g["D"], g["z"][rows, :, sl], g["bias"], True)
    sq, en = seq.to(DEV), ends.to(DEV)
    pool, base = make_pool(pool_kind, num_slots, dim, N, pool_dtype)
    out, x, out_z = native.selective_scan_varlen_states_fwd(*args(), sq, en, pool)
    ref_out, ref_x, ref_out_z = native.selective_scan_varlen_fwd(*args(), sq)
    assert torch.equal(out, ref_out) and torch.equal(x, ref_x) and torch.equal(out_z, ref_out_z)          # the other outputs: untouched
    first = base.clone()
    named = set()
    for r, start, t, slot in entries:
        _, xa, _ = native.selective_scan_general_fwd(*args(slice(start, t + 1), slice(r, r + 1)))
        want = xa[0, :, -1, 1::2].to(pool_dtype)
        assert torch.equal(pool[slot], want), f"row {r} piece [{start}, {t}] slot {slot}: max diff {float((pool[slot].float() - want.float()).abs().max()):.3e}"
        named.add(slot)
    for s in set(range(num_slots)) - named:
        assert bool((pool[s] == 7.0).all()), s
    mask = torch.ones(num_slots, dtype=torch.bool)
    mask[list(named)] = False
    if pool_kind == "contig":
        assert bool((base[mask.to(DEV)] == 7.0).all())
    else:                                                                   # everything of the buffer outside the named slots' elements
        probe = torch.zeros_like(base, dtype=torch.bool)
        view = probe[:, :, :N] if pool_kind == "slice" else probe.transpose(1, 2) if pool_kind == "transposed" else probe[1:].view(num_slots, dim, N)
        view[list(named)] = True
        assert bool((base[~probe] == 7.0).all())
    native.selective_scan_varlen_states_fwd(*args(), sq, en, pool)
    assert torch.equal(base, first)                                         # two launches, the same bits


@pytest.mark.parametrize("N", [16, 17, 64, 80])
@pytest.mark.parametrize("dt,pool_f32", [("f32", True), ("f16", True), ("f16", False), ("bf16", True), ("bf16", False)])
def test_scan_stores_the_state_after_every_named_position(dt, pool_f32, N):
    """dim 130 (two full 64-channel blocks and a partial one), batch 3 and 1; dstate 16 (one wave), 17 (a second, nearly empty wave), 64,
    80 (the 1024-work-item instantiation); the pool layouts in turn"""
    dtype = DTYPES[dt]
    pool_dtype = torch.float32 if pool_f32 else dtype
    k = [16, 17, 64, 80].index(N) + (2 if pool_f32 else 0)
    run_scan(SCAN_ROWS, 130, N, 23, dtype, pool_dtype, POOLS[k % 4], seed=N)
    run_scan(SCAN_ROWS[:1], 130, N, 23, dtype, pool_dtype, POOLS[(k + 1) % 4], seed=N + 1)


def test_scan_across_the_chunk_edge():
    """L = 2051, batch 1: one segment from 2040 on spans the 2048-step chunk edge, with entries at 2047 and 2048 inside it and at L - 1"""
    rows = [[(5, True), (2039, True), (2047, False), (2048, False), (2050, True)]]
    run_scan(rows, 130, 16, 2051, torch.float32, torch.float32, "contig", seed=3)
    run_scan(rows, 70, 80, 2051, torch.bfloat16, torch.bfloat16, "transposed", seed=4)


# ---- the conv ------------------------------------------------------------------------------------------------------------------------------------------
def conv_rows(L):
    """entries at t = 0 (a segment of length 1), 2 (length 2), 5 (length 3), 255 / 256 / 257 / 258 (the carried halo of the 256-element step;
    three segments of length 1), one inside a segment (300) and L - 1; a row with one entry; a row whose tail is padding"""
    return [[(0, True), (2, True), (5, True), (255, True), (256, True), (257, True), (258, True), (300, False), (L - 1, True)],
            [(L - 1, True)],
            [(1, True), (258, False), (259, True)]]


def run_conv(ends_rows, dim, width, L, dtype, pool_kind, seed, misalign=False, act=True, bias=True):
    from dimsum_amd import native
    seq, ends, entries, num_slots = layout(ends_rows, L)
    batch = len(ends_rows)
    g = torch.Generator().manual_seed(seed)
    if misalign:                                                            # x one element off 16-byte alignment: the scalar path at L % 4 == 0
        buf = torch.randn(batch * dim * L + 1, generator=g).to(dtype).to(DEV)
        x = buf[1:].view(batch, dim, L)
    else:
        x = torch.randn(batch, dim, L, generator=g).to(dtype).to(DEV)
    w = torch.randn(dim, width, generator=g).to(DEV)
    b = torch.randn(dim, generator=g).to(DEV) if bias else None
    sq, en = seq.to(DEV), ends.to(DEV)
    pool, base = make_pool(pool_kind, num_slots, dim, width, dtype)
    out = native.causal_conv1d_varlen_states_fwd(x, w, b, act, sq, en, pool)
    assert torch.equal(out, native.causal_conv1d_varlen_fwd(x, w, b, act, sq))
    first = base.clone()
    named = set()
    for r, start, t, slot in entries:
        piece = x[r, :, max(start, t - width + 1):t + 1]                    # a plain slice of x: moved, not converted
        want = torch.nn.functional.pad(piece, (width - piece.shape[-1], 0))
        assert torch.equal(pool[slot], want), f"row {r} piece [{start}, {t}] slot {slot}"
        named.add(slot)
    probe = torch.zeros_like(base, dtype=torch.bool)
    view = {"contig": lambda: probe, "slice": lambda: probe[:, :, :width], "transposed": lambda: probe.transpose(1, 2),
            "offset": lambda: probe[1:].view(num_slots, dim, width)}[pool_kind]()
    view[list(named)] = True
    assert bool((base[~probe] == 7.0).all())                                # unnamed slots and everything around the pool: untouched
    native.causal_conv1d_varlen_states_fwd(x, w, b, act, sq, en, pool)
    assert torch.equal(base, first)


@pytest.mark.parametrize("width", [2, 3, 4])
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_conv_stores_the_tail_of_every_named_position(dt, width):
    """dim 130: batch 3 (390 rows) and batch 1 (130 rows), neither a multiple of the 16 rows of a workgroup pass, so clamped rows exist.
    L = 520 on the 16-byte path, L = 523 and a misaligned x on the scalar path; the pool layouts in turn"""
    dtype = DTYPES[dt]
    k = width + list(DTYPES).index(dt)
    run_conv(conv_rows(520), 130, width, 520, dtype, POOLS[k % 4], seed=width)
    run_conv(conv_rows(523), 130, width, 523, dtype, POOLS[(k + 1) % 4], seed=width + 10)
    run_conv(conv_rows(520)[:1], 130, width, 520, dtype, POOLS[(k + 2) % 4], seed=width + 20, misalign=True, act=False, bias=False)
    run_conv(conv_rows(520)[:1], 130, width, 520, dtype, POOLS[(k + 3) % 4], seed=width + 30)


def test_native_refuses_a_pool_of_another_dtype():
    from dimsum_amd import _lib, native
    x, w = torch.randn(1, 8, 8, device=DEV), torch.randn(8, 4, device=DEV)
    seq, ends = torch.zeros(1, 8, dtype=torch.int32, device=DEV), torch.full((1, 8), -1, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="conv_state must have x's dtype"):
        native.causal_conv1d_varlen_states_fwd(x, w, None, True, seq, ends, torch.zeros(2, 8, 4, device=DEV, dtype=torch.float16))
    E = _lib.ConvVarlenStatesParams()                                       # the entry point itself: DIMSUM_ERR_UNSUPPORTED, nothing launched
    pool, out = torch.full((2, 8, 4), 7.0, device=DEV, dtype=torch.float16), torch.full_like(x, 7.0)
    native._fill_conv(E.varlen.conv, x, w, None, True, out)
    E.varlen.seq_idx_ptr, E.varlen.seq_idx_batch_stride = seq.data_ptr(), 8
    E.num_slots, E.end_slots_ptr, E.end_slots_batch_stride, E.state_ptr, E.state_dtype = 2, ends.data_ptr(), 8, pool.data_ptr(), 1
    E.state_slot_stride, E.state_c_stride, E.state_w_stride = pool.stride()
    assert _lib.load().dimsum_causal_conv1d_varlen_states_fwd(E, None) == 5
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((pool == 7.0).all())


# ---- the module ----------------------------------------------------------------------------------------------------------------------------------------
def ulp(x, dtype=torch.float32):
    return 2.0 ** (math.floor(math.log2(max(float(x), 2.0 ** -126))) - (23 if dtype == torch.float32 else 10 if dtype == torch.float16 else 7))


def mixer_states_f64(m, x, seq, ends, num_slots):
    """the mixer's conv and SSM pools after a packed prompt pass, in float64 on the restatements: in_proj -> conv -> x_proj / dt_proj -> scan"""
    from dimsum_amd.ops import causal_conv1d_varlen_torch, selective_scan_varlen_torch
    d = lambda t: t.detach().double().cpu()
    D, R, N = m.d_inner, m.dt_rank, m.d_state
    xz = (d(x) @ d(m.in_proj.weight).t()).transpose(1, 2)                   # (B, 2 D, L)
    conv_pool = torch.zeros(num_slots, D, m.d_conv, dtype=torch.float64)
    ssm_pool = torch.zeros(num_slots, D, N, dtype=torch.float64)
    cw = d(m.conv1d.weight).reshape(D, -1)
    conv_out = causal_conv1d_varlen_torch(xz[:, :D], cw, d(m.conv1d.bias), "silu", seq, end_slots=ends, conv_state=conv_pool)
    x_dbl = conv_out.transpose(1, 2) @ d(m.x_proj.weight).t()               # (B, L, R + 2N)
    delta = (x_dbl[..., :R] @ d(m.dt_proj.weight).t()).transpose(1, 2)
    Bm, Cm = x_dbl[..., R:R + N].transpose(1, 2), x_dbl[..., R + N:].transpose(1, 2)
    selective_scan_varlen_torch(conv_out, delta, -torch.exp(d(m.A_log)), Bm, Cm, d(m.D), xz[:, D:], d(m.dt_proj.bias), True, seq_idx=seq,
                                end_slots=ends, ssm_state=ssm_pool)
    return conv_pool, ssm_pool


def test_mamba_packed_pass_fills_the_slots_like_alone_prefills(exact_fp32):  # noqa: F811
    """Mamba.forward(seq_idx=, inference_params with prefill_slots) on a pool against each segment prefilled alone into a batch-1 cache
    through the same seq_idx route (a single-segment id row). Equality where it holds; where the in_proj / x_proj GEMMs are not
    row-count-invariant the packed-row bound applies: |packed - float64| <= 2 |alone - float64| + one ulp of the state's dtype at the
    largest reference value (the float64 side: the restatements)."""
    from dimsum_amd.modules.mamba_simple import Mamba
    from dimsum_amd.utils import InferenceParams, plan_packed_prefill
    torch.manual_seed(2)
    m = Mamba(64, d_state=16, d_conv=4, expand=2, layer_idx=0).to(DEV).eval()
    lengths, slots = [5, 1, 9, 2, 3, 7], [4, 0, 6, 2, 7, 1]
    for rows in (1, 2):
        plan = plan_packed_prefill(lengths, slots, rows=rows, pad_multiple=4)
        x = torch.randn(rows, plan["seqlen"], 64, generator=torch.Generator().manual_seed(rows)).to(DEV)
        pool = tuple(t.fill_(7.0) for t in m.allocate_inference_cache(9, 32))
        seq, ends = plan["seq_idx"].to(DEV), plan["end_slots"].to(DEV)
        with torch.no_grad():
            y = m(x, seq_idx=seq, inference_params=InferenceParams(32, rows, key_value_memory_dict={0: pool}, prefill_slots=ends))
            assert torch.equal(y, m(x, seq_idx=seq))                        # the outputs are the packed pass's
            conv64, ssm64 = mixer_states_f64(m, x, plan["seq_idx"], plan["end_slots"], 9)
            equal, e_p, e_a, big = True, [0.0, 0.0], [0.0, 0.0], [0.0, 0.0]
            for (r, start), n, s in zip(plan["segments"], lengths, slots):
                own = InferenceParams(32, 1)
                m(x[r:r + 1, start:start + n], seq_idx=torch.zeros(1, n, dtype=torch.int32, device=DEV), inference_params=own)
                for k, (got, want, ref) in enumerate(zip((pool[0][s], pool[1][s]), own.key_value_memory_dict[0], (conv64[s], ssm64[s]))):
                    equal &= torch.equal(got, want[0])
                    e_p[k] = max(e_p[k], float((got.double().cpu() - ref).abs().max()))
                    e_a[k] = max(e_a[k], float((want[0].double().cpu() - ref).abs().max()))
                    big[k] = max(big[k], float(ref.abs().max()))
        for k, name in enumerate(("conv_state", "ssm_state")):
            bound = 2 * e_a[k] + ulp(big[k])
            print(f"rows={rows} {name}: bit-identical to the alone prefills {equal}; packed err {e_p[k]:.3e}, alone err {e_a[k]:.3e}, bound {bound:.3e}")
            assert equal or e_p[k] <= bound, name
        for t in pool:
            assert bool((t[[3, 5, 8]] == 7.0).all())                        # unnamed slots untouched


# ---- the engine ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefill_rows", [1, 2])
def test_engine_with_packed_prefill_reproduces_every_request_alone(prefill_rows, exact_fp32, monkeypatch):  # noqa: F811
    """six requests (prompts of 3..9 tokens, 2..12 new tokens), greedy with pinned uniforms, on DecodeEngine(max_batch=4, num_slots=5,
    cg=True, packed_prefill=True): every sequence equals generate() of that request alone. The packed pass runs the general scan and GEMMs
    over other row counts, so the logits follow the rule of test_slots_gpu.py where routes differ: max |logit - alone logit| < min_gap / 4
    with min_gap the smallest top-1 / top-2 gap of the ALONE runs (seed 5 of test_slots_gpu.lm(): checked below to be >= 1e-3)."""
    from dimsum_amd.utils.serving import DecodeEngine
    monkeypatch.setenv("DIMSUM_FUSED_DECODE", "1")
    m, prompts = lm()
    want = [alone(m, p, n) for p, (_, n) in zip(prompts, REQUESTS)]
    top = torch.cat([s for _, s in want]).topk(2, dim=-1).values
    min_gap = float((top[:, 0] - top[:, 1]).min())
    assert min_gap >= 1e-3, min_gap                                         # a tie cannot hide a failure
    passes = []
    hook = m.register_forward_pre_hook(lambda mod, args, kwargs: passes.append(tuple(args[0].shape)) if kwargs.get("seq_idx") is not None else None,
                                       with_kwargs=True)
    eng = DecodeEngine(m, max_batch=4, num_slots=5, max_seqlen=32, vocab_size=VOCAB, cg=True, output_scores=True, packed_prefill=True,
                       prefill_rows=prefill_rows)
    for conv, ssm in eng.pool.values():
        conv.fill_(7.0)
        ssm.fill_(7.0)
    g = torch.Generator().manual_seed(9)
    rids = [eng.submit(p, n, uniforms=torch.rand(n, generator=g)) for p, (_, n) in zip(prompts, REQUESTS)]
    with torch.no_grad():
        eng._admit()                                                            # the first admission alone: four requests, one pass, slots 0..3
    assert passes == [(prefill_rows, passes[0][1])] and eng.n_prefill_passes == 1 and [s for _, s in eng.slot_history] == [0, 1, 2, 3]
    for conv, ssm in eng.pool.values():
        assert bool((conv[4] == 7.0).all()) and bool((ssm[4] == 7.0).all())     # the slot nobody named: untouched by the admission
        assert not bool((conv[:4] == 7.0).all(-1).all(-1).any()) and not bool((ssm[:4] == 7.0).any())
    out = eng.run()
    hook.remove()
    assert eng.n_captures == 1 and eng.n_prefill_passes < len(REQUESTS)
    assert_a_released_slot_was_reused(eng)
    err = max(float((torch.stack(eng.scores(rid)) - scores).abs().max()) for rid, (_, scores) in zip(rids, want))
    print(f"packed prefill, prefill_rows={prefill_rows}: max |logit - alone logit| {err:.3e}, alone min_gap {min_gap:.3e}, prompt passes {eng.n_prefill_passes}")
    assert err < min_gap / 4
    for rid, (seq, _) in zip(rids, want):
        assert torch.equal(out[rid], seq), rid
    assert sorted(eng.free_slots) == list(range(5)) and eng.slots.tolist() == [-1] * 4
