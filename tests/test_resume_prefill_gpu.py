"""Resumed packed prefill on the GPU: the kStart instantiations of csrc/ssm_scan_general.hip and
csrc/causal_conv1d.hip, and DecodeEngine(chunked_prefill=True).

Kernels: EQUALITY, no tolerance. A resumed segment's out / out_z and the state it stores are held against the plain general scan on that piece
alone entered with initial_state= the same values (dimsum_ssm_scan_carry_fwd: the same instruction sequence per step); the conv's stored states
against plain slices of concat(initial_states[s], piece), and its out against dimsum_causal_conv1d_varlen_fwd on a row where every resumed
segment is written out with its width - 1 carried values in front under the same id (the same expression on the same values). Memory nobody
names keeps its bits, and two launches from equal inputs give the same bits."""
import pytest
import torch

from test_mixer_step_gpu import exact_fp32  # noqa: F401  (a fixture)
from test_packed_prefill_gpu import DTYPES, make_pool, scan_inputs
from test_slots_gpu import VOCAB, alone

pytestmark = pytest.mark.gpu
DEV = "cuda"
POOLS = ["contig", "slice", "transposed"]


def rows_of(segs_rows, L, first_slot=0):
    """segs_rows: per row [(start, length, resumed, stored)] in ascending order, what follows the last segment is padding ->
    seq_idx, end_slots, start_slots (init row k at the k-th resumed segment, pool slot k at the k-th stored one; scrambled), entries
    [(row, start, length, init row or -1, slot or -1)], n_init, num_slots"""
    n_res = sum(s[2] for r in segs_rows for s in r)
    n_end = sum(s[3] for r in segs_rows for s in r)
    n_init, num_slots = n_res + 2, n_end + 3
    perm = lambda n: [(5 * i + 1) % n for i in range(n)] if n % 5 else list(range(n))[::-1]
    ip, sp = perm(n_init), perm(num_slots)
    B = len(segs_rows)
    seq, ends, starts = torch.zeros(B, L, dtype=torch.int32), torch.full((B, L), -1, dtype=torch.int32), torch.full((B, L), -1, dtype=torch.int32)
    entries, ki, ke = [], 0, 0
    for r, row in enumerate(segs_rows):
        t = 0
        for sid, (start, n, resumed, stored) in enumerate(row):
            assert start == t
            seq[r, start:start + n] = sid
            a = e = -1
            if resumed:
                a, ki = ip[ki], ki + 1
                starts[r, start] = a
            if stored:
                e, ke = sp[ke], ke + 1
                ends[r, start + n - 1] = e
            entries.append((r, start, n, a, e))
            t = start + n
        seq[r, t:] = len(row)
    return seq, ends, starts, entries, n_init, num_slots


def lens(*lengths, skip=()):
    """consecutive segments of these lengths from 0, all resumed and stored except the indices in `skip` (neither)"""
    out, t = [], 0
    for i, n in enumerate(lengths):
        out.append((t, n, i not in skip, i not in skip))
        t += n
    return out


# ---- the scan ------------------------------------------------------------------------------------------------------------------------------------------
# L = 23: starts at t = 0, 1, 3, 5, 6 (two in the tile 4..7), 9, 10, 15, 16: t % 4 = 0, 1, 3, 1, 2, 1, 2, 3, 0; segments of 1, 2 and 3 tokens
SCAN_ROWS = [lens(1, 2, 2, 1, 3, 1, 5, 1, 7),
             lens(23),
             [(0, 4, False, True), (4, 8, True, False)]]                   # from zeros into a slot; a continuation that stores nothing; padding


def run_scan(segs_rows, dim, N, L, dtype, state_dtype, kind, seed, in_place=False):
    from dimsum_amd import native
    seq, ends, starts, entries, n_init, num_slots = rows_of(segs_rows, L)
    g = scan_inputs(len(segs_rows), dim, N, L, dtype, seed)
    sq, en, st = seq.to(DEV), ends.to(DEV), starts.to(DEV)
    gen = torch.Generator().manual_seed(seed + 77)
    pool, base = make_pool(kind, num_slots, dim, N, state_dtype)
    if in_place:                                                            # every resumed-and-stored segment goes s -> s of the pool itself
        entries = [(r, s, n, e if a >= 0 and e >= 0 else a, e) for r, s, n, a, e in entries]
        assert all(a == e for _, _, _, a, e in entries if a >= 0)
        for r, s, n, a, e in entries:
            if a >= 0:
                st[r, s] = a
                pool[a] = torch.randn(dim, N, generator=gen).to(state_dtype).to(DEV)
        init, init_base = pool, base
    else:
        init, init_base = make_pool(POOLS[(POOLS.index(kind) + 1) % 3], n_init, dim, N, state_dtype)
        init.copy_(torch.randn(n_init, dim, N, generator=gen).to(state_dtype))
    before, init_before = base.clone(), init_base.clone()
    args = (g["u"], g["delta"], g["A"], g["B"], g["C"], g["D"], g["z"], g["bias"], True)
    out, x, out_z = native.selective_scan_varlen_resume_fwd(*args, sq, en, pool, st, init)
    if not in_place:
        assert torch.equal(init_base, init_before)                          # init and what surrounds it: read only
    named = set()
    for r, s, n, a, e in entries:
        sl, rw = slice(s, s + n), slice(r, r + 1)
        h0 = (before if in_place else init_before)
        h0 = (pool_view(h0, kind if in_place else POOLS[(POOLS.index(kind) + 1) % 3], N, dim)[a:a + 1].clone() if a >= 0
              else torch.zeros(1, dim, N, dtype=state_dtype, device=DEV))
        hT = torch.empty_like(h0)
        piece = (g["u"][rw, :, sl], g["delta"][rw, :, sl], g["A"], g["B"][rw, :, :, sl], g["C"][rw, :, :, sl], g["D"])
        want_z = native.selective_scan_carry_fwd(*piece, g["z"][rw, :, sl], g["bias"], True, h0, hT)
        want = native.selective_scan_carry_fwd(*piece, None, g["bias"], True, h0, None)
        assert torch.equal(out_z[rw, :, sl], want_z) and torch.equal(out[rw, :, sl], want), f"row {r} segment [{s}, {s + n}) from {a}"
        if e >= 0:
            assert torch.equal(pool[e], hT[0]), f"row {r} segment [{s}, {s + n}) from {a} into {e}: {float((pool[e].float() - hT[0].float()).abs().max()):.3e}"
            named.add(e)
    probe = torch.zeros_like(base, dtype=torch.bool)
    pool_view(probe, kind, N, dim)[sorted(named)] = True
    assert torch.equal(base[~probe], before[~probe])                        # unnamed slots (7.0) and everything around the pool
    if not in_place:
        assert bool((base[~probe] == 7.0).all())
    again, again_base = make_pool(kind, num_slots, dim, N, state_dtype)
    again_base.copy_(before)
    o2, _, oz2 = native.selective_scan_varlen_resume_fwd(*args, sq, en, again, st, again if in_place else init)
    assert torch.equal(again_base, base) and torch.equal(o2, out) and torch.equal(oz2, out_z)       # equal inputs, the same bits


def pool_view(base, kind, n, dim):
    return base if kind == "contig" else base[:, :, :n] if kind == "slice" else base.transpose(1, 2)


@pytest.mark.parametrize("N", [16, 17, 64, 80])
@pytest.mark.parametrize("dt,f32_state", [("f32", True), ("f16", True), ("f16", False), ("bf16", True), ("bf16", False)])
def test_scan_resumes_every_segment_from_its_slot(dt, f32_state, N):
    """dim 130 at batch 3 and 1; dstate 16, 17, 64 (256 work-items) and 80 (the 1024-work-item instantiation); f32 and same-dtype states;
    the layouts in turn; then IN PLACE: every segment from slot s into slot s of one tensor"""
    dtype = DTYPES[dt]
    sd = torch.float32 if f32_state else dtype
    k = [16, 17, 64, 80].index(N) + f32_state
    run_scan(SCAN_ROWS, 130, N, 23, dtype, sd, POOLS[k % 3], seed=N)
    run_scan(SCAN_ROWS[:1], 130, N, 23, dtype, sd, POOLS[(k + 1) % 3], seed=N + 1)
    run_scan(SCAN_ROWS[:2], 130, N, 23, dtype, sd, POOLS[(k + 2) % 3], seed=N + 2, in_place=True)


def test_scan_resumes_across_the_chunk_edge():
    """L = 2051, batch 1: starts at 2047 and 2048, either side of the 2048-step chunk edge"""
    rows = [lens(2047, 1, 3)]
    run_scan(rows, 130, 16, 2051, torch.float32, torch.float32, "contig", seed=3)
    run_scan(rows, 70, 80, 2051, torch.bfloat16, torch.bfloat16, "transposed", seed=4, in_place=True)


@pytest.mark.parametrize("dt,f32_state", [("f32", True), ("bf16", True), ("bf16", False)])
@pytest.mark.parametrize("N", [16, 80])
def test_scan_chain_of_pieces_is_the_unsplit_scan(dt, f32_state, N):
    """40 tokens in pieces of 1, 2, 3, 5, 29 through one slot of a pool over five launches, each piece behind an unrelated 3-token segment
    (so its place in the 4-step tile moves). f32 pool: out and the final state equal ONE unsplit launch of the same kernels, bit for bit (the
    per-step expressions do not depend on the tile position). 16-bit pool: the state is rounded at every hand-over, so the comparison is the
    plain kernel run piecewise with the same rounding."""
    from dimsum_amd import native
    dtype = DTYPES[dt]
    sd = torch.float32 if f32_state else dtype
    dim, T, pre = 130, 40, 3
    g = scan_inputs(1, dim, N, T, dtype, seed=N)
    pool = torch.full((4, dim, N), 7.0, dtype=sd, device=DEV)
    t, outs = 0, []
    for i, n in enumerate([1, 2, 3, 5, 29]):
        seq, ends, starts, _, _, _ = rows_of([[(0, pre, False, False), (pre, n, i > 0, True)]], pre + n)
        ends[ends >= 0], starts[starts >= 0] = 2, 2
        f = scan_inputs(1, dim, N, pre + n, dtype, seed=100 + i)               # the neighbour's inputs; the piece's are copied in
        for k in ("u", "delta", "B", "C", "z"):
            f[k][..., pre:] = g[k][..., t:t + n]
        _, _, oz = native.selective_scan_varlen_resume_fwd(f["u"], f["delta"], g["A"], f["B"], f["C"], g["D"], f["z"], g["bias"], True, seq.to(DEV),
                                                           ends.to(DEV), pool, starts.to(DEV), pool)
        outs.append(oz[:, :, pre:])
        t += n
    got = torch.cat(outs, -1)
    if f32_state:
        one = torch.full((1, dim, N), 7.0, dtype=sd, device=DEV)
        ends = torch.full((1, T), -1, dtype=torch.int32, device=DEV)
        ends[0, -1] = 0
        _, _, want = native.selective_scan_varlen_states_fwd(g["u"], g["delta"], g["A"], g["B"], g["C"], g["D"], g["z"], g["bias"], True,
                                                             torch.zeros(1, T, dtype=torch.int32, device=DEV), ends, one)
        state = one[0]
    else:
        h, t, wants = torch.zeros(1, dim, N, dtype=sd, device=DEV), 0, []
        for n in [1, 2, 3, 5, 29]:
            sl = slice(t, t + n)
            wants.append(native.selective_scan_carry_fwd(g["u"][:, :, sl], g["delta"][:, :, sl], g["A"], g["B"][..., sl], g["C"][..., sl], g["D"],
                                                         g["z"][:, :, sl], g["bias"], True, h, h))
            t += n
        want, state = torch.cat(wants, -1), h[0]
    assert torch.equal(got, want), float((got.float() - want.float()).abs().max())
    assert torch.equal(pool[2], state) and bool((pool[[0, 1, 3]] == 7.0).all())


# ---- the conv ------------------------------------------------------------------------------------------------------------------------------------------
def conv_rows(L):
    """starts at 0, 255, 256, 257, 258 (the lane-63 -> lane-0 halo across a 256-element step), segments of 1, 1, 1, 2 and 3 tokens there
    (at width 4 the carried values shift), one segment from zeros; a row that is one resumed segment; a row without any start entry"""
    return [lens(255, 1, 1, 1, 2, 3, 40, L - 303, skip=(6,)),
            lens(L),
            [(0, 7, False, True), (7, L - 20, False, True)]]


def run_conv(segs_rows, dim, width, L, dtype, kind, seed, misalign=False, act=True, bias=True):
    from dimsum_amd import native
    seq, ends, starts, entries, n_init, num_slots = rows_of(segs_rows, L)
    batch = len(segs_rows)
    g = torch.Generator().manual_seed(seed)
    if misalign:                                                            # x one element off 16-byte alignment: the scalar path at L % 4 == 0
        x = torch.randn(batch * dim * L + 1, generator=g).to(dtype).to(DEV)[1:].view(batch, dim, L)
    else:
        x = torch.randn(batch, dim, L, generator=g).to(dtype).to(DEV)
    w = torch.randn(dim, width, generator=g).to(DEV)
    b = torch.randn(dim, generator=g).to(DEV) if bias else None
    sq, en, st = seq.to(DEV), ends.to(DEV), starts.to(DEV)
    pool, base = make_pool(kind, num_slots, dim, width, dtype)
    ikind = POOLS[(POOLS.index(kind) + 1) % 3]
    init, init_base = make_pool(ikind, n_init, dim, width, dtype)
    init.copy_(torch.randn(n_init, dim, width, generator=g).to(dtype))
    init_before = init_base.clone()
    out = native.causal_conv1d_varlen_resume_fwd(x, w, b, act, sq, en, pool, st, init)
    assert torch.equal(init_base, init_before)
    named = set()
    for r in range(batch):
        # the row written out: every resumed segment with its width - 1 carried values in front, under the same id
        cols, ids, keep = [], [], []
        for rr, s, n, a, e in entries:
            if rr != r:
                continue
            if a >= 0:
                cols.append(init[a][:, 1:])
                ids += [len(keep)] * (width - 1)
            cols.append(x[r, :, s:s + n])
            keep.append((sum(c.shape[-1] for c in cols) - n, n, s))
            ids += [len(keep) - 1] * n
            if e >= 0:
                tail = torch.cat([init[a] if a >= 0 else torch.zeros(dim, width, dtype=dtype, device=DEV), x[r, :, s:s + n]], -1)[:, -width:]
                assert torch.equal(pool[e], tail), f"row {r} segment [{s}, {s + n}) from {a} into {e}"
                named.add(e)
        end = max(s + n for rr, s, n, _, _ in entries if rr == r)
        if end < L:                                                         # the padding: a segment of its own
            cols.append(x[r, :, end:])
            keep.append((sum(c.shape[-1] for c in cols) - (L - end), L - end, end))
            ids += [len(keep) - 1] * (L - end)
        wide = torch.cat(cols, -1).unsqueeze(0).contiguous()
        ref = native.causal_conv1d_varlen_fwd(wide, w, b, act, torch.tensor([ids], dtype=torch.int32, device=DEV))
        for at, n, s in keep:
            assert torch.equal(out[r, :, s:s + n], ref[0, :, at:at + n]), f"row {r} out [{s}, {s + n})"
    probe = torch.zeros_like(base, dtype=torch.bool)
    pool_view(probe, kind, width, dim)[sorted(named)] = True
    assert bool((base[~probe] == 7.0).all())                                # unnamed slots and everything around the pool: untouched
    first = base.clone()
    assert torch.equal(native.causal_conv1d_varlen_resume_fwd(x, w, b, act, sq, en, pool, st, init), out) and torch.equal(base, first)
    # no start entry anywhere: the kEmit kernels' bits, out and pool
    plain, plain_base = make_pool(kind, num_slots, dim, width, dtype)
    none, none_base = make_pool(kind, num_slots, dim, width, dtype)
    want = native.causal_conv1d_varlen_states_fwd(x, w, b, act, sq, en, plain)
    got = native.causal_conv1d_varlen_resume_fwd(x, w, b, act, sq, en, none, torch.full_like(st, -1), init)
    assert torch.equal(got, want) and torch.equal(none_base, plain_base)
    nostart = [r for r in range(batch) if not bool((starts[r] >= 0).any())]
    assert torch.equal(out[nostart], want[nostart])


@pytest.mark.parametrize("width", [2, 3, 4])
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_conv_resumes_every_segment_from_its_carried_inputs(dt, width):
    """dim 130 at batch 3 and 1 (clamped rows exist). L = 520 on the 16-byte path, L = 523 and a misaligned x on the scalar path"""
    dtype = DTYPES[dt]
    k = width + list(DTYPES).index(dt)
    run_conv(conv_rows(520), 130, width, 520, dtype, POOLS[k % 3], seed=width)
    run_conv(conv_rows(523), 130, width, 523, dtype, POOLS[(k + 1) % 3], seed=width + 10)
    run_conv(conv_rows(520)[:1], 130, width, 520, dtype, POOLS[(k + 2) % 3], seed=width + 20, misalign=True, act=False, bias=False)


def test_operators_take_the_new_arguments():
    """causal_conv1d_fn / selective_scan_fn with start_slots: a continuation that stores nothing (end_slots absent) gives the resumed
    outputs; the conv refuses initial_states that overlap the pool it stores into"""
    from dimsum_amd import native
    from dimsum_amd.ops import causal_conv1d_fn, selective_scan_fn
    g = scan_inputs(1, 64, 16, 12, torch.float32, seed=1)
    seq = torch.zeros(1, 12, dtype=torch.int32, device=DEV)
    starts = torch.full((1, 12), -1, dtype=torch.int32, device=DEV)
    starts[0, 0] = 1
    h = torch.randn(3, 64, 16, device=DEV)
    got = selective_scan_fn(g["u"], g["delta"], g["A"], g["B"], g["C"], g["D"], g["z"], g["bias"], True, seq_idx=seq, start_slots=starts, initial_states=h)
    want = selective_scan_fn(g["u"], g["delta"], g["A"], g["B"], g["C"], g["D"], g["z"], g["bias"], True, initial_state=h[1:2])
    assert torch.equal(got, want)
    w, cs = torch.randn(64, 4, device=DEV), torch.randn(3, 64, 4, device=DEV)
    out = causal_conv1d_fn(g["u"], w, None, "silu", seq_idx=seq, start_slots=starts, initial_states=cs)
    state = cs[1:2].clone()
    # the carried-state kernel computes the same five fp32 terms, possibly contracted into other fused multiply-adds: |terms| stay below
    # ~20 here, so 1e-5 is several roundings of the sum
    torch.testing.assert_close(out, native.causal_conv1d_chunk(g["u"], state, w, None, True), rtol=0, atol=1e-5)
    ends = torch.full((1, 12), -1, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="initial_states overlaps conv_state"):
        causal_conv1d_fn(g["u"], w, None, "silu", seq_idx=seq, end_slots=ends, conv_state=cs, start_slots=starts, initial_states=cs[1:])


# ---- the model -----------------------------------------------------------------------------------------------------------------------------------------
def lm_f64(m, prompt):
    """the LM on one prompt alone, in float64 on the CPU in plain torch (the restatements for the conv and the scan) ->
    (last-token logits (V,), [(conv_state (D, d_conv), ssm_state (D, N)) per layer]): pre-norm blocks with RMSNorm, the tied head"""
    from dimsum_amd.ops import causal_conv1d_varlen_torch, selective_scan_varlen_torch
    d = lambda t: t.detach().double().cpu()
    rms = lambda x, n: x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + n.eps) * d(n.weight)
    b = m.backbone
    assert all(blk.norm.bias is None and blk.mixer.in_proj.bias is None and blk.mixer.out_proj.bias is None for blk in b.layers)
    hidden, residual, states = d(b.embedding.weight)[prompt.cpu()].unsqueeze(0), None, []
    for blk in b.layers:
        residual = hidden if residual is None else hidden + residual
        mx = blk.mixer
        D, R, N = mx.d_inner, mx.dt_rank, mx.d_state
        xz = (rms(residual, blk.norm) @ d(mx.in_proj.weight).t()).transpose(1, 2)                 # (1, 2 D, L)
        conv_out = causal_conv1d_varlen_torch(xz[:, :D], d(mx.conv1d.weight).reshape(D, -1), d(mx.conv1d.bias), "silu")
        x_dbl = conv_out.transpose(1, 2) @ d(mx.x_proj.weight).t()
        delta = (x_dbl[..., :R] @ d(mx.dt_proj.weight).t()).transpose(1, 2)
        y, last = selective_scan_varlen_torch(conv_out, delta, -torch.exp(d(mx.A_log)), x_dbl[..., R:R + N].transpose(1, 2),
                                              x_dbl[..., R + N:].transpose(1, 2), d(mx.D), xz[:, D:], d(mx.dt_proj.bias), True, True)
        states.append((torch.nn.functional.pad(xz[0, :D], (mx.d_conv, 0))[:, -mx.d_conv:], last[0]))
        hidden = y.transpose(1, 2) @ d(mx.out_proj.weight).t()
    return (rms(hidden + residual, b.norm_f) @ d(m.lm_head.weight).t())[0, -1], states


def test_lm_prompt_in_three_resumed_passes_is_the_prompt_in_one(exact_fp32):  # noqa: F811
    """MambaLMHeadModel.forward: a 21-token prompt fed 8 + 8 + 5 over three packed passes through slot 2 of a pool -- InferenceParams.
    prefill_starts on the second and third -- each next to another request's segment (before it, after it, before it), against the same
    prompt prefilled in ONE packed pass next to a neighbour. The GEMMs see other row counts, so equality is not expected; the bound is
    test_packed_prefill_gpu.py's packed-row bound: |split - float64| <= 2 |one pass - float64| + one ulp of fp32 at the largest reference
    value, for the last-token logits and for every layer's conv and SSM state of the slot (the float64 side: lm_f64)."""
    from test_lm_cpu import tiny_model
    from test_packed_prefill_gpu import ulp
    from test_slots_gpu import SEED
    from dimsum_amd.utils import InferenceParams, plan_packed_prefill
    torch.manual_seed(SEED)
    m = tiny_model(1, 1, vocab_size=VOCAB).to(DEV)
    g = torch.Generator().manual_seed(21)
    prompt = torch.randint(0, VOCAB, (21,), generator=g).to(DEV)
    others = [torch.randint(0, VOCAB, (n,), generator=g).to(DEV) for n in (5, 3, 6, 4)]

    def one_pass(pool, segs, rows=1):
        """segs: [(tokens, slot, resumed)] -> the logits row of every segment"""
        plan = plan_packed_prefill([t.numel() for t, _, _ in segs], [s for _, s, _ in segs], rows=rows, resume=[f for _, _, f in segs])
        ids = torch.zeros(rows, plan["seqlen"], dtype=torch.long, device=DEV)
        for (t, _, _), (r, at) in zip(segs, plan["segments"]):
            ids[r, at:at + t.numel()] = t
        starts = {k: plan[k].to(DEV) for k in ("start_slots", "start_rows", "start_list")} if plan["start_list"].numel() else None
        p = InferenceParams(64, rows, key_value_memory_dict=pool, prefill_slots=plan["end_slots"].to(DEV), prefill_starts=starts)
        return m(ids, inference_params=p, seq_idx=plan["seq_idx"].to(DEV), logits_positions=plan["logits_positions"].to(DEV)).logits

    def fresh():
        pool = m.allocate_inference_cache(6, 64)
        for conv, ssm in pool.values():
            conv.fill_(7.0)
            ssm.fill_(7.0)
        return pool

    with torch.no_grad():
        whole, split = fresh(), fresh()
        want = one_pass(whole, [(others[0], 0, False), (prompt, 2, False)])[1]
        one_pass(split, [(others[0], 0, False), (prompt[:8], 2, False)])
        # the resumed slot is ordinal 0 here and ordinal 1 in the third pass, where the neighbour in front of it resumes slot 0 with one token more
        one_pass(split, [(prompt[8:16], 2, True), (others[1], 1, False)])
        got = one_pass(split, [(others[2][:1], 0, True), (prompt[16:], 2, True), (others[3], 3, False)])[1]
        ref_logits, ref_states = lm_f64(m, prompt)
    err = lambda t, ref: float((t.double().cpu() - ref).abs().max())
    checks = [("logits", got, want, ref_logits)]
    for k, (conv64, ssm64) in enumerate(ref_states):
        checks += [(f"layer {k} conv_state", split[k][0][2], whole[k][0][2], conv64), (f"layer {k} ssm_state", split[k][1][2], whole[k][1][2], ssm64)]
    for name, a, b, ref in checks:
        e_split, e_one, bound = err(a, ref), err(b, ref), 2 * err(b, ref) + ulp(float(ref.abs().max()))
        print(f"{name}: bit-identical {torch.equal(a, b)}; split err {e_split:.3e}, one-pass err {e_one:.3e}, bound {bound:.3e}")
        assert torch.equal(a, b) or e_split <= bound, name
    for k in split:
        # slot 0 went on by one token in the third pass: it no longer holds what the first pass left (the other request's resume was served)
        assert not torch.equal(split[k][1][0], whole[k][1][0])
        assert bool((split[k][0][[4, 5]] == 7.0).all()) and bool((split[k][1][[4, 5]] == 7.0).all())      # the slots nobody named
        assert not bool((split[k][1][[1, 3]] == 7.0).any())


# ---- the engine ----------------------------------------------------------------------------------------------------------------------------------------
CHUNKED = [(3, 6), (8, 4), (9, 5), (21, 3), (40, 6), (5, 4)]                # (prompt tokens, new tokens)


@pytest.mark.parametrize("prefill_rows", [1, 2])
def test_engine_with_chunked_prefill_reproduces_every_request_alone(prefill_rows, exact_fp32, monkeypatch):  # noqa: F811
    """six requests with prompts of 3, 8, 9, 21, 40 and 5 tokens on DecodeEngine(max_batch=4, num_slots=5, cg=True, packed_prefill=True,
    max_prefill_tokens=8, chunked_prefill=True): every sequence equals generate() of that request alone, by the rule of test_slots_gpu.py
    where routes differ: max |logit - alone logit| < min_gap / 4 with min_gap the smallest top-1 / top-2 gap of the ALONE runs."""
    from test_slots_gpu import SEED
    from test_lm_cpu import tiny_model
    from dimsum_amd.utils.serving import DecodeEngine
    monkeypatch.setenv("DIMSUM_FUSED_DECODE", "1")
    torch.manual_seed(SEED)
    m = tiny_model(1, 1, vocab_size=VOCAB).to(DEV)
    gp = torch.Generator().manual_seed(300 + SEED)
    prompts = [torch.randint(0, VOCAB, (n,), generator=gp).to(DEV) for n, _ in CHUNKED]
    want = [alone(m, p, n) for p, (_, n) in zip(prompts, CHUNKED)]
    top = torch.cat([s for _, s in want]).topk(2, dim=-1).values
    min_gap = float((top[:, 0] - top[:, 1]).min())
    assert min_gap >= 1e-3, min_gap                                         # a tie cannot hide a failure
    eng = DecodeEngine(m, max_batch=4, num_slots=5, max_seqlen=64, vocab_size=VOCAB, cg=True, output_scores=True, packed_prefill=True,
                       prefill_rows=prefill_rows, max_prefill_tokens=8, chunked_prefill=True)
    for conv, ssm in eng.pool.values():
        conv.fill_(7.0)
        ssm.fill_(7.0)
    eng.free_slots.remove(4)                                                # withheld: a slot of the pool that no request is ever given
    g = torch.Generator().manual_seed(9)
    rids = [eng.submit(p, n, uniforms=torch.rand(n, generator=g)) for p, (_, n) in zip(prompts, CHUNKED)]
    with torch.no_grad():
        eng._admit()                                                        # the first admission: 3 tokens + the first 5 of the 8-token prompt
    assert eng.prefill_pass_tokens == [8] and [s for _, s in eng.slot_history] == [0, 1] and [r.rid for r in eng._prefilling] == [1]
    for conv, ssm in eng.pool.values():
        assert bool((conv[2:] == 7.0).all()) and bool((ssm[2:] == 7.0).all())       # the slots nobody named: untouched
        assert not bool((ssm[:2] == 7.0).any())
    steps = 0
    while not eng.idle():
        for rid, _, _ in eng.step():
            assert eng.requests[rid].done == eng.requests[rid].prompt.numel()
        steps += 1
        assert steps < 200
    assert eng.n_captures == 1
    assert max(eng.prefill_pass_tokens) <= 8 and sum(eng.prefill_pass_tokens) == sum(n for n, _ in CHUNKED)
    assert eng.n_prefill_passes == len(eng.prefill_pass_tokens) and eng.n_prefill_pieces > len(CHUNKED)
    seen, reused = set(), False
    for _, slot in eng.slot_history:
        reused |= slot in seen
        seen.add(slot)
    assert reused and len(eng.slot_history) == len(CHUNKED), eng.slot_history
    err = max(float((torch.stack(eng.scores(rid)) - scores).abs().max()) for rid, (_, scores) in zip(rids, want))
    print(f"chunked prefill, prefill_rows={prefill_rows}: max |logit - alone logit| {err:.3e}, alone min_gap {min_gap:.3e}, passes {eng.prefill_pass_tokens}")
    assert err < min_gap / 4
    for rid, (seq, _) in zip(rids, want):
        assert torch.equal(eng.sequence(rid), seq), rid
    assert sorted(eng.free_slots) == list(range(4)) and eng.slots.tolist() == [-1] * 4 and 4 not in {s for _, s in eng.slot_history}
    for conv, ssm in eng.pool.values():                                     # after every resumed pass and decode step: the withheld slot's bits
        assert bool((conv[4] == 7.0).all()) and bool((ssm[4] == 7.0).all())
        assert not bool((ssm[:4] == 7.0).any())                             # ... and every other slot was used
