"""The routing passes of csrc/moe.hip on the paths that only real sizes reach -- input builders, float64 oracles and the preconditions of
tests/test_moe_paths_gpu.py, all on the CPU:

  A. the counting sort's scan with more than 64 blocks of 64 tokens (moe_scan_kernel: seg = ceil(nblk / 64) blocks per lane, seg >= 2 from 4097
     tokens on), steered by construction: x[t] = onehot(f(t)), router weight 8 I, so the float64 logits are exactly 8 and 0;
  B. the router forward at hidden > 2048 (a lane keeps 8 x 16 bytes of a row in registers, columns from 2048 on go through a tail loop);
  C. moe_route_bwd against float64 autograd on inputs no forward kernel made: more than one group of 8 experts, more than one strip of 1024
     columns, rows_per_wg = roundup(ceil(T / 512), 64) in {64, 128};
  D. SwitchMLP with 9 and 16 experts.

Every claim about which leaf a case reaches restates the host's arithmetic here and is asserted, so a changed constant in the kernel file shows up
as a failed claim, not as a silently idle case."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from procedural import seeded
from test_moe_cpu import make_switch, moe_route_bwd
from test_moe_gpu import MIN_GAP, ROW_TOL, route_inputs, route_oracle

T = torch.from_numpy
MODES = ("softmax", "sigmoid")
K_BLK, K_XR_COLS, K_EG, K_STRIP, K_ROWS, K_ROW_GROUPS = 64, 2048, 8, 1024, 64, 512       # csrc/moe.hip: kBlk, kXr * 256, kEG, 256 * 4, kRows, 512


def cdiv(a, b):
    return -(-a // b)


def tolerance(want, rtol, atol=0.0, scale_atol=0.0):
    """conftest.assert_close's elementwise bound as a tensor"""
    want = want.double()
    return atol + scale_atol * (want.abs().max().item() if want.numel() else 0.0) + rtol * want.abs()


def worst_ratio(got, want, rtol, atol=0.0, scale_atol=0.0):
    """max |got - want| / tolerance: <= 1 is what conftest.assert_close(got, want, rtol, atol, scale_atol=...) accepts"""
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    if want.numel() == 0:
        return 0.0
    return ((got - want).abs() / tolerance(want, rtol, atol, scale_atol).clamp_min(1e-300)).max().item()


def route_of(logits, mode):
    return torch.sigmoid(logits) if mode == "sigmoid" else torch.softmax(logits, dim=1)


# ---- A. the sort at more than 64 blocks ---------------------------------------------------------------------------------------------------------
SORT_E = 64
# tokens -> (nblk, seg, lanes that hold a block, blocks of the last such lane)
SORT_TOKENS = {4096: (64, 1, 64, 1), 4097: (65, 2, 33, 1), 8193: (129, 3, 43, 3), 65537: (1025, 17, 61, 5)}
SORT_PATTERNS = ("mod", "block", "block_reversed", "all_63_but_token_0", "all_0_but_the_last", "random_9_of_64")


def sort_pattern(tokens, pattern):
    """f (tokens) int64: the expert every token is steered to"""
    t = torch.arange(tokens)
    if pattern == "mod":
        return t % 64
    if pattern == "block":                                  # every block of 64 tokens holds a single expert
        return (t // 64) % 64
    if pattern == "block_reversed":
        return 63 - (t // 64) % 64
    if pattern == "all_63_but_token_0":
        f = torch.full((tokens,), 63)
        f[0] = 0
        return f
    if pattern == "all_0_but_the_last":
        f = torch.zeros(tokens, dtype=torch.long)
        f[-1] = 63
        return f
    assert pattern == "random_9_of_64"
    rs = np.random.RandomState(tokens)
    used = np.sort(rs.choice(SORT_E, 9, replace=False))
    return T(used[rs.randint(0, 9, tokens)]).long()


@functools.lru_cache(maxsize=None)
def sort_inputs(tokens, pattern):
    """x (tokens, 64) = onehot(f), router weight 8 I, f"""
    f = sort_pattern(tokens, pattern)
    return F.one_hot(f, SORT_E).float(), 8.0 * torch.eye(SORT_E), f


def sort_geometry(tokens):
    """moe_scan_kernel's split of the nblk count rows over the 64 lanes: (nblk, seg, lanes with b0 < nblk, blocks of the last of them)"""
    nblk = cdiv(tokens, K_BLK)
    seg = cdiv(nblk, 64)
    lanes = cdiv(nblk, seg)
    return nblk, seg, lanes, nblk - (lanes - 1) * seg


def test_the_sort_cases_split_the_blocks_as_claimed():
    for tokens, want in SORT_TOKENS.items():
        assert sort_geometry(tokens) == want, tokens
    assert sort_geometry(1000)[:2] == (16, 1)              # the largest token count of test_moe_gpu: one block per lane at most
    segs = [g[1] for g in SORT_TOKENS.values()]
    assert segs[0] == 1 and min(segs[1:]) >= 2 and SORT_TOKENS[4096][2] == 64          # seg = 1 with the last lane in use, then seg > 1
    assert any(last < seg for _, seg, _, last in SORT_TOKENS.values())                  # a lane whose run the min(.., nblk) clamp cuts short
    assert any(lanes < 64 and seg > 1 for _, seg, lanes, _ in SORT_TOKENS.values())     # lanes with b0 == b1 == nblk


@pytest.mark.parametrize("pattern", SORT_PATTERNS)
@pytest.mark.parametrize("tokens", list(SORT_TOKENS))
def test_the_steered_logits_are_exact_and_choose_f(tokens, pattern):
    x, w, f = sort_inputs(tokens, pattern)
    assert x.shape == (tokens, SORT_E) and f.min() >= 0 and f.max() < SORT_E
    for mode in MODES:
        _, e, logits, gap = route_oracle(x, w, None, mode)
        assert torch.equal(logits, 8.0 * x.double()) and torch.equal(e, f) and gap >= MIN_GAP, (mode, gap)
    assert torch.equal((x.double() @ w.double().t()).float().double(), 8.0 * x.double())           # (8 and 0 are fp32 values: no rounding anywhere)
    counts = torch.bincount(f, minlength=SORT_E)
    if pattern == "random_9_of_64":
        used = counts.nonzero().squeeze(1)
        assert used.numel() == 9 and (counts[used[0]:used[-1]] == 0).any()                          # empty experts between used ones
    if pattern in ("block", "block_reversed"):
        assert all(f[i:i + 64].unique().numel() == 1 for i in range(0, tokens, 64))
    if pattern.startswith("all_"):
        assert sorted(counts[counts > 0].tolist()) == [1, tokens - 1]


# (tokens, hidden, experts, mode, seed): seeded inputs through the real arithmetic; 1 % more candidate tokens are drawn, those whose float64
# best / second-best gap is below MIN_GAP are dropped and the first `tokens` of the rest are the case
SORT_SEEDED = [(8193, 8, 9, "softmax", 7100), (8193, 64, 3, "sigmoid", 7200)]


def token_gaps(x, w, b, mode):
    logits = x.double() @ w.double().t() + (0 if b is None else b.double())
    top = route_of(logits, mode).topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


@functools.lru_cache(maxsize=None)
def filtered_route_inputs(tokens, hidden, experts, mode, seed):
    """-> x (tokens, hidden), w, b, the number of candidates kept (of tokens + ceil(tokens / 100))"""
    x, w, b = route_inputs(tokens + cdiv(tokens, 100), hidden, experts, seed)
    keep = token_gaps(x, w, b, mode) >= MIN_GAP
    return x[keep][:tokens].contiguous(), w, b, int(keep.sum())


@pytest.mark.parametrize("tokens,hidden,experts,mode,seed", SORT_SEEDED)
def test_enough_candidates_pass_the_gap_filter(tokens, hidden, experts, mode, seed):
    x, w, b, kept = filtered_route_inputs(tokens, hidden, experts, mode, seed)
    print(f"{tokens} x {hidden}, {experts} experts, {mode}: {tokens + cdiv(tokens, 100) - kept} of {tokens + cdiv(tokens, 100)} candidates dropped")
    assert kept >= tokens and x.shape == (tokens, hidden)
    _, e, _, gap = route_oracle(x, w, b, mode)
    assert gap >= MIN_GAP and sort_geometry(tokens)[1] == 3
    assert (torch.bincount(e, minlength=experts) > 0).all()


# ---- B. the router forward at hidden > 2048 -----------------------------------------------------------------------------------------------------
# (tokens, hidden, experts, mode, seed, with a router bias); the seeds were picked on the CPU for the two preconditions below
WIDE_AXES = ([1, 65], [2048, 2052, 2304, 4100], [2, 9, 64])
WIDE_CASES = [
    (1, 2048, 2, "softmax", 8000, True), (65, 2052, 9, "softmax", 8010, True), (1, 2304, 64, "softmax", 8020, True), (65, 4100, 2, "softmax", 8030, True),
    (65, 2048, 64, "sigmoid", 8040, True), (1, 2052, 2, "sigmoid", 8050, True), (65, 2304, 9, "sigmoid", 8060, True), (1, 4100, 9, "sigmoid", 8070, True),
    (65, 4100, 9, "softmax", 8080, False), (65, 2052, 64, "sigmoid", 8090, False),
]


@functools.lru_cache(maxsize=None)
def wide_inputs(tokens, hidden, experts, seed, biased):
    x, w, b = route_inputs(tokens, hidden, experts, seed)
    return x, w, (b if biased else None)


def test_the_wide_cases_show_every_value_with_each_mode():
    for mode in MODES:
        mine = [c for c in WIDE_CASES if c[3] == mode]
        for axis, values in enumerate(WIDE_AXES):
            assert {c[axis] for c in mine} == set(values), (mode, axis)
        assert sum(not c[5] for c in mine) == 1 and sum(c[5] for c in mine) >= 4
    assert all(not c[5] and c[1] > K_XR_COLS for c in WIDE_CASES if not c[5])           # the calls without a bias run the tail loop too
    # the tail loop's shapes: none, one 16-byte piece for 1 lane, one piece for every lane, 8 rounds and a piece
    assert sorted({(h - K_XR_COLS) / 256 for h in WIDE_AXES[1]}) == [0.0, 4 / 256, 1.0, 8 + 4 / 256]


@pytest.mark.parametrize("tokens,hidden,experts,mode,seed,biased", WIDE_CASES)
def test_the_wide_cases_meet_their_preconditions(tokens, hidden, experts, mode, seed, biased):
    x, w, b = wide_inputs(tokens, hidden, experts, seed, biased)
    _, _, logits, gap = route_oracle(x, w, b, mode)
    assert gap >= MIN_GAP, f"smallest best / second-best gap {gap:.3e}"
    if hidden > K_XR_COLS:              # a kernel that dropped the columns from 2048 on misses ROW_TOL on every token's logits
        cut = route_oracle(x[:, :K_XR_COLS], w[:, :K_XR_COLS], b, mode)[2]
        off = (cut - logits).abs() > tolerance(logits, *ROW_TOL)
        assert off.any(dim=1).all(), f"{int((~off.any(dim=1)).sum())} tokens whose logits do not need the tail"


# ---- C. moe_route_bwd ---------------------------------------------------------------------------------------------------------------------------
BWD_SHAPES = [(1, 4, 1), (63, 260, 3), (65, 1024, 8), (257, 1028, 9), (257, 2052, 17), (65, 64, 64), (1000, 1152, 16), (32768, 8, 9), (32833, 8, 9)]
BWD_CASES = [s + (mode,) for s in BWD_SHAPES for mode in MODES] + [(32833, 4, 64, "softmax")]


def bwd_oracle(c, drop=None):
    """float64 autograd through route -> p = route[t, expert[t]] -> sum(p dprob), then the three products. drop: a slice of experts whose dl is zeroed"""
    leaf = c["logits"].double().requires_grad_()
    p = route_of(leaf, c["mode"])[torch.arange(leaf.shape[0]), c["expert"].long()]
    (p * c["dprob"].double()).sum().backward()
    dl = leaf.grad
    if drop is not None:
        dl = dl.clone()
        dl[:, drop] = 0
    x, w = c["x"].double(), c["w"].double()
    return c["dxp"].double()[c["inv"].long()] + dl @ w, dl.t() @ x, dl.sum(0)


@functools.lru_cache(maxsize=None)
def bwd_case(tokens, hidden, experts, mode):
    """inputs of native.moe_route_bwd that no forward kernel made, and the oracle's dx, dw, db. logits: the fp32 rounding of the float64 logits;
    expert, prob: the float64 route's; inv: a seeded permutation, not the sort's table"""
    seed = 9000 + 40 * BWD_CASES.index((tokens, hidden, experts, mode))
    x, w, b = route_inputs(tokens, hidden, experts, seed)
    prob, e, logits, _ = route_oracle(x, w, b, mode)
    c = dict(mode=mode, x=x, w=w, logits=logits.float(), prob=prob.float(), expert=e.int(),
             inv=T(np.random.RandomState(seed + 3).permutation(tokens).astype(np.int32)),
             dprob=T(seeded((tokens,), seed + 4)), dxp=T(seeded((tokens, hidden), seed + 5)))
    c["dx"], c["dw"], c["db"] = bwd_oracle(c)
    return c


def bwd_geometry(tokens, hidden, experts):
    """dimsum_moe_route_bwd's launch, restated"""
    groups, strips = cdiv(experts, K_EG), cdiv(hidden, K_STRIP)
    rpw = cdiv(cdiv(tokens, K_ROW_GROUPS), K_ROWS) * K_ROWS
    row_groups = cdiv(tokens, rpw)
    last_rows = tokens - (row_groups - 1) * rpw
    return dict(groups=groups, last_group=experts - (groups - 1) * K_EG, strips=strips, last_strip_threads=(hidden - (strips - 1) * K_STRIP) // 4,
                rpw=rpw, row_groups=row_groups, last_rows=last_rows)


def test_the_backward_cases_reach_every_leaf():
    geo = {s: bwd_geometry(*s) for s in {c[:3] for c in BWD_CASES}}
    assert {g["groups"] for g in geo.values()} >= {1, 2, 3, 8}
    assert any(g["groups"] > 1 and g["last_group"] < K_EG for g in geo.values())                # a partial last group after a full one
    assert any(g["groups"] > 1 and g["last_group"] == K_EG for g in geo.values())
    assert {g["strips"] for g in geo.values()} == {1, 2, 3}
    assert any(g["strips"] > 1 and g["last_strip_threads"] < 256 for g in geo.values())         # inactive threads in the last of several strips
    assert any(g["strips"] == 1 and g["last_strip_threads"] == 256 for g in geo.values())
    assert {g["rpw"] for g in geo.values()} == {64, 128}
    assert any(g["rpw"] == 128 and g["last_rows"] > K_ROWS and g["last_rows"] % K_ROWS for g in geo.values())     # two tiles, the second short
    assert any(g["rpw"] == 64 and g["last_rows"] % K_ROWS for g in geo.values())
    g = geo[(32768, 8, 9)]
    assert (g["rpw"], g["row_groups"], g["last_rows"]) == (64, 512, 64)
    g = geo[(32833, 8, 9)]
    assert (g["rpw"], g["row_groups"], g["last_rows"]) == (128, 257, 65)
    for s in BWD_SHAPES:
        assert {c[3] for c in BWD_CASES if c[:3] == s} == set(MODES), s
    assert any(c[3] == "sigmoid" and c[2] > 4 for c in BWD_CASES)
    # what test_moe_gpu's module tests reach: one group, one strip, one tile per workgroup
    assert all(bwd_geometry(t, h, 4) == dict(bwd_geometry(t, h, 4), groups=1, strips=1, rpw=64) for t in (48, 513) for h in (32, 128))


@pytest.mark.parametrize("tokens,hidden,experts,mode", BWD_CASES)
def test_the_backward_oracle_agrees_with_the_standin_in_float64(tokens, hidden, experts, mode):
    c = bwd_case(tokens, hidden, experts, mode)
    assert c["logits"].dtype == torch.float32 and c["expert"].dtype == torch.int32 and c["inv"].dtype == torch.int32
    assert torch.equal(torch.sort(c["inv"].long()).values, torch.arange(tokens))
    logits = c["logits"].double()
    prob = route_of(logits, mode)[torch.arange(tokens), c["expert"].long()]                   # the route value of the logits the oracle differentiates
    assert (prob - c["prob"].double()).abs().max() <= 2.0 ** -22                               # (and the fp32 prob handed to the kernel is that value)
    got = moe_route_bwd(c["x"].double(), c["w"].double(), logits, prob, c["expert"], c["inv"], c["dprob"].double(), c["dxp"].double(), mode)
    for name, a in zip(("dx", "dw", "db"), got):
        assert (a - c[name]).abs().max() <= 1e-12 * max(c[name].abs().max().item(), 1e-300), name


@pytest.mark.parametrize("tokens,hidden,experts,mode", BWD_CASES)
def test_the_backward_cases_would_catch_a_skipped_group_or_strip(tokens, hidden, experts, mode):
    from test_blocks_linear_window_gpu import SUM_TOL
    c = bwd_case(tokens, hidden, experts, mode)
    if experts > K_EG:
        dx1, dw1, db1 = bwd_oracle(c, drop=slice(K_EG, None))         # a kernel that stopped after the first group of experts
        assert worst_ratio(dx1, c["dx"], *ROW_TOL) > 1
        assert torch.count_nonzero(c["dw"][K_EG:]) > 0 and torch.count_nonzero(c["db"][K_EG:]) > 0
        for g0 in range(K_EG, experts, K_EG):                         # ... or that skipped any one of the later groups
            dx1, dw1, db1 = bwd_oracle(c, drop=slice(g0, g0 + K_EG))
            assert worst_ratio(dx1, c["dx"], *ROW_TOL) > 1, g0
            assert worst_ratio(dw1, c["dw"], **SUM_TOL) > 1 and worst_ratio(db1, c["db"], **SUM_TOL) > 1, g0
    for c0 in range(K_STRIP, hidden, K_STRIP):                        # a kernel that skipped a strip of columns after the first
        assert torch.count_nonzero(c["dw"][:, c0:c0 + K_STRIP]) > 0
        lost = c["dw"].clone()
        lost[:, c0:c0 + K_STRIP] = 0
        assert worst_ratio(lost, c["dw"], **SUM_TOL) > 1, c0
    assert worst_ratio(c["dxp"].double()[c["inv"].long()], c["dx"], *ROW_TOL) > 1 or experts == 1 and mode == "softmax"      # dl @ w shows in dx
    assert tokens == 1 or worst_ratio(c["dx"] - c["dxp"].double()[c["inv"].long()] + c["dxp"].double(), c["dx"], *ROW_TOL) > 1      # and so does the gather


# ---- D. the layer with more than 8 experts ------------------------------------------------------------------------------------------------------
LAYER_DIM, LAYER_SHAPE = 64, (3, 171)
LAYER_CASES = [(experts, mode, gated, bias) for experts in (9, 16) for mode in ("top1", "sinkhorn") for gated, bias in ((True, True), (False, False))]
# case -> (procedural_fill seed of the module, seed of x): picked on the CPU for the gap precondition
LAYER_SEEDS = {
    (9, "top1", True, True): (60, 700), (9, "top1", False, False): (61, 710), (9, "sinkhorn", True, True): (62, 720), (9, "sinkhorn", False, False): (63, 730),
    (16, "top1", True, True): (64, 742), (16, "top1", False, False): (65, 752), (16, "sinkhorn", True, True): (66, 762), (16, "sinkhorn", False, False): (67, 770),
}


def layer_case(experts, mode, gated, bias):
    """-> a fresh SwitchMLP(64, E experts) on the CPU, x (3, 171, 64), dout"""
    fill, xseed = LAYER_SEEDS[(experts, mode, gated, bias)]
    return (make_switch(mode, gated, bias, fill, dim=LAYER_DIM, experts=experts), T(seeded(LAYER_SHAPE + (LAYER_DIM,), xseed)),
            T(seeded(LAYER_SHAPE + (LAYER_DIM,), 502)))


@pytest.mark.parametrize("experts,mode,gated,bias", LAYER_CASES)
def test_the_layer_cases_meet_the_gap_precondition(experts, mode, gated, bias):
    m, x, _ = layer_case(experts, mode, gated, bias)
    assert len(m.local_experts) == experts and cdiv(experts, K_EG) == 2
    _, e, _, gap = route_oracle(x.reshape(-1, LAYER_DIM), m.router.weight.detach(), m.router.bias.detach(), "sigmoid" if mode == "sinkhorn" else "softmax")
    assert gap >= MIN_GAP, f"smallest best / second-best gap {gap:.3e}"
    assert (torch.bincount(e, minlength=experts) > 0).all()          # every expert works, those of the router backward's second group included
