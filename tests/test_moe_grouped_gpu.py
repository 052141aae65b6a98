"""The grouped expert GEMM (csrc/moe_gemm.hip) on the GPU: the kernel against float64 on hand-made offset tables around its tile edges, the grouped
SwitchMLP forward against the reference's fixtures and against the ungrouped forward of the same module, and an is_moe model replayed from a
captured hipGraph on batches whose expert counts differ from the captured batch's.

The kernel's bound (every comparison below uses it, none uses a measured tolerance): an fp32 value v is staged as hi = bf16(v), lo = bf16(v - hi);
round-to-nearest leaves |v - hi - lo| <= 2^-18 |v|. Of (a_hi + a_lo)(b_hi + b_lo) the kernel drops a_lo b_lo, and the two residuals a - a_hi - a_lo,
b - b_hi - b_lo never enter: each of the three is at most 2^-18 |a b|; a factor 4 instead of 3 covers the second-order terms. The rest is fp32
accumulation of K (+ 3) terms. With S = sum_k |a_k| |b_k| in float64:   |got - exact| <= (4 * 2^-18 + (K + 3) * 2^-24) S + 2^-24 |bias|."""
import numpy as np
import pytest
import torch

from conftest import assert_close, golden
from procedural import procedural_fill, seeded
from test_blocks_linear_window_gpu import Y_TOL
from test_moe_cpu import CASES, FILES, make_switch, tag_of, _tiny

pytestmark = pytest.mark.gpu
T = torch.from_numpy
U = 2.0 ** -24
SENTINEL = -12345.678


@pytest.fixture(autouse=True)
def _fp32_matmul():
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.set_float32_matmul_precision("highest")


def eps_grouped(K):
    return 4 * 2.0 ** -18 + (K + 3) * U


def _tiles():
    from dimsum_amd import native
    return native.MOE_GEMM_BM, native.MOE_GEMM_BN


def kernel_cases():
    """(name, expert row counts, K, N, bias): counts from {0, 1, BM - 1, BM, BM + 1, 2 BM + 3}, K from {32, 64, 160}, N from {32, BN, BN + 32}"""
    BM, BN = _tiles()
    big = 2 * BM + 3
    many = [0] * 64
    many[5], many[17], many[40], many[63] = BM + 1, 1, BM, big
    return [
        ("one_expert", [big], 32, 32, True),
        ("first_empty", [0, BM + 1, BM - 1], 64, BN, False),
        ("last_empty", [BM, 1, 0], 160, BN + 32, True),
        ("all_in_one_of_8", [0, 0, 0, big, 0, 0, 0, 0], 32, BN + 32, False),
        ("every_count", [1, 0, BM - 1, BM, BM + 1, big, 0, 1], 160, BN, True),
        ("every_count_narrow", [BM + 1, big, 1, 0, BM, BM - 1, 1, 0], 64, 32, False),
        ("64_experts_mostly_empty", many, 64, BN + 32, True),
        ("64_experts_one_row_each", [1] * 64, 32, BN, False),
    ]


def test_the_kernel_cases_cover_what_they_claim():
    BM, BN = _tiles()
    cases = kernel_cases()
    assert {c for _, cs, *_ in cases for c in cs} == {0, 1, BM - 1, BM, BM + 1, 2 * BM + 3}
    assert {len(cs) for _, cs, *_ in cases} == {1, 3, 8, 64}
    assert {k for *_, k, _, _ in cases} == {32, 64, 160} and {n for *_, n, _ in cases} == {32, BN, BN + 32}
    assert {b for *_, b in cases} == {True, False}
    assert any(cs[0] == 0 for _, cs, *_ in cases) and any(cs[-1] == 0 and len(cs) > 1 for _, cs, *_ in cases)
    assert any(len(cs) > 1 and sorted(cs)[-2] == 0 for _, cs, *_ in cases)           # every token in one expert of several


@pytest.mark.parametrize("case", range(8))
def test_kernel_against_float64(case):
    from dimsum_amd import native
    name, counts, K, N, biased = kernel_cases()[case]
    E, rows = len(counts), sum(counts)
    x = T(seeded((rows, K), 700 + case))
    w = T(seeded((E, N, K), 720 + case, scale=K ** -0.5))
    b = T(seeded((E, N), 740 + case)) if biased else None
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    e = torch.from_numpy(np.repeat(np.arange(E), counts)).long()
    exact = torch.einsum("tk,tnk->tn", x.double(), w.double()[e])
    S = torch.einsum("tk,tnk->tn", x.double().abs(), w.double().abs()[e])
    bound = eps_grouped(K) * S
    if biased:
        exact = exact + b.double()[e]
        bound = bound + U * b.double().abs()[e]
    guard, ldc = 3, N + 12
    buf = torch.full((guard + rows + guard, ldc), SENTINEL, device="cuda")
    out = buf[guard:guard + rows, :N]
    ws = [w[i].cuda().contiguous() for i in range(E)]
    args = (x.cuda(), T(off).cuda(), ws, None if b is None else b.cuda())
    got = native.moe_gemm(*args, out=out)
    assert got.data_ptr() == out.data_ptr()
    err = (got.double().cpu() - exact).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{name}: max |err| / bound = {worst:.3f}, max |err| = {err.max().item():.3e}")
    assert (err <= bound).all(), f"{name}: max |err| / bound = {worst:.3f}"                 # (a row left unwritten holds the sentinel: far outside)
    image = buf.cpu()
    keep = torch.full_like(image, SENTINEL)
    keep[guard:guard + rows, :N] = image[guard:guard + rows, :N]
    assert torch.equal(image.view(torch.int32), keep.view(torch.int32)), f"{name}: a guard row or guard column was written"
    again = native.moe_gemm(*args)
    assert again.is_contiguous() and torch.equal(again.view(torch.int32), got.contiguous().view(torch.int32)), f"{name}: two calls differ"


def test_rows_outside_every_range_are_not_written_and_an_empty_call_runs():
    from dimsum_amd import native
    BM, _ = _tiles()
    x = torch.randn(BM + 9, 32, device="cuda")
    ws = [torch.randn(32, 32, device="cuda") for _ in range(3)]
    out = torch.full((BM + 9, 32), SENTINEL, device="cuda")
    native.moe_gemm(x, torch.tensor([2, 2, BM + 4, BM + 4], dtype=torch.int32, device="cuda"), ws, out=out)       # rows [2, BM + 4) of expert 1 only
    assert (out[:2] == SENTINEL).all() and (out[BM + 4:] == SENTINEL).all() and (out[2:BM + 4] != SENTINEL).all()
    zero = torch.zeros(4, dtype=torch.int32, device="cuda")
    native.moe_gemm(x, zero, ws, out=out.fill_(SENTINEL))                                     # every expert empty: nothing is written
    assert (out == SENTINEL).all()
    assert native.moe_gemm(x[:0], zero, ws).shape == (0, 32)


def test_a_table_that_is_not_monotonic_writes_no_row_twice():
    """offsets [0, BM + 8, 4, BM + 20]: expert 1's range would start inside expert 0's; it is cut to start where expert 0's ended"""
    from dimsum_amd import native
    BM, _ = _tiles()
    rows = BM + 20
    x = torch.randn(rows, 32, device="cuda")
    ws = [torch.randn(32, 32, device="cuda") for _ in range(3)]
    got = native.moe_gemm(x, torch.tensor([0, BM + 8, 4, rows], dtype=torch.int32, device="cuda"), ws)
    want = native.moe_gemm(x, torch.tensor([0, BM + 8, BM + 8, rows], dtype=torch.int32, device="cuda"), ws)
    assert torch.equal(got, want)
    exact = torch.cat([x[:BM + 8].double() @ ws[0].double().t(), x[BM + 8:].double() @ ws[2].double().t()])
    S = torch.cat([x[:BM + 8].double().abs() @ ws[0].double().abs().t(), x[BM + 8:].double().abs() @ ws[2].double().abs().t()])
    assert ((got.double() - exact).abs() <= eps_grouped(32) * S).all()


# ---- the layer -----------------------------------------------------------------------------------------------------------------------------------
def _gelu64(v):
    return torch.nn.functional.gelu(v)


def layer_bound(m, x, gated):
    """Elementwise bound on |grouped - ungrouped| of one SwitchMLP forward, from float64 restatements of the layer's intermediates. Both paths share
    the routing, permute, activation and combine kernels bit for bit; they differ in the two GEMMs. Per sorted row, e = its expert:
      fc1: the grouped product is within eps_grouped(K1) S1 of the exact one, the ungrouped fp32 GEMM within (K1 + 3) 2^-24 S1 (fp32 accumulation in
           any order), S1 = |x| |W1_e|^T:  d1 = (eps_grouped(K1) + (K1 + 3) 2^-24) S1.
      activation h = gelu(a) g (gated) or gelu(a), a and g carrying their bias: |gelu'| <= 1.13, so
           dh = 1.13 d1_a (|g| + d1_g) + |gelu(a)| d1_g, plus 2^-20 (|gelu(a)| + |a|) (|g| + d1_g) for the two fp32 evaluations of the same kernel
           (erf-GELU and one product: a few ulps of |a| and of the result each); not gated: dh = 1.13 d1 + 2^-20 (|gelu(a)| + |a|).
      fc2: dy = dh |W2_e|^T + (eps_grouped(K2) + (K2 + 3) 2^-24) (|h| + dh) |W2_e|^T + 2^-23 |b2_e|.
      combine: out = prob y with the same prob bits on both sides: d out = prob dy + 2^-23 |out|."""
    ex = m.local_experts
    H = x.shape[-1]
    x2 = x.double().reshape(-1, H)
    logits = x2 @ m.router.weight.double().t() + m.router.bias.double()
    route = torch.sigmoid(logits) if m.routing == "sinkhorn" else torch.softmax(logits, 1)
    prob, e = route.max(1)
    W1 = torch.stack([q.linear_fc1.weight.double() for q in ex])[e]
    W2 = torch.stack([q.linear_fc2.weight.double() for q in ex])[e]
    biased = ex[0].linear_fc1.bias is not None
    K1, K2 = W1.shape[2], W2.shape[2]
    a = torch.einsum("tk,tnk->tn", x2, W1)
    d1 = (eps_grouped(K1) + (K1 + 3) * U) * torch.einsum("tk,tnk->tn", x2.abs(), W1.abs())
    if biased:
        a = a + torch.stack([q.linear_fc1.bias.double() for q in ex])[e]
    if gated:
        (aa, g), (da, dg) = a.chunk(2, 1), d1.chunk(2, 1)
        h = _gelu64(aa) * g
        dh = 1.13 * da * (g.abs() + dg) + _gelu64(aa).abs() * dg + 2.0 ** -20 * (_gelu64(aa).abs() + aa.abs()) * (g.abs() + dg)
    else:
        h = _gelu64(a)
        dh = 1.13 * d1 + 2.0 ** -20 * (h.abs() + a.abs())
    y = torch.einsum("tk,tnk->tn", h, W2)
    dy = torch.einsum("tk,tnk->tn", dh, W2.abs()) + (eps_grouped(K2) + (K2 + 3) * U) * torch.einsum("tk,tnk->tn", h.abs() + dh, W2.abs())
    if biased:
        b2 = torch.stack([q.linear_fc2.bias.double() for q in ex])[e]
        y, dy = y + b2, dy + 2 * U * b2.abs()
    out = prob.unsqueeze(1) * y
    return (prob.unsqueeze(1) * dy + 2 * U * out.abs()).view(x.shape), e


@pytest.mark.parametrize("mode,gated,bias", CASES)
def test_grouped_layer_on_the_fixtures(mode, gated, bias):
    """the grouped forward under no_grad: the fixture's expert for every token, the fixture's output at Y_TOL, and the ungrouped forward of the same
    module within layer_bound (its docstring states the propagation through the activation and fc2)"""
    from dimsum_amd import native
    g, tag = golden(FILES[mode]), tag_of(gated, bias)
    m = make_switch(mode, gated, bias, int(g[tag + ".seed"]))
    x = T(g["x"])
    bound, e64 = layer_bound(m, x, gated)
    assert torch.equal(e64, T(g[tag + ".expert"]))
    m = m.cuda()
    xg = x.cuda()
    with torch.no_grad():
        plain = m(xg)
        m.set_grouped(True)
        grouped = m(xg)
        expert = native.moe_route_fwd(xg.reshape(-1, x.shape[-1]), m.router.weight.detach(), m.router.bias.detach(),
                                      "sigmoid" if mode == "sinkhorn" else "softmax")[1]
    assert torch.equal(expert.long().cpu(), T(g[tag + ".expert"]))
    assert_close(grouped.cpu().numpy(), g[tag + ".out"], what="out (fixture)", **Y_TOL)
    err = (grouped.double() - plain.double()).abs().cpu()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{mode} {tag}: max |grouped - ungrouped| / bound = {worst:.3f}, max |diff| = {err.max().item():.3e}")
    assert (err <= bound).all(), f"max |grouped - ungrouped| / bound = {worst:.3f}"
    assert not torch.equal(grouped, plain)                      # (another kernel did run)


def test_a_grouped_module_that_trains_gives_the_ungrouped_gradients_bit_for_bit():
    g = golden(FILES["top1"])
    x, dout = T(g["x"]).cuda(), T(g["dout"]).cuda()
    grads = []
    for grouped in (False, True):
        m = make_switch("top1", True, True, 3).cuda()
        m.set_grouped(grouped)
        xg = x.clone().requires_grad_()
        out = m(xg)
        out.backward(dout)
        grads.append([out.detach(), xg.grad] + [p.grad for p in m.parameters()])
    assert len(grads[0]) == len(grads[1]) > 4 and all(torch.equal(a, b) for a, b in zip(*grads))


# ---- capture ---------------------------------------------------------------------------------------------------------------------------------------
# input seeds chosen on the CPU with the float64 router (the model of test_moe_cpu._tiny, procedural_fill seed 5): per-layer expert counts and the
# smallest best / second-best route gap per layer
#   106: [8, 19, 4, 1] (gap 2.6e-2), [6, 13, 2, 11] (1.5e-2)      144: [13, 13, 3, 3] (3.1e-2), [12, 8, 4, 8] (1.6e-2)
#   100: [17, 8, 4, 3] (3.9e-2), [16, 10, 0, 6] (2.2e-2): expert 2 of the second layer receives no token
CAPTURE_SEEDS = {"A": (106, [[8, 19, 4, 1], [6, 13, 2, 11]]), "B": (144, [[13, 13, 3, 3], [12, 8, 4, 8]]), "C": (100, [[17, 8, 4, 3], [16, 10, 0, 6]])}


def capture_inputs(seed):
    return (T(seeded((2, 4, 8, 8), seed)).cuda(), T(seeded((2,), seed + 1000, kind="uniform")).cuda(),
            torch.tensor([(seed * 3) % 10, (seed * 7 + 1) % 10]).cuda())


def test_hip_graph_replay_of_a_grouped_moe_model(monkeypatch):
    """captured on batch A, replayed on B (other expert counts in both layers) and on C (an expert without tokens): bit-identical to the eager grouped
    forward, the criterion of test_model_gpu.test_hip_graph_replay_is_bit_identical"""
    from dimsum_amd import native, switch_mlp
    from dimsum_amd.hip_graph import GraphedForward
    m = procedural_fill(_tiny(), seed=5).cuda().eval()
    assert switch_mlp.set_grouped(m, True) == 2
    counts, eager = {}, {}
    real = native.moe_route_fwd
    with monkeypatch.context() as mp:                            # the precondition, from an eager run: a host read here is the test's, not the layer's
        seen = []
        mp.setattr(native, "moe_route_fwd", lambda *a: (lambda r: (seen.append(torch.diff(r[3]).tolist()), r)[1])(real(*a)))
        for name, (seed, want) in CAPTURE_SEEDS.items():
            seen.clear()
            with torch.no_grad():
                eager[name] = m(*capture_inputs(seed))
            counts[name] = list(seen)
            assert counts[name] == want, f"precondition: batch {name} routes {counts[name]}, the float64 router {want}"
    assert all(a != b for a, b in zip(counts["A"], counts["B"])) and any(0 in c for c in counts["C"])
    assert eager["A"].abs().max() > 0 and not torch.equal(eager["A"], eager["B"])
    g = GraphedForward(m)
    for name in ("A", "B", "C", "A"):
        assert torch.equal(g(*capture_inputs(CAPTURE_SEEDS[name][0])), eager[name]), f"replay on batch {name}"
    assert len(g.graphs) == 1
