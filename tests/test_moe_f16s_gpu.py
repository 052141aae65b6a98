"""The grouped expert GEMM on scaled-fp16 images (csrc/moe_gemm_f16.hip) and the grouped SwitchMLP forward under the "f16s" policy, on the GPU:
the two producers against rows_f16s of the fp32 passes bit for bit, the kernel against float64 on the decoded images at the tile edges of
test_moe_grouped_gpu.kernel_cases(), the product next to emulated TF32, the layer against float64 next to an emulated-TF32 run, the launches a
layer issues, and an is_moe model replayed from a captured hipGraph.

The kernel's bound (derived, not measured): the operands ARE the fp16 images, the product of two fp16 values is exact in fp32 and the two inverse
scales are powers of two, so the only error is the fp32 accumulation of K terms (and the bias add):
    |got - exact| <= (K + 3) 2^-24 S + 2^-24 |bias|,   S = x_inv w_inv sum_k |x16| |w16|
-- the accumulation term of the fp32 grouped kernel's bound (test_moe_grouped_gpu)."""
import numpy as np
import pytest
import torch

from procedural import procedural_fill, seeded
from test_moe_cpu import CASES, make_switch, switch_args, _tiny
from test_moe_grouped_gpu import CAPTURE_SEEDS, SENTINEL, U, capture_inputs, kernel_cases, _tiles

pytestmark = pytest.mark.gpu
T = torch.from_numpy


@pytest.fixture
def policy(monkeypatch):
    """the "f16s" policy under allow_tf32, restored afterwards"""
    from dimsum_amd import gemm
    monkeypatch.delenv("DIMSUM_MOE_F16S", raising=False)
    monkeypatch.setenv("DIMSUM_SPLIT3_MIN_ROWS", "0")              # (the image carriers' row threshold: these layers are small)
    monkeypatch.setattr(torch.backends.cuda.matmul, "allow_tf32", True)
    gemm.set_policy("f16s")
    yield gemm
    gemm.set_policy("default")


def same_image(got, want):
    return (got.data.shape == want.data.shape and torch.equal(got.data.view(torch.int16), want.data.view(torch.int16)) and torch.equal(got.inv, want.inv))


# ---- 1. the producers, bit for bit ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [32, 160, 1024, 2560])          # (2560: past the 2048 columns a wave keeps in registers)
def test_permute_writes_the_image_of_the_permuted_rows(H):
    from dimsum_amd import native
    g = torch.Generator(device="cuda").manual_seed(H)
    rows = 203                                                # no multiple of the 4 rows of a workgroup
    x = torch.randn(rows, H, device="cuda", generator=g) * torch.logspace(-6, 6, rows, device="cuda")[:, None]
    x[7] = 0.0                                                # a zero row
    x[11, H // 3] = 1e4 * x[11].abs().max()                   # one outlier
    perm = torch.randperm(rows, device="cuda", generator=g).to(torch.int32)
    got = native.moe_permute(x, perm, split3="f16s")
    want = native.rows_f16s(native.moe_permute(x, perm))
    assert isinstance(got, native.F16Image) and same_image(got, want)
    assert torch.isfinite(got.data).all()
    assert native.moe_permute(x[:0], perm[:0], split3="f16s").data.shape == (0, H)


@pytest.mark.parametrize("W", [32, 1024, 5120, 5152])         # (5152: past the pass's width, converted by the host)
@pytest.mark.parametrize("gated", [True, False])
def test_activation_writes_the_image_of_h(W, gated, monkeypatch):
    from dimsum_amd import native
    g = torch.Generator(device="cuda").manual_seed(W + gated)
    rows, S = 37, (2 * W if gated else W)
    x = torch.randn(rows, S, device="cuda", generator=g) * torch.logspace(-3, 3, rows, device="cuda")[:, None]
    x[5] = 0.0
    singles = []
    real = native.rows_f16s
    for E in (1, 8):
        bias_table = torch.randn(E, S, device="cuda", generator=g)
        row_expert = torch.sort(torch.randint(0, E, (rows,), device="cuda", generator=g)).values.to(torch.int32)
        for bias in (None, bias_table):
            for re in ((None, row_expert) if E == 1 else (row_expert,)):
                want = real(native.moe_act_fwd(x, bias, re, gated))
                with monkeypatch.context() as mp:
                    mp.setattr(native, "rows_f16s", lambda *a, **k: (singles.append(1), real(*a, **k))[1])
                    got = native.moe_act_fwd(x, bias, re, gated, split3="f16s")
                assert same_image(got, want), (E, bias is not None, re is not None)
    assert (len(singles) > 0) == (W > 5120)                   # the pass writes the image itself up to its width limit


# ---- 2. the kernel against float64 on the decoded images --------------------------------------------------------------------------------------------
def _case_operands(case):
    from dimsum_amd import native
    name, counts, K, N, biased = kernel_cases()[case]
    E, rows = len(counts), sum(counts)
    x = T(seeded((rows, K), 800 + case)).cuda()
    w = T(seeded((E, N, K), 820 + case, scale=K ** -0.5)).cuda()
    b = T(seeded((E, N), 840 + case)).cuda() if biased else None
    off = T(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).cuda()
    x16 = native.rows_f16s(x)
    w16 = [native.rows_f16s(w[i].contiguous()) for i in range(E)]
    return name, counts, K, N, x16, w16, b, off


def exact_and_bound(x16, w16, b, e, K):
    """float64 on the decoded images: (exact, bound) per output element; e: the expert of every row"""
    xd, xi = x16.data.double().cpu(), x16.inv.double().cpu()
    wd = torch.stack([w.data.double().cpu() for w in w16])[e]
    wi = torch.stack([w.inv.double().cpu() for w in w16])[e]
    scale = xi[:, None] * wi
    exact = torch.einsum("tk,tnk->tn", xd, wd) * scale
    bound = (K + 3) * U * torch.einsum("tk,tnk->tn", xd.abs(), wd.abs()) * scale
    if b is not None:
        exact = exact + b.double().cpu()[e]
        bound = bound + U * b.double().cpu().abs()[e]
    return exact, bound


@pytest.mark.parametrize("case", range(8))
def test_kernel_against_float64_on_the_decoded_images(case):
    from dimsum_amd import native
    name, counts, K, N, x16, w16, b, off = _case_operands(case)
    rows = sum(counts)
    e = torch.from_numpy(np.repeat(np.arange(len(counts)), counts)).long()
    exact, bound = exact_and_bound(x16, w16, b, e, K)
    guard, ldc = 3, N + 12
    buf = torch.full((guard + rows + guard, ldc), SENTINEL, device="cuda")
    out = buf[guard:guard + rows, :N]
    got = native.moe_gemm_f16s(x16, off, w16, b, out=out)
    assert got.data_ptr() == out.data_ptr()
    err = (got.double().cpu() - exact).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{name}: max |err| / bound = {worst:.3f}, max |err| = {err.max().item():.3e}")
    assert (err <= bound).all(), f"{name}: max |err| / bound = {worst:.3f}"                 # (a row left unwritten holds the sentinel: far outside)
    image = buf.cpu()
    keep = torch.full_like(image, SENTINEL)
    keep[guard:guard + rows, :N] = image[guard:guard + rows, :N]
    assert torch.equal(image.view(torch.int32), keep.view(torch.int32)), f"{name}: a guard row or guard column was written"
    again = native.moe_gemm_f16s(x16, off, w16, b)
    assert again.is_contiguous() and torch.equal(again.view(torch.int32), got.contiguous().view(torch.int32)), f"{name}: two calls differ"


def _small(rows, E=3, K=32, N=32):
    from dimsum_amd import native
    x16 = native.rows_f16s(torch.randn(rows, K, device="cuda"))
    w16 = [native.rows_f16s(torch.randn(N, K, device="cuda")) for _ in range(E)]
    return x16, w16


def test_rows_outside_every_range_are_not_written_and_an_empty_call_runs():
    from dimsum_amd import native
    BM, _ = _tiles()
    x16, w16 = _small(BM + 9)
    out = torch.full((BM + 9, 32), SENTINEL, device="cuda")
    native.moe_gemm_f16s(x16, torch.tensor([2, 2, BM + 4, BM + 4], dtype=torch.int32, device="cuda"), w16, out=out)       # rows [2, BM + 4) of expert 1 only
    assert (out[:2] == SENTINEL).all() and (out[BM + 4:] == SENTINEL).all() and (out[2:BM + 4] != SENTINEL).all()
    zero = torch.zeros(4, dtype=torch.int32, device="cuda")
    native.moe_gemm_f16s(x16, zero, w16, out=out.fill_(SENTINEL))                              # every expert empty: nothing is written
    assert (out == SENTINEL).all()
    empty = native.F16Image(x16.data[:0], x16.inv[:0])
    assert native.moe_gemm_f16s(empty, zero, w16).shape == (0, 32)                            # T = 0


def test_a_table_that_is_not_monotonic_writes_no_row_twice():
    """offsets [0, BM + 8, 4, BM + 20]: expert 1's range would start inside expert 0's; it is cut to start where expert 0's ended"""
    from dimsum_amd import native
    BM, _ = _tiles()
    rows = BM + 20
    x16, w16 = _small(rows)
    got = native.moe_gemm_f16s(x16, torch.tensor([0, BM + 8, 4, rows], dtype=torch.int32, device="cuda"), w16)
    want = native.moe_gemm_f16s(x16, torch.tensor([0, BM + 8, BM + 8, rows], dtype=torch.int32, device="cuda"), w16)
    assert torch.equal(got, want)
    e = torch.tensor([0] * (BM + 8) + [2] * 12)
    exact, bound = exact_and_bound(x16, w16, None, e, 32)
    assert ((got.double().cpu() - exact).abs() <= bound).all()


# ---- 3. never less accurate than TF32 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adversarial", [False, True])
def test_product_is_never_less_accurate_than_tf32(adversarial):
    """the rule and the factors of test_f16s_gpu.test_product_is_never_less_accurate_than_tf32, per expert range of one grouped launch"""
    from dimsum_amd import native
    from dimsum_amd.utils.tf32_emulation import round_tf32
    BM, BN = _tiles()
    counts, K, N = [2 * BM + 3, 0, BM - 1, BM + 1], 160, BN + 32
    rows, E = sum(counts), len(counts)
    g = torch.Generator(device="cuda").manual_seed(5)
    x, w = torch.randn(rows, K, device="cuda", generator=g), torch.randn(E, N, K, device="cuda", generator=g) * K ** -0.5
    if adversarial:
        x = x * torch.logspace(-6, 6, rows, device="cuda")[:, None]
        x[torch.arange(rows), torch.randint(0, K, (rows,), device="cuda", generator=g)] *= 1e4
        w = w * torch.logspace(-3, 3, N, device="cuda")[None, :, None]
    e = torch.from_numpy(np.repeat(np.arange(E), counts)).long().cuda()
    ref = torch.einsum("tk,tnk->tn", x.double(), w.double()[e])
    row = ref.abs().amax(-1, keepdim=True)                                        # errors are judged per output row (its own magnitude)
    off = T(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).cuda()
    got = native.moe_gemm_f16s(native.rows_f16s(x), off, [native.rows_f16s(w[i].contiguous()) for i in range(E)])
    tf = torch.einsum("tk,tnk->tn", round_tf32(x).double(), round_tf32(w).double()[e]).float()           # exact products of TF32 operands, one fp32 rounding
    e_got, e_tf = ((got.double() - ref).abs() / row), ((tf.double() - ref).abs() / row)
    print(f"adversarial={adversarial}: f16s max {e_got.max().item():.3e} rms {e_got.pow(2).mean().sqrt().item():.3e}, "
          f"TF32 max {e_tf.max().item():.3e} rms {e_tf.pow(2).mean().sqrt().item():.3e}")
    assert torch.isfinite(got).all()
    assert e_got.max().item() <= 1.05 * e_tf.max().item() + 1e-6, (e_got.max().item(), e_tf.max().item())
    assert e_got.pow(2).mean().sqrt().item() <= 1.05 * e_tf.pow(2).mean().sqrt().item() + 1e-7


# ---- 4. the layer ------------------------------------------------------------------------------------------------------------------------------------
LAYER_CASES = [(mode, gated, bias, 32, 4) for mode, gated, bias in CASES] + [("top1", True, True, 160, 8)]


@pytest.mark.parametrize("mode,gated,bias,dim,experts", LAYER_CASES)
def test_layer_under_the_policy(mode, gated, bias, dim, experts, policy, monkeypatch):
    """SwitchMLP(grouped=True) under the policy: the experts of the default policy exactly; the output against float64 switch_mlp_torch next to an
    emulated-TF32 run of the same layer (the margins of test_f16s_gpu's module-level comparisons: 1.25 x in max, 1.1 x in rms); switched off by
    DIMSUM_MOE_F16S=0 or without allow_tf32 it is the parent path bit for bit and the new kernel is not called"""
    from dimsum_amd import native
    from dimsum_amd.ops import switch_mlp_torch
    from dimsum_amd.utils.tf32_emulation import emulated_tf32
    gemm = policy
    m = make_switch(mode, gated, bias, 11, dim=dim, experts=experts)
    x = T(seeded((4, 96, dim), 31))
    ref, e64 = switch_mlp_torch(x, *[a if a is None or torch.is_tensor(a) else list(a) for a in switch_args(m)], routing_mode=mode, gated=gated)
    ref = ref.detach()
    m = m.cuda()
    xg = x.cuda()
    experts_seen, f16s_calls = [], []
    real_route, real_gemm = native.moe_route_fwd, native.moe_gemm_f16s
    monkeypatch.setattr(native, "moe_route_fwd", lambda *a: (lambda r: (experts_seen.append(r[1].clone()), r)[1])(real_route(*a)))
    monkeypatch.setattr(native, "moe_gemm_f16s", lambda *a, **k: (f16s_calls.append(1), real_gemm(*a, **k))[1])
    with torch.no_grad():
        with emulated_tf32():
            tf = m(xg)                                           # (ungrouped: its per-expert torch products with TF32-rounded operands)
        m.set_grouped(True)
        one = m(xg)
        assert len(f16s_calls) == 2
        gemm.set_policy("default")
        parent = m(xg)
        gemm.set_policy("f16s")
        monkeypatch.setenv("DIMSUM_MOE_F16S", "0")
        off_env = m(xg)
        monkeypatch.delenv("DIMSUM_MOE_F16S")
        monkeypatch.setattr(torch.backends.cuda.matmul, "allow_tf32", False)
        off_tf32 = m(xg)
        monkeypatch.setattr(torch.backends.cuda.matmul, "allow_tf32", True)
    assert len(f16s_calls) == 2                                  # none of the three switched-off runs called the new kernel
    assert torch.equal(off_env, parent) and torch.equal(off_tf32, parent) and not torch.equal(one, parent)
    assert len(experts_seen) == 5 and all(torch.equal(s, experts_seen[0]) for s in experts_seen)
    assert torch.equal(experts_seen[1].long().cpu(), e64)
    d1, dt = (one.double().cpu() - ref).abs(), (tf.double().cpu() - ref).abs()
    (m1, r1), (mt, rt) = (d1.max().item(), d1.pow(2).mean().sqrt().item()), (dt.max().item(), dt.pow(2).mean().sqrt().item())
    print(f"{mode} gated={gated} bias={bias} dim={dim}: f16s max {m1:.3e} rms {r1:.3e}, emulated TF32 max {mt:.3e} rms {rt:.3e}")
    assert m1 <= 1.25 * mt and r1 <= 1.1 * rt, ((m1, r1), (mt, rt))


# ---- 5. the launches ---------------------------------------------------------------------------------------------------------------------------------
def test_a_layer_issues_six_launches_and_no_conversion_of_its_own(policy, monkeypatch):
    from dimsum_amd import native
    gemm = policy
    m = make_switch("top1", True, True, 11, dim=160, experts=8).cuda()
    m.set_grouped(True)
    x = T(seeded((4, 96, 160), 31)).cuda()
    log = []
    for name in ("moe_route_fwd", "moe_permute", "moe_gemm", "moe_gemm_f16s", "moe_act_fwd", "moe_combine_fwd", "rows_f16s", "rows_f16s_multi", "split3_rows"):
        real = getattr(native, name)
        monkeypatch.setattr(native, name, (lambda real, name: lambda *a, **k: (log.append(name), real(*a, **k))[1])(real, name))
    six = ["moe_route_fwd", "moe_permute", "moe_gemm_f16s", "moe_act_fwd", "moe_gemm_f16s", "moe_combine_fwd"]
    with torch.no_grad():
        bare = m(x)
        assert [n for n in log if n != "rows_f16s_multi"] == six and log.count("rows_f16s_multi") == 1       # 16 weights: one multi-job launch
        log.clear()
        with gemm.forward_scope(m, x.shape[0] * x.shape[1]):
            assert log == ["rows_f16s_multi"]                    # the scope's launch holds the 2 E expert images
            log.clear()
            scoped = m(x)
        assert log == six
    assert torch.equal(scoped, bare)


# ---- 6. capture --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.usefixtures("allow_torch_sdpa")
def test_hip_graph_replay_of_a_grouped_moe_model_under_the_policy(policy, monkeypatch):
    """captured on batch A, replayed on B (other expert counts in both layers) and on C (an expert without tokens): bit-identical to the eager grouped
    forward under the policy (the pattern and the batches of test_moe_grouped_gpu)"""
    from dimsum_amd import native, switch_mlp
    from dimsum_amd.hip_graph import GraphedForward
    m = procedural_fill(_tiny(), seed=5).cuda().eval()
    assert switch_mlp.set_grouped(m, True) == 2
    counts, eager, calls = {}, {}, []
    real, real_gemm = native.moe_route_fwd, native.moe_gemm_f16s
    monkeypatch.setattr(native, "moe_gemm_f16s", lambda *a, **k: (calls.append(1), real_gemm(*a, **k))[1])
    with monkeypatch.context() as mp:                            # the precondition, from an eager run: a host read here is the test's, not the layer's
        seen = []
        mp.setattr(native, "moe_route_fwd", lambda *a: (lambda r: (seen.append(torch.diff(r[3]).tolist()), r)[1])(real(*a)))
        for name, (seed, _) in CAPTURE_SEEDS.items():
            seen.clear()
            with torch.no_grad():
                eager[name] = m(*capture_inputs(seed))
            counts[name] = list(seen)
    assert len(calls) == 3 * 4                                   # two layers, two products each, per batch
    assert all(a != b for a, b in zip(counts["A"], counts["B"])) and any(0 in c for c in counts["C"]), counts
    assert eager["A"].abs().max() > 0 and not torch.equal(eager["A"], eager["B"])
    g = GraphedForward(m)
    for name in ("A", "B", "C", "A"):
        assert torch.equal(g(*capture_inputs(CAPTURE_SEEDS[name][0])), eager[name]), f"replay on batch {name}"
    assert len(g.graphs) == 1
