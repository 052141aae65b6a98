"""The mixture-of-experts row passes (csrc/moe.hip, csrc/act_rows.hip) and layers on the GPU, against float64 restatements on the CPU, the fixtures of the
reference (tests/golden/moe_switch*.npz) and the CPU stand-ins of test_moe_cpu.

Routing inputs are seeded so that, in float64, every token's best and second-best route values differ by at least 1e-4 (asserted on the CPU
before anything is compared): an fp32 kernel whose logits are good to ~1e-6 then has to choose the oracle's expert for every token."""
import numpy as np
import pytest
import torch

from conftest import assert_close, golden
from procedural import procedural_fill, seeded
from test_blocks_linear_window_gpu import G_TOL, SUM_TOL, Y_TOL
from test_moe_cpu import CASES, FILES, STANDINS, make_switch, named_grads, switch_args, tag_of, tiny_inputs, _tiny

pytestmark = pytest.mark.gpu
T = torch.from_numpy
ROW_TOL = (3e-4, 1e-3)          # the suite's fp32 row-pass tolerance (rtol, atol)
MIN_GAP = 1e-4


@pytest.fixture(autouse=True)
def _fp32_matmul():
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.set_float32_matmul_precision("highest")


def n(t):
    return t.detach().cpu().numpy()


def route_inputs(tokens, hidden, experts, seed):
    return (T(seeded((tokens, hidden), seed)), T(seeded((experts, hidden), seed + 1, scale=hidden ** -0.5)), T(seeded((experts,), seed + 2, scale=0.1)))


def route_oracle(x, w, b, mode):
    """float64 on the CPU -> prob, expert, logits, and the smallest best / second-best gap over the tokens"""
    logits = x.double() @ w.double().t() + (0 if b is None else b.double())
    route = torch.sigmoid(logits) if mode == "sigmoid" else torch.softmax(logits, dim=1)
    prob, e = torch.max(route, dim=1)
    gap = float("inf") if w.shape[0] == 1 else (route.topk(2, dim=1).values @ torch.tensor([1.0, -1.0], dtype=torch.float64)).min().item()
    return prob, e, logits, gap


def check_tables(e, experts, offsets, perm, inv, row_expert):
    """the sort's tables against a stable argsort of the chosen experts, exactly"""
    e = e.cpu().long()
    want_perm = torch.argsort(e, stable=True)
    want_inv = torch.empty_like(want_perm)
    want_inv[want_perm] = torch.arange(e.numel())
    want_off = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(torch.bincount(e, minlength=experts), 0)])
    assert torch.equal(offsets.cpu().long(), want_off)
    assert torch.equal(perm.cpu().long(), want_perm) and torch.equal(inv.cpu().long(), want_inv) and torch.equal(row_expert.cpu().long(), e[want_perm])


# (tokens, hidden, experts, mode, seed): pairwise covering -- every pair of values of every two of the four axes (tokens x hidden, tokens x experts,
# tokens x mode, hidden x experts, hidden x mode, experts x mode) occurs in at least one case (test_route_cases_cover_every_pair enumerates them);
# the seeds were picked on the CPU for the gap precondition
ROUTE_CASES = [
    (1, 4, 1, "softmax", 100), (63, 64, 2, "sigmoid", 110), (65, 260, 3, "softmax", 120), (257, 1152, 8, "sigmoid", 131), (1000, 64, 9, "softmax", 140),
    (1000, 1152, 64, "sigmoid", 160), (257, 4, 64, "softmax", 184), (65, 64, 8, "softmax", 170), (63, 260, 9, "sigmoid", 180),
    (1, 1152, 2, "softmax", 190), (1000, 260, 1, "sigmoid", 200), (257, 64, 3, "sigmoid", 210), (1000, 4, 2, "sigmoid", 221),
    (65, 1152, 9, "softmax", 230), (63, 4, 8, "sigmoid", 240), (257, 260, 2, "softmax", 250), (1, 64, 64, "sigmoid", 260), (1000, 260, 8, "softmax", 270),
    (65, 4, 1, "sigmoid", 280), (63, 1152, 3, "softmax", 290), (1, 260, 9, "softmax", 300), (257, 1152, 1, "softmax", 310), (63, 64, 64, "softmax", 320),
    (65, 260, 64, "sigmoid", 330), (1000, 64, 3, "sigmoid", 340), (1, 4, 8, "softmax", 350), (257, 64, 9, "sigmoid", 360), (65, 1152, 2, "sigmoid", 370),
    (63, 4, 3, "softmax", 380), (1, 4, 3, "sigmoid", 390), (1, 64, 9, "sigmoid", 400), (63, 64, 1, "sigmoid", 500), (65, 4, 9, "softmax", 510),
    (63, 4, 1, "softmax", 520),
]
ROUTE_AXES = ([1, 63, 65, 257, 1000], [4, 64, 260, 1152], [1, 2, 3, 8, 9, 64], ["softmax", "sigmoid"])


def test_route_cases_cover_every_pair():
    import itertools
    for i, j in itertools.combinations(range(4), 2):
        have = {(c[i], c[j]) for c in ROUTE_CASES}
        assert not [(a, b) for a in ROUTE_AXES[i] for b in ROUTE_AXES[j] if (a, b) not in have], (i, j)


@pytest.mark.parametrize("tokens,hidden,experts,mode,seed", ROUTE_CASES)
def test_route_and_sort(tokens, hidden, experts, mode, seed):
    from dimsum_amd import native
    x, w, b = route_inputs(tokens, hidden, experts, seed)
    prob, e, logits, gap = route_oracle(x, w, b, mode)
    assert gap >= MIN_GAP, f"precondition: smallest best / second-best gap {gap:.3e}"
    got = native.moe_route_fwd(x.cuda(), w.cuda(), b.cuda(), mode)
    again = native.moe_route_fwd(x.cuda(), w.cuda(), b.cuda(), mode)
    assert torch.equal(got[1].cpu().long(), e)
    assert_close(n(got[0]), n(prob), *ROW_TOL, "prob")
    assert_close(n(got[2]), n(logits), *ROW_TOL, "logits")
    check_tables(got[1], experts, *got[3:])
    for a, c in zip(got, again):
        assert torch.equal(a, c)
    assert all(t.dtype == torch.int32 for t in (got[1],) + tuple(got[3:]))


@pytest.mark.parametrize("mode", ["softmax", "sigmoid"])
def test_exact_ties_go_to_the_lower_index(mode):
    """experts 1 and 2 share their router row and bias: their route values are equal bit for bit, and expert 2 is never chosen"""
    from dimsum_amd import native
    x, w, b = route_inputs(257, 260, 4, 77)
    w[2], b[2] = w[1], b[1]
    w[0], w[3] = -w[1], 0.0
    _, e, _, _ = route_oracle(x, w, b, mode)
    assert (e == 1).sum() > 50 and (e == 2).sum() == 0          # (torch's own rule on the oracle's exact ties)
    got = native.moe_route_fwd(x.cuda(), w.cuda(), b.cuda(), mode)
    assert torch.equal(got[2][:, 1], got[2][:, 2])
    ge = got[1].cpu().long()
    assert (ge == 2).sum() == 0 and torch.equal(ge == 1, e == 1)
    check_tables(got[1], 4, *got[3:])


def test_degenerate_routing():
    from dimsum_amd import native
    x, w, b = route_inputs(257, 64, 4, 88)
    b[3] = 50.0                                                   # every token to expert 3
    got = native.moe_route_fwd(x.cuda(), w.cuda(), b.cuda(), "softmax")
    assert torch.equal(got[1].cpu(), torch.full((257,), 3, dtype=torch.int32))
    assert got[3].tolist() == [0, 0, 0, 0, 257] and torch.equal(got[4].cpu().long(), torch.arange(257))
    b[3] = -50.0                                                  # expert 3 receives no token
    got = native.moe_route_fwd(x.cuda(), w.cuda(), b.cuda(), "softmax")
    assert (got[1] == 3).sum() == 0 and got[3].tolist()[3] == got[3].tolist()[4] == 257
    check_tables(got[1], 4, *got[3:])


@pytest.mark.parametrize("tokens,hidden", [(257, 260), (1000, 1152), (1, 4), (65, 64)])
def test_permute_and_combine(tokens, hidden):
    from dimsum_amd import native
    perm = torch.from_numpy(np.random.RandomState(tokens).permutation(tokens))
    x, y, prob = T(seeded((tokens, hidden), 1)), T(seeded((tokens, hidden), 2)), T(seeded((tokens,), 3, kind="uniform"))
    xg, yg, pg, permg = x.cuda(), y.cuda(), prob.cuda(), perm.int().cuda()
    assert torch.equal(native.moe_permute(xg, permg).cpu(), x[perm])
    want = torch.empty_like(y)
    want[perm] = prob[perm].unsqueeze(1) * y
    assert torch.equal(native.moe_combine_fwd(yg, permg, pg).cpu(), want)
    dy, dprob = native.moe_combine_bwd(xg, yg, permg, pg)        # (x plays dout)
    d = x.double()[perm]
    want_dprob = torch.empty(tokens, dtype=torch.float64)
    want_dprob[perm] = (d * y.double()).sum(1)
    assert_close(n(dy), n(prob.double()[perm].unsqueeze(1) * d), *ROW_TOL, "dy")
    assert_close(n(dprob), n(want_dprob), *ROW_TOL, "dprob")


# 200 sorted rows over 7 experts: the first chunk of 64 rows holds two expert boundaries (rows 10, 40), the second three (70, 90, 100); expert 6 has no row
ROW_EXPERT = torch.tensor([0] * 10 + [1] * 30 + [2] * 30 + [3] * 20 + [4] * 10 + [5] * 100, dtype=torch.int32)


@pytest.mark.parametrize("biased", [True, False])
@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize("width", [8, 1024, 1028])
def test_activation_forward_and_backward(width, gated, biased):
    from dimsum_amd import native
    from dimsum_amd.ops import moe_act_torch
    rows, S = ROW_EXPERT.numel(), (2 if gated else 1) * width
    x, dh = T(seeded((rows, S), 5)), T(seeded((rows, width), 6))
    bias = T(seeded((7, S), 7, scale=0.5)) if biased else None
    xr = x.double().requires_grad_()
    br = None if bias is None else bias.double().requires_grad_()
    want = moe_act_torch(xr, br, ROW_EXPERT, gated)
    want.backward(dh.double())
    re, bg = ROW_EXPERT.cuda(), (None if bias is None else bias.cuda())
    assert_close(n(native.moe_act_fwd(x.cuda(), bg, re, gated)), n(want), *ROW_TOL, "h")
    dx, dbias = native.moe_act_bwd(x.cuda(), bg, re, dh.cuda(), gated)
    assert_close(n(dx), n(xr.grad), *ROW_TOL, "dx")
    if biased:
        assert_close(n(dbias), n(br.grad), 0, 0, "dbias", scale_atol=rows * 2.0 ** -23)
        assert torch.count_nonzero(dbias[6]) == 0
    else:
        assert dbias is None


def test_activation_without_a_table_is_the_one_expert_pass():
    from dimsum_amd.ops import moe_act, moe_act_torch
    x, b = T(seeded((70, 24), 8)).cuda().requires_grad_(), T(seeded((24,), 9)).cuda().requires_grad_()
    y = moe_act(x, b, gated=True)
    y.backward(torch.ones_like(y))
    xr, br = x.detach().cpu().double().requires_grad_(), b.detach().cpu().double().requires_grad_()
    want = moe_act_torch(xr, br.reshape(1, -1), None, True)
    want.backward(torch.ones_like(want))
    assert_close(n(y), n(want), *ROW_TOL, "h")
    assert_close(n(x.grad), n(xr.grad), *ROW_TOL, "dx")
    assert_close(n(b.grad), n(br.grad), 0, 0, "dbias", scale_atol=70 * 2.0 ** -23)


MODULE_SEEDS = {(32, 48): 501, (32, 513): 613, (128, 48): 621, (128, 513): 634}


@pytest.mark.parametrize("mode,gated,bias", CASES)
@pytest.mark.parametrize("dim,shape", [(32, (2, 24)), (32, (3, 171)), (128, (2, 24)), (128, (3, 171))])
def test_switch_mlp_forward_and_all_gradients(dim, shape, mode, gated, bias):
    from dimsum_amd.ops import switch_mlp_torch
    ci = CASES.index((mode, gated, bias)) % 4
    m = make_switch(mode, gated, bias, 40 + ci, dim=dim)
    x = T(seeded(shape + (dim,), MODULE_SEEDS[(dim, shape[0] * shape[1])]))
    dout = T(seeded(shape + (dim,), 502))
    args = switch_args(m)
    xr = x.double().requires_grad_()
    want, e = switch_mlp_torch(xr, *args, routing_mode=mode, gated=gated)
    want.backward(dout.double())
    gap = route_oracle(x.reshape(-1, dim), m.router.weight.detach(), m.router.bias.detach(), "sigmoid" if mode == "sinkhorn" else "softmax")[3]
    assert gap >= MIN_GAP, f"precondition: smallest best / second-best gap {gap:.3e}"
    want_grads = named_grads(m, args)
    m = m.cuda()
    xg = x.cuda().requires_grad_()
    out = m(xg)
    out.backward(dout.cuda())
    assert_close(n(out), n(want), what="out", **Y_TOL)
    assert_close(n(xg.grad), n(xr.grad), what="dx", **G_TOL)
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        assert_close(n(p.grad), n(want_grads[k]), what=k, **SUM_TOL)
    if dim == 32 and shape == (2, 24):                  # the reference's own numbers
        g, tag = golden(FILES[mode]), tag_of(gated, bias)
        assert int(g[tag + ".seed"]) == 40 + ci and np.array_equal(g["x"], n(x)) and np.array_equal(g["dout"], n(dout))
        assert_close(n(out), g[tag + ".out"], what="out (fixture)", **Y_TOL)
        assert_close(n(xg.grad), g[tag + ".dx"], what="dx (fixture)", **G_TOL)
        for k, p in m.named_parameters():
            assert_close(n(p.grad), g[f"{tag}.grad.{k}"], what=k + " (fixture)", **SUM_TOL)


def test_an_expert_without_tokens_gets_zero_gradients():
    m = make_switch("top1", True, True, 3)
    with torch.no_grad():
        m.router.bias[1] = -1e4
    m = m.cuda()
    x = T(seeded((2, 24, 32), 9)).cuda().requires_grad_()
    m(x).square().sum().backward()
    assert all(p.grad is not None and torch.count_nonzero(p.grad) == 0 for p in m.local_experts[1].parameters())
    assert all(torch.count_nonzero(p.grad) > 0 for p in m.local_experts[0].parameters())


def _published_tiny():
    """what `train.py --is-moe` builds (create_model.published_config), at the tiny size: fused add + RMSNorm in every block -- MoEBlock's
    rms_norm_fn(prenorm=True) branch --, "combined" blocks with conditioned mixers, the shared attention block every 4 layers"""
    from test_model_cpu import _published
    return _tiny(**{k: v for k, v in _published().items() if k not in ("img_resolution", "num_classes")})


DIM_CONFIGS = {"default": lambda: _tiny(), "final_norm": lambda: _tiny(use_final_norm=True), "published": _published_tiny}


@pytest.mark.usefixtures("allow_torch_sdpa")
@pytest.mark.parametrize("config", list(DIM_CONFIGS))
def test_dim_is_moe_forward_and_backward_match_the_cpu_standins(config, monkeypatch):
    """The same model on the GPU and on the CPU stand-ins: output and every parameter gradient. Every router's best / second-best route gap is
    asserted on the CPU run (>= 1e-4, as in the routing tests), so no token can change its expert between two fp32 implementations.
    In "default" (no final norm, no attention block) the LAST MoE block's output goes straight into the final layer's LayerNorm, which does not see
    a token's scale: d out / d prob of that block is zero up to the norm's eps, the kernel's <dout, y> cancels to ~7e-6 of its terms (measured
    on the CPU stand-ins) and that one router's gradient is roundoff in ANY fp32 implementation -- it is the only gradient left out, and only
    there. In "final_norm" (norm_f over residual + x) and "published" (the shared attention block adds its branches to x first) the same dot
    product keeps ~1e-1 of its terms (measured likewise) and every gradient is compared."""
    from dimsum_amd import native
    from oracle.torch_backend import cpu_oracle_backend
    make = DIM_CONFIGS[config]
    x, t, y = tiny_inputs()
    gpu = procedural_fill(make(), seed=5).cuda().eval()
    assert gpu.blocks[1].fused_add_norm == (config == "published")
    out = gpu(x.cuda(), t.cuda(), y.cuda())
    out.square().sum().backward()
    cpu = procedural_fill(make(), seed=5).eval()
    gaps = []

    with monkeypatch.context() as mp:
        for k, f in STANDINS.items():
            mp.setattr(native, k, f)
        real = native.moe_route_fwd
        mp.setattr(native, "moe_route_fwd", lambda x_, w_, b_, mode: (gaps.append(route_oracle(x_, w_, b_, mode)[3]), real(x_, w_, b_, mode))[1])
        with cpu_oracle_backend():
            want = cpu(x, t, y)
            want.square().sum().backward()
    assert len(gaps) == 2 and min(gaps) >= MIN_GAP, f"precondition: smallest best / second-best gap per router {gaps}"
    assert want.abs().max() > 0
    assert_close(n(out), n(want), what="out", **Y_TOL)
    skip = () if config != "default" else ("blocks.3.mixer.router.weight", "blocks.3.mixer.router.bias")
    compared = 0
    for (k, p), q in zip(gpu.named_parameters(), cpu.parameters()):
        assert (p.grad is None) == (q.grad is None), k
        if q.grad is not None and k not in skip:
            assert_close(n(p.grad), n(q.grad), what=k, **SUM_TOL)
            compared += 1
    assert compared > 40 and gpu.blocks[1].mixer.router.weight.grad.abs().max() > 0


def test_fp16_policy_serves_inference_only():
    """gemm.set_policy("fp16") is an inference policy: a forward that trains keeps fp32 expert GEMMs (bit for bit the default policy's), a forward
    under no_grad multiplies fp16 operands. Bound of the latter: each operand rounds to 11 bits (2^-11 relative), so a product's terms move by
    <= 2^-10 ~ 1e-3 and two chained GEMMs by ~2e-3 of the terms' magnitude; 1e-2 of max|out| leaves the accumulation's cancellation room."""
    from dimsum_amd import gemm
    m = make_switch("top1", True, False, 3, dim=128).cuda()
    x = T(seeded((2, 24, 128), 9)).cuda()
    with torch.no_grad():
        base = m(x)
    old = gemm.get_policy()
    gemm.set_policy("fp16")
    try:
        train = m(x)                                   # (the parameters require grad)
        with torch.no_grad():
            inf = m(x)
    finally:
        gemm.set_policy(old)
    assert train.requires_grad and torch.equal(train.detach(), base)
    assert not torch.equal(inf, base)
    assert_close(n(inf), n(base), 0, 0, "fp16 policy", scale_atol=1e-2)


def test_an_empty_batch_runs():
    m = make_switch("top1", True, True, 3).cuda()
    x = torch.zeros(0, 24, 32, device="cuda", requires_grad=True)
    out = m(x)
    assert out.shape == (0, 24, 32)
    out.sum().backward()
    assert x.grad.shape == x.shape and all(p.grad is not None and torch.count_nonzero(p.grad) == 0 for p in m.parameters())


def test_hip_graph_capture_is_refused():
    from dimsum_amd.hip_graph import GraphedForward
    m = _tiny().cuda().eval()
    with pytest.raises(NotImplementedError, match="MoEBlock"):
        GraphedForward(m.forward)
