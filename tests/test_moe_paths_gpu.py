"""The routing passes of csrc/moe.hip on the GPU on the paths that only real sizes reach, against float64 on the CPU. The cases, their oracles and the
preconditions that make each comparison decisive live in test_moe_paths_cpu (which runs without a GPU):

  A. the counting sort with more than 64 blocks (seg >= 2 in moe_scan_kernel), routing steered by construction, everything compared exactly;
  B. the router forward at hidden > 2048 (the tail loop past the 8 register pieces of a row);
  C. moe_route_bwd called directly: several expert groups, several column strips, rows_per_wg 64 and 128;
  D. SwitchMLP with 9 and 16 experts, trained against float64 and grouped against ungrouped.

Every comparison prints max |err| / tolerance before it asserts (pytest -s shows them), and the running maximum of its section."""
import pytest
import torch

from conftest import assert_close
from test_blocks_linear_window_gpu import G_TOL, SUM_TOL, Y_TOL
from test_moe_cpu import named_grads, switch_args
from test_moe_gpu import MIN_GAP, ROW_TOL, check_tables, route_oracle
from test_moe_grouped_gpu import layer_bound
from test_moe_paths_cpu import (BWD_CASES, LAYER_CASES, LAYER_DIM, MODES, SORT_E, SORT_PATTERNS, SORT_SEEDED, SORT_TOKENS, WIDE_CASES, bwd_case,
                                filtered_route_inputs, layer_case, route_of, sort_inputs, wide_inputs, worst_ratio)

pytestmark = pytest.mark.gpu
WORST = {}


@pytest.fixture(autouse=True)
def _fp32_matmul():
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.set_float32_matmul_precision("highest")


def n(t):
    return t.detach().cpu().numpy()


def check(section, what, got, want, rtol, atol=0.0, scale_atol=0.0):
    r = worst_ratio(got, want, rtol, atol, scale_atol)
    WORST[section] = max(WORST.get(section, 0.0), r)
    print(f"[{section}] {what}: max |err| / tolerance = {r:.4f} (section {section} so far: {WORST[section]:.4f})")
    assert_close(n(got), n(want), rtol, atol, what, scale_atol=scale_atol)


def bits(t):
    return t.contiguous().view(torch.int32)


def route_and_compare(section, x, w, b, mode):
    """native.moe_route_fwd against route_oracle as test_moe_gpu.test_route_and_sort compares them: the oracle's expert for every token, prob and
    logits at ROW_TOL, the sort's tables exactly, two calls bit-identical"""
    from dimsum_amd import native
    prob, e, logits, gap = route_oracle(x, w, b, mode)
    assert gap >= MIN_GAP, f"precondition: smallest best / second-best gap {gap:.3e}"
    args = (x.cuda(), w.cuda(), None if b is None else b.cuda(), mode)
    got, again = native.moe_route_fwd(*args), native.moe_route_fwd(*args)
    assert torch.equal(got[1].cpu().long(), e)
    check(section, "prob", got[0], prob, *ROW_TOL)
    check(section, "logits", got[2], logits, *ROW_TOL)
    check_tables(e, w.shape[0], *got[3:])
    for a, c in zip(got, again):
        assert torch.equal(bits(a), bits(c))
    assert all(t.dtype == torch.int32 for t in (got[1],) + tuple(got[3:]))


# ---- A ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pattern", SORT_PATTERNS)
@pytest.mark.parametrize("tokens", list(SORT_TOKENS))
def test_sort_with_more_than_64_blocks(tokens, pattern, mode):
    from dimsum_amd import native
    x, w, f = sort_inputs(tokens, pattern)
    xg, wg = x.cuda(), w.cuda()
    got, again = native.moe_route_fwd(xg, wg, None, mode), native.moe_route_fwd(xg, wg, None, mode)
    assert torch.equal(got[1].cpu().long(), f)
    assert torch.equal(got[2].cpu(), 8.0 * x)                                 # the logits are 8 and 0 in fp32 too
    check_tables(f, SORT_E, *got[3:])
    hot = torch.zeros(1, SORT_E, dtype=torch.float64)
    hot[0, 0] = 8.0
    check("A", f"{tokens} {pattern} {mode} prob", got[0], route_of(hot, mode)[0, 0].expand(tokens), *ROW_TOL)
    for a, c in zip(got, again):
        assert torch.equal(bits(a), bits(c))


@pytest.mark.parametrize("tokens,hidden,experts,mode,seed", SORT_SEEDED)
def test_sort_with_more_than_64_blocks_on_seeded_inputs(tokens, hidden, experts, mode, seed):
    x, w, b, kept = filtered_route_inputs(tokens, hidden, experts, mode, seed)
    assert kept >= tokens and x.shape[0] == tokens
    route_and_compare("A", x, w, b, mode)


# ---- B ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tokens,hidden,experts,mode,seed,biased", WIDE_CASES)
def test_route_forward_on_wide_rows(tokens, hidden, experts, mode, seed, biased):
    x, w, b = wide_inputs(tokens, hidden, experts, seed, biased)
    assert (b is None) == (not biased)
    route_and_compare("B", x, w, b, mode)


# ---- C ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tokens,hidden,experts,mode", BWD_CASES)
def test_route_backward_against_float64(tokens, hidden, experts, mode):
    from dimsum_amd import native
    c = bwd_case(tokens, hidden, experts, mode)
    args = [c[k].cuda() for k in ("x", "w", "logits", "prob", "expert", "inv", "dprob", "dxp")]
    dx, dw, db = native.moe_route_bwd(*args, mode)
    dx2, dw2, db2 = native.moe_route_bwd(*args, mode)
    tag = f"{tokens} x {hidden}, {experts} experts, {mode}"
    check("C", tag + " dx", dx, c["dx"], *ROW_TOL)
    check("C", tag + " dw", dw, c["dw"], **SUM_TOL)
    check("C", tag + " db", db, c["db"], **SUM_TOL)
    check("C", tag + " dw (second call)", dw2, c["dw"], **SUM_TOL)
    check("C", tag + " db (second call)", db2, c["db"], **SUM_TOL)
    assert torch.equal(bits(dx), bits(dx2))                                   # no atomic touches dx (dw and db are atomic sums: not compared so)
    for k, a in zip(("x", "w", "logits", "prob", "expert", "inv", "dprob", "dxp"), args):
        assert torch.equal(a.cpu(), c[k]), f"{k} was written"


# ---- D ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("experts,mode,gated,bias", LAYER_CASES)
def test_switch_mlp_with_more_than_8_experts_forward_and_all_gradients(experts, mode, gated, bias):
    from dimsum_amd.ops import switch_mlp_torch
    m, x, dout = layer_case(experts, mode, gated, bias)
    args = switch_args(m)
    xr = x.double().requires_grad_()
    want, e = switch_mlp_torch(xr, *args, routing_mode=mode, gated=gated)
    want.backward(dout.double())
    gap = route_oracle(x.reshape(-1, LAYER_DIM), m.router.weight.detach(), m.router.bias.detach(), "sigmoid" if mode == "sinkhorn" else "softmax")[3]
    assert gap >= MIN_GAP, f"precondition: smallest best / second-best gap {gap:.3e}"
    want_grads = named_grads(m, args)
    m = m.cuda()
    xg = x.cuda().requires_grad_()
    out = m(xg)
    out.backward(dout.cuda())
    tag = f"{experts} experts {mode} {'gated' if gated else 'plain'}"
    check("D", tag + " out", out, want, **Y_TOL)
    check("D", tag + " dx", xg.grad, xr.grad, **G_TOL)
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        check("D", f"{tag} {k}", p.grad, want_grads[k], **SUM_TOL)


@pytest.mark.parametrize("experts,mode,gated,bias", LAYER_CASES)
def test_grouped_layer_with_more_than_8_experts_against_the_ungrouped_forward(experts, mode, gated, bias):
    m, x, _ = layer_case(experts, mode, gated, bias)
    bound, _ = layer_bound(m, x, gated)
    m = m.cuda()
    xg = x.cuda()
    with torch.no_grad():
        plain = m(xg)
        m.set_grouped(True)
        grouped = m(xg)
    err = (grouped.double() - plain.double()).abs().cpu()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    WORST["D grouped"] = max(WORST.get("D grouped", 0.0), worst)
    print(f"[D grouped] {experts} experts {mode} {'gated' if gated else 'plain'}: max |grouped - ungrouped| / bound = {worst:.4f}, "
          f"max |diff| = {err.max().item():.3e} (so far: {WORST['D grouped']:.4f})")
    assert (err <= bound).all(), f"max |grouped - ungrouped| / bound = {worst:.3f}"
    assert not torch.equal(grouped, plain)                      # (another kernel did run)
