"""Training on the grouped expert GEMM, on the GPU: the two gradient kernels (csrc/moe_gemm_bwd.hip) against float64 slice products on hand-made
offset tables (routing is not a variable), the SwitchMLP that trains on them against the float64 restatement with every synchronising tensor method
patched to raise, and one training step of an is_moe model with and without `set_grouped_train`.

Bounds.
 * the kernels: an fp32 value v is staged as hi = bf16(v), lo = bf16(v - hi). bf16 keeps 8 significant bits: |v - hi| <= 2^-8 |v|, and the
   remainder, below 2^-8 of v's binade, is rounded with a spacing of 2^-16 of it: |v - hi - lo| <= 2^-17 |v|. Of (a_hi + a_lo)(b_hi + b_lo) the
   kernels drop a_lo b_lo <= 2^-16 |a b|, and the two residuals never enter: 2^-17 |a b| each. One product is therefore within 2^-15 |a b| of the
   exact one -- a worst case that a reduction over ONE row (an expert with one token, in the tables below) has no other terms to average out, which
   is why the forward's constant 4 * 2^-18 (tests/test_moe_grouped_gpu.py: sums over K >= 32) is not used here. The rest is fp32 accumulation of
   R terms, R the reduction length (dgrad: N; wgrad: the expert's row count). With S = sum |a| |b| in float64:
       |got - exact| <= (2^-15 + (R + 3) 2^-24) S     elementwise (the 3 covers the second-order terms).
   An empty range has S = 0: its dW must be exactly zero. db is a plain fp32 sum of R terms: (R + 3) 2^-24 sum |dy|.
 * the layer: per compared gradient, the maximum error of the path that trains on the slice GEMMs (_SwitchMlpFn, the path every MoE test before
   this file checks) against float64 on the same inputs is measured first; the grouped path passes if its own maximum error is at most 4 x that,
   with a floor of 1e-6 max|ref|. Both run under torch.backends.cuda.matmul.allow_tf32 = True: train.py's default and the reference's policy, under
   which the library forms an fp32 product from the same three bf16 products as the kernels here (the error of the slice path with allow_tf32 off
   is printed next to it, not asserted on).
 * the model: there is no float64 model to measure either path against, so the two steps are compared with each other at the tolerances the suite
   holds the slice path's model to against its CPU restatement: loss rtol 1e-4 (test_train_gpu), parameters after a plain SGD step of size 1 -- the
   clipped gradients -- at SUM_TOL (test_moe_gpu)."""
import numpy as np
import pytest
import torch

from conftest import assert_close
from procedural import procedural_fill, seeded
from test_blocks_linear_window_gpu import SUM_TOL
from test_moe_cpu import CASES, make_switch, named_grads, switch_args, tiny_inputs, _tiny
from test_moe_gpu import MIN_GAP, MODULE_SEEDS, route_oracle
from test_moe_grouped_cpu import no_host_reads
from test_moe_grouped_gpu import SENTINEL, U
from test_train_gpu import _fixed_transport

pytestmark = pytest.mark.gpu
T = torch.from_numpy

def eps_grouped(R):
    return 2.0 ** -15 + (R + 3) * U


MANY = [0] * 64
MANY[3], MANY[20], MANY[41], MANY[63] = 7, 1, 31, 1
TABLES = {
    "ranges": [0, 0, 1, 66, 200],                       # an empty first expert, 1 row, 65 rows across a 64-row tile, 134 rows
    "one_holds_all": [0, 0, 0, 200, 200],
    "one_expert": [0, 70],
    "64_mostly_empty": [0] + list(np.cumsum(MANY)),     # 40 rows
    "tails": [0, 31, 63, 96, 161],                      # wgrad's last 32-row step: 31, 32, 33 and 65 rows
}
WIDTHS = [(32, 32), (160, 96), (128, 32), (96, 160)]    # (N, K): below one column tile, a ragged last column tile, an exact tile, two k tiles


def _operands(table, N, K, seed):
    off = np.asarray(TABLES[table] if isinstance(table, str) else table, np.int32)
    E, rows = len(off) - 1, int(off[-1])
    dy, x = T(seeded((rows, N), seed)), T(seeded((rows, K), seed + 1))
    w = T(seeded((E, N, K), seed + 2, scale=N ** -0.5))
    return off, E, rows, dy, x, w


def _exact(off, dy, x, w):
    """float64, slice by slice -> (dx, its bound, dW (E, N, K), its bound, db (E, N), its bound)"""
    E, (N, K) = len(off) - 1, w.shape[1:]
    dx, bdx = torch.zeros(dy.shape[0], K, dtype=torch.float64), torch.zeros(dy.shape[0], K, dtype=torch.float64)
    dw, bdw = torch.zeros(E, N, K, dtype=torch.float64), torch.zeros(E, N, K, dtype=torch.float64)
    db, bdb = torch.zeros(E, N, dtype=torch.float64), torch.zeros(E, N, dtype=torch.float64)
    for e in range(E):
        o0, o1 = int(off[e]), int(off[e + 1])
        a, b, m = dy[o0:o1].double(), x[o0:o1].double(), w[e].double()
        dx[o0:o1], bdx[o0:o1] = a @ m, eps_grouped(N) * (a.abs() @ m.abs())
        dw[e], bdw[e] = a.t() @ b, eps_grouped(o1 - o0) * (a.abs().t() @ b.abs())
        db[e], bdb[e] = a.sum(0), (o1 - o0 + 3) * U * a.abs().sum(0)
    return dx, bdx, dw, bdw, db, bdb


def _within(got, exact, bound, what):
    err = (got.double().cpu() - exact).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    print(f"{what}: max |err| / bound = {worst:.3f}, max |err| = {err.max().item() if err.numel() else 0.0:.3e}")
    assert (err <= bound).all(), f"{what}: max |err| / bound = {worst:.3f}"


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("N,K", WIDTHS)
@pytest.mark.parametrize("table", list(TABLES))
def test_kernels_against_float64(table, N, K):
    from dimsum_amd import native
    off, E, rows, dy, x, w = _operands(table, N, K, 900 + 10 * list(TABLES).index(table) + WIDTHS.index((N, K)))
    dx, bdx, dw, bdw, db, bdb = _exact(off, dy, x, w)
    ws = [w[e].cuda().contiguous() for e in range(E)]
    dyg, xg, offg = dy.cuda(), x.cuda(), T(off).cuda()
    # dgrad into a view with guard rows and guard columns
    guard, ldc = 3, K + 12
    buf = torch.full((guard + rows + guard, ldc), SENTINEL, device="cuda")
    out = buf[guard:guard + rows, :K]
    got = native.moe_gemm_dgrad(dyg, offg, ws, out=out)
    assert got.data_ptr() == out.data_ptr()
    _within(got, dx, bdx, f"dgrad {table} {N}x{K}")                   # (a row left unwritten holds the sentinel: far outside)
    image = buf.cpu()
    keep = torch.full_like(image, SENTINEL)
    keep[guard:guard + rows, :K] = image[guard:guard + rows, :K]
    assert _same_bits(image, keep), "dgrad: a guard row or guard column was written"
    assert _same_bits(native.moe_gemm_dgrad(dyg, offg, ws), got), "dgrad: two calls differ"
    # wgrad with the bias gradient
    gw, gb = native.moe_gemm_wgrad(dyg, xg, offg, E, need_dbias=True)
    assert len(gw) == E and all(g.shape == (N, K) and g.is_contiguous() for g in gw) and gb.shape == (E, N)
    _within(torch.stack(gw), dw, bdw, f"wgrad {table} {N}x{K}")
    _within(gb, db, bdb, f"dbias {table} {N}x{K}")
    for e in range(E):
        if off[e + 1] == off[e]:                                      # an expert without rows: zeros stored by the kernel, exactly
            assert torch.count_nonzero(gw[e]) == 0 and torch.count_nonzero(gb[e]) == 0, e
    gw2, gb2 = native.moe_gemm_wgrad(dyg, xg, offg, E, need_dbias=True)
    assert all(_same_bits(a, b) for a, b in zip(gw, gw2)) and _same_bits(gb, gb2), "wgrad: two calls differ"
    gw3, none = native.moe_gemm_wgrad(dyg, xg, offg, E)
    assert none is None and all(_same_bits(a, b) for a, b in zip(gw, gw3)), "wgrad: the bias gradient changes the weight gradient"


def test_the_tables_cover_what_they_claim():
    counts = {k: list(np.diff(v)) for k, v in TABLES.items()}
    assert counts["ranges"] == [0, 1, 65, 134] and counts["one_holds_all"] == [0, 0, 200, 0] and counts["one_expert"] == [70]
    assert len(counts["64_mostly_empty"]) == 64 and sum(counts["64_mostly_empty"]) == 40 and sum(c == 0 for c in counts["64_mostly_empty"]) == 60
    assert counts["tails"] == [31, 32, 33, 65]
    assert {n for n, _ in WIDTHS} >= {32, 160, 128} and {k for _, k in WIDTHS} >= {32, 96, 160}


# a table the clamping rule makes well defined (entries clamped to [0, T], a range starts no earlier than the last non-empty one ended), and the
# well-formed table it must behave as
MALFORMED = [([-7, 40, 30, 250], [0, 40, 40, 100]),     # negative, decreasing, above T
             ([5, 40, 12, 90], [5, 40, 40, 90]),        # decreasing; rows [0, 5) and [90, 100) belong to nobody
             ([120, 100, 60, 60], [100, 100, 100, 100])]    # nothing is left of any range


@pytest.mark.parametrize("case", range(len(MALFORMED)))
def test_a_malformed_table_is_clamped_and_cut_like_the_forwards(case):
    from dimsum_amd import native
    bad, good = MALFORMED[case]
    rows, N, K, E = 100, 64, 96, 3
    dy, x = T(seeded((rows, N), 990)).cuda(), T(seeded((rows, K), 991)).cuda()
    w = T(seeded((E, N, K), 992, scale=N ** -0.5))
    ws = [w[e].cuda().contiguous() for e in range(E)]
    tab = lambda t: torch.tensor(t, dtype=torch.int32, device="cuda")      # noqa: E731
    got = native.moe_gemm_dgrad(dy, tab(bad), ws, out=torch.full((rows, K), SENTINEL, device="cuda"))
    want = native.moe_gemm_dgrad(dy, tab(good), ws, out=torch.full((rows, K), SENTINEL, device="cuda"))
    assert _same_bits(got, want)
    inside = torch.zeros(rows, dtype=torch.bool)
    for e in range(E):
        inside[good[e]:good[e + 1]] = True
    assert (got.cpu()[~inside] == SENTINEL).all() and (got.cpu()[inside] != SENTINEL).all()      # rows outside every range keep what they held
    off = np.asarray(good, np.int32)
    dx, bdx, dw, bdw, db, bdb = _exact(off, dy.cpu(), x.cpu(), w)
    _within(got.cpu()[inside], dx[inside], bdx[inside], "dgrad")
    gw, gb = native.moe_gemm_wgrad(dy, x, tab(bad), E, need_dbias=True)
    ww, wb = native.moe_gemm_wgrad(dy, x, tab(good), E, need_dbias=True)
    assert all(_same_bits(a, b) for a, b in zip(gw, ww)) and _same_bits(gb, wb)
    _within(torch.stack(gw), dw, bdw, "wgrad")
    _within(gb, db, bdb, "dbias")


def test_a_call_without_rows_launches_nothing():
    from dimsum_amd import native
    ws = [torch.randn(64, 32, device="cuda") for _ in range(3)]
    zero = torch.zeros(4, dtype=torch.int32, device="cuda")
    assert native.moe_gemm_dgrad(torch.empty(0, 64, device="cuda"), zero, ws).shape == (0, 32)
    gw, gb = native.moe_gemm_wgrad(torch.empty(0, 64, device="cuda"), torch.empty(0, 32, device="cuda"), zero, 3, need_dbias=True)
    assert len(gw) == 3 and all(g.shape == (64, 32) and torch.count_nonzero(g) == 0 for g in gw) and gb.shape == (3, 64) and torch.count_nonzero(gb) == 0


# ---- the layer -------------------------------------------------------------------------------------------------------------------------------------
def _layer_grads(m, x, dout, patched):
    import contextlib
    m.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_()
    with (no_host_reads() if patched else contextlib.nullcontext()):
        out = m(xg)
        out.backward(dout)
    return out.detach(), dict({"x": xg.grad}, **{k: p.grad for k, p in m.named_parameters()})


@pytest.mark.parametrize("mode,gated,bias", CASES)
def test_the_layer_trains_on_the_grouped_gemm_without_a_host_read(mode, gated, bias):
    from dimsum_amd.ops import switch_mlp_torch
    dim, shape = 32, (2, 24)
    m = make_switch(mode, gated, bias, 40 + CASES.index((mode, gated, bias)) % 4, dim=dim)
    x, dout = T(seeded(shape + (dim,), MODULE_SEEDS[(dim, 48)])), T(seeded(shape + (dim,), 502))
    args = switch_args(m)
    xr = x.double().requires_grad_()
    want, _ = switch_mlp_torch(xr, *args, routing_mode=mode, gated=gated)
    want.backward(dout.double())
    gap = route_oracle(x.reshape(-1, dim), m.router.weight.detach(), m.router.bias.detach(), "sigmoid" if mode == "sinkhorn" else "softmax")[3]
    assert gap >= MIN_GAP, f"precondition: smallest best / second-best gap {gap:.3e}"
    ref = dict(named_grads(m, args), x=xr.grad)
    m = m.cuda()
    xg, dg = x.cuda(), dout.cuda()
    torch.backends.cuda.matmul.allow_tf32 = False
    _, exact_fp32 = _layer_grads(m, xg, dg, False)
    torch.backends.cuda.matmul.allow_tf32 = True                      # train.py's default: the setting both compared paths run under
    _, slices = _layer_grads(m, xg, dg, False)
    m.set_grouped_train(True)
    out, grouped = _layer_grads(m, xg, dg, True)                      # forward and backward with tolist / item / cpu patched to raise
    with torch.no_grad():
        m.set_grouped(True)
        assert torch.equal(m(xg), out), "the forward is not the grouped inference forward bit for bit"
    assert set(grouped) == set(ref) and all(g is not None for g in grouped.values())
    failures = []
    for k, r in ref.items():
        err = lambda g: (g.double().cpu().reshape(r.shape) - r).abs().max().item()      # noqa: E731
        e_g, e_s, e_f, floor = err(grouped[k]), err(slices[k]), err(exact_fp32[k]), 1e-6 * r.abs().max().item()
        line = f"{k}: grouped {e_g:.3e}, slices {e_s:.3e} (allow_tf32 off: {e_f:.3e}), floor {floor:.3e}"
        print(line)
        if not e_g <= max(4 * e_s, floor):
            failures.append(line)
    assert not failures, "\n".join(failures)


def test_an_expert_without_tokens_gets_exact_zeros():
    m = make_switch("top1", True, True, 3)
    with torch.no_grad():
        m.router.bias[1] = -1e4
    m = m.cuda()
    m.set_grouped_train(True)
    x = T(seeded((2, 24, 32), 9)).cuda().requires_grad_()
    with no_host_reads():
        m(x).square().sum().backward()
    assert all(p.grad is not None and torch.count_nonzero(p.grad) == 0 for p in m.local_experts[1].parameters())
    assert all(torch.count_nonzero(p.grad) > 0 for p in m.local_experts[0].parameters())


# ---- the model -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.usefixtures("allow_torch_sdpa")
def test_one_training_step_of_an_is_moe_model_with_and_without_grouped_train():
    """use_final_norm: the configuration in which every router's gradient is more than roundoff (test_moe_gpu's model test says why)"""
    import copy
    from dimsum_amd import switch_mlp
    from dimsum_amd.train import train_step
    torch.backends.cuda.matmul.allow_tf32 = True
    x, t, y = tiny_inputs()
    tr = _fixed_transport(t, T(seeded((2, 4, 8, 8), 83)))
    base = procedural_fill(_tiny(use_final_norm=True), seed=5).cuda()
    runs = {}
    for on in (False, True):
        torch.manual_seed(0)
        model = copy.deepcopy(base).train()
        assert switch_mlp.set_grouped_train(model, on) == 2
        ema = copy.deepcopy(model).requires_grad_(False)
        loss = train_step(model, ema, torch.optim.SGD(model.parameters(), lr=1.0), tr, x.cuda(), y.cuda(), max_grad_norm=2.0, ema_decay=0.5)
        runs[on] = (loss.item(), {k: v.detach().cpu().numpy() for k, v in model.named_parameters()})
    (loss_s, par_s), (loss_g, par_g) = runs[False], runs[True]
    print(f"loss: slices {loss_s!r}, grouped {loss_g!r}")
    assert abs(loss_g - loss_s) <= 1e-4 * abs(loss_s)
    n0 = {k: v.detach().cpu().numpy() for k, v in base.named_parameters()}
    moved = 0
    for k in par_s:
        step_s, step_g = par_s[k] - n0[k], par_g[k] - n0[k]
        assert_close(step_g, step_s, what=k, **SUM_TOL)
        moved += bool(np.abs(step_s).max() > 0)
    assert moved > 40 and np.abs(par_s["blocks.1.mixer.local_experts.0.linear_fc1.weight"] - n0["blocks.1.mixer.local_experts.0.linear_fc1.weight"]).max() > 0
