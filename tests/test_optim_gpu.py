"""dimsum_amd.optim.FusedAdamWEMA (clip -> AdamW -> EMA on the library's two launches) against a float64 restatement of the formulas.

The bound, per tensor and for each of p, exp_avg, exp_avg_sq, ema:   max|fused - ref64| <= 2 max|torch32 - ref64| + ulp32(max|ref64|)
where torch32 is torch's own unfused fp32 path (clip_grad_norm_ / AdamW with foreach=False, mul_ / add_ for the EMA) fed the same inputs: the
yardstick is torch's fp32 arithmetic, the factor 2 covers a different but legitimate operation order (FMA contraction, b1 m + (1 - b1) g
against lerp), the ulp term covers tensors where torch lands exactly. Every element is compared.
The returned norm: relative error against float64 <= max(4 x that of fp32 clip_grad_norm_(foreach=False), 1e-6)."""
import copy
import math

import numpy as np
import pytest
import torch

from procedural import procedural_fill, seeded

pytestmark = pytest.mark.gpu
T = torch.from_numpy

LR, B1, B2, EPS, MAXN, DECAY = 1e-4, 0.9, 0.999, 1e-8, 2.0, 0.9999
SIZES = [1, 3, 5, 1023, 4096, 65543, 777, 300]      # [6]: its gradient is a view at a 4-byte (not 16-byte) aligned address; [7]: no gradient
VIEW, NOGRAD = 6, 7


class Bag(torch.nn.Module):
    def __init__(self, tensors, requires_grad=True):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(t, requires_grad=requires_grad) for t in tensors])


def _inputs(steps, sizes=SIZES, nograd=(NOGRAD,), seed=1):
    g0 = torch.Generator().manual_seed(seed)
    p0 = [torch.randn(n, generator=g0) for n in sizes]
    grads = [[None if i in nograd else torch.randn(n, generator=g0) * 3 for i, n in enumerate(sizes)] for _ in range(steps)]
    return p0, grads


def _norm64(gs):
    return math.sqrt(sum(float((g.double() ** 2).sum()) for g in gs if g is not None))


def ref64(p0, grads, wd=0.0, max_norm=MAXN, decay=DECAY, lr=LR):
    """the formulas of the fused step, in float64 on the CPU -> p, m, v, ema, norms"""
    ps, es = [p.double().clone() for p in p0], [p.double().clone() for p in p0]
    ms, vs, ts = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps], [0] * len(ps)
    norms = []
    for gs in grads:
        nrm = _norm64(gs)
        norms.append(nrm)
        c = 1.0 if max_norm is None else min(1.0, max_norm / (nrm + 1e-6))
        for i, (p, e, m, v, g) in enumerate(zip(ps, es, ms, vs, gs)):
            if g is not None:
                ts[i] += 1
                g = g.double() * c
                p.mul_(1 - lr * wd)
                m.mul_(B1).add_(g, alpha=1 - B1)
                v.mul_(B2).add_(g * g, alpha=1 - B2)
                p.sub_((lr / (1 - B1 ** ts[i])) * m / (v.sqrt() / math.sqrt(1 - B2 ** ts[i]) + EPS))
            if decay is not None:
                e.mul_(decay).add_(p, alpha=1 - decay)
    return ps, ms, vs, es, norms


def torch_path(p0, grads, dtype, wd=0.0, max_norm=MAXN, decay=DECAY, device="cpu", lr=LR):
    """torch's own tail, unfused (foreach=False): clip_grad_norm_ -> AdamW.step -> ema.mul_(d).add_(p, alpha=1 - d) -> p, m, v, ema, norms"""
    ps = [torch.nn.Parameter(p.to(device=device, dtype=dtype).clone()) for p in p0]
    es = [p.detach().clone() for p in ps]
    opt = torch.optim.AdamW(ps, lr=lr, betas=(B1, B2), eps=EPS, weight_decay=wd, foreach=False)
    norms = []
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = None if g is None else g.to(device=device, dtype=dtype).clone()
        with_g = [p for p in ps if p.grad is not None]
        if max_norm is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_(with_g, max_norm, foreach=False)))
        opt.step()
        if decay is not None:
            with torch.no_grad():
                for e, p in zip(es, ps):
                    e.mul_(decay).add_(p, alpha=1 - decay)
    z = lambda p, k: opt.state[p][k] if p in opt.state and opt.state[p] else torch.zeros_like(p)      # noqa: E731
    return [p.detach() for p in ps], [z(p, "exp_avg") for p in ps], [z(p, "exp_avg_sq") for p in ps], es, norms


GUARD = 12345.0


def _ema_buffer(p0):
    """EMA copies as 16-byte aligned views of ONE buffer with 4 guard floats in front of, between and behind them -> (buffer, views, guard mask)"""
    offs, o = [], 4
    for p in p0:
        offs.append(o)
        o = (o + p.numel() + 3) // 4 * 4 + 4
    buf = torch.full((o,), GUARD, device="cuda")
    mask = torch.ones(o, dtype=torch.bool, device="cuda")
    views = []
    for p, a in zip(p0, offs):
        buf[a:a + p.numel()] = p.cuda()
        mask[a:a + p.numel()] = False
        views.append(buf[a:a + p.numel()])
    return buf, views, mask


def _set_grads(bag, gs):
    """fresh gradient tensors; VIEW's is a view one float into its allocation"""
    for i, (p, g) in enumerate(zip(bag.ps, gs)):
        if g is None:
            p.grad = None
        elif i == VIEW and len(bag.ps) == len(SIZES):
            buf = torch.empty(g.numel() + 1, device="cuda")
            buf[1:].copy_(g)
            p.grad = buf[1:]
            assert p.grad.data_ptr() % 16 == 4 and p.grad.is_contiguous()
        else:
            p.grad = g.cuda() if not g.is_cuda else g.clone()


def fused_path(p0, grads, wd=0.0, max_norm=MAXN, decay=DECAY, attach=True, plain_step=False):
    from dimsum_amd.optim import FusedAdamWEMA
    bag = Bag([p.cuda() for p in p0])
    buf, views, mask = _ema_buffer(p0)
    ema = Bag(views, requires_grad=False)
    opt = FusedAdamWEMA(bag.parameters(), lr=LR, betas=(B1, B2), eps=EPS, weight_decay=wd)
    if attach:
        opt.attach_ema(bag, ema)
    norms = []
    for gs in grads:
        _set_grads(bag, gs)
        if plain_step:
            opt.step()
        else:
            n = opt.step_fused(max_norm, decay)
            assert n.is_cuda and n.dim() == 0 and n.dtype == torch.float32
            norms.append(n)
    state = lambda p, k: opt.state[p][k] if opt.state.get(p) else torch.zeros_like(p)      # noqa: E731
    out = ([p.detach().cpu() for p in bag.ps], [state(p, "exp_avg").cpu() for p in bag.ps], [state(p, "exp_avg_sq").cpu() for p in bag.ps],
           [e.detach().cpu() for e in ema.ps], [float(n) for n in norms])
    assert bool((buf[mask] == GUARD).all()), "a guard float next to an EMA tensor was overwritten"
    return out, opt, bag, (buf, views)


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def check_bound(got, t32, ref, what, names=("p", "exp_avg", "exp_avg_sq", "ema")):
    """every element of every tensor; prints each figure before it asserts"""
    bad = []
    for name, G, S, R in zip(names, got, t32, ref):
        for i, (g, s, r) in enumerate(zip(G, S, R)):
            err = float((g.double().cpu() - r).abs().max())
            bound = 2 * float((s.double().cpu() - r).abs().max()) + ulp32(float(r.abs().max()))
            print(f"{what} {name}[{i}] n={r.numel()}: fused err {err:.3e} bound {bound:.3e}")
            if not err <= bound:
                bad.append((name, i, err, bound))
    assert not bad, f"{what}: {bad}"


def check_norms(got, t32, ref, what):
    for k, (g, s, r) in enumerate(zip(got, t32, ref)):
        rel, bound = abs(g - r) / r, max(4 * abs(s - r) / r, 1e-6)
        print(f"{what} norm step {k}: fused rel err {rel:.3e} bound {bound:.3e}")
        assert rel <= bound, (what, k, rel, bound)


def test_reference_restatement_agrees_with_torch_in_float64():
    p0, grads = _inputs(5)
    for wd in (0.0, 0.01):
        a, b = ref64(p0, grads, wd), torch_path(p0, grads, torch.float64, wd)
        for A, B in zip(a[:4], b[:4]):
            assert max(float((x - y).abs().max()) for x, y in zip(A, B)) < 1e-14
        assert max(abs(x - y) / x for x, y in zip(a[4], b[4])) < 1e-13        # norm of per-tensor norms against one sum: 1e-14


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_values_over_five_steps(wd):
    p0, grads = _inputs(5)
    ref, t32 = ref64(p0, grads, wd), torch_path(p0, grads, torch.float32, wd)
    assert all(n > 10 * MAXN for n in ref[4])                                # clipping is active
    got, opt, bag, _ = fused_path(p0, grads, wd)
    check_bound(got[:4], t32[:4], ref[:4], f"wd={wd}")
    check_norms(got[4], t32[4], ref[4], f"wd={wd}")
    assert torch.equal(got[0][NOGRAD], p0[NOGRAD]) and len(opt.state.get(bag.ps[NOGRAD], {})) == 0
    assert all(float(opt.state[p]["step"]) == 5.0 for i, p in enumerate(bag.ps) if i != NOGRAD)


def test_norm_with_grid_stride():
    n = 2 ** 24 + 3
    p0, grads = _inputs(1, sizes=[n], nograd=())
    ref_norm = _norm64(grads[0])
    g32 = torch.nn.Parameter(torch.zeros(n))
    g32.grad = grads[0][0].clone()
    t32 = float(torch.nn.utils.clip_grad_norm_([g32], MAXN, foreach=False))
    got, *_ = fused_path(p0, grads)
    check_norms(got[4], [t32], [ref_norm], "2^24+3")
    ref = ref64(p0, grads)
    t = torch_path(p0, grads, torch.float32)
    check_bound(got[:4], t[:4], ref[:4], "2^24+3")


def test_tensor_without_gradient():
    """p bit-identical, no optimizer state, the EMA still blends, and the norm is that of the other tensors"""
    p0, grads = _inputs(3)
    got, opt, bag, (_, views) = fused_path(p0, grads, decay=0.5)
    assert torch.equal(got[0][NOGRAD], p0[NOGRAD])
    assert len(opt.state.get(bag.ps[NOGRAD], {})) == 0 and NOGRAD not in opt.state_dict()["state"]
    ref = ref64(p0, grads, decay=0.5)
    t32 = torch_path(p0, grads, torch.float32, decay=0.5)
    check_bound([[got[3][NOGRAD]]], [[t32[3][NOGRAD]]], [[ref[3][NOGRAD]]], "no-gradient", names=("ema",))
    # the EMA started at p and p never moved: d e + (1 - d) p stays p to rounding
    assert float((got[3][NOGRAD] - p0[NOGRAD]).abs().max()) <= ulp32(float(p0[NOGRAD].abs().max()))
    without = [[g for g in gs if g is not None] for gs in grads]
    p1 = [p for i, p in enumerate(p0) if i != NOGRAD]
    got1, *_ = fused_path(p1, without, decay=0.5)
    t32n = torch_path(p1, without, torch.float32)[4]
    check_norms(got[4], t32n, [_norm64(gs) for gs in without], "no-gradient")
    assert all(abs(a - b) <= 1e-6 * b for a, b in zip(got[4], got1[4]))


def test_no_clip_and_no_ema():
    """max_grad_norm=None and no EMA attached: p, m, v follow the unclipped reference and nothing else is written (the would-be EMA copies and the
    guard floats around them keep their bits); plain step() is the same kernel"""
    p0, grads = _inputs(3)
    ref, t32 = ref64(p0, grads, max_norm=None, decay=None), torch_path(p0, grads, torch.float32, max_norm=None, decay=None)
    for kw in (dict(max_norm=None, decay=None, attach=False), dict(max_norm=None, decay=DECAY, attach=False), dict(plain_step=True),
               dict(plain_step=True, attach=False)):
        got, _, _, (buf, views) = fused_path(p0, grads, **kw)                        # guards checked inside
        check_bound(got[:3], t32[:3], ref[:3], f"no clip {kw}")
        assert all(torch.equal(v.cpu(), p) for v, p in zip(views, p0)), kw
        if not kw.get("plain_step"):
            check_norms(got[4], [_norm64(gs) for gs in grads], [_norm64(gs) for gs in grads], "no clip")     # the norm is still returned


@pytest.mark.parametrize("sizes,nograd", [(SIZES, (NOGRAD,)), ([2 ** 24 + 3], ())])
def test_bit_reproducible(sizes, nograd):
    p0, grads = _inputs(2, sizes=sizes, nograd=nograd)
    a, *_ = fused_path(p0, grads)
    b, *_ = fused_path(p0, grads)
    for A, B in zip(a[:4], b[:4]):
        assert all(torch.equal(x, y) for x, y in zip(A, B))
    assert a[4] == b[4]


def test_fresh_gradient_allocations_without_synchronisation():
    """8 steps back to back; every step's gradients are new tensors, and the previous step's are freed and their memory refilled with
    unrelated values at once: a cached pointer table, or a staging buffer reused too early, reads those values"""
    from dimsum_amd.optim import FusedAdamWEMA
    p0, grads = _inputs(8)
    ref, t32 = ref64(p0, grads), torch_path(p0, grads, torch.float32)
    staged = [[None if g is None else g.cuda() for g in gs] for gs in grads]
    bag = Bag([p.cuda() for p in p0])
    buf, views, mask = _ema_buffer(p0)
    ema = Bag(views, requires_grad=False)
    opt = FusedAdamWEMA(bag.parameters(), lr=LR, betas=(B1, B2), eps=EPS, weight_decay=0.0)
    opt.attach_ema(bag, ema)
    torch.cuda.synchronize()
    norms = []
    for gs in staged:
        _set_grads(bag, gs)
        norms.append(opt.step_fused(MAXN, DECAY))
        opt.zero_grad(set_to_none=True)                                           # frees this step's gradients ...
        junk = [torch.randn(n + (1 if i == VIEW else 0), device="cuda") * 1e3 for i, n in enumerate(SIZES) if i != NOGRAD]   # ... and reuses them
        del junk
    got = ([p.detach().cpu() for p in bag.ps], [opt.state[p]["exp_avg"].cpu() if opt.state.get(p) else torch.zeros_like(p).cpu() for p in bag.ps],
           [opt.state[p]["exp_avg_sq"].cpu() if opt.state.get(p) else torch.zeros_like(p).cpu() for p in bag.ps], [e.detach().cpu() for e in ema.ps])
    check_bound(got, t32[:4], ref[:4], "8 steps")
    check_norms([float(n) for n in norms], t32[4], ref[4], "8 steps")
    assert bool((buf[mask] == GUARD).all())


def _gpu_opt(kind, ps, **kw):
    from dimsum_amd.optim import FusedAdamWEMA
    if kind == "ours":
        return FusedAdamWEMA(ps, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=0.01)
    return torch.optim.AdamW(ps, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=0.01, **kw)


def _steps(opt, ps, grads):
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.cuda()
        if hasattr(opt, "step_fused"):
            opt.step_fused(MAXN, None)
        else:
            torch.nn.utils.clip_grad_norm_(ps, MAXN)
            opt.step()


@pytest.mark.parametrize("first,second,kw", [("torch", "ours", dict(fused=True)), ("ours", "torch", dict(fused=True)),
                                             ("torch", "ours", dict(foreach=False))])
def test_state_dict_interchange(first, second, kw):
    """two steps with one optimizer, its state_dict() loaded into the other kind (fresh parameter objects), one more step there; the third
    case is the reference's non-fused layout, whose "step" entries are CPU tensors"""
    sizes = SIZES[:6]
    p0, grads = _inputs(3, sizes=sizes, nograd=())
    ref, t32 = ref64(p0, grads, wd=0.01, decay=None), torch_path(p0, grads, torch.float32, wd=0.01, decay=None)
    ps = [torch.nn.Parameter(p.cuda()) for p in p0]
    a = _gpu_opt(first, ps, **kw)
    _steps(a, ps, grads[:2])
    sd = a.state_dict()
    if first == "torch" and "foreach" in kw:
        assert all(not s["step"].is_cuda for s in sd["state"].values())
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    b = _gpu_opt(second, qs, **({} if second == "ours" else dict(fused=True)))
    b.load_state_dict(copy.deepcopy(sd))
    sd2 = b.state_dict()
    assert sd.keys() == sd2.keys() and sd["state"].keys() == sd2["state"].keys()
    assert all(sd["state"][k].keys() == sd2["state"][k].keys() for k in sd["state"])
    assert all(g.keys() == h.keys() for g, h in zip(sd["param_groups"], sd2["param_groups"]))
    fresh = _gpu_opt("torch", [torch.nn.Parameter(torch.zeros(1, device="cuda"))], fused=True).state_dict()
    assert all(g.keys() == fresh["param_groups"][0].keys() for g in sd2["param_groups"])
    assert all(float(s["step"]) == 2.0 for s in sd2["state"].values())
    for g in b.param_groups:                                                     # load_checkpoint's lr override goes through param_groups
        assert g["lr"] == LR
    _steps(b, qs, grads[2:])
    got = ([q.detach().cpu() for q in qs], [b.state[q]["exp_avg"].cpu() for q in qs], [b.state[q]["exp_avg_sq"].cpu() for q in qs])
    check_bound(got, t32[:3], ref[:3], f"{first}->{second} {kw}")
    assert all(float(b.state[q]["step"]) == 3.0 for q in qs)


def test_lr_is_read_from_param_groups_every_step():
    p0, grads = _inputs(2, sizes=SIZES[:6], nograd=())
    ps = [torch.nn.Parameter(p.cuda()) for p in p0]
    opt = _gpu_opt("ours", ps)
    _steps(opt, ps, grads[:1])
    before = [p.detach().clone() for p in ps]
    for g in opt.param_groups:
        g["lr"] = 0.0
        g["weight_decay"] = 0.0
    _steps(opt, ps, grads[1:])
    assert all(torch.equal(a, b) for a, b in zip(before, ps))


KW = dict(img_resolution=32, in_channels=4, label_dropout=0.0, num_classes=1000, learn_sigma=False, scan_type="none", pe_type="ape",
          block_type="combined", cond_mamba=True, scanning_continuity=False, drop_path=0.0, rms_norm=True, fused_add_norm=True,
          learnable_pe=True, use_final_norm=False, use_attn_every_k_layers=4, use_gated_mlp=True)


def _model():
    from dimsum_amd.models_dim import DiM
    m = DiM(depth=4, hidden_size=64, patch_size=2, **KW)
    procedural_fill(m, seed=3)
    return m


def _batch():
    from dimsum_amd.transport import create_transport
    x, y = T(seeded((4, 4, 32, 32), 81)).cuda(), torch.tensor([1, 22, 333, 999], device="cuda")
    tr = create_transport("GVP", "velocity")
    t, x0 = T(seeded((4,), 82, kind="uniform")), T(seeded((4, 4, 32, 32), 83))
    tr.sample = lambda x1: (t.to(x1), x0.to(x1), x1)
    return tr, x, y


@pytest.mark.usefixtures("allow_torch_sdpa")      # hidden 64: head_dim 4 (conftest)
def test_train_step_runs_the_fused_tail():
    """one train_step with build_training(fused_step=True) against the three torch operations applied to deep copies from the SAME gradients
    (one step on purpose: Adam's first update is ~ -lr sign(g), two runs whose gradients differ in the last bit diverge legitimately)"""
    from dimsum_amd.optim import FusedAdamWEMA
    from dimsum_amd.train import build_training, train_step, update_ema
    torch.backends.cuda.matmul.allow_tf32 = False
    lr, decay = 1e-4, 0.5
    model, ema, opt = build_training(_model().cuda(), "cuda", lr=lr, fused_step=True)
    assert isinstance(opt, FusedAdamWEMA)
    model2, ema2 = copy.deepcopy(model), copy.deepcopy(ema)
    start = {k: v.detach().clone() for k, v in model.named_parameters()}
    captured, orig = {}, opt.step_fused

    def spy(max_grad_norm, ema_decay):
        captured.update({k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()})
        captured["norm"] = orig(max_grad_norm, ema_decay)
        return captured["norm"]

    opt.step_fused = spy
    tr, x, y = _batch()
    loss = train_step(model.train(), ema, opt, tr, x, y, max_grad_norm=2.0, ema_decay=decay)
    assert math.isfinite(loss.item()) and "norm" in captured
    names = [k for k, _ in model.named_parameters()]
    dead = [k for k in names if captured[k] is None]
    assert any("cond_proj" in k for k in dead) and len(dead) < len(names) // 2
    for k, p in model.named_parameters():
        if captured[k] is None:
            assert p.grad is None and torch.equal(p, start[k]) and len(opt.state.get(p, {})) == 0, k      # cond_proj: untouched
        else:
            assert torch.equal(p.grad, captured[k]), k                                      # .grad keeps the unclipped gradient
    # the parent's tail on the copies
    opt2 = torch.optim.AdamW(model2.parameters(), lr=lr, weight_decay=0, fused=True)
    for k, p in model2.named_parameters():
        p.grad = None if captured[k] is None else captured[k].clone()
    norm2 = torch.nn.utils.clip_grad_norm_(model2.parameters(), 2.0)
    opt2.step()
    update_ema(ema2, model2, decay)
    # float64 restatement from the same gradients
    p0 = [start[k].cpu() for k in names]
    ref = ref64(p0, [[None if captured[k] is None else captured[k].cpu() for k in names]], max_norm=2.0, decay=decay, lr=lr)
    t32 = ([dict(model2.named_parameters())[k].detach() for k in names], None, None, [dict(ema2.named_parameters())[k].detach() for k in names])
    got = ([dict(model.named_parameters())[k].detach() for k in names], None, None, [dict(ema.named_parameters())[k].detach() for k in names])
    check_bound((got[0], got[3]), (t32[0], t32[3]), (ref[0], ref[3]), "train_step", names=("p", "ema"))
    check_norms([float(captured["norm"])], [float(norm2)], ref[4], "train_step")


@pytest.mark.usefixtures("allow_torch_sdpa")
def test_default_path_is_unchanged(monkeypatch):
    """DIMSUM_FUSED_STEP unset: torch's AdamW, and train_step equals clip_grad_norm_ -> step -> update_ema by hand, bit for bit"""
    from dimsum_amd import train
    monkeypatch.delenv("DIMSUM_FUSED_STEP", raising=False)
    torch.backends.cuda.matmul.allow_tf32 = False
    lr, decay = 1e-4, 0.5
    model, ema, opt = train.build_training(_model().cuda(), "cuda", lr=lr)
    assert type(opt) is torch.optim.AdamW and opt.param_groups[0]["fused"] is True
    model2, ema2 = copy.deepcopy(model), copy.deepcopy(ema)
    captured, clip = {}, torch.nn.utils.clip_grad_norm_

    def spy(params, max_norm, *a, **k):
        captured.update({n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()})
        return clip(params, max_norm, *a, **k)

    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", spy)
    tr, x, y = _batch()
    train.train_step(model.train(), ema, opt, tr, x, y, max_grad_norm=2.0, ema_decay=decay)
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", clip)
    assert captured
    opt2 = torch.optim.AdamW(model2.parameters(), lr=lr, weight_decay=0, fused=True)
    for n, p in model2.named_parameters():
        p.grad = None if captured[n] is None else captured[n].clone()
    torch.nn.utils.clip_grad_norm_(model2.parameters(), 2.0)
    opt2.step()
    train.update_ema(ema2, model2, decay)
    for (n, a), (_, b) in zip(model.named_parameters(), model2.named_parameters()):
        assert torch.equal(a, b), n
        assert (a.grad is None and b.grad is None) or torch.equal(a.grad, b.grad), n       # clipped in place, as before
    for (n, a), (_, b) in zip(ema.named_parameters(), ema2.named_parameters()):
        assert torch.equal(a, b), n
