"""GPU parity of the general selective scan (csrc/ssm_scan_general.hip) through selective_scan_fn / native / the Mamba modules, against the
float64 / complex128 restatement of the operator (scan_general_ref.py, pinned to the reference by test_scan_general_cpu.py) on the same
rounded inputs. Tolerances are test_scan_gpu.py's, unchanged: tol(L) for the forward, _bwd_tol(L) / _bwd_tol(L, True) for the gradients
(mamba/tests/ops/test_selective_scan.py:49-54,158-172), the reference's per-dtype rtol / atol for 16-bit I/O.
The backward adds dA, dB, dC, dD and ddelta_bias with fp32 atomics: two launches agree within tolerance, not bit
for bit; the forward and du / ddelta / dz are sums in a fixed order and must be bit-equal."""
import numpy as np
import pytest
import torch

from conftest import assert_close
from scan_general_ref import make_case, scan_restated
from test_scan_gpu import _bwd_tol, tol

pytestmark = pytest.mark.gpu

_REF = {}


def _case(key, softplus=True, **kw):
    if key not in _REF:
        c = make_case(**kw)
        res, out, last, ends = scan_restated(c["u"], c["delta"], c["A"], c["B"], c["C"], c["D"], c["z"], c["delta_bias"], softplus)
        res.backward(c["dout"])
        _REF[key] = (c, dict(res=res.detach(), out=out.detach(), last=last.detach(), ends=ends.detach()))
    return _REF[key]


def _gpu_leaves(c, dtype=torch.float32):
    """the case's operands on the GPU in the kernels' dtypes (I/O `dtype`, weights float32 / complex64) as leaves"""
    out = {}
    for k, v in c.items():
        if v is None:
            out[k] = None
            continue
        weight = k in ("A", "D", "delta_bias") or (k in ("B", "C") and v.dim() == 2)
        t = v.detach().to(torch.complex64 if v.is_complex() else (torch.float32 if weight else dtype)).cuda()
        out[k] = t.requires_grad_() if k != "dout" else t
    return out


def _np(t):
    t = t.detach().cpu()
    if t.is_complex():
        return torch.view_as_real(t.to(torch.complex128)).numpy()
    return t.double().numpy()


def _check_all(c, ref, g, res, last, L, fwd_tol, grad_tol, wgrad_tol):
    assert_close(_np(res), _np(ref["res"]), what="out", **fwd_tol)
    if last is not None:
        assert_close(_np(last), _np(ref["last"]), what="last_state", **fwd_tol)
    for k in ("u", "delta", "z"):
        if c[k] is not None:
            assert_close(_np(g[k].grad), _np(c[k].grad), what="d" + k, **grad_tol)
    for k in ("B", "C"):
        assert g[k].grad.dtype == g[k].dtype and g[k].grad.shape == g[k].shape
        assert_close(_np(g[k].grad), _np(c[k].grad), what="d" + k, **(grad_tol if c[k].dim() == 4 else wgrad_tol))
    for k in ("A", "D", "delta_bias"):
        if c[k] is not None:
            assert_close(_np(g[k].grad), _np(c[k].grad), what="d" + k, **wgrad_tol)


def _run_fn(g, softplus=True):
    from dimsum_amd.ops import selective_scan_fn
    res, last = selective_scan_fn(g["u"], g["delta"], g["A"], g["B"], g["C"], g["D"], g["z"], g["delta_bias"], delta_softplus=softplus,
                                  return_last_state=True)
    res.backward(g["dout"])
    torch.cuda.synchronize()
    return res, last


COMBOS = [(cplx, vB, vC) for cplx in (False, True) for vB in (True, False) for vC in (True, False)]


# complex: the list of state sizes thinned to an odd value, a partial block, the largest 4-wave workgroup and 256
ODD_CASES = [(cplx, vB, vC, N) for cplx, vB, vC in COMBOS for N in ((3, 12, 64, 256) if cplx else (1, 3, 12, 20, 64, 256))]


@pytest.mark.parametrize("cplx,vB,vC,N", ODD_CASES)
def test_fn_masked_lanes_odd_length(cplx, vB, vC, N):
    """(2, 72, 37): lanes 8..63 of the second channel block masked, a partial last tile; every weight / B / C combination, every state-block
    count incl. a partial one (complex thinned to an odd value, 12, 64 and 256)"""
    L = 37
    c, ref = _case(("odd", cplx, vB, vC, N), batch=2, dim=72, L=L, N=N, cplx=cplx, var_B=vB, var_C=vC, seed=N)
    g = _gpu_leaves(c)
    res, last = _run_fn(g)
    _check_all(c, ref, g, res, last, L, tol(L), _bwd_tol(L), _bwd_tol(L, True))


@pytest.mark.parametrize("cplx,vB,vC,N,has_z,has_D,has_bias,sp", [(False, True, True, 12, False, False, False, False), (False, True, False, 64, True, False, True, False),
                                                                 (True, True, True, 12, False, True, False, True), (True, False, True, 3, True, False, False, False),
                                                                 (False, True, True, 64, True, True, True, True), (True, True, True, 64, True, True, True, True)])
def test_fn_two_groups_and_optional_operands(cplx, vB, vC, N, has_z, has_D, has_bias, sp):
    """(2, 128, 64) with n_groups = 2 (one 64-channel block per group), with and without z / D / delta_bias / softplus"""
    L = 64
    c, ref = _case(("grp", cplx, vB, vC, N, has_z, has_D, has_bias, sp), softplus=sp, batch=2, dim=128, L=L, N=N, cplx=cplx, var_B=vB, var_C=vC, groups=2,
                   has_D=has_D, has_z=has_z, has_bias=has_bias, seed=7)
    g = _gpu_leaves(c)
    res, last = _run_fn(g, sp)
    _check_all(c, ref, g, res, last, L, tol(L), _bwd_tol(L), _bwd_tol(L, True))


@pytest.mark.parametrize("cplx", [False, True])
def test_two_chunks(cplx):
    """L = 2048 + 40: the chunk-end states x in the reference's layout, return_last_state, and the long-sequence tolerances"""
    from dimsum_amd import native
    L, N = 2048 + 40, 12
    c, ref = _case(("chunks", cplx), batch=1, dim=8, L=L, N=N, cplx=cplx, var_B=True, var_C=True, seed=3)
    g = _gpu_leaves(c)
    res, last = _run_fn(g)
    _check_all(c, ref, g, res, last, L, tol(L), _bwd_tol(L), _bwd_tol(L, True))
    with torch.no_grad():
        out, x, out_z = native.selective_scan_general_fwd(g["u"], g["delta"], g["A"], g["B"], g["C"], g["D"], g["z"], g["delta_bias"], True)
    assert x.shape == (1, 8, 2, 2 * N) and x.dtype == g["A"].dtype
    assert_close(_np(x[..., 1::2]), _np(ref["ends"]), what="x.h", **tol(L))
    assert_close(_np(out), _np(ref["out"]), what="out", **tol(L))
    # the running product of exp(dt A) over the prefix
    dt = torch.nn.functional.softplus(c["delta"].detach() + c["delta_bias"].detach()[None, :, None])
    prod = torch.stack([torch.exp(dt[..., :2048].sum(-1)[..., None] * c["A"].detach()), torch.exp(dt.sum(-1)[..., None] * c["A"].detach())], dim=2)
    if not cplx:
        assert_close(_np(x[..., 0::2]), _np(prod), 2e-3, 1e-30, "x.prod_a")      # test_scan_gpu.py's bound for the same quantity
    else:
        # a bound from the number format, not from a measurement of the reference (its float32 selective_scan_ref returns no running product):
        # the phase of the product is A.im sum(dt): sum(dt) ~ 2000 carries an fp32 rounding of 2^-24 x 2048 = 1.2e-4 (the kernel's sum is
        # compensated), the argument A.im sum(dt) of sin / cos another one, |A.im| <~ 4 -> 4 x 2.4e-4 = 1e-3 of each element's modulus; x 2
        got, want = x[..., 0::2].cpu().to(torch.complex128), prod
        assert ((got - want).abs() <= 2e-3 * want.abs() + 1e-30).all(), ((got - want).abs() / (want.abs() + 1e-300)).max()


@pytest.mark.parametrize("dtype,rtol,atol", [(torch.bfloat16, 3e-2, 5e-2), (torch.float16, 3e-3, 5e-3)])
@pytest.mark.parametrize("cplx", [False, True])
def test_half_dtypes(cplx, dtype, rtol, atol):
    """16-bit I/O on one real and one complex combination: forward at the reference's per-dtype tolerance (test_selective_scan.py:49-53),
    gradients at its rtolw / atolw rule for them (:158-172: the same rtol, atol x 5 for the sums over channels / batch / time)"""
    L, N = 37, 12
    c, ref = _case(("half", cplx, dtype), batch=2, dim=72, L=L, N=N, cplx=cplx, var_B=True, var_C=not cplx, seed=5, dtype=dtype)
    g = _gpu_leaves(c, dtype)
    res, last = _run_fn(g)
    assert res.dtype == dtype
    f, w = dict(rtol=rtol, atol=atol), dict(rtol=rtol, atol=5 * atol)
    _check_all(c, ref, g, res, last, L, f, f, w)


def test_xz_halves_and_d_major_delta():
    """u and z as the two halves of one xz buffer, delta d-major (strides (L, B L, 1)), dz into a caller's view -- MambaInnerFn's layouts"""
    from dimsum_amd import native
    Bt, D, L, N = 2, 72, 37, 12
    c, ref = _case(("odd", False, True, True, N), batch=Bt, dim=D, L=L, N=N, cplx=False, var_B=True, var_C=True, seed=N)
    f = lambda k: c[k].detach().float().cuda()
    xz = torch.cat([f("u"), f("z")], dim=1)
    u, z = xz.chunk(2, dim=1)
    delta = f("delta").permute(1, 0, 2).contiguous().permute(1, 0, 2)
    dout = f("dout").permute(1, 0, 2).contiguous().permute(1, 0, 2)
    assert delta.stride() == (L, Bt * L, 1) and u.stride(0) == 2 * D * L
    out, x, out_z = native.selective_scan_general_fwd(u, delta, f("A"), f("B"), f("C"), f("D"), z, f("delta_bias"), True)
    assert out.stride() == delta.stride()
    dxz = torch.full_like(xz, float("nan"))
    du, ddelta, dA, dB, dC, dD, dbias, dz = native.selective_scan_general_bwd(u, delta, f("A"), f("B"), f("C"), f("D"), z, f("delta_bias"), dout, out,
                                                                            dxz.chunk(2, dim=1)[1], True)
    torch.cuda.synchronize()
    assert_close(_np(out_z), _np(ref["res"]), what="out_z", **tol(L))
    assert dz.data_ptr() == dxz.chunk(2, dim=1)[1].data_ptr() and torch.isnan(dxz[:, :D]).all()
    for got, k in ((du, "u"), (ddelta, "delta"), (dz, "z"), (dB, "B"), (dC, "C")):
        assert_close(_np(got), _np(c[k].grad), what="d" + k, **_bwd_tol(L))
    for got, k in ((dA, "A"), (dD, "D"), (dbias, "delta_bias")):
        assert_close(_np(got), _np(c[k].grad), what="d" + k, **_bwd_tol(L, True))


def test_forced_general_against_the_tuned_kernel():
    """dstate 16, real, input-dependent B / C: the general kernels asked for by name against the tuned ones, at the forward tolerance (and the
    gradients at theirs)"""
    from dimsum_amd import native
    from dimsum_amd.ops import selective_scan_fn
    L = 64
    c, _ = _case(("tuned",), batch=2, dim=128, L=L, N=16, cplx=False, var_B=True, var_C=True, groups=1, seed=9)
    runs = []
    for force in (False, True):
        g = _gpu_leaves(c)
        with native.scan_force_general(force):
            assert native.scan_takes_general_path(16, force=native.scan_general_forced()) == force
            res = selective_scan_fn(g["u"], g["delta"], g["A"], g["B"], g["C"], g["D"], g["z"], g["delta_bias"], delta_softplus=True)
            res.backward(g["dout"])
        runs.append((res, g))
    torch.cuda.synchronize()
    (r0, g0), (r1, g1) = runs
    assert_close(_np(r1), _np(r0), what="out", **tol(L))
    for k in ("u", "delta", "z", "B", "C"):
        assert_close(_np(g1[k].grad), _np(g0[k].grad), what="d" + k, **_bwd_tol(L))
    for k in ("A", "D", "delta_bias"):
        assert_close(_np(g1[k].grad), _np(g0[k].grad), what="d" + k, **_bwd_tol(L, True))


def test_two_launches():
    """fixed-order sums are bit-equal between two launches; the atomically added ones agree within the gradient tolerance"""
    L = 37
    c, _ = _case(("odd", True, True, False, 12), batch=2, dim=72, L=L, N=12, cplx=True, var_B=True, var_C=False, seed=12)
    g0, g1 = _gpu_leaves(c), _gpu_leaves(c)
    (r0, l0), (r1, l1) = _run_fn(g0), _run_fn(g1)
    assert torch.equal(r0, r1) and torch.equal(torch.view_as_real(l0), torch.view_as_real(l1))
    for k in ("u", "delta", "z"):
        assert torch.equal(g0[k].grad, g1[k].grad), k
    assert_close(_np(g1["B"].grad), _np(g0["B"].grad), what="dB", **_bwd_tol(L))
    for k in ("A", "C", "D", "delta_bias"):
        assert_close(_np(g1[k].grad), _np(g0[k].grad), what="d" + k, **_bwd_tol(L, True))


# ---- the modules --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,d_state", [("Mamba", 64), ("CondMamba", 12)])
def test_mamba_modules_any_d_state(which, d_state):
    """forward and every parameter gradient of Mamba(d_model=32, d_state=64) / CondMamba(d_state=12) on the GPU against the same module on the
    CPU oracle backend"""
    import copy

    from dimsum_amd.modules import mamba_simple
    from oracle import torch_backend
    torch.manual_seed(0)
    cls = getattr(mamba_simple, which)
    m = cls(d_model=32, d_state=d_state)
    x = torch.randn(2, 24, 32)
    cond = torch.randn(2, 32) if which == "CondMamba" else None
    dy = torch.randn(2, 24, 32)
    mg = copy.deepcopy(m).cuda()
    args = (x.cuda(),) if cond is None else (x.cuda(), cond.cuda())
    yg = mg(*args)
    yg.backward(dy.cuda())
    with torch_backend.cpu_oracle_backend():       # (CPU tensors keep to native.selective_scan_fwd / _bwd, which the oracle stands in for)
        yc = m(x) if cond is None else m(x, cond)
        yc.backward(dy)
    torch.cuda.synchronize()
    assert_close(yg.detach().cpu().numpy(), yc.detach().numpy(), what="y", **tol(24))
    for (n, pg), (_, pc) in zip(mg.named_parameters(), m.named_parameters()):
        if pc.grad is None:
            assert pg.grad is None, n
            continue
        assert_close(pg.grad.cpu().numpy(), pc.grad.numpy(), what=n, **_bwd_tol(24, True))


# ---- a model -------------------------------------------------------------------------------------------------------------------------------
def _dim_d_state_64():
    from dimsum_amd.models_dim import DiM
    from procedural import procedural_fill
    from test_train_gpu import KW
    m = DiM(depth=2, hidden_size=64, patch_size=2, ssm_cfg={"d_state": 64}, **{**KW, "use_attn_every_k_layers": 2})
    procedural_fill(m, seed=3)
    return m


@pytest.mark.usefixtures("allow_torch_sdpa")      # hidden 64: head_dim 4 (conftest)
def test_dim_d_state_64_forward_and_training_step():
    """a tiny DiM(ssm_cfg={"d_state": 64}): the no-grad forward (inference route of the mixers: transposed x_proj, no `out` / `x` stores) and
    one training step on the HIP path against the same through the CPU oracle backend -- finite, forward at the model tests' rule
    (rtol 1e-3 + 1e-4 max|ref|), loss and gradients at test_train_gpu.py's (loss rtol 1e-4, gradients rtol 1e-3 + 2e-4 max|ref|)"""
    from dimsum_amd.train import build_training, train_step
    from oracle.torch_backend import cpu_oracle_backend
    from procedural import seeded
    from test_train_gpu import _fixed_transport
    T = torch.from_numpy
    torch.backends.cuda.matmul.allow_tf32 = False

    def run(dev):
        x, y = T(seeded((2, 4, 32, 32), 81)).to(dev), torch.tensor([1, 333], device=dev)
        t = T(seeded((2,), 82, kind="uniform")).to(dev)
        model, ema, opt = build_training(_dim_d_state_64().to(dev), dev, lr=1e-4)
        with torch.no_grad():
            fwd = model.eval()(x, t, y).cpu().numpy()
        tr = _fixed_transport(t.cpu(), T(seeded((2, 4, 32, 32), 83)))
        loss = train_step(model.train(), ema, opt, tr, x, y, max_grad_norm=2.0, ema_decay=0.5)
        return fwd, loss.item(), {k: (None if p.grad is None else p.grad.detach().cpu().numpy()) for k, p in model.named_parameters()}, \
            {k: v.detach().cpu().numpy() for k, v in model.named_parameters()}

    fwd_g, loss_g, grads_g, params_g = run("cuda")
    with cpu_oracle_backend():
        fwd_c, loss_c, grads_c, _ = run("cpu")
    assert np.isfinite(fwd_g).all() and np.isfinite(loss_g) and all(np.isfinite(v).all() for v in params_g.values())
    assert_close(fwd_g, fwd_c, 1e-3, 0, "forward", scale_atol=1e-4)
    assert abs(loss_g - loss_c) <= 1e-4 * abs(loss_c), (loss_g, loss_c)
    n_live = 0
    for k, gc in grads_c.items():
        if gc is None:
            assert grads_g[k] is None or not grads_g[k].any(), k
            continue
        assert_close(grads_g[k], gc, 1e-3, 0, "grad " + k, scale_atol=2e-4)
        n_live += 1
    assert n_live > 20 and any("A_log" in k and grads_c[k] is not None and grads_c[k].shape[-1] == 64 for k in grads_c)
