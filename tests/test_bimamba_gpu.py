"""bimamba_inner_fn on the MI355X: the bidirectional scan (native.selective_scan_bidir_fwd / _bwd, csrc/ssm_scan_fwd_kernel.hpp and
csrc/ssm_scan_bwd.hip with kRev) against the reference's goldens, against the existing HIP scan run on explicitly flipped copies, against the
CPU oracle composed with flips, in fp16 / bf16, for determinism, and for the absence of flip / copy kernels in the forward.

Bounds. Kernel level: the reversed direction does exactly the arithmetic of the existing kernel on flipped copies, and the sum of the two
directions is formed in the same order as the composition's flip-and-add -- so out, out_b, out_z, the saved states, du, ddelta, dz, dB and dC
are required BITWISE equal. dA, dA_b, dD and ddelta_bias are float atomics over workgroups (as in the existing backward): 1e-5 of max|ref|.
Goldens (fp32): the tolerances of the mamba_inner golden (test_model_gpu.py), north star 1e-3 relative."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close, golden

pytestmark = pytest.mark.gpu

T = torch.from_numpy


# ---- goldens: bimamba_inner_ref fwd + autograd on the CPU (tools/gen_golden.py, target "bimamba") -----------------------------------------
def _run_golden(g, dev="cuda"):
    from dimsum_amd.ops import bimamba_inner_fn
    names = [k for k in ("conv_w", "conv_b", "x_proj_w", "dt_proj_w", "out_proj_w", "out_proj_b", "A", "A_b", "Dv", "dt_bias",
                         "B_proj_b", "C_proj_b") if k in g.files]
    p = {k: T(g[k]).to(dev).requires_grad_() for k in names}
    xz = T(g["xz"]).to(dev).requires_grad_()
    out = bimamba_inner_fn(xz, p["conv_w"], p["conv_b"], p["x_proj_w"], p["dt_proj_w"], p["out_proj_w"], p.get("out_proj_b"), p["A"], p["A_b"],
                           None, None, p["Dv"], delta_bias=p["dt_bias"], B_proj_bias=p.get("B_proj_b"), C_proj_bias=p.get("C_proj_b"),
                           delta_softplus=True)
    out.backward(T(g["dout"]).to(dev))
    return out.detach(), xz.grad, {k: v.grad for k, v in p.items()}


@pytest.mark.parametrize("tf32", [True, False])
@pytest.mark.parametrize("case", ["bimamba_w4_n16", "bimamba_w3_n8"])
def test_golden(case, tf32):
    """forward and every gradient vs autograd through bimamba_inner_ref -- the true derivative (dxz's z half holds BOTH directions' dz, which
    the reference's BiMambaInnerFn.backward does not return): under the reference's allow_tf32 and in exact fp32"""
    g = golden(case)
    old = torch.backends.cuda.matmul.allow_tf32
    try:
        torch.backends.cuda.matmul.allow_tf32 = tf32
        out, dxz, grads = _run_golden(g)
    finally:
        torch.backends.cuda.matmul.allow_tf32 = old
    s = 1.0 if not tf32 else 5.0
    assert_close(out.cpu().numpy(), g["out"], 2e-4 * s, 0, "out", scale_atol=2e-5 * s)
    assert_close(dxz.cpu().numpy(), g["dxz"], 5e-4 * s, 0, "dxz", scale_atol=5e-5 * s)
    assert set(grads) == {k[2:] for k in g.files if k.startswith("g_")}
    for k, v in grads.items():
        assert_close(v.cpu().numpy(), g["g_" + k], 1e-3, 0, "g_" + k, scale_atol=2e-4)


# ---- kernel level: the bidirectional pair vs the existing scan on flipped copies --------------------------------------------------------
def _operands(b, d, L, N, dtype=torch.float32, seed=0):
    """the layouts the mixer hands the scan: u, z = halves of xz; delta d-major (strides (L, b L, 1)); B, C rows of a (2N, b L) matrix"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    xz = torch.randn(b, 2 * d, L, device="cuda", generator=g).to(dtype)
    u, z = xz.chunk(2, dim=1)
    delta = (0.5 * torch.rand(d, b * L, device="cuda", generator=g) - 0.3).to(dtype).view(d, b, L).permute(1, 0, 2)
    bc = torch.randn(2 * N, b * L, device="cuda", generator=g).to(dtype)
    Bm = bc[:N].view(N, b, L).permute(1, 0, 2).unsqueeze(1)
    Cm = bc[N:].view(N, b, L).permute(1, 0, 2).unsqueeze(1)
    A = -0.5 * torch.rand(d, N, device="cuda", generator=g) - 0.05
    A_b = -0.5 * torch.rand(d, N, device="cuda", generator=g) - 0.05
    D = torch.randn(d, device="cuda", generator=g)
    bias = 0.5 * torch.rand(d, device="cuda", generator=g)
    dout = torch.randn(b, d, L, device="cuda", generator=g).to(dtype)
    return u, delta, A, A_b, Bm, Cm, D, z, bias, dout


def _fl(t):
    return t.flip(-1).contiguous()


def _composed(u, delta, A, A_b, Bm, Cm, D, z, bias, dout):
    """what the fused pair replaces: flips of u / delta / B / C / z (/ dout), two launches of the existing scan (on the kernel the pair runs),
    flip-and-add of out_z (of the gradients)"""
    from dimsum_amd import native
    b, d, L, N = u.shape + (A.shape[1],)
    with native.scan_fwd_variant(native.scan_bidir_fwd_kernel_for(b, d, L, N)):
        out_f, _, oz_f, ck_f = native.selective_scan_fwd(u, delta, A, Bm, Cm, D, z, bias, True, need_x=False, need_ckpt=True)
        fu, fd, fB, fC, fz = _fl(u), _fl(delta), _fl(Bm), _fl(Cm), _fl(z)
        out_b, _, oz_b, ck_b = native.selective_scan_fwd(fu, fd, A_b, fB, fC, D, fz, bias, True, need_x=False, need_ckpt=True)
    fwd = dict(out=out_f, out_b=out_b.flip(-1), out_z=oz_f + oz_b.flip(-1), ckpt=ck_f, ckpt_b=ck_b)
    f = native.selective_scan_bwd(u, delta, A, Bm, Cm, D, z, bias, dout, None, out_f, None, True, False, ckpt=ck_f)
    r = native.selective_scan_bwd(fu, fd, A_b, fB, fC, D, fz, bias, _fl(dout), None, out_b, None, True, False, ckpt=ck_b)
    bwd = dict(du=f[0] + r[0].flip(-1), ddelta=f[1] + r[1].flip(-1), dA=f[2], dA_b=r[2], dB=f[3] + r[3].flip(-1), dC=f[4] + r[4].flip(-1),
               dD=f[5] + r[5], ddelta_bias=f[6] + r[6], dz=f[7] + r[7].flip(-1))
    return fwd, bwd


def _fused(u, delta, A, A_b, Bm, Cm, D, z, bias, dout):
    from dimsum_amd import native
    out, out_b, out_z, ck, ck_b = native.selective_scan_bidir_fwd(u, delta, A, A_b, Bm, Cm, D, z, bias, True, need_out=True, need_ckpt=True)
    fwd = dict(out=out, out_b=out_b, out_z=out_z, ckpt=ck, ckpt_b=ck_b)
    du, ddelta, dA, dA_b, dB, dC, dD, dbias, dz, oz = native.selective_scan_bidir_bwd(u, delta, A, A_b, Bm, Cm, D, z, bias, dout, out, out_b,
                                                                                     ck, ck_b, True, True)
    bwd = dict(du=du, ddelta=ddelta, dA=dA, dA_b=dA_b, dB=dB, dC=dC, dD=dD, ddelta_bias=dbias, dz=dz)
    return fwd, bwd, oz


ATOMIC = ("dA", "dA_b", "dD", "ddelta_bias")
KERNEL_SHAPES = [(256, 1024, 256, 16), (2, 128, 4096, 16), (2, 96, 333, 8), (3, 80, 256, 4), (2, 64, 200, 32), (2, 18, 333, 16),
                 (1, 64, 4096, 16)]


@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_vs_flipped_composition(shape):
    """as-run mixer shape, L = 4096 (two 2048-chunks), odd L (element-wise path), dim not a multiple of 64 (masked lanes), dstate 4 .. 32;
    the small dstate-16 launches run on the one-lane-per-state kernel (odd L and dim % 4 != 0 among them)"""
    from dimsum_amd import native
    b, d, L, N = shape
    assert native.scan_bidir_fwd_kernel_for(b, d, L, N) == (16 if N == 16 and b * d <= 256 else 1)
    ops = _operands(b, d, L, N)
    fwd_r, bwd_r = _composed(*ops)
    fwd, bwd, oz = _fused(*ops)
    torch.cuda.synchronize()
    for k, v in fwd.items():
        assert torch.equal(v, fwd_r[k]), f"{k}: max |diff| {(v - fwd_r[k]).abs().max().item():.3e}"
    assert (oz - fwd_r["out_z"]).abs().max().item() <= 1e-6 * fwd_r["out_z"].abs().max().item(), "recomputed out_z"
    for k, v in bwd.items():
        if k in ATOMIC:
            ref = bwd_r[k]
            assert (v - ref).abs().max().item() <= 1e-5 * ref.abs().max().item(), k
        else:
            assert torch.equal(v, bwd_r[k]), f"{k}: max |diff| {(v - bwd_r[k]).abs().max().item():.3e}"


def test_kernel_is_deterministic():
    """two calls at the as-run shape: the outputs and the non-atomic gradients bit for bit"""
    ops = _operands(256, 1024, 256, 16, seed=3)
    a = _fused(*ops)
    b = _fused(*ops)
    for k in a[0]:
        assert torch.equal(a[0][k], b[0][k]), k
    for k in a[1]:
        if k not in ATOMIC:
            assert torch.equal(a[1][k], b[1][k]), k


# ---- the mixer against the CPU oracle composed with flips ------------------------------------------------------------------------------
def _mixer_params(d_model, d_inner, N, R, W, dtype=torch.float32, seed=0, biases=False):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    p = dict(conv_w=rn(d_inner, 1, W) * 0.5, conv_b=rn(d_inner) * 0.1, x_proj_w=(rn(R + 2 * N, d_inner) / d_inner ** 0.5).to(dtype),
             dt_proj_w=(rn(d_inner, R) / R ** 0.5).to(dtype), out_proj_w=(rn(d_model, d_inner) / d_inner ** 0.5).to(dtype),
             A=-torch.exp(torch.log(torch.arange(1, N + 1).float()).repeat(d_inner, 1) + 0.1 * rn(d_inner, N)),
             A_b=-torch.exp(torch.log(torch.arange(1, N + 1).float()).repeat(d_inner, 1) + 0.1 * rn(d_inner, N)),
             Dv=1 + 0.1 * rn(d_inner), dt_bias=rn(d_inner) * 0.5 - 4.0)
    if biases:
        p.update(out_proj_b=0.1 * rn(d_model), B_proj_b=0.1 * rn(N), C_proj_b=0.1 * rn(N))
    return p


def _oracle_mixer(xz, p):
    """bimamba_inner_ref's math on the CPU: conv / projections in float64 torch, both scans on the C oracle, the second on flipped arrays"""
    from oracle import c_ops
    xz = xz.double().cpu()
    q = {k: v.double().cpu() for k, v in p.items()}
    d = q["conv_w"].shape[0]
    R, N = q["dt_proj_w"].shape[1], q["A"].shape[1]
    bsz, L = xz.shape[0], xz.shape[-1]
    x, z = xz[:, :d], xz[:, d:]
    W = q["conv_w"].shape[-1]
    x = F.silu(F.conv1d(F.pad(x, (W - 1, 0)), q["conv_w"], q["conv_b"], groups=d))
    x_dbl = torch.einsum("bdl,rd->brl", x, q["x_proj_w"])
    delta = torch.einsum("brl,dr->bdl", x_dbl[:, :R], q["dt_proj_w"])
    Bm = x_dbl[:, R:R + N] + (q["B_proj_b"][:, None] if "B_proj_b" in q else 0)
    Cm = x_dbl[:, R + N:] + (q["C_proj_b"][:, None] if "C_proj_b" in q else 0)
    f32 = lambda t: np.ascontiguousarray(t.float().numpy())
    fl = lambda t: np.ascontiguousarray(f32(t)[..., ::-1])
    _, oz_f, _ = c_ops.selective_scan_fwd(f32(x), f32(delta), f32(q["A"]), f32(Bm)[:, None], f32(Cm)[:, None], f32(q["Dv"]), f32(z),
                                          f32(q["dt_bias"]), True)
    _, oz_b, _ = c_ops.selective_scan_fwd(fl(x), fl(delta), f32(q["A_b"]), fl(Bm)[:, None], fl(Cm)[:, None], f32(q["Dv"]), fl(z),
                                          f32(q["dt_bias"]), True)
    y = torch.from_numpy(oz_f.astype(np.float64) + oz_b[..., ::-1].astype(np.float64))
    out = torch.einsum("bdl,ed->ble", y, q["out_proj_w"])
    if "out_proj_b" in q:
        out = out + q["out_proj_b"]
    return out.numpy()


def _call(xz, p):
    from dimsum_amd.ops import bimamba_inner_fn
    return bimamba_inner_fn(xz, p["conv_w"], p["conv_b"], p["x_proj_w"], p["dt_proj_w"], p["out_proj_w"], p.get("out_proj_b"), p["A"], p["A_b"],
                            None, None, p["Dv"], delta_bias=p["dt_bias"], B_proj_bias=p.get("B_proj_b"), C_proj_bias=p.get("C_proj_b"))


@pytest.mark.parametrize("grad", [False, True])
def test_model_sized_mixer_vs_oracle(grad):
    """(batch 4, d_inner 2048, L 256): DiM-L/2's mixer width, d_model 1024, dt_rank 64, dstate 16; exact fp32 GEMMs. With grad the training
    launch (saved `out` / states, out_proj on the kept out_z) runs, and the backward goes through"""
    bsz, d_model, d_inner, L, N, R = 4, 1024, 2048, 256, 16, 64
    p = _mixer_params(d_model, d_inner, N, R, 4, biases=True)
    xz = torch.randn(bsz, 2 * d_inner, L, generator=torch.Generator().manual_seed(7))
    ref = _oracle_mixer(xz, p)
    pc = {k: v.cuda().requires_grad_(grad) for k, v in p.items()}
    xc = xz.cuda().requires_grad_(grad)
    old = torch.backends.cuda.matmul.allow_tf32
    try:
        torch.backends.cuda.matmul.allow_tf32 = False
        out = _call(xc, pc)
        if grad:
            out.backward(torch.randn_like(out))
    finally:
        torch.backends.cuda.matmul.allow_tf32 = old
    assert_close(out.detach().cpu().numpy(), ref, 2e-4, 0, "out", scale_atol=2e-5)
    if grad:
        for k, v in pc.items():
            assert v.grad is not None and torch.isfinite(v.grad).all(), k
        assert torch.isfinite(xc.grad).all()


@pytest.mark.parametrize("dtype,rtol,atol", [(torch.float16, 3e-3, 5e-3), (torch.bfloat16, 3e-2, 5e-2)], ids=["fp16", "bf16"])
def test_half_dtypes_vs_fp32_oracle(dtype, rtol, atol):
    """xz and the projection weights in fp16 / bf16 (conv, A, A_b, D, delta_bias fp32), as in the reference's own test
    (test_selective_scan.py:312-396, dim 768, dt_rank 48, dstate 8, width 3), against the fp32 oracle on the same rounded inputs, at that
    test's tolerances -- its absolute part taken relative to max|ref| (the output is a sum over 768 channels)"""
    bsz, d_model, d_inner, L, N, R = 2, 384, 768, 256, 8, 48
    p = _mixer_params(d_model, d_inner, N, R, 3, dtype=dtype, seed=2)
    xz = torch.randn(bsz, 2 * d_inner, L, generator=torch.Generator().manual_seed(9)).to(dtype)
    ref = _oracle_mixer(xz, p)
    pc = {k: v.cuda().requires_grad_() for k, v in p.items()}
    xc = xz.cuda().requires_grad_()
    out = _call(xc, pc)
    assert out.dtype == dtype
    out.backward(torch.randn_like(out))
    assert_close(out.detach().float().cpu().numpy(), ref, rtol, 0, "out", scale_atol=atol)
    assert xc.grad.dtype == dtype and torch.isfinite(xc.grad.float()).all()
    for k, v in pc.items():
        assert torch.isfinite(v.grad.float()).all(), k


def test_mixer_is_deterministic():
    """two forward + backward passes give bit-identical outputs and gradients. Batch 1: the float atomics of the existing conv / scan
    backwards (dA, dD, ddelta_bias, conv weight) then see one addend per address and launch, which is what makes the comparison meaningful"""
    p = _mixer_params(256, 512, 16, 16, 4, biases=True, seed=4)
    xz = torch.randn(1, 1024, 512, generator=torch.Generator().manual_seed(5))
    dout = None
    res = []
    for _ in range(2):
        pc = {k: v.cuda().requires_grad_() for k, v in p.items()}
        xc = xz.cuda().requires_grad_()
        out = _call(xc, pc)
        if dout is None:
            dout = torch.randn_like(out)
        out.backward(dout)
        res.append([out.detach(), xc.grad] + [pc[k].grad for k in sorted(pc)])
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_no_flip_or_copy_kernels_in_the_forward():
    """the kernels between the conv and out_proj: the x_proj / dt_proj GEMMs and the two scan launches -- no flip, no copy"""
    from torch.profiler import ProfilerActivity, profile
    p = {k: v.cuda() for k, v in _mixer_params(256, 512, 16, 16, 4, seed=6).items()}
    xz = torch.randn(2, 1024, 256, device="cuda")
    with torch.no_grad():
        _call(xz, p)                                     # warm-up (library handles, allocator)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            _call(xz, p)
            torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    conv = [i for i, n in enumerate(names) if "conv1d" in n]
    scans = [i for i, n in enumerate(names) if "ssm_scan_fwd" in n]
    assert conv and len(scans) == 2, names
    between = names[conv[0] + 1:scans[-1]]
    bad = [n for n in between if any(w in n.lower() for w in ("flip", "copy", "elementwise", "reverse"))]
    assert not bad, between
    assert sum("ssm_scan_fwd" in n for n in between) == 1 and len(between) <= 4, between
