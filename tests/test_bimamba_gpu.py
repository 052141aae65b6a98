"""bimamba_inner_fn on the MI355X: the bidirectional scan (native.selective_scan_bidir_fwd / _bwd, csrc/ssm_scan_fwd_kernel.hpp and
csrc/ssm_scan_bwd.hip with kRev) against the reference's goldens, against the existing HIP scan run on explicitly flipped copies, against the
CPU oracle composed with flips, in fp16 / bf16, for determinism, and for the absence of flip / copy kernels in the forward. The pair also
against the C oracle at the launch-path edges (L < 4, whole and partial 2048-step chunks, two groups, unaligned dB / dC, optional operands
off), and the mixer's gradients against autograd through a float64 reference whose scans run on the C oracle.

Bounds. Kernel level, fp32: the reversed direction does exactly the arithmetic of the existing kernel on flipped copies, and the sum of the
two directions is formed in the same order as the composition's flip-and-add -- so out, out_b, out_z, the saved states, du, ddelta, dz, dB
and dC are required BITWISE equal. dA, dA_b, dD and ddelta_bias are float atomics over workgroups (as in the existing backward): 1e-5 of
max|ref|. Only fp32 is bitwise: in fp16 / bf16 the reversed direction adds its UNROUNDED fp32 half to the forward half already rounded to
the I/O type and rounds once (the composition rounds each half, then their sum), so the pair is within one unit in the last place of the
composition, 2^-p (|forward half| + |reversed half|) elementwise. Against the C oracle: tol(L) / _bwd_tol(L, weight)
of test_scan_gpu.py in fp32, 1.5 tol_rel max|ref| in fp16 / bf16 (test_bwd_half_dtypes).
Goldens and the mixer (fp32): the tolerances of the mamba_inner golden (test_model_gpu.py), north star 1e-3 relative; fp16 / bf16 mixer:
those of the reference's own test."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close, golden
from test_scan_gpu import _bwd_tol, tol

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


def _f32(t):
    return np.ascontiguousarray(t.detach().float().numpy())


class _OracleScan(torch.autograd.Function):
    """one direction of the scan inside a float64 autograd graph: forward = c_ops.selective_scan_fwd's out_z, backward = c_ops.selective_scan_bwd
    (delta_softplus on, as in the mixer)"""

    @staticmethod
    def forward(ctx, u, delta, A, B, C, D, z, delta_bias):
        from oracle import c_ops
        ctx.save_for_backward(u, delta, A, B, C, D, z, delta_bias)
        return torch.from_numpy(c_ops.selective_scan_fwd(*(_f32(t) for t in (u, delta, A, B, C, D, z, delta_bias)), True)[1]).double()

    @staticmethod
    def backward(ctx, dout):
        from oracle import c_ops
        r = c_ops.selective_scan_bwd(*(_f32(t) for t in ctx.saved_tensors), True, _f32(dout))
        return tuple(torch.from_numpy(r[k]).double() for k in ("du", "ddelta", "dA", "dB", "dC", "dD", "dz", "ddelta_bias"))


def _ref_mixer_autograd(xz, p, dout):
    """bimamba_inner_ref with autograd on the CPU: conv, x_proj, dt_proj, the B / C biases, the flips and out_proj in float64 torch (as
    _oracle_mixer), each direction's scan on the C oracle (_OracleScan) -> out, d xz, {parameter: gradient} as float64 numpy"""
    xz = xz.detach().double().requires_grad_()
    q = {k: v.detach().double().requires_grad_() for k, v in p.items()}
    d, W = q["conv_w"].shape[0], q["conv_w"].shape[-1]
    R, N = q["dt_proj_w"].shape[1], q["A"].shape[1]
    x, z = xz[:, :d], xz[:, d:]
    x = F.silu(F.conv1d(F.pad(x, (W - 1, 0)), q["conv_w"], q["conv_b"], groups=d))
    x_dbl = torch.einsum("bdl,rd->brl", x, q["x_proj_w"])
    delta = torch.einsum("brl,dr->bdl", x_dbl[:, :R], q["dt_proj_w"])
    Bm = x_dbl[:, R:R + N] + (q["B_proj_b"][:, None] if "B_proj_b" in q else 0)
    Cm = x_dbl[:, R + N:] + (q["C_proj_b"][:, None] if "C_proj_b" in q else 0)
    fl = lambda t: t.flip(-1)
    scan = _OracleScan.apply
    y = (scan(x, delta, q["A"], Bm[:, None], Cm[:, None], q["Dv"], z, q["dt_bias"])
         + fl(scan(fl(x), fl(delta), q["A_b"], fl(Bm)[:, None], fl(Cm)[:, None], q["Dv"], fl(z), q["dt_bias"])))
    out = torch.einsum("bdl,ed->ble", y, q["out_proj_w"])
    if "out_proj_b" in q:
        out = out + q["out_proj_b"]
    out.backward(dout.double())
    return out.detach().numpy(), xz.grad.numpy(), {k: v.grad.numpy() for k, v in q.items()}


def _call(xz, p):
    from dimsum_amd.ops import bimamba_inner_fn
    return bimamba_inner_fn(xz, p["conv_w"], p["conv_b"], p["x_proj_w"], p["dt_proj_w"], p["out_proj_w"], p.get("out_proj_b"), p["A"], p["A_b"],
                            None, None, p["Dv"], delta_bias=p["dt_bias"], B_proj_bias=p.get("B_proj_b"), C_proj_bias=p.get("C_proj_b"))


def _model_sized(grad, biases):
    bsz, d_model, d_inner, L, N, R = 4, 1024, 2048, 256, 16, 64
    p = _mixer_params(d_model, d_inner, N, R, 4, biases=biases)
    xz = torch.randn(bsz, 2 * d_inner, L, generator=torch.Generator().manual_seed(7))
    dout = torch.randn(bsz, L, d_model, generator=torch.Generator().manual_seed(8))
    pc = {k: v.cuda().requires_grad_(grad) for k, v in p.items()}
    xc = xz.cuda().requires_grad_(grad)
    old = torch.backends.cuda.matmul.allow_tf32
    try:
        torch.backends.cuda.matmul.allow_tf32 = False
        out = _call(xc, pc)
        if grad:
            out.backward(dout.cuda())
    finally:
        torch.backends.cuda.matmul.allow_tf32 = old
    if not grad:
        assert_close(out.detach().cpu().numpy(), _oracle_mixer(xz, p), 2e-4, 0, "out", scale_atol=2e-5)
        return
    ref, ref_dxz, ref_g = _ref_mixer_autograd(xz, p, dout)
    assert_close(out.detach().cpu().numpy(), ref, 2e-4, 0, "out", scale_atol=2e-5)
    assert_close(xc.grad.cpu().numpy(), ref_dxz, 5e-4, 0, "dxz", scale_atol=5e-5)
    assert set(ref_g) == set(pc)
    for k, v in pc.items():
        assert_close(v.grad.cpu().numpy(), ref_g[k], 1e-3, 0, "g_" + k, scale_atol=2e-4)


@pytest.mark.parametrize("grad", [False, True])
def test_model_sized_mixer_vs_oracle(grad):
    """(batch 4, d_inner 2048, L 256): DiM-L/2's mixer width, d_model 1024, dt_rank 64, dstate 16; exact fp32 GEMMs; all biases (out_proj on
    F.linear). With grad the training launch (saved `out` / states, out_proj on the kept out_z) runs, and dxz and every parameter gradient are
    compared with autograd through the float64 reference (_ref_mixer_autograd) for the same dout, at the golden test's exact-fp32 bounds"""
    _model_sized(grad, biases=True)


def test_model_sized_mixer_grads_without_biases_vs_oracle():
    """as test_model_sized_mixer_vs_oracle[True] without out_proj / B_proj / C_proj biases: out_proj on gemm.linear, no bias rows in the
    backward"""
    _model_sized(True, biases=False)


@pytest.mark.parametrize("dtype,rtol,atol", [(torch.float16, 3e-3, 5e-3), (torch.bfloat16, 3e-2, 5e-2)], ids=["fp16", "bf16"])
def test_half_dtypes_vs_fp32_oracle(dtype, rtol, atol):
    """xz and the projection weights in fp16 / bf16 (conv, A, A_b, D, delta_bias fp32), as in the reference's own test
    (test_selective_scan.py:312-396, dim 768, dt_rank 48, dstate 8, width 3), against the fp32 oracle on the same rounded inputs, at that
    test's tolerances -- its absolute part taken relative to max|ref| (the output is a sum over 768 channels). The gradients against autograd
    through the float64 reference (_ref_mixer_autograd) on the same rounded inputs and dout, also at that test's tolerances: xz.grad at
    2 rtol / 2 atol, the parameters at rtolw = max(1e-3, rtol), atolw = max(1e-3, atol). This run takes the half-precision branch of the
    backward, where dB / dC are cast and copied into d x_dbl."""
    bsz, d_model, d_inner, L, N, R = 2, 384, 768, 256, 8, 48
    p = _mixer_params(d_model, d_inner, N, R, 3, dtype=dtype, seed=2)
    xz = torch.randn(bsz, 2 * d_inner, L, generator=torch.Generator().manual_seed(9)).to(dtype)
    dout = torch.randn(bsz, L, d_model, generator=torch.Generator().manual_seed(10)).to(dtype)
    ref, ref_dxz, ref_g = _ref_mixer_autograd(xz, p, dout)
    pc = {k: v.cuda().requires_grad_() for k, v in p.items()}
    xc = xz.cuda().requires_grad_()
    out = _call(xc, pc)
    assert out.dtype == dtype
    out.backward(dout.cuda())
    assert_close(out.detach().float().cpu().numpy(), ref, rtol, 0, "out", scale_atol=atol)
    assert xc.grad.dtype == dtype
    assert_close(xc.grad.float().cpu().numpy(), ref_dxz, 2 * rtol, 0, "dxz", scale_atol=2 * atol)
    rtolw, atolw = max(1e-3, rtol), max(1e-3, atol)
    assert set(ref_g) == set(pc)
    for k, v in pc.items():
        assert_close(v.grad.float().cpu().numpy(), ref_g[k], rtolw, 0, "g_" + k, scale_atol=atolw)


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


@pytest.mark.parametrize("env", [{"DIMSUM_MAMBA_CHECKPOINT_LVL": "1"}, {"DIMSUM_RECOMPUTE_OUT_Z": "1"},
                                 {"DIMSUM_MAMBA_CHECKPOINT_LVL": "1", "DIMSUM_RECOMPUTE_OUT_Z": "1"}],
                         ids=["checkpoint_lvl1", "recompute_out_z", "both"])
def test_mixer_switches_match_the_default_path(env, monkeypatch):
    """the two documented switches change what _BiMambaInner saves (conv_out and delta dropped and recomputed in the backward / out_z dropped
    and recomputed by the scan backward) but not what it computes: output and every gradient bit for bit those of the default path. Batch 1,
    as in test_mixer_is_deterministic: the float atomics see one addend per address; and the level-1 conv recompute, written contiguous
    (b, d, l) where the forward wrote it d-major, has the same memory layout then, so its products take the same GEMM paths"""
    p = _mixer_params(256, 512, 16, 16, 4, biases=True, seed=4)
    xz = torch.randn(1, 1024, 512, generator=torch.Generator().manual_seed(5))
    dout = torch.randn(1, 512, 256, generator=torch.Generator().manual_seed(6)).cuda()

    def run():
        pc = {k: v.cuda().requires_grad_() for k, v in p.items()}
        xc = xz.cuda().requires_grad_()
        out = _call(xc, pc)
        saved = out.grad_fn.saved_tensors
        kept = (saved[7] is not None, saved[8] is not None, saved[-1] is not None)       # conv_out, delta, out_z
        out.backward(dout)
        return kept, [("out", out.detach()), ("dxz", xc.grad)] + [(k, pc[k].grad) for k in sorted(pc)]

    for k in env:
        monkeypatch.delenv(k, raising=False)
    kept, ref = run()
    assert kept == (True, True, True)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    kept, got = run()
    lvl1 = "DIMSUM_MAMBA_CHECKPOINT_LVL" in env
    assert kept == (not lvl1, not lvl1, "DIMSUM_RECOMPUTE_OUT_Z" not in env), kept
    for (name, a), (_, b) in zip(got, ref):
        assert torch.equal(a, b), f"{name}: max |diff| {(a - b).abs().max().item():.3e}"


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


# ---- kernel level at the launch-path edges: the pair vs the C oracle composed with flips ---------------------------------------------------
ROWS = ("du", "ddelta", "dB", "dC", "dz")

# (batch, dim, L, dstate, n_groups, forced forward kernel (0 = the library's choice), the kernel that serves it). Both directions take one
# launch path. Forward: "full" = vector I/O with every channel slot of every tile live, "vec" = vector I/O with a partial channel tile,
# "scalar" = element-wise (L % 4 != 0). Backward: the same three, full needing vec and dim / n_groups % 64 == 0. The dB / dC reduce: vec4 on
# 16-byte aligned buffers at L % 4 == 0 (the plain run), scalar otherwise (every mixer-layout run: its dB / dC start one float into their
# buffer). lanes = one lane per state, 64-ch = 64 channels per wave. In reversed time a partial chunk is the FIRST one in memory.
EDGE_CASES = [
    (2, 64, 1, 16, 1, 0, 16),       # lanes fwd scalar, L == 1; bwd scalar; reduce scalar
    (2, 64, 3, 8, 1, 0, 1),         # 64-ch fwd scalar, L < 4; bwd scalar; reduce scalar
    (1, 70, 5, 32, 1, 0, 1),        # 64-ch fwd scalar, masked channels, one 4-step group + 1; bwd scalar; reduce scalar
    (2, 64, 2048, 4, 1, 0, 1),      # 64-ch fwd full, exactly one chunk; bwd full; reduce vec4 / scalar
    (1, 64, 2052, 16, 1, 0, 16),    # lanes fwd full, partial 2nd chunk of 4 steps; bwd full; reduce vec4 / scalar
    (3, 128, 3000, 16, 1, 1, 1),    # 64-ch fwd full (forced), partial 2nd chunk; bwd full; reduce vec4 / scalar
    (2, 130, 2049, 8, 1, 0, 1),     # 64-ch fwd scalar, partial 2nd chunk of 1 step, masked channels; bwd scalar; reduce scalar
    (3, 128, 4100, 16, 1, 0, 16),   # lanes fwd full, 3 chunks, ragged; bwd full; reduce vec4 / scalar
    (2, 40, 4100, 32, 1, 0, 1),     # 64-ch fwd vec (40 of 64 channels), 3 chunks; bwd vec; reduce vec4 / scalar
    (2, 128, 300, 16, 2, 0, 16),    # lanes fwd full, 2 groups of 64 channels; bwd full; reduce vec4 / scalar
    (2, 96, 256, 8, 2, 0, 1),       # 64-ch fwd vec, 2 groups of 48 channels; bwd vec; reduce vec4 / scalar
    (2, 70, 256, 16, 1, 0, 16),     # lanes fwd vec (70 % 4 != 0); bwd vec; reduce vec4 / scalar
    (1, 36, 2051, 16, 1, 0, 16),    # lanes fwd scalar, partial 2nd chunk of 3 steps; bwd scalar; reduce scalar
]


def _edge_id(c):
    return "x".join(map(str, c[:4])) + (f"_g{c[4]}" if c[4] > 1 else "") + ("_forced64ch" if c[5] == 1 else "")


def _edge_values(b, d, L, N, G, seed=0, softplus=True):
    """the operands' values on the CPU (the oracle reads them; both GPU layouts are built from them)"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    ru = lambda *s: torch.rand(*s, generator=g)
    # without softplus delta is used as is: kept positive (a negative step makes exp(delta A) > 1)
    delta = 0.5 * ru(b, d, L) - 0.3 if softplus else 0.5 * ru(b, d, L) + 0.01
    return dict(u=rn(b, d, L), delta=delta, A=-0.5 * ru(d, N) - 0.05, A_b=-0.5 * ru(d, N) - 0.05, B=rn(b, G, N, L), C=rn(b, G, N, L),
                D=rn(d), z=rn(b, d, L), bias=0.5 * ru(d), dout=rn(b, d, L))


def _edge_plain(v, dtype=torch.float32):
    """contiguous operands on the GPU; u, delta, B, C, z, dout in `dtype`"""
    h = lambda t: t.to(dtype).cuda()
    return dict(u=h(v["u"]), delta=h(v["delta"]), A=v["A"].cuda(), A_b=v["A_b"].cuda(), B=h(v["B"]), C=h(v["C"]), D=v["D"].cuda(),
                z=h(v["z"]), bias=v["bias"].cuda(), dout=h(v["dout"]), dz=None, dB=None, dC=None)


def _edge_mixer(v):
    """the layouts _BiMambaInner hands the pair: u, z = halves of xz; delta and dout d-major; B, C rows of one (2 G N, b L) matrix; dz written
    into a NaN-filled dxz; dB / dC fp32 views whose rows start one float into their NaN-filled buffer (not 16-byte aligned)"""
    b, d, L = v["u"].shape
    G, N = v["B"].shape[1:3]
    xz = torch.cat([v["u"], v["z"]], 1).cuda()
    dm = lambda t: t.permute(1, 0, 2).contiguous().cuda().permute(1, 0, 2)
    bc = torch.stack([v["B"], v["C"]]).permute(0, 2, 3, 1, 4).contiguous().cuda()            # (2, G, N, b, L)
    dxz = torch.full_like(xz, float("nan"))
    n = b * G * N * L
    buf = torch.full((1 + 2 * n,), float("nan"), device="cuda")
    rows = lambda t: t.view(G, N, b, L).permute(2, 0, 1, 3)
    return dict(u=xz[:, :d], delta=dm(v["delta"]), A=v["A"].cuda(), A_b=v["A_b"].cuda(), B=rows(bc[0]), C=rows(bc[1]), D=v["D"].cuda(),
                z=xz[:, d:], bias=v["bias"].cuda(), dout=dm(v["dout"]), dz=dxz[:, d:], dB=rows(buf[1:1 + n]), dC=rows(buf[1 + n:]),
                dxz=dxz, buf=buf)


def _pair(o, D=True, bias=True, softplus=True, recompute=False):
    """the bidirectional pair on the operands of _edge_plain / _edge_mixer -> forward dict, backward dict, recomputed out_z (or None)"""
    from dimsum_amd import native
    Dv, bv = (o["D"] if D else None), (o["bias"] if bias else None)
    out, out_b, out_z, ck, ck_b = native.selective_scan_bidir_fwd(o["u"], o["delta"], o["A"], o["A_b"], o["B"], o["C"], Dv, o["z"], bv, softplus,
                                                                  need_out=True, need_ckpt=True)
    res = native.selective_scan_bidir_bwd(o["u"], o["delta"], o["A"], o["A_b"], o["B"], o["C"], Dv, o["z"], bv, o["dout"], out, out_b, ck, ck_b,
                                          softplus, recompute, dz=o["dz"], dB=o["dB"], dC=o["dC"])
    fwd = dict(out=out, out_b=out_b, out_z=out_z, ckpt=ck, ckpt_b=ck_b)
    bwd = dict(zip(("du", "ddelta", "dA", "dA_b", "dB", "dC", "dD", "ddelta_bias", "dz"), res[:9]))
    return fwd, bwd, (res[9] if recompute else None)


def _pair_composed(o, D=True, bias=True, softplus=True):
    """_composed with groups and optional operands; also returns the two halves of out_z, du, ddelta and dz (each in the I/O type)"""
    from dimsum_amd import native
    Dv, bv = (o["D"] if D else None), (o["bias"] if bias else None)
    u, delta, B, C, z = o["u"], o["delta"], o["B"], o["C"], o["z"]
    fu, fd, fB, fC, fz = _fl(u), _fl(delta), _fl(B), _fl(C), _fl(z)
    b, d, L = u.shape
    with native.scan_fwd_variant(native.scan_bidir_fwd_kernel_for(b, d, L, o["A"].shape[1], B.shape[1])):
        out_f, _, oz_f, ck_f = native.selective_scan_fwd(u, delta, o["A"], B, C, Dv, z, bv, softplus, need_x=False, need_ckpt=True)
        out_b, _, oz_b, ck_b = native.selective_scan_fwd(fu, fd, o["A_b"], fB, fC, Dv, fz, bv, softplus, need_x=False, need_ckpt=True)
    f = native.selective_scan_bwd(u, delta, o["A"], B, C, Dv, z, bv, o["dout"], None, out_f, None, softplus, False, ckpt=ck_f)
    r = native.selective_scan_bwd(fu, fd, o["A_b"], fB, fC, Dv, fz, bv, _fl(o["dout"]), None, out_b, None, softplus, False, ckpt=ck_b)
    halves = dict(out_z=(oz_f, oz_b.flip(-1)), du=(f[0], r[0].flip(-1)), ddelta=(f[1], r[1].flip(-1)), dz=(f[7], r[7].flip(-1)))
    fwd = dict(out=out_f, out_b=out_b.flip(-1), out_z=oz_f + oz_b.flip(-1), ckpt=ck_f, ckpt_b=ck_b)
    bwd = dict(du=f[0] + r[0].flip(-1), ddelta=f[1] + r[1].flip(-1), dA=f[2], dA_b=r[2], dB=f[3] + r[3].flip(-1), dC=f[4] + r[4].flip(-1),
               dD=None if f[5] is None else f[5] + r[5], ddelta_bias=None if f[6] is None else f[6] + r[6], dz=f[7] + r[7].flip(-1))
    return fwd, bwd, halves


def _pair_oracle(v, D=True, bias=True, softplus=True, cast=None):
    """the C oracle on the forward arrays (A) and on flipped copies (A_b), the second result flipped back, the two added in float64 (dA and
    dA_b apart, dD and ddelta_bias summed). `cast`: u, delta, B, C, z, dout rounded to that dtype first, as the half-precision runs see them"""
    from oracle import c_ops
    f32 = lambda t: np.ascontiguousarray(t.float().numpy())
    f = lambda t: f32(t if cast is None else t.to(cast))
    fl = lambda t: np.ascontiguousarray(f(t)[..., ::-1])
    A, A_b, Dv, bv = f32(v["A"]), f32(v["A_b"]), (f32(v["D"]) if D else None), (f32(v["bias"]) if bias else None)
    y_f, oz_f, _ = c_ops.selective_scan_fwd(f(v["u"]), f(v["delta"]), A, f(v["B"]), f(v["C"]), Dv, f(v["z"]), bv, softplus)
    y_b, oz_b, _ = c_ops.selective_scan_fwd(fl(v["u"]), fl(v["delta"]), A_b, fl(v["B"]), fl(v["C"]), Dv, fl(v["z"]), bv, softplus)
    rf = c_ops.selective_scan_bwd(f(v["u"]), f(v["delta"]), A, f(v["B"]), f(v["C"]), Dv, f(v["z"]), bv, softplus, f(v["dout"]))
    rb = c_ops.selective_scan_bwd(fl(v["u"]), fl(v["delta"]), A_b, fl(v["B"]), fl(v["C"]), Dv, fl(v["z"]), bv, softplus, fl(v["dout"]))
    d64 = lambda a: np.asarray(a, np.float64)
    back = lambda a: d64(a)[..., ::-1]
    fwd = dict(out=d64(y_f), out_b=back(y_b), out_z=d64(oz_f) + back(oz_b))
    bwd = {k: d64(rf[k]) + back(rb[k]) for k in ROWS}
    bwd.update(dA=d64(rf["dA"]), dA_b=d64(rb["dA"]), dD=d64(rf["dD"]) + d64(rb["dD"]), ddelta_bias=d64(rf["ddelta_bias"]) + d64(rb["ddelta_bias"]))
    return fwd, bwd


_EDGE_ORACLE = {}


def _edge_oracle(case):
    """one oracle run per case (the plain and the mixer-layout run of a case see the same values and run back to back)"""
    if case not in _EDGE_ORACLE:
        _EDGE_ORACLE.clear()
        _EDGE_ORACLE[case] = _pair_oracle(_edge_values(*case[:5]))
    return _EDGE_ORACLE[case]


def _check_vs_oracle(fwd, bwd, ref_fwd, ref_bwd, L, skip=()):
    n = lambda t: t.float().cpu().numpy()
    for k in ("out", "out_b", "out_z"):
        assert_close(n(fwd[k]), ref_fwd[k], what=k, **tol(L))
    for k in ROWS:
        assert_close(n(bwd[k]), ref_bwd[k], what=k, **_bwd_tol(L))
    for k in ATOMIC:
        if k not in skip:
            assert_close(n(bwd[k]), ref_bwd[k], what=k, **_bwd_tol(L, True))


@pytest.mark.parametrize("layout", ["plain", "mixer"])
@pytest.mark.parametrize("case", EDGE_CASES, ids=_edge_id)
def test_kernel_vs_oracle_at_edges(case, layout):
    """out, out_b, out_z and every gradient against the oracle. plain: contiguous operands, fresh (aligned) dB / dC; the inference launch (no
    out, no saved states) must give the training launch's out_z bit for bit, and the backward's recomputed out_z is checked. mixer: d-major
    delta / dout, B / C rows of one matrix, dz into a NaN-filled dxz (its x half stays NaN), dB / dC one float into their buffer (the
    scalar reduce at any L; the float before them stays NaN)"""
    from dimsum_amd import native
    b, d, L, N, G, force, want = case
    ref_fwd, ref_bwd = _edge_oracle(case)
    v = _edge_values(b, d, L, N, G)
    with native.scan_fwd_variant(force):
        assert native.scan_bidir_fwd_kernel_for(b, d, L, N, G) == want
        o = _edge_plain(v) if layout == "plain" else _edge_mixer(v)
        fwd, bwd, oz = _pair(o, recompute=layout == "plain")
        if layout == "plain":
            inf = native.selective_scan_bidir_fwd(o["u"], o["delta"], o["A"], o["A_b"], o["B"], o["C"], o["D"], o["z"], o["bias"], True,
                                                  need_out=False, need_ckpt=False)
    torch.cuda.synchronize()
    _check_vs_oracle(fwd, bwd, ref_fwd, ref_bwd, L)
    if layout == "plain":
        assert inf[0] is None and inf[1] is None and torch.equal(inf[2], fwd["out_z"]), "inference launch out_z"
        assert (oz - fwd["out_z"]).abs().max().item() <= 1e-6 * fwd["out_z"].abs().max().item(), "recomputed out_z"
    else:
        assert bwd["dz"].data_ptr() == o["dz"].data_ptr() and bwd["dB"].data_ptr() == o["dB"].data_ptr() == o["buf"].data_ptr() + 4
        assert torch.isnan(o["dxz"][:, :d]).all(), "dz wrote outside its half of dxz"
        assert torch.isnan(o["buf"][0]), "dB wrote before its first element"


@pytest.mark.parametrize("opt", [dict(D=False), dict(bias=False), dict(softplus=False)], ids=["no_D", "no_delta_bias", "no_softplus"])
@pytest.mark.parametrize("case", [(2, 70, 300, 16, 1, 0, 16), (2, 96, 300, 8, 1, 0, 1)], ids=_edge_id)
def test_kernel_optional_operands_vs_oracle(case, opt):
    """D, delta_bias, softplus off one at a time, on each forward kernel (one lane per state; 64 channels per wave): against the oracle, and
    bitwise against the composition"""
    from dimsum_amd import native
    b, d, L, N, G, force, want = case
    assert native.scan_bidir_fwd_kernel_for(b, d, L, N, G) == want
    v = _edge_values(b, d, L, N, G, seed=1, softplus=opt.get("softplus", True))
    ref_fwd, ref_bwd = _pair_oracle(v, **opt)
    o = _edge_plain(v)
    fwd, bwd, _ = _pair(o, **opt)
    cfwd, cbwd, _ = _pair_composed(o, **opt)
    torch.cuda.synchronize()
    skip = (("dD",) if not opt.get("D", True) else ()) + (("ddelta_bias",) if not opt.get("bias", True) else ())
    for k in skip:
        assert bwd[k] is None, k
    _check_vs_oracle(fwd, bwd, ref_fwd, ref_bwd, L, skip)
    for k in ("out", "out_b", "out_z", "ckpt", "ckpt_b"):
        assert torch.equal(fwd[k], cfwd[k]), k
    for k in ROWS:
        assert torch.equal(bwd[k], cbwd[k]), k


@pytest.mark.parametrize("case", EDGE_CASES, ids=_edge_id)
def test_kernel_vs_flipped_composition_at_edges(case):
    """test_kernel_vs_flipped_composition at the edge shapes, mixer layout (unaligned dB / dC: the reversed scalar reduce at every L): outputs,
    BOTH directions' saved states (which the oracle cannot see) and the non-atomic gradients bit for bit"""
    from dimsum_amd import native
    b, d, L, N, G, force, want = case
    v = _edge_values(b, d, L, N, G, seed=2)
    with native.scan_fwd_variant(force):
        o = _edge_mixer(v)
        fwd, bwd, _ = _pair(o)
        cfwd, cbwd, _ = _pair_composed(o)
    torch.cuda.synchronize()
    for k, t in fwd.items():
        assert torch.equal(t, cfwd[k]), f"{k}: max |diff| {(t - cfwd[k]).abs().max().item():.3e}"
    for k, t in bwd.items():
        if k in ATOMIC:
            assert (t - cbwd[k]).abs().max().item() <= 1e-5 * cbwd[k].abs().max().item(), k
        else:
            assert torch.equal(t, cbwd[k]), f"{k}: max |diff| {(t - cbwd[k]).abs().max().item():.3e}"


HALF = [(torch.float16, 6e-3, 10), (torch.bfloat16, 4e-2, 7)]
HALF_CASES = [(2, 96, 512, 16, 1, 0, 16),      # one chunk: lanes fwd full, bwd vec
              (1, 64, 4100, 8, 1, 0, 1)]       # 3 chunks, ragged: 64-ch fwd full, bwd full


@pytest.mark.parametrize("dtype,tol_rel,p", HALF, ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", HALF_CASES, ids=_edge_id)
def test_kernel_half_dtypes_vs_oracle(case, dtype, tol_rel, p):
    """16-bit u, delta, B, C, z, dout (fp32 A, A_b, D, delta_bias) against the oracle on the same rounded values: every output and gradient
    within 1.5 tol_rel max|ref| (the bound of test_bwd_half_dtypes: the backward also sees its forward's `out` rounded to the I/O type)"""
    from dimsum_amd import native
    b, d, L, N, G, force, want = case
    assert native.scan_bidir_fwd_kernel_for(b, d, L, N, G) == want
    v = _edge_values(b, d, L, N, G, seed=3)
    ref_fwd, ref_bwd = _pair_oracle(v, cast=dtype)
    fwd, bwd, _ = _pair(_edge_plain(v, dtype))
    torch.cuda.synchronize()
    assert fwd["out_z"].dtype == dtype and bwd["du"].dtype == dtype and bwd["dB"].dtype == dtype
    got = dict(out=fwd["out"], out_b=fwd["out_b"], out_z=fwd["out_z"], **bwd)
    for k, t in got.items():
        ref = ref_fwd[k] if k in ref_fwd else ref_bwd[k]
        err, scale = np.abs(t.float().cpu().numpy() - ref).max(), np.abs(ref).max()
        assert err <= 1.5 * tol_rel * scale, (k, err, scale)


@pytest.mark.parametrize("dtype,tol_rel,p", HALF, ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", HALF_CASES, ids=_edge_id)
def test_kernel_half_dtypes_accumulation_rule(case, dtype, tol_rel, p):
    """the pair in fp16 / bf16 against the composition in the same dtype. The forward direction's half is stored rounded to the I/O type; the
    reversed direction adds its UNROUNDED fp32 half to it and rounds once (the composition rounds both halves, then their sum) -- so only
    fp32 is bitwise. Elementwise |fused - composed| <= 2^-p (|forward half| + |reversed half|): one unit in the last place of the result
    (p = 10 fp16, 7 bf16; plus one ulp of the subnormal range) for out_z, du, ddelta and dz. out, out_b and the saved states (one direction
    each) stay bitwise."""
    b, d, L, N, G, force, want = case
    o = _edge_plain(_edge_values(b, d, L, N, G, seed=4), dtype)
    fwd, bwd, _ = _pair(o)
    cfwd, cbwd, halves = _pair_composed(o)
    torch.cuda.synchronize()
    for k in ("out", "out_b", "ckpt", "ckpt_b"):
        assert torch.equal(fwd[k], cfwd[k]), k
    floor = torch.finfo(dtype).tiny * 2.0 ** -p
    for k in ("out_z", "du", "ddelta", "dz"):
        got = (fwd[k] if k == "out_z" else bwd[k]).float()
        ref = (cfwd[k] if k == "out_z" else cbwd[k]).float()
        hf, hr = (h.float() for h in halves[k])
        excess = ((got - ref).abs() - (2.0 ** -p * (hf.abs() + hr.abs()) + floor)).max().item()
        assert excess <= 0, (k, excess)
