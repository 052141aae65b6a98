#!/usr/bin/env python3
"""Generate golden fixtures under tests/golden/ by importing the REFERENCE (read-only, /root/reference) with the
shims of tools/ref_shim.py. Runs in the build container only; the fixtures (data: inputs + expected outputs) are
committed, the reference never travels. Re-run:  python tools/gen_golden.py [--only NAME ...]

Every fixture records which reference function produced it (file:line) in its `__doc__` field.
Inputs follow the reference tests' distributions (mamba/tests/ops/test_selective_scan.py:62-95,
causal-conv1d/tests/test_causal_conv1d.py:39-49).
"""
import argparse
import hashlib
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
warnings.filterwarnings("ignore", category=FutureWarning)

import ref_shim  # noqa: E402
from procedural import procedural_fill, seeded, toy_denoiser  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
T = torch.from_numpy


def save(name, doc, **arrs):
    path = os.path.join(OUT, name + ".npz")
    conv = {}
    for k, v in arrs.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        conv[k] = np.asarray(v)
    np.savez_compressed(path, __doc__=np.array(doc), **conv)
    print(f"  wrote {name}.npz  {os.path.getsize(path)/1024:.0f} KiB")


# ---------------------------------------------------------------------------------------------------------------
def gen_scan(ns):
    """selective_scan_ref fwd + autograd grads (selective_scan_interface.py:104-171)."""
    cases = {
        # name: (B, D, L, N, has_D, has_z, has_bias, softplus, groups)
        "scan_main": (2, 72, 256, 16, True, True, True, True, 1),
        "scan_long": (1, 8, 4096, 16, True, True, True, True, 1),
        "scan_odd": (2, 5, 151, 8, True, True, True, True, 1),
        "scan_plain": (2, 4, 64, 8, False, False, False, False, 1),
        "scan_nosoftplus_z": (2, 4, 128, 8, True, True, False, False, 1),
        "scan_groups2": (2, 4, 128, 8, True, True, True, True, 2),
    }
    for name, (B, D, L, N, has_D, has_z, has_b, sp, G) in cases.items():
        torch.manual_seed(0)
        A = (-0.5 * torch.rand(D, N)).requires_grad_()
        Bm = torch.randn(B, G, N, L, requires_grad=True)
        Cm = torch.randn(B, G, N, L, requires_grad=True)
        Dv = torch.randn(D, requires_grad=True) if has_D else None
        z = torch.randn(B, D, L, requires_grad=True) if has_z else None
        db = (0.5 * torch.rand(D)).requires_grad_() if has_b else None
        u = torch.randn(B, D, L, requires_grad=True)
        delta = (0.5 * torch.rand(B, D, L)).requires_grad_()
        out, last = ns.ssi.selective_scan_ref(u, delta, A, Bm, Cm, Dv, z, db, sp, return_last_state=True)
        g = torch.randn_like(out)
        out.backward(g)
        # `out` before gating (the CUDA kernel's first output) = ref without z
        with torch.no_grad():
            y = ns.ssi.selective_scan_ref(u, delta, A, Bm, Cm, Dv, None, db, sp)
        arrs = dict(u=u, delta=delta, A=A, B=Bm, C=Cm, dout=g, out=out, y=y, last_state=last,
                    du=u.grad, ddelta=delta.grad, dA=A.grad, dB=Bm.grad, dC=Cm.grad,
                    softplus=np.array(sp))
        if has_D:
            arrs.update(D=Dv, dD=Dv.grad)
        if has_z:
            arrs.update(z=z, dz=z.grad)
        if has_b:
            arrs.update(delta_bias=db, ddelta_bias=db.grad)
        save(name, "selective_scan_ref fwd + autograd (mamba/mamba_ssm/ops/selective_scan_interface.py:104-171); "
             "distributions of mamba/tests/ops/test_selective_scan.py:62-95", **arrs)


def gen_scan_general(ns):
    """selective_scan_ref in float64 / complex128 over the axes of mamba/tests/ops/test_selective_scan.py (is_variable_B, is_variable_C, real /
    complex weights) at state sizes the tuned kernels do not take: forward, last state and autograd gradients."""
    cases = {
        # name: (B, D, L, N, complex, variable B, variable C, groups, has_D, has_z, has_bias, softplus)
        "scang_real_vv_n12": (2, 6, 21, 12, False, True, True, 2, True, True, True, True),
        "scang_real_cv_n3": (2, 5, 19, 3, False, False, True, 1, True, False, True, True),
        "scang_real_cc_n20": (1, 4, 17, 20, False, False, False, 1, False, True, False, False),
        "scang_cplx_vv_n5": (2, 6, 21, 5, True, True, True, 2, True, True, True, True),
        "scang_cplx_vc_n12": (2, 5, 19, 12, True, True, False, 1, True, True, False, True),
        "scang_cplx_cc_n3": (1, 4, 17, 3, True, False, False, 1, False, False, True, False),
    }
    f8 = torch.float64
    for name, (B, D, L, N, cplx, vB, vC, G, has_D, has_z, has_b, sp) in cases.items():
        torch.manual_seed(0)
        wdt = torch.complex128 if cplx else f8
        A = -0.5 * torch.rand(D, N, dtype=f8)
        A = (A + 1j * torch.randn(D, N, dtype=f8) if cplx else A).requires_grad_()
        Bm = (torch.randn(B, G, N, L * (2 if cplx else 1), dtype=f8) if vB else torch.randn(D, N, dtype=wdt)).requires_grad_()
        Cm = (torch.randn(B, G, N, L * (2 if cplx else 1), dtype=f8) if vC else torch.randn(D, N, dtype=wdt)).requires_grad_()
        Dv = torch.randn(D, dtype=f8, requires_grad=True) if has_D else None
        z = torch.randn(B, D, L, dtype=f8, requires_grad=True) if has_z else None
        db = (0.5 * torch.rand(D, dtype=f8)).requires_grad_() if has_b else None
        u = torch.randn(B, D, L, dtype=f8, requires_grad=True)
        delta = (0.5 * torch.rand(B, D, L, dtype=f8)).requires_grad_()
        # selective_scan_ref works in float32 (`.float()`); the float64 run goes through a module copy whose Tensor.float is the identity
        out, last = ref_shim.in_float64(ns.ssi.selective_scan_ref, u, delta, A, Bm, Cm, Dv, z, db, sp, return_last_state=True)
        assert out.dtype == f8
        g = torch.randn_like(out)
        out.backward(g)
        arrs = dict(u=u, delta=delta, A=A, B=Bm, C=Cm, dout=g, out=out, last_state=last, du=u.grad, ddelta=delta.grad, dA=A.grad, dB=Bm.grad,
                    dC=Cm.grad, softplus=np.array(sp))
        if has_D:
            arrs.update(D=Dv, dD=Dv.grad)
        if has_z:
            arrs.update(z=z, dz=z.grad)
        if has_b:
            arrs.update(delta_bias=db, ddelta_bias=db.grad)
        save(name, "selective_scan_ref fwd + autograd in float64 / complex128 (mamba/mamba_ssm/ops/selective_scan_interface.py:104-171)", **arrs)


def gen_conv(ns):
    """causal_conv1d_ref fwd + autograd (causal_conv1d_interface.py:48-64)."""
    cases = {
        "conv_L8_w4_silu": (2, 72, 8, 4, True, True),
        "conv_L151_w4_silu": (2, 72, 151, 4, True, True),
        "conv_L256_w4_silu": (2, 72, 256, 4, True, True),
        "conv_L1134_w4_silu": (2, 8, 1134, 4, True, True),
        "conv_L256_w3_nosilu": (2, 8, 256, 3, False, True),
        "conv_L64_w2_nobias": (2, 8, 64, 2, True, False),
        "conv_L4096_w4_silu": (1, 4, 4096, 4, True, True),
    }
    for name, (B, D, L, W, silu, has_bias) in cases.items():
        torch.manual_seed(0)
        # strided view, like test_causal_conv1d.py:39-49 and like x = xz.chunk(2,1)[0]
        xz = torch.randn(B, 2 * D, L)
        x = xz[:, :D].detach().clone().requires_grad_()
        w = torch.randn(D, W, requires_grad=True)
        b = torch.randn(D, requires_grad=True) if has_bias else None
        out = ns.cci.causal_conv1d_ref(x, w, b, "silu" if silu else None)
        g = torch.randn_like(out)
        out.backward(g)
        arrs = dict(x=x, weight=w, dout=g, out=out, dx=x.grad, dweight=w.grad, silu=np.array(silu))
        if has_bias:
            arrs.update(bias=b, dbias=b.grad)
        save(name, "causal_conv1d_ref fwd + autograd (causal-conv1d/causal_conv1d/causal_conv1d_interface.py:48-64)",
             **arrs)


def gen_norm(ns):
    """rms_norm_ref / layer_norm_ref (ops/triton/layernorm.py:19-45), upcast=True, prenorm."""
    for name, (M, N, has_res, is_rms) in {
        "rmsnorm_prenorm_res": (24, 1024, True, True),
        "rmsnorm_prenorm_nores": (33, 384, False, True),
        "rmsnorm_odd": (7, 200, True, True),
        "layernorm_prenorm_res": (16, 256, True, False),
    }.items():
        torch.manual_seed(0)
        x = torch.randn(M, N, requires_grad=True)
        res = torch.randn(M, N, requires_grad=True) if has_res else None
        w = (1 + 0.1 * torch.randn(N)).requires_grad_()
        b = (0.1 * torch.randn(N)).requires_grad_() if not is_rms else None
        fn = ns.ln.rms_norm_ref if is_rms else ns.ln.layer_norm_ref
        y, res_out = fn(x, w, b, residual=res, eps=1e-5, prenorm=True, upcast=True)
        gy, gr = torch.randn_like(y), torch.randn_like(res_out)
        (y * gy).sum().add((res_out * gr).sum()).backward()
        arrs = dict(x=x, weight=w, y=y, res_out=res_out, dy=gy, dres_out=gr, dx=x.grad, dweight=w.grad,
                    eps=np.array(1e-5))
        if has_res:
            arrs.update(residual=res, dresidual=res.grad)
        if b is not None:
            arrs.update(bias=b, dbias=b.grad)
        save(name, "rms_norm_ref/layer_norm_ref prenorm, upcast (mamba/mamba_ssm/ops/triton/layernorm.py:19-45)", **arrs)


def gen_perm(ns):
    """SCAN_ZOO tables + inverses (dimsum/scanning_orders.py:7-253,419-423) and block-level reorders."""
    so = ns.scanning_orders
    arrs, shas = {}, {}
    for kind in ("sweep", "zigma", "jpeg"):
        for N in (4, 8, 16, 32):
            paths = np.stack(so.SCAN_ZOO[kind](N)).astype(np.int64)
            inv = np.stack([so.reverse_permut_np(p) for p in paths]).astype(np.int64)
            arrs[f"{kind}{N}"] = paths.astype(np.int16)
            arrs[f"{kind}{N}_inv"] = inv.astype(np.int16)
            shas[f"{kind}{N}"] = hashlib.sha256(paths.tobytes()).hexdigest()[:16]
    for k, v in shas.items():
        arrs["sha_" + k] = np.array(v)
    # local_scan / local_reverse (scanning_orders.py:347-367,393-416) as index tables
    for (H, w) in ((4, 2), (16, 4), (32, 8), (8, 2)):
        L = H * H
        ids = torch.arange(L, dtype=torch.float32).view(1, L, 1)
        for cf in (False, True):
            p = so.local_scan(ids.clone(), w=w, H=H, W=H, column_first=cf).view(-1).long()
            back = so.local_reverse(p.view(1, L, 1).float(), w=w, H=H, W=H, column_first=cf).view(-1).long()
            assert torch.equal(back, torch.arange(L))
            arrs[f"local_H{H}_w{w}_{'col' if cf else 'row'}"] = p.numpy().astype(np.int16)
    save("perm_tables", "SCAN_ZOO[...](N), reverse_permut_np, local_scan (dimsum/scanning_orders.py)", **arrs)


def _block_order(ns, reverse, transpose, cont, H):
    """Order seen by the mixer inside DiMBlockRaw.forward (models_dim.py:1496-1507)."""
    from einops import rearrange
    L = H * H
    hs = torch.arange(L, dtype=torch.float32).view(1, L, 1)
    if transpose:
        hs = rearrange(hs, "n (h w) c -> n (w h) c", h=H, w=H)
    if cont:
        hs = rearrange(hs.clone(), "n (w h) c -> n c w h", h=H, w=H)
        hs[:, :, 1::2] = hs[:, :, 1::2].flip(-1)
        hs = rearrange(hs, "n c w h -> n (w h) c", h=H, w=H)
    if reverse:
        hs = hs.flip(1)
    return hs.view(-1).long().numpy()


def gen_block_orders(ns):
    arrs = {}
    for H in (4, 16, 32):
        for r in (0, 1):
            for t in (0, 1):
                for c in (0, 1):
                    arrs[f"H{H}_r{r}_t{t}_c{c}"] = _block_order(ns, r, t, c, H).astype(np.int16)
    save("block_orders", "token order seen by the mixer, DiMBlockRaw.forward (dimsum/models_dim.py:1496-1507)", **arrs)


def gen_wavelet_dct(ns):
    md = ns.models_dim
    blk = md.WaveDiMBlock.__new__(md.WaveDiMBlock)
    torch.nn.Module.__init__(blk)
    blk.num_wavelet_lv = 2
    blk.dwt = ns.wavelet_layer.DWT_2D("haar")
    blk.idwt = ns.wavelet_layer.IDWT_2D("haar")
    arrs = {}
    for (H, C) in ((16, 8), (32, 4), (4, 3)):
        x = T(seeded((2, H * H, C), 11 + H)).requires_grad_()
        y = blk._dwt_fast(x)
        g = T(seeded(tuple(y.shape), 12 + H))
        y.backward(g)
        xr = blk._idwt_fast(y.detach())
        y2 = T(seeded((2, H * H, C), 13 + H)).requires_grad_()
        xi = blk._idwt_fast(y2)
        gi = T(seeded(tuple(xi.shape), 14 + H))
        xi.backward(gi)
        arrs.update({f"H{H}_x": x, f"H{H}_dwt": y, f"H{H}_dwt_g": g, f"H{H}_dwt_dx": x.grad, f"H{H}_roundtrip": xr,
                     f"H{H}_y2": y2, f"H{H}_idwt": xi, f"H{H}_idwt_g": gi, f"H{H}_idwt_dy": y2.grad})
    # the equivalent 16x16 per-4x4-block matrix: apply to unit impulses
    eye = torch.zeros(16, 16, 1)
    for i in range(16):
        eye[i, i, 0] = 1.0
    arrs["haar4x4_matrix"] = blk._dwt_fast(eye)[:, :, 0].t().contiguous()  # out = M @ in  (index = 4*row+col in tile)
    save("haar", "WaveDiMBlock._dwt_fast/_idwt_fast (dimsum/models_dim.py:572-604) over DWT_2D/IDWT_2D "
         "(dimsum/wavelet_layer.py:7-115)", **arrs)

    # DCT: dct_conv + rearrange / rearrange + idct_conv (models_dim.py:876-882, 919-928)
    from einops import rearrange
    arrs = {}
    for (H, C) in ((16, 8), (32, 4)):
        dct = ns.dct_layer.init_dct_kernel(C, 4, 4)
        idct = torch.nn.Sequential(ns.dct_layer.init_idct_kernel(C, 4, 4), torch.nn.PixelShuffle(4))
        x = T(seeded((2, H * H, C), 21 + H))
        h = rearrange(x, "b (h w) d -> b d h w", h=H)
        h = dct(h)
        h = rearrange(h, "b (c p1 p2) h w -> b (h p1 w p2) c", c=C, p1=4).contiguous()
        h2 = rearrange(h, "b (h p1 w p2) c -> b (c p1 p2) h w", c=C, p1=4, p2=4, h=H // 4).contiguous()
        back = rearrange(idct(h2), "b c h w -> b (h w) c")
        arrs.update({f"H{H}_x": x, f"H{H}_dct": h, f"H{H}_roundtrip": back})
        if H == 16:
            arrs["dct_weight_1ch"] = dct.weight[:16].detach()
            arrs["idct_weight_1ch"] = idct[0].weight[:16].detach()
    save("dct", "DCTBlock 4x4 DCT/IDCT path (dimsum/models_dim.py:876-882,919-928; dimsum/dct_layer.py:6-84)", **arrs)


def gen_fusion(ns):
    torch.manual_seed(0)
    for name, (B, L, dim) in {"fusion_128": (2, 256, 128), "fusion_hd24": (2, 64, 384)}.items():
        m = ns.attention_fusion.CrossAttentionFusion(dim, num_heads=8, qkv_bias=True, swap_k=False)
        procedural_fill(m, seed=5)
        x1 = T(seeded((B, L, dim // 2), 31)).requires_grad_()
        x2 = T(seeded((B, L, dim // 2), 32)).requires_grad_()
        y = m(x1, x2)
        g = T(seeded(tuple(y.shape), 33))
        y.backward(g)
        save(name, "CrossAttentionFusion.forward (dimsum/attention_fusion.py:61-84), procedural weights seed 5",
             x1=x1, x2=x2, y=y, dy=g, dx1=x1.grad, dx2=x2.grad,
             **{"g_" + k: v.grad for k, v in m.named_parameters()})


def gen_inner(ns):
    """mamba_inner_ref (selective_scan_interface.py:1455-1500) fwd + autograd, routed to the reference's own refs."""
    torch.manual_seed(0)
    B, Dm, L, N, W = 2, 48, 96, 16, 4
    D = 2 * Dm
    R = 3
    xz = torch.randn(B, 2 * D, L, requires_grad=True)
    p = dict(
        conv_w=torch.randn(D, 1, W) * 0.5, conv_b=torch.randn(D) * 0.1,
        x_proj_w=torch.randn(R + 2 * N, D) / D ** 0.5, dt_proj_w=torch.randn(D, R) / R ** 0.5,
        out_proj_w=torch.randn(Dm, D) / D ** 0.5, A=-torch.exp(torch.log(torch.arange(1, N + 1).float()).repeat(D, 1)
                                                           + 0.1 * torch.randn(D, N)),
        Dv=1 + 0.1 * torch.randn(D), dt_bias=torch.randn(D) * 0.5 - 4.0,
    )
    for v in p.values():
        v.requires_grad_()
    out = ns.ssi.mamba_inner_ref(xz, p["conv_w"], p["conv_b"], p["x_proj_w"], p["dt_proj_w"], p["out_proj_w"], None,
                                 p["A"], None, None, p["Dv"], delta_bias=p["dt_bias"], delta_softplus=True)
    g = torch.randn_like(out)
    out.backward(g)
    save("mamba_inner", "mamba_inner_ref fwd+autograd (mamba/mamba_ssm/ops/selective_scan_interface.py:1455-1500)",
         xz=xz, out=out, dout=g, dxz=xz.grad, **{k: v for k, v in p.items()},
         **{"g_" + k: v.grad for k, v in p.items()})


def gen_bimamba(ns):
    """bimamba_inner_ref (selective_scan_interface.py:1503-1561) fwd + autograd (the true derivative: BiMambaInnerFn.backward drops the
    reversed direction's dz), routed to the reference's own refs. Case 1: width 4, dstate 16, dt_rank 3, out_proj / B / C proj biases;
    case 2: the reference test's width 3, dstate 8, dt_rank 48 (test_selective_scan.py:312-396) at a smaller dim."""
    for name, (B, Dm, L, N, W, R, biases, seed) in {
        "bimamba_w4_n16": (2, 48, 96, 16, 4, 3, True, 0),
        "bimamba_w3_n8": (2, 64, 77, 8, 3, 48, False, 1),
    }.items():
        torch.manual_seed(seed)
        D = 2 * Dm
        xz = torch.randn(B, 2 * D, L, requires_grad=True)
        p = dict(
            conv_w=torch.randn(D, 1, W) * 0.5, conv_b=torch.randn(D) * 0.1,
            x_proj_w=torch.randn(R + 2 * N, D) / D ** 0.5, dt_proj_w=torch.randn(D, R) / R ** 0.5,
            out_proj_w=torch.randn(Dm, D) / D ** 0.5,
            A=-torch.exp(torch.log(torch.arange(1, N + 1).float()).repeat(D, 1) + 0.1 * torch.randn(D, N)),
            A_b=-torch.exp(torch.log(torch.arange(1, N + 1).float()).repeat(D, 1) + 0.1 * torch.randn(D, N)),
            Dv=1 + 0.1 * torch.randn(D), dt_bias=torch.randn(D) * 0.5 - 4.0,
        )
        if biases:
            p.update(out_proj_b=0.1 * torch.randn(Dm), B_proj_b=0.1 * torch.randn(N), C_proj_b=0.1 * torch.randn(N))
        for v in p.values():
            v.requires_grad_()
        out = ns.ssi.bimamba_inner_ref(xz, p["conv_w"], p["conv_b"], p["x_proj_w"], p["dt_proj_w"], p["out_proj_w"], p.get("out_proj_b"),
                                       p["A"], p["A_b"], None, None, p["Dv"], delta_bias=p["dt_bias"], B_proj_bias=p.get("B_proj_b"),
                                       C_proj_bias=p.get("C_proj_b"), delta_softplus=True)
        g = torch.randn_like(out)
        out.backward(g)
        save(name, "bimamba_inner_ref fwd+autograd (mamba/mamba_ssm/ops/selective_scan_interface.py:1503-1561)",
             xz=xz, out=out, dout=g, dxz=xz.grad, **{k: v for k, v in p.items()},
             **{"g_" + k: v.grad for k, v in p.items()})


def gen_mixer(ns):
    """CondMamba / Mamba slow path (mamba_simple.py:562-701) incl. the zigzag gather semantics of :627-657."""
    for name, kw in {
        "condmamba_none": dict(cls="CondMamba", scan_type="none"),
        "mamba_none": dict(cls="Mamba", scan_type="none"),
        "condmamba_zigma8": dict(cls="CondMamba", scan_type="zigma_8"),
        "condmamba_v2": dict(cls="CondMamba", scan_type="v2"),
    }.items():
        d_model, L, B, H = 32, 64, 2, 8
        extra = {}
        if kw["scan_type"].startswith("zigma"):
            so = ns.scanning_orders
            paths = so.SCAN_ZOO["zigma"](H)[:8]
            extra["zigzag_paths"] = torch.stack([T(p) for p in paths])
            extra["zigzag_paths_reverse"] = torch.stack([T(so.reverse_permut_np(p)) for p in paths])
        cls = getattr(ns.ms, kw["cls"])
        ckw = dict(layer_idx=3, scan_type=kw["scan_type"], **extra)
        if kw["cls"] == "CondMamba":
            ckw["d_cond"] = 48
        m = cls(d_model, **ckw)
        procedural_fill(m, seed=7)
        x = T(seeded((B, L, d_model), 41)).requires_grad_()
        c = T(seeded((B, 48), 42))
        if kw["scan_type"] == "v2":    # the reference's own fast-path code (:593-625) over its *_ref ops
            ref_shim.route_no_out_proj_to_refs(ns)
            assert m.use_fast_path
        else:
            m.use_fast_path = False
            ref_shim.slow_path(m)      # wraps the zigzag gather around the slow path (mamba_simple.py:627-657)
        y = m(x, c) if kw["cls"] == "CondMamba" else m(x)
        g = T(seeded(tuple(y.shape), 43))
        y.backward(g)
        save(name, "CondMamba/Mamba.forward slow path (mamba/mamba_ssm/modules/mamba_simple.py:562-701); zigzag per "
             ":627-657; procedural weights seed 7", x=x, c=c, y=y, dy=g, dx=x.grad,
             **{"g_" + k: v.grad for k, v in m.named_parameters() if v.grad is not None})


STEP_CONV_CASES = ((2, 5, 2), (2, 5, 3), (3, 65, 4))              # (B, D, W)
STEP_SSU_CASES = ((2, 5, 1), (2, 65, 16), (1, 7, 64))             # (B, D, N)
STEP_MIXER = dict(d_model=32, d_state=16, d_conv=4, expand=2)     # B = 2, 12 tokens: 5 as a prompt, 7 steps
STEP_B, STEP_L, STEP_PREFILL = 2, 12, 5


def gen_step(ns):
    """the recurrent form: causal_conv1d_update_ref (causal_conv1d_interface.py:79-100), selective_state_update_ref
    (ops/triton/selective_state_update.py:193-228), Mamba / CondMamba forward(inference_params=...) + step (mamba_simple.py:162-380, :562-784)"""
    import dataclasses
    from mamba_ssm.ops.triton.selective_state_update import selective_state_update_ref as ssu_ref      # (plain torch + einops)
    arrs = {}
    for B, D, W in STEP_CONV_CASES:
        for has_bias in (False, True):
            for silu in (False, True):
                torch.manual_seed(0)        # distributions of causal-conv1d/tests/test_causal_conv1d.py:101-108
                x, state, w = torch.randn(B, D), torch.randn(B, D, W), torch.randn(D, W)
                b = torch.randn(D) if has_bias else None
                tag = f"conv_B{B}D{D}W{W}_b{int(has_bias)}s{int(silu)}_"
                arrs.update({tag + "x": x, tag + "state_in": state.clone(), tag + "weight": w})
                if has_bias:
                    arrs[tag + "bias"] = b
                arrs[tag + "out"] = ns.cci.causal_conv1d_update_ref(x, state, w, b, "silu" if silu else None)
                arrs[tag + "state_out"] = state
    for B, D, N in STEP_SSU_CASES:
        for has_z in (False, True):
            for has_D in (False, True):
                torch.manual_seed(0)        # distributions of mamba/tests/ops/triton/test_selective_state_update.py:24-36
                state, x, dt = torch.randn(B, D, N), torch.randn(B, D), torch.randn(B, D)
                dt_bias, A = torch.rand(D) - 4.0, -torch.rand(D, N) - 1.0
                Bm, Cm, Dv, z = torch.randn(B, N), torch.randn(B, N), torch.randn(D), torch.randn(B, D)
                tag = f"ssu_B{B}D{D}N{N}_z{int(has_z)}d{int(has_D)}_"
                arrs.update({tag + "state_in": state.clone(), tag + "x": x, tag + "dt": dt, tag + "dt_bias": dt_bias, tag + "A": A,
                             tag + "B": Bm, tag + "C": Cm})
                if has_D:
                    arrs[tag + "D"] = Dv
                if has_z:
                    arrs[tag + "z"] = z
                arrs[tag + "out"] = ssu_ref(state, x, dt, A, Bm, Cm, D=Dv if has_D else None, z=z if has_z else None, dt_bias=dt_bias,
                                            dt_softplus=True)
                arrs[tag + "state_out"] = state

    @dataclasses.dataclass
    class Params:       # the fields of mamba_ssm/utils/generation.py:12-21 that the mixers read
        max_seqlen: int
        max_batch_size: int
        seqlen_offset: int = 0
        key_value_memory_dict: dict = dataclasses.field(default_factory=dict)

    # the step's two operators as their own *_ref functions (the module's inline fallbacks, :306-312 / :329-337, are the same arithmetic)
    ns.ms.causal_conv1d_update = ns.cci.causal_conv1d_update_ref
    ns.ms.selective_state_update = ssu_ref
    for cls in ("Mamba", "CondMamba"):
        kw = dict(STEP_MIXER, layer_idx=3, scan_type="none", **({"d_cond": 48} if cls == "CondMamba" else {}))
        m = getattr(ns.ms, cls)(**kw)
        procedural_fill(m, seed=7)
        m.use_fast_path = False
        x = T(seeded((STEP_B, STEP_L, STEP_MIXER["d_model"]), 51))
        c = T(seeded((STEP_B, 48), 52))
        args = (c,) if cls == "CondMamba" else ()
        with torch.no_grad():
            y_full = m(x, *args)
            p = Params(max_seqlen=STEP_L, max_batch_size=STEP_B)
            ys = [m(x[:, :STEP_PREFILL], *args, inference_params=p)]
            for t in range(STEP_PREFILL, STEP_L):
                p.seqlen_offset = t
                ys.append(m(x[:, t:t + 1], *args, inference_params=p))
            conv_state, ssm_state = p.key_value_memory_dict[3]
        arrs.update({f"{cls}_x": x, f"{cls}_c": c, f"{cls}_y_full": y_full, f"{cls}_y_steps": torch.cat(ys, 1),
                     f"{cls}_conv_state": conv_state, f"{cls}_ssm_state": ssm_state})
    save("mixer_step", "causal_conv1d_update_ref (causal-conv1d/causal_conv1d/causal_conv1d_interface.py:79-100); selective_state_update_ref "
         "(mamba/mamba_ssm/ops/triton/selective_state_update.py:193-228), distributions of the reference tests; Mamba / CondMamba slow path "
         "(mamba/mamba_ssm/modules/mamba_simple.py): one forward of 12 tokens, and forward(inference_params) over 5 tokens + 7 steps with the "
         "final conv / SSM states; procedural weights seed 7", **arrs)


def _mk_block(ns, hidden, reverse, transpose, cont=False, fourier=False):
    md = ns.models_dim
    blk = md.create_block(hidden, norm_epsilon=1e-5, rms_norm=True, residual_in_fp32=True, fused_add_norm=True,
                          layer_idx=1, scan_type="none", block_type="combined_fourier" if fourier else "combined",
                          reverse=reverse, transpose=transpose, cond_mamba=True, scanning_continuity=cont,
                          use_gated_mlp=True, block_kwargs={},
                          block_kwargs2=_jpeg2_kwargs(ns, 16, 2) if fourier else {})
    return ref_shim.slow_path(blk)


def _jpeg2_kwargs(ns, grid, depth):
    so = ns.scanning_orders
    zz = so.SCAN_ZOO["jpeg"](grid)[:2]
    rev = [so.reverse_permut_np(x) for x in zz]
    return dict(zigzag_paths=torch.cat([T(x)[None] for x in zz] * depth, 0),
                zigzag_paths_reverse=torch.cat([T(x)[None] for x in rev] * depth, 0), scan_type="jpeg_2")


def gen_block(ns):
    """DiMBlockCombined fwd + input grads for the 4 (reverse, transpose) sweep orders (+continuity)."""
    hidden, B, L = 128, 2, 256
    arrs = {}
    x = T(seeded((B, L, hidden), 51))
    res = T(seeded((B, L, hidden), 52))
    c = T(seeded((B, hidden), 53))
    gy = T(seeded((B, L, hidden), 54))
    gr = T(seeded((B, L, hidden), 55))
    arrs.update(x=x, residual=res, c=c, dy=gy, dres=gr)
    for (r, t, cont) in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (1, 1, 1), (0, 1, 1)):
        blk = _mk_block(ns, hidden, bool(r), bool(t), bool(cont))
        procedural_fill(blk, seed=9)
        xi, ri, ci = x.clone().requires_grad_(), res.clone().requires_grad_(), c.clone().requires_grad_()
        y, ro = blk(xi, ri, ci)
        ((y * gy).sum() + (ro * gr).sum()).backward()
        tag = f"r{r}t{t}c{cont}"
        arrs.update({f"{tag}_y": y, f"{tag}_res_out": ro, f"{tag}_dx": xi.grad, f"{tag}_dres": ri.grad,
                     f"{tag}_dc": ci.grad})
    save("block_combined", "DiMBlockCombined.forward (dimsum/models_dim.py:1055-1117) via create_block(:2001-2160), "
         "hidden 128, procedural weights seed 9", **arrs)
    # the same at DiM-S/2's width (hidden 384: fusion head_dim 24, the smallest the MFMA attention kernels are built for),
    # one batch row, the richest flag combination -- so that a GPU block test runs every HIP kernel incl. attention
    hidden, B = 384, 1
    x, res, c = T(seeded((B, L, hidden), 56)), T(seeded((B, L, hidden), 57)), T(seeded((B, hidden), 58))
    gy, gr = T(seeded((B, L, hidden), 59)), T(seeded((B, L, hidden), 60))
    blk = _mk_block(ns, hidden, True, True, True)
    procedural_fill(blk, seed=9)
    xi, ri, ci = x.clone().requires_grad_(), res.clone().requires_grad_(), c.clone().requires_grad_()
    y, ro = blk(xi, ri, ci)
    ((y * gy).sum() + (ro * gr).sum()).backward()
    f16 = lambda t: t.detach().numpy().astype(np.float32)
    save("block_combined_384", "DiMBlockCombined.forward + input grads (dimsum/models_dim.py:1055-1117), hidden 384, reverse / transpose / "
         "continuity all on, procedural weights seed 9; inputs = seeded(56..60)", y=f16(y), res_out=f16(ro), dx=f16(xi.grad), dres=f16(ri.grad),
         dc=f16(ci.grad), g_qkv1=f16(blk.proj.qkv1.weight.grad), g_A_log=f16(blk.spatial_mamba.mixer.A_log.grad),
         g_norm2=f16(blk.norm_2.weight.grad))


def gen_block_1024(ns):
    """BASELINE configs[2]'s block at ITS width: DiMBlockCombined(1024) (DiM-L/2: mixers d_model 512 / D 1024 / R 32, fusion
    head_dim 64, MLP 1024 -> 8192 -> 4096 -> 1024), reverse + transpose on, continuity off (published), batch 2."""
    hidden, B, L = 1024, 2, 256
    x, res, c = T(seeded((B, L, hidden), 91)), T(seeded((B, L, hidden), 92)), T(seeded((B, hidden), 93))
    gy, gr = T(seeded((B, L, hidden), 94)), T(seeded((B, L, hidden), 95))
    blk = _mk_block(ns, hidden, True, True, False)
    procedural_fill(blk, seed=9)
    xi, ri, ci = x.clone().requires_grad_(), res.clone().requires_grad_(), c.clone().requires_grad_()
    y, ro = blk(xi, ri, ci)
    ((y * gy).sum() + (ro * gr).sum()).backward()
    f = lambda t: t.detach().numpy().astype(np.float32)
    sm, fm = blk.spatial_mamba.mixer, blk.freq_mamba.mixer
    save("block_combined_1024", "DiMBlockCombined.forward + input grads + parameter grads (dimsum/models_dim.py:974-1117 via create_block "
         ":2001-2160), hidden 1024, reverse / transpose on, continuity off, batch 2, procedural weights seed 9; inputs = seeded(91..95)",
         y=f(y), res_out=f(ro), dx=f(xi.grad), dres=f(ri.grad), dc=f(ci.grad),
         g_qkv1_rows64=f(blk.proj.qkv1.weight.grad[:64]), g_qkv2_bias=f(blk.proj.qkv2.bias.grad), g_proj_bias=f(blk.proj.proj.bias.grad),
         g_A_log=f(sm.A_log.grad), g_D_freq=f(fm.D.grad), g_x_proj=f(sm.x_proj.weight.grad), g_dt_bias_freq=f(fm.dt_proj.bias.grad),
         g_conv1d=f(sm.conv1d.weight.grad), g_in_proj_rows64=f(fm.in_proj.weight.grad[:64]), g_out_proj_rows64=f(sm.out_proj.weight.grad[:64]),
         g_norm2=f(blk.norm_2.weight.grad), g_norm=f(blk.norm.weight.grad), g_w12_bias=f(blk.mlp.w12.bias.grad),
         g_w3_rows16=f(blk.mlp.w3.weight.grad[:16]), g_adaLN_bias=f(blk.adaLN_modulation[1].bias.grad))


def _window_order(ns, transpose, reverse, shift, H):
    """Order seen by the mixer inside DiMBlockWindow.forward (models_dim.py:465-477); the chain of :488-497 must undo it."""
    from einops import rearrange
    so = ns.scanning_orders
    L = H * H
    hs = so.local_scan(torch.arange(L, dtype=torch.float32).view(1, L, 1), w=4, H=H, W=H, column_first=bool(transpose)).contiguous()
    if shift:
        hs = torch.roll(rearrange(hs, "b (h w) c -> b h w c", h=H), shifts=(-1, -1), dims=(1, 2)).reshape(-1, L, 1)
    if reverse:
        hs = hs.flip(1)
    back = hs.flip(1) if reverse else hs
    if shift:
        back = torch.roll(rearrange(back, "b (h w) c -> b h w c", h=H), shifts=(1, 1), dims=(1, 2)).reshape(-1, L, 1)
    back = so.local_reverse(back, w=4, H=H, W=H, column_first=bool(transpose))
    assert torch.equal(back.view(-1), torch.arange(L, dtype=torch.float32))
    return hs.view(-1).long().numpy()


_LW_FLAGS = dict(norm_epsilon=1e-5, rms_norm=True, residual_in_fp32=True, fused_add_norm=True, layer_idx=1, scan_type="none",
                 cond_mamba=True, use_gated_mlp=True, block_kwargs={}, block_kwargs2={})
# (file tag, create_block keywords): DiMBlock over every (reverse, transpose, continuity); the same block with create_block's OWN defaults
# (LayerNorm, unfused add + norm, the unconditional Mamba); DiMBlockWindow for both values of the flag it is built from (create_block
# maps its `reverse` to the window block's `transpose`, models_dim.py:2080-2081)
LW_CASES = ([(f"linear_r{r}t{t}c{c}", dict(_LW_FLAGS, block_type="linear", reverse=bool(r), transpose=bool(t), scanning_continuity=bool(c)))
             for r in (0, 1) for t in (0, 1) for c in (0, 1)]
            + [("linear_default", dict(layer_idx=1, reverse=True, transpose=True))]
            + [(f"window_t{t}", dict(_LW_FLAGS, block_type="window", reverse=bool(t), transpose=False, scanning_continuity=False)) for t in (0, 1)])
LW_BIG, LW_STEP = 16384, 16      # parameters with more elements than LW_BIG: the gradient rows [::LW_STEP] (keeps every file below 1 MiB)


def gen_block_linear_window(ns):
    """DiMBlock / DiMBlockWindow (dimsum/models_dim.py:223-502 via create_block :2001-2160): forward, residual output, input / c gradients and
    every parameter gradient at hidden 128, 16x16 tokens, batch 2; and the token orders of both blocks as index vectors."""
    hidden, B, L = 128, 2, 256
    x, res, c = T(seeded((B, L, hidden), 101)), T(seeded((B, L, hidden), 102)), T(seeded((B, hidden), 103))
    gy, gr = T(seeded((B, L, hidden), 104)), T(seeded((B, L, hidden), 105))
    common = {}
    for H in (4, 16):
        for r in (0, 1):
            for t in (0, 1):
                for k in (0, 1):
                    common[f"linear_H{H}_r{r}_t{t}_c{k}"] = _block_order(ns, r, t, k, H).astype(np.int16)
                    common[f"window_H{H}_t{t}_r{r}_s{k}"] = _window_order(ns, t, r, k, H).astype(np.int16)
    for tag, kw in LW_CASES:
        blk = ref_shim.slow_path(ns.models_dim.create_block(hidden, **kw))
        procedural_fill(blk, seed=9)
        xi, ri, ci = x.clone().requires_grad_(), res.clone().requires_grad_(), c.clone().requires_grad_()
        y, ro = blk(xi, ri, ci)
        ((y * gy).sum() + (ro * gr).sum()).backward()
        assert torch.equal(ro, common.setdefault("res_out", ro.detach()))      # x + residual whatever the block: stored once
        arrs = dict(y=y, dx=xi.grad, dres=ri.grad, dc=ci.grad, keys=np.array(sorted(blk.state_dict().keys())))
        for k, v in blk.named_parameters():
            if v.grad is not None:
                arrs[("g16_" if v.numel() > LW_BIG else "g_") + k] = v.grad[::LW_STEP] if v.numel() > LW_BIG else v.grad
        save("block_" + tag, f"{type(blk).__name__}.forward + every gradient (dimsum/models_dim.py:223-502) via create_block({kw}), hidden 128, "
             f"procedural weights seed 9; inputs = seeded(101..105); g16_*: rows [::{LW_STEP}] of the gradient", **arrs)
    save("block_linear_window", "token orders seen by the mixer in DiMBlock.forward (dimsum/models_dim.py:322-333) and DiMBlockWindow.forward "
         "(:465-477) as index vectors; res_out shared by the block_linear_* / block_window_* fixtures", **common)


def gen_model_tiny_linear_window(ns):
    """model_tiny with block_type linear / window: forward, dx and the state_dict key list"""
    for bt in ("linear", "window"):
        m = _mk_model(ns, "tiny", block_type=bt)
        procedural_fill(m, seed=3)
        x = T(seeded((2, 4, 32, 32), 61)).requires_grad_()
        t, y = T(seeded((2,), 62, kind="uniform")), torch.tensor([3, 7])
        out = m(x, t, y)
        g = T(seeded(tuple(out.shape), 63))
        out.backward(g)
        save("model_tiny_" + bt, f"DiM.forward (dimsum/models_dim.py:1796-1884), depth 4 hidden 64, published flags (scripts/train.sh) with "
             f"block_type={bt!r}, procedural weights seed 3", x=x, t=t, y=y, out=out, dout=g, dx=x.grad,
             n_keys=np.array(len(m.state_dict())), keys=np.array(sorted(m.state_dict().keys())))


PE_ROPE_CASES = ((64, 4), (128, 16))                  # (hidden, grid) of the stored rotary tables
PE_CPE_CASES = ((2, 4, 64), (2, 6, 136))              # (B, grid, C) of the stored AdaInPosCNN cases
PE_BIG = 4096                                         # parameters with more elements: the gradient rows [::LW_STEP] (the adaLN head's weight)


def gen_pe(ns):
    """The rope and cpe positional encodings: get_2d_sincos_rotary_embed / apply_rotary (dimsum/pe/my_rotary.py:11-72), AdaInPosCNN
    (dimsum/pe/cpe.py:29-48) forward + every gradient, and DiM(pe_type="rope" | "cpe") on the tiny recipe (models_dim.py:1627-1633,1812-1822).
    The reference's block loop tests `self.pe_tpe == "cpe"` (models_dim.py:1843), an attribute that does not exist: the cpe model gets the
    instance attribute `pe_tpe = pe_type` (all three branches of that loop make the same call); no reference file is touched."""
    rot, cpe = sys.modules["pe.my_rotary"], sys.modules["pe.cpe"]
    arrs = {}
    for i, (H, grid) in enumerate(PE_ROPE_CASES):
        sin, cos = rot.get_2d_sincos_rotary_embed(H, grid)
        sin, cos = T(sin).to(torch.float32), T(cos).to(torch.float32)         # as DiM.__init__ stores them (models_dim.py:1629-1630)
        x = T(seeded((2, grid * grid, H), 111 + i)).requires_grad_()
        y = rot.apply_rotary(x, sin, cos)
        g = T(seeded(tuple(y.shape), 113 + i))
        y.backward(g)
        tag = f"H{H}_g{grid}"
        arrs.update({tag + "_sin": sin, tag + "_cos": cos})
        if i == 0:          # (y and dx of the larger case alone would be 512 KiB)
            arrs.update({tag + "_y": y, tag + "_dx": x.grad})
    save("pe_rope", "get_2d_sincos_rotary_embed as float32 (dimsum/pe/my_rotary.py:11-60) for (hidden, grid) in "
         f"{PE_ROPE_CASES}; apply_rotary fwd / autograd (:63-72) for the first, batch 2, x = seeded(111), dy = seeded(113)", **arrs)
    arrs = {}
    for i, (B, grid, C) in enumerate(PE_CPE_CASES):
        m = cpe.AdaInPosCNN(C, C)
        procedural_fill(m, seed=13)
        x = T(seeded((B, grid * grid, C), 121 + i)).requires_grad_()
        c = T(seeded((B, C), 123 + i)).requires_grad_()
        y = m(x, c, H=grid, W=grid)
        g = T(seeded(tuple(y.shape), 125 + i))
        y.backward(g)
        tag = f"B{B}_g{grid}_C{C}"
        arrs.update({tag + "_y": y, tag + "_dx": x.grad, tag + "_dc": c.grad})
        for k, v in m.named_parameters():
            big = v.numel() > PE_BIG
            arrs[f"{tag}_{'g16' if big else 'g'}_{k}"] = v.grad[::LW_STEP] if big else v.grad
    save("pe_cpe", "AdaInPosCNN.forward + every gradient (dimsum/pe/cpe.py:29-48) for (B, grid, C) in "
         f"{PE_CPE_CASES}, procedural weights seed 13; x = seeded(121 + i), c = seeded(123 + i), dy = seeded(125 + i); "
         f"g16_*: rows [::{LW_STEP}] of the gradient (parameters above {PE_BIG} elements)", **arrs)
    for pe in ("rope", "cpe"):
        m = _mk_model(ns, "tiny", pe_type=pe)
        if pe == "cpe":
            m.pe_tpe = m.pe_type
        procedural_fill(m, seed=3)
        x = T(seeded((2, 4, 32, 32), 61)).requires_grad_()
        t, y = T(seeded((2,), 62, kind="uniform")), torch.tensor([3, 7])
        out = m(x, t, y)
        g = T(seeded(tuple(out.shape), 63))
        out.backward(g)
        save("model_tiny_" + pe, f"DiM.forward (dimsum/models_dim.py:1796-1884), depth 4 hidden 64, published flags (scripts/train.sh) with "
             f"pe_type={pe!r}" + (" and the instance attribute pe_tpe = pe_type (:1843)" if pe == "cpe" else "") + ", procedural weights seed 3",
             x=x, t=t, y=y, out=out, dout=g, dx=x.grad, n_keys=np.array(len(m.state_dict())), keys=np.array(sorted(m.state_dict().keys())))


EINFFT_CASES = (("small", (2, 16, 32), "module", 131), ("unit", (2, 64, 192), "unit", 133))      # (tag, (B, N, C), parameter regime, seed)


def _einfft_fractions(m, x):
    """fractions of layer-1 elements with ReLU on and of layer-2 elements outside the shrink zone, per channel block: (4,), (4,)"""
    with torch.no_grad():
        B, N, C = x.shape
        s = torch.fft.fft2(x.view(B, N, 4, C // 4), dim=(1, 2), norm="ortho")
        mul = m.multiply
        w1, b1, w2, b2 = m.complex_weight_1, m.complex_bias_1, m.complex_weight_2, m.complex_bias_2
        pr, pi = mul(s.real, w1[0]) - mul(s.imag, w1[1]) + b1[0], mul(s.real, w1[1]) + mul(s.imag, w1[0]) + b1[1]
        hr, hi = pr.relu(), pi.relu()
        qr, qi = mul(hr, w2[0]) - mul(hi, w2[1]) + b2[0], mul(hr, w2[1]) + mul(hi, w2[0]) + b2[1]
        relu_on = torch.stack((pr > 0, pi > 0)).float().mean(dim=(0, 1, 2, 4))
        passed = (torch.stack((qr, qi)).abs() > m.sparsity_threshold).float().mean(dim=(0, 1, 2, 4))
    return relu_on, passed


def gen_einfft(ns):
    """EinFFT.forward + every gradient (dimsum/models_dim.py:713-775) in the module's own 0.02-scale parameter regime and in a unit-gain one
    (weights randn * bs^-0.5, biases randn * 0.1); one DiMBlockCombinedEinFFT (:1267-1399) at hidden 64 on a 4 x 4 grid; the tiny model with
    block_type="combined_einfft". Every case records the fractions of ReLU-on and shrink-pass elements and refuses a degenerate one."""
    md = ns.models_dim
    arrs = {}
    for tag, (B, N, C), regime, seed in EINFFT_CASES:
        torch.manual_seed(seed)
        m = md.EinFFT(C)
        if regime == "unit":
            bs = C // 4
            with torch.no_grad():
                for w in (m.complex_weight_1, m.complex_weight_2):
                    w.copy_(torch.randn_like(w) * bs ** -0.5)
                for b in (m.complex_bias_1, m.complex_bias_2):
                    b.copy_(torch.randn_like(b) * 0.1)
        x = T(seeded((B, N, C), seed + 1)).requires_grad_()
        y = m(x)
        g = T(seeded((B, N, C), seed + 2))
        y.backward(g)
        relu_on, passed = _einfft_fractions(m, x.detach())
        for f in (relu_on.mean().item(), passed.mean().item()):
            assert 0.2 <= f <= 0.995, (tag, f)
        arrs.update({f"{tag}_x": x, f"{tag}_dy": g, f"{tag}_y": y, f"{tag}_dx": x.grad, f"{tag}_relu_on": relu_on.mean(), f"{tag}_shrink_pass": passed.mean()})
        for k, v in m.named_parameters():
            arrs[f"{tag}_{k}"], arrs[f"{tag}_g_{k}"] = v.detach(), v.grad
    save("einfft", f"EinFFT.forward + every gradient (dimsum/models_dim.py:713-775) for (tag, (B, N, C), regime, seed) in {EINFFT_CASES}: 'module' = the "
         "constructor's randn * 0.02 parameters, 'unit' = weights randn * bs^-0.5, biases randn * 0.1; x = seeded(seed + 1), dy = seeded(seed + 2); "
         "relu_on / shrink_pass: the fractions of layer-1 elements with ReLU on and of layer-2 elements outside the shrink zone", **arrs)

    hidden, B, L = 64, 2, 16
    x, res, c = T(seeded((B, L, hidden), 141)), T(seeded((B, L, hidden), 142)), T(seeded((B, hidden), 143))
    gy, gr = T(seeded((B, L, hidden), 144)), T(seeded((B, L, hidden), 145))
    kw = dict(_LW_FLAGS, block_type="combined_einfft", reverse=True, transpose=True, scanning_continuity=False)
    blk = ref_shim.slow_path(md.create_block(hidden, **kw))
    procedural_fill(blk, seed=9)
    xi, ri, ci = x.clone().requires_grad_(), res.clone().requires_grad_(), c.clone().requires_grad_()
    y, ro = blk(xi, ri, ci)
    ((y * gy).sum() + (ro * gr).sum()).backward()
    relu_on, passed = _einfft_fractions(blk.freq_mamba, blk.norm(xi.detach() + ri.detach())[..., hidden // 2:].contiguous())
    arrs = dict(y=y, res_out=ro, dx=xi.grad, dres=ri.grad, dc=ci.grad, keys=np.array(sorted(blk.state_dict().keys())), relu_on=relu_on, shrink_pass=passed)
    for k, v in blk.named_parameters():
        if v.grad is not None:
            arrs[("g16_" if v.numel() > LW_BIG else "g_") + k] = v.grad[::LW_STEP] if v.numel() > LW_BIG else v.grad
    save("block_einfft", f"DiMBlockCombinedEinFFT.forward + every gradient (dimsum/models_dim.py:1267-1399) via create_block({kw}), hidden 64, 4 x 4 tokens, "
         f"procedural weights seed 9; inputs = seeded(141..145); g16_*: rows [::{LW_STEP}] of the gradient", **arrs)

    m = _mk_model(ns, "tiny", block_type="combined_einfft")
    procedural_fill(m, seed=3)
    seen = []
    hooks = [b.freq_mamba.register_forward_pre_hook(lambda mod, inp: seen.append(_einfft_fractions(mod, inp[0].detach().contiguous()))) for b in m.blocks]
    x = T(seeded((2, 4, 32, 32), 61)).requires_grad_()
    t, y = T(seeded((2,), 62, kind="uniform")), torch.tensor([3, 7])
    out = m(x, t, y)
    for h in hooks:
        h.remove()
    g = T(seeded(tuple(out.shape), 63))
    out.backward(g)
    passed = torch.stack([p for _, p in seen])            # (layers, 4): the fraction of non-zero Z per layer and channel block
    assert passed.max().item() >= 0.2, passed
    save("model_tiny_einfft", "DiM.forward (dimsum/models_dim.py:1796-1884), depth 4 hidden 64, published flags (scripts/train.sh) with "
         "block_type='combined_einfft', procedural weights seed 3 (complex weights: std 1 / (2 bs)); shrink_pass: the fraction of non-zero Z per "
         "layer and channel block", x=x, t=t, y=y, out=out, dout=g, dx=x.grad, n_keys=np.array(len(m.state_dict())),
         keys=np.array(sorted(m.state_dict().keys())), relu_on=torch.stack([r for r, _ in seen]), shrink_pass=passed)



def _mk_model(ns, name, **over):
    md = ns.models_dim
    kw = dict(img_resolution=32, in_channels=4, label_dropout=0.15, num_classes=1000, learn_sigma=False,
              scan_type="none", pe_type="ape", block_type="combined", cond_mamba=True, scanning_continuity=False,
              enable_fourier_layers=False, drop_path=0.0, rms_norm=True, fused_add_norm=True, learnable_pe=True,
              use_final_norm=False, use_attn_every_k_layers=4, use_gated_mlp=True)
    kw.update(over)
    if name == "tiny":
        m = md.DiM(depth=4, hidden_size=64, patch_size=2, **kw)
    elif name == "S/2":
        m = md.DiM(depth=12, hidden_size=384, patch_size=2, **kw)   # SURVEY finding 6: DiT-S analogy
    else:
        m = md.DiM_models[name](**kw)
    return ref_shim.slow_path(m).eval()


def gen_models(ns, which, only_tags=()):
    if "tiny" in which:
        ref_shim.allow_zigzag_through_dim(ns)
        for tag, over in {"tiny": {}, "tiny_cont": dict(scanning_continuity=True),
                          "tiny_fourier": dict(block_type="combined_fourier"),
                          "tiny_final_norm": dict(use_final_norm=True, num_classes=10),
                          "tiny_zigma8": dict(scan_type="zigma_8"), "tiny_jpeg8": dict(scan_type="jpeg_8"),
                          "tiny_sweep8": dict(scan_type="sweep_8")}.items():
            if only_tags and tag not in only_tags:
                continue
            m = _mk_model(ns, "tiny", **over)
            procedural_fill(m, seed=3)
            x = T(seeded((2, 4, 32, 32), 61)).requires_grad_()
            t = T(seeded((2,), 62, kind="uniform"))
            y = torch.tensor([3, 7])
            out = m(x, t, y)
            g = T(seeded(tuple(out.shape), 63))
            out.backward(g)
            arrs = dict(x=x, t=t, y=y, out=out, dout=g, dx=x.grad, n_keys=np.array(len(m.state_dict())),
                        keys=np.array(sorted(m.state_dict().keys())))
            if tag == "tiny":
                with torch.no_grad():
                    x4 = T(seeded((4, 4, 32, 32), 64))
                    t4 = T(seeded((4,), 65, kind="uniform"))
                    y4 = torch.tensor([3, 7, 1000, 1000])
                    arrs.update(cfg_x=x4, cfg_t=t4, cfg_y=y4, cfg_out=m.forward_with_cfg(x4, t4, y4, cfg_scale=1.4),
                                adacfg_out=m.forward_with_adacfg(x4, t4, y4, cfg_scale=3.8, scale_pow=4.0),
                                out_nolabel=m(x4, t4, None))
            save("model_" + tag, "DiM.forward (dimsum/models_dim.py:1796-1884), depth 4 hidden 64, "
                 "published flags (scripts/train.sh), procedural weights seed 3", **arrs)
    for name, tag, B in (("S/2", "model_S2", 4), ("DiM-L/2", "model_L2", 2), ("DiM-XL/2", "model_XL2_512", 1),
                         ("DiM-XL/2", "model_XL2_512_zigma8", 1)):
        if tag not in which:
            continue
        over = dict(img_resolution=64) if "512" in tag else {}
        if tag.endswith("zigma8"):      # BASELINE configs[4]: 8-way zigzag scanning orders inside the mixers
            ref_shim.allow_zigzag_through_dim(ns)
            over["scan_type"] = "zigma_8"
        m = _mk_model(ns, name, **over)
        procedural_fill(m, seed=3)
        R = 64 if "512" in tag else 32
        x = T(seeded((B, 4, R, R), 71))
        t = T(seeded((B,), 72, kind="uniform"))
        y = torch.arange(B) * 37 % 1000
        with torch.no_grad():
            out = m(x, t, y)
        nparam = sum(p.numel() for p in m.parameters())
        save(tag, f"DiM.forward {name} (dimsum/models_dim.py:1796-1884,2163-2236), procedural weights seed 3; "
             "inputs = seeded(71/72)", t=t, y=y, out=out, n_params=np.array(nparam),
             n_keys=np.array(len(m.state_dict())), keys=np.array(sorted(m.state_dict().keys())),
             shapes=np.array([str(tuple(v.shape)) for _, v in sorted(m.state_dict().items())]))
        del m


TRANSPORT_PATHS = ("GVP", "Linear", "VP")
TRANSPORT_PREDS = ("velocity", "noise", "score")
# explicit end-point margins: with the defaults the reference leaves sample_eps = None for VP and for noise / score
# prediction (transport/__init__.py:50-55 tests `train_eps is None` after assigning it), which its samplers cannot use
TRANSPORT_EPS = dict(train_eps=1e-3, sample_eps=2e-3)
SDE_CASES = (  # (sampling_method, diffusion_form, diffusion_norm, last_step, last_step_size)
    ("Euler", "SBDM", 1.0, "Mean", 0.04), ("Euler", "SBDM", 1.0, None, 0.04), ("Euler", "SBDM", 1.0, "Tweedie", 0.04),
    ("Euler", "SBDM", 1.0, "Euler", -1), ("Heun", "SBDM", 1.0, "Mean", 0.04), ("Heun", "SBDM", 1.0, "Tweedie", -1),
    ("Heun", "sigma", 0.7, "Euler", 0.04), ("Heun", "constant", 0.5, None, 0.04), ("Euler", "constant", 0.5, "Mean", 0.04),
    ("Euler", "sigma", 1.0, "Mean", 0.04), ("Euler", "linear", 1.0, "Mean", 0.04), ("Euler", "decreasing", 1.0, "Mean", 0.04),
    ("Euler", "increasing-decreasing", 1.0, "Tweedie", 0.04), ("Euler", "log", 1.0, "Euler", 0.04), ("Euler", "none", 1.0, "Mean", 0.04),
)


def gen_transport(_ns=None):
    """The reference's flow-matching harness around a closed-form denoiser (tests/golden/procedural.py:toy_denoiser):
    Transport.training_losses (dimsum/transport/transport.py:127-164) for {GVP, Linear, VP} x {velocity, noise, score} x
    loss weights; Sampler.sample_sde (:286-341; integrators.py:5-73) for Euler-Maruyama / Heun x diffusion forms x last
    steps; Sampler.sample_ode (:343-386) on the fixed Euler grid (through ref_shim's declared
    stand-in for torchdiffeq's euler). Random draws come from the CPU generator after torch.manual_seed(seed) exactly as
    the reference draws them (randn_like(x1) then rand(B); randn(x.size()) per SDE step)."""
    tp = ref_shim.load_transport()
    arrs = {}
    x1 = T(seeded((5, 3, 4, 4), 81))
    y = torch.tensor([3, 0, 7, 1, 5])
    arrs.update(loss_x1=x1, y=y)
    for pt in TRANSPORT_PATHS:
        for pred in TRANSPORT_PREDS:
            for lw in ((None,) if pred == "velocity" else (None, "velocity", "likelihood")):
                tr = tp.create_transport(pt, pred, lw, **TRANSPORT_EPS)
                seen = {}

                def model(xt, t, y=None):
                    seen["xt"], seen["t"] = xt, t
                    return toy_denoiser(xt, t, y)

                seed = 1000 + len(arrs)
                torch.manual_seed(seed)
                terms = tr.training_losses(model, x1, dict(y=y))
                tag = f"loss_{pt}_{pred}_{lw}"
                arrs.update({tag + "_seed": np.array(seed), tag + "_t": seen["t"], tag + "_xt": seen["xt"],
                             tag + "_loss": terms["loss"], tag + "_pred": terms["pred"]})
    # logit-normal time sampling (transport.py:116-121)
    tr = tp.create_transport("GVP", "velocity", None, t_sample_mode="logitnormal")
    torch.manual_seed(77)
    seen = {}

    def model(xt, t, y=None):
        seen["t"] = t
        return toy_denoiser(xt, t, y)

    terms = tr.training_losses(model, x1, dict(y=y))
    arrs.update(loss_logitnormal_t=seen["t"], loss_logitnormal_loss=terms["loss"])

    z = T(seeded((3, 3, 4, 4), 82))
    yz = torch.tensor([2, 9, 4])
    arrs.update(z=z, yz=yz)
    for pt in TRANSPORT_PATHS:
        for pred in TRANSPORT_PREDS:
            tr = tp.create_transport(pt, pred, **TRANSPORT_EPS)
            # velocity prediction on GVP / Linear: create_transport forces both margins to 0 (__init__.py:56-58), with which the
            # SBDM diffusion (alpha' / alpha at t = 0) is infinite; the SDE fixtures set the margin on the object instead
            tr.train_eps, tr.sample_eps = TRANSPORT_EPS["train_eps"], TRANSPORT_EPS["sample_eps"]
            smp = tp.Sampler(tr)
            for i, (method, form, norm, last, lss) in enumerate(SDE_CASES):
                torch.manual_seed(2000 + i)
                xs = smp.sample_sde(sampling_method=method, diffusion_form=form, diffusion_norm=norm, last_step=last,
                                    last_step_size=lss, num_steps=10)(z, toy_denoiser, y=yz)
                arrs[f"sde_{pt}_{pred}_{i}_last"] = xs[-1]
                arrs[f"sde_{pt}_{pred}_{i}_prev"] = xs[-2]
                arrs[f"sde_{pt}_{pred}_{i}_len"] = np.array(len(xs))
            # (reverse=True cannot run in the reference: check_interval returns t0 > t1 and integrators.py:90 asserts)
            traj = smp.sample_ode(sampling_method="euler", num_steps=9)(z, toy_denoiser, y=yz)
            arrs[f"ode_{pt}_{pred}"] = traj[-1]
            arrs[f"ode_{pt}_{pred}_mid"] = traj[4]
            # likelihood ODE (transport.py:388-443): data -> prior with Hutchinson's divergence estimate, (x, delta_logp) tuple state;
            # under no_grad like its callers (the reference sets x.requires_grad on the solver's state, which must be a leaf)
            torch.manual_seed(3000)
            with torch.no_grad():
                logp, zprior = smp.sample_ode_likelihood(sampling_method="euler", num_steps=9)(z, toy_denoiser, y=yz)
            arrs[f"lik_{pt}_{pred}_logp"], arrs[f"lik_{pt}_{pred}_z"] = logp, zprior
    arrs["sde_cases"] = np.array([repr(c) for c in SDE_CASES])
    save("transport", "dimsum/transport: Transport.training_losses (transport.py:127-164), Sampler.sample_sde (:286-341, "
         "integrators.py:5-73), Sampler.sample_ode on the euler grid (:343-386, integrators.py:98-111 with the declared torchdiffeq "
         "euler stand-in of tools/ref_shim.py:load_transport), path.py:21-246; denoiser = tests/golden/procedural.py:toy_denoiser", **arrs)


BLUR_CASES = (("p4", (5, 3, 8, 8), 4), ("p8", (3, 2, 8, 8), 8), ("p2", (3, 2, 8, 8), 2), ("p4_32", (2, 4, 32, 32), 4))
BLUR_LOSS_CASES = (("GVP", "velocity", None), ("Linear", "velocity", None), ("VP", "velocity", None), ("GVP", "noise", "velocity"),
                   ("GVP", "score", "likelihood"))
BLUR_SIGMA_MAX = 3


def gen_transport_blur(_ns=None):
    """The reference's DCT-blurred path: DCTBlur(x, p, sigmas, 1e-3) (dimsum/transport/path.py:249-259 over blurring.py's FFT-based DCT) for
    BLUR_CASES (x = procedural.seeded(shape, x_seed), not stored), the per-sample sigmas including exactly 0 and exactly blur_sigma_max; and Transport.training_losses with
    path_args use_blurring=True (path.py:159-169) around toy_denoiser for BLUR_LOSS_CASES. A fixture of its own: transport.npz stays as it is."""
    tp = ref_shim.load_transport()
    ref_path = sys.modules[tp.__name__ + ".path"]
    arrs = {}
    for i, (tag, shape, p) in enumerate(BLUR_CASES):
        x = T(seeded(shape, 91 + i))
        sig = torch.linspace(0, BLUR_SIGMA_MAX, shape[0]) if shape[0] > 2 else torch.tensor([0.0, float(BLUR_SIGMA_MAX)])
        if shape[0] > 3:
            sig[1:-1] = T(seeded((shape[0] - 2,), 95 + i)).abs().clamp(0.05, 2.9)          # uneven levels between the two ends
        assert sig[0] == 0 and sig[-1] == BLUR_SIGMA_MAX
        out = ref_path.DCTBlur(x, p, sig.view(-1, 1, 1, 1), 1e-3, x.device)
        arrs.update({f"blur_{tag}_x_seed": np.array(91 + i), f"blur_{tag}_shape": np.array(shape), f"blur_{tag}_p": np.array(p), f"blur_{tag}_sigmas": sig, f"blur_{tag}_out": out})
    arrs["blur_cases"] = np.array([c[0] for c in BLUR_CASES])
    x1 = T(seeded((5, 3, 8, 8), 83))
    y = torch.tensor([3, 0, 7, 1, 5])
    arrs.update(loss_x1=x1, y=y, blur_sigma_max=np.array(BLUR_SIGMA_MAX), blur_upscale=np.array(4))
    for n, (pt, pred, lw) in enumerate(BLUR_LOSS_CASES):
        tr = tp.create_transport(pt, pred, lw, **TRANSPORT_EPS,
                                 path_args=dict(use_blurring=True, blur_sigma_max=BLUR_SIGMA_MAX, blur_upscale=4))
        seen = {}

        def model(xt, t, y=None):
            seen["xt"], seen["t"] = xt, t
            return toy_denoiser(xt, t, y)

        seed = 4000 + n
        torch.manual_seed(seed)
        terms = tr.training_losses(model, x1, dict(y=y))
        tag = f"loss_{pt}_{pred}_{lw}"
        arrs.update({tag + "_seed": np.array(seed), tag + "_t": seen["t"], tag + "_xt": seen["xt"], tag + "_loss": terms["loss"],
                     tag + "_pred": terms["pred"]})
    arrs["loss_cases"] = np.array([repr(c) for c in BLUR_LOSS_CASES])
    save("transport_blur", "dimsum/transport: DCTBlur (path.py:249-259, blurring.py:32-149) and Transport.training_losses "
         "(transport.py:127-164) with path_args use_blurring=True, blur_sigma_max=3, blur_upscale=4 (path.py:159-169); "
         "denoiser = tests/golden/procedural.py:toy_denoiser", **arrs)


def gen_dit_keys(_ns=None):
    """tests/golden/dit_keys.json: [[state_dict key, shape], ...] of the reference's DiT-S/2 (dimsum/models_dit.py, imported with the timm
    stand-ins of tools/ref_shim.py: timm 0.9.12's PatchEmbed / Attention / Mlp parameter names), in state_dict order"""
    import json
    import models_dit          # (ref_shim.load() put the reference's dimsum/ on sys.path)
    assert os.path.realpath(models_dit.__file__).startswith(os.path.realpath(ref_shim.REF)), models_dit.__file__
    m = models_dit.DiT_models["DiT-S/2"]()
    keys = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "dit_keys.json")
    with open(path, "w") as f:
        json.dump(keys, f, indent=0)
        f.write("\n")
    print(f"  dit_keys.json: {len(keys)} keys")


def gen_moe(ns):
    """tests/golden/moe_switch.npz (routing_mode "top1": softmax) and moe_switch_sinkhorn.npz (routing_mode "sinkhorn": sigmoid) -- the reference's
    SwitchMLP (dimsum/switch_mlp.py) on the CPU at dim 32, tokens (2, 24), 4 experts over {gated, plain} x {bias, no bias}: output, chosen expert
    per token, d x and every parameter gradient; weights = procedural_fill(module, seed) (not stored: the test fills its own module the same
    way). One file per routing mode keeps each under the repository's size limit. moe_switch.npz also holds one sinkhorn() input / output pair,
    one MLP forward and one MoEBlock(SwitchMLP, nn.LayerNorm) forward. tests/golden/moe_keys.json: state_dict keys and shapes of that block."""
    import json
    from functools import partial
    md = ns.models_dim
    import switch_mlp as sw
    assert os.path.realpath(sw.__file__).startswith(os.path.realpath(ref_shim.REF)), sw.__file__
    dim, E = 32, 4
    x, dout = T(seeded((2, 24, dim), 501)), T(seeded((2, 24, dim), 502))
    for mode, name in (("top1", "moe_switch"), ("sinkhorn", "moe_switch_sinkhorn")):
        arrs = {"x": x, "dout": dout}
        for ci, (gated, bias) in enumerate(((True, True), (True, False), (False, True), (False, False))):
            tag = f"{'gated' if gated else 'plain'}_{'bias' if bias else 'nobias'}"
            seed = 40 + ci
            m = procedural_fill(sw.SwitchMLP(dim, layer_idx=1, num_moe_experts=E, add_bias_linear=bias, gated_linear_unit=gated, routing_mode=mode), seed=seed)
            xr = x.clone().requires_grad_()
            out = m(xr)
            out.backward(dout)
            with torch.no_grad():
                logits = m.router(x).view(-1, E)
                route = torch.sigmoid(logits) if mode == "sinkhorn" else torch.softmax(logits, dim=1)
            arrs.update({f"{tag}.seed": np.int64(seed), f"{tag}.out": out, f"{tag}.dx": xr.grad, f"{tag}.expert": torch.max(route, dim=1)[1]})
            for k, p_ in m.named_parameters():
                arrs[f"{tag}.grad.{k}"] = torch.zeros_like(p_) if p_.grad is None else p_.grad
        if mode == "top1":
            cost = T(seeded((6, E), 503, scale=0.5))
            arrs.update({"sinkhorn.cost": cost, "sinkhorn.out": sw.sinkhorn(cost)})
            mlp = procedural_fill(ns.mlp.MLP(dim, add_bias_linear=True, gated_linear_unit=True), seed=50)
            arrs["mlp.out"] = mlp(x)
            blk = procedural_fill(md.MoEBlock(dim, mixer_cls=partial(md.SwitchMLP, layer_idx=1, num_moe_experts=E), norm_cls=torch.nn.LayerNorm), seed=51)
            h, r = blk(x, dout)
            arrs.update({"block.out": h, "block.residual": r})
            keys = [[k, list(v.shape)] for k, v in blk.state_dict().items()]
            with open(os.path.join(OUT, "moe_keys.json"), "w") as f:
                json.dump(keys, f, indent=0)
                f.write("\n")
            print(f"  moe_keys.json: {len(keys)} keys")
        save(name, f"reference SwitchMLP (dimsum/switch_mlp.py:24-99) on the CPU, routing_mode={mode}, dim {dim}, tokens (2, 24), {E} experts; weights: "
                   "procedural_fill(module, <tag>.seed); x, dout: stored", **arrs)


LM_TINY = dict(d_model=64, n_layer=2, vocab_size=90, pad_vocab_size_multiple=8, ssm_cfg=dict(d_state=16, d_conv=4, expand=2))
LM_VARIANTS = tuple((f"rms{r}_fp32res{f}", dict(rms_norm=bool(r), residual_in_fp32=bool(f), fused_add_norm=True)) for r in (0, 1) for f in (0, 1))
LM_B, LM_PROMPT, LM_STEPS = 2, 9, 7


def gen_lm(_ns=None):
    """tests/golden/lm_tiny_<variant>.npz: the reference's MambaLMHeadModel (mixer_seq_simple.py:166-226) on its slow path in fp32 at LM_TINY for
    rms_norm x residual_in_fp32: the weights (procedural_fill with the first seed whose greedy continuation is decided by a clear margin), the
    prompt's logits, the logits of LM_STEPS cached greedy steps (Mamba.step, mamba_simple.py:299-344), the generated ids and min_gap, the
    smallest top-1 minus top-2 logit over the generated steps. tests/golden/lm_keys.json: state-dict keys and shapes."""
    import json
    lm = ref_shim.load_lm()
    for tag, flags in LM_VARIANTS:
        for seed in range(11, 40):
            torch.manual_seed(0)
            m = lm.mss.MambaLMHeadModel(**LM_TINY, **flags).eval()
            procedural_fill(m, seed=seed)
            m.tie_weights()
            ref_shim.slow_path(m)
            prompt = T(np.random.RandomState(seed).randint(0, LM_TINY["vocab_size"], size=(LM_B, LM_PROMPT)).astype(np.int64))
            with torch.no_grad():
                p = lm.gen.InferenceParams(max_seqlen=LM_PROMPT + LM_STEPS, max_batch_size=LM_B)
                prompt_logits = m(prompt, inference_params=p).logits
                full_logits = m(prompt).logits
                assert torch.allclose(prompt_logits, full_logits, rtol=1e-5, atol=1e-6)
                p.seqlen_offset = LM_PROMPT
                tok = prompt_logits[:, -1].argmax(-1, keepdim=True)
                ids, steps = [tok], []
                gaps = [prompt_logits[:, -1].topk(2).values]
                for _ in range(LM_STEPS):
                    logits = m(tok, inference_params=p, num_last_tokens=1).logits[:, 0]
                    p.seqlen_offset += 1
                    steps.append(logits)
                    gaps.append(logits.topk(2).values)
                    tok = logits.argmax(-1, keepdim=True)
                    ids.append(tok)
            steps = torch.stack(steps, 1)                                   # (B, LM_STEPS, vocab)
            top2 = torch.stack(gaps, 1)                                     # every row an argmax was taken from
            min_gap = float((top2[..., 0] - top2[..., 1]).min())
            max_logit = float(torch.maximum(prompt_logits.abs().max(), steps.abs().max()))
            if min_gap >= 1e-3 * max_logit:
                break
        assert min_gap >= 1e-3 * max_logit, (tag, min_gap, max_logit)
        arrs = {"w." + k: v for k, v in m.state_dict().items()}
        save(f"lm_tiny_{tag}", f"reference MambaLMHeadModel (mamba/mamba_ssm/models/mixer_seq_simple.py:166-226) slow path, fp32, {LM_TINY}, {flags}, "
             f"procedural_fill seed {seed}; prompt (B {LM_B}, {LM_PROMPT} tokens) -> prompt_logits; {LM_STEPS} greedy cached steps -> step_logits "
             "(B, steps, vocab); ids (B, steps + 1): the argmax of the prompt's last row, then of every step; min_gap: the smallest top-1 minus "
             "top-2 logit over the rows those argmaxes were taken from; w.*: the state dict", prompt=prompt, prompt_logits=prompt_logits,
             step_logits=steps, ids=torch.cat(ids, 1), min_gap=np.float64(min_gap), max_logit=np.float64(max_logit), seed=np.int64(seed), **arrs)
    doc = {name: [[k, list(v.shape)] for k, v in lm.mss.MambaLMHeadModel(**LM_TINY, rms_norm=rms, fused_add_norm=True).state_dict().items()]
           for name, rms in (("layer_norm", False), ("rms_norm", True))}
    with open(os.path.join(OUT, "lm_keys.json"), "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print(f"  lm_keys.json: {len(doc['layer_norm'])} / {len(doc['rms_norm'])} keys")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    args = ap.parse_args()
    ns = ref_shim.load()
    torch.set_num_threads(8)
    steps = {
        "scan": lambda: gen_scan(ns), "conv": lambda: gen_conv(ns), "norm": lambda: gen_norm(ns),
        "perm": lambda: gen_perm(ns), "orders": lambda: gen_block_orders(ns), "wavelet": lambda: gen_wavelet_dct(ns),
        "fusion": lambda: gen_fusion(ns), "inner": lambda: gen_inner(ns), "bimamba": lambda: gen_bimamba(ns), "mixer": lambda: gen_mixer(ns),
        "block": lambda: gen_block(ns), "tiny": lambda: gen_models(ns, {"tiny"}),
        "S2": lambda: gen_models(ns, {"model_S2"}), "L2": lambda: gen_models(ns, {"model_L2"}),
        "XL2": lambda: gen_models(ns, {"model_XL2_512"}),
        "zigzag": lambda: gen_models(ns, {"tiny"}, only_tags=("tiny_zigma8", "tiny_jpeg8", "tiny_sweep8")),
        "XL2zigzag": lambda: gen_models(ns, {"model_XL2_512_zigma8"}),
        "transport": lambda: gen_transport(ns), "block1024": lambda: gen_block_1024(ns),
        "transport_blur": lambda: gen_transport_blur(ns),
        "block_linear_window": lambda: gen_block_linear_window(ns), "tiny_linear_window": lambda: gen_model_tiny_linear_window(ns),
        "pe": lambda: gen_pe(ns), "einfft": lambda: gen_einfft(ns), "dit_keys": lambda: gen_dit_keys(ns), "step": lambda: gen_step(ns),
        "scan_general": lambda: gen_scan_general(ns), "moe": lambda: gen_moe(ns), "lm": lambda: gen_lm(ns),
    }
    for k, fn in steps.items():
        if args.only is None or k in args.only:
            print(f"[{k}]")
            fn()


if __name__ == "__main__":
    main()
