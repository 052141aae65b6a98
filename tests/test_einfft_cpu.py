"""Block type "combined_einfft" without a GPU: the torch restatement of the spectral branch (ops/einfft.py:einfft_torch) against the reference
fixture einfft.npz, forward and all gradients; the block and the tiny model against block_einfft.npz / model_tiny_einfft.npz on the CPU oracle
backend with the four native.einfft_* entry points replaced by the plain-torch stand-ins below (the oracle package knows nothing of them); the
state-dict keys; the constructor's and the parsers' refusals; the C ABI of the four entry points.
Tolerances: test_model_cpu.TOL, and test_blocks_linear_window_cpu.SUM_TOL for sums over rows (parameter gradients)."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from conftest import assert_close, golden
from oracle.torch_backend import cpu_oracle_backend
from procedural import procedural_fill, seeded
from test_blocks_linear_window_cpu import PUBLISHED, SUM_TOL
from test_host_logic import _header_layout
from test_model_cpu import TOL, _published

T = torch.from_numpy
n = lambda t: t.detach().cpu().numpy()      # noqa: E731
CASES = {"small": (2, 16, 32), "unit": (2, 64, 192)}
PARAMS = ("complex_weight_1", "complex_bias_1", "complex_weight_2", "complex_bias_2")
EINFFT_KEYS = ["freq_mamba." + k for k in sorted(PARAMS)]
BLOCK_KW = dict(PUBLISHED, block_type="combined_einfft", reverse=True, transpose=True, scanning_continuity=False)
BLOCK_SHAPE = (2, 16, 64)


# ---- plain-torch stand-ins of native.einfft_dft / einfft_idft_real / einfft_mlp_fwd / einfft_mlp_bwd (same signatures and results) ---------------
def einfft_dft(x):
    from dimsum_amd.ops.einfft import dft_torch
    with torch.no_grad():
        re, im = dft_torch(x)
    return re.contiguous(), im.contiguous()


def einfft_idft_real(re, im, out=None):
    from dimsum_amd.ops.einfft import idft_real_torch
    with torch.no_grad():
        y = idft_real_torch(re, im)
    return y.contiguous() if out is None else out.copy_(y)


def einfft_mlp_fwd(re, im, w1, b1, w2, b2, lam):
    from dimsum_amd.ops.einfft import mlp_torch
    with torch.no_grad():
        zr, zi, _ = mlp_torch(re, im, w1, b1, w2, b2, lam)
    return zr.contiguous(), zi.contiguous()


def einfft_mlp_bwd(dzr, dzi, re, im, zr, zi, w1, b1, w2, b2, lam):
    from dimsum_amd.ops.einfft import _cmul_torch
    B, N, C = re.shape
    sh, pl = (B, N, 4, C // 4), (B, N, C)
    with torch.enable_grad():
        xr, xi = re.detach().reshape(sh).requires_grad_(), im.detach().reshape(sh).requires_grad_()
        pr, pi = _cmul_torch(xr, xi, w1.detach(), b1.detach())
        hr, hi = pr.relu().detach().requires_grad_(), pi.relu().detach().requires_grad_()
        qr, qi = _cmul_torch(hr, hi, w2.detach(), b2.detach())
        dz2r, dz2i = dzr * (zr != 0), dzi * (zi != 0)
        dhr, dhi = torch.autograd.grad((qr, qi), (hr, hi), (dz2r.reshape(sh), dz2i.reshape(sh)))
        dp1r, dp1i = dhr * (hr > 0), dhi * (hi > 0)
        dxr, dxi = torch.autograd.grad((pr, pi), (xr, xi), (dp1r, dp1i))
    d = lambda t: t.detach().reshape(pl).contiguous()       # noqa: E731
    return d(dxr), d(dxi), (d(hr), d(hi)), (d(dz2r), d(dz2i)), (d(dp1r), d(dp1i))


_STANDINS = dict(einfft_dft=einfft_dft, einfft_idft_real=einfft_idft_real, einfft_mlp_fwd=einfft_mlp_fwd, einfft_mlp_bwd=einfft_mlp_bwd)


@contextlib.contextmanager
def torch_einfft_backend():
    from dimsum_amd import native
    saved = {k: getattr(native, k) for k in _STANDINS}
    try:
        for k, f in _STANDINS.items():
            setattr(native, k, f)
        yield
    finally:
        for k, f in saved.items():
            setattr(native, k, f)


# ---- the restatement and the operator on the stand-ins against the reference ---------------------------------------------------------------------
def check_einfft_against_fixture(fn, tag, dev, y_tol, g_tol, sum_tol):
    """fn(x, w1, b1, w2, b2, lam) against case `tag` of einfft.npz: y, dx and the four parameter gradients"""
    g = golden("einfft")
    assert 0.2 <= float(g[tag + "_relu_on"]) <= 0.995 and 0.2 <= float(g[tag + "_shrink_pass"]) <= 0.995
    x = T(g[tag + "_x"]).to(dev).requires_grad_()
    p = {k: T(g[f"{tag}_{k}"]).to(dev).requires_grad_() for k in PARAMS}
    y = fn(x, *(p[k] for k in PARAMS), 0.01)
    assert y.shape == x.shape and y.dtype == torch.float32
    y.backward(T(g[tag + "_dy"]).to(dev))
    assert_close(n(y), g[tag + "_y"], what=tag + " y", **y_tol)
    assert_close(n(x.grad), g[tag + "_dx"], what=tag + " dx", **g_tol)
    for k in PARAMS:
        assert p[k].grad.shape == p[k].shape
        assert_close(n(p[k].grad), g[f"{tag}_g_{k}"], what=f"{tag} g {k}", **sum_tol)


@pytest.mark.parametrize("tag", list(CASES))
def test_einfft_torch_matches_the_reference(tag):
    from dimsum_amd.ops.einfft import einfft_torch
    assert tuple(golden("einfft")[tag + "_x"].shape) == CASES[tag]
    check_einfft_against_fixture(einfft_torch, tag, "cpu", TOL, TOL, SUM_TOL)


@pytest.mark.parametrize("tag", list(CASES))
def test_operator_on_the_stand_ins_matches_the_reference(tag):
    """the autograd.Function's own backward (dft of dy, the mask chain, the bmm products, the column sums) on the stand-ins"""
    from dimsum_amd.ops.einfft import einfft
    with torch_einfft_backend():
        check_einfft_against_fixture(einfft, tag, "cpu", TOL, TOL, SUM_TOL)


def test_transform_passes_are_each_others_transpose():
    from dimsum_amd.ops.einfft import dft_torch, idft_real_torch
    x, gr, gi = (T(seeded((2, 32, 64), s)).double() for s in (1, 2, 3))
    re, im = dft_torch(x)
    lhs, rhs = (re * gr).sum() + (im * gi).sum(), (x * idft_real_torch(gr, gi)).sum()
    assert abs(lhs - rhs) <= 1e-12 * x.norm() * torch.sqrt(gr.norm() ** 2 + gi.norm() ** 2)
    assert torch.allclose(idft_real_torch(re, im), x, rtol=0, atol=1e-13)


def check_block_against_fixture(dev, tol, gtol, sum_tol):
    from dimsum_amd.models_dim import DiMBlockCombinedEinFFT, create_block
    g = golden("block_einfft")
    blk = create_block(64, **BLOCK_KW)
    assert type(blk) is DiMBlockCombinedEinFFT
    assert sorted(blk.state_dict().keys()) == [str(k) for k in g["keys"]]
    procedural_fill(blk, seed=9)
    blk = blk.to(dev)
    x, res, cc = (T(seeded(sh, sd)).to(dev).requires_grad_() for sh, sd in ((BLOCK_SHAPE, 141), (BLOCK_SHAPE, 142), ((2, 64), 143)))
    y, ro = blk(x, res, cc)
    ((y * T(seeded(BLOCK_SHAPE, 144)).to(dev)).sum() + (ro * T(seeded(BLOCK_SHAPE, 145)).to(dev)).sum()).backward()
    assert_close(n(y), g["y"], what="y", **tol)
    assert_close(n(ro), g["res_out"], what="res_out", **tol)
    assert_close(n(x.grad), g["dx"], what="dx", **gtol)
    assert_close(n(res.grad), g["dres"], what="dres", **gtol)
    assert_close(n(cc.grad), g["dc"], what="dc", **sum_tol)
    checked = 0
    for k, v in blk.named_parameters():
        if "g_" + k in g.files:
            assert_close(n(v.grad), g["g_" + k], what=k, **sum_tol)
        elif "g16_" + k in g.files:
            assert_close(n(v.grad[::16]), g["g16_" + k], what=k + "[::16]", **sum_tol)
        else:
            assert "cond_proj" in k and (v.grad is None or not v.grad.any()), k      # SURVEY finding 1: dead parameter
            continue
        checked += 1
    assert checked == len([f for f in g.files if f.startswith(("g_", "g16_"))]) >= 17
    assert all(f"g_freq_mamba.{k}" in g.files for k in PARAMS)


def test_block_on_the_cpu_oracle():
    with cpu_oracle_backend(), torch_einfft_backend():
        check_block_against_fixture("cpu", TOL, TOL, SUM_TOL)


def test_tiny_model_on_the_cpu_oracle_and_its_keys():
    from dimsum_amd.models_dim import DiM
    g = golden("model_tiny_einfft")
    assert float(g["shrink_pass"].max()) >= 0.2                 # not the all-shrunk case
    m = DiM(depth=4, hidden_size=64, patch_size=2, **_published(block_type="combined_einfft")).eval()
    keys = sorted(m.state_dict().keys())
    assert keys == [str(k) for k in g["keys"]] and len(keys) == int(g["n_keys"])
    assert [k for k in keys if k.startswith("blocks.0.freq_mamba.")] == ["blocks.0." + k for k in EINFFT_KEYS]
    sd = m.state_dict()
    assert sd["blocks.0.freq_mamba.complex_weight_1"].shape == (2, 4, 8, 8) and sd["blocks.0.freq_mamba.complex_bias_2"].shape == (2, 4, 8)
    procedural_fill(m, seed=3)
    x = T(g["x"]).clone().requires_grad_()
    with cpu_oracle_backend(), torch_einfft_backend():
        out = m(x, T(g["t"]), T(g["y"]))
        out.backward(T(g["dout"]))
    assert_close(out.detach().numpy(), g["out"], what="out", **TOL)
    assert_close(x.grad.numpy(), g["dx"], what="dx", **TOL)
    for b in m.blocks:
        assert all(getattr(b.freq_mamba, k).grad is not None and getattr(b.freq_mamba, k).grad.any() for k in PARAMS)


# ---- construction, refusals, parsers ---------------------------------------------------------------------------------------------------------------
def test_construction_and_refusals():
    from dimsum_amd.models_dim import DiM, DiMBlockCombinedEinFFT, DiMBlockRaw, EinFFT, create_block
    blk = create_block(64, block_type="combined_einfft")
    assert type(blk) is DiMBlockCombinedEinFFT and type(blk.freq_mamba) is EinFFT and type(blk.spatial_mamba) is DiMBlockRaw
    f = blk.freq_mamba
    assert (f.hidden_size, f.num_blocks, f.block_size, f.sparsity_threshold) == (32, 4, 8, 0.01)
    assert 0.01 < f.complex_weight_1.std().item() < 0.03                 # randn * 0.02
    for width in (32, 80):
        with pytest.raises(NotImplementedError, match="combined_einfft"):
            create_block(width, block_type="combined_einfft")
    with pytest.raises(NotImplementedError, match="combined_einfft"):      # a 3 x 3 token grid: 9 tokens
        DiM(depth=1, hidden_size=64, patch_size=2, **_published(block_type="combined_einfft", img_resolution=6))
    with pytest.raises(NotImplementedError, match="combined_einfft"):      # 64 x 64 tokens: above the LDS transform's 1024
        DiM(depth=1, hidden_size=64, patch_size=1, **_published(block_type="combined_einfft", img_resolution=64))
    m = DiM(depth=1, hidden_size=64, patch_size=2, **_published(block_type="combined_einfft"))
    assert m.block_type == "combined_einfft" and type(m.blocks[0]) is DiMBlockCombinedEinFFT


def test_parsers_take_the_seven_block_types():
    from dimsum_amd import sample_ddp, train
    from dimsum_amd.create_model import published_config
    seven = ("raw", "wave", "combined", "combined_fourier", "combined_einfft", "linear", "window")
    assert tuple(sorted(train.BLOCK_TYPES)) == tuple(sorted(seven))
    for parser in (train.build_parser, sample_ddp.build_parser):
        assert parser().parse_args([]).block_type == "combined"
        for bt in seven:
            assert parser().parse_args(["--block-type", bt]).block_type == bt
        with pytest.raises(SystemExit):
            parser().parse_args(["--block-type", "bogus"])
    assert published_config().block_type == "combined" and published_config(block_type="combined_einfft").block_type == "combined_einfft"


def test_wrappers_refuse_clearly():
    from dimsum_amd import native
    x = torch.zeros(2, 16, 32)
    w, b = torch.zeros(2, 4, 8, 8), torch.zeros(2, 4, 8)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        native.einfft_dft(x)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        native.einfft_idft_real(x, x)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        native.einfft_mlp_fwd(x, x, w, b, w, b, 0.01)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        native.einfft_mlp_bwd(x, x, x, x, x, x, w, b, w, b, 0.01)
    for N in (48, 2048, 8):
        with pytest.raises(RuntimeError, match="power of two"):
            native.einfft_dft(torch.zeros(1, N, 32))
    with pytest.raises(RuntimeError, match="multiple of 32"):
        native.einfft_dft(torch.zeros(1, 16, 40))
    with pytest.raises(RuntimeError, match="float32"):
        native.einfft_dft(x.half())


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------------------------
STRUCTS = [("dimsum_einfft_dft_params_t", "EinfftDftParams"), ("dimsum_einfft_mlp_params_t", "EinfftMlpParams"),
           ("dimsum_einfft_mlp_bwd_params_t", "EinfftMlpBwdParams")]
SYMBOLS = (("dimsum_einfft_dft", "EinfftDftParams"), ("dimsum_einfft_idft_real", "EinfftDftParams"), ("dimsum_einfft_mlp_fwd", "EinfftMlpParams"),
           ("dimsum_einfft_mlp_bwd", "EinfftMlpBwdParams"))


def test_struct_layouts_exports_and_stale_structs():
    from dimsum_amd import _lib
    pairs = [(c, getattr(_lib, m)) for c, m in STRUCTS]
    layout = _header_layout(pairs)
    for cname, mirror in pairs:
        size, offs = layout[cname]
        assert size == ctypes.sizeof(mirror), cname
        assert offs == {f: getattr(mirror, f).offset for f, _ in mirror._fields_}, cname
        assert mirror().struct_size == size
    lib = _lib.load()
    for name, m in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(lib, name)
        fn, p = getattr(lib, name), getattr(_lib, m)()
        assert fn(p, None) == 1                                   # a zeroed struct of the right size: the first NULL pointer, nothing launched
        p.struct_size -= 8
        assert fn(p, None) == 7                                   # a stale struct is refused before anything is read
        assert fn(None, None) == 1


def test_library_refuses_bad_shapes_before_any_launch():
    """every pointer set (to host memory that is never dereferenced: the checks run on the host and return before a launch)"""
    from dimsum_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    addr = ctypes.addressof(buf)
    P = _lib.EinfftDftParams()
    P.x = P.re = P.im = addr
    for B, N, C, want in ((1, 48, 32, 3), (1, 2048, 32, 3), (1, 8, 32, 3), (1, 16, 40, 3), (1, 16, 16, 3), (0, 16, 32, 3), (70000, 16, 32, 3)):
        P.batch, P.tokens, P.channels, P.x_batch_stride, P.x_token_stride = B, N, C, N * C, C
        assert lib.dimsum_einfft_dft(P, None) == want and lib.dimsum_einfft_idft_real(P, None) == want, (B, N, C)
    P.batch, P.tokens, P.channels, P.x_batch_stride, P.x_token_stride = 2, 16, 32, 16 * 32, 16
    assert lib.dimsum_einfft_dft(P, None) == 4                    # rows that overlap
    P.x_token_stride, P.x_batch_stride = 32, 32
    assert lib.dimsum_einfft_idft_real(P, None) == 4              # batch elements that overlap
    Q = _lib.EinfftMlpParams()
    for f in ("xr", "xi", "w1", "b1", "w2", "b2", "zr", "zi"):
        setattr(Q, f, addr)
    for rows, C, lam, want in ((0, 32, 0.01, 3), (4, 40, 0.01, 3), (4, 1056, 0.01, 3), (4, 32, -1.0, 3)):
        Q.rows, Q.channels, Q.lam = rows, C, lam
        assert lib.dimsum_einfft_mlp_fwd(Q, None) == want, (rows, C, lam)
    R = _lib.EinfftMlpBwdParams()
    R.fwd = Q
    R.fwd.rows, R.fwd.channels, R.fwd.lam = 4, 32, 0.01
    assert lib.dimsum_einfft_mlp_bwd(R, None) == 1                # the backward's own pointers are missing
