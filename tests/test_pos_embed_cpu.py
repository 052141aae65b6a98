"""The rope and cpe positional encodings without a GPU: the rotary tables against the reference's (tests/golden/pe_rope.npz, bit for bit), the
state_dict layouts, the constructor's refusals, the C ABI of the three new entry points (struct layouts, stale structs refused, exported
symbols), the host wrappers' refusals, and both tiny models against their reference fixtures on the CPU oracle backend -- with the three new
native entry points replaced by the plain-torch restatements below, stacked on cpu_oracle_backend() (the oracle package knows nothing of them).
Tolerance of the model tests: test_model_cpu.TOL."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close, golden
from oracle.torch_backend import cpu_oracle_backend
from procedural import procedural_fill
from test_host_logic import _header_layout
from test_model_cpu import TOL, _published

T = torch.from_numpy
CPE_KEYS = ["pos_cnn.adaLN_modulation.1.bias", "pos_cnn.adaLN_modulation.1.weight", "pos_cnn.norm.bias", "pos_cnn.norm.weight",
            "pos_cnn.proj.0.bias", "pos_cnn.proj.0.weight"]


# ---- plain-torch restatements of native.pos_rope / pos_cpe_fwd / pos_cpe_bwd (same signatures and results) ----------------------------------
def _rotate_half(x):
    r = torch.empty_like(x)
    r[..., 0::2], r[..., 1::2] = -x[..., 1::2], x[..., 0::2]
    return r


def pos_rope(x, sin, cos, inverse=False):
    if not inverse:
        return x * cos + _rotate_half(x) * sin
    g = x * sin                               # the transpose of the map above: d/dx <dy, x cos + R x sin> = dy cos + R^T (dy sin), R^T = -R
    return x * cos - _rotate_half(g)


def _cpe(x, weight, bias, gamma, beta, shift, scale, grid, eps):
    B, L, C = x.shape
    img = x.transpose(1, 2).reshape(B, C, grid, grid)
    v = (F.conv2d(img, weight.reshape(C, 1, 3, 3), bias, padding=1, groups=C) + img).flatten(2).transpose(1, 2)
    return F.layer_norm(v, (C,), gamma, beta, eps) * (1 + scale.unsqueeze(1)) + shift.unsqueeze(1), v


def pos_cpe_fwd(x, weight, bias, gamma, beta, shift, scale, grid, eps=1e-5, need_stats=False, need_v=False):
    with torch.no_grad():
        y, v = _cpe(x, weight, bias, gamma, beta, shift, scale, grid, eps)
        mean = v.mean(-1).reshape(-1)
        rstd = (v.var(-1, unbiased=False) + eps).rsqrt().reshape(-1)
    return y, (mean if need_stats else None), (rstd if need_stats else None), (v if need_v else None)


def pos_cpe_bwd(dy, x, weight, bias, gamma, beta, shift, scale, mean, rstd, grid, eps=1e-5):
    leaves = [t.detach().clone().requires_grad_() for t in (x, weight, bias, gamma, beta, shift, scale)]
    with torch.enable_grad():
        y, _ = _cpe(*leaves, grid, eps)
        dx, dw, db, dg, dbeta, dshift, dscale = torch.autograd.grad(y, leaves, dy)
    return dx, dw, db, dg, dbeta, torch.cat([dshift, dscale], dim=1)


@contextlib.contextmanager
def torch_pos_backend():
    from dimsum_amd import native
    saved = {n: getattr(native, n) for n in ("pos_rope", "pos_cpe_fwd", "pos_cpe_bwd")}
    try:
        native.pos_rope, native.pos_cpe_fwd, native.pos_cpe_bwd = pos_rope, pos_cpe_fwd, pos_cpe_bwd
        yield
    finally:
        for n, f in saved.items():
            setattr(native, n, f)


# ---- tables, keys, refusals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden,grid", [(64, 4), (128, 16)])
def test_rotary_tables_equal_the_reference_bitwise(hidden, grid):
    from dimsum_amd.pe.my_rotary import get_2d_sincos_rotary_embed
    g = golden("pe_rope")
    sin, cos = get_2d_sincos_rotary_embed(hidden, grid)
    assert sin.shape == cos.shape == (grid * grid, hidden)
    for got, key in ((sin, "sin"), (cos, "cos")):
        want = g[f"H{hidden}_g{grid}_{key}"]
        got = T(got).to(dtype=torch.float32).numpy()
        assert want.dtype == np.float32 and np.array_equal(got, want), key
        assert np.array_equal(got[:, 0::2], got[:, 1::2])             # one frequency per channel pair


def test_model_tables_are_buffers_outside_the_state_dict():
    from dimsum_amd.models_dim import DiM
    m = DiM(depth=4, hidden_size=64, patch_size=2, **_published(pe_type="rope"))
    from dimsum_amd.pe.my_rotary import get_2d_sincos_rotary_embed
    sin, cos = get_2d_sincos_rotary_embed(64, 16)
    assert m.emb_sin.dtype == m.emb_cos.dtype == torch.float32 and m.emb_sin.shape == (256, 64)
    assert torch.equal(m.emb_sin, T(sin).float()) and torch.equal(m.emb_cos, T(cos).float())
    assert {"emb_sin", "emb_cos"} <= {n for n, _ in m.named_buffers()}
    assert not [k for k in m.state_dict() if "emb_" in k]


def test_state_dict_keys():
    from dimsum_amd.models_dim import DiM
    ape = sorted(DiM(depth=4, hidden_size=64, patch_size=2, **_published()).state_dict().keys())
    for pe in ("rope", "cpe"):
        g = golden("model_tiny_" + pe)
        m = DiM(depth=4, hidden_size=64, patch_size=2, **_published(pe_type=pe))
        keys = sorted(m.state_dict().keys())
        assert keys == [str(k) for k in g["keys"]] and len(keys) == int(g["n_keys"])
        if pe == "rope":
            assert keys == ape
        else:
            assert sorted(set(keys) - set(ape)) == CPE_KEYS and set(ape) <= set(keys)
            sd = m.state_dict()
            assert sd["pos_cnn.proj.0.weight"].shape == (64, 1, 3, 3) and sd["pos_cnn.adaLN_modulation.1.weight"].shape == (128, 64)
            assert m.pos_cnn.norm.eps == torch.nn.LayerNorm(64).eps and m.pos_cnn.norm.elementwise_affine
            # initialize_weights leaves this head alone; _init_weights zeroes its Linear bias (models_dim.py:1761-1779, 1969-1975)
            assert not sd["pos_cnn.adaLN_modulation.1.bias"].any() and sd["pos_cnn.adaLN_modulation.1.weight"].any()


def test_refusals_and_defaults():
    from dimsum_amd.models_dim import DiM
    with pytest.raises(ValueError, match="pe_type"):
        DiM(depth=1, hidden_size=64, patch_size=2, **_published(pe_type="bogus"))
    m = DiM(depth=1, hidden_size=64, patch_size=2, **_published())
    assert m.pe_type == "ape" and not hasattr(m, "pos_cnn") and not hasattr(m, "emb_sin")
    assert DiM(depth=1, hidden_size=64, patch_size=2, img_resolution=32, num_classes=10).pe_type == "ape"
    from dimsum_amd.train import build_parser
    assert build_parser().parse_args([]).pe_type == "ape" and build_parser().parse_args(["--pe-type", "cpe"]).pe_type == "cpe"
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--pe-type", "bogus"])


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------------------
STRUCTS = [("dimsum_pos_rope_params_t", "PosRopeParams"), ("dimsum_pos_cpe_params_t", "PosCpeParams"), ("dimsum_pos_cpe_bwd_params_t", "PosCpeBwdParams")]
SYMBOLS = ("dimsum_pos_rope", "dimsum_pos_cpe_fwd", "dimsum_pos_cpe_bwd")


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
    assert lib.dimsum_abi_version() == 18
    for name, (_, m) in zip(SYMBOLS, STRUCTS):
        assert name in _lib.EXPORTS and hasattr(lib, name)
        fn, ptype = getattr(lib, name), getattr(_lib, m)
        p = ptype()
        assert fn(p, None) == 1                                   # a zeroed struct of the right size: the first NULL pointer, nothing launched
        p.struct_size -= 8
        assert fn(p, None) == 7                                   # a stale struct is refused before anything is read
        assert fn(None, None) == 1


def test_library_refuses_bad_shapes_before_any_launch():
    """every pointer set (to host memory that is never dereferenced: the checks run on the host and return before a launch)"""
    from dimsum_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    addr = ctypes.addressof(buf) // 16 * 16 + 16
    P = _lib.PosRopeParams()
    P.x = P.sin = P.cos = P.y = addr
    for B, L, C, want in ((1, 1, 6, 3), (1, 1, 0, 3), (0, 1, 4, 3), (1, 0, 4, 3)):
        P.batch, P.tokens, P.channels = B, L, C
        P.x_batch_stride = P.y_batch_stride = L * C
        P.x_token_stride = P.y_token_stride = C
        assert lib.dimsum_pos_rope(P, None) == want, (B, L, C)
    P.batch, P.tokens, P.channels, P.x_token_stride, P.y_token_stride = 1, 1, 8, 4, 8
    assert lib.dimsum_pos_rope(P, None) == 4                       # rows that overlap
    P.x_token_stride, P.x = 8, addr + 4
    assert lib.dimsum_pos_rope(P, None) == 4                       # not 16-byte aligned
    Q = _lib.PosCpeParams()
    for n in ("x", "weight", "conv_bias", "gamma", "beta", "shift", "scale", "y"):
        setattr(Q, n, addr)
    for B, G, C, want in ((1, 2, 2052, 3), (1, 2, 6, 3), (1, 0, 8, 3), (70000, 2, 8, 3)):
        Q.batch, Q.grid, Q.channels = B, G, C
        Q.x_token_stride = Q.y_token_stride = Q.mod_batch_stride = C
        Q.x_batch_stride = Q.y_batch_stride = G * G * C
        assert lib.dimsum_pos_cpe_fwd(Q, None) == want, (B, G, C)
    Q.batch, Q.grid, Q.channels = 1, 2, 8
    Q.x_token_stride = Q.y_token_stride = Q.mod_batch_stride = 8
    Q.x_batch_stride = Q.y_batch_stride = 32
    Q.mean = addr                                                  # mean without rstd
    assert lib.dimsum_pos_cpe_fwd(Q, None) == 1


def test_wrappers_refuse_clearly():
    from dimsum_amd import native
    x = torch.zeros(2, 16, 8)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        native.pos_rope(x, torch.zeros(16, 8), torch.zeros(16, 8))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        native.pos_cpe_fwd(x, torch.zeros(8, 1, 3, 3), *(torch.zeros(8),) * 3, torch.zeros(2, 8), torch.zeros(2, 8), 4)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        native.pos_rope(torch.zeros(2, 16, 6), torch.zeros(16, 6), torch.zeros(16, 6))
    with pytest.raises(RuntimeError, match="float32"):
        native.pos_rope(x.half(), torch.zeros(16, 8), torch.zeros(16, 8))
    with pytest.raises(RuntimeError, match="square grid"):
        native._square_grid("pos_cpe_fwd", 12, 3)


# ---- the restatements against the reference, then the models on them ---------------------------------------------------------------------------
def test_restatements_match_the_reference_fixtures():
    g = golden("pe_rope")
    from procedural import seeded
    sin, cos = T(g["H64_g4_sin"]), T(g["H64_g4_cos"])
    x, dy = T(seeded((2, 16, 64), 111)), T(seeded((2, 16, 64), 113))
    assert torch.equal(pos_rope(x, sin, cos), T(g["H64_g4_y"]))
    assert torch.equal(pos_rope(dy, sin, cos, inverse=True), T(g["H64_g4_dx"]))


def check_ops_against_pe_fixtures(dev, y_tol, g_tol, sum_tol):
    """ops.pos_embed.rotary / the AdaInPosCNN module against pe_rope.npz / pe_cpe.npz: forward, dx, dc and the six parameter gradients"""
    from dimsum_amd.ops import pos_embed
    from dimsum_amd.pe.cpe import AdaInPosCNN
    from procedural import seeded
    n = lambda t: t.detach().cpu().numpy()
    g = golden("pe_rope")
    x = T(seeded((2, 16, 64), 111)).to(dev).requires_grad_()
    y = pos_embed.rotary(x, T(g["H64_g4_sin"]).to(dev), T(g["H64_g4_cos"]).to(dev))
    y.backward(T(seeded((2, 16, 64), 113)).to(dev))
    bound = 4 * 2.0 ** -24 * (np.abs(n(x))[..., 0::2] + np.abs(n(x))[..., 1::2]).repeat(2, axis=-1)
    assert (np.abs(n(y).astype(np.float64) - g["H64_g4_y"]) <= bound).all()
    dyv = np.abs(seeded((2, 16, 64), 113))
    assert (np.abs(n(x.grad).astype(np.float64) - g["H64_g4_dx"]) <= 4 * 2.0 ** -24 * (dyv[..., 0::2] + dyv[..., 1::2]).repeat(2, axis=-1)).all()
    g = golden("pe_cpe")
    for i, (B, grid, C) in enumerate(((2, 4, 64), (2, 6, 136))):
        tag = f"B{B}_g{grid}_C{C}"
        m = AdaInPosCNN(C, C)
        procedural_fill(m, seed=13)
        m = m.to(dev)
        x = T(seeded((B, grid * grid, C), 121 + i)).to(dev).requires_grad_()
        c = T(seeded((B, C), 123 + i)).to(dev).requires_grad_()
        y = m(x, c, H=grid, W=grid)
        y.backward(T(seeded((B, grid * grid, C), 125 + i)).to(dev))
        assert_close(n(y), g[tag + "_y"], what=tag + " y", **y_tol)
        assert_close(n(x.grad), g[tag + "_dx"], what=tag + " dx", **g_tol)
        assert_close(n(c.grad), g[tag + "_dc"], what=tag + " dc", **sum_tol)
        seen = 0
        for k, v in m.named_parameters():
            if f"{tag}_g_{k}" in g.files:
                assert_close(n(v.grad), g[f"{tag}_g_{k}"], what=f"{tag} g {k}", **sum_tol)
            else:
                assert_close(n(v.grad[::16]), g[f"{tag}_g16_{k}"], what=f"{tag} g16 {k}", **sum_tol)
            seen += 1
        assert seen == 6


def test_ops_on_the_restatements_match_the_reference_fixtures():
    with torch_pos_backend():
        check_ops_against_pe_fixtures("cpu", TOL, TOL, dict(rtol=5e-4, atol=0, scale_atol=1e-4))


@pytest.mark.parametrize("pe", ["rope", "cpe"])
def test_tiny_models_on_the_cpu_oracle(pe):
    from dimsum_amd.models_dim import DiM
    g = golden("model_tiny_" + pe)
    m = DiM(depth=4, hidden_size=64, patch_size=2, **_published(pe_type=pe)).eval()
    procedural_fill(m, seed=3)
    x = T(g["x"]).clone().requires_grad_()
    with cpu_oracle_backend(), torch_pos_backend():
        out = m(x, T(g["t"]), T(g["y"]))
        out.backward(T(g["dout"]))
    assert_close(out.detach().numpy(), g["out"], what="out", **TOL)
    assert_close(x.grad.numpy(), g["dx"], what="dx", **TOL)
    if pe == "rope":
        assert m.pos_embed.requires_grad and m.pos_embed.grad is None          # unused, as in the reference
    else:
        assert all(p.grad is not None and p.grad.any() for p in m.pos_cnn.parameters())


@pytest.mark.parametrize("pe", ["rope", "cpe"])
def test_ddp_wrapper_takes_the_unused_pos_embed(pe, tmp_path):
    """two steps through build_training's DistributedDataParallel branch (gloo, one process): without a frozen pos_embed the second step
    raises "Expected to have finished reduction in the prior iteration" """
    import torch.distributed as dist
    from dimsum_amd.models_dim import DiM
    from dimsum_amd.train import build_training, train_step
    from dimsum_amd.transport import create_transport
    from procedural import seeded
    m = DiM(depth=2, hidden_size=64, patch_size=2, **_published(pe_type=pe, use_attn_every_k_layers=-1))
    procedural_fill(m, seed=3)
    before = m.pos_embed.detach().clone()
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/store", rank=0, world_size=1)
    try:
        model, ema, opt = build_training(m, "cpu", lr=1e-3, world_size=2, fused_step=False)
        assert isinstance(model, torch.nn.parallel.DistributedDataParallel)
        x, y = T(seeded((2, 4, 32, 32), 81)), torch.tensor([1, 22])
        tr = create_transport("GVP", "velocity")
        torch.manual_seed(0)
        with cpu_oracle_backend(), torch_pos_backend():
            for _ in range(2):
                assert torch.isfinite(train_step(model.train(), ema, opt, tr, x, y)).item()
    finally:
        dist.destroy_process_group()
    assert torch.equal(m.pos_embed, before) and m.pos_embed.grad is None
