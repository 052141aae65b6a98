"""The rope and cpe positional encodings on the HIP passes (csrc/pos_embed.hip): against the reference fixtures pe_rope.npz / pe_cpe.npz where
stored, against the torch composition in float64 on the CPU elsewhere; the zero-padding of the 3x3 window bit for bit; both tiny models against
their goldens with a spy on the aten ops of the forward; two training steps per encoding; hipGraph replay of the rope model.
Bounds: rope forward elementwise 4 * 2^-24 * (|x_even| + |x_odd|) (two fp32 products and one add, with or without FMA contraction; |sin|,
|cos| <= 1), the round trip twice that; cpe: Y_TOL / G_TOL / SUM_TOL of tests/test_blocks_linear_window_gpu.py."""
from collections import Counter

import numpy as np
import pytest
import torch

from conftest import assert_close, golden
from procedural import procedural_fill, seeded
from test_blocks_linear_window_gpu import G_TOL, SUM_TOL, Y_TOL, _AtenLog
from test_model_cpu import _published
from test_pos_embed_cpu import _cpe, check_ops_against_pe_fixtures
from test_train_gpu import KW, _fixed_transport

pytestmark = pytest.mark.gpu
T = torch.from_numpy
n = lambda t: t.detach().cpu().numpy()      # noqa: E731


@pytest.fixture(autouse=True)
def _fp32_matmul():
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.set_float32_matmul_precision("highest")


def _pair_bound(x):
    a = np.abs(np.asarray(x, np.float64))
    return 4 * 2.0 ** -24 * (a[..., 0::2] + a[..., 1::2]).repeat(2, axis=-1)


def test_ops_match_the_reference_fixtures():
    """rotary at (2, 4, 64) and AdaInPosCNN at (2, 4, 64), (2, 6, 136): y, dx, dc and the six parameter gradients of the reference"""
    check_ops_against_pe_fixtures("cuda", Y_TOL, G_TOL, SUM_TOL)


@pytest.mark.parametrize("B,grid,C", [(2, 4, 64), (3, 6, 136), (2, 4, 1152)])
def test_rope_forward_inverse_and_backward(B, grid, C):
    from dimsum_amd import native
    from dimsum_amd.ops import pos_embed
    from dimsum_amd.pe.my_rotary import get_2d_sincos_rotary_embed
    sin, cos = (T(t).to(dtype=torch.float32) for t in get_2d_sincos_rotary_embed(C, grid))
    x = T(seeded((B, grid * grid, C), 131))
    xd, rot = x.double(), torch.empty(x.shape, dtype=torch.float64)
    rot[..., 0::2], rot[..., 1::2] = -xd[..., 1::2], xd[..., 0::2]
    ref = (xd * cos.double() + rot * sin.double()).numpy()
    xg = x.cuda().requires_grad_()
    y = pos_embed.rotary(xg, sin.cuda(), cos.cuda())
    err = np.abs(n(y).astype(np.float64) - ref)
    print(f"rope {B, grid, C}: max err / bound {np.max(err / np.maximum(_pair_bound(x), 1e-300)):.3f}")
    assert (err <= _pair_bound(x)).all()
    back = native.pos_rope(y.detach(), sin.cuda(), cos.cuda(), inverse=True)
    assert (np.abs(n(back).astype(np.float64) - x.numpy()) <= 2 * _pair_bound(x)).all()
    dy = T(seeded((B, grid * grid, C), 132)).cuda()
    y.backward(dy)
    assert torch.equal(xg.grad, native.pos_rope(dy, sin.cuda(), cos.cuda(), inverse=True))
    # a batch-strided view (the first half of the channels of a wider tensor) is read in place
    wide = T(seeded((B, grid * grid, 2 * C), 133)).cuda()
    assert torch.equal(native.pos_rope(wide[..., :C], sin.cuda(), cos.cuda()), native.pos_rope(wide[..., :C].contiguous(), sin.cuda(), cos.cuda()))


def _module(C, dev, dtype=torch.float32):
    from dimsum_amd.pe.cpe import AdaInPosCNN
    m = AdaInPosCNN(C, C)
    procedural_fill(m, seed=13)
    return m.to(device=dev, dtype=dtype)


@pytest.mark.parametrize("B,grid,C", [(1, 1, 64), (2, 3, 1152)])
def test_cpe_against_float64_torch(B, grid, C):
    """the shapes without a fixture: a single token without neighbours; XL/2's width on a 3 x 3 grid (one interior token)"""
    L = grid * grid
    x, c, dy = seeded((B, L, C), 141), seeded((B, C), 142), seeded((B, L, C), 143)
    m = _module(C, "cuda")
    xg, cg = T(x).cuda().requires_grad_(), T(c).cuda().requires_grad_()
    y = m(xg, cg, H=grid, W=grid)
    y.backward(T(dy).cuda())
    r = _module(C, "cpu", torch.float64)
    xr, cr = T(x).double().requires_grad_(), T(c).double().requires_grad_()
    shift, scale = r.adaLN_modulation(cr).chunk(2, dim=1)
    yr, _ = _cpe(xr, r.proj[0].weight, r.proj[0].bias, r.norm.weight, r.norm.bias, shift, scale, grid, r.norm.eps)
    yr.backward(T(dy).double())
    assert_close(n(y), n(yr), what="y", **Y_TOL)
    assert_close(n(xg.grad), n(xr.grad), what="dx", **G_TOL)
    assert_close(n(cg.grad), n(cr.grad), what="dc", **SUM_TOL)
    for (k, p), (_, q) in zip(m.named_parameters(), r.named_parameters()):
        assert p.grad is not None and p.grad.data_ptr() % 16 == 0 and p.grad._base is None, k      # a tensor of its own
        assert_close(n(p.grad), n(q.grad), what="g " + k, **SUM_TOL)


@pytest.mark.parametrize("grid,C", [(4, 64), (5, 136)])
def test_cpe_zero_padding_and_neighbour_indices(grid, C):
    """centre tap 1, bias 0: v == 2 x exactly and y is the fused LayerNorm + modulate pass on 2 x. One off-centre tap of 1: v is x plus x moved by
    one grid cell with zeros entering at the border, bit for bit -- for each of the eight neighbours"""
    from dimsum_amd import native
    B, L = 2, grid * grid
    x = T(seeded((B, L, C), 151)).cuda()
    gamma, beta = (T(seeded((C,), s, scale=0.3)).cuda() for s in (152, 153))
    gamma += 1
    mod = T(seeded((B, 2 * C), 154, scale=0.3)).cuda()
    shift, scale = mod[:, :C], mod[:, C:]
    zero = torch.zeros(C, device="cuda")
    for i in range(3):
        for j in range(3):
            w = torch.zeros(C, 1, 3, 3, device="cuda")
            w[:, 0, i, j] = 1
            y, _, _, v = native.pos_cpe_fwd(x, w, zero, gamma, beta, shift, scale, grid, 1e-5, need_v=True)
            img = x.view(B, grid, grid, C)
            moved = torch.zeros_like(img)             # moved[h, w] = x[h + i - 1, w + j - 1] inside the grid
            hs, ws = slice(max(0, 1 - i), grid - max(0, i - 1)), slice(max(0, 1 - j), grid - max(0, j - 1))
            hd, wd = slice(max(0, i - 1), grid - max(0, 1 - i)), slice(max(0, j - 1), grid - max(0, 1 - j))
            moved[:, hs, ws] = img[:, hd, wd]
            # (v = fl(x + neighbour) is ONE rounding, so "v - x" is compared in the form that is exact in fp32: v against x + moved)
            assert torch.equal(v, x + moved.view(B, L, C)), (i, j)
            border = (moved.view(B, L, C) == 0).all(-1)
            assert torch.equal(v[border], x[border]) and int(border.sum()) == (B * (2 * grid - 1) if (i != 1 and j != 1) else B * grid if (i, j) != (1, 1) else 0)
            if (i, j) == (1, 1):
                assert torch.equal(v, 2 * x)
                ln = native.layer_norm_fwd((2 * x).view(B * L, C), gamma, beta, 1e-5, is_rms_norm=False, mod_scale=scale, mod_shift=shift,
                                           rows_per_batch=L)[0]
                assert_close(n(y), n(ln.view(B, L, C)), what="y vs the fused norm pass", **Y_TOL)


def test_cpe_refuses_what_it_cannot_run():
    from dimsum_amd import native
    x = torch.zeros(1, 4, 2052, device="cuda")
    with pytest.raises(RuntimeError, match="2048"):
        native.pos_cpe_fwd(x, torch.zeros(2052, 1, 3, 3, device="cuda"), *(torch.zeros(2052, device="cuda"),) * 3,
                           *(torch.zeros(1, 2052, device="cuda"),) * 2, 2)
    with pytest.raises(RuntimeError, match="square grid"):
        native.pos_cpe_fwd(torch.zeros(1, 6, 8, device="cuda"), torch.zeros(8, 1, 3, 3, device="cuda"), *(torch.zeros(8, device="cuda"),) * 3,
                           *(torch.zeros(1, 8, device="cuda"),) * 2, 2)


def _tiny(pe):
    from dimsum_amd.models_dim import DiM
    m = DiM(depth=4, hidden_size=64, patch_size=2, **_published(pe_type=pe))
    procedural_fill(m, seed=3)
    return m.cuda().eval()


@pytest.mark.usefixtures("allow_torch_sdpa")        # (the shared DiTBlock of a hidden-64 model has head_dim 4: conftest)
@pytest.mark.parametrize("pe", ["rope", "cpe"])
def test_tiny_models_forward_all_hip(pe):
    from dimsum_amd import utils
    g = golden("model_tiny_" + pe)
    m = _tiny(pe)
    args = tuple(T(g[k]).cuda() for k in ("x", "t", "y"))
    with torch.no_grad():
        m(*args)                                    # (lazy tables)
    before = utils.torch_path_counts()
    with torch.no_grad(), _AtenLog() as log:
        out = m(*args)
    added = Counter(utils.torch_path_counts()) - Counter(before)
    assert_close(out.cpu().numpy(), g["out"], 2e-4, 0, "out", scale_atol=2e-5)
    assert len(log.ops) > 0
    assert len([op for op in log.ops if "conv" in op]) <= 1, log.ops      # at most the patch embed's own (a Linear here): the 3x3 conv is in the HIP pass
    assert not [op for op in log.ops if "native_layer_norm" in op], log.ops
    # what the encoding adds to the "ape" forward's aten ops: no copy into a strided slice, nothing elementwise (rotate_half as torch ops is
    # two copy_ into x_r[..., 0::2] / [..., 1::2], a neg and two mul), no staging clone
    ape = _tiny("ape")
    with torch.no_grad():
        ape(*args)
        before = utils.torch_path_counts()
        with _AtenLog() as base:
            ape(*args)
    # the torch-path book (a hidden-64 model's head_dim-4 attention cores, opted into above) moves by what the "ape" forward moves it: the
    # encoding itself is on no torch path
    assert added == Counter(utils.torch_path_counts()) - Counter(before), added
    extra = Counter(log.ops) - Counter(base.ops)
    assert not [op for op in extra if any(s in op for s in ("copy_", "slice_scatter", "aten.neg", "aten.mul", "aten.clone", "aten.index"))], extra


@pytest.mark.usefixtures("allow_torch_sdpa")
@pytest.mark.parametrize("fused_step", [False, True])
@pytest.mark.parametrize("pe", ["rope", "cpe"])
def test_two_training_steps(pe, fused_step):
    from dimsum_amd.models_dim import DiM
    from dimsum_amd.train import build_training, train_step
    m = DiM(depth=4, hidden_size=64, patch_size=2, **dict(KW, pe_type=pe))
    procedural_fill(m, seed=3)
    model, ema, opt = build_training(m.cuda(), "cuda", lr=1e-3, fused_step=fused_step)
    start = {k: v.detach().clone() for k, v in model.named_parameters()}
    x, y = T(seeded((4, 4, 32, 32), 81)).cuda(), torch.tensor([1, 22, 333, 999], device="cuda")
    tr = _fixed_transport(T(seeded((4,), 82, kind="uniform")), T(seeded((4, 4, 32, 32), 83)))
    for _ in range(2):
        loss = train_step(model.train(), ema, opt, tr, x, y, max_grad_norm=2.0, ema_decay=0.5)
        assert torch.isfinite(loss).item()
    now = dict(model.named_parameters())
    if pe == "cpe":
        for k in start:
            if k.startswith("pos_cnn."):
                assert not torch.equal(now[k], start[k]), k
        assert sum(k.startswith("pos_cnn.") for k in start) == 6
    else:
        assert now["pos_embed"].grad is None and torch.equal(now["pos_embed"], start["pos_embed"])
    assert not torch.equal(now["x_embedder.proj.weight"], start["x_embedder.proj.weight"])


@pytest.mark.usefixtures("allow_torch_sdpa")
def test_hip_graph_replay_of_the_rope_model_is_bit_identical():
    from dimsum_amd.hip_graph import GraphedForward
    m = _tiny("rope")
    g = GraphedForward(m)
    gen = torch.Generator(device="cuda").manual_seed(0)
    for _ in range(2):
        x, t = torch.randn(4, 4, 32, 32, device="cuda", generator=gen), torch.rand(4, device="cuda", generator=gen)
        y = torch.randint(0, 1000, (4,), device="cuda", generator=gen)
        with torch.no_grad():
            ref = m(x, t, y)
        assert torch.equal(g(x, t, y), ref)
    assert len(g.graphs) == 1
