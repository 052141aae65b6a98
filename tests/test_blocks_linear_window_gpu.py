"""DiMBlock ("linear") and DiMBlockWindow ("window") on the HIP path vs the reference fixtures of tests/test_blocks_linear_window_cpu.py.
Tolerances are those of tests/test_model_gpu.py's block tests: rtol 2e-4 + 2e-5 * max|ref| on y, 5e-4 + 5e-5 on dx / dres, 1e-3 + 2e-4 on dc
and on parameter gradients, in exact fp32 and under allow_tf32 (split-bf16 products: fp32-class); an inference forward on operand images
(split-bf16, then the scaled-fp16 policy) holds the single-block f16s bound 1e-3 + 1e-3 * max|ref| and is not further from the golden than
1.25 x the maximum / 1.1 x the rms of the emulated-TF32 forward of the same block."""
import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.utils._python_dispatch import TorchDispatchMode

from conftest import assert_close, golden
from procedural import procedural_fill, seeded
from test_blocks_linear_window_cpu import CASES, SHAPE, check_block
from test_model_cpu import _published
from test_model_gpu import _count_f16s_products, f16s_policy  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
T = torch.from_numpy
Y_TOL, G_TOL, SUM_TOL = (dict(rtol=2e-4, atol=0.0, scale_atol=2e-5), dict(rtol=5e-4, atol=0.0, scale_atol=5e-5),
                         dict(rtol=1e-3, atol=0.0, scale_atol=2e-4))


@pytest.fixture(autouse=True)
def _fp32_matmul():
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.set_float32_matmul_precision("highest")


@pytest.mark.parametrize("tf32", [False, True])
@pytest.mark.parametrize("tag", list(CASES))
def test_block_forward_and_all_gradients_all_hip(tag, tf32):
    from dimsum_amd import utils
    before = utils.torch_path_counts()
    old = torch.backends.cuda.matmul.allow_tf32
    try:
        torch.backends.cuda.matmul.allow_tf32 = tf32
        check_block(tag, "cuda", Y_TOL, G_TOL, SUM_TOL)
    finally:
        torch.backends.cuda.matmul.allow_tf32 = old
    assert utils.torch_path_counts() == before


def _block(tag):
    from dimsum_amd.models_dim import create_block
    blk = create_block(128, **CASES[tag])
    procedural_fill(blk, seed=9)
    return blk.cuda().eval(), tuple(T(seeded(sh, sd)).cuda() for sh, sd in ((SHAPE, 101), (SHAPE, 102), ((2, 128), 103)))


def _vs_emulated_tf32(tag, blk, args, y):
    from dimsum_amd import gemm
    from dimsum_amd.utils.tf32_emulation import emulated_tf32
    gemm.set_policy("default")
    torch.backends.cuda.matmul.allow_tf32 = False
    with torch.no_grad(), emulated_tf32():
        y_tf = blk(*args)[0]
    ref = T(golden("block_" + tag)["y"]).cuda().double()
    e1, et, scale = (y.double() - ref).abs(), (y_tf.double() - ref).abs(), ref.abs().max().item()
    print(f"{tag} vs reference golden, max / rms over max|y|: {e1.max().item() / scale:.2e} / {e1.pow(2).mean().sqrt().item() / scale:.2e}, "
          f"emulated TF32 {et.max().item() / scale:.2e} / {et.pow(2).mean().sqrt().item() / scale:.2e}")
    assert e1.max().item() <= 1.25 * et.max().item() and e1.pow(2).mean().sqrt().item() <= 1.1 * et.pow(2).mean().sqrt().item()


@pytest.mark.parametrize("tag", list(CASES))
def test_block_inference_on_split_bf16_images_vs_reference_golden(tag, monkeypatch):
    """allow_tf32 with the operand images forced on (512 rows is below their default threshold): the pre-mixer pass writes the in_proj image,
    the norm_2 pass the w12 image; fp32-class, so the exact-fp32 tolerance holds -- and the emulated-TF32 yardstick"""
    monkeypatch.setenv("DIMSUM_SPLIT3_MIN_ROWS", "0")
    monkeypatch.setattr(torch.backends.cuda.matmul, "allow_tf32", True)
    blk, args = _block(tag)
    with torch.no_grad():
        y, ro = blk(*args)
    assert np.array_equal(ro.cpu().numpy(), golden("block_linear_window")["res_out"])
    assert_close(y.cpu().numpy(), golden("block_" + tag)["y"], what="y (allow_tf32, images)", **Y_TOL)
    _vs_emulated_tf32(tag, blk, args, y)


@pytest.mark.parametrize("tag", list(CASES))
def test_block_inference_under_the_f16s_policy_vs_reference_golden(tag, f16s_policy, monkeypatch):  # noqa: F811
    from dimsum_amd import utils
    blk, args = _block(tag)
    before = utils.torch_path_counts()
    seen = _count_f16s_products(monkeypatch)
    with torch.no_grad():
        y, ro = blk(*args)
    assert seen["f16s"] >= 1 and utils.torch_path_counts() == before, seen          # at least w12 + gate: 512 rows x 1024 fits the 256-row panels
    assert np.array_equal(ro.cpu().numpy(), golden("block_linear_window")["res_out"])
    assert_close(y.cpu().numpy(), golden("block_" + tag)["y"], 1e-3, 0, "y (f16s policy)", scale_atol=1e-3)
    _vs_emulated_tf32(tag, blk, args, y)


class _PassThrough(nn.Module):
    def forward(self, x, c=None, **kw):
        return x


def _flag_sweep():
    from dimsum_amd.models_dim import DiMBlock, DiMBlockWindow
    mixer = lambda dim: _PassThrough()
    for r in (False, True):
        for t in (False, True):
            for k in (False, True):
                yield DiMBlock(128, mixer, norm_cls=nn.Identity, reverse=r, transpose=t, scanning_continuity=k)
                yield DiMBlockWindow(128, mixer, norm_cls=nn.Identity, reverse=r, transpose=t, shift_window=k)


@pytest.mark.parametrize("grad", [False, True])
def test_permutation_only(grad):
    """norms, mixer and MLP replaced by the identity. Gates 0 (shift / scale arbitrary): the output IS the input, bit for bit. Mixer gate 1,
    shift = scale = 0: the mixer branch is P^-1(P(x)), so the output is exactly 2 x -- a wrong inverse table moves tokens and shows here."""
    x = T(seeded(SHAPE, 106)).cuda()
    c = torch.zeros(2, 128, device="cuda")
    for blk in _flag_sweep():
        blk.mlp = _PassThrough()
        blk = blk.cuda()
        lin = blk.adaLN_modulation[1]
        for gate_ssm, want in ((0.0, x), (1.0, 2 * x)):
            with torch.no_grad():
                lin.weight.zero_()
                b = lin.bias.view(6, 128)
                b[:] = T(seeded((6, 128), 107)).cuda() if gate_ssm == 0.0 else 0.0
                b[2], b[5] = gate_ssm, 0.0
            with torch.set_grad_enabled(grad):
                y, res = blk(x.clone().requires_grad_(grad), None, c)
            what = (type(blk).__name__, blk.reverse, blk.transpose, blk.scanning_continuity, getattr(blk, "shift_window", None), gate_ssm)
            assert torch.equal(y.detach(), want), what
            assert torch.equal(res.detach(), x), what


@pytest.mark.usefixtures("allow_torch_sdpa")        # (the shared DiTBlock of a hidden-64 model has head_dim 4: conftest)
@pytest.mark.parametrize("block_type", ["linear", "window"])
def test_tiny_models_forward(block_type):
    from dimsum_amd.models_dim import DiM
    g = golden("model_tiny_" + block_type)
    m = DiM(depth=4, hidden_size=64, patch_size=2, **_published(block_type=block_type))
    procedural_fill(m, seed=3)
    m = m.cuda().eval()
    with torch.no_grad():
        out = m(T(g["x"]).cuda(), T(g["t"]).cuda(), T(g["y"]).cuda())
    assert_close(out.cpu().numpy(), g["out"], 2e-4, 0, "out", scale_atol=2e-5)


class _AtenLog(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.ops = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.ops.append(str(func))
        return func(*args, **(kwargs or {}))


_REORDER_OPS = ("index_select", "gather", "flip", "roll", "aten.index.", "take", "scatter", "index_put", "index_copy", "index_add")


@pytest.mark.parametrize("grad", [False, True])
@pytest.mark.parametrize("tag", ["linear_r1t1c1", "linear_default", "window_t1"])
def test_the_reorder_lives_inside_the_token_passes(tag, grad, monkeypatch):
    """launch spy: a block forward calls token_transform once with the table on its output side (pre-mixer) and once on its input side
    (post-mixer), and no torch gather / index_select / flip / roll runs"""
    from dimsum_amd import native
    blk, args = _block(tag)
    tables = {"out": 0, "in": 0}
    real = native.token_transform

    def spy(*a, **kw):
        tables["out"] += int(kw.get("out_index") is not None)
        tables["in"] += int(kw.get("in_index") is not None)
        return real(*a, **kw)
    monkeypatch.setattr(native, "token_transform", spy)
    blk(*args)          # (tables are built on the first call)
    tables.update({"out": 0, "in": 0})
    with torch.set_grad_enabled(grad), _AtenLog() as log:
        blk(*(a.clone().requires_grad_(grad) for a in args))
    assert tables == {"out": 1, "in": 1}, tables
    assert len(log.ops) > 0 and not [op for op in log.ops if any(s in op for s in _REORDER_OPS)], log.ops
