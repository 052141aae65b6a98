"""DiMBlock (block_type "linear" and every unlisted value) and DiMBlockWindow ("window") on the CPU oracle backend vs fixtures captured from
the reference blocks with identical procedural weights (tools/gen_golden.py::gen_block_linear_window, gen_model_tiny_linear_window).
Tolerance: the one test_model_cpu.py holds block_combined to -- rtol 2e-4 + 2e-5 * max|ref| on y / dx / dres, rtol 5e-4 + 1e-4 * max|ref| on
dc; parameter gradients are sums over the tokens like dc and take dc's."""
import numpy as np
import pytest
import torch

from conftest import assert_close, golden
from oracle.torch_backend import cpu_oracle_backend
from procedural import procedural_fill, seeded
from test_model_cpu import TOL, _published

T = torch.from_numpy
SUM_TOL = dict(rtol=5e-4, atol=0, scale_atol=1e-4)
PUBLISHED = dict(norm_epsilon=1e-5, rms_norm=True, residual_in_fp32=True, fused_add_norm=True, layer_idx=1, scan_type="none", cond_mamba=True,
                 use_gated_mlp=True)
# fixture tag -> create_block keywords (the same table as tools/gen_golden.py::LW_CASES)
CASES = {f"linear_r{r}t{t}c{c}": dict(PUBLISHED, block_type="linear", reverse=bool(r), transpose=bool(t), scanning_continuity=bool(c))
         for r in (0, 1) for t in (0, 1) for c in (0, 1)}
CASES["linear_default"] = dict(layer_idx=1, reverse=True, transpose=True)       # create_block's own defaults: LayerNorm, unfused, Mamba
CASES.update({f"window_t{t}": dict(PUBLISHED, block_type="window", reverse=bool(t), transpose=False, scanning_continuity=False) for t in (0, 1)})
SHAPE = (2, 256, 128)


def check_block(tag, dev, tol, gtol, sum_tol):
    """forward, residual output, dx / dres / dc and every parameter gradient of fixture `tag` (big matrices: the stored rows [::16])"""
    from dimsum_amd.models_dim import DiMBlock, DiMBlockWindow, create_block
    g, common = golden("block_" + tag), golden("block_linear_window")
    blk = create_block(128, **CASES[tag])
    assert type(blk) is (DiMBlockWindow if tag.startswith("window") else DiMBlock)
    assert sorted(blk.state_dict().keys()) == [str(k) for k in g["keys"]]
    procedural_fill(blk, seed=9)
    blk = blk.to(dev)
    x, res, cc = (T(seeded(sh, sd)).to(dev).requires_grad_() for sh, sd in ((SHAPE, 101), (SHAPE, 102), ((2, 128), 103)))
    y, ro = blk(x, res, cc)
    ((y * T(seeded(SHAPE, 104)).to(dev)).sum() + (ro * T(seeded(SHAPE, 105)).to(dev)).sum()).backward()
    n = lambda t: t.detach().cpu().numpy()
    assert_close(n(y), g["y"], what="y", **tol)
    assert np.array_equal(n(ro), common["res_out"])
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
            assert k.startswith("mixer.cond_proj") and (v.grad is None or not v.grad.any()), k      # SURVEY finding 1: dead parameter
            continue
        checked += 1
    assert checked == len([f for f in g.files if f.startswith(("g_", "g16_"))]) >= 17


@pytest.mark.parametrize("tag", list(CASES))
def test_block_forward_and_all_gradients(tag):
    with cpu_oracle_backend():
        check_block(tag, "cpu", TOL, TOL, SUM_TOL)


@pytest.mark.parametrize("block_type", ["linear", "window", "some_unlisted_name"])
def test_dim_with_default_arguments_constructs(block_type):
    """DiM()'s own default is block_type="linear"; every unlisted value falls through to DiMBlock (dimsum/models_dim.py:2129-2141).
    Depth and the per-layer flag rule are the reference's (:1594, :1686-1688, :2080-2081)."""
    from dimsum_amd.models_dim import DiM, DiMBlock, DiMBlockWindow
    with torch.device("meta"):
        m = DiM() if block_type == "linear" else DiM(block_type=block_type)
    assert m.block_type == block_type and m.depth == len(m.blocks) == 16 and m.use_attn_every_k_layers == -1
    assert not hasattr(m, "attn_block")
    for i, b in enumerate(m.blocks):
        if block_type == "window":
            assert type(b) is DiMBlockWindow
            assert (b.reverse, b.transpose, b.shift_window) == (False, i % 2 > 0, False)
        else:
            assert type(b) is DiMBlock
            assert (b.reverse, b.transpose) == (i % 2 > 0, i % 4 >= 2)


def test_create_block_window_and_the_one_refused_type():
    from dimsum_amd.models_dim import DiMBlockWindow, create_block
    blk = create_block(32, layer_idx=0, block_type="window", reverse=True, transpose=True)
    assert type(blk) is DiMBlockWindow and (blk.reverse, blk.transpose, blk.shift_window, blk.layer_idx) == (False, True, False, 0)
    with pytest.raises(NotImplementedError, match="combined_einfft"):
        create_block(32, layer_idx=0, block_type="combined_einfft")


def _blocks_for_tables(H):
    """(fixture key, block) over every flag combination of both blocks"""
    from dimsum_amd.models_dim import DiMBlock, DiMBlockWindow
    mixer = lambda dim: torch.nn.Identity()
    for r in (0, 1):
        for t in (0, 1):
            for k in (0, 1):
                yield f"linear_H{H}_r{r}_t{t}_c{k}", DiMBlock(8, mixer, reverse=bool(r), transpose=bool(t), scanning_continuity=bool(k))
                yield f"window_H{H}_t{t}_r{r}_s{k}", DiMBlockWindow(8, mixer, reverse=bool(r), transpose=bool(t), shift_window=bool(k))


@pytest.mark.parametrize("H", [4, 16])
def test_composed_tables_are_the_reference_orders(H):
    """the block's ONE gather table vs the reference's rearrange / flip / local_scan / roll chain applied to arange(L), bit for bit; the
    inverse table after the forward table is the identity"""
    common = golden("block_linear_window")
    L = H * H
    ident = torch.arange(L)
    for key, blk in _blocks_for_tables(H):
        tab = blk._table(L, "cpu", blk._order)
        want = common[key].astype(np.int64)
        if tab is None:
            assert np.array_equal(want, np.arange(L)), key
            continue
        assert tab["fwd"].dtype == torch.int64 and tab["inv32"].dtype == torch.int32
        assert np.array_equal(tab["fwd"].numpy(), want), key
        assert torch.equal(tab["fwd"][tab["inv"]], ident) and torch.equal(tab["inv"][tab["fwd"]], ident), key
        assert torch.equal(tab["inv32"].long(), tab["inv"]), key


def test_window_block_refuses_a_grid_the_windows_do_not_tile():
    from dimsum_amd.models_dim import DiMBlockWindow
    blk = DiMBlockWindow(8, lambda dim: torch.nn.Identity())
    with pytest.raises(NotImplementedError, match="zero-pads"):
        blk._table(36, "cpu", blk._order)


@pytest.mark.parametrize("block_type", ["linear", "window"])
def test_tiny_models(block_type):
    from dimsum_amd.models_dim import DiM
    g = golden("model_tiny_" + block_type)
    m = DiM(depth=4, hidden_size=64, patch_size=2, **_published(block_type=block_type)).eval()
    assert sorted(m.state_dict().keys()) == [str(k) for k in g["keys"]] and len(g["keys"]) == int(g["n_keys"])
    procedural_fill(m, seed=3)
    x = T(g["x"]).clone().requires_grad_()
    with cpu_oracle_backend():
        out = m(x, T(g["t"]), T(g["y"]))
        out.backward(T(g["dout"]))
    assert_close(out.detach().numpy(), g["out"], what="out", **TOL)
    assert_close(x.grad.numpy(), g["dx"], what="dx", **TOL)
