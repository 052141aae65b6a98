"""The DiT baseline family (dimsum_amd/models_dit.py) and the plain Mlp (dimsum_amd/mlp.py), host side.

tests/golden/dit_keys.json -- [[state_dict key, shape], ...] of the reference's DiT-S/2 in state_dict order -- was written by
`tools/gen_golden.py --only dit_keys` from the IMPORTED reference module (dimsum/models_dit.py); timm is not installed where the fixture was
made, so its three classes were the stand-ins of tools/ref_shim.py, which carry timm 0.9.12's parameter names (PatchEmbed.proj,
Attention.qkv / proj, Mlp.fc1 / fc2).

The forwards run on the CPU through the suite's CPU oracle backend (oracle/torch_backend.py) plus, for the one native entry it does not know,
a torch stand-in of native.gelu_fwd / gelu_bwd defined here: a checker, not a product path -- without it the Mlp refuses CPU tensors, which
is a test of its own."""
import json
import os
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN
from procedural import procedural_fill, seeded

T = torch.from_numpy
NAMES = [f"DiT-{s}/{p}" for s in ("S", "B", "L", "XL") for p in (2, 4, 8)]
SIZES = {"S": (12, 384, 6), "B": (12, 768, 12), "L": (24, 1024, 16), "XL": (28, 1152, 16)}       # depth, hidden, heads (models_dit.py:354-399)


def _cfg(name, **over):
    from dimsum_amd.create_model import published_config
    return published_config(name, **over)


@pytest.fixture
def cpu_backend(monkeypatch):
    from dimsum_amd import native
    from oracle.torch_backend import cpu_oracle_backend

    def gelu_fwd(x, bias=None, split3=False, scales=None):
        assert split3 is False
        return F.gelu(x if bias is None else x + bias, approximate="tanh")

    def gelu_bwd(x, bias, dh, need_dbias=True, split3=False):
        xr = (x.detach() if bias is None else x.detach() + bias.detach()).clone().requires_grad_()
        with torch.enable_grad():
            F.gelu(xr, approximate="tanh").backward(dh)
        return xr.grad, (xr.grad.reshape(-1, x.shape[-1]).sum(0) if bias is not None and need_dbias else None)

    monkeypatch.setattr(native, "gelu_fwd", gelu_fwd)
    monkeypatch.setattr(native, "gelu_bwd", gelu_bwd)
    monkeypatch.setenv("DIMSUM_ALLOW_TORCH_SDPA", "1")
    with cpu_oracle_backend():
        yield


@pytest.mark.parametrize("name", NAMES)
def test_create_model_builds_every_zoo_entry(name):
    """on the meta device (no storage): depth, width, heads, patch and the MLP class of each of the reference's twelve entries"""
    from dimsum_amd.create_model import create_model
    from dimsum_amd.mlp import Mlp
    from dimsum_amd.models_dit import DiT, DiT_models
    assert list(DiT_models) == [f"DiT-{s}/{p}" for s in ("XL", "L", "B", "S") for p in (2, 4, 8)]       # the reference's order
    with torch.device("meta"):
        m = create_model(_cfg(name, learn_sigma=True))
    size, patch = name[4:].split("/")
    depth, hidden, heads = SIZES[size]
    assert isinstance(m, DiT) and len(m.blocks) == depth and m.pos_embed.shape == (1, (32 // int(patch)) ** 2, hidden)
    assert m.num_heads == heads and m.blocks[0].attn.num_heads == heads and m.patch_size == int(patch) and m.out_channels == 8
    assert all(isinstance(b.mlp, Mlp) and b.mlp._fused and b.mlp.fc1.weight.shape == (4 * hidden, hidden) for b in m.blocks)
    assert not m.pos_embed.requires_grad and m.y_embedder.embedding_table.weight.shape[0] == 1001


def test_names_in_neither_zoo_are_refused():
    from dimsum_amd.create_model import create_model
    for name in ("DiT-H/2", "UViT-L/2", "DiT-L/3"):
        with pytest.raises(NotImplementedError):
            create_model(_cfg(name))


def test_state_dict_keys_equal_the_references():
    from dimsum_amd.models_dit import DiT_models
    with open(os.path.join(GOLDEN, "dit_keys.json")) as f:
        want = [(k, tuple(s)) for k, s in json.load(f)]
    with torch.device("meta"):
        m = DiT_models["DiT-S/2"]()
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == want


def test_use_gated_mlp_false_keeps_the_fc_keys():
    """the flag's Mlp inside DiM (shared attention block and the combined blocks' tail): parameter names unchanged"""
    from dimsum_amd.models_dim import DiTBlock, _make_mlp
    assert sorted(_make_mlp(64, use_gated_mlp=False).state_dict()) == ["fc1.bias", "fc1.weight", "fc2.bias", "fc2.weight"]
    assert {k for k in DiTBlock(64, 2, use_gated_mlp=False).state_dict() if k.startswith("mlp.")} == {"mlp.fc1.bias", "mlp.fc1.weight", "mlp.fc2.bias", "mlp.fc2.weight"}


def _tiny(**kw):
    from dimsum_amd.models_dit import DiT
    return DiT(input_size=8, patch_size=2, hidden_size=64, depth=2, num_heads=2, num_classes=10, **kw).eval()


def _inputs(n=4):
    return T(seeded((n, 4, 8, 8), 11)), T(seeded((n,), 12, kind="uniform")), torch.tensor([1, 3, 5, 7][:n])


def test_fresh_model_outputs_exactly_zero(cpu_backend):
    """adaLN-zero (models_dit.py:219-228): zero gates, zero final modulation and a zero final Linear"""
    m = _tiny(learn_sigma=True)
    assert all(torch.count_nonzero(b.adaLN_modulation[-1].weight) == 0 for b in m.blocks)
    assert torch.count_nonzero(m.blocks[0].mlp.fc1.weight) > 0 and torch.count_nonzero(m.blocks[0].mlp.fc1.bias) == 0
    x, t, y = _inputs()
    with torch.no_grad():
        out = m(x, t, y)
    assert out.shape == (4, 8, 8, 8) and torch.count_nonzero(out) == 0


def test_forward_with_cfg_is_the_hand_combination(cpu_backend):
    m = procedural_fill(_tiny(learn_sigma=True), seed=4)
    x, t, _ = _inputs()
    half = x[:2]
    xx, tt = torch.cat([half, half]), torch.cat([t[:2], t[:2]])
    y = torch.tensor([1, 3, 10, 10])                    # [cond | null class]
    with torch.no_grad():
        got = m.forward_with_cfg(xx, tt, y, cfg_scale=2.5)
        cond, unc = m(half, t[:2], y[:2]), m(half, t[:2], y[2:])
    assert got.abs().max() > 0
    eps = unc[:, :4] + 2.5 * (cond[:, :4] - unc[:, :4])
    want = torch.cat([torch.cat([eps, eps]), torch.cat([cond[:, 4:], unc[:, 4:]])], dim=1)
    # the batch of 4 and the two batches of 2 take different blockings in the CPU matmuls: fp32 forwards that agree to ~1e-6 of max|out|,
    # and the guidance combination weighs them by 1 + 2 * 2.5 = 6
    tol = dict(rtol=1e-5, atol=1e-5 * want.abs().max().item())
    torch.testing.assert_close(got, want, **tol)
    with torch.no_grad():                                # y = None is the null class
        torch.testing.assert_close(m(half, t[:2]), unc, **tol)


def test_mlp_on_cpu_tensors_is_refused():
    from dimsum_amd.mlp import Mlp, bias_gelu
    mlp = Mlp(16, 64, act_layer=lambda: torch.nn.GELU(approximate="tanh"))
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        mlp(torch.zeros(2, 4, 16))
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        bias_gelu(torch.zeros(4, 16))


def test_cli_model_construction_ignores_dim_flags_with_one_line():
    from dimsum_amd.create_model import model_from_cli
    from dimsum_amd.models_dim import DiM
    from dimsum_amd.models_dit import DiT
    lines = []
    args = SimpleNamespace(model="DiT-S/8", image_size=64, num_classes=10, pe_type="rope", block_type="window")
    with torch.device("meta"):
        m = model_from_cli(args, log=lines.append)
        assert isinstance(m, DiT) and len(lines) == 1 and "--block-type" in lines[0] and "--pe-type" in lines[0]
        args.model = "DiM-S/2"
        assert isinstance(model_from_cli(args, log=lines.append), DiM) and len(lines) == 1


def test_gelu_entries_are_declared_and_exported():
    from dimsum_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "dimsum_hip.h")).read()
    for name in ("dimsum_gelu_fwd", "dimsum_gelu_bwd"):
        assert name in _lib.EXPORTS and hasattr(lib, name) and f"int {name}(" in header, name
    assert _lib.GEMM_EPI_GELU_F16 == 7 and "DIMSUM_GEMM_EPI_GELU_F16 = 7" in header
    import ctypes
    P = _lib.GeluParams()                                # a stale struct size is refused before anything is read
    P.struct_size -= 8
    assert lib.dimsum_gelu_fwd(ctypes.byref(P), None) == 7 and lib.dimsum_gelu_bwd(ctypes.byref(P), None) == 7
