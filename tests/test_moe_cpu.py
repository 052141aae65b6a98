"""The mixture-of-experts layers (dimsum_amd/switch_mlp.py, mlp.MLP, models_dim.MoEBlock, DiM(is_moe=True)), host side.

tests/golden/moe_switch.npz (routing_mode "top1"), moe_switch_sinkhorn.npz (routing_mode "sinkhorn") and moe_keys.json were written by
`tools/gen_golden.py --only moe` from the IMPORTED reference modules (dimsum/switch_mlp.py, mlp.py, models_dim.MoEBlock) on the CPU: outputs,
chosen experts and all gradients at dim 32, tokens (2, 24), 4 experts; the weights are procedural_fill(module, seed) on both sides.

The forwards run on the CPU with torch stand-ins of the native.moe_* entries defined here (`moe_standins`): checkers, not product paths --
without them SwitchMLP refuses CPU tensors, which is a test of its own."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, golden
from procedural import procedural_fill, seeded

T = torch.from_numpy
FILES = {"top1": "moe_switch", "sinkhorn": "moe_switch_sinkhorn"}
CASES = [(mode, gated, bias) for mode in ("top1", "sinkhorn") for gated in (True, False) for bias in (True, False)]
DIM, E = 32, 4


def tag_of(gated, bias):
    return f"{'gated' if gated else 'plain'}_{'bias' if bias else 'nobias'}"


# ---- torch stand-ins of the native entries (any device, the dtype of their inputs) -------------------------------------------------------------------
def _route(logits, mode):
    return torch.sigmoid(logits) if mode == "sigmoid" else torch.softmax(logits, dim=1)


def moe_route_fwd(x, w, b, mode):
    logits = x @ w.t() if b is None else x @ w.t() + b
    prob, e = torch.max(_route(logits, mode), dim=1)
    perm = torch.argsort(e, stable=True)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(perm.numel(), device=perm.device)
    offsets = torch.cat([e.new_zeros(1), torch.cumsum(torch.bincount(e, minlength=w.shape[0]), 0)])
    return prob, e.int(), logits, offsets.int(), perm.int(), inv.int(), e[perm].int()


def moe_route_bwd(x, w, logits, prob, expert, inv, dprob, dxp, mode):
    hot = F.one_hot(expert.long(), w.shape[0]).to(x.dtype)
    if mode == "sigmoid":
        dl = hot * (dprob * prob * (1 - prob)).unsqueeze(1)
    else:
        dl = (dprob * prob).unsqueeze(1) * (hot - torch.softmax(logits, dim=1))
    return dxp[inv.long()] + dl @ w, dl.t() @ x, dl.sum(0)


def moe_permute(x, perm):
    return x[perm.long()]


def moe_combine_fwd(y, perm, prob):
    out = torch.empty_like(y)
    out[perm.long()] = prob[perm.long()].unsqueeze(1) * y
    return out


def moe_combine_bwd(dout, y, perm, prob):
    p = perm.long()
    d = dout[p]
    dprob = torch.empty_like(prob)
    dprob[p] = (d * y).sum(1)
    return prob[p].unsqueeze(1) * d, dprob


def _act(x, bias, row_expert, gated):
    if bias is not None:
        x = x + (bias[row_expert.long()] if row_expert is not None else bias[0])
    if gated:
        a, g = x.chunk(2, dim=-1)
        return F.gelu(a) * g
    return F.gelu(x)


def moe_act_fwd(x, bias=None, row_expert=None, gated=True):
    return _act(x, bias, row_expert, gated)


def moe_act_bwd(x, bias, row_expert, dh, gated=True, need_dbias=True):
    xr = x.detach().clone().requires_grad_()
    br = None if bias is None else bias.detach().clone().requires_grad_()
    with torch.enable_grad():
        _act(xr, br, row_expert, gated).backward(dh)
    return xr.grad, (br.grad if (br is not None and need_dbias) else None)


STANDINS = dict(moe_route_fwd=moe_route_fwd, moe_route_bwd=moe_route_bwd, moe_permute=moe_permute, moe_combine_fwd=moe_combine_fwd,
                moe_combine_bwd=moe_combine_bwd, moe_act_fwd=moe_act_fwd, moe_act_bwd=moe_act_bwd)


@pytest.fixture
def moe_standins(monkeypatch):
    from dimsum_amd import native
    for k, f in STANDINS.items():
        monkeypatch.setattr(native, k, f)


@pytest.fixture
def cpu_backend(moe_standins, monkeypatch):
    from oracle.torch_backend import cpu_oracle_backend
    monkeypatch.setenv("DIMSUM_ALLOW_TORCH_SDPA", "1")
    with cpu_oracle_backend():
        yield


def make_switch(mode, gated, bias, seed, dim=DIM, experts=E):
    from dimsum_amd.switch_mlp import SwitchMLP
    return procedural_fill(SwitchMLP(dim, layer_idx=1, num_moe_experts=experts, add_bias_linear=bias, gated_linear_unit=gated, routing_mode=mode), seed=seed)


def switch_args(m, dtype=torch.float64, device="cpu"):
    """the module's parameters as the leaf tensors switch_mlp_torch takes: (router w, router b, fc1 ws, fc2 ws, fc1 bs, fc2 bs)"""
    leaf = lambda p: None if p is None else p.detach().to(device=device, dtype=dtype).requires_grad_()     # noqa: E731
    ex = m.local_experts
    biased = ex[0].linear_fc1.bias is not None
    return (leaf(m.router.weight), leaf(m.router.bias), [leaf(e.linear_fc1.weight) for e in ex], [leaf(e.linear_fc2.weight) for e in ex],
            [leaf(e.linear_fc1.bias) for e in ex] if biased else None, [leaf(e.linear_fc2.bias) for e in ex] if biased else None)


def named_grads(m, args):
    """{parameter name: gradient} of switch_args' leaves under the module's parameter names"""
    rw, rb, w1, w2, b1, b2 = args
    out = {"router.weight": rw.grad, "router.bias": rb.grad}
    for i in range(len(w1)):
        out[f"local_experts.{i}.linear_fc1.weight"], out[f"local_experts.{i}.linear_fc2.weight"] = w1[i].grad, w2[i].grad
        if b1 is not None:
            out[f"local_experts.{i}.linear_fc1.bias"], out[f"local_experts.{i}.linear_fc2.bias"] = b1[i].grad, b2[i].grad
    return {k: (torch.zeros(tuple(dict(m.named_parameters())[k].shape), dtype=torch.float64) if v is None else v) for k, v in out.items()}


def close(got, want, what):
    """rtol 1e-5, atol 1e-6 max|ref|: the bound of test_dit_cpu for fp32 CPU forwards"""
    want = torch.as_tensor(want)
    torch.testing.assert_close(got.detach().to(want.dtype).cpu(), want, rtol=1e-5, atol=1e-6 * max(want.abs().max().item(), 1e-30), msg=lambda m: f"{what}: {m}")


def test_state_dict_keys_equal_the_references():
    from functools import partial
    from dimsum_amd.models_dim import MoEBlock
    from dimsum_amd.switch_mlp import SwitchMLP
    with open(os.path.join(GOLDEN, "moe_keys.json")) as f:
        want = [(k, tuple(s)) for k, s in json.load(f)]
    blk = MoEBlock(DIM, mixer_cls=partial(SwitchMLP, layer_idx=1, num_moe_experts=E), norm_cls=torch.nn.LayerNorm)
    assert [(k, tuple(v.shape)) for k, v in blk.state_dict().items()] == want


@pytest.mark.parametrize("mode,gated,bias", CASES)
def test_restatement_reproduces_the_reference(mode, gated, bias):
    from dimsum_amd.ops import switch_mlp_torch
    g, tag = golden(FILES[mode]), tag_of(gated, bias)
    m = make_switch(mode, gated, bias, int(g[tag + ".seed"]))
    args = switch_args(m)
    x = T(g["x"]).double().requires_grad_()
    out, e = switch_mlp_torch(x, *args, routing_mode=mode, gated=gated)
    assert torch.equal(e, T(g[tag + ".expert"]))
    out.backward(T(g["dout"]).double())
    close(out, g[tag + ".out"], "out")
    close(x.grad, g[tag + ".dx"], "dx")
    for k, v in named_grads(m, args).items():
        close(v, g[f"{tag}.grad.{k}"], k)


@pytest.mark.parametrize("mode,gated,bias", CASES)
def test_module_reproduces_the_reference(mode, gated, bias, moe_standins):
    g, tag = golden(FILES[mode]), tag_of(gated, bias)
    m = make_switch(mode, gated, bias, int(g[tag + ".seed"]))
    x = T(g["x"]).requires_grad_()
    out = m(x)
    out.backward(T(g["dout"]))
    close(out, g[tag + ".out"], "out")
    close(x.grad, g[tag + ".dx"], "dx")
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        close(p.grad, g[f"{tag}.grad.{k}"], k)
    from dimsum_amd import native
    assert torch.equal(native.moe_route_fwd(x.detach().reshape(-1, DIM), m.router.weight.detach(), m.router.bias.detach(),
                                            "sigmoid" if mode == "sinkhorn" else "softmax")[1].long(), T(g[tag + ".expert"]))


def test_mlp_and_block_reproduce_the_reference(moe_standins):
    from functools import partial
    from dimsum_amd.mlp import MLP
    from dimsum_amd.models_dim import MoEBlock
    from dimsum_amd.switch_mlp import SwitchMLP
    g = golden("moe_switch")
    x, r = T(g["x"]), T(g["dout"])
    mlp = procedural_fill(MLP(DIM, add_bias_linear=True, gated_linear_unit=True), seed=50)
    close(mlp(x), g["mlp.out"], "mlp")
    blk = procedural_fill(MoEBlock(DIM, mixer_cls=partial(SwitchMLP, layer_idx=1, num_moe_experts=E), norm_cls=torch.nn.LayerNorm), seed=51)
    h, res = blk(x, r)
    close(h, g["block.out"], "block out")
    close(res, g["block.residual"], "block residual")


def test_sinkhorn_reproduces_its_fixture():
    from dimsum_amd.switch_mlp import sinkhorn
    g = golden("moe_switch")
    close(sinkhorn(T(g["sinkhorn.cost"])), g["sinkhorn.out"], "sinkhorn")


def test_create_block_builds_a_moe_block_on_odd_layers():
    from dimsum_amd.models_dim import MoEBlock, create_block
    from dimsum_amd.switch_mlp import SwitchMLP
    odd = create_block(32, layer_idx=1, is_moe=True, num_moe_experts=3)
    assert isinstance(odd, MoEBlock) and isinstance(odd.mixer, SwitchMLP) and odd.mixer.num_moe_experts == 3 and odd.layer_idx == 1
    assert not hasattr(odd, "adaLN_modulation") and not hasattr(odd, "drop_path")
    assert not isinstance(create_block(32, layer_idx=0, is_moe=True), MoEBlock)
    assert not isinstance(create_block(32, layer_idx=1, is_moe=False), MoEBlock)


def test_mamba_moe_layers_pick_the_expert_count_per_layer():
    from dimsum_amd.models_dim import create_block
    from dimsum_amd.switch_mlp import SwitchMLP
    layers = ["a2", "b3", "c5", "d7"]
    assert [SwitchMLP(8, layer_idx=i, mamba_moe_layers=layers, num_moe_experts=8).num_moe_experts for i in (1, 2, 3, 4)] == [2, 3, 5, 7]
    assert SwitchMLP(8, layer_idx=0, mamba_moe_layers=layers).num_moe_experts == 7                 # (entry layer_idx - 1 = -1, as in the reference)
    assert create_block(32, layer_idx=3, is_moe=True, mamba_moe_layers=layers).mixer.num_moe_experts == 5
    assert len(create_block(32, layer_idx=3, is_moe=True, mamba_moe_layers=layers).mixer.local_experts) == 5


def _tiny(**over):
    from dimsum_amd.models_dim import DiM
    kw = dict(img_resolution=8, num_classes=10, is_moe=True, num_moe_experts=4)       # (the constructor's defaults otherwise: block_type "linear")
    kw.update(over)
    return DiM(depth=4, hidden_size=64, patch_size=2, **kw)


def tiny_inputs(n=2):
    return T(seeded((n, 4, 8, 8), 21)), T(seeded((n,), 22, kind="uniform")), torch.tensor([1, 3, 5, 7][:n])


def test_dim_is_moe_constructs_and_a_fresh_model_outputs_zero(cpu_backend):
    from dimsum_amd.models_dim import MoEBlock
    m = _tiny().eval()
    assert [isinstance(b, MoEBlock) for b in m.blocks] == [False, True, False, True]
    assert torch.count_nonzero(m.blocks[1].mixer.local_experts[0].linear_fc2.weight) > 0
    x, t, y = tiny_inputs()
    with torch.no_grad():
        out = m(x, t, y)
    assert out.shape == (2, 4, 8, 8) and torch.count_nonzero(out) == 0


def test_dim_is_moe_every_parameter_gets_a_gradient(cpu_backend):
    m = procedural_fill(_tiny(), seed=5).eval()
    with torch.no_grad():
        m.blocks[1].mixer.router.bias[2] = -1e4          # expert 2 of layer 1 receives no token
    x, t, y = tiny_inputs()
    out = m(x, t, y)
    assert out.abs().max() > 0
    out.square().sum().backward()
    missing = [k for k, p in m.named_parameters() if p.requires_grad and p.grad is None]
    assert not missing, missing
    idle = m.blocks[1].mixer.local_experts[2]
    assert all(torch.count_nonzero(p.grad) == 0 for p in idle.parameters())
    assert all(torch.count_nonzero(p.grad) > 0 for p in m.blocks[1].mixer.local_experts[0].parameters())
    assert torch.count_nonzero(m.blocks[1].mixer.router.weight.grad) > 0


def test_switch_mlp_on_cpu_tensors_is_refused():
    from dimsum_amd.mlp import MLP
    m = make_switch("top1", True, False, 1)
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        m(torch.zeros(2, 4, DIM))
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        MLP(16)(torch.zeros(4, 16))
    with pytest.raises(RuntimeError, match="float32"):
        m(torch.zeros(2, 4, DIM, dtype=torch.float64))


def test_hip_graph_refuses_a_model_with_a_moe_block():
    from dimsum_amd.hip_graph import GraphedForward
    m = _tiny()
    with pytest.raises(NotImplementedError, match="MoEBlock"):
        GraphedForward(m.forward)
    with pytest.raises(NotImplementedError, match="MoEBlock"):
        GraphedForward(m)


def test_moe_entries_are_declared_exported_and_versioned():
    from dimsum_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "dimsum_hip.h")).read()
    entries = {"dimsum_moe_route_fwd": _lib.MoeRouteParams, "dimsum_moe_route_bwd": _lib.MoeRouteParams, "dimsum_moe_permute": _lib.MoeRowsParams,
               "dimsum_moe_combine_fwd": _lib.MoeRowsParams, "dimsum_moe_combine_bwd": _lib.MoeRowsParams, "dimsum_moe_act_fwd": _lib.MoeActParams,
               "dimsum_moe_act_bwd": _lib.MoeActParams}
    for name, ptype in entries.items():
        assert name in _lib.EXPORTS and hasattr(lib, name) and f"int {name}(" in header, name
        P = ptype()
        for f, v in (("tokens", 1), ("rows", 1), ("hidden", 4), ("width", 4), ("num_experts", 1)):
            if hasattr(P, f):
                setattr(P, f, v)
        assert getattr(lib, name)(ctypes.byref(P), None) == 1, name          # the right size, one row, no pointers: DIMSUM_ERR_NULL
        P.struct_size -= 8                                                   # a stale struct size is refused before anything is read
        assert getattr(lib, name)(ctypes.byref(P), None) == 7, name
    assert "dimsum_moe_route_work_bytes" in _lib.EXPORTS and "int64_t dimsum_moe_route_work_bytes(" in header
    assert lib.dimsum_moe_route_work_bytes(65, 8) == 2 * 8 * 4 and lib.dimsum_moe_route_work_bytes(64, 3) == 3 * 4


def test_shapes_outside_the_kernels_are_error_codes():
    from dimsum_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.addressof(buf)
    P = _lib.MoeActParams()
    P.x_ptr = P.out_ptr = ptr
    P.rows, P.width, P.num_experts = 1, 6, 1                                  # width % 4 != 0
    assert lib.dimsum_moe_act_fwd(ctypes.byref(P), None) == 3
    P.width, P.num_experts = 8, 65
    assert lib.dimsum_moe_act_fwd(ctypes.byref(P), None) == 3
    R = _lib.MoeRouteParams()
    for f in ("x_ptr", "w_ptr", "prob_ptr", "expert_ptr", "logits_ptr", "inv_ptr", "offsets_ptr", "perm_ptr", "row_expert_ptr", "work_ptr"):
        setattr(R, f, ptr)
    R.tokens, R.hidden, R.num_experts, R.work_bytes = 4, 8, 65, 1 << 20
    assert lib.dimsum_moe_route_fwd(ctypes.byref(R), None) == 3
    R.num_experts, R.mode = 4, 2
    assert lib.dimsum_moe_route_fwd(ctypes.byref(R), None) == 5
    R.mode, R.work_bytes = 0, 0                                               # a workspace that is too small
    assert lib.dimsum_moe_route_fwd(ctypes.byref(R), None) == 3


@pytest.mark.parametrize("driver", ["train", "sample_ddp"])
def test_the_drivers_take_the_moe_flags(driver):
    import importlib
    mod = importlib.import_module("dimsum_amd." + driver)
    ap = mod.build_parser()
    dests = {a.dest: a for a in ap._actions}
    assert {"is_moe", "num_moe_experts", "mamba_moe_layers"} <= set(dests)
    assert dests["is_moe"].default is False and dests["num_moe_experts"].default == 8 and dests["mamba_moe_layers"].default is None
    assert dests["mamba_moe_layers"].nargs == "*" and dests["num_moe_experts"].type is int


def test_create_model_forwards_the_moe_flags():
    from dimsum_amd.create_model import create_model, published_config
    from dimsum_amd.models_dim import MoEBlock
    with torch.device("meta"):
        m = create_model(published_config("DiM-S/2", is_moe=True, num_moe_experts=8, mamba_moe_layers=[f"l{2 + i % 3}" for i in range(64)]))
    moe = [b for b in m.blocks if isinstance(b, MoEBlock)]
    assert len(moe) == len(m.blocks) // 2 and all(b.mixer.num_moe_experts == 2 + (b.layer_idx - 1) % 3 for b in moe)
