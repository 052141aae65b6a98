"""Training on the grouped expert GEMM (csrc/moe_gemm_bwd.hip, native.moe_gemm_dgrad / moe_gemm_wgrad, ops.moe._SwitchMlpGroupedFn), host side: the two
entry points' declarations, struct layouts and refusals (no GPU is touched: every check runs before the launch), the opt-in rules of `grouped_train`
(off by default, DIMSUM_MOE_GROUPED_TRAIN=1, both setters, independent of `grouped`), and the layer's forward + backward on torch stand-ins with every
synchronising tensor method patched to raise."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from test_host_logic import _header_layout
from test_moe_cpu import DIM, E, STANDINS, _tiny, close, make_switch, named_grads, switch_args
from test_moe_grouped_cpu import _header, moe_gemm, no_host_reads

OK, ERR_NULL, ERR_SHAPE, ERR_ABI = 0, 1, 3, 7
ENTRIES = {"dimsum_moe_gemm_dgrad": ("dimsum_moe_gemm_dgrad_params_t", "MoeGemmDgradParams"),
           "dimsum_moe_gemm_wgrad": ("dimsum_moe_gemm_wgrad_params_t", "MoeGemmWgradParams")}


# ---- torch stand-ins of the two gradients that, like the kernels, never bring the offsets to the host ----------------------------------------------
def _row_expert(rows, offsets, experts, device):
    return torch.bucketize(torch.arange(rows, device=device), offsets[1:].long(), right=True).clamp_(max=experts - 1)


def moe_gemm_dgrad(dy, offsets, weights, out=None):
    e = _row_expert(dy.shape[0], offsets, len(weights), dy.device)
    dx = torch.bmm(dy.unsqueeze(1), torch.stack(list(weights))[e]).squeeze(1)
    if out is None:
        return dx
    out.copy_(dx)
    return out


def moe_gemm_wgrad(dy, x, offsets, num_experts, need_dbias=False):
    hot = F.one_hot(_row_expert(dy.shape[0], offsets, num_experts, dy.device), num_experts).to(dy.dtype)
    dw = torch.einsum("te,tn,tk->enk", hot, dy, x)
    return list(dw.unbind(0)), (hot.t() @ dy if need_dbias else None)


@pytest.fixture
def train_standins(monkeypatch):
    from dimsum_amd import native
    for k, f in dict(STANDINS, moe_gemm=moe_gemm, moe_gemm_dgrad=moe_gemm_dgrad, moe_gemm_wgrad=moe_gemm_wgrad).items():
        monkeypatch.setattr(native, k, f)


@pytest.fixture
def calls(monkeypatch):
    """the names of the paths switch_mlp_fn takes, in order"""
    from dimsum_amd.ops import moe
    seen = []
    for name, attr, static in (("grouped", "switch_mlp_grouped_fwd", False), ("autograd", "_SwitchMlpFn", True), ("grouped_train", "_SwitchMlpGroupedFn", True)):
        if static:
            real = getattr(moe, attr).apply
            monkeypatch.setattr(getattr(moe, attr), "apply", staticmethod(lambda *a, _n=name, _r=real: (seen.append(_n), _r(*a))[1]))
        else:
            real = getattr(moe, attr)
            monkeypatch.setattr(moe, attr, lambda *a, _n=name, _r=real, **k: (seen.append(_n), _r(*a, **k))[1])
    return seen


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------------------
def test_both_entries_are_declared_exported_and_resolve_and_the_abi_is_still_18():
    from dimsum_amd import _lib
    lib, header = _lib.load(), _header()
    for name, (cname, _) in ENTRIES.items():
        assert f"int {name}(const {cname} *p, void *stream);" in header
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.dimsum_abi_version() == 18 and "#define DIMSUM_ABI_VERSION 18" in header
    assert len(_lib.MoeGemmParams._fields_) == 12                  # (the forward's struct is what it was)


def test_the_ctypes_structs_have_the_headers_layout():
    from dimsum_amd import _lib
    pairs = [(cname, getattr(_lib, mirror)) for cname, mirror in ENTRIES.values()]
    layout = _header_layout(pairs)
    for cname, mirror in pairs:
        size, offsets = layout[cname]
        assert ctypes.sizeof(mirror) == size and mirror().struct_size == size, cname
        assert {f: getattr(mirror, f).offset for f, _ in mirror._fields_} == offsets, cname
        names = [f for f, _ in mirror._fields_]
        assert names[0] == "struct_size" and offsets["struct_size"] == 0 and names[-1] == "ext" and offsets["ext"] == size - 8, cname


def _params(entry, tokens=4, k=32, n=32, experts=2, pointers=True):
    from dimsum_amd import _lib
    P = getattr(_lib, ENTRIES[entry][1])()
    P.tokens, P.k, P.n, P.num_experts = tokens, k, n, experts
    keep = []
    if pointers:                                   # host memory, never dereferenced: every refusal below comes before the launch
        buf = (ctypes.c_float * 64)()
        base = (ctypes.addressof(buf) + 15) // 16 * 16
        table = (_lib.vp * 64)(*([base] * 64))
        P.dy_ptr = P.offsets_ptr = base
        if entry.endswith("dgrad"):
            P.ldc, P.w_ptrs, P.dx_ptr = k, table, base
        else:
            P.x_ptr, P.dw_ptrs, P.db_ptr = base, table, base
        keep = [buf, table]
    return P, keep


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_shapes_outside_the_kernels_are_error_codes(entry):
    from dimsum_amd import _lib
    call = getattr(_lib.load(), entry)
    assert call(None, None) == ERR_NULL
    P, keep = _params(entry, pointers=False)
    P.struct_size -= 8                                             # a stale struct size is refused before any pointer is read (there is none to read)
    assert call(ctypes.byref(P), None) == ERR_ABI
    P, keep = _params(entry, k=48)
    P.struct_size += 8                                             # ... and before the shapes are
    assert call(ctypes.byref(P), None) == ERR_ABI
    for kw in (dict(k=48), dict(k=8), dict(k=0), dict(n=48), dict(n=8), dict(n=0), dict(experts=0), dict(experts=65), dict(tokens=-1)):
        P, keep = _params(entry, **kw)
        assert call(ctypes.byref(P), None) == ERR_SHAPE, kw
    P, keep = _params(entry, pointers=False)                       # rows, but no operands
    assert call(ctypes.byref(P), None) == ERR_NULL
    for missing in ("dy_ptr", "offsets_ptr") + (("dx_ptr",) if entry.endswith("dgrad") else ("x_ptr",)):
        P, keep = _params(entry)
        setattr(P, missing, None)
        assert call(ctypes.byref(P), None) == ERR_NULL, missing
    P, keep = _params(entry)
    keep[1][1] = None                                              # one expert's matrix is missing
    assert call(ctypes.byref(P), None) == ERR_NULL
    for kw in (dict(k=32, n=256), dict(k=128, n=32), dict(k=160, n=96, experts=64)):
        P, keep = _params(entry, tokens=0, pointers=False, **kw)
        assert call(ctypes.byref(P), None) == OK, kw               # no rows: a valid call that launches nothing
    P, keep = _params(entry, tokens=0, k=48, pointers=False)
    assert call(ctypes.byref(P), None) == ERR_SHAPE                # ... but still a checked one


def test_the_native_functions_refuse_cpu_tensors_unserved_widths_and_wrong_shapes():
    from dimsum_amd import native
    off = torch.zeros(3, dtype=torch.int32)
    z = torch.zeros
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        native.moe_gemm_dgrad(z(4, 32), off, [z(32, 64)] * 2)
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        native.moe_gemm_wgrad(z(4, 32), z(4, 64), off, 2, need_dbias=True)
    for width in (8, 48):                                          # refused, not emulated, whichever of the two widths it is
        for n, k in ((width, 32), (32, width)):
            with pytest.raises(RuntimeError, match="multiples of 32"):
                native.moe_gemm_dgrad(z(4, n), off, [z(n, k)] * 2)
            with pytest.raises(RuntimeError, match="multiples of 32"):
                native.moe_gemm_wgrad(z(4, n), z(4, k), off, 2)
    with pytest.raises(RuntimeError, match="experts"):
        native.moe_gemm_wgrad(z(4, 32), z(4, 32), z(66, dtype=torch.int32), 65)
    with pytest.raises(RuntimeError, match="experts"):
        native.moe_gemm_dgrad(z(4, 32), z(1, dtype=torch.int32), [])
    with pytest.raises(RuntimeError, match="float32"):
        native.moe_gemm_dgrad(z(4, 32).double(), off, [z(32, 32)] * 2)
    with pytest.raises(RuntimeError, match="float32"):
        native.moe_gemm_wgrad(z(4, 32), z(4, 32).double(), off, 2)
    with pytest.raises(RuntimeError, match="contiguous"):
        native.moe_gemm_dgrad(z(4, 64)[:, :32], off, [z(32, 32)] * 2)
    with pytest.raises(RuntimeError, match="x must be"):
        native.moe_gemm_wgrad(z(4, 32), z(5, 32), off, 2)            # another row count
    with pytest.raises(RuntimeError, match="every weight"):
        native.moe_gemm_dgrad(z(4, 32), off, [z(32, 32), z(64, 32)])
    with pytest.raises(RuntimeError, match="offsets"):
        native.moe_gemm_dgrad(z(4, 32), off.long(), [z(32, 32)] * 2)
    with pytest.raises(RuntimeError, match="offsets"):
        native.moe_gemm_wgrad(z(4, 32), z(4, 32), off, 3)
    with pytest.raises(RuntimeError, match="out must be"):
        native.moe_gemm_dgrad(z(4, 32), off, [z(32, 64)] * 2, out=z(4, 32))


# ---- the switch ------------------------------------------------------------------------------------------------------------------------------------
def test_grouped_train_is_off_by_default_opt_in_and_independent_of_grouped(monkeypatch):
    from dimsum_amd import switch_mlp
    from dimsum_amd.switch_mlp import SwitchMLP
    monkeypatch.delenv("DIMSUM_MOE_GROUPED_TRAIN", raising=False)
    monkeypatch.delenv("DIMSUM_MOE_GROUPED", raising=False)
    assert SwitchMLP(DIM, num_moe_experts=E).grouped_train is False
    assert SwitchMLP(DIM, num_moe_experts=E, grouped=True).grouped_train is False
    m = SwitchMLP(DIM, num_moe_experts=E, grouped_train=True)
    assert m.grouped_train is True and m.grouped is False
    monkeypatch.setenv("DIMSUM_MOE_GROUPED_TRAIN", "1")
    m = SwitchMLP(DIM, num_moe_experts=E)
    assert m.grouped_train is True and m.grouped is False
    assert SwitchMLP(DIM, num_moe_experts=E, grouped_train=False).grouped_train is False
    monkeypatch.setenv("DIMSUM_MOE_GROUPED_TRAIN", "0")
    assert SwitchMLP(DIM, num_moe_experts=E).grouped_train is False
    monkeypatch.setenv("DIMSUM_MOE_GROUPED", "1")
    m = SwitchMLP(DIM, num_moe_experts=E)
    assert m.grouped is True and m.grouped_train is False
    monkeypatch.delenv("DIMSUM_MOE_GROUPED")
    m.set_grouped_train(True)
    assert m.grouped_train is True and m.grouped is True
    m.set_grouped(False)
    assert m.grouped_train is True
    m.set_grouped_train(False)
    assert m.grouped_train is False
    tiny = _tiny()
    layers = [b.mixer for b in tiny.blocks if isinstance(b.mixer, SwitchMLP)]
    assert len(layers) == 2 and not any(l.grouped_train for l in layers)
    assert switch_mlp.set_grouped_train(tiny) == 2 and all(l.grouped_train for l in layers) and not any(l.grouped for l in layers)
    assert switch_mlp.set_grouped_train(tiny, False) == 2 and not any(l.grouped_train for l in layers)


def test_widths_the_kernels_do_not_serve_are_refused_and_the_model_setter_refuses_atomically(monkeypatch):
    from dimsum_amd import switch_mlp
    from dimsum_amd.switch_mlp import SwitchMLP
    monkeypatch.delenv("DIMSUM_MOE_GROUPED_TRAIN", raising=False)
    with pytest.raises(NotImplementedError, match="multiples of 32"):
        SwitchMLP(8, num_moe_experts=2, grouped_train=True)
    m = SwitchMLP(8, num_moe_experts=2)                              # (fine on the slice GEMMs)
    with pytest.raises(NotImplementedError, match="multiples of 32"):
        m.set_grouped_train(True)
    assert m.grouped_train is False
    monkeypatch.setenv("DIMSUM_MOE_GROUPED_TRAIN", "1")
    with pytest.raises(NotImplementedError, match="multiples of 32"):
        SwitchMLP(8, num_moe_experts=2)
    monkeypatch.delenv("DIMSUM_MOE_GROUPED_TRAIN")
    model = torch.nn.Sequential(SwitchMLP(DIM, num_moe_experts=2), SwitchMLP(8, num_moe_experts=2))       # the second one's widths are not served
    with pytest.raises(NotImplementedError, match="multiples of 32"):
        switch_mlp.set_grouped_train(model, True)
    assert [m.grouped_train for m in model] == [False, False]


def test_train_takes_the_flag():
    from dimsum_amd import train
    dests = {a.dest: a for a in train.build_parser()._actions}
    assert dests["moe_grouped_train"].default is False and dests["moe_grouped_train"].const is True
    assert "--moe-grouped-train" in dests["moe_grouped_train"].option_strings


# ---- dispatch and the layer on the stand-ins ---------------------------------------------------------------------------------------------------------
def test_only_grouped_train_sends_a_training_call_to_the_grouped_function(train_standins, calls):
    m = make_switch("top1", True, True, 3)
    x = torch.randn(2, 6, DIM)
    m.set_grouped(True)                                               # grouped alone: a call that trains keeps the slice GEMMs
    assert m(x).requires_grad and calls == ["autograd"]
    m.set_grouped_train(True)
    out = m(x)
    assert out.requires_grad and calls == ["autograd", "grouped_train"]
    with torch.no_grad():                                             # a call that does not train: `grouped` decides, as before
        m(x)
        m.set_grouped(False)
        m(x)
    assert calls == ["autograd", "grouped_train", "grouped", "autograd"]
    assert m(x).requires_grad and calls[4:] == ["grouped_train"]      # grouped_train without grouped
    m.set_grouped_train(False)
    m(x)
    assert calls[5:] == ["autograd"]


@pytest.mark.parametrize("mode,gated,bias", [("top1", True, True), ("sinkhorn", False, False), ("top1", False, True), ("sinkhorn", True, False)])
def test_forward_and_backward_run_without_a_host_read_and_match_float64(mode, gated, bias, train_standins, calls):
    from dimsum_amd.ops import switch_mlp_torch
    m = make_switch(mode, gated, bias, 3)
    m.set_grouped_train(True)
    x = torch.randn(2, 24, DIM, generator=torch.Generator().manual_seed(5))
    dout = torch.randn(2, 24, DIM, generator=torch.Generator().manual_seed(6))
    xg = x.clone().requires_grad_()
    with no_host_reads():
        out = m(xg)
        out.backward(dout)
    assert calls == ["grouped_train"]
    with torch.no_grad():
        m.set_grouped(True)
        assert torch.equal(m(x), out.detach())                        # the grouped inference forward, bit for bit: the same calls on the same data
    args = switch_args(m)
    xr = x.double().requires_grad_()
    want, _ = switch_mlp_torch(xr, *args, routing_mode=mode, gated=gated)
    want.backward(dout.double())
    close(out, want.detach(), "out")
    close(xg.grad, xr.grad, "dx")
    grads = named_grads(m, args)
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        close(p.grad, grads[k], k)


def test_an_expert_without_tokens_gets_exact_zeros_without_a_host_read(train_standins):
    m = make_switch("top1", True, True, 3)
    m.set_grouped_train(True)
    with torch.no_grad():
        m.router.bias[1] = -1e4
    x = torch.randn(2, 24, DIM, generator=torch.Generator().manual_seed(7)).requires_grad_()
    with no_host_reads():
        m(x).square().sum().backward()
    assert all(p.grad is not None and torch.count_nonzero(p.grad) == 0 for p in m.local_experts[1].parameters())
    assert all(torch.count_nonzero(p.grad) > 0 for p in m.local_experts[0].parameters())
    assert torch.count_nonzero(x.grad) > 0 and torch.count_nonzero(m.router.weight.grad) > 0


def test_the_patched_methods_do_catch_the_slice_path_that_trains(train_standins):
    m = make_switch("top1", True, False, 1)
    with pytest.raises(AssertionError, match="tolist"), no_host_reads():
        m(torch.zeros(2, 4, DIM))


def test_frozen_inputs_skip_their_launches(train_standins, monkeypatch):
    """needs_input_grad: frozen experts launch no wgrad; with x and the router frozen too the last dgrad and the router's adjoint are skipped"""
    from dimsum_amd import native
    seen = []
    for name in ("moe_gemm_dgrad", "moe_gemm_wgrad", "moe_route_bwd", "moe_act_bwd"):
        monkeypatch.setattr(native, name, lambda *a, _n=name, _r=getattr(native, name), **k: (seen.append(_n), _r(*a, **k))[1])
    m = make_switch("top1", True, True, 3)
    m.set_grouped_train(True)
    x = torch.randn(2, 6, DIM)
    m(x.clone().requires_grad_()).sum().backward()
    assert seen == ["moe_gemm_wgrad", "moe_gemm_dgrad", "moe_act_bwd", "moe_gemm_wgrad", "moe_gemm_dgrad", "moe_route_bwd"]
    seen.clear()
    for p in m.local_experts.parameters():
        p.requires_grad_(False)
    m.zero_grad()
    m(x).sum().backward()                                             # the router still trains
    assert seen == ["moe_gemm_dgrad", "moe_act_bwd", "moe_gemm_dgrad", "moe_route_bwd"]
    assert m.router.weight.grad is not None and all(p.grad is None for p in m.local_experts.parameters())
    seen.clear()
    for p in m.parameters():
        p.requires_grad_(False)
    for p in m.local_experts[0].linear_fc1.parameters():
        p.requires_grad_(True)
    m(x).sum().backward()                                             # only fc1 of one expert: no fc2 wgrad, no last dgrad, no router adjoint
    assert seen == ["moe_gemm_dgrad", "moe_act_bwd", "moe_gemm_wgrad"]
    assert m.local_experts[0].linear_fc1.weight.grad is not None and m.local_experts[1].linear_fc1.weight.grad is None
