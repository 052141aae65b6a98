"""The grouped expert GEMM (csrc/moe_gemm.hip, native.moe_gemm) and the grouped inference forward of SwitchMLP, host side: the entry point's
declaration, struct layout and refusals (no GPU is touched: every check runs before the launch), the grouped forward on torch stand-ins against
the reference's fixtures with every synchronising tensor method patched to raise, and the opt-in rules (off by default, DIMSUM_MOE_GROUPED=1,
set_grouped, what hip_graph.GraphedForward accepts, training calls keep the autograd function)."""
import contextlib
import ctypes
import os
import re

import pytest
import torch

from conftest import GOLDEN, golden
from test_moe_cpu import CASES, DIM, E, FILES, STANDINS, _tiny, close, make_switch, tag_of

T = torch.from_numpy
OK, ERR_NULL, ERR_SHAPE, ERR_ABI = 0, 1, 3, 7


def moe_gemm(xp, offsets, weights, bias=None, out=None):
    """torch stand-in of native.moe_gemm that, like the kernel, never brings the offsets to the host: the expert of row j is the number of range ends
    <= j, and every row multiplies its own expert's matrix"""
    rows = torch.arange(xp.shape[0], device=xp.device)
    e = torch.bucketize(rows, offsets[1:].long(), right=True).clamp_(max=len(weights) - 1)
    y = torch.bmm(torch.stack(list(weights))[e], xp.unsqueeze(2)).squeeze(2)
    if bias is not None:
        y = y + bias[e]
    if out is None:
        return y
    out.copy_(y)
    return out


@pytest.fixture
def grouped_standins(monkeypatch):
    from dimsum_amd import native
    for k, f in dict(STANDINS, moe_gemm=moe_gemm).items():
        monkeypatch.setattr(native, k, f)


def _header():
    return open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "dimsum_hip.h")).read()


def test_the_entry_is_declared_exported_and_resolves_and_the_abi_is_still_18():
    from dimsum_amd import _lib, native
    lib = _lib.load()
    header = _header()
    assert "int dimsum_moe_gemm(const dimsum_moe_gemm_params_t *p, void *stream);" in header
    assert "dimsum_moe_gemm" in _lib.EXPORTS and hasattr(lib, "dimsum_moe_gemm")
    assert lib.dimsum_abi_version() == 18 and "#define DIMSUM_ABI_VERSION 18" in header
    bm, bn = (int(re.search(rf"#define DIMSUM_MOE_GEMM_{k}\s+(\d+)", header).group(1)) for k in ("BM", "BN"))
    assert (native.MOE_GEMM_BM, native.MOE_GEMM_BN) == (bm, bn)


def test_the_ctypes_struct_has_the_headers_layout():
    from dimsum_amd import _lib
    body = re.search(r"typedef struct \{([^}]*)\} dimsum_moe_gemm_params_t;", _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype = ("u32" if decl.startswith("uint32_t") else "i32" if decl.startswith("int32_t") else "i64" if decl.startswith("int64_t") else "ptr")
        assert ctype != "ptr" or "*" in decl, decl
        fields += [(name, ctype) for name in re.findall(r"(\w+)\s*(?:,|$)", decl)]
    kinds = {_lib.u32: "u32", _lib.i32: "i32", _lib.i64: "i64"}
    assert [(n, kinds.get(t, "ptr")) for n, t in _lib.MoeGemmParams._fields_] == fields
    assert fields[0] == ("struct_size", "u32") and fields[-1] == ("ext", "ptr") and len(fields) == 12
    assert ctypes.sizeof(_lib.MoeGemmParams) == 2 * 4 + 4 * 8 + 6 * 8
    assert _lib.MoeGemmParams().struct_size == ctypes.sizeof(_lib.MoeGemmParams)


def _params(tokens=4, k=32, n=32, experts=2, pointers=True):
    from dimsum_amd import _lib
    P = _lib.MoeGemmParams()
    P.tokens, P.k, P.n, P.ldc, P.num_experts = tokens, k, n, n, experts
    keep = []
    if pointers:                               # host memory, never dereferenced: every refusal below comes before the launch
        buf = (ctypes.c_float * 64)()
        base = (ctypes.addressof(buf) + 15) // 16 * 16
        table = (_lib.vp * 64)(*([base] * 64))
        P.x_ptr = P.offsets_ptr = P.bias_ptr = P.out_ptr = base
        P.w_ptrs = table
        keep = [buf, table]
    return P, keep


def test_shapes_outside_the_kernel_are_error_codes():
    from dimsum_amd import _lib
    call = _lib.load().dimsum_moe_gemm
    assert call(None, None) == ERR_NULL
    P, keep = _params()
    P.struct_size -= 8                                              # a stale struct size is refused before anything else is read
    assert call(ctypes.byref(P), None) == ERR_ABI
    for kw in (dict(k=48), dict(k=0), dict(n=48), dict(n=0), dict(experts=0), dict(experts=65), dict(tokens=-1)):
        P, keep = _params(**kw)
        assert call(ctypes.byref(P), None) == ERR_SHAPE, kw
    P, keep = _params(pointers=False)                               # rows, but no operands
    assert call(ctypes.byref(P), None) == ERR_NULL
    for missing in ("x_ptr", "offsets_ptr", "out_ptr"):
        P, keep = _params()
        setattr(P, missing, None)
        assert call(ctypes.byref(P), None) == ERR_NULL, missing
    P, keep = _params()
    keep[1][1] = None                                               # one expert's matrix is missing
    assert call(ctypes.byref(P), None) == ERR_NULL
    for kw in (dict(k=32, n=256), dict(k=32, n=128), dict(k=128, n=32), dict(k=64, n=512), dict(k=160, n=32, experts=64)):      # the fixtures' and the tiny model's widths
        P, keep = _params(tokens=0, pointers=False, **kw)
        assert call(ctypes.byref(P), None) == OK, kw                # no rows: a valid call that launches nothing
    P, keep = _params(tokens=0, k=48, pointers=False)
    assert call(ctypes.byref(P), None) == ERR_SHAPE                 # ... but still a checked one


def test_native_moe_gemm_refuses_cpu_tensors_and_unserved_widths():
    from dimsum_amd import native
    assert native.moe_gemm_serves(32, 256, 4) and native.moe_gemm_serves(128, 32, 64) and native.moe_gemm_serves(64, 512, 1)
    assert not native.moe_gemm_serves(48, 32, 4) and not native.moe_gemm_serves(32, 48, 4) and not native.moe_gemm_serves(32, 32, 65)
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        native.moe_gemm(torch.zeros(4, 32), torch.zeros(3, dtype=torch.int32), [torch.zeros(32, 32)] * 2)


@contextlib.contextmanager
def no_host_reads():
    """inside: Tensor.tolist / .item / .cpu raise"""
    def refuse(name):
        def f(*a, **k):
            raise AssertionError(f"the forward called Tensor.{name}: a host synchronisation")
        return f
    with pytest.MonkeyPatch.context() as mp:
        for name in ("tolist", "item", "cpu"):
            mp.setattr(torch.Tensor, name, refuse(name))
        yield


@pytest.mark.parametrize("mode,gated,bias", CASES)
def test_grouped_forward_reproduces_the_reference_without_a_host_read(mode, gated, bias, grouped_standins):
    g, tag = golden(FILES[mode]), tag_of(gated, bias)
    m = make_switch(mode, gated, bias, int(g[tag + ".seed"]))
    m.set_grouped(True)
    x = T(g["x"])
    with no_host_reads(), torch.no_grad():
        out = m(x)
    close(out, g[tag + ".out"], "out")
    for p in m.parameters():                       # nothing requires grad: the grouped path serves the call in grad mode too
        p.requires_grad_(False)
    with no_host_reads():
        out = m(x)
    close(out, g[tag + ".out"], "out (grad mode on, nothing requires grad)")


def test_the_patched_methods_do_catch_the_ungrouped_forward(grouped_standins):
    m = make_switch("top1", True, False, 1)
    with pytest.raises(AssertionError, match="tolist"), no_host_reads(), torch.no_grad():
        m(torch.zeros(2, 4, DIM))


def test_grouped_is_off_by_default_and_opt_in(monkeypatch):
    from dimsum_amd import switch_mlp
    from dimsum_amd.switch_mlp import SwitchMLP
    monkeypatch.delenv("DIMSUM_MOE_GROUPED", raising=False)
    assert SwitchMLP(DIM, num_moe_experts=E).grouped is False
    assert SwitchMLP(DIM, num_moe_experts=E, grouped=True).grouped is True
    monkeypatch.setenv("DIMSUM_MOE_GROUPED", "1")
    assert SwitchMLP(DIM, num_moe_experts=E).grouped is True
    assert SwitchMLP(DIM, num_moe_experts=E, grouped=False).grouped is False
    monkeypatch.setenv("DIMSUM_MOE_GROUPED", "0")
    assert SwitchMLP(DIM, num_moe_experts=E).grouped is False
    m = _tiny()
    layers = [b.mixer for b in m.blocks if isinstance(b.mixer, SwitchMLP)]
    assert len(layers) == 2 and not any(l.grouped for l in layers)
    assert switch_mlp.set_grouped(m, True) == 2 and all(l.grouped for l in layers)
    assert switch_mlp.set_grouped(m, False) == 2 and not any(l.grouped for l in layers)


def test_a_grouped_layer_the_kernel_does_not_serve_is_refused_at_construction(monkeypatch):
    from dimsum_amd.switch_mlp import SwitchMLP
    monkeypatch.delenv("DIMSUM_MOE_GROUPED", raising=False)
    with pytest.raises(NotImplementedError, match="multiples of 32"):
        SwitchMLP(8, num_moe_experts=2, grouped=True)
    m = SwitchMLP(8, num_moe_experts=2)                      # (fine ungrouped)
    with pytest.raises(NotImplementedError, match="multiples of 32"):
        m.set_grouped(True)
    assert m.grouped is False
    monkeypatch.setenv("DIMSUM_MOE_GROUPED", "1")
    with pytest.raises(NotImplementedError, match="multiples of 32"):
        SwitchMLP(8, num_moe_experts=2)


def test_set_grouped_on_a_model_checks_every_layer_before_it_flips_any():
    from dimsum_amd import switch_mlp
    from dimsum_amd.switch_mlp import SwitchMLP
    model = torch.nn.Sequential(SwitchMLP(DIM, num_moe_experts=2), SwitchMLP(8, num_moe_experts=2))       # the second one's widths are not served
    with pytest.raises(NotImplementedError, match="multiples of 32"):
        switch_mlp.set_grouped(model, True)
    assert [m.grouped for m in model] == [False, False]


def test_hip_graph_accepts_a_model_only_when_every_layer_is_grouped():
    from dimsum_amd import switch_mlp
    from dimsum_amd.hip_graph import GraphedForward
    m = _tiny()
    with pytest.raises(NotImplementedError, match="MoEBlock"):
        GraphedForward(m)
    m.blocks[1].mixer.set_grouped(True)                      # one of the two layers
    with pytest.raises(NotImplementedError, match="MoEBlock"):
        GraphedForward(m)
    with pytest.raises(NotImplementedError, match="MoEBlock"):
        GraphedForward(m.forward)
    switch_mlp.set_grouped(m, True)
    assert GraphedForward(m).fn is m and GraphedForward(m.forward).graphs == {}


def test_a_grouped_layer_that_trains_takes_the_autograd_function(grouped_standins, monkeypatch):
    from dimsum_amd.ops import moe
    calls = []
    real_grouped, real_apply = moe.switch_mlp_grouped_fwd, moe._SwitchMlpFn.apply
    monkeypatch.setattr(moe, "switch_mlp_grouped_fwd", lambda *a, **k: (calls.append("grouped"), real_grouped(*a, **k))[1])
    monkeypatch.setattr(moe._SwitchMlpFn, "apply", staticmethod(lambda *a: (calls.append("autograd"), real_apply(*a))[1]))
    m = make_switch("top1", True, True, 3)
    m.set_grouped(True)
    x = torch.randn(2, 6, DIM)
    out = m(x)                                               # the parameters require grad
    assert calls == ["autograd"] and out.requires_grad
    out.sum().backward()
    assert all(p.grad is not None for p in m.parameters())
    with torch.no_grad():
        quiet = m(x)
    assert calls == ["autograd", "grouped"] and not quiet.requires_grad
    close(quiet, out.detach().double(), "grouped against the autograd function")
    m.set_grouped(False)
    with torch.no_grad():
        m(x)
    assert calls == ["autograd", "grouped", "autograd"]


def test_sample_ddp_takes_the_flag():
    from dimsum_amd import sample_ddp
    dests = {a.dest: a for a in sample_ddp.build_parser()._actions}
    assert dests["moe_grouped"].default is False and dests["moe_grouped"].const is True
