"""The grouped expert GEMM on scaled-fp16 images (csrc/moe_gemm_f16.hip, native.moe_gemm_f16s) and the grouped SwitchMLP forward under the "f16s" policy,
host side: the three new entry points' declarations, struct layouts and refusals (no GPU is touched: every check runs before the launch), the gate
(gemm.moe_f16s_enabled), and the layer on torch stand-ins of the new entry points with every synchronising tensor method patched to raise."""
import ctypes
import os
import re

import pytest
import torch

from conftest import GOLDEN, golden
from test_moe_cpu import CASES, DIM, E, FILES, STANDINS, close, make_switch, tag_of
from test_moe_grouped_cpu import moe_gemm as moe_gemm_standin, no_host_reads

T = torch.from_numpy
OK, ERR_NULL, ERR_SHAPE, ERR_ABI = 0, 1, 3, 7
ENTRIES = {"dimsum_moe_gemm_f16s": "dimsum_moe_gemm_f16s_params_t", "dimsum_moe_permute_f16s": "dimsum_moe_permute_f16s_params_t",
           "dimsum_moe_act_fwd_f16s": "dimsum_moe_act_f16s_params_t"}


def _header():
    return open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "dimsum_hip.h")).read()


def test_the_entries_are_declared_exported_and_resolve_and_the_abi_is_still_18():
    from dimsum_amd import _lib
    lib = _lib.load()
    header = _header()
    for name, struct in ENTRIES.items():
        assert f"int {name}(const {struct} *p, void *stream);" in header, name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.dimsum_abi_version() == 18 and "#define DIMSUM_ABI_VERSION 18" in header


def _header_fields(struct):
    body = re.search(r"typedef struct \{([^}]*)\} " + struct + ";", _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype = ("u32" if decl.startswith("uint32_t") else "i32" if decl.startswith("int32_t") else "i64" if decl.startswith("int64_t") else "ptr")
        assert ctype != "ptr" or "*" in decl, decl
        fields += [(name, ctype) for name in re.findall(r"(\w+)\s*(?:,|$)", decl)]
    return fields


def test_the_ctypes_structs_have_the_headers_layout_and_the_old_structs_keep_their_size():
    from dimsum_amd import _lib
    kinds = {_lib.u32: "u32", _lib.i32: "i32", _lib.i64: "i64"}
    for cls, struct, size in ((_lib.MoeGemmF16sParams, "dimsum_moe_gemm_f16s_params_t", 2 * 4 + 4 * 8 + 8 * 8),
                              (_lib.MoePermuteF16sParams, "dimsum_moe_permute_f16s_params_t", 2 * 4 + 2 * 8 + 5 * 8),
                              (_lib.MoeActF16sParams, "dimsum_moe_act_f16s_params_t", 4 * 4 + 2 * 8 + 6 * 8)):
        fields = _header_fields(struct)
        assert [(n, kinds.get(t, "ptr")) for n, t in cls._fields_] == fields, struct
        assert fields[0] == ("struct_size", "u32") and fields[-1] == ("ext", "ptr")
        assert ctypes.sizeof(cls) == size and cls().struct_size == size, struct
    assert ctypes.sizeof(_lib.MoeGemmParams) == 2 * 4 + 4 * 8 + 6 * 8                      # (new structs are new structs)
    assert ctypes.sizeof(_lib.MoeRowsParams) == 2 * 4 + 2 * 8 + 7 * 8 and ctypes.sizeof(_lib.MoeActParams) == 4 * 4 + 2 * 8 + 7 * 8


def _base():
    buf = (ctypes.c_float * 64)()                 # host memory, never dereferenced: every refusal below comes before the launch
    return buf, (ctypes.addressof(buf) + 15) // 16 * 16


def _gemm_params(tokens=4, k=32, n=32, experts=2, pointers=True):
    from dimsum_amd import _lib
    P = _lib.MoeGemmF16sParams()
    P.tokens, P.k, P.n, P.ldc, P.num_experts = tokens, k, n, n, experts
    keep = []
    if pointers:
        buf, base = _base()
        tables = [(_lib.vp * 64)(*([base] * 64)) for _ in range(2)]
        P.x_ptr = P.x_inv_ptr = P.offsets_ptr = P.bias_ptr = P.out_ptr = base
        P.w_ptrs, P.w_inv_ptrs = tables
        keep = [buf] + tables
    return P, keep


def test_gemm_shapes_outside_the_kernel_are_error_codes():
    from dimsum_amd import _lib
    call = _lib.load().dimsum_moe_gemm_f16s
    assert call(None, None) == ERR_NULL
    P, keep = _gemm_params()
    P.struct_size -= 8
    assert call(ctypes.byref(P), None) == ERR_ABI
    for kw in (dict(k=48), dict(k=0), dict(n=48), dict(n=0), dict(experts=0), dict(experts=65), dict(tokens=-1)):
        P, keep = _gemm_params(**kw)
        assert call(ctypes.byref(P), None) == ERR_SHAPE, kw
    P, keep = _gemm_params(pointers=False)
    assert call(ctypes.byref(P), None) == ERR_NULL
    for missing in ("x_ptr", "x_inv_ptr", "offsets_ptr", "out_ptr"):
        P, keep = _gemm_params()
        setattr(P, missing, None)
        assert call(ctypes.byref(P), None) == ERR_NULL, missing
    for table in (1, 2):
        P, keep = _gemm_params()
        keep[table][1] = None                                           # one expert's image / scales are missing
        assert call(ctypes.byref(P), None) == ERR_NULL
    for kw in (dict(k=32, n=256), dict(k=128, n=32), dict(k=160, n=32, experts=64)):
        P, keep = _gemm_params(tokens=0, pointers=False, **kw)
        assert call(ctypes.byref(P), None) == OK, kw                    # no rows: a valid call that launches nothing
    P, keep = _gemm_params(tokens=0, k=48, pointers=False)
    assert call(ctypes.byref(P), None) == ERR_SHAPE


def test_producer_shapes_outside_the_kernels_are_error_codes():
    from dimsum_amd import _lib
    lib = _lib.load()
    buf, base = _base()
    assert lib.dimsum_moe_permute_f16s(None, None) == ERR_NULL and lib.dimsum_moe_act_fwd_f16s(None, None) == ERR_NULL
    P = _lib.MoePermuteF16sParams()
    P.rows, P.hidden = 4, 32
    assert lib.dimsum_moe_permute_f16s(ctypes.byref(P), None) == ERR_NULL            # rows, but no pointers
    P.hidden = 30
    assert lib.dimsum_moe_permute_f16s(ctypes.byref(P), None) == ERR_SHAPE
    P.rows, P.hidden = 0, 32
    assert lib.dimsum_moe_permute_f16s(ctypes.byref(P), None) == OK
    P.struct_size -= 8
    assert lib.dimsum_moe_permute_f16s(ctypes.byref(P), None) == ERR_ABI
    A = _lib.MoeActF16sParams()
    A.rows, A.width, A.num_experts = 4, 32, 1
    assert lib.dimsum_moe_act_fwd_f16s(ctypes.byref(A), None) == ERR_NULL
    for kw in (dict(width=30), dict(width=5124), dict(num_experts=0), dict(num_experts=65), dict(rows=-1)):
        A = _lib.MoeActF16sParams()
        A.rows, A.width, A.num_experts = 4, 32, 1
        for k, v in kw.items():
            setattr(A, k, v)
        assert lib.dimsum_moe_act_fwd_f16s(ctypes.byref(A), None) == ERR_SHAPE, kw
    A = _lib.MoeActF16sParams()
    A.rows, A.width, A.num_experts = 4, 32, 2
    A.x_ptr = A.out_ptr = A.inv_scale_ptr = base                                     # two experts need row_expert
    assert lib.dimsum_moe_act_fwd_f16s(ctypes.byref(A), None) == ERR_NULL
    A.rows = 0
    assert lib.dimsum_moe_act_fwd_f16s(ctypes.byref(A), None) == OK


def _image(rows, k, dtype=torch.float16, inv_dtype=torch.float32):
    from dimsum_amd.native import F16Image
    return F16Image(torch.zeros(rows, k, dtype=dtype), torch.ones(rows, dtype=inv_dtype))


def test_native_moe_gemm_f16s_refuses_before_the_device():
    from dimsum_amd import native
    off = torch.zeros(3, dtype=torch.int32)
    call = native.moe_gemm_f16s
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        call(_image(4, 32), off, [_image(32, 32)] * 2)
    with pytest.raises(RuntimeError, match="F16Images"):
        call(torch.zeros(4, 32), off, [_image(32, 32)] * 2)
    with pytest.raises(RuntimeError, match="F16Images"):
        call(_image(4, 32), off, [torch.zeros(32, 32)] * 2)
    with pytest.raises(RuntimeError, match="x16 must be contiguous float16"):
        call(_image(4, 32, dtype=torch.bfloat16), off, [_image(32, 32)] * 2)
    with pytest.raises(RuntimeError, match="x16 must be contiguous float16"):
        call(_image(4, 32, inv_dtype=torch.float64), off, [_image(32, 32)] * 2)
    with pytest.raises(RuntimeError, match="every weight image must be contiguous float16"):
        call(_image(4, 32), off, [_image(32, 32), _image(32, 32, dtype=torch.bfloat16)])
    with pytest.raises(RuntimeError, match="every weight image must be contiguous float16"):
        call(_image(4, 32), off, [_image(32, 32), _image(64, 32)])
    with pytest.raises(RuntimeError, match=r"K % 32 == 0 and N % 32 == 0 \(got K 48, N 32\)"):
        call(_image(4, 48), off, [_image(32, 48)] * 2)
    with pytest.raises(RuntimeError, match=r"K % 32 == 0 and N % 32 == 0 \(got K 32, N 48\)"):
        call(_image(4, 32), off, [_image(48, 32)] * 2)
    with pytest.raises(RuntimeError, match="1 <= experts <= 64"):
        call(_image(4, 32), off, [])
    with pytest.raises(RuntimeError, match="1 <= experts <= 64"):
        call(_image(4, 32), torch.zeros(66, dtype=torch.int32), [_image(32, 32)] * 65)
    for bad in (torch.zeros(3, dtype=torch.int64), torch.zeros(4, dtype=torch.int32), torch.zeros(6, dtype=torch.int32)[::2]):
        with pytest.raises(RuntimeError, match=r"offsets must be contiguous int32 \(3,\)"):
            call(_image(4, 32), bad, [_image(32, 32)] * 2)
    with pytest.raises(RuntimeError, match=r"bias must be contiguous float32 \(2, 32\)"):
        call(_image(4, 32), off, [_image(32, 32)] * 2, bias=torch.zeros(2, 16))
    for bad in (torch.zeros(4, 32, dtype=torch.float64), torch.zeros(5, 32), torch.zeros(32, 4).t(), torch.zeros(4, 64)[:, ::2]):
        with pytest.raises(RuntimeError, match=r"out must be a float32 \(4, 32\) view"):
            call(_image(4, 32), off, [_image(32, 32)] * 2, out=bad)


def test_the_producers_refuse_cpu_tensors_and_unknown_images():
    from dimsum_amd import native
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        native.moe_permute(torch.zeros(4, 32), torch.zeros(4, dtype=torch.int32), split3="f16s")
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        native.moe_act_fwd(torch.zeros(4, 64), None, None, True, split3="f16s")
    with pytest.raises(RuntimeError, match="split3 is False or 'f16s'"):
        native.moe_permute(torch.zeros(4, 32), torch.zeros(4, dtype=torch.int32), split3=True)
    with pytest.raises(RuntimeError, match="split3 is False or 'f16s'"):
        native.moe_act_fwd(torch.zeros(4, 64), split3="pair")


# ---- the gate --------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def policy(monkeypatch):
    from dimsum_amd import gemm
    monkeypatch.delenv("DIMSUM_MOE_F16S", raising=False)
    monkeypatch.setenv("DIMSUM_SPLIT3_MIN_ROWS", "0")              # (the image carriers' row threshold: these layers are small)
    monkeypatch.setattr(torch.backends.cuda.matmul, "allow_tf32", True)
    yield gemm
    gemm.set_policy("default")


def _layer_weights(dim=DIM, experts=E):
    m = make_switch("top1", True, True, 1, dim=dim, experts=experts)
    return [q.linear_fc1.weight for q in m.local_experts], [q.linear_fc2.weight for q in m.local_experts]


def test_the_gate(policy, monkeypatch):
    gemm = policy
    w1, w2 = _layer_weights()
    x = torch.zeros(6, DIM)
    assert gemm.get_policy() == "default" and not gemm.moe_f16s_enabled(x, w1, w2)           # off by default: the policy is opt-in
    gemm.set_policy("fp16")
    assert not gemm.moe_f16s_enabled(x, w1, w2)
    gemm.set_policy("f16s")
    assert gemm.moe_f16s_enabled(x, w1, w2) is True                                         # on under the policy
    assert not gemm.moe_f16s_enabled(x, w1, w2, trains=True)                                # a call that trains
    monkeypatch.setattr(torch.backends.cuda.matmul, "allow_tf32", False)
    assert not gemm.moe_f16s_enabled(x, w1, w2)
    monkeypatch.setattr(torch.backends.cuda.matmul, "allow_tf32", True)
    monkeypatch.setenv("DIMSUM_MOE_F16S", "0")
    assert not gemm.moe_f16s_enabled(x, w1, w2)
    monkeypatch.setenv("DIMSUM_MOE_F16S", "1")
    assert gemm.moe_f16s_enabled(x, w1, w2)
    assert not gemm.moe_f16s_enabled(x.double(), w1, w2)
    monkeypatch.delenv("DIMSUM_SPLIT3_MIN_ROWS")                                            # the carriers' default threshold: 8192 rows
    assert not gemm.moe_f16s_enabled(x, w1, w2) and not gemm.moe_f16s_enabled(torch.zeros(8191, DIM), w1, w2)
    assert gemm.moe_f16s_enabled(torch.zeros(2, 4096, DIM), w1, w2)
    monkeypatch.setenv("DIMSUM_SPLIT3_MIN_ROWS", "0")
    narrow = [torch.zeros(24, 8)] * 2, [torch.zeros(8, 12)] * 2                              # widths the kernel does not serve
    assert not gemm.moe_f16s_enabled(torch.zeros(6, 8), *narrow)


def test_the_plan_holds_the_experts_of_grouped_layers_only(policy, monkeypatch):
    gemm = policy
    m = make_switch("top1", True, False, 1)
    model = torch.nn.Sequential(m)
    assert gemm.f16s_plan(model) == []
    m.set_grouped(True)
    plan = gemm.f16s_plan(model)
    want = [lin.weight for q in m.local_experts for lin in (q.linear_fc1, q.linear_fc2)]
    assert len(plan) == 2 * E and all(p[0] is w and p[1:] == ("plain", None, None) for p, w in zip(plan, want))
    monkeypatch.setenv("DIMSUM_MOE_F16S", "0")
    assert gemm.f16s_plan(model) == []


# ---- the layer on stand-ins ------------------------------------------------------------------------------------------------------------------------
def _to_image(x):
    """torch restatement of the scaled-fp16 image (csrc/common.hpp, f16s_scales / f16s_pack4) without a host read"""
    from dimsum_amd.native import F16Image
    m = x.abs().amax(-1, keepdim=True)
    e = torch.floor(torch.log2(m.double().clamp_min(2.0 ** -112))).clamp(-112, 127)
    scale = torch.pow(torch.tensor(2.0, dtype=torch.float64), 14 - e).float()
    return F16Image((x * scale).half(), (1.0 / scale.double()).float().squeeze(-1))


@pytest.fixture
def f16s_standins(monkeypatch):
    from dimsum_amd import gemm, native
    calls = {k: 0 for k in ("permute_f16s", "act_f16s", "gemm_f16s", "images", "permute", "act", "gemm")}

    def count(key, fn):
        def f(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        return f

    def permute(x, perm, split3=False):
        calls["permute_f16s" if split3 else "permute"] += 1
        xp = STANDINS["moe_permute"](x, perm)
        return _to_image(xp) if split3 else xp

    def act(x, bias=None, row_expert=None, gated=True, split3=False):
        calls["act_f16s" if split3 else "act"] += 1
        h = STANDINS["moe_act_fwd"](x, bias, row_expert, gated)
        return _to_image(h) if split3 else h

    def gemm_f16s(x16, offsets, images, bias=None, out=None):
        return moe_gemm_standin(x16.float(), offsets, [w.float() for w in images], bias, out)

    for k, f in STANDINS.items():
        monkeypatch.setattr(native, k, f)
    monkeypatch.setattr(native, "moe_permute", permute)
    monkeypatch.setattr(native, "moe_act_fwd", act)
    monkeypatch.setattr(native, "moe_gemm", count("gemm", moe_gemm_standin))
    monkeypatch.setattr(native, "moe_gemm_f16s", count("gemm_f16s", gemm_f16s))
    monkeypatch.setattr(gemm, "expert_images_f16s", count("images", lambda ws: [_to_image(w) for w in ws]))
    return calls


@pytest.mark.parametrize("mode,gated,bias", CASES)
def test_the_layer_under_the_policy_calls_the_new_entries_without_a_host_read(mode, gated, bias, f16s_standins, policy):
    calls = f16s_standins
    g, tag = golden(FILES[mode]), tag_of(gated, bias)
    m = make_switch(mode, gated, bias, int(g[tag + ".seed"]))
    m.set_grouped(True)
    x = T(g["x"])
    policy.set_policy("f16s")
    with no_host_reads(), torch.no_grad():
        out = m(x)
    assert calls == dict(permute_f16s=1, act_f16s=1, gemm_f16s=2, images=1, permute=0, act=0, gemm=0)
    # (wiring, not accuracy -- the GPU tests bound the kernels: the stand-ins round the operands to fp16's 11 bits, so the fixture is met to a
    # few 2^-11 of its magnitude and not to fp32 roundoff)
    want = T(g[tag + ".out"]).double()
    assert (out.double() - want).abs().max().item() <= 1e-2 * want.abs().max().item()
    assert not torch.equal(out.double(), want)
    for k in calls:
        calls[k] = 0
    policy.set_policy("default")                                   # the default policy: the fp32 grouped path, the fixture at its own tolerance
    with no_host_reads(), torch.no_grad():
        out = m(x)
    assert calls == dict(permute_f16s=0, act_f16s=0, gemm_f16s=0, images=0, permute=1, act=1, gemm=2)
    close(out, g[tag + ".out"], "out")


def test_a_call_that_trains_keeps_the_autograd_function_under_the_policy(f16s_standins, policy):
    calls = f16s_standins
    policy.set_policy("f16s")
    m = make_switch("top1", True, True, 3)
    m.set_grouped(True)
    out = m(torch.randn(2, 6, DIM))
    assert out.requires_grad and calls["gemm_f16s"] == calls["permute_f16s"] == calls["act_f16s"] == calls["images"] == 0
