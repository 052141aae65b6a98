"""The recurrent form of the mixer without a GPU: the two plain-torch restatements (ops: causal_conv1d_update_torch,
selective_state_update_torch) against the reference fixture mixer_step.npz; Mamba / CondMamba forward(inference_params=...) + step against the
fixture's module rows, on the CPU oracle backend with the two native entry points of the step replaced by the restatements (the oracle package
knows nothing of them); the inference cache; every refusal; the C ABI of the two entry points.
Bound: the reference tests' own fp32 one, rtol 3e-4, atol 1e-3 (causal-conv1d/tests/test_causal_conv1d.py:93,
mamba/tests/ops/triton/test_selective_state_update.py:18); the conv state is compared exactly."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden
from oracle.torch_backend import cpu_oracle_backend
from procedural import procedural_fill
from test_host_logic import _header_layout
from test_model_cpu import build_mixer

T = torch.from_numpy
FP32 = dict(rtol=3e-4, atol=1e-3)
CONV_CASES = [(B, D, W, b, s) for B, D, W in ((2, 5, 2), (2, 5, 3), (3, 65, 4)) for b in (0, 1) for s in (0, 1)]
SSU_CASES = [(B, D, N, z, d) for B, D, N in ((2, 5, 1), (2, 65, 16), (1, 7, 64)) for z in (0, 1) for d in (0, 1)]
MIXER = dict(d_model=32, d_state=16, d_conv=4, expand=2)
L, PREFILL = 12, 5


def close(a, b, what):
    a, b = (np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, np.float64) for t in (a, b))
    assert a.shape == b.shape, what
    err = np.abs(a - b) - (FP32["atol"] + FP32["rtol"] * np.abs(b))
    assert (err <= 0).all(), f"{what}: max |err| {np.abs(a - b).max():.3e}"


def conv_case(g, B, D, W, b, s):
    tag = f"conv_B{B}D{D}W{W}_b{b}s{s}_"
    return {k: T(g[tag + k]).clone() if tag + k in g.files else None for k in ("x", "state_in", "weight", "bias", "out", "state_out")}


def ssu_case(g, B, D, N, z, d):
    tag = f"ssu_B{B}D{D}N{N}_z{z}d{d}_"
    return {k: T(g[tag + k]).clone() if tag + k in g.files else None
            for k in ("state_in", "x", "dt", "dt_bias", "A", "B", "C", "D", "z", "out", "state_out")}


# ---- plain-torch stand-ins of native.causal_conv1d_update / native.selective_state_update (same signatures and results) ------------------------
def native_conv_update(x, conv_state, weight, bias, silu_activation):
    from dimsum_amd.ops import causal_conv1d_update_torch
    return causal_conv1d_update_torch(x, conv_state, weight, bias, "silu" if silu_activation else None)


def native_state_update(state, x, dt, A, B, C, D=None, z=None, dt_bias=None, dt_softplus=False, dt_proj=None):
    from dimsum_amd.ops import selective_state_update_torch
    if dt_proj is not None:
        assert dt is None
        dt = F.linear(dt_proj[1], dt_proj[0])
    return selective_state_update_torch(state, x, dt, A, B, C, D, z, dt_bias, dt_softplus)


@pytest.fixture
def step_backend(monkeypatch):
    from dimsum_amd import native
    monkeypatch.setattr(native, "causal_conv1d_update", native_conv_update)
    monkeypatch.setattr(native, "selective_state_update", native_state_update)
    with cpu_oracle_backend():
        yield


def mixer(cls, **over):
    from dimsum_amd.modules import mamba_simple
    kw = dict(MIXER, layer_idx=3, scan_type="none", **({"d_cond": 48} if cls == "CondMamba" else {}))
    kw.update(over)
    m = getattr(mamba_simple, cls)(**kw).eval()
    procedural_fill(m, seed=7)
    return m


def run_recurrent(m, x, args, prefill, params=None):
    """forward over `prefill` tokens with a cache, then one step per remaining token -> (outputs (B, L, d_model), the InferenceParams)"""
    from dimsum_amd.utils import InferenceParams
    p = params or InferenceParams(max_seqlen=x.shape[1], max_batch_size=x.shape[0])
    with torch.no_grad():
        ys = [m(x[:, :prefill], *args, inference_params=p)]
        for t in range(prefill, x.shape[1]):
            p.seqlen_offset = t
            ys.append(m(x[:, t:t + 1], *args, inference_params=p))
    return torch.cat(ys, 1), p


# ---- the restatements ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "B%dD%dW%d_b%ds%d" % c)
def test_conv_update_restatement_reproduces_the_fixture(case):
    from dimsum_amd.ops import causal_conv1d_update_torch
    c = conv_case(golden("mixer_step"), *case)
    state = c["state_in"].clone()
    out = causal_conv1d_update_torch(c["x"], state, c["weight"], c["bias"], "silu" if case[4] else None)
    assert np.array_equal(state.numpy(), c["state_out"].numpy())
    assert torch.equal(state[:, :, :-1], c["state_in"][:, :, 1:]) and torch.equal(state[:, :, -1], c["x"])
    close(out, c["out"], "out")
    with pytest.raises(NotImplementedError):
        causal_conv1d_update_torch(c["x"], state, c["weight"], c["bias"], "gelu")


@pytest.mark.parametrize("case", SSU_CASES, ids=lambda c: "B%dD%dN%d_z%dd%d" % c)
def test_state_update_restatement_reproduces_the_fixture(case):
    from dimsum_amd.ops import selective_state_update_torch
    c = ssu_case(golden("mixer_step"), *case)
    state = c["state_in"].clone()
    out = selective_state_update_torch(state, c["x"], c["dt"], c["A"], c["B"], c["C"], D=c["D"], z=c["z"], dt_bias=c["dt_bias"], dt_softplus=True)
    close(state, c["state_out"], "state")
    close(out, c["out"], "out")
    # ... and in float64 (what the GPU tests compare the kernel with) it is the same function
    c64 = {k: v.double() if v is not None else None for k, v in c.items()}
    out64 = selective_state_update_torch(c64["state_in"], c64["x"], c64["dt"], c64["A"], c64["B"], c64["C"], D=c64["D"], z=c64["z"],
                                         dt_bias=c64["dt_bias"], dt_softplus=True)
    assert out64.dtype == torch.float64
    close(out64, c["out"], "out64")
    close(c64["state_in"], c["state_out"], "state64")


# ---- the modules -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["Mamba", "CondMamba"])
def test_prefill_then_steps_match_the_reference_module(cls, step_backend):
    g = golden("mixer_step")
    m = mixer(cls)
    x = T(g[f"{cls}_x"])
    args = (T(g[f"{cls}_c"]),) if cls == "CondMamba" else ()
    ys, p = run_recurrent(m, x, args, PREFILL)
    conv_state, ssm_state = p.key_value_memory_dict[3]
    close(ys, g[f"{cls}_y_steps"], "prefill + steps")
    close(ys, g[f"{cls}_y_full"], "prefill + steps vs one forward")
    close(conv_state, g[f"{cls}_conv_state"], "conv_state")
    close(ssm_state, g[f"{cls}_ssm_state"], "ssm_state")
    with torch.no_grad():
        close(m(x, *args), g[f"{cls}_y_full"], "one forward, no cache")       # inference_params=None: the path every other test runs


def test_step_signature_and_in_place_states(step_backend):
    g = golden("mixer_step")
    m = mixer("Mamba")
    x = T(g["Mamba_x"])
    conv_state, ssm_state = m.allocate_inference_cache(2, L)
    with torch.no_grad():
        outs = []
        for t in range(L):
            out, cs, ss = m.step(x[:, t:t + 1], conv_state, ssm_state)
            assert out.shape == (2, 1, 32) and cs is conv_state and ss is ssm_state
            outs.append(out)
    close(torch.cat(outs, 1), g["Mamba_y_full"], "12 steps from zero states")
    close(conv_state, g["Mamba_conv_state"], "conv_state")
    close(ssm_state, g["Mamba_ssm_state"], "ssm_state")
    with pytest.raises(AssertionError, match="1 token"):
        m.step(x[:, :2], conv_state, ssm_state)
    from dimsum_amd.utils import InferenceParams
    p = InferenceParams(max_seqlen=L, max_batch_size=2, seqlen_offset=3)
    with pytest.raises(AssertionError, match="1 token"):
        m(x[:, :2], inference_params=p)


def test_inference_cache(step_backend):
    from dimsum_amd.utils import InferenceParams
    m0, m1 = mixer("Mamba", layer_idx=0), mixer("CondMamba", layer_idx=1)
    conv_state, ssm_state = m0.allocate_inference_cache(3, 99)
    assert conv_state.shape == (3, 64, 4) and ssm_state.shape == (3, 64, 16)
    assert conv_state.dtype == m0.conv1d.weight.dtype and ssm_state.dtype == m0.dt_proj.weight.dtype
    assert not conv_state.any() and not ssm_state.any()
    c16, s16 = m0.allocate_inference_cache(1, 9, dtype=torch.float16)
    assert c16.dtype == s16.dtype == torch.float16 and c16.shape == (1, 64, 4) and s16.shape == (1, 64, 16)
    # two layers share one InferenceParams, keyed by layer_idx; reset() rewinds, initialize_states zeroes in place
    p = InferenceParams(max_seqlen=L, max_batch_size=2)
    assert p.seqlen_offset == 0 and p.key_value_memory_dict == {}
    x = T(golden("mixer_step")["Mamba_x"])
    with torch.no_grad():
        h = m0(x[:, :PREFILL], inference_params=p)
        m1(h, None, inference_params=p)
    assert sorted(p.key_value_memory_dict) == [0, 1]
    (c0, s0), (c1, s1) = p.key_value_memory_dict[0], p.key_value_memory_dict[1]
    assert c0.data_ptr() != c1.data_ptr() and c0.any() and s0.any() and c1.any() and s1.any() and not torch.equal(s0, s1)
    got = m0._get_states_from_cache(p, 2)
    assert got[0] is c0 and got[1] is s0 and c0.any()
    got = m0._get_states_from_cache(p, 2, initialize_states=True)
    assert got[0] is c0 and not c0.any() and not s0.any() and c1.any()
    p.seqlen_offset = 7
    p.reset(5, 1)
    assert (p.max_seqlen, p.max_batch_size, p.seqlen_offset) == (5, 1, 0)
    with pytest.raises(AssertionError):
        mixer("Mamba", layer_idx=None)._get_states_from_cache(p, 2)


def test_the_cache_carries_no_autograd_edge(step_backend):
    """a prompt processed with grad enabled (a module left in train mode): the output is differentiable as ever, the cache is plain data"""
    from dimsum_amd.utils import InferenceParams
    m = mixer("Mamba").train()
    x = T(golden("mixer_step")["Mamba_x"]).clone().requires_grad_()
    p = InferenceParams(max_seqlen=L, max_batch_size=2)
    y = m(x[:, :PREFILL], inference_params=p)
    conv_state, ssm_state = p.key_value_memory_dict[3]
    assert y.requires_grad and conv_state.any() and ssm_state.any()
    for t in (conv_state, ssm_state):
        assert not t.requires_grad and t.grad_fn is None
    y.sum().backward()
    assert x.grad is not None and x.grad[:, :PREFILL].any()


@pytest.mark.parametrize("short", [1, 2, 3])
def test_a_prompt_shorter_than_d_conv_is_zero_padded_on_the_left(short, step_backend):
    g = golden("mixer_step")
    m = mixer("Mamba")
    x = T(g["Mamba_x"])
    ys, p = run_recurrent(m, x, (), short)
    conv_state = p.key_value_memory_dict[3][0]
    close(ys, g["Mamba_y_full"], "short prompt + steps")
    close(conv_state, g["Mamba_conv_state"], "conv_state")
    # the cache right after the prompt: the same as a prompt with d_conv - short zero tokens in front (zero inputs -> zero pre-conv values)
    from dimsum_amd.utils import InferenceParams
    pa, pb = (InferenceParams(max_seqlen=L, max_batch_size=2) for _ in range(2))
    with torch.no_grad():
        m(x[:, :short], inference_params=pa)
        m(F.pad(x[:, :short], (0, 0, 4 - short, 0)), inference_params=pb)
    ca, cb = pa.key_value_memory_dict[3][0], pb.key_value_memory_dict[3][0]
    assert torch.equal(ca, cb) and not ca[:, :, :4 - short].any() and ca[:, :, 4 - short:].any()


def test_refusals(step_backend):
    from dimsum_amd.models_dim import DiM, create_block
    from dimsum_amd.utils import InferenceParams
    from test_model_cpu import _published
    p = InferenceParams(max_seqlen=64, max_batch_size=2)
    x = torch.zeros(2, 64, 32)
    v2, zig = build_mixer("condmamba_v2"), build_mixer("condmamba_zigma8")
    for m, why in ((v2, "no causal recurrence"), (zig, "no token-by-token order")):
        with pytest.raises(NotImplementedError, match=why):
            m(x, None, inference_params=p)
        with pytest.raises(NotImplementedError, match=why):
            m.step(x[:, :1], *m.allocate_inference_cache(2, 64))
    plain = mixer("Mamba")
    with pytest.raises(NotImplementedError, match="do not combine"):
        plain(None, inference_params=p, x3=torch.zeros(2, 64, 96, dtype=torch.bfloat16))
    assert p.key_value_memory_dict == {}                                   # refused before a cache entry is made
    blk = create_block(128, norm_epsilon=1e-5, rms_norm=True, residual_in_fp32=True, fused_add_norm=True, layer_idx=1, scan_type="none",
                       block_type="combined", reverse=False, transpose=False, cond_mamba=True, scanning_continuity=False, use_gated_mlp=True)
    with pytest.raises(NotImplementedError, match="none of that is causal"):
        blk(torch.zeros(2, 16, 128), None, torch.zeros(2, 128), inference_params=p)
    with pytest.raises(NotImplementedError, match="none of that is causal"):
        blk.allocate_inference_cache(2, 16)
    model = DiM(depth=2, hidden_size=64, patch_size=2, **_published(img_resolution=8)).eval()
    with pytest.raises(NotImplementedError, match="none of that is causal"):
        model(torch.zeros(2, 4, 8, 8), torch.zeros(2), torch.zeros(2, dtype=torch.long), inference_params=p)


def test_wrappers_refuse_clearly():
    from dimsum_amd import native, ops
    x, st, w = torch.zeros(2, 8), torch.zeros(2, 8, 4), torch.zeros(8, 4)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        native.causal_conv1d_update(x, st, w, None, True)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.causal_conv1d_update(x, st, w, None, "silu")
    with pytest.raises(NotImplementedError, match="silu"):
        ops.causal_conv1d_update(x, st, w, None, "gelu")
    s, A, B = torch.zeros(2, 8, 16), torch.zeros(8, 16), torch.zeros(2, 16)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        native.selective_state_update(s, x, x, A, B, B)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.selective_state_update(s, x, x, A, B, B, dt_softplus=True)


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------------------------
STRUCTS = [("dimsum_conv_update_params_t", "ConvUpdateParams"), ("dimsum_state_update_params_t", "StateUpdateParams"),
           ("dimsum_state_update_ext_t", "StateUpdateExt")]
SYMBOLS = (("dimsum_causal_conv1d_update", "ConvUpdateParams"), ("dimsum_selective_state_update", "StateUpdateParams"))


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
    header = open(_lib.os.path.join(_lib._HERE, "..", "include", "dimsum_hip.h")).read()
    for name, m in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(lib, name) and f"int {name}(" in header, name
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
    P = _lib.ConvUpdateParams()
    P.x_ptr = P.weight_ptr = P.conv_state_ptr = P.out_ptr = addr
    for B, D, W in ((1, 4, 1), (1, 4, 5), (0, 4, 4), (1, 0, 4), (-1, 4, 4)):
        P.batch, P.dim, P.width = B, D, W
        assert lib.dimsum_causal_conv1d_update(P, None) == 3, (B, D, W)
    P.batch, P.dim, P.width, P.dtype = 1, 4, 4, 3
    assert lib.dimsum_causal_conv1d_update(P, None) == 2
    Q = _lib.StateUpdateParams()
    for f in ("state_ptr", "x_ptr", "dt_ptr", "A_ptr", "B_ptr", "C_ptr", "out_ptr"):
        setattr(Q, f, addr)
    for B, D, N in ((1, 4, 0), (1, 4, 257), (0, 4, 16), (1, 0, 16)):
        Q.batch, Q.dim, Q.dstate = B, D, N
        assert lib.dimsum_selective_state_update(Q, None) == 3, (B, D, N)
    Q.batch, Q.dim, Q.dstate = 1, 4, 16
    for dtype, sdt, bdt, want in ((3, 0, 0, 2), (1, 2, 0, 2), (1, 0, 2, 2)):
        Q.dtype, Q.state_dtype, Q.bc_dtype = dtype, sdt, bdt
        assert lib.dimsum_selective_state_update(Q, None) == want, (dtype, sdt, bdt)
    Q.dtype = Q.state_dtype = Q.bc_dtype = 0
    Q.dt_ptr = None
    assert lib.dimsum_selective_state_update(Q, None) == 1        # neither dt nor the dt_proj extension
    E = _lib.attach_ext(Q, _lib.StateUpdateExt)
    E.dt_w_ptr = addr
    assert lib.dimsum_selective_state_update(Q, None) == 1        # dt_w without dt_x
    E.dt_x_ptr = addr
    assert lib.dimsum_selective_state_update(Q, None) == 3        # dt_rank 0
    E.struct_size += 8
    assert lib.dimsum_selective_state_update(Q, None) == 7        # an extension larger than the library's
