"""The decode step on the GPU: dimsum_decode_linear (csrc/decode_step.hip) against float64 on every path its launcher takes, its add + norm
prologue and conv-update epilogue against float64 with the existing unfused chain as the yardstick, bit-reproducibility; the language model's
prompt + cached steps against the reference fixtures, fused against unfused, generate() eager against graph-captured, the launches of one
fused step, a 16-bit model.

Bounds. The plain product, per element: the first-order bound of a K-term fp32 dot product in any order, K 2^-24 sum_k |x_k W_nk|, with a
factor 2, plus half an ulp of T at |y| for a 16-bit output. Prologue / epilogue: at most twice the error of the unfused chain
(layer_norm_fn -> F.linear -> causal_conv1d_update on the same inputs) against the same float64 restatement -- the factor 2 is for the
different summation order -- plus 4 * 2^-24 * max|y|. Model: the fp32 tolerances test_mixer_step_gpu.py uses under `exact_fp32`, and
test_state_update_dtype_pairings' for 16 bits."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from conftest import golden
from test_lm_cpu import PROMPT, STEPS, VARIANTS, decode_linear_torch, run_cached, tiny_model
from test_mixer_step_gpu import SSU_TOL, close, exact_fp32, rnd  # noqa: F401  (exact_fp32: a fixture)

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = "cuda"
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
HALF_ULP = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
# the issue's shapes, then the launcher's other paths: K over more than one 4-KiB chunk of x' (1024 fp32 / 2048 16-bit elements) with a
# tail, and N at the threshold from which a wave owns four rows (16384: 4099 waves' rows, the last wave with one valid row)
SHAPES = [(1, 7), (5, 64), (96, 260), (1001, 128), (6, 2307), (16389, 40)]


def linear_case(batch, N, K, dtype, seed=0):
    return rnd(batch, K, dtype=dtype, seed=seed), rnd(N, K, dtype=dtype, seed=seed + 1) * K ** -0.5, rnd(N, dtype=dtype, seed=seed + 2)


def check_linear(x, w, b, what):
    from dimsum_amd import native
    y = native.decode_linear(x, w, b)
    assert y.dtype == x.dtype and y.shape == (x.shape[0], w.shape[0])
    x64, w64 = x.double(), w.double()
    want = x64 @ w64.t() + (b.double() if b is not None else 0.0)
    mag = x64.abs() @ w64.abs().t() + (b.double().abs() if b is not None else 0.0)
    bound = 2 * x.shape[1] * 2.0 ** -24 * mag + HALF_ULP[x.dtype] * want.abs() + 1e-30
    err = (y.double() - want).abs()
    worst = (err / bound).max().item()
    print(f"{what}: max err {err.max().item():.3e}, worst err / bound {worst:.3f}")
    assert worst <= 1.0, what
    return y


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%dK%d" % s)
def test_decode_linear_against_float64(shape, dtype):
    N, K = shape
    for batch in (1, 3, 16):
        x, w, b = linear_case(batch, N, K, dtype, seed=batch)
        for bias in (None, b):
            check_linear(x, w, bias, f"B{batch} N{N} K{K} bias={bias is not None}")
        wide = rnd(batch, K + 5, dtype=dtype, seed=batch + 7)              # a row-strided view, its base off 16-byte alignment
        xv = wide[:, 3:3 + K]
        assert torch.equal(check_linear(xv, w, b, "strided x"), check_linear(xv.contiguous(), w, b, "its copy"))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_two_launches_are_bit_identical_and_rows_do_not_depend_on_the_grid(dtype):
    """of the grid, only the batch tile varies here; the same rows on 1 / 4 / 8 waves and under one and four rows per wave are
    test_decode_paths_gpu.py::test_rows_do_not_depend_on_the_grid"""
    from dimsum_amd import native
    for N, K in ((1001, 128), (96, 260), (16389, 40)):
        x, w, b = linear_case(16, N, K, dtype, seed=3)
        y1, y2 = native.decode_linear(x, w, b), native.decode_linear(x, w, b)
        assert torch.equal(y1, y2)
        assert torch.equal(native.decode_linear(x[:5], w, b), y1[:5])         # a batch row's sum does not depend on the batch tile


def prologue_case(dtype, res_dtype, width):
    B, K, N, D = 3, 64, 256, 128
    x, w, b = linear_case(B, N, K, dtype, seed=11)
    res = rnd(B, K, dtype=res_dtype, seed=14)
    nw, nb = (1 + 0.1 * rnd(K, seed=15)).to(dtype), (0.1 * rnd(K, seed=16)).to(dtype)
    cw, cb, st = rnd(D, width, dtype=dtype, seed=17), rnd(D, dtype=dtype, seed=18), rnd(B, D, width, dtype=dtype, seed=19)
    return x, w, b, res, nw, nb, cw, cb, st


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("rms", [True, False], ids=["rms", "ln"])
@pytest.mark.parametrize("res32", [True, False], ids=["res32", "resT"])
def test_prologue_and_epilogue(dtype, rms, res32):
    from dimsum_amd import native
    from dimsum_amd.ops import causal_conv1d_update
    from dimsum_amd.ops.layernorm import layer_norm_fn
    res_dtype = torch.float32 if res32 else dtype
    for width, silu in itertools.product((3, 4), (True, False)):
        x, w, b, res, nw, nb, cw, cb, st = prologue_case(dtype, res_dtype, width)
        nb_ = None if rms else nb
        D = cw.shape[0]
        s_fused, s_chain = st.clone(), st.clone()
        y, ro = native.decode_linear(x, w, b, norm=(nw, nb_, 1e-5, rms), residual=res, residual_out=res_dtype, conv=(s_fused, cw, cb, silu))
        pre = native.decode_linear(x, w, b, norm=(nw, nb_, 1e-5, rms), residual=res)           # the same launch without the epilogue
        assert ro.dtype == res_dtype and torch.equal(ro, x.to(res_dtype) + res)              # a single add in the residual's dtype
        assert torch.equal(s_fused, torch.cat([st[:, :, 1:], pre[:, :D, None]], dim=2))         # the roll, then the stored pre-activation value
        assert torch.equal(y[:, D:], pre[:, D:])
        # the unfused chain on the same inputs
        h, ro_chain = layer_norm_fn(x, nw, nb_, residual=res, eps=1e-5, prenorm=True, residual_in_fp32=res32, is_rms_norm=rms)
        xz = F.linear(h, w, b)
        chain = torch.cat([causal_conv1d_update(xz[:, :D], s_chain, cw, cb, "silu" if silu else None), xz[:, D:]], 1)
        assert torch.equal(ro_chain, ro)
        # float64: the restatement on the inputs as rounded to T (x' stays unrounded in it: both chains carry the rounding of x' to T as error)
        s64 = st.double()
        want = decode_linear_torch(x.double(), w.double(), b.double(), norm=(nw.double(), None if rms else nb.double(), 1e-5, rms),
                                   residual=res.double(), conv=(s64, cw.double(), cb.double(), silu))
        want_pre = decode_linear_torch(x.double(), w.double(), b.double(), norm=(nw.double(), None if rms else nb.double(), 1e-5, rms), residual=res.double())
        slack = 4 * 2.0 ** -24
        for name, got, ref, yard in (("y", y, want, chain), ("pre-activation", pre, want_pre, xz),
                                     ("state", s_fused[:, :, -1], s64[:, :, -1], s_chain[:, :, -1])):
            e_fused, e_chain = (got.double() - ref).abs().max().item(), (yard.double() - ref).abs().max().item()
            bound = 2 * e_chain + slack * ref.abs().max().item()
            print(f"{name} W{width} silu={silu}: fused err {e_fused:.3e}, unfused chain err {e_chain:.3e}, bound {bound:.3e}")
            assert e_fused <= bound, (name, width, silu)


def test_first_layer_and_head_forms_of_the_prologue():
    """no incoming residual (the first block: residual_out = x in the residual dtype) and no residual_out (the head: prenorm=False)"""
    from dimsum_amd import native
    for dtype in (torch.float32, torch.bfloat16):
        x, w, b, res, nw, nb, *_ = prologue_case(dtype, torch.float32, 4)
        y, ro = native.decode_linear(x, w, None, norm=(nw, None, 1e-5, True), residual_out=torch.float32)
        assert ro.dtype == torch.float32 and torch.equal(ro, x.float())
        want = decode_linear_torch(x.double(), w.double(), None, norm=(nw.double(), None, 1e-5, True))
        close(y, want, SSU_TOL[dtype], "first layer")
        y = native.decode_linear(x, w, None, norm=(nw, nb, 1e-5, False), residual=res)
        want = decode_linear_torch(x.double(), w.double(), None, norm=(nw.double(), nb.double(), 1e-5, False), residual=res.double())
        close(y, want, SSU_TOL[dtype], "head")


# ---- the model -------------------------------------------------------------------------------------------------------------------------------------
def gpu_model(rms, fp32res, dtype=None):
    g = golden(f"lm_tiny_rms{rms}_fp32res{fp32res}")
    m = tiny_model(rms, fp32res, g).to(DEV)
    return (m if dtype is None else m.to(dtype)), g


@pytest.mark.parametrize("rms,fp32res", VARIANTS)
def test_prompt_and_steps_match_the_fixtures_fused_and_unfused(rms, fp32res, exact_fp32, monkeypatch):  # noqa: F811
    m, g = gpu_model(rms, fp32res)
    tol = SSU_TOL[torch.float32]
    outs = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("DIMSUM_FUSED_DECODE", fused)
        pl, sl, ids = run_cached(m, T(g["prompt"]).to(DEV), STEPS)
        close(pl, T(g["prompt_logits"]), tol, f"prompt logits fused={fused}")
        close(sl, T(g["step_logits"]), tol, f"step logits fused={fused}")
        err = max((pl.cpu() - T(g["prompt_logits"])).abs().max().item(), (sl.cpu() - T(g["step_logits"])).abs().max().item())
        print(f"fused={fused}: max |logit error| {err:.3e}, min_gap {float(g['min_gap']):.3e}")
        assert err < float(g["min_gap"]) / 4
        assert torch.equal(ids.cpu(), T(g["ids"]))
        outs[fused] = sl
    close(outs["1"], outs["0"], tol, "fused vs unfused steps")


def test_generate_from_a_captured_graph_equals_eager(exact_fp32):  # noqa: F811
    m, g = gpu_model(1, 1)
    prompt = T(g["prompt"]).to(DEV)
    other = (prompt + 5) % 90
    L = PROMPT + STEPS + 1
    eager = m.generate(prompt, max_length=L, return_dict_in_generate=True, output_scores=True)
    assert torch.equal(eager.sequences[:, PROMPT:].cpu(), T(g["ids"]))
    cg = m.generate(prompt, max_length=L, return_dict_in_generate=True, output_scores=True, cg=True)
    assert torch.equal(cg.sequences, eager.sequences) and len(cg.scores) == len(eager.scores) == STEPS + 1
    for a, b in zip(cg.scores, eager.scores):
        assert torch.equal(a, b)
    cache = m._decoding_cache
    assert cache.n_captures == 1 and list(cache.callables) == [(2, 1)]
    cg2 = m.generate(other, max_length=L, return_dict_in_generate=True, output_scores=True, cg=True)
    eager2 = m.generate(other, max_length=L, return_dict_in_generate=True, output_scores=True)
    assert m._decoding_cache is cache and cache.n_captures == 1                 # another prompt of the same batch size: nothing new captured
    assert torch.equal(cg2.sequences, eager2.sequences) and all(torch.equal(a, b) for a, b in zip(cg2.scores, eager2.scores))
    one = m.generate(prompt[:1], max_length=L, return_dict_in_generate=True, output_scores=True, cg=True)
    assert cache.n_captures == 2 and sorted(cache.callables) == [(1, 1), (2, 1)]  # batch 1 gets its own graph
    eager1 = m.generate(prompt[:1], max_length=L, return_dict_in_generate=True, output_scores=True)
    assert torch.equal(one.sequences, eager1.sequences) and all(torch.equal(a, b) for a, b in zip(one.scores, eager1.scores))
    again = m.generate(prompt, max_length=L, cg=True)                          # back to batch 2: its graph is still there
    assert cache.n_captures == 2 and torch.equal(again, eager.sequences)


def one_step_calls(m, g):
    """the library calls of ONE cached step after the fixture's prompt -> the list of their names"""
    from dimsum_amd import gemm, native
    from dimsum_amd.utils import InferenceParams
    prompt = T(g["prompt"]).to(DEV)
    p = InferenceParams(max_seqlen=PROMPT + 1, max_batch_size=2)
    calls = []
    with torch.no_grad(), pytest.MonkeyPatch.context() as mp:
        m(prompt, inference_params=p)
        p.seqlen_offset = PROMPT

        def spy(mod, name):
            fn = getattr(mod, name)
            mp.setattr(mod, name, lambda *a, **k: calls.append(name) or fn(*a, **k))

        for name in ("decode_linear", "selective_state_update", "causal_conv1d_update", "layer_norm_fwd"):
            spy(native, name)
        spy(gemm, "neg_exp")
        spy(F, "linear")
        m(prompt[:, :1], inference_params=p, num_last_tokens=1)
    return calls


def test_the_launches_of_one_fused_step(exact_fp32, monkeypatch):  # noqa: F811
    m, g = gpu_model(1, 1)
    monkeypatch.setenv("DIMSUM_FUSED_DECODE", "1")
    layer = ["decode_linear", "decode_linear", "neg_exp", "selective_state_update", "decode_linear"]
    assert one_step_calls(m, g) == layer * 2 + ["decode_linear"]
    monkeypatch.setenv("DIMSUM_FUSED_DECODE", "0")
    calls = one_step_calls(m, g)
    assert "decode_linear" not in calls and calls.count("linear") == 3 * 2 + 1 and calls.count("layer_norm_fwd") == 3


def test_a_16_bit_model_takes_the_fused_path(monkeypatch):
    m, g = gpu_model(1, 1, torch.bfloat16)
    monkeypatch.setenv("DIMSUM_FUSED_DECODE", "1")
    calls = one_step_calls(m, g)
    layer = ["decode_linear", "decode_linear", "neg_exp", "decode_linear", "selective_state_update", "decode_linear"]   # dt_proj: its own GEMV
    assert calls == layer * 2 + ["decode_linear"]
    outs = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("DIMSUM_FUSED_DECODE", fused)
        outs[fused] = run_cached(m, T(g["prompt"]).to(DEV), STEPS, teacher=T(g["ids"]).to(DEV))      # the fixture's tokens: one trajectory for both
        assert outs[fused][1].dtype == torch.bfloat16
    assert torch.equal(outs["1"][0], outs["0"][0])                             # the prompt takes one path
    close(outs["1"][1], outs["0"][1], SSU_TOL[torch.bfloat16], "fused vs unfused bf16 steps")
