"""The CPU twin of test_decode_paths_gpu.py: its case builders run on the CPU and every case must sit on the launch route it is meant to
reach (`decode_route`, all but the base-pointer alignment of a GPU allocation), so a shape edit that loses a leaf of the decode launcher fails
here as well; the LayerNorm conditioning case has teeth (a one-pass variance in float32 breaks the bound the two-pass one keeps); the float64
model reference of the GPU test reproduces the model's own cached steps."""
import pytest
import torch
import torch.nn.functional as F

import test_decode_paths_gpu as G
import test_mixer_step_gpu
from test_lm_cpu import decode_linear_torch, lm_backend, run_cached, tiny_model  # noqa: F401  (lm_backend: a fixture)
from test_lm_gpu import DTYPES
from test_mixer_step_cpu import close


@pytest.fixture(autouse=True)
def build_on_the_cpu(monkeypatch):
    monkeypatch.setattr(test_mixer_step_gpu, "DEV", "cpu")                    # where `rnd` puts what it draws


def test_decode_route_at_the_launcher_thresholds():
    x = lambda b, k, dt=torch.float32: torch.zeros(b, k, dtype=dt)  # noqa: E731
    w = lambda n, k, dt=torch.float32: torch.zeros(n, k, dtype=dt)  # noqa: E731
    r = lambda *a, **k: G.decode_route(*a, check_ptr=False, **k)  # noqa: E731
    assert [r(x(1, 8), w(n, 8))["rows"] for n in (16383, 16384)] == [1, 4]
    assert [r(x(1, 8), w(n, 8))["waves"] for n in (512, 513)] == [1, 4]
    assert [r(x(b, 8), w(513, 8))["waves"] for b in (4, 5)] == [4, 8]
    assert r(x(16, 8), w(16390, 8))["waves"] == 8                              # 4098 wave-rows
    assert [r(x(b, 8), w(4, 8))["kbatch"] for b in range(1, 17)] == [1, 2, 4, 4] + [8] * 4 + [16] * 8
    assert [r(x(1, k), w(4, k))["chunks"] for k in (1024, 1025, 2048, 2049)] == [1, 2, 2, 3]
    assert [r(x(1, k, torch.bfloat16), w(4, k, torch.bfloat16))["chunks"] for k in (2048, 2049)] == [1, 2]
    assert r(x(2, 6), w(4, 6)) == dict(vec_w=False, vec_x=False, rows=1, waves=1, kbatch=2, chunks=1)       # 24-byte rows
    assert r(x(1, 6), w(1, 6))["vec_w"] and r(x(1, 6), w(1, 6))["vec_x"]       # one row: only the base counts
    assert not r(x(2, 8), w(4, 8), norm=(None, None))["vec_x"]                 # the prologue stages x' itself
    assert not r(x(2, 12)[:, 1:9], w(4, 8))["vec_x"] and not r(x(2, 8), w(4, 12)[:, 1:9])["vec_w"]        # a base 4 bytes past alignment


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("cases", G.PLAIN_BUILDERS, ids=lambda f: f.__name__)
def test_plain_cases_sit_on_their_routes(cases, dtype):
    n = 0
    for c in cases(dtype):
        assert c["x"].device.type == "cpu" and c["x"].dtype == c["w"].dtype == c["b"].dtype == dtype
        assert c["x"].shape[1] == c["w"].shape[1] and c["b"].shape == c["w"].shape[:1] and c["x"].stride(1) == c["w"].stride(1) == 1
        G.on_route(c["x"], c["w"], check_ptr=False, **c["route"])
        n += 1
    assert n >= 2


def test_plain_cases_cover_the_leaves_together():
    for dtype in DTYPES:
        routes = [dict(G.decode_route(c["x"], c["w"], check_ptr=False), batch=c["x"].shape[0], x_stride=c["x"].stride(0), k=c["x"].shape[1])
                  for cases in G.PLAIN_BUILDERS for c in cases(dtype)]
        assert {r["kbatch"] for r in routes if r["vec_w"] and r["chunks"] > 1} == {1, 2, 4, 8, 16}
        assert {r["waves"] for r in routes if r["vec_w"] and r["chunks"] > 1} == {1, 4, 8}
        assert {r["chunks"] for r in routes if r["vec_w"]} >= {1, 2, 3}
        assert any(r["vec_x"] and r["batch"] > 1 and r["x_stride"] != r["k"] and r["chunks"] > 1 for r in routes)
        assert any(r["rows"] == 4 and r["chunks"] > 1 for r in routes) and any(not r["vec_w"] and r["chunks"] > 1 for r in routes)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_prologue_and_epilogue_cases_sit_on_their_routes(dtype):
    seen = set()
    for B, N, K, head, route in G.prologue_shapes(dtype):
        x, w, b, res, nw, nb = G.prologue_inputs(dtype, torch.float32, B, N, K)
        assert res.shape == x.shape and res.stride(0) == K and nw.shape == nb.shape == (K,)
        assert (nw[-1] - nw[0]).item() > 0.5 and (nb[0] - nb[-1]).item() > 0.5       # the ramp outweighs the noise
        G.on_route(x, w, norm=(nw, nb), check_ptr=False, **route)
        seen.add((route["waves"], route["rows"], route["chunks"]))
    assert seen == {(8, 1, 1), (4, 1, 1), (1, 1, 2), (4, 4, 1), (8, 4, 1)}
    for B, route in ((16, dict(waves=8, kbatch=16)), (3, dict(waves=4, kbatch=4)), (7, dict(waves=8, kbatch=8))):
        x, w, *_, nw, nb = G.epilogue_operands(dtype, True, B)
        G.on_route(x, w, norm=(nw, nb), check_ptr=False, rows=1, **route)
    for B in (2, 16):
        x, w, *_, nw, nb = G.epilogue_operands(dtype, True, B, 16390, 72)
        G.on_route(x, w, norm=(nw, nb), check_ptr=False, rows=4, kbatch=B)


def test_state_layouts_have_the_strides_they_are_named_for():
    B, D, W = 3, 7, 4
    cw, cb, st = G.conv_inputs(torch.float32, B, D, W)
    (_, a, abuf, am), (_, t, tbuf, tm), (_, p, pbuf, pm) = G.state_layouts(st)
    for v in (a, t, p):
        assert v.shape == (B, D, W) and torch.equal(v, st)
    assert abuf.shape == (B + 2, D, W) and a.stride() == (D * W, W, 1) and am.sum().item() == 2 * D * W
    assert t.stride() == (W * D, 1, D) and tm.sum().item() == 0               # state_w_stride == D
    assert p.stride() == (D * (W + 1), W + 1, 1) and pm.sum().item() == B * D  # rows not W-packed


# ---- the LayerNorm conditioning case has teeth -------------------------------------------------------------------------------------------------------
def layer_norm_linear_f32(x, w, b, res, nw, nb, one_pass):
    """the kernel's LayerNorm prologue and product restated in float32; one_pass: the variance as E[r^2] - mean^2"""
    r = x + res
    mean = r.mean(-1, keepdim=True)
    var = ((r * r).mean(-1, keepdim=True) - mean * mean) if one_pass else ((r - mean) ** 2).mean(-1, keepdim=True)
    return F.linear((r - mean) * torch.rsqrt(var + 1e-5) * nw + nb, w, b)


def test_the_conditioning_case_tells_a_one_pass_variance_from_a_two_pass_one():
    x, w, b, res, nw, nb = G.conditioning_inputs()
    assert x.dtype == torch.float32 and x.shape == (4, 768) and w.shape == (64, 768)
    r = x + res
    assert abs(r.mean().item() - G.COND_MEAN) < 0.1 and 0.9 < r.std(-1).min().item() and r.std(-1).max().item() < 1.2
    ref = decode_linear_torch(*G.dbl(x, w, b), norm=(nw.double(), nb.double(), 1e-5, False), residual=res.double())
    chain = F.linear(F.layer_norm(r, (768,), nw, nb, 1e-5), w, b)               # the unfused chain: torch's own float32 LayerNorm
    err = lambda y: (y.double() - ref).abs().max().item()  # noqa: E731
    bound = 2 * err(chain) + G.SLACK * ref.abs().max().item()
    two, one = err(layer_norm_linear_f32(x, w, b, res, nw, nb, False)), err(layer_norm_linear_f32(x, w, b, res, nw, nb, True))
    also = err(decode_linear_torch(x, w, b, norm=(nw, nb, 1e-5, False), residual=res))
    print(f"mean {G.COND_MEAN}: bound {bound:.3e}, two-pass err {two:.3e} ({also:.3e} through decode_linear_torch), one-pass err {one:.3e}")
    assert two <= bound and also <= bound
    assert one > bound


# ---- the float64 model reference -------------------------------------------------------------------------------------------------------------------
def test_the_float64_reference_walk_reproduces_the_models_cached_steps(lm_backend, monkeypatch):  # noqa: F811
    """reference_step_logits (every token through the recurrent form from zero states, float64) against the model's own prompt + cached steps
    in float32 on the CPU backend, on one layer of the tiny sizes"""
    torch.manual_seed(3)
    m = tiny_model(1, 1, n_layer=1)
    g = torch.Generator().manual_seed(4)
    prompt, teacher = torch.randint(0, 90, (2, G.LM_PROMPT), generator=g), torch.randint(0, 90, (2, G.LM_STEPS + 1), generator=g)
    ref = G.reference_step_logits(m, prompt, teacher)
    assert ref.dtype == torch.float64 and ref.shape == (2, G.LM_STEPS, 96)
    for fused in ("1", "0"):
        monkeypatch.setenv("DIMSUM_FUSED_DECODE", fused)
        close(run_cached(m, prompt, G.LM_STEPS, teacher=teacher)[1], ref.float(), f"steps fused={fused}")


def test_the_paths_model_has_the_sizes_the_gpu_test_routes_on():
    m = G.paths_model()
    mixer = m.backbone.layers[0].mixer
    assert mixer.in_proj.weight.shape == (2304, 576) and mixer.x_proj.weight.shape == (68, 1152) and mixer.out_proj.weight.shape == (576, 1152)
    assert m.lm_head.weight.shape == (16390, 576) and mixer.conv1d.weight.shape == (1152, 1, 4)
    x = torch.zeros(16, 2304)[:, :1152]
    r = G.decode_route(x, mixer.x_proj.weight, check_ptr=False)
    assert r["vec_x"] and r["vec_w"] and r["chunks"] == 2 and G.decode_route(x[:, :576], m.lm_head.weight, (1, None), check_ptr=False)["rows"] == 4
