"""dimsum_decode_linear (csrc/decode_step.hip) on the launch paths only real sizes reach: K over several 4-KiB chunks of x' on the vector-weight
path, strided x and weight rows, every batch tile, four rows per wave, the add + norm prologue on 1 / 4 / 8 waves and over two chunks, the conv
epilogue at every width, without a bias, on strided states and taps and where conv_dim falls inside a wave's four rows; then the language
model at the smallest sizes whose step reaches those leaves, against its own weights in float64.

The launcher's choice cannot be seen from Python: `decode_route` restates it, every case asserts the route it is meant to reach before it
launches, and test_decode_paths_cpu.py builds the same cases on the CPU and asserts the same routes (all but the base-pointer alignment), so
that a shape edit which loses a leaf fails without a GPU too.

Bounds: the two of test_lm_gpu.py, unchanged. The plain product per element, 2 K 2^-24 sum_k |x_k W_nk| + half an ulp of T (`check_linear`).
Prologue / epilogue / model, as maxima: fused error <= 2 * (error of the unfused chain on the same inputs) + 4 * 2^-24 * max|ref|, both
against the float64 restatement `decode_linear_torch`."""
import copy
import functools
import itertools

import pytest
import torch
import torch.nn.functional as F

from test_lm_cpu import LM_TINY, decode_linear_torch, run_cached, tiny_model
from test_lm_gpu import DTYPES, check_linear, linear_case
from test_mixer_step_cpu import native_state_update
from test_mixer_step_gpu import SSU_TOL, close, exact_fp32, rnd  # noqa: F401  (exact_fp32: a fixture)

pytestmark = pytest.mark.gpu
CH = {torch.float32: 1024, torch.float16: 2048, torch.bfloat16: 2048}       # elements of K per chunk: 256 pieces of 16 bytes
SLACK = 4 * 2.0 ** -24
WORST = {}                                                                  # what the tests print at the end of each: the worst ratio per section


# ---- 0. the launcher restated ----------------------------------------------------------------------------------------------------------------------
def decode_route(x, w, norm=None, check_ptr=True):
    """launch_decode_linear / dispatch_decode_linear (csrc/decode_step.hip) restated -> dict(vec_w, vec_x, rows, waves, kbatch, chunks).
    check_ptr=False (tensors built on the CPU, whose allocator is not the GPU's): a base counts as aligned when its storage offset is."""
    size = x.element_size()
    batch, K = x.shape
    N = w.shape[0]
    base = (lambda t: t.data_ptr() % 16 == 0) if check_ptr else (lambda t: (t.storage_offset() * size) % 16 == 0)
    rows = 4 if N >= 16384 else 1
    wave_rows = -(-N // rows)
    return dict(vec_w=base(w) and (N == 1 or (w.stride(0) * size) % 16 == 0),
                vec_x=norm is None and base(x) and (batch == 1 or (x.stride(0) * size) % 16 == 0),
                rows=rows, waves=1 if wave_rows <= 512 else (4 if batch <= 4 else 8),
                kbatch=next(v for v in (1, 2, 4, 8, 16) if batch <= v), chunks=-(-K // (256 * 16 // size)))


def on_route(x, w, norm=None, check_ptr=True, **want):
    got = decode_route(x, w, norm, check_ptr)
    assert {k: got[k] for k in want} == want, (got, want)


def waves_of(N, batch):
    return 1 if -(-N // (4 if N >= 16384 else 1)) <= 512 else (4 if batch <= 4 else 8)


def note(section, ratio):
    if ratio > WORST.get(section, 0.0):
        WORST[section] = ratio
        print(f"worst ratio so far, section {section}: {ratio:.3f}")


# ---- 1. the plain product: case builders (each yields dict(what, x, w, b, route); the CPU twin walks them too) -------------------------------------
def multi_chunk_cases(dtype):
    c = CH[dtype]
    for N, K, chunks in ((520, c + 8, 2), (520, 2 * c + 24, 3), (96, 2 * c, 2)):
        for batch in (1, 3, 16):
            x, w, b = linear_case(batch, N, K, dtype, seed=batch)
            yield dict(what=f"B{batch} N{N} K{K}", x=x, w=w, b=b, route=dict(vec_w=True, vec_x=True, chunks=chunks, waves=waves_of(N, batch), rows=1))


def element_tail_cases(dtype):
    K = CH[dtype] + 8 + 3
    for N in (96, 1):                                                       # an odd row stride: element by element, unless there is one row
        x, w, b = linear_case(1, N, K, dtype, seed=5)
        yield dict(what=f"B1 N{N} K{K}", x=x, w=w, b=b, route=dict(vec_w=N == 1, chunks=2, waves=1, kbatch=1))


def strided_x_cases(dtype):
    N, K = 96, CH[dtype] + 8
    for batch in (4, 16):
        _, w, b = linear_case(batch, N, K, dtype, seed=batch)
        x = rnd(batch, 2 * K, dtype=dtype, seed=batch + 7)[:, :K]           # as step_fused hands x_proj xz[:, :D]
        assert x.stride(0) != K
        yield dict(what=f"strided x B{batch}", x=x, w=w, b=b, route=dict(vec_w=True, vec_x=True, chunks=2, kbatch=batch))


def wide_rows_cases(dtype):
    N, K = 16390, CH[dtype] + 8
    for batch in (1, 16):
        x, w, b = linear_case(batch, N, K, dtype, seed=batch)
        yield dict(what=f"B{batch} N{N} K{K}", x=x, w=w, b=b, route=dict(vec_w=True, rows=4, chunks=2, waves=waves_of(N, batch), kbatch=batch))


def strided_weight_cases(dtype):
    N, K = 520, 264
    for batch, pad in itertools.product((1, 3, 16), (8, 3)):
        x, _, b = linear_case(batch, N, K, dtype, seed=batch)
        w = (rnd(N, K + pad, dtype=dtype, seed=batch + 1) * K ** -0.5)[:, :K]
        assert w.stride(0) == K + pad
        yield dict(what=f"W rows {K + pad} apart B{batch}", x=x, w=w, b=b, route=dict(vec_w=pad == 8, chunks=1, waves=waves_of(N, batch)))


def every_batch_cases(dtype):
    N, K = 520, CH[dtype] + 8
    x, w, b = linear_case(16, N, K, dtype, seed=9)
    for batch in range(1, 17):
        kbatch = 1 if batch == 1 else 2 if batch == 2 else 4 if batch <= 4 else 8 if batch <= 8 else 16
        yield dict(what=f"B{batch} N{N} K{K}", x=x[:batch], w=w, b=b, route=dict(vec_w=True, vec_x=True, chunks=2, kbatch=kbatch, waves=waves_of(N, batch)))


def grid_cases(dtype):
    """one (x, w, b) at N 16390 (four rows per wave), then its first n rows: one row per wave on 1 wave, and on 4 or 8 waves"""
    N, K = 16390, CH[dtype] + 8
    for batch in (3, 16):
        x, w, b = linear_case(batch, N, K, dtype, seed=batch + 20)
        yield dict(what=f"B{batch} full", x=x, w=w, b=b, route=dict(vec_w=True, rows=4, chunks=2))
        for n in (1, 512, 513, 16383):
            yield dict(what=f"B{batch} first {n} rows", x=x, w=w[:n], b=b[:n],
                       route=dict(vec_w=True, rows=1, chunks=2, waves=1 if n <= 512 else (4 if batch <= 4 else 8)))


PLAIN_BUILDERS = [multi_chunk_cases, element_tail_cases, strided_x_cases, wide_rows_cases, strided_weight_cases, every_batch_cases, grid_cases]


def run_plain(c):
    on_route(c["x"], c["w"], **c["route"])
    ys = [check_linear(c["x"], c["w"], bias, f"{c['what']} bias={bias is not None}") for bias in (None, c["b"])]
    return ys[1]


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("cases", [multi_chunk_cases, element_tail_cases, wide_rows_cases, strided_weight_cases], ids=lambda f: f.__name__)
def test_plain_product_against_float64(cases, dtype):
    for c in cases(dtype):
        run_plain(c)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_strided_x_over_two_chunks(dtype):
    """the vector staging of x' at k0 > 0 for a batch of rows whose stride is not K: float64, and bitwise the call on the copy"""
    for c in strided_x_cases(dtype):
        y = run_plain(c)
        assert torch.equal(y, check_linear(c["x"].contiguous(), c["w"], c["b"], "its copy"))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_every_batch_against_float64_and_its_rows_alone(dtype):
    """batches 1..16 (every batch tile, full and partly filled): float64, and row j bitwise the batch-1 call on row j"""
    from dimsum_amd import native
    cases = list(every_batch_cases(dtype))
    x, w, b = cases[-1]["x"], cases[-1]["w"], cases[-1]["b"]
    alone = torch.cat([native.decode_linear(x[j:j + 1], w, b) for j in range(16)])
    for c in cases:
        y = run_plain(c)
        assert torch.equal(y, alone[:y.shape[0]]), c["what"]


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_rows_do_not_depend_on_the_grid(dtype):
    """the same weight rows under four rows per wave, and under one row per wave on 1 wave and on 4 / 8 waves: bitwise equal. The per-lane FMA
    order and the cross-lane tree are functions of K alone."""
    from dimsum_amd import native
    full = None
    for c in grid_cases(dtype):
        on_route(c["x"], c["w"], **c["route"])
        y = native.decode_linear(c["x"], c["w"], c["b"])
        if c["route"]["rows"] == 4:
            full = y
        else:
            assert torch.equal(y, full[:, :y.shape[1]]), c["what"]


# ---- 2. the prologue -------------------------------------------------------------------------------------------------------------------------------
def prologue_inputs(dtype, res_dtype, B, N, K, seed=40):
    """x, w, b, a residual as the (B, 1, K)[:, 0] view the model holds, norm weight and bias with a clear dependence on k (a ramp plus noise:
    an index of chunk 0 used in chunk 1 cannot pass)"""
    x, w, b = linear_case(B, N, K, dtype, seed=seed)
    res = rnd(B, 1, K, dtype=res_dtype, seed=seed + 3)[:, 0]
    ramp = torch.linspace(0.0, 1.0, K, device=x.device)
    nw = (0.5 + ramp + 0.1 * rnd(K, seed=seed + 4)).to(dtype)
    nb = (0.5 - ramp + 0.1 * rnd(K, seed=seed + 5)).to(dtype)
    return x, w, b, res, nw, nb


def prologue_shapes(dtype):
    """(B, N, K, head form, route)"""
    return [(16, 1030, 200, False, dict(waves=8, kbatch=16, chunks=1, rows=1, vec_x=False)),     # two batch rows per wave, unequal lane trips
            (3, 1030, 40, False, dict(waves=4, kbatch=4, chunks=1, rows=1, vec_x=False)),        # wave 3 owns no batch row; 24 idle lanes
            (5, 300, CH[dtype] + 40, False, dict(waves=1, kbatch=8, chunks=2, rows=1, vec_x=False)),
            (2, 16390, 72, True, dict(waves=4, kbatch=2, chunks=1, rows=4, vec_x=False)),
            (16, 16390, 72, True, dict(waves=8, kbatch=16, chunks=1, rows=4, vec_x=False))]


def conditioning_inputs():
    """LayerNorm on rows of mean COND_MEAN and unit spread: a one-pass variance E[r^2] - mean^2 loses the spread in float32"""
    B, K, N = 4, 768, 64
    x, w, b = linear_case(B, N, K, torch.float32, seed=60)
    res = COND_MEAN + 0.25 * rnd(B, K, seed=63)
    nw, nb = 1 + 0.1 * rnd(K, seed=64), 0.1 * rnd(K, seed=65)
    return x, w, b, res, nw, nb


COND_MEAN = 64.0


def dbl(*ts):
    return [None if t is None else t.double() for t in ts]


def fused_within_twice_the_chain(pairs, what, section):
    """pairs: (name, fused, float64 reference, unfused chain)"""
    for name, got, ref, yard in pairs:
        e_fused, e_chain = (got.double() - ref).abs().max().item(), (yard.double() - ref).abs().max().item()
        bound = 2 * e_chain + SLACK * ref.abs().max().item()
        print(f"{what} {name}: fused err {e_fused:.3e}, unfused chain err {e_chain:.3e}, bound {bound:.3e}, ratio {e_fused / bound:.3f}")
        note(section, e_fused / bound)
        assert e_fused <= bound, (what, name)


def unfused_add_norm(x, nw, nb, res, rms):
    """the unfused chain's first launch -> (h, residual_out): layer_norm_fn. csrc/norm.hip serves rows of up to 2048 columns, and two chunks
    of 16-bit x' are more: there the yardstick is that launch's arithmetic in torch (the unrounded sum, float32 statistics in two passes,
    the output rounded to T) -- no less accurate than the kernel, so the bound it sets is no wider"""
    from dimsum_amd.ops.layernorm import layer_norm_fn
    K = x.shape[1]
    if K <= 2048:
        return layer_norm_fn(x, nw, nb, residual=res, eps=1e-5, prenorm=True, residual_in_fp32=res.dtype == torch.float32, is_rms_norm=rms)
    r = x.float() + res.float()
    if rms:
        h = r * torch.rsqrt(r.pow(2).mean(-1, keepdim=True) + 1e-5) * nw.float() + (0.0 if nb is None else nb.float())
    else:
        h = F.layer_norm(r, (K,), nw.float(), nb.float(), 1e-5)
    return h.to(x.dtype), r.to(res.dtype)


def check_prologue(x, w, b, res, nw, nb, rms, head, what):
    from dimsum_amd import native
    h, ro_chain = unfused_add_norm(x, nw, nb, res, rms)
    if head:
        y = native.decode_linear(x, w, b, norm=(nw, nb, 1e-5, rms), residual=res)
    else:
        y, ro = native.decode_linear(x, w, b, norm=(nw, nb, 1e-5, rms), residual=res, residual_out=res.dtype)
        # every element written (the buffer comes from torch.empty), by workgroup 0 alone: a single add in the residual's dtype
        assert ro.dtype == res.dtype and torch.equal(ro, x.to(res.dtype) + res) and torch.equal(ro, ro_chain), what
    assert y.dtype == x.dtype and y.shape == (x.shape[0], w.shape[0])
    x64, w64, b64, res64, nw64, nb64 = dbl(x, w, b, res, nw, nb)
    want = decode_linear_torch(x64, w64, b64, norm=(nw64, nb64, 1e-5, rms), residual=res64)
    fused_within_twice_the_chain([("y", y, want, F.linear(h, w, b))], what, "2")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("rms", [True, False], ids=["rms", "ln"])
@pytest.mark.parametrize("res32", [True, False], ids=["res32", "resT"])
def test_prologue_where_real_sizes_put_it(dtype, rms, res32, exact_fp32):  # noqa: F811
    res_dtype = torch.float32 if res32 else dtype
    for B, N, K, head, route in prologue_shapes(dtype):
        x, w, b, res, nw, nb = prologue_inputs(dtype, res_dtype, B, N, K)
        assert res.stride(0) == K and res._base is not None
        for bias in ((None, nb) if rms else (nb,)):                          # RMSNorm with a norm bias too: the kernel adds it
            on_route(x, w, norm=(nw, bias), **route)
            check_prologue(x, w, None if head else b, res, nw, bias, rms, head, f"B{B} N{N} K{K} norm bias={bias is not None}")


def test_layer_norm_statistics_on_rows_far_from_zero(exact_fp32):  # noqa: F811
    """the regression test of the corrected second pass (csrc/decode_step.hip, `corr`): with x' = (r - mean) * rstd alone this case stood at
    1.72 x its bound (fused 2.66e-5, chain 7.2e-6), the mean of the 768-term fp32 sum being off by more than an ulp of 64; now 0.37"""
    x, w, b, res, nw, nb = conditioning_inputs()
    on_route(x, w, norm=(nw, nb), waves=1, kbatch=4, chunks=1, rows=1)
    r = x + res
    print(f"row mean {r.mean().item():.2f}, spread {r.std().item():.3f}")
    check_prologue(x, w, b, res, nw, nb, False, False, f"LayerNorm on rows of mean {COND_MEAN}")


# ---- 3. the conv epilogue --------------------------------------------------------------------------------------------------------------------------
def conv_inputs(dtype, B, D, W, seed=70):
    """the taps, their bias and a contiguous state"""
    return rnd(D, W, dtype=dtype, seed=seed), rnd(D, dtype=dtype, seed=seed + 1), rnd(B, D, W, dtype=dtype, seed=seed + 2)


def state_layouts(st):
    """-> [(name, the (B, D, W) view holding st's values, its whole buffer, the mask of the buffer's elements outside the view)]"""
    B, D, W = st.shape
    cache = rnd(B + 2, D, W, dtype=st.dtype, seed=90)
    cache[:B] = st
    m1 = torch.ones_like(cache, dtype=torch.bool)
    m1[:B] = False
    bwd = st.transpose(1, 2).contiguous()                                   # (B, W, D)
    padded = rnd(B, D, W + 1, dtype=st.dtype, seed=91)
    padded[:, :, :W] = st
    m3 = torch.zeros_like(padded, dtype=torch.bool)
    m3[:, :, W] = True
    return [("cache[:B]", cache[:B], cache, m1), ("(B, W, D) transposed", bwd.transpose(1, 2), bwd, torch.zeros_like(bwd, dtype=torch.bool)),
            ("(B, D, W + 1)[:, :, :W]", padded[:, :, :W], padded, m3)]


def check_epilogue(x, w, b, res, nw, nb, rms, st, cw, cb, silu, what, buffer=None, outside=None):
    """st: the (B, D, W) state view the launch updates in place"""
    from dimsum_amd import native
    from dimsum_amd.ops import causal_conv1d_update
    from dimsum_amd.ops.layernorm import layer_norm_fn
    D = cw.shape[0]
    res32 = res.dtype == torch.float32
    st0 = st.clone()
    before = None if buffer is None else buffer.clone()
    s_chain = st0.contiguous().clone()
    y, ro = native.decode_linear(x, w, b, norm=(nw, nb, 1e-5, rms), residual=res, residual_out=res.dtype, conv=(st, cw, cb, silu))
    pre = native.decode_linear(x, w, b, norm=(nw, nb, 1e-5, rms), residual=res)             # the same launch without the epilogue
    assert torch.equal(ro, x.to(res.dtype) + res), what
    assert torch.equal(st, torch.cat([st0[:, :, 1:], pre[:, :D, None]], dim=2)), what        # the roll, then the stored pre-activation value
    assert torch.equal(y[:, D:], pre[:, D:]), what
    if buffer is not None:
        assert torch.equal(buffer[outside], before[outside]), what                          # nothing outside the (b < B, n < D, w < W) view
    h, ro_chain = layer_norm_fn(x, nw, nb, residual=res, eps=1e-5, prenorm=True, residual_in_fp32=res32, is_rms_norm=rms)
    xz = F.linear(h, w, b)
    chain = torch.cat([causal_conv1d_update(xz[:, :D], s_chain, cw.contiguous(), cb, "silu" if silu else None), xz[:, D:]], 1)
    assert torch.equal(ro_chain, ro)
    x64, w64, b64, res64, nw64, nb64, cw64, cb64 = dbl(x, w, b, res, nw, nb, cw, cb)
    s64 = st0.double()
    want = decode_linear_torch(x64, w64, b64, norm=(nw64, nb64, 1e-5, rms), residual=res64, conv=(s64, cw64, cb64, silu))
    want_pre = decode_linear_torch(x64, w64, b64, norm=(nw64, nb64, 1e-5, rms), residual=res64)
    fused_within_twice_the_chain([("y", y, want, chain), ("pre-activation", pre, want_pre, xz),
                                  ("state", st[:, :, -1], s64[:, :, -1], s_chain[:, :, -1])], what, "3")


def epilogue_operands(dtype, rms, B, N=1030, K=200):
    """section 2's prologue at (B, N, K): RMSNorm on a float32 residual stream, LayerNorm on one of T"""
    x, w, b, res, nw, nb = prologue_inputs(dtype, torch.float32 if rms else dtype, B, N, K)
    return x, w, b, res, nw, None if rms else nb


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("rms", [True, False], ids=["rms", "ln"])
def test_epilogue_widths_activation_and_bias(dtype, rms, exact_fp32):  # noqa: F811
    """D 517: no multiple of 4, 8 or 64 -- conv rows and plain rows share a workgroup of 8 waves"""
    B, D = 16, 517
    ops = epilogue_operands(dtype, rms, B)
    on_route(ops[0], ops[1], norm=ops[4:], waves=8, kbatch=16, rows=1)
    for W, silu, has_cb in itertools.product((2, 3, 4), (True, False), (True, False)):
        cw, cb, st = conv_inputs(dtype, B, D, W)
        check_epilogue(*ops, rms, st, cw, cb if has_cb else None, silu, f"W{W} silu={silu} conv bias={has_cb}")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_epilogue_on_four_waves_and_on_the_batch_tile_of_eight(dtype, exact_fp32):  # noqa: F811
    for B, route in ((3, dict(waves=4, kbatch=4)), (7, dict(waves=8, kbatch=8))):
        ops = epilogue_operands(dtype, True, B)
        on_route(ops[0], ops[1], norm=ops[4:], **route)
        cw, cb, st = conv_inputs(dtype, B, 517, 4)
        check_epilogue(*ops, True, st, cw, cb, True, f"B{B} W4")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_epilogue_on_strided_states_and_taps(dtype, exact_fp32):  # noqa: F811
    B, D = 16, 517
    ops = epilogue_operands(dtype, True, B)
    for W in (2, 4):
        cw, cb, st = conv_inputs(dtype, B, D, W)
        for name, view, buffer, outside in state_layouts(st):
            assert view.shape == st.shape and torch.equal(view, st)
            check_epilogue(*ops, True, view, cw, cb, True, f"W{W} state {name}", buffer, outside)
        taps = cw.t().contiguous().t()                                      # a (W, D) buffer transposed: the width stride is D
        assert taps.stride() == (1, D) and torch.equal(taps, cw)
        check_epilogue(*ops, True, st, taps, cb, True, f"W{W} taps (W, D) transposed")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_epilogue_under_four_rows_per_wave(dtype, exact_fp32):  # noqa: F811
    """conv_dim inside a wave's four rows (16386 = 4 * 4096 + 2; 6 = 4 + 2); at batch 16 all 64 lanes of a wave end with a value"""
    N, K = 16390, 72
    for B, D in itertools.product((2, 16), (16386, 6)):
        assert D % 4 != 0
        ops = epilogue_operands(dtype, True, B, N, K)
        on_route(ops[0], ops[1], norm=ops[4:], rows=4, kbatch=B, waves=waves_of(N, B))
        cw, cb, st = conv_inputs(dtype, B, D, 4)
        check_epilogue(*ops, True, st, cw, cb, True, f"B{B} N{N} D{D}")


# ---- 4. the model ----------------------------------------------------------------------------------------------------------------------------------
LM_PATHS = dict(d_model=576, n_layer=1, vocab_size=16390, pad_vocab_size_multiple=1)       # d_inner 1152, dt_rank 36
LM_PROMPT, LM_STEPS = 5, 4


def paths_model():
    torch.manual_seed(0)
    m = tiny_model(1, 1, **LM_PATHS)
    assert m.config["ssm_cfg"] == LM_TINY["ssm_cfg"] and m.backbone.layers[0].mixer.d_inner == 1152 and m.backbone.layers[0].mixer.dt_rank == 36
    return m


def paths_tokens(batch=16):
    g = torch.Generator().manual_seed(1)
    return (torch.randint(0, LM_PATHS["vocab_size"], (batch, LM_PROMPT), generator=g),
            torch.randint(0, LM_PATHS["vocab_size"], (batch, LM_STEPS + 1), generator=g))


def reference_step_logits(m, prompt, teacher):
    """the step logits of `m`'s weights in float64 on the CPU: every token, the prompt's included, walks the recurrent form from zero states
    through `step_fused` on the torch restatements test_lm_cpu.py's `lm_backend` installs (decode_linear_torch and native_state_update compute
    in the precision of their operands) -> (B, LM_STEPS, V)"""
    from dimsum_amd import gemm, native
    m64 = copy.deepcopy(m).cpu().double()
    bb, (layer,) = m64.backbone, m64.backbone.layers
    B = prompt.shape[0]
    conv_state = torch.zeros(B, layer.mixer.d_inner, layer.mixer.d_conv, dtype=torch.float64)
    ssm_state = torch.zeros(B, layer.mixer.d_inner, layer.mixer.d_state, dtype=torch.float64)
    tokens = torch.cat([prompt, teacher[:, :LM_STEPS]], 1)
    nf = bb.norm_f
    out = []
    with torch.no_grad(), pytest.MonkeyPatch.context() as mp:
        mp.setattr(native, "decode_linear", decode_linear_torch)
        mp.setattr(native, "selective_state_update", native_state_update)
        mp.setattr(gemm, "neg_exp", lambda a_log: -torch.exp(a_log))
        for t in range(tokens.shape[1]):
            hidden, residual = layer.mixer.step_fused(bb.embedding(tokens[:, t]), None, layer.norm, torch.float64, conv_state, ssm_state)
            out.append(decode_linear_torch(hidden, m64.lm_head.weight, None, norm=(nf.weight, nf.bias, nf.eps, True), residual=residual))
    return torch.stack(out[LM_PROMPT:], 1)


@functools.lru_cache(maxsize=None)
def paths_reference():
    """model, tokens and the float64 step logits at batch 16, computed once; a smaller batch is its first rows"""
    m = paths_model()
    prompt, teacher = paths_tokens()
    return m, prompt, teacher, reference_step_logits(m, prompt, teacher)


def spied_routes(m, prompt, teacher):
    """run_cached with native.decode_linear spied -> (its returns, the routes of the decode_linear calls of the first step)"""
    from dimsum_amd import native
    routes = []
    with pytest.MonkeyPatch.context() as mp:
        fn = native.decode_linear

        def spy(x, w, bias=None, norm=None, residual=None, residual_out=None, conv=None):
            routes.append(dict(decode_route(x, w, norm), n=w.shape[0], k=w.shape[1], prologue=norm is not None, epilogue=conv is not None,
                               x_stride=x.stride(0)))
            return fn(x, w, bias, norm=norm, residual=residual, residual_out=residual_out, conv=conv)

        mp.setattr(native, "decode_linear", spy)
        outs = run_cached(m, prompt, LM_STEPS, teacher=teacher)
    return outs, routes


@pytest.mark.parametrize("batch", [2, 16])
def test_model_steps_on_the_real_size_leaves_against_float64(batch, exact_fp32, monkeypatch):  # noqa: F811
    m, prompt, teacher, ref = paths_reference()
    m = copy.deepcopy(m).to("cuda")
    prompt, teacher, ref = prompt[:batch].to("cuda"), teacher[:batch].to("cuda"), ref[:batch].to("cuda")
    monkeypatch.setenv("DIMSUM_FUSED_DECODE", "1")
    (_, fused, _), routes = spied_routes(m, prompt, teacher)
    assert len(routes) == 4 * LM_STEPS
    in_proj, x_proj, out_proj, head = routes[:4]
    many = 4 if batch <= 4 else 8
    assert in_proj["n"] == 2304 and in_proj["prologue"] and in_proj["epilogue"] and in_proj["waves"] == many and in_proj["vec_w"]
    assert (x_proj["n"], x_proj["k"]) == (68, 1152) and x_proj["chunks"] == 2 and x_proj["vec_w"] and x_proj["vec_x"] and x_proj["x_stride"] == 2304
    assert (out_proj["n"], out_proj["k"]) == (576, 1152) and out_proj["chunks"] == 2 and out_proj["vec_w"] and out_proj["waves"] == many
    assert head["n"] == 16390 and head["rows"] == 4 and head["prologue"] and not head["epilogue"] and head["kbatch"] == batch
    monkeypatch.setenv("DIMSUM_FUSED_DECODE", "0")
    (_, unfused, _), routes = spied_routes(m, prompt, teacher)
    assert routes == []
    e_fused, e_unfused = (fused.double() - ref).abs().max().item(), (unfused.double() - ref).abs().max().item()
    bound = 2 * e_unfused + SLACK * ref.abs().max().item()
    print(f"batch {batch}: fused err {e_fused:.3e}, unfused err {e_unfused:.3e}, max|ref| {ref.abs().max().item():.3e}, bound {bound:.3e}, "
          f"ratio {e_fused / bound:.3f}")
    note("4", e_fused / bound)
    assert e_fused <= bound


def test_model_in_bf16_takes_the_fused_path_on_those_leaves(monkeypatch):
    m, prompt, teacher, _ = paths_reference()
    m = copy.deepcopy(m).to("cuda").to(torch.bfloat16)
    prompt, teacher = prompt[:2].to("cuda"), teacher[:2].to("cuda")
    outs = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("DIMSUM_FUSED_DECODE", fused)
        outs[fused], routes = spied_routes(m, prompt, teacher)
        assert len(routes) == (5 * LM_STEPS if fused == "1" else 0)           # dt_proj: its own GEMV in 16 bits
        assert outs[fused][1].dtype == torch.bfloat16
    assert torch.equal(outs["1"][0], outs["0"][0])                             # the prompt takes one path
    close(outs["1"][1], outs["0"][1], SSU_TOL[torch.bfloat16], "fused vs unfused bf16 steps")


def test_generate_at_batch_16_from_a_captured_graph_equals_eager(exact_fp32, monkeypatch):  # noqa: F811
    m, prompt, _, _ = paths_reference()
    m = copy.deepcopy(m).to("cuda")
    prompt = prompt.to("cuda")
    monkeypatch.setenv("DIMSUM_FUSED_DECODE", "1")
    L = LM_PROMPT + LM_STEPS + 1
    eager = m.generate(prompt, max_length=L, return_dict_in_generate=True, output_scores=True)
    cg = m.generate(prompt, max_length=L, return_dict_in_generate=True, output_scores=True, cg=True)
    assert torch.equal(cg.sequences, eager.sequences) and len(cg.scores) == len(eager.scores) == LM_STEPS + 1
    for a, b in zip(cg.scores, eager.scores):
        assert torch.equal(a, b)
    assert list(m._decoding_cache.callables) == [(16, 1)]
