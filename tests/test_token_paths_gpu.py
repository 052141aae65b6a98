"""The token-pass kernels (csrc/token_transform.hip) on the leaves of launch_tt's dispatch the older unit tests do not reach: the scalar family
(VEC == 1), token_rows_kernel<4 | 8, *> and its lane guard / fall-through / row grid stride, the token tail of kind `none`, the multi-group
walk and the nsub == 4 / nsub == 1 forms of the reduction passes, the second trip of the channel loop, _PreMixerFork's adjoint with the
tail gradient as `residual`, and the run-time-presence instantiations (DIMSUM_TT_FIX=0).

Reference: ONE helper, `reference`, in float64 on the CPU -- gather by in_index, gate, the plain expression of the transform from
ops/token_ops.py (pinned against the reference's goldens in tests/test_token_host_cpu.py), modulate, scatter by out_index, add the residual;
wdot / wsum / tsum are float64 sums of the same float64 T(.).
Tolerances (|err| <= rtol |ref| + scale_atol max|ref|), the project's own for these passes: forward tensors 1e-5 / 1e-6 (2e-6 for dct),
backward tensors 2e-5 / 2e-6, per-(batch, channel) reductions 1e-4 / 1e-5. Pure moves are compared with torch.equal, operand images bit for
bit with the stand-alone converter applied to the same call's fp32 output.

There is no kernel-selection query: the comment on each case names the leaf of launch_tt it reaches and the rule that sends it there, read
from launch_tt and from the head of token_transform_kernel:
  vec    = C % 4 == 0 and every base pointer / stride a multiple of 16 bytes                              -> launch_tt<4>, else launch_tt<1>
  rows   = kind none, y, no w, no tsum, C <= 2048, vec            -> token_rows_kernel<2 (C <= 512) | 4 (C <= 1024) | 8, 0 fp32 | 1 split | 2 f16s>
  f16s   = otherwise, y_split3 == 2 (blocked kinds only, see below)  -> token_transform_kernel<K, 4, true, 1 pre | 2 post | 0>
  kFix   = otherwise, vec: 1 scale + shift | 2 gate + residual (blocked kinds, y only); 3 scale + w + y | 4 w, no y | 5 scale + w + tsum + y
           (no shift / gate / residual)                               -> token_transform_kernel<K, 4, false, kFix>; DIMSUM_TT_FIX=0 turns all of them off
  else                                                                -> token_transform_kernel<K, VEC> (run-time operand presence)
  blocked kinds run a 64 / 128 / 256-thread block for <= 64 / <= 128 / more channel groups (C / VEC); the channel loop makes a second trip
  when there are more groups than threads. Kind none: nsub = 4 / 2 / 1 for <= 64 / <= 128 / more groups; nsub > 1 takes the sub-path (the
  16 tokens split over idle threads), nsub == 1 the channel loop. With reductions gx = ceil(L / 16) is halved while even and
  (gx / 2) * B >= 1024 (512 without y): a workgroup then walks several 16-token groups and flushes its sums once.
(token_transform_kernel<NONE, 4, true, *> is instantiated but unreachable: a scaled-fp16 image takes no reductions and at most 2048 channels
for kind none, which is exactly the row kernel's domain. The f16s epilogue's token-tail guard therefore cannot fire.)"""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from conftest import assert_close

pytestmark = pytest.mark.gpu

FWD = {"none": (1e-5, 1e-6), "haar": (1e-5, 1e-6), "dct": (1e-5, 2e-6)}
BWD = (2e-5, 2e-6)
RED = (1e-4, 1e-5)
KINDS = [("none", True), ("haar", True), ("haar", False), ("dct", True), ("dct", False)]
BLOCKED = KINDS[1:]


def _plain(kind, forward):
    from dimsum_amd.ops import token_ops as to
    return {("haar", True): to.haar_dwt_tokens, ("haar", False): to.haar_idwt_tokens, ("dct", True): to.dct_tokens, ("dct", False): to.idct_tokens}[(kind, forward)]


def _d(t):
    return None if t is None else t.detach().double().cpu()


def reference(x, kind, forward, in_index=None, out_index=None, gate=None, scale=None, shift=None, residual=None, w=None):
    """the pass in float64 on the CPU -> dict(y, tsum[, wdot, wsum])"""
    x, gate, scale, shift, residual, w = (_d(t) for t in (x, gate, scale, shift, residual, w))
    v = x if in_index is None else x[:, in_index.long().cpu()]
    if gate is not None:
        v = v * gate[:, None]
    t = v if kind == "none" else _plain(kind, forward)(v)
    o = t
    if scale is not None:
        o = o * (1 + scale[:, None])
    if shift is not None:
        o = o + shift[:, None]
    y, idx = o, None
    if out_index is not None:
        idx = out_index.long().cpu()
        y = torch.empty_like(o)
        y[:, idx] = o
    if residual is not None:
        y = y + residual
    out = {"y": y, "tsum": t.sum(1)}
    if w is not None:
        wg = w if idx is None else w[:, idx]
        out["wdot"], out["wsum"] = (t * wg).sum(1), wg.sum(1)
    return out


def _close(got, want, tol, what):
    assert_close(got.detach().double().cpu().numpy(), want.numpy(), tol[0], 0, what, scale_atol=tol[1])


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _operands(B, L, C, seed, off=0):
    """x and the residual as channel slices of ONE wider tensor (x `off` floats into it), gate / scale / shift as slices of one (B, 3C)
    tensor, w dense, a random permutation"""
    g = _gen(seed)
    wide = torch.randn(B, L, 2 * C + 4 * off, device="cuda", generator=g)
    mods = 0.5 * torch.randn(B, 3 * C, device="cuda", generator=g)
    w = torch.randn(B, L, C, device="cuda", generator=g)
    perm = torch.randperm(L, device="cuda", generator=g).to(torch.int32)
    return types.SimpleNamespace(x=wide[:, :, off:off + C], res=wide[:, :, C + off:2 * C + off], gate=mods[:, :C], scale=mods[:, C:2 * C], shift=mods[:, 2 * C:],
                                 w=w, perm=perm)


def _forms(o):
    return {"pre": dict(out_index=o.perm, scale=o.scale, shift=o.shift), "post": dict(in_index=o.perm, gate=o.gate, residual=o.res),
            "mixed": dict(out_index=o.perm, scale=o.scale)}


def _bits(t):
    return t.contiguous().view(torch.int16)


def _check_images(x, kind, forward, kw, y, modes):
    """the image outputs of the call that gave the fp32 y, bit for bit against the converters on y"""
    from dimsum_amd import native
    B, L, C = y.shape
    rows = y.reshape(B * L, C)
    if "split3" in modes:
        y3 = native.token_transform(x, kind, forward, split3=True, **kw)
        assert y3.dtype == torch.bfloat16 and tuple(y3.shape) == (B, L, 3 * C)
        assert torch.equal(_bits(y3.reshape(B * L, -1)), _bits(native.split3_rows(rows, left=True))), "split3"
    if "pair" in modes:
        yp = native.token_transform(x, kind, forward, split3="pair", **kw)
        assert isinstance(yp, native.PairImage) and tuple(yp.data.shape) == (B, L, 2 * C)
        assert torch.equal(_bits(yp.data.reshape(B * L, -1)), _bits(native.split3_rows(rows, "pair").data)), "pair"
    if "f16s" in modes:
        yi = native.token_transform(x, kind, forward, split3="f16s", **kw)
        want = native.rows_f16s(rows)
        assert torch.equal(_bits(yi.data.reshape(B * L, C)), _bits(want.data)), "f16s data"
        assert torch.equal(yi.inv.reshape(-1), want.inv), "f16s inv"


# ---- the scalar family (VEC == 1) ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [
    "pre",      # out_index + scale + shift: store_out's scalar modulate and scattered store
    "post",     # in_index + gate + residual (a slice of the wide tensor): load_in's scalar gather and gate, store_out's residual load
])
@pytest.mark.parametrize("kind,forward", [
    ("none", True),     # token_transform_kernel<NONE, 1>: vec false; nsub > 1 and C % 1 == 0 -> the sub-path with one channel per thread
    ("haar", True),     # <HAAR_FWD, 1>: vec false; scalar LDS image writes and the scalar phase 2 read haar_lds(c * 16 + k)
    ("haar", False),    # <HAAR_INV, 1>: vec false; scalar phase 1 writes haar_lds((c + 0) * 16 + k), scalar reads of the 16 bands
    ("dct", True),      # <DCT_FWD, 1>: vec false; one channel per thread through dct16
    ("dct", False),     # <DCT_INV, 1>: vec false
])
@pytest.mark.parametrize("C,off", [
    (6, 0),     # C % 4 != 0 -> launch_tt<1>; 6 groups: 64-thread block with 6 busy lanes (blocked), nsub 4 with 24 busy threads (none)
    (66, 0),    # C % 4 != 0 -> launch_tt<1>; 66 groups: 128-thread block, second wave 2 lanes busy (blocked), nsub 2 (none)
    (8, 1),     # C % 4 == 0 but x = wide[:, :, 1:9]: base 4 bytes past a 16-byte boundary -> vec false -> launch_tt<1>
])
def test_scalar_family(C, off, kind, forward, form):
    from dimsum_amd import native
    o = _operands(2, 64, C, 100 * C + off)
    kw = _forms(o)[form]
    y = native.token_transform(o.x, kind, forward, **kw)
    _close(y, reference(o.x, kind, forward, **kw)["y"], FWD[kind], f"{kind} {form}")


def test_scalar_reductions_and_tail():
    """<NONE, 1> (C = 6: vec false), L = 50: four 16-token groups, the last with 2 live tokens (load_in / store_out return on pos_of(k) >= tokens),
    with w, wsum and tsum: the scalar flush_red; gx = 4 (2 * 2 workgroups are far below 1024)"""
    from dimsum_amd import native
    o = _operands(2, 50, 6, 7)
    kw = dict(out_index=o.perm, scale=o.scale, w=o.w)
    y, wdot, wsum, tsum = native.token_transform(o.x, "none", True, want_wsum=True, want_tsum=True, **kw)
    ref = reference(o.x, "none", True, **kw)
    _close(y, ref["y"], FWD["none"], "y")
    for name, got in (("wdot", wdot), ("wsum", wsum), ("tsum", tsum)):
        _close(got, ref[name], RED, name)


def test_scalar_haar_reduction_without_y():
    """<HAAR_FWD, 1> (C = 6) with w and want_y=False: phase 2 reads the scalar LDS image only to reduce it against w"""
    from dimsum_amd import native
    o = _operands(2, 64, 6, 8)
    y, wdot, wsum = native.token_transform(o.x, "haar", True, out_index=o.perm, w=o.w, want_y=False)
    assert y is None and wsum is None
    _close(wdot, reference(o.x, "haar", True, out_index=o.perm, w=o.w)["wdot"], RED, "wdot")


@pytest.mark.parametrize("mode,width", [(True, 3), ("pair", 2)])
def test_image_of_a_misaligned_slice_is_refused(mode, width):
    """the split-bf16 images need the 16-byte layout: on x = wide[:, :, 1:9] the entry point returns DIMSUM_ERR_STRIDE in front of
    launch_tt (the wrapper raises) and the image buffer stays as it was"""
    from dimsum_amd import _lib, native
    o = _operands(2, 64, 8, 9, off=1)
    with pytest.raises(RuntimeError):
        native.token_transform(o.x, "haar", True, scale=o.scale, shift=o.shift, split3=mode)
    img = torch.full((2, 64, width * 8), 7.0, device="cuda", dtype=torch.bfloat16)
    P = _lib.TtParams()
    P.batch, P.tokens, P.channels, P.grid, P.kind, P.y_split3 = 2, 64, 8, 8, 1, 1 if mode is True else 3
    P.x_batch_stride, P.x_token_stride, P.y_batch_stride, P.y_token_stride = o.x.stride(0), o.x.stride(1), img.stride(0), img.stride(1)
    P.x_ptr, P.y_ptr = o.x.data_ptr(), img.data_ptr()
    assert _lib.load().dimsum_token_transform(P, torch.cuda.current_stream().cuda_stream) == 4          # DIMSUM_ERR_STRIDE
    torch.cuda.synchronize()
    assert (img == 7.0).all()


# ---- token_rows_kernel ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [
    508,    # token_rows_kernel<2, *>: C <= 512; the second piece's last lane has c = 508 >= C: the lane guard on loads and stores
    512,    # <2, *>: C <= 512, both pieces full
    516,    # <4, *>: 512 < C <= 1024; the third piece has one busy lane, the fourth none
    1020,   # <4, *>: the fourth piece's last lane idle
    1024,   # <4, *>: C <= 1024, all pieces full
    1028,   # <8, *>: 1024 < C <= 2048; pieces 6..8 all idle, piece 5 one lane
    2044,   # <8, *>: the eighth piece's last lane idle
    2048,   # <8, *>: C <= 2048, all pieces full
    2052,   # channels > 2048: falls through to token_transform_kernel<NONE, 4> (no kFix for kind none without w), nsub 1, three c trips
])
def test_row_kernel(C):
    """kind none, no reductions, all four modulators as slices of wider tensors, a random permutation on the input side in one call and on
    the output side in the next; fp32 against float64, the three images against the converters"""
    from dimsum_amd import native
    o = _operands(2, 24, C, C)
    for side in ("in_index", "out_index"):
        kw = {side: o.perm, "gate": o.gate, "scale": o.scale, "shift": o.shift, "residual": o.res}
        y = native.token_transform(o.x, "none", True, **kw)
        _close(y, reference(o.x, "none", True, **kw)["y"], FWD["none"], f"C={C} {side}")
        _check_images(o.x, "none", True, kw, y, ("split3", "pair", "f16s") if C <= 2048 else ("split3", "pair"))
        if C > 2048:
            with pytest.raises(RuntimeError):                      # the wrapper refuses the scaled-fp16 image beyond the row kernel's width
                native.token_transform(o.x, "none", True, split3="f16s", **kw)


def test_row_kernel_grid_stride():
    """token_rows_kernel<2, 0>: B * L = 17920 rows > 4 * 4096 workgroups' worth: the first 1536 waves take a second row; pure moves"""
    from dimsum_amd import native
    g = _gen(3)
    x = torch.randn(70, 256, 8, device="cuda", generator=g)
    perm = torch.randperm(256, device="cuda", generator=g).to(torch.int32)
    assert torch.equal(native.token_transform(x, "none", True, in_index=perm), x[:, perm.long()])
    want = torch.empty_like(x)
    want[:, perm.long()] = x
    assert torch.equal(native.token_transform(x, "none", True, out_index=perm), want)
    assert torch.equal(native.token_transform(native.token_transform(x, "none", True, out_index=perm), "none", False, in_index=perm), x)


@pytest.mark.parametrize("C", [
    40,     # token_rows_kernel<2, 2>
    516,    # <4, 2>: idle lanes contribute 0 to the row maximum
    1028,   # <8, 2>
])
def test_row_kernel_f16s_zero_row_and_outlier(C):
    from dimsum_amd import native
    from test_f16s_gpu import _expected_image
    g = _gen(C)
    x = torch.randn(2, 24, C, device="cuda", generator=g) * torch.logspace(-20, 20, 24, device="cuda")[None, :, None]
    x[0, 3] = 0.0
    x[1, 5, C - 1] = 1e4 * x[1, 5].abs().max()
    gate = torch.randn(2, C, device="cuda", generator=g)
    perm = torch.randperm(24, device="cuda", generator=g).to(torch.int32)
    y = native.token_transform(x, "none", True, out_index=perm, gate=gate)
    img = native.token_transform(x, "none", True, out_index=perm, gate=gate, split3="f16s")
    want, inv = _expected_image(y)
    assert torch.equal(_bits(img.data), _bits(want)) and torch.equal(img.inv, inv)
    assert torch.isfinite(img.data).all() and torch.isfinite(img.inv).all()
    assert (y[0, perm[3].item()] == 0).all() and (img.data[0, perm[3].item()] == 0).all()
    top = img.data.float().abs().amax(-1)
    assert ((top >= 2.0 ** 14) & (top < 2.0 ** 15))[y.abs().amax(-1) > 0].all()


# ---- the token tail of kind none -----------------------------------------------------------------------------------------------------------
TAIL_L = [1, 15, 17, 50]        # one group with 1 / 15 live tokens, two with 1 in the second, four with 2 in the last


@pytest.mark.parametrize("L", TAIL_L)
def test_tail_without_reductions(L):
    """C = 40, fp32 and f16s: kind none without reductions is token_rows_kernel<2, 0 | 2> whatever L (one wave per row of B * L rows, no
    16-token groups): its tail is the last workgroup's waves past the last row"""
    from dimsum_amd import native
    o = _operands(3, L, 40, L)
    for kw in (_forms(o)["pre"], _forms(o)["post"]):
        y = native.token_transform(o.x, "none", True, **kw)
        assert tuple(y.shape) == (3, L, 40)
        _close(y, reference(o.x, "none", True, **kw)["y"], FWD["none"], f"L={L}")
        _check_images(o.x, "none", True, kw, y, ("f16s",))


def _run_form(form, x, kind, forward, scale, w, out_index):
    """the reduction passes as the model issues them (3, 4, 5: kFix of that number) and the two run-time forms -> (got, reference)"""
    from dimsum_amd import native
    tt = native.token_transform
    got = {}
    if form == "3":            # scale + w -> y, wdot
        got["y"], got["wdot"], none = tt(x, kind, forward, out_index=out_index, scale=scale, w=w)
        assert none is None
    elif form == "4":          # w only, no y, wsum
        none, got["wdot"], got["wsum"] = tt(x, kind, forward, out_index=out_index, w=w, want_y=False, want_wsum=True)
        assert none is None
    elif form == "5":          # scale + w + tsum -> y, wdot, tsum
        got["y"], got["wdot"], none, got["tsum"] = tt(x, kind, forward, out_index=out_index, scale=scale, w=w, want_tsum=True)
        assert none is None
    elif form == "a":          # tsum only (kFix 0: no w)
        y, wdot, wsum, got["tsum"] = tt(x, kind, forward, out_index=out_index, want_y=False, want_tsum=True)
        assert y is None and wdot is None and wsum is None
    else:                      # "b": scale + w + tsum without y (kFix 0: none of 3, 4, 5)
        y, got["wdot"], wsum, got["tsum"] = tt(x, kind, forward, out_index=out_index, scale=scale, w=w, want_y=False, want_tsum=True)
        assert y is None and wsum is None
    return got


def _check_form(got, ref, kind, what):
    for name, t in got.items():
        assert torch.isfinite(t).all(), f"{what}: {name} not finite"
        _close(t, ref[name], BWD if name == "y" else RED, f"{what}: {name}")


@pytest.mark.parametrize("form", [
    "5",    # scale + w + tsum + y: kFix 5
    "4",    # w, want_y=False, wsum: kFix 4 (store_out returns after the sums)
])
@pytest.mark.parametrize("C", [
    40,     # token_transform_kernel<NONE, 4, false, kFix>: 10 groups -> nsub 4, the sub-path (4 tokens per thread)
    512,    # 128 groups -> nsub 2 (8 tokens per thread)
    1152,   # 288 groups -> nsub 1: the channel loop, second trip for c >= 1024
])
@pytest.mark.parametrize("L", TAIL_L)
def test_tail_with_reductions(L, C, form):
    """load_in returns zeros and store_out returns for pos_of(k) >= tokens: nothing past L enters y or a sum. The second call reads x and w as
    the leading L tokens of longer NaN-filled buffers (same token stride): a read past `tokens` would put a NaN into a sum."""
    o = _operands(3, L, C, 10 * L + C)
    ref = reference(o.x, "none", True, out_index=o.perm, scale=o.scale, w=o.w)
    _check_form(_run_form(form, o.x, "none", True, o.scale, o.w, o.perm), ref, "none", f"L={L} C={C} form {form}")
    xl, wl = (torch.full((3, L + 16, t.shape[2]), float("nan"), device="cuda") for t in (o.x, o.w))
    xl[:, :L], wl[:, :L] = o.x, o.w
    assert xl[:, :L].stride(1) == o.w.stride(1)
    _check_form(_run_form(form, xl[:, :L], "none", True, o.scale, wl[:, :L], o.perm), ref, "none", f"L={L} C={C} form {form}, NaN beyond the tail")


# ---- reduction passes of kind none: nsub, second trip, several groups per workgroup --------------------------------------------------------
ALL_FORMS = [
    "3",    # scale + w: token_transform_kernel<NONE, 4, false, 3>
    "4",    # w only, want_y=False, want_wsum: <NONE, 4, false, 4>
    "5",    # scale + w + want_tsum: <NONE, 4, false, 5>
    "a",    # want_tsum only, no y: no w -> kFix 0: <NONE, 4> with has_* read from the pointers
    "b",    # scale + w + want_tsum, want_y=False: w without y but with scale -> none of 3 / 4 / 5 -> kFix 0
]


@pytest.mark.parametrize("form", ALL_FORMS)
@pytest.mark.parametrize("C", [
    64,     # 16 channel groups -> nsub 4: 64 busy threads, 4 tokens each
    256,    # 64 groups -> nsub 4, all 256 threads busy
    512,    # 128 groups -> nsub 2, 8 tokens per thread
    516,    # 129 groups -> nsub 1: the channel loop, one trip, threads 129.. idle
    1152,   # 288 groups -> nsub 1: the second trip (c = 1024 + 4 tid for 32 threads) after flush_red(c) reset the first trip's sums
])
def test_reduction_forms(C, form):
    """B = 3, L = 64: gx = 4 workgroups per batch element (no halving: 2 * 3 < 512), each flushes once per channel and trip"""
    o = _operands(3, 64, C, C + 1)
    ref = reference(o.x, "none", True, out_index=o.perm, scale=o.scale, w=o.w)
    _check_form(_run_form(form, o.x, "none", True, o.scale, o.w, o.perm), ref, "none", f"C={C} form {form}")


@pytest.mark.parametrize("B,L,C,form", [
    (256, 64, 8, "4"),      # no y: min 512 workgroups; gx 4 -> 2 (2 * 256 >= 512), not 1 (256 < 512): sub-path, 2 groups per workgroup
    (256, 64, 8, "a"),      # the same walk on the run-time form (kFix 0)
    (512, 64, 8, "3"),      # y: min 1024; gx 4 -> 2 (2 * 512 >= 1024), not 1 (512 < 1024): the walk with the y stores
    (512, 64, 8, "5"),      # the same with the token sums
    (512, 64, 8, "4"),      # no y: gx 4 -> 2 -> 1 (1 * 512 >= 512): ONE workgroup per batch element walks all 4 groups
    (512, 64, 8, "b"),      # the same on the run-time form
    (512, 96, 8, "3"),      # y: gx 6 -> 3 (3 * 512 >= 1024), then 3 is odd: the halving stops; groups grp and grp + 3
    (512, 96, 8, "5"),      # the same with the token sums
    (512, 96, 8, "4"),      # no y: gx 6 -> 3, odd
    (512, 24, 516, "4"),    # nsub 1 (129 channel groups): gx 2 -> 1: the CHANNEL LOOP's walk over the further groups; group 1 has 8 live tokens
    (512, 24, 516, "a"),    # the same on the run-time form
    (1024, 24, 516, "5"),   # y: gx 2 -> 1 (1 * 1024 >= 1024): the channel loop's walk with the y stores and the tail
])
def test_reduction_multi_group(B, L, C, form):
    """a workgroup walks several 16-token groups and flushes once. Run twice into fresh buffers: both runs meet the tolerance (the sums are
    atomic adds over the workgroups of a batch element: the two runs need not agree bit for bit)"""
    g = _gen(B + L + C)
    x, w = torch.randn(B, L, C, device="cuda", generator=g), torch.randn(B, L, C, device="cuda", generator=g)
    scale = 0.5 * torch.randn(B, C, device="cuda", generator=g)
    perm = torch.randperm(L, device="cuda", generator=g).to(torch.int32)
    ref = reference(x, "none", True, out_index=perm, scale=scale, w=w)
    for run in (0, 1):
        _check_form(_run_form(form, x, "none", True, scale, w, perm), ref, "none", f"({B}, {L}, {C}) form {form} run {run}")


# ---- blocked kinds beyond one trip of the channel loop ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [
    "pre",      # scale + shift: token_transform_kernel<K, 4, false, 1>
    "post",     # gate + residual: <K, 4, false, 2>
])
@pytest.mark.parametrize("kind,forward", BLOCKED)
@pytest.mark.parametrize("C", [
    1028,   # 257 channel groups on a 256-thread block: thread 0 alone makes the second trip (phase 1, the transform and phase 2 for Haar)
    1152,   # 288 groups: 32 threads make the second trip (the DiT-XL width)
])
def test_blocked_second_trip(C, kind, forward, form):
    from dimsum_amd import native
    o = _operands(2, 64, C, C + 7)
    kw = _forms(o)[form]
    y = native.token_transform(o.x, kind, forward, **kw)
    _close(y, reference(o.x, kind, forward, **kw)["y"], FWD[kind], f"{kind} {form} C={C}")


@pytest.mark.parametrize("form", [
    "3",    # token_transform_kernel<HAAR_*, 4, false, 3>: flush_red(c) after each trip's 16 stores
    "4",    # <HAAR_*, 4, false, 4>
    "5",    # <HAAR_*, 4, false, 5>
])
@pytest.mark.parametrize("forward", [True, False])
def test_blocked_second_trip_reductions(forward, form):
    """C = 1152 (two trips), haar: the sums of the second trip's channels must not carry the first trip's"""
    o = _operands(2, 64, 1152, 11)
    ref = reference(o.x, "haar", forward, out_index=o.perm, scale=o.scale, w=o.w)
    _check_form(_run_form(form, o.x, "haar", forward, o.scale, o.w, o.perm), ref, "haar", f"haar fwd={forward} form {form}")


@pytest.mark.parametrize("form", [
    "pre",      # token_transform_kernel<K, 4, true, 1>
    "post",     # <K, 4, true, 2>
    "mixed",    # scale only: neither pre nor post -> <K, 4, true, 0>
])
@pytest.mark.parametrize("kind,forward", BLOCKED)
def test_blocked_f16s_partly_idle_wave(kind, forward, form):
    """C = 260: 65 channel groups -> a 128-thread block whose second wave has ONE busy lane: the idle lanes' row maxima (0) and the `c < C`
    guard of the image store. fp32 against float64, the image against the converter on the fp32 output"""
    from dimsum_amd import native
    o = _operands(2, 64, 260, 260)
    kw = _forms(o)[form]
    y = native.token_transform(o.x, kind, forward, **kw)
    _close(y, reference(o.x, kind, forward, **kw)["y"], FWD[kind], f"{kind} {form}")
    _check_images(o.x, kind, forward, kw, y, ("f16s",))


@pytest.mark.parametrize("forward", [True, False])
def test_haar_at_the_lds_bound(forward):
    """C = 2408: 602 channel groups x 68 dwords = 163744 bytes of LDS, the most launch_tt serves (2412 is refused: tests/test_token_host_cpu.py);
    token_transform_kernel<HAAR_*, 4> on a 256-thread block, three trips"""
    from dimsum_amd import native
    x = torch.randn(1, 16, 2408, device="cuda", generator=_gen(2408))
    _close(native.token_transform(x, "haar", forward), reference(x, "haar", forward)["y"], FWD["haar"], "haar C=2408")


# ---- pre_mixer_fork ------------------------------------------------------------------------------------------------------------------------
def _fork_case(kind, C, H):
    g = _gen(C + H + len(kind))
    B, L = 2, H * H
    rn = lambda *s: torch.randn(s, device="cuda", generator=g)
    inv32 = torch.randperm(L, device="cuda", generator=g).to(torch.int32)
    return types.SimpleNamespace(x=rn(B, L, C), mods=0.5 * rn(B, 2 * C), g=rn(B, L, C), dy1=rn(B, L, C), dy2=rn(B, L, C), inv32=inv32,
                                 fwd=torch.argsort(inv32.long().cpu()))


def _fork_reference(c, kind, use):
    """float64 autograd through the plain expression: t = modulate(P(T(x))), loss = <t, dy1> + <x g, dy2> -> (t, dx, dshift, dscale)"""
    from dimsum_amd.ops import token_ops as to
    x, mods = _d(c.x).requires_grad_(), _d(c.mods).requires_grad_()
    shift, scale = mods.chunk(2, dim=1)
    t = to.modulate((x if kind == "none" else _plain(kind, True)(x)).index_select(1, c.fwd), shift, scale)
    loss = 0.0
    if use != "tail":
        loss = loss + (t * _d(c.dy1)).sum()
    if use != "t":
        loss = loss + (x * _d(c.g) * _d(c.dy2)).sum()
    loss.backward()
    dm = torch.zeros_like(mods) if mods.grad is None else mods.grad
    C = c.x.shape[2]
    return t.detach(), x.grad, dm[:, :C], dm[:, C:]


@pytest.mark.parametrize("use", [
    "both",     # dy and dtail: the adjoint pass adds the tail gradient as its residual
    "tail",     # only the second output is used (autograd hands the pass a zero dy): dx must be the tail gradient, d shift = d scale = 0
    "t",        # only t is used (a zero tail gradient as the residual)
])
@pytest.mark.parametrize("C,H", [
    (64, 8),    # 16 channel groups: 64-thread block (blocked kinds); none: token_rows_kernel<2, 0> for dx, nsub 4 for the sums
    (516, 8),   # 129 groups: 256-thread block with 127 idle threads; none: token_rows_kernel<4, 0>, nsub 1
])
@pytest.mark.parametrize("kind", [
    "haar",     # dx: token_transform_kernel<HAAR_INV, 4, false, 2> (gate + residual on the forward kind's inverse); sums: <HAAR_FWD, 4, false, 4>
    "dct",      # dx: <DCT_INV, 4, false, 2>; sums: <DCT_FWD, 4, false, 4>
    "none",     # dx: the row kernel with gate + residual; sums: <NONE, 4, false, 4>
])
def test_pre_mixer_fork(kind, C, H, use):
    from dimsum_amd.ops import token_ops as to
    c = _fork_case(kind, C, H)
    x, mods = c.x.clone().requires_grad_(), c.mods.clone().requires_grad_()
    shift, scale = mods.chunk(2, dim=1)
    t, x2 = to.pre_mixer_fork(x, kind, {"inv32": c.inv32}, shift, scale)
    assert torch.equal(x2, x)
    loss = 0.0
    if use != "tail":
        loss = loss + (t * c.dy1).sum()
    if use != "t":
        loss = loss + (x2 * c.g * c.dy2).sum()
    loss.backward()
    rt, rdx, rdshift, rdscale = _fork_reference(c, kind, use)
    dm = torch.zeros_like(mods) if mods.grad is None else mods.grad
    _close(t, rt, FWD[kind], "t")
    _close(x.grad, rdx, BWD, "dx")
    _close(dm[:, :C], rdshift, RED, "d shift")
    _close(dm[:, C:], rdscale, RED, "d scale")


@pytest.mark.parametrize("kind", ["haar", "dct", "none"])
def test_pre_mixer_fork_absent_gradients(kind):
    """_PreMixerFork.backward with a gradient that is None (an engine that does not materialise zeros): dy None -> the tail gradient itself
    and no modulation gradients; dtail None -> the adjoint without a residual (gate only: no kFix -> token_transform_kernel<K_INV, 4>, the
    row kernel for kind none)"""
    from dimsum_amd.ops import token_ops as to
    C = 64
    c = _fork_case(kind, C, 8)
    shift, scale = c.mods[:, :C], c.mods[:, C:]
    ctx = types.SimpleNamespace(kind=kind, inv32=c.inv32, saved_tensors=(c.x, scale), needs_input_grad=(True, True, True, False, False))
    dtail = c.g * c.dy2
    out = to._PreMixerFork.backward(ctx, None, dtail)
    assert out[0] is dtail and all(o is None for o in out[1:])
    dx, dshift, dscale, *rest = to._PreMixerFork.backward(ctx, c.dy1, None)
    assert all(o is None for o in rest)
    _, rdx, rdshift, rdscale = _fork_reference(c, kind, "t")
    _close(dx, rdx, BWD, "dx")
    _close(dshift, rdshift, RED, "d shift")
    _close(dscale, rdscale, RED, "d scale")


# ---- DIMSUM_TT_FIX=0: the run-time-presence instantiations ------------------------------------------------------------------------------------
FIX_SHAPES = [(2, 64, 40), (2, 64, 516)]      # 10 channel groups (64-thread block, nsub 4) and 129 (256-thread block, nsub 1)


def _fix_calls():
    """pre- and post-form of none / haar / dct as fp32 and as the scaled-fp16 image, and the reduction forms 3 / 4 / 5 of none and haar, from
    a fixed seed -> {name: CPU tensor}. With DIMSUM_TT_FIX=0 every blocked call and every reduction pass lands on a kFix-0 instantiation
    (token_transform_kernel<K, 4, false | true, 0>); kind none without reductions is the row kernel either way."""
    from dimsum_amd import native
    out = {}
    for B, L, C in FIX_SHAPES:
        o = _operands(B, L, C, 4000 + C)
        for kind in ("none", "haar", "dct"):
            for form, forward in (("pre", True), ("post", False)):
                kw = _forms(o)[form]
                y = native.token_transform(o.x, kind, forward, **kw)
                img = native.token_transform(o.x, kind, forward, split3="f16s", **kw)
                want = native.rows_f16s(y.reshape(B * L, C))
                key = f"{kind}/{form}/{C}"
                out[key + "/y"], out[key + "/img"], out[key + "/inv"] = y.cpu(), img.data.cpu(), img.inv.cpu()
                out[key + "/img_is_image_of_y"] = torch.tensor(bool(torch.equal(_bits(img.data.reshape(B * L, C)), _bits(want.data)) and torch.equal(img.inv.reshape(-1), want.inv)))
            if kind != "dct":
                for form in ("3", "4", "5"):
                    for name, t in _run_form(form, o.x, kind, True, o.scale, o.w, o.perm).items():
                        out[f"{kind}/form{form}/{C}/{name}"] = t.cpu()
    return out


def test_run_time_presence_instantiations(tmp_path):
    """one fresh child process with DIMSUM_TT_FIX=0 (the switch is read once per process) runs _fix_calls; this process runs the same calls
    on the kFix instantiations. none and haar: torch.equal (their bodies hold nothing the compiler can contract differently: adds, and
    multiplies by powers of two; load_in / store_out have contraction off); dct: the forward tolerance, and each process's image is the image
    of its own fp32 output. The reductions of both processes against float64."""
    path = str(tmp_path / "fix0.pt")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env={**os.environ, "DIMSUM_TT_FIX": "0"}, timeout=120,
                       capture_output=True, text=True)
    assert r.returncode == 0, f"the DIMSUM_TT_FIX=0 child exited with {r.returncode}:\n{r.stderr[-4000:]}"
    child = torch.load(path)
    mine = _fix_calls()
    assert set(child) == set(mine) and len(mine) == 2 * (3 * 2 * 4 + 2 * 7)
    refs = {}
    for key, got in mine.items():
        kind, form, C, name = key.split("/")
        if form.startswith("form"):
            if (kind, C) not in refs:
                o = _operands(*next(s for s in FIX_SHAPES if s[2] == int(C)), 4000 + int(C))
                refs[(kind, C)] = reference(o.x, kind, True, out_index=o.perm, scale=o.scale, w=o.w)
            for t in (got, child[key]):
                _close(t, refs[(kind, C)][name], BWD if name == "y" else RED, key)
            if name == "y":
                assert torch.equal(got, child[key]), key
        elif name == "img_is_image_of_y":
            assert bool(got) and bool(child[key]), key
        elif kind == "dct":
            if name == "y":
                _close(child[key], got.double(), FWD["dct"], key)
        else:
            assert torch.equal(got, child[key]), key


if __name__ == "__main__":          # the child of test_run_time_presence_instantiations
    assert os.environ.get("DIMSUM_TT_FIX") == "0"
    torch.save(_fix_calls(), sys.argv[1])
