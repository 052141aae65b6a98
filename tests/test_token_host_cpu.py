"""Host side of the token passes (csrc/token_transform.hip, ops/token_ops.py) and of the gated-GeLU row passes (csrc/act_rows.hip), CPU-only.

(a) The plain torch expressions of the transforms in ops/token_ops.py (haar_dwt_tokens, dct_tokens, ...) are the reference the GPU tests of
    the token passes use (tests/test_token_paths_gpu.py evaluates them in float64). Here they are pinned themselves: against the reference's
    goldens haar.npz / dct.npz with the keys and tolerances tests/test_oracle_golden.py uses for the numpy oracle, against the numpy oracle
    on random input, and against the adjoint identities the module's docstring builds the backward passes on (T^t = T^-1 / 16 for Haar, an
    orthonormal T for the DCT), in float64 to 1e-12.

(b) The status of every refusal dimsum_token_transform and the six dimsum_gated_gelu_* entry points can give before a kernel is launched.
    Every pointer is a made-up, suitably aligned address that is never read: each case is refused (a status that is neither DIMSUM_OK nor
    DIMSUM_ERR_LAUNCH) or has batch == 0 / rows == 0 and returns DIMSUM_OK in front of the launch, so nothing is launched. A condition joined
    by `||` (or the conjunction `vec`, whose negation is one) has one case per disjunct where the disjunct can be the only fault.
    `return` lines and disjuncts without a case of their own:
      * every `return launch_status()` (DIMSUM_ERR_LAUNCH): a kernel has to go out first;
      * `(wdot_ptr || wsum_ptr) && !w_ptr` without y and tsum: the "nothing to produce" line in front refuses it (same status); the cases
        below give y as well;
      * the two `if (p.y_split3 == 2) return DIMSUM_ERR_STRIDE` of launch_tt<1>: the entry point refuses a scaled-fp16 image without the
        16-byte layout first (same status);
      * the scaled-fp16 image's `w_ptr` alone: w needs wdot or wsum with it to get past the NULL checks (the case gives wdot);
      * the Haar LDS bound's largest SERVED channel count (2408 = the smallest refused multiple of four - 4) launches a kernel, which made-up
        addresses must never reach: it runs on real tensors in tests/test_token_paths_gpu.py::test_haar_at_the_lds_bound.
    The statuses were read from the library and checked against the entry points' text; none looked wrong."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import assert_close, golden
from dimsum_amd import _lib
from dimsum_amd.ops import token_ops as to
from oracle import np_ops

OK, NULL, DTYPE, SHAPE, STRIDE, UNSUPPORTED, LAUNCH, ABI = range(8)
NONE, HAAR_FWD, HAAR_INV, DCT_FWD, DCT_INV = range(5)


# ---- (a) the plain expressions ------------------------------------------------------------------------------------------------------------
def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def test_haar_expressions_vs_golden():
    g = golden("haar")
    for H in (16, 32, 4):
        assert_close(to.haar_dwt_tokens(_t64(g[f"H{H}_x"])).numpy(), g[f"H{H}_dwt"], 1e-5, 1e-6, f"dwt H{H}")
        assert_close(to.haar_idwt_tokens(_t64(g[f"H{H}_y2"])).numpy(), g[f"H{H}_idwt"], 1e-5, 1e-6, f"idwt H{H}")
        assert_close(to.haar_idwt_tokens(to.haar_dwt_tokens(_t64(g[f"H{H}_x"]))).numpy(), g[f"H{H}_x"], 1e-5, 1e-6, "roundtrip")
        # the reference's autograd results: dwt^T = idwt / 16, idwt^T = 16 dwt
        assert_close(to.haar_idwt_tokens(_t64(g[f"H{H}_dwt_g"])).numpy() / 16.0, g[f"H{H}_dwt_dx"], 1e-5, 1e-6, "dwt grad")
        assert_close(to.haar_dwt_tokens(_t64(g[f"H{H}_idwt_g"])).numpy() * 16.0, g[f"H{H}_idwt_dy"], 1e-5, 1e-6, "idwt grad")


def test_dct_expressions_vs_golden():
    g = golden("dct")
    for H in (16, 32):
        assert_close(to.dct_tokens(_t64(g[f"H{H}_x"])).numpy(), g[f"H{H}_dct"], 1e-5, 2e-6, f"dct H{H}")
        assert_close(to.idct_tokens(_t64(g[f"H{H}_dct"])).numpy(), g[f"H{H}_roundtrip"], 1e-5, 2e-6, f"idct H{H}")
    assert_close(to.dct_matrix("cpu", torch.float64).reshape(16, 1, 4, 4).numpy(), g["dct_weight_1ch"], 0, 1e-7, "basis")


def test_expressions_vs_numpy_oracle():
    """(2, 64, 6) random float64: the Haar pair is exact in both (1e-12); the oracle's DCT keeps the reference's float32 basis and returns
    float32, so it gets the goldens' tolerance"""
    x = np.random.RandomState(0).standard_normal((2, 64, 6))
    assert_close(to.haar_dwt_tokens(_t64(x)).numpy(), np_ops.haar_dwt_tokens(x), 1e-12, 1e-12, "dwt")
    assert_close(to.haar_idwt_tokens(_t64(x)).numpy(), np_ops.haar_idwt_tokens(x), 1e-12, 1e-12, "idwt")
    assert_close(to.dct_tokens(_t64(x)).numpy(), np_ops.dct_tokens(x), 1e-5, 2e-6, "dct")
    assert_close(to.idct_tokens(_t64(x)).numpy(), np_ops.idct_tokens(x), 1e-5, 2e-6, "idct")


def _matrix(fn, L, Cn):
    """the (L Cn, L Cn) matrix of a linear token operator: column i = fn(unit vector i)"""
    n = L * Cn
    return fn(torch.eye(n, dtype=torch.float64).reshape(n, L, Cn)).reshape(n, n).t()


@pytest.mark.parametrize("L,Cn", [(16, 2), (64, 3)])
def test_adjoint_identities(L, Cn):
    """token_ops' docstring: T T^t = I / 16 and T^t = T^-1 / 16 (Haar), T orthonormal (DCT) -- what makes the adjoint of each fused pass the
    other pass with a rescaled gate (_ADJ). float64, 1e-12."""
    eye = np.eye(L * Cn)
    T, Ti = _matrix(to.haar_dwt_tokens, L, Cn).numpy(), _matrix(to.haar_idwt_tokens, L, Cn).numpy()
    assert_close(T @ Ti, eye, 0, 1e-12, "haar: T T^-1")
    assert_close(T @ T.T, eye / 16.0, 0, 1e-12, "haar: T T^t = I / 16")
    assert_close(T.T, Ti * to._ADJ["haar"], 0, 1e-12, "haar: T^t = T^-1 / 16")
    D, Di = _matrix(to.dct_tokens, L, Cn).numpy(), _matrix(to.idct_tokens, L, Cn).numpy()
    assert_close(D @ D.T, eye, 0, 1e-12, "dct: orthonormal")
    assert_close(D.T, Di * to._ADJ["dct"], 0, 1e-12, "dct: T^t = T^-1")
    assert to._ADJ["none"] == 1.0
    # the same through inner products on random vectors: <T x, y> = <x, T^t y>
    rs = np.random.RandomState(L)
    x, y = _t64(rs.standard_normal((2, L, Cn))), _t64(rs.standard_normal((2, L, Cn)))
    assert abs(((to.haar_dwt_tokens(x) * y).sum() - (x * to.haar_idwt_tokens(y)).sum() / 16.0).item()) <= 1e-12 * L * Cn
    assert abs(((to.dct_tokens(x) * y).sum() - (x * to.idct_tokens(y)).sum()).item()) <= 1e-12 * L * Cn


# ---- (b) refusals of dimsum_token_transform -----------------------------------------------------------------------------------------------
def _addr(i):
    return 0x10000000 + 0x100000 * i                 # 1-MB aligned, distinct, never dereferenced


X, Y, GATE, SCALE, SHIFT, RES, W, WDOT, WSUM, TSUM, INV, IN_IDX, OUT_IDX = (_addr(i) for i in range(13))
# the served base call: (2, 64, 8) fp32, contiguous, y only; the overlays add operands with a layout that is served as well
TT = dict(batch=2, tokens=64, channels=8, grid=8, kind=NONE, x_batch_stride=512, x_token_stride=8, y_batch_stride=512, y_token_stride=8,
          red_batch_stride=8, x_ptr=X, y_ptr=Y)
MODS = dict(mod_batch_stride=8, gate_ptr=GATE, scale_ptr=SCALE, shift_ptr=SHIFT)
RESID = dict(residual_ptr=RES, res_batch_stride=512, res_token_stride=8)
WRED = dict(w_ptr=W, w_batch_stride=512, w_token_stride=8, wdot_ptr=WDOT)
IMG3 = dict(y_split3=1, y_batch_stride=64 * 24, y_token_stride=24)              # [hi | hi | lo] bf16 rows
PAIR = dict(y_split3=3, y_batch_stride=64 * 16, y_token_stride=16)              # [hi | lo]
F16S = dict(y_split3=2, y_inv_scale_ptr=INV)                                    # fp16 rows of C elements + (batch, tokens) inverse scales
TT_OVERLAYS = {"MODS": MODS, "RESID": RESID, "WRED": WRED, "IMG3": IMG3, "PAIR": PAIR, "F16S": F16S}

# every conjunct of `vec` (the 16-byte layout) broken alone: refused wherever an image output needs vec
_NOT_VEC = [
    ((), {"channels": 6, "x_token_stride": 8}), ((), {"x_ptr": X + 4}), ((), {"y_ptr": Y + 8}), ((), {"x_batch_stride": 514}), ((), {"x_token_stride": 10}),
    ((), {"y_batch_stride": 64 * 24 + 2}), ((), {"y_token_stride": 26}),
    (("MODS",), {"mod_batch_stride": 10}), (("MODS",), {"gate_ptr": GATE + 4}), (("MODS",), {"scale_ptr": SCALE + 8}), (("MODS",), {"shift_ptr": SHIFT + 12}),
    (("RESID",), {"residual_ptr": RES + 4}), (("RESID",), {"res_batch_stride": 514}), (("RESID",), {"res_token_stride": 9}),
    (("WRED",), {"w_ptr": W + 4}), (("WRED",), {"w_batch_stride": 514}), (("WRED",), {"w_token_stride": 9}),
]

# (overlays on TT, the one change, status)
TT_CASES = (
    [((), m, s) for m, s in [
        ({"null": 1}, NULL), ({"struct_size": 0}, ABI), ({"struct_size": C.sizeof(_lib.TtParams) + 8}, ABI), ({"x_ptr": None}, NULL),
        # nothing to produce: no y, no tsum, no (w with wdot or wsum)
        ({"y_ptr": None}, NULL), ({"y_ptr": None, "w_ptr": W}, NULL), ({"y_ptr": None, "wdot_ptr": WDOT}, NULL), ({"y_ptr": None, "wsum_ptr": WSUM}, NULL),
        # a reduction against w without w
        ({"wdot_ptr": WDOT}, NULL), ({"wsum_ptr": WSUM}, NULL), ({"y_ptr": None, "tsum_ptr": TSUM, "wdot_ptr": WDOT}, NULL),
        ({"batch": -1}, SHAPE), ({"tokens": 0}, SHAPE), ({"tokens": -64}, SHAPE), ({"channels": 0}, SHAPE), ({"channels": -8}, SHAPE),
        ({"kind": HAAR_FWD, "grid": 6, "tokens": 36}, SHAPE), ({"kind": DCT_INV, "grid": 8, "tokens": 60}, SHAPE), ({"kind": HAAR_INV, "grid": 0}, SHAPE),
        # the order of the checks: NULL, then SHAPE, then the batch == 0 return, then the image layout
        ({"x_ptr": None, "tokens": 0}, NULL), ({"struct_size": 0, "x_ptr": None}, ABI), ({"batch": 0, "tokens": 0}, SHAPE),
        ({"batch": 0, "kind": DCT_FWD, "grid": 6}, SHAPE),
        # launch_tt, in front of any launch: an unknown kind on each of its switches (run-time form, kFix form, scalar family) ...
        ({"kind": 5}, SHAPE), ({"kind": -1}, SHAPE), ({"kind": 5, "x_ptr": X + 4}, SHAPE),
        # ... and the Haar image's LDS bound (68 dwords per 4 channels <= 160 KB): 2412 is the smallest refused multiple of four, 2409 the
        # smallest refused channel count of the scalar family (603 groups of four either way; 2408 is served: see the module docstring)
        ({"kind": HAAR_FWD, "channels": 2412, "x_token_stride": 2412, "y_token_stride": 2412, "x_batch_stride": 64 * 2412, "y_batch_stride": 64 * 2412}, SHAPE),
        ({"kind": HAAR_INV, "channels": 2412, "x_token_stride": 2412, "y_token_stride": 2412, "x_batch_stride": 64 * 2412, "y_batch_stride": 64 * 2412}, SHAPE),
        ({"kind": HAAR_FWD, "channels": 2409, "x_token_stride": 2409, "y_token_stride": 2409, "x_batch_stride": 64 * 2409, "y_batch_stride": 64 * 2409}, SHAPE),
    ]]
    + [(("MODS",), {"kind": 5, "gate_ptr": None}, SHAPE)]                                    # unknown kind on the kFix switch (scale + shift: kFix 1)
    + [(("WRED", "MODS"), {"kind": 7, "gate_ptr": None, "shift_ptr": None}, SHAPE)]           # ... (scale + w: kFix 3)
    + [(("F16S",), m, s) for m, s in [
        ({"y_ptr": None, "tsum_ptr": TSUM}, NULL), ({"y_inv_scale_ptr": None}, NULL),
        ({"y_token_stride": 4}, STRIDE), ({"channels": 2052, "x_token_stride": 2052, "y_token_stride": 2052}, STRIDE),
        ({"kind": HAAR_FWD, "channels": 1028, "x_token_stride": 1028, "y_token_stride": 1028}, STRIDE),
        ({"kind": DCT_INV, "channels": 1028, "x_token_stride": 1028, "y_token_stride": 1028}, STRIDE),
        ({"tsum_ptr": TSUM}, STRIDE), ({"kind": 5}, SHAPE), ({"y_inv_scale_ptr": None, "channels": 6}, NULL),
    ]]
    + [(("F16S", "WRED"), {}, STRIDE)]
    + [(("F16S",) + ov, {k: (v if k != "y_batch_stride" else 514) for k, v in m.items()}, STRIDE) for ov, m in _NOT_VEC if "y_token_stride" not in m and "WRED" not in ov]
    + [(("F16S",), {"y_token_stride": 10}, STRIDE)]
    + [(("IMG3",) + ov, m, STRIDE) for ov, m in _NOT_VEC]
    + [(("IMG3",), m, s) for m, s in [({"y_ptr": None, "tsum_ptr": TSUM}, STRIDE), ({"y_token_stride": 20}, STRIDE), ({"y_token_stride": 16}, STRIDE), ({"kind": 5}, SHAPE)]]
    + [(("PAIR",), m, s) for m, s in [({"y_token_stride": 12}, STRIDE), ({"x_ptr": X + 4}, STRIDE), ({"channels": 6}, STRIDE), ({"y_ptr": None, "tsum_ptr": TSUM}, STRIDE)]]
)

# batch == 0 returns DIMSUM_OK in front of the layout checks and of launch_tt: even an image without the 16-byte layout, an unknown kind, a
# Haar image beyond the LDS bound
TT_EMPTY = [((), {}), (("MODS", "RESID"), {}), (("WRED",), {"tsum_ptr": TSUM}), (("IMG3",), {"x_ptr": X + 4}), (("F16S",), {"channels": 6}), ((), {"kind": 5}),
            ((), {"kind": HAAR_FWD, "channels": 2412})]


def _tt_status(overlays, mut, **extra):
    fields = dict(TT)
    for name in overlays:
        fields.update(TT_OVERLAYS[name])
    fields.update(mut)
    fields.update(extra)
    P = _lib.TtParams()
    for key, val in fields.items():
        if key != "null":
            setattr(P, key, val)
    return _lib.load().dimsum_token_transform(None if fields.get("null") else P, None)


def _tt_id(case):
    return "+".join(("tt",) + case[0]) + ":" + ",".join(f"{k}={v}" for k, v in case[1].items())


@pytest.mark.parametrize("case", TT_CASES, ids=_tt_id)
def test_token_transform_refusals(case):
    overlays, mut, want = case
    assert want not in (OK, LAUNCH)                  # a refusal: nothing is launched
    assert _tt_status(overlays, mut) == want


@pytest.mark.parametrize("case", TT_EMPTY, ids=_tt_id)
def test_token_transform_empty_batch_is_ok(case):
    assert _tt_status(case[0], case[1], batch=0) == OK


def test_token_transform_cases_break_a_base_that_passes_the_checks():
    """every overlay combination the refusals start from gets past all checks with batch == 0 -- and so does every refused case that is
    not refused in front of the batch == 0 return, which shows the refusal is due to the one change and comes from behind that line"""
    seen = {c[0] for c in TT_CASES}
    for overlays in seen:
        assert _tt_status(overlays, {}, batch=0) == OK, overlays
    behind = [c for c in TT_CASES if c[2] == STRIDE or ("kind" in c[1] and c[1]["kind"] in (5, 7, -1)) or c[1].get("channels") in (2409, 2412)]
    assert len(behind) > 40
    for overlays, mut, _ in behind:
        assert _tt_status(overlays, mut, batch=0) == OK, (overlays, mut)


# ---- (b) refusals of the gated-GeLU entry points ------------------------------------------------------------------------------------------
X12, BIAS, H_OUT, DH, DX12, DBIAS, INV_S = (_addr(20 + i) for i in range(7))
BIG_ROWS = 1 << 42                                   # x hidden / 4 pieces / 1024 per workgroup: 2^32 workgroups > 2^31 - 1
BIG_CHUNKS = 65536 * 64                              # 65536 chunks of 64 rows: one more than the backward's grid.y takes
GG_FWD = ("dimsum_gated_gelu_fwd", "dimsum_gated_gelu_fwd_split3")
GG_BWD = ("dimsum_gated_gelu_bwd", "dimsum_gated_gelu_bwd_split3", "dimsum_gated_gelu_bwd_pair")
_GG_SHAPE = [({"rows": -1}, SHAPE), ({"hidden": 0}, SHAPE), ({"hidden": -8}, SHAPE), ({"hidden": 10}, SHAPE)]
GG_BASE = dict(x12=X12, bias=BIAS, h=H_OUT, dh=DH, dx12=DX12, inv=INV_S, dbias=DBIAS, rows=64, hidden=8)
GG_ARGS = {**{n: ("x12", "bias", "h") for n in GG_FWD}, **{n: ("x12", "bias", "dh", "dx12", "dbias") for n in GG_BWD},
           "dimsum_gated_gelu_bwd_f16s": ("x12", "bias", "dh", "dx12", "inv", "dbias")}
GG_CASES = (
    [(n, m, s) for n in GG_FWD for m, s in _GG_SHAPE + [
        ({"x12": None}, NULL), ({"h": None}, NULL), ({"x12": X12 + 8}, STRIDE), ({"h": H_OUT + 4}, STRIDE), ({"bias": BIAS + 8}, STRIDE),
        ({"rows": BIG_ROWS, "hidden": 4}, SHAPE),
        ({"x12": None, "hidden": 0}, NULL), ({"hidden": 10, "h": H_OUT + 4}, SHAPE), ({"rows": 0, "h": H_OUT + 4}, STRIDE), ({"rows": 0, "hidden": 10}, SHAPE)]]
    + [(n, m, s) for n in GG_BWD for m, s in _GG_SHAPE + [
        ({"x12": None}, NULL), ({"dh": None}, NULL), ({"dx12": None}, NULL),
        ({"x12": X12 + 8}, STRIDE), ({"dh": DH + 4}, STRIDE), ({"dx12": DX12 + 8}, STRIDE), ({"bias": BIAS + 8}, STRIDE),
        ({"rows": BIG_CHUNKS}, SHAPE),
        ({"dh": None, "rows": -1}, NULL), ({"hidden": 10, "dh": DH + 4}, SHAPE), ({"rows": 0, "dx12": DX12 + 8}, STRIDE), ({"rows": 0, "hidden": 10}, SHAPE)]]
    + [("dimsum_gated_gelu_bwd_f16s", m, s) for m, s in _GG_SHAPE + [
        ({"x12": None}, NULL), ({"dh": None}, NULL), ({"dx12": None}, NULL), ({"inv": None}, NULL), ({"hidden": 5124}, SHAPE),
        ({"x12": X12 + 8}, STRIDE), ({"dh": DH + 8}, STRIDE), ({"dx12": DX12 + 4}, STRIDE), ({"bias": BIAS + 8}, STRIDE),
        ({"inv": None, "hidden": 5124}, NULL), ({"hidden": 5124, "x12": X12 + 8}, SHAPE), ({"rows": 0, "dx12": DX12 + 4}, STRIDE), ({"rows": 0, "hidden": 5124}, SHAPE)]]
)
# rows == 0 returns DIMSUM_OK behind the checks: the optional operands absent, the widest row the image pass takes, its 8-byte image rows
GG_EMPTY = ([(n, m) for n in GG_FWD + GG_BWD for m in ({}, {"bias": None}, {"hidden": 1 << 20})]
            + [(n, {"dbias": None}) for n in GG_BWD]
            + [("dimsum_gated_gelu_bwd_f16s", m) for m in ({}, {"bias": None, "dbias": None}, {"hidden": 5120}, {"dx12": DX12 + 8})])


def _gg_status(name, mut, **extra):
    f = {**GG_BASE, **mut, **extra}
    return getattr(_lib.load(), name)(*[f[a] for a in GG_ARGS[name]], f["rows"], f["hidden"], None)


def _gg_id(case):
    return case[0].replace("dimsum_gated_gelu_", "") + ":" + ",".join(f"{k}={v}" for k, v in case[1].items())


@pytest.mark.parametrize("case", GG_CASES, ids=_gg_id)
def test_gated_gelu_refusals(case):
    name, mut, want = case
    assert want not in (OK, LAUNCH)
    assert _gg_status(name, mut) == want


@pytest.mark.parametrize("case", GG_EMPTY, ids=_gg_id)
def test_gated_gelu_no_rows_is_ok(case):
    assert _gg_status(case[0], case[1], rows=0) == OK
