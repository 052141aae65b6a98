"""Characterisation of the GEMM host layer (csrc/gemm_nt.hip): the status code of every refusal the entry points dimsum_gemm_nt (asked through
dimsum_gemm_nt_kernel_for, which runs the same checks, launches nothing and returns the negated status), dimsum_gemm_tn and dimsum_gemm_nn can
give before a kernel is launched, and the kernel family dimsum_gemm_nt_kernel_for picks over a grid of launch shapes. The numbers were
recorded from the library BEFORE the host layer was refactored and are kept verbatim: a refactor of that layer has to reproduce them.

CPU-only. Every pointer is a made-up, suitably aligned address that is never read: each TN / NN case is refused (a status that is neither
DIMSUM_OK nor DIMSUM_ERR_LAUNCH) and the NT cases go through the query, so nothing is launched.

A condition joined by `||` has one case per disjunct where the disjunct can be the only fault. `return DIMSUM_ERR_*` lines and disjuncts that
have no case of their own:
  * every `return launch_status()` (DIMSUM_ERR_LAUNCH): a kernel has to go out first;
  * f16_qkv `257 * ldc * 2 >= 2^31` and gated `257 * ldc * 2 + 6 F >= 2^31`: the common `257 * ldc * 4 >= 2^31` refuses those ldc first;
  * `a_alias_rows % 64 != 0` / `b_alias_rows % 64 != 0` alone: k = 3 * rows is then no multiple of 64, which is refused first (same status;
    the cases below break both);
  * TN `tn_pair_b_cols` given without `tn_pair_a_cols`: the three pieces' split count is then read as row ranges and the shape check in
    front refuses it (same status);
  * NN `k / splits % 8 != 0`: implied by whole 64-row tiles, which the shape check in front asks for.

The dispatch grid's persistent-stream rule asks the CURRENT device for its CU count and falls back to 256 without a device; an MI355X has
256 CUs, so the recorded grid holds on a box without a GPU and on an MI355X alike."""
import ctypes as C

import pytest

from dimsum_amd import _lib

OK, NULL, DTYPE, SHAPE, STRIDE, UNSUPPORTED, LAUNCH, ABI = range(8)
F32, F16, BF16 = _lib.F32, _lib.F16, _lib.BF16
E_F32, E_SPLIT3, E_GATED16, E_BIAS, E_GATERES, E_QKV, E_CONV = range(7)
_BASE_FIELDS = {n for n, _ in _lib.GemmParams._fields_}


def _addr(i):
    return 0x10000000 + 0x100000 * i                 # 1-MB aligned, distinct, never dereferenced


# ---- the served base calls (a case = a base, or a base with an epilogue's operands on top, changed in ONE respect) ----------------------
# NT: (256, 128) x (256, 128)^T fp16, plain fp32 output
NT = dict(m=256, n=256, k=128, operand_dtype=F16, epilogue=E_F32, out_scale=1.0, lda=128, ldb=128, ldc=256, a_ptr=_addr(0), b_ptr=_addr(1), c_ptr=_addr(3))
SCALES = dict(a_inv_scale_ptr=_addr(6), b_inv_scale_ptr=_addr(7))
BIAS = dict(epilogue=E_BIAS, bias_ptr=_addr(2))
GATERES = dict(epilogue=E_GATERES, bias_ptr=_addr(2), residual_ptr=_addr(4), residual_ld=256, gate_ptr=_addr(5), gate_ld=256, rows_per_batch=256)
QKV = dict(epilogue=E_QKV, **SCALES, gate_bound_ptr=_addr(8), rows_per_batch=256, qkv_q_cols=64)
CONV = dict(epilogue=E_CONV, conv_weight_ptr=_addr(9), conv_bias_ptr=_addr(10), conv_rows=256, conv_width=4, conv_seq=64, conv_weight_ld=4)
SPLIT3 = dict(epilogue=E_SPLIT3, operand_dtype=BF16, ldc=384)                       # F = 128: (M, 3 F) bf16
GATED16 = dict(epilogue=E_GATED16, ldc=128)
BOUND = dict(**GATED16, **SCALES, gate_bound_ptr=_addr(8), h_inv_scale_ptr=_addr(11))
X12 = dict(**SPLIT3, x12_ptr=_addr(12), x12_ld=256)
X12_F16 = dict(**BOUND, x12_ptr=_addr(12), x12_ld=256)
A_ALIAS = dict(operand_dtype=BF16, k=192, ldb=192, a_alias_rows=64)                 # lda = 128 = the [hi | lo] pair
B_ALIAS = dict(operand_dtype=BF16, k=192, lda=192, b_alias_rows=64)
# TN: (128, 256)^T x (128, 256) bf16, one range; NN: (256, 128) x (128, 256) fp16 with the factor table
TN = dict(m=256, n=256, k=128, operand_dtype=BF16, epilogue=E_F32, out_scale=1.0, lda=256, ldb=256, ldc=256, a_ptr=_addr(0), b_ptr=_addr(1), c_ptr=_addr(3),
          splits=1, c_split_stride=256 * 256)
TN_SCALES = dict(operand_dtype=F16, **SCALES)
TN_BLOCKS = dict(operand_dtype=F16, a_block_inv_ptr=_addr(13), a_block_inv_ld=2, b_inv_scale_ptr=_addr(7))
TN_ROWFAC = dict(operand_dtype=F16, k_scale_ptr=_addr(14), c_scale_ptr=_addr(15))
TN_ROWINV = dict(operand_dtype=F16, k_inv_a_ptr=_addr(16), k_inv_b_ptr=_addr(17))
TN_PAIRS = dict(lda=512, ldb=512, tn_pair_a_cols=256, tn_pair_b_cols=256, splits=3)
TN_ALIAS = dict(k=192, a_alias_rows=64)
TWO = dict(k=256, splits=2)                                                          # two ranges of two K tiles
NN = dict(m=256, n=256, k=128, operand_dtype=F16, epilogue=E_F32, out_scale=1.0, lda=128, ldb=256, ldc=256, a_ptr=_addr(0), b_ptr=_addr(1), c_ptr=_addr(3),
          a_inv_scale_ptr=_addr(6), k_scale_ptr=_addr(14), c_scale_ptr=_addr(15), splits=1, c_split_stride=256 * 256)
NN_ROWINV = dict(k_scale_ptr=None, c_scale_ptr=None, k_inv_a_ptr=_addr(16), k_inv_b_ptr=_addr(17))
BASES = {"nt": NT, "tn": TN, "nn": NN}


def _structs(fields):
    G = _lib.GemmParams()
    X = None if fields.get("no_ext") else _lib.attach_ext(G, _lib.GemmExt)
    for key, val in fields.items():
        if key in ("splits", "c_split_stride", "no_ext", "null"):
            continue
        if key == "ext_size":
            X.struct_size = val
        elif key in _BASE_FIELDS:
            setattr(G, key, val)
        else:
            setattr(X, key, val)
    return G, X


def _status(entry, fields):
    """the status of one call: NT through the query (negated there), TN / NN from the entry point itself"""
    lib = _lib.load()
    G, _ = _structs(fields)
    P = None if fields.get("null") else G
    if entry == "nt":
        rc = lib.dimsum_gemm_nt_kernel_for(P)
        return -rc if rc < 0 else OK
    return (lib.dimsum_gemm_tn if entry == "tn" else lib.dimsum_gemm_nn)(P, fields["splits"], fields["c_split_stride"], None)


BIG_ROWS = 1 << 22          # 256 rows of this many 16-bit elements reach 2^31 bytes
BIG_KROWS = 1 << 24         # 64 rows do
BIG_C = 1 << 21             # 257 fp32 rows do
EXT_TOO_BIG = C.sizeof(_lib.GemmExt) + 8
_STRUCT = [({"null": 1}, NULL), ({"struct_size": 0}, ABI), ({"struct_size": C.sizeof(_lib.GemmParams) + 8}, ABI), ({"ext_size": EXT_TOO_BIG}, ABI), ({"ext_size": 2}, ABI)]
_ABC = [({"a_ptr": None}, NULL), ({"b_ptr": None}, NULL), ({"c_ptr": None}, NULL)]
_C_ROWS = [({"ldc": 258}, STRIDE), ({"ldc": 252}, STRIDE), ({"c_ptr": _addr(3) + 8}, STRIDE)]       # fp32 output rows: ldc % 4, ldc >= n, 16-byte base

# (entry, overlays on the entry's base, the one change, status)
CASES = (
    [("nt", (), m, s) for m, s in _STRUCT + _ABC + _C_ROWS + [
        ({"operand_dtype": F32}, DTYPE), ({"operand_dtype": 3}, DTYPE), ({"operand_dtype": -1}, DTYPE),
        ({"m": 0}, SHAPE), ({"n": 0}, SHAPE), ({"n": -4}, SHAPE), ({"k": 64}, SHAPE), ({"m": 384}, SHAPE), ({"k": 160, "lda": 160, "ldb": 160}, SHAPE), ({"n": 254}, SHAPE),
        ({"lda": 132}, STRIDE), ({"ldb": 132}, STRIDE), ({"lda": 64}, STRIDE), ({"ldb": 64}, STRIDE), ({"a_ptr": _addr(0) + 8}, STRIDE), ({"b_ptr": _addr(1) + 8}, STRIDE),
        ({"lda": BIG_ROWS}, STRIDE), ({"ldb": BIG_ROWS}, STRIDE), ({"ldc": BIG_C}, STRIDE),
        ({"a_alias_weight_order": 1}, SHAPE),
        ({"a_inv_scale_ptr": _addr(6)}, NULL), ({"b_inv_scale_ptr": _addr(7)}, NULL), ({**SCALES, "b_inv_scale_ptr": _addr(7) + 8}, STRIDE),
        ({"tune_variant": 1}, UNSUPPORTED), ({"tune_variant": 100}, UNSUPPORTED), ({"tune_variant": 511}, UNSUPPORTED), ({"tune_variant": 515}, UNSUPPORTED),
        ({"tune_variant": -1}, UNSUPPORTED), ({"tune_variant": 512, "operand_dtype": BF16}, UNSUPPORTED),
        ({"epilogue": 7}, UNSUPPORTED), ({"epilogue": -1}, UNSUPPORTED),
        ({"operand_dtype": F32, "m": 0}, DTYPE), ({"m": 0, "lda": 132}, SHAPE), ({"a_ptr": None, "operand_dtype": F32}, NULL),          # the order of the common checks
        ({"tune_variant": 1, "ldc": 258}, UNSUPPORTED), ({"a_inv_scale_ptr": _addr(6), "tune_variant": 1}, NULL),
    ]]
    + [("nt", (A_ALIAS,), m, s) for m, s in [
        ({"a_alias_rows": -64}, SHAPE), ({"a_alias_rows": 32, "k": 128}, SHAPE), ({"k": 128}, SHAPE), ({"k": 256}, SHAPE), ({"lda": 64}, STRIDE), ({"lda": 120}, STRIDE),
    ]]
    + [("nt", (B_ALIAS,), m, s) for m, s in [
        ({"b_alias_rows": -64}, SHAPE), ({"b_alias_rows": 32, "k": 128}, SHAPE), ({"k": 128}, SHAPE), ({"ldb": 64}, STRIDE), ({"a_alias_weight_order": 1}, SHAPE),
        (BIAS, SHAPE), (GATERES, SHAPE), (SPLIT3, SHAPE), (GATED16, SHAPE),
    ]]
    + [("nt", (BIAS,), m, s) for m, s in _C_ROWS + [({"bias_ptr": None}, NULL), ({"bias_ptr": _addr(2) + 8}, NULL)]]
    + [("nt", (GATERES,), m, s) for m, s in _C_ROWS + [
        ({"residual_ptr": None}, NULL), ({"residual_ld": 258}, STRIDE), ({"residual_ld": 252}, STRIDE), ({"residual_ptr": _addr(4) + 8}, STRIDE),
        ({"bias_ptr": _addr(2) + 8}, STRIDE), ({"gate_ld": 258}, STRIDE), ({"gate_ptr": _addr(5) + 8}, STRIDE),
        ({"rows_per_batch": 0}, SHAPE), ({"rows_per_batch": 128}, SHAPE), ({"m": 768, "rows_per_batch": 512}, SHAPE),
        ({"residual_ptr": None, "ldc": 258}, NULL), ({"ldc": 258, "rows_per_batch": 0}, STRIDE),
    ]]
    + [("nt", (QKV,), m, s) for m, s in [
        ({"operand_dtype": BF16}, NULL), ({"a_inv_scale_ptr": None, "b_inv_scale_ptr": None}, NULL), ({"gate_bound_ptr": None}, NULL),
        ({"rows_per_batch": 0}, SHAPE), ({"rows_per_batch": 128}, SHAPE), ({"m": 768, "rows_per_batch": 512}, SHAPE), ({"qkv_q_cols": 0}, SHAPE), ({"qkv_q_cols": 8}, SHAPE),
        ({"qkv_q_cols": 512}, SHAPE), ({"n": 252}, SHAPE),
        ({"ldc": 260}, STRIDE), ({"ldc": 248}, STRIDE), ({"c_ptr": _addr(3) + 8}, STRIDE), ({"bias_ptr": _addr(2) + 8}, STRIDE),
        ({"gate_bound_ptr": None, "n": 252}, NULL), ({"n": 252, "ldc": 260}, SHAPE),
    ]]
    + [("nt", (CONV,), m, s) for m, s in _C_ROWS + [
        ({"conv_weight_ptr": None}, NULL), ({"conv_rows": 0}, SHAPE), ({"conv_rows": 128}, SHAPE), ({"conv_rows": 512}, SHAPE), ({"conv_width": 1}, SHAPE),
        ({"conv_width": 5, "conv_weight_ld": 8}, SHAPE), ({"conv_seq": 0}, SHAPE), ({"conv_seq": 96}, SHAPE), ({"conv_seq": 2}, SHAPE),
        ({"conv_seq": 128, "n": 320, "ldc": 320}, SHAPE), ({"conv_weight_ld": 2}, SHAPE), ({"conv_weight_ptr": None, "conv_rows": 0}, NULL), ({"conv_rows": 0, "ldc": 258}, SHAPE),
    ]]
    + [("nt", (SPLIT3,), m, s) for m, s in [
        ({"n": 264}, SHAPE), ({"c_image_pieces": 1}, UNSUPPORTED), ({"c_image_pieces": 4}, UNSUPPORTED), ({"ldc": 388}, STRIDE), ({"ldc": 376}, STRIDE),
        ({"c_image_pieces": 2, "ldc": 248}, STRIDE), ({"c_ptr": _addr(3) + 8}, STRIDE), ({"bias_ptr": _addr(2) + 8}, STRIDE), ({"gate_bound_ptr": _addr(8)}, NULL),
        ({"x12_ptr": _addr(12), "x12_ld": 256, "operand_dtype": F16}, UNSUPPORTED), ({"x12_ptr": _addr(12), "x12_ld": 256, **SCALES}, UNSUPPORTED),
    ]]
    + [("nt", (GATED16,), m, s) for m, s in [
        ({"n": 264}, SHAPE), ({"c_image_pieces": 2}, UNSUPPORTED), ({"ldc": 132}, STRIDE), ({"ldc": 120}, STRIDE), ({"c_ptr": _addr(3) + 8}, STRIDE),
        ({"bias_ptr": _addr(2) + 8}, STRIDE), ({"gate_bound_ptr": _addr(8), "h_inv_scale_ptr": _addr(11)}, NULL), ({**SCALES, "gate_bound_ptr": _addr(8)}, NULL),
        ({"x12_ptr": _addr(12), "x12_ld": 256}, UNSUPPORTED), ({"x12_ptr": _addr(12), "x12_ld": 256, **SCALES}, UNSUPPORTED),
        ({"x12_ptr": _addr(12), "x12_ld": 256, "operand_dtype": BF16}, UNSUPPORTED),
    ]]
    + [("nt", (X12,), m, s) for m, s in [({"x12_ld": 258}, STRIDE), ({"x12_ld": 252}, STRIDE), ({"x12_ptr": _addr(12) + 8}, STRIDE), ({"x12_ld": BIG_C}, STRIDE)]]
    + [("nt", (X12_F16,), m, s) for m, s in [({"x12_ld": 258}, STRIDE), ({"x12_ptr": _addr(12) + 8}, STRIDE), ({"operand_dtype": BF16}, UNSUPPORTED), ({"h_inv_scale_ptr": None}, NULL)]]
    + [("tn", (), m, s) for m, s in _STRUCT + _ABC + _C_ROWS + [
        ({"operand_dtype": F32}, DTYPE), ({"operand_dtype": 3}, DTYPE), ({"epilogue": E_BIAS}, UNSUPPORTED), ({"bias_ptr": _addr(2)}, UNSUPPORTED),
        ({"operand_dtype": F16, "a_inv_scale_ptr": _addr(6)}, NULL), ({"operand_dtype": F16, "b_inv_scale_ptr": _addr(7)}, NULL),
        ({"operand_dtype": F16, "a_block_inv_ptr": _addr(13), "a_block_inv_ld": 2}, NULL), ({"operand_dtype": F16, "k_inv_b_ptr": _addr(17)}, NULL),
        ({"splits": 0}, SHAPE), ({"splits": -1}, SHAPE), ({"m": 0}, SHAPE), ({"n": 0}, SHAPE), ({"m": 384, "lda": 384}, SHAPE), ({"n": 254}, SHAPE), ({"n": 128, "ldb": 128}, SHAPE),
        ({"k": 192, "splits": 2}, SHAPE), ({"k": 128, "splits": 2}, SHAPE), ({"k": 64}, SHAPE),
        ({"lda": 260}, STRIDE), ({"ldb": 260}, STRIDE), ({"lda": 128}, STRIDE), ({"ldb": 248}, STRIDE), ({"a_ptr": _addr(0) + 8}, STRIDE), ({"b_ptr": _addr(1) + 8}, STRIDE),
        ({**TWO, "c_split_stride": 256 * 256 + 2}, STRIDE), ({**TWO, "c_split_stride": 256 * 256 - 4}, STRIDE),
        ({"lda": BIG_KROWS}, STRIDE), ({"ldb": BIG_KROWS}, STRIDE), ({"ldc": BIG_C}, STRIDE),
        ({"b_alias_rows": 64}, UNSUPPORTED), ({"a_alias_weight_order": 1}, UNSUPPORTED),
        ({"operand_dtype": F32, "epilogue": E_BIAS}, DTYPE), ({"epilogue": E_BIAS, "m": 0}, UNSUPPORTED), ({"m": 0, "lda": 260}, SHAPE), ({"b_alias_rows": 64, "m": 0}, SHAPE),
        ({"b_alias_rows": 64, "lda": 260}, STRIDE),
    ]]
    + [("tn", (TN_SCALES,), m, s) for m, s in [
        ({"operand_dtype": BF16}, UNSUPPORTED), (TWO, UNSUPPORTED), ({"tn_pair_a_cols": 256}, UNSUPPORTED), ({"a_alias_rows": 64, "k": 192}, UNSUPPORTED),
        ({"b_inv_scale_ptr": _addr(7) + 8}, STRIDE), ({"a_block_inv_ptr": _addr(13), "a_block_inv_ld": 2}, SHAPE),
    ]]
    + [("tn", (TN_BLOCKS,), m, s) for m, s in [
        ({"operand_dtype": BF16}, UNSUPPORTED), (TWO, UNSUPPORTED), ({"a_block_inv_ld": 1}, SHAPE), ({"k": 8192, "a_block_inv_ld": 128}, SHAPE), ({"b_inv_scale_ptr": None}, NULL),
    ]]
    + [("tn", (TN_ROWFAC,), m, s) for m, s in [
        ({"c_scale_ptr": None}, NULL), ({"k_inv_a_ptr": _addr(16)}, NULL), ({"operand_dtype": BF16}, UNSUPPORTED), (SCALES, UNSUPPORTED),
        ({"a_block_inv_ptr": _addr(13), "a_block_inv_ld": 2, "b_inv_scale_ptr": _addr(7)}, UNSUPPORTED), ({"tn_pair_a_cols": 256}, UNSUPPORTED),
        ({"a_alias_rows": 64, "k": 192}, UNSUPPORTED), ({"splits": 0}, SHAPE), ({"k": 32768}, SHAPE), ({"k_scale_ptr": _addr(14) + 8}, STRIDE),
        ({"c_scale_ptr": _addr(15) + 2}, STRIDE), ({"k_scale_ptr": _addr(14) + 8, "m": 0}, STRIDE), ({"k": 32768, "operand_dtype": BF16}, UNSUPPORTED),
    ]]
    + [("tn", (TN_ROWINV,), m, s) for m, s in [
        ({"k_scale_ptr": _addr(14)}, NULL), ({"c_scale_ptr": _addr(15)}, NULL), ({"operand_dtype": BF16}, UNSUPPORTED), ({"splits": 0}, SHAPE), ({"k": 32768}, SHAPE),
        ({"k_inv_a_ptr": _addr(16) + 8}, STRIDE), ({"k_inv_b_ptr": _addr(17) + 8}, STRIDE), ({"k": 132}, STRIDE), ({"k_inv_b_ptr": None, "k": 132}, STRIDE),
    ]]
    + [("tn", (TN_PAIRS,), m, s) for m, s in [
        ({"tn_pair_b_cols": 0}, SHAPE), ({"tn_pair_a_cols": 0}, SHAPE), ({"tn_pair_a_cols": -8}, SHAPE), ({"splits": 2}, SHAPE), ({"splits": 4}, SHAPE),
        ({"a_alias_rows": 64, "k": 192}, SHAPE), ({"tn_pair_a_cols": 260, "lda": 520}, SHAPE), ({"tn_pair_b_cols": 260, "ldb": 520}, SHAPE), ({"n": 128}, SHAPE),
        ({"lda": 256}, STRIDE), ({"ldb": 256}, STRIDE), ({"lda": 256, "splits": 4}, SHAPE),
    ]]
    + [("tn", (TN_ALIAS,), m, s) for m, s in [
        ({"k": 384, "a_alias_rows": 128, "splits": 3}, SHAPE), ({"a_alias_rows": -64}, SHAPE), ({"a_alias_rows": 32}, SHAPE), ({"k": 128}, SHAPE), ({"k": 256}, SHAPE),
    ]]
    + [("nn", (), m, s) for m, s in _STRUCT + _ABC + _C_ROWS + [
        ({"k_scale_ptr": None}, NULL), ({"c_scale_ptr": None}, NULL), ({"k_scale_ptr": None, "c_scale_ptr": None}, NULL), ({"k_inv_a_ptr": _addr(16)}, NULL),
        ({"k_inv_b_ptr": _addr(17)}, NULL), ({"operand_dtype": BF16}, DTYPE), ({"operand_dtype": F32}, DTYPE), ({"operand_dtype": F32, "k_scale_ptr": None}, NULL),
        ({"epilogue": E_BIAS}, UNSUPPORTED), ({"bias_ptr": _addr(2)}, UNSUPPORTED), ({"b_inv_scale_ptr": _addr(7)}, UNSUPPORTED),
        ({"a_block_inv_ptr": _addr(13)}, UNSUPPORTED), ({"tn_pair_a_cols": 256}, UNSUPPORTED), ({"a_alias_rows": 64}, UNSUPPORTED), ({"b_alias_rows": 64}, UNSUPPORTED),
        ({"a_alias_weight_order": 1}, UNSUPPORTED), ({"operand_dtype": BF16, "epilogue": E_BIAS}, DTYPE), ({"epilogue": E_BIAS, "m": 0}, UNSUPPORTED),
        ({"splits": 0}, SHAPE), ({"m": 0}, SHAPE), ({"n": 0}, SHAPE), ({"m": 384}, SHAPE), ({"n": 128}, SHAPE), ({"k": 192, "lda": 192, "splits": 2}, SHAPE),
        ({"splits": 2}, SHAPE), ({"k": 64}, SHAPE), ({"k": 32768, "lda": 32768}, SHAPE), ({"m": 0, "lda": 132}, SHAPE), ({"m": 0, "k_scale_ptr": _addr(14) + 8}, SHAPE),
        ({"lda": 132}, STRIDE), ({"ldb": 260}, STRIDE), ({"lda": 64}, STRIDE), ({"ldb": 248}, STRIDE), ({"a_ptr": _addr(0) + 8}, STRIDE), ({"b_ptr": _addr(1) + 8}, STRIDE),
        ({"k": 256, "lda": 256, "splits": 2, "c_split_stride": 256 * 256 + 2}, STRIDE), ({"k": 256, "lda": 256, "splits": 2, "c_split_stride": 256 * 256 - 4}, STRIDE),
        ({"k_scale_ptr": _addr(14) + 8}, STRIDE), ({"c_scale_ptr": _addr(15) + 2}, STRIDE),
        ({"lda": BIG_ROWS}, STRIDE), ({"ldb": BIG_KROWS}, STRIDE), ({"ldc": BIG_C}, STRIDE),
    ]]
    + [("nn", (NN_ROWINV,), m, s) for m, s in [
        ({"k_scale_ptr": _addr(14)}, NULL), ({"c_scale_ptr": _addr(15)}, NULL), ({"k_inv_a_ptr": _addr(16) + 8}, STRIDE), ({"k_inv_b_ptr": _addr(17) + 8}, STRIDE),
        ({"k": 32768, "lda": 32768}, SHAPE),
    ]]
)


def _fields(case):
    entry, overlays, mut, _ = case
    fields = dict(BASES[entry])
    for o in overlays:
        fields.update(o)
    fields.update(mut)
    return fields


def _name(d):
    return next(k for k, v in globals().items() if v is d and k.isupper())


def _case_id(case):
    entry, overlays, mut, _ = case
    return "+".join([entry] + [_name(o) for o in overlays]) + ":" + ",".join(f"{k}={v}" for k, v in mut.items())


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_refused_inputs_keep_their_status(case):
    want = case[3]
    assert want not in (OK, LAUNCH)                  # a refusal: nothing is launched
    assert _status(case[0], _fields(case)) == want


WEIGHT_ORDER, PIECES2, NO_EXT = {"a_alias_weight_order": 1}, {"c_image_pieces": 2}, {"no_ext": 1}
NT_SERVED = [((), 1), ((SCALES,), 1), ((BIAS,), 1), ((GATERES,), 0), ((QKV,), 1), ((CONV,), 1), ((SPLIT3,), 0), ((GATED16,), 0), ((BOUND,), 0), ((X12,), 0), ((X12_F16,), 0),
             ((A_ALIAS,), 0), ((B_ALIAS,), 0), ((A_ALIAS, WEIGHT_ORDER), 0), ((B_ALIAS, CONV), 0), ((A_ALIAS, SPLIT3), 0), ((SPLIT3, PIECES2), 0), ((NO_EXT,), 1)]


@pytest.mark.parametrize("overlays,family", NT_SERVED, ids=["+".join(["nt"] + [_name(o) for o in ov]) for ov, _ in NT_SERVED])
def test_nt_base_calls_are_what_the_cases_break(overlays, family):
    """the NT bases pass every check (a refusal above is due to the one change made): the query, which runs those checks and launches nothing,
    names a kernel family for them. (The TN / NN entry points have no such query: their bases cannot be called here.)"""
    fields = dict(NT)
    for o in overlays:
        fields.update(o)
    G, _ = _structs(fields)
    assert _lib.load().dimsum_gemm_nt_kernel_for(G) == family


# ---- dimsum_gemm_nt_kernel_for over a grid of launch shapes -----------------------------------------------------------------------------
DTYPES, EPILOGUES, TUNES, KS = (F16, BF16), tuple(range(7)), (0, 512, 513, 514), (128, 192, 576, 640, 1024)
# (m, n): tiles_m * ceil(n / 256) below, at (m = 4352: next to) and above the 256 workgroups of the persistent stream, n % 256 zero and non-zero
MN = ([(256, n) for n in (65152, 65280, 65408, 65536, 65664, 65792)] + [(4352, n) for n in (3712, 3840, 3968, 4096)]
      + [(16384, n) for n in (640, 768, 896, 1024, 1152, 1280)])
ALIASES = ((0, 0), (1, 0), (0, 1), (1, 1))           # (a_alias_rows, b_alias_rows) = k / 3 each where set (refused unless k = 3 x 64 j)
_CODE = "012" + "?" * 7
_REFUSED = {-NULL: "N", -DTYPE: "D", -SHAPE: "S", -STRIDE: "T", -UNSUPPORTED: "U", -LAUNCH: "L", -ABI: "A"}


def _grid_rows():
    """one row per (dtype, epilogue, tune_variant, k): the answers over (m, n) x scales x alias mode x x12, one character each: the family
    0 / 1 / 2, or the refusal's letter (N NULL, D dtype, S shape, T stride, U unsupported). Every epilogue's own operands are given
    (bias, residual + gate, q_cols, conv taps ...); "scales" adds gate_bound (+ h_inv_scale for gated_f16) where the epilogue takes them"""
    lib = _lib.load()
    G, X = _structs(dict(out_scale=1.0, lda=1024, ldb=1024, a_ptr=_addr(0), b_ptr=_addr(1), bias_ptr=_addr(2), c_ptr=_addr(3), residual_ptr=_addr(4), gate_ptr=_addr(5),
                         rows_per_batch=256, qkv_q_cols=64, conv_weight_ptr=_addr(9), conv_bias_ptr=_addr(10), conv_rows=256, conv_width=4, conv_seq=64, conv_weight_ld=4))
    rows = []
    for dtype in DTYPES:
        for epi in EPILOGUES:
            for tune in TUNES:
                for k in KS:
                    G.operand_dtype, G.epilogue, X.tune_variant, G.k = dtype, epi, tune, k
                    row = []
                    for m, n in MN:
                        G.m, G.n, G.ldc, X.residual_ld, X.gate_ld, X.x12_ld = m, n, 2 * n, n, n, n
                        for scales in (0, 1):
                            G.a_inv_scale_ptr, G.b_inv_scale_ptr = (_addr(6), _addr(7)) if scales else (None, None)
                            bound = scales and epi in (E_GATED16, E_QKV)
                            X.gate_bound_ptr = _addr(8) if bound else None
                            X.h_inv_scale_ptr = _addr(11) if bound and epi == E_GATED16 else None
                            for alias_a, alias_b in ALIASES:
                                X.a_alias_rows, X.b_alias_rows = alias_a * (k // 3), alias_b * (k // 3)
                                for x12 in (0, 1):
                                    X.x12_ptr = _addr(12) if x12 else None
                                    rc = int(lib.dimsum_gemm_nt_kernel_for(G))
                                    row.append(_CODE[rc] if rc >= 0 else _REFUSED[rc])
                    rows.append("".join(row))
    return rows


# the 280 recorded rows are 25 distinct ones: ROWS in the order they first appear, GRID one line per (dtype, epilogue) with one letter per (tune_variant, k)
ROWS = """
11SSSSSS11SSSSSS11SSSSSS11SSSSSS11SSSSSS11SSSSSS11SSSSSS11SSSSSS11SSSSSS11SSSSSS11SSSSSS11SSSSSS11SSSSSS11SSSSSS11SSSSSS11SSSSSS11SSSSSS11SSSSSS11SSSSSS11SSSSSS11SSSSSS11SSSSSS11SSSSSS11SSSSSS11SSSSSS11SSSSSS11SSSSSS11SSSSSS11SSSSSS11SSSSSS11SSSSSS11SSSSSS
1111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111
00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS
0000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000
0USSSSSS0USSSSSS0USSSSSS0USSSSSS0USSSSSS0USSSSSS0USSSSSS0USSSSSS0USSSSSS0USSSSSS0USSSSSS0USSSSSS0USSSSSS0USSSSSS0USSSSSS0USSSSSS0USSSSSS0USSSSSS0USSSSSS0USSSSSS0USSSSSS0USSSSSS0USSSSSS0USSSSSS0USSSSSS0USSSSSS0USSSSSS0USSSSSS0USSSSSS0USSSSSS0USSSSSS0USSSSSS
0U0USSSS0U0USSSS0U0USSSS0U0USSSS0U0USSSS0U0USSSS0U0USSSS0U0USSSS0U0USSSS0U0USSSS0U0USSSS0U0USSSS0U0USSSS0U0USSSS0U0USSSS0U0USSSS0U0USSSS0U0USSSS0U0USSSS0U0USSSS0U0USSSS0U0USSSS0U0USSSS0U0USSSS0U0USSSS0U0USSSS0U0USSSS0U0USSSS0U0USSSS0U0USSSS0U0USSSS0U0USSSS
0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS
0U0USSSS0000SSSS0U0USSSS0000SSSS0U0USSSS0000SSSS0U0USSSS0000SSSS0U0USSSS0000SSSS0U0USSSS0000SSSS0U0USSSS0000SSSS0U0USSSS0000SSSS0U0USSSS0000SSSS0U0USSSS0000SSSS0U0USSSS0000SSSS0U0USSSS0000SSSS0U0USSSS0000SSSS0U0USSSS0000SSSS0U0USSSS0000SSSS0U0USSSS0000SSSS
0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS2USSSSSS20SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS2USSSSSS20SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS2USSSSSS20SSSSSS
1USSSSSS10SSSSSS1USSSSSS10SSSSSS1USSSSSS10SSSSSS1USSSSSS10SSSSSS1USSSSSS10SSSSSS1USSSSSS10SSSSSS1USSSSSS10SSSSSS1USSSSSS10SSSSSS1USSSSSS10SSSSSS1USSSSSS10SSSSSS1USSSSSS10SSSSSS1USSSSSS10SSSSSS1USSSSSS10SSSSSS1USSSSSS10SSSSSS1USSSSSS10SSSSSS1USSSSSS10SSSSSS
1U1USSSS1010SSSS1U1USSSS1010SSSS1U1USSSS1010SSSS1U1USSSS1010SSSS1U1USSSS1010SSSS1U1USSSS1010SSSS1U1USSSS1010SSSS1U1USSSS1010SSSS1U1USSSS1010SSSS1U1USSSS1010SSSS1U1USSSS1010SSSS1U1USSSS1010SSSS1U1USSSS1010SSSS1U1USSSS1010SSSS1U1USSSS1010SSSS1U1USSSS1010SSSS
1111SSSS1111SSSS1111SSSS1111SSSS1111SSSS1111SSSS1111SSSS1111SSSS1111SSSS1111SSSS1111SSSS1111SSSS1111SSSS1111SSSS1111SSSS1111SSSS1111SSSS1111SSSS1111SSSS1111SSSS1111SSSS1111SSSS1111SSSS1111SSSS1111SSSS1111SSSS1111SSSS1111SSSS1111SSSS1111SSSS1111SSSS1111SSSS
0000SSSS0000SSSS0000SSSS0000SSSS0000SSSS0000SSSS0000SSSS0000SSSS0000SSSS0000SSSS0000SSSS0000SSSS0000SSSS0000SSSS0000SSSS0000SSSS0000SSSS0000SSSS0000SSSS0000SSSS0000SSSS0000SSSS0000SSSS0000SSSS0000SSSS0000SSSS0000SSSS0000SSSS0000SSSS0000SSSS0000SSSS0000SSSS
00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS22SSSSSS22SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS22SSSSSS22SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS00SSSSSS22SSSSSS22SSSSSS
NNSSSSSS11SSSSSSNNSSSSSS11SSSSSSNNSSSSSS11SSSSSSNNSSSSSS11SSSSSSNNSSSSSS11SSSSSSNNSSSSSS11SSSSSSNNSSSSSS11SSSSSSNNSSSSSS11SSSSSSNNSSSSSS11SSSSSSNNSSSSSS11SSSSSSNNSSSSSS11SSSSSSNNSSSSSS11SSSSSSNNSSSSSS11SSSSSSNNSSSSSS11SSSSSSNNSSSSSS11SSSSSSNNSSSSSS11SSSSSS
NNNNSSSS1111SSSSNNNNSSSS1111SSSSNNNNSSSS1111SSSSNNNNSSSS1111SSSSNNNNSSSS1111SSSSNNNNSSSS1111SSSSNNNNSSSS1111SSSSNNNNSSSS1111SSSSNNNNSSSS1111SSSSNNNNSSSS1111SSSSNNNNSSSS1111SSSSNNNNSSSS1111SSSSNNNNSSSS1111SSSSNNNNSSSS1111SSSSNNNNSSSS1111SSSSNNNNSSSS1111SSSS
NNSSSSSS00SSSSSSNNSSSSSS00SSSSSSNNSSSSSS00SSSSSSNNSSSSSS00SSSSSSNNSSSSSS00SSSSSSNNSSSSSS00SSSSSSNNSSSSSS00SSSSSSNNSSSSSS00SSSSSSNNSSSSSS00SSSSSSNNSSSSSS00SSSSSSNNSSSSSS00SSSSSSNNSSSSSS00SSSSSSNNSSSSSS00SSSSSSNNSSSSSS00SSSSSSNNSSSSSS00SSSSSSNNSSSSSS00SSSSSS
NNNNSSSS0000SSSSNNNNSSSS0000SSSSNNNNSSSS0000SSSSNNNNSSSS0000SSSSNNNNSSSS0000SSSSNNNNSSSS0000SSSSNNNNSSSS0000SSSSNNNNSSSS0000SSSSNNNNSSSS0000SSSSNNNNSSSS0000SSSSNNNNSSSS0000SSSSNNNNSSSS0000SSSSNNNNSSSS0000SSSSNNNNSSSS0000SSSSNNNNSSSS0000SSSSNNNNSSSS0000SSSS
UUSSSSSSUUSSSSSSUUSSSSSSUUSSSSSSUUSSSSSSUUSSSSSSUUSSSSSSUUSSSSSSUUSSSSSSUUSSSSSSUUSSSSSSUUSSSSSSUUSSSSSSUUSSSSSSUUSSSSSSUUSSSSSSUUSSSSSSUUSSSSSSUUSSSSSSUUSSSSSSUUSSSSSSUUSSSSSSUUSSSSSSUUSSSSSSUUSSSSSSUUSSSSSSUUSSSSSSUUSSSSSSUUSSSSSSUUSSSSSSUUSSSSSSUUSSSSSS
UUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUUU
00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS00SSSSSS0USSSSSS
0000SSSS0U0USSSS0000SSSS0U0USSSS0000SSSS0U0USSSS0000SSSS0U0USSSS0000SSSS0U0USSSS0000SSSS0U0USSSS0000SSSS0U0USSSS0000SSSS0U0USSSS0000SSSS0U0USSSS0000SSSS0U0USSSS0000SSSS0U0USSSS0000SSSS0U0USSSS0000SSSS0U0USSSS0000SSSS0U0USSSS0000SSSS0U0USSSS0000SSSS0U0USSSS
UUUUSSSSUUUUSSSSUUUUSSSSUUUUSSSSUUUUSSSSUUUUSSSSUUUUSSSSUUUUSSSSUUUUSSSSUUUUSSSSUUUUSSSSUUUUSSSSUUUUSSSSUUUUSSSSUUUUSSSSUUUUSSSSUUUUSSSSUUUUSSSSUUUUSSSSUUUUSSSSUUUUSSSSUUUUSSSSUUUUSSSSUUUUSSSSUUUUSSSSUUUUSSSSUUUUSSSSUUUUSSSSUUUUSSSSUUUUSSSSUUUUSSSSUUUUSSSS
NNSSSSSSNNSSSSSSNNSSSSSSNNSSSSSSNNSSSSSSNNSSSSSSNNSSSSSSNNSSSSSSNNSSSSSSNNSSSSSSNNSSSSSSNNSSSSSSNNSSSSSSNNSSSSSSNNSSSSSSNNSSSSSSNNSSSSSSNNSSSSSSNNSSSSSSNNSSSSSSNNSSSSSSNNSSSSSSNNSSSSSSNNSSSSSSNNSSSSSSNNSSSSSSNNSSSSSSNNSSSSSSNNSSSSSSNNSSSSSSNNSSSSSSNNSSSSSS
NNNNSSSSNNNNSSSSNNNNSSSSNNNNSSSSNNNNSSSSNNNNSSSSNNNNSSSSNNNNSSSSNNNNSSSSNNNNSSSSNNNNSSSSNNNNSSSSNNNNSSSSNNNNSSSSNNNNSSSSNNNNSSSSNNNNSSSSNNNNSSSSNNNNSSSSNNNNSSSSNNNNSSSSNNNNSSSSNNNNSSSSNNNNSSSSNNNNSSSSNNNNSSSSNNNNSSSSNNNNSSSSNNNNSSSSNNNNSSSSNNNNSSSSNNNNSSSS
""".split()

GRID = [ROWS[ord(c) - ord("a")] for c in "".join("""
abbccabbaacddcccddcc
effeeeffeeeffeeeffee
ghhiijkkjjghhggghhii
allccallaacmmcccmmcc
cmmccallaacmmcccmmnn
oppqqoppooqrrqqqrrqq
abbccabbaacddcccddcc
cddccsttsscddcccddcc
uvvuuswwssuvvuuuvvuu
effeeswwsseffeeeffee
cmmccswwsscmmcccmmcc
cmmccswwsscmmcccmmcc
xyyxxswwssxyyxxxyyxx
cddccsttsscddcccddcc
""".split())]


def test_kernel_family_grid():
    rows = _grid_rows()
    assert len(rows) == len(GRID) == len(DTYPES) * len(EPILOGUES) * len(TUNES) * len(KS)
    for i, (got, want) in enumerate(zip(rows, GRID)):
        assert got == want, f"row {i} (dtype, epilogue, tune, k = {DTYPES[i // 140]}, {i // 20 % 7}, {TUNES[i // 5 % 4]}, {KS[i % 5]})"
