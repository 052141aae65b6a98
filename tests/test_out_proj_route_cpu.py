"""Decision table of the mixer's out_proj route (dimsum_amd/gemm.py): which of the three inference carriers of out_proj -- the scan's
split-bf16 planes, its block-scaled fp16 out_z, or the fp16 image built by a conversion pass behind a state-split scan kernel -- the
predicates gemm.out_proj_planes_enabled / out_proj_f16_enabled / out_proj_f16_convert_enabled grant a call. No GPU: the predicates read
`is_cuda`, `dtype`, `stride()` and `data_ptr()` of xz (a stand-in here), the weight's shape / dtype / strides, the policy,
torch.backends.cuda.matmul.allow_tf32 and the environment. Every case flips ONE conjunct of the base call (8192 tokens of a (512, 128)
weight, seqlen 256, everything aligned), on the 64-channel scan kernel (1) and on a state-split one (4)."""
import pytest
import torch

from dimsum_amd import gemm

ENV = ("DIMSUM_OUT_PROJ_PLANES", "DIMSUM_OUT_PROJ_F16", "DIMSUM_SPLIT3", "DIMSUM_SPLIT3_MIN_ROWS", "DIMSUM_GEMM_NT")


class _XZ:
    """what the predicates read of the (batch, 2 d_inner, seqlen) in_proj output"""

    def __init__(self, shape, stride, ptr, dtype, is_cuda):
        self.shape, self._stride, self._ptr, self.dtype, self.is_cuda = shape, stride, ptr, dtype, is_cuda

    def stride(self, i=None):
        return self._stride if i is None else self._stride[i]

    def data_ptr(self):
        return self._ptr


BASE = dict(policy="f16s", tf32=True, env={}, rows=8192, seqlen=256, n_out=512, D=128, ptr=4096, stride=None, xz_dtype=torch.float32,
            w_dtype=torch.float32, w_t=False, is_cuda=True)

# (what flips, overrides, {scan kernel: (planes, fp16 from the scan, fp16 through the conversion pass)})
TABLE = [
    ("base", {}, {1: (0, 1, 0), 4: (1, 0, 1)}),
    ("policy_default", dict(policy="default"), {1: (0, 0, 0), 4: (1, 0, 0)}),
    ("policy_fp16", dict(policy="fp16"), {1: (0, 0, 0), 4: (0, 0, 0)}),
    ("allow_tf32_off", dict(tf32=False), {1: (0, 0, 0), 4: (0, 0, 0)}),
    ("planes_env_0", dict(env={"DIMSUM_OUT_PROJ_PLANES": "0"}), {1: (0, 1, 0), 4: (0, 0, 1)}),
    ("planes_env_1", dict(env={"DIMSUM_OUT_PROJ_PLANES": "1"}), {1: (1, 1, 0), 4: (1, 0, 1)}),
    ("planes_env_1_policy_default", dict(policy="default", env={"DIMSUM_OUT_PROJ_PLANES": "1"}), {1: (1, 0, 0), 4: (1, 0, 0)}),
    ("f16_env_0", dict(env={"DIMSUM_OUT_PROJ_F16": "0"}), {1: (0, 0, 0), 4: (1, 0, 0)}),
    ("split3_env_0", dict(env={"DIMSUM_SPLIT3": "0"}), {1: (0, 0, 0), 4: (0, 0, 0)}),
    ("own_gemm_env_0", dict(env={"DIMSUM_GEMM_NT": "0"}), {1: (0, 0, 0), 4: (0, 0, 0)}),
    ("rows_not_256", dict(rows=8320, seqlen=64), {1: (0, 0, 0), 4: (0, 0, 0)}),
    ("seqlen_not_32", dict(rows=8448, seqlen=48), {1: (0, 0, 0), 4: (1, 0, 0)}),
    ("seqlen_not_32_planes_env_1", dict(rows=8448, seqlen=48, env={"DIMSUM_OUT_PROJ_PLANES": "1"}), {1: (1, 0, 0), 4: (1, 0, 0)}),
    ("n_out_576", dict(n_out=576), {1: (0, 0, 0), 4: (0, 0, 1)}),
    ("n_out_258", dict(n_out=258), {1: (0, 0, 0), 4: (0, 0, 0)}),
    ("D_64", dict(D=64), {1: (0, 0, 0), 4: (0, 0, 0)}),
    ("D_160", dict(D=160), {1: (0, 0, 0), 4: (0, 0, 0)}),
    ("D_4096", dict(D=4096), {1: (0, 1, 0), 4: (1, 0, 1)}),
    ("D_4160", dict(D=4160), {1: (0, 1, 0), 4: (1, 0, 0)}),
    ("base_pointer_misaligned", dict(ptr=4100), {1: (0, 0, 0), 4: (0, 0, 0)}),
    ("row_stride_not_4", dict(stride=(256 * 258, 258, 1)), {1: (0, 0, 0), 4: (0, 0, 0)}),
    ("batch_stride_not_4", dict(stride=(256 * 256 + 2, 256, 1)), {1: (0, 0, 0), 4: (0, 0, 0)}),
    ("last_stride_not_1", dict(stride=(256 * 512, 512, 2)), {1: (0, 0, 0), 4: (0, 0, 0)}),
    ("rows_at_min_rows", dict(env={"DIMSUM_SPLIT3_MIN_ROWS": "8192"}), {1: (0, 1, 0), 4: (1, 0, 1)}),
    ("rows_one_below_min_rows", dict(env={"DIMSUM_SPLIT3_MIN_ROWS": "8193"}), {1: (0, 0, 0), 4: (0, 0, 0)}),
    ("rows_below_default_min_rows", dict(rows=7936), {1: (0, 0, 0), 4: (0, 0, 0)}),
    ("min_rows_256", dict(rows=256, env={"DIMSUM_SPLIT3_MIN_ROWS": "256"}), {1: (0, 1, 0), 4: (1, 0, 1)}),
    ("last_rows_inside_32_bits", dict(rows=2 ** 24 - 256), {1: (0, 1, 0), 4: (1, 0, 1)}),
    ("first_rows_past_32_bits", dict(rows=2 ** 24), {1: (0, 0, 0), 4: (0, 0, 0)}),
    ("xz_bf16", dict(xz_dtype=torch.bfloat16), {1: (0, 0, 0), 4: (0, 0, 0)}),
    ("weight_bf16", dict(w_dtype=torch.bfloat16), {1: (0, 0, 0), 4: (0, 0, 0)}),
    ("weight_last_stride_not_1", dict(w_t=True), {1: (0, 0, 0), 4: (0, 0, 0)}),
    ("xz_not_on_the_gpu", dict(is_cuda=False), {1: (0, 0, 0), 4: (0, 0, 0)}),
]
CASES = [pytest.param(over, k, want[k], id=f"{name}-k{k}") for name, over, want in TABLE for k in (1, 4)]


@pytest.fixture
def call(monkeypatch):
    """sets policy, allow_tf32 and the environment of a case (restored afterwards) and returns its operands"""
    old_policy = gemm.get_policy()

    def make(over):
        c = dict(BASE, **over)
        for name in ENV:
            monkeypatch.delenv(name, raising=False)
        for name, value in c["env"].items():
            monkeypatch.setenv(name, value)
        monkeypatch.setattr(torch.backends.cuda.matmul, "allow_tf32", c["tf32"])
        gemm.set_policy(c["policy"])
        bsz, d2, L = c["rows"] // c["seqlen"], 2 * c["D"], c["seqlen"]
        xz = _XZ((bsz, d2, L), c["stride"] or (d2 * L, L, 1), c["ptr"], c["xz_dtype"], c["is_cuda"])
        w = torch.empty(c["n_out"], c["D"], dtype=c["w_dtype"]) if not c["w_t"] else torch.empty(c["D"], c["n_out"], dtype=c["w_dtype"]).t()
        return xz, w, c["rows"], c["seqlen"]
    yield make
    gemm.set_policy(old_policy)


def _caller_route(planes, f16, conv):
    """the precedence _MambaInner.forward gives the three: conversion, then planes, then fp16 from the scan"""
    return "f16_convert" if conv else "planes" if planes else "f16_scan" if f16 else "none"


@pytest.mark.parametrize("over,scan_kernel,want", CASES)
def test_the_three_predicates(call, over, scan_kernel, want):
    xz, w, rows, seqlen = call(over)
    got = (gemm.out_proj_planes_enabled(xz, w, rows, scan_kernel), gemm.out_proj_f16_enabled(xz, w, rows, seqlen, scan_kernel),
           gemm.out_proj_f16_convert_enabled(xz, w, rows, seqlen, scan_kernel))
    assert tuple(map(bool, got)) == tuple(map(bool, want))
    assert not (got[1] and got[2]), "both fp16 routes at once"
    p, f, c = want
    assert _caller_route(*got) == ("f16_convert" if c else "planes" if p else "f16_scan" if f else "none")


@pytest.mark.parametrize("over,scan_kernel,want", CASES)
def test_the_route_function(call, over, scan_kernel, want):
    """gemm.out_proj_route, the one function behind the three predicates: the caller's precedence over the same table"""
    xz, w, rows, seqlen = call(over)
    assert gemm.out_proj_route(xz, w, rows, seqlen, scan_kernel) == _caller_route(*want)


def test_default_scan_kernel_is_the_64_channel_one(call):
    xz, w, rows, seqlen = call({})
    assert gemm.out_proj_f16_enabled(xz, w, rows, seqlen) and not gemm.out_proj_planes_enabled(xz, w, rows)
