"""tools/bench_dit.py (GPU box): the plain MLP's HIP path and the DiT baseline on it, in one process --
  1. the bias + GELU row pass (csrc/act_rows.hip) at (65536, 4096): forward (fp32 and the scaled-fp16 image) and backward, microseconds and GB/s of
     algorithmic traffic, next to the torch-eager expression;
  2. fc1 + GELU epilogue (DIMSUM_GEMM_EPI_GELU_F16) at 65536 x (1024 -> 4096) against the F32_BIAS GEMM + the row pass writing the same image;
  3. one DiT-L/2 inference forward at batch 256 under the scaled-fp16 policy and in exact fp32.
Device events around windows of calls, the arms alternating, minimum and median over the windows. Reads nothing outside the repository."""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dimsum_amd import gemm, native  # noqa: E402
from dimsum_amd.models_dit import DiT_models  # noqa: E402


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def compare(arms, n=20, rounds=7, bytes_of=None):
    """arms: {name: fn}; alternating windows so that all arms see the same neighbours on the machine"""
    for fn in arms.values():
        for _ in range(3):
            fn()
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            times[k].append(window(fn, n))
    for k, t in times.items():
        t.sort()
        gbs = f" ({bytes_of[k] / t[0] / 1e3:6.0f} GB/s)" if bytes_of and k in bytes_of else ""
        print(f"    {k:34s} {t[0]:9.1f} us min {t[rounds // 2]:9.1f} median{gbs}", flush=True)


def main():
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)      # noqa: E731
    M, K, H = 65536, 1024, 4096
    x, dh, bias = rnd(M, H), rnd(M, H), 0.1 * rnd(H)
    e = M * H
    print(f"row pass ({M}, {H})")
    compare({"gelu_fwd fp32": lambda: native.gelu_fwd(x, bias), "gelu_fwd f16s image": lambda: native.gelu_fwd(x, bias, split3="f16s"),
             "torch F.gelu(x + b)": lambda: F.gelu(x + bias, approximate="tanh")},
            bytes_of={"gelu_fwd fp32": 8 * e, "gelu_fwd f16s image": 6 * e})
    compare({"gelu_bwd fp32 + dbias": lambda: native.gelu_bwd(x, bias, dh), "gelu_bwd f16s image + dbias": lambda: native.gelu_bwd(x, bias, dh, split3="f16s")},
            bytes_of={"gelu_bwd fp32 + dbias": 12 * e, "gelu_bwd f16s image + dbias": 10 * e})
    del x, dh
    print(f"fc1 ({M}, {K} -> {H}), scaled-fp16 operands")
    x16 = native.rows_f16s(rnd(M, K))
    w16, l1 = native.rows_f16s(rnd(H, K) * K ** -0.5, want_l1=True)
    bound = torch.cat([l1 * gemm._K10, bias.abs().max().reshape(1)]).contiguous()
    sc = (x16.inv, w16.inv)
    compare({"GEMM with the GELU epilogue": lambda: native.gemm_nt(x16.data, w16.data, bias=bias, epilogue="gelu_f16", scales=sc, gate_bound=bound),
             "GEMM (F32_BIAS) + row pass": lambda: native.gelu_fwd(native.gemm_nt(x16.data, w16.data, bias=bias, scales=sc), None, split3="f16s", scales=(x16.inv, bound))})
    del x16, w16
    print("DiT-L/2 forward, batch 256, 256 px")
    model = DiT_models["DiT-L/2"](input_size=32).cuda().eval()
    with torch.no_grad():
        for p in model.parameters():                # (adaLN-zero would multiply every branch by 0: same kernels, but keep the values alive)
            if torch.count_nonzero(p) == 0:
                p.normal_(std=0.02, generator=g)
    z, t, y = rnd(256, 4, 32, 32), torch.rand(256, device="cuda", generator=g), torch.randint(0, 1000, (256,), device="cuda", generator=g)

    def forward(policy, tf32):
        def run():
            old = torch.backends.cuda.matmul.allow_tf32
            torch.backends.cuda.matmul.allow_tf32 = tf32
            gemm.set_policy(policy)
            try:
                with torch.no_grad():
                    model(z, t, y)
            finally:
                gemm.set_policy("default")
                torch.backends.cuda.matmul.allow_tf32 = old
        return run
    compare({"f16s policy": forward("f16s", True), "allow_tf32 (split-bf16 images)": forward("default", True), "exact fp32": forward("default", False)}, n=3, rounds=5)


if __name__ == "__main__":
    main()
