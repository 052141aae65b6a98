"""tools/bench_moe_train.py (GPU box): one SwitchMLP forward + backward at the DiM-L/2 MoE layer's shape -- 65536 tokens x 1024 channels, 8 gated
experts, float32 -- on the slice GEMMs (_SwitchMlpFn: one host read of the offsets, 6 E library GEMM launches) and on the grouped GEMM with its two
gradients (grouped_train=True, csrc/moe_gemm_bwd.hip: no host read, 6 launches), in the same process on the same weights and inputs. The two
variants alternate window by window (machines and minutes differ by several per cent: only figures taken next to each other compare); device
events around windows of steps after a warm-up, minimum and median over the windows. Also per variant: the host time to ISSUE a step (wall clock
from a drained queue to the return of backward(), no synchronisation of the script's own: the slice path's includes its wait for the offsets), and the
number of kernel launches of one step as the profiler counts them. Prints figures only: no threshold is asserted anywhere.
[--tokens N --dim H --experts E --bias --tf32/--no-tf32]"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dimsum_amd.switch_mlp import SwitchMLP  # noqa: E402


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def issue_ms(fn, n=5):
    t = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
    return sorted(t)[n // 2]


def launches(fn):
    """kernel launches of one call, or None where the profiler records no device activity"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in ev.name.lower() and "memset" not in ev.name.lower())
    return n or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=65536)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--experts", type=int, default=8)
    ap.add_argument("--bias", action="store_true")
    ap.add_argument("--tf32", action=argparse.BooleanOptionalAction, default=True, help="torch.backends.cuda.matmul.allow_tf32 (train.py's default)")
    ap.add_argument("--steps", type=int, default=3, help="steps per window")
    ap.add_argument("--rounds", type=int, default=5, help="windows per variant")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_moe_train.py needs the GPU"
    torch.backends.cuda.matmul.allow_tf32 = args.tf32
    T, H, E = args.tokens, args.dim, args.experts
    torch.manual_seed(0)
    m = SwitchMLP(H, layer_idx=1, num_moe_experts=E, add_bias_linear=args.bias).cuda()
    x = torch.randn(1, T, H, device="cuda", requires_grad=True)
    dout = torch.randn_like(x)

    def step(on):
        def run():
            m.set_grouped_train(on)
            m.zero_grad(set_to_none=True)
            x.grad = None
            m(x).backward(dout)
        return run

    variants = {"slice GEMMs": step(False), "grouped_train": step(True)}
    grads = {}
    for name, fn in variants.items():              # warm-up (the library picks its kernels here), and the two paths' agreement
        for _ in range(3):
            fn()
        grads[name] = [x.grad.clone()] + [p.grad.clone() for p in m.parameters()]
    worst = max(((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item() for a, b in zip(grads["grouped_train"], grads["slice GEMMs"]))
    print(f"SwitchMLP forward + backward, {T} x {H}, {E} experts, float32, allow_tf32 {args.tf32}; max over the gradients of max |grouped - slices| / max |slices| = {worst:.3e}")
    times = {name: [] for name in variants}
    for _ in range(args.rounds):                   # alternate: a drift of the machine falls on both
        for name, fn in variants.items():
            times[name].append(window(fn, args.steps))
    for name, fn in variants.items():
        t = sorted(times[name])
        print(f"  {name:14s} min {t[0]:8.3f} ms  median {t[len(t) // 2]:8.3f} ms per step   host issue {issue_ms(fn):8.3f} ms   kernel launches {launches(fn)}")


if __name__ == "__main__":
    main()
