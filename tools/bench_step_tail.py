#!/usr/bin/env python3
"""Micro-benchmark of the training-step tail at DiM-L/2's parameter list (GPU box). In ONE process, interleaved, after warm-up, by device events:
  (a) torch: clip_grad_norm_ -> AdamW(fused=True).step() -> update_ema, exactly as train_step runs them by default;
  (b) fused: FusedAdamWEMA.step_fused (dimsum_optim_grad_sumsq + dimsum_optim_adamw_ema_step);
  (c) step:  FusedAdamWEMA.step() with the EMA on: the counter launch + the update kernel without the norm pass, i.e. the update kernel's time.
Every timed call gets gradient tensors allocated just before it (clones made outside the timed window), so (b) and (c) include the refresh of the
gradient pointer table. The shapes come from the model built on the meta device; values are synthetic.
Prints one JSON line: median / min / max milliseconds of each, fused / torch, the spread of (a), and the update kernel's achieved bytes per second
(9 fp32 streams: reads g, p, m, v, ema, writes p, m, v, ema) against 6.3 TB/s."""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dimsum_amd.optim import FusedAdamWEMA  # noqa: E402
from dimsum_amd.train import update_ema  # noqa: E402

ACHIEVABLE = 6.3e12


class Bag(torch.nn.Module):
    def __init__(self, shapes, gen):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(s, device="cuda", generator=gen) * 0.02) for s in shapes])


def shapes_of(name):
    from dimsum_amd.create_model import create_model, published_config
    with torch.device("meta"):
        m = create_model(published_config(name, 256, 1000))
    return [tuple(p.shape) for p in m.parameters()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="DiM-L/2")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-grad-norm", type=float, default=2.0)
    ap.add_argument("--ema-decay", type=float, default=0.9999)
    a = ap.parse_args()
    shapes = shapes_of(a.model)
    n = sum(int(torch.Size(s).numel()) for s in shapes)
    gen = torch.Generator(device="cuda").manual_seed(0)
    net_t = Bag(shapes, gen)
    net_f, net_s = copy.deepcopy(net_t), copy.deepcopy(net_t)
    ema_t, ema_f, ema_s = (copy.deepcopy(net_t).requires_grad_(False) for _ in range(3))
    grads = [torch.randn(s, device="cuda", generator=gen) for s in shapes]
    opt_t = torch.optim.AdamW(net_t.parameters(), lr=1e-4, weight_decay=0, fused=True)
    opt_f = FusedAdamWEMA(net_f.parameters(), lr=1e-4, weight_decay=0)
    opt_f.attach_ema(net_f, ema_f)
    opt_s = FusedAdamWEMA(net_s.parameters(), lr=1e-4, weight_decay=0)
    opt_s.attach_ema(net_s, ema_s, decay=a.ema_decay)

    def torch_tail():
        torch.nn.utils.clip_grad_norm_(net_t.parameters(), a.max_grad_norm)
        opt_t.step()
        update_ema(ema_t, net_t, a.ema_decay)

    runs = {"torch": (net_t, torch_tail), "fused": (net_f, lambda: opt_f.step_fused(a.max_grad_norm, a.ema_decay)), "step": (net_s, opt_s.step)}
    times = {k: [] for k in runs}
    for it in range(a.warmup + a.iters):
        for name, (net, fn) in runs.items():
            for p, g in zip(net.ps, grads):
                p.grad = g.clone()                                   # a new allocation, like autograd's after zero_grad(set_to_none=True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
            for p in net.ps:
                p.grad = None
    # the same gradients went through both: the results must agree (fp32 rounding apart)
    diff = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(net_t.ps, net_f.ps))
    ediff = max(float((p - q).abs().max()) for p, q in zip(ema_t.ps, ema_f.ps))
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"tool": "bench_step_tail", "model": a.model, "tensors": len(shapes), "elements": n, "iters": a.iters}
    for k, v in times.items():
        out[k + "_ms"] = {"median": round(med[k], 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    out["fused_over_torch"] = round(med["fused"] / med["torch"], 4)
    out["torch_spread"] = round((max(times["torch"]) - min(times["torch"])) / med["torch"], 4)
    out["update_kernel_bytes_per_s"] = round(9 * 4 * n / (med["step"] * 1e-3), 0)
    out["update_kernel_share_of_6.3TBps"] = round(9 * 4 * n / (med["step"] * 1e-3) / ACHIEVABLE, 4)
    out["norm_pass_ms"] = round(med["fused"] - med["step"], 4)
    out["norm_pass_bytes_per_s"] = round(4 * n / max((med["fused"] - med["step"]) * 1e-3, 1e-9), 0)
    out["max_abs_diff_p"], out["max_abs_diff_ema"] = diff, ediff
    print(json.dumps(out))


if __name__ == "__main__":
    main()
