#!/usr/bin/env python3
"""The LM training loss at the Mamba-130m head shape (d = 768, V = 50280 in a weight padded to 50288 rows, M = 8192 tokens), float32 and
bfloat16, the HIP path (csrc/cross_entropy.hip) against torch's, the two alternating round by round in one process:

  (a) cross_entropy_loss forward + backward against F.cross_entropy forward + backward on the same materialised logits (reduction "mean"),
      and each kernel alone with its achieved bytes/s -- M * V * sizeof(T) for the forward's one read, twice that for the backward's read
      and write -- next to the HBM peak (8.0 TB/s by specification, about 6.3 TB/s achievable by a float4 copy);
  (b) linear_cross_entropy against lm_head + F.cross_entropy, forward + backward from the hidden states: time and the rise of
      torch.cuda.max_memory_allocated over the call.

Times are device times between two events around `--iters` back-to-back calls after a warm-up of each side; the median of `--rounds` rounds
and the spread max / min of the rounds.

    python tools/bench_lm_loss.py [--rows 8192] [--rounds 5] [--iters 5] [--out lm_loss_bench.json]
prints one JSON line per measurement and a markdown table at the end."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D, V, VP = 768, 50280, 50288
HBM_PEAK_TBS, HBM_COPY_TBS = 8.0, 6.3


def device_ms(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def alternate(sides, rounds, iters):
    """{name: fn} -> {name: (median ms, spread)}: a warm-up of each side, then `rounds` rounds in which the sides take turns"""
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            times[k].append(device_ms(fn, iters))
    return {k: (statistics.median(v), max(v) / min(v)) for k, v in times.items()}


def peak_rise(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--chunk-rows", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lm_loss needs the GPU"
    from dimsum_amd import native
    from dimsum_amd.ops import CrossEntropyLoss, linear_cross_entropy
    M = args.rows
    out = []
    for dtype in (torch.float32, torch.bfloat16):
        name, size = str(dtype).split(".")[-1], torch.empty((), dtype=dtype).element_size()
        g = torch.Generator("cuda").manual_seed(0)
        hidden = torch.randn(M, D, device="cuda", generator=g).to(dtype)
        weight = (torch.randn(VP, D, device="cuda", generator=g) * D ** -0.5).to(dtype)
        labels = torch.randint(0, V, (M,), device="cuda", generator=g)
        labels[::97] = -100
        logits = F.linear(hidden, weight)[:, :V]                                # the [..., :vocab] view of the padded logits, as a model has it
        # ---- (a) the loss on materialised logits ----
        ours_loss, one = CrossEntropyLoss(), torch.ones(M, device="cuda")

        def ours():
            x = logits.detach().requires_grad_()
            ours_loss(x, labels).backward()

        def torch_path():
            x = logits.detach().requires_grad_()
            F.cross_entropy(x, labels).backward()

        r = alternate({"hip": ours, "torch": torch_path}, args.rounds, args.iters)
        lse = native.cross_entropy_fwd(logits, labels)[1]
        k = alternate({"fwd": lambda: native.cross_entropy_fwd(logits, labels),
                       "bwd": lambda: native.cross_entropy_bwd(one, logits, lse, labels)}, args.rounds, args.iters)
        row = dict(what="loss fwd+bwd on logits", dtype=name, rows=M, hip_ms=round(r["hip"][0], 3), torch_ms=round(r["torch"][0], 3),
                   torch_over_hip=round(r["torch"][0] / r["hip"][0], 2), spread_hip=round(r["hip"][1], 3), spread_torch=round(r["torch"][1], 3),
                   fwd_kernel_ms=round(k["fwd"][0], 3), fwd_tb_s=round(M * V * size / k["fwd"][0] / 1e9, 2),
                   bwd_kernel_ms=round(k["bwd"][0], 3), bwd_tb_s=round(2 * M * V * size / k["bwd"][0] / 1e9, 2),
                   hbm_peak_tb_s=HBM_PEAK_TBS, hbm_copy_tb_s=HBM_COPY_TBS)
        out.append(row)
        print(json.dumps(row), flush=True)
        del logits, lse
        # ---- (b) from the hidden states ----
        def chunked():
            h, w = hidden.detach().requires_grad_(), weight.detach().requires_grad_()
            linear_cross_entropy(h, w, labels, chunk_rows=args.chunk_rows, vocab_size=V).backward()

        def materialised():
            h, w = hidden.detach().requires_grad_(), weight.detach().requires_grad_()
            F.cross_entropy(F.linear(h, w)[:, :V], labels).backward()

        r = alternate({"hip": chunked, "torch": materialised}, args.rounds, max(1, args.iters // 2))
        mem = {"hip": peak_rise(chunked), "torch": peak_rise(materialised)}
        row = dict(what="head + loss fwd+bwd from hidden", dtype=name, rows=M, chunk_rows=args.chunk_rows, hip_ms=round(r["hip"][0], 3),
                   torch_ms=round(r["torch"][0], 3), torch_over_hip=round(r["torch"][0] / r["hip"][0], 2), spread_hip=round(r["hip"][1], 3),
                   spread_torch=round(r["torch"][1], 3), hip_peak_mb=round(mem["hip"] / 1e6, 1), torch_peak_mb=round(mem["torch"] / 1e6, 1))
        out.append(row)
        print(json.dumps(row), flush=True)
        del hidden, weight
        torch.cuda.empty_cache()
    print("\n| what | dtype | HIP ms | torch ms | torch / HIP | notes |\n|---|---|---|---|---|---|")
    for r in out:
        note = (f"fwd kernel {r['fwd_kernel_ms']} ms = {r['fwd_tb_s']} TB/s, bwd kernel {r['bwd_kernel_ms']} ms = {r['bwd_tb_s']} TB/s" if "fwd_tb_s" in r
                else f"peak rise {r['hip_peak_mb']:.0f} MB vs {r['torch_peak_mb']:.0f} MB")
        print(f"| {r['what']} | {r['dtype']} | {r['hip_ms']} | {r['torch_ms']} | {r['torch_over_hip']} | {note} |")
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
