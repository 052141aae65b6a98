#!/usr/bin/env python3
"""Decode throughput of the Mamba language model: the fused decode step (csrc/decode_step.hip) against DIMSUM_FUSED_DECODE=0 (the unfused
step: the parent's step kernels plus the BLAS GEMVs -- the baseline), in one process, the two alternating round by round.

Model: a random-init Mamba-130m shape (d_model 768, n_layer 24, vocab 50280 padded to a multiple of 8, rms_norm, fused_add_norm,
residual_in_fp32). For batch in {1, 8, 16} x {float32, bfloat16} x {eager, graph-captured}: tokens/s = batch * steps / wall time of `steps`
decode steps between two device synchronisations (greedy sampling outside the graph, as generate() runs it), the median of `--rounds`
rounds per path after a warm-up round of each. Both paths decode the same tokens from the same prompt and their logits are compared first.

    python tools/bench_decode.py [--steps 256] [--rounds 5] [--out decode_bench.json]
prints one JSON line per configuration and a markdown table at the end.

With --fused-sampling {0,1,both} the tool measures the SAMPLER instead (DIMSUM_FUSED_DECODE left as it is): generate() of `steps` tokens under
--top-k / --top-p / --temperature with the fused sampler (csrc/sample_logits.hip; under cg inside the captured step) and with the unfused
`sample` (the baseline), alternating round by round when both are asked for; tokens/s = batch * steps / wall time of the whole call between
two device synchronisations, the prompt's forward included on both sides. It ends with the sampler kernel's time per launch on (batch, 50280)
logits: device events around 200 back-to-back launches.

    python tools/bench_decode.py --fused-sampling both --top-k 50 --top-p 0.9 [--batches 1 8] [--dtypes float32 bfloat16] [--modes eager graph]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPE = dict(d_model=768, n_layer=24, vocab_size=50280, pad_vocab_size_multiple=8, rms_norm=True, fused_add_norm=True, residual_in_fp32=True)
PROMPT = 16


def timed_decode(model, prompt, steps, cg, fused):
    """-> (seconds for `steps` decode steps, the last step's logits)"""
    from dimsum_amd.utils import InferenceParams
    from dimsum_amd.utils.generation import update_graph_cache
    os.environ["DIMSUM_FUSED_DECODE"] = "1" if fused else "0"
    batch = prompt.shape[0]
    max_len = PROMPT + steps + 1
    with torch.no_grad():
        if cg:
            cache = model._caches.get(fused)
            cache = model._caches[fused] = update_graph_cache(model, cache, batch, PROMPT, max_len)      # one cache (and capture) per path
            params = cache.params_for(batch)
            params.reset(max_len, batch)
        else:
            params = InferenceParams(max_seqlen=max_len, max_batch_size=batch)
        logits = model(prompt, inference_params=params, num_last_tokens=1).logits[:, -1]
        params.seqlen_offset = PROMPT
        tok = logits.argmax(-1, keepdim=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            if cg:
                logits = cache.run(tok, params.seqlen_offset)[:, 0]
            else:
                logits = model(tok, inference_params=params, num_last_tokens=1).logits[:, 0]
            params.seqlen_offset += 1
            tok = logits.argmax(-1, keepdim=True)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, logits


def timed_generate(model, prompt, steps, cg, fused_sampling, args):
    """-> (seconds for generate() of `steps` tokens, the sequences)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    seq = model.generate(prompt, max_length=PROMPT + steps, cg=cg, top_k=args.top_k, top_p=args.top_p, temperature=args.temperature,
                         vocab_size=SHAPE["vocab_size"], fused_sampling=fused_sampling, generator=torch.Generator("cuda").manual_seed(1))
    torch.cuda.synchronize()
    return time.perf_counter() - t0, seq


def sampler_kernel_time(args, dtype, batch, launches=200):
    """-> microseconds per sample_logits launch on (batch, 50280) logits read through the padded row stride"""
    from dimsum_amd import native
    V = SHAPE["vocab_size"]
    g = torch.Generator("cuda").manual_seed(0)
    logits = (torch.randn(batch, V + 8, device="cuda", generator=g) * 4).to(dtype)[:, :V]
    u = torch.rand(batch, device="cuda", generator=g)
    out = torch.empty(batch, dtype=torch.long, device="cuda")
    kw = dict(top_k=args.top_k, top_p=args.top_p, temperature=args.temperature, out=out)
    for _ in range(10):
        native.sample_logits(logits, u, **kw)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(launches):
        native.sample_logits(logits, u, **kw)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / launches


def sampling_bench(args):
    from dimsum_amd.models.mixer_seq_simple import MambaLMHeadModel
    sides = {"0": [False], "1": [True], "both": [True, False]}[args.fused_sampling]
    setting = dict(top_k=args.top_k, top_p=args.top_p, temperature=args.temperature)
    rows = []
    for name in args.dtypes:
        dtype = getattr(torch, name)
        torch.manual_seed(0)
        model = MambaLMHeadModel(**SHAPE, device="cuda", dtype=dtype).eval()
        for batch in args.batches:
            prompt = torch.randint(0, SHAPE["vocab_size"], (batch, PROMPT), device="cuda", generator=torch.Generator("cuda").manual_seed(batch))
            for mode in args.modes:
                cg = mode == "graph"
                model._decoding_cache = None
                for f in sides:                                                 # warm-up (and capture)
                    timed_generate(model, prompt, min(args.steps, 32), cg, f, args)
                    timed_generate(model, prompt, args.steps, cg, f, args)
                times = {f: [] for f in sides}
                for _ in range(args.rounds):
                    for f in sides:
                        times[f].append(timed_generate(model, prompt, args.steps, cg, f, args)[0])
                row = dict(setting, dtype=name, batch=batch, mode=mode, steps=args.steps, rounds=args.rounds)
                for f in sides:
                    side = "fused" if f else "unfused"
                    row[f"{side}_tokens_per_s"] = round(batch * args.steps / statistics.median(times[f]), 1)
                    row[f"spread_{side}"] = round(max(times[f]) / min(times[f]), 3)
                if len(sides) == 2:
                    row["ratio"] = round(row["fused_tokens_per_s"] / row["unfused_tokens_per_s"], 3)
                rows.append(row)
                print(json.dumps(row), flush=True)
            model._decoding_cache = None
            row = dict(setting, dtype=name, batch=batch, sampler_kernel_us_per_launch=round(sampler_kernel_time(args, dtype, batch), 1))
            rows.append(row)
            print(json.dumps(row), flush=True)
        del model
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 8, 16])
    ap.add_argument("--out", default=None)
    ap.add_argument("--fused-sampling", choices=["0", "1", "both"], default=None, help="measure the sampler: fused, unfused or the two alternating")
    ap.add_argument("--top-k", type=int, default=1)
    ap.add_argument("--top-p", type=float, default=0.0)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--dtypes", nargs="*", default=["float32", "bfloat16"])
    ap.add_argument("--modes", nargs="*", choices=["eager", "graph"], default=["eager", "graph"])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_decode needs the GPU"
    if args.fused_sampling is not None:
        return sampling_bench(args)
    from dimsum_amd.models.mixer_seq_simple import MambaLMHeadModel
    rows = []
    for dtype in (torch.float32, torch.bfloat16):
        torch.manual_seed(0)
        model = MambaLMHeadModel(**SHAPE, device="cuda", dtype=dtype).eval()
        for batch in args.batches:
            prompt = torch.randint(0, SHAPE["vocab_size"], (batch, PROMPT), device="cuda", generator=torch.Generator("cuda").manual_seed(batch))
            for cg in (False, True):
                model._caches = {}
                warm = {f: timed_decode(model, prompt, min(args.steps, 32), cg, f)[1] for f in (True, False)}     # warm-up (and capture)
                diff = (warm[True].float() - warm[False].float()).abs().max().item()
                times = {True: [], False: []}
                for _ in range(args.rounds):
                    for f in (True, False):
                        times[f].append(timed_decode(model, prompt, args.steps, cg, f)[0])
                tps = {f: batch * args.steps / statistics.median(times[f]) for f in times}
                row = dict(dtype=str(dtype).split(".")[-1], batch=batch, mode="graph" if cg else "eager", fused_tokens_per_s=round(tps[True], 1),
                           unfused_tokens_per_s=round(tps[False], 1), ratio=round(tps[True] / tps[False], 3),
                           spread_fused=round(max(times[True]) / min(times[True]), 3), spread_unfused=round(max(times[False]) / min(times[False]), 3),
                           max_logit_diff=diff, steps=args.steps, rounds=args.rounds)
                rows.append(row)
                print(json.dumps(row), flush=True)
                model._caches = {}
        del model
        torch.cuda.empty_cache()
    print("\n| dtype | batch | mode | fused tok/s | unfused tok/s | fused / unfused |\n|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['dtype']} | {r['batch']} | {r['mode']} | {r['fused_tokens_per_s']:.0f} | {r['unfused_tokens_per_s']:.0f} | {r['ratio']:.2f} |")
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
