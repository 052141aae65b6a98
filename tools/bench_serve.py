#!/usr/bin/env python3
"""Serving throughput of the Mamba language model on a ragged workload: continuous batching (dimsum_amd.utils.serving.DecodeEngine, a slot
pool and ONE captured step for every membership) against static batches through generate(cg=True), in one process, the two alternating
round by round; then the time of one captured decode step with and without the slot index at equal batch.

Model: a random-init Mamba-130m shape, as tools/bench_decode.py. Workload, seeded: `--requests` (64) requests, prompts of 16..128 tokens,
16..256 new tokens each, greedy, no eos (every request runs to its length, so both sides produce the same number of USEFUL tokens: the sum
of the requests' new tokens).
  (a) engine: DecodeEngine(max_batch=B, num_slots=B, cg=True): all requests submitted, run() until idle. Each prompt is prefilled alone.
  (b) static: the requests in submission order in batches of B through generate(cg=True, fused_sampling=True), prompts left-padded to the
      batch's longest with the padding as a segment of its own (seq_idx), each batch decoding to its longest member: the tokens a shorter
      member produces beyond its own length are waste.
Both sides sample with the fused sampler inside the captured step. Useful tokens/s = useful tokens / wall time between two device
synchronisations, prompt passes included on both sides; the median of `--rounds` rounds after one warm-up round of each (captures, the graph
cache grown to its final size). DIMSUM_FUSED_DECODE is left as the caller set it (unset: the fused step for float32 at batch <= 4).

Step time: the model's forward on a (B, 1) token buffer at seqlen_offset > 0 captured twice -- on a cache of B rows, and on a pool of B slots
with state_indices = a permutation of 0..B-1 -- `--steps` replays each between two synchronisations, alternating, median of `--rounds`,
with DIMSUM_FUSED_DECODE=1 and =0. The un-indexed kernels are the parent commit's instruction for instruction, so the
first of the two is the parent's step.

--packed-prefill off (default): the engine admits every prompt alone, as above. on: the engine of (a) runs DecodeEngine(packed_prefill=True).
both: instead of the two comparisons above, the engine with packed admission against the same engine with alone admission on the same
workload (alternating round by round after a warm-up round of each; median and max / min spread of `--rounds`), then an admission-only
timing: k = 1, 4, 16 prompts of 64 tokens admitted into an idle engine of max_batch 16, packed against alone, between two synchronisations.

--chunked-prefill both: chunked admission (DecodeEngine(chunked_prefill=True)) against unchunked packed admission at the same
--max-prefill-tokens, alternating in one process, on the workload with --long-prompts prompts of --long-len tokens among the short ones:
useful tok/s and the LARGEST single step() wall time (the decode stall), median of --rounds with the spread.
--shared-prefix P (on top of --chunked-prefill on): every request's prompt is one common P-token prefix plus its own tail (the workload's
prompt). Two engines with chunked admission alternate round by round in one process: "full" submits the full prompts, so every request
prefills the prefix again; "held" prefills it once (`hold`) and submits the tails as forks (`start=`), one state-copy launch per admission. Wall
times (median, max / min spread) and the prompt tokens that went through the model on each side; then one dimsum_state_copy_slots timing:
100 launches of 8 pairs on this model's pool between two device events, beside the same copies made layer by layer with index_copy_.
    python tools/bench_serve.py [--batches 4 16] [--rounds 5] [--requests 64] [--dtype float32] [--packed-prefill off|on|both]
                                [--chunked-prefill off|on|both --max-prefill-tokens 512 --long-prompts 4 --long-len 4096] [--shared-prefix 1024]
                                [--out serve_bench.json]
prints one JSON line per measurement and two markdown tables at the end."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPE = dict(d_model=768, n_layer=24, vocab_size=50280, pad_vocab_size_multiple=8, rms_norm=True, fused_add_norm=True, residual_in_fp32=True)
PROMPT_RANGE, NEW_RANGE = (16, 128), (16, 256)


def workload(n_requests, seed=0, vocab=SHAPE["vocab_size"]):
    """-> [(prompt (L,) int64 on the host, new tokens)]: seeded, prompt lengths and new-token counts uniform over their ranges (inclusive)"""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(PROMPT_RANGE[0], PROMPT_RANGE[1] + 1, (n_requests,), generator=g).tolist()
    news = torch.randint(NEW_RANGE[0], NEW_RANGE[1] + 1, (n_requests,), generator=g).tolist()
    return [(torch.randint(0, vocab, (n,), generator=g), m) for n, m in zip(lens, news)]


def static_batches(requests, B):
    """-> [(ids (b, L) left-padded with token 0, seq_idx (b, L) int32, max_length)] of the requests in order, B at a time"""
    from dimsum_amd.utils import seq_idx_from_lengths
    out = []
    for i in range(0, len(requests), B):
        part = requests[i:i + B]
        L = max(p.numel() for p, _ in part)
        ids = torch.stack([torch.cat([p.new_zeros(L - p.numel()), p]) for p, _ in part])
        seq = torch.stack([seq_idx_from_lengths([L - p.numel(), p.numel()]) for p, _ in part])
        out.append((ids, seq, L + max(n for _, n in part)))
    return out


def run_engine(eng, requests):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rids = [eng.submit(p, n) for p, n in requests]
    out = eng.run()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert all(out[r].numel() == p.numel() + n for r, (p, n) in zip(rids, requests))
    eng.requests.clear()                                     # the results are out: the next round starts from an empty book
    return dt


def run_static(model, batches):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for ids, seq, max_length in batches:
        model.generate(ids, max_length=max_length, cg=True, fused_sampling=True, vocab_size=SHAPE["vocab_size"], seq_idx=seq)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def packed_bench(model, requests, B, rounds):
    """the engine with packed admission against the same engine with alone admission (the default), alternating round by round"""
    from dimsum_amd.utils.serving import DecodeEngine
    useful = sum(n for _, n in requests)
    kw = dict(max_batch=B, num_slots=B, max_seqlen=PROMPT_RANGE[1] + NEW_RANGE[1], vocab_size=SHAPE["vocab_size"], cg=True)
    engines = {"alone": DecodeEngine(model, packed_prefill=False, **kw), "packed": DecodeEngine(model, packed_prefill=True, **kw)}
    for eng in engines.values():
        run_engine(eng, requests)                            # warm-up round of each (the capture)
    times = {k: [] for k in engines}
    for _ in range(rounds):
        for k, eng in engines.items():
            times[k].append(run_engine(eng, requests))
    row = dict(batch=B, requests=len(requests), useful_tokens=useful, rounds=rounds,
               prompt_passes={k: eng.n_prefill_passes // (rounds + 1) for k, eng in engines.items()})
    for k, v in times.items():
        row[f"{k}_tokens_per_s"] = round(useful / statistics.median(v), 1)
        row[f"spread_{k}"] = round(max(v) / min(v), 3)
    row["packed_over_alone"] = round(row["packed_tokens_per_s"] / row["alone_tokens_per_s"], 3)
    return row


def run_engine_steps(eng, requests):
    """run_engine, step by step -> (wall time, the largest single step() wall time: what a live decode row waits behind an admission)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rids = [eng.submit(p, n) for p, n in requests]
    worst = 0.0
    while not eng.idle():
        t1 = time.perf_counter()
        eng.step()
        torch.cuda.synchronize()                             # a step without a live row returns before the host read: its prompt pass counts here
        worst = max(worst, time.perf_counter() - t1)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert all(eng.sequence(r).numel() == p.numel() + n for r, (p, n) in zip(rids, requests))
    eng.requests.clear()
    return dt, worst


def chunked_bench(model, requests, B, rounds, budget, long_prompts, long_len, seed=0):
    """chunked admission against unchunked packed admission at the same max_prefill_tokens, alternating round by round, on the workload
    with `long_prompts` prompts of `long_len` tokens put among the short ones (evenly spaced)"""
    from dimsum_amd.utils.serving import DecodeEngine
    g = torch.Generator().manual_seed(seed + 1)
    requests = list(requests)
    for i in range(long_prompts):
        at = (i + 1) * len(requests) // (long_prompts + 1)
        requests[at] = (torch.randint(0, SHAPE["vocab_size"], (long_len,), generator=g), requests[at][1])
    useful = sum(n for _, n in requests)
    kw = dict(max_batch=B, num_slots=B, max_seqlen=long_len + NEW_RANGE[1], vocab_size=SHAPE["vocab_size"], cg=True, packed_prefill=True,
              max_prefill_tokens=budget)
    engines = {"unchunked": DecodeEngine(model, **kw), "chunked": DecodeEngine(model, chunked_prefill=True, **kw)}
    for eng in engines.values():
        run_engine_steps(eng, requests)                      # warm-up round of each (the capture)
    times, worst = {k: [] for k in engines}, {k: [] for k in engines}
    for _ in range(rounds):
        for k, eng in engines.items():
            dt, w = run_engine_steps(eng, requests)
            times[k].append(dt)
            worst[k].append(w)
    row = dict(batch=B, requests=len(requests), useful_tokens=useful, rounds=rounds, max_prefill_tokens=budget, long_prompts=long_prompts,
               long_len=long_len, prompt_passes={k: eng.n_prefill_passes // (rounds + 1) for k, eng in engines.items()})
    for k in engines:
        row[f"{k}_tokens_per_s"] = round(useful / statistics.median(times[k]), 1)
        row[f"spread_{k}"] = round(max(times[k]) / min(times[k]), 3)
        row[f"{k}_max_step_ms"] = round(1e3 * statistics.median(worst[k]), 2)
        row[f"spread_max_step_{k}"] = round(max(worst[k]) / min(worst[k]), 3)
    row["chunked_over_unchunked"] = round(row["chunked_tokens_per_s"] / row["unchunked_tokens_per_s"], 3)
    return row


def shared_prefix_bench(model, requests, B, rounds, budget, P, seed=0):
    """one common P-token prefix in front of every prompt: full prompts (every request prefills the prefix) against one hold and forks, both
    with chunked admission under the same budget, alternating round by round"""
    from dimsum_amd.utils.serving import DecodeEngine
    prefix = torch.randint(0, SHAPE["vocab_size"], (P,), generator=torch.Generator().manual_seed(seed + 2))
    useful = sum(n for _, n in requests)
    kw = dict(max_batch=B, max_seqlen=P + PROMPT_RANGE[1] + NEW_RANGE[1], vocab_size=SHAPE["vocab_size"], cg=True, packed_prefill=True,
              max_prefill_tokens=budget, chunked_prefill=True)
    engines = {"full": DecodeEngine(model, num_slots=B, **kw), "held": DecodeEngine(model, num_slots=B + 1, **kw)}      # one slot more: the hold's

    def run(name):
        eng = engines[name]
        before = sum(eng.prefill_pass_tokens)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if name == "full":
            rids = [eng.submit(torch.cat([prefix, p]), n) for p, n in requests]
        else:
            h = eng.hold(prefix)
            rids = [eng.submit(p, n, start=h) for p, n in requests]
        eng.run()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert all(eng.context(r).numel() == P + p.numel() + n for r, (p, n) in zip(rids, requests))
        if name == "held":
            eng.release(h)
        eng.requests.clear()
        return dt, sum(eng.prefill_pass_tokens) - before

    for name in engines:
        run(name)                                            # warm-up round of each (the capture)
    times, tokens = {k: [] for k in engines}, {}
    for _ in range(rounds):
        for name in engines:
            dt, tokens[name] = run(name)
            times[name].append(dt)
    row = dict(batch=B, requests=len(requests), useful_tokens=useful, rounds=rounds, max_prefill_tokens=budget, shared_prefix=P, prefill_tokens=tokens)
    for k, v in times.items():
        row[f"{k}_s"] = round(statistics.median(v), 4)
        row[f"spread_{k}"] = round(max(v) / min(v), 3)
    row["full_over_held"] = round(row["full_s"] / row["held_s"], 3)
    return row


def state_copy_bench(model, pairs=8, launches=100, rounds=5):
    """dimsum_state_copy_slots (ONE launch for every layer) beside the same copies made layer by layer with index_copy_, on a pool of
    2 * pairs slots of this model: `launches` copies between two device events, alternating, median of `rounds` -> us per copy of `pairs` slots"""
    from dimsum_amd import native
    dtype = next(iter(model.parameters())).dtype
    pool = model.allocate_inference_cache(2 * pairs, 8, dtype)
    table = native.state_pool_table(pool)
    src, dst = torch.arange(pairs, device="cuda"), torch.arange(pairs, 2 * pairs, device="cuda")
    dev_pairs = torch.stack([src, dst], 1).to(torch.int32)

    def per_layer():
        for states in pool.values():
            for t in states:
                t.index_copy_(0, dst, t.index_select(0, src))
    sides = {"state_copy_slots": lambda: native.state_copy_slots(table, dev_pairs), "index_copy": per_layer}

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / launches * 1e3
    for f in sides.values():
        timed(f)
    times = {k: [] for k in sides}
    for _ in range(rounds):
        for k, f in sides.items():
            times[k].append(timed(f))
    row = dict(pairs=pairs, launches=launches, rounds=rounds, tensors=len(table.tensors),
               slot_bytes=sum(t[0].numel() * t.element_size() for t in table.tensors))
    for k, v in times.items():
        row[f"{k}_us"] = round(statistics.median(v), 1)
        row[f"spread_{k}"] = round(max(v) / min(v), 3)
    row["index_copy_over_state_copy"] = round(row["index_copy_us"] / row["state_copy_slots_us"], 2)
    return row


def admission_bench(model, k, rounds, prompt_len=64, B=16):
    """the time of admitting k prompts of prompt_len tokens into an idle engine (prompt passes, first-token sampling, the scatter into the
    step's buffers; no decode step), packed against alone"""
    from dimsum_amd.utils.serving import DecodeEngine
    g = torch.Generator().manual_seed(k)
    prompts = [torch.randint(0, SHAPE["vocab_size"], (prompt_len,), generator=g) for _ in range(k)]
    kw = dict(max_batch=B, num_slots=B, max_seqlen=PROMPT_RANGE[1] + NEW_RANGE[1], vocab_size=SHAPE["vocab_size"], cg=True)
    engines = {"alone": DecodeEngine(model, packed_prefill=False, **kw), "packed": DecodeEngine(model, packed_prefill=True, **kw)}

    def timed(eng):
        for p in prompts:
            eng.submit(p, 1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            eng._admit()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        for row, rid in enumerate(eng.rows):                 # back to idle without a decode step: the slots are free again
            if rid is not None:
                eng._retire(row, eng.requests[rid])
        eng._fresh.clear()
        eng.requests.clear()
        return dt * 1e3

    for eng in engines.values():
        timed(eng)
    times = {n: [] for n in engines}
    for _ in range(rounds):
        for n, eng in engines.items():
            times[n].append(timed(eng))
    row = dict(prompts=k, prompt_len=prompt_len, rounds=rounds)
    for n, v in times.items():
        row[f"{n}_ms"] = round(statistics.median(v), 3)
        row[f"spread_{n}"] = round(max(v) / min(v), 3)
    row["alone_over_packed"] = round(row["alone_ms"] / row["packed_ms"], 3)
    return row


def serve_bench(model, requests, B, rounds, packed=False, chunked=None):
    from dimsum_amd.utils.serving import DecodeEngine
    useful = sum(n for _, n in requests)
    batches = [(ids.cuda(), seq.cuda(), m) for ids, seq, m in static_batches(requests, B)]
    decoded = sum(ids.shape[0] * (m - ids.shape[1]) for ids, _, m in batches)
    model._decoding_cache = None
    eng = DecodeEngine(model, max_batch=B, num_slots=B, max_seqlen=PROMPT_RANGE[1] + NEW_RANGE[1], vocab_size=SHAPE["vocab_size"], cg=True,
                       packed_prefill=packed or chunked is not None,
                       **({"chunked_prefill": True, "max_prefill_tokens": chunked} if chunked is not None else {}))
    # the static side's cache at its final size before anything is timed: the longest batch first, so no later batch re-captures
    longest = max(batches, key=lambda b: b[2])
    model.generate(longest[0], max_length=longest[2], cg=True, fused_sampling=True, vocab_size=SHAPE["vocab_size"], seq_idx=longest[1])
    run_engine(eng, requests)                                # warm-up round of each
    run_static(model, batches)
    times = {"engine": [], "static": []}
    for _ in range(rounds):
        times["engine"].append(run_engine(eng, requests))
        times["static"].append(run_static(model, batches))
    row = dict(batch=B, requests=len(requests), useful_tokens=useful, static_decoded_tokens=decoded, rounds=rounds, engine_captures=eng.n_captures)
    for k, v in times.items():
        row[f"{k}_tokens_per_s"] = round(useful / statistics.median(v), 1)
        row[f"spread_{k}"] = round(max(v) / min(v), 3)
    row["engine_over_static"] = round(row["engine_tokens_per_s"] / row["static_tokens_per_s"], 3)
    model._decoding_cache = None
    return row


def captured_step(model, params, B):
    """-> replay(): one forward of the model on a static (B, 1) token buffer at seqlen_offset > 0, captured after two warm-up runs"""
    ids = torch.zeros(B, 1, dtype=torch.long, device="cuda")
    step = lambda: model(ids, inference_params=params, num_last_tokens=1).logits
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
        side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    return graph.replay


def step_bench(model, B, steps, rounds, fused):
    from dimsum_amd.utils import InferenceParams
    os.environ["DIMSUM_FUSED_DECODE"] = fused
    dtype = next(iter(model.parameters())).dtype
    with torch.no_grad():
        plain = InferenceParams(max_seqlen=8, max_batch_size=B, seqlen_offset=1, key_value_memory_dict=model.allocate_inference_cache(B, 8, dtype))
        perm = torch.randperm(B, generator=torch.Generator().manual_seed(B)).to(torch.int32).cuda()
        pooled = InferenceParams(max_seqlen=8, max_batch_size=B, seqlen_offset=1, key_value_memory_dict=model.allocate_inference_cache(B, 8, dtype),
                                 state_indices=perm)
        sides = {"plain": captured_step(model, plain, B), "slots": captured_step(model, pooled, B)}

    def timed(replay):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            replay()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e6

    for r in sides.values():
        timed(r)
    times = {k: [] for k in sides}
    for _ in range(rounds):
        for k, r in sides.items():
            times[k].append(timed(r))
    row = dict(batch=B, fused_decode=fused, steps=steps, rounds=rounds)
    for k, v in times.items():
        row[f"{k}_step_us"] = round(statistics.median(v), 1)
        row[f"spread_{k}"] = round(max(v) / min(v), 3)
    row["slots_over_plain"] = round(row["slots_step_us"] / row["plain_step_us"], 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="*", default=[4, 16])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--requests", type=int, default=64)
    ap.add_argument("--steps", type=int, default=512, help="replays per timed window of the step comparison")
    ap.add_argument("--dtype", default="float32")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--packed-prefill", choices=["off", "on", "both"], default="off")
    ap.add_argument("--chunked-prefill", choices=["off", "on", "both"], default="off",
                    help="on: the engine of the default comparison admits in chunks; both: chunked against unchunked packed admission")
    ap.add_argument("--max-prefill-tokens", type=int, default=512, help="the admission budget of --chunked-prefill")
    ap.add_argument("--long-prompts", type=int, default=4, help="--chunked-prefill both: prompts of --long-len tokens among the short ones")
    ap.add_argument("--long-len", type=int, default=4096)
    ap.add_argument("--shared-prefix", type=int, default=0, help="with --chunked-prefill on: a common prefix of this many tokens, full prompts against hold + forks")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_serve needs the GPU"
    from dimsum_amd.models.mixer_seq_simple import MambaLMHeadModel
    policy = os.environ.get("DIMSUM_FUSED_DECODE")
    torch.manual_seed(0)
    model = MambaLMHeadModel(**SHAPE, device="cuda", dtype=getattr(torch, args.dtype)).eval()
    requests = workload(args.requests, args.seed)
    if args.shared_prefix:
        assert args.chunked_prefill == "on", "--shared-prefix rides on chunked admission: pass --chunked-prefill on"
        rows = [dict(shared_prefix_bench(model, requests, B, args.rounds, args.max_prefill_tokens, args.shared_prefix, args.seed), dtype=args.dtype,
                     fused_decode=policy or "unset") for B in args.batches]
        copy = dict(state_copy_bench(model, rounds=args.rounds), dtype=args.dtype)
        for row in rows + [copy]:
            print(json.dumps(row), flush=True)
        print("\n| B | prefix | full prompts s (spread) | hold + forks s (spread) | full / held | prompt tokens full | prompt tokens held |\n|---|---|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['batch']} | {r['shared_prefix']} | {r['full_s']:.3f} ({r['spread_full']:.3f}) | {r['held_s']:.3f} ({r['spread_held']:.3f}) | "
                  f"{r['full_over_held']:.2f} | {r['prefill_tokens']['full']} | {r['prefill_tokens']['held']} |")
        print("\n| pairs | tensors | bytes per slot | state_copy_slots us (spread) | per-layer index_copy_ us (spread) | index_copy_ / state_copy_slots |\n|---|---|---|---|---|---|")
        print(f"| {copy['pairs']} | {copy['tensors']} | {copy['slot_bytes']} | {copy['state_copy_slots_us']:.1f} ({copy['spread_state_copy_slots']:.3f}) | "
              f"{copy['index_copy_us']:.1f} ({copy['spread_index_copy']:.3f}) | {copy['index_copy_over_state_copy']:.2f} |")
        if args.out:
            with open(args.out, "w") as f:
                json.dump(dict(shared_prefix=rows, state_copy=copy), f, indent=1)
        return
    if args.chunked_prefill == "both":
        rows = [dict(chunked_bench(model, requests, B, args.rounds, args.max_prefill_tokens, args.long_prompts, args.long_len, args.seed),
                     dtype=args.dtype, fused_decode=policy or "unset") for B in args.batches]
        for row in rows:
            print(json.dumps(row), flush=True)
        print("\n| B | budget | unchunked tok/s (spread) | chunked tok/s (spread) | chunked / unchunked | largest step ms unchunked (spread) | "
              "largest step ms chunked (spread) |\n|---|---|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['batch']} | {r['max_prefill_tokens']} | {r['unchunked_tokens_per_s']:.0f} ({r['spread_unchunked']:.3f}) | "
                  f"{r['chunked_tokens_per_s']:.0f} ({r['spread_chunked']:.3f}) | {r['chunked_over_unchunked']:.3f} | "
                  f"{r['unchunked_max_step_ms']:.2f} ({r['spread_max_step_unchunked']:.3f}) | {r['chunked_max_step_ms']:.2f} ({r['spread_max_step_chunked']:.3f}) |")
        if args.out:
            with open(args.out, "w") as f:
                json.dump(dict(chunked=rows), f, indent=1)
        return
    if args.packed_prefill == "both":
        packed = [dict(packed_bench(model, requests, B, args.rounds), dtype=args.dtype, fused_decode=policy or "unset") for B in args.batches]
        admit = [dict(admission_bench(model, k, args.rounds), dtype=args.dtype) for k in (1, 4, 16)]
        for row in packed + admit:
            print(json.dumps(row), flush=True)
        print("\n| B | useful tokens | alone tok/s (spread) | packed tok/s (spread) | packed / alone | prompt passes alone / packed |\n|---|---|---|---|---|---|")
        for r in packed:
            print(f"| {r['batch']} | {r['useful_tokens']} | {r['alone_tokens_per_s']:.0f} ({r['spread_alone']:.3f}) | {r['packed_tokens_per_s']:.0f} "
                  f"({r['spread_packed']:.3f}) | {r['packed_over_alone']:.3f} | {r['prompt_passes']['alone']} / {r['prompt_passes']['packed']} |")
        print("\n| prompts x 64 tokens | alone ms (spread) | packed ms (spread) | alone / packed |\n|---|---|---|---|")
        for r in admit:
            print(f"| {r['prompts']} | {r['alone_ms']:.2f} ({r['spread_alone']:.3f}) | {r['packed_ms']:.2f} ({r['spread_packed']:.3f}) | {r['alone_over_packed']:.2f} |")
        if args.out:
            with open(args.out, "w") as f:
                json.dump(dict(packed=packed, admission=admit), f, indent=1)
        return
    serve, steps = [], []
    for B in args.batches:
        row = dict(serve_bench(model, requests, B, args.rounds, packed=args.packed_prefill == "on",
                               chunked=args.max_prefill_tokens if args.chunked_prefill == "on" else None), dtype=args.dtype, fused_decode=policy or "unset")
        serve.append(row)
        print(json.dumps(row), flush=True)
    for B in args.batches:
        for fused in ("1", "0"):
            row = dict(step_bench(model, B, args.steps, args.rounds, fused), dtype=args.dtype)
            steps.append(row)
            print(json.dumps(row), flush=True)
    if policy is None:
        os.environ.pop("DIMSUM_FUSED_DECODE", None)
    else:
        os.environ["DIMSUM_FUSED_DECODE"] = policy
    print("\n| B | useful tokens | engine tok/s | static tok/s | engine / static | static decoded tokens |\n|---|---|---|---|---|---|")
    for r in serve:
        print(f"| {r['batch']} | {r['useful_tokens']} | {r['engine_tokens_per_s']:.0f} | {r['static_tokens_per_s']:.0f} | {r['engine_over_static']:.2f} | "
              f"{r['static_decoded_tokens']} |")
    print("\n| B | DIMSUM_FUSED_DECODE | un-indexed step us | slot-indexed step us | slots / plain |\n|---|---|---|---|---|")
    for r in steps:
        print(f"| {r['batch']} | {r['fused_decode']} | {r['plain_step_us']:.1f} | {r['slots_step_us']:.1f} | {r['slots_over_plain']:.3f} |")
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(serve=serve, step=steps), f, indent=1)


if __name__ == "__main__":
    main()
