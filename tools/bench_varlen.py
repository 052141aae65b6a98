#!/usr/bin/env python3
"""Packed variable-length rows (seq_idx) against padding, at equal real-token count: one Mamba mixer forward + backward and one
MambaLMHeadModel.loss step (forward + backward), float32, on a fixed long-tailed set of document lengths (LENGTHS below: 33 documents,
8192 tokens, the longest 2048), three ways that take turns round by round in one process:

  (a) packed    the documents packed first-fit-decreasing into rows of `--row` tokens (4 rows of 2048), with seq_idx: the packed-row
                instantiations of the general scan family and of the conv;
  (b) padded    one row per document, padded to the longest (33 rows of 2048, 8.25 x the tokens), no seq_idx: the tuned kernels;
  (c) packed, no seq_idx   the same 4 rows as one unbroken sequence each: the tuned route on the packed shape. Numerically WRONG (the
                documents see each other); it is here to show what the general route of (a) costs against the tuned one.

Times are device times between two events around `--iters` back-to-back calls after a warm-up of each variant; the median of `--rounds`
rounds and the spread max / min of the rounds.

    python tools/bench_varlen.py [--rounds 5] [--iters 3] [--layers 4] [--out varlen_bench.json]
prints one JSON line per measurement and a markdown table at the end."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# a long-tailed corpus sample, fixed: a few long documents, many short ones (sum 8192, max 2048, median 96)
LENGTHS = [2048, 1024, 768, 512, 512, 384, 384, 256, 256, 256, 192, 192, 128, 128, 128, 128, 96, 96, 96, 64, 64, 64, 64, 64, 48, 48, 32, 32, 32,
           32, 32, 16, 16]
D_MODEL, VOCAB = 768, 50280


def pack(lengths, row):
    """first-fit-decreasing -> [[lengths of the documents of one row]]"""
    rows = []
    for n in sorted(lengths, reverse=True):
        for r in rows:
            if sum(r) + n <= row:
                r.append(n)
                break
        else:
            rows.append([n])
    return rows


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--row", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_varlen needs the GPU"
    from dimsum_amd.models.mixer_seq_simple import MambaLMHeadModel
    from dimsum_amd.modules.mamba_simple import Mamba
    from dimsum_amd.utils import packed_labels, seq_idx_from_lengths
    assert max(LENGTHS) <= args.row
    rows = pack(LENGTHS, args.row)
    real = sum(LENGTHS)
    seq = torch.stack([seq_idx_from_lengths(r, args.row) for r in rows]).cuda()
    g = torch.Generator().manual_seed(0)
    ids_packed = torch.randint(0, VOCAB, (len(rows), args.row), generator=g).cuda()
    ids_padded = torch.randint(0, VOCAB, (len(LENGTHS), args.row), generator=g).cuda()
    labels_packed = packed_labels(ids_packed, seq)
    for r, docs in enumerate(rows):                                   # a trailing remainder is padding: no targets
        labels_packed[r, sum(docs):] = -100
    labels_padded = torch.cat([ids_padded[:, 1:], ids_padded.new_full((len(LENGTHS), 1), -100)], dim=1)
    for r, n in enumerate(LENGTHS):
        labels_padded[r, n - 1:] = -100
    shapes = dict(real_tokens=real, packed_tokens=len(rows) * args.row, padded_tokens=len(LENGTHS) * args.row, documents=len(LENGTHS))
    print(json.dumps(dict(what="workload", rows_packed=[len(r) for r in rows], **shapes)), flush=True)
    out = []

    torch.manual_seed(0)
    mixer = Mamba(D_MODEL, d_state=16, d_conv=4, expand=2, layer_idx=0).cuda()
    x_packed = torch.randn(len(rows), args.row, D_MODEL, device="cuda")
    x_padded = torch.randn(len(LENGTHS), args.row, D_MODEL, device="cuda")

    def mixer_step(x, **kw):
        def run():
            xin = x.detach().requires_grad_()
            mixer(xin, **kw).sum().backward()
            mixer.zero_grad(set_to_none=True)
        return run

    r = alternate({"packed": mixer_step(x_packed, seq_idx=seq), "padded": mixer_step(x_padded), "packed_no_seq_idx": mixer_step(x_packed)},
                  args.rounds, args.iters)
    out.append(dict(what="mixer fwd+bwd", **{f"{k}_ms": round(v[0], 3) for k, v in r.items()}, **{f"{k}_spread": round(v[1], 3) for k, v in r.items()}))
    print(json.dumps(out[-1]), flush=True)
    del mixer, x_packed, x_padded
    torch.cuda.empty_cache()

    model = MambaLMHeadModel(D_MODEL, args.layers, VOCAB, pad_vocab_size_multiple=8, rms_norm=True, fused_add_norm=True, residual_in_fp32=True).cuda()

    def loss_step(ids, labels, **kw):
        def run():
            model.loss(ids, labels, **kw).backward()
            model.zero_grad(set_to_none=True)
        return run

    r = alternate({"packed": loss_step(ids_packed, labels_packed, seq_idx=seq), "padded": loss_step(ids_padded, labels_padded),
                   "packed_no_seq_idx": loss_step(ids_packed, labels_packed)}, args.rounds, args.iters)
    out.append(dict(what=f"LM loss step fwd+bwd, {args.layers} layers", **{f"{k}_ms": round(v[0], 3) for k, v in r.items()},
                    **{f"{k}_spread": round(v[1], 3) for k, v in r.items()}))
    print(json.dumps(out[-1]), flush=True)

    print(f"\n{shapes}")
    print("| what | (a) packed + seq_idx ms | (b) padded ms | (c) packed, no seq_idx ms | (b) / (a) | (a) / (c) | spread a / b / c |\n|---|---|---|---|---|---|---|")
    for r in out:
        print(f"| {r['what']} | {r['packed_ms']} | {r['padded_ms']} | {r['packed_no_seq_idx_ms']} | {r['padded_ms'] / r['packed_ms']:.2f} | "
              f"{r['packed_ms'] / r['packed_no_seq_idx_ms']:.2f} | {r['packed_spread']} / {r['padded_spread']} / {r['packed_no_seq_idx_spread']} |")
    if args.out:
        with open(args.out, "w") as f:
            json.dump([shapes] + out, f, indent=1)


if __name__ == "__main__":
    main()
