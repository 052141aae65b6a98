"""tools/bench_conv_cl.py (GPU box): the channel-last causal conv1d (csrc/causal_conv1d_cl.hip) against the route a channel-last caller
had before it: a transposing copy to (batch, dim, seqlen), the seqlen-contiguous kernel (csrc/causal_conv1d.hip), a transposing copy back.

  python tools/bench_conv_cl.py [--rounds 7] [--inner 20]

One process, every arm warmed up, interleaved rounds timed with device events. Prints one JSON line per shape and dtype: the median and
minimum time of both routes, forward and backward, and the share of the streaming bytes (2 B D L s forward, 3 B D L s backward) over the
6.29 TB/s a float4 copy reaches on this chip that the new kernels achieve. Numbers quoted in DESIGN.md section 3.3b come from here."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dimsum_amd import native  # noqa: E402

COPY_TBS = 6.29          # measured float4 copy rate of an MI355X, TB/s
SHAPES = ((64, 1024, 2048), (256, 256, 1024))      # (B, L, D)


def timed(fn, n):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(n):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / n


def bench(B, L, D, dtype, rounds, inner, width=4):
    g = torch.Generator(device="cuda").manual_seed(B + L + D)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)
    x, dout = (rn(B, L, D).to(dtype).transpose(1, 2) for _ in range(2))          # (B, D, L) views with channel stride 1
    w, b = rn(D, width), rn(D)
    out, dx = (torch.empty(B, L, D, device="cuda", dtype=dtype).transpose(1, 2) for _ in range(2))
    xc = x.contiguous()                                                           # what the old forward saved for its backward

    def old_fwd():
        out.copy_(native.causal_conv1d_fwd(x.contiguous(), w, b, True))

    def old_bwd():
        dx.copy_(native.causal_conv1d_bwd(xc, w, b, dout.contiguous(), None, True)[0])

    arms = {"fwd channel-last": lambda: native.causal_conv1d_fwd(x, w, b, True, out=out),
            "fwd copy + kernel + copy": old_fwd,
            "bwd channel-last": lambda: native.causal_conv1d_bwd(x, w, b, dout, dx, True),
            "bwd copy + kernel + copy": old_bwd}
    # the two routes compute the same thing (fp32: within the FMA order; half precision: within one rounding of the output)
    new_out, old_out = arms["fwd channel-last"]().clone(), native.causal_conv1d_fwd(xc, w, b, True)
    new_dx, old_dx = arms["bwd channel-last"]()[0].clone(), native.causal_conv1d_bwd(xc, w, b, dout.contiguous(), None, True)[0]
    diff = {"out": (new_out.float() - old_out.float()).abs().max().item(), "dx": (new_dx.float() - old_dx.float()).abs().max().item()}
    for f in arms.values():
        f()
    torch.cuda.synchronize()
    res = {k: [] for k in arms}
    for _ in range(rounds):
        for k, f in arms.items():
            res[k].append(timed(f, inner))
    elems = B * L * D * x.element_size()
    row = {"B": B, "L": L, "D": D, "dtype": str(dtype)[6:], "width": width, "max_abs_diff_vs_old_kernel": diff}
    for k, v in res.items():
        v.sort()
        med = v[len(v) // 2]
        row[k] = {"ms_median": round(med, 4), "ms_min": round(v[0], 4)}
        if "channel-last" in k:
            tbs = (2 if k.startswith("fwd") else 3) * elems / med / 1e9
            row[k].update(streaming_TBs=round(tbs, 3), share_of_copy_rate=round(tbs / COPY_TBS, 3))
    for d in ("fwd", "bwd"):
        row[f"{d} speedup"] = round(row[f"{d} copy + kernel + copy"]["ms_median"] / row[f"{d} channel-last"]["ms_median"], 2)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_conv_cl.py needs the GPU"
    for B, L, D in SHAPES:
        for dtype in (torch.float32, torch.bfloat16):
            bench(B, L, D, dtype, args.rounds, args.inner)


if __name__ == "__main__":
    main()
