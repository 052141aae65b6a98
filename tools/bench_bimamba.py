#!/usr/bin/env python3
"""Micro-benchmark of the bidirectional selective scan (bimamba_inner_fn's scan; GPU box). In ONE process it times the fused launch pairs
(native.selective_scan_bidir_fwd / _bwd) against what they replace: the reference's composition -- .flip(-1) copies of u, delta, B, C, z
(backward: and of dout), two launches of the existing scan (the library's own kernel choice), flip-and-add of out_z (backward: of du, ddelta,
dz, dB, dC). Training forward (saved `out` and states, what the backward consumes) and inference forward (out_z only) are timed apart.
Operands have the layouts the mixer hands the scan (d-major delta and dout, u / z halves of xz, B / C rows of x_proj's transposed output).
Prints one JSON line: per shape, median milliseconds per call and fused / composed ratios."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dimsum_amd import native  # noqa: E402


def _time(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def bench_shape(b, d, L, N, iters, warmup):
    dev = "cuda"
    xz = torch.randn(2 * d, b, L, device=dev).permute(1, 0, 2)                  # in_proj's d-major output
    u, z = xz.chunk(2, dim=1)
    delta = (0.5 * torch.rand(d, b * L, device=dev)).view(d, b, L).permute(1, 0, 2)
    bc = torch.randn(2 * N, b * L, device=dev)
    Bm = bc[:N].view(N, b, L).permute(1, 0, 2).unsqueeze(1)
    Cm = bc[N:].view(N, b, L).permute(1, 0, 2).unsqueeze(1)
    A, A_b = -0.5 * torch.rand(d, N, device=dev), -0.5 * torch.rand(d, N, device=dev)
    D, bias = torch.randn(d, device=dev), 0.5 * torch.rand(d, device=dev)
    dout = torch.randn(d, b, L, device=dev).permute(1, 0, 2)
    fl = lambda t: t.flip(-1)                                                     # noqa: E731

    def fused_fwd(train=True):
        return native.selective_scan_bidir_fwd(u, delta, A, A_b, Bm, Cm, D, z, bias, True, need_out=train, need_ckpt=train)

    def composed_fwd(train=True):
        out, _, oz, *ck = native.selective_scan_fwd(u, delta, A, Bm, Cm, D, z, bias, True, need_out=train, need_x=False, need_ckpt=train)
        fu, fd, fB, fC, fz = fl(u), fl(delta), fl(Bm), fl(Cm), fl(z)
        out_b, _, oz_b, *ck_b = native.selective_scan_fwd(fu, fd, A_b, fB, fC, D, fz, bias, True, need_out=train, need_x=False, need_ckpt=train)
        return oz + oz_b.flip(-1), out, out_b, ck, ck_b

    out, out_b, _, ck, ck_b = fused_fwd()
    _, out_c, out_bc, ckc, ckc_b = composed_fwd()

    def fused_bwd():
        return native.selective_scan_bidir_bwd(u, delta, A, A_b, Bm, Cm, D, z, bias, dout, out, out_b, ck, ck_b, True, False)

    def composed_bwd():
        f = native.selective_scan_bwd(u, delta, A, Bm, Cm, D, z, bias, dout, None, out_c, None, True, False, ckpt=ckc[0])
        r = native.selective_scan_bwd(fl(u), fl(delta), A_b, fl(Bm), fl(Cm), D, fl(z), bias, fl(dout), None, out_bc, None, True, False, ckpt=ckc_b[0])
        return (f[0] + r[0].flip(-1), f[1] + r[1].flip(-1), f[3] + r[3].flip(-1), f[4] + r[4].flip(-1), f[7] + r[7].flip(-1),
                f[5] + r[5], f[6] + r[6])

    res = {"shape": [b, d, L, N], "fwd_kernel": native.scan_bidir_fwd_kernel_for(b, d, L, N),
           "composed_fwd_kernel": native.scan_fwd_kernel_for(b, d, L, N)}
    for name, fa, fb in (("fwd_train", lambda: fused_fwd(True), lambda: composed_fwd(True)),
                         ("fwd_infer", lambda: fused_fwd(False), lambda: composed_fwd(False)),
                         ("bwd", fused_bwd, composed_bwd)):
        tf, tc = _time(fa, iters, warmup), _time(fb, iters, warmup)
        res[name] = {"fused_ms": round(tf, 4), "composed_ms": round(tc, 4), "ratio": round(tf / tc, 3)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="256x1024x256x16,4x256x512x16", help="batch x dim x seqlen x dstate, comma-separated")
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    out = {"tool": "bench_bimamba", "dtype": "float32", "results": [bench_shape(*s, a.iters, a.warmup) for s in shapes]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
