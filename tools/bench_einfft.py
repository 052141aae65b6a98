"""tools/bench_einfft.py (GPU box): the spectral branch of block type "combined_einfft" (csrc/einfft.hip) at (B, N, C) = (256, 256, 512) and
(64, 1024, 576) next to the torch composition it replaces (ops/einfft.py:einfft_torch: torch.fft, einsum, relu, softshrink), in one process:
microseconds per call (device events around windows of calls, the two alternating, minimum and median over the windows) for the three passes
alone, the branch forward and forward + backward, and GB/s of the passes against their algorithmic traffic (dft 3, mlp 4, idft 3 units of
B N C 4 bytes)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dimsum_amd import native  # noqa: E402
from dimsum_amd.ops import einfft as ops  # noqa: E402


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def compare(name, unit_bytes, hip, eager, units=None, n=10, rounds=7):
    fns = [f for f in (hip, eager) if f is not None]
    for fn in fns:
        for _ in range(3):
            fn()
    times = [[] for _ in fns]
    for _ in range(rounds):                 # alternate: both see the same neighbours on the machine
        for t, fn in zip(times, fns):
            t.append(window(fn, n))
    for t in times:
        t.sort()
    line = f"{name:14s} HIP {times[0][0]:9.1f} us min {times[0][rounds // 2]:9.1f} median"
    if units:
        line += f" ({units * unit_bytes / times[0][0] / 1e3:6.0f} GB/s over {units} units)"
    if eager is not None:
        line += f"   torch {times[1][0]:9.1f} us min {times[1][rounds // 2]:9.1f} median   x{times[1][rounds // 2] / times[0][rounds // 2]:.2f}"
    print(line, flush=True)


def bench(B, N, C):
    print(f"(B, N, C) = ({B}, {N}, {C}), bs = {C // 4}", flush=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)      # noqa: E731
    bs, unit = C // 4, B * N * C * 4
    wide, dy = rnd(B, N, 2 * C), rnd(B, N, C)
    x = wide[..., C:]                                                 # the branch input as the block hands it over: a channel-half view
    w1, w2 = rnd(2, 4, bs, bs) * bs ** -0.5, rnd(2, 4, bs, bs) * bs ** -0.5
    b1, b2 = 0.1 * rnd(2, 4, bs), 0.1 * rnd(2, 4, bs)
    with torch.no_grad():
        re, im = native.einfft_dft(x)
        zr, zi = native.einfft_mlp_fwd(re, im, w1, b1, w2, b2, 0.01)
        compare("dft", unit, lambda: native.einfft_dft(x), lambda: ops.dft_torch(x), 3)
        compare("mlp", unit, lambda: native.einfft_mlp_fwd(re, im, w1, b1, w2, b2, 0.01), lambda: ops.mlp_torch(re, im, w1, b1, w2, b2, 0.01), 4)
        compare("idft_real", unit, lambda: native.einfft_idft_real(zr, zi), lambda: ops.idft_real_torch(zr, zi), 3)
        compare("mlp bwd", unit, lambda: native.einfft_mlp_bwd(re, im, re, im, zr, zi, w1, b1, w2, b2, 0.01), None, 14)
        compare("branch fwd", unit, lambda: ops.einfft(x, w1, b1, w2, b2), lambda: ops.einfft_torch(x, w1, b1, w2, b2))
    leaves = [wide.requires_grad_()] + [t.requires_grad_() for t in (w1, b1, w2, b2)]

    def fwd_bwd(fn):
        def run():
            for t in leaves:
                t.grad = None
            fn(leaves[0][..., C:], *leaves[1:]).backward(dy)
        return run
    compare("branch fwd+bwd", unit, fwd_bwd(ops.einfft), fwd_bwd(ops.einfft_torch), n=5)


def main():
    for shape in ((256, 256, 512), (64, 1024, 576)):
        bench(*shape)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
