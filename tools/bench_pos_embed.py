"""tools/bench_pos_embed.py (GPU box): the positional-encoding passes (csrc/pos_embed.hip) at (B, L, C) = (256, 256, 1024) next to the
torch-eager composition they replace, in one process: microseconds per call (device events around windows of calls, the two alternating,
minimum and median over the windows) and GB/s of algorithmic traffic of the HIP pass."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dimsum_amd.ops import pos_embed  # noqa: E402
from dimsum_amd.pe.my_rotary import get_2d_sincos_rotary_embed  # noqa: E402


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def compare(name, hip, eager, tensors, n=20, rounds=7):
    for fn in (hip, eager):
        for _ in range(3):
            fn()
    th, te = [], []
    for _ in range(rounds):                 # alternate: both see the same neighbours on the machine
        th.append(window(hip, n))
        te.append(window(eager, n))
    th.sort(), te.sort()
    gbs = tensors * B * L * C * 4 / th[0] / 1e3
    print(f"{name:12s} HIP {th[0]:8.1f} us min {th[rounds // 2]:8.1f} median ({gbs:6.0f} GB/s over {tensors} tensors)   "
          f"torch eager {te[0]:8.1f} us min {te[rounds // 2]:8.1f} median", flush=True)


B, L, C, G = 256, 256, 1024, 16


def main():
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)      # noqa: E731
    x, dy = rnd(B, L, C), rnd(B, L, C)
    sin, cos = (torch.from_numpy(t).float().cuda() for t in get_2d_sincos_rotary_embed(C, G))
    compare("rope fwd", lambda: pos_embed.rotary(x, sin, cos), lambda: pos_embed.rotary_torch(x, sin, cos), 2)
    compare("rope bwd", lambda: pos_embed.rotary(dy, sin, cos), lambda: pos_embed.rotary_torch(dy, sin, cos, inverse=True), 2)
    w, b, gamma, beta, mod = rnd(C, 1, 3, 3) / 3, 0.1 * rnd(C), 1 + 0.1 * rnd(C), 0.1 * rnd(C), 0.1 * rnd(B, 2 * C)
    with torch.no_grad():
        compare("cpe fwd", lambda: pos_embed.cpe(x, w, b, gamma, beta, mod, G), lambda: pos_embed.cpe_torch(x, w, b, gamma, beta, mod, G), 2)
    leaves = [t.requires_grad_() for t in (x, w, b, gamma, beta, mod)]

    def fwd_bwd(fn):
        def run():
            for t in leaves:
                t.grad = None
            fn(*leaves, G).backward(dy)
        return run
    compare("cpe fwd+bwd", fwd_bwd(pos_embed.cpe), fwd_bwd(pos_embed.cpe_torch), 7, n=10)


if __name__ == "__main__":
    main()
