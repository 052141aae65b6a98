"""tools/bench_moe.py (GPU box): one SwitchMLP (dimsum_amd/switch_mlp.py) at DiM-L/2's token shape -- 65536 tokens x 1024 channels, 8 experts,
float32 -- forward and forward + backward, against a torch composition written as the reference writes it (a loop over the experts with
nonzero(), indexed gathers and indexed scatters into a zero-filled buffer; switch_mlp.py:69-99) in the same process on the same weights; then
each row pass of csrc/moe.hip and the experts' activation (csrc/act_rows.hip) alone with its algorithmic bytes over its time, next to gelu_fwd at equal bytes. Device events around windows of
calls, minimum and median over the windows. The grouped rows: the same layer with grouped=True (the inference forward on the grouped expert GEMM of
csrc/moe_gemm.hip, no host read of the offsets) and its two GEMM launches alone with their FLOP rate; the same grouped layer under the "f16s" policy
(csrc/moe_gemm_f16.hip) next to DIMSUM_MOE_F16S=0, and the fp16 GEMM and its two image producers alone. Prints figures only: no threshold is asserted anywhere.   [--tokens N --dim H --experts E]"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dimsum_amd import native  # noqa: E402
from dimsum_amd.switch_mlp import SwitchMLP  # noqa: E402


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def timed(fn, n=10, rounds=5):
    for _ in range(3):
        fn()
    t = sorted(window(fn, n) for _ in range(rounds))
    return t[0], t[rounds // 2]


def reference_forward(m, x):
    """SwitchMLP.forward as the reference composes it from torch operators"""
    shape = x.shape
    route = torch.softmax(m.router(x).view(-1, m.num_moe_experts), dim=1) if m.routing != "sinkhorn" else torch.sigmoid(m.router(x).view(-1, m.num_moe_experts))
    p, ind = torch.max(route, dim=1)
    h = x.view(-1, shape[-1])
    total = torch.zeros_like(h)
    for i, ex in enumerate(m.local_experts):
        idx = (ind == i).nonzero()
        a = F.linear(h[idx, :], ex.linear_fc1.weight, ex.linear_fc1.bias)
        if m.gated_linear_unit:
            a1, a2 = torch.chunk(a, 2, dim=-1)
            a = F.gelu(a1) * a2
        else:
            a = F.gelu(a)
        total[idx, :] = F.linear(a, ex.linear_fc2.weight, ex.linear_fc2.bias)
    return (total * p.unsqueeze(1)).view(shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=65536)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--experts", type=int, default=8)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_moe.py needs the GPU"
    T, H, E = args.tokens, args.dim, args.experts
    torch.manual_seed(0)
    m = SwitchMLP(H, layer_idx=1, num_moe_experts=E).cuda()
    x = torch.randn(1, T, H, device="cuda", requires_grad=True)
    dout = torch.randn_like(x)

    def fb(fwd):
        def run():
            m.zero_grad(set_to_none=True)
            x.grad = None
            fwd(m, x).backward(dout)
        return run

    with torch.no_grad():
        ours, ref = m(x), reference_forward(m, x)
    print(f"SwitchMLP {T} x {H}, {E} experts, float32; max |ours - composition| = {(ours - ref).abs().max().item():.3e} (max |out| {ref.abs().max().item():.3e})")
    with torch.no_grad():
        for name, fn in (("fused passes", lambda: m(x)), ("torch composition", lambda: reference_forward(m, x))):
            lo, med = timed(fn)
            print(f"  forward            {name:18s} min {lo:8.3f} ms  median {med:8.3f} ms")
        m.set_grouped(True)
        grouped = m(x)
        print(f"  grouped: max |grouped - fused passes| = {(grouped - ours).abs().max().item():.3e}")
        lo, med = timed(lambda: m(x))
        print(f"  forward            {'grouped GEMM':18s} min {lo:8.3f} ms  median {med:8.3f} ms")
        # the same grouped layer under the "f16s" policy (allow_tf32): the expert GEMMs on scaled-fp16 images (csrc/moe_gemm_f16.hip), next to the same
        # policy with DIMSUM_MOE_F16S=0 -- the fp32 grouped kernel, what the layer ran under the policy before -- inside one frozen_weights() scope
        # each (a sampler's: the weight images are built once) and bare (2 E images per call in one multi-job launch)
        from dimsum_amd import gemm
        old_tf32 = torch.backends.cuda.matmul.allow_tf32
        torch.backends.cuda.matmul.allow_tf32 = True
        gemm.set_policy("f16s")
        try:
            one = m(x)
            print(f"  grouped, policy f16s: max |f16s - fused passes| = {(one - ours).abs().max().item():.3e}")
            for label, env in (("grouped f16s", "1"), ("grouped f16s off", "0")):
                os.environ["DIMSUM_MOE_F16S"] = env
                lo, med = timed(lambda: m(x))
                with gemm.frozen_weights():
                    lo_f, med_f = timed(lambda: m(x))
                print(f"  forward            {label:18s} min {lo:8.3f} ms  median {med:8.3f} ms   frozen weights: min {lo_f:8.3f} ms  median {med_f:8.3f} ms")
        finally:
            os.environ.pop("DIMSUM_MOE_F16S", None)
            gemm.set_policy("default")
            torch.backends.cuda.matmul.allow_tf32 = old_tf32
        m.set_grouped(False)
    for name, fn in (("fused passes", fb(lambda mm, xx: mm(xx))), ("torch composition", fb(reference_forward))):
        lo, med = timed(fn, n=5)
        print(f"  forward + backward {name:18s} min {lo:8.3f} ms  median {med:8.3f} ms")

    # the passes alone: algorithmic bytes / time
    with torch.no_grad():
        x2 = x.detach().view(T, H)
        w, b = m.router.weight.detach(), m.router.bias.detach()
        prob, expert, logits, offsets, perm, inv, row_expert = native.moe_route_fwd(x2, w, b, "softmax")
        xp = native.moe_permute(x2, perm)
        h1 = torch.randn(T, 8 * H, device="cuda")
        hh = native.moe_act_fwd(h1, None, row_expert, True)
        dh = torch.randn_like(hh)
        y, dprob = torch.randn_like(x2), torch.randn(T, device="cuda")
        f4 = 4.0
        passes = [
            ("moe_route_fwd (+ sort)", lambda: native.moe_route_fwd(x2, w, b, "softmax"), T * H * f4),
            ("moe_permute", lambda: native.moe_permute(x2, perm), 2 * T * H * f4),
            ("moe_act_fwd (gated)", lambda: native.moe_act_fwd(h1, None, row_expert, True), 12 * T * H * f4),
            ("moe_act_bwd (gated)", lambda: native.moe_act_bwd(h1, None, row_expert, dh, True), 20 * T * H * f4),
            ("moe_combine_fwd", lambda: native.moe_combine_fwd(y, perm, prob), 2 * T * H * f4),
            ("moe_combine_bwd", lambda: native.moe_combine_bwd(x2, y, perm, prob), 3 * T * H * f4),
            ("moe_route_bwd", lambda: native.moe_route_bwd(x2, w, logits, prob, expert, inv, dprob, xp, "softmax"), 3 * T * H * f4),
            ("gelu_fwd (2 T H 4 bytes)", lambda: native.gelu_fwd(x2), 2 * T * H * f4),
            ("gelu_fwd (12 T H 4 bytes)", lambda: native.gelu_fwd(h1.view(-1)[:6 * T * H].view(T, 6 * H)), 12 * T * H * f4),
        ]
        for name, fn, nbytes in passes:
            lo, med = timed(fn, n=20)
            print(f"  {name:28s} min {lo * 1e3:9.1f} us  median {med * 1e3:9.1f} us  {nbytes / lo / 1e6:8.1f} GB/s")
        w1 = [ex.linear_fc1.weight.detach() for ex in m.local_experts]
        w2 = [ex.linear_fc2.weight.detach() for ex in m.local_experts]
        for name, a, ws in (("moe_gemm fc1", xp, w1), ("moe_gemm fc2", hh, w2)):
            lo, med = timed(lambda: native.moe_gemm(a, offsets, ws), n=10)
            flop = 2.0 * T * ws[0].shape[0] * ws[0].shape[1]
            print(f"  {name:28s} min {lo * 1e3:9.1f} us  median {med * 1e3:9.1f} us  {flop / lo / 1e9:8.1f} TFLOP/s (fp32-equivalent; 3 bf16 products each)")
        xp16, hh16 = native.moe_permute(x2, perm, split3="f16s"), native.moe_act_fwd(h1, None, row_expert, True, split3="f16s")
        for name, a, ws in (("moe_gemm_f16s fc1", xp16, w1), ("moe_gemm_f16s fc2", hh16, w2)):
            imgs = [native.rows_f16s(w_) for w_ in ws]
            lo, med = timed(lambda: native.moe_gemm_f16s(a, offsets, imgs), n=10)
            flop = 2.0 * T * ws[0].shape[0] * ws[0].shape[1]
            print(f"  {name:28s} min {lo * 1e3:9.1f} us  median {med * 1e3:9.1f} us  {flop / lo / 1e9:8.1f} TFLOP/s (one fp16 product)")
        for name, fn, nbytes in (("moe_permute (f16s image)", lambda: native.moe_permute(x2, perm, split3="f16s"), T * H * (f4 + 2)),
                                 ("moe_act_fwd (gated, f16s)", lambda: native.moe_act_fwd(h1, None, row_expert, True, split3="f16s"), T * H * (8 * f4 + 4 * 2))):
            lo, med = timed(fn, n=20)
            print(f"  {name:28s} min {lo * 1e3:9.1f} us  median {med * 1e3:9.1f} us  {nbytes / lo / 1e6:8.1f} GB/s")


if __name__ == "__main__":
    main()
