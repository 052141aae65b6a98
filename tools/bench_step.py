"""tools/bench_step.py (GPU box): the recurrent form of the mixer (Mamba.step: in_proj -> causal_conv1d_update -> x_proj ->
selective_state_update with dt_proj inside -> out_proj; csrc/mixer_step.hip) at DiM-L's mixer geometry, d_model 512, d_inner 1024, d_state 16,
dt_rank 32, float32, for batch 1, 32 and 256: microseconds per step and tokens/s, eager and replayed from a captured graph (device events
around windows of steps, minimum and median over the windows); the two kernels called alone with their algorithmic bytes (conv: 2 B D W 4 of state +
2 B D 4; state update: 2 B D N 4 of state + O(B D)) over the CALL time (enqueue-bound at these sizes: a floor of the kernels' rate, not it); the kernel launches of one step as the profiler counts them."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dimsum_amd import native  # noqa: E402
from dimsum_amd.modules.mamba_simple import Mamba  # noqa: E402

D_MODEL, N, W, R = 512, 16, 4, 32
D = 2 * D_MODEL


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def timed(fn, n=400, rounds=7):
    for _ in range(5):
        fn()
    t = sorted(window(fn, n) for _ in range(rounds))
    return t[0], t[rounds // 2]


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
               and "memset" not in e.name.lower())


def bench(m, B):
    g = torch.Generator(device="cuda").manual_seed(B)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)      # noqa: E731
    token = rnd(B, 1, D_MODEL)
    conv_state, ssm_state = m.allocate_inference_cache(B, 1)
    step = lambda: m.step(token, conv_state, ssm_state)               # noqa: E731
    eager = timed(step)
    n_launch = launches(step)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    replay = timed(graph.replay)
    print(f"batch {B:4d}  step eager {eager[0]:7.1f} us min {eager[1]:7.1f} median ({B / eager[1] * 1e6:11.0f} tokens/s)   "
          f"graph replay {replay[0]:7.1f} us min {replay[1]:7.1f} median ({B / replay[1] * 1e6:11.0f} tokens/s)   kernel launches per step: {n_launch}",
          flush=True)
    xz, x_db = rnd(B, 2 * D), rnd(B, R + 2 * N)
    x, z = xz.chunk(2, dim=-1)
    cw, A = m.conv1d.weight.reshape(D, W), -torch.exp(m.A_log.float())
    conv_bytes = 2 * B * D * W * 4 + 2 * B * D * 4
    ssu_bytes = 2 * B * D * N * 4 + 3 * B * D * 4 + (D * N + D * R + 2 * D) * 4 + B * (R + 2 * N) * 4
    for name, nbytes, fn in (
            ("causal_conv1d_update", conv_bytes, lambda: native.causal_conv1d_update(x, conv_state, cw, m.conv1d.bias, True)),
            ("selective_state_update", ssu_bytes, lambda: native.selective_state_update(ssm_state, x, None, A, x_db[:, R:R + N], x_db[:, R + N:], m.D, z,
                                                                                         m.dt_proj.bias, True, dt_proj=(m.dt_proj.weight, x_db[:, :R])))):
        t = timed(fn)
        print(f"            {name:24s} {t[0]:7.1f} us min {t[1]:7.1f} median   {nbytes / 1e6:8.3f} MB algorithmic / call time = {nbytes / t[0] / 1e3:7.1f} GB/s (enqueue-bound: a floor, not the kernel's rate)",
              flush=True)


def main():
    assert torch.cuda.is_available(), "bench_step.py needs the GPU"
    print(f"{torch.cuda.get_device_name(0)}; Mamba.step, float32, d_model {D_MODEL}, d_inner {D}, d_state {N}, d_conv {W}, dt_rank {R}", flush=True)
    torch.manual_seed(0)
    m = Mamba(D_MODEL, d_state=N, d_conv=W, expand=2, layer_idx=0).cuda().eval()
    with torch.no_grad():
        for B in (1, 32, 256):
            bench(m, B)


if __name__ == "__main__":
    main()
