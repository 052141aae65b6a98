"""tools/bench_prefill.py (GPU box): a prompt through ONE Mamba mixer in one shot (forward(inference_params=...): the fused prompt path on the
tuned scan kernels) against dimsum_amd.utils.chunked_prefill at a few chunk sizes (first chunk on the same prompt path, the rest through
Mamba.extend: causal_conv1d_chunk + the general scan entered with the cached state), at a given (batch, d_model, prompt), float32: milliseconds
(device events around windows of calls, minimum and median over the windows) and the peak of torch's allocated memory above what was
allocated before the call. One process, one JSON line.
    python tools/bench_prefill.py [--batch 8] [--d-model 512] [--prompt 4096] [--chunks 256,1024] [--d-state 16]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dimsum_amd.modules.mamba_simple import Mamba  # noqa: E402
from dimsum_amd.utils import InferenceParams, chunked_prefill  # noqa: E402


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def timed(fn, n=5, rounds=5):
    for _ in range(2):
        fn()
    t = sorted(window(fn, n) for _ in range(rounds))
    return t[0], t[rounds // 2]


def peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--d-model", type=int, default=512)
    ap.add_argument("--d-state", type=int, default=16)
    ap.add_argument("--prompt", type=int, default=4096)
    ap.add_argument("--chunks", default="256,1024")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_prefill.py needs the GPU"
    torch.manual_seed(0)
    m = Mamba(a.d_model, d_state=a.d_state, d_conv=4, expand=2, layer_idx=0).cuda().eval()
    x = torch.randn(a.batch, a.prompt, a.d_model, device="cuda")
    params = InferenceParams(max_seqlen=a.prompt, max_batch_size=a.batch)

    def run(chunk):
        params.seqlen_offset = 0
        with torch.no_grad():
            return m(x, inference_params=params) if chunk is None else chunked_prefill(m, x, params, chunk)

    want = run(None)
    res = {"device": torch.cuda.get_device_name(0), "dtype": "float32", "batch": a.batch, "d_model": a.d_model, "d_inner": 2 * a.d_model,
           "d_state": a.d_state, "prompt": a.prompt, "allow_tf32": bool(torch.backends.cuda.matmul.allow_tf32)}
    t = timed(lambda: run(None))
    res["one_shot"] = {"ms_min": round(t[0], 4), "ms_median": round(t[1], 4), "peak_mb": round(peak_mb(lambda: run(None)), 2)}
    res["chunked"] = {}
    for chunk in (int(c) for c in a.chunks.split(",")):
        got = run(chunk)
        err = ((got - want).abs().max() / want.abs().max()).item()
        t = timed(lambda: run(chunk))
        res["chunked"][str(chunk)] = {"ms_min": round(t[0], 4), "ms_median": round(t[1], 4), "peak_mb": round(peak_mb(lambda: run(chunk)), 2),
                                      "ms_ratio_to_one_shot": round(t[0] / res["one_shot"]["ms_min"], 3), "max_err_rel_to_one_shot": err}
        del got
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
