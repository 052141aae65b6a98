"""Packed variable-length rows (seq_idx) on the GPU: the packed-row instantiations of csrc/causal_conv1d.hip and csrc/ssm_scan_general.hip
against the float64 restatements (pinned by test_varlen_cpu.py), with the kernels that were here before them as the yardstick.

The rule for everything a kernel writes in a fixed order (outputs, last_state, du, ddelta, dz, the conv's dx): every segment of a packed row
is also run ALONE through the existing non-packed entry point (for the scan: the general kernel family, which is what seq_idx runs on), and
    max |packed - float64| <= 2 x max over the segments |alone - float64| + one fp32 ulp of the largest reference value.
The factor 2 allows for a segment sitting at another tile phase than when it runs alone. Both errors are printed, and so is whether the packed
and the per-segment results are bit-identical (DESIGN.md section 3.18 records the finding; the bound is the pass condition).
What is summed with atomics (dB / dC, dA, dD, ddelta_bias, the conv's dweight / dbias) is not bit-repeatable: held against the float64 sum
over the segments under the tolerances test_scan_general_gpu.py uses for the same sums (_bwd_tol(L) for dB / dC, _bwd_tol(L, True) for the
sums over batch and time).
Contamination: the same packed rows twice, the first segment's inputs 1e3 times larger the second time: everything the later segments get
must be bit-identical. Model: the tiny LM fixture, packed documents against per-document runs under test_lm_gpu.py's model tolerance
(SSU_TOL[float32] under exact fp32) and test_cross_entropy_gpu.py's training-step rule (3e-4 of the largest gradient element; the loss,
a mean of the same per-token terms in another order, relative 3e-4)."""
import math

import pytest
import torch

from conftest import assert_close
from test_lm_gpu import gpu_model
from test_mixer_step_gpu import SSU_TOL, close, exact_fp32  # noqa: F401  (exact_fp32: a fixture)
from test_scan_gpu import _bwd_tol
from test_varlen_cpu import BATCHES, ROWS, ids_from, segments

pytestmark = pytest.mark.gpu
DEV = "cuda"
L = 37


def ulp32(x):
    """one fp32 ulp at |x|"""
    return 2.0 ** (math.floor(math.log2(max(float(x), 2.0 ** -126))) - 23)


def held(name, packed, alone, want, report):
    """the 2x rule of the module docstring for one quantity: packed / alone / want are lists of per-segment tensors"""
    e_p = max((p.double().cpu() - w).abs().max().item() for p, w in zip(packed, want))
    e_a = max((a.double().cpu() - w).abs().max().item() for a, w in zip(alone, want))
    big = max(w.abs().max().item() for w in want)
    bit = all(torch.equal(p, a) for p, a in zip(packed, alone))
    bound = 2 * e_a + ulp32(big)
    report.append(f"{name}: packed err {e_p:.3e}, per-segment err {e_a:.3e}, bound {bound:.3e}, bit-identical {bit}")
    return e_p <= bound, bit


def all_segments(seq):
    return [(r, s, e) for r in range(seq.shape[0]) for s, e in segments(seq[r])]


def cut(t, segs):
    """the per-segment pieces of a (batch, ..., seqlen) tensor"""
    return [t[r:r + 1, ..., s:e] for r, s, e in segs]


# ---- the conv ------------------------------------------------------------------------------------------------------------------------------------------
def conv_case(seq, dim, width, bias, act, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    B, Ln = seq.shape
    xz = torch.randn(B, 2 * dim, Ln, generator=g).to(dtype)                        # x is one half of an xz buffer: a strided view
    w, b = torch.randn(dim, width, generator=g), (torch.randn(dim, generator=g) if bias else None)
    dy = torch.randn(B, dim, Ln, generator=g).to(dtype)
    return xz, w, b, dy, act


def conv_reference(xz, w, b, dy, act, seq):
    from dimsum_amd.ops import causal_conv1d_varlen_torch
    dim = w.shape[0]
    x = xz[:, :dim].double().requires_grad_()
    w64, b64 = w.double().requires_grad_(), (b.double().requires_grad_() if b is not None else None)
    y = causal_conv1d_varlen_torch(x, w64, b64, act, seq)
    grads = torch.autograd.grad(y, [x, w64] + ([b64] if b is not None else []), dy.double())
    return y.detach(), grads


def run_conv(seq, dim, width, bias, act, seed):
    """-> (ok, report): forward and backward of the packed conv on one batch of rows against float64 and the per-segment plain kernel"""
    from dimsum_amd.ops import causal_conv1d_fn
    xz, w, b, dy, act = conv_case(seq, dim, width, bias, act, seed)
    want_y, want_g = conv_reference(xz, w, b, dy, act, seq)
    segs = all_segments(seq)
    xg = xz.to(DEV)
    x = xg[:, :dim].detach().requires_grad_()
    assert not x.is_contiguous()
    wg, bg, dyg, sq = w.to(DEV).requires_grad_(), (b.to(DEV).requires_grad_() if bias else None), dy.to(DEV), seq.to(DEV)
    y = causal_conv1d_fn(x, wg, bg, act, seq_idx=sq)
    got = torch.autograd.grad(y, [x, wg] + ([bg] if bias else []), dyg)
    alone_y, alone_dx = [], []
    for r, s, e in segs:                                                           # the kernel that was here before, one segment at a time
        xs = xg[r:r + 1, :dim, s:e].detach().requires_grad_()
        ys = causal_conv1d_fn(xs, wg, bg, act)
        alone_y.append(ys.detach())
        alone_dx.append(torch.autograd.grad(ys, xs, dyg[r:r + 1, :, s:e])[0])
    torch.cuda.synchronize()
    report, oks, bits = [], [], []
    for name, p, a, wnt in (("out", y.detach(), alone_y, want_y), ("dx", got[0], alone_dx, want_g[0])):
        ok, bit = held(f"conv W{width} dim{dim} {name}", cut(p, segs), a, cut(wnt, segs), report)
        oks.append(ok)
        bits.append(bit)
    tolw = _bwd_tol(seq.shape[1], True)
    assert_close(got[1].double().cpu().numpy(), want_g[1].numpy(), what="dweight", **tolw)
    if bias:
        assert_close(got[2].double().cpu().numpy(), want_g[2].numpy(), what="dbias", **tolw)
    return all(oks), report


@pytest.mark.parametrize("bias,act", [(True, "silu"), (False, None)], ids=["bias_silu", "plain"])
@pytest.mark.parametrize("width", [2, 3, 4])
def test_conv_packed_rows(width, bias, act):
    """batch 2, dim 64 and 72 (a partly filled block of rows), L = 37 on a strided view: every segmentation of test_varlen_cpu.ROWS"""
    lines, ok = [], True
    for dim in (64, 72):
        for i, names in enumerate(BATCHES):
            good, rep = run_conv(torch.stack([ROWS[n] for n in names]), dim, width, bias, act, seed=10 * width + i)
            ok, lines = ok and good, lines + [f"{'+'.join(names)} {line}" for line in rep]
    print("\n".join(lines))
    assert ok, "\n".join(lines)


def test_conv_boundaries_at_the_lane_and_step_halo():
    """L = 520 (the 16-byte path, three 256-element steps): boundaries at 255, 256, 257 -- lane 63 of the first step, lane 0 of the second
    (its halo comes across the step) and inside that lane -- and at 3, 4, 5, 256, 511, 512, 513 in the second row, with ids that come back"""
    seq = torch.stack([ids_from([255, 1, 1, 263]), ids_from([3, 1, 1, 251, 255, 1, 1, 7], [4, -1, 4, 9, 9 + 1, 3, 3 + 1, 0])])
    assert seq.shape == (2, 520)
    lines, ok = [], True
    for width, bias, act in ((4, True, "silu"), (3, False, None), (2, True, None)):
        good, rep = run_conv(seq, 64, width, bias, act, seed=width)
        ok, lines = ok and good, lines + rep
    print("\n".join(lines))
    assert ok, "\n".join(lines)


# ---- the scan ------------------------------------------------------------------------------------------------------------------------------------------
def scan_case(seq, dim, N, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    B, Ln = seq.shape
    mk = lambda *s: torch.randn(*s, generator=g)
    c = dict(u=mk(B, dim, Ln).to(dtype), delta=(0.5 * mk(B, dim, Ln)).to(dtype), A=-0.5 * torch.rand(dim, N, generator=g) - 0.05,
             B=mk(B, 1, N, Ln).to(dtype), C=mk(B, 1, N, Ln).to(dtype), D=mk(dim), z=mk(B, dim, Ln).to(dtype), delta_bias=0.3 * mk(dim))
    return c, mk(B, dim, Ln).to(dtype)


ORDER = ("u", "delta", "A", "B", "C", "D", "z", "delta_bias")


def scan_reference(c, dout, seq):
    from dimsum_amd.ops import selective_scan_varlen_torch
    leaves = {k: v.double().requires_grad_() for k, v in c.items()}
    y, last = selective_scan_varlen_torch(*(leaves[k] for k in ORDER), True, return_last_state=True, seq_idx=seq)
    grads = dict(zip(ORDER, torch.autograd.grad(y, [leaves[k] for k in ORDER], dout.double())))
    return y.detach(), last.detach(), grads


def run_scan(seq, dim, N, seed):
    """-> (ok, report) for one batch of rows: selective_scan_fn(seq_idx=...) with autograd against float64 and the per-segment general kernel"""
    from dimsum_amd import native
    from dimsum_amd.ops import selective_scan_fn
    c, dout = scan_case(seq, dim, N, seed)
    want_y, want_last, want_g = scan_reference(c, dout, seq)
    segs = all_segments(seq)
    g = {k: v.to(DEV).requires_grad_() for k, v in c.items()}
    dg, sq = dout.to(DEV), seq.to(DEV)
    y, last = selective_scan_fn(*(g[k] for k in ORDER), delta_softplus=True, return_last_state=True, seq_idx=sq)
    grads = dict(zip(ORDER, torch.autograd.grad(y, [g[k] for k in ORDER], dg)))
    alone = {k: [] for k in ("out", "last", "u", "delta", "z")}
    with torch.no_grad():
        for r, s, e in segs:                                                       # the general kernel that was here before, one segment at a time
            a = [g[k].detach()[r:r + 1, ..., s:e] if g[k].dim() >= 3 else g[k].detach() for k in ORDER]
            out, x, out_z = native.selective_scan_general_fwd(*a, True)
            du, ddelta, _, _, _, _, _, dz = native.selective_scan_general_bwd(*a, dg[r:r + 1, :, s:e], out, None, True)
            for k, v in (("out", out_z), ("last", x[:, :, -1, 1::2]), ("u", du), ("delta", ddelta), ("z", dz)):
                alone[k].append(v)
    torch.cuda.synchronize()
    report, oks = [], []
    oks.append(held(f"scan N{N} dim{dim} out", cut(y.detach(), segs), alone["out"], cut(want_y, segs), report)[0])
    for k in ("u", "delta", "z"):
        oks.append(held(f"scan N{N} dim{dim} d{k}", cut(grads[k], segs), alone[k], cut(want_g[k], segs), report)[0])
    last_segs = [(r, *segments(seq[r])[-1]) for r in range(seq.shape[0])]
    alone_last = [alone["last"][segs.index(t)] for t in last_segs]
    oks.append(held(f"scan N{N} dim{dim} last_state", [last[r:r + 1] for r in range(seq.shape[0])], alone_last,
                    [want_last[r:r + 1] for r in range(seq.shape[0])], report)[0])
    Ln = seq.shape[1]
    for k in ("B", "C"):
        assert_close(grads[k].double().cpu().numpy(), want_g[k].numpy(), what="d" + k, **_bwd_tol(Ln))
    for k in ("A", "D", "delta_bias"):
        assert_close(grads[k].double().cpu().numpy(), want_g[k].numpy(), what="d" + k, **_bwd_tol(Ln, True))
    return all(oks), report


@pytest.mark.parametrize("dim", [64, 72])
@pytest.mark.parametrize("N", [16, 64, 5], ids=["N16_one_wave", "N64_four_waves", "N5_ragged"])
def test_scan_packed_rows(N, dim):
    """batch 2, L = 37: every segmentation of test_varlen_cpu.ROWS; dstate 16 takes the general family too (seq_idx always does)"""
    lines, ok = [], True
    for i, names in enumerate(BATCHES):
        good, rep = run_scan(torch.stack([ROWS[n] for n in names]), dim, N, seed=N + i)
        ok, lines = ok and good, lines + [f"{'+'.join(names)} {line}" for line in rep]
    print("\n".join(lines))
    assert ok, "\n".join(lines)


def test_scan_boundaries_around_the_chunk_checkpoint():
    """batch 1, dim 64, L = 2056: boundaries at 2047, 2048 and 2049. The first chunk's checkpoint holds the state of the one-position segment
    [2047] and a running product of 0; the second one the last segment's state"""
    from dimsum_amd import native
    from dimsum_amd.ops import selective_scan_varlen_torch
    seq = ids_from([2047, 1, 1, 7])[None]
    good, rep = run_scan(seq, 64, 16, seed=4)
    print("\n".join(rep))
    assert good, "\n".join(rep)
    c, _ = scan_case(seq, 64, 16, seed=4)
    g = {k: v.to(DEV) for k, v in c.items()}
    out, x, out_z = native.selective_scan_varlen_fwd(*(g[k] for k in ORDER), True, seq.to(DEV))
    assert x.shape == (1, 64, 2, 32)
    c64 = {k: (v[..., :2048] if v.dim() >= 3 else v).double() for k, v in c.items()}
    _, h2047 = selective_scan_varlen_torch(*(c64[k] for k in ORDER), True, return_last_state=True, seq_idx=seq[:, :2048])
    err = (x[:, :, 0, 1::2].double().cpu() - h2047).abs().max().item()
    print(f"checkpoint state at 2047: max err {err:.3e} of {h2047.abs().max().item():.3e}")
    assert err <= 4 * 2.0 ** -24 * h2047.abs().max().item()          # one product dt B u: three roundings and the softplus
    assert bool((x[..., 0::2] == 0).all())                           # a boundary lies behind both chunk ends


# ---- 16 bits ---------------------------------------------------------------------------------------------------------------------------------------------
def test_bf16_forward():
    """bf16 I/O at one shape, forward only, at the per-dtype tolerance test_scan_general_gpu.py::test_half_dtypes uses (rtol 3e-2, atol 5e-2)"""
    from dimsum_amd.ops import causal_conv1d_fn, selective_scan_fn
    seq = torch.stack([ROWS[n] for n in BATCHES[0]])
    c, dout = scan_case(seq, 72, 16, seed=9, dtype=torch.bfloat16)
    want_y, want_last, _ = scan_reference({k: v.float() for k, v in c.items()}, dout.float(), seq)
    g = {k: v.to(DEV) for k, v in c.items()}
    y, last = selective_scan_fn(*(g[k] for k in ORDER), delta_softplus=True, return_last_state=True, seq_idx=seq.to(DEV))
    assert y.dtype == torch.bfloat16
    close(y, want_y, (3e-2, 5e-2), "bf16 scan")
    xz, w, b, dy, act = conv_case(seq, 72, 4, True, "silu", seed=9, dtype=torch.bfloat16)
    want, _ = conv_reference(xz.float(), w, b, dy.float(), act, seq)
    got = causal_conv1d_fn(xz.to(DEV)[:, :72], w.to(DEV), b.to(DEV), act, seq_idx=seq.to(DEV))
    assert got.dtype == torch.bfloat16
    close(got, want, (3e-2, 5e-2), "bf16 conv")


# ---- contamination -----------------------------------------------------------------------------------------------------------------------------------------
def test_later_segments_do_not_see_the_first_one():
    """the same packed rows twice, the first segment's inputs 1e3 times larger the second time: outputs and input gradients of every later
    position are bit-identical (a kernel that ignores seq_idx, or masks most of it, changes them)"""
    from dimsum_amd.ops import causal_conv1d_fn, selective_scan_fn
    seq = torch.stack([ROWS["inside_tiles"], ROWS["at_one_and_short_runs"]])
    first = [segments(seq[r])[0][1] for r in range(2)]                     # where each row's first segment ends: 5 and 1
    sq = seq.to(DEV)

    def blow(t):
        t = t.clone()
        for r, e in enumerate(first):
            t[r, ..., :e] *= 1e3
        return t

    def later(t):
        return [t[r, ..., e:] for r, e in enumerate(first)]

    for dim, N in ((72, 16), (64, 64), (64, 5), (72, 72)):                  # 72 states: the 1024-work-item builds, a half-empty fifth wave
        c, dout = scan_case(seq, dim, N, seed=dim + N)
        runs = []
        for big in (False, True):
            g = {k: ((blow(v) if big and v.dim() >= 3 else v).to(DEV).requires_grad_()) for k, v in c.items()}
            y = selective_scan_fn(*(g[k] for k in ORDER), delta_softplus=True, seq_idx=sq)
            du, ddelta, dz = torch.autograd.grad(y, [g["u"], g["delta"], g["z"]], dout.to(DEV))
            runs.append([y.detach(), du, ddelta, dz])
        for name, a, b in zip(("out", "du", "ddelta", "dz"), *runs):
            assert bool(torch.isfinite(b).all()), name
            assert all(torch.equal(p, q) for p, q in zip(later(a), later(b))), f"scan N{N}: {name} of a later segment changed"
        assert not torch.equal(runs[0][0][0, :, :first[0]], runs[1][0][0, :, :first[0]])
    for width in (2, 3, 4):
        xz, w, b, dy, act = conv_case(seq, 72, width, True, "silu", seed=width)
        runs = []
        for big in (False, True):
            x = (blow(xz) if big else xz).to(DEV)[:, :72].detach().requires_grad_()
            y = causal_conv1d_fn(x, w.to(DEV), b.to(DEV), act, seq_idx=sq)
            runs.append([y.detach(), torch.autograd.grad(y, x, dy.to(DEV))[0]])
        for name, a, b_ in zip(("out", "dx"), *runs):
            assert all(torch.equal(p, q) for p, q in zip(later(a), later(b_))), f"conv W{width}: {name} of a later segment changed"


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------------------
DOCS = [[5, 1, 11], [9, 8]]


def packed_ids(vocab=90, seed=3):
    from dimsum_amd.utils import seq_idx_from_lengths
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, vocab, (len(DOCS), sum(DOCS[0])), generator=g)
    return ids.to(DEV), torch.stack([seq_idx_from_lengths(d) for d in DOCS]).to(DEV)


def documents():
    return [(r, sum(d[:i]), sum(d[:i + 1])) for r, d in enumerate(DOCS) for i in range(len(d))]


def test_model_packed_logits_loss_and_gradients(exact_fp32):  # noqa: F811
    from dimsum_amd.utils import packed_labels
    m, _ = gpu_model(1, 1)
    ids, seq = packed_ids()
    with torch.no_grad():
        logits = m(ids, seq_idx=seq).logits
        for r, s, e in documents():
            close(logits[r:r + 1, s:e], m(ids[r:r + 1, s:e]).logits, SSU_TOL[torch.float32], f"logits of document ({r}, {s}:{e})")
    m.train()
    loss = m.loss(ids, packed_labels(ids, seq), seq_idx=seq)
    loss.backward()
    got = {k: p.grad.clone() for k, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    total, count = 0.0, 0
    for r, s, e in documents():
        if e - s > 1:
            part = m.loss(ids[r:r + 1, s:e], reduction="sum")
            part.backward()                                                # accumulates: the sum over the documents
            total, count = total + part.item(), count + e - s - 1
    want = total / count
    print(f"packed loss {loss.item():.6f}, token-weighted per-document mean {want:.6f}")
    assert abs(loss.item() - want) <= 3e-4 * abs(want)
    for k, p in m.named_parameters():
        ref = p.grad / count
        err, scale = (got[k] - ref).abs().max().item(), ref.abs().max().item()
        assert err <= 3e-4 * scale, f"{k}: max |err| {err:.3e} against max |grad| {scale:.3e}"


def padded_prompts():
    """two prompts of 3 and 9 tokens, the short one left-padded to 9 with its padding as a segment of its own"""
    from dimsum_amd.utils import seq_idx_from_lengths
    g = torch.Generator().manual_seed(5)
    long, short = torch.randint(0, 90, (9,), generator=g), torch.randint(0, 90, (3,), generator=g)
    ids = torch.stack([torch.cat([torch.zeros(6, dtype=torch.long), short]), long]).to(DEV)
    seq = torch.stack([seq_idx_from_lengths([6, 3]), seq_idx_from_lengths([9])]).to(DEV)
    return ids, seq, [short[None].to(DEV), long[None].to(DEV)]


def test_left_padded_prefill_and_generate(exact_fp32):  # noqa: F811
    from dimsum_amd.utils import InferenceParams
    m, _ = gpu_model(1, 1)
    ids, seq, alone = padded_prompts()
    tol = SSU_TOL[torch.float32]
    with torch.no_grad():
        p = InferenceParams(max_seqlen=16, max_batch_size=2)
        last = m(ids, inference_params=p, num_last_tokens=1, seq_idx=seq).logits[:, -1]
        for r, prompt in enumerate(alone):
            q = InferenceParams(max_seqlen=16, max_batch_size=1)
            close(last[r:r + 1], m(prompt, inference_params=q, num_last_tokens=1).logits[:, -1], tol, f"last-position logits of prompt {r}")
            for layer, (conv_state, ssm_state) in p.key_value_memory_dict.items():
                close(conv_state[r:r + 1], q.key_value_memory_dict[layer][0], tol, f"conv_state of layer {layer}, prompt {r}")
                close(ssm_state[r:r + 1], q.key_value_memory_dict[layer][1], tol, f"ssm_state of layer {layer}, prompt {r}")
        p.seqlen_offset = 9
        with pytest.raises(ValueError, match="seqlen_offset > 0"):
            m(ids[:, :1], inference_params=p, seq_idx=seq[:, :1])
    # greedy decoding: meaningful only where the logit errors stay well inside the gap between the two best tokens (test_lm_gpu.py's precondition)
    packed = m.generate(ids, max_length=13, top_k=1, seq_idx=seq, return_dict_in_generate=True, output_scores=True)
    assert packed.sequences.shape == (2, 13)
    for r, prompt in enumerate(alone):
        one = m.generate(prompt, max_length=prompt.shape[1] + 4, top_k=1, return_dict_in_generate=True, output_scores=True)
        scores = torch.stack(one.scores, 1)[0]
        top2 = scores.topk(2, -1).values
        gap = (top2[:, 0] - top2[:, 1]).min().item()
        err = (torch.stack(packed.scores, 1)[r] - scores).abs().max().item()
        print(f"prompt {r}: max |logit error| {err:.3e}, min_gap {gap:.3e}")
        assert err < gap / 4
        assert torch.equal(packed.sequences[r, 9:], one.sequences[0, prompt.shape[1]:])


# ---- seq_idx=None launches what the parent launches ---------------------------------------------------------------------------------------------------------
class _LibSpy:
    """the loaded library with every launch entry point recorded by name"""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("dimsum_") or name.endswith(("_bytes", "_variant", "_kernel_for", "_string", "_version", "_arch")):
            return fn

        def call(*a):
            self._log.append(name)
            return fn(*a)
        return call


def test_no_seq_idx_launches_are_the_parents(monkeypatch):
    """one mixer forward + backward: without seq_idx (and with seq_idx=None) the conv and the scan are the plain conv kernel and the TUNED
    scan kernels, one launch each way, and no packed-row entry point is reached; with seq_idx the same pass runs the four packed-row ones"""
    from dimsum_amd import _lib
    from dimsum_amd.modules.mamba_simple import Mamba
    torch.manual_seed(0)
    m = Mamba(64, d_state=16, d_conv=4, expand=2, layer_idx=0).to(DEV)
    x = torch.randn(2, 24, 64, device=DEV, requires_grad=True)
    seq = torch.stack([ids_from([10, 14]), ids_from([24])]).to(DEV)
    lib, logs = _lib.load(), {}
    for key, kw in (("absent", {}), ("none", {"seq_idx": None}), ("packed", {"seq_idx": seq})):
        log = logs[key] = []
        monkeypatch.setattr(_lib, "load", lambda _l=log: _LibSpy(lib, _l))
        m(x, **kw).sum().backward()
        torch.cuda.synchronize()
    monkeypatch.undo()
    core = lambda log: [n for n in log if "conv1d" in n or "ssm_scan" in n]
    assert logs["none"] == logs["absent"]
    assert core(logs["absent"]) == ["dimsum_causal_conv1d_fwd", "dimsum_ssm_scan_fwd", "dimsum_ssm_scan_bwd", "dimsum_causal_conv1d_bwd"]
    assert core(logs["packed"]) == ["dimsum_causal_conv1d_varlen_fwd", "dimsum_ssm_scan_varlen_fwd", "dimsum_ssm_scan_varlen_bwd",
                                    "dimsum_causal_conv1d_varlen_bwd"]
