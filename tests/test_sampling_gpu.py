"""dimsum_sample_logits (csrc/sample_logits.hip) on the GPU against `sample_logits_torch`, the float64 yardstick of test_sampling_cpu.py: exact
token equality on inputs built so that the float64 reference alone decides, the tie / -inf / NaN / u-edge rules, determinism, the
row_index / out_table seam, the distribution over 65 536 draws, and generate() with the sampler eager and inside the captured step.

How the inputs make the reference decide (asserted on the reference before anything is launched):
  (a) the logits of a row are distinct -- Gaussian, standard deviation 4, duplicates redrawn. In float16 / bfloat16 this is only possible for
      small V (bfloat16 has 256 values in 2 <= |x| < 4, where a third of the draws fall): it is asserted for float32 at every V and for the
      16-bit types at V <= 257; the 16-bit rows of 4096 and more logits have equal logits by pigeonhole, and there the documented rank rule
      (ascending index among equals), which the yardstick states with a stable sort, decides;
  (b) u is the fp32 rounding of the midpoint of the target token's CDF interval, for targets of probability >= 4e-4: at least 1e-4 from
      either end, about 8x the issue's a-priori fp32 bound of a blocked sum of 50 288 terms (1.2e-5; the kernel's own bound is smaller:
      its sums are exact integers);
  (c) top_p is the midpoint of two adjacent descending exclusive cumulative masses at least 2e-4 apart, chosen so that it also stays 1e-4
      away from every such mass of every row of the launch (top_p is one number per launch)."""
import functools

import pytest
import torch

from conftest import golden
from test_lm_cpu import PROMPT, STEPS, tiny_model
from test_mixer_step_gpu import exact_fp32  # noqa: F401  (a fixture)
from test_sampling_cpu import U_MAX, sample_logits_torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = torch.from_numpy
INF = float("inf")
ROWS_MAX = 16
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
VOCABS = [1, 7, 64, 257, 4096, 4097, 50280]
P_MIN, U_MARGIN, P_GAP = 4e-4, 1e-4, 2e-4


def native():
    from dimsum_amd import native as n
    return n


def stride_of(V):
    return 50288 if V == 50280 else V


def make_logits(V, dtype, seed=0):
    """(ROWS_MAX, stride_of(V)) of dtype on the CPU: Gaussian with standard deviation 4, duplicates within a row redrawn while that can work;
    the padding columns hold 100, which would win every argmax if it were read"""
    g = torch.Generator().manual_seed(seed * 1000 + V)
    x = (torch.randn(ROWS_MAX, V, generator=g) * 4).to(dtype)
    for r in range(ROWS_MAX if distinct_is_possible(V, dtype) else 0):
        for _ in range(200):
            srt, order = torch.sort(x[r].float(), stable=True)
            dup = order[1:][srt[1:] == srt[:-1]]
            if dup.numel() == 0:
                break
            x[r, dup] = (torch.randn(dup.numel(), generator=g) * 4).to(dtype)
    buf = torch.full((ROWS_MAX, stride_of(V)), 100.0, dtype=dtype)
    buf[:, :V] = x
    return buf


def distinct_is_possible(V, dtype):
    return dtype == torch.float32 or V <= 257


def effective_k(top_k, V):
    return 0 if top_k <= 0 or top_k >= V else top_k


@functools.lru_cache(maxsize=None)
def case(V, dtype):
    """the shared reference of one (V, dtype): the logits, and per (effective top_k, temperature) the launch's top_p (c) and per
    (effective top_k, cut by top_p or not, temperature) and row up to three (token, u) targets: the first, a middle and the last kept
    index of probability >= P_MIN. Computed once, never changed."""
    buf = make_logits(V, dtype)
    x = buf[:, :V]
    if distinct_is_possible(V, dtype):
        for r in range(ROWS_MAX):
            assert torch.unique(x[r].double()).numel() == V, "(a): distinct logits within a row"
    ref = {"logits": buf, "top_p": {}, "targets": {}}

    def distribution(r, k, top_p, temp):
        d = []
        sample_logits_torch(x[r:r + 1], torch.tensor([0.5]), k, top_p, temp, details=d)
        return d[0][0], d[0][1]

    def targets_of(kept, p):
        cdf = torch.cumsum(p, 0)
        big = torch.nonzero(p >= P_MIN)[:, 0].tolist()
        out = []
        for j in sorted({big[0], big[len(big) // 2], big[-1]}) if big else []:
            lo, hi = (float(cdf[j - 1]) if j else 0.0), float(cdf[j])
            u = torch.tensor((lo + hi) / 2, dtype=torch.float64).float().item()
            assert lo + U_MARGIN <= u <= hi - U_MARGIN and u < 1.0, "(b): u at least 1e-4 inside the target's CDF interval"
            out.append((int(kept[j]), u))
        return out

    for k in sorted({effective_k(t, V) for t in (2, 50, 0)}):
        for temp in (1.0, 0.7):
            masses = []
            for r in range(ROWS_MAX):
                kept, p = distribution(r, k, 0.0, temp)
                ref["targets"][k, False, temp, r] = targets_of(kept, p)
                desc = torch.sort(p, descending=True).values
                masses.append(torch.cumsum(desc, 0) - desc)
            # (c): a midpoint of adjacent masses of some row, nearest 0.6, that keeps its distance from every mass of every row
            mids = torch.cat([(m[1:] + m[:-1])[(m[1:] - m[:-1]) >= P_GAP] / 2 for m in masses])
            top_p = None
            for mid in mids[torch.argsort((mids - 0.6).abs())].tolist():
                if all(float((m - mid).abs().min()) >= U_MARGIN for m in masses) and 0.0 < mid < 1.0:
                    top_p = torch.tensor(mid).float().item()
                    break
            if top_p is None:                       # V == 1: a single mass, nothing to cut between
                assert V == 1
                top_p = 0.5
            for m in masses:
                assert V == 1 or float((m - top_p).abs().min()) >= U_MARGIN * 0.999, "(c): top_p 1e-4 away from every cumulative mass"
            ref["top_p"][k, temp] = top_p
            for r in range(ROWS_MAX):
                ref["targets"][k, True, temp, r] = targets_of(*distribution(r, k, top_p, temp))
    return ref


def launch(x, u, **kw):
    return native().sample_logits(x, u, **kw)


# ---- against the yardstick -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("rows", [1, 3, 16])
@pytest.mark.parametrize("V", VOCABS)
def test_tokens_equal_the_float64_yardstick(V, rows, dtype):
    ref = case(V, dtype)
    x = ref["logits"].to(DEV)[:rows, :V]
    argmax = torch.tensor([sample_logits_torch(ref["logits"][r:r + 1, :V], None, top_k=1).item() for r in range(rows)])
    checked = 0
    for top_k in (1, 2, 50, V, V + 5, 0):
        k = effective_k(top_k, V)
        for temp in (1.0, 0.7):
            for top_p, cut in ((0.0, False), (ref["top_p"].get((k, temp), 0.5), True), (1.0, False)):
                if top_k == 1:
                    got = launch(x, None, top_k=1, top_p=top_p, temperature=temp).cpu()
                    assert torch.equal(got, argmax), (top_k, top_p, temp)
                    continue
                per_row = [ref["targets"][k, cut, temp, r] for r in range(rows)]
                for which in range(3):                                          # first / middle / last target of every row in one launch
                    pick = [t[min(which, len(t) - 1)] for t in per_row]
                    u = torch.tensor([p[1] for p in pick], dtype=torch.float32, device=DEV)
                    got = launch(x, u, top_k=top_k, top_p=top_p, temperature=temp).cpu()
                    want = torch.tensor([p[0] for p in pick])
                    assert torch.equal(got, want), (top_k, top_p, temp, which, got.tolist(), want.tolist())
                    checked += rows
    assert checked == sum(t != 1 for t in (1, 2, 50, V, V + 5, 0)) * 2 * 3 * 3 * rows
    if V > 1 and dtype == torch.float32:
        assert max(len(t) for key, t in ref["targets"].items() if key[0] == 0 and not key[1]) >= 2      # first and last differ: u decides


# ---- rules and edges -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [7, 4097])
def test_ties_rank_by_ascending_index(V):
    x = torch.randn(3, V, generator=torch.Generator().manual_seed(5))
    x[:, [2, 5, V - 1]] = 9.0                                                  # three equal maxima
    xd = x.to(DEV)
    assert launch(xd, None, top_k=1).tolist() == [2, 2, 2]
    # a tie across the top_k = 2 cut keeps indices 2 and 5: whatever u, never V - 1; the ends of u reach both
    for uv, want in ((0.0, 2), (U_MAX, 5), (0.49, 2), (0.51, 5)):
        u = torch.full((3,), uv, device=DEV)
        assert launch(xd, u, top_k=2).tolist() == [want] * 3
        assert launch(xd, u, top_k=2).tolist() == sample_logits_torch(x, u.cpu(), top_k=2).tolist()
    # the same tie at the top_p cut: the three maxima hold almost all the mass, a third each; top_p 0.5 keeps two of them
    for uv, want in ((0.0, 2), (U_MAX, 5)):
        u = torch.full((3,), uv, device=DEV)
        assert launch(xd + 20 * (xd == 9.0), u, top_k=0, top_p=0.5).tolist() == [want] * 3


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("V", [7, 257, 4097])
def test_masked_rows_nan_and_the_ends_of_u(V, dtype):
    g = torch.Generator().manual_seed(9)
    x = torch.randn(4, V, generator=g).to(dtype)
    masked = torch.rand(4, V, generator=g) < 0.5
    masked[:, 3] = False
    x[masked] = -INF
    x[2] = -INF                                                                # a row of all -inf
    x[3, 1] = float("nan")                                                     # NaN counts as -inf
    x[3, 5:] = float("nan")
    xd = x.to(DEV)
    for top_k, top_p in ((0, 0.0), (3, 0.0), (0, 0.8), (V + 5, 1.0)):
        for uv in (0.0, 0.3, U_MAX, 1.0, 2.5, -1.0, float("nan")):
            u = torch.full((4,), uv)
            got = launch(xd, u.to(DEV), top_k=top_k, top_p=top_p, temperature=0.7).cpu()
            assert bool(((got >= 0) & (got < V)).all())
            assert got[2].item() == 0                                          # no finite logit
            for r in (0, 1, 3):
                assert torch.isfinite(x[r, got[r]].float()), (r, got[r])       # never a masked token
            details = []
            sample_logits_torch(x, u, top_k, top_p, 0.7, details=details)
            if uv in (0.0, -1.0) or uv != uv:
                assert got[:2].tolist() == [int(d[0][torch.nonzero(d[1] > 0)[0, 0]]) for d in details[:2]]     # the first kept index
            if uv >= U_MAX:
                assert got[:2].tolist() == [int(d[0][torch.nonzero(d[1] > 0)[-1, 0]]) for d in details[:2]]    # the last kept index
    assert launch(torch.full((2, V), float("nan"), dtype=dtype, device=DEV), torch.rand(2, device=DEV), top_k=0).tolist() == [0, 0]
    inf_row = x.clone()
    inf_row[:, 4] = INF                                                        # +inf takes all the mass
    assert launch(inf_row.to(DEV), torch.rand(4, device=DEV), top_k=0, top_p=0.9).tolist() == [4, 4, 4, 4]


# ---- determinism -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("V", [257, 4097, 50280])
def test_launches_rows_and_alignment_do_not_change_a_token(V, dtype):
    ref = case(V, dtype)
    x = ref["logits"].to(DEV)[:, :V]
    u = torch.rand(ROWS_MAX, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    for kw in (dict(top_k=0), dict(top_k=50, top_p=0.9, temperature=0.8), dict(top_k=0, top_p=0.9), dict(top_k=1)):
        a = launch(x, u, **kw)
        assert torch.equal(a, launch(x, u, **kw))                              # two launches are bit-identical
        assert launch(x[11:12], u[11:12], **kw).item() == a[11].item()          # row 11 of 16 alone
        flat = torch.zeros(ROWS_MAX * (stride_of(V) + 8) + 1, dtype=dtype, device=DEV)
        off = flat[1:].view(ROWS_MAX, stride_of(V) + 8)[:, :V]                  # every row starts one element off 16-byte alignment
        assert off.data_ptr() % 16 != 0
        off.copy_(x)
        assert torch.equal(launch(off, u, **kw), a)


def test_row_index_and_out_table_file_one_step():
    ref = case(257, torch.float32)
    x = ref["logits"].to(DEV)[:3, :257]
    table_u = torch.rand(5, 3, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
    tokens = torch.full((5, 3), -7, dtype=torch.long, device=DEV)
    step = torch.tensor([3], device=DEV)
    out = torch.zeros(3, 1, dtype=torch.long, device=DEV)
    got = launch(x, table_u, top_k=0, top_p=0.9, out=out, row_index=step, out_table=tokens)
    want = launch(x, table_u[3].contiguous(), top_k=0, top_p=0.9)
    assert got is out and torch.equal(out[:, 0], want) and torch.equal(tokens[3], want)
    assert bool((tokens[[0, 1, 2, 4]] == -7).all()) and step.item() == 3
    for bad, clamped in ((-2, 0), (9, 4)):                                     # a step outside the table is clamped into it: nothing beyond is touched
        tokens.fill_(-7)
        launch(x, table_u, top_k=0, out=out, row_index=torch.tensor([bad], device=DEV), out_table=tokens)
        assert torch.equal(tokens[clamped], launch(x, table_u[clamped].contiguous(), top_k=0))
        assert int((tokens == -7).sum()) == 12


# ---- the distribution ------------------------------------------------------------------------------------------------------------------------------
def test_frequencies_over_65536_rows():
    row = torch.tensor([0.3, -1.2, 2.0, 0.9, -0.4, 1.4, -2.5, 0.0])
    n = 65536
    u = torch.rand(n, device=DEV, generator=torch.Generator(DEV).manual_seed(1234))
    got = launch(row.to(DEV).repeat(n, 1), u, top_k=0, top_p=0.0)
    assert bool(((got >= 0) & (got < 8)).all())
    p = torch.softmax(row.double(), 0)
    freq = torch.bincount(got.cpu(), minlength=8).double() / n
    sd = torch.sqrt(p * (1 - p) / n)
    print("frequency - p in standard deviations:", ((freq - p) / sd).tolist())
    assert bool(((freq - p).abs() <= 5 * sd).all())


# ---- the model -------------------------------------------------------------------------------------------------------------------------------------
def gpu_model():
    g = golden("lm_tiny_rms1_fp32res1")
    return tiny_model(1, 1, g).to(DEV), T(g["prompt"]).to(DEV)


def test_greedy_inside_the_graph_equals_the_unfused_graph(exact_fp32):  # noqa: F811
    m, prompt = gpu_model()
    L = PROMPT + STEPS + 1
    unfused = m.generate(prompt, max_length=L, cg=True, return_dict_in_generate=True, output_scores=True)
    fused = m.generate(prompt, max_length=L, cg=True, fused_sampling=True, top_k=1, return_dict_in_generate=True, output_scores=True)
    assert torch.equal(fused.sequences, unfused.sequences) and len(fused.scores) == STEPS + 1
    assert all(torch.equal(a, b) for a, b in zip(fused.scores, unfused.scores))
    assert torch.equal(m.generate(prompt, max_length=L, cg=True, fused_sampling=True, vocab_size=90), unfused.sequences)
    assert m.generate(prompt, max_length=L, cg=True, fused_sampling=True, return_dict_in_generate=True).scores is None


def test_sampled_decoding_eager_and_graph_agree_and_captures_are_keyed(exact_fp32):  # noqa: F811
    from dimsum_amd.utils.generation import sample_fused
    m, prompt = gpu_model()
    L = PROMPT + STEPS + 1
    table = torch.rand(L, 2, device=DEV, generator=torch.Generator(DEV).manual_seed(21))
    kw = dict(max_length=L, fused_sampling=True, top_k=5, top_p=0.9, temperature=0.8, uniforms=table, return_dict_in_generate=True, output_scores=True)
    eager = m.generate(prompt, **kw)
    graph = m.generate(prompt, cg=True, **kw)
    assert torch.equal(eager.sequences, graph.sequences) and len(eager.scores) == len(graph.scores) == STEPS + 1
    assert all(torch.equal(a, b) for a, b in zip(eager.scores, graph.scores))  # bit-identical scores
    for i, s in enumerate(graph.scores):                                       # each step's token from its own scores and its own uniforms
        assert torch.equal(graph.sequences[:, PROMPT + i], sample_fused(s, table[i].contiguous(), 5, 0.9, 0.8))
        assert torch.equal(graph.sequences[:, PROMPT + i].cpu(), sample_logits_torch(s.cpu(), table[i].cpu(), 5, 0.9, 0.8))
    cache = m._decoding_cache
    assert cache.n_captures == 1 and list(cache.callables) == [(2, 1, 5, 0.9, 0.8, None)]
    again = m.generate((prompt + 5) % 90, cg=True, **kw)
    assert m._decoding_cache is cache and cache.n_captures == 1                 # the same shape and parameters: nothing new captured
    assert torch.equal(again.sequences, m.generate((prompt + 5) % 90, **kw).sequences)
    other = m.generate(prompt, cg=True, **dict(kw, top_p=0.5))
    assert cache.n_captures == 2                                               # another top_p is another graph node
    assert torch.equal(other.sequences, m.generate(prompt, **dict(kw, top_p=0.5)).sequences)
    plain = m.generate(prompt, max_length=L, cg=True)                          # the graph without a sampler is keyed apart
    assert cache.n_captures == 3 and (2, 1) in cache.callables and torch.equal(plain, m.generate(prompt, max_length=L))
    assert torch.equal(m.generate(prompt, cg=True, **kw).sequences, eager.sequences) and cache.n_captures == 3


def test_both_paths_stop_at_the_same_eos(exact_fp32):  # noqa: F811
    m, prompt = gpu_model()
    L = PROMPT + STEPS + 1
    table = torch.rand(L, 1, device=DEV, generator=torch.Generator(DEV).manual_seed(8))
    kw = dict(max_length=L, fused_sampling=True, top_k=5, top_p=0.9, temperature=0.8, uniforms=table)
    full = m.generate(prompt[:1], **kw)
    eos = int(full[0, PROMPT + 3])                                             # a token the pinned run does emit
    first = (full[0, PROMPT:] == eos).nonzero()[0, 0].item()
    eager = m.generate(prompt[:1], eos_token_id=eos, **kw)
    graph = m.generate(prompt[:1], eos_token_id=eos, cg=True, **kw)
    assert eager.shape == graph.shape == (1, PROMPT + first + 1) and torch.equal(eager, graph) and torch.equal(eager, full[:, :PROMPT + first + 1])
