"""The fused token sampler without a GPU: `sample_logits_torch`, the float64 statement of dimsum_sample_logits' semantics (rank, cut, inverse
CDF in index order) that the GPU tests compare the kernel with, against the distribution of the existing `sample()` on hand-computed rows;
the C ABI checks of dimsum_sample_logits in their documented order with host pointers that are never dereferenced, nothing launched, and
the struct mirror against the header; decode / generate with native.sample_logits replaced by the yardstick on the lm_tiny fixtures."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import golden
from oracle.torch_backend import cpu_oracle_backend
from test_host_logic import _header_layout
from test_lm_cpu import PROMPT, STEPS, decode_linear_torch, tiny_model
from test_mixer_step_cpu import native_conv_update, native_state_update

T = torch.from_numpy
INF = float("inf")
U_MAX = 1.0 - 2.0 ** -24


def sample_logits_torch(logits, u, top_k=1, top_p=0.0, temperature=1.0, out=None, row_index=None, out_table=None, details=None):
    """native.sample_logits restated in float64 straight from the semantics in include/dimsum_hip.h: same signature, same writes.
    details: a list that receives per row (kept indices ascending, their probabilities, the token), for the tests that look inside"""
    x = logits.detach().to("cpu", torch.float64)
    x = torch.where(torch.isnan(x), torch.full_like(x, -INF), x)
    M, V = x.shape
    step = None if row_index is None else int(row_index.item())
    uu = None if u is None else (u if step is None else u[step]).detach().to("cpu", torch.float64)
    toks = []
    for r in range(M):
        row = x[r]
        order = torch.sort(row, descending=True, stable=True).indices          # RANK: descending logit, ascending index among equals
        mx = row[order[0]]
        if top_k == 1 or V == 1 or mx == -INF:
            toks.append(int(order[0]) if mx > -INF else 0)
            if details is not None:
                details.append((order[:1].clone(), torch.ones(1, dtype=torch.float64), toks[-1]))
            continue
        kept = order[:V if top_k <= 0 or top_k >= V else top_k]
        w = torch.where(row[kept] == mx, torch.ones((), dtype=torch.float64), torch.exp((row[kept] - mx) / temperature))
        p = w / w.sum()
        if 0.0 < top_p < 1.0:
            above = torch.cumsum(p, 0) - p                                     # the kept-set mass ranked strictly above
            stay = above < top_p
            kept, p = kept[stay], p[stay] / p[stay].sum()
        by_index = torch.sort(kept).indices
        kept, p = kept[by_index], p[by_index]
        cdf = torch.cumsum(p, 0)
        ur = min(max(float(uu[r]), 0.0), U_MAX) if uu[r] == uu[r] else 0.0
        hit = torch.nonzero(cdf > ur)
        tok = int(kept[hit[0, 0]]) if hit.numel() else int(kept[torch.nonzero(p > 0)[-1, 0]])
        toks.append(tok)
        if details is not None:
            details.append((kept, p, tok))
    res = torch.tensor(toks, dtype=torch.int64, device=logits.device)
    if out is not None:
        out.view(-1).copy_(res)
    if out_table is not None:
        out_table[step].copy_(res)
    return res if out is None else out


# ---- the yardstick against sample() ----------------------------------------------------------------------------------------------------------------
def sample_distribution(row, top_k, top_p, temperature):
    """{token: probability} of the existing `sample()`: its own steps up to the multinomial draw"""
    from dimsum_amd.utils.generation import modify_logits_for_top_p_filtering
    logits = row[None].clone()
    if top_k > 0:
        vals, idx = torch.topk(logits, min(top_k, logits.shape[-1]), dim=-1)
        vals = vals / temperature
        modify_logits_for_top_p_filtering(vals, top_p)
        p = torch.softmax(vals, dim=-1)[0]
        return {int(i): float(q) for i, q in zip(idx[0], p) if q > 0}
    vals = logits / temperature
    modify_logits_for_top_p_filtering(vals, top_p)
    p = torch.softmax(vals, dim=-1)[0]
    return {i: float(q) for i, q in enumerate(p) if q > 0}


HAND_ROWS = [torch.log(torch.tensor([0.04, 0.30, 0.11, 0.25, 0.20, 0.10], dtype=torch.float64)),
             torch.tensor([1.5, -0.25, 3.0, 0.75, 2.5, -2.0, 2.0, 0.0], dtype=torch.float64),
             torch.randn(33, dtype=torch.float64, generator=torch.Generator().manual_seed(2)) * 2]


@pytest.mark.parametrize("temperature", [1.0, 0.7])
@pytest.mark.parametrize("top_p", [0.0, 0.6])
@pytest.mark.parametrize("top_k", [0, 3])
def test_yardstick_has_the_distribution_of_sample(top_k, top_p, temperature):
    for row in HAND_ROWS:
        want = sample_distribution(row, top_k, top_p, temperature)
        details = []
        sample_logits_torch(row[None], torch.tensor([0.5]), top_k, top_p, temperature, details=details)
        kept, p, _ = details[0]
        assert sorted(want) == kept.tolist(), (top_k, top_p, temperature)
        assert np.allclose([want[int(v)] for v in kept], p.numpy(), rtol=1e-12, atol=0)
    # the first hand row by hand: probabilities 0.30 0.25 0.20 0.11 0.10 0.04; top_p 0.6 at temperature 1 keeps 0.30 0.25 0.20 (0.55 < 0.6 above the third)
    if (top_k, temperature) == (0, 1.0):
        details = []
        sample_logits_torch(HAND_ROWS[0][None], torch.tensor([0.5]), 0, top_p, 1.0, details=details)
        kept, p, tok = details[0]
        if top_p == 0.6:
            assert kept.tolist() == [1, 3, 4] and np.allclose(p.numpy(), np.array([0.30, 0.25, 0.20]) / 0.75, rtol=1e-12)
            assert tok == 3                                                  # index order: 0.4, 0.733, 1: 0.5 falls on token 3
        else:
            assert kept.tolist() == list(range(6)) and tok == 3               # 0.04 0.34 0.45 0.70: 0.5 falls on token 3


def test_yardstick_rules():
    u = torch.tensor([0.3])
    tied = torch.tensor([[1.0, 5.0, 2.0, 5.0, 5.0, 0.0]])
    assert sample_logits_torch(tied, None, top_k=1).tolist() == [1]            # the lowest index among equal maxima
    details = []
    sample_logits_torch(tied, u, top_k=2, details=details)
    assert details[0][0].tolist() == [1, 3]                                     # a tie across the cut keeps the lowest indices
    masked = torch.tensor([[-INF, 0.0, -INF, 1.0]])
    for uu in (0.0, 0.5, U_MAX, 1.0, 7.0):
        assert sample_logits_torch(masked, torch.tensor([uu]), top_k=0).item() in (1, 3)
    assert sample_logits_torch(masked, torch.tensor([0.0]), top_k=0).item() == 1 and sample_logits_torch(masked, torch.tensor([1.0]), top_k=0).item() == 3
    assert sample_logits_torch(torch.full((1, 5), -INF), u, top_k=0).item() == 0
    assert sample_logits_torch(torch.tensor([[float("nan"), float("nan")]]), u, top_k=0).item() == 0
    assert sample_logits_torch(torch.tensor([[float("nan"), 0.5, float("nan")]]), u, top_k=0).item() == 1      # NaN counts as -inf
    table, idx = torch.full((5, 3), -1), torch.tensor([3])
    uu = torch.rand(5, 3, generator=torch.Generator().manual_seed(0))
    x = torch.randn(3, 9, generator=torch.Generator().manual_seed(1))
    out = torch.zeros(3, 1, dtype=torch.int64)
    got = sample_logits_torch(x, uu, top_k=0, out=out, row_index=idx, out_table=table)
    assert got is out and torch.equal(table[3], out[:, 0]) and torch.equal(out[:, 0], sample_logits_torch(x, uu[3], top_k=0))
    assert bool((table[[0, 1, 2, 4]] == -1).all())


# ---- the wrapper and the C ABI -----------------------------------------------------------------------------------------------------------------
def test_wrapper_refuses_clearly():
    from dimsum_amd import native
    x, u = torch.zeros(4, 8), torch.zeros(4)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        native.sample_logits(x, u, top_k=0)
    with pytest.raises(RuntimeError, match="float32, float16 or bfloat16"):
        native.sample_logits(x.double(), u)
    with pytest.raises(RuntimeError, match="unit column stride"):
        native.sample_logits(torch.zeros(8, 4).t(), u)
    with pytest.raises(RuntimeError, match="row stride >= vocab"):
        native.sample_logits(torch.zeros(1, 8).expand(4, 8), u)
    with pytest.raises(RuntimeError, match="temperature"):
        native.sample_logits(x, u, temperature=0.0)
    with pytest.raises(RuntimeError, match="u is required"):
        native.sample_logits(x, None, top_k=5)
    with pytest.raises(RuntimeError, match="u must be contiguous float32"):
        native.sample_logits(x, u.double(), top_k=5)
    with pytest.raises(RuntimeError, match="out_table needs row_index"):
        native.sample_logits(x, u, out_table=torch.zeros(2, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="out must be"):
        native.sample_logits(x, u, out=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="u must be \\(steps, rows\\)"):
        native.sample_logits(x, u, row_index=torch.zeros(1, dtype=torch.int64))


def test_struct_layout_and_export():
    from dimsum_amd import _lib
    size, offs = _header_layout([("dimsum_sample_logits_params_t", _lib.SampleLogitsParams)])["dimsum_sample_logits_params_t"]
    assert size == ctypes.sizeof(_lib.SampleLogitsParams) == _lib.SampleLogitsParams().struct_size
    assert offs == {f: getattr(_lib.SampleLogitsParams, f).offset for f, _ in _lib.SampleLogitsParams._fields_}
    fields = [f for f, _ in _lib.SampleLogitsParams._fields_]
    assert fields[0] == "struct_size" and fields[-3:] == ["row_index_ptr", "out_table_ptr", "table_steps"]   # the optional fields come last
    lib = _lib.load()
    assert lib.dimsum_abi_version() == 18                                      # a new symbol only: the ABI number stands
    header = open(os.path.join(_lib._HERE, "..", "include", "dimsum_hip.h")).read()
    assert "dimsum_sample_logits" in _lib.EXPORTS and hasattr(lib, "dimsum_sample_logits") and "int dimsum_sample_logits(" in header


def test_library_checks_in_their_documented_order():
    """every pointer set to host memory that is never dereferenced: the checks run on the host and return before a launch. The struct starts
    out wrong in every way, and each repair uncovers the next check in the documented order; the last call still fails, so nothing launches"""
    from dimsum_amd import _lib
    fn = _lib.load().dimsum_sample_logits
    NULL, DTYPE, SHAPE, STRIDE, ABI, ALIAS = 1, 2, 3, 4, 7, 8
    buf = (ctypes.c_float * 8192)()
    addr = ctypes.addressof(buf)
    assert fn(None, None) == NULL
    P = _lib.SampleLogitsParams()
    P.struct_size += 8
    assert fn(P, None) == ABI                                                  # before anything else is read
    P = _lib.SampleLogitsParams()
    P.rows, P.vocab, P.dtype, P.logits_row_stride, P.top_k, P.temperature = 0, 8, 3, 4, 5, 0.0
    # logits: 4 rows of 8 floats (128 bytes) from addr + 1024; out starts inside them
    for f, a in (("logits_ptr", addr + 1024), ("out_ptr", addr + 1024 + 64), ("u_ptr", addr)):
        assert fn(P, None) == NULL, f                                          # while a required pointer is missing
        setattr(P, f, a)
    P.out_table_ptr = addr + 1024 + 120
    assert fn(P, None) == NULL                                                 # out_table without row_index
    P.row_index_ptr = addr + 512
    P.top_k, P.u_ptr = 1, None                                                 # top_k == 1 draws nothing: u may be NULL
    for dt in (3, -1):
        P.dtype = dt
        assert fn(P, None) == DTYPE
    P.dtype = 0
    for r, v in ((0, 8), (-1, 8), (4, 0), (1 << 31, 8), (4, (1 << 31) - 16)):
        P.rows, P.vocab = r, v
        assert fn(P, None) == SHAPE, (r, v)
    P.rows, P.vocab = 4, 8
    for t in (0.0, -1.0, float("inf"), float("nan")):
        P.temperature = t
        assert fn(P, None) == SHAPE, t
    P.temperature = 0.7
    assert fn(P, None) == SHAPE                                                # row_index with table_steps 0
    P.table_steps = 5
    assert fn(P, None) == STRIDE                                               # logits_row_stride 4 < vocab 8
    P.logits_row_stride = 8
    for off in (64, 124, -28):                                                 # out: 4 int64 = 32 bytes
        P.out_ptr = addr + 1024 + off
        assert fn(P, None) == ALIAS, off
    P.out_ptr = addr + 1024 + 128                                              # the first byte after the logits
    assert fn(P, None) == ALIAS                                                # out_table (5 x 4 int64 = 160 bytes) still overlaps
    P.out_table_ptr = addr + 1024 - 156
    assert fn(P, None) == ALIAS
    P.out_table_ptr, P.dtype = addr + 1024 + 64, 1                             # 16-bit logits are 64 bytes: the table now starts after them ...
    P.out_ptr = addr + 1024 + 60
    assert fn(P, None) == ALIAS                                                # ... and out is the one that overlaps (a call that passed would launch)


# ---- decode / generate on the yardstick ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def sampling_backend(monkeypatch):
    """the lm_backend of test_lm_cpu.py plus native.sample_logits -> the yardstick; yields the list of the sampler's calls"""
    from dimsum_amd import native
    calls = []

    def counted(*a, **k):
        calls.append(k)
        return sample_logits_torch(*a, **k)

    monkeypatch.setattr(native, "causal_conv1d_update", native_conv_update)
    monkeypatch.setattr(native, "selective_state_update", native_state_update)
    monkeypatch.setattr(native, "decode_linear", decode_linear_torch)
    monkeypatch.setattr(native, "sample_logits", counted)
    monkeypatch.delenv("DIMSUM_FUSED_SAMPLING", raising=False)
    with cpu_oracle_backend():
        yield calls


def test_fused_greedy_reproduces_the_fixture(sampling_backend):
    g = golden("lm_tiny_rms1_fp32res1")
    m, prompt, L = tiny_model(1, 1, g), T(g["prompt"]), PROMPT + STEPS + 1
    out = m.generate(prompt, max_length=L, fused_sampling=True, top_k=1, return_dict_in_generate=True, output_scores=True)
    assert torch.equal(out.sequences[:, :PROMPT], prompt) and np.array_equal(out.sequences[:, PROMPT:].numpy(), g["ids"])
    assert len(sampling_backend) == STEPS + 1 and len(out.scores) == STEPS + 1  # one launch per token
    assert np.allclose(torch.stack(out.scores[1:], 1).numpy(), g["step_logits"], rtol=3e-4, atol=1e-3)
    # vocab_size limits the classes through a view: what reaches the sampler is 90 wide over rows of 96
    del sampling_backend[:]
    seen = []
    from dimsum_amd import native
    inner = native.sample_logits
    native.sample_logits = lambda logits, *a, **k: seen.append((tuple(logits.shape), logits.stride(0))) or inner(logits, *a, **k)
    try:
        ids = m.generate(prompt, max_length=PROMPT + 3, fused_sampling=True, vocab_size=90)
    finally:
        native.sample_logits = inner
    assert seen == [((2, 90), 96)] * 3 and torch.equal(ids, out.sequences[:, :PROMPT + 3])
    assert m.generate(prompt, max_length=PROMPT + 3, fused_sampling=True, return_dict_in_generate=True).scores is None


def test_a_pinned_table_gives_the_same_ids_and_the_table_decides(sampling_backend):
    g = golden("lm_tiny_rms1_fp32res1")
    m, prompt, L = tiny_model(1, 1, g), T(g["prompt"]), PROMPT + STEPS + 1
    table = torch.rand(L, 2, generator=torch.Generator().manual_seed(11))
    kw = dict(max_length=L, fused_sampling=True, top_k=5, top_p=0.9, temperature=0.8)
    a = m.generate(prompt, uniforms=table, return_dict_in_generate=True, output_scores=True, **kw)
    b = m.generate(prompt, uniforms=table.clone(), **kw)
    assert torch.equal(a.sequences, b)
    for i, s in enumerate(a.scores):                                           # step i draws with row i
        assert torch.equal(a.sequences[:, PROMPT + i], sample_logits_torch(s, table[i], 5, 0.9, 0.8))
    other = m.generate(prompt, uniforms=1.0 - table, **kw)
    assert not torch.equal(other, b)
    # without a table: one torch.rand draw per call from `generator`
    c = m.generate(prompt, generator=torch.Generator().manual_seed(4), **kw)
    d = m.generate(prompt, generator=torch.Generator().manual_seed(4), **kw)
    want = m.generate(prompt, uniforms=torch.rand(L, 2, generator=torch.Generator().manual_seed(4)), **kw)
    assert torch.equal(c, d) and torch.equal(c, want)
    with pytest.raises(ValueError, match="uniforms must be"):
        m.generate(prompt, uniforms=table[:-1], **kw)
    # eos: the run stops where every row's newest token is the one the pinned run emitted there
    col = a.sequences[:, PROMPT + 2]
    if bool((col == col[0]).all()):
        assert m.generate(prompt, uniforms=table, eos_token_id=int(col[0]), **kw).shape[1] <= PROMPT + 3
    one = m.generate(prompt[:1], uniforms=table[:, :1].contiguous(), eos_token_id=int(a.sequences[0, PROMPT + 2]), **kw)
    first = (a.sequences[0, PROMPT:] == a.sequences[0, PROMPT + 2]).nonzero()[0, 0].item()
    assert one.shape == (1, PROMPT + first + 1) and torch.equal(one[0], a.sequences[0, :PROMPT + first + 1])


def test_the_environment_is_read_per_call_and_the_default_is_sample(sampling_backend, monkeypatch):
    g = golden("lm_tiny_rms1_fp32res1")
    m, prompt, L = tiny_model(1, 1, g), T(g["prompt"]), PROMPT + 4
    want = m.generate(prompt, max_length=L)
    assert sampling_backend == []                                              # the defaults leave `sample` as the sampler
    m.generate(prompt, max_length=L, top_k=3, generator=torch.Generator().manual_seed(0))
    assert sampling_backend == []
    monkeypatch.setenv("DIMSUM_FUSED_SAMPLING", "1")
    assert torch.equal(m.generate(prompt, max_length=L), want) and len(sampling_backend) == 4
    monkeypatch.setenv("DIMSUM_FUSED_SAMPLING", "0")
    m.generate(prompt, max_length=L)
    assert len(sampling_backend) == 4
    m.generate(prompt, max_length=L, fused_sampling=True)                      # the argument beats the environment
    assert len(sampling_backend) == 8
    monkeypatch.setenv("DIMSUM_FUSED_SAMPLING", "1")
    m.generate(prompt, max_length=L, fused_sampling=False)
    teacher = want.clone()
    m.generate(prompt, max_length=L, teacher_outputs=teacher)                  # teacher_outputs keeps the unfused path
    assert len(sampling_backend) == 8
