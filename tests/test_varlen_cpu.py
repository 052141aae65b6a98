"""Packed variable-length rows (seq_idx) without a GPU: the float64 restatements `causal_conv1d_varlen_torch` / `selective_scan_varlen_torch`
against per-segment runs of the restatements that were here before them (this pins the semantics: a packed row gives, segment by segment,
what each segment gives as a row of its own; parameter gradients are the sums over the segments); the two helpers of dimsum_amd.utils against
hand-written rows; the four new symbols, their structs and their refusals in the documented order, nothing launched; Mamba / MambaLMHeadModel
with the restatements in the operators' place; seq_idx=None reaching native exactly as before; the refusals of what has no packed-row form."""
import ctypes

import pytest
import torch

from oracle.torch_backend import cpu_oracle_backend
from test_cross_entropy_cpu import ce_backend  # noqa: F401  (fixture)
from test_host_logic import _header_layout
from test_lm_cpu import tiny_model

STRUCTS = [("dimsum_conv_varlen_params_t", "ConvVarlenParams"), ("dimsum_conv_varlen_bwd_params_t", "ConvVarlenBwdParams"),
           ("dimsum_ssm_varlen_params_t", "SsmVarlenParams"), ("dimsum_ssm_varlen_bwd_params_t", "SsmVarlenBwdParams")]
SYMBOLS = (("dimsum_causal_conv1d_varlen_fwd", "ConvVarlenParams"), ("dimsum_causal_conv1d_varlen_bwd", "ConvVarlenBwdParams"),
           ("dimsum_ssm_scan_varlen_fwd", "SsmVarlenParams"), ("dimsum_ssm_scan_varlen_bwd", "SsmVarlenBwdParams"))
OK, NULL, DTYPE, SHAPE, STRIDE, UNSUPPORTED, ABI = 0, 1, 2, 3, 4, 5, 7
L = 37


def ids_from(lengths, values=None):
    """one row of ids from segment lengths; values: the id of each segment (default 0, 1, 2, ...)"""
    values = list(range(len(lengths))) if values is None else values
    return torch.tensor([v for n, v in zip(lengths, values) for _ in range(n)], dtype=torch.int32)


def segments(row):
    """[(start, stop)] of a row of ids"""
    cuts = [0] + [t for t in range(1, len(row)) if row[t] != row[t - 1]] + [len(row)]
    return list(zip(cuts[:-1], cuts[1:]))


# rows of length 37: boundaries at tile edges and inside tiles, at t = 1, runs of segments shorter than the conv, one segment, ids that come
# back ([7, 7, 2, 2, 7, 7]) and negative ids
ROWS = {
    "tile_edges": ids_from([4, 8, 12, 13]),
    "inside_tiles": ids_from([5, 6, 7, 19]),
    "at_one_and_short_runs": ids_from([1, 1, 2, 3, 1, 1, 2, 26]),
    "single": ids_from([37]),
    "not_monotone": ids_from([2, 2, 2, 31], [7, 2, 7, 2]),
    "negative": ids_from([3, 9, 25], [-5, -2147483648, 2147483647]),
}
BATCHES = [("tile_edges", "at_one_and_short_runs"), ("inside_tiles", "single"), ("not_monotone", "negative")]


def test_segments_helper():
    assert segments(ROWS["not_monotone"]) == [(0, 2), (2, 4), (4, 6), (6, 37)]
    assert segments(ROWS["single"]) == [(0, 37)]


# ---- the restatements against per-segment runs of the ones that were here before -------------------------------------------------------------------
@pytest.mark.parametrize("names", BATCHES, ids=["+".join(b) for b in BATCHES])
@pytest.mark.parametrize("width,bias,act", [(4, True, "silu"), (3, False, None), (2, True, None)])
def test_conv_restatement_is_the_per_segment_conv(names, width, bias, act):
    from dimsum_amd.ops import causal_conv1d_chunk_torch, causal_conv1d_varlen_torch
    g = torch.Generator().manual_seed(1)
    seq = torch.stack([ROWS[n] for n in names])
    x = torch.randn(2, 6, L, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(6, width, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(6, generator=g, dtype=torch.float64, requires_grad=True) if bias else None
    dy = torch.randn(2, 6, L, generator=g, dtype=torch.float64)
    y = causal_conv1d_varlen_torch(x, w, b, act, seq)
    got = torch.autograd.grad(y, [x, w] + ([b] if bias else []), dy)
    parts = []
    for r in range(2):
        for s, e in segments(seq[r]):
            parts.append((r, s, e, causal_conv1d_chunk_torch(x[r:r + 1, :, s:e], torch.zeros(1, 6, width, dtype=torch.float64), w, b, act)))
    want_y = torch.zeros_like(y)
    for r, s, e, p in parts:
        want_y[r, :, s:e] = p[0]
    want = torch.autograd.grad(want_y, [x, w] + ([b] if bias else []), dy)
    torch.testing.assert_close(y, want_y, rtol=1e-12, atol=1e-12)
    for a, c in zip(got, want):
        torch.testing.assert_close(a, c, rtol=1e-12, atol=1e-12)
    if names[1] == "single":                               # no seq_idx at all: the plain conv
        torch.testing.assert_close(causal_conv1d_varlen_torch(x[1:], w, b, act), y[1:], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("names", BATCHES, ids=["+".join(b) for b in BATCHES])
@pytest.mark.parametrize("N,groups,gate", [(16, 1, True), (5, 2, False)])
def test_scan_restatement_is_the_per_segment_scan(names, N, groups, gate):
    from dimsum_amd.ops import selective_scan_carry_torch, selective_scan_varlen_torch
    g = torch.Generator().manual_seed(2)
    seq = torch.stack([ROWS[n] for n in names])
    D_ = 6
    mk = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    u, delta, z = mk(2, D_, L).requires_grad_(), (0.5 * mk(2, D_, L)).requires_grad_(), mk(2, D_, L).requires_grad_()
    A = (-0.5 * torch.rand(D_, N, generator=g, dtype=torch.float64) - 0.1).requires_grad_()
    B, C = mk(2, groups, N, L).requires_grad_(), mk(2, groups, N, L).requires_grad_()
    Dv, db = mk(D_).requires_grad_(), (0.3 * mk(D_)).requires_grad_()
    leaves = [u, delta, A, B, C, Dv, db] + ([z] if gate else [])
    dy = mk(2, D_, L)
    y, last = selective_scan_varlen_torch(u, delta, A, B, C, Dv, z if gate else None, db, True, return_last_state=True, seq_idx=seq)
    got = torch.autograd.grad(y, leaves, dy)
    want_y, want_last = torch.zeros_like(y), torch.zeros_like(last)
    for r in range(2):
        for s, e in segments(seq[r]):
            o, h = selective_scan_carry_torch(u[r:r + 1, :, s:e], delta[r:r + 1, :, s:e], A, B[r:r + 1, ..., s:e], C[r:r + 1, ..., s:e], Dv,
                                              z[r:r + 1, :, s:e] if gate else None, db, True)
            want_y[r, :, s:e] = o[0]
            want_last[r] = h[0]                            # the last one written is the row's last segment
    want = torch.autograd.grad(want_y, leaves, dy)
    torch.testing.assert_close(y, want_y, rtol=1e-11, atol=1e-11)
    torch.testing.assert_close(last, want_last, rtol=1e-11, atol=1e-11)
    for a, c in zip(got, want):
        torch.testing.assert_close(a, c, rtol=1e-10, atol=1e-10)


# ---- the helpers -------------------------------------------------------------------------------------------------------------------------------------
def test_seq_idx_from_lengths_and_packed_labels():
    from dimsum_amd.utils import packed_labels, seq_idx_from_lengths
    assert seq_idx_from_lengths([2, 1, 3]).tolist() == [0, 0, 1, 2, 2, 2] and seq_idx_from_lengths([2, 1, 3]).dtype == torch.int32
    assert seq_idx_from_lengths([2, 1], seqlen=6).tolist() == [0, 0, 1, 2, 2, 2]              # the remainder is a segment of its own
    assert seq_idx_from_lengths([6, 3]).tolist() == [0] * 6 + [1] * 3                          # a prompt of 3 left-padded to 9
    assert seq_idx_from_lengths([], seqlen=3).tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        seq_idx_from_lengths([4, 4], seqlen=7)
    ids = torch.tensor([[10, 11, 12, 13, 14, 15], [20, 21, 22, 23, 24, 25]])
    seq = torch.stack([seq_idx_from_lengths([2, 1, 3]), torch.tensor([7, 7, 2, 2, 7, 7], dtype=torch.int32)])
    assert packed_labels(ids, seq).tolist() == [[11, -100, -100, 14, 15, -100], [21, -100, 23, -100, 25, -100]]
    assert packed_labels(ids, seq, ignore_index=-1)[0].tolist() == [11, -1, -1, 14, 15, -1]
    assert packed_labels(ids, seq).dtype == torch.int64


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------------------
def test_symbols_structs_and_abi_version():
    from dimsum_amd import _lib
    layout = _header_layout([(c, getattr(_lib, m)) for c, m in STRUCTS])
    for cname, mname in STRUCTS:
        mirror = getattr(_lib, mname)
        size, offsets = layout[cname]
        assert size == ctypes.sizeof(mirror), cname
        assert offsets == {n: getattr(mirror, n).offset for n, _ in mirror._fields_}, cname
    # the embedded structs are the existing ones, whole and untouched
    assert _lib.ConvVarlenParams.conv.size == ctypes.sizeof(_lib.ConvParams) == _header_layout([("dimsum_conv_params_t", _lib.ConvParams)])["dimsum_conv_params_t"][0]
    assert _lib.SsmVarlenParams.scan.size == ctypes.sizeof(_lib.SsmGeneralParams)
    assert _lib.SsmVarlenBwdParams.bwd.size == ctypes.sizeof(_lib.SsmGeneralBwdParams)
    lib = _lib.load()
    assert lib.dimsum_abi_version() == 18
    header = open(_lib.os.path.join(_lib._HERE, "..", "include", "dimsum_hip.h")).read()
    assert "#define DIMSUM_ABI_VERSION 18" in header
    for name, m in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(lib, name) and f"int {name}(" in header, name
        fn, p = getattr(lib, name), getattr(_lib, m)()
        assert fn(p, None) == NULL                                # a zeroed struct of the right size: the first NULL pointer, nothing launched
        p.struct_size -= 8
        assert fn(p, None) == ABI
        assert fn(None, None) == NULL


def _scan_params(addr, backward):
    """a varlen scan struct whose every check passes up to the one a test trips (host memory, never dereferenced: nothing is launched)"""
    from dimsum_amd import _lib
    V = _lib.SsmVarlenBwdParams() if backward else _lib.SsmVarlenParams()
    s = V.bwd.fwd if backward else V.scan
    for f in ("A_ptr", "B_ptr", "C_ptr", "u_ptr", "delta_ptr"):
        setattr(s, f, addr)
    s.batch, s.dim, s.seqlen, s.dstate, s.n_groups, s.n_chunks = 2, 8, 5, 16, 1, 1
    s.is_variable_B = s.is_variable_C = 1
    if backward:
        for f in ("dout_ptr", "dA_ptr", "dB_ptr", "dC_ptr", "du_ptr", "ddelta_ptr", "workspace_ptr"):
            setattr(V.bwd, f, addr)
        V.bwd.workspace_bytes = 1 << 30
    V.seq_idx_ptr, V.seq_idx_batch_stride = addr, 5
    return V, s


@pytest.mark.parametrize("backward", [False, True], ids=["fwd", "bwd"])
def test_scan_refusals_in_order(backward):
    """the general entry point's checks first, in their order; then seq_idx NULL, its stride, complex A / constant B or C. Every call
    fails a host-side check: no launch is reached (there is no GPU here)"""
    from dimsum_amd import _lib
    lib = _lib.load()
    fn = lib.dimsum_ssm_scan_varlen_bwd if backward else lib.dimsum_ssm_scan_varlen_fwd
    buf = (ctypes.c_float * 64)()
    addr = ctypes.addressof(buf)                                 # 16-byte aligned enough for the workspace check: ctypes arrays are
    addr += (-addr) % 16
    V, s = _scan_params(addr, backward)
    s.dstate = 257
    V.seq_idx_ptr = None
    assert fn(V, None) == SHAPE                                  # the shape is refused before the missing ids are
    V, s = _scan_params(addr, backward)
    s.dtype = 3
    s.is_complex = 1
    V.seq_idx_ptr = None
    assert fn(V, None) == DTYPE
    V, s = _scan_params(addr, backward)
    s.u_d_stride = -1
    V.seq_idx_ptr = None
    assert fn(V, None) == STRIDE
    V, s = _scan_params(addr, backward)
    V.seq_idx_ptr = None
    s.is_complex = 1
    assert fn(V, None) == NULL                                   # seq_idx NULL comes before everything else that is new
    V, s = _scan_params(addr, backward)
    V.seq_idx_batch_stride = 4                                   # rows of 5 ids would overlap
    s.is_complex = 1
    assert fn(V, None) == STRIDE
    V.seq_idx_batch_stride = -5
    assert fn(V, None) == STRIDE
    for field, value in (("is_complex", 1), ("is_variable_B", 0), ("is_variable_C", 0)):
        V, s = _scan_params(addr, backward)
        setattr(s, field, value)
        assert fn(V, None) == UNSUPPORTED, field


@pytest.mark.parametrize("backward", [False, True], ids=["fwd", "bwd"])
def test_conv_refusals_in_order(backward):
    from dimsum_amd import _lib
    lib = _lib.load()
    fn = lib.dimsum_causal_conv1d_varlen_bwd if backward else lib.dimsum_causal_conv1d_varlen_fwd
    buf = (ctypes.c_float * 64)()
    addr = ctypes.addressof(buf)

    def params():
        V = _lib.ConvVarlenBwdParams() if backward else _lib.ConvVarlenParams()
        c = V.conv.fwd if backward else V.conv
        c.batch, c.dim, c.seqlen, c.width = 2, 8, 5, 4
        c.x_ptr = c.weight_ptr = addr
        if backward:
            V.conv.dout_ptr = V.conv.dx_ptr = V.conv.dweight_ptr = addr
        else:
            c.out_ptr = addr
        V.seq_idx_ptr, V.seq_idx_batch_stride = addr, 5
        return V, c

    V, c = params()
    c.width = 5
    V.seq_idx_ptr = None
    assert fn(V, None) == SHAPE
    V, c = params()
    c.dtype = 3
    V.seq_idx_ptr = None
    assert fn(V, None) == DTYPE
    V, c = params()
    V.seq_idx_ptr = None
    V.seq_idx_batch_stride = 1
    assert fn(V, None) == NULL
    V, c = params()
    V.seq_idx_batch_stride = 4
    assert fn(V, None) == STRIDE
    V, c = params()
    c.batch = 0
    assert fn(V, None) == OK                                     # nothing to do, nothing launched


def test_operator_refusals_carry_their_reason():
    from dimsum_amd.ops import bimamba_inner_fn, mamba_inner_fn, mamba_inner_fn_cond, mamba_inner_fn_no_out_proj_cond, selective_scan_fn
    u = torch.randn(1, 4, 6)
    seq = torch.zeros(1, 6, dtype=torch.int32)
    A, Bv = -torch.rand(4, 3), torch.randn(1, 3, 6)
    with pytest.raises(NotImplementedError, match="complex A"):
        selective_scan_fn(u, u, torch.complex(A, A), torch.randn(1, 3, 12), torch.randn(1, 3, 12), seq_idx=seq)
    with pytest.raises(NotImplementedError, match="constant"):
        selective_scan_fn(u, u, A, torch.randn(4, 3), Bv, seq_idx=seq)
    with pytest.raises(NotImplementedError, match="initial_state"):
        selective_scan_fn(u, u, A, Bv, Bv, seq_idx=seq, initial_state=torch.zeros(1, 4, 3))
    xz, cw, xp, dp, op = torch.randn(1, 8, 6), torch.randn(4, 1, 4), torch.randn(1 + 6, 4), torch.randn(4, 1), torch.randn(2, 4)
    with pytest.raises(NotImplementedError, match="conv_done"):
        mamba_inner_fn_cond(xz, cw, None, xp, dp, op, None, A, seq_idx=seq, conv_done=True)
    with pytest.raises(NotImplementedError, match="init_states"):
        mamba_inner_fn_cond(xz, cw, None, xp, dp, op, None, A, seq_idx=seq, init_states=torch.zeros(1, 4))
    with pytest.raises(NotImplementedError, match="conditional"):
        mamba_inner_fn_no_out_proj_cond(xz, cw, None, xp, dp, A, seq_idx=seq)
    with pytest.raises(TypeError, match="seq_idx"):               # its signature is the reference's, pinned by test_bimamba_cpu.py: no such argument
        bimamba_inner_fn(xz, cw, None, xp, dp, op, None, A, A, seq_idx=seq)
    with pytest.raises(NotImplementedError, match="complex A"):
        mamba_inner_fn(xz, cw, None, xp, dp, op, None, torch.complex(A, A), seq_idx=seq)
    # native: the ids' own checks need no GPU
    from dimsum_amd import native
    u2 = torch.randn(2, 4, 6)
    for bad in (torch.zeros(2, 6, dtype=torch.int64), torch.zeros(2, 5, dtype=torch.int32), torch.zeros(6, 2, dtype=torch.int32).t()):
        with pytest.raises(RuntimeError, match="seq_idx must be a contiguous int32"):
            native.causal_conv1d_varlen_fwd(u2, torch.randn(4, 4), None, True, bad)


# ---- the modules with the restatements in the operators' place -------------------------------------------------------------------------------------
@pytest.fixture
def varlen_backend(monkeypatch, ce_backend):  # noqa: F811
    """the two packed-row operators replaced by their torch restatements (same signatures), everything else on the CPU oracle backend"""
    from dimsum_amd.ops import causal_conv1d_varlen_torch, selective_scan_interface, selective_scan_varlen_torch
    monkeypatch.setattr(selective_scan_interface, "causal_conv1d_fn", causal_conv1d_varlen_torch)
    monkeypatch.setattr(selective_scan_interface, "selective_scan_fn", selective_scan_varlen_torch)
    with cpu_oracle_backend():
        yield


DOCS = [[5, 1, 11], [9, 8]]                                    # two packed rows of 17 tokens


def _packed_batch(vocab=90, seed=3):
    from dimsum_amd.utils import seq_idx_from_lengths
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, vocab, (len(DOCS), sum(DOCS[0])), generator=g)
    return ids, torch.stack([seq_idx_from_lengths(d) for d in DOCS])


def test_mixer_packed_forward_is_the_per_document_forward(varlen_backend):
    from dimsum_amd.modules.mamba_simple import Mamba
    from dimsum_amd.utils import InferenceParams
    torch.manual_seed(0)
    m = Mamba(32, d_state=5, d_conv=4, expand=2, layer_idx=0).eval()
    ids, seq = _packed_batch()
    x = torch.randn(2, 17, 32)
    p = InferenceParams(max_seqlen=32, max_batch_size=2)
    with torch.no_grad():
        y = m(x, seq_idx=seq)
        y_cached = m(x, inference_params=p, seq_idx=seq)
        torch.testing.assert_close(y_cached, y)
        conv_state, ssm_state = p.key_value_memory_dict[0]
        for r, docs in enumerate(DOCS):
            s = 0
            for n in docs:
                q = InferenceParams(max_seqlen=32, max_batch_size=1)
                alone = m(x[r:r + 1, s:s + n], inference_params=q)
                torch.testing.assert_close(y[r:r + 1, s:s + n], alone, rtol=1e-4, atol=1e-5)
                s += n
            # the cache holds the row's last document, as if it had been prefilled alone (short ones zero-padded on the left)
            torch.testing.assert_close(conv_state[r:r + 1], q.key_value_memory_dict[0][0], rtol=1e-5, atol=1e-6)
            torch.testing.assert_close(ssm_state[r:r + 1], q.key_value_memory_dict[0][1], rtol=1e-4, atol=1e-5)
        p.seqlen_offset = 17
        with pytest.raises(ValueError, match="seqlen_offset > 0"):
            m(x[:, :1], inference_params=p, seq_idx=seq[:, :1])


def test_lm_packed_logits_loss_and_gradients_are_the_per_document_ones(varlen_backend):
    from dimsum_amd.utils import packed_labels
    torch.manual_seed(0)
    m = tiny_model(1, 1).train()
    ids, seq = _packed_batch()
    logits = m(ids, seq_idx=seq).logits
    loss = m.loss(ids, packed_labels(ids, seq), seq_idx=seq)
    grads = torch.autograd.grad(loss, list(m.parameters()))
    total, count, want_grads = 0.0, 0, [torch.zeros_like(p) for p in m.parameters()]
    for r, docs in enumerate(DOCS):
        s = 0
        for n in docs:
            doc = ids[r:r + 1, s:s + n]
            torch.testing.assert_close(logits[r:r + 1, s:s + n], m(doc).logits, rtol=3e-4, atol=1e-3)
            if n > 1:
                part = m.loss(doc, reduction="sum")
                for acc, gr in zip(want_grads, torch.autograd.grad(part, list(m.parameters()), allow_unused=True)):
                    if gr is not None:
                        acc += gr
                total, count = total + part.item(), count + n - 1
            s += n
    assert count == sum(n - 1 for d in DOCS for n in d)
    assert abs(loss.item() - total / count) < 1e-5 * abs(total / count) + 1e-6         # the token-weighted mean of the per-document losses
    for (name, _), a, c in zip(m.named_parameters(), grads, want_grads):
        torch.testing.assert_close(a, c / count, rtol=2e-3, atol=2e-5, msg=lambda s, n=name: f"{n}: {s}")


# ---- seq_idx=None is the call it always was ------------------------------------------------------------------------------------------------------
def test_no_seq_idx_calls_native_as_before(monkeypatch):
    """one mixer forward + backward without seq_idx under a spy on native: the conv and scan entry points of the parent, with the parent's
    argument counts and keywords -- and none of the packed-row ones"""
    from dimsum_amd import native
    from dimsum_amd.modules.mamba_simple import Mamba
    calls = []
    with cpu_oracle_backend(), monkeypatch.context() as spy:      # the spies come off before the backend does: neither outlives this test
        for name in ("causal_conv1d_fwd", "causal_conv1d_bwd", "selective_scan_fwd", "selective_scan_bwd", "causal_conv1d_varlen_fwd",
                     "causal_conv1d_varlen_bwd", "selective_scan_varlen_fwd", "selective_scan_varlen_bwd", "selective_scan_general_fwd",
                     "selective_scan_general_bwd"):
            real = getattr(native, name)
            spy.setattr(native, name, lambda *a, _n=name, _r=real, **k: calls.append((_n, len(a), tuple(sorted(k)))) or _r(*a, **k))
        torch.manual_seed(0)
        m = Mamba(32, d_state=16, d_conv=4, expand=2, layer_idx=0)
        x = torch.randn(2, 12, 32, requires_grad=True)
        m(x).sum().backward()
        m(x, seq_idx=None).sum().backward()
    want = [("causal_conv1d_fwd", 4, ()), ("selective_scan_fwd", 9, ("need_ckpt", "need_out", "need_x")),
            ("selective_scan_bwd", 14, ("ckpt",)), ("causal_conv1d_bwd", 6, ())]       # (the row-major x_dbl of a CPU call: no dB / dC buffers)
    assert calls == want + want, calls


def test_modules_that_have_no_packed_form_say_so():
    from dimsum_amd.modules.mamba_simple import CondMamba, Mamba
    seq = torch.zeros(1, 6, dtype=torch.int32)
    x = torch.randn(1, 6, 16)
    with pytest.raises(NotImplementedError, match='scan_type "v2"'):
        Mamba(16, scan_type="v2")(x, seq_idx=seq)
    with pytest.raises(NotImplementedError, match="x3"):
        Mamba(16)(None, x3=x, seq_idx=seq)
    with pytest.raises(ValueError, match="int32"):
        Mamba(16)(x, seq_idx=seq.long())
    with pytest.raises(TypeError):
        CondMamba(16, d_cond=8)(x, torch.randn(1, 8), seq_idx=seq)         # the conditional mixer takes no seq_idx at all
