"""CPU tests of resumed packed prefill: the start_slots / initial_states contract on the float64 restatements,
plan_packed_prefill(resume=), the refusals with their reasons, DecodeEngine(chunked_prefill=True) on the torch stand-ins, and the two C entry
points' host checks in their documented order (host memory that is never dereferenced: every call fails a check before any launch)."""
import ctypes
import math

import pytest
import torch

from test_host_logic import _header_layout
from test_lm_cpu import tiny_model
from test_packed_prefill_cpu import packed_backend  # noqa: F401  (a fixture)
from test_slots_cpu import _alone

OK, NULL, DTYPE, SHAPE, STRIDE, UNSUPPORTED, ABI = 0, 1, 2, 3, 4, 5, 7
F64 = torch.float64
PIECES, TOTAL, SLOT, POOL = [1, 2, 3, 5, 29], 40, 2, 4


def _piece_row(n, first, other=4, pad=3):
    """one packed row: an unrelated segment of `other` tokens (slot 0, from zeros), the piece (slot SLOT, resumed unless it is the first),
    padding -> seq_idx, end_slots, start_slots, where the piece begins"""
    from dimsum_amd.utils import seq_idx_from_lengths
    L = other + n + pad
    seq = seq_idx_from_lengths([other, n], L).view(1, L)
    ends, starts = torch.full((1, L), -1, dtype=torch.int32), torch.full((1, L), -1, dtype=torch.int32)
    ends[0, other - 1], ends[0, other + n - 1] = 0, SLOT
    if not first:
        starts[0, other] = SLOT
    return seq, ends, starts, other


# ---- the contract on float64 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [2, 3, 4])
def test_conv_restatement_in_pieces_is_the_unsplit_conv(width):
    from dimsum_amd.ops import causal_conv1d_varlen_torch
    g = torch.Generator().manual_seed(width)
    D = 5
    x, w, b = torch.randn(1, D, TOTAL, generator=g, dtype=F64), torch.randn(D, width, generator=g, dtype=F64), torch.randn(D, generator=g, dtype=F64)
    whole = causal_conv1d_varlen_torch(x, w, b, "silu")
    pool = torch.full((POOL, D, width), 7.0, dtype=F64)
    t, outs = 0, []
    for i, n in enumerate(PIECES):
        seq, ends, starts, at = _piece_row(n, i == 0)
        row = torch.randn(1, D, seq.shape[1], generator=g, dtype=F64)
        row[:, :, at:at + n] = x[:, :, t:t + n]
        out = causal_conv1d_varlen_torch(row, w, b, "silu", seq, end_slots=ends, conv_state=pool, start_slots=starts, initial_states=pool.clone())
        outs.append(out[:, :, at:at + n])
        # the neighbour and the padding are what they are without the new arguments
        plain = causal_conv1d_varlen_torch(row, w, b, "silu", seq)
        assert torch.equal(out[:, :, :at], plain[:, :, :at]) and torch.equal(out[:, :, at + n:], plain[:, :, at + n:])
        t += n
        want = torch.nn.functional.pad(x[0, :, :t], (max(width - t, 0), 0))[:, -width:]           # values only move: exact
        assert torch.equal(pool[SLOT], want), n
    assert float((torch.cat(outs, -1) - whole).abs().max()) <= 8 * torch.finfo(F64).eps * float(whole.abs().max())
    assert bool((pool[[1, 3]] == 7.0).all())


@pytest.mark.parametrize("N", [16, 17])
def test_scan_restatement_in_pieces_is_the_unsplit_scan(N):
    from dimsum_amd.ops import selective_scan_varlen_torch
    g = torch.Generator().manual_seed(N)
    D = 4
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    u, dt, A, B, C = r(1, D, TOTAL), 0.5 * torch.rand(1, D, TOTAL, generator=g, dtype=F64), -torch.rand(D, N, generator=g, dtype=F64), r(1, N, TOTAL), r(1, N, TOTAL)
    Dv, z, bias = r(D), r(1, D, TOTAL), r(D)
    whole, last = selective_scan_varlen_torch(u, dt, A, B, C, Dv, z, bias, True, True)
    pool = torch.full((POOL, D, N), 7.0, dtype=F64)
    t, outs = 0, []
    for i, n in enumerate(PIECES):
        seq, ends, starts, at = _piece_row(n, i == 0)
        L = seq.shape[1]

        def put(full, shape):
            row = r(*shape, L) if full is not dt else 0.5 * torch.rand(*shape, L, generator=g, dtype=F64)
            row[..., at:at + n] = full[..., t:t + n]
            return row
        out = selective_scan_varlen_torch(put(u, (1, D)), put(dt, (1, D)), A, put(B, (1, N)), put(C, (1, N)), Dv, put(z, (1, D)), bias, True, seq_idx=seq,
                                          end_slots=ends, ssm_state=pool, start_slots=starts, initial_states=pool)      # in place: the pool itself
        outs.append(out[:, :, at:at + n])
        t += n
    # the same float64 recurrence step by step; only torch's vectorised exp on tensors of another length may differ, by an ulp per step
    tol = 64 * torch.finfo(F64).eps
    assert float((torch.cat(outs, -1) - whole).abs().max()) <= tol * float(whole.abs().max())
    assert float((pool[SLOT] - last[0]).abs().max()) <= tol * float(last.abs().max())
    assert bool((pool[[1, 3]] == 7.0).all())


# ---- plan_packed_prefill(resume=) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 2])
def test_plan_resume(rows):
    from dimsum_amd.utils import plan_packed_prefill
    lengths, slots, resume = [5, 3, 7, 1, 4], [2, 0, 4, 1, 3], [False, True, True, False, True]
    old = plan_packed_prefill(lengths, slots, rows=rows)
    assert sorted(old) == ["end_slots", "logits_positions", "segments", "seq_idx", "seqlen"]
    same = plan_packed_prefill(lengths, slots, rows=rows, resume=None)
    assert sorted(same) == sorted(old) and all(torch.equal(old[k], same[k]) if torch.is_tensor(old[k]) else old[k] == same[k] for k in old)
    plan = plan_packed_prefill(lengths, slots, rows=rows, resume=resume)
    assert all(torch.equal(old[k], plan[k]) if torch.is_tensor(old[k]) else old[k] == plan[k] for k in old)
    ss, sr, sl = plan["start_slots"], plan["start_rows"], plan["start_list"]
    assert ss.shape == sr.shape == old["seq_idx"].shape and ss.dtype == sr.dtype == torch.int32 and sl.dtype == torch.int64
    assert sl.tolist() == [0, 4, 3] and int((ss >= 0).sum()) == int((sr >= 0).sum()) == 3
    k = 0
    for (r, start), s, f in zip(plan["segments"], slots, resume):
        if f:
            assert int(ss[r, start]) == s and int(sr[r, start]) == k and (start == 0 or int(plan["seq_idx"][r, start]) != int(plan["seq_idx"][r, start - 1]))
            k += 1
        else:
            assert int(ss[r, start]) == int(sr[r, start]) == -1
    none = plan_packed_prefill(lengths, slots, rows=rows, resume=[False] * 5)
    assert none["start_list"].numel() == 0 and bool((none["start_slots"] == -1).all())
    with pytest.raises(ValueError, match="one resume flag per segment"):
        plan_packed_prefill(lengths, slots, resume=[True])
    with pytest.raises(ValueError, match="plan_packed_prefill"):
        plan_packed_prefill([1, 2], [3, 3], resume=[True, False])


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_operator_refusals_carry_their_reason():
    from dimsum_amd import native
    from dimsum_amd.ops import causal_conv1d_fn, mamba_inner_fn_cond, selective_scan_fn
    x, w = torch.randn(2, 4, 6), torch.randn(4, 4)
    seq, ends = torch.zeros(2, 6, dtype=torch.int32), torch.full((2, 6), -1, dtype=torch.int32)
    starts = ends.clone()
    pool, init = torch.zeros(3, 4, 4), torch.zeros(2, 4, 4)
    with pytest.raises(ValueError, match="start_slots without seq_idx"):
        causal_conv1d_fn(x, w, start_slots=starts, initial_states=init)
    with pytest.raises(ValueError, match="start_slots and initial_states go together"):
        causal_conv1d_fn(x, w, seq_idx=seq, start_slots=starts)
    with pytest.raises(ValueError, match="end_slots and conv_state go together"):
        causal_conv1d_fn(x, w, seq_idx=seq, start_slots=starts, initial_states=init, end_slots=ends)
    with pytest.raises(NotImplementedError, match="inference arguments"):
        causal_conv1d_fn(x.requires_grad_(), w, seq_idx=seq, start_slots=starts, initial_states=init)
    x = x.detach()
    # the conv's carried inputs may not overlap the pool it stores into -- unless nothing is stored
    for bad in (pool, pool[1:], pool.view(-1)[3:3 + 32].view(2, 4, 4)):
        with pytest.raises(ValueError, match="initial_states overlaps conv_state"):
            causal_conv1d_fn(x, w, seq_idx=seq, end_slots=ends, conv_state=pool, start_slots=starts, initial_states=bad)
    big = torch.zeros(6, 4, 4)
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):                              # disjoint halves of one allocation pass the check
        causal_conv1d_fn(x, w, seq_idx=seq, end_slots=ends, conv_state=big[:3], start_slots=starts, initial_states=big[3:])
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):                              # no end_slots: overlap is nobody's problem
        causal_conv1d_fn(x, w, seq_idx=seq, start_slots=starts, initial_states=pool)
    A, Bm, st = -torch.rand(4, 3), torch.randn(2, 3, 6), torch.zeros(3, 4, 3)
    with pytest.raises(ValueError, match="start_slots without seq_idx"):
        selective_scan_fn(x, x, A, Bm, Bm, start_slots=starts, initial_states=st)
    with pytest.raises(ValueError, match="start_slots and initial_states go together"):
        selective_scan_fn(x, x, A, Bm, Bm, seq_idx=seq, initial_states=st)
    with pytest.raises(NotImplementedError, match="inference arguments"):
        selective_scan_fn(x, x, A.requires_grad_(), Bm, Bm, seq_idx=seq, start_slots=starts, initial_states=st)
    A = A.detach()
    with pytest.raises(NotImplementedError, match="carried initial_state"):
        selective_scan_fn(x, x, A, Bm, Bm, seq_idx=seq, start_slots=starts, initial_states=st, initial_state=torch.zeros(2, 4, 3))
    with pytest.raises(NotImplementedError, match="constant"):
        selective_scan_fn(x, x, A, torch.randn(4, 3), Bm, seq_idx=seq, start_slots=starts, initial_states=st)
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):                              # the scan may alias its pool
        selective_scan_fn(x, x, A, Bm, Bm, seq_idx=seq, end_slots=ends, ssm_state=st, start_slots=starts, initial_states=st)
    # the five refusals of the parent stay
    with pytest.raises(NotImplementedError, match="end_slots together with a carried initial_state is not built"):
        selective_scan_fn(x, x, A, Bm, Bm, seq_idx=seq, end_slots=ends, ssm_state=st, initial_state=torch.zeros(2, 4, 3))
    with pytest.raises(NotImplementedError, match="seq_idx together with a carried initial_state is not built"):
        selective_scan_fn(x, x, A, Bm, Bm, seq_idx=seq, initial_state=torch.zeros(2, 4, 3))
    xz, cw, xp, dp, op = torch.randn(2, 8, 6), torch.randn(4, 1, 4), torch.randn(1 + 6, 4), torch.randn(4, 1), torch.randn(2, 4)
    with pytest.raises(ValueError, match="start_slots, start_rows and conv_initial_states go together"):
        mamba_inner_fn_cond(xz, cw, None, xp, dp, op, None, A, seq_idx=seq, end_slots=ends, conv_state=pool, ssm_state=st, start_slots=starts)
    with pytest.raises(ValueError, match="start_slots without end_slots"):
        mamba_inner_fn_cond(xz, cw, None, xp, dp, op, None, A, seq_idx=seq, start_slots=starts, start_rows=starts, conv_initial_states=init)
    # native: dtype, rank, shape and contiguity of start_slots need no GPU, initial_states' shape and dtype are named, the device comes last
    B4 = Bm.unsqueeze(1)
    for bad in (starts.long(), starts[:, :5].contiguous(), torch.full((6, 2), -1, dtype=torch.int32).t(), starts[0]):
        with pytest.raises(RuntimeError, match="start_slots must be a contiguous int32"):
            native.causal_conv1d_varlen_resume_fwd(x, w, None, True, seq, ends, pool, bad, init)
        with pytest.raises(RuntimeError, match="start_slots must be a contiguous int32"):
            native.selective_scan_varlen_resume_fwd(x, x, A, B4, B4, None, None, None, True, seq, ends, st, bad, st)
    with pytest.raises(RuntimeError, match=r"initial_states must be \(n_init >= 1, dim, width\)"):
        native.causal_conv1d_varlen_resume_fwd(x, w, None, True, seq, ends, pool, starts, init[:, :, :3])
    with pytest.raises(RuntimeError, match="initial_states must have x's dtype"):
        native.causal_conv1d_varlen_resume_fwd(x, w, None, True, seq, ends, pool, starts, init.half())
    with pytest.raises(RuntimeError, match=r"initial_states must be \(n_init >= 1, dim, dstate\)"):
        native.selective_scan_varlen_resume_fwd(x, x, A, B4, B4, None, None, None, True, seq, ends, st, starts, st[:, :, :2])
    with pytest.raises(RuntimeError, match="initial_states must be float32 or of u's dtype"):
        native.selective_scan_varlen_resume_fwd(x, x, A, B4, B4, None, None, None, True, seq, ends, st, starts, st.double())
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        native.causal_conv1d_varlen_resume_fwd(x, w, None, True, seq, ends, pool, starts, init)


def test_module_refusals_carry_their_reason(packed_backend):  # noqa: F811
    from dimsum_amd.modules.mamba_simple import Mamba
    from dimsum_amd.utils import InferenceParams, plan_packed_prefill
    m = tiny_model(1, 1)
    plan = plan_packed_prefill([3, 2], [1, 0], resume=[True, False])
    starts = {k: plan[k] for k in ("start_slots", "start_rows", "start_list")}
    ids = torch.randint(0, 90, (1, 5))
    new = lambda **kw: InferenceParams(**{**dict(max_seqlen=8, max_batch_size=1, key_value_memory_dict=m.allocate_inference_cache(3, 8),
                                                 prefill_slots=plan["end_slots"], prefill_starts=starts), **kw})
    assert InferenceParams(max_seqlen=8, max_batch_size=1).prefill_starts is None
    p = new()
    p.reset(9, 1)
    assert p.prefill_starts is starts
    mixer = m.backbone.layers[0].mixer
    with torch.no_grad():
        m(ids, inference_params=new(), seq_idx=plan["seq_idx"], logits_positions=plan["logits_positions"])       # the accepted form
        with pytest.raises(ValueError, match="prefill_starts without prefill_slots"):
            m(ids, inference_params=new(prefill_slots=None), seq_idx=plan["seq_idx"])
        with pytest.raises(ValueError, match="prefill_slots without seq_idx"):
            m(ids, inference_params=new())
        with pytest.raises(ValueError, match="prefill_slots at seqlen_offset > 0"):
            mixer(torch.zeros(1, 5, 64), inference_params=new(seqlen_offset=5), seq_idx=plan["seq_idx"])
        for bad in (dict(starts, start_slots=plan["start_slots"][:, :4]), dict(starts, start_rows=plan["start_rows"].long()),
                    dict(starts, start_list=plan["start_list"].int()), dict(starts, start_list=plan["start_list"][:0]), {"start_slots": plan["start_slots"]}):
            with pytest.raises(ValueError, match="prefill_starts must hold"):
                m(ids, inference_params=new(prefill_starts=bad), seq_idx=plan["seq_idx"])
        pools = lambda mod: {0: mod.allocate_inference_cache(3, 8)}
        kw = dict(d_state=4, d_conv=4, expand=2, layer_idx=0)
        for scan_type, reason in (("v2", 'scan_type "v2"'), ("zigma8", "zigma8")):
            mod = Mamba(16, scan_type=scan_type, num_patches=4, **kw).eval() if scan_type != "v2" else Mamba(16, scan_type="v2", **kw).eval()
            with pytest.raises(NotImplementedError, match=reason):
                mod(torch.zeros(1, 5, 16), inference_params=InferenceParams(8, 1, key_value_memory_dict=pools(mod), prefill_slots=plan["end_slots"],
                                                                            prefill_starts=starts), seq_idx=plan["seq_idx"])
        plain = Mamba(16, **kw).eval()
        with pytest.raises(NotImplementedError, match=r"operand-image input \(x3\)"):
            plain(None, inference_params=InferenceParams(8, 1, key_value_memory_dict=pools(plain), prefill_slots=plan["end_slots"], prefill_starts=starts),
                  x3=torch.zeros(1, 5, 16), seq_idx=plan["seq_idx"])
        with pytest.raises(NotImplementedError, match=r"conditional conv entry \(cond\)"):
            plain._mix(torch.zeros(1, 5, 16), torch.zeros(1, 32), states=pools(plain)[0], seq_idx=plan["seq_idx"], prefill_slots=plan["end_slots"],
                       prefill_starts=starts)
    with pytest.raises(NotImplementedError, match="inference argument"):                          # grad mode
        plain(torch.zeros(1, 5, 16), inference_params=InferenceParams(8, 1, key_value_memory_dict=pools(plain), prefill_slots=plan["end_slots"],
                                                                      prefill_starts=starts), seq_idx=plan["seq_idx"])


# ---- the engine ------------------------------------------------------------------------------------------------------------------------------------------
PROMPTS, BUDGET = [3, 8, 9, 21, 40], 8


@pytest.mark.parametrize("prefill_rows", [1, 2])
def test_engine_chunked_prefill_equals_unchunked(prefill_rows, packed_backend, monkeypatch):  # noqa: F811
    from dimsum_amd.utils.serving import DecodeEngine
    monkeypatch.setenv("DIMSUM_FUSED_DECODE", "1")
    m = tiny_model(1, 1)
    g = torch.Generator().manual_seed(11)
    prompts = [torch.randint(0, 90, (n,), generator=g) for n in PROMPTS]
    kw = dict(max_batch=3, num_slots=4, max_seqlen=64, vocab_size=90, cg=False, fused_sampling=False, packed_prefill=True, prefill_rows=prefill_rows,
              max_prefill_tokens=BUDGET)
    for bad in (dict(kw, packed_prefill=False), dict(kw, max_prefill_tokens=None)):
        with pytest.raises(ValueError, match="chunked_prefill"):
            DecodeEngine(m, chunked_prefill=True, **bad)
    ref = DecodeEngine(m, **kw)
    assert ref.chunked_prefill is False                                                           # off by default
    eng = DecodeEngine(m, chunked_prefill=True, **kw)
    rids = [eng.submit(p, 4) for p in prompts]
    for p in prompts:
        ref.submit(p, 4)
    want = ref.run()
    seen, step = {}, 0
    while not eng.idle():
        events = eng.step()
        for rid, _, _ in events:
            r = eng.requests[rid]
            assert r.done == r.prompt.numel(), rid                                                # never before its last piece
            seen.setdefault(rid, step)
        # a prefilling request holds a row and a slot, but the decode step's slot buffer does not name it
        for r in eng._prefilling:
            assert eng.rows[r.row] == r.rid and eng.slots[r.row].item() == -1 and r.slot not in eng.free_slots and not r.tokens
        step += 1
        assert step < 200
    for rid in rids:
        assert torch.equal(eng.sequence(rid), want[rid]), rid
        assert torch.equal(eng.sequence(rid), _alone(m, prompts[rid], 4)[0]), rid
    assert max(eng.prefill_pass_tokens) <= BUDGET and sum(eng.prefill_pass_tokens) == sum(PROMPTS)
    assert eng.n_prefill_passes == len(eng.prefill_pass_tokens)
    # every prompt is cut where the budget of its pass ends: at least ceil(n / budget) pieces each, one more per pass boundary inside it
    assert eng.n_prefill_pieces >= sum(math.ceil(n / BUDGET) for n in PROMPTS)
    # worked out by hand for three rows, four new tokens each (a request holds its row for three steps from its last piece on):
    #   step 1: 3 + the first 5 of 8 | 2: 3 of 8 + 5 of 9 | 3: 4 of 9, no row free | 4: 8 of 21 | 5: 8 of 21 | 6: 5 of 21 + 3 of 40 |
    #   7 - 11: 8, 8, 8, 8, 5 of 40
    assert eng.prefill_pass_tokens == [8, 8, 4, 8, 8, 8, 8, 8, 8, 8, 5] and eng.n_prefill_pieces == 14
    assert eng.n_prefill_pieces == _pieces_by_budget(PROMPTS, BUDGET, eng)
    assert seen[4] >= math.ceil(40 / BUDGET) - 1                                                  # the 40-token prompt took its passes
    assert len({slot for _, slot in eng.slot_history}) < len(PROMPTS)                             # a released slot is reused


def _pieces_by_budget(prompts, budget, eng):
    """the piece count the budget implies for this engine's row / slot supply, replayed on the host from its admission order: every pass
    takes the prefilling requests first and then new ones, each cut at what is left of the budget"""
    return sum(1 for _ in _replay(prompts, budget, eng))


def _replay(prompts, budget, eng):
    left = {rid: n for rid, n in enumerate(prompts)}
    for tokens in eng.prefill_pass_tokens:
        rest = tokens
        for rid in sorted(left):
            if rest == 0:
                break
            n = min(rest, left[rid])
            left[rid] -= n
            rest -= n
            if left[rid] == 0:
                del left[rid]
            yield rid, n
        assert rest == 0
    assert not left


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------------------------
STRUCTS = [("dimsum_conv_varlen_resume_params_t", "ConvVarlenResumeParams", "ConvVarlenStatesParams", "dimsum_conv_varlen_states_params_t",
            ["init_slot_stride", "init_c_stride", "init_w_stride", "init_dtype", "reserved"]),
           ("dimsum_ssm_varlen_resume_params_t", "SsmVarlenResumeParams", "SsmVarlenStatesParams", "dimsum_ssm_varlen_states_params_t",
            ["init_slot_stride", "init_d_stride", "init_dstate_stride", "init_f32", "reserved"])]
SYMBOLS = ("dimsum_causal_conv1d_varlen_resume_fwd", "dimsum_ssm_scan_varlen_resume_fwd")


def test_structs_symbols_and_abi_version():
    from dimsum_amd import _lib
    layout = _header_layout([(c, getattr(_lib, m)) for c, m, _, _, _ in STRUCTS] + [(c, getattr(_lib, m)) for _, _, m, c, _ in STRUCTS])
    for cname, mname, inner, inner_c, tail in STRUCTS:
        mirror = getattr(_lib, mname)
        size, offsets = layout[cname]
        assert size == ctypes.sizeof(mirror) == mirror().struct_size, cname
        assert offsets == {n: getattr(mirror, n).offset for n, _ in mirror._fields_}, cname
        assert [n for n, _ in mirror._fields_] == ["struct_size", "n_init", "states", "start_slots_ptr", "start_slots_batch_stride", "init_ptr"] + tail
        assert mirror.n_init.offset == 4
        assert mirror.states.size == ctypes.sizeof(getattr(_lib, inner)) == layout[inner_c][0], cname      # embedded whole
    lib = _lib.load()
    assert lib.dimsum_abi_version() == 18                                                         # no existing struct or symbol changed
    header = open(_lib.os.path.join(_lib._HERE, "..", "include", "dimsum_hip.h")).read()
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(lib, name) and f"int {name}(" in header, name


@pytest.mark.parametrize("which", [0, 1], ids=["conv", "scan"])
def test_library_checks_in_their_documented_order(which):
    """each call breaks one rule AND every later one's, so the code names the first failing check; nothing is ever launched"""
    from dimsum_amd import _lib
    fn, mirror = getattr(_lib.load(), SYMBOLS[which]), getattr(_lib, STRUCTS[which][1])
    buf = (ctypes.c_float * 64)()
    addr = ctypes.addressof(buf)
    addr += (-addr) % 16
    assert fn(None, None) == NULL
    for delta in (-8, 8, -ctypes.sizeof(mirror) + 4):
        P = mirror()
        P.struct_size += delta
        assert fn(P, None) == ABI, delta
    P = mirror()
    P.struct_size = ctypes.sizeof(getattr(_lib, STRUCTS[which][2]))                               # a stale caller: the states struct's size
    assert fn(P, None) == ABI
    P = mirror()                                                                                  # zeroed: every later rule is broken too
    assert fn(P, None) == SHAPE                                                                   # n_init
    P.n_init = -1
    assert fn(P, None) == SHAPE
    P.n_init = 3
    assert fn(P, None) == NULL                                                                    # start_slots_ptr
    P.start_slots_ptr = addr
    assert fn(P, None) == NULL                                                                    # init_ptr
    P.init_ptr = addr
    S = P.states
    inner = S.varlen.conv if which == 0 else S.varlen.scan
    inner.batch, inner.seqlen = 2, 5
    P.start_slots_batch_stride = -1
    assert fn(P, None) == STRIDE
    P.start_slots_batch_stride = 4                                                                # rows of 5 entries would overlap
    assert fn(P, None) == STRIDE
    P.start_slots_batch_stride = 5
    P.init_slot_stride = -1
    assert fn(P, None) == STRIDE
    P.init_slot_stride = 0
    # then the states entry's checks in their order
    assert fn(P, None) == SHAPE                                                                   # num_slots
    S.num_slots = 5
    assert fn(P, None) == NULL                                                                    # end_slots_ptr
    S.end_slots_ptr = addr
    assert fn(P, None) == NULL                                                                    # state_ptr
    S.state_ptr = addr
    S.end_slots_batch_stride = 4
    assert fn(P, None) == STRIDE
    S.end_slots_batch_stride = 5
    S.state_slot_stride = -1
    assert fn(P, None) == STRIDE
    S.state_slot_stride = 0
    assert fn(P, None) == NULL                                                                    # the varlen entry point's pointers
    for f, _ in inner._fields_:
        if f.endswith("_ptr"):
            setattr(inner, f, addr)
    assert fn(P, None) == SHAPE                                                                   # width / dim / dstate still zero
    if which == 0:
        inner.dim, inner.width = 8, 4
        inner.dtype = 3
        assert fn(P, None) == DTYPE
        inner.dtype = 1
        assert fn(P, None) == NULL                                                                # seq_idx_ptr
        S.varlen.seq_idx_ptr, S.varlen.seq_idx_batch_stride = addr, 4
        assert fn(P, None) == STRIDE
        S.varlen.seq_idx_batch_stride = 5
        S.state_dtype = 0
        assert fn(P, None) == UNSUPPORTED                                                         # the pool's dtype is not x's
        S.state_dtype = 1
        P.init_dtype = 0
        assert fn(P, None) == UNSUPPORTED                                                         # init's dtype is not x's: last
        inner.batch, P.init_dtype = 0, 1
        assert fn(P, None) == OK                                                                  # nothing to do, nothing launched
    else:
        inner.dim, inner.dstate, inner.n_groups, inner.n_chunks = 8, 16, 1, 1
        inner.is_variable_B = inner.is_variable_C = 1
        inner.dtype = 3
        assert fn(P, None) == DTYPE
        inner.dtype = 0
        inner.u_d_stride = -1
        assert fn(P, None) == STRIDE
        inner.u_d_stride = 5
        assert fn(P, None) == NULL                                                                # seq_idx_ptr
        S.varlen.seq_idx_ptr, S.varlen.seq_idx_batch_stride = addr, 4
        assert fn(P, None) == STRIDE
        S.varlen.seq_idx_batch_stride = 5
        for field in ("is_complex", "is_variable_B", "is_variable_C"):
            old = getattr(inner, field)
            setattr(inner, field, 1 - old)
            assert fn(P, None) == UNSUPPORTED, field
            setattr(inner, field, old)
