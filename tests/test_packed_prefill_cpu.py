"""CPU tests of packed prefill into slots: the end_slots contract on the float64 restatements, plan_packed_prefill,
the refusals with their reasons, DecodeEngine(packed_prefill=True) on the torch stand-ins, and the two C entry points' host checks in
their documented order (host memory that is never dereferenced: every call fails a check before any launch)."""
import ctypes

import pytest
import torch

from oracle.torch_backend import cpu_oracle_backend
from test_host_logic import _header_layout
from test_lm_cpu import tiny_model
from test_slots_cpu import REQUESTS, _alone, _prompts, decode_linear_slots_torch, native_conv_update, native_state_update

OK, NULL, DTYPE, SHAPE, STRIDE, UNSUPPORTED, ABI = 0, 1, 2, 3, 4, 5, 7
F64 = torch.float64


# ---- the contract on float64 ---------------------------------------------------------------------------------------------------------------------------
def _row(lengths, slots, pad=0):
    """one packed row: ids, end_slots (slot at every segment's last position, -1 elsewhere; a trailing padding segment stores nothing)"""
    from dimsum_amd.utils import seq_idx_from_lengths
    L = sum(lengths) + pad
    seq = seq_idx_from_lengths(lengths, L).view(1, L)
    ends = torch.full((1, L), -1, dtype=torch.int32)
    t = 0
    for n, s in zip(lengths, slots):
        t += n
        ends[0, t - 1] = s
    return seq, ends


LENGTHS, SLOTS, POOL = [1, 5, 2, 3, 1, 6], [4, 0, 6, 2, 7, 1], 9       # lengths 1, 2, 3 < width 4; slots 3, 5, 8 belong to nobody


@pytest.mark.parametrize("width", [2, 3, 4])
def test_conv_restatement_stores_every_segments_tail(width):
    from dimsum_amd.ops import causal_conv1d_varlen_torch
    g = torch.Generator().manual_seed(width)
    seq, ends = _row(LENGTHS, SLOTS, pad=3)
    L, D = seq.shape[1], 5
    x, w, b = torch.randn(1, D, L, generator=g, dtype=F64), torch.randn(D, width, generator=g, dtype=F64), torch.randn(D, generator=g, dtype=F64)
    pool = torch.full((POOL, D, width), 7.0, dtype=F64)
    out = causal_conv1d_varlen_torch(x, w, b, "silu", seq, end_slots=ends, conv_state=pool)
    assert torch.equal(out, causal_conv1d_varlen_torch(x, w, b, "silu", seq))                     # the outputs do not change
    t = 0
    for n, s in zip(LENGTHS, SLOTS):
        alone = x[0, :, t:t + n]                                                                  # the segment as a row of its own
        want = torch.nn.functional.pad(alone, (max(width - n, 0), 0))[:, -width:]                 # its tail, zero-padded on the left
        assert torch.equal(pool[s], want), (n, s)
        t += n
    for s in set(range(POOL)) - set(SLOTS):
        assert bool((pool[s] == 7.0).all()), s                                                    # unnamed slots untouched
    none = torch.full_like(pool, 7.0)
    causal_conv1d_varlen_torch(x, w, b, "silu", seq, end_slots=torch.full_like(ends, -1), conv_state=none)
    assert bool((none == 7.0).all())                                                              # -1 stores nothing


@pytest.mark.parametrize("N", [3, 16])
def test_scan_restatement_stores_every_segments_last_state(N):
    from dimsum_amd.ops import selective_scan_varlen_torch
    g = torch.Generator().manual_seed(N)
    seq, ends = _row(LENGTHS, SLOTS, pad=2)
    L, D = seq.shape[1], 4
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    u, dt, A, B, C, Dv, z, bias = r(1, D, L), 0.5 * torch.rand(1, D, L, generator=g, dtype=F64), -torch.rand(D, N, generator=g, dtype=F64), r(1, N, L), r(1, N, L), r(D), r(1, D, L), r(D)
    pool = torch.full((POOL, D, N), 7.0, dtype=F64)
    out, last = selective_scan_varlen_torch(u, dt, A, B, C, Dv, z, bias, True, True, seq_idx=seq, end_slots=ends, ssm_state=pool)
    plain, plain_last = selective_scan_varlen_torch(u, dt, A, B, C, Dv, z, bias, True, True, seq_idx=seq)
    assert torch.equal(out, plain) and torch.equal(last, plain_last)
    t = 0
    for n, s in zip(LENGTHS, SLOTS):
        sl = slice(t, t + n)
        _, alone = selective_scan_varlen_torch(u[:, :, sl], dt[:, :, sl], A, B[:, :, sl], C[:, :, sl], Dv, z[:, :, sl], bias, True, True)
        # the same float64 expressions on tensors of another length: torch's vectorised exp may differ from its scalar tail by an ulp per
        # step, and a segment has at most 6 steps with |exp(dt A)| <= 1 -- 64 eps of the state's magnitude bounds that with room
        assert float((pool[s] - alone[0]).abs().max()) <= 64 * torch.finfo(F64).eps * float(alone.abs().max()), (n, s)
        t += n
    for s in set(range(POOL)) - set(SLOTS):
        assert bool((pool[s] == 7.0).all()), s
    none = torch.full_like(pool, 7.0)
    selective_scan_varlen_torch(u, dt, A, B, C, Dv, z, bias, True, seq_idx=seq, end_slots=torch.full_like(ends, -1), ssm_state=none)
    assert bool((none == 7.0).all())


# ---- plan_packed_prefill ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 2])
@pytest.mark.parametrize("pad_multiple", [1, 4])
def test_plan_packs_every_token_once(rows, pad_multiple):
    from dimsum_amd.utils import plan_packed_prefill
    lengths, slots = [5, 3, 7, 1, 4], [2, 0, 4, 1, 3]
    plan = plan_packed_prefill(lengths, slots, rows=rows, pad_multiple=pad_multiple)
    again = plan_packed_prefill(lengths, slots, rows=rows, pad_multiple=pad_multiple)
    assert all(torch.equal(plan[k], again[k]) for k in ("seq_idx", "end_slots", "logits_positions")) and plan["segments"] == again["segments"]
    seq, ends, L = plan["seq_idx"], plan["end_slots"], plan["seqlen"]
    assert seq.shape == ends.shape == (rows, L) and seq.dtype == ends.dtype == torch.int32 and L % pad_multiple == 0
    assert plan["logits_positions"].dtype == torch.int64 and not seq.is_cuda
    cover = torch.zeros(rows, L, dtype=torch.long)
    for (r, start), n, s, pos in zip(plan["segments"], lengths, slots, plan["logits_positions"].tolist()):
        cover[r, start:start + n] += 1
        ids = seq[r, start:start + n]
        assert bool((ids == ids[0]).all())                                                        # one id per segment ...
        assert start == 0 or int(seq[r, start - 1]) != int(ids[0])                                # ... that differs from its neighbours'
        assert start + n == L or int(seq[r, start + n]) != int(ids[0])
        assert pos == r * L + start + n - 1 and int(ends.view(-1)[pos]) == s                      # the last token: logits and slot
    assert int(cover.max()) == 1 and int(cover.sum()) == sum(lengths)                             # every real token once
    assert bool((ends[cover == 0] == -1).all()) and int((ends >= 0).sum()) == len(lengths)        # padding stores nothing
    if rows == 1:
        assert plan["segments"] == [(0, 0), (0, 5), (0, 8), (0, 15), (0, 16)]
    else:
        assert plan["segments"] == [(0, 0), (1, 0), (1, 3), (0, 5), (0, 6)]                       # greedily onto the shortest row
    for bad in (dict(lengths=[0], slots=[0]), dict(lengths=[1, 2], slots=[3, 3]), dict(lengths=[1], slots=[-1]), dict(lengths=[1], slots=[0, 1]),
                dict(lengths=[1], slots=[0], rows=0)):
        with pytest.raises(ValueError, match="plan_packed_prefill"):
            plan_packed_prefill(**bad)


# ---- the refusals, each with its reason ------------------------------------------------------------------------------------------------------------------
def test_operator_refusals_carry_their_reason():
    from dimsum_amd import native
    from dimsum_amd.ops import causal_conv1d_fn, mamba_inner_fn_cond, selective_scan_fn
    x, w = torch.randn(2, 4, 6), torch.randn(4, 4)
    seq, ends = torch.zeros(2, 6, dtype=torch.int32), torch.full((2, 6), -1, dtype=torch.int32)
    pool = torch.zeros(3, 4, 4)
    with pytest.raises(ValueError, match="end_slots without seq_idx"):
        causal_conv1d_fn(x, w, end_slots=ends, conv_state=pool)
    with pytest.raises(ValueError, match="go together"):
        causal_conv1d_fn(x, w, seq_idx=seq, end_slots=ends)
    with pytest.raises(NotImplementedError, match="inference arguments"):
        causal_conv1d_fn(x.requires_grad_(), w, seq_idx=seq, end_slots=ends, conv_state=pool)
    x = x.detach()
    A, Bm, st = -torch.rand(4, 3), torch.randn(2, 3, 6), torch.zeros(3, 4, 3)
    with pytest.raises(ValueError, match="end_slots without seq_idx"):
        selective_scan_fn(x, x, A, Bm, Bm, end_slots=ends, ssm_state=st)
    with pytest.raises(ValueError, match="go together"):
        selective_scan_fn(x, x, A, Bm, Bm, seq_idx=seq, ssm_state=st)
    with pytest.raises(NotImplementedError, match="inference arguments"):
        selective_scan_fn(x, x, A.requires_grad_(), Bm, Bm, seq_idx=seq, end_slots=ends, ssm_state=st)
    A = A.detach()
    with pytest.raises(NotImplementedError, match="initial_state"):
        selective_scan_fn(x, x, A, Bm, Bm, seq_idx=seq, end_slots=ends, ssm_state=st, initial_state=torch.zeros(2, 4, 3))
    with pytest.raises(NotImplementedError, match="constant"):
        selective_scan_fn(x, x, A, torch.randn(4, 3), Bm, seq_idx=seq, end_slots=ends, ssm_state=st)
    xz, cw, xp, dp, op = torch.randn(2, 8, 6), torch.randn(4, 1, 4), torch.randn(1 + 6, 4), torch.randn(4, 1), torch.randn(2, 4)
    with pytest.raises(ValueError, match="end_slots without seq_idx"):
        mamba_inner_fn_cond(xz, cw, None, xp, dp, op, None, A, end_slots=ends, conv_state=pool, ssm_state=st)
    with pytest.raises(ValueError, match="go together"):
        mamba_inner_fn_cond(xz, cw, None, xp, dp, op, None, A, seq_idx=seq, end_slots=ends, conv_state=pool)
    # native: dtype, rank, shape and contiguity of end_slots need no GPU, the pool's dtype is named with the reason, the device comes last
    for bad in (ends.long(), ends[:, :5].contiguous(), torch.full((6, 2), -1, dtype=torch.int32).t(), ends[0]):
        with pytest.raises(RuntimeError, match="end_slots must be a contiguous int32"):
            native.causal_conv1d_varlen_states_fwd(x, w, None, True, seq, bad, pool)
        with pytest.raises(RuntimeError, match="end_slots must be a contiguous int32"):
            native.selective_scan_varlen_states_fwd(x, x, A, Bm.unsqueeze(1), Bm.unsqueeze(1), None, None, None, True, seq, bad, st)
    with pytest.raises(RuntimeError, match="conv_state must have x's dtype"):
        native.causal_conv1d_varlen_states_fwd(x, w, None, True, seq, ends, pool.half())
    with pytest.raises(RuntimeError, match=r"pool \(num_slots >= 1, dim, width\)"):
        native.causal_conv1d_varlen_states_fwd(x, w, None, True, seq, ends, torch.zeros(3, 4, 3))
    with pytest.raises(RuntimeError, match="ssm_state must be float32 or of u's dtype"):
        native.selective_scan_varlen_states_fwd(x, x, A, Bm.unsqueeze(1), Bm.unsqueeze(1), None, None, None, True, seq, ends, st.double())
    with pytest.raises(RuntimeError, match="expected a GPU tensor"):
        native.causal_conv1d_varlen_states_fwd(x, w, None, True, seq, ends, pool)


@pytest.fixture
def packed_backend(monkeypatch):
    """the two packed-row operators replaced by their torch restatements (same signatures) and the three slot launches by test_slots_cpu's
    stand-ins, everything else on the CPU oracle backend"""
    from dimsum_amd import native
    from dimsum_amd.ops import causal_conv1d_varlen_torch, selective_scan_interface, selective_scan_varlen_torch
    monkeypatch.setattr(selective_scan_interface, "causal_conv1d_fn", causal_conv1d_varlen_torch)
    monkeypatch.setattr(selective_scan_interface, "selective_scan_fn", selective_scan_varlen_torch)
    monkeypatch.setattr(native, "causal_conv1d_update", native_conv_update)
    monkeypatch.setattr(native, "selective_state_update", native_state_update)
    monkeypatch.setattr(native, "decode_linear", decode_linear_slots_torch)
    with cpu_oracle_backend():
        yield


def test_module_refusals_carry_their_reason(packed_backend):
    from dimsum_amd.modules.mamba_simple import CondMamba, Mamba
    from dimsum_amd.utils import InferenceParams, chunked_prefill, plan_packed_prefill
    m = tiny_model(1, 1)
    plan = plan_packed_prefill([3, 2], [1, 0])
    ids = torch.randint(0, 90, (1, 5))
    new = lambda **kw: InferenceParams(max_seqlen=8, max_batch_size=1, key_value_memory_dict=m.allocate_inference_cache(3, 8),
                                       prefill_slots=plan["end_slots"], **kw)
    assert InferenceParams(max_seqlen=8, max_batch_size=1).prefill_slots is None
    p = new()
    p.reset(9, 1)
    assert p.prefill_slots is plan["end_slots"]                                                   # reset leaves it alone
    with torch.no_grad():
        with pytest.raises(ValueError, match="prefill_slots without seq_idx"):
            m(ids, inference_params=new())
        with pytest.raises(ValueError, match="seq_idx at seqlen_offset > 0|prefill_slots at seqlen_offset > 0"):
            m(ids, inference_params=new(seqlen_offset=5), seq_idx=plan["seq_idx"])
        mixer = m.backbone.layers[0].mixer
        with pytest.raises(ValueError, match="prefill_slots at seqlen_offset > 0"):
            mixer(torch.zeros(1, 5, 64), inference_params=new(seqlen_offset=5), seq_idx=plan["seq_idx"])
        with pytest.raises(ValueError, match="prefill_slots together with state_indices"):
            m(ids, inference_params=new(state_indices=torch.zeros(1, dtype=torch.int32)), seq_idx=plan["seq_idx"])
        with pytest.raises(ValueError, match="prefill_slots must be an int32"):
            p = new()
            p.prefill_slots = plan["end_slots"][:, :4]
            m(ids, inference_params=p, seq_idx=plan["seq_idx"])
        with pytest.raises(ValueError, match="need a pool"):
            mixer(torch.zeros(1, 5, 64), inference_params=InferenceParams(max_seqlen=8, max_batch_size=1, prefill_slots=plan["end_slots"]),
                  seq_idx=plan["seq_idx"])
        with pytest.raises(NotImplementedError, match="extend with prefill_slots"):
            mixer.extend(torch.zeros(1, 3, 64), *new().key_value_memory_dict[0], prefill_slots=plan["end_slots"])
        with pytest.raises(NotImplementedError, match="chunked_prefill with prefill_slots"):
            chunked_prefill(mixer, torch.zeros(1, 4, 64), new(), 2)
        p = new()
        p.key_value_memory_dict = {k: (c.half(), s) for k, (c, s) in p.key_value_memory_dict.items()}
        with pytest.raises(NotImplementedError, match="the conv pool is torch.float16 but the activations are torch.float32"):
            m(ids, inference_params=p, seq_idx=plan["seq_idx"])
        pools = lambda mod: {0: mod.allocate_inference_cache(3, 8)}
        kw = dict(d_state=4, d_conv=4, expand=2, layer_idx=0)
        for scan_type, reason in (("v2", 'scan_type "v2"'), ("zigma8", "zigma8")):
            mod = Mamba(16, scan_type=scan_type, num_patches=4, **kw).eval() if scan_type != "v2" else Mamba(16, scan_type="v2", **kw).eval()
            with pytest.raises(NotImplementedError, match=reason):
                mod(torch.zeros(1, 5, 16), inference_params=InferenceParams(8, 1, key_value_memory_dict=pools(mod), prefill_slots=plan["end_slots"]),
                    seq_idx=plan["seq_idx"])
        plain = Mamba(16, **kw).eval()
        with pytest.raises(NotImplementedError, match=r"operand-image input \(x3\)"):
            plain(None, inference_params=InferenceParams(8, 1, key_value_memory_dict=pools(plain), prefill_slots=plan["end_slots"]),
                  x3=torch.zeros(1, 5, 16), seq_idx=plan["seq_idx"])
        with pytest.raises(NotImplementedError, match=r"conditional conv entry \(cond\)"):
            plain._mix(torch.zeros(1, 5, 16), torch.zeros(1, 32), states=pools(plain)[0], seq_idx=plan["seq_idx"], prefill_slots=plan["end_slots"])
        cm = CondMamba(16, **kw).eval()                                                           # its forward takes no seq_idx at all
        with pytest.raises(ValueError, match="prefill_slots without seq_idx"):
            cm(torch.zeros(1, 5, 16), inference_params=InferenceParams(8, 1, key_value_memory_dict=pools(cm), prefill_slots=plan["end_slots"]))
        # the head's row gather
        with pytest.raises(ValueError, match="logits_positions without seq_idx"):
            m(ids, logits_positions=plan["logits_positions"])
        with pytest.raises(ValueError, match="together with num_last_tokens"):
            m(ids, seq_idx=plan["seq_idx"], logits_positions=plan["logits_positions"], num_last_tokens=1)
        with pytest.raises(ValueError, match="1-D int64"):
            m(ids, seq_idx=plan["seq_idx"], logits_positions=plan["logits_positions"].int())


def test_packed_pass_fills_the_slots_like_alone_prefills(packed_backend):
    """the LM on one packed pass: every request's states land in its slot as an alone prefill through the same packed-row route leaves them,
    the gathered logits are the requests' last-token logits, unnamed slots stay 7.0"""
    from dimsum_amd.utils import InferenceParams, plan_packed_prefill
    m = tiny_model(1, 1)
    prompts = _prompts()[:4]
    slots = [3, 0, 4, 1]
    for rows in (1, 2):
        plan = plan_packed_prefill([p.numel() for p in prompts], slots, rows=rows)
        ids = torch.zeros(rows, plan["seqlen"], dtype=torch.long)
        for p, (r, s) in zip(prompts, plan["segments"]):
            ids[r, s:s + p.numel()] = p
        pool = m.allocate_inference_cache(6, 16)
        for conv, ssm in pool.values():
            conv.fill_(7.0)
            ssm.fill_(7.0)
        with torch.no_grad():
            logits = m(ids, inference_params=InferenceParams(16, rows, key_value_memory_dict=pool, prefill_slots=plan["end_slots"]),
                       seq_idx=plan["seq_idx"], logits_positions=plan["logits_positions"]).logits
            assert logits.shape[0] == 4 and logits.dim() == 2
            for i, (p, s) in enumerate(zip(prompts, slots)):
                own = InferenceParams(16, 1)
                want = m(p.unsqueeze(0), inference_params=own, seq_idx=torch.zeros(1, p.numel(), dtype=torch.int32), num_last_tokens=1).logits[0, -1]
                torch.testing.assert_close(logits[i], want, rtol=1e-4, atol=1e-5)
                for k, (conv, ssm) in pool.items():
                    torch.testing.assert_close(conv[s:s + 1], own.key_value_memory_dict[k][0], rtol=1e-5, atol=1e-6)
                    torch.testing.assert_close(ssm[s:s + 1], own.key_value_memory_dict[k][1], rtol=1e-4, atol=1e-5)
        for conv, ssm in pool.values():
            assert bool((conv[[2, 5]] == 7.0).all()) and bool((ssm[[2, 5]] == 7.0).all())


# ---- the engine ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefill_rows", [1, 2])
def test_engine_admits_k_requests_with_one_model_pass(prefill_rows, packed_backend, monkeypatch):
    from dimsum_amd.utils.serving import DecodeEngine
    monkeypatch.setenv("DIMSUM_FUSED_DECODE", "1")
    m = tiny_model(1, 1)
    prompts = _prompts()
    alone = [_alone(m, p, n) for p, (_, n) in zip(prompts, REQUESTS)]
    calls = []
    hook = m.register_forward_pre_hook(lambda mod, args, kwargs: calls.append(args[0].shape if kwargs.get("seq_idx") is not None else None), with_kwargs=True)
    eng = DecodeEngine(m, max_batch=2, num_slots=3, max_seqlen=32, vocab_size=90, cg=False, fused_sampling=False, packed_prefill=True,
                       prefill_rows=prefill_rows)
    assert DecodeEngine(m, max_batch=2, max_seqlen=32, cg=False, fused_sampling=False).packed_prefill is False       # off by default
    rids = [eng.submit(p, n) for p, (_, n) in zip(prompts, REQUESTS)]
    eng.step()
    # the first step: ONE prompt pass admitted the two requests that fit (two rows), then one decode step
    assert [c for c in calls if c is not None] == [(prefill_rows, calls[0][1])] and len(calls) == 2 and eng.n_prefill_passes == 1
    assert eng.slot_history == [(0, 0), (1, 1)] and eng.free_slots[0] == 2 and eng.n_captures == 0
    step = 1
    while not eng.idle():
        eng.step()
        held = [eng.requests[rid].slot for rid in eng.rows if rid is not None]
        assert len(set(held)) == len(held) and sorted(held + eng.free_slots) == [0, 1, 2]         # slot bookkeeping as before
        assert eng.slots.tolist() == [-1 if rid is None else eng.requests[rid].slot for rid in eng.rows]
        step += 1
        assert step < 100
    hook.remove()
    for rid, (seq, _) in zip(rids, alone):
        assert torch.equal(eng.sequence(rid), seq), rid
    reused = [slot for _, slot in eng.slot_history]
    assert len(reused) == 6 and len(set(reused)) == 3 and eng.n_prefill_passes < 6                # released slots reused; fewer passes than requests
    # the token budget: one request always fits, a second one only within the budget
    eng = DecodeEngine(m, max_batch=4, max_seqlen=32, vocab_size=90, cg=False, fused_sampling=False, packed_prefill=True, max_prefill_tokens=8)
    for p, (_, n) in zip(prompts, REQUESTS):
        eng.submit(p, n)
    eng.step()
    assert [rid for rid, _ in eng.slot_history] == [0, 1]                                         # 5 + 3 tokens fit 8, the 7-token prompt waits
    monkeypatch.setenv("DIMSUM_PACKED_PREFILL", "1")
    assert DecodeEngine(m, max_batch=2, max_seqlen=32, cg=False, fused_sampling=False).packed_prefill is True
    with pytest.raises(ValueError, match="prefill_rows"):
        DecodeEngine(m, max_batch=2, max_seqlen=32, cg=False, fused_sampling=False, prefill_rows=0)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------------------------
STRUCTS = [("dimsum_conv_varlen_states_params_t", "ConvVarlenStatesParams", "ConvVarlenParams", "dimsum_conv_varlen_params_t",
            ["state_slot_stride", "state_c_stride", "state_w_stride", "state_dtype", "reserved"]),
           ("dimsum_ssm_varlen_states_params_t", "SsmVarlenStatesParams", "SsmVarlenParams", "dimsum_ssm_varlen_params_t",
            ["state_slot_stride", "state_d_stride", "state_dstate_stride", "state_f32", "reserved"])]
SYMBOLS = ("dimsum_causal_conv1d_varlen_states_fwd", "dimsum_ssm_scan_varlen_states_fwd")


def test_structs_symbols_and_abi_version():
    from dimsum_amd import _lib
    layout = _header_layout([(c, getattr(_lib, m)) for c, m, _, _, _ in STRUCTS] + [(c, getattr(_lib, m)) for _, _, m, c, _ in STRUCTS])
    for cname, mname, inner, inner_c, tail in STRUCTS:
        mirror = getattr(_lib, mname)
        size, offsets = layout[cname]
        assert size == ctypes.sizeof(mirror) == mirror().struct_size, cname
        assert offsets == {n: getattr(mirror, n).offset for n, _ in mirror._fields_}, cname
        assert [n for n, _ in mirror._fields_] == ["struct_size", "num_slots", "varlen", "end_slots_ptr", "end_slots_batch_stride", "state_ptr"] + tail
        assert mirror.num_slots.offset == 4                                                       # the 4 bytes after struct_size
        assert mirror.varlen.size == ctypes.sizeof(getattr(_lib, inner)) == layout[inner_c][0], cname      # embedded whole
    lib = _lib.load()
    assert lib.dimsum_abi_version() == 18
    header = open(_lib.os.path.join(_lib._HERE, "..", "include", "dimsum_hip.h")).read()
    assert "#define DIMSUM_ABI_VERSION 18" in header
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
    P.struct_size = ctypes.sizeof(getattr(_lib, STRUCTS[which][2]))                               # a stale caller: the varlen struct's size
    assert fn(P, None) == ABI
    P = mirror()                                                                                  # zeroed: every later rule is broken too
    assert fn(P, None) == SHAPE
    P.num_slots = -1
    assert fn(P, None) == SHAPE
    P.num_slots = 5
    assert fn(P, None) == NULL                                                                    # end_slots_ptr
    P.end_slots_ptr = addr
    assert fn(P, None) == NULL                                                                    # state_ptr
    P.state_ptr = addr
    inner = P.varlen.conv if which == 0 else P.varlen.scan
    inner.batch, inner.seqlen = 2, 5
    P.end_slots_batch_stride = -1
    assert fn(P, None) == STRIDE
    P.end_slots_batch_stride = 4                                                                  # rows of 5 entries would overlap
    assert fn(P, None) == STRIDE
    P.end_slots_batch_stride = 5
    P.state_slot_stride = -1
    assert fn(P, None) == STRIDE
    P.state_slot_stride = 0
    assert fn(P, None) == NULL                                                                    # then the varlen entry point's checks: its pointers
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
        P.varlen.seq_idx_ptr, P.varlen.seq_idx_batch_stride = addr, 4
        assert fn(P, None) == STRIDE
        P.varlen.seq_idx_batch_stride = 5
        P.state_dtype = 0
        assert fn(P, None) == UNSUPPORTED                                                         # the pool's dtype is not x's: last
        inner.batch, P.state_dtype = 0, 1
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
        P.varlen.seq_idx_ptr, P.varlen.seq_idx_batch_stride = addr, 4
        assert fn(P, None) == STRIDE
        P.varlen.seq_idx_batch_stride = 5
        for field in ("is_complex", "is_variable_B", "is_variable_C"):
            old = getattr(inner, field)
            setattr(inner, field, 1 - old)
            assert fn(P, None) == UNSUPPORTED, field
            setattr(inner, field, old)
