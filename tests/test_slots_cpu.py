"""Slot-indexed decode states without a GPU: the three new symbols, their structs and their refusals in the documented order, nothing launched;
the refusals of native's `state_indices` (shape first, device last); the plain-torch restatements with slots against the un-indexed
restatements on gathered rows; InferenceParams.state_indices and where it is refused; DecodeEngine's scheduling on the torch stand-ins of the
step (test_lm_cpu.py's, taught the slot argument through the restatements), each request against generate() of that request alone."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from oracle.torch_backend import cpu_oracle_backend
from test_host_logic import _header_layout
from test_lm_cpu import decode_linear_torch, tiny_model

STRUCTS = [("dimsum_conv_update_slots_params_t", "ConvUpdateSlotsParams", "conv", "ConvUpdateParams", "dimsum_conv_update_params_t"),
           ("dimsum_state_update_slots_params_t", "StateUpdateSlotsParams", "update", "StateUpdateParams", "dimsum_state_update_params_t"),
           ("dimsum_decode_linear_slots_params_t", "DecodeLinearSlotsParams", "linear", "DecodeLinearParams", "dimsum_decode_linear_params_t")]
SYMBOLS = ("dimsum_causal_conv1d_update_slots", "dimsum_selective_state_update_slots", "dimsum_decode_linear_slots")
OK, NULL, DTYPE, SHAPE, STRIDE, UNSUPPORTED, ABI = 0, 1, 2, 3, 4, 5, 7
SLOTS = [5, -1, 0, 3]                                      # batch 4 on a pool of 7: one padding row, slots out of order
POOL = 7


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------------------
def test_structs_symbols_and_abi_version():
    from dimsum_amd import _lib
    layout = _header_layout([(c, getattr(_lib, m)) for c, m, _, _, _ in STRUCTS] + [(c, getattr(_lib, m)) for _, _, _, m, c in STRUCTS])
    for cname, mname, field, inner, inner_c in STRUCTS:
        mirror = getattr(_lib, mname)
        size, offsets = layout[cname]
        assert size == ctypes.sizeof(mirror) == mirror().struct_size, cname
        assert offsets == {n: getattr(mirror, n).offset for n, _ in mirror._fields_}, cname
        assert [n for n, _ in mirror._fields_] == ["struct_size", "num_slots", field, "slots_ptr", "slots_stride"]
        # the embedded struct is the existing one, whole and untouched
        assert getattr(mirror, field).size == ctypes.sizeof(getattr(_lib, inner)) == layout[inner_c][0], cname
    lib = _lib.load()
    assert lib.dimsum_abi_version() == 18                  # new symbols only: the ABI number stands
    header = open(_lib.os.path.join(_lib._HERE, "..", "include", "dimsum_hip.h")).read()
    assert "#define DIMSUM_ABI_VERSION 18" in header
    for name in SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(lib, name) and f"int {name}(" in header, name


@pytest.mark.parametrize("name,mname,field", [(s, m, f) for s, (_, m, f, _, _) in zip(SYMBOLS, STRUCTS)])
def test_library_checks_in_their_documented_order(name, mname, field):
    """host memory that is never dereferenced; each call breaks one rule AND every later one's, so the code names the first failing check"""
    from dimsum_amd import _lib
    fn, mirror = getattr(_lib.load(), name), getattr(_lib, mname)
    buf = (ctypes.c_float * 1024)()
    addr = ctypes.addressof(buf)
    assert fn(None, None) == NULL
    for delta in (-8, 8, -ctypes.sizeof(mirror) + 4):      # truncated, grown (a newer header), only the size field
        P = mirror()
        P.struct_size += delta
        assert fn(P, None) == ABI, delta
    P = mirror()
    P.struct_size = ctypes.sizeof(getattr(_lib, mname.replace("Slots", "")))     # a stale caller: the plain struct's size
    assert fn(P, None) == ABI
    P = mirror()                                           # zeroed: num_slots 0, slots NULL, every pointer of the embedded struct NULL
    assert fn(P, None) == SHAPE
    P.num_slots = -3
    assert fn(P, None) == SHAPE
    P.num_slots = 7
    assert fn(P, None) == NULL                             # slots_ptr
    P.slots_ptr, P.slots_stride = addr, -1
    assert fn(P, None) == STRIDE
    P.slots_stride = 1
    inner = getattr(P, field)
    if name == "dimsum_decode_linear_slots":
        assert fn(P, None) == UNSUPPORTED                  # no epilogue, no state to index
        inner.conv_dim = 1
    assert fn(P, None) == NULL                             # then the plain entry point's checks: its pointers first
    for f, _ in inner._fields_:
        if f.endswith("_ptr"):
            setattr(inner, f, addr)
    inner.batch = 0
    assert fn(P, None) == SHAPE                            # pointers set, sizes still zero: nothing was launched on host memory


# ---- native's refusals: they need no GPU, and the device comes last ------------------------------------------------------------------------------------
def _conv_args():
    return torch.zeros(4, 6), torch.zeros(POOL, 6, 4), torch.zeros(6, 4), None, True


def _ssu_args():
    return torch.zeros(POOL, 6, 16), torch.zeros(4, 6), torch.zeros(4, 6), torch.zeros(6, 16), torch.zeros(4, 16), torch.zeros(4, 16)


CALLS = {
    "conv": lambda idx: __import__("dimsum_amd").native.causal_conv1d_update(*_conv_args(), state_indices=idx),
    "ssu": lambda idx: __import__("dimsum_amd").native.selective_state_update(*_ssu_args(), state_indices=idx),
    "linear": lambda idx: __import__("dimsum_amd").native.decode_linear(torch.zeros(4, 8), torch.zeros(12, 8), conv=(torch.zeros(POOL, 6, 4), torch.zeros(6, 4), None, True), state_indices=idx),
}


@pytest.mark.parametrize("which", list(CALLS))
def test_native_refuses_bad_indices_shape_first_device_last(which):
    import dimsum_amd.native  # noqa: F401
    call = CALLS[which]
    good = torch.tensor(SLOTS, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="int32"):
        call(good.long())
    with pytest.raises(RuntimeError, match="int32"):
        call(torch.zeros(3, 2, dtype=torch.int64))         # wrong in every way: the dtype is named first
    with pytest.raises(RuntimeError, match="1-D"):
        call(good.view(2, 2))
    with pytest.raises(RuntimeError, match="1-D"):
        call(torch.zeros(5, 1, dtype=torch.int32))         # 2-D and the wrong length: the rank first
    with pytest.raises(RuntimeError, match="batch = 4 entries, got 3"):
        call(good[:3])
    with pytest.raises(RuntimeError, match="state_indices must be a GPU tensor"):
        call(good)                                         # everything right but the device: the last check of the index
    with pytest.raises(RuntimeError, match="int32"):
        call(SLOTS)                                        # a list is no tensor


def test_decode_linear_indices_need_the_conv_epilogue():
    from dimsum_amd import native
    with pytest.raises(RuntimeError, match="need `conv`"):
        native.decode_linear(torch.zeros(4, 8), torch.zeros(12, 8), state_indices=torch.tensor(SLOTS, dtype=torch.int32))


# ---- the restatements with slots: an independent statement of the semantics ----------------------------------------------------------------------------
def _gather(pool, slots):
    live = [b for b, s in enumerate(slots) if s >= 0]
    return live, pool[[slots[b] for b in live]].clone()


@pytest.mark.parametrize("width,bias,act", [(4, True, "silu"), (3, False, None), (2, True, None)])
def test_conv_restatement_with_slots(width, bias, act):
    from dimsum_amd.ops import causal_conv1d_update_torch
    g = torch.Generator().manual_seed(3)
    x, pool, w = (torch.randn(*s, generator=g, dtype=torch.float64) for s in ((4, 6), (POOL, 6, width), (6, width)))
    b = torch.randn(6, generator=g, dtype=torch.float64) if bias else None
    before = pool.clone()
    live, rows = _gather(pool, SLOTS)
    want = causal_conv1d_update_torch(x[live], rows, w, b, act)
    out = causal_conv1d_update_torch(x, pool, w, b, act, state_indices=torch.tensor(SLOTS, dtype=torch.int32))
    assert torch.equal(out[live], want) and torch.equal(out[1], torch.zeros(6, dtype=torch.float64))
    for i, bi in enumerate(live):
        assert torch.equal(pool[SLOTS[bi]], rows[i])
    for s in set(range(POOL)) - {s for s in SLOTS if s >= 0}:
        assert torch.equal(pool[s], before[s]), s
    idle = torch.full((4,), -1, dtype=torch.int32)                     # every row padding: zeros out, and nothing in the pool moves
    after_live = pool.clone()
    assert not torch.equal(after_live, before)
    assert not causal_conv1d_update_torch(x, pool, w, b, act, state_indices=idle).any() and torch.equal(pool, after_live)


@pytest.mark.parametrize("N,gate", [(16, True), (5, False)])
def test_state_update_restatement_with_slots(N, gate):
    from dimsum_amd.ops import selective_state_update_torch
    g = torch.Generator().manual_seed(4)
    mk = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    pool, x, dt, B, C, D, db = mk(POOL, 6, N), mk(4, 6), 0.5 * mk(4, 6), mk(4, N), mk(4, N), mk(6), 0.3 * mk(6)
    A = -0.5 * torch.rand(6, N, generator=g, dtype=torch.float64) - 0.1
    z = mk(4, 6) if gate else None
    before = pool.clone()
    live, rows = _gather(pool, SLOTS)
    want = selective_state_update_torch(rows, x[live], dt[live], A, B[live], C[live], D, z[live] if gate else None, db, True)
    out = selective_state_update_torch(pool, x, dt, A, B, C, D, z, db, True, state_indices=torch.tensor(SLOTS, dtype=torch.int32))
    assert torch.equal(out[live], want) and not out[1].any()
    for i, bi in enumerate(live):
        assert torch.equal(pool[SLOTS[bi]], rows[i]) and not torch.equal(pool[SLOTS[bi]], before[SLOTS[bi]])
    for s in set(range(POOL)) - {s for s in SLOTS if s >= 0}:
        assert torch.equal(pool[s], before[s]), s
    after_live = pool.clone()
    idle = torch.full((4,), -1, dtype=torch.int32)
    out = selective_state_update_torch(pool, x, dt, A, B, C, D, z, db, True, state_indices=idle)
    assert not out.any() and torch.equal(pool, after_live)


# ---- torch stand-ins of the three launches that take the slot argument (test_lm_cpu.py's, through the restatements) ------------------------------------
def native_conv_update(x, conv_state, weight, bias, silu_activation, state_indices=None):
    from dimsum_amd.ops import causal_conv1d_update_torch
    return causal_conv1d_update_torch(x, conv_state, weight, bias, "silu" if silu_activation else None, state_indices=state_indices)


def native_state_update(state, x, dt, A, B, C, D=None, z=None, dt_bias=None, dt_softplus=False, dt_proj=None, state_indices=None):
    from dimsum_amd.ops import selective_state_update_torch
    if dt_proj is not None:
        assert dt is None
        dt = F.linear(dt_proj[1], dt_proj[0])
    return selective_state_update_torch(state, x, dt, A, B, C, D, z, dt_bias, dt_softplus, state_indices=state_indices)


def decode_linear_slots_torch(x, weight, bias=None, norm=None, residual=None, residual_out=None, conv=None, state_indices=None):
    """decode_linear_torch with the slot argument: the epilogue of row b on conv_state[slots[b]]; a padding row leaves zeros in y[b, :D]"""
    if state_indices is None:
        return decode_linear_torch(x, weight, bias, norm=norm, residual=residual, residual_out=residual_out, conv=conv)
    pool, cw, cb, silu = conv
    slots = state_indices.tolist()
    live = [b for b, s in enumerate(slots) if s >= 0]
    rows = pool.new_zeros((x.shape[0],) + tuple(pool.shape[1:]))
    rows[live] = pool[[slots[b] for b in live]]
    got = decode_linear_torch(x, weight, bias, norm=norm, residual=residual, residual_out=residual_out, conv=(rows, cw, cb, silu))
    pool[[slots[b] for b in live]] = rows[live]
    y = got if residual_out is None else got[0]
    y[[b for b, s in enumerate(slots) if s < 0], :cw.shape[0]] = 0
    return got


@pytest.fixture
def slots_backend(monkeypatch):
    from dimsum_amd import native
    monkeypatch.setattr(native, "causal_conv1d_update", native_conv_update)
    monkeypatch.setattr(native, "selective_state_update", native_state_update)
    monkeypatch.setattr(native, "decode_linear", decode_linear_slots_torch)
    with cpu_oracle_backend():
        yield


# ---- InferenceParams.state_indices -----------------------------------------------------------------------------------------------------------------------
def test_inference_params_carry_the_index_and_prompts_refuse_it(slots_backend):
    from dimsum_amd.utils import InferenceParams, chunked_prefill
    p = InferenceParams(max_seqlen=8, max_batch_size=2)
    assert p.state_indices is None
    idx = torch.tensor([1, 0], dtype=torch.int32)
    m = tiny_model(1, 1)
    p = InferenceParams(max_seqlen=8, max_batch_size=2, key_value_memory_dict=m.allocate_inference_cache(3, 8), state_indices=idx)
    p.reset(9, 2)
    assert p.state_indices is idx and p.seqlen_offset == 0                    # reset leaves it alone
    ids = torch.tensor([[1, 2, 3], [4, 5, 6]])
    with torch.no_grad():
        with pytest.raises(ValueError, match="state_indices at seqlen_offset == 0"):
            m(ids, inference_params=p)
        mixer = m.backbone.layers[0].mixer
        with pytest.raises(NotImplementedError, match="extend with state_indices"):
            mixer.extend(torch.zeros(2, 3, 64), *p.key_value_memory_dict[0], state_indices=idx)
        with pytest.raises(NotImplementedError, match="chunked_prefill with state_indices"):
            chunked_prefill(mixer, torch.zeros(2, 4, 64), p, 2)
        fresh = InferenceParams(max_seqlen=8, max_batch_size=2, seqlen_offset=1, state_indices=idx)    # no pool to index
        with pytest.raises(ValueError, match="need a pool"):
            mixer(torch.zeros(2, 1, 64), inference_params=fresh)


@pytest.mark.parametrize("fused", ["1", "0"], ids=["fused", "unfused"])
def test_a_step_on_pool_slots_is_the_step_on_the_rows_own_states(fused, slots_backend, monkeypatch):
    """two sequences prefilled into slots 2 and 0 of a 3-slot pool through views, then decoded as rows (0, 1, padding) with slots [2, 0, -1]:
    the logits are those of the same two sequences on a cache of their own; the untouched slot stays as it was"""
    from dimsum_amd.utils import InferenceParams
    monkeypatch.setenv("DIMSUM_FUSED_DECODE", fused)
    m = tiny_model(1, 1)
    g = torch.Generator().manual_seed(5)
    prompts = torch.randint(0, 90, (2, 6), generator=g)
    with torch.no_grad():
        own = InferenceParams(max_seqlen=16, max_batch_size=2)
        tok = m(prompts, inference_params=own, num_last_tokens=1).logits[:, -1].argmax(-1, keepdim=True)
        own.seqlen_offset = 6
        pool = m.allocate_inference_cache(3, 16)
        for conv, ssm in pool.values():
            conv.fill_(7.0)                                                    # nothing is zeroed: the prompt pass overwrites the slots it
            ssm.fill_(7.0)                                                     # fills, and slot 1 belongs to nobody
        for row, s in ((0, 2), (1, 0)):
            view = InferenceParams(max_seqlen=16, max_batch_size=1, key_value_memory_dict={k: tuple(t[s:s + 1] for t in st) for k, st in pool.items()})
            m(prompts[row:row + 1], inference_params=view, num_last_tokens=1)
        p = InferenceParams(max_seqlen=16, max_batch_size=3, seqlen_offset=6, key_value_memory_dict=pool,
                            state_indices=torch.tensor([2, 0, -1], dtype=torch.int32))
        for _ in range(3):
            want = m(tok, inference_params=own, num_last_tokens=1).logits[:, -1]
            got = m(torch.cat([tok, tok[:1]]), inference_params=p, num_last_tokens=1).logits[:, -1]
            assert torch.allclose(got[:2], want, rtol=1e-5, atol=1e-6) and torch.isfinite(got).all()
            tok = want.argmax(-1, keepdim=True)
        for conv, ssm in pool.values():
            assert bool((conv[1] == 7.0).all()) and bool((ssm[1] == 7.0).all())


@pytest.mark.parametrize("short", [1, 2, 3])
def test_a_short_prompt_overwrites_a_dirty_slot(short, slots_backend):
    """slots are not zeroed on release: a prompt shorter than d_conv (4) goes through the zero-padded branch of the prompt pass, and what it
    leaves in a slot full of 7.0 is bit for bit what it leaves in a fresh cache of its own -- both states, every layer; the neighbours stay"""
    from dimsum_amd.utils import InferenceParams
    m = tiny_model(1, 1)
    prompt = torch.randint(0, 90, (1, short), generator=torch.Generator().manual_seed(short))
    with torch.no_grad():
        own = InferenceParams(max_seqlen=8, max_batch_size=1)
        want = m(prompt, inference_params=own, num_last_tokens=1).logits
        pool = m.allocate_inference_cache(3, 8)
        for conv, ssm in pool.values():
            conv.fill_(7.0)
            ssm.fill_(7.0)
        view = InferenceParams(max_seqlen=8, max_batch_size=1, key_value_memory_dict={k: tuple(t[1:2] for t in st) for k, st in pool.items()})
        assert torch.equal(m(prompt, inference_params=view, num_last_tokens=1).logits, want)
    for i, (conv, ssm) in pool.items():
        own_conv, own_ssm = own.key_value_memory_dict[i]
        assert torch.equal(conv[1:2], own_conv) and torch.equal(ssm[1:2], own_ssm), i
        assert not conv[1, :, :4 - short].any() and conv[1, :, 4 - short:].any()               # zero-padded on the left, no 7.0 left over
        assert bool((conv[[0, 2]] == 7.0).all()) and bool((ssm[[0, 2]] == 7.0).all())


def test_bench_serve_workload_is_seeded_and_in_range():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("bench_serve", os.path.join(os.path.dirname(__file__), "..", "tools", "bench_serve.py"))
    bs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bs)
    reqs, again = bs.workload(64, seed=0), bs.workload(64, seed=0)
    assert len(reqs) == 64 and all(torch.equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(reqs, again))
    assert all(16 <= p.numel() <= 128 and 16 <= n <= 256 and p.dtype == torch.long and int(p.max()) < 50280 for p, n in reqs)
    assert len({p.numel() for p, _ in reqs}) > 8 and len({n for _, n in reqs}) > 8              # ragged
    batches = bs.static_batches(reqs, 16)
    assert len(batches) == 4
    for k, (ids, seq, max_length) in enumerate(batches):
        part = reqs[16 * k:16 * k + 16]
        L = max(p.numel() for p, _ in part)
        assert ids.shape == seq.shape == (16, L) and seq.dtype == torch.int32 and max_length == L + max(n for _, n in part)
        for row, (p, _) in enumerate(part):
            pad = L - p.numel()
            assert torch.equal(ids[row, pad:], p) and not ids[row, :pad].any()
            assert bool((seq[row, pad:] == seq[row, -1]).all()) and (pad == 0 or bool((seq[row, :pad] != seq[row, -1]).all()))


# ---- DecodeEngine: the scheduler alone ---------------------------------------------------------------------------------------------------------------------
REQUESTS = [(5, 6), (3, 2), (7, 9), (4, 1), (6, 4), (3, 7)]                   # (prompt tokens, new tokens)


def _prompts():
    g = torch.Generator().manual_seed(11)
    return [torch.randint(0, 90, (n,), generator=g) for n, _ in REQUESTS]


def _alone(m, prompt, new):
    out = m.generate(prompt.unsqueeze(0), max_length=prompt.numel() + new, vocab_size=90, return_dict_in_generate=True, output_scores=True)
    return out.sequences[0], torch.stack(out.scores, 0)[:, 0]


@pytest.mark.parametrize("fused", ["1", "0"], ids=["fused", "unfused"])
def test_engine_schedules_slots_and_reproduces_every_request_alone(fused, slots_backend, monkeypatch):
    from dimsum_amd.utils.serving import DecodeEngine
    monkeypatch.setenv("DIMSUM_FUSED_DECODE", fused)
    m = tiny_model(1, 1)
    prompts = _prompts()
    alone = [_alone(m, p, n) for p, (_, n) in zip(prompts, REQUESTS)]
    gaps = torch.cat([s.topk(2, dim=-1).values for _, s in alone])
    assert float((gaps[:, 0] - gaps[:, 1]).min()) > 1e-4                         # no near-tie that a batched product could flip
    eng = DecodeEngine(m, max_batch=2, num_slots=3, max_seqlen=32, vocab_size=90, cg=False, fused_sampling=False)
    rids = [eng.submit(p, n) for p, (_, n) in zip(prompts, REQUESTS)]
    assert rids == list(range(6)) and len(eng.queue) == 6 and eng.free_slots == [0, 1, 2]       # submit only queues
    admitted_at, finished_at, step = {}, {}, 0
    while not eng.idle():
        events = eng.step()
        for rid, slot in eng.slot_history:
            admitted_at.setdefault(rid, step)
        for rid, token, fin in events:
            assert 0 <= token < 90
            if fin:
                finished_at[rid] = step
        held = [eng.requests[rid].slot for rid in eng.rows if rid is not None]
        assert len(set(held)) == len(held) and all(0 <= s < 3 for s in held)                    # no slot held twice
        assert sorted(held + eng.free_slots) == [0, 1, 2]                                       # handed out or free, never lost
        assert eng.slots.tolist() == [-1 if rid is None else eng.requests[rid].slot for rid in eng.rows]
        step += 1
        assert step < 100
    assert eng.free_slots and sorted(eng.free_slots) == [0, 1, 2] and eng.rows == [None, None]
    for rid, (seq, _) in zip(rids, alone):
        assert torch.equal(eng.sequence(rid), seq), rid                                         # max_new_tokens honoured, tokens equal
    assert eng.run().keys() == set(rids)
    # requests 0 and 1 start at once; 2 waits for a row and enters the step after the first of them has finished
    assert admitted_at[0] == admitted_at[1] == 0 and admitted_at[2] == min(finished_at[0], finished_at[1]) + 1
    assert admitted_at[3] >= admitted_at[2]                                                     # first come, first served
    reused = [slot for _, slot in eng.slot_history]
    assert len(reused) == 6 and len(set(reused)) == 3                                           # released slots were handed out again


def test_engine_stops_a_request_at_eos(slots_backend, monkeypatch):
    from dimsum_amd.utils.serving import DecodeEngine
    monkeypatch.setenv("DIMSUM_FUSED_DECODE", "1")
    m = tiny_model(1, 1)
    prompts = _prompts()
    alone = [_alone(m, p, n)[0][p.numel():].tolist() for p, (_, n) in zip(prompts, REQUESTS)]
    eos = alone[2][3]                                                                           # the fourth new token of request 2
    eng = DecodeEngine(m, max_batch=4, max_seqlen=32, vocab_size=90, eos_token_id=eos, cg=False, fused_sampling=False)
    rids = [eng.submit(p, n) for p, (_, n) in zip(prompts, REQUESTS)]
    out = eng.run()
    for rid, p, new in zip(rids, prompts, alone):
        want = new[:new.index(eos) + 1] if eos in new else new
        assert out[rid].tolist() == p.tolist() + want, rid
    assert len(out[rids[2]]) <= prompts[2].numel() + 4


def test_engine_refuses_what_it_cannot_schedule(slots_backend):
    from dimsum_amd.utils.serving import DecodeEngine
    m = tiny_model(1, 1)
    with pytest.raises(ValueError, match="num_slots >= max_batch"):
        DecodeEngine(m, max_batch=4, num_slots=3, max_seqlen=8, cg=False, fused_sampling=False)
    eng = DecodeEngine(m, max_batch=2, max_seqlen=8, cg=False, fused_sampling=False)
    with pytest.raises(ValueError, match="1-D"):
        eng.submit(torch.zeros(2, 3, dtype=torch.long), 4)
    with pytest.raises(ValueError, match="uniforms pin the draws of the fused sampler"):
        eng.submit(torch.zeros(3, dtype=torch.long), 4, uniforms=torch.zeros(4))
    fused = DecodeEngine(m, max_batch=2, max_seqlen=8, cg=False, fused_sampling=True)
    with pytest.raises(ValueError, match="uniforms must be"):
        fused.submit(torch.zeros(3, dtype=torch.long), 4, uniforms=torch.zeros(3))
    assert eng.step() == [] and eng.idle()
