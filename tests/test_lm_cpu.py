"""The language model without a GPU: Block / MixerModel / MambaLMHeadModel and generate() against the reference fixtures lm_tiny_*.npz on the
CPU oracle backend, with the native entry points of the decode step replaced by plain-torch restatements (as test_mixer_step_cpu.py does; the
restatement of native.decode_linear is `decode_linear_torch` below, which the GPU tests reuse in float64); the sampling helpers against
hand-computed rows; checkpoint directories; the C ABI checks of dimsum_decode_linear in their documented order, nothing launched.
Bound on logits: the fp32 one of the reference's own tests, rtol 3e-4, atol 1e-3 (test_mixer_step_cpu.py)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden
from oracle.torch_backend import cpu_oracle_backend
from test_host_logic import _header_layout
from test_mixer_step_cpu import close, native_conv_update, native_state_update

T = torch.from_numpy
LM_TINY = dict(d_model=64, n_layer=2, vocab_size=90, pad_vocab_size_multiple=8, ssm_cfg=dict(d_state=16, d_conv=4, expand=2))
VARIANTS = [(r, f) for r in (0, 1) for f in (0, 1)]
PROMPT, STEPS = 9, 7


def decode_linear_torch(x, weight, bias=None, norm=None, residual=None, residual_out=None, conv=None):
    """native.decode_linear restated in torch, in the arithmetic of its operands' dtype promoted to at least float32 (float64 operands make it
    the GPU tests' yardstick): same signature, same in-place conv state update, same returns"""
    wide = torch.float64 if x.dtype == torch.float64 else torch.float32
    res_out = None
    xp = x.to(wide)
    if norm is not None:
        nw, nb, eps, is_rms = norm
        r = xp if residual is None else xp + residual.to(wide)
        if residual_out is not None:
            res_out = r.to(residual_out)
        if is_rms:
            xp = r * torch.rsqrt(r.pow(2).mean(-1, keepdim=True) + eps) * nw.to(wide)
        else:
            xp = (r - r.mean(-1, keepdim=True)) * torch.rsqrt(r.var(-1, unbiased=False, keepdim=True) + eps) * nw.to(wide)
        if nb is not None:
            xp = xp + nb.to(wide)
        xp = xp.to(x.dtype).to(wide)                        # the kernel hands x' to the product rounded to T
    y = xp @ weight.to(wide).t()
    if bias is not None:
        y = y + bias.to(wide)
    if conv is not None:
        state, cw, cb, silu = conv
        D = cw.shape[0]
        state.copy_(torch.cat([state[:, :, 1:], y[:, :D].to(state.dtype).unsqueeze(-1)], dim=-1))
        out = (state.to(wide) * cw.to(wide)).sum(-1)
        if cb is not None:
            out = out + cb.to(wide)
        y = torch.cat([F.silu(out) if silu else out, y[:, D:]], dim=1)
    y = y.to(x.dtype)
    return y if residual_out is None else (y, res_out)


@pytest.fixture
def lm_backend(monkeypatch):
    from dimsum_amd import native
    monkeypatch.setattr(native, "causal_conv1d_update", native_conv_update)
    monkeypatch.setattr(native, "selective_state_update", native_state_update)
    monkeypatch.setattr(native, "decode_linear", decode_linear_torch)
    with cpu_oracle_backend():
        yield


def tiny_model(rms, fp32res, g=None, **over):
    from dimsum_amd.models.mixer_seq_simple import MambaLMHeadModel
    kw = dict(LM_TINY, rms_norm=bool(rms), residual_in_fp32=bool(fp32res), fused_add_norm=True)
    kw.update(over)
    m = MambaLMHeadModel(**kw).eval()
    if g is not None:
        m.load_state_dict({k[2:]: T(g[k]) for k in g.files if k.startswith("w.")})
    return m


def run_cached(m, prompt, steps, teacher=None):
    """the prompt's logits, then `steps` greedy cached steps -> (prompt_logits (B, L, V), step_logits (B, steps, V), ids (B, steps + 1));
    teacher (B, steps + 1): the tokens fed to the steps instead of the argmaxes (which are still returned)"""
    from dimsum_amd.utils import InferenceParams
    p = InferenceParams(max_seqlen=prompt.shape[1] + steps, max_batch_size=prompt.shape[0])
    with torch.no_grad():
        pl = m(prompt, inference_params=p).logits
        p.seqlen_offset = prompt.shape[1]
        tok = pl[:, -1].argmax(-1, keepdim=True)
        ids, outs = [tok], []
        for _ in range(steps):
            feed = tok if teacher is None else teacher[:, len(outs):len(outs) + 1]
            logits = m(feed, inference_params=p, num_last_tokens=1).logits[:, 0]
            p.seqlen_offset += 1
            outs.append(logits)
            tok = logits.argmax(-1, keepdim=True)
            ids.append(tok)
    return pl, torch.stack(outs, 1), torch.cat(ids, 1)


# ---- the model -------------------------------------------------------------------------------------------------------------------------------------
def test_state_dict_keys_equal_the_reference():
    doc = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "lm_keys.json")))
    for rms, name in ((0, "layer_norm"), (1, "rms_norm")):
        got = [[k, list(v.shape)] for k, v in tiny_model(rms, 0).state_dict().items()]
        assert got == doc[name], name
    m = tiny_model(1, 1)
    assert m.lm_head.weight is m.backbone.embedding.weight and m.lm_head.weight.shape == (96, 64)        # tied, vocab padded to a multiple of 8
    assert tiny_model(1, 1, pad_vocab_size_multiple=1).lm_head.weight.shape == (90, 64)


@pytest.mark.parametrize("fused", ["1", "0"], ids=["fused", "unfused"])
@pytest.mark.parametrize("rms,fp32res", VARIANTS)
def test_prompt_logits_and_cached_steps_match_the_fixtures(rms, fp32res, fused, lm_backend, monkeypatch):
    monkeypatch.setenv("DIMSUM_FUSED_DECODE", fused)
    g = golden(f"lm_tiny_rms{rms}_fp32res{fp32res}")
    m = tiny_model(rms, fp32res, g)
    calls = []
    from dimsum_amd import native
    monkeypatch.setattr(native, "decode_linear", lambda *a, **k: calls.append(1) or decode_linear_torch(*a, **k))
    pl, sl, ids = run_cached(m, T(g["prompt"]), STEPS)
    close(pl, g["prompt_logits"], "prompt logits")
    close(sl, g["step_logits"], "step logits")
    err = max(np.abs(pl.numpy() - g["prompt_logits"]).max(), np.abs(sl.numpy() - g["step_logits"]).max())
    assert err < float(g["min_gap"]) / 4, (err, float(g["min_gap"]))
    assert np.array_equal(ids.numpy(), g["ids"])
    assert len(calls) == (STEPS * (3 * 2 + 1) if fused == "1" else 0)          # 3 per layer + the head, or none at all
    with torch.no_grad():
        close(m(T(g["prompt"])).logits, g["prompt_logits"], "one forward, no cache")
        last2 = m(T(g["prompt"]), num_last_tokens=2).logits
    assert last2.shape == (2, 2, 96)
    close(last2, g["prompt_logits"][:, -2:], "num_last_tokens")


def test_block_returns_the_pair_with_the_residual_dtype(lm_backend):
    from dimsum_amd.models.mixer_seq_simple import create_block
    x = torch.randn(2, 5, 64, generator=torch.Generator().manual_seed(0))
    for fused_add_norm in (True, False):
        for rms in (True, False):
            blk = create_block(64, ssm_cfg=LM_TINY["ssm_cfg"], rms_norm=rms, residual_in_fp32=True, fused_add_norm=fused_add_norm, layer_idx=0).eval()
            assert blk.layer_idx == 0
            with torch.no_grad():
                h, r = blk(x)
                assert h.shape == r.shape == x.shape and r.dtype == torch.float32 and torch.equal(r, x)
                h2, r2 = blk(h, r)
            assert torch.allclose(r2, h + r) and h2.shape == x.shape
    half = create_block(64, ssm_cfg=LM_TINY["ssm_cfg"], rms_norm=True, residual_in_fp32=True, fused_add_norm=False, layer_idx=0)
    assert half.allocate_inference_cache(3, 8)[0].shape == (3, 128, 4)
    # residual_in_fp32 next to 16-bit activations: the residual stream is float32 (the unfused-norm branch runs on plain torch modules)
    ln = create_block(64, ssm_cfg=LM_TINY["ssm_cfg"], rms_norm=False, residual_in_fp32=True, fused_add_norm=False, layer_idx=0).eval()
    ln.mixer = torch.nn.Identity()
    ln.mixer.forward = lambda h, inference_params=None: h
    with torch.no_grad():
        h, r = ln.to(torch.bfloat16)(x.to(torch.bfloat16))
    assert h.dtype == torch.bfloat16 and r.dtype == torch.float32


def test_checkpoint_directory_round_trip(tmp_path, lm_backend):
    from dimsum_amd.models.mixer_seq_simple import MambaLMHeadModel
    g = golden("lm_tiny_rms1_fp32res1")
    m = tiny_model(1, 1, g)
    m.save_pretrained(tmp_path / "ckpt")
    assert sorted(os.listdir(tmp_path / "ckpt")) == ["config.json", "pytorch_model.bin"]
    cfg = json.load(open(tmp_path / "ckpt" / "config.json"))
    assert cfg["vocab_size"] == 90 and cfg["pad_vocab_size_multiple"] == 8 and cfg["rms_norm"] is True
    m2 = MambaLMHeadModel.from_pretrained(tmp_path / "ckpt").eval()
    assert m2.lm_head.weight is m2.backbone.embedding.weight
    for (k, a), (k2, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert k == k2 and torch.equal(a, b), k
    with torch.no_grad():
        assert torch.equal(m2(T(g["prompt"])).logits, m(T(g["prompt"])).logits)
    assert MambaLMHeadModel.from_pretrained(str(tmp_path / "ckpt"), dtype=torch.bfloat16).lm_head.weight.dtype == torch.bfloat16
    for bad in (tmp_path / "nope", tmp_path / "ckpt" / "config.json", "state-spaces/mamba-130m"):
        with pytest.raises(FileNotFoundError, match="not an existing directory"):
            MambaLMHeadModel.from_pretrained(bad)


def test_the_package_does_not_import_transformers():
    import subprocess
    import sys
    code = ("import sys; import dimsum_amd.models.mixer_seq_simple, dimsum_amd.utils.generation; "
            "assert not [m for m in sys.modules if m.split('.')[0] in ('transformers', 'huggingface_hub')]")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=root)


# ---- sampling --------------------------------------------------------------------------------------------------------------------------------------
def test_top_k_and_top_p_filters_against_hand_computed_rows():
    from dimsum_amd.utils.generation import modify_logits_for_top_k_filtering, modify_logits_for_top_p_filtering
    inf = float("inf")
    logits = torch.tensor([[1.0, 3.0, 2.0, 0.0], [0.5, 0.5, -1.0, 4.0]])
    a = logits.clone()
    modify_logits_for_top_k_filtering(a, 2)
    assert a.tolist() == [[-inf, 3.0, 2.0, -inf], [0.5, 0.5, -inf, 4.0]]        # ties with the k-th largest stay
    # probabilities 0.1, 0.2, 0.3, 0.4: ascending cumulative sums 0.1, 0.3, 0.6, 1.0; top_p 0.65 removes those <= 0.35
    b = torch.log(torch.tensor([[0.2, 0.4, 0.1, 0.3]]))
    modify_logits_for_top_p_filtering(b, 0.65)
    assert torch.isinf(b[0]).tolist() == [True, False, True, False]
    c = torch.log(torch.tensor([[0.2, 0.4, 0.1, 0.3]]))
    modify_logits_for_top_p_filtering(c, 0.95)                                 # removes those <= 0.05: nothing
    assert not torch.isinf(c).any()
    for p in (0.0, 1.0):
        d = logits.clone()
        modify_logits_for_top_p_filtering(d, p)
        assert torch.equal(d, logits)


def test_sample():
    from dimsum_amd.utils.generation import sample
    logits = torch.randn(5, 33, generator=torch.Generator().manual_seed(3))
    assert torch.equal(sample(logits, top_k=1), logits.argmax(-1))
    top3 = logits.topk(3).indices
    gen = torch.Generator().manual_seed(5)
    seen = set()
    for _ in range(40):
        tok = sample(logits.clone(), top_k=3, temperature=2.0, generator=gen)
        assert bool((tok.unsqueeze(1) == top3).any(1).all())
        seen.update(zip(range(5), tok.tolist()))
    assert len(seen) > 5                                                       # not the argmax alone
    a = sample(logits.clone(), top_k=3, generator=torch.Generator().manual_seed(9))
    assert torch.equal(a, sample(logits.clone(), top_k=3, generator=torch.Generator().manual_seed(9)))
    # top_k 0 with a top_p that keeps the two likeliest tokens of a peaked row
    peaked = torch.log(torch.tensor([[0.05, 0.5, 0.05, 0.4]])).repeat(64, 1)
    tok = sample(peaked, top_k=0, top_p=0.85, generator=torch.Generator().manual_seed(1))
    assert set(tok.tolist()) == {1, 3}
    with pytest.raises(AssertionError, match="top-p"):
        sample(logits, top_k=3, top_p=1.5)


def test_generate_stops_at_max_length_and_at_eos(lm_backend):
    from dimsum_amd.utils.generation import GenerationOutput
    g = golden("lm_tiny_rms1_fp32res1")
    m = tiny_model(1, 1, g)
    prompt = T(g["prompt"])
    out = m.generate(prompt, max_length=PROMPT + STEPS + 1, return_dict_in_generate=True, output_scores=True)
    assert isinstance(out, GenerationOutput) and out.sequences.shape == (2, PROMPT + STEPS + 1) and len(out.scores) == STEPS + 1
    assert torch.equal(out.sequences[:, :PROMPT], prompt) and np.array_equal(out.sequences[:, PROMPT:].numpy(), g["ids"])
    close(torch.stack(out.scores[1:], 1), g["step_logits"], "scores")
    seq = m.generate(prompt, max_length=PROMPT + 3)
    assert isinstance(seq, torch.Tensor) and torch.equal(seq, out.sequences[:, :PROMPT + 3])
    assert m.generate(prompt, max_length=PROMPT + 3, return_dict_in_generate=True).scores is None
    # a teacher that makes every row emit token 7 as the third new token: generation ends there
    teacher = out.sequences.clone()
    teacher[:, PROMPT + 2] = 7
    stopped = m.generate(prompt, max_length=PROMPT + STEPS + 1, eos_token_id=7, teacher_outputs=teacher)
    assert stopped.shape == (2, PROMPT + 3) and bool((stopped[:, -1] == 7).all())
    one_row = teacher.clone()
    one_row[1, PROMPT + 2] = 8                                                 # only one row at eos: no stop
    assert m.generate(prompt, max_length=PROMPT + 5, eos_token_id=7, teacher_outputs=one_row).shape == (2, PROMPT + 5)


# ---- the restatement and the wrapper ---------------------------------------------------------------------------------------------------------------
def test_restatement_is_the_unfused_chain():
    """decode_linear_torch == add -> norm -> F.linear -> causal_conv1d_update_torch on the CPU, for both norms"""
    from dimsum_amd.ops import causal_conv1d_update_torch
    gen = torch.Generator().manual_seed(0)
    x, res, w, b = (torch.randn(*s, generator=gen) for s in ((3, 64), (3, 64), (256, 64), (256,)))
    nw, nb, cw, cb, st = (torch.randn(*s, generator=gen) for s in ((64,), (64,), (128, 4), (128,), (3, 128, 4)))
    for rms in (True, False):
        s1, s2 = st.clone(), st.clone()
        y, ro = decode_linear_torch(x, w, b, norm=(nw, None if rms else nb, 1e-5, rms), residual=res, residual_out=torch.float32, conv=(s1, cw, cb, True))
        r = x + res
        h = r * torch.rsqrt(r.pow(2).mean(-1, keepdim=True) + 1e-5) * nw if rms else F.layer_norm(r, (64,), nw, nb, 1e-5)
        xz = F.linear(h, w, b)
        want = torch.cat([causal_conv1d_update_torch(xz[:, :128], s2, cw, cb, "silu"), xz[:, 128:]], 1)
        assert torch.equal(ro, r) and torch.equal(s1[:, :, :-1], s2[:, :, :-1]) and torch.allclose(s1, s2, rtol=1e-5, atol=1e-5)
        assert torch.allclose(y, want, rtol=1e-5, atol=1e-5)


def test_wrapper_refuses_clearly():
    from dimsum_amd import native
    x, w = torch.zeros(2, 8), torch.zeros(5, 8)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        native.decode_linear(x, w)
    with pytest.raises(RuntimeError, match="batch must be 1..16"):
        native.decode_linear(torch.zeros(17, 8), w)
    with pytest.raises(RuntimeError, match="of x's dtype"):
        native.decode_linear(x, w.half())
    with pytest.raises(RuntimeError, match="norm prologue"):
        native.decode_linear(x, w, residual=x)
    with pytest.raises(RuntimeError, match="width between 2 and 4"):
        native.decode_linear(x, w, conv=(torch.zeros(2, 4, 5), torch.zeros(4, 5), None, True))
    assert native.decode_linear_serves(x, w, None, w) and not native.decode_linear_serves(torch.zeros(17, 8), w)
    assert not native.decode_linear_serves(x, w, w.half()) and not native.decode_linear_serves(x.double(), w.double())


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------------------------
def test_struct_layout_and_export():
    from dimsum_amd import _lib
    layout = _header_layout([("dimsum_decode_linear_params_t", _lib.DecodeLinearParams)])
    size, offs = layout["dimsum_decode_linear_params_t"]
    assert size == ctypes.sizeof(_lib.DecodeLinearParams) == _lib.DecodeLinearParams().struct_size
    assert offs == {f: getattr(_lib.DecodeLinearParams, f).offset for f, _ in _lib.DecodeLinearParams._fields_}
    lib = _lib.load()
    assert lib.dimsum_abi_version() == 18                                      # new symbols only: the ABI number stands
    header = open(os.path.join(_lib._HERE, "..", "include", "dimsum_hip.h")).read()
    assert "dimsum_decode_linear" in _lib.EXPORTS and hasattr(lib, "dimsum_decode_linear") and "int dimsum_decode_linear(" in header
    assert "DIMSUM_ERR_ALIAS = 8" in header and b"overlaps" in lib.dimsum_status_string(8)


def test_library_checks_in_their_documented_order():
    """every pointer set to host memory that is never dereferenced: the checks run on the host and return before a launch. Each call breaks
    one rule AND every later one's, so the code that comes back names the first check that fails"""
    from dimsum_amd import _lib
    lib = _lib.load()
    fn = lib.dimsum_decode_linear
    NULL, DTYPE, SHAPE, STRIDE, UNSUPPORTED, ABI, ALIAS = 1, 2, 3, 4, 5, 7, 8
    buf = (ctypes.c_float * 4096)()
    addr = ctypes.addressof(buf)
    assert fn(None, None) == NULL
    P = _lib.DecodeLinearParams()
    P.struct_size -= 8
    assert fn(P, None) == ABI                                                  # before anything else is read
    P = _lib.DecodeLinearParams()
    P.batch, P.dtype, P.x_row_stride = 17, 3, -1                               # wrong in every later way
    assert fn(P, None) == NULL                                                 # x, W, y
    P.x_ptr = P.w_ptr = addr
    assert fn(P, None) == NULL
    P.y_ptr = addr + 8192
    P.norm = 2
    assert fn(P, None) == NULL                                                 # norm without its weight
    P.norm_weight_ptr = addr
    P.conv_dim = 1
    assert fn(P, None) == NULL                                                 # conv without weight / state
    P.conv_weight_ptr = P.conv_state_ptr = addr
    for batch, n, k in ((0, 4, 4), (17, 4, 4), (-1, 4, 4), (1, 0, 4), (1, 4, 0)):
        P.batch, P.n, P.k = batch, n, k
        assert fn(P, None) == SHAPE, (batch, n, k)
    P.batch, P.n, P.k = 2, 4, 8
    for width in (1, 5):
        P.conv_width = width
        assert fn(P, None) == SHAPE, width
    P.conv_width, P.conv_dim = 4, 5
    assert fn(P, None) == SHAPE                                                # conv_dim > n
    P.conv_dim, P.norm = 4, 3
    assert fn(P, None) == SHAPE
    P.norm = 2
    assert fn(P, None) == DTYPE                                                # dtype 3
    P.dtype, P.residual_dtype = 1, 2
    assert fn(P, None) == DTYPE                                                # a residual neither float32 nor of the dtype
    P.dtype, P.residual_dtype = 0, 0
    assert fn(P, None) == STRIDE                                               # x_row_stride -1
    P.x_row_stride = 8
    for f in ("w_row_stride", "y_row_stride", "state_batch_stride", "state_c_stride", "state_w_stride", "conv_weight_c_stride",
              "conv_weight_width_stride"):
        setattr(P, f, -1)
        assert fn(P, None) == STRIDE, f
        setattr(P, f, 8)
    P.residual_ptr, P.residual_row_stride = addr + 4096, -8
    assert fn(P, None) == STRIDE
    P.residual_row_stride = 8
    # residual_out over x (batch 2, k 8, row stride 8: 64 bytes from addr + 1024) and over residual (64 bytes from addr + 4096), by one
    # element at either end or wholly
    P.x_ptr, P.residual_out_row_stride = addr + 1024, 8
    for base in (1024, 4096):
        for off in (0, 60, -60):
            P.residual_out_ptr = addr + base + off
            assert fn(P, None) == ALIAS, (base, off)
    P.norm, P.residual_out_ptr = 0, addr + 2048
    assert fn(P, None) == UNSUPPORTED                                          # residual pointers without the prologue
    Q = _lib.DecodeLinearParams()                                              # a 16-bit x overlapped by a float32 residual_out
    Q.batch, Q.n, Q.k, Q.dtype, Q.residual_dtype, Q.norm = 1, 1, 8, 2, 0, 2
    Q.x_ptr, Q.w_ptr, Q.y_ptr, Q.norm_weight_ptr = addr + 16, addr + 4096, addr + 8192, addr + 4096
    Q.residual_out_ptr = addr                                                  # 32 bytes of float32 reach the 16 bytes of x at addr + 16
    assert fn(Q, None) == ALIAS
