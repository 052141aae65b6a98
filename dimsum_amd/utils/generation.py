"""Token generation on the recurrent form -- `sample`, `decode`, `GenerationMixin.generate` and graph-captured decoding with the call signatures
of mamba/mamba_ssm/utils/generation.py, minus `transformers`: `generate(return_dict_in_generate=True)` returns this module's GenerationOutput
(`sequences`, `scores`) where the reference returns a transformers output class.

cg=True: one decode step (the model's forward on a (batch, 1) token buffer at seqlen_offset > 0) is captured per batch size into a hipGraph,
on the capture's single stream -- the step has no parallel branches -- after warm-up runs on a side stream, and replayed from static buffers;
sampling stays outside the graph unless fused sampling is asked for (`fused_sampling=` / DIMSUM_FUSED_SAMPLING=1, off by default): the sampler
is then ONE launch of csrc/sample_logits.hip per token on a table of uniforms drawn once per call, and under cg=True it is part of the
captured step, which writes the token straight into its own input buffer: a token is one graph replay. The cache (states, graphs) hangs on the model as `_decoding_cache` and is reused by later calls that fit it.
`decode` and the capture run under torch.no_grad(), not the reference's inference_mode: a capture begun in inference mode makes the generator's
graph-safe state inference tensors, and every later capture of the process outside inference mode then fails on their in-place update."""
import dataclasses
import gc
import os
from typing import Callable, Optional

import torch

from . import InferenceParams
from .. import native


@dataclasses.dataclass
class GenerationOutput:
    """sequences (batch, length) incl. the prompt; scores: a tuple of the (batch, vocab) logits each new token was chosen from, or None"""
    sequences: torch.Tensor
    scores: Optional[tuple] = None


def modify_logits_for_top_k_filtering(logits, top_k):
    """every logit below the row's top_k-th largest <- -inf, in place"""
    indices_to_remove = logits < torch.topk(logits, top_k)[0][..., -1, None]
    logits.masked_fill_(indices_to_remove, float("-inf"))


def modify_logits_for_top_p_filtering(logits, top_p):
    """the low-probability tail whose cumulative probability stays within 1 - top_p <- -inf, in place; top_p outside (0, 1) keeps everything"""
    if top_p <= 0.0 or top_p >= 1.0:
        return
    sorted_logits, sorted_indices = torch.sort(logits, descending=False)
    cumulative_probs = sorted_logits.softmax(dim=-1).cumsum(dim=-1)
    sorted_remove = cumulative_probs <= (1 - top_p)
    logits.masked_fill_(sorted_remove.scatter(1, sorted_indices, sorted_remove), float("-inf"))


def sample(logits, top_k=1, top_p=0.0, temperature=1.0, generator=None):
    """logits (batch, vocab) -> token ids (batch,). top_k == 1: argmax. top_k > 1: among the k largest (then top_p inside them); top_k == 0: over
    the whole vocabulary (top_p if set). `generator` (no reference counterpart) seeds the multinomial draw."""
    if top_k == 1:
        return logits.argmax(dim=-1)
    if top_p > 0.0:
        assert top_p <= 1.0, "top-p should be in (0, 1]."
    if top_k > 0:
        top_k = min(top_k, logits.size(-1))
        logits_top, indices = torch.topk(logits, top_k, dim=-1)
        if temperature != 1.0:
            logits_top /= temperature
        modify_logits_for_top_p_filtering(logits_top, top_p)
        pick = torch.multinomial(torch.softmax(logits_top, dim=-1), num_samples=1, generator=generator).squeeze(dim=-1)
        return indices[torch.arange(indices.shape[0], device=indices.device), pick]
    logits_top = logits / temperature if temperature != 1.0 else logits.clone()
    modify_logits_for_top_p_filtering(logits_top, top_p)
    return torch.multinomial(torch.softmax(logits_top, dim=-1), num_samples=1, generator=generator).squeeze(dim=-1)


def sample_fused(logits, u, top_k=1, top_p=0.0, temperature=1.0):
    """`sample` in one launch of csrc/sample_logits.hip: logits (batch, vocab) -> token ids (batch,), with the argument meanings of `sample`
    and u (batch,) float32 uniforms in [0, 1) in the place of `generator`: the token is a pure function of (logits, top_k, top_p, temperature,
    u). Same distribution as `sample`; equal logits rank by ascending index (include/dimsum_hip.h, dimsum_sample_logits)."""
    return native.sample_logits(logits, u, top_k=top_k, top_p=top_p, temperature=temperature)


def fused_sampling_enabled(fused_sampling=None):
    """the argument when given; else DIMSUM_FUSED_SAMPLING, read at call time: 1 = on, anything else (and unset) = off"""
    if fused_sampling is not None:
        return bool(fused_sampling)
    return os.environ.get("DIMSUM_FUSED_SAMPLING", "") == "1"


def _decode_fused(input_ids, model, max_length, top_k, top_p, temperature, eos_token_id, vocab_size, cg, generator, uniforms, output_scores,
                  seq_idx=None):
    """`decode` on the fused sampler. uniforms (max_length, batch): row i draws the i-th new token. Eager: one sample_logits launch per token
    on the step's row. cg: the captured step samples from its own logits into its own input buffer and files the token in the cache's token
    table at the cache's step counter; the host only replays (and reads the newest token when it has to look for eos_token_id)."""
    batch_size, seqlen_og = input_ids.shape
    device = input_ids.device
    if uniforms is None:
        uniforms = torch.rand((max_length, batch_size), device=device, dtype=torch.float32, generator=generator)
    elif tuple(uniforms.shape) != (max_length, batch_size) or uniforms.dtype != torch.float32:
        raise ValueError(f"decode: uniforms must be (max_length, batch) = ({max_length}, {batch_size}) float32, got {tuple(uniforms.shape)} {uniforms.dtype}")
    kw = dict(top_k=top_k, top_p=top_p, temperature=temperature)
    if cg:
        sampling = (int(top_k), float(top_p), float(temperature), vocab_size)
        cache = model._decoding_cache = update_graph_cache(model, getattr(model, "_decoding_cache", None), batch_size, seqlen_og, max_length,
                                                           sampling=sampling)
        inference_params = cache.params_for(batch_size)
        inference_params.reset(max_length, batch_size)
        step = cache.callables[(batch_size, 1) + sampling]
        table, counter, tokens = cache.sampling_buffers(batch_size)
        table[:max_length].copy_(uniforms)
        counter.zero_()
        tokens.zero_()
    else:
        inference_params = InferenceParams(max_seqlen=max_length, max_batch_size=batch_size)
        table = uniforms.to(device).contiguous()
        tokens = torch.zeros((max_length, batch_size), dtype=torch.long, device=device)
    scores, n = [], 0
    while True:
        if n == 0:
            logits = model(input_ids, inference_params=inference_params, num_last_tokens=1, **_prompt_kw(seq_idx)).logits[:, -1]
        elif cg:
            logits = step()[:, -1]                          # forward, sample, count: tokens[n] and the next input are in place
        else:
            logits = model(tokens[n - 1].unsqueeze(1), inference_params=inference_params, num_last_tokens=1).logits[:, -1]
        inference_params.seqlen_offset += seqlen_og if n == 0 else 1
        view = logits[..., :vocab_size] if vocab_size is not None else logits     # a view: the row stride limits the classes
        if output_scores:
            scores.append(view.clone() if cg and n > 0 else view)                 # the graph's logits are a static buffer
        if cg and n == 0:
            native.sample_logits(view, table, out=step.input_ids, row_index=counter, out_table=tokens, **kw)
            counter.add_(1)
        elif not cg:
            native.sample_logits(view, table[n], out=tokens[n], **kw)
        n += 1
        if eos_token_id is not None and bool((tokens[n - 1] == eos_token_id).all()):
            break
        if inference_params.seqlen_offset >= max_length - 1:
            break
    return GenerationOutput(sequences=torch.cat([input_ids, tokens[:n].t()], dim=1), scores=tuple(scores))


def _prompt_kw(seq_idx):
    """what the prompt forward gets beyond the usual: the sequence ids of a packed / left-padded prompt, when there are any"""
    return {} if seq_idx is None else {"seq_idx": seq_idx}


@torch.no_grad()
def decode(input_ids, model, max_length, top_k=1, top_p=0.0, temperature=1.0, eos_token_id=None, teacher_outputs=None, vocab_size=None, cg=False,
           enable_timing=False, generator=None, fused_sampling=None, uniforms=None, output_scores=True, seq_idx=None):
    """greedy / top-k / top-p decoding of input_ids (batch, seqlen), all rows of one length, up to max_length tokens in all; stops early once
    every row's newest token is eos_token_id. teacher_outputs (batch, seqlen'): tokens taken instead of sampled ones (testing).
    fused_sampling (None: DIMSUM_FUSED_SAMPLING, off when unset): sample with `sample_fused` on a (max_length, batch) float32 table of
    uniforms -- `uniforms`, or one torch.rand(generator=generator) draw per call -- whose row i draws the i-th new token; with cg=True the
    sampler is part of the captured step. teacher_outputs keeps the unfused sampler. output_scores=False lets the fused path skip the
    per-token copy of the logits.
    seq_idx (batch, seqlen) int32: sequence ids of the prompt, handed to the prompt forward only -- rows of different lengths are left-padded
    to one length with the padding as a segment of its own (dimsum_amd.utils.seq_idx_from_lengths([pad, n])), and every row then prefills and
    decodes as if it stood alone. The decode steps continue every row's last segment and take no ids.
    -> GenerationOutput(sequences (batch, <= max_length), scores: one (batch, vocab) per generated token)"""
    if teacher_outputs is None and fused_sampling_enabled(fused_sampling):
        if enable_timing:
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
        out = _decode_fused(input_ids, model, max_length, top_k, top_p, temperature, eos_token_id, vocab_size, cg, generator, uniforms, output_scores,
                            seq_idx=seq_idx)
        if enable_timing:
            end.record()
            torch.cuda.synchronize()
            print(f"Prompt processing + decoding time: {start.elapsed_time(end):.0f}ms")
        return out
    batch_size, seqlen_og = input_ids.shape
    teacher_output_len = teacher_outputs.shape[1] if teacher_outputs is not None else 0
    if cg:
        if not hasattr(model, "_decoding_cache"):
            model._decoding_cache = None
        model._decoding_cache = update_graph_cache(model, model._decoding_cache, batch_size, seqlen_og, max_length)
        inference_params = model._decoding_cache.params_for(batch_size)
        inference_params.reset(max_length, batch_size)
    else:
        inference_params = InferenceParams(max_seqlen=max_length, max_batch_size=batch_size)

    def get_logits(ids):
        decoding = inference_params.seqlen_offset > 0
        if not cg or not decoding:
            logits = model(ids, inference_params=inference_params, num_last_tokens=1, **({} if decoding else _prompt_kw(seq_idx))).logits.squeeze(dim=1)
        else:
            logits = model._decoding_cache.run(ids, inference_params.seqlen_offset).squeeze(dim=1)
        return logits[..., :vocab_size] if vocab_size is not None else logits

    def sample_tokens(logits):
        if teacher_outputs is None or teacher_output_len <= inference_params.seqlen_offset:
            token = sample(logits, top_k=top_k, top_p=top_p, temperature=temperature, generator=generator)
        else:
            token = teacher_outputs[:, inference_params.seqlen_offset]
        return token.unsqueeze(1)

    def should_stop(current_token):
        if inference_params.seqlen_offset == 0:
            return False
        if eos_token_id is not None and bool((current_token == eos_token_id).all()):
            return True
        return inference_params.seqlen_offset >= max_length - 1

    if enable_timing:
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
    scores, sequences = [], [input_ids]
    while not should_stop(sequences[-1]):
        scores.append(get_logits(sequences[-1]))
        inference_params.seqlen_offset += sequences[-1].shape[1]
        sequences.append(sample_tokens(scores[-1]))
    if enable_timing:
        end.record()
        torch.cuda.synchronize()
        print(f"Prompt processing + decoding time: {start.elapsed_time(end):.0f}ms")
    return GenerationOutput(sequences=torch.cat(sequences, dim=1), scores=tuple(scores))


class GenerationMixin:
    def allocate_inference_cache(self, batch_size, max_seqlen, dtype=None, **kwargs):
        raise NotImplementedError

    def generate(self, input_ids, max_length, top_k=1, top_p=0.0, temperature=1.0, return_dict_in_generate=False, output_scores=False, **kwargs):
        """kwargs: cg, eos_token_id, teacher_outputs, vocab_size, enable_timing, generator, fused_sampling, uniforms, seq_idx (see `decode`)"""
        output = decode(input_ids, self, max_length, top_k=top_k, top_p=top_p, temperature=temperature, output_scores=output_scores, **kwargs)
        if not output_scores:
            output.scores = None
        return output if return_dict_in_generate else output.sequences


@dataclasses.dataclass
class DecodingCGCache:
    """the states of a model for up to max_batch_size sequences of max_seqlen tokens and one captured decode step per (batch, seqlen 1) -- and,
    for fused sampling, per (batch, seqlen 1, top_k, top_p, temperature, vocab_size): the sampler's parameters are baked into its graph node.
    Those steps share three static buffers: the uniforms, the token table (both (max_seqlen, batch) over one flat allocation) and the step counter."""
    max_batch_size: int = 0
    max_seqlen: int = 0
    device = None
    dtype = None
    callables: dict = dataclasses.field(default_factory=dict)
    mempool = None
    inference_params: Optional[InferenceParams] = None
    run: Optional[Callable] = None
    n_captures: int = 0                                     # graphs captured so far (tests count them)
    batch_params: dict = dataclasses.field(default_factory=dict)
    sample_u: Optional[torch.Tensor] = None                 # (max_seqlen * max_batch_size,) float32
    sample_tokens: Optional[torch.Tensor] = None            # (max_seqlen * max_batch_size,) int64
    sample_counter: Optional[torch.Tensor] = None           # (1,) int64: the step the next sample belongs to

    def sampling_buffers(self, batch_size):
        """-> (uniforms, counter, tokens): the (max_seqlen, batch_size) views that the captured sampling steps of this batch size address"""
        n = self.max_seqlen * batch_size
        return self.sample_u[:n].view(self.max_seqlen, batch_size), self.sample_counter, self.sample_tokens[:n].view(self.max_seqlen, batch_size)

    def params_for(self, batch_size):
        """the InferenceParams of a batch of this size: the first batch_size rows of every cached state, as views"""
        if batch_size == self.max_batch_size:
            return self.inference_params
        if batch_size not in self.batch_params:
            views = {k: tuple(t[:batch_size] for t in states) for k, states in self.inference_params.key_value_memory_dict.items()}
            self.batch_params[batch_size] = InferenceParams(max_seqlen=self.max_seqlen, max_batch_size=batch_size, key_value_memory_dict=views)
        return self.batch_params[batch_size]


@torch.no_grad()
def update_graph_cache(model, cache, batch_size, seqlen_og, max_seqlen, decoding_seqlens=(1,), dtype=None, n_warmups=2, sampling=None):
    """-> the cache, (re)allocated when the device, dtype, batch size or length outgrow it, holding a captured step for this batch size.
    sampling = (top_k, top_p, temperature, vocab_size): the step that also samples (fused sampling), keyed apart from the plain one"""
    if cache is None:
        cache = DecodingCGCache()
    param_example = next(iter(model.parameters()))
    device = param_example.device
    if dtype is None:
        dtype = param_example.dtype
    if (device, dtype) != (cache.device, cache.dtype) or batch_size > cache.max_batch_size or max_seqlen > cache.max_seqlen:
        cache.callables, cache.batch_params = {}, {}      # the graphs hold the old states' addresses: drop them with the states
        cache.mempool = None
        cache.inference_params = None
        cache.sample_u = cache.sample_tokens = cache.sample_counter = None
        gc.collect()
        cache.device, cache.dtype = device, dtype
        cache.max_batch_size, cache.max_seqlen = batch_size, max_seqlen
        inf_cache = model.allocate_inference_cache(batch_size, max_seqlen, dtype)
        cache.inference_params = InferenceParams(max_seqlen=max_seqlen, max_batch_size=batch_size, seqlen_offset=seqlen_og,
                                                 key_value_memory_dict=inf_cache)
        cache.mempool = torch.cuda.graphs.graph_pool_handle()
    if sampling is not None and cache.sample_u is None:
        n = cache.max_seqlen * cache.max_batch_size
        cache.sample_u = torch.zeros(n, dtype=torch.float32, device=device)
        cache.sample_tokens = torch.zeros(n, dtype=torch.long, device=device)
        cache.sample_counter = torch.zeros(1, dtype=torch.long, device=device)
    for decoding_seqlen in decoding_seqlens:
        key = (batch_size, decoding_seqlen) + (tuple(sampling) if sampling is not None else ())
        if key not in cache.callables:
            cache.callables[key] = capture_graph(model, cache.params_for(batch_size), batch_size, max_seqlen, decoding_seqlen=decoding_seqlen,
                                                 mempool=cache.mempool, n_warmups=n_warmups, sampling=sampling,
                                                 sampling_buffers=cache.sampling_buffers(batch_size) if sampling is not None else None)
            cache.n_captures += 1

    def dispatch(input_ids, seqlen):
        return cache.callables[input_ids.shape[0], input_ids.shape[1]](input_ids, seqlen)

    cache.run = dispatch
    cache.inference_params.seqlen_offset = 0
    return cache


def capture_graph(model, inference_params, batch_size, max_seqlen, decoding_seqlen=1, mempool=None, n_warmups=2, sampling=None,
                  sampling_buffers=None):
    """one forward of the model on a static (batch_size, decoding_seqlen) token buffer at seqlen_offset > 0, captured -> run(new_input_ids,
    seqlen) that copies the tokens in, replays and returns a copy of the logits. The warm-up runs (library handles, the allocator's blocks) go
    to a side stream before the capture; the capture itself records on one stream.
    sampling = (top_k, top_p, temperature, vocab_size) with sampling_buffers = (uniforms, counter, tokens): the step goes on, on the same
    stream, with sample_logits on its own logits at the counter's step -- the token lands in the static token buffer (the next replay's
    input) and in `tokens` -- and counter += 1 -> step() that only replays and returns the static logits (no copy in, no clone);
    step.input_ids is the static token buffer, for the caller to put the first token in."""
    device = next(iter(model.parameters())).device
    input_ids = torch.full((batch_size, decoding_seqlen), 0, dtype=torch.long, device=device)
    if sampling is not None:
        assert decoding_seqlen == 1, "a step that samples feeds itself: one token per row"
        top_k, top_p, temperature, vocab_size = sampling
        table, counter, tokens = sampling_buffers

    def forward():
        logits = model(input_ids, inference_params=inference_params, num_last_tokens=decoding_seqlen).logits
        if sampling is not None:
            last = logits[:, -1]
            native.sample_logits(last[..., :vocab_size] if vocab_size is not None else last, table, top_k=top_k, top_p=top_p,
                                 temperature=temperature, out=input_ids, row_index=counter, out_table=tokens)
            counter.add_(1)
        return logits

    seqlen_offset_og = inference_params.seqlen_offset
    inference_params.seqlen_offset = max_seqlen - decoding_seqlen
    assert inference_params.seqlen_offset > 0, "a decode step is captured at seqlen_offset > 0: max_seqlen must exceed the step's length"
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(n_warmups):
            logits = forward()
        s.synchronize()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, pool=mempool):
        logits = forward()

    def run(new_input_ids, seqlen):
        input_ids.copy_(new_input_ids)
        graph.replay()
        return logits.clone()

    def step():
        graph.replay()
        return logits

    step.input_ids = input_ids
    inference_params.seqlen_offset = seqlen_offset_og
    return run if sampling is None else step
