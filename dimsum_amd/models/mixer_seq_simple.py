"""The Mamba language model -- `create_block`, `_init_weights`, `MixerModel`, `MambaLMHeadModel` with the constructor arguments, forward
contracts and state-dict keys of mamba/mamba_ssm/models/mixer_seq_simple.py, on this package's HIP operators.

Prompts run the fused add + norm kernel and the mixers' fused prompt path, which leaves the per-layer (conv_state, ssm_state) caches behind; one
token of a cached sequence runs the fused decode step (modules/mamba_simple.py: Block, `step_fused`; csrc/decode_step.hip): four launches per
layer, the residual add of a layer in the next layer's prologue, and the model's last add + norm_f in the prologue of the lm_head launch.

`from_pretrained(path)` / `save_pretrained(path)` read and write a LOCAL directory (config.json + pytorch_model.bin, the layout of the published
Mamba checkpoints); nothing here reaches for a hub."""
import json
import math
import os
from collections import namedtuple
from functools import partial

import torch
import torch.nn as nn

from .. import native
from ..modules.mamba_simple import Block, Mamba, fused_decode_enabled
from ..ops.cross_entropy import linear_cross_entropy
from ..ops.layernorm import RMSNorm, layer_norm_fn
from ..utils.generation import GenerationMixin

CausalLMOutput = namedtuple("CausalLMOutput", ["logits"])
CONFIG_NAME, WEIGHTS_NAME = "config.json", "pytorch_model.bin"


def create_block(d_model, ssm_cfg=None, norm_epsilon=1e-5, rms_norm=False, residual_in_fp32=False, fused_add_norm=False, layer_idx=None,
                 device=None, dtype=None):
    fk = {"device": device, "dtype": dtype}
    mixer_cls = partial(Mamba, layer_idx=layer_idx, **(ssm_cfg or {}), **fk)
    norm_cls = partial(RMSNorm if rms_norm else nn.LayerNorm, eps=norm_epsilon, **fk)
    block = Block(d_model, mixer_cls, norm_cls=norm_cls, fused_add_norm=fused_add_norm, residual_in_fp32=residual_in_fp32)
    block.layer_idx = layer_idx
    return block


def _init_weights(module, n_layer, initializer_range=0.02, rescale_prenorm_residual=True, n_residuals_per_layer=1):
    """the GPT-2 scheme of mixer_seq_simple.py:48-77: Linear biases to zero (unless marked _no_reinit: dt_proj's), embeddings N(0,
    initializer_range^2), and the projections that write into the residual stream (out_proj / fc2) re-drawn and divided by
    sqrt(n_residuals_per_layer * n_layer)"""
    if isinstance(module, nn.Linear):
        if module.bias is not None and not getattr(module.bias, "_no_reinit", False):
            nn.init.zeros_(module.bias)
    elif isinstance(module, nn.Embedding):
        nn.init.normal_(module.weight, std=initializer_range)
    if rescale_prenorm_residual:
        for name, p in module.named_parameters():
            if name in ("out_proj.weight", "fc2.weight"):
                nn.init.kaiming_uniform_(p, a=math.sqrt(5))       # re-drawn, not rescaled in place: this runs once per enclosing module
                with torch.no_grad():
                    p /= math.sqrt(n_residuals_per_layer * n_layer)


class MixerModel(nn.Module):
    def __init__(self, d_model, n_layer, vocab_size, ssm_cfg=None, norm_epsilon=1e-5, rms_norm=False, initializer_cfg=None, fused_add_norm=False,
                 residual_in_fp32=False, device=None, dtype=None):
        fk = {"device": device, "dtype": dtype}
        super().__init__()
        self.residual_in_fp32 = residual_in_fp32
        self.fused_add_norm = fused_add_norm
        self.embedding = nn.Embedding(vocab_size, d_model, **fk)
        self.layers = nn.ModuleList([create_block(d_model, ssm_cfg=ssm_cfg, norm_epsilon=norm_epsilon, rms_norm=rms_norm,
                                                  residual_in_fp32=residual_in_fp32, fused_add_norm=fused_add_norm, layer_idx=i, **fk)
                                     for i in range(n_layer)])
        self.norm_f = (RMSNorm if rms_norm else nn.LayerNorm)(d_model, eps=norm_epsilon, **fk)
        self.apply(partial(_init_weights, n_layer=n_layer, **(initializer_cfg or {})))

    def allocate_inference_cache(self, batch_size, max_seqlen, dtype=None, **kwargs):
        return {i: layer.allocate_inference_cache(batch_size, max_seqlen, dtype=dtype, **kwargs) for i, layer in enumerate(self.layers)}

    def forward(self, input_ids, inference_params=None, final_norm=True, seq_idx=None):
        """seq_idx (B, L) int32: packed rows -- the sequences of one row do not see each other in any mixer (modules/mamba_simple.py).
        -> the normed hidden states (B, L, d_model); final_norm=False (no reference counterpart): (hidden_states, residual) of the last block,
        for a caller that folds the last add + norm_f into its own launch (MambaLMHeadModel's decode step)"""
        hidden_states = self.embedding(input_ids)
        residual = None
        for layer in self.layers:
            hidden_states, residual = layer(hidden_states, residual, inference_params=inference_params,
                                            **({"seq_idx": seq_idx} if seq_idx is not None else {}))
        if not final_norm:
            return hidden_states, residual
        if not self.fused_add_norm:
            residual = (hidden_states + residual) if residual is not None else hidden_states
            return self.norm_f(residual.to(dtype=self.norm_f.weight.dtype))
        return layer_norm_fn(hidden_states, self.norm_f.weight, self.norm_f.bias, residual=residual, eps=self.norm_f.eps, prenorm=False,
                             residual_in_fp32=self.residual_in_fp32, is_rms_norm=isinstance(self.norm_f, RMSNorm))


class MambaLMHeadModel(nn.Module, GenerationMixin):
    def __init__(self, d_model, n_layer, vocab_size, initializer_cfg=None, pad_vocab_size_multiple=1, device=None, dtype=None, **backbone_kwargs):
        fk = {"device": device, "dtype": dtype}
        super().__init__()
        # what save_pretrained writes: the arguments as given (vocab_size before padding, as in the published config.json files)
        self.config = dict(d_model=d_model, n_layer=n_layer, vocab_size=vocab_size, pad_vocab_size_multiple=pad_vocab_size_multiple,
                           **({"initializer_cfg": initializer_cfg} if initializer_cfg is not None else {}), **backbone_kwargs)
        if vocab_size % pad_vocab_size_multiple != 0:
            vocab_size += pad_vocab_size_multiple - (vocab_size % pad_vocab_size_multiple)
        self.backbone = MixerModel(d_model=d_model, n_layer=n_layer, vocab_size=vocab_size, initializer_cfg=initializer_cfg, **backbone_kwargs, **fk)
        self.lm_head = nn.Linear(d_model, vocab_size, bias=False, **fk)
        self.apply(partial(_init_weights, n_layer=n_layer, **(initializer_cfg or {})))
        self.tie_weights()

    def tie_weights(self):
        self.lm_head.weight = self.backbone.embedding.weight

    def allocate_inference_cache(self, batch_size, max_seqlen, dtype=None, **kwargs):
        return self.backbone.allocate_inference_cache(batch_size, max_seqlen, dtype=dtype, **kwargs)

    def _fused_head(self, input_ids, inference_params):
        """one token of a cached sequence whose last add + norm_f can ride in the lm_head launch"""
        b = self.backbone
        if not (b.fused_add_norm and len(b.layers) > 0 and inference_params is not None and inference_params.seqlen_offset > 0
                and input_ids.dim() == 2 and input_ids.shape[1] == 1 and fused_decode_enabled(input_ids.shape[0], self.lm_head.weight.dtype)
                and not torch.is_grad_enabled()):
            return False
        w = self.lm_head.weight
        return (input_ids.shape[0] <= 16 and w.dtype in (torch.float32, torch.float16, torch.bfloat16)
                and all(t is None or t.dtype == w.dtype for t in (self.lm_head.bias, b.norm_f.weight, b.norm_f.bias)))

    def forward(self, input_ids, position_ids=None, inference_params=None, num_last_tokens=0, seq_idx=None, logits_positions=None):
        """position_ids: accepted and unused, as in the reference. num_last_tokens > 0: logits of the last n tokens only.
        seq_idx (B, L) int32: packed rows (several documents per row, or a left-padded prompt whose padding is a segment of its own); with
        inference_params at seqlen_offset == 0 the cache is left holding every row's last segment (with inference_params.prefill_slots: every
        segment's states go to its slot of the pools); at seqlen_offset > 0 it raises.
        logits_positions (S,) int64 on the device, with seq_idx: flattened positions b * L + t -- the final hidden rows are gathered there
        (index_select, no host read), the head runs on those S rows only and .logits is (S, V). Not together with num_last_tokens > 0."""
        if logits_positions is not None:
            if seq_idx is None:
                raise ValueError("logits_positions without seq_idx: they name the last tokens of a packed row's segments (plan_packed_prefill)")
            if num_last_tokens > 0:
                raise ValueError("logits_positions together with num_last_tokens > 0: both choose the rows the head runs on; pass one")
            if not (torch.is_tensor(logits_positions) and logits_positions.dtype == torch.int64 and logits_positions.dim() == 1):
                raise ValueError("logits_positions must be a 1-D int64 tensor of flattened positions b * seqlen + t")
        if seq_idx is not None:
            if inference_params is not None and inference_params.seqlen_offset > 0:
                raise ValueError("seq_idx at seqlen_offset > 0: sequence ids belong to the prompt pass (seqlen_offset == 0)")
            hidden_states = self.backbone(input_ids, inference_params=inference_params, seq_idx=seq_idx)
            if logits_positions is not None:
                rows = hidden_states.reshape(-1, hidden_states.shape[-1]).index_select(0, logits_positions)
                return CausalLMOutput(logits=self.lm_head(rows))
            if num_last_tokens > 0:
                hidden_states = hidden_states[:, -num_last_tokens:]
            return CausalLMOutput(logits=self.lm_head(hidden_states))
        if self._fused_head(input_ids, inference_params):
            hidden, residual = self.backbone(input_ids, inference_params=inference_params, final_norm=False)
            nf = self.backbone.norm_f
            if hidden.dtype == self.lm_head.weight.dtype and residual.dtype in (torch.float32, hidden.dtype):
                logits = native.decode_linear(hidden[:, 0], self.lm_head.weight, self.lm_head.bias,
                                              norm=(nf.weight, nf.bias, nf.eps, isinstance(nf, RMSNorm)), residual=residual[:, 0])
                return CausalLMOutput(logits=logits.unsqueeze(1))
            hidden_states = layer_norm_fn(hidden, nf.weight, nf.bias, residual=residual, eps=nf.eps, prenorm=False,
                                          residual_in_fp32=self.backbone.residual_in_fp32, is_rms_norm=isinstance(nf, RMSNorm))
        else:
            hidden_states = self.backbone(input_ids, inference_params=inference_params)
        if num_last_tokens > 0:
            hidden_states = hidden_states[:, -num_last_tokens:]
        return CausalLMOutput(logits=self.lm_head(hidden_states))

    def loss(self, input_ids, labels=None, *, chunk_rows=4096, ignore_index=-100, label_smoothing=0.0, lse_square_scale=0.0, reduction="mean",
             seq_idx=None):
        """-> the scalar training loss (no reference counterpart as a method: its recipes run a fused cross-entropy on forward()'s logits).
        The backbone, then the head product and the cross-entropy chunk_rows tokens at a time on csrc/cross_entropy.hip
        (ops.linear_cross_entropy): the (batch * seqlen, vocab) logits never exist. labels (batch, seqlen) int64, ignore_index where a
        position does not count; None = next-token prediction: input_ids shifted left, the last position ignored. Only the first
        config["vocab_size"] rows of lm_head.weight are classes: the vocabulary padding takes no part and gets a zero gradient.
        seq_idx (batch, seqlen) int32: packed rows, handed to the backbone. The loss's own arithmetic does not change: the caller marks what
        does not count -- a document's last token must not predict the next document's first -- e.g. with
        labels = dimsum_amd.utils.packed_labels(input_ids, seq_idx)."""
        hidden_states = self.backbone(input_ids) if seq_idx is None else self.backbone(input_ids, seq_idx=seq_idx)
        if labels is None:
            labels = torch.cat([input_ids[:, 1:], input_ids.new_full((input_ids.shape[0], 1), ignore_index)], dim=1)
        return linear_cross_entropy(hidden_states, self.lm_head.weight, labels, self.lm_head.bias, chunk_rows=chunk_rows, reduction=reduction,
                                    vocab_size=self.config["vocab_size"], label_smoothing=label_smoothing, lse_square_scale=lse_square_scale,
                                    ignore_index=ignore_index)

    @classmethod
    def from_pretrained(cls, pretrained_model_name, device=None, dtype=None, **kwargs):
        """pretrained_model_name: an existing local directory holding config.json and pytorch_model.bin. Anything else raises: there is no hub
        download in this package."""
        path = os.fspath(pretrained_model_name)
        if not os.path.isdir(path):
            raise FileNotFoundError(f"from_pretrained: {path!r} is not an existing directory (this package reads local checkpoint directories "
                                    f"with {CONFIG_NAME} + {WEIGHTS_NAME} only and never downloads)")
        with open(os.path.join(path, CONFIG_NAME)) as f:
            config = json.load(f)
        model = cls(**config, device=device, dtype=dtype, **kwargs)
        state = torch.load(os.path.join(path, WEIGHTS_NAME), map_location="cpu", weights_only=True)
        if dtype is not None:
            state = {k: v.to(dtype=dtype) for k, v in state.items()}
        model.load_state_dict(state)
        return model

    def save_pretrained(self, save_directory):
        """writes config.json (the constructor arguments) and pytorch_model.bin (the state dict) into save_directory, created if missing"""
        path = os.fspath(save_directory)
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, CONFIG_NAME), "w") as f:
            json.dump(self.config, f, indent=2)
            f.write("\n")
        torch.save({k: v.detach().cpu() for k, v in self.state_dict().items()}, os.path.join(path, WEIGHTS_NAME))
