"""ctypes loader of libdimsum_hip.so + mirrors of the C structs in include/dimsum_hip.h."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DIMSUM_HIP_LIB") or os.path.join(_HERE, "lib", "libdimsum_hip.so")   # override: kernel-variant experiments

F32, F16, BF16 = 0, 1, 2
i32, i64, vp, f32 = C.c_int32, C.c_int64, C.c_void_p, C.c_float


u32 = C.c_uint32


class _Sized(C.Structure):
    """parameter structs of ABI >= 17 start with `struct_size` = sizeof(the struct as the caller knows it): filled in on construction
    (a struct nested inside another one is part of the parent's buffer and is not constructed: the library ignores the nested size)"""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_size = C.sizeof(type(self))


class SsmExt(_Sized):
    """dimsum_ssm_ext_t: everything beyond the reference's SSMParamsBase"""
    _fields_ = [("struct_size", u32), ("kernel_variant", i32), ("ckpt_ptr", vp), ("timing_start_event", vp), ("timing_stop_event", vp),
                ("out_z_lo_offset", i64), ("dt_w_ptr", vp), ("dt_x_ptr", vp), ("dt_w_row_stride", i64), ("dt_x_row_stride", i64),
                ("dt_rank", i32), ("out_z_f16", i32), ("out_z_scale_ptr", vp), ("out_z_scale_ld", i64)]


class SsmParams(_Sized):
    _fields_ = ([("struct_size", u32)]
                + [(n, i32) for n in ("batch", "dim", "seqlen", "dstate", "n_groups", "n_chunks", "delta_softplus", "dtype", "reserved")]
                + [(n, i64) for n in ("A_d_stride", "A_dstate_stride", "B_batch_stride", "B_group_stride",
                                      "B_dstate_stride", "C_batch_stride", "C_group_stride", "C_dstate_stride",
                                      "u_batch_stride", "u_d_stride", "delta_batch_stride", "delta_d_stride",
                                      "z_batch_stride", "z_d_stride", "out_batch_stride", "out_d_stride",
                                      "out_z_batch_stride", "out_z_d_stride")]
                + [(n, vp) for n in ("A_ptr", "B_ptr", "C_ptr", "D_ptr", "u_ptr", "delta_ptr", "delta_bias_ptr",
                                     "z_ptr", "out_ptr", "x_ptr", "out_z_ptr")]
                + [("ext", C.POINTER(SsmExt))])


def attach_ext(P, ext_type):
    """a fresh, zeroed extension struct linked to P.ext (P keeps it alive) -> the extension"""
    E = ext_type()
    P.ext = C.pointer(E)
    return E


class SsmBwdParams(_Sized):
    _fields_ = ([("struct_size", u32), ("reserved", u32), ("fwd", SsmParams)]
                + [(n, i64) for n in ("dout_batch_stride", "dout_d_stride", "dA_d_stride", "dA_dstate_stride",
                                      "dB_batch_stride", "dB_group_stride", "dB_dstate_stride", "dC_batch_stride",
                                      "dC_group_stride", "dC_dstate_stride", "du_batch_stride", "du_d_stride",
                                      "dz_batch_stride", "dz_d_stride", "ddelta_batch_stride", "ddelta_d_stride")]
                + [(n, vp) for n in ("dout_ptr", "dA_ptr", "dB_ptr", "dC_ptr", "dD_ptr", "du_ptr", "dz_ptr",
                                     "ddelta_ptr", "ddelta_bias_ptr", "workspace_ptr")]
                + [("workspace_bytes", i64)])


class SsmBidirParams(_Sized):
    """dimsum_ssm_bidir_params_t: the shared operands + forward direction in `fwd`, the reversed direction's A / out / saved states"""
    _fields_ = [("struct_size", u32), ("reserved", u32), ("fwd", SsmParams), ("A_b_ptr", vp), ("A_b_d_stride", i64), ("A_b_dstate_stride", i64),
                ("out_b_ptr", vp), ("out_b_batch_stride", i64), ("out_b_d_stride", i64), ("ckpt_b_ptr", vp)]


class SsmBidirBwdParams(_Sized):
    """dimsum_ssm_bidir_bwd_params_t"""
    _fields_ = [("struct_size", u32), ("reserved", u32), ("bwd", SsmBwdParams), ("A_b_ptr", vp), ("A_b_d_stride", i64), ("A_b_dstate_stride", i64),
                ("out_b_ptr", vp), ("out_b_batch_stride", i64), ("out_b_d_stride", i64), ("ckpt_b_ptr", vp),
                ("dA_b_ptr", vp), ("dA_b_d_stride", i64), ("dA_b_dstate_stride", i64)]


class SsmGeneralParams(_Sized):
    """dimsum_ssm_general_params_t: the general scan -- any dstate in 1..256, constant B / C, complex A"""
    _fields_ = ([("struct_size", u32)]
                + [(n, i32) for n in ("batch", "dim", "seqlen", "dstate", "n_groups", "n_chunks", "delta_softplus", "dtype", "is_variable_B",
                                      "is_variable_C", "is_complex", "reserved")]
                + [(n, i64) for n in ("A_d_stride", "A_dstate_stride", "B_batch_stride", "B_d_stride", "B_group_stride", "B_dstate_stride",
                                      "C_batch_stride", "C_d_stride", "C_group_stride", "C_dstate_stride", "u_batch_stride", "u_d_stride",
                                      "delta_batch_stride", "delta_d_stride", "z_batch_stride", "z_d_stride", "out_batch_stride", "out_d_stride",
                                      "out_z_batch_stride", "out_z_d_stride")]
                + [(n, vp) for n in ("A_ptr", "B_ptr", "C_ptr", "D_ptr", "u_ptr", "delta_ptr", "delta_bias_ptr", "z_ptr", "out_ptr", "x_ptr",
                                     "out_z_ptr")])


class SsmGeneralBwdParams(_Sized):
    """dimsum_ssm_general_bwd_params_t"""
    _fields_ = ([("struct_size", u32), ("reserved", u32), ("fwd", SsmGeneralParams)]
                + [(n, i64) for n in ("dout_batch_stride", "dout_d_stride", "dA_d_stride", "dA_dstate_stride", "dB_batch_stride", "dB_d_stride",
                                      "dB_group_stride", "dB_dstate_stride", "dC_batch_stride", "dC_d_stride", "dC_group_stride", "dC_dstate_stride",
                                      "du_batch_stride", "du_d_stride", "dz_batch_stride", "dz_d_stride", "ddelta_batch_stride", "ddelta_d_stride")]
                + [(n, vp) for n in ("dout_ptr", "dA_ptr", "dB_ptr", "dC_ptr", "dD_ptr", "du_ptr", "dz_ptr", "ddelta_ptr", "ddelta_bias_ptr",
                                     "workspace_ptr")]
                + [("workspace_bytes", i64)])


class SsmCarryParams(_Sized):
    """dimsum_ssm_carry_params_t: the general forward entered with a carried (batch, dim, dstate) state h0, leaving hT (may be h0: in place)"""
    _fields_ = ([("struct_size", u32), ("state_dtype", i32), ("scan", SsmGeneralParams)]
                + [(n, i64) for n in ("h0_batch_stride", "h0_d_stride", "h0_dstate_stride", "hT_batch_stride", "hT_d_stride", "hT_dstate_stride")]
                + [("h0_ptr", vp), ("hT_ptr", vp)])


class SsmVarlenParams(_Sized):
    """dimsum_ssm_varlen_params_t: the general forward on packed rows -- a (batch, seqlen) int32 sequence id per token, the state restarts where it changes"""
    _fields_ = [("struct_size", u32), ("reserved", u32), ("scan", SsmGeneralParams), ("seq_idx_ptr", vp), ("seq_idx_batch_stride", i64)]


class SsmVarlenBwdParams(_Sized):
    """dimsum_ssm_varlen_bwd_params_t"""
    _fields_ = [("struct_size", u32), ("reserved", u32), ("bwd", SsmGeneralBwdParams), ("seq_idx_ptr", vp), ("seq_idx_batch_stride", i64)]


class SsmVarlenStatesParams(_Sized):
    """dimsum_ssm_varlen_states_params_t: SsmVarlenParams + end_slots (batch, seqlen) int32 -- where it is >= 0 the state after that position
    goes into that slot of a (num_slots, dim, dstate) pool"""
    _fields_ = ([("struct_size", u32), ("num_slots", i32), ("varlen", SsmVarlenParams), ("end_slots_ptr", vp), ("end_slots_batch_stride", i64),
                 ("state_ptr", vp)] + [(n, i64) for n in ("state_slot_stride", "state_d_stride", "state_dstate_stride")]
                + [("state_f32", i32), ("reserved", i32)])


class SsmVarlenResumeParams(_Sized):
    """dimsum_ssm_varlen_resume_params_t: SsmVarlenStatesParams + start_slots (batch, seqlen) int32 -- where it is >= 0 (a segment's first
    position) the segment continues that row of a (n_init, dim, dstate) tensor of states, which may be the pool itself"""
    _fields_ = ([("struct_size", u32), ("n_init", i32), ("states", SsmVarlenStatesParams), ("start_slots_ptr", vp), ("start_slots_batch_stride", i64),
                 ("init_ptr", vp)] + [(n, i64) for n in ("init_slot_stride", "init_d_stride", "init_dstate_stride")]
                + [("init_f32", i32), ("reserved", i32)])


class OptimParams(_Sized):
    """dimsum_optim_params_t: device tables of the tensor list + hyper-parameters of one clip / AdamW / EMA step"""
    _fields_ = ([("struct_size", u32), ("n_tensors", i32), ("n_chunks", i32), ("n_partials", i32)]
                + [(n, vp) for n in ("p_ptrs", "g_ptrs", "m_ptrs", "v_ptrs", "ema_ptrs", "step_ptrs", "numel", "chunk_table", "partials", "total_norm")]
                + [(n, C.c_double) for n in ("lr", "beta1", "beta2", "eps", "weight_decay", "max_norm", "ema_decay")]
                + [("reserved", i64 * 4)])


OPTIM_CHUNK, OPTIM_MAX_PARTIALS = 4096, 2048       # DIMSUM_OPTIM_CHUNK, DIMSUM_OPTIM_MAX_PARTIALS


class FmPlanParams(_Sized):
    """dimsum_fm_plan_params_t: x_t / u_t of the interpolation plan from a (5, batch) coefficient table, optional DCT blur of x1 for x_t"""
    _fields_ = ([("struct_size", u32)] + [(n, i32) for n in ("batch", "channels", "height", "width", "patch")] + [("min_scale", f32), ("reserved", i32)]
                + [("x1_batch_stride", i64)] + [(n, vp) for n in ("x1", "x0", "coef", "xt", "ut")] + [("reserved2", i64 * 2)])


class FmLossParams(_Sized):
    """dimsum_fm_loss_params_t: loss_b = w_b mean (c_b out + sign tgt)^2 and its gradient with respect to out"""
    _fields_ = ([("struct_size", u32), ("batch", i32), ("n", i64), ("sign", f32), ("reserved", i32)]
                + [(n, vp) for n in ("out", "tgt", "w", "c", "loss", "gloss", "dout")] + [("reserved2", i64 * 2)])


class PosRopeParams(_Sized):
    """dimsum_pos_rope_params_t: y = x cos + rotate_half(x) sin over channel pairs, or (inverse) the transpose of that map"""
    _fields_ = ([("struct_size", u32)] + [(n, i32) for n in ("batch", "tokens", "channels", "inverse", "reserved")]
                + [(n, i64) for n in ("x_batch_stride", "x_token_stride", "y_batch_stride", "y_token_stride")]
                + [(n, vp) for n in ("x", "sin", "cos", "y")] + [("reserved2", i64 * 2)])


class PosCpeParams(_Sized):
    """dimsum_pos_cpe_params_t: depthwise 3x3 conv on the token grid + x, LayerNorm, affine, modulate"""
    _fields_ = ([("struct_size", u32)] + [(n, i32) for n in ("batch", "grid", "channels")] + [("eps", f32), ("reserved", i32)]
                + [(n, i64) for n in ("x_batch_stride", "x_token_stride", "y_batch_stride", "y_token_stride", "mod_batch_stride")]
                + [(n, vp) for n in ("x", "weight", "conv_bias", "gamma", "beta", "shift", "scale", "y", "mean", "rstd", "v")]
                + [("reserved2", i64 * 2)])


class PosCpeBwdParams(_Sized):
    """dimsum_pos_cpe_bwd_params_t"""
    _fields_ = ([("struct_size", u32), ("reserved", u32), ("fwd", PosCpeParams)]
                + [(n, i64) for n in ("dy_batch_stride", "dy_token_stride", "dmod_batch_stride")]
                + [(n, vp) for n in ("dy", "dv", "dx", "dweight", "dconv_bias", "dgamma", "dbeta", "dshift", "dscale")]
                + [("reserved2", i64 * 2)])


class EinfftDftParams(_Sized):
    """dimsum_einfft_dft_params_t: the real tensor x and the two planes of its spectrum (dft reads x, idft_real writes it)"""
    _fields_ = ([("struct_size", u32)] + [(n, i32) for n in ("batch", "tokens", "channels")] + [("x_batch_stride", i64), ("x_token_stride", i64)]
                + [(n, vp) for n in ("x", "re", "im")] + [("reserved2", i64 * 2)])


class EinfftMlpParams(_Sized):
    """dimsum_einfft_mlp_params_t: the block-diagonal complex two-layer MLP + softshrink over (rows, channels) plane pairs"""
    _fields_ = ([("struct_size", u32), ("channels", i32), ("rows", i64), ("lam", f32), ("reserved", i32)]
                + [(n, vp) for n in ("xr", "xi", "w1", "b1", "w2", "b2", "zr", "zi")] + [("reserved2", i64 * 2)])


class EinfftMlpBwdParams(_Sized):
    """dimsum_einfft_mlp_bwd_params_t"""
    _fields_ = ([("struct_size", u32), ("reserved", u32), ("fwd", EinfftMlpParams)]
                + [(n, vp) for n in ("w1t", "w2t", "dzr", "dzi", "dxr", "dxi", "h1r", "h1i", "dz2r", "dz2i", "dp1r", "dp1i")]
                + [("reserved2", i64 * 2)])


class ConvParams(_Sized):
    _fields_ = ([("struct_size", u32)] + [(n, i32) for n in ("batch", "dim", "seqlen", "width", "silu_activation", "dtype", "reserved")]
                + [(n, i64) for n in ("x_batch_stride", "x_c_stride", "weight_c_stride", "weight_width_stride",
                                      "out_batch_stride", "out_c_stride")]
                + [(n, vp) for n in ("x_ptr", "weight_ptr", "bias_ptr", "out_ptr")])


class ConvBwdParams(_Sized):
    _fields_ = ([("struct_size", u32), ("reserved", u32), ("fwd", ConvParams)]
                + [(n, i64) for n in ("dout_batch_stride", "dout_c_stride", "dx_batch_stride", "dx_c_stride",
                                      "dweight_c_stride", "dweight_width_stride")]
                + [(n, vp) for n in ("dout_ptr", "dx_ptr", "dweight_ptr", "dbias_ptr")])


class ConvVarlenParams(_Sized):
    """dimsum_conv_varlen_params_t: the causal conv1d on packed rows -- taps that cross a change of the (batch, seqlen) int32 sequence id are dropped"""
    _fields_ = [("struct_size", u32), ("reserved", u32), ("conv", ConvParams), ("seq_idx_ptr", vp), ("seq_idx_batch_stride", i64)]


class ConvVarlenBwdParams(_Sized):
    """dimsum_conv_varlen_bwd_params_t"""
    _fields_ = [("struct_size", u32), ("reserved", u32), ("conv", ConvBwdParams), ("seq_idx_ptr", vp), ("seq_idx_batch_stride", i64)]


class ConvVarlenStatesParams(_Sized):
    """dimsum_conv_varlen_states_params_t: ConvVarlenParams + end_slots (batch, seqlen) int32 -- where it is >= 0 the conv state of the segment
    ending there goes into that slot of a (num_slots, dim, width) pool of x's dtype"""
    _fields_ = ([("struct_size", u32), ("num_slots", i32), ("varlen", ConvVarlenParams), ("end_slots_ptr", vp), ("end_slots_batch_stride", i64),
                 ("state_ptr", vp)] + [(n, i64) for n in ("state_slot_stride", "state_c_stride", "state_w_stride")]
                + [("state_dtype", i32), ("reserved", i32)])


class ConvVarlenResumeParams(_Sized):
    """dimsum_conv_varlen_resume_params_t: ConvVarlenStatesParams + start_slots (batch, seqlen) int32 -- where it is >= 0 (a segment's first
    position) the taps that reach before the segment read that row of a (n_init, dim, width) tensor of conv states of x's dtype"""
    _fields_ = ([("struct_size", u32), ("n_init", i32), ("states", ConvVarlenStatesParams), ("start_slots_ptr", vp), ("start_slots_batch_stride", i64),
                 ("init_ptr", vp)] + [(n, i64) for n in ("init_slot_stride", "init_c_stride", "init_w_stride")]
                + [("init_dtype", i32), ("reserved", i32)])


class ConvClParams(_Sized):
    """dimsum_conv_cl_params_t: the causal conv1d on channel-last operands, (batch, seqlen, dim) with channel stride 1"""
    _fields_ = ([("struct_size", u32), ("reserved", u32)]
                + [(n, i32) for n in ("batch", "dim", "seqlen", "width", "silu_activation", "dtype")]
                + [(n, i64) for n in ("x_batch_stride", "x_l_stride", "weight_c_stride", "weight_width_stride",
                                      "out_batch_stride", "out_l_stride")]
                + [(n, vp) for n in ("x_ptr", "weight_ptr", "bias_ptr", "out_ptr")])


class ConvClBwdParams(_Sized):
    """dimsum_conv_cl_bwd_params_t"""
    _fields_ = ([("struct_size", u32), ("reserved", u32), ("fwd", ConvClParams)]
                + [(n, i64) for n in ("dout_batch_stride", "dout_l_stride", "dx_batch_stride", "dx_l_stride",
                                      "dweight_c_stride", "dweight_width_stride")]
                + [(n, vp) for n in ("dout_ptr", "dx_ptr", "dweight_ptr", "dbias_ptr")])


class ConvUpdateParams(_Sized):
    """dimsum_conv_update_params_t: one step of the causal conv1d on a carried (batch, dim, width) state, in place"""
    _fields_ = ([("struct_size", u32)] + [(n, i32) for n in ("batch", "dim", "width", "silu_activation", "dtype")] + [("reserved", i32 * 2)]
                + [(n, i64) for n in ("x_batch_stride", "x_c_stride", "state_batch_stride", "state_c_stride", "state_w_stride",
                                      "weight_c_stride", "weight_width_stride", "out_batch_stride", "out_c_stride")]
                + [(n, vp) for n in ("x_ptr", "weight_ptr", "bias_ptr", "conv_state_ptr", "out_ptr")])


class ConvChunkParams(_Sized):
    """dimsum_conv_chunk_params_t: any number of tokens of the causal conv1d on a carried (batch, dim, width) state, in place"""
    _fields_ = ([("struct_size", u32)] + [(n, i32) for n in ("batch", "dim", "seqlen", "width", "silu_activation", "dtype", "reserved")]
                + [(n, i64) for n in ("x_batch_stride", "x_c_stride", "state_batch_stride", "state_c_stride", "state_w_stride",
                                      "weight_c_stride", "weight_width_stride", "out_batch_stride", "out_c_stride")]
                + [(n, vp) for n in ("x_ptr", "weight_ptr", "bias_ptr", "conv_state_ptr", "out_ptr")])


class StateUpdateExt(_Sized):
    """dimsum_state_update_ext_t: dt_proj formed inside the step, dt[b, d] = dt_w[d, :] . dt_x[b, :]"""
    _fields_ = ([("struct_size", u32), ("dt_rank", i32), ("dt_w_ptr", vp), ("dt_x_ptr", vp)]
                + [(n, i64) for n in ("dt_w_d_stride", "dt_w_r_stride", "dt_x_batch_stride", "dt_x_r_stride")])


class StateUpdateParams(_Sized):
    """dimsum_state_update_params_t: one step of the selective scan on a carried (batch, dim, dstate) state, in place"""
    _fields_ = ([("struct_size", u32)] + [(n, i32) for n in ("batch", "dim", "dstate", "dt_softplus", "dtype", "state_dtype", "bc_dtype")]
                + [(n, i64) for n in ("state_batch_stride", "state_d_stride", "state_n_stride", "x_batch_stride", "x_d_stride",
                                      "dt_batch_stride", "dt_d_stride", "A_d_stride", "A_n_stride", "B_batch_stride", "B_n_stride",
                                      "C_batch_stride", "C_n_stride", "z_batch_stride", "z_d_stride", "out_batch_stride", "out_d_stride")]
                + [(n, vp) for n in ("state_ptr", "x_ptr", "dt_ptr", "A_ptr", "B_ptr", "C_ptr", "D_ptr", "z_ptr", "dt_bias_ptr", "out_ptr")]
                + [("ext", C.POINTER(StateUpdateExt))])


class DecodeLinearParams(_Sized):
    """dimsum_decode_linear_params_t: the weight-streaming linear layer of a decode step, with the add + norm prologue and the conv-update epilogue"""
    _fields_ = ([("struct_size", u32)]
                + [(n, i32) for n in ("batch", "n", "k", "dtype", "residual_dtype", "norm", "conv_dim", "conv_width", "silu_activation")]
                + [("eps", f32), ("reserved", i32)]
                + [(n, i64) for n in ("x_row_stride", "w_row_stride", "y_row_stride", "residual_row_stride", "residual_out_row_stride",
                                      "state_batch_stride", "state_c_stride", "state_w_stride", "conv_weight_c_stride", "conv_weight_width_stride")]
                + [(n, vp) for n in ("x_ptr", "w_ptr", "bias_ptr", "residual_ptr", "norm_weight_ptr", "norm_bias_ptr", "conv_weight_ptr", "conv_bias_ptr",
                                     "y_ptr", "residual_out_ptr", "conv_state_ptr")])


class ConvUpdateSlotsParams(_Sized):
    """dimsum_conv_update_slots_params_t: dimsum_causal_conv1d_update on a pool of states -- row b works on conv_state[slots[b]], slots[b] < 0 is a padding row"""
    _fields_ = [("struct_size", u32), ("num_slots", i32), ("conv", ConvUpdateParams), ("slots_ptr", vp), ("slots_stride", i64)]


class StateUpdateSlotsParams(_Sized):
    """dimsum_state_update_slots_params_t: dimsum_selective_state_update on a pool of states, addressed like ConvUpdateSlotsParams"""
    _fields_ = [("struct_size", u32), ("num_slots", i32), ("update", StateUpdateParams), ("slots_ptr", vp), ("slots_stride", i64)]


class DecodeLinearSlotsParams(_Sized):
    """dimsum_decode_linear_slots_params_t: dimsum_decode_linear whose conv epilogue works on a pool of conv states, addressed like ConvUpdateSlotsParams"""
    _fields_ = [("struct_size", u32), ("num_slots", i32), ("linear", DecodeLinearParams), ("slots_ptr", vp), ("slots_stride", i64)]


class StateCopyParams(_Sized):
    """dimsum_state_copy_params_t: rows src -> dst of every tensor of a state pool, pairs and the pool's table read on the device"""
    _fields_ = [("struct_size", u32), ("num_slots", i32), ("n_tensors", i32), ("n_pairs", i32), ("table_ptr", vp), ("pairs_ptr", vp),
                ("pairs_stride", i64), ("max_row_bytes", i64), ("reserved", i64 * 2)]


STATE_COPY_CHUNK_BYTES = 16384           # DIMSUM_STATE_COPY_CHUNK_BYTES

DECODE_NORM_NONE, DECODE_NORM_LAYER, DECODE_NORM_RMS = 0, 1, 2
DECODE_MAX_BATCH = 16


class CrossEntropyParams(_Sized):
    """dimsum_cross_entropy_params_t: the LM loss over rows of logits (fwd) and its gradient, optionally in place (bwd)"""
    _fields_ = ([("struct_size", u32), ("dtype", i32)]
                + [(n, i64) for n in ("rows", "vocab", "logits_row_stride", "dlogits_row_stride", "dloss_stride", "ignore_index")]
                + [(n, f32) for n in ("label_smoothing", "logit_scale", "lse_square_scale")] + [("reserved", i32)]
                + [(n, vp) for n in ("logits_ptr", "labels_ptr", "dloss_ptr", "loss_ptr", "lse_ptr", "z_loss_ptr", "dlogits_ptr")])


CROSS_ENTROPY_WAVE_ROW_MAX = 4096        # kCeWaveRowMax: a row of up to this many logits is one wave's, a longer one a workgroup's


class SampleLogitsParams(_Sized):
    """dimsum_sample_logits_params_t: one token per row of logits under top-k / top-p / temperature, drawn with the caller's uniforms"""
    _fields_ = ([("struct_size", u32), ("dtype", i32)] + [(n, i64) for n in ("rows", "vocab", "logits_row_stride")]
                + [("top_k", i32), ("top_p", f32), ("temperature", f32), ("reserved", i32)]
                + [(n, vp) for n in ("logits_ptr", "u_ptr", "out_ptr", "row_index_ptr", "out_table_ptr")] + [("table_steps", i64)])


class NormParams(_Sized):
    _fields_ = ([("struct_size", u32)] + [(n, i32) for n in ("rows", "cols", "is_rms_norm", "x_dtype", "residual_dtype", "out_dtype")]
                + [("eps", f32)]
                + [(n, i64) for n in ("x_row_stride", "residual_row_stride", "y_row_stride", "residual_out_row_stride")]
                + [(n, vp) for n in ("x_ptr", "residual_ptr", "weight_ptr", "bias_ptr", "y_ptr", "residual_out_ptr",
                                     "mean_ptr", "rstd_ptr", "xbias_ptr", "mod_scale_ptr", "mod_shift_ptr")]
                + [("mod_row_stride", i64), ("rows_per_batch", i32), ("y_split3", i32), ("y_inv_scale_ptr", vp)])


class NormBwdParams(_Sized):
    _fields_ = ([("struct_size", u32)] + [(n, i32) for n in ("rows", "cols", "is_rms_norm")] + [("eps", f32), ("reserved", i32)]
                + [(n, i64) for n in ("r_row_stride", "dy_row_stride", "dres_row_stride", "dx_row_stride")]
                + [(n, vp) for n in ("r_ptr", "weight_ptr", "mean_ptr", "rstd_ptr", "dy_ptr", "dres_ptr", "dx_ptr",
                                     "dweight_ptr", "dbias_ptr")])


class TtParams(_Sized):
    _fields_ = ([("struct_size", u32)] + [(n, i32) for n in ("batch", "tokens", "channels", "grid", "kind", "y_split3")]
                + [(n, i64) for n in ("x_batch_stride", "x_token_stride", "res_batch_stride", "res_token_stride",
                                      "y_batch_stride", "y_token_stride", "mod_batch_stride", "w_batch_stride",
                                      "w_token_stride", "red_batch_stride")]
                + [(n, vp) for n in ("x_ptr", "in_index_ptr", "out_index_ptr", "gate_ptr", "scale_ptr", "shift_ptr",
                                     "residual_ptr", "y_ptr", "w_ptr", "wdot_ptr", "wsum_ptr", "tsum_ptr", "y_inv_scale_ptr")]
                + [("y_f16s_lds_offset", i32), ("reserved", i32)])


class XattnParams(_Sized):
    _fields_ = ([("struct_size", u32)] + [(n, i32) for n in ("batch", "seqlen", "heads", "head_dim")] + [("scale", f32), ("n_dirs", i32)]
                + [(n, i64) for n in ("qkv_batch_stride", "qkv_token_stride", "out_batch_stride", "out_token_stride")]
                + [(n, vp) for n in ("qkv1_ptr", "qkv2_ptr", "out_ptr", "lse_ptr", "bias1_ptr", "bias2_ptr")]
                + [("precision", i32), ("out_split3", i32)]
                + [(n, vp) for n in ("x1_inv_ptr", "x2_inv_ptr", "kv_bound_ptr", "out_inv_ptr")] + [("qkv_f16", i32), ("reserved2", i32)])


class XattnBwdParams(_Sized):
    _fields_ = ([("struct_size", u32), ("reserved", u32), ("fwd", XattnParams)] + [(n, i64) for n in ("dqkv_batch_stride", "dqkv_token_stride")]
                + [(n, vp) for n in ("dout_ptr", "dqkv1_ptr", "dqkv2_ptr", "delta_ptr")])


class GemmExt(_Sized):
    """dimsum_gemm_ext_t: fused-epilogue operands, operand-image read modes, timing, tuning"""
    _fields_ = ([("struct_size", u32), ("rows_per_batch", i32), ("timing_start_event", vp), ("timing_stop_event", vp)]
                + [(n, i32) for n in ("tune_variant", "tune_group_m", "tune_reserved", "c_image_pieces")]
                + [(n, vp) for n in ("gate_bound_ptr", "h_inv_scale_ptr", "residual_ptr", "gate_ptr")]
                + [("residual_ld", i64), ("gate_ld", i64), ("x12_ptr", vp), ("x12_ld", i64), ("a_alias_rows", i64), ("b_alias_rows", i64),
                   ("a_alias_weight_order", i32), ("qkv_q_cols", i32), ("conv_weight_ptr", vp), ("conv_bias_ptr", vp),
                   ("conv_rows", i32), ("conv_width", i32), ("conv_seq", i32), ("conv_weight_ld", i32),
                   ("a_block_inv_ptr", vp), ("a_block_inv_ld", i64), ("tn_pair_a_cols", i64), ("tn_pair_b_cols", i64),
                   ("k_scale_ptr", vp), ("c_scale_ptr", vp), ("k_inv_a_ptr", vp), ("k_inv_b_ptr", vp)])


class GemmParams(_Sized):
    _fields_ = ([("struct_size", u32)] + [(n, i32) for n in ("m", "n", "k", "operand_dtype", "epilogue")] + [("out_scale", f32), ("reserved", i32)]
                + [(n, i64) for n in ("lda", "ldb", "ldc")]
                + [(n, vp) for n in ("a_ptr", "b_ptr", "bias_ptr", "c_ptr", "a_inv_scale_ptr", "b_inv_scale_ptr")]
                + [("ext", C.POINTER(GemmExt))])


class GeluExt(_Sized):
    """dimsum_gelu_ext_t: the bound-derived row scale of the forward's scaled-fp16 image"""
    _fields_ = [("struct_size", u32), ("reserved", i32), ("row_inv_ptr", vp), ("bound_ptr", vp)]


class GeluParams(_Sized):
    """dimsum_gelu_params_t: bias + GELU(tanh) of the plain MLP as a row pass, forward and backward"""
    _fields_ = ([("struct_size", u32), ("out_image", i32), ("rows", i64), ("hidden", i64)]
                + [(n, vp) for n in ("x_ptr", "bias_ptr", "dh_ptr", "out_ptr", "inv_scale_ptr", "dbias_ptr")] + [("ext", C.POINTER(GeluExt))])


GELU_OUT_F32, GELU_OUT_SPLIT3, GELU_OUT_PAIR, GELU_OUT_F16S = 0, 1, 2, 3


class MoeExt(_Sized):
    """dimsum_moe_ext_t: nothing yet"""
    _fields_ = [("struct_size", u32), ("reserved", i32)]


class MoeRouteParams(_Sized):
    """dimsum_moe_route_params_t: the router, top-1 choice and counting sort (fwd); the router's adjoint (bwd)"""
    _fields_ = ([("struct_size", u32), ("mode", i32), ("num_experts", i32), ("reserved", i32), ("tokens", i64), ("hidden", i64)]
                + [(n, vp) for n in ("x_ptr", "w_ptr", "b_ptr", "prob_ptr", "expert_ptr", "logits_ptr", "offsets_ptr", "perm_ptr", "inv_ptr",
                                     "row_expert_ptr", "work_ptr")]
                + [("work_bytes", i64)] + [(n, vp) for n in ("dprob_ptr", "dxp_ptr", "dx_ptr", "dw_ptr", "db_ptr")] + [("ext", C.POINTER(MoeExt))])


class MoeRowsParams(_Sized):
    """dimsum_moe_rows_params_t: permute, combine forward and backward"""
    _fields_ = ([("struct_size", u32), ("reserved", i32), ("rows", i64), ("hidden", i64)]
                + [(n, vp) for n in ("src_ptr", "perm_ptr", "prob_ptr", "y_ptr", "dst_ptr", "dprob_ptr")] + [("ext", C.POINTER(MoeExt))])


class MoeActParams(_Sized):
    """dimsum_moe_act_params_t: the experts' exact-GELU activation over the sorted rows"""
    _fields_ = ([("struct_size", u32), ("gated", i32), ("num_experts", i32), ("reserved", i32), ("rows", i64), ("width", i64)]
                + [(n, vp) for n in ("x_ptr", "bias_ptr", "row_expert_ptr", "dh_ptr", "out_ptr", "dbias_ptr")] + [("ext", C.POINTER(MoeExt))])


class MoeGemmParams(_Sized):
    """dimsum_moe_gemm_params_t: the grouped expert GEMM on device offsets (w_ptrs: a host array of device pointers)"""
    _fields_ = ([("struct_size", u32), ("num_experts", i32), ("tokens", i64), ("k", i64), ("n", i64), ("ldc", i64), ("x_ptr", vp), ("offsets_ptr", vp),
                 ("w_ptrs", C.POINTER(vp)), ("bias_ptr", vp), ("out_ptr", vp), ("ext", C.POINTER(MoeExt))])


class MoeGemmDgradParams(_Sized):
    """dimsum_moe_gemm_dgrad_params_t: the data gradient of the grouped expert GEMM (w_ptrs: a host array of device pointers)"""
    _fields_ = ([("struct_size", u32), ("num_experts", i32), ("tokens", i64), ("k", i64), ("n", i64), ("ldc", i64), ("dy_ptr", vp), ("offsets_ptr", vp),
                 ("w_ptrs", C.POINTER(vp)), ("dx_ptr", vp), ("ext", C.POINTER(MoeExt))])


class MoeGemmWgradParams(_Sized):
    """dimsum_moe_gemm_wgrad_params_t: the weight (and bias) gradients of the grouped expert GEMM (dw_ptrs: a host array of device pointers)"""
    _fields_ = ([("struct_size", u32), ("num_experts", i32), ("tokens", i64), ("k", i64), ("n", i64), ("dy_ptr", vp), ("x_ptr", vp), ("offsets_ptr", vp),
                 ("dw_ptrs", C.POINTER(vp)), ("db_ptr", vp), ("ext", C.POINTER(MoeExt))])


class MoeGemmF16sParams(_Sized):
    """dimsum_moe_gemm_f16s_params_t: the grouped expert GEMM on scaled-fp16 images (w_ptrs / w_inv_ptrs: host arrays of device pointers)"""
    _fields_ = ([("struct_size", u32), ("num_experts", i32), ("tokens", i64), ("k", i64), ("n", i64), ("ldc", i64), ("x_ptr", vp), ("x_inv_ptr", vp),
                 ("offsets_ptr", vp), ("w_ptrs", C.POINTER(vp)), ("w_inv_ptrs", C.POINTER(vp)), ("bias_ptr", vp), ("out_ptr", vp), ("ext", C.POINTER(MoeExt))])


class MoePermuteF16sParams(_Sized):
    """dimsum_moe_permute_f16s_params_t: the permute pass writing the scaled-fp16 image of the sorted rows"""
    _fields_ = ([("struct_size", u32), ("reserved", i32), ("rows", i64), ("hidden", i64)]
                + [(n, vp) for n in ("src_ptr", "perm_ptr", "dst_ptr", "inv_scale_ptr")] + [("ext", C.POINTER(MoeExt))])


class MoeActF16sParams(_Sized):
    """dimsum_moe_act_f16s_params_t: the experts' activation writing the scaled-fp16 image of h"""
    _fields_ = ([("struct_size", u32), ("gated", i32), ("num_experts", i32), ("reserved", i32), ("rows", i64), ("width", i64)]
                + [(n, vp) for n in ("x_ptr", "bias_ptr", "row_expert_ptr", "out_ptr", "inv_scale_ptr")] + [("ext", C.POINTER(MoeExt))])


MOE_ROUTE_SOFTMAX, MOE_ROUTE_SIGMOID = 0, 1
MOE_GEMM_BM, MOE_GEMM_BN = 64, 128      # DIMSUM_MOE_GEMM_BM / _BN: the output tile of dimsum_moe_gemm


class F16sJob(C.Structure):
    _fields_ = ([(n, vp) for n in ("src", "dst", "inv_scale_ptr", "l1max_ptr", "absmax_ptr")]
                + [(n, i64) for n in ("rows", "cols", "src_row_stride", "dst_row_stride")] + [("l1_factor", f32), ("reserved", i32)])


GEMM_EPI_F32, GEMM_EPI_GATED_GELU_SPLIT3, GEMM_EPI_GATED_GELU_F16, GEMM_EPI_F32_BIAS, GEMM_EPI_F32_GATE_RESIDUAL, GEMM_EPI_F16_QKV, GEMM_EPI_F32_CONV, GEMM_EPI_GELU_F16 = 0, 1, 2, 3, 4, 5, 6, 7

# every symbol include/dimsum_hip.h declares (tests check the library exports all of them)
EXPORTS = (
    "dimsum_status_string", "dimsum_abi_version", "dimsum_target_arch",
    "dimsum_event_create", "dimsum_event_destroy", "dimsum_event_elapsed_ms",
    "dimsum_ssm_scan_fwd", "dimsum_ssm_scan_bwd", "dimsum_ssm_scan_bwd_workspace_bytes", "dimsum_ssm_scan_fwd_variant",
    "dimsum_ssm_scan_bidir_fwd", "dimsum_ssm_scan_bidir_bwd", "dimsum_ssm_scan_bidir_fwd_variant",
    "dimsum_ssm_scan_general_fwd", "dimsum_ssm_scan_general_bwd", "dimsum_ssm_scan_general_bwd_workspace_bytes",
    "dimsum_ssm_scan_carry_fwd", "dimsum_causal_conv1d_chunk",
    "dimsum_causal_conv1d_varlen_fwd", "dimsum_causal_conv1d_varlen_bwd", "dimsum_ssm_scan_varlen_fwd", "dimsum_ssm_scan_varlen_bwd",
    "dimsum_causal_conv1d_varlen_states_fwd", "dimsum_ssm_scan_varlen_states_fwd",
    "dimsum_causal_conv1d_varlen_resume_fwd", "dimsum_ssm_scan_varlen_resume_fwd",
    "dimsum_optim_grad_sumsq", "dimsum_optim_adamw_ema_step", "dimsum_optim_write_ptrs",
    "dimsum_fm_plan", "dimsum_fm_loss_fwd", "dimsum_fm_loss_bwd",
    "dimsum_pos_rope", "dimsum_pos_cpe_fwd", "dimsum_pos_cpe_bwd",
    "dimsum_einfft_dft", "dimsum_einfft_idft_real", "dimsum_einfft_mlp_fwd", "dimsum_einfft_mlp_bwd",
    "dimsum_causal_conv1d_fwd", "dimsum_causal_conv1d_bwd", "dimsum_causal_conv1d_update", "dimsum_selective_state_update",
    "dimsum_decode_linear", "dimsum_cross_entropy_fwd", "dimsum_cross_entropy_bwd", "dimsum_sample_logits",
    "dimsum_causal_conv1d_update_slots", "dimsum_selective_state_update_slots", "dimsum_decode_linear_slots", "dimsum_state_copy_slots",
    "dimsum_causal_conv1d_cl_fwd", "dimsum_causal_conv1d_cl_bwd",
    "dimsum_norm_fwd", "dimsum_norm_bwd", "dimsum_token_transform", "dimsum_xattn_fusion_fwd", "dimsum_xattn_fusion_bwd",
    "dimsum_gated_gelu_fwd", "dimsum_gated_gelu_bwd", "dimsum_gated_gelu_fwd_split3", "dimsum_gated_gelu_bwd_split3", "dimsum_gated_gelu_bwd_pair", "dimsum_gated_gelu_bwd_f16s", "dimsum_split3", "dimsum_split3_t",
    "dimsum_gelu_fwd", "dimsum_gelu_bwd",
    "dimsum_moe_route_work_bytes", "dimsum_moe_route_fwd", "dimsum_moe_route_bwd", "dimsum_moe_permute", "dimsum_moe_combine_fwd",
    "dimsum_moe_combine_bwd", "dimsum_moe_act_fwd", "dimsum_moe_act_bwd", "dimsum_moe_gemm",
    "dimsum_moe_gemm_dgrad", "dimsum_moe_gemm_wgrad", "dimsum_moe_gemm_f16s", "dimsum_moe_permute_f16s", "dimsum_moe_act_fwd_f16s",
    "dimsum_gemm_nt", "dimsum_gemm_nt_kernel_for", "dimsum_gemm_tn", "dimsum_gemm_nn", "dimsum_row_factors", "dimsum_rows_block_f16s", "dimsum_rows_f16s", "dimsum_rows_f16s_multi",
)

_P = C.POINTER
# (symbol, restype, argtypes) of every function load() binds
_SIGNATURES = (
    [("dimsum_status_string", C.c_char_p, [C.c_int]), ("dimsum_target_arch", C.c_char_p, None), ("dimsum_abi_version", C.c_int, None),
     ("dimsum_event_create", vp, []), ("dimsum_event_destroy", None, [vp]), ("dimsum_event_elapsed_ms", C.c_float, [vp, vp])]
    # the launches that take one parameter struct and a stream
    + [(name, C.c_int, [_P(ptype), vp]) for name, ptype in (
        ("dimsum_ssm_scan_fwd", SsmParams), ("dimsum_ssm_scan_bwd", SsmBwdParams), ("dimsum_ssm_scan_bidir_fwd", SsmBidirParams),
        ("dimsum_ssm_scan_bidir_bwd", SsmBidirBwdParams), ("dimsum_optim_grad_sumsq", OptimParams), ("dimsum_optim_adamw_ema_step", OptimParams),
        ("dimsum_causal_conv1d_fwd", ConvParams), ("dimsum_causal_conv1d_bwd", ConvBwdParams), ("dimsum_norm_fwd", NormParams),
        ("dimsum_norm_bwd", NormBwdParams), ("dimsum_token_transform", TtParams), ("dimsum_xattn_fusion_fwd", XattnParams),
        ("dimsum_xattn_fusion_bwd", XattnBwdParams), ("dimsum_gemm_nt", GemmParams), ("dimsum_fm_plan", FmPlanParams),
        ("dimsum_fm_loss_fwd", FmLossParams), ("dimsum_fm_loss_bwd", FmLossParams), ("dimsum_pos_rope", PosRopeParams),
        ("dimsum_pos_cpe_fwd", PosCpeParams), ("dimsum_pos_cpe_bwd", PosCpeBwdParams), ("dimsum_einfft_dft", EinfftDftParams),
        ("dimsum_einfft_idft_real", EinfftDftParams), ("dimsum_einfft_mlp_fwd", EinfftMlpParams), ("dimsum_einfft_mlp_bwd", EinfftMlpBwdParams),
        ("dimsum_gelu_fwd", GeluParams), ("dimsum_gelu_bwd", GeluParams), ("dimsum_causal_conv1d_update", ConvUpdateParams),
        ("dimsum_selective_state_update", StateUpdateParams), ("dimsum_ssm_scan_general_fwd", SsmGeneralParams),
        ("dimsum_ssm_scan_general_bwd", SsmGeneralBwdParams), ("dimsum_moe_route_fwd", MoeRouteParams), ("dimsum_moe_route_bwd", MoeRouteParams),
        ("dimsum_moe_permute", MoeRowsParams), ("dimsum_moe_combine_fwd", MoeRowsParams), ("dimsum_moe_combine_bwd", MoeRowsParams),
        ("dimsum_moe_act_fwd", MoeActParams), ("dimsum_moe_act_bwd", MoeActParams), ("dimsum_moe_gemm", MoeGemmParams),
        ("dimsum_moe_gemm_dgrad", MoeGemmDgradParams), ("dimsum_moe_gemm_wgrad", MoeGemmWgradParams),
        ("dimsum_moe_gemm_f16s", MoeGemmF16sParams), ("dimsum_moe_permute_f16s", MoePermuteF16sParams), ("dimsum_moe_act_fwd_f16s", MoeActF16sParams),
        ("dimsum_causal_conv1d_cl_fwd", ConvClParams), ("dimsum_causal_conv1d_cl_bwd", ConvClBwdParams),
        ("dimsum_ssm_scan_carry_fwd", SsmCarryParams), ("dimsum_causal_conv1d_chunk", ConvChunkParams),
        ("dimsum_decode_linear", DecodeLinearParams), ("dimsum_cross_entropy_fwd", CrossEntropyParams),
        ("dimsum_cross_entropy_bwd", CrossEntropyParams), ("dimsum_sample_logits", SampleLogitsParams),
        ("dimsum_causal_conv1d_varlen_fwd", ConvVarlenParams), ("dimsum_causal_conv1d_varlen_bwd", ConvVarlenBwdParams),
        ("dimsum_ssm_scan_varlen_fwd", SsmVarlenParams), ("dimsum_ssm_scan_varlen_bwd", SsmVarlenBwdParams),
        ("dimsum_causal_conv1d_update_slots", ConvUpdateSlotsParams), ("dimsum_selective_state_update_slots", StateUpdateSlotsParams),
        ("dimsum_decode_linear_slots", DecodeLinearSlotsParams), ("dimsum_state_copy_slots", StateCopyParams),
        ("dimsum_causal_conv1d_varlen_states_fwd", ConvVarlenStatesParams), ("dimsum_ssm_scan_varlen_states_fwd", SsmVarlenStatesParams),
        ("dimsum_causal_conv1d_varlen_resume_fwd", ConvVarlenResumeParams), ("dimsum_ssm_scan_varlen_resume_fwd", SsmVarlenResumeParams))]
    # the gated-GeLU passes: n pointers, rows, cols, stream
    + [(name, C.c_int, [vp] * nptr + [i64, i64, vp]) for name, nptr in (
        ("dimsum_gated_gelu_fwd", 3), ("dimsum_gated_gelu_bwd", 5), ("dimsum_gated_gelu_fwd_split3", 3), ("dimsum_gated_gelu_bwd_split3", 5),
        ("dimsum_gated_gelu_bwd_pair", 5), ("dimsum_gated_gelu_bwd_f16s", 6))]
    + [("dimsum_optim_write_ptrs", C.c_int, [vp, i64, _P(vp), i32, vp]),
       ("dimsum_gemm_nt_kernel_for", C.c_int, [_P(GemmParams)]),
       ("dimsum_gemm_tn", C.c_int, [_P(GemmParams), i32, i64, vp]),
       ("dimsum_gemm_nn", C.c_int, [_P(GemmParams), i32, i64, vp]),
       ("dimsum_rows_block_f16s", C.c_int, [vp, i64, i64, i64, vp, i64, vp, i64, vp]),
       ("dimsum_row_factors", C.c_int, [vp, vp, i64, vp, vp, vp]),
       ("dimsum_split3", C.c_int, [vp, i64, i64, i64, vp, i32, vp]),
       ("dimsum_split3_t", C.c_int, [vp, i64, i64, i64, vp, vp]),
       ("dimsum_rows_f16s", C.c_int, [vp, i64, i64, i64, vp, i64, vp, vp, vp]),
       ("dimsum_rows_f16s_multi", C.c_int, [_P(F16sJob), i32, vp]),
       ("dimsum_moe_route_work_bytes", i64, [i64, i32]),
       ("dimsum_ssm_scan_bwd_workspace_bytes", i64, [i32] * 5),
       ("dimsum_ssm_scan_general_bwd_workspace_bytes", i64, [i32] * 6),
       ("dimsum_ssm_scan_fwd_variant", C.c_int, [_P(SsmParams)]),
       ("dimsum_ssm_scan_bidir_fwd_variant", C.c_int, [_P(SsmBidirParams)])])

_lib = None


def load():
    """Loads the HIP library. Raises RuntimeError (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"dimsum_amd: {LIB_PATH} not found. Build it with `python -c 'import __graft_entry__ as g; "
                           f"g.build()'` or `make -C dimsum_amd/csrc`. There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, restype, argtypes in _SIGNATURES:
        if hasattr(lib, name):               # a library that misses a symbol is an older ABI: the version check below says so
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    if lib.dimsum_abi_version() != 18:
        raise RuntimeError("dimsum_amd: libdimsum_hip.so ABI version mismatch; rebuild")
    _lib = lib
    return lib


GEMM_NT_KERNELS = {0: "gemm_nt_kernel<256 x 256 tiles>", 1: "gemm_nt_m128_kernel<128 x 256 tiles>", 2: "gemm_nt_persist_kernel"}   # dimsum_gemm_nt_kernel_for()
SCAN_FWD_KERNELS = {1: "ssm_scan_fwd_kernel", 2: "ssm_scan_fwd_split_kernel<2 lanes per channel>",
                    4: "ssm_scan_fwd_split_kernel<4 lanes per channel>",
                    16: "ssm_scan_fwd_lanes_kernel<one lane per state>"}      # dimsum_ssm_scan_fwd_variant() -> kernel


def check(status, what):
    if status != 0:
        raise RuntimeError(f"{what}: {load().dimsum_status_string(status).decode()} (status {status})")
