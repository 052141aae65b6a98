/*
 * dimsum_hip.h -- C ABI of libdimsum_hip.so: the MI355X (gfx950) native kernels of the DiMSUM denoiser hot path.
 *
 * This is the drop-in boundary. Each entry point replaces one function of the reference's two pybind extension
 * modules (or the Triton kernels it has no ROCm path for) and is what a reference-side FFI would bind:
 *
 *   dimsum_ssm_scan_fwd        <- selective_scan_cuda.fwd      mamba/csrc/selective_scan/selective_scan.cpp:226-336
 *   dimsum_ssm_scan_bwd        <- selective_scan_cuda.bwd      mamba/csrc/selective_scan/selective_scan.cpp:338-492
 *   dimsum_ssm_scan_bidir_fwd / _bwd <- the two selective_scan_cuda calls (+ flips) of BiMambaInnerFn  mamba/mamba_ssm/ops/selective_scan_interface.py:1010-1388
 *   dimsum_optim_grad_sumsq / dimsum_optim_adamw_ema_step <- clip_grad_norm_ + AdamW.step + update_ema   dimsum/train.py:55-64,317-321
 *   dimsum_fm_plan / dimsum_fm_loss_fwd / _bwd <- ICPlan.plan + DCTBlur, the loss of Transport.training_losses   dimsum/transport/path.py:159-259, transport.py:127-164
 *   dimsum_pos_rope / dimsum_pos_cpe_fwd / _bwd <- apply_rotary, AdaInPosCNN.forward (+ autograd)   dimsum/pe/my_rotary.py:63-72, pe/cpe.py:37-48
 *   dimsum_einfft_dft / _idft_real / _mlp_fwd / _mlp_bwd <- EinFFT.forward (+ autograd)   dimsum/models_dim.py:713-775
 *   dimsum_causal_conv1d_fwd   <- causal_conv1d_cuda.causal_conv1d_fwd[_cond]   causal-conv1d/csrc/causal_conv1d.cpp:221-336
 *   dimsum_causal_conv1d_bwd   <- causal_conv1d_cuda.causal_conv1d_bwd[_cond]   causal-conv1d/csrc/causal_conv1d.cpp:338-509
 *   dimsum_causal_conv1d_cl_fwd / _cl_bwd <- the same two entries on channel-last operands   causal-conv1d/csrc/causal_conv1d.cpp:242-247, 376-379
 *   dimsum_causal_conv1d_update <- causal_conv1d_cuda.causal_conv1d_update        causal-conv1d/csrc/causal_conv1d.cpp:512-569
 *   dimsum_selective_state_update <- selective_state_update (Triton)              mamba/mamba_ssm/ops/triton/selective_state_update.py:115-190
 *   dimsum_causal_conv1d_chunk / dimsum_ssm_scan_carry_fwd <- no counterpart: the conv and the scan entered with a cache's states, any number of tokens
 *   dimsum_norm_fwd / _bwd     <- _layer_norm_fwd / _layer_norm_bwd (Triton)     mamba/mamba_ssm/ops/triton/layernorm.py:120-364
 *   dimsum_token_transform     <- einops/flip/local_scan/DWT/DCT chains          dimsum/models_dim.py:572-604,656-705,876-928,1496-1524
 *   dimsum_xattn_fusion_fwd/_bwd <- F.scaled_dot_product_attention x2 (+ autograd)  dimsum/attention_fusion.py:44-75
 *   dimsum_gated_gelu_fwd/_bwd <- gelu_tanh(x1) * x2                             dimsum/mlp.py:66-70
 *   dimsum_gelu_fwd/_bwd       <- timm Mlp's act: gelu_tanh(fc1(x) + b)                  dimsum/models_dit.py:124
 *   dimsum_moe_*               <- SwitchMLP's routing, nonzero() gathers / scatters and exact-GELU experts  dimsum/switch_mlp.py:69-99, mlp.py:7-46
 *   dimsum_gemm_nt             <- nn.Linear / F.linear of the bias-free projections (cuBLAS TF32 GEMMs under train.py:20-21), and
 *                                 w12 + bias + gelu_tanh(x1) * x2 of the GatedMLP as ONE kernel    dimsum/mlp.py:49-70
 *
 * Conventions (same as the reference's host wrappers, minus ATen):
 *   - plain pointers, sizes and ELEMENT strides; no torch types. The caller allocates every output, including the
 *     zero-filled fp32 accumulators of the backward passes (selective_scan.cpp:458-466, causal_conv1d.cpp:405-407).
 *   - asynchronous on the hipStream_t passed in (`stream`, a `void*` so that plain C / ctypes can include this);
 *     no allocation, no synchronisation, no global state (the library has no mutable statics at all). Re-entrant.
 *   - return value: DIMSUM_OK or an error code; dimsum_status_string() gives the message the host layer raises
 *     (the reference raises RuntimeError from TORCH_CHECK at the same places).
 *   - innermost (sequence / feature) stride must be 1 for every activation tensor, like selective_scan.cpp:252-253.
 *
 * Versioning (ABI 18). Every parameter struct starts with `struct_size`: sizeof() of the struct AS THE CALLER COMPILED IT. An entry point
 * whose struct_size differs from the library's own sizeof returns DIMSUM_ERR_ABI before it reads anything else -- a caller built against an
 * older or newer header can never make a kernel read past its struct. (Inside the *_bwd_params_t structs only the outer struct_size is
 * checked; `fwd.struct_size` is ignored, `fwd.ext` is honoured.)
 * The two structs that mirror reference structs (dimsum_ssm_params_t <- SSMParamsBase, dimsum_gemm_params_t <- the arguments of F.linear)
 * hold ONLY the reference interface; everything this library offers beyond it (inference fusions, saved states, timing events, tuning)
 * lives behind `ext`, a pointer to a dimsum_*_ext_t that may be NULL (= the reference interface, nothing else). An ext struct carries its
 * own struct_size and only ever grows at its end: the library accepts any struct_size up to its own sizeof and reads the fields past the
 * caller's struct_size as 0 / NULL, so a new kernel option does not move the ABI version; an ext LARGER than the library's is
 * DIMSUM_ERR_ABI (the caller asks for something this library does not know).
 */
#ifndef DIMSUM_HIP_H
#define DIMSUM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DIMSUM_ABI_VERSION 18

typedef enum {
    DIMSUM_OK = 0,
    DIMSUM_ERR_NULL = 1,          /* a required pointer is NULL */
    DIMSUM_ERR_DTYPE = 2,         /* unsupported dtype code */
    DIMSUM_ERR_SHAPE = 3,         /* bad size (dstate, width, n_groups, ...) */
    DIMSUM_ERR_STRIDE = 4,        /* stride not supported (innermost != 1, overflow) */
    DIMSUM_ERR_UNSUPPORTED = 5,   /* valid in the reference but not served by THIS entry point (the tuned scan: complex A, constant B/C -> dimsum_ssm_scan_general_*; fusions a kernel does not offer) */
    DIMSUM_ERR_LAUNCH = 6,        /* hipGetLastError() after the launch */
    DIMSUM_ERR_ABI = 7,           /* struct_size of a parameter struct does not match this library (stale / foreign header) */
    DIMSUM_ERR_ALIAS = 8          /* an output overlaps an input that other workgroups still read (dimsum_decode_linear: residual_out) */
} dimsum_status_t;

typedef enum { DIMSUM_F32 = 0, DIMSUM_F16 = 1, DIMSUM_BF16 = 2 } dimsum_dtype_t;

const char *dimsum_status_string(int status);
int dimsum_abi_version(void);

/* Measurement helpers (benchmarks; no reference counterpart): HIP events (hipEvent_t behind void*) for the per-call
 * `timing_start_event` / `timing_stop_event` fields of dimsum_ssm_ext_t. Stateless wrappers of hipEventCreate / Destroy / ElapsedTime. */
void *dimsum_event_create(void);
void dimsum_event_destroy(void *event);
float dimsum_event_elapsed_ms(void *start_event, void *stop_event);   /* after the stream has been synchronised; < 0 on error */
/* name of the gfx target the kernels were compiled for ("gfx950") */
const char *dimsum_target_arch(void);

/* ---------------------------------------------------------------------------------------------------------------
 * Selective scan (Mamba S6), real A, input-dependent B and C.   Mirrors SSMParamsBase / SSMParamsBwd
 * (mamba/csrc/selective_scan/selective_scan.h:26-101). Shapes:
 *   u, delta, z, out, out_z, dout, du, ddelta, dz : (batch, dim, seqlen)      dtype `dtype`, innermost stride 1
 *   A : (dim, dstate) f32      D, delta_bias : (dim) f32 or NULL
 *   B, C : (batch, n_groups, dstate, seqlen)  dtype `dtype`, innermost stride 1
 *   x : (batch, dim, n_chunks, 2*dstate) f32 contiguous, n_chunks = ceil(seqlen/2048)   (selective_scan.cpp:307-313)
 *       x[...,2n] = running product of exp(delta*A_n), x[...,2n+1] = state h_n at the end of each 2048-chunk
 *   out   = C.h + D*u          out_z = out * silu(z)  (written iff z_ptr != NULL)
 * ------------------------------------------------------------------------------------------------------------- */
/* Everything beyond the reference interface (SSMParamsBase has none of it). All 0 / NULL by default; nothing here is process state. */
typedef struct {
    uint32_t struct_size;     /* sizeof(dimsum_ssm_ext_t) as the caller compiled it (see "Versioning" at the top) */
    int32_t kernel_variant;   /* forward kernel: 0 = automatic (dimsum_ssm_scan_fwd_variant tells which), else lanes per channel:
                                 1 (64 channels per wave), 2, 4, 16 (one lane per state; dstate 16). A variant the shape does
                                 not support (dstate % 4, % 8, != 16) falls back to 1. For tests and tuning. */
    void *ckpt_ptr;   /* optional (batch, ceil(seqlen/8), dstate, dim) f32: the state h BEFORE every 8th step.
                         forward: written when non-NULL (training callers keep it for the backward);
                         backward: read when non-NULL, otherwise rebuilt into workspace_ptr by one extra sweep.
                         Not part of the reference interface (its backward re-scans whole rows instead). */
    void *timing_start_event, *timing_stop_event;   /* optional hipEvent_t pair: recorded at the begin of the call's first kernel
                                 and the end of its last one (hipExtLaunchKernel: the kernels' own dispatch timestamps, the
                                 durations rocprofv3 reports). In dimsum_ssm_bwd_params_t.fwd they bracket the whole backward
                                 call incl. the state-rebuild sweep of a caller without ckpt_ptr. Not capturable into a hipGraph. */
    int64_t out_z_lo_offset;  /* forward, float32 I/O only; 0 = out_z is a `dtype` tensor (the reference's interface). != 0: out_z is written as
                                 its split-bf16 pair -- out_z_ptr = the bfloat16 `hi` plane (out_z_*_stride in bfloat16 elements), the `lo`
                                 plane lies out_z_lo_offset elements behind it; hi = bf16(x), lo = bf16(x - hi): the same 4 bytes per
                                 element (seqlen % 8 == 0), already the operand image of out_proj's GEMM (dimsum_gemm_tn with a_alias_rows), which then
                                 needs no conversion pass (mamba_simple.py:352-354 out_proj under allow_tf32). */
    /* Fused dt_proj (forward, inference, float32 I/O; no reference counterpart as a kernel: selective_scan_interface.py:840-841 computes
     * delta = dt_proj.weight @ x_dbl[:, :R]^T as a TF32 GEMM of its own and hands the (batch, dim, seqlen) result to the scan). With
     * dt_w_ptr != NULL the scan forms delta[b, d, t] = sum_r dt_w[d, r] * dt_x[r, b * seqlen + t] itself, tile by tile on the matrix
     * cores (three bf16 products per fp32 product: the arithmetic of the library GEMM it replaces), delta_ptr is NOT read (it may be
     * NULL) and the (batch, dim, seqlen) delta tensor never exists: one launch and 2 B D L 4 bytes of traffic less per mixer.
     * Served by the 64-channels-per-wave kernel on its full vector path (dim / n_groups % 64 == 0, z given, no ckpt_ptr); any other
     * call with dt_w_ptr set is DIMSUM_ERR_UNSUPPORTED (dimsum_ssm_scan_fwd_variant() == 1 tells the host beforehand). */
    const void *dt_w_ptr;     /* (dim, dt_rank) f32, 16-byte aligned rows, dt_rank % 4 == 0, dt_rank <= 32 */
    const void *dt_x_ptr;     /* (dt_rank, batch * seqlen) f32: the first dt_rank rows of x_proj's output written r-major (x_proj.weight @ conv_out
                                 as a (R + 2N, batch seqlen) matrix, the layout whose B / C rows the scan reads without a transposing copy) */
    int64_t dt_w_row_stride, dt_x_row_stride;     /* in elements; dt_w_row_stride % 4 == 0 */
    int32_t dt_rank;
    /* Block-scaled fp16 out_z (forward, inference, float32 I/O; same kernel path as dt_w_ptr): out_z_f16 != 0 -> out_z_ptr is a float16 buffer
     * (out_z_*_stride in float16 elements, rows 16-byte aligned, seqlen % 32 == 0): the 64 channels x 32 steps a wave finishes at a time are
     * stored as fp16(out_z * 2^s) with 2^-s (f32) at out_z_scale_ptr[((b * seqlen + t) / 32) * out_z_scale_ld + d / 64] -- the A operand of
     * out_proj as ONE fp16 product per element (dimsum_gemm_tn with a_block_inv_ptr): the reference multiplies out_z under TF32
     * (selective_scan_interface.py:954-981 under train.py:20-21), i.e. with 10-bit mantissas. */
    int32_t out_z_f16;
    void *out_z_scale_ptr;
    int64_t out_z_scale_ld;
} dimsum_ssm_ext_t;

/* The reference interface: field for field what set_ssm_params_fwd fills into SSMParamsBase (selective_scan.cpp:64-143;
 * selective_scan.h:26-68), plus the dtype code ATen carries in the tensors. `ext` = NULL is exactly that interface. */
typedef struct {
    uint32_t struct_size;     /* sizeof(dimsum_ssm_params_t) as the caller compiled it; anything else -> DIMSUM_ERR_ABI */
    int32_t batch, dim, seqlen, dstate, n_groups, n_chunks;
    int32_t delta_softplus;   /* bool */
    int32_t dtype;            /* dimsum_dtype_t of u/delta/z/B/C/out/out_z */
    int32_t reserved;         /* 0 */

    int64_t A_d_stride, A_dstate_stride;
    int64_t B_batch_stride, B_group_stride, B_dstate_stride;
    int64_t C_batch_stride, C_group_stride, C_dstate_stride;
    int64_t u_batch_stride, u_d_stride;
    int64_t delta_batch_stride, delta_d_stride;
    int64_t z_batch_stride, z_d_stride;
    int64_t out_batch_stride, out_d_stride;
    int64_t out_z_batch_stride, out_z_d_stride;

    const void *A_ptr, *B_ptr, *C_ptr, *D_ptr, *u_ptr, *delta_ptr, *delta_bias_ptr, *z_ptr;
    void *out_ptr;    /* may be NULL: inference-only callers that need just out_z skip the store */
    void *x_ptr;      /* may be NULL: skip the chunk-state store */
    void *out_z_ptr;  /* required iff z_ptr != NULL */
    const dimsum_ssm_ext_t *ext;   /* NULL = the reference interface */
} dimsum_ssm_params_t;

typedef struct {
    uint32_t struct_size;      /* sizeof(dimsum_ssm_bwd_params_t) */
    uint32_t reserved;         /* 0 */
    dimsum_ssm_params_t fwd;   /* forward operands (out_ptr = forward `out`, needed when z_ptr != NULL;
                                  out_z_ptr != NULL => recompute_out_z, selective_scan.cpp:443-449); fwd.ext->ckpt_ptr = the saved states */
    int64_t dout_batch_stride, dout_d_stride;
    int64_t dA_d_stride, dA_dstate_stride;
    int64_t dB_batch_stride, dB_group_stride, dB_dstate_stride;
    int64_t dC_batch_stride, dC_group_stride, dC_dstate_stride;
    int64_t du_batch_stride, du_d_stride;
    int64_t dz_batch_stride, dz_d_stride;
    int64_t ddelta_batch_stride, ddelta_d_stride;
    const void *dout_ptr;
    void *dA_ptr;          /* (dim, dstate) f32, zero-filled by the caller, accumulated with atomics */
    void *dB_ptr, *dC_ptr; /* (batch, n_groups, dstate, seqlen) F32 always; fully overwritten (no zero-fill needed): the
                              per-workgroup (64-channel) partial sums go through the workspace and are added in a fixed order */
    void *dD_ptr;          /* (dim) f32 zero-filled, or NULL */
    void *du_ptr, *dz_ptr, *ddelta_ptr;
    void *ddelta_bias_ptr; /* (dim) f32 zero-filled, or NULL */
    void *workspace_ptr;   /* scratch, 16-byte aligned, contents undefined on entry and exit:
                              per-workgroup partial dB / dC (2 * ceil(dim/64) * batch * dstate * seqlen f32) and, iff
                              fwd.ckpt_ptr == NULL, the rebuilt states. dimsum_ssm_scan_bwd_workspace_bytes(...) bytes
                              always suffice. */
    int64_t workspace_bytes;
} dimsum_ssm_bwd_params_t;

int dimsum_ssm_scan_fwd(const dimsum_ssm_params_t *p, void *stream);
int dimsum_ssm_scan_bwd(const dimsum_ssm_bwd_params_t *p, void *stream);
/* upper bound of the backward's workspace (partial dB / dC + rebuilt states) */
int64_t dimsum_ssm_scan_bwd_workspace_bytes(int32_t batch, int32_t dim, int32_t seqlen, int32_t dstate, int32_t n_groups);
/* Which forward kernel dimsum_ssm_scan_fwd launches for these parameters, p->kernel_variant included (a pure function of *p;
 * measurement / diagnostics; no reference counterpart: the reference has one kernel, selective_scan_fwd_kernel.cuh:67-303).
 * Lanes per channel:
 *   1 = ssm_scan_fwd_kernel        lane = channel, 64 channels per wave (launches that fill the chip)
 *   2 = ssm_scan_fwd_split_kernel  lane = (channel, state half), 32 channels per wave
 *   4 = ssm_scan_fwd_split_kernel  lane = (channel, state quarter), 16 channels per wave (few channels, long sequences)
 *  16 = ssm_scan_fwd_lanes_kernel  lane = (channel, state), 4 channels per wave, dstate 16 (fewer channels still)
 * -1 on invalid parameters. */
int dimsum_ssm_scan_fwd_variant(const dimsum_ssm_params_t *p);

/* Bidirectional selective scan (bimamba_inner_fn): a forward-time scan with A and a reversed-time scan with A_b over the SAME u, delta, B, C,
 * z, D, delta_bias, summed:  out_z = out * silu(z) + out_b * silu(z), where
 *   out[t]   = C_t.h_t + D u_t,   h_t = exp(dt_t A) h_{t-1} + dt_t B_t u_t
 *   out_b[t] = C_t.g_t + D u_t,   g_t = exp(dt_t A_b) g_{t+1} + dt_t B_t u_t      (D u counted once per direction, as the reference does)
 * No reversed copy of any operand is made: the reversed direction reads the forward layouts backwards. One out_z store per direction, the
 * second one adding to the first (fixed order). z is required; x_ptr must be NULL; the inference fusions of the extension struct: split-bf16 /
 * fp16 out_z, fused dt_proj, are DIMSUM_ERR_UNSUPPORTED; kernel_variant is ignored: see dimsum_ssm_scan_bidir_fwd_variant. */
typedef struct {
    uint32_t struct_size;      /* sizeof(dimsum_ssm_bidir_params_t) */
    uint32_t reserved;         /* 0 */
    dimsum_ssm_params_t fwd;   /* the shared operands + the forward direction: A_ptr = its A, out_ptr = its `out` (or NULL), out_z_ptr = the SUM;
                                  fwd.ext->ckpt_ptr = its saved states (or NULL). fwd.struct_size is ignored, fwd.ext is honoured */
    const void *A_b_ptr;       /* (dim, dstate) f32: A of the reversed direction */
    int64_t A_b_d_stride, A_b_dstate_stride;
    void *out_b_ptr;           /* the reversed direction's `out` in FORWARD time order (or NULL; training callers keep it for the backward) */
    int64_t out_b_batch_stride, out_b_d_stride;
    void *ckpt_b_ptr;          /* its saved states (or NULL): (batch, ceil(seqlen/8), dstate, dim) f32, indexed in REVERSED time */
} dimsum_ssm_bidir_params_t;

/* The matching backward. du, ddelta, dz, dB, dC, dD, ddelta_bias receive the sum over both directions (dB / dC fully overwritten, fixed
 * order: no atomics); dA and dA_b stay apart. bwd.fwd.out_z_ptr != NULL recomputes the summed out_z. Both directions' saved states are
 * required (bwd.fwd.ext->ckpt_ptr, ckpt_b_ptr); the workspace needs only the partial dB / dC part:
 * dimsum_ssm_scan_bwd_workspace_bytes(...) - batch * ceil(seqlen/8) * dstate * dim * 4 bytes. */
typedef struct {
    uint32_t struct_size;      /* sizeof(dimsum_ssm_bidir_bwd_params_t) */
    uint32_t reserved;         /* 0 */
    dimsum_ssm_bwd_params_t bwd;   /* as for dimsum_ssm_scan_bwd, forward direction (bwd.struct_size is ignored) */
    const void *A_b_ptr;
    int64_t A_b_d_stride, A_b_dstate_stride;
    const void *out_b_ptr;     /* the reversed direction's `out` of the forward call (forward time order) */
    int64_t out_b_batch_stride, out_b_d_stride;
    const void *ckpt_b_ptr;    /* the reversed direction's saved states of the forward call */
    void *dA_b_ptr;            /* (dim, dstate) f32, zero-filled by the caller, accumulated with atomics */
    int64_t dA_b_d_stride, dA_b_dstate_stride;
} dimsum_ssm_bidir_bwd_params_t;

int dimsum_ssm_scan_bidir_fwd(const dimsum_ssm_bidir_params_t *p, void *stream);
int dimsum_ssm_scan_bidir_bwd(const dimsum_ssm_bidir_bwd_params_t *p, void *stream);
/* which forward kernel serves both directions (lanes per channel, as dimsum_ssm_scan_fwd_variant; fwd.ext->kernel_variant honoured the same
 * way): 16 = one lane per state where that is the choice for the shape (dstate 16, launches far too small to fill the chip), else 1 = the
 * 64-channel kernel -- the state-split kernels have no reversed form; -1 on invalid parameters (a wrong struct_size included) */
int dimsum_ssm_scan_bidir_fwd_variant(const dimsum_ssm_bidir_params_t *p);

/* General selective scan: what selective_scan_cuda takes and the entry points above refuse -- any dstate in 1..256, constant B and / or C,
 * complex A (selective_scan.cpp:226-492; the axes of mamba/tests/ops/test_selective_scan.py). One kernel family (csrc/ssm_scan_general.hip),
 * none of the extensions of dimsum_ssm_ext_t. The entry points above are unchanged: they keep refusing these calls. Shapes as above, and
 *   A : (dim, dstate) f32, or complex64 when is_complex (strides in elements of A's type: a complex element is a float pair)
 *   B, C input-dependent (is_variable_* != 0): (batch, n_groups, dstate, seqlen) of `dtype`; with is_complex (batch, n_groups, dstate,
 *       2 * seqlen): real and imaginary part interleaved along the last axis, as selective_scan_ref reads them (:131-134)
 *   B, C constant (is_variable_* == 0): (dim, dstate) f32 / complex64 like A; *_d_stride and *_dstate_stride in elements of that type.
 *       Both constant => n_groups must be 1.
 *   x : (batch, dim, n_chunks, 2 * dstate) f32 / complex64: [2n] = running product of exp(delta A_n), [2n + 1] = state h_n
 *   out = sum_n C h + D u; with is_complex out = 2 Re(sum_n C h) + D u -- the reference's convention (selective_scan_ref :163-164, its
 *   kernel likewise): a complex state stands for itself and its conjugate. batch <= 65535.
 * Checks, in this order: NULL struct / struct_size (DIMSUM_ERR_ABI) / required pointers / shape / dtype / negative strides or a
 * misaligned x (DIMSUM_ERR_STRIDE); the backward then its own pointers, strides, workspace alignment and size (DIMSUM_ERR_SHAPE). */
typedef struct {
    uint32_t struct_size;     /* sizeof(dimsum_ssm_general_params_t) */
    int32_t batch, dim, seqlen, dstate, n_groups, n_chunks;
    int32_t delta_softplus;   /* bool */
    int32_t dtype;            /* dimsum_dtype_t of u / delta / z / out / out_z and of input-dependent B / C */
    int32_t is_variable_B, is_variable_C;   /* SSMParamsBase::is_variable_B / is_variable_C */
    int32_t is_complex;       /* weight_t of the reference is complex: A (and constant B / C) complex64 */
    int32_t reserved;         /* 0 */

    int64_t A_d_stride, A_dstate_stride;
    int64_t B_batch_stride, B_d_stride, B_group_stride, B_dstate_stride;   /* batch / group: input-dependent; d: constant */
    int64_t C_batch_stride, C_d_stride, C_group_stride, C_dstate_stride;
    int64_t u_batch_stride, u_d_stride;
    int64_t delta_batch_stride, delta_d_stride;
    int64_t z_batch_stride, z_d_stride;
    int64_t out_batch_stride, out_d_stride;
    int64_t out_z_batch_stride, out_z_d_stride;

    const void *A_ptr, *B_ptr, *C_ptr, *D_ptr, *u_ptr, *delta_ptr, *delta_bias_ptr, *z_ptr;
    void *out_ptr;    /* may be NULL in the forward */
    void *x_ptr;      /* may be NULL */
    void *out_z_ptr;  /* forward: required iff z_ptr != NULL; the backward does not recompute out_z */
} dimsum_ssm_general_params_t;

/* The backward. du, ddelta, dz are fully written. Everything summed over channels, batch or time -- dA (complex64 with is_complex), dB, dC,
 * dD, ddelta_bias -- is ADDED with fp32 atomics into buffers the caller zero-fills: the result is not bit-repeatable between two launches.
 *   input-dependent dB / dC : (batch, n_groups, dstate, seqlen) f32 always (2 * seqlen with is_complex), summed over a group's channels
 *   constant dB / dC        : (dim, dstate) f32 / complex64, summed over batch and time
 * Complex gradients are torch.autograd's (dL/dRe + i dL/dIm). fwd.out_ptr = the forward's `out`, required with z. */
typedef struct {
    uint32_t struct_size;      /* sizeof(dimsum_ssm_general_bwd_params_t) */
    uint32_t reserved;         /* 0 */
    dimsum_ssm_general_params_t fwd;   /* fwd.struct_size is ignored */
    int64_t dout_batch_stride, dout_d_stride;
    int64_t dA_d_stride, dA_dstate_stride;
    int64_t dB_batch_stride, dB_d_stride, dB_group_stride, dB_dstate_stride;
    int64_t dC_batch_stride, dC_d_stride, dC_group_stride, dC_dstate_stride;
    int64_t du_batch_stride, du_d_stride;
    int64_t dz_batch_stride, dz_d_stride;
    int64_t ddelta_batch_stride, ddelta_d_stride;
    const void *dout_ptr;
    void *dA_ptr, *dB_ptr, *dC_ptr;
    void *dD_ptr;              /* (dim) f32 zero-filled, or NULL */
    void *du_ptr, *dz_ptr, *ddelta_ptr;
    void *ddelta_bias_ptr;     /* (dim) f32 zero-filled, or NULL */
    void *workspace_ptr;       /* scratch, 16-byte aligned: the states before every tile of the sequence, rebuilt by the kernel's own forward
                                  sweep; dimsum_ssm_scan_general_bwd_workspace_bytes(...) bytes */
    int64_t workspace_bytes;
} dimsum_ssm_general_bwd_params_t;

int dimsum_ssm_scan_general_fwd(const dimsum_ssm_general_params_t *p, void *stream);
int dimsum_ssm_scan_general_bwd(const dimsum_ssm_general_bwd_params_t *p, void *stream);
/* the backward's workspace; -1 on an invalid shape */
int64_t dimsum_ssm_scan_general_bwd_workspace_bytes(int32_t batch, int32_t dim, int32_t seqlen, int32_t dstate, int32_t n_groups, int32_t is_complex);

/* The general forward on a CARRIED state (inference only, no backward): the scan enters with h0 instead of zeros and leaves the state after
 * the last step in hT -- a cached sequence continued by any number of tokens (no reference counterpart: selective_scan_cuda.fwd hands a
 * state out through x and takes none in). `scan` is read exactly as dimsum_ssm_scan_general_fwd reads it (scan.struct_size is ignored); with
 * h0_ptr == hT_ptr == NULL the launch IS that entry point's, bit for bit.
 *   h0, hT : (batch, dim, dstate), each with its own three ELEMENT strides (a slice of a larger cache is a view). `state_dtype` is
 *       DIMSUM_F32 or == scan.dtype -- the rule of dimsum_selective_state_update; with scan.is_complex the state is complex64 (a float pair
 *       per element, strides in complex elements) and state_dtype must be DIMSUM_F32. h0_ptr NULL = start from zero; hT_ptr NULL = not wanted.
 *   In place: hT_ptr may EQUAL h0_ptr with equal strides (a cache updated in place). The lane that owns (channel, state) reads its h0
 *       element before it walks the sequence and writes its hT element after it, and no other lane touches that element. Any other overlap
 *       of the two is undefined.
 *   Arithmetic is fp32 throughout: a 16-bit state is widened on load and rounded once, on the store.
 *   x keeps its meaning: [2n] = the running product of exp(delta A_n) counted from THIS call's first step, [2n + 1] = the state h_n, which
 *       includes what h0 carried in.
 * Checks, in the order of the general entry points: NULL struct / struct_size (DIMSUM_ERR_ABI) / required pointers / shape / dtype (scan.dtype,
 * then state_dtype where a state pointer is set: DIMSUM_ERR_DTYPE) / negative strides, the state's included, or a misaligned x
 * (DIMSUM_ERR_STRIDE). Nothing is launched before all of them pass. */
typedef struct {
    uint32_t struct_size;     /* sizeof(dimsum_ssm_carry_params_t) */
    int32_t state_dtype;      /* dimsum_dtype_t of h0 / hT */
    dimsum_ssm_general_params_t scan;
    int64_t h0_batch_stride, h0_d_stride, h0_dstate_stride;
    int64_t hT_batch_stride, hT_d_stride, hT_dstate_stride;
    const void *h0_ptr;       /* NULL = zero */
    void *hT_ptr;             /* NULL = not wanted; may equal h0_ptr */
} dimsum_ssm_carry_params_t;

int dimsum_ssm_scan_carry_fwd(const dimsum_ssm_carry_params_t *p, void *stream);

/* The general scan on PACKED rows (upstream Mamba's seq_idx; see dimsum_conv_varlen_params_t for seq_idx and what a boundary is). With
 * r_t = 1 at a boundary and 0 elsewhere:
 *     h_t = (1 - r_t) exp(dt_t A) h_{t-1} + dt_t B_t u_t        (the state restarts; h_{t-1} is dropped by a select, not multiplied by 0)
 *   and everything else as dimsum_ssm_scan_general_fwd: the last chunk's x holds h_{L-1}, the state of the row's last segment; the running
 *   product in x is 0 from the row's first boundary on. Backward: g_t = C_t dy_t + (1 - r_{t+1}) a_{t+1} g_{t+1}; the dA and ddelta terms
 *   through a_t h_{t-1} vanish at a boundary (masked explicitly).
 * Real A with input-dependent B and C only (any dstate in 1..256, n_groups, every dtype): complex A or a constant B / C is
 * DIMSUM_ERR_UNSUPPORTED. There is no carried-state form. `scan` / `bwd` are read exactly as the general entry points read them (their
 * struct_size is ignored); the backward's workspace is dimsum_ssm_scan_general_bwd_workspace_bytes(...).
 * Checks: NULL struct / struct_size (DIMSUM_ERR_ABI) / the general entry point's checks in their order / seq_idx_ptr NULL (DIMSUM_ERR_NULL) /
 * a negative seq_idx_batch_stride or one below seqlen with batch > 1 (DIMSUM_ERR_STRIDE) / complex A or constant B / C. */
typedef struct {
    uint32_t struct_size;     /* sizeof(dimsum_ssm_varlen_params_t) */
    uint32_t reserved;        /* 0 */
    dimsum_ssm_general_params_t scan;
    const void *seq_idx_ptr;
    int64_t seq_idx_batch_stride;
} dimsum_ssm_varlen_params_t;

typedef struct {
    uint32_t struct_size;     /* sizeof(dimsum_ssm_varlen_bwd_params_t) */
    uint32_t reserved;        /* 0 */
    dimsum_ssm_general_bwd_params_t bwd;
    const void *seq_idx_ptr;
    int64_t seq_idx_batch_stride;
} dimsum_ssm_varlen_bwd_params_t;

int dimsum_ssm_scan_varlen_fwd(const dimsum_ssm_varlen_params_t *p, void *stream);
int dimsum_ssm_scan_varlen_bwd(const dimsum_ssm_varlen_bwd_params_t *p, void *stream);

/* dimsum_ssm_scan_varlen_fwd that also leaves PER-SEGMENT states in a pool (forward only; see dimsum_conv_varlen_states_params_t for
 * end_slots and the caller's contract): where end_slots[b, t] = s >= 0 the state h_t -- the value step t + 1 would read -- is stored to
 * state[s, d, n] for every channel d and state n < dstate, by the one lane that holds it. `state` is (num_slots, dim, dstate) with three
 * free ELEMENT strides, float32 (state_f32 != 0) or of scan.dtype (rounded once, on the store, as hT of dimsum_ssm_scan_carry_fwd).
 * out, out_z, x and the last chunk's state are exactly what dimsum_ssm_scan_varlen_fwd gives on the same inputs.
 * Checks, in this order: NULL struct / struct_size (DIMSUM_ERR_ABI, before anything else is read) / num_slots < 1 (DIMSUM_ERR_SHAPE) /
 * end_slots_ptr or state_ptr NULL (DIMSUM_ERR_NULL) / a negative end_slots_batch_stride or one below seqlen with batch > 1, or a negative
 * state stride (DIMSUM_ERR_STRIDE) / dimsum_ssm_scan_varlen_fwd's checks on the embedded struct in their order (its struct_size is ignored).
 * Nothing is launched, allocated or synchronised before all of them pass. One launch. */
typedef struct {
    uint32_t struct_size;     /* sizeof(dimsum_ssm_varlen_states_params_t) */
    int32_t num_slots;        /* rows of the pool, >= 1 */
    dimsum_ssm_varlen_params_t varlen;
    const void *end_slots_ptr;        /* int32 (batch, seqlen), unit stride along seqlen */
    int64_t end_slots_batch_stride;
    void *state_ptr;
    int64_t state_slot_stride, state_d_stride, state_dstate_stride;
    int32_t state_f32;        /* != 0: the pool is float32; 0: of scan.dtype */
    int32_t reserved;         /* 0 */
} dimsum_ssm_varlen_states_params_t;

int dimsum_ssm_scan_varlen_states_fwd(const dimsum_ssm_varlen_states_params_t *p, void *stream);

/* dimsum_ssm_scan_varlen_states_fwd whose segments may CONTINUE a stored state (forward only; see dimsum_conv_varlen_resume_params_t for
 * start_slots): where start_slots[b, t] = s >= 0 the state entering position t is init[s, d, n] where the plain entry uses 0 -- at a
 * boundary, and at t = 0. `init` is (n_init, dim, dstate) with three free ELEMENT strides, float32 (init_f32 != 0) or of scan.dtype.
 * init MAY BE the pool `states.state_ptr` stores into: each (channel, state) element is loaded, at the segment's first step, and stored, at
 * the segment's end, by ONE lane in its own program order. For that to hold a slot stored in this launch may be read only by the segment
 * that stores it (the caller's contract, not checked).
 * Checks, in this order: NULL struct / struct_size (DIMSUM_ERR_ABI) / n_init < 1 (DIMSUM_ERR_SHAPE) / start_slots_ptr or init_ptr NULL
 * (DIMSUM_ERR_NULL) / a negative start_slots_batch_stride or one below seqlen with batch > 1, or a negative init stride (DIMSUM_ERR_STRIDE) /
 * dimsum_ssm_scan_varlen_states_fwd's checks on the embedded struct in their order (its struct_size is ignored). Nothing is launched,
 * allocated or synchronised before all of them pass. One launch. */
typedef struct {
    uint32_t struct_size;     /* sizeof(dimsum_ssm_varlen_resume_params_t) */
    int32_t n_init;           /* rows of init, >= 1 */
    dimsum_ssm_varlen_states_params_t states;
    const void *start_slots_ptr;      /* int32 (batch, seqlen), unit stride along seqlen */
    int64_t start_slots_batch_stride;
    const void *init_ptr;
    int64_t init_slot_stride, init_d_stride, init_dstate_stride;
    int32_t init_f32;         /* != 0: init is float32; 0: of scan.dtype */
    int32_t reserved;         /* 0 */
} dimsum_ssm_varlen_resume_params_t;

int dimsum_ssm_scan_varlen_resume_fwd(const dimsum_ssm_varlen_resume_params_t *p, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Training-step tail: global gradient-norm clip + AdamW + parameter EMA over a list of fp32 tensors, two launches
 * (<- torch.nn.utils.clip_grad_norm_, torch.optim.AdamW.step and update_ema of dimsum/train.py:55-64,317-321).
 * Added under ABI 18 (new symbols only). One struct serves both calls. Everything it points to is DEVICE memory:
 *   p_ptrs, g_ptrs, m_ptrs, v_ptrs, ema_ptrs, step_ptrs : n_tensors pointers each (tensor t: contiguous fp32 of numel[t] elements at any
 *       4-byte-aligned address; step_ptrs[t]: ONE fp32, the count of updates so far -- torch's fused AdamW state layout)
 *       g_ptrs[t] NULL: tensor t takes no part in the norm, p / m / v / step stay untouched (m / v / step pointers may be NULL), only the EMA blends.
 *       ema_ptrs NULL, or ema_ptrs[t] NULL: no EMA (for that tensor).
 *   numel       : n_tensors int64
 *   chunk_table : n_chunks pairs of int32 (tensor index, chunk number c within that tensor): elements [c, c + 1) * DIMSUM_OPTIM_CHUNK of the tensor.
 *       One workgroup works on one chunk at a time, chunk i on workgroup i % grid: the order of every sum is a function of the tables alone
 *       (not of addresses or alignment), so equal gradients give bit-equal norms on every run and every rank.
 *   partials    : n_partials floats (1 .. DIMSUM_OPTIM_MAX_PARTIALS), written by dimsum_optim_grad_sumsq (one per workgroup), read by the step
 *   total_norm  : one float (or NULL), written by the step: sqrt of the sum of squares of all gradients
 * dimsum_optim_grad_sumsq: partials[w] = workgroup w's share of sum g^2, and step[t] += 1 for every tensor with a gradient (one lane per tensor:
 *   the step kernel only reads the counters). partials NULL: only the counters advance (a step without norm).
 * dimsum_optim_adamw_ema_step, with clip = min(1, max_norm / (total_norm + 1e-6)) (max_norm <= 0 or partials NULL: 1), g' = clip g, t = step[tensor]:
 *   p = p (1 - lr weight_decay);  m = beta1 m + (1 - beta1) g';  v = beta2 v + (1 - beta2) g'^2
 *   p = p - lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps);  ema = ema_decay ema + (1 - ema_decay) p
 *   g is only read. A NaN norm makes clip NaN (torch's clip_grad_norm_ with error_if_nonfinite=False).
 * ------------------------------------------------------------------------------------------------------------- */
#define DIMSUM_OPTIM_CHUNK 4096
#define DIMSUM_OPTIM_MAX_PARTIALS 2048
typedef struct {
    uint32_t struct_size;      /* sizeof(dimsum_optim_params_t) */
    int32_t n_tensors;
    int32_t n_chunks;
    int32_t n_partials;
    const void *p_ptrs, *g_ptrs, *m_ptrs, *v_ptrs, *ema_ptrs, *step_ptrs;
    const void *numel;
    const void *chunk_table;
    void *partials;
    void *total_norm;
    double lr, beta1, beta2, eps, weight_decay;
    double max_norm;           /* <= 0: no clipping */
    double ema_decay;
    int64_t reserved[4];       /* 0 */
} dimsum_optim_params_t;

int dimsum_optim_grad_sumsq(const dimsum_optim_params_t *p, void *stream);
int dimsum_optim_adamw_ema_step(const dimsum_optim_params_t *p, void *stream);
/* dst_table[first + i] = src[i], i < count: `src` is HOST memory, read before the call returns (the values travel as kernel arguments,
 * DIMSUM_OPTIM_PTRS_PER_LAUNCH per launch), the writes are ordered on `stream` like any kernel -- how a caller refreshes g_ptrs every step
 * (autograd allocates new gradients) without a synchronisation or a staging buffer that a later step could overwrite too early. */
#define DIMSUM_OPTIM_PTRS_PER_LAUNCH 448
int dimsum_optim_write_ptrs(void *dst_table, int64_t first, const void *const *src, int32_t count, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Training-step head: the interpolation plan of the flow-matching transport with the optional DCT blur of the data, and the per-sample
 * loss with its gradient (<- ICPlan.plan + DCTBlur  dimsum/transport/path.py:159-188,249-259 and the three loss expressions of
 * Transport.training_losses  dimsum/transport/transport.py:127-164). Added under ABI 18 (new symbols only). fp32 only, no atomics, no
 * synchronisation; the caller allocates every output.
 *
 * dimsum_fm_plan, one launch. x1: (batch, channels, height, width), innermost three dimensions contiguous, x1_batch_stride elements
 * between samples (a batch-strided view); x0, xt, ut: contiguous tensors of the same shape. coef: (5, batch) contiguous, rows alpha, sigma,
 * d_alpha, d_sigma, blur_t (= blur_sigma^2 / 2) -- the path's formulas stay with the caller.
 *   xt = alpha_b * B(x1) + sigma_b * x0        ut = d_alpha_b * x1 + d_sigma_b * x0        (ut from the UNBLURRED x1, like the reference)
 *   patch == 0: B is the identity (the blur_t row is not read). patch in {2, 4, 8}: height == width, a multiple of patch; every patch x patch
 *   tile X of every channel becomes C^T (G_b o (C X C^T)) C, C the orthonormal patch-point DCT-II matrix,
 *   G_b[i][j] = exp(-(f_i^2 + f_j^2) blur_t_b) (1 - min_scale) + min_scale, f_k = pi k / patch. One tile per lane, in registers.
 *   x0 NULL: the sigma terms are left out (xt = alpha_b * B(x1): the blur alone with alpha = 1). ut NULL: not written.
 *   Each product is rounded before the sum (no contraction), so patch == 0 gives bit for bit what the expression gives in separate passes.
 *   Alignment: patch 4 and 8 read and write 16-byte vectors, patch 2 8-byte ones (base pointers and x1_batch_stride), else DIMSUM_ERR_STRIDE.
 *
 * dimsum_fm_loss_fwd / dimsum_fm_loss_bwd. out, tgt, dout: (batch, n) contiguous; w, c, gloss, loss: (batch); w or c NULL: 1; sign: +1 or -1.
 *   forward : loss_b = w_b * mean_i (c_b * out_i + sign * tgt_i)^2
 *   backward: dout_i = gloss_b * 2 * w_b * c_b * (c_b * out_i + sign * tgt_i) / n
 *   velocity prediction: c = 1, tgt = ut, sign = -1, w = 1; noise: c = 1, tgt = x0, sign = -1, w = weight; score: c = sigma_t, tgt = x0, sign = +1.
 *   One workgroup per sample. Lane l of the workgroup owns the elements [1024 k + 4 l, + 4), k = 0, 1, ..., whatever the alignment and the
 *   tail; the lanes of a wave are summed by a butterfly, the four waves in order through LDS: the order of every sum is a function of n
 *   alone, so equal inputs give bit-equal losses. n is arbitrary (1 <= n < 2^31).
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct {
    uint32_t struct_size;      /* sizeof(dimsum_fm_plan_params_t) */
    int32_t batch, channels, height, width;
    int32_t patch;             /* 0 (no blur), 2, 4 or 8 */
    float min_scale;           /* the floor of the blur's gain (the reference: 1e-3) */
    int32_t reserved;          /* 0 */
    int64_t x1_batch_stride;   /* elements */
    const void *x1, *x0, *coef;
    void *xt, *ut;
    int64_t reserved2[2];      /* 0 */
} dimsum_fm_plan_params_t;

typedef struct {
    uint32_t struct_size;      /* sizeof(dimsum_fm_loss_params_t) */
    int32_t batch;
    int64_t n;                 /* elements per sample */
    float sign;                /* +1 or -1 */
    int32_t reserved;          /* 0 */
    const void *out, *tgt, *w, *c;
    void *loss;                /* forward: written; backward: not read */
    const void *gloss;         /* backward: the gradient of each loss_b */
    void *dout;                /* backward: written */
    int64_t reserved2[2];      /* 0 */
} dimsum_fm_loss_params_t;

int dimsum_fm_plan(const dimsum_fm_plan_params_t *p, void *stream);
int dimsum_fm_loss_fwd(const dimsum_fm_loss_params_t *p, void *stream);
int dimsum_fm_loss_bwd(const dimsum_fm_loss_params_t *p, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Positional encodings of the embed pass: DiM(pe_type = "rope" | "cpe") (<- apply_rotary  dimsum/pe/my_rotary.py:63-72 and AdaInPosCNN.forward
 * dimsum/pe/cpe.py:37-48, as called at dimsum/models_dim.py:1815-1822). Added under ABI 18 (new symbols only). fp32 only; activations are
 * (batch, tokens, channels) with the channels contiguous, channels % 4 == 0, every pointer and stride 16-byte aligned; no allocation, no
 * synchronisation; the caller allocates every output, including the zero-filled accumulators of the backward.
 *
 * dimsum_pos_rope, one launch. sin, cos: (tokens, channels) contiguous.
 *   inverse == 0:  y[2i] = x[2i] cos[2i] - x[2i+1] sin[2i]         y[2i+1] = x[2i+1] cos[2i+1] + x[2i] sin[2i+1]      (x cos + rotate_half(x) sin)
 *   inverse != 0:  y[2i] = x[2i] cos[2i] + x[2i+1] sin[2i+1]       y[2i+1] = x[2i+1] cos[2i+1] - x[2i] sin[2i]        (its transpose)
 *   The transpose is the backward of the forward for ANY tables; for the rotary tables (sin and cos equal within a channel pair,
 *   sin^2 + cos^2 = 1) the map is a rotation, so the transpose is also its inverse: the flag is the sign of sin.
 *
 * dimsum_pos_cpe_fwd, one launch. tokens == grid * grid, token l = h * grid + w. weight: (channels, 3, 3) contiguous (nn.Conv2d's
 * (channels, 1, 3, 3) of a depthwise convolution), conv_bias, gamma, beta: (channels); shift, scale: (batch, channels) rows mod_batch_stride apart.
 *   v[b, l, c] = x[b, l, c] + conv_bias[c] + sum_{i, j} weight[c, i, j] x[b, (h + i - 1) grid + (w + j - 1), c]      (neighbours off the grid: 0)
 *   y = ((v - mean) rstd gamma + beta) (1 + scale[b]) + shift[b],   mean, rstd over the channels of the row, rstd = 1 / sqrt(var + eps)
 *   mean, rstd: (batch * tokens) each, written when non-NULL. v is written only when asked for (tests): the backward rebuilds it from x.
 *   A workgroup owns consecutive token rows of one batch element, a lane 4 adjacent channels: channels <= 2048.
 *
 * dimsum_pos_cpe_bwd, two launches. Reads x, dy, mean, rstd and the parameters of the forward.
 *   launch 1, per row: v again, the LayerNorm / modulation backward -> dv (written to dv, a (batch, tokens, channels) contiguous scratch tensor);
 *             dgamma, dbeta, dconv_bias (channels), dweight (channels, 3, 3), dshift, dscale (batch, channels; rows dmod_batch_stride apart) as
 *             fp32 atomic adds of per-workgroup partial sums into the caller's ZERO-FILLED tensors.
 *   launch 2, per row: dx = dv + conv^T(dv)     (dx contiguous)
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct {
    uint32_t struct_size;      /* sizeof(dimsum_pos_rope_params_t) */
    int32_t batch, tokens, channels;
    int32_t inverse;           /* 0: the forward, != 0: its transpose (= the backward, = the inverse rotation) */
    int32_t reserved;          /* 0 */
    int64_t x_batch_stride, x_token_stride, y_batch_stride, y_token_stride;   /* elements */
    const void *x, *sin, *cos;
    void *y;
    int64_t reserved2[2];      /* 0 */
} dimsum_pos_rope_params_t;

typedef struct {
    uint32_t struct_size;      /* sizeof(dimsum_pos_cpe_params_t) */
    int32_t batch, grid, channels;   /* tokens = grid * grid */
    float eps;
    int32_t reserved;          /* 0 */
    int64_t x_batch_stride, x_token_stride, y_batch_stride, y_token_stride, mod_batch_stride;   /* elements */
    const void *x, *weight, *conv_bias, *gamma, *beta, *shift, *scale;
    void *y, *mean, *rstd;     /* mean, rstd: forward written (optional), backward read */
    void *v;                   /* forward, optional (tests): v as a (batch, tokens, channels) contiguous tensor; the backward never reads it */
    int64_t reserved2[2];      /* 0 */
} dimsum_pos_cpe_params_t;

typedef struct {
    uint32_t struct_size;      /* sizeof(dimsum_pos_cpe_bwd_params_t) */
    uint32_t reserved;         /* 0 */
    dimsum_pos_cpe_params_t fwd;     /* the forward's operands; y is not read */
    int64_t dy_batch_stride, dy_token_stride, dmod_batch_stride;    /* elements */
    const void *dy;
    void *dv, *dx;             /* (batch, tokens, channels) contiguous: scratch of launch 1, the result */
    void *dweight, *dconv_bias, *dgamma, *dbeta, *dshift, *dscale;   /* zero-filled by the caller */
    int64_t reserved2[2];      /* 0 */
} dimsum_pos_cpe_bwd_params_t;

int dimsum_pos_rope(const dimsum_pos_rope_params_t *p, void *stream);
int dimsum_pos_cpe_fwd(const dimsum_pos_cpe_params_t *p, void *stream);
int dimsum_pos_cpe_bwd(const dimsum_pos_cpe_bwd_params_t *p, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The spectral branch of block type "combined_einfft" (<- EinFFT.forward  dimsum/models_dim.py:713-775 + autograd). Added under ABI 18 (new
 * symbols only). fp32 only, fp32 arithmetic; no allocation, no synchronisation. channels = 4 bs, channel c = k bs + j is column j of block k;
 * channels % 32 == 0 (bs % 8 == 0).
 *
 * dimsum_einfft_dft, one launch. x: real (batch, tokens, channels), channels contiguous, rows x_token_stride apart (a channel-half view is
 * read in place). re, im: the two planes of the spectrum, (batch, tokens, channels) contiguous each:
 *   (re + i im)[b, m, q bs + j] = (4 tokens)^-1/2 sum_{n, k} x[b, n, k bs + j] exp(-2 pi i (n m / tokens + k q / 4))
 *   tokens: a power of two in [16, 1024].
 * dimsum_einfft_idft_real, one launch, the same struct: reads re, im, WRITES x (any row stride >= channels):
 *   x[b, n, k bs + j] = Re (4 tokens)^-1/2 sum_{m, q} (re + i im)[b, m, q bs + j] exp(+2 pi i (n m / tokens + k q / 4))
 *   Each pass is the transpose of the other (the transform matrix is symmetric and unitary): the backward of one is the other.
 *
 * dimsum_einfft_mlp_fwd, one launch. xr, xi, zr, zi: (rows, channels) contiguous planes. w1, w2: (2, 4, bs, bs) = [re | im][block][in][out],
 * b1, b2: (2, 4, bs), all contiguous. Per row and block, with W = Wr + i Wi, b = br + i bi:
 *   h = relu(Re(x W1 + b1)) + i relu(Im(x W1 + b1)),  z = softshrink(Re(h W2 + b2), lambda) + i softshrink(Im(h W2 + b2), lambda)
 *   h never leaves the chip. bs <= 256.
 * dimsum_einfft_mlp_bwd, one launch. fwd: the forward's operands AND its output (zr, zi are read: softshrink passes the gradient exactly where
 * z != 0). w1t, w2t: the weights with the last two axes swapped, contiguous. dzr, dzi: the gradient of z. Written, all (rows, channels) planes:
 *   h1 = h again;  dz2 = dz where z != 0;  dp1 = (dz2 conj-transpose(W2)) where h > 0;  dx = dp1 conj-transpose(W1)
 *   The parameter gradients are products of these planes (dW2 = h1^T dz2, dW1 = x^T dp1 per block, in complex arithmetic) and the bias
 *   gradients their column sums: the caller's library GEMMs.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct {
    uint32_t struct_size;      /* sizeof(dimsum_einfft_dft_params_t) */
    int32_t batch, tokens, channels;
    int64_t x_batch_stride, x_token_stride;   /* elements */
    void *x;                   /* dft: read; idft_real: written */
    void *re, *im;             /* dft: written; idft_real: read */
    int64_t reserved2[2];      /* 0 */
} dimsum_einfft_dft_params_t;

typedef struct {
    uint32_t struct_size;      /* sizeof(dimsum_einfft_mlp_params_t) */
    int32_t channels;
    int64_t rows;
    float lam;                 /* softshrink threshold lambda, >= 0 */
    int32_t reserved;          /* 0 */
    const void *xr, *xi, *w1, *b1, *w2, *b2;
    void *zr, *zi;             /* forward: written; backward: read */
    int64_t reserved2[2];      /* 0 */
} dimsum_einfft_mlp_params_t;

typedef struct {
    uint32_t struct_size;      /* sizeof(dimsum_einfft_mlp_bwd_params_t) */
    uint32_t reserved;         /* 0 */
    dimsum_einfft_mlp_params_t fwd;
    const void *w1t, *w2t, *dzr, *dzi;
    void *dxr, *dxi, *h1r, *h1i, *dz2r, *dz2i, *dp1r, *dp1i;
    int64_t reserved2[2];      /* 0 */
} dimsum_einfft_mlp_bwd_params_t;

int dimsum_einfft_dft(const dimsum_einfft_dft_params_t *p, void *stream);
int dimsum_einfft_idft_real(const dimsum_einfft_dft_params_t *p, void *stream);
int dimsum_einfft_mlp_fwd(const dimsum_einfft_mlp_params_t *p, void *stream);
int dimsum_einfft_mlp_bwd(const dimsum_einfft_mlp_bwd_params_t *p, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Causal depthwise conv1d, width 2..4, optional bias, optional SiLU.  Mirrors ConvParamsBase / ConvParamsBwd
 * (causal-conv1d/csrc/causal_conv1d.h:9-52).  x, out, dout, dx : (batch, dim, seqlen) innermost stride 1.
 * weight (dim, width), bias (dim): f32.  dweight/dbias: f32 zero-filled by the caller (atomics across batch).
 * The reference's `_cond` entry points alias `out` to the caller's init_x buffer and are otherwise identical
 * (SURVEY finding 1): pass that buffer as out_ptr.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct {
    uint32_t struct_size;     /* sizeof(dimsum_conv_params_t) */
    int32_t batch, dim, seqlen, width;
    int32_t silu_activation;  /* bool */
    int32_t dtype;            /* of x/out */
    int32_t reserved;         /* 0 */
    int64_t x_batch_stride, x_c_stride;
    int64_t weight_c_stride, weight_width_stride;
    int64_t out_batch_stride, out_c_stride;
    const void *x_ptr, *weight_ptr, *bias_ptr;
    void *out_ptr;
} dimsum_conv_params_t;

typedef struct {
    uint32_t struct_size;     /* sizeof(dimsum_conv_bwd_params_t) */
    uint32_t reserved;        /* 0 */
    dimsum_conv_params_t fwd; /* out_ptr unused */
    int64_t dout_batch_stride, dout_c_stride;
    int64_t dx_batch_stride, dx_c_stride;
    int64_t dweight_c_stride, dweight_width_stride;
    const void *dout_ptr;
    void *dx_ptr, *dweight_ptr, *dbias_ptr;
} dimsum_conv_bwd_params_t;

int dimsum_causal_conv1d_fwd(const dimsum_conv_params_t *p, void *stream);
int dimsum_causal_conv1d_bwd(const dimsum_conv_bwd_params_t *p, void *stream);

/* The same conv on PACKED rows (upstream Mamba's seq_idx): several sequences share one (batch, seqlen) row and must not see each other.
 *   seq_idx : (batch, seqlen) int32, unit stride along seqlen, rows seq_idx_batch_stride ELEMENTS apart. Position t >= 1 of a row is a
 *       boundary iff seq_idx[b, t] != seq_idx[b, t - 1]; position 0 never is. The values are only compared with each other -- never an
 *       index or an offset: any int32 content is memory-safe.
 *   out[b, d, t] = act(bias[d] + sum_j W[d, width - 1 - j] x[b, d, t - j]) over the taps j with t - j >= 0 and no boundary in (t - j, t].
 *   Backward: dx[t] collects only from later positions of its own segment; dweight sums the unmasked (tap, position) pairs, dbias every
 *       position. A masked value is replaced by 0 (a select), so what lies beyond a boundary cannot reach a result whatever it holds.
 * `conv` is read exactly as dimsum_causal_conv1d_fwd / _bwd read it (conv.struct_size is ignored). Checks: NULL struct / struct_size
 * (DIMSUM_ERR_ABI) / the plain entry point's checks in their order / seq_idx_ptr NULL (DIMSUM_ERR_NULL) / a negative seq_idx_batch_stride or
 * one below seqlen with batch > 1 (DIMSUM_ERR_STRIDE). Only the seqlen-contiguous layout; the channel-last kernels take no seq_idx. */
typedef struct {
    uint32_t struct_size;     /* sizeof(dimsum_conv_varlen_params_t) */
    uint32_t reserved;        /* 0 */
    dimsum_conv_params_t conv;
    const void *seq_idx_ptr;
    int64_t seq_idx_batch_stride;
} dimsum_conv_varlen_params_t;

typedef struct {
    uint32_t struct_size;     /* sizeof(dimsum_conv_varlen_bwd_params_t) */
    uint32_t reserved;        /* 0 */
    dimsum_conv_bwd_params_t conv;
    const void *seq_idx_ptr;
    int64_t seq_idx_batch_stride;
} dimsum_conv_varlen_bwd_params_t;

int dimsum_causal_conv1d_varlen_fwd(const dimsum_conv_varlen_params_t *p, void *stream);
int dimsum_causal_conv1d_varlen_bwd(const dimsum_conv_varlen_bwd_params_t *p, void *stream);

/* dimsum_causal_conv1d_varlen_fwd that also leaves PER-SEGMENT conv states in a pool (forward only): one packed prompt pass over several
 * requests writes every request's state into that request's slot (the pool of the *_slots decode entries below).
 *   end_slots : (batch, seqlen) int32, unit stride along seqlen, rows end_slots_batch_stride ELEMENTS apart; it rides next to seq_idx.
 *       end_slots[b, t] = s >= 0: the state after position t of row b is stored into slot s. A negative entry stores nothing (padding, and
 *       every position that is not a segment's last). The contract does not depend on where the boundaries lie.
 *   state : (num_slots, dim, width) of conv.dtype (state_dtype, else DIMSUM_ERR_UNSUPPORTED), three free ELEMENT strides.
 *       state[s, d, width - 1 - j] = x[b, d, t - j] for the taps j < width with t - j >= 0 and no boundary in (t - j, t], else 0: the
 *       window dimsum_causal_conv1d_update shifts, zero-padded on the left for a segment shorter than width. The x elements are moved,
 *       not converted. out is exactly dimsum_causal_conv1d_varlen_fwd's.
 * THE CALLER'S CONTRACT (the one of the slot-indexed decode entries; not checkable without a device read, so not checked): every
 * non-negative entry is < num_slots, and no non-negative value appears twice in one launch. Both are undefined behaviour otherwise.
 * Checks, in this order: NULL struct / struct_size (DIMSUM_ERR_ABI, before anything else is read) / num_slots < 1 (DIMSUM_ERR_SHAPE) /
 * end_slots_ptr or state_ptr NULL (DIMSUM_ERR_NULL) / a negative end_slots_batch_stride or one below seqlen with batch > 1, or a negative
 * state stride (DIMSUM_ERR_STRIDE) / dimsum_causal_conv1d_varlen_fwd's checks on the embedded struct in their order (its struct_size is
 * ignored) / state_dtype != conv.dtype (DIMSUM_ERR_UNSUPPORTED). Nothing is launched, allocated or synchronised before all of them pass. */
typedef struct {
    uint32_t struct_size;     /* sizeof(dimsum_conv_varlen_states_params_t) */
    int32_t num_slots;        /* rows of the pool, >= 1 */
    dimsum_conv_varlen_params_t varlen;
    const void *end_slots_ptr;
    int64_t end_slots_batch_stride;
    void *state_ptr;
    int64_t state_slot_stride, state_c_stride, state_w_stride;
    int32_t state_dtype;      /* dimsum_dtype_t of the pool: must equal conv.dtype */
    int32_t reserved;         /* 0 */
} dimsum_conv_varlen_states_params_t;

int dimsum_causal_conv1d_varlen_states_fwd(const dimsum_conv_varlen_states_params_t *p, void *stream);

/* dimsum_causal_conv1d_varlen_states_fwd whose segments may CONTINUE a carried conv state (forward only): a long prompt fed in pieces.
 *   start_slots : (batch, seqlen) int32 laid out like end_slots. start_slots[b, t] = s >= 0 is allowed only where t is the first position
 *       of a segment (t == 0 or seq_idx[b, t] != seq_idx[b, t - 1]): the segment beginning at t continues init[s]. A negative entry is
 *       the plain entry's behaviour (zero state, dropped taps). A non-negative entry anywhere else, or one >= n_init, is undefined
 *       behaviour (not checked: it would take a device read).
 *   init : (n_init, dim, width) of conv.dtype (init_dtype, else DIMSUM_ERR_UNSUPPORTED), three free ELEMENT strides: the last `width`
 *       inputs of the earlier piece, newest last. Every tap of an output in [t, t + width - 2] that reaches before t reads
 *       x[t - k] := init[s, d, width - k] where the plain entry uses 0, and a state stored through end_slots is the last `width` values of
 *       concat(init[s], the segment) (the carried values shift left in a segment shorter than width - 1). The elements are moved, not
 *       converted. init MUST NOT OVERLAP a slot of the pool that this launch stores: different lanes (and, in a long row, different loop
 *       steps) read and write one slot (the caller's contract; the Python operator compares the storage ranges).
 * Checks, in this order: NULL struct / struct_size (DIMSUM_ERR_ABI) / n_init < 1 (DIMSUM_ERR_SHAPE) / start_slots_ptr or init_ptr NULL
 * (DIMSUM_ERR_NULL) / a negative start_slots_batch_stride or one below seqlen with batch > 1, or a negative init stride (DIMSUM_ERR_STRIDE) /
 * dimsum_causal_conv1d_varlen_states_fwd's checks on the embedded struct in their order (its struct_size is ignored) / init_dtype !=
 * conv.dtype (DIMSUM_ERR_UNSUPPORTED). Nothing is launched, allocated or synchronised before all of them pass. */
typedef struct {
    uint32_t struct_size;     /* sizeof(dimsum_conv_varlen_resume_params_t) */
    int32_t n_init;           /* rows of init, >= 1 */
    dimsum_conv_varlen_states_params_t states;
    const void *start_slots_ptr;
    int64_t start_slots_batch_stride;
    const void *init_ptr;
    int64_t init_slot_stride, init_c_stride, init_w_stride;
    int32_t init_dtype;       /* dimsum_dtype_t of init: must equal conv.dtype */
    int32_t reserved;         /* 0 */
} dimsum_conv_varlen_resume_params_t;

int dimsum_causal_conv1d_varlen_resume_fwd(const dimsum_conv_varlen_resume_params_t *p, void *stream);

/* The same conv on CHANNEL-LAST operands (causal_conv1d_channellast_fwd_kernel / _bwd_kernel, causal-conv1d/csrc/
 * causal_conv1d_fwd.cu:193-319, causal_conv1d_bwd.cu:306-494; host checks causal_conv1d.cpp:242-247, 376-379, 395-396):
 *   out[b, t, d] = act(bias[d] + sum_k W[d, k] * x[b, t - (width-1-k), d]),   x[.., t < 0, ..] = 0
 * x, out, dout, dx are addressed as (batch, seqlen, dim) with channel stride 1; every tensor has its own batch and token
 * ELEMENT strides (64-bit), so a channel slice of a wider buffer -- one half of a (batch, seqlen, 2 dim) xz -- is a view.
 * Any dim >= 1 and seqlen >= 1 (the reference's dim % 8 == 0 is not required): 16-byte accesses along the channels where
 * dim, the strides and the base pointers are multiples of 16 bytes, element accesses otherwise. batch == 0 launches
 * nothing. weight (dim, width), bias (dim): f32. dweight / dbias: f32, zero-filled by the caller, added to with atomics.
 * Checks in order: NULL struct, struct_size (DIMSUM_ERR_ABI), required pointers, width / sizes (DIMSUM_ERR_SHAPE), dtype,
 * negative strides (DIMSUM_ERR_STRIDE). Each chunk of DIMSUM_CONV_CL_CHUNK tokens is walked by one wave per 64 channel
 * vectors, its width - 1 halo rows re-read from memory. */
#define DIMSUM_CONV_CL_CHUNK 64

typedef struct {
    uint32_t struct_size;     /* sizeof(dimsum_conv_cl_params_t) */
    uint32_t reserved;        /* 0 */
    int32_t batch, dim, seqlen, width;
    int32_t silu_activation;  /* bool */
    int32_t dtype;            /* of x/out */
    int64_t x_batch_stride, x_l_stride;
    int64_t weight_c_stride, weight_width_stride;
    int64_t out_batch_stride, out_l_stride;
    const void *x_ptr, *weight_ptr, *bias_ptr;   /* bias_ptr may be NULL */
    void *out_ptr;
} dimsum_conv_cl_params_t;

typedef struct {
    uint32_t struct_size;     /* sizeof(dimsum_conv_cl_bwd_params_t) */
    uint32_t reserved;        /* 0 */
    dimsum_conv_cl_params_t fwd; /* out_ptr and the out strides unused */
    int64_t dout_batch_stride, dout_l_stride;
    int64_t dx_batch_stride, dx_l_stride;
    int64_t dweight_c_stride, dweight_width_stride;
    const void *dout_ptr;
    void *dx_ptr, *dweight_ptr, *dbias_ptr;      /* dbias_ptr may be NULL */
} dimsum_conv_cl_bwd_params_t;

int dimsum_causal_conv1d_cl_fwd(const dimsum_conv_cl_params_t *p, void *stream);
int dimsum_causal_conv1d_cl_bwd(const dimsum_conv_cl_bwd_params_t *p, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The recurrent (token by token) form of the mixer: one step of the causal conv1d and one step of the selective scan on
 * carried states, both updated IN PLACE. One work-item owns one (batch, channel) row; every dim of every tensor has its
 * own ELEMENT stride (cache slices, the two halves of a (batch, 2 dim) in_proj output and transposed caches are views).
 *
 * dimsum_causal_conv1d_update  <- causal_conv1d_cuda.causal_conv1d_update   causal-conv1d/csrc/causal_conv1d.cpp:512-569
 *   (semantics of causal_conv1d_update_ref, causal_conv1d_interface.py:79-100)
 *   conv_state (batch, dim, width) <- its last width - 1 columns, then x;   out = act(sum_w conv_state[.., w] weight[d, w] + bias[d])
 *   x, out (batch, dim) and conv_state share `dtype`; weight (dim, width), bias (dim) f32. The state written back holds the
 *   input values themselves (moved, never converted). width 2..4, else DIMSUM_ERR_SHAPE; batch or dim < 1: DIMSUM_ERR_SHAPE.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct {
    uint32_t struct_size;     /* sizeof(dimsum_conv_update_params_t) */
    int32_t batch, dim, width;
    int32_t silu_activation;  /* bool */
    int32_t dtype;            /* of x / conv_state / out */
    int32_t reserved[2];      /* 0 */
    int64_t x_batch_stride, x_c_stride;
    int64_t state_batch_stride, state_c_stride, state_w_stride;
    int64_t weight_c_stride, weight_width_stride;
    int64_t out_batch_stride, out_c_stride;
    const void *x_ptr, *weight_ptr, *bias_ptr;   /* bias_ptr may be NULL */
    void *conv_state_ptr, *out_ptr;
} dimsum_conv_update_params_t;

int dimsum_causal_conv1d_update(const dimsum_conv_update_params_t *p, void *stream);

/* dimsum_causal_conv1d_chunk: dimsum_causal_conv1d_update for any number of tokens per call (no reference counterpart: its update takes one
 * token, its sequence kernel starts from zeros). With v = concat(conv_state[b, d, 1:], x[b, d, :]):
 *     out[b, d, t] = act(bias[d] + sum_k weight[d, k] v[t + k]);   conv_state[b, d, :] <- the last `width` values of concat(conv_state, x)
 *   x, out (batch, dim, seqlen) of `dtype` with innermost stride 1 and free batch / channel strides (the d-major half of an in_proj output is
 *   a view); out must not overlap x. conv_state (batch, dim, width) of `dtype`, three free ELEMENT strides, updated IN PLACE: its values are
 *   moved, never converted (seqlen < width keeps the newest width - seqlen old ones in front of x; seqlen == 1 leaves exactly what
 *   dimsum_causal_conv1d_update leaves). weight (dim, width), bias (dim): f32; bias_ptr may be NULL.
 *   One wave owns whole (batch, channel) rows, as in the sequence kernel (csrc/causal_conv1d.hip): lane k < width reads conv_state[k] before
 *   the row is walked and the same lane writes it afterwards, so the in-place update cannot race. 16-byte accesses where seqlen, the strides
 *   and the bases of x and out allow, element accesses otherwise.
 * Checks in order: NULL struct, struct_size (DIMSUM_ERR_ABI), required pointers, width 2..4 / batch, dim, seqlen >= 1 (DIMSUM_ERR_SHAPE), dtype,
 * negative strides (DIMSUM_ERR_STRIDE). */
typedef struct {
    uint32_t struct_size;     /* sizeof(dimsum_conv_chunk_params_t) */
    int32_t batch, dim, seqlen, width;
    int32_t silu_activation;  /* bool */
    int32_t dtype;            /* of x / conv_state / out */
    int32_t reserved;         /* 0 */
    int64_t x_batch_stride, x_c_stride;
    int64_t state_batch_stride, state_c_stride, state_w_stride;
    int64_t weight_c_stride, weight_width_stride;
    int64_t out_batch_stride, out_c_stride;
    const void *x_ptr, *weight_ptr, *bias_ptr;   /* bias_ptr may be NULL */
    void *conv_state_ptr, *out_ptr;
} dimsum_conv_chunk_params_t;

int dimsum_causal_conv1d_chunk(const dimsum_conv_chunk_params_t *p, void *stream);

/* dimsum_selective_state_update  <- selective_state_update (Triton, no ROCm path)   mamba/mamba_ssm/ops/triton/selective_state_update.py:115-190
 *   (semantics of selective_state_update_ref, :193-228), f32 arithmetic throughout:
 *   dt' = dt + dt_bias, softplus(dt') when dt_softplus (threshold 20, as in the scan kernels)
 *   state (batch, dim, dstate) <- state exp(dt' A) + dt' B x;   out = sum_n state C + D x, times silu(z) when z is given
 *   x, dt, z, out (batch, dim): `dtype`. state: `state_dtype`, B, C (batch, dstate): `bc_dtype` -- each DIMSUM_F32 or == dtype.
 *   A (dim, dstate), D, dt_bias (dim): f32; D, z, dt_bias may be NULL. dstate 1..256, else DIMSUM_ERR_SHAPE.
 * The extension fuses dt_proj into the step (no reference counterpart as a kernel: Mamba.step computes F.linear(dt, dt_proj.weight) as a
 * GEMV launch of its own): with dt_w_ptr set, dt[b, d] = sum_r dt_w[d, r] dt_x[b, r] is formed here and dt_ptr is not read (may be NULL). */
typedef struct {
    uint32_t struct_size;     /* sizeof(dimsum_state_update_ext_t) as the caller compiled it (see "Versioning" at the top) */
    int32_t dt_rank;          /* >= 1 when dt_w_ptr is set */
    const void *dt_w_ptr;     /* (dim, dt_rank) f32 */
    const void *dt_x_ptr;     /* (batch, dt_rank), `dtype` */
    int64_t dt_w_d_stride, dt_w_r_stride, dt_x_batch_stride, dt_x_r_stride;
} dimsum_state_update_ext_t;

typedef struct {
    uint32_t struct_size;     /* sizeof(dimsum_state_update_params_t) as the caller compiled it; anything else -> DIMSUM_ERR_ABI */
    int32_t batch, dim, dstate;
    int32_t dt_softplus;      /* bool */
    int32_t dtype, state_dtype, bc_dtype;
    int64_t state_batch_stride, state_d_stride, state_n_stride;
    int64_t x_batch_stride, x_d_stride;
    int64_t dt_batch_stride, dt_d_stride;
    int64_t A_d_stride, A_n_stride;
    int64_t B_batch_stride, B_n_stride, C_batch_stride, C_n_stride;
    int64_t z_batch_stride, z_d_stride;
    int64_t out_batch_stride, out_d_stride;
    void *state_ptr;
    const void *x_ptr, *dt_ptr, *A_ptr, *B_ptr, *C_ptr, *D_ptr, *z_ptr, *dt_bias_ptr;
    void *out_ptr;
    const dimsum_state_update_ext_t *ext;   /* NULL = the reference interface */
} dimsum_state_update_params_t;

int dimsum_selective_state_update(const dimsum_state_update_params_t *p, void *stream);

/* dimsum_decode_linear: the weight-streaming linear layer of a decode step (no reference counterpart as a kernel: Mamba.step and Block.forward,
 * mamba_simple.py:299-344, :408-432, run a fused add + norm launch, F.linear GEMVs and causal_conv1d_update as launches of their own).
 *     y[b, n] = sum_k x'[b, k] W[n, k] (+ bias[n])      batch 1..16 (else DIMSUM_ERR_SHAPE), any n, k >= 1, fp32 accumulation
 *   x (batch, k), W (n, k), bias (n), y (batch, n): all of `dtype`, unit innermost stride, free row strides. W is read exactly once (16-byte
 *   streaming loads where its base and row stride allow, element loads otherwise and after the last whole piece of a row). No atomics and no
 *   split-K across workgroups: two launches from equal inputs are bit-identical.
 *   Prologue (norm != 0): r = x (+ residual); x' = norm(r) * norm_weight (+ norm_bias), rounded to `dtype` (what the unfused norm hands to
 *   the GEMV); norm 1 = LayerNorm, 2 = RMSNorm, statistics in fp32 on the unrounded r. residual, residual_out (batch, k): `residual_dtype`,
 *   DIMSUM_F32 or == dtype; norm_weight, norm_bias (k): `dtype`. residual_out = r is written by ONE workgroup while the others still read x
 *   and residual: a residual_out that overlaps either is DIMSUM_ERR_ALIAS. Without the prologue x' = x, and residual / residual_out /
 *   norm_bias must be NULL (DIMSUM_ERR_UNSUPPORTED).
 *   Epilogue (conv_dim > 0) on the outputs n < conv_dim: one step of dimsum_causal_conv1d_update by the lane that holds y[b, n]:
 *     conv_state[b, n, :] <- its last conv_width - 1 columns, then y[b, n] rounded to `dtype`;
 *     y[b, n] <- act(conv_bias[n] + sum_w conv_weight[n, w] conv_state[b, n, w]),  act = SiLU when silu_activation
 *   conv_state (batch, conv_dim, conv_width), conv_weight (conv_dim, conv_width), conv_bias (conv_dim): `dtype`, free ELEMENT strides; width 2..4.
 *   y is ONE (batch, n) buffer: with the epilogue its columns [0, conv_dim) hold the conv output and [conv_dim, n) the plain outputs (the
 *   mixer's x and z halves are views of it).
 * Checks, in this order: NULL struct / struct_size (DIMSUM_ERR_ABI) / required pointers (x, W, y; norm_weight with norm; conv_weight and
 * conv_state with conv_dim) / shape (batch, n, k, norm, conv_dim, conv_width) / dtype (dtype, then residual_dtype) / pointers that need the
 * prologue (DIMSUM_ERR_UNSUPPORTED) / negative strides (DIMSUM_ERR_STRIDE) / residual_out overlapping x, then residual (DIMSUM_ERR_ALIAS).
 * Nothing is launched before all of them pass. */
typedef struct {
    uint32_t struct_size;     /* sizeof(dimsum_decode_linear_params_t) as the caller compiled it; anything else -> DIMSUM_ERR_ABI */
    int32_t batch, n, k;
    int32_t dtype;            /* of x, W, bias, y, the norm and conv weights, conv_state */
    int32_t residual_dtype;   /* of residual / residual_out: DIMSUM_F32 or == dtype */
    int32_t norm;             /* 0: no prologue, 1: LayerNorm, 2: RMSNorm */
    int32_t conv_dim;         /* 0: no epilogue */
    int32_t conv_width;
    int32_t silu_activation;  /* bool */
    float eps;
    int32_t reserved;         /* 0 */
    int64_t x_row_stride, w_row_stride, y_row_stride, residual_row_stride, residual_out_row_stride;
    int64_t state_batch_stride, state_c_stride, state_w_stride, conv_weight_c_stride, conv_weight_width_stride;
    const void *x_ptr, *w_ptr, *bias_ptr, *residual_ptr, *norm_weight_ptr, *norm_bias_ptr, *conv_weight_ptr, *conv_bias_ptr;
    void *y_ptr, *residual_out_ptr, *conv_state_ptr;
} dimsum_decode_linear_params_t;

int dimsum_decode_linear(const dimsum_decode_linear_params_t *p, void *stream);

/* Slot-indexed states (upstream Mamba's conv_state_indices / state_batch_indices; no reference counterpart): the three launches of a decode
 * step that touch a carried state, on a POOL of states with a per-row slot index read on the device -- requests of different lengths share
 * one decode batch, and one captured graph serves every membership of it, because the host only rewrites a few ints between replays.
 *   slots : int32, one entry per batch row, slots_stride ELEMENTS apart (a device pointer; never read by the host).
 *   The state tensor of the embedded struct (conv.conv_state_ptr / update.state_ptr / linear.conv_state_ptr) is the pool
 *   (num_slots, dim, width | dstate) with the same three free ELEMENT strides as ever (its batch stride is the SLOT stride); num_slots is
 *   independent of batch. Row b reads and writes state[slots[b]] where the plain entry point addresses state[b]; every other operand
 *   (x, dt, z, B, C, dt_x, out, y) stays indexed by b. The arithmetic is the plain entry point's, expression by expression in the same
 *   order (the same device function, entered with another row address): on equal state rows the results are bit-identical. The 16-byte and
 *   element-walk predicates are evaluated on the pool: base alignment, unit inner stride, row and slot stride multiples of 4 elements.
 *   slots[b] < 0 is a PADDING row: no state element of any slot is read or written and the row's outputs are zeros -- out[b, :] of the two
 *   update entries; y[b, 0 : conv_dim) of dimsum_decode_linear_slots, whose plain columns y[b, conv_dim : n) are the GEMV of whatever x'
 *   held, written as ever. Everything downstream of a padding row stays finite without the host's help.
 * THE CALLER'S CONTRACT, which the host cannot check without a device read and therefore does not check: every slots[b] is < num_slots
 * (a larger one addresses memory outside the pool), and no non-negative slot is named by two rows of one launch (the two rows race on one
 * state). Both are undefined behaviour. dimsum_amd.utils.serving.DecodeEngine guarantees them by construction (a free list of slots).
 * Checks, in this order: NULL struct (DIMSUM_ERR_NULL) / struct_size (DIMSUM_ERR_ABI, before anything else is read) / num_slots < 1
 * (DIMSUM_ERR_SHAPE) / slots_ptr NULL (DIMSUM_ERR_NULL) / a negative slots_stride (DIMSUM_ERR_STRIDE) / then the plain entry point's checks
 * on the embedded struct in their order (its struct_size is ignored; its `ext` is honoured); dimsum_decode_linear_slots also wants
 * conv_dim > 0 (DIMSUM_ERR_UNSUPPORTED: without the epilogue there is no state to index). Nothing is launched before all of them pass; no
 * allocation, no synchronisation. One launch each, as the plain entry points. */
typedef struct {
    uint32_t struct_size;     /* sizeof(dimsum_conv_update_slots_params_t) */
    int32_t num_slots;        /* rows of the pool, >= 1 */
    dimsum_conv_update_params_t conv;
    const void *slots_ptr;    /* int32 (batch) */
    int64_t slots_stride;
} dimsum_conv_update_slots_params_t;

typedef struct {
    uint32_t struct_size;     /* sizeof(dimsum_state_update_slots_params_t) */
    int32_t num_slots;
    dimsum_state_update_params_t update;
    const void *slots_ptr;
    int64_t slots_stride;
} dimsum_state_update_slots_params_t;

typedef struct {
    uint32_t struct_size;     /* sizeof(dimsum_decode_linear_slots_params_t) */
    int32_t num_slots;
    dimsum_decode_linear_params_t linear;
    const void *slots_ptr;
    int64_t slots_stride;
} dimsum_decode_linear_slots_params_t;

int dimsum_causal_conv1d_update_slots(const dimsum_conv_update_slots_params_t *p, void *stream);
int dimsum_selective_state_update_slots(const dimsum_state_update_slots_params_t *p, void *stream);
int dimsum_decode_linear_slots(const dimsum_decode_linear_slots_params_t *p, void *stream);

/* dimsum_state_copy_slots: duplicate slots of a state pool -- ONE launch copies, for every pair (src, dst), row `src` onto row `dst` of
 * EVERY tensor of the pool: all layers' conv_state and ssm_state (csrc/state_copy.hip; no reference counterpart). A move of bits: no
 * conversion, no arithmetic, plain vector stores, no atomics.
 *   table : DEVICE memory, n_tensors entries of three int64 each: {base pointer, slot stride in BYTES, row bytes}. Entry i describes a tensor
 *       whose slot s occupies the row_bytes contiguous bytes at base + s * slot_stride, for s in [0, num_slots). The tensors may differ in
 *       dtype and row size; slot_stride >= row_bytes (a view of a larger buffer). It is built once per pool and kept.
 *   pairs : DEVICE int32 (n_pairs, 2), rows pairs_stride ELEMENTS apart (>= 2): pairs[i] = (src, dst), read by the kernel, never by the host,
 *       so a captured launch copies whatever the buffer holds at replay. A pair with src < 0 or dst < 0 is skipped (the padding convention of
 *       the *_slots entries), and so is one with an index >= num_slots: no address outside the pool is formed. One src may feed many dst.
 *       The result is defined when no dst equals another pair's src or dst: THE CALLER'S CONTRACT.
 *   max_row_bytes : the largest row_bytes of the table (it sizes the grid; a smaller positive value is still correct, only slower).
 * A tensor whose base, slot stride and row bytes are all multiples of 16 moves in 16-byte pieces, any other in pieces of the largest of
 * 4, 2, 1 bytes that divides the three; the choice is made on the device, per tensor, and gives the same bits.
 * Checks, in this order: NULL struct / struct_size (DIMSUM_ERR_ABI) / table_ptr or pairs_ptr NULL (DIMSUM_ERR_NULL) / num_slots < 1, a
 * negative n_tensors, n_pairs or max_row_bytes, or more (pair, tensor, chunk) workgroups than a grid holds (DIMSUM_ERR_SHAPE) /
 * pairs_stride < 2 (DIMSUM_ERR_STRIDE). n_pairs == 0, n_tensors == 0 or max_row_bytes == 0 then returns DIMSUM_OK without a launch. */
typedef struct {
    uint32_t struct_size;     /* sizeof(dimsum_state_copy_params_t) */
    int32_t num_slots;        /* rows of every tensor of the pool, >= 1 */
    int32_t n_tensors, n_pairs;
    const void *table_ptr;
    const void *pairs_ptr;
    int64_t pairs_stride;
    int64_t max_row_bytes;
    int64_t reserved[2];      /* 0 */
} dimsum_state_copy_params_t;

#define DIMSUM_STATE_COPY_CHUNK_BYTES 16384   /* one workgroup's share of a row per round: 256 lanes x 4 pieces of 16 bytes */

int dimsum_state_copy_slots(const dimsum_state_copy_params_t *p, void *stream);

/* dimsum_cross_entropy_fwd / _bwd: the LM training loss over rows of logits and its gradient (csrc/cross_entropy.hip; the reference's training
 * recipes use a fused cross-entropy in this place). Per row m, with s = logit_scale * logits[m, :] and eps = label_smoothing:
 *     lse = logsumexp(s)      z = lse_square_scale * lse^2      loss = lse - (1 - eps) s[label] - (eps / vocab) sum(s) + z
 *     dlogits[m, v] = dloss[m] * logit_scale * ((1 + 2 lse_square_scale lse) exp(s_v - lse) - (1 - eps) [v == label] - eps / vocab)
 *   logits (rows, vocab) of `dtype`, unit column stride, any row stride >= vocab (a [..., :vocab] view of a padded buffer is read in place:
 *   nothing beyond column vocab - 1 of a row is read or written); no alignment is asked of the base (rows that start 16-byte aligned move in
 *   16-byte pieces, others element by element, with the same bits). labels (rows) int64; loss, z_loss (rows) f32, lse (rows) f64, contiguous;
 *   z_loss may be NULL. lse is a double so that the backward's exp(s_v - lse) keeps fp32 accuracy whatever the row's offset (an fp32 lse of
 *   80 is known to 4e-6 only, and so would be every probability). Row offsets are 64-bit.
 *   label == ignore_index: loss = z_loss = 0 and a zero gradient row; lse is still written. Any other label outside [0, vocab): loss = NaN
 *   and a NaN gradient row; nothing outside the row is touched.
 *   fwd reads logits, labels; writes loss, lse, z_loss. bwd reads logits, labels, lse, dloss ((rows) f32, any element stride >= 0: 0 is an
 *   expanded scalar); writes dlogits (rows, vocab) of `dtype` with row stride dlogits_row_stride >= vocab. dlogits may BE logits (equal
 *   pointers and equal row strides: the in-place backward); any other overlap of the two is DIMSUM_ERR_ALIAS.
 *   No atomics; the summation order depends on vocab and dtype alone: two launches on equal inputs are bit-identical, and a row's results do
 *   not depend on `rows` or on the row's index.
 * Checks, in this order: NULL struct / struct_size (DIMSUM_ERR_ABI) / required pointers (logits, labels, lse; fwd: loss; bwd: dloss, dlogits) /
 * shape (rows in [1, 2^31), vocab in [1, 2^31 - 16)) / dtype / strides (logits_row_stride < vocab; bwd: dlogits_row_stride < vocab,
 * dloss_stride < 0) / bwd: dlogits overlapping logits other than in place (DIMSUM_ERR_ALIAS) / unsupported (label_smoothing outside [0, 1),
 * a non-finite logit_scale or lse_square_scale). Nothing is launched before all of them pass. */
typedef struct {
    uint32_t struct_size;     /* sizeof(dimsum_cross_entropy_params_t) as the caller compiled it; anything else -> DIMSUM_ERR_ABI */
    int32_t dtype;            /* of logits and dlogits */
    int64_t rows, vocab;
    int64_t logits_row_stride, dlogits_row_stride, dloss_stride;
    int64_t ignore_index;
    float label_smoothing, logit_scale, lse_square_scale;
    int32_t reserved;         /* 0 */
    const void *logits_ptr, *labels_ptr, *dloss_ptr;
    void *loss_ptr, *lse_ptr, *z_loss_ptr, *dlogits_ptr;     /* lse: written by fwd, read by bwd */
} dimsum_cross_entropy_params_t;

int dimsum_cross_entropy_fwd(const dimsum_cross_entropy_params_t *p, void *stream);
int dimsum_cross_entropy_bwd(const dimsum_cross_entropy_params_t *p, void *stream);

/* dimsum_sample_logits: one token id per row of logits under top-k / top-p / temperature, drawn with a uniform number the caller supplies
 * (csrc/sample_logits.hip; the distribution of the reference's sample(), mamba_ssm/utils/generation.py:55-80, stated without a sort). Nothing
 * in the kernel generates random numbers: out[r] is a pure function of (logits[r, :], top_k, top_p, temperature, u of the row).
 *   RANK: the tokens of a row by descending logit; equal logits rank by ascending index (torch.topk / sort leave this open). NaN counts as
 *   -inf, -0 as +0.
 *   top_k == 1: the rank-0 token (argmax, the lowest index among equal maxima); u is not read and may be NULL.
 *   Otherwise the KEPT set starts as the top_k highest ranks; top_k <= 0 or >= vocab: all tokens. Inside it p_v ~ exp((l_v - max) / temperature).
 *   With 0 < top_p < 1 a token is then dropped iff the kept-set probability mass of the tokens ranked strictly above it is >= top_p (the
 *   reference's "ascending inclusive cumulative sum <= 1 - top_p is removed", restated from the top); top_p outside (0, 1): no cut.
 *   DRAW: the inverse CDF over the kept tokens in ascending vocabulary index (not rank order: the distribution does not depend on the order):
 *   the first kept v whose running mass exceeds u * Z, Z the kept mass; u is clamped into [0, 1) (NaN -> 0).
 *   -inf logits have probability 0 and are never returned while the row has a finite logit; a row with none yields token 0.
 *   ARITHMETIC: a weight exp2((l_v - max) log2(e) / temperature) is cut to 40 fractional bits and every mass is a 64-bit INTEGER sum of weights:
 *   sums are exact in any order and the comparisons with top_p * Z and u * Z are integer comparisons (target ceil(top_p Z), floor(u Z) + 1). A
 *   token whose weight is below 2^-40 of the maximum's has mass 0. Two launches on equal inputs are bit-identical; a row's token depends
 *   neither on `rows`, nor on the row's index, nor on the alignment of its base.
 *   SAFETY: whatever the inputs, the value written is in [0, vocab).
 *   logits (rows, vocab) of `dtype`, unit column stride, any row stride >= vocab (a [..., :vocab] view of a padded buffer is read in place);
 *   no alignment is asked of the base. Row offsets are 64-bit. u: f32; out: int64 (rows).
 *   row_index (optional): a DEVICE int64; the row's uniform is u[step * rows + r] instead of u[r], step = row_index[0] clamped into
 *   [0, table_steps). out_table (optional, needs row_index): int64 (table_steps, rows); the token is also written to out_table[step * rows + r].
 *   With the two a replayed graph finds its step's uniforms and files its token with no host work.
 * Checks, in this order: NULL struct / struct_size (DIMSUM_ERR_ABI) / required pointers (logits, out; u unless top_k == 1; row_index with
 * out_table) / dtype / shape (rows in [1, 2^31), vocab in [1, 2^31 - 16), temperature finite and > 0, table_steps >= 1 with row_index) /
 * stride (logits_row_stride < vocab) / out, then out_table, overlapping the logits (DIMSUM_ERR_ALIAS). Nothing is launched before all pass. */
typedef struct {
    uint32_t struct_size;     /* sizeof(dimsum_sample_logits_params_t) as the caller compiled it; anything else -> DIMSUM_ERR_ABI */
    int32_t dtype;            /* of logits */
    int64_t rows, vocab;
    int64_t logits_row_stride;
    int32_t top_k;
    float top_p, temperature;
    int32_t reserved;         /* 0 */
    const void *logits_ptr, *u_ptr;
    void *out_ptr;
    const void *row_index_ptr;  /* optional from here on */
    void *out_table_ptr;
    int64_t table_steps;      /* rows of u and out_table that row_index may address */
} dimsum_sample_logits_params_t;

int dimsum_sample_logits(const dimsum_sample_logits_params_t *p, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Fused residual-add + RMSNorm / LayerNorm over rows (M, N), f32 statistics.
 *   r = x (+ x_bias) (+ residual) ; residual_out = r (if residual_out_ptr) ; y = norm(r) * weight (+ bias)
 *   optionally followed by the adaLN modulation of the row's batch element (rows_per_batch consecutive rows each):
 *       y = y * (1 + mod_scale[row / rows_per_batch, :]) + mod_shift[row / rows_per_batch, :]
 *   (x_bias = the bias of the Linear that produced x, so that the GEMM runs without a bias epilogue; with it and the
 *   modulation, "h + proj(x) -> RMSNorm -> modulate" of a DiM block is ONE pass instead of three.)
 *   rstd (M) f32 always written; mean (M) f32 written for LayerNorm.
 *   y_split3: y is written as the split-bf16 operand image the following Linear consumes (below, dimsum_split3).
 * bwd: dx = d(norm)/dr . dy (+ dresidual_out) ; dweight/dbias (N) f32 accumulated with atomics into zero-filled
 * buffers (the Triton reference reduces per-SM partials on the host, layernorm.py:324-359).
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct {
    uint32_t struct_size;     /* sizeof(dimsum_norm_params_t) */
    int32_t rows, cols;
    int32_t is_rms_norm;
    int32_t x_dtype, residual_dtype, out_dtype; /* dimsum_dtype_t; residual_dtype covers residual and residual_out */
    float eps;
    int64_t x_row_stride, residual_row_stride, y_row_stride, residual_out_row_stride;
    const void *x_ptr, *residual_ptr, *weight_ptr, *bias_ptr;
    void *y_ptr, *residual_out_ptr, *mean_ptr, *rstd_ptr;
    const void *xbias_ptr;                      /* (N) f32 or NULL */
    const void *mod_scale_ptr, *mod_shift_ptr;  /* (M / rows_per_batch, N) f32, both or none */
    int64_t mod_row_stride;
    int32_t rows_per_batch;
    int32_t y_split3;   /* 1: y is a split-bf16 left operand image, rows of 3 N bf16 [hi | hi | lo] (out_dtype BF16, N % 4 == 0,
                         * y_row_stride >= 3 N): see dimsum_split3.  2: y is a scaled-fp16 operand image (out_dtype F16, N % 4 == 0):
                         * row r = fp16(y_r * 2^s_r) with 2^-s_r written to y_inv_scale_ptr[r]: see dimsum_rows_f16s.
                         * 3: like 1 but as the PAIR [hi | lo], rows of 2 N bf16 (y_row_stride >= 2 N), for a consumer that reads it as
                         * [hi | hi | lo] (dimsum_gemm_ext_t.a_alias_rows / b_alias_rows): a third less image traffic */
    void *y_inv_scale_ptr;                      /* (M) f32, y_split3 == 2 only */
} dimsum_norm_params_t;

typedef struct {
    uint32_t struct_size;     /* sizeof(dimsum_norm_bwd_params_t) */
    int32_t rows, cols;
    int32_t is_rms_norm;
    float eps;
    int32_t reserved;         /* 0 */
    int64_t r_row_stride, dy_row_stride, dres_row_stride, dx_row_stride;
    const void *r_ptr;       /* saved residual_out (f32) = the normalised input */
    const void *weight_ptr, *mean_ptr, *rstd_ptr;
    const void *dy_ptr;      /* f32 */
    const void *dres_ptr;    /* gradient flowing into residual_out, or NULL */
    void *dx_ptr;            /* f32; equals dresidual_in when a residual was added */
    void *dweight_ptr, *dbias_ptr; /* (N) f32 zero-filled; dbias may be NULL */
} dimsum_norm_bwd_params_t;

int dimsum_norm_fwd(const dimsum_norm_params_t *p, void *stream);
int dimsum_norm_bwd(const dimsum_norm_bwd_params_t *p, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Split-bf16 operand images for the library GEMMs (csrc/operand_split.hip). No reference counterpart: the reference's
 * Linears are TF32 GEMMs (allow_tf32, dimsum/train.py:20-21); gfx950 has no TF32 MFMA and hipBLASLt splits fp32 operands
 * into hi + lo bf16 inside the GEMM. x = hi + lo with hi = bf16(x), lo = bf16(x - hi); a (rows, cols) f32 matrix becomes
 * (rows, 3 cols) bf16:  left != 0: [hi | hi | lo]  (activations),  left == 0: [hi | lo | hi]  (weights), so that
 *     left_image (M, 3K) . weight_image (N, 3K)^T  =  hi.hi + hi.lo + lo.hi   accumulated in f32 by ONE bf16 GEMM.
 * Producer kernels write the left image directly (dimsum_norm_params_t.y_split3, dimsum_gated_gelu_fwd_split3).
 * left == 2: the PAIR [hi | lo] ((rows, 2 cols) bf16) for dimsum_gemm_ext_t.a_alias_rows / tn_pair_*_cols.
 * cols % 4 == 0, src rows 16-byte aligned (src_row_stride % 4 == 0), dst contiguous and 8-byte aligned.
 * ------------------------------------------------------------------------------------------------------------- */
int dimsum_split3(const void *src, int64_t rows, int64_t cols, int64_t src_row_stride, void *dst, int32_t left, void *stream);
/* weight (rows = N, cols = K) float32 -> (3 K, N) bfloat16: the ROW stack [hi; lo; hi] of its transpose -- the b operand of dimsum_gemm_tn when
   the a operand is a d-major activation pair of planes (out_proj behind the scan's out_z_lo_offset output). rows % 2 == 0. */
int dimsum_split3_t(const void *src, int64_t rows, int64_t cols, int64_t src_row_stride, void *dst, void *stream);

/* Scaled-fp16 operand image ("f16s") -- the single-product carrier of the same policy: TF32 keeps 10 mantissa bits of each operand and
 * accumulates in fp32; fp16 has exactly that mantissa, and its narrow exponent is taken out of the picture by an exact power-of-two
 * scale per row: dst[r, :] = fp16(src[r, :] * 2^s_r), 2^s_r * max|src[r, :]| in [2^14, 2^15), inv_scale[r] = 2^-s_r. The GEMM multiplies
 * the images (v_mfma_f32_16x16x32_f16, fp32 accumulation) and its epilogue applies a_inv_scale[m] * b_inv_scale[n] (dimsum_gemm_nt).
 *   src (rows, cols) f32, cols % 4 == 0; dst (rows, cols) f16; inv_scale (rows) f32;
 *   l1max: NULL, or one f32 (zeroed by the caller) that receives max_r sum_c |src[r, c]| (weights: the bound the gated epilogue uses).
 * Producer kernels write the image directly (dimsum_norm_params_t.y_split3 == 2, dimsum_tt_params_t.y_split3 == 2, GATED_GELU_F16). */
int dimsum_rows_f16s(const void *src, int64_t rows, int64_t cols, int64_t src_row_stride, void *dst, int64_t dst_row_stride,
                     void *inv_scale, void *l1max, void *stream);

/* Block-scaled fp16 image of a d-major f32 matrix (rows = channels, cols = batch x tokens): every 64 rows x 32 cols block as fp16(x 2^s), 2^-s (f32) at
 * table[(col / 32) * table_ld + row / 64] -- the layout dimsum_ssm_ext_t.out_z_f16 makes the 64-channel scan kernel write, produced here from the f32
 * out_z of a launch the state-split scan kernels serve, for dimsum_gemm_tn's a_block_inv_ptr (out_proj as one fp16 product). rows % 64 == 0,
 * cols % 256 == 0, src rows 16-byte aligned. */
int dimsum_rows_block_f16s(const void *src, int64_t rows, int64_t cols, int64_t src_row_stride, void *dst, int64_t dst_row_stride, void *table,
                           int64_t table_ld, void *stream);

/* Many scaled-fp16 conversions in ONE launch (per 24 jobs): the weight images, largest row L1 norms and bias maxima a whole denoiser forward
 * needs under the scaled-fp16 policy (host: dimsum_amd/gemm.py forward_scope). No reference counterpart: the reference's cuBLAS TF32 GEMMs
 * read the fp32 weights directly (dimsum/train.py:20-21). Same image as dimsum_rows_f16s, bit for bit. */
typedef struct {
    const void *src;            /* (rows, cols) f32 rows, 16-byte aligned, cols % 4 == 0, src_row_stride % 4 == 0 */
    void *dst;                  /* (rows, cols) f16 image, or NULL: reduce only (a bias vector: rows = 1) */
    void *inv_scale_ptr;        /* (rows) f32, required with dst */
    void *l1max_ptr;            /* 1 f32, ZERO-FILLED by the caller, or NULL: l1_factor * max_r sum_k |x_rk| */
    void *absmax_ptr;           /* 1 f32, ZERO-FILLED by the caller, or NULL: max |x| over the matrix */
    int64_t rows, cols, src_row_stride, dst_row_stride;
    float l1_factor;            /* 0 = 1 */
    int32_t reserved;
} dimsum_f16s_job_t;
int dimsum_rows_f16s_multi(const dimsum_f16s_job_t *jobs, int32_t n_jobs, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Token-space transforms on (batch, L = grid*grid tokens, channels) f32 tensors: ONE pass that fuses
 *   - a per-channel gate at load:             v[s, c] = x[b, in_index[s], c] * gate[b, c]
 *   - a transform T on every 4x4 token block of the grid (position s = row-major grid index):
 *       HAAR_FWD / HAAR_INV : 2-level Haar DWT / inverse incl. the reference's subband->channel regrouping
 *                             (WaveDiMBlock._dwt_fast / _idwt_fast, dimsum/models_dim.py:572-604)
 *       DCT_FWD / DCT_INV   : 4x4 DCT-II / inverse (dimsum/dct_layer.py:6-84, models_dim.py:876-882, 919-928)
 *   - a token permutation at load (in_index) and/or at store (out_index): int32 tables composed on the host from
 *     transpose / continuity / flip / window-scan / zigzag orders (dimsum/scanning_orders.py, models_dim.py:1496-1524)
 *   - the adaLN affine and a residual at store:
 *       y[b, out_index[s], c] = T(v)[s, c] * (1 + scale[b, c]) + shift[b, c] + residual[b, out_index[s], c]
 *   - for the backward passes (the adjoint of an orthogonal T is its inverse up to a constant, so the adjoints of
 *     both block-side fusions are again this kernel), two per-(batch, channel) reductions against a weight tensor w
 *     indexed like y:   wdot[b, c] += sum_s T(v)[s, c] * w[b, out_index[s], c]      wsum[b, c] += sum_s w[b, out_index[s], c]
 *     and the plain token sum   tsum[b, c] += sum_s T(v)[s, c]
 *     (f32 atomics into caller-zeroed (batch, channels) arrays: d scale / d gate and d shift of the adaLN modulation).
 *     With y_ptr == NULL only the reductions are produced.
 * Every optional pointer may be NULL (identity / 0). Streaming op: 2*B*L*C*4 bytes (+ residual / + w).
 * ------------------------------------------------------------------------------------------------------------- */
typedef enum {
    DIMSUM_TT_NONE = 0, DIMSUM_TT_HAAR_FWD = 1, DIMSUM_TT_HAAR_INV = 2, DIMSUM_TT_DCT_FWD = 3, DIMSUM_TT_DCT_INV = 4
} dimsum_tt_kind_t;

typedef struct {
    uint32_t struct_size;                  /* sizeof(dimsum_tt_params_t) */
    int32_t batch, tokens, channels, grid; /* tokens = grid*grid, grid % 4 == 0 unless kind == NONE */
    int32_t kind;                          /* dimsum_tt_kind_t */
    int32_t y_split3;                      /* 1: y is the split-bf16 left operand image of the Linear that consumes it: rows of
                                              3 C bf16 [hi | hi | lo] (dimsum_split3); y strides in bf16 elements, channels % 4 == 0.
                                              2: y is the scaled-fp16 image (dimsum_rows_f16s): fp16 rows of C (strides in fp16 elements,
                                              channels % 4 == 0, channels <= 1024), y_inv_scale_ptr[b * tokens + token] = 2^-s.
                                              3: like 1 as the pair [hi | lo], rows of 2 C bf16 (see dimsum_norm_params_t.y_split3) */
    int64_t x_batch_stride, x_token_stride;           /* channel stride 1 everywhere */
    int64_t res_batch_stride, res_token_stride;
    int64_t y_batch_stride, y_token_stride;
    int64_t mod_batch_stride;                         /* row stride of gate / scale / shift, each (batch, channels) */
    int64_t w_batch_stride, w_token_stride;
    int64_t red_batch_stride;                         /* row stride of wdot / wsum, each (batch, channels) */
    const void *x_ptr;
    const int32_t *in_index_ptr, *out_index_ptr;      /* (tokens) or NULL */
    const void *gate_ptr, *scale_ptr, *shift_ptr, *residual_ptr;
    void *y_ptr;                                      /* may be NULL when only the reductions are wanted */
    const void *w_ptr;                                /* (batch, tokens, channels) f32 or NULL */
    void *wdot_ptr, *wsum_ptr;                        /* (batch, channels) f32 accumulators (atomicAdd) or NULL */
    void *tsum_ptr;                                   /* (batch, channels) f32: tsum[b, c] += sum_s T(v)[s, c], or NULL */
    void *y_inv_scale_ptr;                            /* (batch, tokens) f32, y_split3 == 2 only */
    int32_t y_f16s_lds_offset;                        /* internal (set by the library) */
    int32_t reserved;                                 /* 0 */
} dimsum_tt_params_t;

int dimsum_token_transform(const dimsum_tt_params_t *p, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Cross-attention fusion core (attention_fusion.py:72-74, swap_k = False), MFMA QK^T / PV, f32 in/out:
 *   out[b, i, h*hd + e]        = softmax_j(q1[b,h,i,:].k2[b,h,j,:] * scale) v2[b,h,j,e]        (x12)
 *   out[b, i, C/2 + h*hd + e]  = softmax_j(q2.k1 * scale) v1                                    (x21)
 * qkv1, qkv2 : (batch, L, 3*heads*hd) as produced by the qkv Linear (q|k|v, head-major inside each).
 * lse (batch, 2, heads, L) f32 saved for the backward, or NULL.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct {
    uint32_t struct_size;   /* sizeof(dimsum_xattn_params_t) */
    int32_t batch, seqlen, heads, head_dim;
    float scale;
    int32_t n_dirs;   /* 0 or 2: the two swapped-KV directions above. 1: plain self-attention out = softmax(q1 k1^T) v1
                         (DiTBlock's attention, models_dim.py:1540): qkv2 / bias2 unused, out (batch, L, heads*hd),
                         lse (batch, 1, heads, L); in the backward dqkv2_ptr is unused and dqkv1 receives dq, dk, dv */
    int64_t qkv_batch_stride, qkv_token_stride;
    int64_t out_batch_stride, out_token_stride;
    const void *qkv1_ptr, *qkv2_ptr;
    void *out_ptr, *lse_ptr;
    const void *bias1_ptr, *bias2_ptr;   /* optional (3*heads*hd) f32: the qkv Linear biases, added while q / k / v are
                                            fetched, so that the qkv GEMMs can run without a bias epilogue */
    int32_t precision;  /* 0: exact fp32 MFMA (v_mfma_f32_16x16x4_f32). 1: split-bf16 -- every fp32 operand
                           x = hi + lo (two bf16), products hi.hi + hi.lo + lo.hi on v_mfma_f32_16x16x32_bf16 with fp32
                           accumulation, ~1e-5 relative: the same arithmetic hipBLASLt uses for the reference's
                           torch.backends.cuda.matmul.allow_tf32 = True policy (train.py:20-21) on gfx950 */
    int32_t out_split3; /* forward, precision 1 only. != 0: out rows are the split-bf16 operand image of the proj Linear:
                           3 x (n_dirs' x heads x hd) bf16 [hi | hi | lo] (dimsum_split3); out strides in bf16 elements. 3 = the pair
                           [hi | lo] (2 x ...), see dimsum_norm_params_t.y_split3.
                           precision 2: 0 (fp32 out) or 2 = the scaled-fp16 image (dimsum_rows_f16s): fp16 rows of n_dirs' x heads x hd
                           (strides in fp16 elements) + out_inv_ptr[b * L + token] */
    /* precision 2 (forward only): ONE fp16 MFMA product per element, the TF32-equivalent arithmetic (10-bit mantissas, fp32
     * accumulation). q is scaled per query row (exact), k / v per batch element from the bound
     *   |k|, |v| <= max_t (2^15 x_inv[b, t]) * wl1 + bmax,   kv_bound = {wl1 of qkv1's weight, max|bias1|, wl1 of qkv2's, max|bias2|}
     * where x*_inv are the inverse row scales (batch, L) of the scaled-fp16 images the qkv GEMMs consumed (wl1 = max_n sum_c |W_nc|). */
    const void *x1_inv_ptr, *x2_inv_ptr, *kv_bound_ptr;
    void *out_inv_ptr;  /* (batch, L) f32, out_split3 == 2 */
    int32_t qkv_f16;    /* precision 2 only. 1: qkv1 / qkv2 are the fp16 outputs of dimsum_gemm_nt's F16_QKV epilogue (biases included, scaled as
                           described there; qkv strides in fp16 elements, bias pointers unused): half the bytes of the fp32 qkv tensors */
    int32_t reserved2;
} dimsum_xattn_params_t;

int dimsum_xattn_fusion_fwd(const dimsum_xattn_params_t *p, void *stream);

/* Backward of the core (replaces the autograd of the two F.scaled_dot_product_attention calls).
 *   fwd      : the forward's operands; out_ptr = the forward's `out`, lse_ptr = its saved log-sum-exp (both required)
 *   dout     : (batch, L, 2*heads*hd) f32, strides like `out`
 *   dqkv1/2  : (batch, L, 3*heads*hd) f32, fully overwritten (direction 0 -> dq1, dk2, dv2; direction 1 -> dq2, dk1, dv1)
 *   delta    : (batch, 2, heads, L) f32 scratch (row sums of dout o out); TWICE that under fwd.precision == 2
 *   fwd.precision: 0 exact fp32 MFMA, 1 split-bf16 (three products), 2 = ONE fp16 product per element (qkv_f16 must be 0: the fp32 qkv
 *                  tensors are read). Under 2 q (times scale), k, v go to fp16 as they are (|.| <= 65504); every dout row (one query of
 *                  one head) is scaled by an exact power of two that brings its maximum to [2^-5, 2^-4), D with it, P travels as 2^8 P, and
 *                  dq is unscaled on store; in the sums over queries (dk, dv) P also carries g_min / g_q <= 1, so that all rows enter
 *                  at the scale of the (batch, head, direction)'s largest gradient row (the second half of `delta` carries the row
 *                  scales from the dq kernel to the dk / dv kernel). Range: max|v| <= 32 at head_dim 64 in the worst case. */
typedef struct {
    uint32_t struct_size;   /* sizeof(dimsum_xattn_bwd_params_t) */
    uint32_t reserved;      /* 0 */
    dimsum_xattn_params_t fwd;
    int64_t dqkv_batch_stride, dqkv_token_stride;
    const void *dout_ptr;
    void *dqkv1_ptr, *dqkv2_ptr, *delta_ptr;
} dimsum_xattn_bwd_params_t;

int dimsum_xattn_fusion_bwd(const dimsum_xattn_bwd_params_t *p, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * GatedMLP epilogue (mlp.py:66-70, GELU tanh), x12 : (M, 2H) f32 = output of the w12 GEMM WITHOUT its bias:
 *   h[m, j] = gelu_tanh(x12[m, j] + bias[j]) * (x12[m, H + j] + bias[H + j])          bias (2H) f32 or NULL
 * bwd: dx12 (M, 2H); dbias (2H) f32 zero-filled by the caller (column sums of dx12, f32 atomics) or NULL.
 * ------------------------------------------------------------------------------------------------------------- */
int dimsum_gated_gelu_fwd(const void *x12, const void *bias, void *h, int64_t rows, int64_t hidden, void *stream);
/* same, h3 = the split-bf16 left operand image of the w3 GEMM: (rows, 3 hidden) bf16, [hi | hi | lo] (dimsum_split3) */
int dimsum_gated_gelu_fwd_split3(const void *x12, const void *bias, void *h3, int64_t rows, int64_t hidden, void *stream);
int dimsum_gated_gelu_bwd(const void *x12, const void *bias, const void *dh, void *dx12, void *dbias, int64_t rows,
                          int64_t hidden, void *stream);
/* same, dx12_image = dx12 as a split-bf16 operand image in WEIGHT order: (rows, 3 x 2 hidden) bf16 [hi | lo | hi] (dimsum_split3),
 * paired with left-order images of W12^T (input gradient) and, through the (3 rows, .) view of both, of the MLP input (weight gradient) */
int dimsum_gated_gelu_bwd_split3(const void *x12, const void *bias, const void *dh, void *dx12_image, void *dbias, int64_t rows,
                                 int64_t hidden, void *stream);
/* the same with dx12 as the PAIR [hi | lo] (rows of 2 x 2 hidden bf16): see dimsum_gemm_ext_t.a_alias_weight_order / tn_pair_a_cols */
int dimsum_gated_gelu_bwd_pair(const void *x12, const void *bias, const void *dh, void *dx12_pair, void *dbias, int64_t rows, int64_t hidden, void *stream);
/* the same with dx12 as a scaled-fp16 operand image (dimsum_rows_f16s): dx12_image (rows, 2 hidden) float16, inv_scale (rows) f32 (exact row maxima):
 * the operand of both backward GEMMs of w12 under the scaled-fp16 policy (dimsum_gemm_nt; dimsum_gemm_tn with k_scale_ptr). hidden <= 5120. */
int dimsum_gated_gelu_bwd_f16s(const void *x12, const void *bias, const void *dh, void *dx12_image, void *inv_scale, void *dbias, int64_t rows,
                               int64_t hidden, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The plain (non-gated) MLP's activation (timm Mlp as dimsum/models_dit.py:124 and use_gated_mlp=False build it: fc1 -> GELU(tanh) -> fc2),
 * x : (rows, hidden) f32 contiguous = output of the fc1 GEMM WITHOUT its bias, hidden % 4 == 0:
 *   fwd: h[m, j]  = gelu_tanh(x[m, j] + bias[j])                       bias (hidden) f32 or NULL
 *   bwd: dx[m, j] = dh[m, j] * gelu_tanh'(x[m, j] + bias[j]);  dbias (hidden) f32 zero-filled by the caller (column sums of dx, f32 atomics:
 *        one per column per 64-row workgroup, like dimsum_gated_gelu_bwd) or NULL.
 * out_image: what out_ptr receives --
 *   DIMSUM_GELU_OUT_F32     (rows, hidden) f32
 *   DIMSUM_GELU_OUT_SPLIT3  the split-bf16 operand image (rows, 3 hidden) bf16: fwd in LEFT order [hi | hi | lo] (fc2's left operand),
 *                           bwd in WEIGHT order [hi | lo | hi] (both gradient GEMMs of fc1), as the gated passes write them
 *   DIMSUM_GELU_OUT_PAIR    the pair [hi | lo] (rows, 2 hidden) bf16 (dimsum_gemm_ext_t.a_alias_rows / a_alias_weight_order / tn_pair_a_cols)
 *   DIMSUM_GELU_OUT_F16S    the scaled-fp16 image (rows, hidden) float16 + inv_scale_ptr (rows) f32, hidden <= 5120. The row scale is the
 *                           exact row maximum's power of two (dimsum_rows_f16s) -- or, fwd with ext->row_inv_ptr and ext->bound_ptr, the
 *                           bound-derived one of DIMSUM_GEMM_EPI_GELU_F16 (same inputs -> the same scales and the same image as that epilogue)
 * ------------------------------------------------------------------------------------------------------------- */
typedef enum { DIMSUM_GELU_OUT_F32 = 0, DIMSUM_GELU_OUT_SPLIT3 = 1, DIMSUM_GELU_OUT_PAIR = 2, DIMSUM_GELU_OUT_F16S = 3 } dimsum_gelu_out_t;

typedef struct {
    uint32_t struct_size;      /* sizeof(dimsum_gelu_ext_t) as the caller compiled it (see "Versioning" at the top) */
    int32_t reserved;          /* 0 */
    /* fwd, DIMSUM_GELU_OUT_F16S: both or none. row_inv (rows) f32 = the inverse row scales of the fc1 GEMM's left image, bound = {wl1, bmax}
     * 2 f32 on the device: scale(2 (2^15 row_inv[m] wl1 + bmax)) instead of the row maximum (no reduction over the row). */
    const void *row_inv_ptr, *bound_ptr;
} dimsum_gelu_ext_t;

typedef struct {
    uint32_t struct_size;      /* sizeof(dimsum_gelu_params_t) as the caller compiled it; anything else -> DIMSUM_ERR_ABI */
    int32_t out_image;         /* dimsum_gelu_out_t */
    int64_t rows, hidden;
    const void *x_ptr, *bias_ptr;
    const void *dh_ptr;        /* bwd only: (rows, hidden) f32 contiguous */
    void *out_ptr;             /* fwd: h, bwd: dx -- or their image */
    void *inv_scale_ptr;       /* DIMSUM_GELU_OUT_F16S: (rows) f32 */
    void *dbias_ptr;           /* bwd only, or NULL */
    const dimsum_gelu_ext_t *ext;   /* NULL = none */
} dimsum_gelu_params_t;

int dimsum_gelu_fwd(const dimsum_gelu_params_t *p, void *stream);
int dimsum_gelu_bwd(const dimsum_gelu_params_t *p, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The row passes of the top-1 mixture-of-experts layer (SwitchMLP, dimsum/switch_mlp.py:69-99; the expert MLP, dimsum/mlp.py:7-46) around the
 * per-expert GEMMs, which the host runs over contiguous row slices of the tokens sorted by expert. Everything is f32 rows, width % 4 == 0,
 * 16-byte aligned; 1 <= num_experts <= 64; other shapes are DIMSUM_ERR_SHAPE. Index tables are int32.
 *
 * dimsum_moe_route_fwd (three launches): x (tokens, hidden), w (E, hidden), b (E) or NULL ->
 *   logits (tokens, E) = x w^T + b: f32 accumulation, the same reduction order for every expert (identical router rows give identical logits);
 *   route = softmax(logits, 1) (DIMSUM_MOE_ROUTE_SOFTMAX) or sigmoid(logits) (DIMSUM_MOE_ROUTE_SIGMOID);
 *   prob (tokens), expert (tokens) = max(route, 1), the first maximum on ties;
 *   the stable counting sort of the tokens by expert: offsets (E + 1), perm (tokens) = the token in sorted row j, inv (tokens) = perm's inverse,
 *   row_expert (tokens) = expert[perm[j]]. Deterministic: no atomic decides a position. work: dimsum_moe_route_work_bytes() bytes of scratch.
 *   tokens == 0 is a valid call of every dimsum_moe_* entry (the row pointers may then be NULL): route_fwd writes E + 1 zero offsets, the others do nothing.
 * dimsum_moe_route_bwd: reads x, w, logits, prob, expert, inv, dprob (tokens), dxp (tokens, hidden) in sorted order ->
 *   dlogit = dprob p (1 - p) at the chosen expert (sigmoid) or dprob p* (delta - p_e) (softmax), formed in the kernel;
 *   dx[t] = dxp[inv[t]] + sum_e dlogit[t, e] w[e];  dw (E, hidden) and db (E): zero-filled by the caller, f32 atomics (one per element per
 *   workgroup). num_experts > 8: dx is written once and updated in place per group of 8 experts.
 * ------------------------------------------------------------------------------------------------------------- */
typedef enum { DIMSUM_MOE_ROUTE_SOFTMAX = 0, DIMSUM_MOE_ROUTE_SIGMOID = 1 } dimsum_moe_route_t;

typedef struct {
    uint32_t struct_size;      /* sizeof(dimsum_moe_ext_t) as the caller compiled it (see "Versioning" at the top) */
    int32_t reserved;          /* 0 */
} dimsum_moe_ext_t;

typedef struct {
    uint32_t struct_size;      /* sizeof(dimsum_moe_route_params_t) as the caller compiled it; anything else -> DIMSUM_ERR_ABI */
    int32_t mode;              /* dimsum_moe_route_t */
    int32_t num_experts;
    int32_t reserved;          /* 0 */
    int64_t tokens, hidden;
    const void *x_ptr, *w_ptr, *b_ptr;
    void *prob_ptr, *expert_ptr, *logits_ptr;                   /* fwd: written; bwd: read */
    void *offsets_ptr, *perm_ptr, *inv_ptr, *row_expert_ptr;    /* fwd: written; bwd: inv is read, the others are ignored */
    void *work_ptr;            /* fwd */
    int64_t work_bytes;
    const void *dprob_ptr, *dxp_ptr;                            /* bwd */
    void *dx_ptr, *dw_ptr, *db_ptr;                             /* bwd */
    const dimsum_moe_ext_t *ext;   /* NULL = none */
} dimsum_moe_route_params_t;

int64_t dimsum_moe_route_work_bytes(int64_t tokens, int32_t num_experts);
int dimsum_moe_route_fwd(const dimsum_moe_route_params_t *p, void *stream);
int dimsum_moe_route_bwd(const dimsum_moe_route_params_t *p, void *stream);

/* dimsum_moe_permute    : dst[j, :] = src[perm[j], :]
 * dimsum_moe_combine_fwd: dst[perm[j], :] = prob[perm[j]] src[j, :]       (perm is a permutation: every row of dst is written exactly once)
 * dimsum_moe_combine_bwd: src = dout (token order), y (sorted order): dst[j, :] = prob[t] dout[t, :], dprob[t] = <dout[t, :], y[j, :]>, t = perm[j]
 * perm's entries must lie in [0, rows). */
typedef struct {
    uint32_t struct_size;      /* sizeof(dimsum_moe_rows_params_t) */
    int32_t reserved;          /* 0 */
    int64_t rows, hidden;
    const void *src_ptr, *perm_ptr, *prob_ptr, *y_ptr;
    void *dst_ptr, *dprob_ptr;
    const dimsum_moe_ext_t *ext;   /* NULL = none */
} dimsum_moe_rows_params_t;

int dimsum_moe_permute(const dimsum_moe_rows_params_t *p, void *stream);
int dimsum_moe_combine_fwd(const dimsum_moe_rows_params_t *p, void *stream);
int dimsum_moe_combine_bwd(const dimsum_moe_rows_params_t *p, void *stream);

/* The experts' activation over the sorted rows, exact (erf) GELU. S = gated ? 2 width : width; x (rows, S) = the fc1 GEMM output WITHOUT bias;
 * bias (num_experts, S) or NULL, the row taken by row_expert[r] (row_expert NULL: num_experts == 1, row 0 for every r).
 *   fwd: out (rows, width) = gelu_erf(x[:, :width] + b) * (x[:, width:] + b)   (gated)   or   gelu_erf(x + b)
 *   bwd: out (rows, S) = d x from dh (rows, width), derivative Phi(a) + a phi(a); dbias (num_experts, S) zero-filled by the caller or NULL:
 *        column sums per expert, held in registers over 64 rows, one f32 atomic per column at an expert boundary and at the chunk's end. */
typedef struct {
    uint32_t struct_size;      /* sizeof(dimsum_moe_act_params_t) */
    int32_t gated;             /* bool */
    int32_t num_experts;
    int32_t reserved;          /* 0 */
    int64_t rows, width;
    const void *x_ptr, *bias_ptr, *row_expert_ptr, *dh_ptr;
    void *out_ptr, *dbias_ptr;
    const dimsum_moe_ext_t *ext;   /* NULL = none */
} dimsum_moe_act_params_t;

int dimsum_moe_act_fwd(const dimsum_moe_act_params_t *p, void *stream);
int dimsum_moe_act_bwd(const dimsum_moe_act_params_t *p, void *stream);

/* dimsum_moe_gemm: the grouped expert GEMM over the sorted rows, out[j, :] = x[j, :] . W_e^T (+ bias[e, :]) for offsets[e] <= j < offsets[e + 1].
 *   x (tokens, k) f32 contiguous; offsets (num_experts + 1) int32 ON THE DEVICE (what dimsum_moe_route_fwd writes: the host never reads them, so a
 *   layer built on this entry has no device-to-host copy and can be captured into a hipGraph); w_ptrs: a HOST array of num_experts device pointers to
 *   (n, k) f32 contiguous matrices (they are copied into the kernel arguments: no device pointer table); bias (num_experts, n) f32 or NULL;
 *   out (tokens, n) f32 with row stride ldc >= n. Rows outside every expert's range are not written. The offsets are expected to be non-decreasing in [0, tokens]; any other table is made so
 *   on the device (entries clamped to [0, tokens], a range starts no earlier than the previous non-empty range ended): no row is written twice.
 *   One launch of (ceil(tokens / DIMSUM_MOE_GEMM_BM) + num_experts) x ceil(n / DIMSUM_MOE_GEMM_BN) workgroups; a workgroup finds its expert from the
 *   offsets, a tile never spans two experts. fp32 operands are split into bf16 hi + lo while they are staged and multiplied as hi.hi + hi.lo + lo.hi
 *   on the bf16 MFMA with fp32 accumulation (the three products of the library's fp32 GEMM under allow_tf32); no split-K, no atomics: bit-reproducible.
 *   Served: k % 32 == 0, n % 32 == 0, 1 <= num_experts <= 64, tokens >= 0 (else DIMSUM_ERR_SHAPE); all pointers 16-byte aligned (offsets: 4),
 *   ldc % 4 == 0 (else DIMSUM_ERR_STRIDE). tokens == 0 is a valid call that launches nothing (the pointers may then be NULL). */
#define DIMSUM_MOE_GEMM_BM 64      /* rows of an output tile */
#define DIMSUM_MOE_GEMM_BN 128     /* columns of an output tile */

typedef struct {
    uint32_t struct_size;      /* sizeof(dimsum_moe_gemm_params_t) */
    int32_t num_experts;
    int64_t tokens, k, n, ldc;
    const void *x_ptr, *offsets_ptr;
    const void *const *w_ptrs; /* host array [num_experts] of device pointers */
    const void *bias_ptr;
    void *out_ptr;
    const dimsum_moe_ext_t *ext;   /* NULL = none */
} dimsum_moe_gemm_params_t;

int dimsum_moe_gemm(const dimsum_moe_gemm_params_t *p, void *stream);

/* The two gradients of dimsum_moe_gemm (csrc/moe_gemm_bwd.hip), on the same device offsets (clamped and cut the same way), the same three bf16
 * products and the same widths (k % 32 == 0, n % 32 == 0, 1 <= num_experts <= 64; else DIMSUM_ERR_SHAPE). No split-K, no atomics: bit-reproducible.
 * The host never reads the offsets: a backward built on these entries has no device-to-host copy. tokens == 0 launches nothing (pointers may be NULL).
 * dimsum_moe_gemm_dgrad: dx[j, :] = dy[j, :] . W_e for offsets[e] <= j < offsets[e + 1]; dy (tokens, n) f32 contiguous, w_ptrs: a HOST array of
 *   num_experts device pointers to the (n, k) f32 matrices of the forward (read transposed while they are staged: no W^T in memory), dx (tokens, k)
 *   f32 with row stride ldc >= k, ldc % 4 == 0. Rows outside every range are not written. Grid: the forward's, over ceil(k / DIMSUM_MOE_GEMM_BN) columns.
 * dimsum_moe_gemm_wgrad: dW_e[n', k'] = sum over offsets[e] <= j < offsets[e + 1] of dy[j, n'] x[j, k']; dy (tokens, n), x (tokens, k) f32 contiguous;
 *   dw_ptrs: a HOST array of num_experts device pointers to (n, k) f32 contiguous outputs, every element of which is written (zeros for an empty
 *   range: no memset before the call); db (num_experts, n) f32 or NULL: db[e, n'] = sum_j dy[j, n'], zeros for an empty range. Grid:
 *   ceil(k / DIMSUM_MOE_GEMM_BN) x ceil(n / DIMSUM_MOE_GEMM_BM) x num_experts; a workgroup walks its expert's rows 32 at a time, rows past the
 *   range's end contribute zeros. All row pointers 16-byte aligned (offsets, db: 4), else DIMSUM_ERR_STRIDE. */
typedef struct {
    uint32_t struct_size;      /* sizeof(dimsum_moe_gemm_dgrad_params_t) */
    int32_t num_experts;
    int64_t tokens, k, n, ldc;
    const void *dy_ptr, *offsets_ptr;
    const void *const *w_ptrs; /* host array [num_experts] of device pointers */
    void *dx_ptr;
    const dimsum_moe_ext_t *ext;   /* NULL = none */
} dimsum_moe_gemm_dgrad_params_t;

typedef struct {
    uint32_t struct_size;      /* sizeof(dimsum_moe_gemm_wgrad_params_t) */
    int32_t num_experts;
    int64_t tokens, k, n;
    const void *dy_ptr, *x_ptr, *offsets_ptr;
    void *const *dw_ptrs;      /* host array [num_experts] of device pointers */
    void *db_ptr;
    const dimsum_moe_ext_t *ext;   /* NULL = none */
} dimsum_moe_gemm_wgrad_params_t;

int dimsum_moe_gemm_dgrad(const dimsum_moe_gemm_dgrad_params_t *p, void *stream);
int dimsum_moe_gemm_wgrad(const dimsum_moe_gemm_wgrad_params_t *p, void *stream);

/* The grouped expert GEMM on scaled-fp16 operand images (csrc/moe_gemm_f16.hip; the images: dimsum_rows_f16s above) -- inference under the
 * scaled-fp16 policy: ONE v_mfma_f32_16x16x32_f16 product per element instead of dimsum_moe_gemm's three bf16 products, fp32 accumulation.
 *   out[j, n] = x_inv[j] * w_inv_e[n] * sum_k x[j, k] w_e[n, k] (+ bias[e, n])  for offsets[e] <= j < offsets[e + 1]
 *   x (tokens, k) f16 contiguous with x_inv (tokens) f32; w_ptrs / w_inv_ptrs: HOST arrays of num_experts device pointers to the (n, k) f16
 *   images and their (n) f32 inverse scales (copied into the kernel arguments); bias (num_experts, n) f32 or NULL; out (tokens, n) f32, row
 *   stride ldc >= n. Offsets, grid, tiles (DIMSUM_MOE_GEMM_BM x _BN), served shapes, alignment rules and the empty call: dimsum_moe_gemm's.
 *   No split-K, no atomics: bit-reproducible. The inverse scales are powers of two: the only rounding is the fp32 accumulation (and the bias add).
 * The two producers write the operand images themselves, bit for bit what dimsum_rows_f16s makes of the f32 pass's output (exact row maxima):
 * dimsum_moe_permute_f16s: dst[j, :] = f16(src[perm[j], :] 2^s_j), inv_scale[j] = 2^-s_j; src (rows, hidden) f32, hidden % 4 == 0.
 * dimsum_moe_act_fwd_f16s: dimsum_moe_act_fwd with out (rows, width) f16 and inv_scale (rows); width <= 5120 (else DIMSUM_ERR_SHAPE). */
typedef struct {
    uint32_t struct_size;      /* sizeof(dimsum_moe_gemm_f16s_params_t) */
    int32_t num_experts;
    int64_t tokens, k, n, ldc;
    const void *x_ptr, *x_inv_ptr, *offsets_ptr;
    const void *const *w_ptrs;     /* host array [num_experts] of device pointers: (n, k) f16 */
    const void *const *w_inv_ptrs; /* host array [num_experts] of device pointers: (n) f32 */
    const void *bias_ptr;
    void *out_ptr;
    const dimsum_moe_ext_t *ext;   /* NULL = none */
} dimsum_moe_gemm_f16s_params_t;

typedef struct {
    uint32_t struct_size;      /* sizeof(dimsum_moe_permute_f16s_params_t) */
    int32_t reserved;          /* 0 */
    int64_t rows, hidden;
    const void *src_ptr, *perm_ptr;
    void *dst_ptr, *inv_scale_ptr;
    const dimsum_moe_ext_t *ext;   /* NULL = none */
} dimsum_moe_permute_f16s_params_t;

typedef struct {
    uint32_t struct_size;      /* sizeof(dimsum_moe_act_f16s_params_t) */
    int32_t gated;             /* bool */
    int32_t num_experts;
    int32_t reserved;          /* 0 */
    int64_t rows, width;
    const void *x_ptr, *bias_ptr, *row_expert_ptr;
    void *out_ptr, *inv_scale_ptr;
    const dimsum_moe_ext_t *ext;   /* NULL = none */
} dimsum_moe_act_f16s_params_t;

int dimsum_moe_gemm_f16s(const dimsum_moe_gemm_f16s_params_t *p, void *stream);
int dimsum_moe_permute_f16s(const dimsum_moe_permute_f16s_params_t *p, void *stream);
int dimsum_moe_act_fwd_f16s(const dimsum_moe_act_f16s_params_t *p, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * NT GEMM with a fused Linear epilogue: C (m, n) = A (m, k) . B (n, k)^T, 16-bit operands (bf16 or fp16 rows, k contiguous), fp32
 * accumulation on v_mfma_f32_16x16x32_*. Replaces the library GEMM behind F.linear(x, weight) for the large bias-free projections
 * of the denoiser (dimsum/mlp.py:66-70 w12 / w3, mamba_simple.py in_proj / out_proj, attention_fusion.py qkv / proj). The operands are
 * what the producer kernels of this library write: split-bf16 images over 3 K ([hi | hi | lo] rows against [hi | lo | hi] weights:
 * the reference's TF32 policy, dimsum_split3) or scaled fp16 rows.
 *   epilogue F32            : C fp32 (m, n), row stride ldc
 *            F32_BIAS       : C = A B^T + bias[n]
 *            GATED_GELU_SPLIT3 : B = the w12 weight (n = 2 F rows: x1 rows [0, F), x2 rows [F, 2 F)), bias (2 F) fp32 or NULL;
 *                             C = the LEFT split-bf16 image (m, 3 F) of h = gelu_tanh(x1 + b1) * (x2 + b2), ldc in bf16 elements:
 *                             the fp32 x12 tensor of mlp.py:68 never exists
 *            GATED_GELU_F16 : same, C = fp16 (m, F) of h * out_scale
 *            GELU_F16       : C = the scaled-fp16 image (m, n) of h = gelu_tanh(A B^T + bias) -- fc1 of the plain MLP (see the enum)
 *            F32_GATE_RESIDUAL : C = residual + gate[row / rows_per_batch] * (A B^T + bias): the residual tail of a block
 *                             ("x = x + gate * mlp(...)", models_dim.py:1107-1113) in the epilogue of its last Linear; residual (m, n) f32,
 *                             gate (m / rows_per_batch, n) f32 or NULL (= 1), rows_per_batch % 256 == 0, bias NULL or (n)
 * Shapes: m % 256 == 0, k % 64 == 0, k >= 128, n % 4 == 0 (gated: n % 16 == 0, ldc % 8 == 0); lda, ldb % 8 == 0; a_ptr, b_ptr, c_ptr
 * 16-byte aligned.
 * ------------------------------------------------------------------------------------------------------------- */
typedef enum {
    DIMSUM_GEMM_EPI_F32 = 0, DIMSUM_GEMM_EPI_GATED_GELU_SPLIT3 = 1, DIMSUM_GEMM_EPI_GATED_GELU_F16 = 2, DIMSUM_GEMM_EPI_F32_BIAS = 3,
    DIMSUM_GEMM_EPI_F32_GATE_RESIDUAL = 4,
    DIMSUM_GEMM_EPI_F32_CONV = 6,   /* in_proj of a Mamba mixer with the causal conv1d + bias + SiLU of its x half in the epilogue (mamba_simple.py in_proj followed
                                       by causal_conv1d_fn, selective_scan_interface.py:616): C (m, n) f32 d-major (rows = channels, columns = tokens); rows
                                       [0, conv_rows) hold silu(conv(A B^T) + conv_bias) along the columns, in sequences of conv_seq columns (256 % conv_seq == 0,
                                       n % conv_seq == 0: zero history at every sequence start), the other rows the plain product. conv_weight (conv_rows,
                                       conv_width 2..4) f32 row stride conv_weight_ld, conv_bias (conv_rows) f32 or NULL. conv_rows % 128 == 0. */
    DIMSUM_GEMM_EPI_F16_QKV = 5,    /* the qkv Linear of the attention fusion under the scaled-fp16 policy (attention_fusion.py:52-60, models_dim.py:1470):
                                       C (m, n = 3 C') fp16 = fp16((A B^T + bias) 2^s), scaled-fp16 operands (a / b_inv_scale_ptr required). Columns
                                       [0, qkv_q_cols) (q) take one power-of-two scale per ROW, the rest (k, v) one per BATCH ELEMENT (rows_per_batch rows,
                                       a multiple of 256), both from the bound |x W^T + b| <= 2^15 a_inv * wl1 + bmax with gate_bound_ptr = {wl1, bmax}:
                                           s_row = scale(2 (2^15 a_inv[row] wl1 + bmax)),  s_batch = scale(2 (2^15 max_t a_inv[b, t] wl1 + bmax))
                                       -- exactly what dimsum_xattn_fusion_fwd (precision 2, qkv_f16 = 1) assumes of its fp16 inputs: it recomputes the
                                       same scales from the same a_inv and bound. Halves the bytes between the two kernels (no fp32 qkv tensor). */
    DIMSUM_GEMM_EPI_GELU_F16 = 7    /* fc1 of the plain MLP (dimsum/models_dit.py:124; use_gated_mlp=False) under the scaled-fp16 policy, inference:
                                       C (m, n) fp16 = fp16(gelu_tanh(A B^T + bias) 2^s_row), scaled-fp16 operands (a / b_inv_scale_ptr required), not
                                       paired, no column interleave. One power-of-two scale per row from the bound |gelu(x)| <= |x| <= 2^15 a_inv wl1 + bmax
                                       with gate_bound_ptr = {wl1, bmax}: s_row = scale(2 (2^15 a_inv[row] wl1 + bmax)); its inverse goes to
                                       h_inv_scale_ptr[row] (required) -- the a_inv_scale of fc2's GEMM. n % 8 == 0, ldc % 8 == 0. bf16 operands, unscaled
                                       operands, a missing bound (no constant out_scale form), aliased operands, x12_ptr and c_image_pieces are not built:
                                       DIMSUM_ERR_UNSUPPORTED (the caller runs F32 + dimsum_gelu_fwd). */
} dimsum_gemm_epilogue_t;

/* Everything beyond C = A B^T (+ bias): fused epilogue operands, operand-image read modes, timing, tuning. All 0 / NULL by default. */
typedef struct {
    uint32_t struct_size;         /* sizeof(dimsum_gemm_ext_t) as the caller compiled it (see "Versioning" at the top) */
    int32_t rows_per_batch;       /* F32_GATE_RESIDUAL with a gate, F16_QKV */
    void *timing_start_event, *timing_stop_event;   /* optional hipEvent_t pair recorded at the kernel's own dispatch boundaries */
    /* tune_variant: 0 = the library's choice of tile shape / schedule (dimsum_gemm_nt_kernel_for reports it). 512 = 128 x 256 tiles by 4-wave
     * workgroups (scaled-fp16 operands only), 513 = 256 x 256 tiles, one workgroup per tile (never the persistent stream), 514 = the persistent
     * K-tile stream (one workgroup per CU walking the tile list) where the shape allows it (k / 64 even and >= 4, more tiles than CUs, no
     * aliased operand), else as 513. Other values: tuning builds only (-DDIMSUM_GEMM_TUNE), DIMSUM_ERR_UNSUPPORTED otherwise.
     * tune_group_m: tile rows per L2 patch of the tile walk (0 = automatic). tune_reserved: start delay of the odd CUs (tuning builds). */
    int32_t tune_variant, tune_group_m, tune_reserved;
    int32_t c_image_pieces;       /* GATED_GELU_SPLIT3: 0 / 3 = the image [hi | hi | lo] (ldc >= 3 F); 2 = the pair [hi | lo] (ldc >= 2 F), for a consumer that
                                     reads it with a_alias_rows: a third less image traffic, the same three products */
    /* GATED_GELU_F16 over scaled operands: the h image gets one power-of-two scale per row, derived WITHOUT a row reduction from the bound
     * |x1|, |x2| <= max|a_m| * gate_bound[0] + gate_bound[1]  (gate_bound = {max_n sum_k |w_nk|, max |bias|}, 2 f32 on the device);
     * its inverse goes to h_inv_scale[m] -- the a_inv_scale of the w3 GEMM. NULL: out_scale for every row. */
    const void *gate_bound_ptr;
    void *h_inv_scale_ptr;        /* (m) f32; GELU_F16: required */
    /* F32_GATE_RESIDUAL */
    const void *residual_ptr, *gate_ptr;
    int64_t residual_ld, gate_ld;
    /* GATED_GELU_SPLIT3, training forward (mlp.py:66-70 under autograd): when non-NULL the bias-free accumulators [x1 | x2] are ALSO stored
       as float32 (m, n) rows with stride x12_ld -- what the gated-GeLU adjoint of the backward reads; bf16 images only. */
    void *x12_ptr;
    int64_t x12_ld;
    /* != 0 = the A operand's reduction indices r >= a_alias_rows are the indices r - a_alias_rows of a_ptr (k = 3 a_alias_rows, % 64 == 0): a
       [hi | lo] pair (dimsum_gemm_nt: 2 C columns per row; dimsum_gemm_tn: a [hi; lo] pair of planes) serves as the left operand image
       [hi | hi | lo] without storing hi twice. */
    int64_t a_alias_rows;
    int64_t b_alias_rows;         /* dimsum_gemm_nt, F32 epilogue: the same for the B rows (in_proj: the activation image is the right operand) */
    /* training (dimsum/mlp.py:66-70 under autograd): the gradient images as pairs too.
       a_alias_weight_order (dimsum_gemm_nt, with a_alias_rows = C): the pair is read in WEIGHT order [hi | lo | hi] (dx = dy_w . (W^T)image).
       tn_pair_a_cols / tn_pair_b_cols (dimsum_gemm_tn): both operands are pairs -- a_ptr rows [hi | lo] with lo at column tn_pair_a_cols (read
       in weight order), b_ptr rows [hi | lo] with lo at column tn_pair_b_cols (read in left order); k = the rows of one piece, splits = 3 x the
       number of row ranges: partial result (piece, range) pairs A's piece with B's piece over that range. */
    int32_t a_alias_weight_order, qkv_q_cols;      /* qkv_q_cols: F16_QKV only (% 16 == 0) */
    const void *conv_weight_ptr, *conv_bias_ptr;   /* F32_CONV only */
    int32_t conv_rows, conv_width, conv_seq, conv_weight_ld;
    /* dimsum_gemm_tn, float16 operands, splits == 1, k <= 4096: block-scaled A (the scan's fp16 out_z, dimsum_ssm_ext_t.out_z_f16, with its
     * table as it is): a_block_inv_ptr is a (m / 32, a_block_inv_ld >= k / 64) float32 table of inverse scales (powers of two): the A values of
     * tokens [32 g, 32 g + 32) in reduction rows [64 t, 64 t + 64) stand for value * a_block_inv[g][t]. The kernel puts a token group on ONE
     * scale -- its row's largest inverse -- by multiplying the blocks by exact powers of two <= 1 as it reads them, and multiplies the result by
     * that scale and b_inv_scale_ptr[n]; a_inv_scale_ptr must be NULL. */
    const void *a_block_inv_ptr;
    int64_t a_block_inv_ld;
    int64_t tn_pair_a_cols, tn_pair_b_cols;
    /* dimsum_gemm_tn, float16 operands: the weight gradient dW = dY^T X of a Linear under the scaled-fp16 policy (torch.mm(dy.t(), x) under
     * train.py:20-21's TF32). Both operands are scaled-fp16 images with one power-of-two scale per ROW -- the images the forward and the input
     * gradient use -- but their rows are the reduction index here: k_scale_ptr[r] (k float16: a_inv[r] b_inv[r] / max_r(a_inv b_inv), powers of
     * two <= 1) multiplies A's row r as it is read and *c_scale_ptr (one f32 on the device: that maximum) multiplies the result;
     * a_inv_scale_ptr / b_inv_scale_ptr NULL. k / splits <= 16384 reduction rows per range. */
    const void *k_scale_ptr;
    const void *c_scale_ptr;
    /* the same factors formed INSIDE the kernel (no dimsum_row_factors launch in front of the product): k_inv_a_ptr (k f32) and k_inv_b_ptr (k f32
     * or NULL = 1) are the two images' inverse row scales; every workgroup multiplies the pair over its OWN reduction range, normalises by the
     * range's maximum (powers of two: exact), keeps the factors in LDS as float16 and multiplies its partial result by that maximum -- ranges
     * are summed in fp32 afterwards, so no global maximum is needed. k_scale_ptr / c_scale_ptr must be NULL then. */
    const void *k_inv_a_ptr;
    const void *k_inv_b_ptr;
} dimsum_gemm_ext_t;

/* The Linear itself: what F.linear(x, weight, bias) is given (plus the operand dtype and the power-of-two scales the scaled-fp16 operand
 * images carry). `ext` = NULL: C = A B^T (+ bias), fp32 (or the gated epilogues with a constant out_scale). */
typedef struct {
    uint32_t struct_size;         /* sizeof(dimsum_gemm_params_t) as the caller compiled it; anything else -> DIMSUM_ERR_ABI */
    int32_t m, n, k;
    int32_t operand_dtype;        /* DIMSUM_BF16 or DIMSUM_F16 (both operands) */
    int32_t epilogue;             /* dimsum_gemm_epilogue_t */
    float out_scale;              /* GATED_GELU_F16 only */
    int32_t reserved;             /* 0 */
    int64_t lda, ldb, ldc;        /* row strides in elements of the respective dtype */
    const void *a_ptr, *b_ptr, *bias_ptr;
    void *c_ptr;
    /* scaled-fp16 operand images (dimsum_rows_f16s): C[m, n] = acc * a_inv_scale[m] * b_inv_scale[n] (exact powers of two), both or none */
    const void *a_inv_scale_ptr;  /* (m) f32 */
    const void *b_inv_scale_ptr;  /* (n) f32 */
    const dimsum_gemm_ext_t *ext; /* NULL = the plain Linear */
} dimsum_gemm_params_t;

int dimsum_gemm_nt(const dimsum_gemm_params_t *p, void *stream);
/* Which kernel dimsum_gemm_nt launches for these parameters (a pure function of *p and of the current device's CU count; nothing is launched):
 *   0 = gemm_nt_kernel         256 x 256 tiles, one 8-wave workgroup per tile
 *   1 = gemm_nt_m128_kernel    128 x 256 tiles, 4-wave workgroups, two per CU (short-K launches with fp32-family epilogues)
 *   2 = gemm_nt_persist_kernel one workgroup per CU walking the tile list as one K-tile stream (the gated w12 GEMM under the scaled-fp16 policy)
 * or -(error status) for parameters dimsum_gemm_nt would refuse. Measurement / tests; no reference counterpart. */
int dimsum_gemm_nt_kernel_for(const dimsum_gemm_params_t *p);

/* The weight-gradient shape of the same Linears under autograd (torch.mm(dy.t(), x) in the reference's autograd graph; dimsum/mlp.py:66-70,
   attention_fusion.py:44-79): C[s] (m, n) float32 = sum over the rows r of reduction range s of A[r, 0..m)^T B[r, 0..n). a_ptr: (k, m) rows
   with stride lda, b_ptr: (k, n) rows with stride ldb (16-bit, the split-bf16 images viewed as (3 rows, features) stacks), k = all
   reduction rows, cut into `splits` equal ranges (k % (64 splits) == 0) whose partial results lie c_split_stride floats apart in c_ptr --
   the caller adds them (a fixed order: bitwise reproducible). m % 256 == 0; n % 256 == 0, or n % 4 == 0 with B's rows ZERO-PADDED to the next multiple
   of 256 columns (ldb >= that multiple: the last column tile reads the padding; only columns < n are stored); epilogue F32 only; the other fields as above. */
int dimsum_gemm_tn(const dimsum_gemm_params_t *p, int32_t splits, int64_t c_split_stride, void *stream);

/* The weight-gradient shape of the Mamba projections under autograd (selective_scan_interface.py:954-981: "eB,dB->ed" d out_proj.weight,
   d in_proj.weight = dxz x): one operand is a d-major activation -- A (m, k) float16 rows CONTIGUOUS along the reduction index (channels x tokens,
   lda) -- the other token-major -- B (k, n) float16 rows OVER the reduction index (ldb): C[s] (m, n) float32 = sum over the rows r of range s of
   A[0..m, r] B[r, 0..n). Scaled-fp16 images only: a_inv_scale_ptr (m) = A's row scales (its rows are output rows; NULL = 1), ext->k_scale_ptr (k)
   float16 = B's row scales as per-reduction-row factors (/ their maximum), ext->c_scale_ptr = that maximum -- or ext->k_inv_a_ptr (k f32) = B's row
   scales themselves, normalised inside the kernel; b_inv_scale_ptr NULL. `splits`
   ranges of k / splits <= 16384 rows, k % (64 splits) == 0; m % 256 == 0, n % 256 == 0; partial results c_split_stride floats apart. */
int dimsum_gemm_nn(const dimsum_gemm_params_t *p, int32_t splits, int64_t c_split_stride, void *stream);
/* the k_scale_ptr / c_scale_ptr operands of the two entry points above from the row scales of the two images: k_scale[r] = float16(a_inv[r] b_inv[r] /
   c_scale), c_scale = max_r a_inv[r] b_inv[r]; a_inv, b_inv (n) f32 inverse row scales (b_inv NULL = 1), k_scale (n) float16, c_scale 1 f32. One launch. */
int dimsum_row_factors(const void *a_inv, const void *b_inv, int64_t n, void *k_scale, void *c_scale, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DIMSUM_HIP_H */
