// ssm_scan_host.hpp -- the selective scan's host layer: what ssm_scan_fwd.hip, ssm_scan_bwd.hip and the launchers next to the kernels
// (ssm_scan_fwd_kernel.hpp, ssm_scan_fwd_split.hpp, ssm_scan_fwd_lanes.hpp) share between the C ABI and the kernels. No device code.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace dimsum {

// ---- kernel launchers: defined next to their kernels, instantiated per I/O dtype in ssm_scan_fwd_{,split_,rev_}{f32,f16,bf16}.hip ------
template <typename T, int kN> void ssm_scan_fwd_launch_v0(const ssm_args_t &p, hipStream_t stream, int tiles, bool vec, bool full);
template <typename T, int kN, int kSP> void ssm_scan_fwd_launch_split(const ssm_args_t &p, hipStream_t stream, int tiles, bool vec, bool full);
template <typename T> void ssm_scan_fwd_launch_lanes(const ssm_args_t &p, hipStream_t stream, int tiles, bool vec, bool full);
template <typename T, int kN> void ssm_scan_fwd_launch_rev(const ssm_args_t &p, hipStream_t stream, int tiles, bool vec, bool full);
template <typename T> void ssm_scan_fwd_launch_lanes_rev(const ssm_args_t &p, hipStream_t stream, int tiles, bool vec, bool full);

// The (HASZ, VEC, FULL) rungs every launcher instantiates its kernel for: LAUNCH(HASZ, VEC, FULL) is invoked with the compile-time image
// of (vec, full); full implies vec. HASZ is passed through (a launcher of both forms goes through DIMSUM_Z_VEC_FULL_LADDER).
#define DIMSUM_VEC_FULL_LADDER(LAUNCH, HASZ, vec, full) \
    do {                                                \
        if (full) LAUNCH(HASZ, true, true);             \
        else if (vec) LAUNCH(HASZ, true, false);        \
        else LAUNCH(HASZ, false, false);                \
    } while (0)
#define DIMSUM_Z_VEC_FULL_LADDER(LAUNCH, has_z, vec, full)            \
    do {                                                              \
        if (has_z) DIMSUM_VEC_FULL_LADDER(LAUNCH, true, vec, full);   \
        else DIMSUM_VEC_FULL_LADDER(LAUNCH, false, vec, full);        \
    } while (0)

// ---- ssm_scan_fwd.hip -------------------------------------------------------------------------------------------------------------------
// the checks every entry point makes on a flat block, in this order: operands (required pointers, the fused dt_proj's operands, z => out_z
// in the forward), then the launch shape. ssm_check = both; a dispatch query, which has no pointers, checks the shape alone.
int ssm_check_operands(const ssm_args_t &p, bool forward);
int ssm_check_shape(const ssm_args_t &p);
inline int ssm_check(const ssm_args_t &p, bool forward) {
    const int rc = ssm_check_operands(p, forward);
    return rc != DIMSUM_OK ? rc : ssm_check_shape(p);
}
int ssm_scan_fwd_variant(const ssm_args_t &p);                  // forward kernel of a launch, as lanes per channel: 1, 2, 4 or 16
int ssm_scan_fwd_run(const ssm_args_t &a, hipStream_t s);       // flat block -> kernels (also the backward's state-rebuild sweep)

// ---- ssm_scan_bwd.hip: the two parts of the backward's workspace ------------------------------------------------------------------------
int64_t ssm_bwd_partial_bytes(int32_t batch, int32_t dim, int32_t seqlen, int32_t dstate, int32_t n_groups);
int64_t ssm_bwd_ckpt_bytes(int32_t batch, int32_t dim, int32_t seqlen, int32_t dstate);

// ---- dtype x dstate dispatch: THE list of I/O types and state sizes the kernels are instantiated for ------------------------------------
// fn(type_tag<T>{}, std::integral_constant<int, kN>{}) -> status; DIMSUM_ERR_DTYPE / DIMSUM_ERR_SHAPE for anything else (dtype first)
template <typename T> struct type_tag { using type = T; };

template <typename Fn> int ssm_dispatch(int32_t dtype, int32_t dstate, Fn &&fn) {
    auto on_dstate = [&](auto t) -> int {
        switch (dstate) {
            case 4: return fn(t, std::integral_constant<int, 4>{});
            case 8: return fn(t, std::integral_constant<int, 8>{});
            case 16: return fn(t, std::integral_constant<int, 16>{});
            case 32: return fn(t, std::integral_constant<int, 32>{});
            default: return DIMSUM_ERR_SHAPE;
        }
    };
    switch (dtype) {
        case DIMSUM_F32: return on_dstate(type_tag<float>{});
        case DIMSUM_F16: return on_dstate(type_tag<__half>{});
        case DIMSUM_BF16: return on_dstate(type_tag<__hip_bfloat16>{});
        default: return DIMSUM_ERR_DTYPE;
    }
}
#define DIMSUM_TAG_T(t) typename decltype(t)::type
#define DIMSUM_TAG_N(n) decltype(n)::value

// vector path of one operand: its base 4-element aligned, its row strides % 4 (the innermost stride is 1)
template <typename T> inline bool ssm_vec4_ok(const void *ptr, int64_t batch_stride, int64_t row_stride) {
    return aligned_to<T>(ptr, 4 * sizeof(T)) && batch_stride % 4 == 0 && row_stride % 4 == 0;
}

// The reversed direction of a bidirectional call: the forward direction's block with A_b / out_b / ckpt_b of the public struct (the forward's
// or the backward's) in place. The timing events bracket the pair -- begin of the first launch, end of the second: f loses its stop event,
// the returned block its start event.
template <typename Pub> inline ssm_args_t ssm_reversed_from(ssm_args_t &f, const Pub &pub) {
    ssm_args_t b = f;
    b.A_ptr = pub.A_b_ptr; b.A_d_stride = pub.A_b_d_stride; b.A_dstate_stride = pub.A_b_dstate_stride;
    b.out_ptr = const_cast<void *>(pub.out_b_ptr); b.out_batch_stride = pub.out_b_batch_stride; b.out_d_stride = pub.out_b_d_stride;
    b.ckpt_ptr = const_cast<void *>(pub.ckpt_b_ptr);
    f.timing_stop_event = nullptr;
    b.timing_start_event = nullptr;
    return b;
}

}  // namespace dimsum
