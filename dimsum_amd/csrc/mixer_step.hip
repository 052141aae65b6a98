// mixer_step.hip -- the recurrent (token by token) form of the Mamba mixer for gfx950: one step of the causal conv1d and one step of the
// selective scan on carried states, both updated in place.
//
// Replaces causal_conv1d_cuda.causal_conv1d_update (causal-conv1d/csrc/causal_conv1d.cpp:512-569; kernel causal_conv1d_update.cu) and the
// Triton selective_state_update (mamba/mamba_ssm/ops/triton/selective_state_update.py:21-190), with the semantics of their *_ref functions:
//     conv_state <- [conv_state[.., 1:], x];   out = act(bias[d] + sum_w W[d, w] conv_state[b, d, w])
//     dt' = softplus(dt + dt_bias);   state <- state exp(dt' A) + dt' B x;   out = (sum_n state C + D x) silu(z)
//
// MI355X design: both are small streaming passes -- 2 B D W s bytes of conv state, 2 B D N s of SSM state (33.5 MB at batch 256, D 1024, N 16:
// a few microseconds at HBM rate), so a step is bound by its launches, not by these kernels. One work-item owns one (batch, channel) row,
// channels along the lanes: x, dt, z and out are coalesced, B[b] and C[b] are the same addresses across a wave (one request), a row of the
// state / of A is walked in 16-byte pieces where it is aligned (kVec) and element by element otherwise, and whatever follows the last whole
// piece of a row is a scalar tail. No LDS, no cross-lane traffic, no atomics: a launch is a pure function of its inputs. One wave per
// workgroup, so that a batch-1 step (1024 rows) still spreads over 16 CUs; the grid's y axis is the batch (no division per work-item).
// Each lane walks its own row of the state, so one 16-byte load of a wave touches 64 cache lines: fine while a step is launch-bound
// (DESIGN.md section 3.13), not the layout for a bandwidth-bound kernel.
//
// Slot-indexed states (dimsum_causal_conv1d_update_slots / dimsum_selective_state_update_slots, kSlots): the state is a pool and row b works
// on state[slots[b]], the index read from device memory by every lane of the row (one address per wave); slots[b] < 0 stores a zero and
// touches no state. A template flag on the two kernels, not sibling kernels: the row functions are entered with the state row's index `sb`
// next to the batch row `b`, so both forms ARE the same expressions in the same order, and kSlots = false (sb = b, the plain parameter
// struct as the only kernel argument) compiles to the kernels as they were. That slots[b] < num_slots and that no slot is named twice is the
// caller's contract (include/dimsum_hip.h): the kernel trusts the index.
#include "common.hpp"

#include <type_traits>

namespace dimsum {

constexpr int kStepBlock = 64;

template <typename T> __device__ __forceinline__ f32x4 load4f(const T *p) { return widen(ld4<T>(p)); }

// ---------------------------------------------------------------------------------------------------------------------
// kVec: width 4 and every state row one aligned 4-element piece: the row moves as ONE load and ONE store of its raw bits
// sb: the row of the state tensor that batch row b works on (b itself without slots)
template <typename T, bool kVec>
__device__ __forceinline__ void conv_update_row(const dimsum_conv_update_params_t &p, int64_t b, int64_t sb, int64_t d, int W);

// the slot form's kernel argument: the plain parameters and the (batch) int32 slot index
template <typename P> struct slots_args_t {
    P p;
    const int32_t *slots;
    int64_t slots_stride;
};
template <typename P> __device__ __forceinline__ const P &step_base(const P &a) { return a; }
template <typename P> __device__ __forceinline__ const P &step_base(const slots_args_t<P> &a) { return a.p; }

// grid: (channel blocks, batch rows): no division per work-item; a batch beyond the grid's y limit is walked with a grid stride
template <typename T, bool kVec, bool kSlots>
__global__ __launch_bounds__(kStepBlock) void causal_conv1d_update_kernel(
    const std::conditional_t<kSlots, slots_args_t<dimsum_conv_update_params_t>, dimsum_conv_update_params_t> a) {
    const dimsum_conv_update_params_t &p = step_base(a);
    const int64_t d = (int64_t)blockIdx.x * kStepBlock + threadIdx.x;
    if (d >= p.dim) return;
    const int W = p.width;
    for (int64_t b = blockIdx.y; b < p.batch; b += gridDim.y) {
        if constexpr (kSlots) {
            const int32_t slot = a.slots[b * a.slots_stride];
            if (slot < 0) reinterpret_cast<T *>(p.out_ptr)[b * p.out_batch_stride + d * p.out_c_stride] = from_f32<T>(0.f);      // a padding row
            else conv_update_row<T, kVec>(p, b, slot, d, W);
        } else {
            conv_update_row<T, kVec>(p, b, b, d, W);
        }
    }
}

template <typename T, bool kVec>
__device__ __forceinline__ void conv_update_row(const dimsum_conv_update_params_t &p, int64_t b, int64_t sb, int64_t d, int W) {
    T *st = reinterpret_cast<T *>(p.conv_state_ptr) + sb * p.state_batch_stride + d * p.state_c_stride;
    const T xin = reinterpret_cast<const T *>(p.x_ptr)[b * p.x_batch_stride + d * p.x_c_stride];
    T s[4];     // the NEW state, right-aligned into 4 slots: s[3] = x, s[2] = the old last column, ...
    if constexpr (kVec) {
        const Raw4<T> old = ld4<T>(st);
        T o[4];
        __builtin_memcpy(o, &old, sizeof(o));
        s[0] = o[1]; s[1] = o[2]; s[2] = o[3]; s[3] = xin;
        Raw4<T> nw;
        __builtin_memcpy(&nw, s, sizeof(s));
        if constexpr (sizeof(T) == 4) *reinterpret_cast<float4 *>(st) = nw.r;
        else *reinterpret_cast<uint2 *>(st) = nw.r;
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] = (k >= 4 - W) ? st[(k - (4 - W) + 1) * p.state_w_stride] : from_f32<T>(0.f);
        s[3] = xin;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k >= 4 - W) st[(k - (4 - W)) * p.state_w_stride] = s[k];
    }
    const float *wp = reinterpret_cast<const float *>(p.weight_ptr) + d * p.weight_c_stride;
    float acc = p.bias_ptr ? reinterpret_cast<const float *>(p.bias_ptr)[d] : 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k >= 4 - W) acc = fmaf(wp[(k - (4 - W)) * p.weight_width_stride], to_f32<T>(s[k]), acc);
    if (p.silu_activation) acc *= sigmoidf_fast(acc);      // out / (1 + exp(-out)), as in the sequence kernel (causal_conv1d.hip)
    reinterpret_cast<T *>(p.out_ptr)[b * p.out_batch_stride + d * p.out_c_stride] = from_f32<T>(acc);
}

// ---------------------------------------------------------------------------------------------------------------------
struct step_args_t {
    dimsum_state_update_params_t p;
    dimsum_state_update_ext_t e;
};

// T: x / dt / z / out, TS: the state, TB: B and C. kVec: the rows of state, A, B and C start 4-element aligned and run with stride 1
template <typename T, typename TS, typename TB, bool kVec>
__device__ __forceinline__ void state_update_row(const dimsum_state_update_params_t &p, const dimsum_state_update_ext_t &e, int64_t b, int64_t sb,
                                                 int64_t d);

template <typename T, typename TS, typename TB, bool kVec, bool kSlots>
__global__ __launch_bounds__(kStepBlock) void selective_state_update_kernel(const std::conditional_t<kSlots, slots_args_t<step_args_t>, step_args_t> a) {
    const dimsum_state_update_params_t &p = step_base(a).p;
    const dimsum_state_update_ext_t &e = step_base(a).e;
    const int64_t d = (int64_t)blockIdx.x * kStepBlock + threadIdx.x;
    if (d >= p.dim) return;
    for (int64_t b = blockIdx.y; b < p.batch; b += gridDim.y) {
        if constexpr (kSlots) {
            const int32_t slot = a.slots[b * a.slots_stride];
            if (slot < 0) reinterpret_cast<T *>(p.out_ptr)[b * p.out_batch_stride + d * p.out_d_stride] = from_f32<T>(0.f);      // a padding row
            else state_update_row<T, TS, TB, kVec>(p, e, b, slot, d);
        } else {
            state_update_row<T, TS, TB, kVec>(p, e, b, b, d);
        }
    }
}

template <typename T, typename TS, typename TB, bool kVec>
__device__ __forceinline__ void state_update_row(const dimsum_state_update_params_t &p, const dimsum_state_update_ext_t &e, int64_t b, int64_t sb,
                                                 int64_t d) {
    const int N = p.dstate;
    const float x = to_f32<T>(reinterpret_cast<const T *>(p.x_ptr)[b * p.x_batch_stride + d * p.x_d_stride]);
    float dt;
    if (e.dt_w_ptr) {       // dt_proj formed here: dt = dt_w[d, :] . dt_x[b, :]
        const float *w = reinterpret_cast<const float *>(e.dt_w_ptr) + d * e.dt_w_d_stride;
        const T *v = reinterpret_cast<const T *>(e.dt_x_ptr) + b * e.dt_x_batch_stride;
        dt = 0.f;
        for (int r = 0; r < e.dt_rank; ++r) dt = fmaf(w[r * e.dt_w_r_stride], to_f32<T>(v[r * e.dt_x_r_stride]), dt);
    } else {
        dt = to_f32<T>(reinterpret_cast<const T *>(p.dt_ptr)[b * p.dt_batch_stride + d * p.dt_d_stride]);
    }
    if (p.dt_bias_ptr) dt += reinterpret_cast<const float *>(p.dt_bias_ptr)[d];
    if (p.dt_softplus) dt = softplus_ref(dt);
    const float dtx = dt * x;

    TS *st = reinterpret_cast<TS *>(p.state_ptr) + sb * p.state_batch_stride + d * p.state_d_stride;
    const float *A = reinterpret_cast<const float *>(p.A_ptr) + d * p.A_d_stride;
    const TB *Bv = reinterpret_cast<const TB *>(p.B_ptr) + b * p.B_batch_stride;
    const TB *Cv = reinterpret_cast<const TB *>(p.C_ptr) + b * p.C_batch_stride;
    float acc = 0.f;
    int n0 = 0;
    if constexpr (kVec) {
        for (; n0 + 4 <= N; n0 += 4) {
            const f32x4 h = load4f<TS>(st + n0), av = load4f<float>(A + n0), bv = load4f<TB>(Bv + n0), cv = load4f<TB>(Cv + n0);
            f32x4 hn;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                hn.v[k] = fmaf(h.v[k], fast_exp(dt * av.v[k]), dtx * bv.v[k]);
                acc = fmaf(hn.v[k], cv.v[k], acc);
            }
            st4<TS>(st + n0, hn);
        }
    }
    for (int n = n0; n < N; ++n) {       // the whole row without kVec, else what follows its last whole piece
        const float h = to_f32<TS>(st[n * p.state_n_stride]);
        const float hn = fmaf(h, fast_exp(dt * A[n * p.A_n_stride]), dtx * to_f32<TB>(Bv[n * p.B_n_stride]));
        acc = fmaf(hn, to_f32<TB>(Cv[n * p.C_n_stride]), acc);
        st[n * p.state_n_stride] = from_f32<TS>(hn);
    }
    if (p.D_ptr) acc = fmaf(reinterpret_cast<const float *>(p.D_ptr)[d], x, acc);
    if (p.z_ptr) {
        const float z = to_f32<T>(reinterpret_cast<const T *>(p.z_ptr)[b * p.z_batch_stride + d * p.z_d_stride]);
        acc *= z * sigmoidf_fast(z);
    }
    reinterpret_cast<T *>(p.out_ptr)[b * p.out_batch_stride + d * p.out_d_stride] = from_f32<T>(acc);
}

// ---- host ----------------------------------------------------------------------------------------------------------
// rows whose starts are multiples of 4 elements from a 4-element aligned base, unit stride along the row
template <typename T> static bool rows_vec4(const void *ptr, int64_t inner, std::initializer_list<int64_t> outer) {
    if (inner != 1 || !aligned_to<T>(ptr, 4 * sizeof(T))) return false;
    for (int64_t s : outer)
        if (s % 4 != 0) return false;
    return true;
}

static dim3 step_grid(int batch, int dim) {
    return dim3((unsigned)(((int64_t)dim + kStepBlock - 1) / kStepBlock), (unsigned)(batch < 65535 ? batch : 65535));
}

// slots != nullptr: the slot form. The predicates are the same ones, on the pool: its slot stride takes the batch stride's place
template <typename T> static int launch_conv_update(const dimsum_conv_update_params_t &p, hipStream_t s, const int32_t *slots = nullptr,
                                                    int64_t slots_stride = 0) {
    const dim3 grid = step_grid(p.batch, p.dim);
    const bool vec = p.width == 4 && rows_vec4<T>(p.conv_state_ptr, p.state_w_stride, {p.state_batch_stride, p.state_c_stride});
    if (slots) {
        const slots_args_t<dimsum_conv_update_params_t> a = {p, slots, slots_stride};
        if (vec) hipLaunchKernelGGL((causal_conv1d_update_kernel<T, true, true>), grid, dim3(kStepBlock), 0, s, a);
        else hipLaunchKernelGGL((causal_conv1d_update_kernel<T, false, true>), grid, dim3(kStepBlock), 0, s, a);
    } else if (vec) hipLaunchKernelGGL((causal_conv1d_update_kernel<T, true, false>), grid, dim3(kStepBlock), 0, s, p);
    else hipLaunchKernelGGL((causal_conv1d_update_kernel<T, false, false>), grid, dim3(kStepBlock), 0, s, p);
    return launch_status();
}

template <typename T, typename TS, typename TB>
static int launch_state_update(const step_args_t &a, hipStream_t s, const int32_t *slots = nullptr, int64_t slots_stride = 0) {
    const dimsum_state_update_params_t &p = a.p;
    const dim3 grid = step_grid(p.batch, p.dim);
    const bool vec = p.dstate >= 4 && rows_vec4<TS>(p.state_ptr, p.state_n_stride, {p.state_batch_stride, p.state_d_stride}) &&
                     rows_vec4<float>(p.A_ptr, p.A_n_stride, {p.A_d_stride}) && rows_vec4<TB>(p.B_ptr, p.B_n_stride, {p.B_batch_stride}) &&
                     rows_vec4<TB>(p.C_ptr, p.C_n_stride, {p.C_batch_stride});
    if (slots) {
        const slots_args_t<step_args_t> sa = {a, slots, slots_stride};
        if (vec) hipLaunchKernelGGL((selective_state_update_kernel<T, TS, TB, true, true>), grid, dim3(kStepBlock), 0, s, sa);
        else hipLaunchKernelGGL((selective_state_update_kernel<T, TS, TB, false, true>), grid, dim3(kStepBlock), 0, s, sa);
    } else if (vec) hipLaunchKernelGGL((selective_state_update_kernel<T, TS, TB, true, false>), grid, dim3(kStepBlock), 0, s, a);
    else hipLaunchKernelGGL((selective_state_update_kernel<T, TS, TB, false, false>), grid, dim3(kStepBlock), 0, s, a);
    return launch_status();
}

// state and B / C are either f32 or of the I/O dtype
template <typename T> static int dispatch_state_update(const step_args_t &a, hipStream_t s, const int32_t *slots = nullptr, int64_t slots_stride = 0) {
    const bool s32 = a.p.state_dtype == DIMSUM_F32, b32 = a.p.bc_dtype == DIMSUM_F32;
    if constexpr (sizeof(T) == 4) return launch_state_update<float, float, float>(a, s, slots, slots_stride);
    else if (s32) return b32 ? launch_state_update<T, float, float>(a, s, slots, slots_stride) : launch_state_update<T, float, T>(a, s, slots, slots_stride);
    else return b32 ? launch_state_update<T, T, float>(a, s, slots, slots_stride) : launch_state_update<T, T, T>(a, s, slots, slots_stride);
}

// the checks of the two plain entry points, shared with their slot forms (p.struct_size is the caller's business)
static int conv_update_check(const dimsum_conv_update_params_t *p) {
    if (!p->x_ptr || !p->weight_ptr || !p->conv_state_ptr || !p->out_ptr) return DIMSUM_ERR_NULL;
    if (p->width < 2 || p->width > 4) return DIMSUM_ERR_SHAPE;      // causal_conv1d.cpp:537
    if (p->batch < 1 || p->dim < 1) return DIMSUM_ERR_SHAPE;
    if (p->dtype < DIMSUM_F32 || p->dtype > DIMSUM_BF16) return DIMSUM_ERR_DTYPE;
    return DIMSUM_OK;
}

static int conv_update_run(const dimsum_conv_update_params_t &p, hipStream_t s, const int32_t *slots, int64_t slots_stride) {
    switch (p.dtype) {
        case DIMSUM_F32: return launch_conv_update<float>(p, s, slots, slots_stride);
        case DIMSUM_F16: return launch_conv_update<__half>(p, s, slots, slots_stride);
        default: return launch_conv_update<__hip_bfloat16>(p, s, slots, slots_stride);
    }
}

static int state_update_run(const dimsum_state_update_params_t *p, hipStream_t s, const int32_t *slots, int64_t slots_stride) {
    step_args_t a;
    a.p = *p;
    const int rc = ext_from(p->ext, a.e);
    if (rc != DIMSUM_OK) return rc;
    a.p.ext = nullptr;
    if (!p->state_ptr || !p->x_ptr || !p->A_ptr || !p->B_ptr || !p->C_ptr || !p->out_ptr) return DIMSUM_ERR_NULL;
    if (a.e.dt_w_ptr ? !a.e.dt_x_ptr : !p->dt_ptr) return DIMSUM_ERR_NULL;
    if (p->dstate < 1 || p->dstate > 256 || p->batch < 1 || p->dim < 1) return DIMSUM_ERR_SHAPE;
    if (a.e.dt_w_ptr && a.e.dt_rank < 1) return DIMSUM_ERR_SHAPE;
    if (p->dtype < DIMSUM_F32 || p->dtype > DIMSUM_BF16) return DIMSUM_ERR_DTYPE;
    if ((p->state_dtype != DIMSUM_F32 && p->state_dtype != p->dtype) || (p->bc_dtype != DIMSUM_F32 && p->bc_dtype != p->dtype)) return DIMSUM_ERR_DTYPE;
    switch (p->dtype) {
        case DIMSUM_F32: return dispatch_state_update<float>(a, s, slots, slots_stride);
        case DIMSUM_F16: return dispatch_state_update<__half>(a, s, slots, slots_stride);
        default: return dispatch_state_update<__hip_bfloat16>(a, s, slots, slots_stride);
    }
}

}  // namespace dimsum

extern "C" int dimsum_causal_conv1d_update(const dimsum_conv_update_params_t *p, void *stream) {
    using namespace dimsum;
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_conv_update_params_t)) return DIMSUM_ERR_ABI;
    const int rc = conv_update_check(p);
    if (rc != DIMSUM_OK) return rc;
    return conv_update_run(*p, reinterpret_cast<hipStream_t>(stream), nullptr, 0);
}

extern "C" int dimsum_selective_state_update(const dimsum_state_update_params_t *p, void *stream) {
    using namespace dimsum;
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_state_update_params_t)) return DIMSUM_ERR_ABI;
    return state_update_run(p, reinterpret_cast<hipStream_t>(stream), nullptr, 0);
}

extern "C" int dimsum_causal_conv1d_update_slots(const dimsum_conv_update_slots_params_t *v, void *stream) {
    using namespace dimsum;
    int rc = slots_check(v);
    if (rc != DIMSUM_OK) return rc;
    rc = conv_update_check(&v->conv);
    if (rc != DIMSUM_OK) return rc;
    return conv_update_run(v->conv, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const int32_t *>(v->slots_ptr), v->slots_stride);
}

extern "C" int dimsum_selective_state_update_slots(const dimsum_state_update_slots_params_t *v, void *stream) {
    using namespace dimsum;
    const int rc = slots_check(v);
    if (rc != DIMSUM_OK) return rc;
    return state_update_run(&v->update, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const int32_t *>(v->slots_ptr), v->slots_stride);
}
