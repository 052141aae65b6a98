// causal_conv1d.hip -- depthwise causal conv1d (width 2..4) + bias + SiLU, forward, backward and the forward on a carried state, for gfx950.
//
// Replaces causal_conv1d_cuda.causal_conv1d_fwd[_cond] / _bwd[_cond] (causal-conv1d/csrc/causal_conv1d.cpp:221-509;
// kernels causal_conv1d_fwd.cu:39-130, causal_conv1d_bwd.cu:46-240):
//     out[b,d,t] = act(bias[d] + sum_k W[d,k] * x[b,d,t-(width-1-k)]),   x[.., t<0] = 0,   act = SiLU or identity
// Pure streaming: 2*B*D*L*s bytes forward, 3*B*D*L*s backward.
//
// MI355X design: one wave64 walks (b,d) rows, four at a time with their loads issued back to back, 256 elements per step
// and row (16 B per lane, fully coalesced 1-KiB requests);
// the 3-element halo comes from the neighbouring lane (one cross-lane move per value) and, across 256-element steps,
// from registers -- no LDS, no block barrier (the reference stages a 128-thread block through shared memory and idles
// half of it at L = 256). Weights and bias are wave-uniform (scalar loads). The backward walks the row from the end
// so the gradient halo is carried the same way, keeps dweight/dbias partial sums in registers across all the batch
// rows a wave owns and issues ONE atomic per wave per tap (the reference: one per block per row).
//
// Packed rows (dimsum_causal_conv1d_varlen_fwd / _bwd, kVarlen): a per-token sequence id rides along, loaded like x (16 bytes per lane, its
// halo from the neighbouring lane and across steps from registers). Tap j of position t counts iff the ids of t-j .. t are pairwise equal
// from one position to the next (no boundary in (t-j, t]); a masked value is replaced by 0 with a select, never multiplied away, so what
// lies beyond a boundary cannot reach the result whatever it holds. Ids are only compared. The backward applies the same rule to the
// gradient halo, which comes from the right. kVarlen = false compiles to the kernels as they were.
//
// Per-segment states (dimsum_causal_conv1d_varlen_states_fwd, kEmit on top of kVarlen, forward only): a second int32 row, end_slots, is
// loaded like the ids. For output element t the lane holds the masked taps x[t], k1 ? x[t-1] : 0, ... -- the conv state of a segment that
// ends at t, zero-padded on the left -- and where end_slots[t] >= 0 it stores the last `width` of them to pool[slot, d, 0 : width),
// x[t] last (the layout causal_conv1d_update shifts). The values are the loaded x elements: widened to fp32 on the load and narrowed back
// on the store, which is the identity on every T. A row the kernel clamped onto the last one stores nothing. kEmit = false compiles to the
// kernels as they were.
//
// Resumed segments (dimsum_causal_conv1d_varlen_resume_fwd, kStart on top of kEmit, forward only): a third int32 row, start_slots, travels as
// the ids do (16 bytes per lane, the halo from the neighbouring lane and across steps from registers), because the output at t + e needs the
// entry of a segment that began up to width - 2 positions earlier. Where such an entry s >= 0 lies dl <= 2 positions before an output of
// its segment, the taps k > dl -- masked to 0 without it -- are loaded from init[s, d, width - (k - dl)]; the same taps are what kEmit
// stores, so a stored state is the last `width` values of concat(init[s], the segment). The loads sit behind a per-lane branch that only a
// lane with a start entry in its window takes. init must not overlap a slot stored in the same launch: the lanes that read a slot are not
// the lane that writes it. kStart = false compiles to the kernels as they were.
#include "common.hpp"

#include <type_traits>

namespace dimsum {

__device__ __forceinline__ float lane_up(float v, float carry_for_lane0) {   // value of lane-1, lane 0 gets the carry
    const float t = __shfl_up(v, 1, kWave);
    return (threadIdx.x & (kWave - 1)) == 0 ? carry_for_lane0 : t;
}
__device__ __forceinline__ float lane_down(float v, float carry_for_lane63) {
    const float t = __shfl_down(v, 1, kWave);
    return (threadIdx.x & (kWave - 1)) == kWave - 1 ? carry_for_lane63 : t;
}
__device__ __forceinline__ int lane_up_i(int v, int carry_for_lane0) {
    const int t = __shfl_up(v, 1, kWave);
    return (threadIdx.x & (kWave - 1)) == 0 ? carry_for_lane0 : t;
}
__device__ __forceinline__ int lane_down_i(int v, int carry_for_lane63) {
    const int t = __shfl_down(v, 1, kWave);
    return (threadIdx.x & (kWave - 1)) == kWave - 1 ? carry_for_lane63 : t;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}
__device__ __forceinline__ float silu_grad(float pre) {   // d/dpre [pre * sigmoid(pre)]   (causal_conv1d_bwd.cu:153-164)
    const float sg = sigmoidf_fast(pre);
    return sg * (1.0f + pre * (1.0f - sg));
}

template <typename T, bool kVec>
__device__ __forceinline__ f32x4 load_row4(const T *row, int t, int L) {
    if constexpr (kVec) {
        if (t < L) return widen(ld4<T>(row + t));
        return {{0.f, 0.f, 0.f, 0.f}};
    } else {
        f32x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) r.v[e] = (t + e < L) ? to_f32<T>(row[t + e]) : 0.f;
        return r;
    }
}
template <typename T, bool kVec>
__device__ __forceinline__ void store_row4(T *row, int t, int L, const f32x4 &v) {
    if constexpr (kVec) {
        if (t < L) st4<T>(row + t, v);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (t + e < L) row[t + e] = from_f32<T>(v.v[e]);
    }
}

// four sequence ids of a packed row, positions t .. t+3 (beyond the row: 0 -- nothing is stored there and the gradients there are 0)
struct alignas(16) i32x4 { int v[4]; };
template <bool kVec> __device__ __forceinline__ i32x4 load_ids4(const int32_t *row, int t, int L) {
    i32x4 r = {{0, 0, 0, 0}};
    if constexpr (kVec) {
        if (t < L) r = *reinterpret_cast<const i32x4 *>(row + t);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (t + e < L) r.v[e] = row[t + e];
    }
    return r;
}

// the kernel argument of the packed-row kernels: the plain one + the ids, (batch, seqlen) int32 with unit stride along seqlen
struct conv_varlen_args_t {
    dimsum_conv_params_t p;
    const int32_t *seq_idx;
    int64_t seq_batch_stride;
};
struct conv_varlen_bwd_args_t {
    dimsum_conv_bwd_params_t q;
    const int32_t *seq_idx;
    int64_t seq_batch_stride;
};
// the kEmit forward: + end_slots, (batch, seqlen) int32 laid out like seq_idx, and the pool (num_slots, dim, width) of x's dtype
struct conv_states_args_t {
    conv_varlen_args_t v;
    const int32_t *end_slots;
    int64_t end_batch_stride;
    void *pool;
    int64_t pool_slot_stride, pool_c_stride, pool_w_stride;
};
// the kStart forward: + start_slots, laid out like end_slots, and init (n_init, dim, width) of x's dtype. Derived: conv_base / conv_ids and
// every a.<kEmit field> of the kernel serve it as they are
struct conv_resume_args_t : conv_states_args_t {
    const int32_t *start_slots;
    int64_t start_batch_stride;
    const void *init;
    int64_t init_slot_stride, init_c_stride, init_w_stride;
};
__host__ __device__ __forceinline__ const dimsum_conv_params_t &conv_base(const conv_states_args_t &a) { return a.v.p; }
__device__ __forceinline__ const conv_varlen_args_t &conv_ids(const conv_varlen_args_t &a) { return a; }
__device__ __forceinline__ const conv_varlen_args_t &conv_ids(const conv_states_args_t &a) { return a.v; }
__host__ __device__ __forceinline__ const dimsum_conv_params_t &conv_base(const dimsum_conv_params_t &a) { return a; }
__host__ __device__ __forceinline__ const dimsum_conv_params_t &conv_base(const conv_varlen_args_t &a) { return a.p; }
__host__ __device__ __forceinline__ const dimsum_conv_bwd_params_t &conv_base(const dimsum_conv_bwd_params_t &a) { return a; }
__host__ __device__ __forceinline__ const dimsum_conv_bwd_params_t &conv_base(const conv_varlen_bwd_args_t &a) { return a.q; }

// ---------------------------------------------------------------------------------------------------------------------
template <typename T, bool kVec, bool kVarlen, bool kEmit = false, bool kStart = false>
__global__ __launch_bounds__(256) void causal_conv1d_fwd_kernel(
    const std::conditional_t<kStart, conv_resume_args_t,
                             std::conditional_t<kEmit, conv_states_args_t, std::conditional_t<kVarlen, conv_varlen_args_t, dimsum_conv_params_t>>> a) {
    static_assert(!kEmit || kVarlen, "per-segment states belong to packed rows");
    static_assert(!kStart || kEmit, "resumed segments ride on the per-segment-states kernel");
    const dimsum_conv_params_t &p = conv_base(a);
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t rows = (int64_t)p.batch * p.dim;
    const int L = p.seqlen, W = p.width;
    // kR rows per wave and iteration, a grid stride apart: their loads are issued back to back (kR x 1 KiB in flight per wave)
    constexpr int kR = 4;
    const int64_t gstride = (int64_t)gridDim.x * 4;
    for (int64_t row0 = (int64_t)blockIdx.x * 4 + wave; row0 < rows; row0 += kR * gstride) {
        const T *x[kR];
        T *o[kR];
        float w4[kR][4], bias[kR], c1[kR], c2[kR], c3[kR];   // taps right-aligned into 4 slots: w4[3] multiplies x[t], w4[2] x[t-1], ...
        bool ok[kR];
        const int32_t *sq[kR];                               // kVarlen: the row's ids and those of t0-1, t0-2, t0-3 carried like c1 .. c3
        int i1[kR], i2[kR], i3[kR];
        const int32_t *eq[kR];                               // kEmit: the row's end_slots and its channel's place in the pool
        T *pl[kR];
        const int32_t *bq[kR];                               // kStart: the row's start_slots, those of t0-1, t0-2 carried like i1, i2 (an entry three
        int s1[kR], s2[kR];                                  // back serves no tap), and its channel's place in init
        const T *pin[kR];
#pragma unroll
        for (int r = 0; r < kR; ++r) {
            const int64_t row = min(row0 + r * gstride, rows - 1);
            ok[r] = row0 + r * gstride < rows;
            const int b = (int)(row / p.dim), d = (int)(row - (int64_t)b * p.dim);
            x[r] = reinterpret_cast<const T *>(p.x_ptr) + (int64_t)b * p.x_batch_stride + (int64_t)d * p.x_c_stride;
            o[r] = reinterpret_cast<T *>(p.out_ptr) + (int64_t)b * p.out_batch_stride + (int64_t)d * p.out_c_stride;
            const float *wp = reinterpret_cast<const float *>(p.weight_ptr) + (int64_t)d * p.weight_c_stride;
#pragma unroll
            for (int k = 0; k < 4; ++k) w4[r][k] = (k >= 4 - W) ? wp[(k - (4 - W)) * p.weight_width_stride] : 0.f;
            bias[r] = p.bias_ptr ? reinterpret_cast<const float *>(p.bias_ptr)[d] : 0.f;
            c1[r] = c2[r] = c3[r] = 0.f;                     // x[t0-1], x[t0-2], x[t0-3] carried across 256-element steps
            if constexpr (kVarlen) {
                sq[r] = conv_ids(a).seq_idx + (int64_t)b * conv_ids(a).seq_batch_stride;
                i1[r] = i2[r] = i3[r] = 0;                   // before the row: the x halo there is 0, whatever the comparison says
            }
            if constexpr (kEmit) {
                eq[r] = a.end_slots + (int64_t)b * a.end_batch_stride;
                pl[r] = reinterpret_cast<T *>(a.pool) + (int64_t)d * a.pool_c_stride;
            }
            if constexpr (kStart) {
                bq[r] = a.start_slots + (int64_t)b * a.start_batch_stride;
                pin[r] = reinterpret_cast<const T *>(a.init) + (int64_t)d * a.init_c_stride;
                s1[r] = s2[r] = -1;                          // before the row: no segment begins there
            }
        }
        for (int t0 = 0; t0 < L; t0 += 4 * kWave) {
            const int t = t0 + lane * 4;
            f32x4 v[kR];
            i32x4 id[kR], es[kR], bs[kR];
#pragma unroll
            for (int r = 0; r < kR; ++r) {
                v[r] = load_row4<T, kVec>(x[r], t, L);
                if constexpr (kVarlen) id[r] = load_ids4<kVec>(sq[r], t, L);
                if constexpr (kEmit) es[r] = load_ids4<kVec>(eq[r], t, L);
                if constexpr (kStart) bs[r] = load_ids4<kVec>(bq[r], t, L);
            }
#pragma unroll
            for (int r = 0; r < kR; ++r) {
                const float m1 = lane_up(v[r].v[3], c1[r]), m2 = lane_up(v[r].v[2], c2[r]), m3 = lane_up(v[r].v[1], c3[r]);
                f32x4 q;
                if constexpr (kVarlen) {
                    // the mask on both halo routes: the ids of t-1 .. t-3 come from the neighbouring lane or, for lane 0, from the step before
                    const int j1 = lane_up_i(id[r].v[3], i1[r]), j2 = lane_up_i(id[r].v[2], i2[r]), j3 = lane_up_i(id[r].v[1], i3[r]);
                    const int I[7] = {j3, j2, j1, id[r].v[0], id[r].v[1], id[r].v[2], id[r].v[3]};          // ids of t-3 .. t+3
                    const float xs[7] = {m3, m2, m1, v[r].v[0], v[r].v[1], v[r].v[2], v[r].v[3]};         // x[t-3] .. x[t+3]
                    int S[6];                                                                            // kStart: start entries of t-2 .. t+3
                    if constexpr (kStart) {
                        S[0] = lane_up_i(bs[r].v[2], s2[r]), S[1] = lane_up_i(bs[r].v[3], s1[r]);
#pragma unroll
                        for (int e = 0; e < 4; ++e) S[2 + e] = bs[r].v[e];
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const bool k1 = I[e + 3] == I[e + 2], k2 = k1 && I[e + 2] == I[e + 1], k3 = k2 && I[e + 1] == I[e];
                        if constexpr (!kStart) {
                        q.v[e] = bias[r] + w4[r][0] * (k3 ? xs[e] : 0.f) + w4[r][1] * (k2 ? xs[e + 1] : 0.f) + w4[r][2] * (k1 ? xs[e + 2] : 0.f) +
                                 w4[r][3] * xs[e + 3];
                        if constexpr (kEmit) {
                            // a segment ends at t + e: its conv state is the masked taps. load_ids4 reads 0 beyond the row, a valid slot: t + e < L
                            if (ok[r] && t + e < L && es[r].v[e] >= 0) {
                                T *st = pl[r] + (int64_t)es[r].v[e] * a.pool_slot_stride;
                                const float tap[4] = {k3 ? xs[e] : 0.f, k2 ? xs[e + 1] : 0.f, k1 ? xs[e + 2] : 0.f, xs[e + 3]};
#pragma unroll
                                for (int k = 0; k < 4; ++k)
                                    if (k >= 4 - W) st[(int64_t)(k - (4 - W)) * a.pool_w_stride] = from_f32<T>(tap[k]);
                            }
                        }
                        } else {
                        float tb[4] = {xs[e + 3], k1 ? xs[e + 2] : 0.f, k2 ? xs[e + 1] : 0.f, k3 ? xs[e] : 0.f};      // the masked taps x[t+e-k]
                        {
                            // the nearest start entry at t+e-dl, dl <= 2, with no boundary in (t+e-dl, t+e]: this output's segment is resumed and
                            // its taps k > dl reach into init. The guards of the kEmit stores: load_ids4 reads 0 beyond the row, a valid slot
                            const int dl = S[e + 2] >= 0 ? 0 : (k1 && S[e + 1] >= 0) ? 1 : (k2 && S[e] >= 0) ? 2 : -1;
                            if (ok[r] && t + e < L && dl >= 0) {
                                const T *in = pin[r] + (int64_t)S[e + 2 - dl] * a.init_slot_stride;
#pragma unroll
                                for (int k = 1; k < 4; ++k)                   // x[f - m] = init[s, d, W - m] with f the segment's first position, m = k - dl
                                    if (k > dl && k < W) tb[k] = to_f32<T>(in[(int64_t)(W - (k - dl)) * a.init_w_stride]);
                            }
                        }
                        q.v[e] = bias[r] + w4[r][0] * tb[3] + w4[r][1] * tb[2] + w4[r][2] * tb[1] + w4[r][3] * tb[0];
                        // a segment ends at t + e: its conv state is these taps, the substituted ones among them
                        if (ok[r] && t + e < L && es[r].v[e] >= 0) {
                            T *st = pl[r] + (int64_t)es[r].v[e] * a.pool_slot_stride;
#pragma unroll
                            for (int k = 0; k < 4; ++k)
                                if (k < W) st[(int64_t)(W - 1 - k) * a.pool_w_stride] = from_f32<T>(tb[k]);
                        }
                        }
                    }
                    i1[r] = __shfl(id[r].v[3], kWave - 1, kWave);
                    i2[r] = __shfl(id[r].v[2], kWave - 1, kWave);
                    i3[r] = __shfl(id[r].v[1], kWave - 1, kWave);
                    if constexpr (kStart) {
                        s1[r] = __shfl(bs[r].v[3], kWave - 1, kWave);
                        s2[r] = __shfl(bs[r].v[2], kWave - 1, kWave);
                    }
                } else {
                q.v[0] = bias[r] + w4[r][0] * m3 + w4[r][1] * m2 + w4[r][2] * m1 + w4[r][3] * v[r].v[0];
                q.v[1] = bias[r] + w4[r][0] * m2 + w4[r][1] * m1 + w4[r][2] * v[r].v[0] + w4[r][3] * v[r].v[1];
                q.v[2] = bias[r] + w4[r][0] * m1 + w4[r][1] * v[r].v[0] + w4[r][2] * v[r].v[1] + w4[r][3] * v[r].v[2];
                q.v[3] = bias[r] + w4[r][0] * v[r].v[0] + w4[r][1] * v[r].v[1] + w4[r][2] * v[r].v[2] + w4[r][3] * v[r].v[3];
                }
                if (p.silu_activation) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) q.v[e] *= sigmoidf_fast(q.v[e]);   // out / (1 + exp(-out)), causal_conv1d_fwd.cu:113-118
                }
                if (ok[r]) store_row4<T, kVec>(o[r], t, L, q);
                c1[r] = __shfl(v[r].v[3], kWave - 1, kWave);
                c2[r] = __shfl(v[r].v[2], kWave - 1, kWave);
                c3[r] = __shfl(v[r].v[1], kWave - 1, kWave);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// the forward on a carried state (dimsum_causal_conv1d_chunk): the same row walk, the left halo of the first 256-element step taken from
// conv_state instead of zeros, and conv_state <- the last W values of concat(conv_state, x) afterwards. One row per wave and pass (a
// continuation is a short sequence: the rows, not the loads of one wave, fill the chip). Lane k < W is the only lane that reads or
// writes conv_state[k] of the wave's row -- the others get the old values through cross-lane moves -- so the in-place update is
// ordered by that lane's own program order. The values travel as raw bits: moved, never converted.
template <typename T> __device__ __forceinline__ unsigned raw_bits(T v) {
    if constexpr (sizeof(T) == 4) {
        unsigned r;
        __builtin_memcpy(&r, &v, 4);
        return r;
    } else {
        unsigned short r;
        __builtin_memcpy(&r, &v, 2);
        return r;
    }
}
template <typename T> __device__ __forceinline__ T from_bits(unsigned r) {
    T v;
    if constexpr (sizeof(T) == 4) {
        __builtin_memcpy(&v, &r, 4);
    } else {
        const unsigned short h = (unsigned short)r;
        __builtin_memcpy(&v, &h, 2);
    }
    return v;
}

template <typename T, bool kVec>
__global__ __launch_bounds__(256) void causal_conv1d_chunk_kernel(const dimsum_conv_chunk_params_t p) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t rows = (int64_t)p.batch * p.dim;
    const int L = p.seqlen, W = p.width;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < rows; row += (int64_t)gridDim.x * 4) {
        const int b = (int)(row / p.dim), d = (int)(row - (int64_t)b * p.dim);
        const T *x = reinterpret_cast<const T *>(p.x_ptr) + (int64_t)b * p.x_batch_stride + (int64_t)d * p.x_c_stride;
        T *o = reinterpret_cast<T *>(p.out_ptr) + (int64_t)b * p.out_batch_stride + (int64_t)d * p.out_c_stride;
        T *st = reinterpret_cast<T *>(p.conv_state_ptr) + (int64_t)b * p.state_batch_stride + (int64_t)d * p.state_c_stride;
        const float *wp = reinterpret_cast<const float *>(p.weight_ptr) + (int64_t)d * p.weight_c_stride;
        float w4[4];                                             // taps right-aligned into 4 slots, as in the forward kernel
#pragma unroll
        for (int k = 0; k < 4; ++k) w4[k] = (k >= 4 - W) ? wp[(k - (4 - W)) * p.weight_width_stride] : 0.f;
        const float bias = p.bias_ptr ? reinterpret_cast<const float *>(p.bias_ptr)[d] : 0.f;
        const unsigned own = lane < W ? raw_bits<T>(st[lane * p.state_w_stride]) : 0u;      // the old state, element `lane`
        // x[-1], x[-2], x[-3] = the state's last W - 1 elements (its first one has left the window); what a narrower conv has no tap for is 0
        const float s1 = to_f32<T>(from_bits<T>(__shfl(own, W - 1, kWave)));
        const float s2 = to_f32<T>(from_bits<T>(__shfl(own, W >= 3 ? W - 2 : 0, kWave)));
        const float s3 = to_f32<T>(from_bits<T>(__shfl(own, 1, kWave)));
        float c1 = s1, c2 = W >= 3 ? s2 : 0.f, c3 = W >= 4 ? s3 : 0.f;
        for (int t0 = 0; t0 < L; t0 += 4 * kWave) {
            const int t = t0 + lane * 4;
            const f32x4 v = load_row4<T, kVec>(x, t, L);
            const float m1 = lane_up(v.v[3], c1), m2 = lane_up(v.v[2], c2), m3 = lane_up(v.v[1], c3);
            f32x4 q;
            q.v[0] = bias + w4[0] * m3 + w4[1] * m2 + w4[2] * m1 + w4[3] * v.v[0];
            q.v[1] = bias + w4[0] * m2 + w4[1] * m1 + w4[2] * v.v[0] + w4[3] * v.v[1];
            q.v[2] = bias + w4[0] * m1 + w4[1] * v.v[0] + w4[2] * v.v[1] + w4[3] * v.v[2];
            q.v[3] = bias + w4[0] * v.v[0] + w4[1] * v.v[1] + w4[2] * v.v[2] + w4[3] * v.v[3];
            if (p.silu_activation) {
#pragma unroll
                for (int e = 0; e < 4; ++e) q.v[e] *= sigmoidf_fast(q.v[e]);
            }
            store_row4<T, kVec>(o, t, L, q);
            c1 = __shfl(v.v[3], kWave - 1, kWave);
            c2 = __shfl(v.v[2], kWave - 1, kWave);
            c3 = __shfl(v.v[1], kWave - 1, kWave);
        }
        // the new state: element k = element k + L of concat(old state, x) -- an old value (seqlen < width) or x[k + L - W]
        const int64_t j = (int64_t)lane + L;
        const unsigned moved = __shfl(own, j < W ? (int)j : 0, kWave);
        if (lane < W) st[lane * p.state_w_stride] = j < W ? from_bits<T>(moved) : x[j - W];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// backward. grid = (dim, n_split): wave (d, s) owns batch rows b = s, s + n_split*4, ... of channel d.
template <typename T, bool kVec, bool kVarlen>
__global__ __launch_bounds__(256) void causal_conv1d_bwd_kernel(const std::conditional_t<kVarlen, conv_varlen_bwd_args_t, dimsum_conv_bwd_params_t> a) {
    const dimsum_conv_bwd_params_t &q = conv_base(a);
    const dimsum_conv_params_t &p = q.fwd;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int d = blockIdx.x;
    const int L = p.seqlen, W = p.width;
    const float *wp = reinterpret_cast<const float *>(p.weight_ptr) + (int64_t)d * p.weight_c_stride;
    float w4[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) w4[k] = (k >= 4 - W) ? wp[(k - (4 - W)) * p.weight_width_stride] : 0.f;
    const float bias = p.bias_ptr ? reinterpret_cast<const float *>(p.bias_ptr)[d] : 0.f;
    float dw[4] = {0.f, 0.f, 0.f, 0.f}, db = 0.f;
    const int n_steps = (L + 4 * kWave - 1) / (4 * kWave);

    for (int b = blockIdx.y * 4 + wave; b < p.batch; b += gridDim.y * 4) {
        const T *x = reinterpret_cast<const T *>(p.x_ptr) + (int64_t)b * p.x_batch_stride + (int64_t)d * p.x_c_stride;
        const T *go = reinterpret_cast<const T *>(q.dout_ptr) + (int64_t)b * q.dout_batch_stride + (int64_t)d * q.dout_c_stride;
        T *dx = reinterpret_cast<T *>(q.dx_ptr) + (int64_t)b * q.dx_batch_stride + (int64_t)d * q.dx_c_stride;
        float g1 = 0.f, g2 = 0.f, g3 = 0.f;   // g[t0+256], g[t0+257], g[t0+258] of the step processed before (later in time)
        const int32_t *sq = nullptr;          // kVarlen: the row's ids; those of t0+256 .. t0+258 carried like g1 .. g3
        int n1 = 0, n2 = 0, n3 = 0;
        if constexpr (kVarlen) sq = a.seq_idx + (int64_t)b * a.seq_batch_stride;
        for (int step = n_steps - 1; step >= 0; --step) {
            const int t0 = step * 4 * kWave, t = t0 + lane * 4;
            const f32x4 v = load_row4<T, kVec>(x, t, L);
            f32x4 g = load_row4<T, kVec>(go, t, L);
            // x halo from the left: neighbour lane, or straight from memory for lane 0 (3 scalar loads per 256 elements)
            float c1 = 0.f, c2 = 0.f, c3 = 0.f;
            if (t0 > 0) { c1 = to_f32<T>(x[t0 - 1]); c2 = to_f32<T>(x[t0 - 2]); c3 = to_f32<T>(x[t0 - 3]); }
            const float m1 = lane_up(v.v[3], c1), m2 = lane_up(v.v[2], c2), m3 = lane_up(v.v[1], c3);
            const float xs[7] = {m3, m2, m1, v.v[0], v.v[1], v.v[2], v.v[3]};   // x[t-3] .. x[t+3]
            if constexpr (kVarlen) {
                // ids of t-3 .. t+6: the left three like the x halo (neighbour lane, memory for lane 0), the right three like the gradient
                // halo (neighbour lane, the step processed before for lane 63). E[k]: no boundary at position t-2+k.
                const i32x4 id = load_ids4<kVec>(sq, t, L);
                int l1 = 0, l2 = 0, l3 = 0;
                if (t0 > 0) { l1 = sq[t0 - 1]; l2 = sq[t0 - 2]; l3 = sq[t0 - 3]; }
                const int I[10] = {lane_up_i(id.v[1], l3), lane_up_i(id.v[2], l2), lane_up_i(id.v[3], l1), id.v[0], id.v[1], id.v[2], id.v[3],
                                   lane_down_i(id.v[0], n1), lane_down_i(id.v[1], n2), lane_down_i(id.v[2], n3)};
                bool E[9];
#pragma unroll
                for (int k = 0; k < 9; ++k) E[k] = I[k] == I[k + 1];
                float xm[4][3];                                                  // x[t+e-1], x[t+e-2], x[t+e-3] as position t+e sees them
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const bool k1 = E[e + 2], k2 = k1 && E[e + 1], k3 = k2 && E[e];
                    xm[e][0] = k1 ? xs[e + 2] : 0.f;
                    xm[e][1] = k2 ? xs[e + 1] : 0.f;
                    xm[e][2] = k3 ? xs[e] : 0.f;
                    if (p.silu_activation) {
                        const float pre = bias + w4[0] * xm[e][2] + w4[1] * xm[e][1] + w4[2] * xm[e][0] + w4[3] * xs[e + 3];
                        g.v[e] *= silu_grad(pre);
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    db += g.v[e];
                    dw[0] = fmaf(g.v[e], xm[e][2], dw[0]);
                    dw[1] = fmaf(g.v[e], xm[e][1], dw[1]);
                    dw[2] = fmaf(g.v[e], xm[e][0], dw[2]);
                    dw[3] = fmaf(g.v[e], xs[e + 3], dw[3]);
                }
                const float p1 = lane_down(g.v[0], g1), p2 = lane_down(g.v[1], g2), p3 = lane_down(g.v[2], g3);
                const float gs[7] = {g.v[0], g.v[1], g.v[2], g.v[3], p1, p2, p3};   // g[t] .. g[t+6]
                f32x4 r;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    // g[t+e+j] reaches dx[t+e] iff no boundary in (t+e, t+e+j]
                    const bool k1 = E[e + 3], k2 = k1 && E[e + 4], k3 = k2 && E[e + 5];
                    r.v[e] = w4[3] * gs[e] + w4[2] * (k1 ? gs[e + 1] : 0.f) + w4[1] * (k2 ? gs[e + 2] : 0.f) + w4[0] * (k3 ? gs[e + 3] : 0.f);
                }
                store_row4<T, kVec>(dx, t, L, r);
                n1 = __shfl(id.v[0], 0, kWave);
                n2 = __shfl(id.v[1], 0, kWave);
                n3 = __shfl(id.v[2], 0, kWave);
            } else {
            if (p.silu_activation) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float pre = bias + w4[0] * xs[e] + w4[1] * xs[e + 1] + w4[2] * xs[e + 2] + w4[3] * xs[e + 3];
                    g.v[e] *= silu_grad(pre);
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                db += g.v[e];
#pragma unroll
                for (int k = 0; k < 4; ++k) dw[k] = fmaf(g.v[e], xs[e + k], dw[k]);
            }
            // dx[s] = sum_k w4[k] * g[s + 3 - k]  -> needs g[t+4], g[t+5], g[t+6] from the right neighbour
            const float p1 = lane_down(g.v[0], g1), p2 = lane_down(g.v[1], g2), p3 = lane_down(g.v[2], g3);
            const float gs[7] = {g.v[0], g.v[1], g.v[2], g.v[3], p1, p2, p3};   // g[t] .. g[t+6]
            f32x4 r;
#pragma unroll
            for (int e = 0; e < 4; ++e) r.v[e] = w4[3] * gs[e] + w4[2] * gs[e + 1] + w4[1] * gs[e + 2] + w4[0] * gs[e + 3];
            store_row4<T, kVec>(dx, t, L, r);
            }
            g1 = __shfl(g.v[0], 0, kWave);
            g2 = __shfl(g.v[1], 0, kWave);
            g3 = __shfl(g.v[2], 0, kWave);
        }
    }
    // one atomic per wave per tap (fp32 accumulators zero-filled by the caller, causal_conv1d.cpp:405-407)
    float *dwp = reinterpret_cast<float *>(q.dweight_ptr) + (int64_t)d * q.dweight_c_stride;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float s = wave_sum(dw[k]);
        if (lane == 0 && k >= 4 - W) atomicAdd(dwp + (k - (4 - W)) * q.dweight_width_stride, s);
    }
    if (q.dbias_ptr) {
        const float s = wave_sum(db);
        if (lane == 0) atomicAdd(reinterpret_cast<float *>(q.dbias_ptr) + d, s);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host. One check (conv_checks), one launch per direction (launch_conv_fwd / _bwd pick kVec), one dtype switch (dispatch_dtype). A new
// variant is a template flag on the kernel, an argument struct behind conv_base, and an entry point that adds its own checks around these.
template <typename T> static bool vec_ok(const void *ptr, int64_t s0, int64_t s1, int L) {
    return L % 4 == 0 && aligned_to<T>(ptr, 4 * sizeof(T)) && s0 % 4 == 0 && s1 % 4 == 0;
}
// the ids of a packed row are read as 16-byte vectors where x is: a 16-byte aligned base and a batch stride that keeps every row so
static bool ids_vec_ok(const void *ids, int64_t batch_stride) { return aligned_to<int32_t>(ids, 16) && batch_stride % 4 == 0; }
// a (batch, seqlen) int32 operand with unit stride along seqlen: its rows must not run backwards or overlap
static bool ids_stride_bad(int64_t batch_stride, const dimsum_conv_params_t &p) { return batch_stride < 0 || (p.batch > 1 && batch_stride < p.seqlen); }

// What the five seqlen-contiguous entry points share, after their own NULL / struct_size test, in this order: the pointers written to (out;
// q != nullptr, a backward: dout, dx, dweight), the inputs, width and sizes (causal_conv1d.cpp:248), the dtype, then with `packed` the ids
// (NULL, then a batch stride that lets rows overlap). DIMSUM_OK with batch == 0 is the caller's early return.
static int conv_checks(const dimsum_conv_params_t &p, const dimsum_conv_bwd_params_t *q, bool packed = false, const void *seq_idx = nullptr,
                       int64_t seq_batch_stride = 0) {
    if (q ? !q->dout_ptr || !q->dx_ptr || !q->dweight_ptr : !p.out_ptr) return DIMSUM_ERR_NULL;
    if (!p.x_ptr || !p.weight_ptr) return DIMSUM_ERR_NULL;
    if (p.width < 2 || p.width > 4 || p.batch < 0 || p.dim <= 0 || p.seqlen <= 0) return DIMSUM_ERR_SHAPE;
    if (p.dtype < DIMSUM_F32 || p.dtype > DIMSUM_BF16) return DIMSUM_ERR_DTYPE;
    if (packed && !seq_idx) return DIMSUM_ERR_NULL;
    if (packed && ids_stride_bad(seq_batch_stride, p)) return DIMSUM_ERR_STRIDE;
    return DIMSUM_OK;
}

// Args: dimsum_conv_params_t, conv_varlen_args_t (kVarlen), conv_states_args_t (kEmit) or conv_resume_args_t (kStart). ids_vec: every int32
// row operand of Args may be read as 16-byte vectors
template <typename T, bool kVarlen, bool kEmit, bool kStart = false, typename Args>
static int launch_conv_fwd(const Args &a, hipStream_t s, bool ids_vec = true) {
    const dimsum_conv_params_t &p = conv_base(a);
    const bool vec = ids_vec && vec_ok<T>(p.x_ptr, p.x_batch_stride, p.x_c_stride, p.seqlen) &&
                     vec_ok<T>(p.out_ptr, p.out_batch_stride, p.out_c_stride, p.seqlen);
    const int64_t rows = (int64_t)p.batch * p.dim;
    const int grid = (int)((rows + 15) / 16 < 256 * 32 ? (rows + 15) / 16 : 256 * 32);   // 4 waves x 4 rows per workgroup and pass (a 2x larger grid measured slower)
    if (vec) hipLaunchKernelGGL((causal_conv1d_fwd_kernel<T, true, kVarlen, kEmit, kStart>), dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((causal_conv1d_fwd_kernel<T, false, kVarlen, kEmit, kStart>), dim3(grid), dim3(256), 0, s, a);
    return launch_status();
}
// Args: dimsum_conv_bwd_params_t or conv_varlen_bwd_args_t (kVarlen)
template <typename T, bool kVarlen, typename Args> static int launch_conv_bwd(const Args &a, hipStream_t s, bool ids_vec = true) {
    const dimsum_conv_bwd_params_t &q = conv_base(a);
    const dimsum_conv_params_t &p = q.fwd;
    const bool vec = ids_vec && vec_ok<T>(p.x_ptr, p.x_batch_stride, p.x_c_stride, p.seqlen) &&
                     vec_ok<T>(q.dout_ptr, q.dout_batch_stride, q.dout_c_stride, p.seqlen) &&
                     vec_ok<T>(q.dx_ptr, q.dx_batch_stride, q.dx_c_stride, p.seqlen);
    // enough waves to fill the chip while keeping >= 4 batch rows per wave when the batch allows it
    int split = 1;
    while ((int64_t)p.dim * split < 2048 && split * 4 < p.batch) split *= 2;
    if (vec) hipLaunchKernelGGL((causal_conv1d_bwd_kernel<T, true, kVarlen>), dim3(p.dim, split), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((causal_conv1d_bwd_kernel<T, false, kVarlen>), dim3(p.dim, split), dim3(256), 0, s, a);
    return launch_status();
}

template <typename T> static int launch_conv_chunk(const dimsum_conv_chunk_params_t &p, hipStream_t s) {
    const bool vec = vec_ok<T>(p.x_ptr, p.x_batch_stride, p.x_c_stride, p.seqlen) &&
                     vec_ok<T>(p.out_ptr, p.out_batch_stride, p.out_c_stride, p.seqlen);
    const int64_t rows = (int64_t)p.batch * p.dim;
    const int grid = (int)((rows + 3) / 4 < 256 * 32 ? (rows + 3) / 4 : 256 * 32);   // 4 waves per workgroup, one row per wave and pass
    if (vec) hipLaunchKernelGGL((causal_conv1d_chunk_kernel<T, true>), dim3(grid), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((causal_conv1d_chunk_kernel<T, false>), dim3(grid), dim3(256), 0, s, p);
    return launch_status();
}

// dimsum_causal_conv1d_varlen_states_fwd behind NULL / struct_size: the entry's own fields first, in the header's order; the state's dtype
// after the shared checks have vouched for conv.dtype. The resume entry runs the same
static int conv_states_check(const dimsum_conv_varlen_states_params_t &e) {
    if (e.num_slots < 1) return DIMSUM_ERR_SHAPE;
    if (!e.end_slots_ptr || !e.state_ptr) return DIMSUM_ERR_NULL;
    const dimsum_conv_params_t &p = e.varlen.conv;
    if (ids_stride_bad(e.end_slots_batch_stride, p) || any_negative({e.state_slot_stride, e.state_c_stride, e.state_w_stride})) return DIMSUM_ERR_STRIDE;
    const int rc = conv_checks(p, nullptr, true, e.varlen.seq_idx_ptr, e.varlen.seq_idx_batch_stride);
    if (rc != DIMSUM_OK) return rc;
    return e.state_dtype != p.dtype ? DIMSUM_ERR_UNSUPPORTED : DIMSUM_OK;      // the state is x's elements, moved
}

// ... and its fill -> whether its int32 rows may be read as 16-byte vectors
template <typename Args> static bool conv_states_fill(Args &a, const dimsum_conv_varlen_states_params_t &e) {
    memset(&a, 0, sizeof(a));
    a.v = {e.varlen.conv, reinterpret_cast<const int32_t *>(e.varlen.seq_idx_ptr), e.varlen.seq_idx_batch_stride};
    a.end_slots = reinterpret_cast<const int32_t *>(e.end_slots_ptr);
    a.end_batch_stride = e.end_slots_batch_stride;
    a.pool = e.state_ptr;
    a.pool_slot_stride = e.state_slot_stride, a.pool_c_stride = e.state_c_stride, a.pool_w_stride = e.state_w_stride;
    return ids_vec_ok(a.v.seq_idx, a.v.seq_batch_stride) && ids_vec_ok(a.end_slots, a.end_batch_stride);
}

}  // namespace dimsum

extern "C" int dimsum_causal_conv1d_chunk(const dimsum_conv_chunk_params_t *p, void *stream) {
    using namespace dimsum;
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_conv_chunk_params_t)) return DIMSUM_ERR_ABI;
    if (!p->x_ptr || !p->weight_ptr || !p->conv_state_ptr || !p->out_ptr) return DIMSUM_ERR_NULL;
    if (p->width < 2 || p->width > 4 || p->batch < 1 || p->dim < 1 || p->seqlen < 1) return DIMSUM_ERR_SHAPE;
    if (p->dtype < DIMSUM_F32 || p->dtype > DIMSUM_BF16) return DIMSUM_ERR_DTYPE;
    if (any_negative({p->x_batch_stride, p->x_c_stride, p->state_batch_stride, p->state_c_stride, p->state_w_stride, p->weight_c_stride,
                      p->weight_width_stride, p->out_batch_stride, p->out_c_stride}))
        return DIMSUM_ERR_STRIDE;
    return dispatch_dtype(p->dtype, [&](auto t) { return launch_conv_chunk<decltype(t)>(*p, reinterpret_cast<hipStream_t>(stream)); });
}

extern "C" int dimsum_causal_conv1d_fwd(const dimsum_conv_params_t *p, void *stream) {
    using namespace dimsum;
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_conv_params_t)) return DIMSUM_ERR_ABI;
    const int rc = conv_checks(*p, nullptr);
    if (rc != DIMSUM_OK || p->batch == 0) return rc;
    return dispatch_dtype(p->dtype, [&](auto t) { return launch_conv_fwd<decltype(t), false, false>(*p, reinterpret_cast<hipStream_t>(stream)); });
}

extern "C" int dimsum_causal_conv1d_bwd(const dimsum_conv_bwd_params_t *q, void *stream) {
    using namespace dimsum;
    if (!q) return DIMSUM_ERR_NULL;
    if (q->struct_size != sizeof(dimsum_conv_bwd_params_t)) return DIMSUM_ERR_ABI;
    const int rc = conv_checks(q->fwd, q);
    if (rc != DIMSUM_OK || q->fwd.batch == 0) return rc;
    return dispatch_dtype(q->fwd.dtype, [&](auto t) { return launch_conv_bwd<decltype(t), false>(*q, reinterpret_cast<hipStream_t>(stream)); });
}

extern "C" int dimsum_causal_conv1d_varlen_fwd(const dimsum_conv_varlen_params_t *v, void *stream) {
    using namespace dimsum;
    if (!v) return DIMSUM_ERR_NULL;
    if (v->struct_size != sizeof(dimsum_conv_varlen_params_t)) return DIMSUM_ERR_ABI;
    const int rc = conv_checks(v->conv, nullptr, true, v->seq_idx_ptr, v->seq_idx_batch_stride);
    if (rc != DIMSUM_OK || v->conv.batch == 0) return rc;
    const conv_varlen_args_t a = {v->conv, reinterpret_cast<const int32_t *>(v->seq_idx_ptr), v->seq_idx_batch_stride};
    const bool ids_vec = ids_vec_ok(a.seq_idx, a.seq_batch_stride);
    return dispatch_dtype(a.p.dtype, [&](auto t) { return launch_conv_fwd<decltype(t), true, false>(a, reinterpret_cast<hipStream_t>(stream), ids_vec); });
}

extern "C" int dimsum_causal_conv1d_varlen_bwd(const dimsum_conv_varlen_bwd_params_t *v, void *stream) {
    using namespace dimsum;
    if (!v) return DIMSUM_ERR_NULL;
    if (v->struct_size != sizeof(dimsum_conv_varlen_bwd_params_t)) return DIMSUM_ERR_ABI;
    const int rc = conv_checks(v->conv.fwd, &v->conv, true, v->seq_idx_ptr, v->seq_idx_batch_stride);
    if (rc != DIMSUM_OK || v->conv.fwd.batch == 0) return rc;
    const conv_varlen_bwd_args_t a = {v->conv, reinterpret_cast<const int32_t *>(v->seq_idx_ptr), v->seq_idx_batch_stride};
    const bool ids_vec = ids_vec_ok(a.seq_idx, a.seq_batch_stride);
    return dispatch_dtype(a.q.fwd.dtype, [&](auto t) { return launch_conv_bwd<decltype(t), true>(a, reinterpret_cast<hipStream_t>(stream), ids_vec); });
}

extern "C" int dimsum_causal_conv1d_varlen_states_fwd(const dimsum_conv_varlen_states_params_t *e, void *stream) {
    using namespace dimsum;
    if (!e) return DIMSUM_ERR_NULL;
    if (e->struct_size != sizeof(dimsum_conv_varlen_states_params_t)) return DIMSUM_ERR_ABI;
    if (const int rc = conv_states_check(*e)) return rc;
    const dimsum_conv_params_t &p = e->varlen.conv;
    if (p.batch == 0) return DIMSUM_OK;
    conv_states_args_t a;
    const bool ids_vec = conv_states_fill(a, *e);
    return dispatch_dtype(p.dtype, [&](auto t) { return launch_conv_fwd<decltype(t), true, true>(a, reinterpret_cast<hipStream_t>(stream), ids_vec); });
}

extern "C" int dimsum_causal_conv1d_varlen_resume_fwd(const dimsum_conv_varlen_resume_params_t *e, void *stream) {
    using namespace dimsum;
    if (!e) return DIMSUM_ERR_NULL;
    if (e->struct_size != sizeof(dimsum_conv_varlen_resume_params_t)) return DIMSUM_ERR_ABI;
    if (e->n_init < 1) return DIMSUM_ERR_SHAPE;
    if (!e->start_slots_ptr || !e->init_ptr) return DIMSUM_ERR_NULL;
    const dimsum_conv_params_t &p = e->states.varlen.conv;
    if (ids_stride_bad(e->start_slots_batch_stride, p) || any_negative({e->init_slot_stride, e->init_c_stride, e->init_w_stride})) return DIMSUM_ERR_STRIDE;
    if (const int rc = conv_states_check(e->states)) return rc;
    if (e->init_dtype != p.dtype) return DIMSUM_ERR_UNSUPPORTED;       // the carried inputs are x's elements, moved
    if (p.batch == 0) return DIMSUM_OK;
    conv_resume_args_t a;
    bool ids_vec = conv_states_fill(a, e->states);
    a.start_slots = reinterpret_cast<const int32_t *>(e->start_slots_ptr);
    a.start_batch_stride = e->start_slots_batch_stride;
    a.init = e->init_ptr;
    a.init_slot_stride = e->init_slot_stride, a.init_c_stride = e->init_c_stride, a.init_w_stride = e->init_w_stride;
    ids_vec = ids_vec && ids_vec_ok(a.start_slots, a.start_batch_stride);
    return dispatch_dtype(p.dtype, [&](auto t) { return launch_conv_fwd<decltype(t), true, true, true>(a, reinterpret_cast<hipStream_t>(stream), ids_vec); });
}
