// decode_step.hip -- the weight-streaming linear layer of a decode step (1..16 tokens in flight, one per sequence) for gfx950:
//     y[b, n] = sum_k x'[b, k] W[n, k] (+ bias[n])        W (N, K) row-major, read exactly once per call
// with an optional prologue on x (the block's residual add + RMSNorm / LayerNorm) and an optional epilogue on the outputs n < conv_dim
// (one step of the causal conv1d on its carried state, csrc/mixer_step.hip). Replaces, for one token, the fused add + norm launch, the
// F.linear GEMV of in_proj / x_proj / out_proj / lm_head and causal_conv1d_update of Mamba.step (mamba/mamba_ssm/modules/mamba_simple.py:299-344,
// Block.forward :408-432): a step is bound by its launches, so the small passes around a GEMV ride in its launch.
//
// MI355X design: a decode GEMV is a pure weight stream (2 N K bytes at batch 1 in 16 bits; x' is batch * K elements out of L2).
//   * A WAVE owns kRows output rows. Its 64 lanes split K in 16-byte pieces (global_load_dwordx4 with the streaming "nt" policy: the weights
//     are used once per token and should not push the states out of L2), straight to VGPRs -- no LDS round trip for an operand no other wave
//     shares. All the loads of a K chunk (up to 4 per lane and row) are issued before the first FMA so that HBM latency is covered by loads in
//     flight, not by occupancy. What follows the last whole piece of a row, and a whole row whose base or stride is not 16-byte aligned, is
//     walked element by element.
//   * x' (after the prologue, rounded to T as the unfused norm's output is) sits in LDS, one 4-KiB chunk per batch row: one weight piece
//     feeds `batch` rows of FMAs, and a piece of x' is one conflict-free ds_read_b128 shared by the wave's rows. K beyond a chunk is walked
//     chunk by chunk (restaged between two barriers).
//   * The lane partials meet in a cross-lane tree that halves the number of live values at every step (63 exchanges for 64 values instead of
//     384) and leaves each (row, batch) total in ONE lane, which adds the bias, runs the conv epilogue and stores. No atomics, no split-K
//     across workgroups: the summation order is a function of the shape alone, two launches from equal inputs are bit-identical.
//   * Grid from N: kRows = 4 rows per wave once N >= 16384 (an LM head), else 1; 1 wave per workgroup up to 512 wave-rows (a batch-1 x_proj
//     with 80 rows is 80 workgroups), else 4 (batch <= 4) or 8 waves, so that the batch * K elements every workgroup stages stay small next
//     to its share of the weights. One workgroup per group of rows; no grid-stride loop.
//   * Prologue: every workgroup recomputes the `batch` row statistics (fp32, two passes for LayerNorm as csrc/norm.hip) from x (+ residual) in
//     L2; workgroup 0 alone writes residual_out. The host refuses a residual_out that overlaps x or residual (other workgroups still read them).
//     LayerNorm's second pass also sums r - mean: the mean of a K-term fp32 sum is off by an ulp or two of ITSELF, which on rows far from
//     zero (mean 64, unit spread) is 1e-5 of the spread and shifts every x' alike; r - mean is exact there, so sum(r - mean) / K recovers what
//     the mean lost, and x' = ((r - mean) - corr) * rstd, var = mean(d^2) - corr^2. RMSNorm has mean = corr = 0: its arithmetic is unchanged.
//   * Epilogue: the lane holding y[b, n], n < conv_dim, rolls conv_state[b, n, :], appends y rounded to T and computes
//     act(bias_c[n] + sum_w Wc[n, w] state[w]) with the expressions of causal_conv1d_update_kernel. Only that lane touches that state row.
//   * Slot-indexed conv states (dimsum_decode_linear_slots, kSlots): conv_state is a pool and the lane holding y[b, n] works on
//     conv_state[slots[b], n, :]; slots[b] < 0 stores a zero and touches no state; the plain columns are written as ever. A template flag on
//     the kernel: one epilogue for both forms, and kSlots = false (the plain struct as the kernel's first argument, the state row b) compiles
//     to the kernel as it was. The index is trusted: < num_slots and unique per launch is the caller's contract (include/dimsum_hip.h).
#include "common.hpp"

#include <type_traits>

namespace dimsum {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kChunkPieces = 256;       // 16-byte pieces of x' per batch row and K chunk: 4 KiB, four passes of 64 lanes
constexpr int kPasses = kChunkPieces / kWave;
constexpr int kMaxBatch = 16;
constexpr int kWideRowsFrom = 16384;    // N from which a wave owns 4 rows
constexpr int kMaxThreads = 512;

template <typename T> struct Piece { static constexpr int kElems = 16 / sizeof(T); };

template <typename T> __device__ __forceinline__ void unpack(const u32x4 &v, float *f);
template <> __device__ __forceinline__ void unpack<float>(const u32x4 &v, float *f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) f[i] = __uint_as_float(v[i]);
}
template <> __device__ __forceinline__ void unpack<__half>(const u32x4 &v, float *f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned u = v[i];
        const float2 t = __half22float2(*reinterpret_cast<const __half2 *>(&u));
        f[2 * i] = t.x;
        f[2 * i + 1] = t.y;
    }
}
template <> __device__ __forceinline__ void unpack<__hip_bfloat16>(const u32x4 &v, float *f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = __uint_as_float(v[i] << 16);
        f[2 * i + 1] = __uint_as_float(v[i] & 0xffff0000u);
    }
}

__device__ __forceinline__ float wave_sum_all(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

// C live values per lane -> their 64-lane totals. While C > 1 a step over the lane bit S halves C: a lane keeps one half of its values and
// hands the other half to its partner (which keeps that half), so that after log2(C) steps every lane holds ONE value, summed over the lane
// bits walked so far; the remaining steps are a plain butterfly. Lane l ends with the total of value tree_index<V>(l) in a[0].
template <int C, int S> __device__ __forceinline__ void tree_reduce(float *a, int lane) {
    if constexpr (S < 6) {
        constexpr int m = 1 << S;
        if constexpr (C > 1) {
            constexpr int h = C / 2;
            const bool up = (lane & m) != 0;
#pragma unroll
            for (int i = 0; i < h; ++i) {
                const float keep = up ? a[i + h] : a[i], send = up ? a[i] : a[i + h];
                a[i] = keep + __shfl_xor(send, m, kWave);
            }
            tree_reduce<h, S + 1>(a, lane);
        } else {
            a[0] += __shfl_xor(a[0], m, kWave);
            tree_reduce<1, S + 1>(a, lane);
        }
    }
}
template <int V> __device__ __forceinline__ int tree_index(int lane) {
    int idx = 0;
#pragma unroll
    for (int s = 0; (1 << s) < V; ++s)
        if ((lane >> s) & 1) idx += V >> (s + 1);
    return idx;
}

struct decode_flags_t {
    int vec_w;      // W rows start 16-byte aligned: whole pieces by vector loads
    int vec_x;      // no prologue and x rows start 16-byte aligned: staged by vector copies
};

// r[b, k] = x (+ residual), in fp32 (the norm works on the unrounded sum, as csrc/norm.hip does)
template <typename T> __device__ __forceinline__ float stream_value(const dimsum_decode_linear_params_t &p, int b, int k) {
    float r = to_f32<T>(reinterpret_cast<const T *>(p.x_ptr)[(int64_t)b * p.x_row_stride + k]);
    if (p.residual_ptr) {
        const int64_t o = (int64_t)b * p.residual_row_stride + k;
        r += p.residual_dtype == DIMSUM_F32 ? reinterpret_cast<const float *>(p.residual_ptr)[o] : to_f32<T>(reinterpret_cast<const T *>(p.residual_ptr)[o]);
    }
    return r;
}

// the slot form's first kernel argument: the plain parameters and the (batch) int32 slot index of the conv epilogue's states
struct decode_slots_args_t {
    dimsum_decode_linear_params_t p;
    const int32_t *slots;
    int64_t slots_stride;
};
__device__ __forceinline__ const dimsum_decode_linear_params_t &decode_base(const dimsum_decode_linear_params_t &a) { return a; }
__device__ __forceinline__ const dimsum_decode_linear_params_t &decode_base(const decode_slots_args_t &a) { return a.p; }

// T: x, W, bias, y, norm and conv weights, conv state. kBatch: the batch rounded up to a power of two (rows beyond p.batch are zeros in LDS).
// kRows: output rows per wave. blockDim.x / 64 waves; workgroup g owns rows [g * waves * kRows, (g + 1) * waves * kRows).
template <typename T, int kBatch, int kRows, bool kSlots>
__global__ __launch_bounds__(kMaxThreads) void decode_linear_kernel(
    const std::conditional_t<kSlots, decode_slots_args_t, dimsum_decode_linear_params_t> ka, const decode_flags_t fl) {
    const dimsum_decode_linear_params_t &p = decode_base(ka);
    constexpr int E = Piece<T>::kElems;
    constexpr int kChunk = kChunkPieces * E;                // elements of K per chunk
    constexpr int V = kRows * kBatch;
    __shared__ u32x4 xs[kBatch * kChunkPieces];
    __shared__ float s_mean[kMaxBatch], s_corr[kMaxBatch], s_rstd[kMaxBatch];
    T *xs_t = reinterpret_cast<T *>(xs);
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nwaves = blockDim.x >> 6;
    const int K = p.k, N = p.n, B = p.batch;

    // ---- prologue statistics: wave w takes batch rows w, w + nwaves, ... ----
    if (p.norm) {
        const float inv_k = 1.0f / (float)K;
        const bool rms = p.norm == 2;
        for (int b = wave; b < B; b += nwaves) {
            float s = 0.f;
            const bool write = blockIdx.x == 0 && p.residual_out_ptr;
            for (int k = lane; k < K; k += kWave) {
                const float r = stream_value<T>(p, b, k);
                if (write) {
                    const int64_t o = (int64_t)b * p.residual_out_row_stride + k;
                    if (p.residual_dtype == DIMSUM_F32) reinterpret_cast<float *>(p.residual_out_ptr)[o] = r;
                    else reinterpret_cast<T *>(p.residual_out_ptr)[o] = from_f32<T>(r);
                }
                s += rms ? r * r : r;
            }
            s = wave_sum_all(s);
            float mean = 0.f, corr = 0.f, var;
            if (rms) {
                var = s * inv_k;
            } else {
                mean = s * inv_k;
                float v1 = 0.f, v2 = 0.f;
                for (int k = lane; k < K; k += kWave) {
                    const float d = stream_value<T>(p, b, k) - mean;
                    v1 += d;
                    v2 += d * d;
                }
                corr = wave_sum_all(v1) * inv_k;     // what the rounded K-term sum left of the mean: rows far from zero (see the header)
                var = fmaxf(wave_sum_all(v2) * inv_k - corr * corr, 0.f);
            }
            if (lane == 0) {
                s_mean[b] = mean;
                s_corr[b] = corr;
                s_rstd[b] = 1.0f / sqrtf(var + p.eps);
            }
        }
        __syncthreads();
    }

    const int64_t row0 = ((int64_t)blockIdx.x * nwaves + wave) * kRows;       // this wave's first row
    const bool active = row0 < N;
    const T *wrow[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const int64_t row = row0 + r < N ? row0 + r : (int64_t)N - 1;             // rows past the end re-read the last one; never stored
        wrow[r] = reinterpret_cast<const T *>(p.w_ptr) + row * p.w_row_stride;
    }
    float acc[V];
#pragma unroll
    for (int i = 0; i < V; ++i) acc[i] = 0.f;

    const T *nw = reinterpret_cast<const T *>(p.norm_weight_ptr), *nb = reinterpret_cast<const T *>(p.norm_bias_ptr);
    for (int k0 = 0; k0 < K; k0 += kChunk) {
        const int len = K - k0 < kChunk ? K - k0 : kChunk;
        if (k0 > 0) __syncthreads();                 // every wave is done with the previous chunk
        // ---- stage x'[:, k0 : k0 + len] ----
        if (fl.vec_x) {
            const int np = len / E;
#pragma unroll 1
            for (int b = 0; b < kBatch; ++b) {
                const T *xr = reinterpret_cast<const T *>(p.x_ptr) + (int64_t)(b < B ? b : 0) * p.x_row_stride + k0;
                for (int pc = threadIdx.x; pc < np; pc += blockDim.x) {
                    u32x4 v = *reinterpret_cast<const u32x4 *>(xr + pc * E);
                    if (b >= B) v = u32x4{0u, 0u, 0u, 0u};
                    xs[b * kChunkPieces + pc] = v;
                }
                for (int k = np * E + threadIdx.x; k < len; k += blockDim.x) xs_t[b * kChunk + k] = b < B ? xr[k] : from_f32<T>(0.f);
            }
        } else {
#pragma unroll 1
            for (int b = 0; b < kBatch; ++b) {
                for (int k = threadIdx.x; k < len; k += blockDim.x) {
                    float v = 0.f;
                    if (b < B) {
                        v = stream_value<T>(p, b, k0 + k);
                        if (p.norm) {
                            v = ((v - s_mean[b]) - s_corr[b]) * s_rstd[b] * to_f32<T>(nw[k0 + k]);
                            if (nb) v += to_f32<T>(nb[k0 + k]);
                        }
                    }
                    xs_t[b * kChunk + k] = from_f32<T>(v);
                }
            }
        }
        __syncthreads();
        if (!active) continue;
        // ---- the wave's rows over this chunk: whole pieces by vector loads, all issued before the first FMA ----
        const int np = fl.vec_w ? len / E : 0;
        u32x4 w[kPasses][kRows];
#pragma unroll
        for (int j = 0; j < kPasses; ++j) {
            const int pc = j * kWave + lane;
#pragma unroll
            for (int r = 0; r < kRows; ++r)
                w[j][r] = pc < np ? __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(wrow[r] + k0 + pc * E)) : u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int j = 0; j < kPasses; ++j) {
            const int pc = j * kWave + lane;
            if (pc < np) {
                float wf[kRows][E];
#pragma unroll
                for (int r = 0; r < kRows; ++r) unpack<T>(w[j][r], wf[r]);
#pragma unroll
                for (int b = 0; b < kBatch; ++b) {
                    float xf[E];
                    unpack<T>(xs[b * kChunkPieces + pc], xf);
#pragma unroll
                    for (int r = 0; r < kRows; ++r)
#pragma unroll
                        for (int e = 0; e < E; ++e) acc[r * kBatch + b] = fmaf(wf[r][e], xf[e], acc[r * kBatch + b]);
                }
            }
        }
        // ---- what follows the last whole piece; the whole chunk when the rows are not 16-byte aligned ----
        for (int k = np * E + lane; k < len; k += kWave) {
            float wv[kRows];
#pragma unroll
            for (int r = 0; r < kRows; ++r) wv[r] = to_f32<T>(wrow[r][k0 + k]);
#pragma unroll
            for (int b = 0; b < kBatch; ++b) {
                const float xv = to_f32<T>(xs_t[b * kChunk + k]);
#pragma unroll
                for (int r = 0; r < kRows; ++r) acc[r * kBatch + b] = fmaf(wv[r], xv, acc[r * kBatch + b]);
            }
        }
    }
    if (!active) return;

    tree_reduce<V, 0>(acc, lane);
    if (lane >= V) return;
    const int idx = tree_index<V>(lane);
    const int b = idx % kBatch;
    const int64_t n = row0 + idx / kBatch;
    if (b >= B || n >= N) return;
    float v = acc[0];
    if (p.bias_ptr) v += to_f32<T>(reinterpret_cast<const T *>(p.bias_ptr)[n]);
    T *y = reinterpret_cast<T *>(p.y_ptr) + (int64_t)b * p.y_row_stride + n;
    if (n >= p.conv_dim) {
        *y = from_f32<T>(v);
        return;
    }
    // ---- one step of the causal conv1d on channel n (conv_update_row of csrc/mixer_step.hip, element path) ----
    const int W = p.conv_width;
    int64_t sb = b;                 // the row of conv_state this batch row works on
    if constexpr (kSlots) {
        sb = ka.slots[b * ka.slots_stride];
        if (sb < 0) {               // a padding row: no state touched, a zero where the conv output goes
            *y = from_f32<T>(0.f);
            return;
        }
    }
    T *st = reinterpret_cast<T *>(p.conv_state_ptr) + sb * p.state_batch_stride + n * p.state_c_stride;
    T s[4];     // the NEW state, right-aligned into 4 slots
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = (k >= 4 - W) ? st[(k - (4 - W) + 1) * p.state_w_stride] : from_f32<T>(0.f);
    s[3] = from_f32<T>(v);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k >= 4 - W) st[(k - (4 - W)) * p.state_w_stride] = s[k];
    const T *cw = reinterpret_cast<const T *>(p.conv_weight_ptr) + n * p.conv_weight_c_stride;
    float a = p.conv_bias_ptr ? to_f32<T>(reinterpret_cast<const T *>(p.conv_bias_ptr)[n]) : 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k >= 4 - W) a = fmaf(to_f32<T>(cw[(k - (4 - W)) * p.conv_weight_width_stride]), to_f32<T>(s[k]), a);
    if (p.silu_activation) a *= sigmoidf_fast(a);
    *y = from_f32<T>(a);
}

// ---- host ----------------------------------------------------------------------------------------------------------
template <typename T, int kBatch> static int launch_decode_linear(const dimsum_decode_linear_params_t &p, hipStream_t s, const int32_t *slots, int64_t slots_stride) {
    decode_flags_t fl;
    fl.vec_w = aligned_to<T>(p.w_ptr, 16) && (p.n == 1 || (p.w_row_stride * (int64_t)sizeof(T)) % 16 == 0);
    fl.vec_x = !p.norm && aligned_to<T>(p.x_ptr, 16) && (p.batch == 1 || (p.x_row_stride * (int64_t)sizeof(T)) % 16 == 0);
    const int rows = p.n >= kWideRowsFrom ? 4 : 1;
    const int64_t wave_rows = ((int64_t)p.n + rows - 1) / rows;
    const int waves = wave_rows <= 512 ? 1 : (p.batch <= 4 ? 4 : kMaxThreads / kWave);
    const dim3 grid((unsigned)((wave_rows + waves - 1) / waves)), block((unsigned)(waves * kWave));
    if (slots) {
        const decode_slots_args_t a = {p, slots, slots_stride};
        if (rows == 4) hipLaunchKernelGGL((decode_linear_kernel<T, kBatch, 4, true>), grid, block, 0, s, a, fl);
        else hipLaunchKernelGGL((decode_linear_kernel<T, kBatch, 1, true>), grid, block, 0, s, a, fl);
    } else if (rows == 4) hipLaunchKernelGGL((decode_linear_kernel<T, kBatch, 4, false>), grid, block, 0, s, p, fl);
    else hipLaunchKernelGGL((decode_linear_kernel<T, kBatch, 1, false>), grid, block, 0, s, p, fl);
    return launch_status();
}

template <typename T> static int dispatch_decode_linear(const dimsum_decode_linear_params_t &p, hipStream_t s, const int32_t *slots, int64_t slots_stride) {
    if (p.batch == 1) return launch_decode_linear<T, 1>(p, s, slots, slots_stride);
    if (p.batch == 2) return launch_decode_linear<T, 2>(p, s, slots, slots_stride);
    if (p.batch <= 4) return launch_decode_linear<T, 4>(p, s, slots, slots_stride);
    if (p.batch <= 8) return launch_decode_linear<T, 8>(p, s, slots, slots_stride);
    return launch_decode_linear<T, 16>(p, s, slots, slots_stride);
}

// [ptr, ptr + ((rows - 1) * stride + cols) * elem) of two (rows, cols) operands with unit column stride
static bool rows_overlap(const void *a, int64_t a_stride, size_t a_elem, const void *b, int64_t b_stride, size_t b_elem, int64_t rows, int64_t cols) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    const uintptr_t a1 = a0 + (uintptr_t)((rows - 1) * a_stride + cols) * a_elem, b1 = b0 + (uintptr_t)((rows - 1) * b_stride + cols) * b_elem;
    return a0 < b1 && b0 < a1;
}

// the checks of dimsum_decode_linear after NULL / struct_size, and the launch; slots != nullptr: the slot form
static int decode_linear_run(const dimsum_decode_linear_params_t *p, hipStream_t s, const int32_t *slots, int64_t slots_stride) {
    if (!p->x_ptr || !p->w_ptr || !p->y_ptr) return DIMSUM_ERR_NULL;
    if (p->norm && !p->norm_weight_ptr) return DIMSUM_ERR_NULL;
    if (p->conv_dim && (!p->conv_weight_ptr || !p->conv_state_ptr)) return DIMSUM_ERR_NULL;
    if (p->batch < 1 || p->batch > kMaxBatch || p->n < 1 || p->k < 1) return DIMSUM_ERR_SHAPE;
    if (p->norm < 0 || p->norm > 2 || p->conv_dim < 0 || p->conv_dim > p->n) return DIMSUM_ERR_SHAPE;
    if (p->conv_dim && (p->conv_width < 2 || p->conv_width > 4)) return DIMSUM_ERR_SHAPE;
    if (p->dtype < DIMSUM_F32 || p->dtype > DIMSUM_BF16) return DIMSUM_ERR_DTYPE;
    if (p->residual_dtype != DIMSUM_F32 && p->residual_dtype != p->dtype) return DIMSUM_ERR_DTYPE;
    if (!p->norm && (p->residual_ptr || p->residual_out_ptr || p->norm_bias_ptr)) return DIMSUM_ERR_UNSUPPORTED;   // the add belongs to the norm prologue
    if (p->x_row_stride < 0 || p->w_row_stride < 0 || p->y_row_stride < 0) return DIMSUM_ERR_STRIDE;
    if ((p->residual_ptr && p->residual_row_stride < 0) || (p->residual_out_ptr && p->residual_out_row_stride < 0)) return DIMSUM_ERR_STRIDE;
    if (p->conv_dim && (p->state_batch_stride < 0 || p->state_c_stride < 0 || p->state_w_stride < 0 || p->conv_weight_c_stride < 0 ||
                        p->conv_weight_width_stride < 0)) return DIMSUM_ERR_STRIDE;
    const size_t ts = p->dtype == DIMSUM_F32 ? 4 : 2, rs = p->residual_dtype == DIMSUM_F32 ? 4 : 2;
    if (p->residual_out_ptr) {
        if (rows_overlap(p->residual_out_ptr, p->residual_out_row_stride, rs, p->x_ptr, p->x_row_stride, ts, p->batch, p->k)) return DIMSUM_ERR_ALIAS;
        if (p->residual_ptr && rows_overlap(p->residual_out_ptr, p->residual_out_row_stride, rs, p->residual_ptr, p->residual_row_stride, rs, p->batch, p->k))
            return DIMSUM_ERR_ALIAS;
    }
    switch (p->dtype) {
        case DIMSUM_F32: return dispatch_decode_linear<float>(*p, s, slots, slots_stride);
        case DIMSUM_F16: return dispatch_decode_linear<__half>(*p, s, slots, slots_stride);
        default: return dispatch_decode_linear<__hip_bfloat16>(*p, s, slots, slots_stride);
    }
}

}  // namespace dimsum

extern "C" int dimsum_decode_linear(const dimsum_decode_linear_params_t *p, void *stream) {
    using namespace dimsum;
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_decode_linear_params_t)) return DIMSUM_ERR_ABI;
    return decode_linear_run(p, reinterpret_cast<hipStream_t>(stream), nullptr, 0);
}

extern "C" int dimsum_decode_linear_slots(const dimsum_decode_linear_slots_params_t *v, void *stream) {
    using namespace dimsum;
    const int rc = slots_check(v);
    if (rc != DIMSUM_OK) return rc;
    if (v->linear.conv_dim == 0) return DIMSUM_ERR_UNSUPPORTED;       // no epilogue, no state to index
    return decode_linear_run(&v->linear, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const int32_t *>(v->slots_ptr), v->slots_stride);
}
