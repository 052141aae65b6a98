// causal_conv1d_cl.hip -- the depthwise causal conv1d of causal_conv1d.hip on CHANNEL-LAST operands, forward and backward, for gfx950.
//
// Replaces causal_conv1d_channellast_fwd_kernel / _bwd_kernel (causal-conv1d/csrc/causal_conv1d_fwd.cu:193-319,
// causal_conv1d_bwd.cu:306-494; host checks causal_conv1d.cpp:242-247, 376-379, 395-396):
//     out[b,t,d] = act(bias[d] + sum_k W[d,k] * x[b,t-(width-1-k),d]),   x[.., t<0, ..] = 0,   act = SiLU or identity
// x, out, dout, dx are (batch, seqlen, dim) with channel stride 1 and independent 64-bit batch / token strides per tensor.
// Pure streaming: 2*B*D*L*s bytes forward, 3*B*D*L*s backward.
//
// MI355X design: lanes run along the channels, 16 bytes (4 fp32 / 8 16-bit channels) per lane, so one wave64 reads whole contiguous
// 1-KiB row segments. A wave owns 64 channel vectors and one chunk of kClChunk tokens, which it walks in time order with the last
// width-1 inputs held in registers as a sliding window; the chunk's width-1 halo rows are re-read from memory (zeros before t = 0):
// (width-1)/kClChunk extra reads, no LDS, no barrier, no cross-lane traffic (the reference transposes a 64 x 64 tile through shared
// memory). Weights and bias are per lane, loaded once. The backward walks a chunk from its end with the gradient halo carried the same
// way (rebuilt at the chunk's end from the width-1 tokens after it), keeps dweight / dbias partial sums per lane in registers over
// every token and batch row the lane visits and adds them with one atomicAdd per lane and tap.
#include "common.hpp"

#include <algorithm>
#include <type_traits>

namespace dimsum {

constexpr int kClChunk = DIMSUM_CONV_CL_CHUNK;

__device__ __forceinline__ float silu_grad_cl(float pre) {   // d/dpre [pre * sigmoid(pre)]   (causal_conv1d_bwd.cu:153-164)
    const float sg = sigmoidf_fast(pre);
    return sg * (1.0f + pre * (1.0f - sg));
}

// one lane's 16 bytes of a token row: 4 fp32 or 8 16-bit channels
struct alignas(16) Raw16 { uint32_t w[4]; };

// kVec: one 16-byte access; otherwise the first n of the lane's channels one by one (the others read as 0 and are not written)
template <typename T, bool kVec>
__device__ __forceinline__ Raw16 load_cvec(const T *p, int n) {
    if constexpr (kVec) {
        return *reinterpret_cast<const Raw16 *>(p);
    } else {
        Raw16 r;
        if constexpr (sizeof(T) == 4) {
            const uint32_t *q = reinterpret_cast<const uint32_t *>(p);
#pragma unroll
            for (int e = 0; e < 4; ++e) r.w[e] = e < n ? q[e] : 0u;
        } else {
            const unsigned short *q = reinterpret_cast<const unsigned short *>(p);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t lo = 2 * i < n ? q[2 * i] : 0u, hi = 2 * i + 1 < n ? q[2 * i + 1] : 0u;
                r.w[i] = lo | (hi << 16);
            }
        }
        return r;
    }
}
template <typename T, bool kVec>
__device__ __forceinline__ void store_cvec(T *p, int n, const Raw16 &r) {
    if constexpr (kVec) {
        *reinterpret_cast<Raw16 *>(p) = r;
    } else if constexpr (sizeof(T) == 4) {
        uint32_t *q = reinterpret_cast<uint32_t *>(p);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < n) q[e] = r.w[e];
    } else {
        unsigned short *q = reinterpret_cast<unsigned short *>(p);
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (e < n) q[e] = (unsigned short)(r.w[e >> 1] >> (16 * (e & 1)));
    }
}
template <typename T>
__device__ __forceinline__ void unpack_cvec(const Raw16 &r, float (&v)[16 / sizeof(T)]) {
    if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = __uint_as_float(r.w[e]);
    } else if constexpr (std::is_same<T, __half>::value) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float2 f = __half22float2(*reinterpret_cast<const __half2 *>(&r.w[i]));
            v[2 * i] = f.x;
            v[2 * i + 1] = f.y;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[2 * i] = __uint_as_float(r.w[i] << 16);
            v[2 * i + 1] = __uint_as_float(r.w[i] & 0xffff0000u);
        }
    }
}
template <typename T>
__device__ __forceinline__ Raw16 pack_cvec(const float (&v)[16 / sizeof(T)]) {
    Raw16 r;
    if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) r.w[e] = __float_as_uint(v[e]);
    } else if constexpr (std::is_same<T, __half>::value) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const __half2 h = __floats2half2_rn(v[2 * i], v[2 * i + 1]);
            r.w[i] = *reinterpret_cast<const uint32_t *>(&h);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const __hip_bfloat16 t[2] = {__float2bfloat16(v[2 * i]), __float2bfloat16(v[2 * i + 1])};
            r.w[i] = *reinterpret_cast<const uint32_t *>(t);
        }
    }
    return r;
}

// the lane's taps, right-aligned into 4 slots (w4[3] multiplies x[t], w4[2] x[t-1], ...; unused slots 0), and its bias
template <int V>
__device__ __forceinline__ void load_taps(const dimsum_conv_cl_params_t &p, int64_t d0, int n, float (&w4)[4][V], float (&bias)[V]) {
    const float *wp = reinterpret_cast<const float *>(p.weight_ptr);
    const float *bp = reinterpret_cast<const float *>(p.bias_ptr);
    const int W = p.width;
#pragma unroll
    for (int e = 0; e < V; ++e) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            w4[k][e] = (k >= 4 - W && e < n) ? wp[(d0 + e) * p.weight_c_stride + (k - (4 - W)) * p.weight_width_stride] : 0.f;
        bias[e] = (bp && e < n) ? bp[d0 + e] : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// forward. grid = (channel blocks of 64 vectors, token chunks / 4, batch); the chunk and batch loops stride by the grid, so a grid
// clamped to the launch limits still covers everything. One wave = one channel block x one chunk.
template <typename T, bool kVec>
__global__ __launch_bounds__(256) void causal_conv1d_cl_fwd_kernel(const dimsum_conv_cl_params_t p) {
    constexpr int V = 16 / sizeof(T);
    constexpr int kU = 8;                                     // token rows in flight per lane: 8 x 1 KiB per wave
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t d0 = ((int64_t)blockIdx.x * kWave + lane) * V;
    if (d0 >= p.dim) return;                                  // no barrier anywhere below
    const int n = (int)min((int64_t)V, (int64_t)p.dim - d0);
    const int W = p.width;
    const int64_t L = p.seqlen;
    const bool silu = p.silu_activation != 0;
    float w4[4][V], bias[V];
    load_taps<V>(p, d0, n, w4, bias);

    const int64_t n_chunks = (L + kClChunk - 1) / kClChunk;
    for (int64_t c = (int64_t)blockIdx.y * 4 + wave; c < n_chunks; c += (int64_t)gridDim.y * 4) {
        const int64_t t0 = c * kClChunk, t1 = min(t0 + kClChunk, L);
        for (int b = blockIdx.z; b < p.batch; b += gridDim.z) {
            const T *x = reinterpret_cast<const T *>(p.x_ptr) + (int64_t)b * p.x_batch_stride + d0;
            T *o = reinterpret_cast<T *>(p.out_ptr) + (int64_t)b * p.out_batch_stride + d0;
            float h[3][V];                                    // x[t-3], x[t-2], x[t-1]: the halo rows, then the sliding window
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int64_t t = t0 - 3 + j;
                if (j >= 4 - W && t >= 0) {
                    unpack_cvec<T>(load_cvec<T, kVec>(x + t * p.x_l_stride, n), h[j]);
                } else {
#pragma unroll
                    for (int e = 0; e < V; ++e) h[j][e] = 0.f;
                }
            }
            auto token = [&](int64_t t, const Raw16 &raw) {
                float v[V], q[V];
                unpack_cvec<T>(raw, v);
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    q[e] = bias[e] + w4[0][e] * h[0][e] + w4[1][e] * h[1][e] + w4[2][e] * h[2][e] + w4[3][e] * v[e];
                    if (silu) q[e] *= sigmoidf_fast(q[e]);    // out / (1 + exp(-out)), causal_conv1d_fwd.cu:113-118
                    h[0][e] = h[1][e];
                    h[1][e] = h[2][e];
                    h[2][e] = v[e];
                }
                store_cvec<T, kVec>(o + t * p.out_l_stride, n, pack_cvec<T>(q));
            };
            int64_t t = t0;
            for (; t + kU <= t1; t += kU) {
                Raw16 raw[kU];
#pragma unroll
                for (int u = 0; u < kU; ++u) raw[u] = load_cvec<T, kVec>(x + (t + u) * p.x_l_stride, n);
#pragma unroll
                for (int u = 0; u < kU; ++u) token(t + u, raw[u]);
            }
            for (; t < t1; ++t) token(t, load_cvec<T, kVec>(x + t * p.x_l_stride, n));
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// backward. The same grid; g = dout * SiLU'(pre) with pre recomputed, dx[s] = sum_k w4[k] * g[s + 3 - k] over the tokens of the same
// sequence. A chunk is walked from its end: the window holds x[s-3 .. s], the halo g[s+1 .. s+3]. The width-1 tokens after the chunk
// are run first, without writing or accumulating anything, to rebuild that halo.
template <typename T, bool kVec>
__global__ __launch_bounds__(256) void causal_conv1d_cl_bwd_kernel(const dimsum_conv_cl_bwd_params_t q) {
    const dimsum_conv_cl_params_t &p = q.fwd;
    constexpr int V = 16 / sizeof(T);
    constexpr int kU = 4;                                     // token rows in flight per lane and tensor
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t d0 = ((int64_t)blockIdx.x * kWave + lane) * V;
    if (d0 >= p.dim) return;
    const int n = (int)min((int64_t)V, (int64_t)p.dim - d0);
    const int W = p.width;
    const int64_t L = p.seqlen;
    const bool silu = p.silu_activation != 0;
    float w4[4][V], bias[V];
    load_taps<V>(p, d0, n, w4, bias);
    float dw[4][V], db[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
        db[e] = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) dw[k][e] = 0.f;
    }
    bool visited = false;

    const int64_t n_chunks = (L + kClChunk - 1) / kClChunk;
    for (int64_t c = (int64_t)blockIdx.y * 4 + wave; c < n_chunks; c += (int64_t)gridDim.y * 4) {
        const int64_t t0 = c * kClChunk, t1 = min(t0 + kClChunk, L);
        const int64_t x_lo = max((int64_t)0, t0 - (W - 1));   // the first x row this chunk needs: rows below it read as 0
        const int64_t g_hi = min(L, t1 + (W - 1));            // one past the last token whose g this chunk needs
        for (int b = blockIdx.z; b < p.batch; b += gridDim.z) {
            visited = true;
            const T *x = reinterpret_cast<const T *>(p.x_ptr) + (int64_t)b * p.x_batch_stride + d0;
            const T *go = reinterpret_cast<const T *>(q.dout_ptr) + (int64_t)b * q.dout_batch_stride + d0;
            T *dx = reinterpret_cast<T *>(q.dx_ptr) + (int64_t)b * q.dx_batch_stride + d0;
            float xw[3][V], gh[3][V];                         // x[s-2], x[s-1], x[s] and g[s+1], g[s+2], g[s+3] of the next token s
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int64_t r = t1 + j;                     // the halo tokens' own inputs: only SiLU' needs them
                if (silu && r < g_hi) {
                    unpack_cvec<T>(load_cvec<T, kVec>(x + r * p.x_l_stride, n), xw[j]);
                } else {
#pragma unroll
                    for (int e = 0; e < V; ++e) xw[j][e] = 0.f;
                }
#pragma unroll
                for (int e = 0; e < V; ++e) gh[j][e] = 0.f;
            }
            // one token s, walking down: xr = row s-3 of x (zeros below x_lo), gr = row s of dout
            auto token = [&](int64_t s, const Raw16 &xr, const Raw16 &gr, bool x_ok, bool g_ok, bool live) {
                float x0[V], g[V], r[V];
                unpack_cvec<T>(xr, x0);
                unpack_cvec<T>(gr, g);
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    x0[e] = x_ok ? x0[e] : 0.f;
                    g[e] = g_ok ? g[e] : 0.f;
                    if (silu) {
                        const float pre = bias[e] + w4[0][e] * x0[e] + w4[1][e] * xw[0][e] + w4[2][e] * xw[1][e] + w4[3][e] * xw[2][e];
                        g[e] *= silu_grad_cl(pre);
                    }
                    if (live) {
                        db[e] += g[e];
                        dw[0][e] = fmaf(g[e], x0[e], dw[0][e]);
                        dw[1][e] = fmaf(g[e], xw[0][e], dw[1][e]);
                        dw[2][e] = fmaf(g[e], xw[1][e], dw[2][e]);
                        dw[3][e] = fmaf(g[e], xw[2][e], dw[3][e]);
                        r[e] = w4[3][e] * g[e] + w4[2][e] * gh[0][e] + w4[1][e] * gh[1][e] + w4[0][e] * gh[2][e];
                    }
                    gh[2][e] = gh[1][e];
                    gh[1][e] = gh[0][e];
                    gh[0][e] = g[e];
                    xw[2][e] = xw[1][e];
                    xw[1][e] = xw[0][e];
                    xw[0][e] = x0[e];
                }
                if (live) store_cvec<T, kVec>(dx + s * q.dx_l_stride, n, pack_cvec<T>(r));
            };
            const Raw16 zero = {{0u, 0u, 0u, 0u}};
            // the halo: tokens t1+2, t1+1, t1 (those below g_hi), loads issued together
            {
                Raw16 xr[3], gr[3];
#pragma unroll
                for (int u = 0; u < 3; ++u) {
                    const int64_t s = t1 + 2 - u;
                    xr[u] = s - 3 >= x_lo ? load_cvec<T, kVec>(x + (s - 3) * p.x_l_stride, n) : zero;
                    gr[u] = s < g_hi ? load_cvec<T, kVec>(go + s * q.dout_l_stride, n) : zero;
                }
#pragma unroll
                for (int u = 0; u < 3; ++u) token(t1 + 2 - u, xr[u], gr[u], true, true, false);
            }
            // the chunk's own tokens, kU at a time; an x row below x_lo is read at x_lo (valid memory) and replaced by 0
            int64_t s = t1 - 1;
            for (; s - (kU - 1) >= t0; s -= kU) {
                Raw16 xr[kU], gr[kU];
#pragma unroll
                for (int u = 0; u < kU; ++u) {
                    xr[u] = load_cvec<T, kVec>(x + max(s - u - 3, x_lo) * p.x_l_stride, n);
                    gr[u] = load_cvec<T, kVec>(go + (s - u) * q.dout_l_stride, n);
                }
#pragma unroll
                for (int u = 0; u < kU; ++u) token(s - u, xr[u], gr[u], s - u - 3 >= x_lo, true, true);
            }
            for (; s >= t0; --s)
                token(s, load_cvec<T, kVec>(x + max(s - 3, x_lo) * p.x_l_stride, n), load_cvec<T, kVec>(go + s * q.dout_l_stride, n),
                      s - 3 >= x_lo, true, true);
        }
    }
    if (!visited) return;
    // per lane and tap (fp32 accumulators zero-filled by the caller, causal_conv1d.cpp:405-407)
    float *dwp = reinterpret_cast<float *>(q.dweight_ptr);
    float *dbp = reinterpret_cast<float *>(q.dbias_ptr);
#pragma unroll
    for (int e = 0; e < V; ++e) {
        if (e < n) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k >= 4 - W) atomicAdd(dwp + (d0 + e) * q.dweight_c_stride + (k - (4 - W)) * q.dweight_width_stride, dw[k][e]);
            if (dbp) atomicAdd(dbp + d0 + e, db[e]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
static int conv_cl_check(const dimsum_conv_cl_params_t &p) {
    if (p.width < 2 || p.width > 4) return DIMSUM_ERR_SHAPE;   // causal_conv1d.cpp:248
    if (p.batch < 0 || p.dim <= 0 || p.seqlen <= 0) return DIMSUM_ERR_SHAPE;
    if (p.dtype < DIMSUM_F32 || p.dtype > DIMSUM_BF16) return DIMSUM_ERR_DTYPE;
    return DIMSUM_OK;
}
// 16-byte accesses along the channels: whole vectors only, every row 16-byte aligned
template <typename T> static bool cl_vec_ok(const void *ptr, int64_t batch_stride, int64_t l_stride, int dim) {
    constexpr int V = 16 / sizeof(T);
    return dim % V == 0 && aligned_to<T>(ptr, 16) && batch_stride % V == 0 && l_stride % V == 0;
}
// (channel blocks, token-chunk blocks, batch rows), clamped to the launch limits (the kernels stride over what a clamp leaves out);
// want_blocks <= 0: one grid row per batch row, else as many as bring the launch to about `want_blocks` workgroups
template <typename T> static dim3 cl_grid(const dimsum_conv_cl_params_t &p, int64_t want_blocks) {
    constexpr int V = 16 / sizeof(T);
    const int64_t vecs = ((int64_t)p.dim + V - 1) / V;
    const int64_t gx = (vecs + kWave - 1) / kWave;
    const int64_t chunks = ((int64_t)p.seqlen + kClChunk - 1) / kClChunk;
    const int64_t gy = std::min<int64_t>((chunks + 3) / 4, 65535);
    int64_t gz = std::min<int64_t>(p.batch, 65535);
    if (want_blocks > 0) gz = std::max<int64_t>(1, std::min<int64_t>(gz, (want_blocks + gx * gy - 1) / (gx * gy)));
    return dim3((unsigned)gx, (unsigned)gy, (unsigned)gz);
}

template <typename T> static int launch_conv_cl_fwd(const dimsum_conv_cl_params_t &p, hipStream_t s) {
    const bool vec = cl_vec_ok<T>(p.x_ptr, p.x_batch_stride, p.x_l_stride, p.dim) &&
                     cl_vec_ok<T>(p.out_ptr, p.out_batch_stride, p.out_l_stride, p.dim);
    const dim3 grid = cl_grid<T>(p, 0);
    if (vec) hipLaunchKernelGGL((causal_conv1d_cl_fwd_kernel<T, true>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((causal_conv1d_cl_fwd_kernel<T, false>), grid, dim3(256), 0, s, p);
    return launch_status();
}
template <typename T> static int launch_conv_cl_bwd(const dimsum_conv_cl_bwd_params_t &q, hipStream_t s) {
    const dimsum_conv_cl_params_t &p = q.fwd;
    const bool vec = cl_vec_ok<T>(p.x_ptr, p.x_batch_stride, p.x_l_stride, p.dim) &&
                     cl_vec_ok<T>(q.dout_ptr, q.dout_batch_stride, q.dout_l_stride, p.dim) &&
                     cl_vec_ok<T>(q.dx_ptr, q.dx_batch_stride, q.dx_l_stride, p.dim);
    // batch rows folded into each wave's register sums: about 1024 workgroups (two resident rounds) keep the chip full while every
    // lane issues its width + 1 atomics per channel once per (chunk, batch rows it owns)
    const dim3 grid = cl_grid<T>(p, 1024);
    if (vec) hipLaunchKernelGGL((causal_conv1d_cl_bwd_kernel<T, true>), grid, dim3(256), 0, s, q);
    else hipLaunchKernelGGL((causal_conv1d_cl_bwd_kernel<T, false>), grid, dim3(256), 0, s, q);
    return launch_status();
}

}  // namespace dimsum

extern "C" int dimsum_causal_conv1d_cl_fwd(const dimsum_conv_cl_params_t *p, void *stream) {
    using namespace dimsum;
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_conv_cl_params_t)) return DIMSUM_ERR_ABI;
    if (!p->x_ptr || !p->weight_ptr || !p->out_ptr) return DIMSUM_ERR_NULL;
    const int rc = conv_cl_check(*p);
    if (rc != DIMSUM_OK) return rc;
    if (any_negative({p->x_batch_stride, p->x_l_stride, p->weight_c_stride, p->weight_width_stride, p->out_batch_stride, p->out_l_stride}))
        return DIMSUM_ERR_STRIDE;
    if (p->batch == 0) return DIMSUM_OK;
    return dispatch_dtype(p->dtype, [&](auto t) { return launch_conv_cl_fwd<decltype(t)>(*p, reinterpret_cast<hipStream_t>(stream)); });
}

extern "C" int dimsum_causal_conv1d_cl_bwd(const dimsum_conv_cl_bwd_params_t *q, void *stream) {
    using namespace dimsum;
    if (!q) return DIMSUM_ERR_NULL;
    if (q->struct_size != sizeof(dimsum_conv_cl_bwd_params_t)) return DIMSUM_ERR_ABI;
    const dimsum_conv_cl_params_t &p = q->fwd;
    if (!p.x_ptr || !p.weight_ptr || !q->dout_ptr || !q->dx_ptr || !q->dweight_ptr) return DIMSUM_ERR_NULL;
    const int rc = conv_cl_check(p);
    if (rc != DIMSUM_OK) return rc;
    if (any_negative({p.x_batch_stride, p.x_l_stride, p.weight_c_stride, p.weight_width_stride, q->dout_batch_stride, q->dout_l_stride,
                      q->dx_batch_stride, q->dx_l_stride, q->dweight_c_stride, q->dweight_width_stride}))
        return DIMSUM_ERR_STRIDE;
    if (p.batch == 0) return DIMSUM_OK;
    return dispatch_dtype(p.dtype, [&](auto t) { return launch_conv_cl_bwd<decltype(t)>(*q, reinterpret_cast<hipStream_t>(stream)); });
}
