// einfft.hip -- the spectral branch of block type "combined_einfft" (see include/dimsum_hip.h):
//   einfft_dft_kernel        real (B, N, C) -> the ortho-normalised 2-D DFT over (N tokens, the 4 channel blocks) as two fp32 planes
//   einfft_idft_real_kernel  planes -> the real part of the inverse transform (the transpose of the kernel above)
//   einfft_mlp_fwd_kernel    per channel block: complex two-layer MLP (ReLU on both parts, complex biases) + softshrink, hidden row in LDS
//   einfft_mlp_bwd_kernel    layer 1 again, both masks, dX and the three plane pairs the parameter gradients are GEMMs of
// fp32 throughout. C = 4 bs; channel c = k bs + j is column j of block k.
//
// The transforms. A workgroup owns TJ columns j of one batch element in all 4 blocks. The 4-point part runs in registers; for a real input it
// gives X0, X2 real and X3 = conj(X1), so a column needs TWO complex N-point transforms, of P = X0 + i X2 and of Q = X1:
//   F(X0)[m] = (F(P)[m] + conj F(P)[N-m]) / 2,  F(X2)[m] = (F(P)[m] - conj F(P)[N-m]) / 2i,  F(X3)[m] = conj F(Q)[N-m].
// The inverse pass mirrors that: only the Hermitian part of each block's spectrum reaches the real output, and two Hermitian spectra travel
// as one complex sequence. The N-point part is an in-place radix-2 decimation-in-frequency FFT in LDS (natural order in, bit-reversed out;
// the epilogue reads at the reversed index), twiddles from an LDS table of N / 2 entries filled with sincospif. The LDS image is
// [n][sequence] (2 TJ sequences, 8 bytes each, the sequence index on the lane): every butterfly access of a wave is one contiguous run, so
// the power-of-two strides of the butterflies never meet the banks. TJ is the largest of {16, 8, 4} with TJ N <= 4096 that divides bs: the
// image is at most 64 KiB + the 4 KiB table, two workgroups per CU.
#include <algorithm>
#include <cmath>

#include "common.hpp"

namespace dimsum {
namespace {

constexpr int kFftBlock = 256;
constexpr int kFftMaxTokens = 1024, kFftMinTokens = 16;
constexpr int kFftMaxElems = 4096;                // TJ * N

__device__ __forceinline__ float2 cmul(float2 a, float2 w) { return make_float2(fmaf(a.x, w.x, -a.y * w.y), fmaf(a.x, w.y, a.y * w.x)); }

// in-place radix-2 DIF over kSeq interleaved sequences of N points: S[n * kSeq + s]. tw[t] = exp(-2 pi i t / N); kInverse conjugates it.
// Ends with a barrier; element m of the result sits at index bitrev(m).
template <int kSeq, bool kInverse> __device__ __forceinline__ void fft_inplace(float2 *S, const float2 *tw, int N) {
    const int work = (N >> 1) * kSeq;
    int tw_step = 1;
    for (int half = N >> 1; half >= 1; half >>= 1, tw_step <<= 1) {
        for (int it = threadIdx.x; it < work; it += kFftBlock) {
            const int s = it % kSeq, t = it / kSeq;
            const int pos = t & (half - 1), i0 = ((t - pos) << 1) + pos, i1 = i0 + half;
            const float2 a = S[i0 * kSeq + s], b = S[i1 * kSeq + s];
            float2 w = tw[pos * tw_step];
            if (kInverse) w.y = -w.y;
            S[i0 * kSeq + s] = make_float2(a.x + b.x, a.y + b.y);
            S[i1 * kSeq + s] = cmul(make_float2(a.x - b.x, a.y - b.y), w);
        }
        __syncthreads();
    }
}

__device__ __forceinline__ void fill_twiddles(float2 *tw, int N) {
    for (int t = threadIdx.x; t < (N >> 1); t += kFftBlock) {
        float s, c;
        sincospif(-2.0f * (float)t / (float)N, &s, &c);        // (the argument is exact: N is a power of two)
        tw[t] = make_float2(c, s);
    }
}

__device__ __forceinline__ int bitrev(int m, int log_n) { return (int)(__brev((unsigned)m) >> (32 - log_n)); }

template <int TJ> __global__ __launch_bounds__(kFftBlock) void einfft_dft_kernel(const dimsum_einfft_dft_params_t p, const int log_n, const float scale) {
    extern __shared__ __attribute__((aligned(16))) float lds_raw[];
    constexpr int kSeq = 2 * TJ;
    const int N = p.tokens, C = p.channels, bs = C >> 2, b = blockIdx.y, j0 = blockIdx.x * TJ;
    float2 *S = reinterpret_cast<float2 *>(lds_raw), *tw = S + N * kSeq;
    fill_twiddles(tw, N);
    const float *xb = static_cast<const float *>(p.x) + (int64_t)b * p.x_batch_stride + j0;
    for (int it = threadIdx.x; it < N * TJ; it += kFftBlock) {
        const int n = it / TJ, j = it % TJ;
        const float *q = xb + (int64_t)n * p.x_token_stride + j;
        const float a = q[0], bb = q[bs], c = q[2 * bs], d = q[3 * bs];
        const float s02 = a + c, s13 = bb + d;
        S[n * kSeq + 2 * j] = make_float2(s02 + s13, s02 - s13);           // P = X0 + i X2
        S[n * kSeq + 2 * j + 1] = make_float2(a - c, d - bb);              // Q = X1 = (a - c) - i (b - d)
    }
    __syncthreads();
    fft_inplace<kSeq, false>(S, tw, N);
    float *re = static_cast<float *>(p.re) + (int64_t)b * N * C + j0, *im = static_cast<float *>(p.im) + (int64_t)b * N * C + j0;
    const float half_scale = 0.5f * scale;
    for (int it = threadIdx.x; it < N * TJ; it += kFftBlock) {
        const int m = it / TJ, j = it % TJ;
        const int pm = bitrev(m, log_n), pn = bitrev((N - m) & (N - 1), log_n);
        const float2 A = S[pm * kSeq + 2 * j], A2 = S[pn * kSeq + 2 * j], Q = S[pm * kSeq + 2 * j + 1], Q2 = S[pn * kSeq + 2 * j + 1];
        const int64_t o = (int64_t)m * C + j;
        re[o] = (A.x + A2.x) * half_scale;
        im[o] = (A.y - A2.y) * half_scale;
        re[o + bs] = Q.x * scale;
        im[o + bs] = Q.y * scale;
        re[o + 2 * bs] = (A.y + A2.y) * half_scale;
        im[o + 2 * bs] = (A2.x - A.x) * half_scale;
        re[o + 3 * bs] = Q2.x * scale;
        im[o + 3 * bs] = -Q2.y * scale;
    }
}

// one spectral row of one column: the inverse 4-point part, U_k = sum_q Z_q i^(k q)
__device__ __forceinline__ void idft4(const float *re, const float *im, int bs, float2 (&U)[4]) {
    const float2 z0 = make_float2(re[0], im[0]), z1 = make_float2(re[bs], im[bs]), z2 = make_float2(re[2 * bs], im[2 * bs]),
                 z3 = make_float2(re[3 * bs], im[3 * bs]);
    const float2 s02 = make_float2(z0.x + z2.x, z0.y + z2.y), s13 = make_float2(z1.x + z3.x, z1.y + z3.y);
    const float2 d02 = make_float2(z0.x - z2.x, z0.y - z2.y), d13 = make_float2(z1.x - z3.x, z1.y - z3.y);
    U[0] = make_float2(s02.x + s13.x, s02.y + s13.y);
    U[2] = make_float2(s02.x - s13.x, s02.y - s13.y);
    U[1] = make_float2(d02.x - d13.y, d02.y + d13.x);
    U[3] = make_float2(d02.x + d13.y, d02.y - d13.x);
}

template <int TJ> __global__ __launch_bounds__(kFftBlock) void einfft_idft_real_kernel(const dimsum_einfft_dft_params_t p, const int log_n, const float scale) {
    extern __shared__ __attribute__((aligned(16))) float lds_raw[];
    constexpr int kSeq = 2 * TJ;
    const int N = p.tokens, C = p.channels, bs = C >> 2, b = blockIdx.y, j0 = blockIdx.x * TJ;
    float2 *S = reinterpret_cast<float2 *>(lds_raw), *tw = S + N * kSeq;
    fill_twiddles(tw, N);
    const float *re = static_cast<const float *>(p.re) + (int64_t)b * N * C + j0, *im = static_cast<const float *>(p.im) + (int64_t)b * N * C + j0;
    // a thread owns the rows m and N - m of one column: G_k = U_k[m] + conj U_k[N - m] is twice the Hermitian part at m, its conjugate the
    // one at N - m; blocks (0, 2) and (1, 3) share a complex sequence. For m = 0 and m = N / 2 both rows are the same one and G_k is real.
    for (int it = threadIdx.x; it < ((N >> 1) + 1) * TJ; it += kFftBlock) {
        const int m = it / TJ, j = it % TJ, m2 = (N - m) & (N - 1);
        float2 U[4], V[4];
        idft4(re + (int64_t)m * C + j, im + (int64_t)m * C + j, bs, U);
        idft4(re + (int64_t)m2 * C + j, im + (int64_t)m2 * C + j, bs, V);
        float2 G[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) G[k] = make_float2(U[k].x + V[k].x, U[k].y - V[k].y);
        S[m * kSeq + 2 * j] = make_float2(G[0].x - G[2].y, G[0].y + G[2].x);
        S[m * kSeq + 2 * j + 1] = make_float2(G[1].x - G[3].y, G[1].y + G[3].x);
        if (m2 != m) {
            S[m2 * kSeq + 2 * j] = make_float2(G[0].x + G[2].y, G[2].x - G[0].y);
            S[m2 * kSeq + 2 * j + 1] = make_float2(G[1].x + G[3].y, G[3].x - G[1].y);
        }
    }
    __syncthreads();
    fft_inplace<kSeq, true>(S, tw, N);
    float *yb = static_cast<float *>(p.x) + (int64_t)b * p.x_batch_stride + j0;
    const float half_scale = 0.5f * scale;
    for (int it = threadIdx.x; it < N * TJ; it += kFftBlock) {
        const int n = it / TJ, j = it % TJ, pn = bitrev(n, log_n);
        const float2 A = S[pn * kSeq + 2 * j], Bq = S[pn * kSeq + 2 * j + 1];
        float *q = yb + (int64_t)n * p.x_token_stride + j;
        q[0] = A.x * half_scale;
        q[bs] = Bq.x * half_scale;
        q[2 * bs] = A.y * half_scale;
        q[3 * bs] = Bq.y * half_scale;
    }
}

// ---- the block-diagonal complex MLP ---------------------------------------------------------------------------------------------------------
// A workgroup owns kMlpRows spectral rows of ONE channel block. Operand tiles live in LDS as [column c of (re | im)][row], rows in groups of 4
// (one 16-byte slot), slot index XOR (c & 7): a wave writes the slots of consecutive c without sharing a bank, and reads one slot per row
// group as a broadcast. A thread's micro-tile is 4 rows x 4 columns {cg, cg + bs/4, cg + 2 bs/4, cg + 3 bs/4} of both parts: consecutive
// lanes hold consecutive columns, so the weight rows (from L2: bs^2 floats per part, layer and block) and the global stores coalesce.
constexpr int kMlpRows = 32;
constexpr int kMlpMaxBs = 256;                    // 2 tiles of 2 bs x 32 floats: 128 KiB of LDS

__device__ __forceinline__ int slot(int c, int rg) { return c * kMlpRows + ((rg ^ (c & 7)) << 2); }

// acc += in . [[A, sgn B], [-sgn B, A]] for the micro-tile (rg, cg): in is an LDS tile, A and B are (bs, bs) row-major [input][output]
__device__ __forceinline__ void cgemm_tile(const float *in, const float *__restrict__ A, const float *__restrict__ Bm, float sgn, int bs, int rg,
                                           int cg, float (&ar)[4][4], float (&ai)[4][4]) {
    const int nq = bs >> 2;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) ar[i][e] = 0.f, ai[i][e] = 0.f;
    for (int d = 0; d < bs; ++d) {
        const float4 xr = *reinterpret_cast<const float4 *>(in + slot(d, rg)), xi = *reinterpret_cast<const float4 *>(in + slot(bs + d, rg));
        const float xrv[4] = {xr.x, xr.y, xr.z, xr.w}, xiv[4] = {xi.x, xi.y, xi.z, xi.w};
        const float *arow = A + (int64_t)d * bs + cg, *brow = Bm + (int64_t)d * bs + cg;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float a = arow[e * nq], bb = sgn * brow[e * nq];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                ar[i][e] = fmaf(xrv[i], a, fmaf(-xiv[i], bb, ar[i][e]));
                ai[i][e] = fmaf(xrv[i], bb, fmaf(xiv[i], a, ai[i][e]));
            }
        }
    }
}

// rows [row0, row0 + 32) of block k of a plane pair -> an LDS tile (rows past `rows`: zeros). A thread: one column, 4 rows, one 16-byte write.
__device__ __forceinline__ void load_tile(float *tile, const float *pr, const float *pi, int64_t row0, int64_t rows, int C, int bs, int k) {
    for (int it = threadIdx.x; it < 2 * bs * (kMlpRows / 4); it += blockDim.x) {
        const int c = it % (2 * bs), rg = it / (2 * bs);
        const float *src = (c < bs ? pr + c : pi + (c - bs)) + k * bs;
        float4 v;
        float *vv = reinterpret_cast<float *>(&v);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t r = row0 + rg * 4 + i;
            vv[i] = r < rows ? src[r * C] : 0.f;
        }
        *reinterpret_cast<float4 *>(tile + slot(c, rg)) = v;
    }
}

__device__ __forceinline__ void put_tile(float *tile, int c, int rg, const float (&v)[4]) {
    *reinterpret_cast<float4 *>(tile + slot(c, rg)) = make_float4(v[0], v[1], v[2], v[3]);
}

__device__ __forceinline__ float softshrink(float v, float lam) { return v > lam ? v - lam : (v < -lam ? v + lam : 0.f); }

__global__ __launch_bounds__(512) void einfft_mlp_fwd_kernel(const dimsum_einfft_mlp_params_t p) {
    extern __shared__ __attribute__((aligned(16))) float lds_raw[];
    const int C = p.channels, bs = C >> 2, nq = bs >> 2, k = blockIdx.y;
    const int64_t rows = p.rows, row0 = (int64_t)blockIdx.x * kMlpRows;
    float *Xs = lds_raw, *Hs = lds_raw + 2 * bs * kMlpRows;
    const float *w1r = static_cast<const float *>(p.w1) + (int64_t)k * bs * bs, *w1i = w1r + (int64_t)4 * bs * bs;
    const float *w2r = static_cast<const float *>(p.w2) + (int64_t)k * bs * bs, *w2i = w2r + (int64_t)4 * bs * bs;
    const float *b1r = static_cast<const float *>(p.b1) + k * bs, *b1i = b1r + 4 * bs, *b2r = static_cast<const float *>(p.b2) + k * bs, *b2i = b2r + 4 * bs;
    load_tile(Xs, static_cast<const float *>(p.xr), static_cast<const float *>(p.xi), row0, rows, C, bs, k);
    __syncthreads();
    const int items = (kMlpRows / 4) * nq;
    float ar[4][4], ai[4][4];
    for (int it = threadIdx.x; it < items; it += blockDim.x) {
        const int cg = it % nq, rg = it / nq;
        cgemm_tile(Xs, w1r, w1i, 1.f, bs, rg, cg, ar, ai);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int o = cg + e * nq;
            const float br = b1r[o], bi = b1i[o];
            float hr[4], hi[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) hr[i] = fmaxf(ar[i][e] + br, 0.f), hi[i] = fmaxf(ai[i][e] + bi, 0.f);
            put_tile(Hs, o, rg, hr);
            put_tile(Hs, bs + o, rg, hi);
        }
    }
    __syncthreads();
    float *zr = static_cast<float *>(p.zr) + k * bs, *zi = static_cast<float *>(p.zi) + k * bs;
    for (int it = threadIdx.x; it < items; it += blockDim.x) {
        const int cg = it % nq, rg = it / nq;
        cgemm_tile(Hs, w2r, w2i, 1.f, bs, rg, cg, ar, ai);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int o = cg + e * nq;
            const float br = b2r[o], bi = b2i[o];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t r = row0 + rg * 4 + i;
                if (r < rows) {
                    zr[r * C + o] = softshrink(ar[i][e] + br, p.lam);
                    zi[r * C + o] = softshrink(ai[i][e] + bi, p.lam);
                }
            }
        }
    }
}

// Backward of the kernel above for one tile: H1 = relu(X W1 + b1) again; dZ2 = dZ where the forward's output z is non-zero (softshrink passes
// exactly the elements it does not zero); dP1 = (dZ2 W2^T) where H1 > 0; dX = dP1 W1^T. w1t / w2t hold the transposed matrices
// ((2, 4, bs, bs) as [output][input]) so that the same coalesced row walk serves the transposed products.
__global__ __launch_bounds__(512) void einfft_mlp_bwd_kernel(const dimsum_einfft_mlp_bwd_params_t p) {
    extern __shared__ __attribute__((aligned(16))) float lds_raw[];
    const dimsum_einfft_mlp_params_t &f = p.fwd;
    const int C = f.channels, bs = C >> 2, nq = bs >> 2, k = blockIdx.y;
    const int64_t rows = f.rows, row0 = (int64_t)blockIdx.x * kMlpRows;
    float *Xs = lds_raw, *Hs = lds_raw + 2 * bs * kMlpRows;
    const int64_t wk = (int64_t)k * bs * bs, wi = (int64_t)4 * bs * bs;
    const float *w1r = static_cast<const float *>(f.w1) + wk, *w1i = w1r + wi;
    const float *w1tr = static_cast<const float *>(p.w1t) + wk, *w1ti = w1tr + wi, *w2tr = static_cast<const float *>(p.w2t) + wk, *w2ti = w2tr + wi;
    const float *b1r = static_cast<const float *>(f.b1) + k * bs, *b1i = b1r + 4 * bs;
    load_tile(Xs, static_cast<const float *>(f.xr), static_cast<const float *>(f.xi), row0, rows, C, bs, k);
    __syncthreads();
    const int items = (kMlpRows / 4) * nq, kb = k * bs;
    float ar[4][4], ai[4][4];
    float *h1r = static_cast<float *>(p.h1r) + kb, *h1i = static_cast<float *>(p.h1i) + kb;
    for (int it = threadIdx.x; it < items; it += blockDim.x) {
        const int cg = it % nq, rg = it / nq;
        cgemm_tile(Xs, w1r, w1i, 1.f, bs, rg, cg, ar, ai);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int o = cg + e * nq;
            const float br = b1r[o], bi = b1i[o];
            float hr[4], hi[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                hr[i] = fmaxf(ar[i][e] + br, 0.f), hi[i] = fmaxf(ai[i][e] + bi, 0.f);
                const int64_t r = row0 + rg * 4 + i;
                if (r < rows) h1r[r * C + o] = hr[i], h1i[r * C + o] = hi[i];
            }
            put_tile(Hs, o, rg, hr);
            put_tile(Hs, bs + o, rg, hi);
        }
    }
    __syncthreads();                                  // every read of the X tile is done: it becomes the dZ2 tile
    {
        const float *dzr = static_cast<const float *>(p.dzr) + kb, *dzi = static_cast<const float *>(p.dzi) + kb;
        const float *zr = static_cast<const float *>(f.zr) + kb, *zi = static_cast<const float *>(f.zi) + kb;
        float *dz2r = static_cast<float *>(p.dz2r) + kb, *dz2i = static_cast<float *>(p.dz2i) + kb;
        for (int it = threadIdx.x; it < 2 * bs * (kMlpRows / 4); it += blockDim.x) {
            const int c = it % (2 * bs), rg = it / (2 * bs), o = c < bs ? c : c - bs;
            const float *g = c < bs ? dzr : dzi, *z = c < bs ? zr : zi;
            float *out = c < bs ? dz2r : dz2i;
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t r = row0 + rg * 4 + i;
                v[i] = 0.f;
                if (r < rows) {
                    v[i] = z[r * C + o] != 0.f ? g[r * C + o] : 0.f;
                    out[r * C + o] = v[i];
                }
            }
            put_tile(Xs, c, rg, v);
        }
    }
    __syncthreads();
    float *dp1r = static_cast<float *>(p.dp1r) + kb, *dp1i = static_cast<float *>(p.dp1i) + kb;
    for (int it = threadIdx.x; it < items; it += blockDim.x) {
        const int cg = it % nq, rg = it / nq;
        cgemm_tile(Xs, w2tr, w2ti, -1.f, bs, rg, cg, ar, ai);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int o = cg + e * nq;
            const float4 mr = *reinterpret_cast<const float4 *>(Hs + slot(o, rg)), mi = *reinterpret_cast<const float4 *>(Hs + slot(bs + o, rg));
            const float mrv[4] = {mr.x, mr.y, mr.z, mr.w}, miv[4] = {mi.x, mi.y, mi.z, mi.w};
            float gr[4], gi[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                gr[i] = mrv[i] > 0.f ? ar[i][e] : 0.f, gi[i] = miv[i] > 0.f ? ai[i][e] : 0.f;
                const int64_t r = row0 + rg * 4 + i;
                if (r < rows) dp1r[r * C + o] = gr[i], dp1i[r * C + o] = gi[i];
            }
            put_tile(Hs, o, rg, gr);                  // (this thread alone reads and writes these two slots in this phase)
            put_tile(Hs, bs + o, rg, gi);
        }
    }
    __syncthreads();
    float *dxr = static_cast<float *>(p.dxr) + kb, *dxi = static_cast<float *>(p.dxi) + kb;
    for (int it = threadIdx.x; it < items; it += blockDim.x) {
        const int cg = it % nq, rg = it / nq;
        cgemm_tile(Hs, w1tr, w1ti, -1.f, bs, rg, cg, ar, ai);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int o = cg + e * nq;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t r = row0 + rg * 4 + i;
                if (r < rows) dxr[r * C + o] = ar[i][e], dxi[r * C + o] = ai[i][e];
            }
        }
    }
}

inline int log2_exact(int n) {
    int l = 0;
    while ((1 << l) < n) ++l;
    return (1 << l) == n ? l : -1;
}

int check_dft(const dimsum_einfft_dft_params_t *p) {
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_einfft_dft_params_t)) return DIMSUM_ERR_ABI;
    if (!p->x || !p->re || !p->im) return DIMSUM_ERR_NULL;
    if (p->batch <= 0 || p->batch > 65535 || p->tokens < kFftMinTokens || p->tokens > kFftMaxTokens || log2_exact(p->tokens) < 0
        || p->channels < 32 || p->channels % 32)
        return DIMSUM_ERR_SHAPE;
    if (p->x_token_stride < p->channels || p->x_batch_stride < 0 || (p->batch > 1 && p->x_batch_stride < (int64_t)(p->tokens - 1) * p->x_token_stride + p->channels))
        return DIMSUM_ERR_STRIDE;
    return DIMSUM_OK;
}

inline int dft_tile(const dimsum_einfft_dft_params_t &p) {
    const int bs = p.channels / 4;
    if (bs % 16 == 0 && 16 * p.tokens <= kFftMaxElems) return 16;
    if (8 * p.tokens <= kFftMaxElems) return 8;
    return 4;
}

template <typename K> int launch_fft(K kernel, const dimsum_einfft_dft_params_t &p, int tj, void *stream) {
    const size_t lds = ((size_t)2 * tj * p.tokens + p.tokens / 2) * sizeof(float2);
    if (lds > 48 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        (void)hipGetLastError();
        return DIMSUM_ERR_LAUNCH;
    }
    const float scale = (float)(1.0 / sqrt(4.0 * (double)p.tokens));
    hipLaunchKernelGGL(kernel, dim3((unsigned)(p.channels / 4 / tj), (unsigned)p.batch), dim3(kFftBlock), lds, reinterpret_cast<hipStream_t>(stream),
                       p, log2_exact(p.tokens), scale);
    return launch_status();
}

int check_mlp(const dimsum_einfft_mlp_params_t &f) {
    if (!f.xr || !f.xi || !f.w1 || !f.b1 || !f.w2 || !f.b2 || !f.zr || !f.zi) return DIMSUM_ERR_NULL;
    if (f.rows <= 0 || f.rows > ((int64_t)1 << 31) - 1 || f.channels < 32 || f.channels % 32 || f.channels / 4 > kMlpMaxBs) return DIMSUM_ERR_SHAPE;
    if (!(f.lam >= 0.f)) return DIMSUM_ERR_SHAPE;
    return DIMSUM_OK;
}

template <typename K, typename P> int launch_mlp(K kernel, const P &p, const dimsum_einfft_mlp_params_t &f, void *stream) {
    const int bs = f.channels / 4;
    const size_t lds = (size_t)2 * 2 * bs * kMlpRows * sizeof(float);
    if (lds > 48 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        (void)hipGetLastError();
        return DIMSUM_ERR_LAUNCH;
    }
    const int items = (kMlpRows / 4) * (bs / 4);
    const int block = std::min(512, (items + kWave - 1) / kWave * kWave);
    const int64_t tiles = (f.rows + kMlpRows - 1) / kMlpRows;
    hipLaunchKernelGGL(kernel, dim3((unsigned)tiles, 4u), dim3((unsigned)block), lds, reinterpret_cast<hipStream_t>(stream), p);
    return launch_status();
}

}  // namespace
}  // namespace dimsum

extern "C" int dimsum_einfft_dft(const dimsum_einfft_dft_params_t *p, void *stream) {
    using namespace dimsum;
    if (const int st = check_dft(p)) return st;
    switch (dft_tile(*p)) {
        case 16: return launch_fft(einfft_dft_kernel<16>, *p, 16, stream);
        case 8: return launch_fft(einfft_dft_kernel<8>, *p, 8, stream);
        default: return launch_fft(einfft_dft_kernel<4>, *p, 4, stream);
    }
}

extern "C" int dimsum_einfft_idft_real(const dimsum_einfft_dft_params_t *p, void *stream) {
    using namespace dimsum;
    if (const int st = check_dft(p)) return st;
    switch (dft_tile(*p)) {
        case 16: return launch_fft(einfft_idft_real_kernel<16>, *p, 16, stream);
        case 8: return launch_fft(einfft_idft_real_kernel<8>, *p, 8, stream);
        default: return launch_fft(einfft_idft_real_kernel<4>, *p, 4, stream);
    }
}

extern "C" int dimsum_einfft_mlp_fwd(const dimsum_einfft_mlp_params_t *p, void *stream) {
    using namespace dimsum;
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_einfft_mlp_params_t)) return DIMSUM_ERR_ABI;
    if (const int st = check_mlp(*p)) return st;
    return launch_mlp(einfft_mlp_fwd_kernel, *p, *p, stream);
}

extern "C" int dimsum_einfft_mlp_bwd(const dimsum_einfft_mlp_bwd_params_t *p, void *stream) {
    using namespace dimsum;
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_einfft_mlp_bwd_params_t)) return DIMSUM_ERR_ABI;
    if (const int st = check_mlp(p->fwd)) return st;
    if (!p->w1t || !p->w2t || !p->dzr || !p->dzi || !p->dxr || !p->dxi || !p->h1r || !p->h1i || !p->dz2r || !p->dz2i || !p->dp1r || !p->dp1i) return DIMSUM_ERR_NULL;
    return launch_mlp(einfft_mlp_bwd_kernel, *p, p->fwd, stream);
}
