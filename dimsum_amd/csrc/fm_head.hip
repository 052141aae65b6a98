// fm_head.hip -- the head of a training step (see include/dimsum_hip.h):
//   fm_plan_plain_kernel     xt = alpha x1 + sigma x0, ut = d_alpha x1 + d_sigma x0, per-sample coefficients from a (5, batch) table
//   fm_plan_blur_kernel<P>   the same with x1 replaced, for xt only, by its DCT-blurred image: one P x P tile per lane, held in registers,
//                            C X C^T as 2 P fully unrolled P-point products against a compile-time table, the gain applied in 2-D, and back
//   fm_loss_fwd_kernel       loss_b = w_b mean (c_b out + sign tgt)^2, one workgroup per sample, one fixed summation order
//   fm_loss_bwd_kernel       dout = gloss_b 2 w_b c_b (c_b out + sign tgt) / n
// fp32 in and out, no atomics, no LDS beyond the four partial sums of the loss.
#include "common.hpp"

namespace dimsum {
namespace {

constexpr int kBlock = 256;
constexpr int kPass = kBlock * 4;                      // elements per pass of a workgroup

// orthonormal DCT-II matrices, c[k][n] = s_k cos(pi (2 n + 1) k / (2 P)), s_0 = sqrt(1 / P), s_k = sqrt(2 / P)
__device__ constexpr float kDct2[2][2] = {
    {0.707106769f, 0.707106769f},
    {0.707106769f, -0.707106769f},
};
__device__ constexpr float kDct4[4][4] = {
    {0.5f, 0.5f, 0.5f, 0.5f},
    {0.65328151f, 0.270598054f, -0.270598054f, -0.65328151f},
    {0.5f, -0.5f, -0.5f, 0.5f},
    {0.270598054f, -0.65328151f, 0.65328151f, -0.270598054f},
};
__device__ constexpr float kDct8[8][8] = {
    {0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f},
    {0.490392625f, 0.415734798f, 0.277785122f, 0.0975451618f, -0.0975451618f, -0.277785122f, -0.415734798f, -0.490392625f},
    {0.461939752f, 0.191341713f, -0.191341713f, -0.461939752f, -0.461939752f, -0.191341713f, 0.191341713f, 0.461939752f},
    {0.415734798f, -0.0975451618f, -0.490392625f, -0.277785122f, 0.277785122f, 0.490392625f, 0.0975451618f, -0.415734798f},
    {0.353553385f, -0.353553385f, -0.353553385f, 0.353553385f, 0.353553385f, -0.353553385f, -0.353553385f, 0.353553385f},
    {0.277785122f, -0.490392625f, 0.0975451618f, 0.415734798f, -0.415734798f, -0.0975451618f, 0.490392625f, -0.277785122f},
    {0.191341713f, -0.461939752f, 0.461939752f, -0.191341713f, -0.191341713f, 0.461939752f, -0.461939752f, 0.191341713f},
    {0.0975451618f, -0.277785122f, 0.415734798f, -0.490392625f, 0.490392625f, -0.415734798f, 0.277785122f, -0.0975451618f},
};
// entry [k][n] of the P-point matrix (kInv: of its transpose, the inverse); k and n are constants after unrolling, so this folds to a literal
template <int P, bool kInv> __device__ __forceinline__ constexpr float dct_c(int k, int n) {
    const int r = kInv ? n : k, c = kInv ? k : n;
    if constexpr (P == 2) return kDct2[r][c];
    else if constexpr (P == 4) return kDct4[r][c];
    else return kDct8[r][c];
}

struct Coef { float alpha, sigma, d_alpha, d_sigma; };
__device__ __forceinline__ Coef coef_at(const float *table, int batch, int b) {
    return {table[b], table[batch + b], table[2 * batch + b], table[3 * batch + b]};
}

// a x (+ s y): every product is rounded before the sum, as in the expression evaluated pass by pass
__device__ __forceinline__ float mix(float a, float x, float s, float y, bool has_y) {
#pragma clang fp contract(off)
    const float ax = a * x;
    if (!has_y) return ax;
    const float sy = s * y;
    return ax + sy;
}

// elements [0, 4) at q; `n` of them exist (n >= 1), the rest read as 0. kVec: q is 16-byte aligned
template <bool kVec> __device__ __forceinline__ f32x4 load4(const float *q, int64_t n) {
    if (kVec && n >= 4) return widen(ld4<float>(q));
    f32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r.v[j] = j < n ? q[j] : 0.f;
    return r;
}
template <bool kVec> __device__ __forceinline__ void store4(float *q, int64_t n, const f32x4 &a) {
    if (kVec && n >= 4) {
        st4<float>(q, a);
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < n) q[j] = a.v[j];
}

// ---- the plan without blur: workgroup = (sample, 1024 consecutive elements of it) -----------------------------------------------------------
template <bool kVec> __global__ __launch_bounds__(kBlock) void fm_plan_plain_kernel(const dimsum_fm_plan_params_t p, const int64_t n, const int blocks_per_sample) {
    const int b = blockIdx.x / blocks_per_sample;
    const int64_t i = ((int64_t)(blockIdx.x - b * blocks_per_sample) * kBlock + threadIdx.x) * 4;
    if (i >= n) return;
    const int64_t left = n - i, o = (int64_t)b * n + i;
    const Coef k = coef_at(static_cast<const float *>(p.coef), p.batch, b);
    const bool has0 = p.x0 != nullptr;
    const f32x4 a = load4<kVec>(static_cast<const float *>(p.x1) + (int64_t)b * p.x1_batch_stride + i, left);
    f32x4 z = {{0.f, 0.f, 0.f, 0.f}}, r;
    if (has0) z = load4<kVec>(static_cast<const float *>(p.x0) + o, left);
#pragma unroll
    for (int j = 0; j < 4; ++j) r.v[j] = mix(k.alpha, a.v[j], k.sigma, z.v[j], has0);
    store4<kVec>(static_cast<float *>(p.xt) + o, left, r);
    if (p.ut) {
#pragma unroll
        for (int j = 0; j < 4; ++j) r.v[j] = mix(k.d_alpha, a.v[j], k.d_sigma, z.v[j], has0);
        store4<kVec>(static_cast<float *>(p.ut) + o, left, r);
    }
}

// ---- the plan with blur: lane = one P x P tile, adjacent lanes = adjacent tiles along the width ---------------------------------------------
template <int P> __device__ __forceinline__ void load_row(const float *q, float (&r)[P]) {
    if constexpr (P == 2) {
        const float2 v = *reinterpret_cast<const float2 *>(q);
        r[0] = v.x, r[1] = v.y;
    } else {
#pragma unroll
        for (int j = 0; j < P; j += 4) {
            const float4 v = *reinterpret_cast<const float4 *>(q + j);
            r[j] = v.x, r[j + 1] = v.y, r[j + 2] = v.z, r[j + 3] = v.w;
        }
    }
}
template <int P> __device__ __forceinline__ void store_row(float *q, const float (&r)[P]) {
    if constexpr (P == 2) {
        *reinterpret_cast<float2 *>(q) = make_float2(r[0], r[1]);
    } else {
#pragma unroll
        for (int j = 0; j < P; j += 4) *reinterpret_cast<float4 *>(q + j) = make_float4(r[j], r[j + 1], r[j + 2], r[j + 3]);
    }
}

// x <- x M^T along the rows, then x <- M x along the columns, M = C (forward) or C^T (inverse), in place: P temporaries
template <int P, bool kInv> __device__ __forceinline__ void dct2d(float (&x)[P][P]) {
#pragma unroll
    for (int r = 0; r < P; ++r) {
        float t[P];
#pragma unroll
        for (int k = 0; k < P; ++k) {
            float acc = 0.f;
#pragma unroll
            for (int n = 0; n < P; ++n) acc = fmaf(x[r][n], dct_c<P, kInv>(k, n), acc);
            t[k] = acc;
        }
#pragma unroll
        for (int k = 0; k < P; ++k) x[r][k] = t[k];
    }
#pragma unroll
    for (int j = 0; j < P; ++j) {
        float t[P];
#pragma unroll
        for (int k = 0; k < P; ++k) {
            float acc = 0.f;
#pragma unroll
            for (int n = 0; n < P; ++n) acc = fmaf(dct_c<P, kInv>(k, n), x[n][j], acc);
            t[k] = acc;
        }
#pragma unroll
        for (int k = 0; k < P; ++k) x[k][j] = t[k];
    }
}

template <int P> __global__ __launch_bounds__(kBlock) void fm_plan_blur_kernel(const dimsum_fm_plan_params_t p) {
    const int wp = p.width / P, hp = p.height / P;
    const int64_t per_sample = (int64_t)p.channels * hp * wp, tile = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (tile >= per_sample * p.batch) return;
    const int b = (int)(tile / per_sample);
    const int64_t rem = tile - b * per_sample, row_of_tiles = rem / wp;         // row_of_tiles = channel * hp + tile row
    const int tw = (int)(rem - row_of_tiles * wp);
    // height == hp * P, so (channel * height + tile row * P) == row_of_tiles * P
    const int64_t in_sample = row_of_tiles * P * p.width + (int64_t)tw * P;
    const int64_t o = (int64_t)b * p.channels * p.height * p.width + in_sample;
    const float *x1 = static_cast<const float *>(p.x1) + (int64_t)b * p.x1_batch_stride + in_sample;
    const float *x0 = p.x0 ? static_cast<const float *>(p.x0) + o : nullptr;
    float *xt = static_cast<float *>(p.xt) + o, *ut = p.ut ? static_cast<float *>(p.ut) + o : nullptr;
    const float *table = static_cast<const float *>(p.coef);
    const Coef k = coef_at(table, p.batch, b);
    const float blur_t = table[4 * p.batch + b];
    const bool has0 = x0 != nullptr;

    // the tile; ut leaves on the way in (it wants the unblurred x1), so that only the tile itself stays in registers across the transform
    float x[P][P];
#pragma unroll
    for (int r = 0; r < P; ++r) {
        load_row<P>(x1 + (int64_t)r * p.width, x[r]);
        if (ut) {
            float z[P], u[P];
            if (has0) load_row<P>(x0 + (int64_t)r * p.width, z);
#pragma unroll
            for (int j = 0; j < P; ++j) u[j] = mix(k.d_alpha, x[r][j], k.d_sigma, has0 ? z[j] : 0.f, has0);
            store_row<P>(ut + (int64_t)r * p.width, u);
        }
    }

    dct2d<P, false>(x);
    // G[i][j] = exp(-(f_i^2 + f_j^2) blur_t) (1 - min_scale) + min_scale: P exponentials per tile, the floor keeps it from being separable
    float e[P];
#pragma unroll
    for (int i = 0; i < P; ++i) {
        constexpr float kPi = 3.14159265358979323846f;
        const float f = kPi * (float)i / (float)P;
        e[i] = expf(-(f * f) * blur_t);
    }
    const float keep = 1.f - p.min_scale;
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
        for (int j = 0; j < P; ++j) x[i][j] *= fmaf(e[i] * e[j], keep, p.min_scale);
    dct2d<P, true>(x);

    // x0 comes a second time (out of the cache: the same lines as a moment ago) instead of living in P * P registers through the transform
#pragma unroll
    for (int r = 0; r < P; ++r) {
        float z[P], y[P];
        if (has0) load_row<P>(x0 + (int64_t)r * p.width, z);
#pragma unroll
        for (int j = 0; j < P; ++j) y[j] = mix(k.alpha, x[r][j], k.sigma, has0 ? z[j] : 0.f, has0);
        store_row<P>(xt + (int64_t)r * p.width, y);
    }
}

// ---- the loss ---------------------------------------------------------------------------------------------------------------------------------
// lane l owns the elements [1024 k + 4 l, + 4) of its sample, as one 16-byte load or as four 4-byte ones: the sums never depend on the alignment
template <bool kVec> __device__ __forceinline__ float sumsq_sample(const float *out, const float *tgt, int64_t n, int tid, float c, float sign) {
    float acc = 0.f;
    for (int64_t i = (int64_t)tid * 4; i < n; i += kPass) {
        const f32x4 a = load4<kVec>(out + i, n - i), t = load4<kVec>(tgt + i, n - i);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float d = fmaf(c, a.v[j], sign * t.v[j]);
            acc = fmaf(d, d, acc);                                  // the padding adds +0
        }
    }
    return acc;
}

__device__ __forceinline__ bool aligned16(const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

__global__ __launch_bounds__(kBlock) void fm_loss_fwd_kernel(const dimsum_fm_loss_params_t p) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const float *out = static_cast<const float *>(p.out) + (int64_t)b * p.n, *tgt = static_cast<const float *>(p.tgt) + (int64_t)b * p.n;
    const float c = p.c ? static_cast<const float *>(p.c)[b] : 1.f;
    float acc = aligned16(out) && aligned16(tgt) ? sumsq_sample<true>(out, tgt, p.n, tid, c, p.sign)
                                                 : sumsq_sample<false>(out, tgt, p.n, tid, c, p.sign);
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, kWave);
    __shared__ float red[kBlock / kWave];
    if ((tid & (kWave - 1)) == 0) red[tid / kWave] = acc;
    __syncthreads();
    if (tid == 0) {
        const float w = p.w ? static_cast<const float *>(p.w)[b] : 1.f;
        static_cast<float *>(p.loss)[b] = w * (((red[0] + red[1]) + (red[2] + red[3])) / (float)p.n);
    }
}

__global__ __launch_bounds__(kBlock) void fm_loss_bwd_kernel(const dimsum_fm_loss_params_t p, const int blocks_per_sample) {
    const int b = blockIdx.x / blocks_per_sample;
    const int64_t i = ((int64_t)(blockIdx.x - b * blocks_per_sample) * kBlock + threadIdx.x) * 4;
    if (i >= p.n) return;
    const int64_t left = p.n - i, o = (int64_t)b * p.n + i;
    const float *out = static_cast<const float *>(p.out) + o, *tgt = static_cast<const float *>(p.tgt) + o;
    float *dout = static_cast<float *>(p.dout) + o;
    const float c = p.c ? static_cast<const float *>(p.c)[b] : 1.f, w = p.w ? static_cast<const float *>(p.w)[b] : 1.f;
    const float k = static_cast<const float *>(p.gloss)[b] * 2.f * w * c / (float)p.n;
    const bool vec = aligned16(out) && aligned16(tgt) && aligned16(dout);
    const f32x4 a = vec ? load4<true>(out, left) : load4<false>(out, left), t = vec ? load4<true>(tgt, left) : load4<false>(tgt, left);
    f32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r.v[j] = k * fmaf(c, a.v[j], p.sign * t.v[j]);
    if (vec) store4<true>(dout, left, r);
    else store4<false>(dout, left, r);
}

// blocks of 1024 elements per sample times the batch, as one grid dimension; 0: does not fit
inline int64_t grid_for(int64_t n, int64_t batch, int *blocks_per_sample) {
    const int64_t per = (n + kPass - 1) / kPass;
    if (per <= 0 || per >= ((int64_t)1 << 31) || per * batch >= ((int64_t)1 << 31)) return 0;
    *blocks_per_sample = (int)per;
    return per * batch;
}

int check_loss(const dimsum_fm_loss_params_t *p, bool bwd) {
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_fm_loss_params_t)) return DIMSUM_ERR_ABI;
    if (!p->out || !p->tgt || (bwd ? (!p->gloss || !p->dout) : !p->loss)) return DIMSUM_ERR_NULL;
    if (p->batch <= 0 || p->n <= 0 || p->n >= ((int64_t)1 << 31)) return DIMSUM_ERR_SHAPE;
    if (p->sign != 1.f && p->sign != -1.f) return DIMSUM_ERR_UNSUPPORTED;
    return DIMSUM_OK;
}

}  // namespace
}  // namespace dimsum

extern "C" int dimsum_fm_plan(const dimsum_fm_plan_params_t *p, void *stream) {
    using namespace dimsum;
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_fm_plan_params_t)) return DIMSUM_ERR_ABI;
    if (!p->x1 || !p->coef || !p->xt) return DIMSUM_ERR_NULL;
    if (p->batch <= 0 || p->channels <= 0 || p->height <= 0 || p->width <= 0) return DIMSUM_ERR_SHAPE;
    const int64_t n = (int64_t)p->channels * p->height * p->width;
    if (n >= ((int64_t)1 << 31) || p->x1_batch_stride < 0) return DIMSUM_ERR_STRIDE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int P = p->patch;
    auto aligned = [&](size_t bytes) {
        return aligned_to<float>(p->x1, bytes) && aligned_to<float>(p->x0, bytes) && aligned_to<float>(p->xt, bytes) && aligned_to<float>(p->ut, bytes)
               && (p->x1_batch_stride * sizeof(float)) % bytes == 0 && (n * sizeof(float)) % bytes == 0;
    };
    if (P == 0) {
        int per = 0;
        const int64_t blocks = grid_for(n, p->batch, &per);
        if (!blocks) return DIMSUM_ERR_SHAPE;
        if (aligned(16)) hipLaunchKernelGGL(fm_plan_plain_kernel<true>, dim3((unsigned)blocks), dim3(kBlock), 0, s, *p, n, per);
        else hipLaunchKernelGGL(fm_plan_plain_kernel<false>, dim3((unsigned)blocks), dim3(kBlock), 0, s, *p, n, per);
        return launch_status();
    }
    if (P != 2 && P != 4 && P != 8) return DIMSUM_ERR_UNSUPPORTED;
    if (p->height != p->width || p->height % P != 0) return DIMSUM_ERR_SHAPE;
    if (!aligned(P == 2 ? 8 : 16)) return DIMSUM_ERR_STRIDE;
    const int64_t tiles = (int64_t)p->batch * p->channels * (p->height / P) * (p->width / P), blocks = (tiles + kBlock - 1) / kBlock;
    if (blocks >= ((int64_t)1 << 31)) return DIMSUM_ERR_SHAPE;
    if (P == 2) hipLaunchKernelGGL(fm_plan_blur_kernel<2>, dim3((unsigned)blocks), dim3(kBlock), 0, s, *p);
    else if (P == 4) hipLaunchKernelGGL(fm_plan_blur_kernel<4>, dim3((unsigned)blocks), dim3(kBlock), 0, s, *p);
    else hipLaunchKernelGGL(fm_plan_blur_kernel<8>, dim3((unsigned)blocks), dim3(kBlock), 0, s, *p);
    return launch_status();
}

extern "C" int dimsum_fm_loss_fwd(const dimsum_fm_loss_params_t *p, void *stream) {
    using namespace dimsum;
    if (const int st = check_loss(p, false)) return st;
    hipLaunchKernelGGL(fm_loss_fwd_kernel, dim3(p->batch), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream), *p);
    return launch_status();
}

extern "C" int dimsum_fm_loss_bwd(const dimsum_fm_loss_params_t *p, void *stream) {
    using namespace dimsum;
    if (const int st = check_loss(p, true)) return st;
    int per = 0;
    const int64_t blocks = grid_for(p->n, p->batch, &per);
    if (!blocks) return DIMSUM_ERR_SHAPE;
    hipLaunchKernelGGL(fm_loss_bwd_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream), *p, per);
    return launch_status();
}
