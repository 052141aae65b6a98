// gelu.hip -- bias + GELU(tanh) of the plain (non-gated) MLP as a row pass, forward and backward: the activation between fc1 and fc2 of timm's
// Mlp as the reference's DiT baseline (dimsum/models_dit.py:124) and DiM's use_gated_mlp=False build it. The siblings of the gated passes in
// token_transform.hip: fp32 in, fp32 or the operand image of the active GEMM policy out (split-bf16 pieces, the [hi | lo] pair, scaled fp16),
// so that fc2 (forward) and both gradient GEMMs of fc1 (backward) read what this pass wrote. HBM-bound: 4 + 4 bytes per element in fp32
// (forward), 8 + 4 (backward); the images write 6 / 4 / 2 bytes instead of 4.
#include "common.hpp"

namespace dimsum {
namespace {

// gelu_tanh(a) = 0.5 a (1 + tanh(u)) = a sigmoid(2 u), u = sqrt(2 / pi) (a + 0.044715 a^3): the form of the GEMM epilogues (gemm_nt_kernel.hpp) --
// no 1 + tanh cancellation on the negative side, relative error a few ulp everywhere
constexpr float kC0 = 0.7978845608028654f, kC1 = 0.044715f;
__device__ __forceinline__ float gelu_tanh(float x) {
    const float u = kC0 * (x + kC1 * x * x * x);
    return x * fast_rcp(1.0f + fast_exp2(-2.0f * kLog2e * u));
}
// d/da [a s(a)], s = sigmoid(2 u): s + a s (1 - s) 2 u'
__device__ __forceinline__ float gelu_tanh_grad(float x) {
    const float x2 = x * x;
    const float u = kC0 * (x + kC1 * x * x2);
    const float s = fast_rcp(1.0f + fast_exp2(-2.0f * kLog2e * u));
    return s * (1.0f + x * (1.0f - s) * (2.0f * kC0) * (1.0f + 3.0f * kC1 * x2));
}
__device__ __forceinline__ f32x4 add4(const float4 &a, const float4 &b) { return {{a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w}}; }
__device__ __forceinline__ float absmax4(const f32x4 &v) { return fmaxf(fmaxf(fabsf(v.v[0]), fabsf(v.v[1])), fmaxf(fabsf(v.v[2]), fabsf(v.v[3]))); }

// 4 columns c .. c + 3 of row r as fp32 or as a split-bf16 image: kImg 0 = fp32 (rows of H), 1 = three pieces (rows of 3 H; kLeft: [hi | hi | lo],
// else weight order [hi | lo | hi]), 2 = the pair [hi | lo] (rows of 2 H)
template <int kImg, bool kLeft> __device__ __forceinline__ void store4(void *out, int64_t r, int64_t c, int64_t H, const f32x4 &v) {
    if constexpr (kImg == 0) *reinterpret_cast<float4 *>(reinterpret_cast<float *>(out) + r * H + c) = make_float4(v.v[0], v.v[1], v.v[2], v.v[3]);
    else if constexpr (kImg == 1) st_split3<kLeft>(reinterpret_cast<unsigned short *>(out) + r * 3 * H, c, H, v);
    else st_split_left(reinterpret_cast<unsigned short *>(out) + r * 2 * H, c, H, v, true);
}

// forward: one thread = 4 columns of one row (one 16-byte load), consecutive threads = consecutive 16-byte pieces; 4 independent pieces in flight
// per thread, a grid stride apart (the flat mapping of gated_gelu_fwd_kernel). No LDS.
template <int kImg>
__global__ __launch_bounds__(256) void gelu_fwd_kernel(const float *x, const float *bias, void *out, int64_t rows, int64_t H) {
    const int64_t q = H / 4, total = rows * q;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x; i0 < total; i0 += 4 * stride) {
        float4 a[4];
        int64_t rr[4], cc[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = min(i0 + k * stride, total - 1);
            rr[k] = i / q; cc[k] = (i - rr[k] * q) * 4;
            a[k] = *reinterpret_cast<const float4 *>(x + rr[k] * H + cc[k]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k * stride >= total) break;
            const float4 b = bias ? *reinterpret_cast<const float4 *>(bias + cc[k]) : make_float4(0.f, 0.f, 0.f, 0.f);
            const f32x4 v = add4(a[k], b);
            store4<kImg, true>(out, rr[k], cc[k], H, f32x4{{gelu_tanh(v.v[0]), gelu_tanh(v.v[1]), gelu_tanh(v.v[2]), gelu_tanh(v.v[3])}});
        }
    }
}

// the maximum over the workgroup's four waves through a two-slot LDS buffer (slot = row parity: the next row's maxima are written while slow
// waves still read this row's); every thread of the workgroup must call it for the same rows
__device__ __forceinline__ float block_allmax(float m, float (*red)[4], int par) {
    m = wave_allmax(m);
    if ((threadIdx.x & 63) == 0) red[par][threadIdx.x >> 6] = m;
    __syncthreads();
    return fmaxf(fmaxf(red[par][0], red[par][1]), fmaxf(red[par][2], red[par][3]));
}

// forward with h as a scaled-fp16 operand image (common.hpp, f16s): rows of H fp16 = fp16(h_r 2^s_r), inv[r] = 2^-s_r. A row's maximum needs the
// whole row: one workgroup walks rows_per_wg rows, a thread holding its 4-column pieces (kStrips x 1024 columns) in registers between the
// maximum and the store (the shape of gated_gelu_bwd_f16s_kernel). row_inv / bound: the bound-derived scale of the GEMM's GELU_F16 epilogue
// instead -- no reduction, the LDS is not touched.
template <int kStrips>
__global__ __launch_bounds__(256) void gelu_fwd_f16s_kernel(const float *x, const float *bias, __half *img, float *inv, const float *row_inv,
                                                            const float *bound, int64_t rows, int64_t H, int rows_per_wg) {
    __shared__ float red[2][4];
    float4 b[kStrips];
#pragma unroll
    for (int s = 0; s < kStrips; ++s) {
        const int64_t c = ((int64_t)s * 256 + threadIdx.x) * 4;
        b[s] = (bias && c < H) ? *reinterpret_cast<const float4 *>(bias + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const float wl1 = row_inv ? bound[0] : 0.f, bmax = row_inv ? bound[1] : 0.f;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_wg, r1 = min(rows, r0 + rows_per_wg);
    for (int64_t r = r0; r < r1; ++r) {
        f32x4 h[kStrips];
        float m = 0.f;
#pragma unroll
        for (int s = 0; s < kStrips; ++s) {
            const int64_t c = ((int64_t)s * 256 + threadIdx.x) * 4;
            h[s] = f32x4{{0.f, 0.f, 0.f, 0.f}};
            if (c < H) {
                const f32x4 v = add4(*reinterpret_cast<const float4 *>(x + r * H + c), b[s]);
                h[s] = f32x4{{gelu_tanh(v.v[0]), gelu_tanh(v.v[1]), gelu_tanh(v.v[2]), gelu_tanh(v.v[3])}};
                m = fmaxf(m, absmax4(h[s]));
            }
        }
        if (row_inv) m = 2.0f * (32768.0f * row_inv[r] * wl1 + bmax);        // (kernel argument: uniform over the workgroup)
        else m = block_allmax(m, red, (int)(r & 1));
        float scale, iv;
        f16s_scales(m, scale, iv);
        if (threadIdx.x == 0) inv[r] = iv;
#pragma unroll
        for (int s = 0; s < kStrips; ++s) {
            const int64_t c = ((int64_t)s * 256 + threadIdx.x) * 4;
            if (c < H) *reinterpret_cast<uint2 *>(img + r * H + c) = f16s_pack4(h[s], scale);
        }
    }
}

// backward: one workgroup = a strip of 1024 columns (4 per thread, 16 B) x a chunk of kRows rows: bias in registers, fully coalesced rows, the
// column sums of dx (= d bias) accumulate in registers: one atomic per column per workgroup (gated_gelu_bwd_kernel's shape)
constexpr int kRows = 64;
template <int kImg>
__global__ __launch_bounds__(256) void gelu_bwd_kernel(const float *x, const float *bias, const float *dh, void *dx, float *dbias, int64_t rows, int64_t H) {
    const int64_t c = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (c >= H) return;
    const float4 b = bias ? *reinterpret_cast<const float4 *>(bias + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    f32x4 sum = {{0.f, 0.f, 0.f, 0.f}};
    const int64_t r0 = (int64_t)blockIdx.y * kRows, r1 = min(rows, r0 + kRows);
    for (int64_t r = r0; r < r1; ++r) {
        const f32x4 a = add4(*reinterpret_cast<const float4 *>(x + r * H + c), b);
        const float4 d = *reinterpret_cast<const float4 *>(dh + r * H + c);
        const f32x4 g = {{d.x * gelu_tanh_grad(a.v[0]), d.y * gelu_tanh_grad(a.v[1]), d.z * gelu_tanh_grad(a.v[2]), d.w * gelu_tanh_grad(a.v[3])}};
        store4<kImg, false>(dx, r, c, H, g);
#pragma unroll
        for (int e = 0; e < 4; ++e) sum.v[e] += g.v[e];
    }
    if (dbias) {
#pragma unroll
        for (int e = 0; e < 4; ++e) atomicAdd(dbias + c + e, sum.v[e]);
    }
}

// the same adjoint with dx as a scaled-fp16 operand image with the exact row maximum's power of two: the operand of BOTH backward GEMMs of fc1
// under the scaled-fp16 policy (gated_gelu_bwd_f16s_kernel's shape: a workgroup walks rows_per_wg rows, the column sums stay in registers)
template <int kStrips>
__global__ __launch_bounds__(256) void gelu_bwd_f16s_kernel(const float *x, const float *bias, const float *dh, __half *img, float *inv, float *dbias,
                                                            int64_t rows, int64_t H, int rows_per_wg) {
    __shared__ float red[2][4];
    float4 b[kStrips];
    f32x4 sum[kStrips];
#pragma unroll
    for (int s = 0; s < kStrips; ++s) {
        const int64_t c = ((int64_t)s * 256 + threadIdx.x) * 4;
        sum[s] = f32x4{{0.f, 0.f, 0.f, 0.f}};
        b[s] = (bias && c < H) ? *reinterpret_cast<const float4 *>(bias + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_wg, r1 = min(rows, r0 + rows_per_wg);
    for (int64_t r = r0; r < r1; ++r) {
        f32x4 g[kStrips];
        float m = 0.f;
#pragma unroll
        for (int s = 0; s < kStrips; ++s) {
            const int64_t c = ((int64_t)s * 256 + threadIdx.x) * 4;
            g[s] = f32x4{{0.f, 0.f, 0.f, 0.f}};
            if (c < H) {
                const f32x4 a = add4(*reinterpret_cast<const float4 *>(x + r * H + c), b[s]);
                const float4 d = *reinterpret_cast<const float4 *>(dh + r * H + c);
                g[s] = f32x4{{d.x * gelu_tanh_grad(a.v[0]), d.y * gelu_tanh_grad(a.v[1]), d.z * gelu_tanh_grad(a.v[2]), d.w * gelu_tanh_grad(a.v[3])}};
                m = fmaxf(m, absmax4(g[s]));
#pragma unroll
                for (int e = 0; e < 4; ++e) sum[s].v[e] += g[s].v[e];
            }
        }
        m = block_allmax(m, red, (int)(r & 1));
        float scale, iv;
        f16s_scales(m, scale, iv);
        if (threadIdx.x == 0) inv[r] = iv;
#pragma unroll
        for (int s = 0; s < kStrips; ++s) {
            const int64_t c = ((int64_t)s * 256 + threadIdx.x) * 4;
            if (c < H) *reinterpret_cast<uint2 *>(img + r * H + c) = f16s_pack4(g[s], scale);
        }
    }
    if (dbias) {
#pragma unroll
        for (int s = 0; s < kStrips; ++s) {
            const int64_t c = ((int64_t)s * 256 + threadIdx.x) * 4;
            if (c < H) {
#pragma unroll
                for (int e = 0; e < 4; ++e) atomicAdd(dbias + c + e, sum[s].v[e]);
            }
        }
    }
}

constexpr int64_t kF16sMaxHidden = 5 * 1024;      // five 1024-column strips of registers per thread

// what both entry points check: the struct sizes, the pointers every mode needs, shapes, alignment
int gelu_params_ok(const dimsum_gelu_params_t *p, dimsum_gelu_ext_t &e, bool bwd) {
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_gelu_params_t)) return DIMSUM_ERR_ABI;
    if (const int rc = ext_from<dimsum_gelu_ext_t>(p->ext, e)) return rc;
    if (!p->x_ptr || !p->out_ptr || (bwd && !p->dh_ptr)) return DIMSUM_ERR_NULL;
    if (p->out_image < DIMSUM_GELU_OUT_F32 || p->out_image > DIMSUM_GELU_OUT_F16S) return DIMSUM_ERR_UNSUPPORTED;
    const bool f16s = p->out_image == DIMSUM_GELU_OUT_F16S;
    if (f16s && !p->inv_scale_ptr) return DIMSUM_ERR_NULL;
    if ((e.row_inv_ptr == nullptr) != (e.bound_ptr == nullptr)) return DIMSUM_ERR_NULL;
    if (e.row_inv_ptr && (bwd || !f16s)) return DIMSUM_ERR_UNSUPPORTED;
    if (p->rows < 0 || p->hidden <= 0 || p->hidden % 4 != 0 || (f16s && p->hidden > kF16sMaxHidden)) return DIMSUM_ERR_SHAPE;
    if (!aligned_to<char>(p->x_ptr, 16) || !aligned_to<char>(p->out_ptr, p->out_image == DIMSUM_GELU_OUT_F32 ? 16 : 8) ||
        (p->bias_ptr && !aligned_to<char>(p->bias_ptr, 16)) || (bwd && !aligned_to<char>(p->dh_ptr, 16)) ||
        (f16s && !aligned_to<char>(p->inv_scale_ptr, 4)) || (p->dbias_ptr && !aligned_to<char>(p->dbias_ptr, 4)) ||
        (e.row_inv_ptr && (!aligned_to<char>(e.row_inv_ptr, 4) || !aligned_to<char>(e.bound_ptr, 4))))
        return DIMSUM_ERR_STRIDE;
    return DIMSUM_OK;
}

// rows per workgroup of the row-walking (f16s) kernels: ONE round of 512 workgroups whatever the row count, 8 rows at least (the measured choice
// of dimsum_gated_gelu_bwd_f16s, token_transform.hip)
inline int rows_per_wg(int64_t rows) {
    const int64_t rpw = (rows + 511) / 512;
    return (int)(rpw < 8 ? 8 : rpw);
}

}  // namespace
}  // namespace dimsum

extern "C" int dimsum_gelu_fwd(const dimsum_gelu_params_t *p, void *stream) {
    using namespace dimsum;
    dimsum_gelu_ext_t e;
    if (const int rc = gelu_params_ok(p, e, false)) return rc;
    if (p->rows == 0) return DIMSUM_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const float *x = reinterpret_cast<const float *>(p->x_ptr), *bias = reinterpret_cast<const float *>(p->bias_ptr);
    if (p->out_image == DIMSUM_GELU_OUT_F16S) {
        const int rpw = rows_per_wg(p->rows);
        const dim3 grid((unsigned)((p->rows + rpw - 1) / rpw));
#define DIMSUM_GF(K) hipLaunchKernelGGL(gelu_fwd_f16s_kernel<K>, grid, dim3(256), 0, s, x, bias, reinterpret_cast<__half *>(p->out_ptr),                 \
                                        reinterpret_cast<float *>(p->inv_scale_ptr), reinterpret_cast<const float *>(e.row_inv_ptr),                     \
                                        reinterpret_cast<const float *>(e.bound_ptr), p->rows, p->hidden, rpw)
        switch ((int)((p->hidden + 1023) / 1024)) {
            case 1: DIMSUM_GF(1); break;
            case 2: DIMSUM_GF(2); break;
            case 3: DIMSUM_GF(3); break;
            case 4: DIMSUM_GF(4); break;
            default: DIMSUM_GF(5); break;
        }
#undef DIMSUM_GF
        return launch_status();
    }
    const int64_t total = p->rows * (p->hidden / 4);
    const int64_t blocks = (total + 256 * 4 - 1) / (256 * 4);
    if (blocks > 0x7fffffff) return DIMSUM_ERR_SHAPE;
    const dim3 grid((unsigned)blocks);
    switch (p->out_image) {
        case DIMSUM_GELU_OUT_F32: hipLaunchKernelGGL(gelu_fwd_kernel<0>, grid, dim3(256), 0, s, x, bias, p->out_ptr, p->rows, p->hidden); break;
        case DIMSUM_GELU_OUT_SPLIT3: hipLaunchKernelGGL(gelu_fwd_kernel<1>, grid, dim3(256), 0, s, x, bias, p->out_ptr, p->rows, p->hidden); break;
        default: hipLaunchKernelGGL(gelu_fwd_kernel<2>, grid, dim3(256), 0, s, x, bias, p->out_ptr, p->rows, p->hidden); break;
    }
    return launch_status();
}

extern "C" int dimsum_gelu_bwd(const dimsum_gelu_params_t *p, void *stream) {
    using namespace dimsum;
    dimsum_gelu_ext_t e;
    if (const int rc = gelu_params_ok(p, e, true)) return rc;
    if (p->rows == 0) return DIMSUM_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const float *x = reinterpret_cast<const float *>(p->x_ptr), *bias = reinterpret_cast<const float *>(p->bias_ptr);
    const float *dh = reinterpret_cast<const float *>(p->dh_ptr);
    float *dbias = reinterpret_cast<float *>(p->dbias_ptr);
    if (p->out_image == DIMSUM_GELU_OUT_F16S) {
        const int rpw = rows_per_wg(p->rows);
        const dim3 grid((unsigned)((p->rows + rpw - 1) / rpw));
#define DIMSUM_GB(K) hipLaunchKernelGGL(gelu_bwd_f16s_kernel<K>, grid, dim3(256), 0, s, x, bias, dh, reinterpret_cast<__half *>(p->out_ptr),             \
                                        reinterpret_cast<float *>(p->inv_scale_ptr), dbias, p->rows, p->hidden, rpw)
        switch ((int)((p->hidden + 1023) / 1024)) {
            case 1: DIMSUM_GB(1); break;
            case 2: DIMSUM_GB(2); break;
            case 3: DIMSUM_GB(3); break;
            case 4: DIMSUM_GB(4); break;
            default: DIMSUM_GB(5); break;
        }
#undef DIMSUM_GB
        return launch_status();
    }
    const int64_t chunks = (p->rows + kRows - 1) / kRows;
    if (chunks > 65535) return DIMSUM_ERR_SHAPE;           // (grid.y: 4 M rows)
    const dim3 grid((unsigned)((p->hidden / 4 + 255) / 256), (unsigned)chunks);
    switch (p->out_image) {
        case DIMSUM_GELU_OUT_F32: hipLaunchKernelGGL(gelu_bwd_kernel<0>, grid, dim3(256), 0, s, x, bias, dh, p->out_ptr, dbias, p->rows, p->hidden); break;
        case DIMSUM_GELU_OUT_SPLIT3: hipLaunchKernelGGL(gelu_bwd_kernel<1>, grid, dim3(256), 0, s, x, bias, dh, p->out_ptr, dbias, p->rows, p->hidden); break;
        default: hipLaunchKernelGGL(gelu_bwd_kernel<2>, grid, dim3(256), 0, s, x, bias, dh, p->out_ptr, dbias, p->rows, p->hidden); break;
    }
    return launch_status();
}
