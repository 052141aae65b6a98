// act_rows.hip -- "bias + GELU between two GEMMs" as a row pass, forward and backward, for the three MLPs of the model families:
//   GatedMLP (dimsum/mlp.py:66-70)              h = gelu_tanh(x1 + b1) (x2 + b2)           dimsum_gated_gelu_fwd / _bwd and their image variants
//   timm's Mlp (dimsum/models_dit.py:124; DiM's use_gated_mlp=False)   h = gelu_tanh(x + b)   dimsum_gelu_fwd / _bwd
//   the experts of SwitchMLP (dimsum/mlp.py:30-38)   gelu_erf, gated or not, the bias row picked by the row's expert   dimsum_moe_act_fwd / _bwd
// fp32 in; fp32 or the operand image of the active GEMM policy out (split-bf16 pieces, the [hi | lo] pair, scaled fp16), so that the next GEMM
// (forward) and both gradient GEMMs of the previous one (backward) read what the pass wrote. HBM-bound: plain 4 + 4 bytes per element in fp32
// (forward), 8 + 4 (backward); the images write 6 / 4 / 2 bytes instead of 4.
// Three loop structures (act_fwd_kernel, act_bwd_kernel, act_f16s_kernel) x an activation policy x gated or not x the output image.
#include "common.hpp"

namespace dimsum {
namespace {

// ---- activation policies: f(a) and df(a) = f'(a) --------------------------------------------------------------------------------------------
// The two tanh forms are the same function on paper and NOT the same bits; merging them changes results, and each is pinned:
//   GeluTanh    -- GatedMLP: 0.5 a (1 + tanh u), what the gated row pass has computed since the goldens and the recorded training runs were made
//   GeluSigmoid -- Mlp / DiT: a sigmoid(2 u), the expression of the GEMM epilogues (gemm_nt_kernel.hpp, gelu_tanh_f): no 1 + tanh cancellation on
//                  the negative side, relative error a few ulp everywhere; the image of gelu_fwd(scales=...) must match the GELU_F16 epilogue's
//                  bit for bit
//   GeluErf     -- the experts: the exact GELU and its derivative Phi(a) + a phi(a)
// u = sqrt(2 / pi) (a + 0.044715 a^3)
constexpr float kC0 = 0.7978845608028654f, kC1 = 0.044715f;
__device__ __forceinline__ float tanh_fast(float x) {           // tanh(x) = 1 - 2 / (exp(2x) + 1)
    return 1.0f - 2.0f * fast_rcp(fast_exp(2.0f * x) + 1.0f);
}
struct GeluTanh {
    static __device__ __forceinline__ float f(float a) {
        const float u = kC0 * (a + kC1 * a * a * a);
        return 0.5f * a * (1.0f + tanh_fast(u));
    }
    static __device__ __forceinline__ float df(float a) {
        const float u = kC0 * (a + kC1 * a * a * a);
        const float t = tanh_fast(u);
        return 0.5f * (1.0f + t) + 0.5f * a * (1.0f - t * t) * kC0 * (1.0f + 3.0f * kC1 * a * a);
    }
};
struct GeluSigmoid {
    static __device__ __forceinline__ float f(float x) {
        const float u = kC0 * (x + kC1 * x * x * x);
        return x * fast_rcp(1.0f + fast_exp2(-2.0f * kLog2e * u));
    }
    static __device__ __forceinline__ float df(float x) {        // d/da [a s(a)], s = sigmoid(2 u): s + a s (1 - s) 2 u'
        const float x2 = x * x;
        const float u = kC0 * (x + kC1 * x * x2);
        const float s = fast_rcp(1.0f + fast_exp2(-2.0f * kLog2e * u));
        return s * (1.0f + x * (1.0f - s) * (2.0f * kC0) * (1.0f + 3.0f * kC1 * x2));
    }
};
struct GeluErf {
    static __device__ __forceinline__ float f(float a) { return 0.5f * a * (1.0f + erff(a * 0.7071067811865476f)); }
    static __device__ __forceinline__ float df(float a) {
        return 0.5f * (1.0f + erff(a * 0.7071067811865476f)) + a * 0.3989422804014327f * expf(-0.5f * a * a);
    }
};

__device__ __forceinline__ f32x4 add4(const float4 &a, const float4 &b) { return {{a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w}}; }
__device__ __forceinline__ float absmax4(const f32x4 &v) { return fmaxf(fmaxf(fabsf(v.v[0]), fabsf(v.v[1])), fmaxf(fabsf(v.v[2]), fabsf(v.v[3]))); }
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// the value and, for a backward pass, the adjoint of 4 columns: a = x1 + b1 (or x + b), g = x2 + b2 (gated), d = dh.
// forward: o = f(a) [g];  backward: da = d [g] f'(a), dg = d f(a) (gated)
template <class Act, bool kGated> __device__ __forceinline__ f32x4 act_value(const f32x4 &a, const f32x4 &g) {
    f32x4 o = {{Act::f(a.v[0]), Act::f(a.v[1]), Act::f(a.v[2]), Act::f(a.v[3])}};
    if constexpr (kGated) {
#pragma unroll
        for (int e = 0; e < 4; ++e) o.v[e] = o.v[e] * g.v[e];
    }
    return o;
}
template <class Act, bool kGated> __device__ __forceinline__ void act_adjoint(const f32x4 &a, const f32x4 &g, const float4 &d4, f32x4 &da, f32x4 &dg) {
    const float d[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if constexpr (kGated) { da.v[e] = d[e] * g.v[e] * Act::df(a.v[e]); dg.v[e] = d[e] * Act::f(a.v[e]); }
        else da.v[e] = d[e] * Act::df(a.v[e]);
    }
}

// ---- the output writer: 4 columns c .. c + 3 of row r of an output of logical row width N (the gated backward writes its two halves as columns
// c and W + c of a row of 2 W). kImg: fp32 (rows of N), three split-bf16 pieces (rows of 3 N; kLeft: [hi | hi | lo], else weight order
// [hi | lo | hi]), the pair [hi | lo] (rows of 2 N)
enum { kImgF32 = 0, kImgSplit3 = 1, kImgPair = 2 };
template <int kImg, bool kLeft> __device__ __forceinline__ void store4(void *out, int64_t r, int64_t c, int64_t N, const f32x4 &v) {
    if constexpr (kImg == kImgF32) stf4(reinterpret_cast<float *>(out) + r * N + c, make_float4(v.v[0], v.v[1], v.v[2], v.v[3]));
    else if constexpr (kImg == kImgSplit3) st_split3<kLeft>(reinterpret_cast<unsigned short *>(out) + r * 3 * N, c, N, v);
    else st_split_left(reinterpret_cast<unsigned short *>(out) + r * 2 * N, c, N, v, true);
}

// ---- 1. flat forward: x (rows, kGated ? 2 W : W) -> out (rows, W). One thread = 4 columns of one row (one 16-byte load per half), consecutive
// threads = consecutive 16-byte pieces; 4 independent pieces in flight per thread, a grid stride apart. No row loop, no LDS.
// kPerExpert: bias is a table (E, S) and row_expert (or NULL: row 0) picks the row's line of it.
template <class Act, bool kGated, int kImg, bool kPerExpert>
__global__ __launch_bounds__(256) void act_fwd_kernel(const float *x, const float *bias, const int *row_expert, void *out, int64_t rows, int64_t W) {
    const int64_t q = W / 4, total = rows * q, S = kGated ? 2 * W : W;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x; i0 < total; i0 += 4 * stride) {
        float4 a[4], g[4];
        int64_t rr[4], cc[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = min(i0 + k * stride, total - 1);
            rr[k] = i / q; cc[k] = (i - rr[k] * q) * 4;
            a[k] = ldf4(x + rr[k] * S + cc[k]);
            if constexpr (kGated) g[k] = ldf4(x + rr[k] * S + W + cc[k]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k * stride >= total) break;
            const float *br = bias;
            if constexpr (kPerExpert) br = bias ? bias + (row_expert ? (int64_t)row_expert[rr[k]] : 0) * S : nullptr;
            const f32x4 av = add4(a[k], br ? ldf4(br + cc[k]) : zero4());
            f32x4 gv = {};
            if constexpr (kGated) gv = add4(g[k], br ? ldf4(br + W + cc[k]) : zero4());
            store4<kImg, true>(out, rr[k], cc[k], W, act_value<Act, kGated>(av, gv));
        }
    }
}

// ---- 2. strip x row-chunk backward: one workgroup = a strip of 1024 columns (4 per thread, 16 B) x a chunk of kChunkRows rows: bias in
// registers, fully coalesced rows, the column sums of dx (= d bias) accumulate in registers: one atomic per column per workgroup.
// kPerExpert: the sums stay in registers while the rows' expert stays the same: flushed at an expert boundary and at the end of the chunk.
constexpr int kChunkRows = 64;
template <class Act, bool kGated, int kImg, bool kPerExpert>
__global__ __launch_bounds__(256) void act_bwd_kernel(const float *x, const float *bias, const int *row_expert, const float *dh, void *dx,
                                                      float *dbias, int64_t rows, int64_t W) {
    const int64_t c = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (c >= W) return;
    const int64_t S = kGated ? 2 * W : W;
    const int64_t r0 = (int64_t)blockIdx.y * kChunkRows, r1 = min(rows, r0 + kChunkRows);
    int cur = kPerExpert ? -1 : 0;
    float4 ba = zero4(), bg = zero4();
    f32x4 sa = {}, sg = {};
    auto load_bias = [&]() {
        if (bias) { ba = ldf4(bias + cur * S + c); if constexpr (kGated) bg = ldf4(bias + cur * S + W + c); }
    };
    auto flush = [&]() {
        if (dbias && cur >= 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                atomicAdd(dbias + cur * S + c + e, sa.v[e]);
                if constexpr (kGated) atomicAdd(dbias + cur * S + W + c + e, sg.v[e]);
            }
        }
        sa = f32x4{}; sg = f32x4{};
    };
    if constexpr (!kPerExpert) load_bias();
    for (int64_t r = r0; r < r1; ++r) {
        if constexpr (kPerExpert) {
            const int ex = row_expert ? row_expert[r] : 0;       // (uniform over the workgroup)
            if (ex != cur) { flush(); cur = ex; load_bias(); }
        }
        const f32x4 a = add4(ldf4(x + r * S + c), ba);
        f32x4 g = {}, da, dg;
        if constexpr (kGated) g = add4(ldf4(x + r * S + W + c), bg);
        act_adjoint<Act, kGated>(a, g, ldf4(dh + r * W + c), da, dg);
        store4<kImg, false>(dx, r, c, S, da);
        if constexpr (kGated) store4<kImg, false>(dx, r, W + c, S, dg);
#pragma unroll
        for (int e = 0; e < 4; ++e) { sa.v[e] += da.v[e]; if constexpr (kGated) sg.v[e] += dg.v[e]; }
    }
    flush();
}

// the maximum over the workgroup's four waves through a two-slot LDS buffer (slot = row parity: the next row's maxima are written while slow
// waves still read this row's); every thread of the workgroup must call it for the same rows
__device__ __forceinline__ float block_allmax(float m, float (*red)[4], int par) {
    m = wave_allmax(m);
    if ((threadIdx.x & 63) == 0) red[par][threadIdx.x >> 6] = m;
    __syncthreads();
    return fmaxf(fmaxf(red[par][0], red[par][1]), fmaxf(red[par][2], red[par][3]));
}

// ---- 3. row-walking pass with the result as a scaled-fp16 operand image (common.hpp, f16s): rows of S fp16 = fp16(v_r 2^s_r) with the exact row
// maximum's power of two, inv[r] = 2^-s_r. Forward (kBwd = false): v = h, the left operand of the next GEMM. Backward: v = dx, the operand of
// BOTH backward GEMMs of the previous one under the scaled-fp16 policy (d input as an NT product, d weight as a TN product with per-reduction-row
// factors, dimsum_gemm_ext_t.k_scale_ptr). A row's maximum needs the whole row: one workgroup walks rows_per_wg rows, a thread holding its
// 4-column pieces (kStrips x 1024 columns, both halves if gated) in registers between the maximum and the store; the column sums (d bias)
// accumulate in registers across the rows. row_inv / bound (forward only): the bound-derived scale of the GEMM's GELU_F16 epilogue instead -- no
// reduction, the LDS is not touched.
// kPerExpert (forward only): bias is a table (E, S) and row_expert (or NULL: row 0) picks the row's line of it; the registers are reloaded where the
// expert changes (the rows are sorted by expert: at most E - 1 times over the whole pass).
template <class Act, bool kGated, bool kBwd, int kStrips, bool kPerExpert = false>
__global__ __launch_bounds__(256) void act_f16s_kernel(const float *x, const float *bias, const float *dh, __half *img, float *inv, float *dbias,
                                                       const float *row_inv, const float *bound, int64_t rows, int64_t W, int rows_per_wg,
                                                       const int *row_expert = nullptr) {
    __shared__ float red[2][4];
    const int64_t S = kGated ? 2 * W : W;
    float4 ba[kStrips], bg[kStrips];
    f32x4 sa[kStrips], sg[kStrips];
#pragma unroll
    for (int s = 0; s < kStrips; ++s) {
        const int64_t c = ((int64_t)s * 256 + threadIdx.x) * 4;
        ba[s] = bg[s] = zero4();
        sa[s] = sg[s] = f32x4{};
        if (!kPerExpert && bias && c < W) { ba[s] = ldf4(bias + c); if constexpr (kGated) bg[s] = ldf4(bias + W + c); }
    }
    int cur = -1;                                 // kPerExpert: the expert whose bias row the registers hold
    const float wl1 = (!kBwd && row_inv) ? bound[0] : 0.f, bmax = (!kBwd && row_inv) ? bound[1] : 0.f;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_wg, r1 = min(rows, r0 + rows_per_wg);
    for (int64_t r = r0; r < r1; ++r) {
        if constexpr (kPerExpert) {
            const int ex = row_expert ? row_expert[r] : 0;       // (uniform over the workgroup)
            if (bias && ex != cur) {
                cur = ex;
#pragma unroll
                for (int s = 0; s < kStrips; ++s) {
                    const int64_t c = ((int64_t)s * 256 + threadIdx.x) * 4;
                    if (c < W) { ba[s] = ldf4(bias + cur * S + c); if constexpr (kGated) bg[s] = ldf4(bias + cur * S + W + c); }
                }
            }
        }
        f32x4 va[kStrips], vg[kStrips];          // h (forward); da, dg (backward)
        float m = 0.f;
#pragma unroll
        for (int s = 0; s < kStrips; ++s) {
            const int64_t c = ((int64_t)s * 256 + threadIdx.x) * 4;
            va[s] = vg[s] = f32x4{};
            if (c < W) {
                const f32x4 a = add4(ldf4(x + r * S + c), ba[s]);
                f32x4 g = {};
                if constexpr (kGated) g = add4(ldf4(x + r * S + W + c), bg[s]);
                if constexpr (kBwd) {
                    act_adjoint<Act, kGated>(a, g, ldf4(dh + r * W + c), va[s], vg[s]);
                    m = fmaxf(m, kGated ? fmaxf(absmax4(va[s]), absmax4(vg[s])) : absmax4(va[s]));
#pragma unroll
                    for (int e = 0; e < 4; ++e) { sa[s].v[e] += va[s].v[e]; if constexpr (kGated) sg[s].v[e] += vg[s].v[e]; }
                } else {
                    va[s] = act_value<Act, kGated>(a, g);
                    m = fmaxf(m, absmax4(va[s]));
                }
            }
        }
        if (!kBwd && row_inv) m = 2.0f * (32768.0f * row_inv[r] * wl1 + bmax);        // (kernel argument: uniform over the workgroup)
        else m = block_allmax(m, red, (int)(r & 1));
        float scale, iv;
        f16s_scales(m, scale, iv);
        if (threadIdx.x == 0) inv[r] = iv;
        __half *row = img + r * (kBwd ? S : W);
#pragma unroll
        for (int s = 0; s < kStrips; ++s) {
            const int64_t c = ((int64_t)s * 256 + threadIdx.x) * 4;
            if (c < W) {
                *reinterpret_cast<uint2 *>(row + c) = f16s_pack4(va[s], scale);
                if constexpr (kBwd && kGated) *reinterpret_cast<uint2 *>(row + W + c) = f16s_pack4(vg[s], scale);
            }
        }
    }
    if (kBwd && dbias) {
#pragma unroll
        for (int s = 0; s < kStrips; ++s) {
            const int64_t c = ((int64_t)s * 256 + threadIdx.x) * 4;
            if (c < W) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    atomicAdd(dbias + c + e, sa[s].v[e]);
                    if constexpr (kGated) atomicAdd(dbias + W + c + e, sg[s].v[e]);
                }
            }
        }
    }
}

// ---- host side: one launcher per loop structure --------------------------------------------------------------------------------------------
inline const float *f32p(const void *p) { return reinterpret_cast<const float *>(p); }
inline bool al16(const void *p) { return aligned_to<char>(p, 16); }
inline bool al4(const void *p) { return aligned_to<char>(p, 4); }

// flat mapping: 4 pieces per thread a quarter of the tensor apart, no row loop: 0.60 ms at (65536, 2 x 4096) against 0.67 ms for the
// strip-per-workgroup form the backward keeps (it needs the row loop for the d bias column sums)
template <class Act, bool kGated, int kImg, bool kPerExpert>
int launch_fwd(const void *x, const void *bias, const void *row_expert, void *out, int64_t rows, int64_t W, void *stream) {
    dim3 grid;
    if (!flat_grid(rows * (W / 4), grid)) return DIMSUM_ERR_SHAPE;
    hipLaunchKernelGGL((act_fwd_kernel<Act, kGated, kImg, kPerExpert>), grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), f32p(x), f32p(bias),
                       reinterpret_cast<const int *>(row_expert), out, rows, W);
    return launch_status();
}

template <class Act, bool kGated, int kImg, bool kPerExpert>
int launch_bwd(const void *x, const void *bias, const void *row_expert, const void *dh, void *dx, void *dbias, int64_t rows, int64_t W, void *stream) {
    const int64_t chunks = (rows + kChunkRows - 1) / kChunkRows;
    if (chunks > 65535) return DIMSUM_ERR_SHAPE;           // (grid.y: 4 M rows)
    const dim3 grid((unsigned)((W / 4 + 255) / 256), (unsigned)chunks);
    hipLaunchKernelGGL((act_bwd_kernel<Act, kGated, kImg, kPerExpert>), grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), f32p(x), f32p(bias),
                       reinterpret_cast<const int *>(row_expert), f32p(dh), dx, reinterpret_cast<float *>(dbias), rows, W);
    return launch_status();
}

constexpr int64_t kF16sMaxHidden = 5 * 1024;      // five 1024-column strips of registers per thread

template <class Act, bool kGated, bool kBwd, bool kPerExpert = false>
int launch_f16s(const void *x, const void *bias, const void *dh, void *img, void *inv, void *dbias, const void *row_inv, const void *bound,
                int64_t rows, int64_t W, void *stream, const void *row_expert = nullptr) {
    // rows per workgroup: ONE round of 512 workgroups (two per CU; three fit), whatever the batch size, 8 rows at least. Measured on the gated
    // backward (tools/scratch/gg_bwd_time.py, rows per workgroup = rows / div): 16384 rows: 128 workgroups 538 us, 256: 320, 390-512: 262,
    // 780: 348 (a dozen workgroups left over for a second round run alone for a whole workgroup's duration), 1024: 309, 2048+: 350; 65536 rows:
    // 512 workgroups 862 us, 1024: 937, 2048: 882, 8192: 1117 (the column sums cost one atomic per column and workgroup: 8192 each).
    int rpw = (int)((rows + 511) / 512);
    rpw = rpw < 8 ? 8 : rpw;
    const dim3 grid((unsigned)((rows + rpw - 1) / rpw));
#define DIMSUM_AF(K) hipLaunchKernelGGL((act_f16s_kernel<Act, kGated, kBwd, K, kPerExpert>), grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), \
                                        f32p(x), f32p(bias), f32p(dh), reinterpret_cast<__half *>(img), reinterpret_cast<float *>(inv),                 \
                                        reinterpret_cast<float *>(dbias), f32p(row_inv), f32p(bound), rows, W, rpw,                                     \
                                        reinterpret_cast<const int *>(row_expert))
    switch ((int)((W + 1023) / 1024)) {
        case 1: DIMSUM_AF(1); break;
        case 2: DIMSUM_AF(2); break;
        case 3: DIMSUM_AF(3); break;
        case 4: DIMSUM_AF(4); break;
        default: DIMSUM_AF(5); break;
    }
#undef DIMSUM_AF
    return launch_status();
}

// ---- what the entry points check, in this order ---------------------------------------------------------------------------------------------
int gated_params_ok(const void *x12, const void *bias, const void *dh, const void *out, bool bwd, int64_t rows, int64_t hidden) {
    if (!x12 || !out || (bwd && !dh)) return DIMSUM_ERR_NULL;
    if (rows < 0 || hidden <= 0 || hidden % 4 != 0) return DIMSUM_ERR_SHAPE;
    if (!al16(x12) || !al16(dh) || !al16(out) || !al16(bias)) return DIMSUM_ERR_STRIDE;
    return DIMSUM_OK;
}

// the struct sizes, the pointers every mode needs, shapes, alignment
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
    if (!al16(p->x_ptr) || !aligned_to<char>(p->out_ptr, p->out_image == DIMSUM_GELU_OUT_F32 ? 16 : 8) || !al16(p->bias_ptr) ||
        (bwd && !al16(p->dh_ptr)) || (f16s && !al4(p->inv_scale_ptr)) || !al4(p->dbias_ptr) || !al4(e.row_inv_ptr) || !al4(e.bound_ptr))
        return DIMSUM_ERR_STRIDE;
    return DIMSUM_OK;
}

// struct sizes, then shapes, then -- for a call with rows -- pointers and alignment; an empty call needs no row pointers
int moe_act_params_ok(const dimsum_moe_act_params_t *p, bool bwd) {
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_moe_act_params_t)) return DIMSUM_ERR_ABI;
    dimsum_moe_ext_t e;
    if (const int rc = ext_from<dimsum_moe_ext_t>(p->ext, e)) return rc;
    if (p->rows < 0 || p->width <= 0 || p->width % 4 != 0 || p->num_experts < 1 || p->num_experts > 64) return DIMSUM_ERR_SHAPE;
    if (p->rows == 0) return DIMSUM_OK;
    if (!p->x_ptr || !p->out_ptr || (bwd && !p->dh_ptr) || (p->dbias_ptr && !p->bias_ptr)) return DIMSUM_ERR_NULL;
    if (!p->row_expert_ptr && p->num_experts != 1) return DIMSUM_ERR_NULL;
    if (!al16(p->x_ptr) || !al16(p->out_ptr) || !al16(p->bias_ptr) || !al16(p->dh_ptr) || !al4(p->row_expert_ptr) || !al4(p->dbias_ptr)) return DIMSUM_ERR_STRIDE;
    return DIMSUM_OK;
}

template <int kImg> int gated_fwd(const void *x12, const void *bias, void *h, int64_t rows, int64_t hidden, void *stream) {
    if (const int rc = gated_params_ok(x12, bias, nullptr, h, false, rows, hidden)) return rc;
    if (rows == 0) return DIMSUM_OK;
    return launch_fwd<GeluTanh, true, kImg, false>(x12, bias, nullptr, h, rows, hidden, stream);
}

template <int kImg> int gated_bwd(const void *x12, const void *bias, const void *dh, void *dx12, void *dbias, int64_t rows, int64_t hidden, void *stream) {
    if (const int rc = gated_params_ok(x12, bias, dh, dx12, true, rows, hidden)) return rc;
    if (rows == 0) return DIMSUM_OK;
    return launch_bwd<GeluTanh, true, kImg, false>(x12, bias, nullptr, dh, dx12, dbias, rows, hidden, stream);
}

}  // namespace
}  // namespace dimsum

using namespace dimsum;

extern "C" int dimsum_gated_gelu_fwd(const void *x12, const void *bias, void *h, int64_t rows, int64_t hidden, void *stream) {
    return gated_fwd<kImgF32>(x12, bias, h, rows, hidden, stream);
}

/* h as the split-bf16 left operand image of the w3 GEMM: rows of 3 hidden bf16 [hi | hi | lo] */
extern "C" int dimsum_gated_gelu_fwd_split3(const void *x12, const void *bias, void *h3, int64_t rows, int64_t hidden, void *stream) {
    return gated_fwd<kImgSplit3>(x12, bias, h3, rows, hidden, stream);
}

extern "C" int dimsum_gated_gelu_bwd(const void *x12, const void *bias, const void *dh, void *dx12, void *dbias, int64_t rows,
                                     int64_t hidden, void *stream) {
    return gated_bwd<kImgF32>(x12, bias, dh, dx12, dbias, rows, hidden, stream);
}

/* dx12 as the split-bf16 operand image of the two GEMMs that consume it (d input = dx12 W12, d weight = dx12^T h): rows of 3 x 2 hidden bf16 in
 * WEIGHT order [hi | lo | hi], to be paired with left-order images of W12^T and of h */
extern "C" int dimsum_gated_gelu_bwd_split3(const void *x12, const void *bias, const void *dh, void *dx12_image, void *dbias, int64_t rows,
                                            int64_t hidden, void *stream) {
    return gated_bwd<kImgSplit3>(x12, bias, dh, dx12_image, dbias, rows, hidden, stream);
}

extern "C" int dimsum_gated_gelu_bwd_pair(const void *x12, const void *bias, const void *dh, void *dx12_pair, void *dbias, int64_t rows,
                                          int64_t hidden, void *stream) {
    return gated_bwd<kImgPair>(x12, bias, dh, dx12_pair, dbias, rows, hidden, stream);
}

/* dx12 as the scaled-fp16 image (rows, 2 hidden) float16 + inv_scale (rows) f32 */
extern "C" int dimsum_gated_gelu_bwd_f16s(const void *x12, const void *bias, const void *dh, void *dx12_image, void *inv_scale, void *dbias, int64_t rows,
                                          int64_t hidden, void *stream) {
    if (!x12 || !dh || !dx12_image || !inv_scale) return DIMSUM_ERR_NULL;
    if (rows < 0 || hidden <= 0 || hidden % 4 != 0 || hidden > kF16sMaxHidden) return DIMSUM_ERR_SHAPE;
    if (!al16(x12) || !al16(dh) || !aligned_to<char>(dx12_image, 8) || !al16(bias)) return DIMSUM_ERR_STRIDE;
    if (rows == 0) return DIMSUM_OK;
    return launch_f16s<GeluTanh, true, true>(x12, bias, dh, dx12_image, inv_scale, dbias, nullptr, nullptr, rows, hidden, stream);
}

extern "C" int dimsum_gelu_fwd(const dimsum_gelu_params_t *p, void *stream) {
    dimsum_gelu_ext_t e;
    if (const int rc = gelu_params_ok(p, e, false)) return rc;
    if (p->rows == 0) return DIMSUM_OK;
    switch (p->out_image) {
        case DIMSUM_GELU_OUT_F16S:
            return launch_f16s<GeluSigmoid, false, false>(p->x_ptr, p->bias_ptr, nullptr, p->out_ptr, p->inv_scale_ptr, nullptr, e.row_inv_ptr, e.bound_ptr,
                                                          p->rows, p->hidden, stream);
        case DIMSUM_GELU_OUT_F32: return launch_fwd<GeluSigmoid, false, kImgF32, false>(p->x_ptr, p->bias_ptr, nullptr, p->out_ptr, p->rows, p->hidden, stream);
        case DIMSUM_GELU_OUT_SPLIT3: return launch_fwd<GeluSigmoid, false, kImgSplit3, false>(p->x_ptr, p->bias_ptr, nullptr, p->out_ptr, p->rows, p->hidden, stream);
        default: return launch_fwd<GeluSigmoid, false, kImgPair, false>(p->x_ptr, p->bias_ptr, nullptr, p->out_ptr, p->rows, p->hidden, stream);
    }
}

extern "C" int dimsum_gelu_bwd(const dimsum_gelu_params_t *p, void *stream) {
    dimsum_gelu_ext_t e;
    if (const int rc = gelu_params_ok(p, e, true)) return rc;
    if (p->rows == 0) return DIMSUM_OK;
    switch (p->out_image) {
        case DIMSUM_GELU_OUT_F16S:
            return launch_f16s<GeluSigmoid, false, true>(p->x_ptr, p->bias_ptr, p->dh_ptr, p->out_ptr, p->inv_scale_ptr, p->dbias_ptr, nullptr, nullptr,
                                                         p->rows, p->hidden, stream);
        case DIMSUM_GELU_OUT_F32:
            return launch_bwd<GeluSigmoid, false, kImgF32, false>(p->x_ptr, p->bias_ptr, nullptr, p->dh_ptr, p->out_ptr, p->dbias_ptr, p->rows, p->hidden, stream);
        case DIMSUM_GELU_OUT_SPLIT3:
            return launch_bwd<GeluSigmoid, false, kImgSplit3, false>(p->x_ptr, p->bias_ptr, nullptr, p->dh_ptr, p->out_ptr, p->dbias_ptr, p->rows, p->hidden, stream);
        default:
            return launch_bwd<GeluSigmoid, false, kImgPair, false>(p->x_ptr, p->bias_ptr, nullptr, p->dh_ptr, p->out_ptr, p->dbias_ptr, p->rows, p->hidden, stream);
    }
}

extern "C" int dimsum_moe_act_fwd(const dimsum_moe_act_params_t *p, void *stream) {
    if (const int rc = moe_act_params_ok(p, false)) return rc;
    if (p->rows == 0) return DIMSUM_OK;
    if (p->gated) return launch_fwd<GeluErf, true, kImgF32, true>(p->x_ptr, p->bias_ptr, p->row_expert_ptr, p->out_ptr, p->rows, p->width, stream);
    return launch_fwd<GeluErf, false, kImgF32, true>(p->x_ptr, p->bias_ptr, p->row_expert_ptr, p->out_ptr, p->rows, p->width, stream);
}

/* the experts' activation with h as the scaled-fp16 left operand image of the fc2 grouped GEMM (dimsum_moe_gemm_f16s): exact row maxima */
extern "C" int dimsum_moe_act_fwd_f16s(const dimsum_moe_act_f16s_params_t *p, void *stream) {
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_moe_act_f16s_params_t)) return DIMSUM_ERR_ABI;
    dimsum_moe_ext_t e;
    if (const int rc = ext_from<dimsum_moe_ext_t>(p->ext, e)) return rc;
    if (p->rows < 0 || p->width <= 0 || p->width % 4 != 0 || p->width > kF16sMaxHidden || p->num_experts < 1 || p->num_experts > 64) return DIMSUM_ERR_SHAPE;
    if (p->rows == 0) return DIMSUM_OK;
    if (!p->x_ptr || !p->out_ptr || !p->inv_scale_ptr) return DIMSUM_ERR_NULL;
    if (!p->row_expert_ptr && p->num_experts != 1) return DIMSUM_ERR_NULL;
    if (!al16(p->x_ptr) || !aligned_to<char>(p->out_ptr, 8) || !al16(p->bias_ptr) || !al4(p->row_expert_ptr) || !al4(p->inv_scale_ptr)) return DIMSUM_ERR_STRIDE;
    if (p->gated)
        return launch_f16s<GeluErf, true, false, true>(p->x_ptr, p->bias_ptr, nullptr, p->out_ptr, p->inv_scale_ptr, nullptr, nullptr, nullptr, p->rows,
                                                       p->width, stream, p->row_expert_ptr);
    return launch_f16s<GeluErf, false, false, true>(p->x_ptr, p->bias_ptr, nullptr, p->out_ptr, p->inv_scale_ptr, nullptr, nullptr, nullptr, p->rows,
                                                    p->width, stream, p->row_expert_ptr);
}

extern "C" int dimsum_moe_act_bwd(const dimsum_moe_act_params_t *p, void *stream) {
    if (const int rc = moe_act_params_ok(p, true)) return rc;
    if (p->rows == 0) return DIMSUM_OK;
    if (p->gated)
        return launch_bwd<GeluErf, true, kImgF32, true>(p->x_ptr, p->bias_ptr, p->row_expert_ptr, p->dh_ptr, p->out_ptr, p->dbias_ptr, p->rows, p->width, stream);
    return launch_bwd<GeluErf, false, kImgF32, true>(p->x_ptr, p->bias_ptr, p->row_expert_ptr, p->dh_ptr, p->out_ptr, p->dbias_ptr, p->rows, p->width, stream);
}
