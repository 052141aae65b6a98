// moe_gemm_f16.hip -- the grouped expert GEMM of moe_gemm.hip on scaled-fp16 operand images (common.hpp, f16s): ONE fp16 MFMA product per element
// instead of the three bf16 products of the fp32 kernel, two-byte operand rows from HBM into LDS instead of four-byte ones.
//   out[j, n] = x_inv[j] w_inv_e[n] sum_k x16[j, k] w16_e[n, k] (+ bias[e, n])     for offsets[e] <= j < offsets[e + 1]
// x16 (T, K) fp16 with x_inv (T) is the image a producer pass wrote (dimsum_moe_permute_f16s, dimsum_moe_act_fwd_f16s, dimsum_rows_f16s); the E weight
// images (N, K) fp16 and their (N) inverse scales are separate tensors whose addresses travel BY VALUE in the kernel arguments.
//
//  * what moe_gemm.hip does is kept: the offsets are read ON THE DEVICE, clamped to [0, T] and cut where they overlap an earlier range; the grid is
//    the static bound (ceil(T / kBM) + E) x ceil(N / kBN); a row tile never spans two experts, a short last tile loads its missing rows from its
//    last valid row and stores nothing for them; a tile index past the last real tile leaves at once; rows outside every range are not written.
//    No split-K, no atomics: one fixed summation order per output element, bit-reproducible.
//  * arithmetic: v_mfma_f32_16x16x32_f16 into fp32 accumulators; products of two fp16 values are exact in fp32, so the only rounding is the fp32
//    accumulation. The two power-of-two inverse scales (exact) and the bias are applied in the epilogue.
//  * workgroup = 4 waves = one 64 x 128 output tile (a wave: 32 rows x 64 columns), K tiles 64 deep = two MFMA steps per barrier; two LDS buffers
//    of 24 KB (x: 64 rows, W: 128 rows of 128 bytes). The global loads of tile t + 1 (six 16-byte loads per thread) are issued before the MFMAs of
//    tile t and written into the other buffer after them; one barrier per K tile.
//  * LDS layout: the 16-byte piece p (0..7) of row r sits at piece p ^ ((r >> 1) & 7). A ds_read_b128 of an MFMA operand (lane l: row l & 15, piece
//    4 s + (l >> 4)) is served in four groups of 16 lanes, each holding the 16 rows once, 8 of them at piece p and 8 at piece p ^ 1: rows of one
//    parity share a 128-byte half of the 256-byte bank row and land on 8 distinct slots of it (the sets {0, 1, 6, 7} and {2, 3, 4, 5} of r >> 1 are
//    closed under ^ 1), so every group touches 16 distinct 16-byte slots. A ds_write_b128 group of 8 lanes fills one whole row: 128 contiguous bytes.
//  * the MFMA takes the weight fragment as A and the token fragment as B (D[n][m]): a lane ends with 4 CONSECUTIVE output columns of one row
//    (16-byte stores, bias and weight-scale loads).
#include "common.hpp"

namespace dimsum {
namespace {

constexpr int kBM = DIMSUM_MOE_GEMM_BM, kBN = DIMSUM_MOE_GEMM_BN, kBK = 64;
constexpr int kMaxE = 64;
constexpr int kRowB = kBK * 2;                       // bytes of an LDS row: 64 fp16
constexpr int kXo = 0, kWo = kBM * kRowB, kBuf = kWo + kBN * kRowB;      // 24576

typedef float f4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct moe_gemm_f16_args_t {
    const __half *x;
    const float *x_inv, *bias;
    const int *offsets;
    float *out;
    int64_t T, ldc;
    int K, N, E;
    const __half *w[kMaxE];
    const float *w_inv[kMaxE];
};

__device__ __forceinline__ int lds_off(int r, int p) { return r * kRowB + ((p ^ ((r >> 1) & 7)) << 4); }
__device__ __forceinline__ u32x4 ld16(const __half *p) { return *reinterpret_cast<const u32x4 *>(p); }

__global__ __launch_bounds__(256) void moe_gemm_f16_kernel(const moe_gemm_f16_args_t a) {
    __shared__ __attribute__((aligned(16))) char lds[2 * kBuf];
    // ---- the row tile's expert, first row and row count (every value wave-uniform): moe_gemm.hip's scan, statement for statement
    const int tile = blockIdx.x;
    const int T = (int)a.T;
    int e = 0, before = 0, row0 = 0, cnt = 0, taken = 0;  // taken: the end of the last non-empty range
    for (; e < a.E; ++e) {
        const int o0 = max(min(max(a.offsets[e], 0), T), taken), o1 = min(max(a.offsets[e + 1], 0), T);
        if (o1 <= o0) continue;
        taken = o1;
        const int nt = (o1 - o0 + kBM - 1) / kBM;
        if (tile < before + nt) {
            row0 = o0 + (tile - before) * kBM;
            cnt = min(kBM, o1 - row0);
            break;
        }
        before += nt;
    }
    if (cnt <= 0) return;                                 // past the last real tile

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wm = wv & 1, wn = wv >> 1;                  // the wave's 32 rows x 64 columns of the tile
    const int K = a.K, N = a.N;
    const int n0 = blockIdx.y * kBN;
    const __half *w = a.w[e];

    // staging: thread = (row tid >> 3, 8 k values tid & 7) of both 32-row halves of the token tile and of the four 32-row quarters of the weight
    // tile; rows past the tile's count / past N read the last valid row (their results are never stored)
    const int sr = tid >> 3, sc = tid & 7;
    const __half *xg[2], *wg[4];
#pragma unroll
    for (int i = 0; i < 2; ++i) xg[i] = a.x + (int64_t)(row0 + min(sr + 32 * i, cnt - 1)) * K;
#pragma unroll
    for (int i = 0; i < 4; ++i) wg[i] = w + (int64_t)min(n0 + sr + 32 * i, N - 1) * K;
    const int so = lds_off(sr, sc);                       // (row sr + 32 i: + 32 i rows, the same piece: (32 i >> 1) & 7 == 0)

    u32x4 gx[2], gw[4];
#define DIMSUM_MG_LOAD(KT)                                                                                                    \
    do {                                                                                                                      \
        const int k_ = min((KT) * kBK + sc * 8, K - 8);                                                                       \
        _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_) gx[i_] = ld16(xg[i_] + k_);                                           \
        _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) gw[i_] = ld16(wg[i_] + k_);                                           \
    } while (0)
#define DIMSUM_MG_WRITE(BUF)                                                                                                  \
    do {                                                                                                                      \
        char *b_ = lds + (BUF) * kBuf + so;                                                                                   \
        _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_) *reinterpret_cast<u32x4 *>(b_ + kXo + i_ * 32 * kRowB) = gx[i_];      \
        _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) *reinterpret_cast<u32x4 *>(b_ + kWo + i_ * 32 * kRowB) = gw[i_];      \
    } while (0)

    f4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

    // operand reads: lane l holds row l & 15 of a 16-row fragment, the 8 k values of piece 4 s + (l >> 4) of MFMA step s
    const int fr = lane & 15, fc = lane >> 4;
    int xo[2], wo[2];                                     // (+ 16 rows: + 16 * kRowB, the same piece: (16 >> 1) & 7 == 0)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        xo[s] = kXo + lds_off(wm * 32 + fr, 4 * s + fc);
        wo[s] = kWo + lds_off(wn * 64 + fr, 4 * s + fc);
    }

    // K % 32 == 0: with an odd number of 32-deep steps the last tile is half a tile. Its pieces 4..7 lie past the row's end: those threads load
    // the row's last piece instead (DIMSUM_MG_LOAD clamps the column) and the tile's second MFMA step is skipped
    const int nk = (K + kBK - 1) / kBK;
    const bool half_tail = (K % kBK) != 0;
    DIMSUM_MG_LOAD(0);
    DIMSUM_MG_WRITE(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const bool more = kt + 1 < nk;                    // (uniform)
        if (more) DIMSUM_MG_LOAD(kt + 1);
        const char *b = lds + (kt & 1) * kBuf;
        const int steps = (half_tail && !more) ? 1 : 2;   // (uniform)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (s < steps) {
                f16x8_t xf[2], wf[4];
#pragma unroll
                for (int i = 0; i < 2; ++i) xf[i] = *reinterpret_cast<const f16x8_t *>(b + xo[s] + i * 16 * kRowB);
#pragma unroll
                for (int j = 0; j < 4; ++j) wf[j] = *reinterpret_cast<const f16x8_t *>(b + wo[s] + j * 16 * kRowB);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[j], xf[i], acc[i][j], 0, 0, 0);
            }
        }
        if (more) DIMSUM_MG_WRITE((kt + 1) & 1);          // the buffer every wave finished reading before the previous barrier
        __syncthreads();
    }
#undef DIMSUM_MG_LOAD
#undef DIMSUM_MG_WRITE

    // ---- epilogue: D[n][m] -- the lane's column is token row m = l & 15, its 4 registers are the output columns 4 (l >> 4) .. + 3
    const float *bias = a.bias ? a.bias + (int64_t)e * N : nullptr;
    const float *winv = a.w_inv[e];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = wm * 32 + i * 16 + fr;
        if (m >= cnt) continue;                           // the rows after a short tile belong to the next expert
        const float xi = a.x_inv[row0 + m];
        float *orow = a.out + (int64_t)(row0 + m) * a.ldc;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + wn * 64 + j * 16 + fc * 4;
            if (n >= N) continue;
            const float4 wi = ldf4(winv + n);
            // (acc xi) wi: two exact multiplications by powers of two, whatever the order
            float4 v = make_float4(acc[i][j][0] * xi * wi.x, acc[i][j][1] * xi * wi.y, acc[i][j][2] * xi * wi.z, acc[i][j][3] * xi * wi.w);
            if (bias) {
                const float4 bv = ldf4(bias + n);
                v.x += bv.x; v.y += bv.y; v.z += bv.z; v.w += bv.w;
            }
            stf4(orow + n, v);
        }
    }
}

inline bool al16(const void *p) { return aligned_to<char>(p, 16); }

}  // namespace
}  // namespace dimsum

// (checks: struct sizes, then shapes, then -- for a call with rows -- pointers, then alignment; tokens == 0 needs no pointers and launches nothing)
extern "C" int dimsum_moe_gemm_f16s(const dimsum_moe_gemm_f16s_params_t *p, void *stream) {
    using namespace dimsum;
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_moe_gemm_f16s_params_t)) return DIMSUM_ERR_ABI;
    dimsum_moe_ext_t ext;
    if (const int rc = ext_from<dimsum_moe_ext_t>(p->ext, ext)) return rc;
    if (p->num_experts < 1 || p->num_experts > kMaxE) return DIMSUM_ERR_SHAPE;
    if (p->tokens < 0 || p->tokens >= ((int64_t)1 << 31) - kBM * (kMaxE + 1)) return DIMSUM_ERR_SHAPE;
    if (p->k <= 0 || p->k % 32 != 0 || p->k >= ((int64_t)1 << 31) || p->n <= 0 || p->n % 32 != 0 || p->n > (int64_t)65535 * kBN) return DIMSUM_ERR_SHAPE;
    if (p->tokens == 0) return DIMSUM_OK;
    if (!p->x_ptr || !p->x_inv_ptr || !p->offsets_ptr || !p->w_ptrs || !p->w_inv_ptrs || !p->out_ptr) return DIMSUM_ERR_NULL;
    if (p->ldc < p->n) return DIMSUM_ERR_STRIDE;
    moe_gemm_f16_args_t a;
    memset(&a, 0, sizeof(a));
    for (int e = 0; e < p->num_experts; ++e) {
        if (!p->w_ptrs[e] || !p->w_inv_ptrs[e]) return DIMSUM_ERR_NULL;
        if (!al16(p->w_ptrs[e]) || !al16(p->w_inv_ptrs[e])) return DIMSUM_ERR_STRIDE;
        a.w[e] = reinterpret_cast<const __half *>(p->w_ptrs[e]);
        a.w_inv[e] = reinterpret_cast<const float *>(p->w_inv_ptrs[e]);
    }
    if (!al16(p->x_ptr) || !aligned_to<char>(p->x_inv_ptr, 4) || !al16(p->out_ptr) || !al16(p->bias_ptr) || !aligned_to<char>(p->offsets_ptr, 4) ||
        p->ldc % 4 != 0)
        return DIMSUM_ERR_STRIDE;
    a.x = reinterpret_cast<const __half *>(p->x_ptr);
    a.x_inv = reinterpret_cast<const float *>(p->x_inv_ptr);
    a.bias = reinterpret_cast<const float *>(p->bias_ptr);
    a.offsets = reinterpret_cast<const int *>(p->offsets_ptr);
    a.out = reinterpret_cast<float *>(p->out_ptr);
    a.T = p->tokens; a.ldc = p->ldc;
    a.K = (int)p->k; a.N = (int)p->n; a.E = p->num_experts;
    const dim3 grid((unsigned)((p->tokens + kBM - 1) / kBM + p->num_experts), (unsigned)((p->n + kBN - 1) / kBN));
    hipLaunchKernelGGL(moe_gemm_f16_kernel, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    return launch_status();
}
