// moe_gemm.hip -- the grouped expert GEMM of the top-1 mixture-of-experts layer: out[j, :] = xp[j, :] . W_e(j)^T (+ b_e(j)) over the rows sorted by
// expert, e(j) = the expert whose range [offsets[e], offsets[e + 1]) holds j. The offsets are read ON THE DEVICE (they are what dimsum_moe_route_fwd
// writes): the host never learns the slice lengths, so the layer's forward has no device-to-host copy and can be captured into a hipGraph.
//
//  * grid: (ceil(T / kBM) + E) row tiles x ceil(N / kBN) column tiles -- a static upper bound: sum_e ceil(n_e / kBM) <= T / kBM + E. A workgroup scans
//    the at most 65 offsets (wave-uniform) for the expert that owns its row tile; a tile index past the last real tile leaves at once. A tile never
//    spans two experts: a short last tile of an expert loads its missing rows from the tile's last valid row and stores nothing for them.
//  * the E weight matrices are separate tensors (separate nn.Parameters): their addresses travel BY VALUE in the kernel arguments.
//  * arithmetic: fp32 operands are split while they are staged, hi = bf16(v), lo = bf16(v - hi) (split2, common.hpp), and every 32-deep step takes the
//    three products hi.hi + hi.lo + lo.hi on v_mfma_f32_16x16x32_bf16 into one fp32 accumulator -- the products the library forms for fp32 operands
//    under allow_tf32. No split-K, no atomics: one fixed summation order per output element, bit-reproducible.
//  * workgroup = 4 waves = one 64 x 128 output tile, K tiles 32 deep, two LDS buffers of 24 KB (xp hi | xp lo | W hi | W lo, 64-byte rows): the
//    global loads of tile t + 1 are issued before the MFMAs of tile t and written (converted, 16 bytes per ds_write) into the other buffer after
//    them; one barrier per K tile. The 16-byte piece c of row r sits at piece c ^ ((4 - (r >> 2)) & 3): the ds_read_b128 of an MFMA operand
//    (lane l: row l & 15, piece l >> 4) then touches 16 distinct 16-byte slots in each of its four 16-lane service groups.
//  * the MFMA takes the weight fragment as A and the token fragment as B (D[n][m]): a lane ends with 4 CONSECUTIVE output columns of one row
//    (16-byte stores, 16-byte bias loads).
#include "common.hpp"

namespace dimsum {
namespace {

constexpr int kBM = DIMSUM_MOE_GEMM_BM, kBN = DIMSUM_MOE_GEMM_BN, kBK = 32;
constexpr int kMaxE = 64;
constexpr int kRowB = kBK * 2;                       // bytes of an LDS row: 32 bf16
constexpr int kXhi = 0, kXlo = kBM * kRowB, kWhi = 2 * kBM * kRowB, kWlo = kWhi + kBN * kRowB, kBuf = kWlo + kBN * kRowB;      // 24576

typedef float f4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct moe_gemm_args_t {
    const float *x, *bias;
    const int *offsets;
    float *out;
    int64_t T, ldc;
    int K, N, E;
    const float *w[kMaxE];
};

__device__ __forceinline__ int lds_off(int r, int c) { return r * kRowB + ((c ^ ((4 - ((r >> 2) & 3)) & 3)) << 4); }

// 8 consecutive fp32 -> 8 bf16 hi, 8 bf16 lo, one 16-byte LDS store each
__device__ __forceinline__ void stage(char *hi, char *lo, const float4 &a, const float4 &b) {
    unsigned h0, h1, h2, h3, l0, l1, l2, l3;
    split2(a.x, a.y, h0, l0);
    split2(a.z, a.w, h1, l1);
    split2(b.x, b.y, h2, l2);
    split2(b.z, b.w, h3, l3);
    *reinterpret_cast<u32x4 *>(hi) = u32x4{h0, h1, h2, h3};
    *reinterpret_cast<u32x4 *>(lo) = u32x4{l0, l1, l2, l3};
}

__global__ __launch_bounds__(256) void moe_gemm_kernel(const moe_gemm_args_t a) {
    __shared__ __attribute__((aligned(16))) char lds[2 * kBuf];
    // ---- the row tile's expert, first row and row count (every value wave-uniform). Offsets are clamped to [0, T] and a range starts no earlier than
    // the previous non-empty one ended: whatever the table holds, no row outside the tensors is read or written and no row is written by two tiles
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
    const float *w = a.w[e];

    // staging: thread = (row tid >> 2, 8 k values tid & 3) of the token tile and of both 64-row halves of the weight tile; rows past the tile's
    // count / past N read the last valid row (their results are never stored)
    const int sr = tid >> 2, sc = tid & 3;
    const float *xg = a.x + (int64_t)(row0 + min(sr, cnt - 1)) * K + sc * 8;
    const float *wg0 = w + (int64_t)min(n0 + sr, N - 1) * K + sc * 8;
    const float *wg1 = w + (int64_t)min(n0 + 64 + sr, N - 1) * K + sc * 8;
    const int so = lds_off(sr, sc);                       // (row sr + 64 of the weight tile: + 64 rows, the same piece)

    float4 gx[2], gw0[2], gw1[2];
#define DIMSUM_MG_LOAD(KT)                                                                                                    \
    do {                                                                                                                      \
        const int k_ = (KT) * kBK;                                                                                            \
        gx[0] = ldf4(xg + k_); gx[1] = ldf4(xg + k_ + 4);                                                                     \
        gw0[0] = ldf4(wg0 + k_); gw0[1] = ldf4(wg0 + k_ + 4);                                                                 \
        gw1[0] = ldf4(wg1 + k_); gw1[1] = ldf4(wg1 + k_ + 4);                                                                 \
    } while (0)
#define DIMSUM_MG_WRITE(BUF)                                                                                                  \
    do {                                                                                                                      \
        char *b_ = lds + (BUF) * kBuf + so;                                                                                   \
        stage(b_ + kXhi, b_ + kXlo, gx[0], gx[1]);                                                                            \
        stage(b_ + kWhi, b_ + kWlo, gw0[0], gw0[1]);                                                                          \
        stage(b_ + kWhi + 64 * kRowB, b_ + kWlo + 64 * kRowB, gw1[0], gw1[1]);                                                \
    } while (0)

    f4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

    // operand reads: lane l holds row l & 15 of a 16-row fragment, the 8 k values of piece l >> 4
    const int fr = lane & 15, fc = lane >> 4;
    const int xo = lds_off(wm * 32 + fr, fc), wo = lds_off(wn * 64 + fr, fc);       // (+ 16 rows: + 16 * kRowB, the same piece)

    const int nk = K / kBK;
    DIMSUM_MG_LOAD(0);
    DIMSUM_MG_WRITE(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const bool more = kt + 1 < nk;                    // (uniform)
        if (more) DIMSUM_MG_LOAD(kt + 1);
        const char *b = lds + (kt & 1) * kBuf;
        bf16x8_t xh[2], xl[2], wh[4], wl[4];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            xh[i] = *reinterpret_cast<const bf16x8_t *>(b + kXhi + xo + i * 16 * kRowB);
            xl[i] = *reinterpret_cast<const bf16x8_t *>(b + kXlo + xo + i * 16 * kRowB);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            wh[j] = *reinterpret_cast<const bf16x8_t *>(b + kWhi + wo + j * 16 * kRowB);
            wl[j] = *reinterpret_cast<const bf16x8_t *>(b + kWlo + wo + j * 16 * kRowB);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[j], xh[i], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[j], xl[i], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl[j], xh[i], acc[i][j], 0, 0, 0);
            }
        if (more) DIMSUM_MG_WRITE((kt + 1) & 1);          // the buffer every wave finished reading before the previous barrier
        __syncthreads();
    }
#undef DIMSUM_MG_LOAD
#undef DIMSUM_MG_WRITE

    // ---- epilogue: D[n][m] -- the lane's column is token row m = l & 15, its 4 registers are the output columns 4 (l >> 4) .. + 3
    const float *bias = a.bias ? a.bias + (int64_t)e * N : nullptr;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = wm * 32 + i * 16 + fr;
        if (m >= cnt) continue;                           // the rows after a short tile belong to the next expert
        float *orow = a.out + (int64_t)(row0 + m) * a.ldc;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + wn * 64 + j * 16 + fc * 4;
            if (n >= N) continue;
            float4 v = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
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
extern "C" int dimsum_moe_gemm(const dimsum_moe_gemm_params_t *p, void *stream) {
    using namespace dimsum;
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_moe_gemm_params_t)) return DIMSUM_ERR_ABI;
    dimsum_moe_ext_t ext;
    if (const int rc = ext_from<dimsum_moe_ext_t>(p->ext, ext)) return rc;
    if (p->num_experts < 1 || p->num_experts > kMaxE) return DIMSUM_ERR_SHAPE;
    if (p->tokens < 0 || p->tokens >= ((int64_t)1 << 31) - kBM * (kMaxE + 1)) return DIMSUM_ERR_SHAPE;
    if (p->k <= 0 || p->k % kBK != 0 || p->k >= ((int64_t)1 << 31) || p->n <= 0 || p->n % 32 != 0 || p->n > (int64_t)65535 * kBN) return DIMSUM_ERR_SHAPE;
    if (p->tokens == 0) return DIMSUM_OK;
    if (!p->x_ptr || !p->offsets_ptr || !p->w_ptrs || !p->out_ptr) return DIMSUM_ERR_NULL;
    if (p->ldc < p->n) return DIMSUM_ERR_STRIDE;
    moe_gemm_args_t a;
    memset(&a, 0, sizeof(a));
    for (int e = 0; e < p->num_experts; ++e) {
        if (!p->w_ptrs[e]) return DIMSUM_ERR_NULL;
        if (!al16(p->w_ptrs[e])) return DIMSUM_ERR_STRIDE;
        a.w[e] = reinterpret_cast<const float *>(p->w_ptrs[e]);
    }
    if (!al16(p->x_ptr) || !al16(p->out_ptr) || !al16(p->bias_ptr) || !aligned_to<char>(p->offsets_ptr, 4) || p->ldc % 4 != 0) return DIMSUM_ERR_STRIDE;
    a.x = reinterpret_cast<const float *>(p->x_ptr);
    a.bias = reinterpret_cast<const float *>(p->bias_ptr);
    a.offsets = reinterpret_cast<const int *>(p->offsets_ptr);
    a.out = reinterpret_cast<float *>(p->out_ptr);
    a.T = p->tokens; a.ldc = p->ldc;
    a.K = (int)p->k; a.N = (int)p->n; a.E = p->num_experts;
    const dim3 grid((unsigned)((p->tokens + kBM - 1) / kBM + p->num_experts), (unsigned)((p->n + kBN - 1) / kBN));
    hipLaunchKernelGGL(moe_gemm_kernel, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    return launch_status();
}
