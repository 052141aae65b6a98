// moe_gemm_bwd.hip -- the two gradients of the grouped expert GEMM (moe_gemm.hip: out[j, :] = x[j, :] . W_e(j)^T) over the rows sorted by expert.
// Both read the E + 1 offsets ON THE DEVICE, clamp them to [0, T] and cut overlapping ranges exactly as moe_gemm_kernel does: a training step's
// backward has no device-to-host copy either, and whatever the table holds nothing outside the tensors is read or written.
//
//   dgrad: dx[j, :] = dy[j, :] . W_e(j)         dy (T, N), W_e (N, K) row-major (the parameter itself), dx (T, K); rows outside every range are not written
//   wgrad: dW_e[n, k] = sum_{j in range e} dy[j, n] x[j, k]   (+ db[e, n] = sum_j dy[j, n]);  an empty range stores zeros: no memset, no host decision
//
//  * arithmetic: the forward's. fp32 operands are split while they are staged (hi = bf16(v), lo = bf16(v - hi), split2) and every 32-deep step takes
//    hi.hi + hi.lo + lo.hi on v_mfma_f32_16x16x32_bf16 into one fp32 accumulator. No split-K, no atomics: one fixed summation order per output
//    element, so a rerun gives the same bits.
//  * LDS: the forward's image, so the forward's argument holds verbatim. An operand tile is [row = output index][32 reduction values] in 64-byte
//    rows, hi and lo images apart; the 16-byte piece c of row r sits at piece c ^ ((4 - (r >> 2)) & 3). The ds_read_b128 of an MFMA operand (lane l:
//    row l & 15, piece l >> 4) is served in four 16-lane groups ({0-3, 12-15, 20-27}, ...): a group's lanes hold, for each of the four values of
//    row >> 2, all four pieces or one piece pair twice over two row quads whose XOR keys differ, i.e. 16 distinct 16-byte slots of the 256-byte bank
//    row -- conflict-free, for every operand of both kernels, because every operand is staged into this one image.
//  * what differs from the forward is the STAGING of the operands whose reduction index runs over ROWS in global memory (dgrad: W_e, reduced over n;
//    wgrad: dy and x, both reduced over j). Nothing is transposed in global memory: a thread loads 8 consecutive reduction rows of one or two
//    columns (a wave's loads of one row are contiguous: 512 / 256 bytes), splits them and writes the 8 values as ONE 16-byte piece of the column's
//    LDS row -- the transposition is the choice of which registers go into a piece. (The 16-byte stores of a wave are 2-way conflicting, 16 against
//    the 13 LDS cycles the store's own data transfer takes; the operand reads, which outnumber them 3 : 1 in issue slots, are the ones kept clean.)
//  * dgrad: the forward's grid and row-tile / expert mapping ((ceil(T / 64) + E) row tiles x ceil(K / 128) column tiles, a tile never spans two
//    experts, a short last tile stores nothing for its missing rows), the forward's pipeline (the loads of step t + 1 fly over the MFMAs of step t).
//  * wgrad: a static grid ceil(K / 128) x ceil(N / 64) x E; a workgroup walks its expert's rows in 32-row steps. The range length is known only on
//    the device: rows at or past the range's end are loaded from the range's last row and REPLACED BY ZEROS before they are split (both operands),
//    so the last partial step adds nothing. db: the workgroups of k tile 0 sum, per thread, the dy values they stage (8 rows of every 32, one
//    column) and add the four waves' partial sums in the order ((w0 + w1) + w2) + w3 through LDS.
//  * the MFMA takes the 128-row operand as A and the 64-row operand as B (D[a][b]): a lane ends with 4 CONSECUTIVE output columns of one row.
#include "common.hpp"

namespace dimsum {
namespace {

constexpr int kBM = DIMSUM_MOE_GEMM_BM, kBN = DIMSUM_MOE_GEMM_BN, kBK = 32;       // 64-row operand, 128-row operand, reduction step
constexpr int kMaxE = 64;
constexpr int kRowB = kBK * 2;                       // bytes of an LDS row: 32 bf16
constexpr int kXhi = 0, kXlo = kBM * kRowB, kWhi = 2 * kBM * kRowB, kWlo = kWhi + kBN * kRowB, kBuf = kWlo + kBN * kRowB;      // 24576

typedef float f4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct moe_dgrad_args_t {
    const float *dy;
    const int *offsets;
    float *dx;
    int64_t T, ldc;
    int K, N, E;
    const float *w[kMaxE];
};

struct moe_wgrad_args_t {
    const float *dy, *x;
    const int *offsets;
    float *db;
    int64_t T;
    int K, N, E;
    float *dw[kMaxE];
};

__device__ __forceinline__ int lds_off(int r, int c) { return r * kRowB + ((c ^ ((4 - ((r >> 2) & 3)) & 3)) << 4); }

// 8 consecutive reduction values -> 8 bf16 hi, 8 bf16 lo, one 16-byte LDS store each
__device__ __forceinline__ void stage8(char *hi, char *lo, float v0, float v1, float v2, float v3, float v4, float v5, float v6, float v7) {
    unsigned h0, h1, h2, h3, l0, l1, l2, l3;
    split2(v0, v1, h0, l0);
    split2(v2, v3, h1, l1);
    split2(v4, v5, h2, l2);
    split2(v6, v7, h3, l3);
    *reinterpret_cast<u32x4 *>(hi) = u32x4{h0, h1, h2, h3};
    *reinterpret_cast<u32x4 *>(lo) = u32x4{l0, l1, l2, l3};
}

__device__ __forceinline__ float2 ldf2(const float *p) { return *reinterpret_cast<const float2 *>(p); }

// range e of the table as the kernels see it: clamped to [0, T], starting no earlier than the last non-empty range before it ended
__device__ __forceinline__ void clamped_range(const int *offsets, int e, int T, int taken, int &o0, int &o1) {
    o0 = max(min(max(offsets[e], 0), T), taken);
    o1 = min(max(offsets[e + 1], 0), T);
}

// one 32-deep step on the LDS buffer b: acc[i][j] += W rows (wo + 16 j) x X rows (xo + 16 i), three products
__device__ __forceinline__ void mfma_step(const char *b, int xo, int wo, f4 (&acc)[2][4]) {
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
}

// ---------------------------------------------------------------------------------------------------------------------
// dgrad
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void moe_gemm_dgrad_kernel(const moe_dgrad_args_t a) {
    __shared__ __attribute__((aligned(16))) char lds[2 * kBuf];
    // ---- the row tile's expert, first row and row count (every value wave-uniform): moe_gemm_kernel's scan
    const int tile = blockIdx.x;
    const int T = (int)a.T;
    int e = 0, before = 0, row0 = 0, cnt = 0, taken = 0;
    for (; e < a.E; ++e) {
        int o0, o1;
        clamped_range(a.offsets, e, T, taken, o0, o1);
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
    const int k0 = blockIdx.y * kBN;
    const float *w = a.w[e];

    // staging of dy: the forward's (thread = row tid >> 2, 8 n values tid & 3); rows past the tile's count read the last valid row
    const int sr = tid >> 2, sc = tid & 3;
    const float *yg = a.dy + (int64_t)(row0 + min(sr, cnt - 1)) * N + sc * 8;
    const int so = lds_off(sr, sc);
    // staging of W_e, transposed: thread = (8 n rows wv, output columns 2 lane and 2 lane + 1); a column pair past K reads the last pair
    const int wc = min(k0 + 2 * lane, K - 2);
    const float *wg = w + (int64_t)(wv * 8) * K + wc;
    const int wso0 = lds_off(2 * lane, wv), wso1 = lds_off(2 * lane + 1, wv);

    float4 gy[2];
    float2 gw[8];
#define DIMSUM_MD_LOAD(NT)                                                                                                    \
    do {                                                                                                                      \
        const int n_ = (NT) * kBK;                                                                                            \
        gy[0] = ldf4(yg + n_); gy[1] = ldf4(yg + n_ + 4);                                                                     \
        _Pragma("unroll") for (int i_ = 0; i_ < 8; ++i_) gw[i_] = ldf2(wg + (int64_t)(n_ + i_) * K);                          \
    } while (0)
#define DIMSUM_MD_WRITE(BUF)                                                                                                  \
    do {                                                                                                                      \
        char *b_ = lds + (BUF) * kBuf;                                                                                        \
        stage8(b_ + kXhi + so, b_ + kXlo + so, gy[0].x, gy[0].y, gy[0].z, gy[0].w, gy[1].x, gy[1].y, gy[1].z, gy[1].w);       \
        stage8(b_ + kWhi + wso0, b_ + kWlo + wso0, gw[0].x, gw[1].x, gw[2].x, gw[3].x, gw[4].x, gw[5].x, gw[6].x, gw[7].x);   \
        stage8(b_ + kWhi + wso1, b_ + kWlo + wso1, gw[0].y, gw[1].y, gw[2].y, gw[3].y, gw[4].y, gw[5].y, gw[6].y, gw[7].y);   \
    } while (0)

    f4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

    // operand reads: lane l holds row l & 15 of a 16-row fragment, the 8 reduction values of piece l >> 4
    const int fr = lane & 15, fc = lane >> 4;
    const int xo = lds_off(wm * 32 + fr, fc), wo = lds_off(wn * 64 + fr, fc);       // (+ 16 rows: + 16 * kRowB, the same piece)

    const int nn = N / kBK;
    DIMSUM_MD_LOAD(0);
    DIMSUM_MD_WRITE(0);
    __syncthreads();
    for (int nt = 0; nt < nn; ++nt) {
        const bool more = nt + 1 < nn;                    // (uniform)
        if (more) DIMSUM_MD_LOAD(nt + 1);
        mfma_step(lds + (nt & 1) * kBuf, xo, wo, acc);
        if (more) DIMSUM_MD_WRITE((nt + 1) & 1);          // the buffer every wave finished reading before the previous barrier
        __syncthreads();
    }
#undef DIMSUM_MD_LOAD
#undef DIMSUM_MD_WRITE

    // ---- epilogue: D[k][m] -- the lane's column is token row m = l & 15, its 4 registers are the output columns 4 (l >> 4) .. + 3
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = wm * 32 + i * 16 + fr;
        if (m >= cnt) continue;                           // the rows after a short tile belong to the next expert
        float *orow = a.dx + (int64_t)(row0 + m) * a.ldc;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + wn * 64 + j * 16 + fc * 4;
            if (k >= K) continue;
            stf4(orow + k, make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]));
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// wgrad
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void moe_gemm_wgrad_kernel(const moe_wgrad_args_t a) {
    __shared__ __attribute__((aligned(16))) char lds[2 * kBuf];
    __shared__ float dbs[4][kBM];
    // ---- the expert's rows [o0, o1) (wave-uniform): the ranges before it decide where a malformed table lets it start
    const int e = blockIdx.z;
    const int T = (int)a.T;
    int taken = 0, o0 = 0, o1 = 0;
    for (int q = 0; q <= e; ++q) {
        clamped_range(a.offsets, q, T, taken, o0, o1);
        if (o1 > o0) taken = o1;
    }
    const int cnt = max(o1 - o0, 0);                      // 0: the loop below does not run and zeros are stored

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wm = wv & 1, wn = wv >> 1;                  // the wave's 32 n x 64 k of the tile
    const int K = a.K, N = a.N;
    const int k0 = blockIdx.x * kBN, n0 = blockIdx.y * kBM;
    const bool want_db = a.db != nullptr && blockIdx.x == 0;

    // staging, both transposed: thread = 8 rows wv of every 32-row step; x: columns 2 lane, 2 lane + 1 of the k tile; dy: column lane of the n tile.
    // Columns past the matrix read its last columns (their results are never stored)
    const int xc = min(k0 + 2 * lane, K - 2), yc = min(n0 + lane, N - 1);
    const int xso0 = lds_off(2 * lane, wv), xso1 = lds_off(2 * lane + 1, wv), yso = lds_off(lane, wv);

    float2 gx[8];
    float gy[8];
    float dbsum = 0.f;
    // rows at or past the range's end: read from the last row of the range, then replaced by zeros -- they add nothing
#define DIMSUM_MW_LOAD(JT)                                                                                                    \
    do {                                                                                                                      \
        const int j_ = (JT) * kBK + wv * 8;                                                                                   \
        _Pragma("unroll") for (int i_ = 0; i_ < 8; ++i_) {                                                                    \
            const bool in_ = j_ + i_ < cnt;                                                                                   \
            const int64_t r_ = o0 + min(j_ + i_, cnt - 1);                                                                    \
            const float2 x_ = ldf2(a.x + r_ * K + xc);                                                                        \
            const float y_ = a.dy[r_ * N + yc];                                                                               \
            gx[i_] = in_ ? x_ : make_float2(0.f, 0.f);                                                                        \
            gy[i_] = in_ ? y_ : 0.f;                                                                                          \
        }                                                                                                                     \
    } while (0)
#define DIMSUM_MW_WRITE(BUF)                                                                                                  \
    do {                                                                                                                      \
        char *b_ = lds + (BUF) * kBuf;                                                                                        \
        stage8(b_ + kXhi + yso, b_ + kXlo + yso, gy[0], gy[1], gy[2], gy[3], gy[4], gy[5], gy[6], gy[7]);                     \
        stage8(b_ + kWhi + xso0, b_ + kWlo + xso0, gx[0].x, gx[1].x, gx[2].x, gx[3].x, gx[4].x, gx[5].x, gx[6].x, gx[7].x);   \
        stage8(b_ + kWhi + xso1, b_ + kWlo + xso1, gx[0].y, gx[1].y, gx[2].y, gx[3].y, gx[4].y, gx[5].y, gx[6].y, gx[7].y);   \
        if (want_db) dbsum += ((gy[0] + gy[1]) + (gy[2] + gy[3])) + ((gy[4] + gy[5]) + (gy[6] + gy[7]));                      \
    } while (0)

    f4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

    const int fr = lane & 15, fc = lane >> 4;
    const int yo = lds_off(wm * 32 + fr, fc), xo = lds_off(wn * 64 + fr, fc);

    const int nj = (cnt + kBK - 1) / kBK;                 // (uniform)
    if (nj > 0) {
        DIMSUM_MW_LOAD(0);
        DIMSUM_MW_WRITE(0);
    }
    __syncthreads();
    for (int jt = 0; jt < nj; ++jt) {
        const bool more = jt + 1 < nj;
        if (more) DIMSUM_MW_LOAD(jt + 1);
        mfma_step(lds + (jt & 1) * kBuf, yo, xo, acc);
        if (more) DIMSUM_MW_WRITE((jt + 1) & 1);
        __syncthreads();
    }
#undef DIMSUM_MW_LOAD
#undef DIMSUM_MW_WRITE

    // ---- epilogue: D[k][n] -- the lane's column is the dW row n = l & 15, its 4 registers are the dW columns 4 (l >> 4) .. + 3
    float *dw = a.dw[e];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int n = n0 + wm * 32 + i * 16 + fr;
        if (n >= N) continue;
        float *orow = dw + (int64_t)n * K;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + wn * 64 + j * 16 + fc * 4;
            if (k >= K) continue;
            stf4(orow + k, make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]));
        }
    }
    if (want_db) {                                        // (uniform) the four waves' partial sums of column lane, added in a fixed order
        dbs[wv][lane] = dbsum;
        __syncthreads();
        if (wv == 0 && n0 + lane < N) a.db[(int64_t)e * N + n0 + lane] = ((dbs[0][lane] + dbs[1][lane]) + dbs[2][lane]) + dbs[3][lane];
    }
}

inline bool al16(const void *p) { return aligned_to<char>(p, 16); }

// the checks both entries share, after struct_size: extension, shapes
inline int check_shapes(const dimsum_moe_ext_t *ext_ptr, int32_t num_experts, int64_t tokens, int64_t k, int64_t n) {
    dimsum_moe_ext_t ext;
    if (const int rc = ext_from<dimsum_moe_ext_t>(ext_ptr, ext)) return rc;
    if (num_experts < 1 || num_experts > kMaxE) return DIMSUM_ERR_SHAPE;
    if (tokens < 0 || tokens >= ((int64_t)1 << 31) - kBM * (kMaxE + 1)) return DIMSUM_ERR_SHAPE;
    if (k <= 0 || k % 32 != 0 || n <= 0 || n % 32 != 0 || k > (int64_t)65535 * kBN || n > (int64_t)65535 * kBM) return DIMSUM_ERR_SHAPE;
    return DIMSUM_OK;
}

}  // namespace
}  // namespace dimsum

// (checks: struct sizes, then shapes, then -- for a call with rows -- pointers, then alignment; tokens == 0 needs no pointers and launches nothing)
extern "C" int dimsum_moe_gemm_dgrad(const dimsum_moe_gemm_dgrad_params_t *p, void *stream) {
    using namespace dimsum;
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_moe_gemm_dgrad_params_t)) return DIMSUM_ERR_ABI;
    if (const int rc = check_shapes(p->ext, p->num_experts, p->tokens, p->k, p->n)) return rc;
    if (p->tokens == 0) return DIMSUM_OK;
    if (!p->dy_ptr || !p->offsets_ptr || !p->w_ptrs || !p->dx_ptr) return DIMSUM_ERR_NULL;
    if (p->ldc < p->k) return DIMSUM_ERR_STRIDE;
    moe_dgrad_args_t a;
    memset(&a, 0, sizeof(a));
    for (int e = 0; e < p->num_experts; ++e) {
        if (!p->w_ptrs[e]) return DIMSUM_ERR_NULL;
        if (!al16(p->w_ptrs[e])) return DIMSUM_ERR_STRIDE;
        a.w[e] = reinterpret_cast<const float *>(p->w_ptrs[e]);
    }
    if (!al16(p->dy_ptr) || !al16(p->dx_ptr) || !aligned_to<char>(p->offsets_ptr, 4) || p->ldc % 4 != 0) return DIMSUM_ERR_STRIDE;
    a.dy = reinterpret_cast<const float *>(p->dy_ptr);
    a.offsets = reinterpret_cast<const int *>(p->offsets_ptr);
    a.dx = reinterpret_cast<float *>(p->dx_ptr);
    a.T = p->tokens; a.ldc = p->ldc;
    a.K = (int)p->k; a.N = (int)p->n; a.E = p->num_experts;
    const dim3 grid((unsigned)((p->tokens + kBM - 1) / kBM + p->num_experts), (unsigned)((p->k + kBN - 1) / kBN));
    hipLaunchKernelGGL(moe_gemm_dgrad_kernel, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    return launch_status();
}

extern "C" int dimsum_moe_gemm_wgrad(const dimsum_moe_gemm_wgrad_params_t *p, void *stream) {
    using namespace dimsum;
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_moe_gemm_wgrad_params_t)) return DIMSUM_ERR_ABI;
    if (const int rc = check_shapes(p->ext, p->num_experts, p->tokens, p->k, p->n)) return rc;
    if (p->tokens == 0) return DIMSUM_OK;
    if (!p->dy_ptr || !p->x_ptr || !p->offsets_ptr || !p->dw_ptrs) return DIMSUM_ERR_NULL;
    moe_wgrad_args_t a;
    memset(&a, 0, sizeof(a));
    for (int e = 0; e < p->num_experts; ++e) {
        if (!p->dw_ptrs[e]) return DIMSUM_ERR_NULL;
        if (!al16(p->dw_ptrs[e])) return DIMSUM_ERR_STRIDE;
        a.dw[e] = reinterpret_cast<float *>(p->dw_ptrs[e]);
    }
    if (!al16(p->dy_ptr) || !al16(p->x_ptr) || !aligned_to<char>(p->db_ptr, 4) || !aligned_to<char>(p->offsets_ptr, 4)) return DIMSUM_ERR_STRIDE;
    a.dy = reinterpret_cast<const float *>(p->dy_ptr);
    a.x = reinterpret_cast<const float *>(p->x_ptr);
    a.offsets = reinterpret_cast<const int *>(p->offsets_ptr);
    a.db = reinterpret_cast<float *>(p->db_ptr);
    a.T = p->tokens;
    a.K = (int)p->k; a.N = (int)p->n; a.E = p->num_experts;
    const dim3 grid((unsigned)((p->k + kBN - 1) / kBN), (unsigned)((p->n + kBM - 1) / kBM), (unsigned)p->num_experts);
    hipLaunchKernelGGL(moe_gemm_wgrad_kernel, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    return launch_status();
}
