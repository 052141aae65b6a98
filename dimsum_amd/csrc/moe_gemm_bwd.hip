// moe_gemm_bwd.hip -- the two gradients of the grouped expert GEMM (moe_gemm.hip: out[j, :] = x[j, :] . W_e(j)^T) over the rows sorted by expert.
// Both read the E + 1 offsets ON THE DEVICE under the table rule of moe_gemm_common.hpp: a training step's backward has no device-to-host copy
// either, and whatever the table holds nothing outside the tensors is read or written.
//
//   dgrad: dx[j, :] = dy[j, :] . W_e(j)         dy (T, N), W_e (N, K) row-major (the parameter itself), dx (T, K); rows outside every range are not written
//   wgrad: dW_e[n, k] = sum_{j in range e} dy[j, n] x[j, k]   (+ db[e, n] = sum_j dy[j, n]);  an empty range stores zeros: no memset, no host decision
//
//  * arithmetic and LDS: the bf16 three-product image of moe_gemm_common.hpp, for every operand of both kernels. No split-K, no atomics: one
//    fixed summation order per output element, so a rerun gives the same bits.
//  * what differs from the forward is the STAGING of the operands whose reduction index runs over ROWS in global memory (dgrad: W_e, reduced over n;
//    wgrad: dy and x, both reduced over j). Nothing is transposed in global memory: a thread loads 8 consecutive reduction rows of one or two
//    columns (a wave's loads of one row are contiguous: 512 / 256 bytes), splits them and writes the 8 values as ONE 16-byte piece of the column's
//    LDS row -- the transposition is the choice of which registers go into a piece. (The 16-byte stores of a wave are 2-way conflicting, 16 against
//    the 13 LDS cycles the store's own data transfer takes; the operand reads, which outnumber them 3 : 1 in issue slots, are the ones kept clean.)
//  * dgrad: the forward's grid and row tiles ((ceil(T / 64) + E) row tiles x ceil(K / 128) column tiles, a short last tile stores nothing for its
//    missing rows), the forward's pipeline (the loads of step t + 1 fly over the MFMAs of step t).
//  * wgrad: a static grid ceil(K / 128) x ceil(N / 64) x E; a workgroup walks its expert's rows in 32-row steps. The range length is known only on
//    the device: rows at or past the range's end are loaded from the range's last row and REPLACED BY ZEROS before they are split (both operands),
//    so the last partial step adds nothing. db: the workgroups of k tile 0 sum, per thread, the dy values they stage (8 rows of every 32, one
//    column) and add the four waves' partial sums in the order ((w0 + w1) + w2) + w3 through LDS.
#include "moe_gemm_common.hpp"

namespace dimsum {
namespace {

using namespace moe_gemm;
using namespace moe_gemm::bf16x3;

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

__device__ __forceinline__ float2 ldf2(const float *p) { return *reinterpret_cast<const float2 *>(p); }

// ---------------------------------------------------------------------------------------------------------------------
// dgrad
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void moe_gemm_dgrad_kernel(const moe_dgrad_args_t a) {
    __shared__ __attribute__((aligned(16))) char lds[2 * kBuf];
    const auto [e, row0, cnt] = find_row_tile(a.offsets, a.E, (int)a.T, blockIdx.x);
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
    const auto load = [&](int nt) {
        const int n = nt * kBK;
        gy[0] = ldf4(yg + n); gy[1] = ldf4(yg + n + 4);
#pragma unroll
        for (int i = 0; i < 8; ++i) gw[i] = ldf2(wg + (int64_t)(n + i) * K);
    };
    const auto write = [&](int buf) {
        char *b = lds + buf * kBuf;
        stage8(b + kXhi + so, b + kXlo + so, gy[0], gy[1]);
        stage8(b + kWhi + wso0, b + kWlo + wso0, gw[0].x, gw[1].x, gw[2].x, gw[3].x, gw[4].x, gw[5].x, gw[6].x, gw[7].x);
        stage8(b + kWhi + wso1, b + kWlo + wso1, gw[0].y, gw[1].y, gw[2].y, gw[3].y, gw[4].y, gw[5].y, gw[6].y, gw[7].y);
    };

    f4 acc[2][4];
    zero_acc(acc);
    const int fr = lane & 15, fc = lane >> 4;
    const int xo = lds_off(wm * 32 + fr, fc), wo = lds_off(wn * 64 + fr, fc);

    const int nn = N / kBK;
    load(0);
    write(0);
    __syncthreads();
    for (int nt = 0; nt < nn; ++nt) {
        const bool more = nt + 1 < nn;                    // (uniform)
        if (more) load(nt + 1);
        mfma_step(lds + (nt & 1) * kBuf, xo, wo, acc);
        if (more) write((nt + 1) & 1);                    // the buffer every wave finished reading before the previous barrier
        __syncthreads();
    }

    store_tile(acc, a.dx, a.ldc, row0, cnt, wm * 32, k0 + wn * 64, K, [](int, int, const float4 &v) { return v; });
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
    const auto load = [&](int jt) {
        const int j = jt * kBK + wv * 8;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const bool in = j + i < cnt;
            const int64_t r = o0 + min(j + i, cnt - 1);
            const float2 xv = ldf2(a.x + r * K + xc);
            const float yv = a.dy[r * N + yc];
            gx[i] = in ? xv : make_float2(0.f, 0.f);
            gy[i] = in ? yv : 0.f;
        }
    };
    const auto write = [&](int buf) {
        char *b = lds + buf * kBuf;
        stage8(b + kXhi + yso, b + kXlo + yso, gy[0], gy[1], gy[2], gy[3], gy[4], gy[5], gy[6], gy[7]);
        stage8(b + kWhi + xso0, b + kWlo + xso0, gx[0].x, gx[1].x, gx[2].x, gx[3].x, gx[4].x, gx[5].x, gx[6].x, gx[7].x);
        stage8(b + kWhi + xso1, b + kWlo + xso1, gx[0].y, gx[1].y, gx[2].y, gx[3].y, gx[4].y, gx[5].y, gx[6].y, gx[7].y);
        if (want_db) dbsum += ((gy[0] + gy[1]) + (gy[2] + gy[3])) + ((gy[4] + gy[5]) + (gy[6] + gy[7]));
    };

    f4 acc[2][4];
    zero_acc(acc);
    const int fr = lane & 15, fc = lane >> 4;
    const int yo = lds_off(wm * 32 + fr, fc), xo = lds_off(wn * 64 + fr, fc);

    const int nj = (cnt + kBK - 1) / kBK;                 // (uniform)
    if (nj > 0) {
        load(0);
        write(0);
    }
    __syncthreads();
    for (int jt = 0; jt < nj; ++jt) {
        const bool more = jt + 1 < nj;
        if (more) load(jt + 1);
        mfma_step(lds + (jt & 1) * kBuf, yo, xo, acc);
        if (more) write((jt + 1) & 1);
        __syncthreads();
    }

    // dW_e rows n0 .. below N (the tile's "rows" are dy's columns), columns k0 .. below K
    store_tile(acc, a.dw[e], K, n0, N - n0, wm * 32, k0 + wn * 64, K, [](int, int, const float4 &v) { return v; });
    if (want_db) {                                        // (uniform) the four waves' partial sums of column lane, added in a fixed order
        dbs[wv][lane] = dbsum;
        __syncthreads();
        if (wv == 0 && n0 + lane < N) a.db[(int64_t)e * N + n0 + lane] = ((dbs[0][lane] + dbs[1][lane]) + dbs[2][lane]) + dbs[3][lane];
    }
}

// the gradients' widths: k tiles of kBN ride on dgrad's gridDim.y (and wgrad's gridDim.x), n tiles of kBM on wgrad's gridDim.y; one pair of
// limits for both entries, so that a step's two gradients are served or refused together
constexpr int64_t kKMax = grid_width_max(kBN), kNMax = grid_width_max(kBM);

}  // namespace
}  // namespace dimsum

extern "C" int dimsum_moe_gemm_dgrad(const dimsum_moe_gemm_dgrad_params_t *p, void *stream) {
    using namespace dimsum;
    if (const int rc = check_call(p, kKMax, kNMax)) return rc;
    if (p->tokens == 0) return DIMSUM_OK;
    if (!p->dy_ptr || !p->offsets_ptr || !p->w_ptrs || !p->dx_ptr) return DIMSUM_ERR_NULL;
    if (p->ldc < p->k) return DIMSUM_ERR_STRIDE;
    moe_dgrad_args_t a;
    memset(&a, 0, sizeof(a));
    if (const int rc = expert_ptrs(p->num_experts, p->w_ptrs, a.w)) return rc;
    if (!al16(p->dy_ptr) || !al16(p->dx_ptr) || !aligned_to<char>(p->offsets_ptr, 4) || p->ldc % 4 != 0) return DIMSUM_ERR_STRIDE;
    fill_table_args(a, p);
    a.dy = reinterpret_cast<const float *>(p->dy_ptr);
    a.dx = reinterpret_cast<float *>(p->dx_ptr);
    a.ldc = p->ldc;
    hipLaunchKernelGGL(moe_gemm_dgrad_kernel, dim3(row_tiles(p->tokens, p->num_experts), tiles(p->k, kBN)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    return launch_status();
}

extern "C" int dimsum_moe_gemm_wgrad(const dimsum_moe_gemm_wgrad_params_t *p, void *stream) {
    using namespace dimsum;
    if (const int rc = check_call(p, kKMax, kNMax)) return rc;
    if (p->tokens == 0) return DIMSUM_OK;
    if (!p->dy_ptr || !p->x_ptr || !p->offsets_ptr || !p->dw_ptrs) return DIMSUM_ERR_NULL;
    moe_wgrad_args_t a;
    memset(&a, 0, sizeof(a));
    if (const int rc = expert_ptrs(p->num_experts, p->dw_ptrs, a.dw)) return rc;
    if (!al16(p->dy_ptr) || !al16(p->x_ptr) || !aligned_to<char>(p->db_ptr, 4) || !aligned_to<char>(p->offsets_ptr, 4)) return DIMSUM_ERR_STRIDE;
    fill_table_args(a, p);
    a.dy = reinterpret_cast<const float *>(p->dy_ptr);
    a.x = reinterpret_cast<const float *>(p->x_ptr);
    a.db = reinterpret_cast<float *>(p->db_ptr);
    hipLaunchKernelGGL(moe_gemm_wgrad_kernel, dim3(tiles(p->k, kBN), tiles(p->n, kBM), (unsigned)p->num_experts), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    return launch_status();
}
