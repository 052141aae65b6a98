// moe_gemm_f16.hip -- the grouped expert GEMM of moe_gemm.hip on scaled-fp16 operand images (common.hpp, f16s): ONE fp16 MFMA product per element
// instead of the three bf16 products of the fp32 kernel, two-byte operand rows from HBM into LDS instead of four-byte ones.
//   out[j, n] = x_inv[j] w_inv_e[n] sum_k x16[j, k] w16_e[n, k] (+ bias[e, n])     for offsets[e] <= j < offsets[e + 1]
// x16 (T, K) fp16 with x_inv (T) is the image a producer pass wrote (dimsum_moe_permute_f16s, dimsum_moe_act_fwd_f16s, dimsum_rows_f16s); the E weight
// images (N, K) fp16 and their (N) inverse scales are separate tensors whose addresses travel BY VALUE in the kernel arguments.
//
//  * what moe_gemm.hip does is kept: the offsets are read ON THE DEVICE under the table rule of moe_gemm_common.hpp; the grid is the static bound
//    (ceil(T / kBM) + E) x ceil(N / kBN); a short last tile loads its missing rows from its last valid row and stores nothing for them; a tile
//    index past the last real tile leaves at once; rows outside every range are not written. No split-K, no atomics: one fixed summation order
//    per output element, bit-reproducible.
//  * arithmetic: v_mfma_f32_16x16x32_f16 into fp32 accumulators; products of two fp16 values are exact in fp32, so the only rounding is the fp32
//    accumulation. The two power-of-two inverse scales (exact) and the bias are applied in the epilogue.
//  * workgroup = 4 waves = one 64 x 128 output tile (a wave: 32 rows x 64 columns), K tiles 64 deep = two MFMA steps per barrier; two LDS buffers
//    of 24 KB (x: 64 rows, W: 128 rows of 128 bytes). The global loads of tile t + 1 (six 16-byte loads per thread) are issued before the MFMAs of
//    tile t and written into the other buffer after them; one barrier per K tile.
//  * LDS layout: the 16-byte piece p (0..7) of row r sits at piece p ^ ((r >> 1) & 7). A ds_read_b128 of an MFMA operand (lane l: row l & 15, piece
//    4 s + (l >> 4)) is served in four groups of 16 lanes, each holding the 16 rows once, 8 of them at piece p and 8 at piece p ^ 1: rows of one
//    parity share a 128-byte half of the 256-byte bank row and land on 8 distinct slots of it (the sets {0, 1, 6, 7} and {2, 3, 4, 5} of r >> 1 are
//    closed under ^ 1), so every group touches 16 distinct 16-byte slots. A ds_write_b128 group of 8 lanes fills one whole row: 128 contiguous bytes.
#include "moe_gemm_common.hpp"

namespace dimsum {
namespace {

using namespace moe_gemm;

constexpr int kBK = 64;
constexpr int kRowB = kBK * 2;                       // bytes of an LDS row: 64 fp16
constexpr int kXo = 0, kWo = kBM * kRowB, kBuf = kWo + kBN * kRowB;      // 24576

typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));

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
    const auto [e, row0, cnt] = find_row_tile(a.offsets, a.E, (int)a.T, blockIdx.x);
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
    const auto load = [&](int kt) {
        const int k = min(kt * kBK + sc * 8, K - 8);
#pragma unroll
        for (int i = 0; i < 2; ++i) gx[i] = ld16(xg[i] + k);
#pragma unroll
        for (int i = 0; i < 4; ++i) gw[i] = ld16(wg[i] + k);
    };
    const auto write = [&](int buf) {
        char *b = lds + buf * kBuf + so;
#pragma unroll
        for (int i = 0; i < 2; ++i) *reinterpret_cast<u32x4 *>(b + kXo + i * 32 * kRowB) = gx[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<u32x4 *>(b + kWo + i * 32 * kRowB) = gw[i];
    };

    f4 acc[2][4];
    zero_acc(acc);

    // operand reads: lane l holds row l & 15 of a 16-row fragment, the 8 k values of piece 4 s + (l >> 4) of MFMA step s
    const int fr = lane & 15, fc = lane >> 4;
    int xo[2], wo[2];                                     // (+ 16 rows: + 16 * kRowB, the same piece: (16 >> 1) & 7 == 0)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        xo[s] = kXo + lds_off(wm * 32 + fr, 4 * s + fc);
        wo[s] = kWo + lds_off(wn * 64 + fr, 4 * s + fc);
    }

    // K % 32 == 0: with an odd number of 32-deep steps the last tile is half a tile. Its pieces 4..7 lie past the row's end: those threads load
    // the row's last piece instead (load clamps the column) and the tile's second MFMA step is skipped
    const int nk = (K + kBK - 1) / kBK;
    const bool half_tail = (K % kBK) != 0;
    load(0);
    write(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const bool more = kt + 1 < nk;                    // (uniform)
        if (more) load(kt + 1);
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
        if (more) write((kt + 1) & 1);                    // the buffer every wave finished reading before the previous barrier
        __syncthreads();
    }

    const float *bias = a.bias ? a.bias + (int64_t)e * N : nullptr;
    const float *winv = a.w_inv[e];
    float xi[2];                                          // the scales of the lane's two rows (a row past the tile's count: the last valid row's, unused)
#pragma unroll
    for (int i = 0; i < 2; ++i) xi[i] = a.x_inv[row0 + min(wm * 32 + i * 16 + fr, cnt - 1)];
    store_tile(acc, a.out, a.ldc, row0, cnt, wm * 32, n0 + wn * 64, N, [&](int i, int n, const float4 &v) {
        const float4 wi = ldf4(winv + n);
        // (acc xi) wi: two exact multiplications by powers of two, whatever the order
        const float4 s = make_float4(v.x * xi[i] * wi.x, v.y * xi[i] * wi.y, v.z * xi[i] * wi.z, v.w * xi[i] * wi.w);
        return bias ? add4(s, ldf4(bias + n)) : s;
    });
}

}  // namespace
}  // namespace dimsum

extern "C" int dimsum_moe_gemm_f16s(const dimsum_moe_gemm_f16s_params_t *p, void *stream) {
    using namespace dimsum;
    if (const int rc = check_call(p, kRowLenMax, grid_width_max(kBN))) return rc;     // k: a row length; n: column tiles on gridDim.y
    if (p->tokens == 0) return DIMSUM_OK;
    if (!p->x_ptr || !p->x_inv_ptr || !p->offsets_ptr || !p->w_ptrs || !p->w_inv_ptrs || !p->out_ptr) return DIMSUM_ERR_NULL;
    if (p->ldc < p->n) return DIMSUM_ERR_STRIDE;
    moe_gemm_f16_args_t a;
    memset(&a, 0, sizeof(a));
    if (const int rc = expert_ptrs(p->num_experts, p->w_ptrs, a.w, p->w_inv_ptrs, a.w_inv)) return rc;
    if (!al16(p->x_ptr) || !aligned_to<char>(p->x_inv_ptr, 4) || !al16(p->out_ptr) || !al16(p->bias_ptr) || !aligned_to<char>(p->offsets_ptr, 4) ||
        p->ldc % 4 != 0)
        return DIMSUM_ERR_STRIDE;
    fill_table_args(a, p);
    a.x = reinterpret_cast<const __half *>(p->x_ptr);
    a.x_inv = reinterpret_cast<const float *>(p->x_inv_ptr);
    a.bias = reinterpret_cast<const float *>(p->bias_ptr);
    a.out = reinterpret_cast<float *>(p->out_ptr);
    a.ldc = p->ldc;
    hipLaunchKernelGGL(moe_gemm_f16_kernel, dim3(row_tiles(p->tokens, p->num_experts), tiles(p->n, kBN)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    return launch_status();
}
