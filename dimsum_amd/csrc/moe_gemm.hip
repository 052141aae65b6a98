// moe_gemm.hip -- the grouped expert GEMM of the top-1 mixture-of-experts layer: out[j, :] = xp[j, :] . W_e(j)^T (+ b_e(j)) over the rows sorted by
// expert, e(j) = the expert whose range [offsets[e], offsets[e + 1]) holds j. The offsets are read ON THE DEVICE under the table rule of
// moe_gemm_common.hpp: the layer's forward has no device-to-host copy and can be captured into a hipGraph.
//
//  * grid: (ceil(T / kBM) + E) row tiles x ceil(N / kBN) column tiles -- a static upper bound. A workgroup finds the expert that owns its row
//    tile (find_row_tile); a tile index past the last real tile leaves at once. A short last tile of an expert loads its missing rows from the
//    tile's last valid row and stores nothing for them.
//  * the E weight matrices are separate tensors (separate nn.Parameters): their addresses travel BY VALUE in the kernel arguments.
//  * arithmetic and LDS: the bf16 three-product image of moe_gemm_common.hpp. No split-K, no atomics: one fixed summation order per output
//    element, bit-reproducible.
//  * workgroup = 4 waves = one 64 x 128 output tile, K tiles 32 deep, two LDS buffers: the global loads of tile t + 1 are issued before the MFMAs
//    of tile t and written (converted, 16 bytes per ds_write) into the other buffer after them; one barrier per K tile.
#include "moe_gemm_common.hpp"

namespace dimsum {
namespace {

using namespace moe_gemm;
using namespace moe_gemm::bf16x3;

struct moe_gemm_args_t {
    const float *x, *bias;
    const int *offsets;
    float *out;
    int64_t T, ldc;
    int K, N, E;
    const float *w[kMaxE];
};

__global__ __launch_bounds__(256) void moe_gemm_kernel(const moe_gemm_args_t a) {
    __shared__ __attribute__((aligned(16))) char lds[2 * kBuf];
    const auto [e, row0, cnt] = find_row_tile(a.offsets, a.E, (int)a.T, blockIdx.x);
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
    const auto load = [&](int kt) {
        const int k = kt * kBK;
        gx[0] = ldf4(xg + k); gx[1] = ldf4(xg + k + 4);
        gw0[0] = ldf4(wg0 + k); gw0[1] = ldf4(wg0 + k + 4);
        gw1[0] = ldf4(wg1 + k); gw1[1] = ldf4(wg1 + k + 4);
    };
    const auto write = [&](int buf) {
        char *b = lds + buf * kBuf + so;
        stage8(b + kXhi, b + kXlo, gx[0], gx[1]);
        stage8(b + kWhi, b + kWlo, gw0[0], gw0[1]);
        stage8(b + kWhi + 64 * kRowB, b + kWlo + 64 * kRowB, gw1[0], gw1[1]);
    };

    f4 acc[2][4];
    zero_acc(acc);
    const int fr = lane & 15, fc = lane >> 4;
    const int xo = lds_off(wm * 32 + fr, fc), wo = lds_off(wn * 64 + fr, fc);

    const int nk = K / kBK;
    load(0);
    write(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const bool more = kt + 1 < nk;                    // (uniform)
        if (more) load(kt + 1);
        mfma_step(lds + (kt & 1) * kBuf, xo, wo, acc);
        if (more) write((kt + 1) & 1);                    // the buffer every wave finished reading before the previous barrier
        __syncthreads();
    }

    const float *bias = a.bias ? a.bias + (int64_t)e * N : nullptr;
    store_tile(acc, a.out, a.ldc, row0, cnt, wm * 32, n0 + wn * 64, N, [&](int, int n, const float4 &v) { return bias ? add4(v, ldf4(bias + n)) : v; });
}

}  // namespace
}  // namespace dimsum

extern "C" int dimsum_moe_gemm(const dimsum_moe_gemm_params_t *p, void *stream) {
    using namespace dimsum;
    if (const int rc = check_call(p, kRowLenMax, grid_width_max(kBN))) return rc;     // k: a row length; n: column tiles on gridDim.y
    if (p->tokens == 0) return DIMSUM_OK;
    if (!p->x_ptr || !p->offsets_ptr || !p->w_ptrs || !p->out_ptr) return DIMSUM_ERR_NULL;
    if (p->ldc < p->n) return DIMSUM_ERR_STRIDE;
    moe_gemm_args_t a;
    memset(&a, 0, sizeof(a));
    if (const int rc = expert_ptrs(p->num_experts, p->w_ptrs, a.w)) return rc;
    if (!al16(p->x_ptr) || !al16(p->out_ptr) || !al16(p->bias_ptr) || !aligned_to<char>(p->offsets_ptr, 4) || p->ldc % 4 != 0) return DIMSUM_ERR_STRIDE;
    fill_table_args(a, p);
    a.x = reinterpret_cast<const float *>(p->x_ptr);
    a.bias = reinterpret_cast<const float *>(p->bias_ptr);
    a.out = reinterpret_cast<float *>(p->out_ptr);
    a.ldc = p->ldc;
    hipLaunchKernelGGL(moe_gemm_kernel, dim3(row_tiles(p->tokens, p->num_experts), tiles(p->n, kBN)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    return launch_status();
}
