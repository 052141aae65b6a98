// moe_gemm_common.hpp -- what the grouped expert GEMM kernels share (moe_gemm.hip: forward; moe_gemm_f16.hip: forward on scaled-fp16 images;
// moe_gemm_bwd.hip: dgrad and wgrad): the rule that turns the device's offset table into row ranges, the bf16 three-product LDS image, the store
// walk over a wave's accumulators, and the host checks of the four entries. Each .hip file keeps what is its own: the argument struct, the
// staging pattern, the pipeline loop and the entry.
//
// THE TABLE RULE. The E + 1 offsets are read ON THE DEVICE (they are what dimsum_moe_route_fwd writes; the host never learns the slice lengths).
// They are expected to be non-decreasing in [0, T]; whatever they hold, range e is [o0, o1) with o1 = offsets[e + 1] clamped to [0, T] and o0 =
// offsets[e] clamped to [0, T] and raised to the end of the last non-empty range before it (clamped_range). So no row outside the tensors is
// read or written and no row belongs to two ranges: no row is written twice. A row tile (find_row_tile) never spans two ranges.
#pragma once
#include "common.hpp"

namespace dimsum {
namespace moe_gemm {

constexpr int kBM = DIMSUM_MOE_GEMM_BM, kBN = DIMSUM_MOE_GEMM_BN;     // the workgroup's tile: 64-row operand x 128-row operand (a wave: 32 x 64)
constexpr int kMaxE = 64;

typedef float f4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// range e of the table under the rule above; taken: the end of the last non-empty range before e
__device__ __forceinline__ void clamped_range(const int *offsets, int e, int T, int taken, int &o0, int &o1) {
    o0 = max(min(max(offsets[e], 0), T), taken);
    o1 = min(max(offsets[e + 1], 0), T);
}

// Row tile `tile` of the grid's static bound ceil(T / kBM) + E >= sum_e ceil(n_e / kBM): its expert, first row and row count (every value
// wave-uniform). A short last tile of a range has cnt < kBM; cnt == 0: past the last real tile.
struct row_tile_t { int e, row0, cnt; };
__device__ __forceinline__ row_tile_t find_row_tile(const int *offsets, int E, int T, int tile) {
    int e = 0, before = 0, row0 = 0, cnt = 0, taken = 0;
    for (; e < E; ++e) {
        int o0, o1;
        clamped_range(offsets, e, T, taken, o0, o1);
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
    return {e, row0, cnt};
}

__device__ __forceinline__ void zero_acc(f4 (&acc)[2][4]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
}

// The MFMAs take the 128-row operand as A and the 64-row operand as B (D[col][row]): of each of its 2 x 4 fragments lane l ends with row l & 15
// and the 4 CONSECUTIVE columns 4 (l >> 4) .. + 3 -- 16-byte stores (and 16-byte bias / scale loads). Stores the wave's rows wrow + 16 i + (l & 15)
// below `rows` (of the tile whose first row is row `row0` of out: the rows after a short tile belong to the next expert), columns c = col0 + 16 j
// + 4 (l >> 4) below `cols`: out[row0 + row][c .. c + 3] = f(i, c, acc).
template <typename F>
__device__ __forceinline__ void store_tile(const f4 (&acc)[2][4], float *out, int64_t ld, int row0, int rows, int wrow, int col0, int cols, F f) {
    const int lane = threadIdx.x & 63, fr = lane & 15, fc = lane >> 4;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = wrow + i * 16 + fr;
        if (m >= rows) continue;
        float *orow = out + (int64_t)(row0 + m) * ld;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = col0 + j * 16 + fc * 4;
            if (c >= cols) continue;
            stf4(orow + c, f(i, c, make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3])));
        }
    }
}

__device__ __forceinline__ float4 add4(const float4 &v, const float4 &b) { return make_float4(v.x + b.x, v.y + b.y, v.z + b.z, v.w + b.w); }

// ---------------------------------------------------------------------------------------------------------------------
// The bf16 three-product image (forward, dgrad, wgrad). fp32 operands are split while they are staged, hi = bf16(v), lo = bf16(v - hi) (split2,
// common.hpp), and every 32-deep step takes hi.hi + hi.lo + lo.hi on v_mfma_f32_16x16x32_bf16 into one fp32 accumulator: the products the
// library forms for fp32 operands under allow_tf32. An operand tile is [row = output index][32 reduction values] in 64-byte rows, hi and lo
// images apart; a buffer is x hi | x lo | W hi | W lo = 24 KB (x: the kBM-row operand, W: the kBN-row operand), and a kernel holds two.
// The 16-byte piece c of row r sits at piece c ^ ((4 - (r >> 2)) & 3). The ds_read_b128 of an MFMA operand (lane l: row l & 15, piece l >> 4) is
// served in four 16-lane groups ({0-3, 12-15, 20-27}, ...): a group's lanes hold, for each of the four values of row >> 2, all four pieces or
// one piece pair twice over two row quads whose XOR keys differ, i.e. 16 distinct 16-byte slots of the 256-byte bank row -- conflict-free for
// every operand of the three kernels, because every operand is staged into this one image.
// ---------------------------------------------------------------------------------------------------------------------
namespace bf16x3 {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
constexpr int kBK = 32;
constexpr int kRowB = kBK * 2;                       // bytes of an LDS row: 32 bf16
constexpr int kXhi = 0, kXlo = kBM * kRowB, kWhi = 2 * kBM * kRowB, kWlo = kWhi + kBN * kRowB, kBuf = kWlo + kBN * kRowB;      // 24576

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
__device__ __forceinline__ void stage8(char *hi, char *lo, const float4 &a, const float4 &b) { stage8(hi, lo, a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w); }

// one 32-deep step on the LDS buffer b: acc[i][j] += W rows (wo + 16 j) x X rows (xo + 16 i), three products. xo, wo: lds_off(the wave's first
// row + (l & 15), l >> 4) -- 16 rows on are + 16 * kRowB, the same piece
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

}  // namespace bf16x3

// ---------------------------------------------------------------------------------------------------------------------
// Host side. Every entry checks in this order: params, struct_size, extension, shapes (check_call); tokens == 0 is then a valid call that needs
// no pointers and launches nothing; required pointers; ldc >= width; the per-expert tables (expert_ptrs); the other alignments and ldc % 4.
// ---------------------------------------------------------------------------------------------------------------------
inline bool al16(const void *p) { return aligned_to<char>(p, 16); }

// What bounds a width depends on the part it plays in the entry's kernels: a width whose tiles of `tile` columns are counted by a grid dimension
// is held to 65535 tiles (gridDim.y's limit; kept for wgrad's gridDim.x too); a width that is only a row length, to int32 element indexing.
constexpr int64_t kRowLenMax = ((int64_t)1 << 31) - 1;
constexpr int64_t grid_width_max(int tile) { return (int64_t)65535 * tile; }
inline unsigned tiles(int64_t n, int tile) { return (unsigned)((n + tile - 1) / tile); }
inline unsigned row_tiles(int64_t tokens, int num_experts) { return tiles(tokens, kBM) + (unsigned)num_experts; }      // find_row_tile's bound

// params, struct_size, extension, shapes of any of the four parameter structs; k_max, n_max: the entry's widest k and n
template <typename P> inline int check_call(const P *p, int64_t k_max, int64_t n_max) {
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(P)) return DIMSUM_ERR_ABI;
    dimsum_moe_ext_t ext;
    if (const int rc = ext_from<dimsum_moe_ext_t>(p->ext, ext)) return rc;
    if (p->num_experts < 1 || p->num_experts > kMaxE) return DIMSUM_ERR_SHAPE;
    if (p->tokens < 0 || p->tokens >= ((int64_t)1 << 31) - kBM * (kMaxE + 1)) return DIMSUM_ERR_SHAPE;      // the grid's row_tiles() x kBM rows fit an int
    if (p->k <= 0 || p->k % 32 != 0 || p->k > k_max || p->n <= 0 || p->n % 32 != 0 || p->n > n_max) return DIMSUM_ERR_SHAPE;
    return DIMSUM_OK;
}

// copies one table of per-expert device pointers (or two that belong together) into the kernel arguments. Expert by expert, and in this order:
// a missing pointer is DIMSUM_ERR_NULL, a pointer that is not 16-byte aligned DIMSUM_ERR_STRIDE
template <typename A, typename B = A>
inline int expert_ptrs(int num_experts, const void *const *src_a, A **dst_a, const void *const *src_b = nullptr, B **dst_b = nullptr) {
    for (int e = 0; e < num_experts; ++e) {
        if (!src_a[e] || (src_b && !src_b[e])) return DIMSUM_ERR_NULL;
        if (!al16(src_a[e]) || (src_b && !al16(src_b[e]))) return DIMSUM_ERR_STRIDE;
        dst_a[e] = reinterpret_cast<A *>(const_cast<void *>(src_a[e]));
        if (src_b) dst_b[e] = reinterpret_cast<B *>(const_cast<void *>(src_b[e]));
    }
    return DIMSUM_OK;
}

// the fields every argument struct has
template <typename A, typename P> inline void fill_table_args(A &a, const P *p) {
    a.offsets = reinterpret_cast<const int *>(p->offsets_ptr);
    a.T = p->tokens;
    a.K = (int)p->k; a.N = (int)p->n; a.E = p->num_experts;
}

}  // namespace moe_gemm
}  // namespace dimsum
