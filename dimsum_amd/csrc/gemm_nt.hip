// gemm_nt.hip -- C ABI of the hand-written NT GEMM (gemm_nt_kernel.hpp): plain fp32 output, and the w12 GEMM of the gated MLP with
// bias + tanh-GeLU + gate as its epilogue (dimsum/mlp.py:66-70), written directly as the operand image of the w3 GEMM.
#include "gemm_nt_kernel.hpp"

namespace dimsum {
namespace gemm_nt {

// base + extension of the public parameter struct, flattened (include/dimsum_hip.h "Versioning"): what the entry points below read
struct gemm_flat_t : dimsum_gemm_ext_t {
    int32_t m, n, k, operand_dtype, epilogue;
    float out_scale;
    int64_t lda, ldb, ldc;
    const void *a_ptr, *b_ptr, *bias_ptr;
    void *c_ptr;
    const void *a_inv_scale_ptr, *b_inv_scale_ptr;
};
static int gemm_flat_from(const dimsum_gemm_params_t *p, gemm_flat_t &f) {
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_gemm_params_t)) return DIMSUM_ERR_ABI;
    const int rc = ext_from<dimsum_gemm_ext_t>(p->ext, f);
    if (rc != DIMSUM_OK) return rc;
    f.m = p->m; f.n = p->n; f.k = p->k; f.operand_dtype = p->operand_dtype; f.epilogue = p->epilogue; f.out_scale = p->out_scale;
    f.lda = p->lda; f.ldb = p->ldb; f.ldc = p->ldc;
    f.a_ptr = p->a_ptr; f.b_ptr = p->b_ptr; f.bias_ptr = p->bias_ptr; f.c_ptr = p->c_ptr;
    f.a_inv_scale_ptr = p->a_inv_scale_ptr; f.b_inv_scale_ptr = p->b_inv_scale_ptr;
    return DIMSUM_OK;
}

// ---- what the three entry points share ---------------------------------------------------------------------------------------------------
// the prologue: the flat block, the operands every product needs, and the part of Args that does not depend on the epilogue (K, the alias
// modes and the split ranges are the entry point's). any_16bit = false: the caller checks the operand type itself (NN: fp16 only, and after
// its factor pointers)
static int gemm_prologue(const dimsum_gemm_params_t *pub, gemm_flat_t &p, Args &a, bool any_16bit = true) {
    const int rc = gemm_flat_from(pub, p);
    if (rc != DIMSUM_OK) return rc;
    if (!p.a_ptr || !p.b_ptr || !p.c_ptr) return DIMSUM_ERR_NULL;
    if (any_16bit && p.operand_dtype != DIMSUM_F16 && p.operand_dtype != DIMSUM_BF16) return DIMSUM_ERR_DTYPE;
    a = Args{};
    a.A = reinterpret_cast<const char *>(p.a_ptr);
    a.C = p.c_ptr;
    a.lda = p.lda; a.ldb = p.ldb; a.ldc = p.ldc;
    a.M = p.m;
    a.tiles_m = p.m / kBM;
    // tile order: groups of 4 tile rows; a matrix of few tile rows (in_proj's d-major product: the weight is the left operand) walks whole tile
    // columns, so that every streamed right-operand panel is loaded once (tools/scratch/gm_sweep.py: 187 -> 178 us at 2048 x 65536 x 512)
    a.group_m = p.tune_group_m > 0 ? p.tune_group_m : (a.tiles_m <= 16 ? a.tiles_m : 4);
    a.out_scale = p.out_scale;
    a.sa = reinterpret_cast<const float *>(p.a_inv_scale_ptr);
    a.sb = reinterpret_cast<const float *>(p.b_inv_scale_ptr);
    return DIMSUM_OK;
}
// the right operand: n columns in tiles of tile_n, one matrix for both 128-column halves of a tile, the bias per column
inline void fill_right(Args &a, const gemm_flat_t &p, int n, int tile_n) {
    a.B0 = a.B1 = reinterpret_cast<const char *>(p.b_ptr);
    a.bias0 = reinterpret_cast<const float *>(p.bias_ptr);
    a.N = n;
    a.tiles_n = (n + tile_n - 1) / tile_n;
}

inline bool rows_16bit_ok(const void *ptr, int64_t ld, int64_t cols) { return ld % 8 == 0 && ld >= cols && aligned_to<char>(ptr, 16); }
inline bool rows_f32_out_ok(const gemm_flat_t &p) { return p.ldc % 4 == 0 && p.ldc >= p.n && aligned_to<char>(p.c_ptr, 16); }
// one 32-bit byte offset per lane: inside a 256-row panel of an operand whose rows run along the reduction, inside a 64-row K tile of one
// whose rows run OVER it (TN: both, NN: the right one), inside a 256-row output panel
inline bool offsets_fit(const gemm_flat_t &p, bool a_over_k, bool b_over_k) {
    const auto fits = [](int64_t ld, bool over_k) { return (over_k ? 64 * ld * 2 + 512 : 256 * ld * 2) < ((int64_t)1 << 31); };
    return fits(p.lda, a_over_k) && fits(p.ldb, b_over_k) && (int64_t)257 * p.ldc * 4 < ((int64_t)1 << 31);
}

// TN / NN: the reduction cut into `ranges` ranges of whole K tiles, two at least; the partial results `stride` elements apart
inline bool ranges_ok(int64_t k, int ranges) { return ranges >= 1 && k % ((int64_t)ranges * kBK) == 0 && k / ranges >= 2 * kBK; }
inline bool split_stride_ok(const gemm_flat_t &p, int splits, int64_t stride) { return splits <= 1 || (stride % 4 == 0 && stride >= (int64_t)p.m * p.ldc); }
// TN / NN per-reduction-row factors: the table + its maximum (k_scale, c_scale), OR the row scales themselves (k_inv_a [, k_inv_b]: the factors
// are formed in the kernel); `required`: NN has no launch without them. The factors of one range live in the 32 KB behind the ring.
constexpr int kRowFacRangeRows = 16384;
inline bool rowfac_pointers_ok(const gemm_flat_t &p, bool required) {
    if (p.k_inv_b_ptr && !p.k_inv_a_ptr) return false;
    if (p.k_inv_a_ptr) return !p.k_scale_ptr && !p.c_scale_ptr;
    return p.k_scale_ptr ? p.c_scale_ptr != nullptr : !required;
}
inline bool rowfac_aligned(const gemm_flat_t &p, int splits) {
    return !(p.k_scale_ptr && (!aligned_to<char>(p.k_scale_ptr, 16) || !aligned_to<char>(p.c_scale_ptr, 4))) &&
           !(p.k_inv_a_ptr && (!aligned_to<char>(p.k_inv_a_ptr, 16) || (p.k_inv_b_ptr && !aligned_to<char>(p.k_inv_b_ptr, 16)) || p.k / splits % 8 != 0));
}
inline void fill_rowfac(Args &a, const gemm_flat_t &p) {
    a.k_fac = reinterpret_cast<const _Float16 *>(p.k_scale_ptr);
    a.c_scale = reinterpret_cast<const float *>(p.c_scale_ptr);
    a.k_inv_a = reinterpret_cast<const float *>(p.k_inv_a_ptr);
    a.k_inv_b = reinterpret_cast<const float *>(p.k_inv_b_ptr);
}

// ---- launching ---------------------------------------------------------------------------------------------------------------------------
// where a launch goes. probe != NULL: nothing is launched, *probe receives the kernel family (0 = 256-row tiles, 1 = 128-row tiles,
// 2 = persistent stream) at the place that would have launched it
struct Where {
    hipStream_t s;
    hipEvent_t e0, e1;
    int *probe;
};
inline Where where(const gemm_flat_t &p, void *stream, int *probe) {
    return {reinterpret_cast<hipStream_t>(stream), reinterpret_cast<hipEvent_t>(p.timing_start_event), reinterpret_cast<hipEvent_t>(p.timing_stop_event), probe};
}
// the one launcher: every kernel of this file goes out here, timed (the extension's events at the dispatch boundaries) or plain
template <auto kKernel> int run(const Args &a, int workgroups, int threads, const Where &w) {
    const dim3 grid((unsigned)workgroups), block((unsigned)threads);
    DIMSUM_LAUNCH_EV(kKernel, grid, block, w.s, w.e0, w.e1, a);
    return launch_status();
}

template <int kOp, int kEpi, int kVar = 0> int launch(const Args &a, const Where &w) {
    if (w.probe) { *w.probe = 0; return DIMSUM_OK; }
    return run<gemm_nt_kernel<kOp, kEpi, kVar>>(a, a.tiles_m * a.tiles_n, 512, w);
}
// the 128 x 256-tile variant (4-wave workgroups, two per CU): launches whose epilogue is a large share of a tile's time (short K)
template <int kOp, int kEpi, int kVar = 0> int launch_m128(const Args &a0, const Where &w) {
    if (w.probe) { *w.probe = 1; return DIMSUM_OK; }
    Args a = a0;
    a.tiles_m = a.M / 128;
    a.group_m = a.tiles_m <= 32 ? a.tiles_m : 2 * a0.group_m;     // the same L2 patch in rows
    return run<gemm_nt_m128_kernel<kOp, kEpi, kVar>>(a, a.tiles_m * a.tiles_n, 256, w);
}
// persistent workgroups (kVarPersist): one per CU (a multiple of 8: the tile walk's XCD ranges), each walking the tile list as one K stream
inline int persist_grid() {        // queried per call for the CURRENT device (no cached state: several devices per process, any thread)
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    return cus >= 8 ? cus / 8 * 8 : 8;
}
template <int kOp, int kEpi, int kVar = 0> int launch_persist(const Args &a, const Where &w) {
    if (w.probe) { *w.probe = 2; return DIMSUM_OK; }
    return run<gemm_nt_persist_kernel<kOp, kEpi, kVar>>(a, persist_grid(), 512, w);
}
// scaled-fp16 operands (one product per element): both tile shapes are built
template <int kEpi, int kVar = 0> int launch_f16(const Args &a, const Where &w, bool m128) {
    return m128 ? launch_m128<kOpF16, kEpi, kVar>(a, w) : launch<kOpF16, kEpi, kVar>(a, w);
}

// ---- shape policy of the NT entry point ----------------------------------------------------------------------------------------------------
// 128-row tiles? They are built for the fp16 operands only (tune_variant 512 with bf16 is refused). tune_variant 512 / 513 force the
// 128-row / 256-row tiles (A / B runs, tools/bench_gemm.py) and 514 keeps the 256-row ones; 0 = by shape: scaled-fp16 operands (one product
// per element) with a short K spend a third to a half of a 256 x 256 tile's time in its epilogue. Per epilogue, for fp16 operands:
//   f32, f32 + bias, f16_qkv, f32_conv   k <= 576, or tune_variant 512
//   f32 gate + residual, gated f16, gelu f16   tune_variant 512 only
//   gated split3                         never (no 128-row build)
inline bool m128_tiles(int epilogue, bool bf, int k, int tune_variant) {
    if (bf || epilogue == DIMSUM_GEMM_EPI_GATED_GELU_SPLIT3) return false;
    if (tune_variant != 0) return tune_variant == 512;
    switch (epilogue) {
        case DIMSUM_GEMM_EPI_F32: case DIMSUM_GEMM_EPI_F32_BIAS: case DIMSUM_GEMM_EPI_F16_QKV: case DIMSUM_GEMM_EPI_F32_CONV: return k <= 576;
        default: return false;
    }
}
// the persistent stream? Built for fp16 operands under the gated f16 epilogue, which takes it by default, and under the fp32 gate + residual
// epilogue, which takes it only where tune_variant 514 asks (A / B only: see DESIGN 3.5). It needs whole column tiles, an even number (>= 4)
// of K tiles, more tiles than workgroups and plain (un-aliased) operands; tune_variant 512 / 513 forbid it (A / B runs)
inline bool persist_ok(const Args &a, int epilogue, bool bf, int tune_variant) {
    const bool gated = epilogue == DIMSUM_GEMM_EPI_GATED_GELU_F16;
    if (bf || tune_variant == 512 || tune_variant == 513 || !(gated || (epilogue == DIMSUM_GEMM_EPI_F32_GATE_RESIDUAL && tune_variant == 514))) return false;
    const int nk = a.K / kBK;
    return a.N % (gated ? 128 : kBN) == 0 && nk >= 4 && nk % 2 == 0 && a.tiles_m * a.tiles_n > persist_grid() && a.a_alias_tiles == 0 && a.b_alias_tiles == 0;
}

}  // namespace gemm_nt
}  // namespace dimsum

#ifdef DIMSUM_GEMM_TUNE      // tuning builds only (tools/scratch/build_variant.sh ... -DDIMSUM_GEMM_TUNE): schedule / store-policy variants of the plain bf16 kernel
#define DIMSUM_GEMM_TUNE_VARIANTS(X) X(1) X(2) X(4) X(8) X(12) X(16) X(3) X(40) X(44) X(72) X(104)
#define DIMSUM_GEMM_TUNE_CASE(V) case V: return launch<kOpBf16, kEpiF32, V>(a, w);
#endif

// `probe` != NULL: nothing is launched, *probe receives the kernel family (0 = 256-row tiles, 1 = 128-row tiles, 2 = persistent stream)
static int gemm_nt_run(const dimsum_gemm_params_t *pub, void *stream, int *probe) {
    using namespace dimsum;
    using namespace dimsum::gemm_nt;
    gemm_flat_t p;
    Args a;
    if (const int rc = gemm_prologue(pub, p, a)) return rc;
    if (p.m <= 0 || p.n <= 0 || p.k < 2 * kBK || p.m % kBM != 0 || p.k % kBK != 0 || p.n % 4 != 0) return DIMSUM_ERR_SHAPE;
    // a_alias_rows = C: the A rows are [hi | lo] pairs (2 C columns) read as the left image [hi | hi | lo] over k = 3 C
    if (p.a_alias_rows != 0 && (p.a_alias_rows < 0 || p.a_alias_rows % kBK != 0 || p.k != 3 * p.a_alias_rows)) return DIMSUM_ERR_SHAPE;
    if (p.b_alias_rows != 0 && (p.b_alias_rows < 0 || p.b_alias_rows % kBK != 0 || p.k != 3 * p.b_alias_rows || (p.epilogue != DIMSUM_GEMM_EPI_F32 && p.epilogue != DIMSUM_GEMM_EPI_F32_CONV))) return DIMSUM_ERR_SHAPE;
    if (!rows_16bit_ok(p.a_ptr, p.lda, p.a_alias_rows ? 2 * p.a_alias_rows : p.k) || !rows_16bit_ok(p.b_ptr, p.ldb, p.b_alias_rows ? 2 * p.b_alias_rows : p.k)) return DIMSUM_ERR_STRIDE;
    if (!offsets_fit(p, false, false)) return DIMSUM_ERR_STRIDE;
    a.K = p.k;
    a.a_alias_tiles = (int)(p.a_alias_rows / kBK);
    a.a_alias_from = a.a_alias_tiles;
    if (p.a_alias_weight_order) {       // the pair read as [hi | lo | hi]: the third piece re-reads the first (shift = two pieces)
        if (!p.a_alias_rows) return DIMSUM_ERR_SHAPE;
        a.a_alias_tiles *= 2;
        a.a_alias_from = a.a_alias_tiles;
    }
    a.b_alias_tiles = (int)(p.b_alias_rows / kBK);
    a.stagger = p.tune_reserved > 0 ? p.tune_reserved : 0;
    if ((p.a_inv_scale_ptr == nullptr) != (p.b_inv_scale_ptr == nullptr)) return DIMSUM_ERR_NULL;
    if (a.sb && !aligned_to<char>(a.sb, 16)) return DIMSUM_ERR_STRIDE;
#ifndef DIMSUM_GEMM_TUNE
    if (p.tune_variant != 0 && p.tune_variant != 512 && p.tune_variant != 513 && p.tune_variant != 514) return DIMSUM_ERR_UNSUPPORTED;
#endif
    const bool bf = p.operand_dtype == DIMSUM_BF16;
    if (p.tune_variant == 512 && bf) return DIMSUM_ERR_UNSUPPORTED;       // (the 128-row tiles are built for the fp16 operands only)
    const bool m128 = m128_tiles(p.epilogue, bf, p.k, p.tune_variant);
    const Where w = where(p, stream, probe);
    constexpr int kShip = kVarFullLineStores | kVarNtStores;      // the fp32 epilogues: 128-byte row segments, streaming stores (tools/bench_gemm.py --tune)
    if (p.epilogue == DIMSUM_GEMM_EPI_F32_GATE_RESIDUAL) {
        if (!p.residual_ptr) return DIMSUM_ERR_NULL;
        if (!rows_f32_out_ok(p) || p.residual_ld % 4 != 0 || p.residual_ld < p.n || !aligned_to<char>(p.residual_ptr, 16) ||
            (p.bias_ptr && !aligned_to<char>(p.bias_ptr, 16)) || (p.gate_ptr && (p.gate_ld % 4 != 0 || !aligned_to<char>(p.gate_ptr, 16))))
            return DIMSUM_ERR_STRIDE;
        if (p.gate_ptr && (p.rows_per_batch <= 0 || p.rows_per_batch % kBM != 0 || p.m % p.rows_per_batch != 0)) return DIMSUM_ERR_SHAPE;
        fill_right(a, p, p.n, kBN);
        a.res = reinterpret_cast<const float *>(p.residual_ptr);
        a.gate = reinterpret_cast<const float *>(p.gate_ptr);
        a.ldr = p.residual_ld; a.ldg = p.gate_ld;
        a.rows_per_batch = p.gate_ptr ? p.rows_per_batch : p.m;
        if (persist_ok(a, p.epilogue, bf, p.tune_variant)) return launch_persist<kOpF16, kEpiF32GateRes, kShip>(a, w);
        return bf ? launch<kOpBf16, kEpiF32GateRes, kShip>(a, w) : launch_f16<kEpiF32GateRes, kShip>(a, w, m128);
    }
    if (p.epilogue == DIMSUM_GEMM_EPI_F16_QKV) {
        if (bf || !a.sa || !p.gate_bound_ptr) return DIMSUM_ERR_NULL;
        if (p.rows_per_batch <= 0 || p.rows_per_batch % kBM != 0 || p.m % p.rows_per_batch != 0 || p.qkv_q_cols <= 0 || p.qkv_q_cols % 16 != 0 ||
            p.qkv_q_cols > p.n || p.n % 8 != 0)
            return DIMSUM_ERR_SHAPE;
        if (p.ldc % 8 != 0 || p.ldc < p.n || !aligned_to<char>(p.c_ptr, 16) || (p.bias_ptr && !aligned_to<char>(p.bias_ptr, 16)) ||
            (int64_t)257 * p.ldc * 2 >= ((int64_t)1 << 31))
            return DIMSUM_ERR_STRIDE;
        fill_right(a, p, p.n, kBN);
        a.gate_bound = reinterpret_cast<const float *>(p.gate_bound_ptr);
        a.rows_per_batch = p.rows_per_batch;
        a.q_cols = p.qkv_q_cols;
        return launch_f16<kEpiF16Qkv>(a, w, m128);
    }
    if (p.epilogue == DIMSUM_GEMM_EPI_GELU_F16) {
        // fc1 of the plain MLP: h = gelu_tanh(A B^T + bias) as the scaled-fp16 image of fc2's GEMM. Built for scaled-fp16 operands with the
        // bound-derived row scale only, on the tile shapes of the gated f16 epilogue's per-tile kernels (256-row; 128-row under tune_variant 512)
        // (unscaled fp16 operands or no bound -- a constant out_scale, as GATED_GELU_F16 allows -- are combinations that are not built either)
        if (bf || !a.sa || !p.gate_bound_ptr || p.a_alias_rows != 0 || p.x12_ptr || p.c_image_pieces != 0) return DIMSUM_ERR_UNSUPPORTED;
        if (!p.h_inv_scale_ptr) return DIMSUM_ERR_NULL;
        if (p.n % 8 != 0) return DIMSUM_ERR_SHAPE;
        if (p.ldc % 8 != 0 || p.ldc < p.n || !aligned_to<char>(p.c_ptr, 16) || (p.bias_ptr && !aligned_to<char>(p.bias_ptr, 16)) ||
            !aligned_to<char>(p.h_inv_scale_ptr, 4) || (int64_t)257 * p.ldc * 2 >= ((int64_t)1 << 31))
            return DIMSUM_ERR_STRIDE;
        fill_right(a, p, p.n, kBN);
        a.gate_bound = reinterpret_cast<const float *>(p.gate_bound_ptr);
        a.inv_out = reinterpret_cast<float *>(p.h_inv_scale_ptr);
        return launch_f16<kEpiGeluF16>(a, w, m128);
    }
    if (p.epilogue == DIMSUM_GEMM_EPI_F32_CONV) {
        if (!p.conv_weight_ptr) return DIMSUM_ERR_NULL;
        if (p.conv_rows <= 0 || p.conv_rows % kBM != 0 || p.conv_rows > p.m || p.conv_width < 2 || p.conv_width > 4 || p.conv_seq <= 0 || 256 % p.conv_seq != 0 ||
            p.conv_seq % 4 != 0 || p.n % p.conv_seq != 0 || p.conv_weight_ld < p.conv_width)
            return DIMSUM_ERR_SHAPE;
        if (!rows_f32_out_ok(p)) return DIMSUM_ERR_STRIDE;
        fill_right(a, p, p.n, kBN);
        a.bias0 = nullptr;      // (the conv's own bias is conv_b; bias_ptr is not looked at)
        a.conv_w = reinterpret_cast<const float *>(p.conv_weight_ptr);
        a.conv_b = reinterpret_cast<const float *>(p.conv_bias_ptr);
        a.conv_rows = p.conv_rows; a.conv_width = p.conv_width; a.conv_seq = p.conv_seq; a.conv_w_ld = p.conv_weight_ld;
        return bf ? launch<kOpBf16, kEpiF32Conv, kShip>(a, w) : launch_f16<kEpiF32Conv, kShip>(a, w, m128);
    }
    if (p.epilogue == DIMSUM_GEMM_EPI_F32 || p.epilogue == DIMSUM_GEMM_EPI_F32_BIAS) {
        if (!rows_f32_out_ok(p)) return DIMSUM_ERR_STRIDE;
        const bool bias = p.epilogue == DIMSUM_GEMM_EPI_F32_BIAS;
        if (bias && (!p.bias_ptr || !aligned_to<char>(p.bias_ptr, 16))) return DIMSUM_ERR_NULL;
        fill_right(a, p, p.n, kBN);
        if (bias) return bf ? launch<kOpBf16, kEpiF32Bias, kShip>(a, w) : launch_f16<kEpiF32Bias, kShip>(a, w, m128);
#ifdef DIMSUM_GEMM_TUNE
        if (bf) switch (p.tune_variant) {
            case 0: case 512: case 513: break;
            case 100: return launch<kOpBf16, kEpiF32, 0>(a, w);
            DIMSUM_GEMM_TUNE_VARIANTS(DIMSUM_GEMM_TUNE_CASE)
            default: return DIMSUM_ERR_UNSUPPORTED;
        }
#endif
        return bf ? launch<kOpBf16, kEpiF32, kShip>(a, w) : launch_f16<kEpiF32, kShip>(a, w, m128);
    }
    if (p.epilogue == DIMSUM_GEMM_EPI_GATED_GELU_SPLIT3 || p.epilogue == DIMSUM_GEMM_EPI_GATED_GELU_F16) {
        // b_ptr: the (2 F, K) weight of w12; n = 2 F; output: (M, 3 F) bf16 left image [hi | hi | lo] or (M, F) fp16
        if (p.n % 16 != 0) return DIMSUM_ERR_SHAPE;
        const int F = p.n / 2;
        const bool img = p.epilogue == DIMSUM_GEMM_EPI_GATED_GELU_SPLIT3;
        if (p.c_image_pieces != 0 && p.c_image_pieces != 3 && !(img && p.c_image_pieces == 2)) return DIMSUM_ERR_UNSUPPORTED;
        a.c_pieces2 = p.c_image_pieces == 2;
        if (p.ldc % 8 != 0 || p.ldc < (img ? (a.c_pieces2 ? 2 : 3) : 1) * (int64_t)F || !aligned_to<char>(p.c_ptr, 16) || (int64_t)257 * p.ldc * 2 + 6 * (int64_t)F >= ((int64_t)1 << 31))
            return DIMSUM_ERR_STRIDE;
        if (p.bias_ptr && !aligned_to<char>(p.bias_ptr, 16)) return DIMSUM_ERR_STRIDE;
        fill_right(a, p, F, 128);       // x1 and x2: the two halves of the weight and of the bias, F columns each
        a.B1 = a.B0 + (int64_t)F * p.ldb * 2;
        a.bias1 = a.bias0 ? a.bias0 + F : nullptr;
        if (p.gate_bound_ptr) {
            if (img || !a.sa || !p.h_inv_scale_ptr) return DIMSUM_ERR_NULL;
            a.gate_bound = reinterpret_cast<const float *>(p.gate_bound_ptr);
            a.inv_out = reinterpret_cast<float *>(p.h_inv_scale_ptr);
        }
        if (p.x12_ptr) {       // training forward: keep the fp32 [x1 | x2] for the backward: split-bf16 images, or scaled-fp16 operands with the bound-derived h scale
            const bool f16_train = !img && !bf && a.sa && p.gate_bound_ptr;
            if (!f16_train && (!img || !bf || a.sa)) return DIMSUM_ERR_UNSUPPORTED;
            if (p.x12_ld % 4 != 0 || p.x12_ld < p.n || !aligned_to<char>(p.x12_ptr, 16) || (int64_t)257 * p.x12_ld * 4 + (int64_t)p.n * 4 >= ((int64_t)1 << 31))
                return DIMSUM_ERR_STRIDE;
            a.x12 = reinterpret_cast<float *>(p.x12_ptr);
            a.ldx = p.x12_ld;
            // (kVarKeepX12 is built on the 256-row tiles only)
            return f16_train ? launch<kOpF16, kEpiGatedF16, kVarKeepX12>(a, w) : launch<kOpBf16, kEpiGatedSplit3, kVarKeepX12>(a, w);
        }
        if (img) return bf ? launch<kOpBf16, kEpiGatedSplit3>(a, w) : launch<kOpF16, kEpiGatedSplit3>(a, w);
        if (persist_ok(a, p.epilogue, bf, p.tune_variant)) return launch_persist<kOpF16, kEpiGatedF16>(a, w);
        return bf ? launch<kOpBf16, kEpiGatedF16>(a, w) : launch_f16<kEpiGatedF16>(a, w, m128);
    }
    return DIMSUM_ERR_UNSUPPORTED;
}

extern "C" int dimsum_gemm_nt(const dimsum_gemm_params_t *p, void *stream) { return gemm_nt_run(p, stream, nullptr); }

extern "C" int dimsum_gemm_nt_kernel_for(const dimsum_gemm_params_t *p) {
    int which = -1;
    const int rc = gemm_nt_run(p, nullptr, &which);
    return rc == DIMSUM_OK ? which : -rc;
}

// dW-shaped product: C[s] (m, n) = sum over rows r in split s of A[r, :m]^T B[r, :n]; A (k, m) and B (k, n) 16-bit rows over the reduction index
extern "C" int dimsum_gemm_tn(const dimsum_gemm_params_t *pub, int32_t splits, int64_t c_split_stride, void *stream) {
    using namespace dimsum;
    using namespace dimsum::gemm_nt;
    gemm_flat_t p;
    Args a;
    if (const int rc = gemm_prologue(pub, p, a)) return rc;
    if (p.epilogue != DIMSUM_GEMM_EPI_F32 || p.bias_ptr) return DIMSUM_ERR_UNSUPPORTED;
    if (((p.a_inv_scale_ptr || p.a_block_inv_ptr) == 0) != (p.b_inv_scale_ptr == nullptr)) return DIMSUM_ERR_NULL;
    if ((p.a_inv_scale_ptr || p.a_block_inv_ptr) && (p.operand_dtype != DIMSUM_F16 || splits != 1 || p.tn_pair_a_cols != 0 || p.a_alias_rows != 0)) return DIMSUM_ERR_UNSUPPORTED;
    if (!rowfac_pointers_ok(p, false)) return DIMSUM_ERR_NULL;
    if (p.k_scale_ptr || p.k_inv_a_ptr) {          // per-reduction-row factors: fp16 operands, plain rows
        if (p.operand_dtype != DIMSUM_F16 || p.a_inv_scale_ptr || p.a_block_inv_ptr || p.tn_pair_a_cols != 0 || p.a_alias_rows != 0) return DIMSUM_ERR_UNSUPPORTED;
        if (splits < 1 || p.k / splits > kRowFacRangeRows) return DIMSUM_ERR_SHAPE;
        if (!rowfac_aligned(p, splits)) return DIMSUM_ERR_STRIDE;
    }
    if (p.a_block_inv_ptr && (p.a_inv_scale_ptr || p.a_block_inv_ld < p.k / kBK || p.k > 64 * kBK)) return DIMSUM_ERR_SHAPE;
    if (p.b_inv_scale_ptr && !aligned_to<char>(p.b_inv_scale_ptr, 16)) return DIMSUM_ERR_STRIDE;
    const int row_splits = (p.tn_pair_a_cols != 0) ? splits / 3 : splits;       // (pairs: the three pieces share the row ranges)
    // (n % 256 != 0: the caller zero-pads B's rows to whole 256-column tiles -- ldb says so -- and only columns < n are stored)
    const int64_t n_pad = (p.n + kBN - 1) / kBN * kBN;
    if (!ranges_ok(p.k, row_splits) || p.m <= 0 || p.n <= 0 || p.m % kBM != 0 || p.n % 4 != 0 || (p.n % kBN != 0 && (p.ldb < n_pad || p.tn_pair_a_cols != 0)))
        return DIMSUM_ERR_SHAPE;
    if (!rows_16bit_ok(p.a_ptr, p.lda, p.m) || !rows_16bit_ok(p.b_ptr, p.ldb, p.n) || !rows_f32_out_ok(p) || !split_stride_ok(p, splits, c_split_stride)) return DIMSUM_ERR_STRIDE;
    if (!offsets_fit(p, true, true)) return DIMSUM_ERR_STRIDE;
    fill_right(a, p, p.n, kBN);
    a.K = p.k / row_splits;
    if (p.b_alias_rows != 0 || p.a_alias_weight_order) return DIMSUM_ERR_UNSUPPORTED;
    if (p.tn_pair_a_cols != 0 || p.tn_pair_b_cols != 0) {
        // both operands as [hi | lo] pairs: k = the rows of ONE piece, splits = 3 x (row ranges); lda >= 2 m-ish is the caller's business
        if (p.tn_pair_a_cols <= 0 || p.tn_pair_b_cols <= 0 || splits % 3 != 0 || p.a_alias_rows != 0 || p.tn_pair_a_cols % 8 != 0 || p.tn_pair_b_cols % 8 != 0)
            return DIMSUM_ERR_SHAPE;
        if (p.lda < p.tn_pair_a_cols + p.m || p.ldb < p.tn_pair_b_cols + p.n) return DIMSUM_ERR_STRIDE;
        a.tn_pieces = 1;
        a.a_pair_cols = p.tn_pair_a_cols;
        a.b_pair_cols = p.tn_pair_b_cols;
    }
    if (p.a_alias_rows != 0) {
        if (splits != 1 || p.a_alias_rows < 0 || p.a_alias_rows % kBK != 0 || p.k != 3 * p.a_alias_rows) return DIMSUM_ERR_SHAPE;
        a.a_alias_tiles = (int)(p.a_alias_rows / kBK);
    }
    a.splits = splits;
    a.c_split_stride = c_split_stride;
    a.out_scale = 1.0f;
    a.a_block_inv = reinterpret_cast<const float *>(p.a_block_inv_ptr);
    a.a_block_inv_ld = (int)p.a_block_inv_ld;
    fill_rowfac(a, p);
    const Where w = where(p, stream, nullptr);
    const int workgroups = a.tiles_m * a.tiles_n * splits;
    constexpr int kShipT = kVarFullLineStores | kVarNtStores | kVarTN;
    if (p.operand_dtype == DIMSUM_BF16) return run<gemm_nt_kernel<kOpBf16, kEpiF32, kShipT>>(a, workgroups, 512, w);
    if (a.k_fac || a.k_inv_a) return run<gemm_tn_rowfac_kernel<kOpF16, kEpiF32, kShipT>>(a, workgroups, 512, w);
    if (a.a_block_inv) return run<gemm_nt_kernel<kOpF16, kEpiF32, kShipT | kVarRebase>>(a, workgroups, 512, w);
    return run<gemm_nt_kernel<kOpF16, kEpiF32, kShipT>>(a, workgroups, 512, w);
}

// C[s] (m, n) = sum over the rows r of range s of A[0..m, r] B[r, 0..n): A rows contiguous along the reduction (NT-style), B rows over it (TN-style)
extern "C" int dimsum_gemm_nn(const dimsum_gemm_params_t *pub, int32_t splits, int64_t c_split_stride, void *stream) {
    using namespace dimsum;
    using namespace dimsum::gemm_nt;
    gemm_flat_t p;
    Args a;
    if (const int rc = gemm_prologue(pub, p, a, false)) return rc;
    if (!rowfac_pointers_ok(p, true)) return DIMSUM_ERR_NULL;
    if (p.operand_dtype != DIMSUM_F16) return DIMSUM_ERR_DTYPE;
    if (p.epilogue != DIMSUM_GEMM_EPI_F32 || p.bias_ptr || p.b_inv_scale_ptr || p.a_block_inv_ptr || p.tn_pair_a_cols != 0 || p.a_alias_rows != 0 ||
        p.b_alias_rows != 0 || p.a_alias_weight_order)
        return DIMSUM_ERR_UNSUPPORTED;
    if (!ranges_ok(p.k, splits) || p.m <= 0 || p.n <= 0 || p.m % kBM != 0 || p.n % kBN != 0 || p.k / splits > kRowFacRangeRows) return DIMSUM_ERR_SHAPE;
    if (!rows_16bit_ok(p.a_ptr, p.lda, p.k) || !rows_16bit_ok(p.b_ptr, p.ldb, p.n) || !rows_f32_out_ok(p) || !split_stride_ok(p, splits, c_split_stride) || !rowfac_aligned(p, splits))
        return DIMSUM_ERR_STRIDE;
    if (!offsets_fit(p, false, true)) return DIMSUM_ERR_STRIDE;
    fill_right(a, p, p.n, kBN);
    a.K = p.k / splits;
    a.splits = splits;
    a.c_split_stride = c_split_stride;
    a.out_scale = 1.0f;
    fill_rowfac(a, p);
    return run<gemm_nn_rowfac_kernel<kOpF16, kEpiF32, kVarFullLineStores | kVarNtStores>>(a, a.tiles_m * a.tiles_n * splits, 512, where(p, stream, nullptr));
}
