// cross_entropy.hip -- the LM training loss over rows of logits for gfx950: per row m, with s = logit_scale * logits[m, :],
//     lse = logsumexp(s)      z = lse_square_scale * lse^2      loss = lse - (1 - eps) s[label] - (eps / V) sum(s) + z
// and its gradient, written as T over a separate buffer or over the logits themselves,
//     dlogits[m, v] = dloss[m] * logit_scale * ((1 + 2 lse_square_scale lse) exp(s_v - lse) - (1 - eps) [v == label] - eps / V).
// What the reference's training recipes take from a fused cross-entropy (one pass for the loss, one in-place pass for the gradient) in place
// of F.cross_entropy's several library passes over the largest tensor of an LM training step.
//
// MI355X design: both kernels are memory-bound row passes; a row is walked in 16-byte PIECES (4 fp32 / 8 16-bit elements).
//   * Forward is ONE read of the row: every lane keeps a running (max, sum) pair -- online logsumexp -- and takes one local maximum and one
//     rescale of its sum per piece, not per element. The lanes' pairs meet in a cross-lane butterfly, the waves' pairs in LDS, where they
//     are folded in wave order. sum(s - s[0]) rides along only in the instantiation with label smoothing. The label's logit is fetched by one lane.
//   * Backward is one read and one write of the row from the saved lse (a double per row: m + log(sum) without the fp32 rounding that a
//     row offset of 80 would turn into a 4e-6 relative error of every probability); a lane reads a piece and writes the same piece, so the gradient may
//     replace the logits in place.
//   * Mapping: a row of more than kWaveRowMax = 4096 elements has one 256-thread workgroup to itself (16 pieces per lane at 16384 f32);
//     shorter rows take one WAVE each, four rows per workgroup, so that a small vocabulary with many rows fills the chip with rows instead
//     of idling three waves of four. The group (wave or workgroup) issues four pieces per lane before it consumes the first one.
//   * A piece is loaded by one 16-byte load when the row starts 16-byte aligned, element by element otherwise; what follows the last whole
//     piece is a PARTIAL piece, always loaded by elements and filled up with -inf (which adds exp(-inf) = 0). Either way piece i goes to lane
//     i % lanes and is folded by the same expressions: the summation order is a function of V and the dtype alone. No atomics. Two launches
//     on equal inputs are bit-identical, a row's bits do not depend on the number of rows or on its place in the grid, and a misaligned view
//     gives the bits of its aligned copy.
//   * Row offsets are 64-bit (M * row_stride passes 2^31 at 8192 x 50288 x 8 already in bytes); columns are 32-bit.
#include "row_pieces.hpp"

#include <cmath>

namespace dimsum {

constexpr int kCeThreads = 256;
constexpr int kCeWaveRowMax = 4096;     // V up to which a row is one wave's; above it, one workgroup's
constexpr int kCeUnroll = 4;            // pieces per lane in flight
constexpr float kLog2eLo = 1.92596299e-8f;      // log2(e) - (float)log2(e)

// (m, s): sum_i exp(x_i) = s * exp(m) over the elements folded so far. An empty or all -inf set is (-inf, 0): the reference point of the
// exponentials is then 0 instead of -inf, so that -inf - (-inf) never forms.
struct ce_pair_t { float m, s; };
// the lanes' pairs are folded in double (and the row's log is taken in double): 14 more fp32 roundings of the sum, and v_log_f32's error on
// top, are an absolute error of lse that every probability of the backward inherits as a relative one
struct ce_pair64_t { float m; double s; };

__device__ __forceinline__ ce_pair64_t ce_combine(const ce_pair64_t &a, const ce_pair64_t &b) {
#pragma clang fp contract(off)      // both partners of an exchange must form the same bits
    const float m = fmaxf(a.m, b.m);
    const float ref = m == -INFINITY ? 0.f : m;
    const double ea = (double)fast_exp2((a.m - ref) * kLog2e), eb = (double)fast_exp2((b.m - ref) * kLog2e);
    const double ta = a.s * ea, tb = b.s * eb;
    return {m, ta + tb};
}

struct ce_flags_t {
    int vec_in;     // logits rows start 16-byte aligned
    int vec_out;    // dlogits rows start 16-byte aligned (backward)
};

__device__ __forceinline__ bool ce_label_ok(int64_t label, int V) { return label >= 0 && label < (int64_t)V; }

// kLanes lanes (64: one wave; 256: the workgroup) own a row; a workgroup of 256 threads holds 256 / kLanes rows.
template <typename T, bool kSmooth, int kLanes>
__global__ __launch_bounds__(kCeThreads) void cross_entropy_fwd_kernel(const dimsum_cross_entropy_params_t p, const ce_flags_t fl) {
    constexpr int E = CePiece<T>::kElems;
    constexpr int kRowsPerWg = kCeThreads / kLanes;
    constexpr int kWaves = kLanes / kWave;
    __shared__ double s_s[kWaves];
    __shared__ float s_m[kWaves], s_t[kWaves];
    const int t = threadIdx.x % kLanes;
    const int64_t row = (int64_t)blockIdx.x * kRowsPerWg + threadIdx.x / kLanes;
    if (kLanes == kWave && row >= p.rows) return;           // whole waves leave; with kLanes == 256 every row of the grid exists
    const int V = (int)p.vocab;
    const T *x = reinterpret_cast<const T *>(p.logits_ptr) + row * p.logits_row_stride;
    const float scale = p.logit_scale;
    const int npieces = (V + E - 1) / E;

    ce_pair_t acc = {-INFINITY, 0.f};
    // label smoothing needs lse - mean(s): the mean is carried as c + mean(s - c) with c = s[0], so that its error scales with the spread of the
    // row, not with its offset (as in a sum of log-probabilities)
    const float c = kSmooth ? to_f32<T>(x[0]) * scale : 0.f;
    float tsum = 0.f;
    for (int p0 = t; p0 < npieces; p0 += kLanes * kCeUnroll) {
        float f[kCeUnroll][E];
#pragma unroll
        for (int u = 0; u < kCeUnroll; ++u) {
            const int pc = p0 + u * kLanes;
            if (pc < npieces) ce_load_piece<T>(x, pc, V, fl.vec_in, -INFINITY, f[u]);
        }
#pragma unroll
        for (int u = 0; u < kCeUnroll; ++u) {
            const int pc = p0 + u * kLanes;
            if (pc < npieces) {
                const bool whole = (pc + 1) * E <= V;
                float pm = -INFINITY;
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    f[u][e] = (whole || pc * E + e < V) ? f[u][e] * scale : -INFINITY;      // a negative scale must not turn the fill into +inf
                    pm = fmaxf(pm, f[u][e]);
                }
                const float m = fmaxf(acc.m, pm);
                const float ref = m == -INFINITY ? 0.f : m;
                float s = acc.s * fast_exp2((acc.m - ref) * kLog2e);
#pragma unroll
                for (int e = 0; e < E; ++e) s += fast_exp2((f[u][e] - ref) * kLog2e);
                acc.m = m;
                acc.s = s;
                if (kSmooth) {
#pragma unroll
                    for (int e = 0; e < E; ++e) tsum += (whole || pc * E + e < V) ? f[u][e] - c : 0.f;
                }
            }
        }
    }
    // ---- the wave's lanes, then the workgroup's waves ----
    ce_pair64_t tot = {acc.m, (double)acc.s};
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const ce_pair64_t other = {__shfl_xor(tot.m, o, kWave), __shfl_xor(tot.s, o, kWave)};
        tot = ce_combine(tot, other);
        if (kSmooth) tsum += __shfl_xor(tsum, o, kWave);
    }
    if (kWaves > 1) {
        const int wave = threadIdx.x >> 6;
        if ((threadIdx.x & (kWave - 1)) == 0) {
            s_m[wave] = tot.m;
            s_s[wave] = tot.s;
            s_t[wave] = tsum;
        }
        __syncthreads();
        if (threadIdx.x != 0) return;
        tot = {s_m[0], s_s[0]};
        tsum = s_t[0];
        for (int w = 1; w < kWaves; ++w) {
            tot = ce_combine(tot, ce_pair64_t{s_m[w], s_s[w]});
            tsum += s_t[w];
        }
    } else if (t != 0) {
        return;
    }
    // ---- one lane per row: the label's logit and the row's three results ----
    // lse = m + log(sum): the row's offset and the (small) log of the rescaled sum are never rounded into one fp32 number -- the loss is formed
    // from differences against m, and the backward gets lse in double, so that exp(s_v - lse) does not lose the bits the offset would cost
    const double lg64 = log(tot.s);                         // once per row
    const float lg = (float)lg64;
    acc.m = tot.m;
    const float lse = acc.m + lg;
    const float z = p.lse_square_scale * lse * lse;
    const int64_t label = reinterpret_cast<const int64_t *>(p.labels_ptr)[row];
    float loss, zl = z;
    if (label == p.ignore_index) {
        loss = 0.f;
        zl = 0.f;
    } else if (!ce_label_ok(label, V)) {
        loss = __uint_as_float(0x7fc00000u);
    } else {
        const float sl = to_f32<T>(x[label]) * scale;
        loss = (acc.m - sl) + lg;                            // differences first: each is exact to its own size
        if (kSmooth) loss = (1.f - p.label_smoothing) * loss + p.label_smoothing * (((acc.m - c) + lg) - tsum / (float)V);
        loss += z;
    }
    reinterpret_cast<float *>(p.loss_ptr)[row] = loss;
    reinterpret_cast<double *>(p.lse_ptr)[row] = (double)acc.m + lg64;
    if (p.z_loss_ptr) reinterpret_cast<float *>(p.z_loss_ptr)[row] = zl;
}

template <typename T, int kLanes>
__global__ __launch_bounds__(kCeThreads) void cross_entropy_bwd_kernel(const dimsum_cross_entropy_params_t p, const ce_flags_t fl) {
    constexpr int E = CePiece<T>::kElems;
    constexpr int kRowsPerWg = kCeThreads / kLanes;
    const int t = threadIdx.x % kLanes;
    const int64_t row = (int64_t)blockIdx.x * kRowsPerWg + threadIdx.x / kLanes;
    if (row >= p.rows) return;
    const int V = (int)p.vocab;
    const T *x = reinterpret_cast<const T *>(p.logits_ptr) + row * p.logits_row_stride;
    T *dx = reinterpret_cast<T *>(p.dlogits_ptr) + row * p.dlogits_row_stride;
    const int npieces = (V + E - 1) / E;
    const int64_t label = reinterpret_cast<const int64_t *>(p.labels_ptr)[row];
    const double lse64 = reinterpret_cast<const double *>(p.lse_ptr)[row];
    const float lse = (float)lse64;                             // lse64 = lse + lse_lo to 48 bits
    const float lse_lo = fabsf(lse) < INFINITY ? (float)(lse64 - (double)lse) : 0.f;
    // the row's three coefficients in double, rounded once: with the element's one fma and v_exp_f32 they are what the gradient's error is made of
    const double g64 = (double)reinterpret_cast<const float *>(p.dloss_ptr)[row * p.dloss_stride] * (double)p.logit_scale;
    const double ks64 = (double)p.label_smoothing / (double)V;
    const float scale = p.logit_scale;
    const bool ignored = label == p.ignore_index, bad = !ignored && !ce_label_ok(label, V);
    const float gk = (float)(g64 * (1.0 + 2.0 * (double)p.lse_square_scale * lse64));      // the z term's share rides on the softmax
    const float gs = (float)(g64 * ks64);
    // the label's element, kp p - (1 - eps) - eps / V, as kp (p - 1) + (2 zscale lse + eps - eps / V): where p is near 1 nothing of size 1 cancels
    const float gf = (float)g64, kpf = (float)(1.0 + 2.0 * (double)p.lse_square_scale * lse64);
    const float clab = (float)(2.0 * (double)p.lse_square_scale * lse64 + (double)p.label_smoothing - ks64);
    const int lab = ignored || bad ? -1 : (int)label;
    const float nan = __uint_as_float(0x7fc00000u);

    for (int p0 = t; p0 < npieces; p0 += kLanes * kCeUnroll) {
        float f[kCeUnroll][E];
        if (!ignored && !bad) {
#pragma unroll
            for (int u = 0; u < kCeUnroll; ++u) {
                const int pc = p0 + u * kLanes;
                if (pc < npieces) ce_load_piece<T>(x, pc, V, fl.vec_in, 0.f, f[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < kCeUnroll; ++u) {
            const int pc = p0 + u * kLanes;
            if (pc < npieces) {
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    float d;
                    if (ignored) {
                        d = 0.f;
                    } else if (bad) {
                        d = nan;
                    } else {
                        const float t = fmaf(f[u][e], scale, -lse) - lse_lo;                  // s_v - lse: exact where p is near 1
                        const float a = t * kLog2e;
                        // what the product and the fp32 constant round away (t = -inf, a logit of -inf: nothing)
                        const float a_lo = t > -INFINITY ? fmaf(t, kLog2e, -a) + t * kLog2eLo : 0.f;
                        const float ex = fast_exp2(a);
                        const float pr = fmaf(ex, a_lo * kLn2, ex);
                        d = fmaf(gk, pr, -gs);                                      // one rounding per element
                        if (pc * E + e == lab) d = gf * fmaf(kpf, expm1f(t), clab);
                    }
                    f[u][e] = d;
                }
                ce_store_piece<T>(dx, pc, V, fl.vec_out, f[u]);
            }
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------
template <typename T> static int launch_cross_entropy_fwd(const dimsum_cross_entropy_params_t &p, hipStream_t s) {
    ce_flags_t fl;
    fl.vec_in = ce_rows_aligned<T>(p.logits_ptr, p.rows, p.logits_row_stride);
    fl.vec_out = 0;
    const bool smooth = p.label_smoothing > 0.f;
    const dim3 block(kCeThreads);
    if (p.vocab > kCeWaveRowMax) {
        const dim3 grid((unsigned)p.rows);
        if (smooth) hipLaunchKernelGGL((cross_entropy_fwd_kernel<T, true, kCeThreads>), grid, block, 0, s, p, fl);
        else hipLaunchKernelGGL((cross_entropy_fwd_kernel<T, false, kCeThreads>), grid, block, 0, s, p, fl);
    } else {
        const dim3 grid((unsigned)((p.rows + kCeThreads / kWave - 1) / (kCeThreads / kWave)));
        if (smooth) hipLaunchKernelGGL((cross_entropy_fwd_kernel<T, true, kWave>), grid, block, 0, s, p, fl);
        else hipLaunchKernelGGL((cross_entropy_fwd_kernel<T, false, kWave>), grid, block, 0, s, p, fl);
    }
    return launch_status();
}

template <typename T> static int launch_cross_entropy_bwd(const dimsum_cross_entropy_params_t &p, hipStream_t s) {
    ce_flags_t fl;
    fl.vec_in = ce_rows_aligned<T>(p.logits_ptr, p.rows, p.logits_row_stride);
    fl.vec_out = ce_rows_aligned<T>(p.dlogits_ptr, p.rows, p.dlogits_row_stride);
    const dim3 block(kCeThreads);
    if (p.vocab > kCeWaveRowMax) {
        hipLaunchKernelGGL((cross_entropy_bwd_kernel<T, kCeThreads>), dim3((unsigned)p.rows), block, 0, s, p, fl);
    } else {
        const dim3 grid((unsigned)((p.rows + kCeThreads / kWave - 1) / (kCeThreads / kWave)));
        hipLaunchKernelGGL((cross_entropy_bwd_kernel<T, kWave>), grid, block, 0, s, p, fl);
    }
    return launch_status();
}

// the checks of both entries, in the documented order
static int ce_check(const dimsum_cross_entropy_params_t *p, bool bwd) {
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_cross_entropy_params_t)) return DIMSUM_ERR_ABI;
    if (!p->logits_ptr || !p->labels_ptr || !p->lse_ptr) return DIMSUM_ERR_NULL;
    if (bwd ? (!p->dloss_ptr || !p->dlogits_ptr) : !p->loss_ptr) return DIMSUM_ERR_NULL;
    if (p->rows < 1 || p->vocab < 1 || p->rows > 0x7fffffff || p->vocab > 0x7fffffff - 16) return DIMSUM_ERR_SHAPE;
    if (p->dtype < DIMSUM_F32 || p->dtype > DIMSUM_BF16) return DIMSUM_ERR_DTYPE;
    if (p->logits_row_stride < p->vocab) return DIMSUM_ERR_STRIDE;
    if (bwd) {
        if (p->dlogits_row_stride < p->vocab || p->dloss_stride < 0) return DIMSUM_ERR_STRIDE;
        // a lane writes the piece it has just read, so dlogits may BE logits (same base, same row stride); any other overlap lets one
        // row's gradient land on logits that another workgroup has yet to read
        const size_t ts = p->dtype == DIMSUM_F32 ? 4 : 2;
        const size_t in_bytes = (size_t)((p->rows - 1) * p->logits_row_stride + p->vocab) * ts;
        const size_t out_bytes = (size_t)((p->rows - 1) * p->dlogits_row_stride + p->vocab) * ts;
        const bool in_place = p->dlogits_ptr == p->logits_ptr && p->dlogits_row_stride == p->logits_row_stride;
        if (!in_place && ce_ranges_overlap(p->dlogits_ptr, out_bytes, p->logits_ptr, in_bytes)) return DIMSUM_ERR_ALIAS;
    }
    if (!(p->label_smoothing >= 0.f && p->label_smoothing < 1.f) || !std::isfinite(p->logit_scale) || !std::isfinite(p->lse_square_scale))
        return DIMSUM_ERR_UNSUPPORTED;
    return DIMSUM_OK;
}

}  // namespace dimsum

extern "C" int dimsum_cross_entropy_fwd(const dimsum_cross_entropy_params_t *p, void *stream) {
    using namespace dimsum;
    const int rc = ce_check(p, false);
    if (rc != DIMSUM_OK) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    switch (p->dtype) {
        case DIMSUM_F32: return launch_cross_entropy_fwd<float>(*p, s);
        case DIMSUM_F16: return launch_cross_entropy_fwd<__half>(*p, s);
        default: return launch_cross_entropy_fwd<__hip_bfloat16>(*p, s);
    }
}

extern "C" int dimsum_cross_entropy_bwd(const dimsum_cross_entropy_params_t *p, void *stream) {
    using namespace dimsum;
    const int rc = ce_check(p, true);
    if (rc != DIMSUM_OK) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    switch (p->dtype) {
        case DIMSUM_F32: return launch_cross_entropy_bwd<float>(*p, s);
        case DIMSUM_F16: return launch_cross_entropy_bwd<__half>(*p, s);
        default: return launch_cross_entropy_bwd<__hip_bfloat16>(*p, s);
    }
}
