// sample_logits.hip -- the token sampler of the decode loop for gfx950: one launch maps (rows, V) logits to one token id per row under
// top-k / top-p / temperature, drawing with a uniform number the CALLER supplies (utils/generation.py:sample's distribution, which there
// is topk + sort + softmax + cumsum + scatter + multinomial: about a dozen launches). Nothing here generates random numbers: the token is
// a pure function of (logits row, top_k, top_p, temperature, u). The semantics are stated in include/dimsum_hip.h.
//
// MI355X design: NO SORT. Every question the sampler asks of a row -- which token has rank k, at which rank the descending cumulative
// mass passes top_p, which index the inverse CDF lands on -- is a SELECTION, answered by an 8-bit radix descent over a 32-bit key:
//   * one histogram pass over the row per digit: 256 bins of (count, mass) of the elements in scope whose key starts with the digits chosen so
//     far; then one wave folds the bins from the top and picks the bin in which the target count / mass is reached.
//       top-k:  key = the order-preserving bit image of the logit, target = k (count).            4 / 3 / 2 digits for f32 / f16 / bf16
//       top-p:  the same key inside the top-k set, target = ceil(top_p * mass of that set).       (what the dtype's values can differ in)
//       ties:   the elements EQUAL to a threshold that only some of may stay are told apart by index: key = ~index, target = how many stay.
//       draw:   key = ~index inside the kept set, target = floor(u * Z) + 1 (mass): the inverse CDF in ascending vocabulary index. ceil(log256 V) digits.
//     A row of 50 280 f32 logits (201 KB) does not fit the LDS: every pass re-reads it (from L2 after the first) in 16-byte pieces.
//   * MASS IS AN INTEGER: w_v = exp2((l_v - max) * log2(e) / temperature), in [0, 1], is cut to 40 fractional bits, and every sum of
//     weights is a 64-bit integer sum (V < 2^31 terms of at most 2^40 stay below 2^63). Integer addition is associative, so the LDS
//     atomics that build the histograms -- integer atomics; there is no atomic on a floating-point value -- give the same bits in any
//     order: two launches are bit-identical, a row's token depends neither on `rows` nor on the row's place in the grid nor on the
//     alignment path, and the comparisons against top_p * Z and u * Z are exact integer comparisons. The only errors are the one of a
//     weight (the fp32 product and v_exp_f32: about (2 + |l_v - max| log2(e) / temperature) 2^-24 relative) and the cut (2^-40 absolute per
//     element): DESIGN.md section 3.16b.
//   * histogram contention: logits crowd into a few exponent bins, and 64 lanes adding to one LDS address serialise. Each bin therefore has
//     kCopies copies in different banks, lane l adds to copy l % kCopies, and the copies are summed (and zeroed for the next pass) before
//     the bins are folded.
//   * Mapping, as cross_entropy.hip: a row of more than 4096 elements has a 256-thread workgroup (32 copies per bin), a shorter one has
//     one WAVE, four rows per workgroup (8 copies per bin), so that many short rows fill the chip. The grid comes from the rows.
//   * Safety: the token written is amax (the row's argmax, in [0, V) by construction) unless the draw yields an index that is checked to be
//     below V. No input -- NaN, infinities, u outside [0, 1), any top_k / top_p -- makes the kernel write anything else.
#include "row_pieces.hpp"

#include <cmath>
#include <type_traits>

namespace dimsum {

typedef unsigned long long sl_u64;

constexpr int kSlThreads = 256;
constexpr int kSlWaveRowMax = 4096;     // V up to which a row is one wave's; above it, one workgroup's
constexpr int kSlUnroll = 4;            // pieces per lane in flight
constexpr int kSlBins = 256;
constexpr int kSlSlots = 8192;          // bins x copies of one workgroup: 32 KB of counts + 64 KB of masses
constexpr unsigned kSlNoCut = 0x7fffffffu;
constexpr unsigned kSlNone = 0xffffffffu;
constexpr int kSlFracBits = 40;         // of a weight

// NaN counts as -inf, -0 as +0 (torch ranks them equal)
__device__ __forceinline__ float sl_canon(float x) { return x != x ? -INFINITY : (x == 0.f ? 0.f : x); }
// a < b <=> key(a) < key(b)
__device__ __forceinline__ unsigned sl_key(float x) {
    const unsigned b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float sl_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// the weight of a logit as an integer of kSlFracBits fractional bits; the row's maximum weighs exactly 2^40. scale = log2(e) / temperature
__device__ __forceinline__ sl_u64 sl_weight(float x, float mx, float scale) {
#pragma clang fp contract(off)
    float e = x == mx ? 1.f : fast_exp2((x - mx) * scale);      // (inf - inf never forms; -inf and a scale of +inf give 0)
    e = fminf(fmaxf(e, 0.f), 1.f);
    const float t = e * 1048576.f;                              // exact
    const float hi = floorf(t);
    const float lo = (t - hi) * 1048576.f;                      // exact: t - hi has at most 24 - 1 significant bits below 1
    return ((sl_u64)(unsigned)hi << 20) + (sl_u64)(unsigned)lo;
}

// a prefix of the row in rank order (descending logit, ascending index among equals): everything above `key`, and of the elements equal
// to it those up to index icut
struct sl_cut_t { unsigned key, icut; };
__device__ __forceinline__ bool sl_kept(const sl_cut_t &c, unsigned key, unsigned idx) { return key > c.key || (key == c.key && idx <= c.icut); }

// what a descent finds: the selected key, the count and mass of the elements in scope above it, the count and mass of those equal to it, and
// the mass target it worked with. n == 0: nothing found (an empty scope).
struct sl_sel_t {
    unsigned key, above_c, n, pad;
    sl_u64 above_m, m, target;
};

// which elements a descent looks at and what it selects by
struct sl_query_t {
    sl_cut_t a, b;              // scope: inside both prefixes ...
    unsigned tie_key;           // ... and, when ties, equal to this key
    bool ties;
    bool by_index;              // the selection key is ~index (ascending index) instead of the logit's key
    bool by_mass;               // the target is a mass (frac of the scope's total), else the count k
    bool draw;                  // mass target floor(frac * total) + 1 instead of ceil(frac * total)
    int levels;                 // digits of the selection key that can differ
    unsigned k;
    float frac;
};

template <int kLanes> struct sl_smem_t {
    static constexpr int kRows = kSlThreads / kLanes;
    static constexpr int kCopies = kSlSlots / kSlBins / kRows;
    sl_u64 mass[kSlSlots];
    sl_u64 bin_m[kRows][kSlBins];
    sl_u64 red[kSlThreads / kWave];
    sl_sel_t res[kRows];
    unsigned cnt[kSlSlots];
    unsigned bin_c[kRows][kSlBins];
};

// the lanes that own a row meet: a workgroup barrier, or (one wave per row) an LDS fence -- a wave's LDS operations complete in order
template <int kLanes> __device__ __forceinline__ void sl_sync() {
    if (kLanes > kWave) {
        __syncthreads();
    } else {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
}

// t: the lane's index among the kLanes of its row; g: the row's index in the workgroup
template <typename T, int kLanes>
__device__ sl_sel_t sl_descend(const T *x, int V, bool vec, float mx, float scale, const sl_query_t q, sl_smem_t<kLanes> &sm, int t, int g) {
    constexpr int E = CePiece<T>::kElems;
    constexpr int kCopies = sl_smem_t<kLanes>::kCopies;
    unsigned *cnt = sm.cnt + g * (kSlBins * kCopies);
    sl_u64 *mass = sm.mass + g * (kSlBins * kCopies);
    const int npieces = (V + E - 1) / E;
    const int copy = t & (kCopies - 1);
    // the digits above the first one that can differ: none of a logit's key, all ones of ~index
    sl_u64 prefix = q.by_index ? (0xffffffffull >> (8 * q.levels)) : 0ull;
    sl_sel_t r = {0u, 0u, 0u, 0u, 0ull, 0ull, 0ull};
    for (int lv = 0; lv < q.levels; ++lv) {
        const int shift = q.by_index ? 8 * (q.levels - 1 - lv) : 24 - 8 * lv;
        // ---- histogram of this digit over the elements in scope under the prefix ----
        for (int p0 = t; p0 < npieces; p0 += kLanes * kSlUnroll) {
            float f[kSlUnroll][E];
#pragma unroll
            for (int u = 0; u < kSlUnroll; ++u) {
                const int pc = p0 + u * kLanes;
                if (pc < npieces) ce_load_piece<T>(x, pc, V, vec, -INFINITY, f[u]);
            }
#pragma unroll
            for (int u = 0; u < kSlUnroll; ++u) {
                const int pc = p0 + u * kLanes;
                if (pc < npieces) {
#pragma unroll
                    for (int e = 0; e < E; ++e) {
                        const unsigned idx = (unsigned)(pc * E + e);
                        const float xv = sl_canon(f[u][e]);
                        const unsigned key = sl_key(xv);
                        const unsigned sel = q.by_index ? ~idx : key;
                        const bool in = idx < (unsigned)V && sl_kept(q.a, key, idx) && sl_kept(q.b, key, idx) && (!q.ties || key == q.tie_key) &&
                                        ((sl_u64)sel >> (shift + 8)) == prefix;
                        if (in) {
                            const int slot = (int)((sel >> shift) & 255u) * kCopies + copy;
                            atomicAdd(&cnt[slot], 1u);
                            if (q.by_mass) atomicAdd(&mass[slot], sl_weight(xv, mx, scale));
                        }
                    }
                }
            }
        }
        sl_sync<kLanes>();
        // ---- the copies of a bin, read from different banks, summed and zeroed for the next pass ----
        for (int b = t; b < kSlBins; b += kLanes) {
            unsigned c = 0;
            sl_u64 m = 0;
#pragma unroll 8
            for (int j = 0; j < kCopies; ++j) {
                const int s = b * kCopies + ((j + b) & (kCopies - 1));
                c += cnt[s];
                m += mass[s];
                cnt[s] = 0u;
                mass[s] = 0ull;
            }
            sm.bin_c[g][b] = c;
            sm.bin_m[g][b] = m;
        }
        sl_sync<kLanes>();
        // ---- one wave folds the bins from the top: lane l holds bins 4 l .. 4 l + 3 ----
        if (t < kWave) {
            unsigned c[4], cs = 0;
            sl_u64 m[4], ms = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                c[j] = sm.bin_c[g][4 * t + j];
                m[j] = sm.bin_m[g][4 * t + j];
                cs += c[j];
                ms += m[j];
            }
            unsigned sc = cs;           // -> the sum over the lanes >= t
            sl_u64 sms = ms;
#pragma unroll
            for (int o = 1; o < kWave; o <<= 1) {
                const unsigned vc = __shfl_down(sc, o, kWave);
                const sl_u64 vm = __shfl_down(sms, o, kWave);
                if (t + o < kWave) {
                    sc += vc;
                    sms += vm;
                }
            }
            if (lv == 0 && q.by_mass) {             // the target from the scope's total mass, which this first histogram holds
                const sl_u64 total = __shfl(sms, 0, kWave);
                const double want = (double)q.frac * (double)total;
                sl_u64 target = q.draw ? (sl_u64)floor(want) + 1ull : (sl_u64)ceil(want);
                target = target < 1ull ? 1ull : target;
                r.target = target > total ? total : target;             // total == 0: nothing below satisfies 0 < target
            }
            if (t == 0) sm.res[g].n = 0u;
            unsigned ac = r.above_c + (sc - cs);    // above this lane's bins
            sl_u64 am = r.above_m + (sms - ms);
#pragma unroll
            for (int j = 3; j >= 0; --j) {
                const bool hit = q.by_mass ? (am < r.target && r.target <= am + m[j]) : (ac < q.k && q.k <= ac + c[j]);
                if (hit) sm.res[g] = sl_sel_t{(unsigned)(4 * t + j), ac, c[j], 0u, am, m[j], r.target};
                ac += c[j];
                am += m[j];
            }
        }
        sl_sync<kLanes>();
        r = sm.res[g];
        if (r.n == 0u) return r;
        prefix = (prefix << 8) | r.key;
    }
    r.key = (unsigned)prefix;
    if (!q.by_index && q.levels < 4) {          // the digits that follow from the sign: zeros of a positive value's key, ones of a negative one's
        const int low = 32 - 8 * q.levels;
        r.key = (r.key << low) | ((r.key >> (8 * q.levels - 1)) & 1u ? 0u : (1u << low) - 1u);
    }
    return r;
}

// the prefix that a descent by logit key selected -> a cut: `stay` of the r.n elements equal to the key stay, the lowest indices first
template <typename T, int kLanes>
__device__ sl_cut_t sl_cut_from(const T *x, int V, bool vec, const sl_sel_t &r, unsigned stay, const sl_cut_t &scope, int index_levels,
                                sl_smem_t<kLanes> &sm, int t, int g) {
    sl_cut_t c = {r.key, kSlNoCut};
    if (stay < r.n) {
        const sl_query_t q = {scope, {0u, kSlNoCut}, r.key, true, true, false, false, index_levels, stay, 0.f};
        const sl_sel_t s = sl_descend<T, kLanes>(x, V, vec, 0.f, 0.f, q, sm, t, g);
        if (s.n != 0u) c.icut = ~s.key;
    }
    return c;
}

struct sl_flags_t {
    int vec_in;         // logits rows start 16-byte aligned
    float scale;        // log2(e) / temperature
};

// kLanes lanes (64: one wave; 256: the workgroup) own a row; a workgroup of 256 threads holds 256 / kLanes rows.
template <typename T, int kLanes>
__global__ __launch_bounds__(kSlThreads) void sample_logits_kernel(const dimsum_sample_logits_params_t p, const sl_flags_t fl) {
    constexpr int E = CePiece<T>::kElems;
    constexpr int kRowsPerWg = kSlThreads / kLanes;
    constexpr int kWaves = kLanes / kWave;
    constexpr int kValueLevels = sizeof(T) == 4 ? 4 : (std::is_same<T, __half>::value ? 3 : 2);
    __shared__ sl_smem_t<kLanes> sm;
    const int t = threadIdx.x % kLanes, g = threadIdx.x / kLanes;
    const int64_t row = (int64_t)blockIdx.x * kRowsPerWg + g;
    if (kLanes == kWave && row >= p.rows) return;           // whole waves leave (they meet nobody: sl_sync is theirs alone)
    const int V = (int)p.vocab;
    const T *x = reinterpret_cast<const T *>(p.logits_ptr) + row * p.logits_row_stride;
    const int npieces = (V + E - 1) / E;
    const bool vec = fl.vec_in;

    constexpr int kCopies = sl_smem_t<kLanes>::kCopies;
    for (int s = t; s < kSlBins * kCopies; s += kLanes) {
        sm.cnt[g * (kSlBins * kCopies) + s] = 0u;
        sm.mass[g * (kSlBins * kCopies) + s] = 0ull;
    }

    // ---- pass 1: the maximum and its lowest index, as the largest (key, ~index) pair ----
    sl_u64 best = 0ull;
    for (int p0 = t; p0 < npieces; p0 += kLanes * kSlUnroll) {
        float f[kSlUnroll][E];
#pragma unroll
        for (int u = 0; u < kSlUnroll; ++u) {
            const int pc = p0 + u * kLanes;
            if (pc < npieces) ce_load_piece<T>(x, pc, V, vec, -INFINITY, f[u]);
        }
#pragma unroll
        for (int u = 0; u < kSlUnroll; ++u) {
            const int pc = p0 + u * kLanes;
            if (pc < npieces) {
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const unsigned idx = (unsigned)(pc * E + e);
                    const sl_u64 comp = ((sl_u64)sl_key(sl_canon(f[u][e])) << 32) | (sl_u64)(kSlNone - idx);
                    if (idx < (unsigned)V && comp > best) best = comp;
                }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const sl_u64 other = __shfl_xor(best, o, kWave);
        best = other > best ? other : best;
    }
    if (kWaves > 1) {
        if ((threadIdx.x & (kWave - 1)) == 0) sm.red[threadIdx.x >> 6] = best;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < kWaves; ++w) best = sm.red[w] > best ? sm.red[w] : best;
    } else {
        sl_sync<kLanes>();          // the zeroed histograms
    }
    const float mx = sl_unkey((unsigned)(best >> 32));
    const unsigned amax = min(kSlNone - (unsigned)best, (unsigned)(V - 1));
    unsigned token = amax;          // top_k == 1; a row without a finite logit (all keys equal: index 0); the fallback of everything below

    int64_t at = row;               // the row's place in u and in out_table
    if (p.row_index_ptr) {
        int64_t step = reinterpret_cast<const int64_t *>(p.row_index_ptr)[0];
        step = step < 0 ? 0 : (step >= p.table_steps ? p.table_steps - 1 : step);
        at = step * p.rows + row;
    }

    if (p.top_k != 1 && V > 1 && mx > -INFINITY) {
        const int index_levels = V <= 256 ? 1 : (V <= 65536 ? 2 : (V <= (1 << 24) ? 3 : 4));
        const sl_cut_t all = {0u, kSlNoCut};
        sl_cut_t cut_k = all, cut_p = all;
        if (p.top_k > 0 && p.top_k < V) {
            const sl_query_t q = {all, all, 0u, false, false, false, false, kValueLevels, (unsigned)p.top_k, 0.f};
            const sl_sel_t r = sl_descend<T, kLanes>(x, V, vec, mx, fl.scale, q, sm, t, g);
            if (r.n != 0u) cut_k = sl_cut_from<T, kLanes>(x, V, vec, r, (unsigned)p.top_k - r.above_c, all, index_levels, sm, t, g);
        }
        if (p.top_p > 0.f && p.top_p < 1.f) {
            const sl_query_t q = {cut_k, all, 0u, false, false, true, false, kValueLevels, 0u, p.top_p};
            const sl_sel_t r = sl_descend<T, kLanes>(x, V, vec, mx, fl.scale, q, sm, t, g);
            if (r.n != 0u) {
                // the r.n elements equal to the key weigh w each; the j-th of them (by index, from 0) stays iff above_m + j w < target
                const sl_u64 w = r.m / r.n, need = r.target - r.above_m;
                const sl_u64 stay = w == 0ull ? (sl_u64)r.n : (need + w - 1ull) / w;
                cut_p = sl_cut_from<T, kLanes>(x, V, vec, r, stay < (sl_u64)r.n ? (unsigned)stay : r.n, cut_k, index_levels, sm, t, g);
            }
        }
        float u = reinterpret_cast<const float *>(p.u_ptr)[at];
        u = fminf(fmaxf(u, 0.f), 0.99999994f);              // NaN -> 0; the largest float below 1
        const sl_query_t q = {cut_k, cut_p, 0u, false, true, true, true, index_levels, 0u, u};
        const sl_sel_t r = sl_descend<T, kLanes>(x, V, vec, mx, fl.scale, q, sm, t, g);
        if (r.n != 0u && ~r.key < (unsigned)V) token = ~r.key;
    }
    if (t == 0) {
        reinterpret_cast<int64_t *>(p.out_ptr)[row] = (int64_t)token;
        if (p.out_table_ptr) reinterpret_cast<int64_t *>(p.out_table_ptr)[at] = (int64_t)token;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------
template <typename T> static int launch_sample_logits(const dimsum_sample_logits_params_t &p, hipStream_t s) {
    sl_flags_t fl;
    fl.vec_in = ce_rows_aligned<T>(p.logits_ptr, p.rows, p.logits_row_stride);
    fl.scale = (float)(1.4426950408889634 / (double)p.temperature);
    const dim3 block(kSlThreads);
    if (p.vocab > kSlWaveRowMax) {
        hipLaunchKernelGGL((sample_logits_kernel<T, kSlThreads>), dim3((unsigned)p.rows), block, 0, s, p, fl);
    } else {
        const dim3 grid((unsigned)((p.rows + kSlThreads / kWave - 1) / (kSlThreads / kWave)));
        hipLaunchKernelGGL((sample_logits_kernel<T, kWave>), grid, block, 0, s, p, fl);
    }
    return launch_status();
}

// the checks, in the documented order
static int sl_check(const dimsum_sample_logits_params_t *p) {
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_sample_logits_params_t)) return DIMSUM_ERR_ABI;
    if (!p->logits_ptr || !p->out_ptr || (p->top_k != 1 && !p->u_ptr) || (p->out_table_ptr && !p->row_index_ptr)) return DIMSUM_ERR_NULL;
    if (p->dtype < DIMSUM_F32 || p->dtype > DIMSUM_BF16) return DIMSUM_ERR_DTYPE;
    if (p->rows < 1 || p->vocab < 1 || p->rows > 0x7fffffff || p->vocab > 0x7fffffff - 16) return DIMSUM_ERR_SHAPE;
    if (!(p->temperature > 0.f) || !std::isfinite(p->temperature)) return DIMSUM_ERR_SHAPE;
    if (p->row_index_ptr && (p->table_steps < 1 || p->table_steps > ((int64_t)1 << 40) / p->rows)) return DIMSUM_ERR_SHAPE;
    if (p->logits_row_stride < p->vocab) return DIMSUM_ERR_STRIDE;
    // a row's token is written while other rows are still read
    const size_t ts = p->dtype == DIMSUM_F32 ? 4 : 2;
    const size_t in_bytes = (size_t)((p->rows - 1) * p->logits_row_stride + p->vocab) * ts;
    if (ce_ranges_overlap(p->out_ptr, (size_t)p->rows * 8, p->logits_ptr, in_bytes)) return DIMSUM_ERR_ALIAS;
    if (p->out_table_ptr && ce_ranges_overlap(p->out_table_ptr, (size_t)(p->table_steps * p->rows) * 8, p->logits_ptr, in_bytes)) return DIMSUM_ERR_ALIAS;
    return DIMSUM_OK;
}

}  // namespace dimsum

extern "C" int dimsum_sample_logits(const dimsum_sample_logits_params_t *p, void *stream) {
    using namespace dimsum;
    const int rc = sl_check(p);
    if (rc != DIMSUM_OK) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    switch (p->dtype) {
        case DIMSUM_F32: return launch_sample_logits<float>(*p, s);
        case DIMSUM_F16: return launch_sample_logits<__half>(*p, s);
        default: return launch_sample_logits<__hip_bfloat16>(*p, s);
    }
}
