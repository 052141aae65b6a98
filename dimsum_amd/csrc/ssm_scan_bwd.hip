// ssm_scan_bwd.hip -- selective scan (Mamba S6) backward for gfx950.
//
// Replaces selective_scan_cuda.bwd (mamba/csrc/selective_scan/selective_scan.cpp:338-492; kernel
// selective_scan_bwd_kernel.cuh:75-489 + reverse_scan.cuh). With dt = softplus(delta + bias), a_t = exp(dt_t A),
// b_t = dt_t B_t u_t, h_t = a_t h_{t-1} + b_t, y_t = C_t.h_t + D u_t, out_z = y silu(z):
//     dy_t  = dout_t silu(z_t)                dz_t = dout_t y_t sig(z_t) (1 + z_t (1 - sig(z_t)))     (bwd_kernel.cuh:171-207)
//     dh_t  = e_{t+1} + C_t dy_t,  e_t = a_t dh_t   (reverse recurrence, carried as e = a dh: no seam bookkeeping)
//     dC_t[n] = sum_d dy_t h_t[n]             dB_t[n] = sum_d dh_t[n] dt_t u_t
//     dA[n]  += dh_t[n] dt_t (a_t h_{t-1})[n] = dt_t e_t[n] h_{t-1}[n]                                  (bwd_kernel.cuh:289)
//     ddt_t  = u_t s1_t + s2_t,  s1 = sum_n dh B,  s2 = sum_n A e_t h_{t-1};   ddelta = ddt * sigmoid(delta+bias)  (:439-452)
//     du_t   = dt_t s1_t + D dy_t             dD += dy_t u_t        ddelta_bias += ddelta_t
//
// MI355X design. lane = (channel, state quarter): a wave64 owns 16 channels of one batch element, DPP row q (16 lanes)
// carries states q dstate/4 .. of its channels; a workgroup is 4 waves = 64 consecutive channels. The sequence is walked
// BACKWARDS in registers. Instead of the reference's per-row block-wide forward + reverse parallel scans (about 3x the
// arithmetic, plus 1024-way global atomic contention on dB/dC):
//   * the state before every 8-step half tile comes from the forward kernel (ckpt_ptr; training callers keep it) or, for
//     callers with the reference's exact interface, from one extra state-only forward sweep into the workspace; a half's
//     states are requested one whole half (~1 us of VALU work) before they are needed;
//   * 32-step tiles (128-B row segments: every HBM line is fetched exactly once) are walked backwards as four 8-step
//     halves. With dstate 16 a lane's 4 states x 8 steps are ONE register sweep: the forward sweep keeps h_t AND
//     a_t = exp2(dt_t A) in 2 x 32 VGPRs, the reverse sweep runs over the same registers (dh_t a_t h_{t-1} = e_t h_{t-1}
//     with h_{t-1} still in its register: no division, no second v_exp_f32): 3 + 1 exp VALU ops per (t, n) forward, 7 backward. Nothing per-(t, n) touches memory;
//   * sums over the states of a channel (s1, s2) are lane-local over dstate/4 states, then a TRANSPOSED exchange over the
//     4 quarters (v_permlane32_swap, v_permlane16_swap: 12 swaps + 12 adds per half) leaves quarter q with the totals of
//     steps 2q, 2q+1 only -- so each lane finishes du / ddelta (softplus chain) for 2 of the 8 steps instead of all of them;
//   * dB / dC are sums over a wave's 16 channels = one DPP row: a TRANSPOSED butterfly inside each row -- 32 values per
//     lane go in, two fully reduced values per lane come out, in 4 levels of DPP adds (~2 VALU ops per value instead of ~8
//     for independent row reductions). The 4 waves of a workgroup collect their (n, t) sums of a tile in LDS, add them
//     there and store ONE partial per 64 channels, 16 B per lane; a second small kernel adds the dim/64 partials of a
//     (batch, group) in a fixed order. No atomics on dB / dC at all (the reference does 1024-way contended atomicAdds
//     per address, selective_scan_bwd_kernel.cuh:297-316) -> bitwise reproducible;
//   * B / C tiles are staged ONCE per workgroup (wave-uniform data of the 4 waves' common batch element) and read back as
//     ds_read_b128 whose address is uniform per DPP row; u, delta, dy tiles are per wave, XOR-swizzled like in the forward;
//     dz / out_z are computed in the coalesced load layout (16 B per lane in and out) and never touch LDS.
//     LDS: 4 x 11 KB + 4.6 KB per workgroup; two __syncthreads() per 32-step tile.
#include <type_traits>

#include "ssm_scan_host.hpp"

namespace dimsum {

#ifndef DIMSUM_SCAN_BWD_WAVES
#define DIMSUM_SCAN_BWD_WAVES 4
#endif
constexpr int kBW = DIMSUM_SCAN_BWD_WAVES;    // waves per workgroup
constexpr int kBC = 16;   // channels per wave (one DPP row per state quarter)
constexpr int kBQ = 4;    // lanes per channel
constexpr int kBT = 32;   // time steps per LDS tile (128 B per row and tensor: whole HBM lines)
constexpr int kBS = 8;    // time steps per register sweep (= distance of the saved states)
constexpr int kBCS = kBT + 4;   // row stride of the B / C tiles: rows dstate/4 apart (the 4 quarters of one read) on distinct banks
constexpr int kDS = kBT + 8;    // row stride of the per-wave dB / dC sums: the 4 rows one ds_write_b64 touches on distinct banks

// 16 rows x 32 columns fp32, row = 8 slots of 16 B, slots XOR-swizzled by (row >> 1) & 7: ds_write_b128 in the load
// layout (8 lanes = one row) and ds_read_b128 / b64 in the lane = row layout are both bank-conflict free, no padding
__device__ __forceinline__ int btile_off(int row, int col4) { return row * kBT + ((col4 ^ ((row >> 1) & 7)) << 2); }

template <typename T> __device__ __forceinline__ const T *at(const T *base, unsigned elem_off) {
    return reinterpret_cast<const T *>(reinterpret_cast<const char *>(base) + (unsigned)(elem_off * (unsigned)sizeof(T)));
}
template <typename T> __device__ __forceinline__ T *at(T *base, unsigned elem_off) {
    return reinterpret_cast<T *>(reinterpret_cast<char *>(base) + (unsigned)(elem_off * (unsigned)sizeof(T)));
}

__device__ __forceinline__ void swap32(float &x, float &y) {      // x.lanes 32-63 <-> y.lanes 0-31
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    x = __uint_as_float(r[0]); y = __uint_as_float(r[1]);
}
__device__ __forceinline__ void swap16(float &x, float &y) {      // x.odd rows <-> y.even rows
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    x = __uint_as_float(r[0]); y = __uint_as_float(r[1]);
}
template <int CTRL> __device__ __forceinline__ float dpp(float v) {
    return __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), CTRL, 0xF, 0xF, true));
}
// sum of v over the 4 quarter lanes of a channel, in all 4 of them
__device__ __forceinline__ float sum_quarters(float v) {
    float a = v, b = v;
    swap32(a, b);
    float r = a + b, c = r;
    swap16(r, c);
    return r + c;
}

// ---- transposed butterfly over one DPP row: NV values per lane in (gen(0) .. gen(NV-1)), NV / 16 fully reduced values per
// lane out. At every level a lane keeps the half of its values its lane bit selects and receives the partner's copy of
// that same half (the partner sends the half it does NOT keep). Pairings: l ^ 8 (row_ror:8), bit 2 (row_half_mirror:
// l <-> 7 - l inside each 8 lanes), l ^ 2, l ^ 1 (quad_perm). Result r[i] of row lane l is the sum over the row of value
//   NV = 32: 2 l + i (i = 0, 1)      NV = 16: l      NV = 8: l >> 1 (both lanes of a pair hold it).
// The first level is fused with the generation so that only 16 temporaries are ever live.
// one level: CNT values per lane in -> CNT / 2 out (a lane keeps the half its bit selects: `hi`); with a single value left
// the two lanes of a pair hold partial sums of the same value -> plain exchange + add
template <int CTRL, int CNT> __device__ __forceinline__ void reduce_level(float (&v)[16], bool hi) {
    if constexpr (CNT >= 2) {
#pragma unroll
        for (int i = 0; i < CNT / 2; ++i) v[i] = (hi ? v[i + CNT / 2] : v[i]) + dpp<CTRL>(hi ? v[i] : v[i + CNT / 2]);
    } else {
        v[0] += dpp<CTRL>(v[0]);
    }
}
template <int NV, typename Gen> __device__ __forceinline__ void transposed_reduce_row(Gen gen, int lane, float (&r)[2]) {
    static_assert(NV == 32 || NV == 16 || NV == 8, "");
    constexpr int M = NV / 2;                          // live values after the first level (fused with the generation)
    float v[16];
    {
        const bool hi = lane & 8;
#pragma unroll
        for (int i = 0; i < M; ++i) {
            const float a = gen(i), b = gen(i + M);
            v[i] = (hi ? b : a) + dpp<0x128>(hi ? a : b);                           // row_ror:8 pairs l <-> l ^ 8
        }
    }
    reduce_level<0x141, M>(v, lane & 4);               // row_half_mirror pairs l <-> 7 - l (bit 2 differs)
    reduce_level<0x4E, M / 2>(v, lane & 2);            // quad_perm [2,3,0,1] pairs l <-> l ^ 2
    reduce_level<0xB1, (M / 4 > 0 ? M / 4 : 1)>(v, lane & 1);   // quad_perm [1,0,3,2] pairs l <-> l ^ 1
    r[0] = v[0];
    r[1] = NV == 32 ? v[1] : 0.f;
}

// NV = 32 with the lanes' state slots permuted (kernel: slot j of row lane c holds state j ^ ((c >> 2) & 3)): at the two levels
// that split on the STATE bits every lane keeps its slots 0, 1 (then 0) and sends slots 2, 3 (then 1) -- the partner's sent
// slots hold exactly the states this lane keeps, because the partners' permutations differ in that bit. No selects at those
// levels (24 of the 30 outputs); the two time-bit levels are as above. Same result layout: r[i] = value 2 l + i.
template <typename Gen> __device__ __forceinline__ void transposed_reduce_row32_perm(Gen gen, int lane, float (&r)[2]) {
    float v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = gen(i) + dpp<0x128>(gen(i + 16));           // slots {0, 1} += partner's slots {2, 3}   (l ^ 8)
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] += dpp<0x141>(v[i + 8]);                       // slot 0 += partner's slot 1               (7 - l)
    reduce_level<0x4E, 8>(v, lane & 2);                                             // time bit 2
    reduce_level<0xB1, 4>(v, lane & 1);                                             // time bit 1
    r[0] = v[0];
    r[1] = v[1];
}

// The same for values that are PRODUCTS y[i & 7] * h[i] (dC). First level: both products of a pair are formed by their owner, then ONE
// v_add_f32 with a DPP source: v_mul, v_mul, v_add_dpp = 4 issue slots per output (a DPP operand costs a second slot). The round-3 form
// fma(dpp(h[i + 16]), dpp(y), y h[i]) looked shorter on paper, but v_fma has no DPP encoding on gfx9: it became v_mul + v_mov_dpp + v_fma
// (4 slots) plus 8 v_mov_dpp for the partner's y (16 slots per half). Contraction is off here: y h[i] + dpp(..) must stay an add.
__device__ __forceinline__ void transposed_reduce_row32_perm_prod(const float (&y)[8], const float (&h)[32], int lane, float (&r)[2]) {
#pragma clang fp contract(off)
    float v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = y[i & 7] * h[i] + dpp<0x128>(y[i & 7] * h[i + 16]);      // v_mul, v_mul, v_add_f32_dpp
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] += dpp<0x141>(v[i + 8]);
    reduce_level<0x4E, 8>(v, lane & 2);
    reduce_level<0xB1, 4>(v, lane & 1);
    r[0] = v[0];
    r[1] = v[1];
}

// dt = softplus(x) (the reference's threshold form, common.hpp softplus_ref) AND its slope sigmoid(x) = e^x / (1 + e^x) from the same
// exponential: one v_rcp_f32 next to the softplus instead of a second exponential + a series per step in the per-step epilogue
// (selective_scan_bwd_kernel.cuh:439-452 recomputes the softplus derivative there too). Without softplus: dt = x, slope 1.
// Straight-line code (the empty asm pins both forms: no per-element branch around the transcendentals).
__device__ __forceinline__ void softplus_and_slope(float x, bool flag, float &dt, float &slope) {
    const float e = fast_exp(x);
    const float w = 1.0f + e;
    float sp = fmaf(e - (w - 1.0f), fmaxf(2.0f - w, 0.0f), fast_log(w));
    float sg = e * fast_rcp(w);
    asm volatile("" : "+v"(sp), "+v"(sg));
    const bool big = x > 20.0f;             // the reference takes dt = x there, slope 1 (e / (1 + e) rounds to 1 from x = 17 on; e overflows at 88)
    dt = flag ? (big ? x : sp) : x;
    slope = flag ? (big ? 1.0f : sg) : 1.0f;
}

// kVec : every row base 4-element aligned and L % 4 == 0 -> 16-byte vector I/O.   kFull: all 64 channel slots are live.
// kRev : the time-reversed direction of the bidirectional scan (bimamba_inner_fn; forward: ssm_scan_fwd_kernel.hpp, kRev). The kernel runs in
//        reversed time t' = L - 1 - t -- so it walks ORIGINAL time forwards -- and only its global addresses are mirrored: a 4-step group t' ..
//        t' + 3 is the memory group L - 4 - t' .. L - 1 - t' with its elements swapped in registers. The saved states are indexed in reversed
//        time (as that forward kernel wrote them), the partial dB / dC too (the reduce kernel mirrors them). It ACCUMULATES: du, ddelta, dz and
//        the optional out_z are read, added to and stored (the forward direction's launch has written them), dA goes to the caller's dA_b.
template <typename T, int kN, bool kHasZ, bool kVec, bool kFull, bool kRev = false>
__global__ __launch_bounds__(kBW * kWave, 2) void ssm_scan_bwd_kernel(const ssm_bwd_args_t q, const float *__restrict__ ckpt, float *__restrict__ part) {
    static_assert(!kRev || kHasZ, "the bidirectional scan gates with z");
    constexpr int kNL = kN / kBQ;                 // states per lane
    constexpr int kBG = kNL < 4 ? kNL : 4;        // states per register sweep
    constexpr int NV = kBG * kBS;                 // (state, step) values per transposed reduction
    constexpr int kNG = kNL / kBG;                // register sweeps (state groups) per half tile: 1 up to dstate 16
    constexpr int kNPc = kBC / 8;                 // 16-byte pieces per lane of a 16 x 32 tile (a piece = 8 rows x 128 B)
    static_assert(kN % kBQ == 0 && kNL % kBG == 0 && (NV == 32 || NV == 16 || NV == 8), "dstate must be 4, 8, 16 or 32");
    const ssm_args_t &p = q.fwd;
    // ONE LDS block: [u | dt (softplus'ed) | dy] per wave, [a wave's dB | dC sums of the tile] per wave, [B | C] shared by the 4 waves.
    // The sweeps address it with byte offsets: the same per-lane offset serves u, dt and dy (constant distances = immediate offsets of
    // the ds instructions), and the 16-byte slot index of a half tile enters by one XOR (btile_off: the row bases have no bits below 128).
    constexpr int kTile = kBC * kBT, kSums = kN * kDS;
    constexpr unsigned kOffD = 4u * kBW * kTile, kOffY = 8u * kBW * kTile, kOffS = 12u * kBW * kTile;   // dt, dy, sigmoid tiles relative to the u tile (bytes)
    constexpr unsigned kOffB = 4u * (4 * kBW * kTile + 2 * kBW * kSums), kOffC = kOffB + 4u * kN * kBCS;   // B, C tiles (bytes)
    __shared__ __attribute__((aligned(16))) float smem[4 * kBW * kTile + 2 * kBW * kSums + 2 * kN * kBCS];
    float(*const sdB)[kSums] = reinterpret_cast<float(*)[kSums]>(smem + 4 * kBW * kTile);
    float(*const sdC)[kSums] = reinterpret_cast<float(*)[kSums]>(smem + 4 * kBW * kTile + kBW * kSums);
    float *const tB = smem + kOffB / 4, *const tC = smem + kOffC / 4;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & (kBC - 1), sh = lane >> 4;
    float *tU = smem + wave * kTile, *tD = tU + kBW * kTile, *tY = tD + kBW * kTile, *tS = tY + kBW * kTile, *tdB = sdB[wave], *tdC = sdC[wave];
    auto lds4 = [&](unsigned off) -> const f32x4 & { return *reinterpret_cast<const f32x4 *>(reinterpret_cast<const char *>(smem) + off); };
    const unsigned ubase = 4u * (unsigned)(wave * kTile + btile_off(c, 0));       // u4 of 4-step slot j of this lane's row: ubase ^ (j << 4)
    const int ns0 = sh * kNL;                     // first state of this lane
    const int L = p.seqlen;
    const int dpg = p.dim / p.n_groups;
    constexpr int kWC = kBW * kBC;                // channels per workgroup
    const int tiles_per_group = (dpg + kWC - 1) / kWC;
    const int tiles_per_batch = p.n_groups * tiles_per_group;
    int wg = blockIdx.x;
    const int nwg = gridDim.x;
    if ((nwg & 7) == 0) wg = (wg & 7) * (nwg >> 3) + (wg >> 3);      // a batch element's workgroups share an XCD (one L2 for B / C)
    const int b = wg / tiles_per_batch;
    const int rem = wg - b * tiles_per_batch;
    const int g = rem / tiles_per_group;
    const int d0 = g * dpg + (rem - g * tiles_per_group) * kWC + wave * kBC;        // first channel of this WAVE
    const int nd = kFull ? kBC : max(0, min(kBC, (g + 1) * dpg - d0));              // live channels of this wave (0: idle wave)
    const bool wave_live = kFull || nd > 0;
    const bool live = kFull || c < nd;
    const int d = kFull ? d0 + c : min(d0 + max(0, min(c, nd - 1)), p.dim - 1);      // (an idle wave's d0 may lie beyond dim: clamp its reads)

    const T *u_base = reinterpret_cast<const T *>(p.u_ptr) + (int64_t)b * p.u_batch_stride + (int64_t)d0 * p.u_d_stride;
    const T *dl_base = reinterpret_cast<const T *>(p.delta_ptr) + (int64_t)b * p.delta_batch_stride + (int64_t)d0 * p.delta_d_stride;
    const T *do_base = reinterpret_cast<const T *>(q.dout_ptr) + (int64_t)b * q.dout_batch_stride + (int64_t)d0 * q.dout_d_stride;
    const T *z_base = kHasZ ? reinterpret_cast<const T *>(p.z_ptr) + (int64_t)b * p.z_batch_stride + (int64_t)d0 * p.z_d_stride : nullptr;
    const T *y_base = kHasZ ? reinterpret_cast<const T *>(p.out_ptr) + (int64_t)b * p.out_batch_stride + (int64_t)d0 * p.out_d_stride : nullptr;
    T *oz_base = (kHasZ && p.out_z_ptr) ? reinterpret_cast<T *>(p.out_z_ptr) + (int64_t)b * p.out_z_batch_stride + (int64_t)d0 * p.out_z_d_stride : nullptr;
    T *dz_base = kHasZ ? reinterpret_cast<T *>(q.dz_ptr) + (int64_t)b * q.dz_batch_stride + (int64_t)d0 * q.dz_d_stride : nullptr;
    T *du_base = reinterpret_cast<T *>(q.du_ptr) + (int64_t)b * q.du_batch_stride + (int64_t)d0 * q.du_d_stride;
    T *dd_base = reinterpret_cast<T *>(q.ddelta_ptr) + (int64_t)b * q.ddelta_batch_stride + (int64_t)d0 * q.ddelta_d_stride;
    const T *Bp = reinterpret_cast<const T *>(p.B_ptr) + (int64_t)b * p.B_batch_stride + (int64_t)g * p.B_group_stride;
    const T *Cp = reinterpret_cast<const T *>(p.C_ptr) + (int64_t)b * p.C_batch_stride + (int64_t)g * p.C_group_stride;
    // partial sums of this workgroup: part[workgroup][dB | dC][n][L]
    float *pB = part + (int64_t)wg * 2 * kN * L, *pC = pB + (int64_t)kN * L;
    const int u_ds = (int)p.u_d_stride, dl_ds = (int)p.delta_d_stride, do_ds = (int)q.dout_d_stride, z_ds = (int)p.z_d_stride;
    const int y_ds = (int)p.out_d_stride, oz_ds = (int)p.out_z_d_stride, dz_ds = (int)q.dz_d_stride, du_ds = (int)q.du_d_stride;
    const int dd_ds = (int)q.ddelta_d_stride;
    const int Bns = (int)p.B_dstate_stride, Cns = (int)p.C_dstate_stride;

    // State slots: slot j of this lane holds state ns0 + (j ^ kperm). With one 4-state sweep per half (dstate 16) the slots are
    // permuted by the row lane's bits 3, 2 so that the dB / dC butterflies need no selects at their two state levels
    // (transposed_reduce_row32_perm); everything per-state below (A, saved states, B / C rows, dA) goes through `sidx`.
    constexpr bool kPerm = kNG == 1 && kBG == 4;
    const int kperm = kPerm ? ((c >> 2) & 3) : 0;
    int sidx[kNL], brow[kNL];                     // state index of slot j (relative to ns0); its row offset in tB / tC
#pragma unroll
    for (int k = 0; k < kNL; ++k) { sidx[k] = k ^ kperm; brow[k] = (ns0 + sidx[k]) * kBCS; }
    unsigned bbyte[kNL];                          // byte offset of slot k's B row in smem (C row: + kOffC - kOffB)
#pragma unroll
    for (int k = 0; k < kNL; ++k) bbyte[k] = kOffB + 4u * (unsigned)brow[k];
    // this lane's 2 steps of a half in the per-(d, t) epilogue: columns 2 q, 2 q + 1 of the half (q = sh)
    const unsigned ebase = ubase ^ ((unsigned)(sh >> 1) << 4) ^ ((unsigned)(sh & 1) << 3);
    const unsigned sums_base = 4u * (unsigned)((4 * kBW * kTile) + wave * kSums + (ns0 + (c >> 2)) * kDS + 2 * (c & 3));   // NV == 32 layout
    // per-lane constants and carries, all in registers (only ever indexed with compile-time constants)
    float A2[kNL], re[kNL], rdA[kNL];             // A log2 e; e = a_{t+1} dh_{t+1} carried across halves; dA accumulators
    {
        const float *Ap = reinterpret_cast<const float *>(p.A_ptr) + (int64_t)d * p.A_d_stride;
#pragma unroll
        for (int k = 0; k < kNL; ++k) { A2[k] = Ap[(ns0 + sidx[k]) * p.A_dstate_stride] * kLog2e; re[k] = 0.f; rdA[k] = 0.f; }   // exp(dt A) = exp2(dt A log2 e)
    }
    const float Dval = p.D_ptr ? reinterpret_cast<const float *>(p.D_ptr)[d] : 0.f;
    const float *bias_p = reinterpret_cast<const float *>(p.delta_bias_ptr);
    const bool softplus = p.delta_softplus != 0;
    float dD = 0.f, dbias = 0.f;                  // this lane's share (its 2 steps of every half)

    const int n_tiles = (L + kBT - 1) / kBT;
    const int n_halves = (L + kBS - 1) / kBS;
    // saved states: [b][half tile][n][d]
    const float *ck_lane = ckpt + (int64_t)b * n_halves * kN * p.dim + (int64_t)ns0 * p.dim + d;
    const int64_t ck_ns = p.dim;                                // stride between states
    // coalesced tile layout: 16 rows x 32 columns = 2 pieces of (8 rows x 8 lanes-per-row x 4 columns): whole 128-B lines
    const int lrow = lane >> 3, lc4 = lane & 7, lcol = lc4 * 4;
    float bias_row[kNPc];                                        // delta_bias of the rows this lane stages
#pragma unroll
    for (int i = 0; i < kNPc; ++i) bias_row[i] = (bias_p && wave_live) ? bias_p[d0 + min(i * 8 + lrow, nd - 1)] : 0.f;

    // states of the last half tile (the first one processed); later halves are prefetched one half ahead
    float hpre[kNL];
#pragma unroll
    for (int k = 0; k < kNL; ++k) hpre[k] = wave_live ? ck_lane[((int64_t)(n_halves - 1) * kN + sidx[k]) * ck_ns] : 0.f;

    // Register-staged prefetch (vector path): the next tile's delta rows -- the operand with the longest dependent chain behind
    // it (softplus) -- and its u rows are requested right after the current tile has been staged, so they fly under the tile's
    // sweeps (16 VGPRs; the kernel sits at 239 of the 256 that 2 waves per SIMD allow, no scratch). dout / z / out are requested
    // where they are staged. Branch-free: rows beyond nd are clamped to the last live row, columns beyond L to the last 4-column
    // group; the masks are applied when the registers are staged.
    Raw4<T> pu[kNPc], pd[kNPc], pg[kNPc], pz[kNPc], py[kNPc];
    auto gcol = [&](int c) { return kRev ? L - 4 - c : c; };            // 4-step group at (reversed) column c -> its first element in memory
    auto gidx = [&](int t) { return kRev ? L - 1 - t : t; };
    auto rv = [](f32x4 v) -> f32x4 {
        if constexpr (kRev) return {{v.v[3], v.v[2], v.v[1], v.v[0]}};
        else return v;
    };
    auto acc4 = [&](T *dst, f32x4 v) {                                  // store v (memory order), or add it to what is there
        if constexpr (kRev) {
            const f32x4 o = widen(ld4<T>(dst));
#pragma unroll
            for (int e = 0; e < 4; ++e) { asm volatile("" : "+v"(v.v[e])); v.v[e] = o.v[e] + v.v[e]; }   // (no fma into the add: o + round(v))
        }
        st4<T>(dst, v);
    };
    auto acc1 = [&](T &dst, float v) {
        if constexpr (kRev) asm volatile("" : "+v"(v));
        dst = from_f32<T>(kRev ? to_f32<T>(dst) + v : v);
    };
    auto tile_addr = [&](const T *base, int ds, int i, int col) -> const T * {
        if constexpr (kFull) return at(base + i * 8 * ds, (unsigned)(lrow * ds + col));
        else return at(base, (unsigned)(min(i * 8 + lrow, nd - 1) * ds + col));
    };
    auto issue_d = [&](int t0n) {
        const int col = gcol(min(t0n + lcol, L - 4));
#pragma unroll
        for (int i = 0; i < kNPc; ++i) { pd[i] = ld4<T>(tile_addr(dl_base, dl_ds, i, col)); pu[i] = ld4<T>(tile_addr(u_base, u_ds, i, col)); }
    };
    auto issue_rest = [&](int t0n) {
        const int col = gcol(min(t0n + lcol, L - 4));
#pragma unroll
        for (int i = 0; i < kNPc; ++i) {
            pg[i] = ld4<T>(tile_addr(do_base, do_ds, i, col));
            if constexpr (kHasZ) { pz[i] = ld4<T>(tile_addr(z_base, z_ds, i, col)); py[i] = ld4<T>(tile_addr(y_base, y_ds, i, col)); }
        }
    };
    if constexpr (kVec) if (wave_live) issue_d((n_tiles - 1) * kBT);

#pragma unroll 1
    for (int tile = n_tiles - 1; tile >= 0; --tile) {
        const int t0 = tile * kBT;
        // ---- B, C of the tile: staged once per workgroup (256 threads x 16 B = 64 rows of 32 steps) --------------------
        for (int idx = tid; idx < 2 * kN * (kBT / 4); idx += kBW * kWave) {
            const int which = idx >= kN * (kBT / 4), r = idx - which * kN * (kBT / 4), n = r >> 3, c4 = r & 7;
            const T *src = which ? Cp : Bp;
            const int ns = which ? Cns : Bns;
            f32x4 v = {{0.f, 0.f, 0.f, 0.f}};
            if constexpr (kVec) {
                if (t0 + c4 * 4 < L) v = rv(widen(ld4<T>(at(src, (unsigned)(n * ns + gcol(t0 + c4 * 4))))));
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (t0 + c4 * 4 + e < L) v.v[e] = to_f32<T>(src[(unsigned)(n * ns + gidx(t0 + c4 * 4 + e))]);
            }
            *reinterpret_cast<f32x4 *>(&(which ? tC : tB)[n * kBCS + c4 * 4]) = v;
        }
        if (wave_live) {
            // ---- stage u, dt = softplus(delta + bias) (0 beyond L and in dead rows: those steps / channels are identities:
            //      a = 1, b = 0, dy = 0 -> every term they feed into dB, dC, dA, s1, s2 is exactly 0) -------------------------
            if constexpr (kVec) {
                issue_rest(t0);
#pragma unroll
                for (int i = 0; i < kNPc; ++i) {
                    const int row = i * 8 + lrow;
                    f32x4 vu = {{0.f, 0.f, 0.f, 0.f}}, vd = {{0.f, 0.f, 0.f, 0.f}}, vs = {{0.f, 0.f, 0.f, 0.f}};
                    if ((kFull || row < nd) && t0 + lcol < L) {
                        vu = rv(widen(pu[i]));
                        vd = rv(widen(pd[i]));
#pragma unroll
                        for (int s = 0; s < 4; ++s) softplus_and_slope(vd.v[s] + bias_row[i], softplus, vd.v[s], vs.v[s]);
                    }
                    *reinterpret_cast<f32x4 *>(&tU[btile_off(row, lc4)]) = vu;
                    *reinterpret_cast<f32x4 *>(&tD[btile_off(row, lc4)]) = vd;
                    *reinterpret_cast<f32x4 *>(&tS[btile_off(row, lc4)]) = vs;
                }
                // ---- dy = dout * silu(z), dz, optional out_z -- in the coalesced layout; only dy goes to LDS ---------------
#pragma unroll
                for (int i = 0; i < kNPc; ++i) {
                    const int row = i * 8 + lrow;
                    f32x4 dy = {{0.f, 0.f, 0.f, 0.f}};
                    if ((kFull || row < nd) && t0 + lcol < L) {
                        const unsigned col = (unsigned)gcol(t0 + lcol);
                        const f32x4 go = widen(pg[i]);     // (memory order: dz / out_z are formed in it, dy is reordered below)
                        if constexpr (kHasZ) {
                            const f32x4 zv = widen(pz[i]);
                            const f32x4 yv = widen(py[i]);
                            f32x4 dz, oz;
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const float sgz = sigmoidf_fast(zv.v[e]), silu = zv.v[e] * sgz;
                                dz.v[e] = go.v[e] * yv.v[e] * sgz * (1.0f + zv.v[e] * (1.0f - sgz));
                                oz.v[e] = yv.v[e] * silu;
                                dy.v[e] = go.v[e] * silu;
                            }
                            acc4(at(dz_base + i * 8 * dz_ds, (unsigned)(lrow * dz_ds) + col), dz);
                            if (oz_base) acc4(at(oz_base + i * 8 * oz_ds, (unsigned)(lrow * oz_ds) + col), oz);
                        } else {
                            dy = go;
                        }
                    }
                    *reinterpret_cast<f32x4 *>(&tY[btile_off(row, lc4)]) = rv(dy);
                }
                if (tile > 0) issue_d(t0 - kBT);                 // flies under the sweeps below
            } else {
                for (int i = 0; i < kBC * kBT / kWave; ++i) {
                    const int idx = i * kWave + lane, row = idx / kBT, col = idx & (kBT - 1), t = gidx(t0 + col);
                    float vu = 0.f, vd = 0.f, dy = 0.f, vs = 0.f;
                    if (row < nd && t0 + col < L) {
                        vu = to_f32<T>(u_base[(unsigned)(row * u_ds + t)]);
                        softplus_and_slope(to_f32<T>(dl_base[(unsigned)(row * dl_ds + t)]) + (bias_p ? bias_p[d0 + row] : 0.f), softplus, vd, vs);
                        const float go = to_f32<T>(do_base[(unsigned)(row * do_ds + t)]);
                        if constexpr (kHasZ) {
                            const float zv = to_f32<T>(z_base[(unsigned)(row * z_ds + t)]), yv = to_f32<T>(y_base[(unsigned)(row * y_ds + t)]);
                            const float sgz = sigmoidf_fast(zv), silu = zv * sgz;
                            acc1(dz_base[(unsigned)(row * dz_ds + t)], go * yv * sgz * (1.0f + zv * (1.0f - sgz)));
                            if (oz_base) acc1(oz_base[(unsigned)(row * oz_ds + t)], yv * silu);
                            dy = go * silu;
                        } else {
                            dy = go;
                        }
                    }
                    tU[btile_off(row, col >> 2) + (col & 3)] = vu;
                    tD[btile_off(row, col >> 2) + (col & 3)] = vd;
                    tY[btile_off(row, col >> 2) + (col & 3)] = dy;
                    tS[btile_off(row, col >> 2) + (col & 3)] = vs;
                }
            }
        }
        __syncthreads();                                         // B / C of the tile are in place (and, from the previous tile:
                                                                 // every wave is done adding up the 4 waves' dB / dC sums)
        if (wave_live) {
#pragma unroll 1
            for (int half = kBT / kBS - 1; half >= 0; --half) {
                const int hidx = tile * (kBT / kBS) + half;      // index of this half tile's saved state
                const int jb = half * (kBS / 4);                 // first 4-step slot of the half
                if (hidx >= n_halves) {                          // a trailing half entirely beyond L: its sums are zero
                    for (int i = lane; i < kN * kBS; i += kWave) { tdB[(i >> 3) * kDS + half * kBS + (i & 7)] = 0.f; tdC[(i >> 3) * kDS + half * kBS + (i & 7)] = 0.f; }
                    continue;
                }
                // the states of the NEXT half (one earlier in time) are requested now, a whole half of VALU work ahead of their use
                float hnext[kNL];
                {
                    const float *ck_next = ck_lane + (int64_t)max(hidx - 1, 0) * kN * ck_ns;
#pragma unroll
                    for (int k = 0; k < kNL; ++k) hnext[k] = ck_next[sidx[k] * ck_ns];
                }
                float s1[kBS], s2[kBS];
#pragma unroll
                for (int t = 0; t < kBS; ++t) { s1[t] = 0.f; s2[t] = 0.f; }
                // byte offsets of the half's two 4-step slots of this lane's u row (dt: + kOffD, dy: + kOffY) and of its B rows
                const unsigned hx = (unsigned)half << 5;
                const unsigned uo[2] = {ubase ^ hx, ubase ^ (hx | 16u)};
                static_assert(kBS == 8, "two 4-step slots per half");
                unsigned bb[kNL];
#pragma unroll
                for (int k = 0; k < kNL; ++k) bb[k] = bbyte[k] + hx;

                // one register sweep over kBG states x kBS steps per iteration (ONE iteration up to dstate 16). With two groups
                // (dstate 32) the loop stays rolled: one copy of the body, uniform selects on statically indexed register arrays
                // (a dynamically indexed private array would live in scratch memory).
#pragma unroll 1
                for (int G = 0; G < kNG; ++G) {
                    const int n0 = G * kBG;                   // first state (lane-local) of the group
                    float H[kBG * kBS];                       // [k][t]: h_t of state n0+k, later overwritten by the dB terms
                    float AE[kBG * kBS];                      // [k][t]: a_t = exp2(dt_t A)
                    float hk[kBG], ek[kBG], dAk[kBG], Ak[kBG];
#pragma unroll
                    for (int k = 0; k < kBG; ++k) {
                        hk[k] = hpre[k]; ek[k] = re[k]; dAk[k] = rdA[k]; Ak[k] = A2[k];
#pragma unroll
                        for (int gq = 1; gq < kNG; ++gq) {
                            hk[k] = (G == gq) ? hpre[gq * kBG + k] : hk[k];
                            ek[k] = (G == gq) ? re[gq * kBG + k] : ek[k];
                            dAk[k] = (G == gq) ? rdA[gq * kBG + k] : dAk[k];
                            Ak[k] = (G == gq) ? A2[gq * kBG + k] : Ak[k];
                        }
                    }
                    float hin[kBG];                           // h before the half's first step (the reverse sweep's h_{t-1} at t = 0)
#pragma unroll
                    for (int k = 0; k < kBG; ++k) hin[k] = hk[k];
                    const int nrow = ns0 + n0;                // row of the group's first state in tB / tC / tdB / tdC
                    // ---- forward sweep: h_t, a_t for the 8 steps of the half ---------------------------------------------------
#pragma unroll
                    for (int jj = 0; jj < kBS / 4; ++jj) {
                        const f32x4 u4 = lds4(uo[jj]);
                        const f32x4 d4 = lds4(uo[jj] + kOffD);
                        float du[4];
#pragma unroll
                        for (int s = 0; s < 4; ++s) du[s] = d4.v[s] * u4.v[s];
#pragma unroll
                        for (int k = 0; k < kBG; ++k) {
                            const f32x4 bq = kPerm ? lds4(bb[k] + 16u * jj) : *reinterpret_cast<const f32x4 *>(&tB[(nrow + k) * kBCS + (jb + jj) * 4]);
#pragma unroll
                            for (int s = 0; s < 4; ++s) {
                                const float a = fast_exp2(d4.v[s] * Ak[k]);
                                hk[k] = fmaf(a, hk[k], bq.v[s] * du[s]);
                                H[k * kBS + jj * 4 + s] = hk[k];
                                AE[k * kBS + jj * 4 + s] = a;
                            }
                        }
                    }
                    // ---- dC[n, t] = sum_d dy_t h_t[n]: transposed reduction of the (k, t) products over the row's 16 channels ----
                    {
                        float y8[kBS];
#pragma unroll
                        for (int jj = 0; jj < kBS / 4; ++jj) {
                            const f32x4 y4 = lds4(uo[jj] + kOffY);
#pragma unroll
                            for (int s = 0; s < 4; ++s) y8[jj * 4 + s] = y4.v[s];
                        }
                        float r[2];
                        if constexpr (kPerm) transposed_reduce_row32_perm_prod(y8, H, lane, r);
                        else transposed_reduce_row<NV>([&](int i) { return y8[i & (kBS - 1)] * H[i]; }, lane, r);
                        if constexpr (NV == 32) {
                            if constexpr (kPerm) *reinterpret_cast<float2 *>(reinterpret_cast<char *>(smem) + (sums_base + 4u * kBW * kSums + hx)) = make_float2(r[0], r[1]);
                            else *reinterpret_cast<float2 *>(&tdC[(nrow + (c >> 2)) * kDS + half * kBS + 2 * (c & 3)]) = make_float2(r[0], r[1]);
                        } else if constexpr (NV == 16) {
                            tdC[(nrow + (c >> 3)) * kDS + half * kBS + (c & 7)] = r[0];
                        } else {
                            if ((c & 1) == 0) tdC[nrow * kDS + half * kBS + (c >> 1)] = r[0];
                        }
                    }
                    // ---- reverse sweep ---------------------------------------------------------------------------------------------
#pragma unroll
                    for (int jj = kBS / 4 - 1; jj >= 0; --jj) {
                        const f32x4 u4 = lds4(uo[jj]);
                        const f32x4 d4 = lds4(uo[jj] + kOffD);
                        const f32x4 y4 = lds4(uo[jj] + kOffY);
                        float du[4];
#pragma unroll
                        for (int s = 0; s < 4; ++s) du[s] = d4.v[s] * u4.v[s];
#pragma unroll
                        for (int k = 0; k < kBG; ++k) {
                            const f32x4 bq = kPerm ? lds4(bb[k] + 16u * jj) : *reinterpret_cast<const f32x4 *>(&tB[(nrow + k) * kBCS + (jb + jj) * 4]);
                            const f32x4 cq = kPerm ? lds4(bb[k] + 16u * jj + (kOffC - kOffB)) : *reinterpret_cast<const f32x4 *>(&tC[(nrow + k) * kBCS + (jb + jj) * 4]);
#pragma unroll
                            for (int s = 3; s >= 0; --s) {
                                const int t = jj * 4 + s;
                                const float dhn = fmaf(cq.v[s], y4.v[s], ek[k]);            // dh_t = a_{t+1} dh_{t+1} + C_t dy_t
                                ek[k] = AE[k * kBS + t] * dhn;                              // e_t = a_t dh_t
                                // dh_t (a_t h_{t-1}) = e_t h_{t-1}: h_{t-1} still sits in H (the sweep runs backwards), no h_t - b_t
                                const float gterm = ek[k] * (t == 0 ? hin[k] : H[k * kBS + (t > 0 ? t - 1 : 0)]);
                                dAk[k] = fmaf(gterm, d4.v[s], dAk[k]);
                                s2[t] = fmaf(gterm, Ak[k], s2[t]);
                                s1[t] = fmaf(dhn, bq.v[s], s1[t]);
                                H[k * kBS + t] = dhn * du[s];                               // dB term
                            }
                        }
                    }
#pragma unroll
                    for (int gq = 0; gq < kNG; ++gq)
#pragma unroll
                        for (int k = 0; k < kBG; ++k) {
                            re[gq * kBG + k] = (G == gq) ? ek[k] : re[gq * kBG + k];
                            rdA[gq * kBG + k] = (G == gq) ? dAk[k] : rdA[gq * kBG + k];
                        }
                    // ---- dB[n, t] = sum_d dh_t[n] dt_t u_t ---------------------------------------------------------------------------
                    {
                        float r[2];
                        if constexpr (kPerm) transposed_reduce_row32_perm([&](int i) { return H[i]; }, lane, r);
                        else transposed_reduce_row<NV>([&](int i) { return H[i]; }, lane, r);
                        if constexpr (NV == 32) {
                            if constexpr (kPerm) *reinterpret_cast<float2 *>(reinterpret_cast<char *>(smem) + (sums_base + hx)) = make_float2(r[0], r[1]);
                            else *reinterpret_cast<float2 *>(&tdB[(nrow + (c >> 2)) * kDS + half * kBS + 2 * (c & 3)]) = make_float2(r[0], r[1]);
                        } else if constexpr (NV == 16) {
                            tdB[(nrow + (c >> 3)) * kDS + half * kBS + (c & 7)] = r[0];
                        } else {
                            if ((c & 1) == 0) tdB[nrow * kDS + half * kBS + (c >> 1)] = r[0];
                        }
                    }
                }
#pragma unroll
                for (int k = 0; k < kNL; ++k) hpre[k] = hnext[k];

                // ---- per-(d, t) results of the half. The 4 lanes of a channel hold sums over their own states. Value 4 q' + j of
                //      the transposed exchange = (P, Q, P, Q)[j] of steps 2 q' + (j >> 1), with P = s1 and Q = ddt = u s1 + s2 (both
                //      linear in the per-lane partials): quarter q' ends up with the channel totals of exactly those four.
                //      (s2 was accumulated with A * log2 e) -------------------------------------------------------------------------
                float z4[4];
                {
                    float val[16];
#pragma unroll
                    for (int jj = 0; jj < kBS / 4; ++jj) {
                        const f32x4 u4 = lds4(uo[jj]);
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
                            const int t = jj * 4 + s;
                            val[2 * t] = s1[t];
                            val[2 * t + 1] = fmaf(u4.v[s], s1[t], s2[t] * kLn2);
                        }
                    }
                    float w[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) { float x = val[j], y = val[j + 8]; swap32(x, y); w[j] = x + y; }   // rows 0, 1 keep val[j], rows 2, 3 val[j + 8]
#pragma unroll
                    for (int j = 0; j < 4; ++j) { float x = w[j], y = w[j + 4]; swap16(x, y); z4[j] = x + y; }      // even rows keep w[j], odd rows w[j + 4]
                }
                {
                    char *const eo = reinterpret_cast<char *>(smem) + (ebase ^ hx);      // columns half * 8 + 2 q, + 1 of row c
                    const float2 u2 = *reinterpret_cast<const float2 *>(eo);
                    const float2 d2 = *reinterpret_cast<const float2 *>(eo + kOffD);
                    const float2 y2 = *reinterpret_cast<const float2 *>(eo + kOffY);
                    // d softplus / d delta = sigmoid(delta + bias), formed where the softplus was (staging: its exp is at hand there); 1 without
                    // softplus; dead steps (t >= L) and dead rows carry 0 (they have u = dy = 0 -> ddt = 0 anyway)
                    const float2 sg2 = *reinterpret_cast<const float2 *>(eo + kOffS);
                    const float du0 = fmaf(d2.x, z4[0], Dval * y2.x), du1 = fmaf(d2.y, z4[2], Dval * y2.y);
                    const float dd0 = z4[1] * sg2.x, dd1 = z4[3] * sg2.y;
                    dD = fmaf(y2.x, u2.x, fmaf(y2.y, u2.y, dD));
                    dbias += dd0 + dd1;
                    *reinterpret_cast<float2 *>(eo) = make_float2(du0, du1);
                    *reinterpret_cast<float2 *>(eo + kOffY) = make_float2(dd0, dd1);
                }
            }

            // ---- coalesced stores of du, ddelta ---------------------------------------------------------------------------
            if constexpr (kVec) {
#pragma unroll
                for (int i = 0; i < kNPc; ++i) {
                    const int row = i * 8 + lrow;
                    const f32x4 a = *reinterpret_cast<const f32x4 *>(&tU[btile_off(row, lc4)]);
                    const f32x4 cv = *reinterpret_cast<const f32x4 *>(&tY[btile_off(row, lc4)]);
                    if ((kFull || row < nd) && t0 + lcol < L) {
                        acc4(at(du_base + i * 8 * du_ds, (unsigned)(lrow * du_ds + gcol(t0 + lcol))), rv(a));
                        acc4(at(dd_base + i * 8 * dd_ds, (unsigned)(lrow * dd_ds + gcol(t0 + lcol))), rv(cv));
                    }
                }
            } else {
                for (int i = 0; i < kBC * kBT / kWave; ++i) {
                    const int idx = i * kWave + lane, row = idx / kBT, col = idx & (kBT - 1), t = gidx(t0 + col);
                    if (row < nd && t0 + col < L) {
                        acc1(du_base[(unsigned)(row * du_ds + t)], tU[btile_off(row, col >> 2) + (col & 3)]);
                        acc1(dd_base[(unsigned)(row * dd_ds + t)], tY[btile_off(row, col >> 2) + (col & 3)]);
                    }
                }
            }
        } else {
            for (int i = lane; i < kN * kBT; i += kWave) { tdB[(i >> 5) * kDS + (i & 31)] = 0.f; tdC[(i >> 5) * kDS + (i & 31)] = 0.f; }   // idle wave: zero sums
        }
        __syncthreads();                                         // the 4 waves' dB / dC sums of the tile are complete
        // ---- this workgroup's partial dB / dC of the tile: 4 waves added in a fixed order, 16 B per lane, rows of 128 B ----
        for (int idx = tid; idx < 2 * kN * (kBT / 4); idx += kBW * kWave) {
            const int which = idx >= kN * (kBT / 4), r = idx - which * kN * (kBT / 4), n = r >> 3, cc = (r & 7) * 4, t = t0 + cc;
            f32x4 acc = *reinterpret_cast<const f32x4 *>(&(which ? sdC : sdB)[0][n * kDS + cc]);
#pragma unroll
            for (int w = 1; w < kBW; ++w) {
                const f32x4 v = *reinterpret_cast<const f32x4 *>(&(which ? sdC : sdB)[w][n * kDS + cc]);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc.v[e] += v.v[e];
            }
            float *dst = (which ? pC : pB) + (int64_t)n * L + t;
            if (t + 3 < L && (L & 3) == 0) {
                st4<float>(dst, acc);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (t + e < L) dst[e] = acc.v[e];
            }
        }
    }

    // dD, ddelta_bias: every quarter lane holds its 2 steps' share -> channel total in all 4, written by quarter 0
    dD = sum_quarters(dD);
    dbias = sum_quarters(dbias);
    if (live) {
        float *dAp = reinterpret_cast<float *>(q.dA_ptr) + (int64_t)d * q.dA_d_stride;
#pragma unroll
        for (int k = 0; k < kNL; ++k) atomicAdd(dAp + (ns0 + sidx[k]) * q.dA_dstate_stride, rdA[k]);
        if (q.dD_ptr && sh == 0) atomicAdd(reinterpret_cast<float *>(q.dD_ptr) + d, dD);
        if (q.ddelta_bias_ptr && sh == 0) atomicAdd(reinterpret_cast<float *>(q.ddelta_bias_ptr) + d, dbias);
    }
}

// dB[b, g, n, t] = sum over the workgroups w of (b, g), in index order, of part[b, g, w][0][n][t]  (same for dC).
// One thread owns 4 consecutive steps (16-byte loads when L % 4 == 0); the partial rows of a (b, g) are 2 N L floats apart.
// kRev: the partials of the reversed direction (indexed in reversed time) are mirrored into dB / dC and ADDED to what is there.
template <bool kVec4, bool kRev = false>
__global__ __launch_bounds__(256) void ssm_scan_bwd_reduce_kernel(const float *__restrict__ part, const ssm_bwd_args_t q, int waves_per_group) {
    const ssm_args_t &p = q.fwd;
    const int L = p.seqlen, N = p.dstate, L4 = (L + 3) / 4;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;          // over (b, g, which, n, t / 4)
    const int64_t total = (int64_t)p.batch * p.n_groups * 2 * N * L4;
    if (i >= total) return;
    const int t = (int)(i % L4) * 4;
    int64_t r = i / L4;
    const int n = (int)(r % N); r /= N;
    const int which = (int)(r & 1); r >>= 1;
    const int g = (int)(r % p.n_groups);
    const int b = (int)(r / p.n_groups);
    const float *src = part + (((int64_t)(b * p.n_groups + g) * waves_per_group) * 2 + which) * N * L + (int64_t)n * L + t;
    const int64_t ws = (int64_t)2 * N * L;
    float *dst = which == 0 ? reinterpret_cast<float *>(q.dB_ptr) + (int64_t)b * q.dB_batch_stride + (int64_t)g * q.dB_group_stride + (int64_t)n * q.dB_dstate_stride
                            : reinterpret_cast<float *>(q.dC_ptr) + (int64_t)b * q.dC_batch_stride + (int64_t)g * q.dC_group_stride + (int64_t)n * q.dC_dstate_stride;
    if constexpr (!kRev) dst += t;
    if constexpr (kVec4) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        int w = 0;
        for (; w + 4 <= waves_per_group; w += 4) {       // 4 independent 16-byte loads in flight per thread
            const float4 v0 = *reinterpret_cast<const float4 *>(src + (int64_t)w * ws), v1 = *reinterpret_cast<const float4 *>(src + (int64_t)(w + 1) * ws);
            const float4 v2 = *reinterpret_cast<const float4 *>(src + (int64_t)(w + 2) * ws), v3 = *reinterpret_cast<const float4 *>(src + (int64_t)(w + 3) * ws);
            acc.x = (((acc.x + v0.x) + v1.x) + v2.x) + v3.x; acc.y = (((acc.y + v0.y) + v1.y) + v2.y) + v3.y;
            acc.z = (((acc.z + v0.z) + v1.z) + v2.z) + v3.z; acc.w = (((acc.w + v0.w) + v1.w) + v2.w) + v3.w;
        }
        for (; w < waves_per_group; ++w) {
            const float4 v = *reinterpret_cast<const float4 *>(src + (int64_t)w * ws);
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
        if constexpr (kRev) {
            float4 *d4 = reinterpret_cast<float4 *>(dst + (L - 4 - t));
            const float4 o = *d4;
            *d4 = make_float4(o.x + acc.w, o.y + acc.z, o.z + acc.y, o.w + acc.x);
        } else {
            *reinterpret_cast<float4 *>(dst) = acc;
        }
    } else {
        for (int e = 0; e < 4 && t + e < L; ++e) {
            float acc = 0.f;
            for (int w = 0; w < waves_per_group; ++w) acc += src[(int64_t)w * ws + e];
            if constexpr (kRev) dst[L - 1 - (t + e)] += acc;
            else dst[e] = acc;
        }
    }
}

// ev0: recorded at the begin of the main kernel unless the state-rebuild sweep of this call already took it (then null)
// kRev: the reversed, accumulating direction of the bidirectional backward (z given)
template <typename T, int kN, bool kRev = false>
static int launch_bwd(const ssm_bwd_args_t &q, const float *ckpt, float *part, hipStream_t stream, hipEvent_t ev0) {
    const ssm_args_t &p = q.fwd;
    const int dpg = p.dim / p.n_groups;
    constexpr int kWC = kBW * kBC;            // channels per workgroup
    const int tiles = p.batch * p.n_groups * ((dpg + kWC - 1) / kWC);
    bool vec = (p.seqlen % 4 == 0) && ssm_vec4_ok<T>(p.u_ptr, p.u_batch_stride, p.u_d_stride) && ssm_vec4_ok<T>(p.delta_ptr, p.delta_batch_stride, p.delta_d_stride) &&
               ssm_vec4_ok<T>(q.dout_ptr, q.dout_batch_stride, q.dout_d_stride) && ssm_vec4_ok<T>(q.du_ptr, q.du_batch_stride, q.du_d_stride) &&
               ssm_vec4_ok<T>(q.ddelta_ptr, q.ddelta_batch_stride, q.ddelta_d_stride) &&
               ssm_vec4_ok<T>(p.B_ptr, p.B_batch_stride, p.B_dstate_stride) && ssm_vec4_ok<T>(p.C_ptr, p.C_batch_stride, p.C_dstate_stride) &&
               p.B_group_stride % 4 == 0 && p.C_group_stride % 4 == 0;
    if (p.z_ptr) {
        vec = vec && ssm_vec4_ok<T>(p.z_ptr, p.z_batch_stride, p.z_d_stride) && ssm_vec4_ok<T>(p.out_ptr, p.out_batch_stride, p.out_d_stride) &&
              ssm_vec4_ok<T>(q.dz_ptr, q.dz_batch_stride, q.dz_d_stride);
        if (p.out_z_ptr) vec = vec && ssm_vec4_ok<T>(p.out_z_ptr, p.out_z_batch_stride, p.out_z_d_stride);
    }
    // in-tile offsets are 32-bit BYTE offsets (saddr + voffset addressing), see offsets_fit_32bit()
    if (!offsets_fit_32bit<T>(p.seqlen, kBC, {p.u_d_stride, p.delta_d_stride, q.dout_d_stride, q.du_d_stride, q.ddelta_d_stride,
                                              p.z_ptr ? p.z_d_stride : 0, p.z_ptr ? p.out_d_stride : 0, p.z_ptr ? q.dz_d_stride : 0,
                                              (p.z_ptr && p.out_z_ptr) ? p.out_z_d_stride : 0}) ||
        !offsets_fit_32bit<T>(p.seqlen, p.dstate, {p.B_dstate_stride, p.C_dstate_stride}))
        return DIMSUM_ERR_STRIDE;
    const bool full = vec && (dpg % kWC == 0);
    dim3 grid(tiles), block(kBW * kWave);
    const hipEvent_t ev1 = reinterpret_cast<hipEvent_t>(p.timing_stop_event), none = nullptr;   // end of the reduce kernel
#define DIMSUM_LAUNCH(HASZ, VEC, FULL) \
    DIMSUM_LAUNCH_EV((ssm_scan_bwd_kernel<T, kN, HASZ, VEC, FULL, kRev>), grid, block, stream, ev0, none, q, ckpt, part)
    if (kRev && !p.z_ptr) return DIMSUM_ERR_NULL;
    if (p.z_ptr) DIMSUM_VEC_FULL_LADDER(DIMSUM_LAUNCH, true, vec, full);
    else if constexpr (!kRev) DIMSUM_VEC_FULL_LADDER(DIMSUM_LAUNCH, false, vec, full);       // (the reversed kernels exist with z only)
#undef DIMSUM_LAUNCH
    if (launch_status() != DIMSUM_OK) return DIMSUM_ERR_LAUNCH;
    const int64_t total = (int64_t)p.batch * p.n_groups * 2 * kN * ((p.seqlen + 3) / 4);
    const bool vec4 = p.seqlen % 4 == 0 && aligned_to<float>(q.dB_ptr, 16) && aligned_to<float>(q.dC_ptr, 16) && q.dB_batch_stride % 4 == 0 &&
                      q.dB_group_stride % 4 == 0 && q.dB_dstate_stride % 4 == 0 && q.dC_batch_stride % 4 == 0 && q.dC_group_stride % 4 == 0 &&
                      q.dC_dstate_stride % 4 == 0;
    const dim3 rgrid((unsigned)((total + 255) / 256)), rblock(256);
    if (vec4) DIMSUM_LAUNCH_EV((ssm_scan_bwd_reduce_kernel<true, kRev>), rgrid, rblock, stream, none, ev1, part, q, (dpg + kWC - 1) / kWC);
    else DIMSUM_LAUNCH_EV((ssm_scan_bwd_reduce_kernel<false, kRev>), rgrid, rblock, stream, none, ev1, part, q, (dpg + kWC - 1) / kWC);
    return launch_status();
}

template <bool kRev>
static int dispatch_bwd(const ssm_bwd_args_t &q, const void *states, hipStream_t stream, hipEvent_t ev0) {
    const float *ckpt = reinterpret_cast<const float *>(states);
    float *part = reinterpret_cast<float *>(q.workspace_ptr);
    return ssm_dispatch(q.fwd.dtype, q.fwd.dstate, [&](auto t, auto n) { return launch_bwd<DIMSUM_TAG_T(t), DIMSUM_TAG_N(n), kRev>(q, ckpt, part, stream, ev0); });
}

// workspace = [per-workgroup partial dB / dC | saved states (only when the caller did not keep the forward's)]
int64_t ssm_bwd_partial_bytes(int32_t batch, int32_t dim, int32_t seqlen, int32_t dstate, int32_t n_groups) {
    const int64_t dpg = dim / n_groups;
    const int64_t wgs = (int64_t)batch * n_groups * ((dpg + kBW * kBC - 1) / (kBW * kBC));
    return wgs * 2 * dstate * seqlen * (int64_t)sizeof(float);                      // (workgroups, dB | dC, dstate, seqlen)
}
int64_t ssm_bwd_ckpt_bytes(int32_t batch, int32_t dim, int32_t seqlen, int32_t dstate) {
    const int64_t n_halves = (seqlen + kBS - 1) / kBS;
    return (int64_t)batch * n_halves * dstate * dim * (int64_t)sizeof(float);       // (batch, half tiles, dstate, dim)
}

// public backward struct -> flat block (the size of `pub` itself is checked by the caller)
static int bwd_args_from(const dimsum_ssm_bwd_params_t *pub, ssm_bwd_args_t &flat) {
    const int arc = ssm_args_from(&pub->fwd, flat.fwd, false);
    if (arc != DIMSUM_OK) return arc;
    flat.dout_batch_stride = pub->dout_batch_stride; flat.dout_d_stride = pub->dout_d_stride;
    flat.dA_d_stride = pub->dA_d_stride; flat.dA_dstate_stride = pub->dA_dstate_stride;
    flat.dB_batch_stride = pub->dB_batch_stride; flat.dB_group_stride = pub->dB_group_stride; flat.dB_dstate_stride = pub->dB_dstate_stride;
    flat.dC_batch_stride = pub->dC_batch_stride; flat.dC_group_stride = pub->dC_group_stride; flat.dC_dstate_stride = pub->dC_dstate_stride;
    flat.du_batch_stride = pub->du_batch_stride; flat.du_d_stride = pub->du_d_stride;
    flat.dz_batch_stride = pub->dz_batch_stride; flat.dz_d_stride = pub->dz_d_stride;
    flat.ddelta_batch_stride = pub->ddelta_batch_stride; flat.ddelta_d_stride = pub->ddelta_d_stride;
    flat.dout_ptr = pub->dout_ptr; flat.dA_ptr = pub->dA_ptr; flat.dB_ptr = pub->dB_ptr; flat.dC_ptr = pub->dC_ptr; flat.dD_ptr = pub->dD_ptr;
    flat.du_ptr = pub->du_ptr; flat.dz_ptr = pub->dz_ptr; flat.ddelta_ptr = pub->ddelta_ptr; flat.ddelta_bias_ptr = pub->ddelta_bias_ptr;
    flat.workspace_ptr = pub->workspace_ptr; flat.workspace_bytes = pub->workspace_bytes;
    return DIMSUM_OK;
}

// what both backward entry points ask of a flat block after ssm_check: the required pointers, z => dz and the forward's `out`, a 16-byte
// aligned workspace -- in this order
static int bwd_check(const ssm_bwd_args_t &q) {
    if (!q.dout_ptr || !q.dA_ptr || !q.dB_ptr || !q.dC_ptr || !q.du_ptr || !q.ddelta_ptr || !q.workspace_ptr) return DIMSUM_ERR_NULL;
    if (q.fwd.z_ptr && (!q.dz_ptr || !q.fwd.out_ptr)) return DIMSUM_ERR_NULL;
    if (!aligned_to<float>(q.workspace_ptr, 16)) return DIMSUM_ERR_STRIDE;
    return DIMSUM_OK;
}

}  // namespace dimsum

extern "C" int64_t dimsum_ssm_scan_bwd_workspace_bytes(int32_t batch, int32_t dim, int32_t seqlen, int32_t dstate, int32_t n_groups) {
    if (batch <= 0 || dim <= 0 || seqlen <= 0 || dstate <= 0 || n_groups <= 0 || dim % n_groups != 0) return 0;
    return dimsum::ssm_bwd_partial_bytes(batch, dim, seqlen, dstate, n_groups) + dimsum::ssm_bwd_ckpt_bytes(batch, dim, seqlen, dstate);
}

extern "C" int dimsum_ssm_scan_bwd(const dimsum_ssm_bwd_params_t *pub, void *stream) {
    using namespace dimsum;
    if (!pub) return DIMSUM_ERR_NULL;
    if (pub->struct_size != sizeof(dimsum_ssm_bwd_params_t)) return DIMSUM_ERR_ABI;
    ssm_bwd_args_t q;
    int rc = bwd_args_from(pub, q);
    if (rc == DIMSUM_OK) rc = ssm_check(q.fwd, false);
    if (rc == DIMSUM_OK) rc = bwd_check(q);
    if (rc != DIMSUM_OK) return rc;
    const ssm_args_t &p = q.fwd;
    const int64_t pbytes = ssm_bwd_partial_bytes(p.batch, p.dim, p.seqlen, p.dstate, p.n_groups);
    if (q.workspace_bytes < pbytes + (p.ckpt_ptr ? 0 : ssm_bwd_ckpt_bytes(p.batch, p.dim, p.seqlen, p.dstate))) return DIMSUM_ERR_SHAPE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipEvent_t ev0 = reinterpret_cast<hipEvent_t>(p.timing_start_event);     // begin of the call's FIRST kernel
    const void *states = p.ckpt_ptr;
    if (!states) {
        // reference-shaped call (no saved states): one state-only forward sweep rebuilds them in the workspace
        ssm_args_t f = p;
        f.z_ptr = nullptr; f.out_ptr = nullptr; f.out_z_ptr = nullptr; f.x_ptr = nullptr; f.D_ptr = nullptr;
        f.ckpt_ptr = reinterpret_cast<char *>(q.workspace_ptr) + pbytes;
        f.timing_stop_event = nullptr;          // (the sweep's begin is the call's begin; its end is not the call's end)
        const int frc = ssm_scan_fwd_run(f, s);
        if (frc != DIMSUM_OK) return frc;
        ev0 = nullptr;
        states = f.ckpt_ptr;
    }
    return dispatch_bwd<false>(q, states, s, ev0);
}

// Bidirectional backward (bimamba_inner_fn): the forward direction on the plain kernels (du, ddelta, dz, dB, dC, out_z written), then the
// reversed direction on the kRev instantiations, which add their half in place. dA and dA_b stay apart; dD / ddelta_bias collect both.
// Both directions' saved states are required (the bidirectional forward writes them); the workspace holds the partial dB / dC only.
extern "C" int dimsum_ssm_scan_bidir_bwd(const dimsum_ssm_bidir_bwd_params_t *pub, void *stream) {
    using namespace dimsum;
    if (!pub) return DIMSUM_ERR_NULL;
    if (pub->struct_size != sizeof(dimsum_ssm_bidir_bwd_params_t)) return DIMSUM_ERR_ABI;
    ssm_bwd_args_t qf;
    int rc = bwd_args_from(&pub->bwd, qf);
    if (rc != DIMSUM_OK) return rc;
    ssm_args_t &p = qf.fwd;
    if (p.dt_w_ptr || p.out_z_lo_offset || p.out_z_f16) return DIMSUM_ERR_UNSUPPORTED;
    rc = ssm_check(p, false);
    if (rc != DIMSUM_OK) return rc;
    // (every refusal of bwd_check before its alignment test is DIMSUM_ERR_NULL too: the status does not depend on where these two lines stand)
    if (!p.z_ptr || !p.ckpt_ptr) return DIMSUM_ERR_NULL;
    if (!pub->A_b_ptr || !pub->out_b_ptr || !pub->ckpt_b_ptr || !pub->dA_b_ptr) return DIMSUM_ERR_NULL;
    rc = bwd_check(qf);
    if (rc != DIMSUM_OK) return rc;
    if (qf.workspace_bytes < ssm_bwd_partial_bytes(p.batch, p.dim, p.seqlen, p.dstate, p.n_groups)) return DIMSUM_ERR_SHAPE;
    const hipEvent_t ev0 = reinterpret_cast<hipEvent_t>(p.timing_start_event);
    ssm_bwd_args_t qb = qf;
    qb.fwd = ssm_reversed_from(p, *pub);        // (the events bracket the whole call: begin of the first kernel, end of the last)
    qb.dA_ptr = pub->dA_b_ptr; qb.dA_d_stride = pub->dA_b_d_stride; qb.dA_dstate_stride = pub->dA_b_dstate_stride;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    rc = dispatch_bwd<false>(qf, p.ckpt_ptr, s, ev0);
    return rc != DIMSUM_OK ? rc : dispatch_bwd<true>(qb, qb.fwd.ckpt_ptr, s, nullptr);
}
