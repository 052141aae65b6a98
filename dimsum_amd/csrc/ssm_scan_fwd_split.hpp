// ssm_scan_fwd_split.hpp -- selective scan forward, state-split variants: lane = (channel, state part), kSP parts.
//
// Same math and interface as ssm_scan_fwd_kernel (ssm_scan_fwd_kernel.hpp; reference selective_scan_fwd_kernel.cuh:67-303).
// The sequence axis cannot be shortened without re-doing the exponentials (a chunk carry costs another v_exp_f32 per
// (t, n), and this kernel family is VALU- / latency-bound once the chip is not full), so launches with few channels are
// widened along the STATE axis instead: a wave64 owns 64 / kSP channels of one batch element and lane (c, s) carries
// dstate / kSP states of channel c.
//   kSP = 2: 32 channels per wave, lanes 0-31 the first dstate/2 states, lanes 32-63 the rest. Half the sequential work
//            per wave, 12 KB of LDS, 3 waves per SIMD, twice the waves per launch.
//   kSP = 4: 16 channels per wave, one DPP row of 16 lanes per state quarter. A quarter of the sequential work per
//            wave, 8.6 KB of LDS, 4 waves per SIMD, four times the waves: DiM-XL/2 at 512 px (64 x 1152 channels x 1024
//            steps) is 1152 waves in the 64-channel kernel -- not even one per SIMD -- and 4608 here.
//   * tiles are (64 / kSP) channels x 32 steps: 128-B row segments, whole HBM lines, XOR-swizzled LDS image (no padding);
//   * dt = softplus(delta + bias) is evaluated once per element in the coalesced load layout (not once per part);
//   * y_t = sum over the lane's states; the parts are joined by a transposed exchange per 4-step group:
//     kSP = 2: one v_permlane32_swap + add per PAIR of steps (low lane keeps steps 0, 2, high lane steps 1, 3);
//     kSP = 4: v_permlane32_swap then v_permlane16_swap, 3 swaps + 3 adds per 4 steps: quarter q ends up with step q.
#pragma once
#include "ssm_scan_fwd_kernel.hpp"   // helpers: at(), Raw4, softplus_if, ... (its kernel template is not instantiated by the split units)

namespace dimsum {

constexpr int kST = 32;   // time steps per tile

__device__ __forceinline__ int stile_off(int row, int col4) { return row * kST + ((col4 ^ ((row >> 1) & 7)) << 2); }

__device__ __forceinline__ void swap_halves(float &x, float &y) {      // x.hi <-> y.lo (v_permlane32_swap)
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    x = __uint_as_float(r[0]); y = __uint_as_float(r[1]);
}

__device__ __forceinline__ void swap_rows(float &x, float &y) {        // x.odd rows <-> y.even rows (v_permlane16_swap)
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    x = __uint_as_float(r[0]); y = __uint_as_float(r[1]);
}

template <typename T, int kN, int kSP, bool kHasZ, bool kVec, bool kFull, bool kCkpt = false>
__global__ __launch_bounds__(kWave, (kSP == 4 && kN <= 16) ? 5 : 3) void ssm_scan_fwd_split_kernel(const ssm_args_t p) {
    static_assert(!kFull || kVec, "kFull implies kVec");
    static_assert(kSP == 2 || kSP == 4, "2 or 4 lanes per channel");
    static_assert(kN % (2 * kSP) == 0, "dstate must be a multiple of 2 * kSP");
    constexpr int kSC = kWave / kSP;               // channels per wave
    constexpr int kNL = kN / kSP;                  // states per lane
    constexpr int kNPc = kSC / 8;                  // 16-byte pieces per lane of a kSC x 32 tile (a piece = 8 rows x 128 B)
    // B / C as [n][t], read back as ds_read_b128 whose address is uniform per state part. With 4 parts a 16-lane service
    // group of the read spans two parts, whose rows (kNL apart) start on the same bank: the 16-byte slots of row n are
    // XOR-permuted by n / kNL, so the parts read different slots (no padding: 8 KB of LDS per wave = 20 waves per CU).
    constexpr int kBS = kST;
    auto bc_off = [](int n, int col4) { return n * kST + (((kSP == 4 ? col4 ^ (n / kNL) : col4)) << 2); };
    // one LDS block, [u | dt | B | C]: the sequential loop addresses it with byte offsets formed by ONE v_xor per tile
    __shared__ __attribute__((aligned(16))) float smem[2 * kSC * kST + 2 * kN * kBS];
    float *const tileU = smem, *const tileD = smem + kSC * kST, *const tileB = smem + 2 * kSC * kST, *const tileC = tileB + kN * kBS;

    const int lane = threadIdx.x, c = lane & (kSC - 1), sh = lane / kSC;
    const int ns0 = sh * kNL;
    const int L = p.seqlen;
    const int dpg = p.dim / p.n_groups;
    const int tiles_per_group = (dpg + kSC - 1) / kSC;
    const int tiles_per_batch = p.n_groups * tiles_per_group;
    int wg = blockIdx.x;
    const int nwg = gridDim.x;
    if ((nwg & 7) == 0) wg = (wg & 7) * (nwg >> 3) + (wg >> 3);   // a batch element's waves share an XCD (one L2 for B / C)
    const int b = wg / tiles_per_batch;
    const int rem = wg - b * tiles_per_batch;
    const int g = rem / tiles_per_group;
    const int d0 = g * dpg + (rem - g * tiles_per_group) * kSC;
    const int nd = kFull ? kSC : min(kSC, (g + 1) * dpg - d0);
    const bool live = kFull || c < nd;
    const int d = d0 + (kFull ? c : min(c, nd - 1));

    const T *u_base = reinterpret_cast<const T *>(p.u_ptr) + (int64_t)b * p.u_batch_stride + (int64_t)d0 * p.u_d_stride;
    const T *dl_base = reinterpret_cast<const T *>(p.delta_ptr) + (int64_t)b * p.delta_batch_stride + (int64_t)d0 * p.delta_d_stride;
    const T *z_base = kHasZ ? reinterpret_cast<const T *>(p.z_ptr) + (int64_t)b * p.z_batch_stride + (int64_t)d0 * p.z_d_stride : nullptr;
    T *out_base = p.out_ptr ? reinterpret_cast<T *>(p.out_ptr) + (int64_t)b * p.out_batch_stride + (int64_t)d0 * p.out_d_stride : nullptr;
    T *oz_base = kHasZ ? reinterpret_cast<T *>(p.out_z_ptr) + (int64_t)b * p.out_z_batch_stride + (int64_t)d0 * p.out_z_d_stride : nullptr;
    unsigned short *oz_planes = (kHasZ && p.out_z_lo_offset) ? reinterpret_cast<unsigned short *>(p.out_z_ptr) + (int64_t)b * p.out_z_batch_stride + (int64_t)d0 * p.out_z_d_stride : nullptr;
    const int u_ds = (int)p.u_d_stride, dl_ds = (int)p.delta_d_stride, z_ds = (int)p.z_d_stride;
    const int out_ds = (int)p.out_d_stride, oz_ds = (int)p.out_z_d_stride;
    const T *Bp = reinterpret_cast<const T *>(p.B_ptr) + (int64_t)b * p.B_batch_stride + (int64_t)g * p.B_group_stride;
    const T *Cp = reinterpret_cast<const T *>(p.C_ptr) + (int64_t)b * p.C_batch_stride + (int64_t)g * p.C_group_stride;
    const int Bns = (int)p.B_dstate_stride, Cns = (int)p.C_dstate_stride;

    float A2[kNL], h[kNL];
    {
        const float *Ap = reinterpret_cast<const float *>(p.A_ptr) + (int64_t)d * p.A_d_stride;
#pragma unroll
        for (int k = 0; k < kNL; ++k) { A2[k] = Ap[(ns0 + k) * p.A_dstate_stride] * kLog2e; h[k] = 0.f; }
    }
    const float Dval = p.D_ptr ? reinterpret_cast<const float *>(p.D_ptr)[d] : 0.f;   // D u_t is added by the lane that ends up with step t
    const float *bias_p = reinterpret_cast<const float *>(p.delta_bias_ptr);
    const bool softplus = p.delta_softplus != 0;
    const bool has_out = out_base != nullptr;
    // prod_t a_t[n] = exp2(A2[n] * sum_t dt_t). Vector path: the sum is kept per STAGED row in the load layout (4 adds per
    // 16-byte piece instead of 4 per lane and 4-step group in the sequential loop) and joined only where x is stored.
    float sum_dt = 0.f, sdt[kNPc];
#pragma unroll
    for (int i = 0; i < kNPc; ++i) sdt[i] = 0.f;
    // LDS offsets (floats) of this lane's u / dt row and B / C rows: the 16-byte slot index enters by XOR and the row bases have
    // no bits below 32, so stile_off(c, j) == uoff0 ^ (j << 2) and bc_off(ns0, j) == boff0 ^ (j << 2): one v_xor per 4-step group
    // (byte offsets into smem; the tile bases are multiples of 512 B as well)
    const unsigned uoff0 = 4u * (unsigned)stile_off(c, 0), boff0 = 4u * (unsigned)(2 * kSC * kST + ns0 * kST + ((kSP == 4 ? sh : 0) << 2));
    const unsigned soff0 = uoff0 + 4u * (unsigned)sh;      // the slot this lane's finished y goes to (kSP == 2: and the one 8 B above)
    auto lds4 = [&](unsigned off) -> const f32x4 & { return *reinterpret_cast<const f32x4 *>(reinterpret_cast<const char *>(smem) + off); };
    float *ck_base = (kCkpt && p.ckpt_ptr && live) ? reinterpret_cast<float *>(p.ckpt_ptr) + (int64_t)b * ((L + 7) / 8) * kN * p.dim + (int64_t)ns0 * p.dim + d : nullptr;

    const int n_tiles = (L + kST - 1) / kST;
    // load layout: piece i of the tile, lane -> (row = i*8 + lane/8, 4 columns at (lane%8)*4)
    const int lrow = lane >> 3, lc4 = lane & 7, lcol = lc4 * 4;
    float brow[kNPc];
#pragma unroll
    for (int i = 0; i < kNPc; ++i) brow[i] = bias_p ? bias_p[d0 + min(i * 8 + lrow, nd - 1)] : 0.f;

    constexpr int kBCPieces = (kN * 8 + kWave - 1) / kWave;
    Raw4<T> ru[kNPc], rd[kNPc], rz[kNPc], rb[kBCPieces], rc[kBCPieces];
    auto col_of = [&](int t0) { return min(t0 + lcol, L - 4); };
    auto piece = [&](const T *base, int ds, int i, int col) -> const T * {
        if constexpr (kFull) return at(base + i * 8 * ds, (unsigned)(lrow * ds + col));
        else return at(base, (unsigned)(min(i * 8 + lrow, nd - 1) * ds + col));
    };
    // With 4 lanes per channel the kernel targets 5 waves per SIMD (<= 96 VGPRs): only the two HBM streams (u, delta) are
    // prefetched a tile ahead in registers; B / C (L2-resident: shared by all waves of a batch element) and z are requested
    // where they are used -- the other 4 waves of the SIMD cover that latency.
    constexpr bool kLean = kSP == 4;
    auto issue_bc = [&](int t0) {
        const int col = col_of(t0);
#pragma unroll
        for (int i = 0; i < kBCPieces; ++i) {
            const int n = min(i * 8 + lrow, kN - 1);
            rb[i] = ld4<T>(at(Bp, (unsigned)(n * Bns + col)));
            rc[i] = ld4<T>(at(Cp, (unsigned)(n * Cns + col)));
        }
    };
    auto issue_loads = [&](int t0) {
        const int col = col_of(t0);
#pragma unroll
        for (int i = 0; i < kNPc; ++i) {
            ru[i] = ld4<T>(piece(u_base, u_ds, i, col));
            rd[i] = ld4<T>(piece(dl_base, dl_ds, i, col));
        }
        if constexpr (!kLean) issue_bc(t0);
    };

    if constexpr (kVec) issue_loads(0);

#pragma unroll 1
    for (int tile = 0; tile < n_tiles; ++tile) {
        const int t0 = tile * kST;
        // ---- stage the tile into LDS: u, dt = softplus(delta + bias) (0 beyond L: a = 1, b = 0, the state is untouched) ----
        if constexpr (kVec) {
            const bool col_ok = t0 + lcol < L;
            if constexpr (kLean) issue_bc(t0);
#pragma unroll
            for (int i = 0; i < kNPc; ++i) {
                const int row = i * 8 + lrow;
                f32x4 vd = widen(rd[i]);
#pragma unroll
                for (int s = 0; s < 4; ++s) vd.v[s] = col_ok ? softplus_if(vd.v[s] + brow[i], softplus) : 0.f;
                sdt[i] += (vd.v[0] + vd.v[1]) + (vd.v[2] + vd.v[3]);
                *reinterpret_cast<f32x4 *>(&tileU[stile_off(row, lc4)]) = widen(ru[i]);
                *reinterpret_cast<f32x4 *>(&tileD[stile_off(row, lc4)]) = vd;
            }
#pragma unroll
            for (int i = 0; i < kBCPieces; ++i) {
                const int n = i * 8 + lrow;
                if (kN * 8 % kWave == 0 || n < kN) {
                    *reinterpret_cast<f32x4 *>(&tileB[bc_off(n, lc4)]) = widen(rb[i]);
                    *reinterpret_cast<f32x4 *>(&tileC[bc_off(n, lc4)]) = widen(rc[i]);
                }
            }
            if (tile + 1 < n_tiles) issue_loads(t0 + kST);   // flies under the compute below
            if constexpr (kHasZ && !kLean) {
                const int col = col_of(t0);
#pragma unroll
                for (int i = 0; i < kNPc; ++i) rz[i] = ld4<T>(piece(z_base, z_ds, i, col));
            }
        } else {
            for (int i = 0; i < kSC * kST / kWave; ++i) {
                const int idx = i * kWave + lane, row = idx / kST, col = idx & (kST - 1);
                const bool ok = row < nd && t0 + col < L;
                float vu = 0.f, vd = 0.f;
                if (ok) {
                    vu = to_f32<T>(u_base[(unsigned)(row * u_ds + t0 + col)]);
                    vd = softplus_if(to_f32<T>(dl_base[(unsigned)(row * dl_ds + t0 + col)]) + (bias_p ? bias_p[d0 + row] : 0.f), softplus);
                }
                tileU[stile_off(row, col >> 2) + (col & 3)] = vu;
                tileD[stile_off(row, col >> 2) + (col & 3)] = vd;
            }
            for (int idx = lane; idx < kN * kST; idx += kWave) {
                const int n = idx / kST, col = idx & (kST - 1), tc = min(t0 + col, L - 1);
                tileB[bc_off(n, col >> 2) + (col & 3)] = to_f32<T>(Bp[(unsigned)(n * Bns + tc)]);
                tileC[bc_off(n, col >> 2) + (col & 3)] = to_f32<T>(Cp[(unsigned)(n * Cns + tc)]);
            }
        }

        // ---- 32 sequential steps, 4 at a time; 5 VALU ops per (t, n): mul, v_exp_f32, mul, fma, fma ---------------------
#pragma unroll 1
        for (int j = 0; j < kST / 4; ++j) {
            const int tj = t0 + j * 4;
            if (tj >= L) break;
            if (kCkpt && ck_base && (j & 1) == 0) {
                float *ck = ck_base + (int64_t)(tj >> 3) * kN * p.dim;
#pragma unroll
                for (int k = 0; k < kNL; ++k) ck[(int64_t)k * p.dim] = h[k];
            }
            const unsigned jx = (unsigned)j << 4, uo = uoff0 ^ jx, bo = boff0 ^ jx;
            const f32x4 u4 = lds4(uo);
            const f32x4 d4 = lds4(uo + 4u * kSC * kST);
            f32x4 bq_nxt = lds4(bo);
            f32x4 cq_nxt = lds4(bo + 4u * kN * kBS);
            // u of the step(s) whose total this lane ends up with (for D u): one b32 read of the slot it overwrites below
            float *slot = reinterpret_cast<float *>(reinterpret_cast<char *>(smem) + (soff0 ^ jx));
            const float uown0 = slot[0], uown2 = kSP == 2 ? slot[2] : 0.f;
            float du[4], y[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if constexpr (!kVec) sum_dt += d4.v[s];
                du[s] = d4.v[s] * u4.v[s];
            }
#pragma unroll
            for (int k = 0; k < kNL; ++k) {
                const f32x4 bq = bq_nxt, cq = cq_nxt;
                if (k + 1 < kNL) {
                    bq_nxt = lds4(bo + 4u * (k + 1) * kBS);
                    cq_nxt = lds4(bo + 4u * (kN + k + 1) * kBS);
                }
                float hn = h[k];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    hn = fmaf(fast_exp2(d4.v[s] * A2[k]), hn, bq.v[s] * du[s]);
                    y[s] = k == 0 ? hn * cq.v[s] : fmaf(hn, cq.v[s], y[s]);
                }
                h[k] = hn;
            }
            if constexpr (kSP == 2) {
                // join the halves: low lane <- totals of steps 0 and 2, high lane <- totals of steps 1 and 3
                swap_halves(y[0], y[1]);
                swap_halves(y[2], y[3]);
                slot[0] = fmaf(Dval, uown0, y[0] + y[1]);
                slot[2] = fmaf(Dval, uown2, y[2] + y[3]);
            } else {
                // join the quarters (rows of 16 lanes): rows 0, 1 <- sums over rows {r, r + 2} of steps 0 / 1, rows 2, 3 of
                // steps 2 / 3; then the even row of each pair keeps the first, the odd row the second: quarter q <- step q
                swap_halves(y[0], y[2]);
                swap_halves(y[1], y[3]);
                float w0 = y[0] + y[2], w1 = y[1] + y[3];
                swap_rows(w0, w1);
                slot[0] = fmaf(Dval, uown0, w0 + w1);
            }
        }

        // ---- chunk-state store at every 2048 boundary and at the end (selective_scan_fwd_kernel.cuh:251-254) ---
        const int t_end = min(t0 + kST, L);
        if (kVec && p.x_ptr && ((t_end & 2047) == 0 || t_end == L)) {
            // join the staged rows' dt sums: 8 partials per row through LDS (the dt tile is consumed), row c read back by lane c
#pragma unroll
            for (int i = 0; i < kNPc; ++i) tileD[(i * 8 + lrow) * 8 + lc4] = sdt[i];
            const f32x4 a = *reinterpret_cast<const f32x4 *>(&tileD[c * 8]), b2 = *reinterpret_cast<const f32x4 *>(&tileD[c * 8 + 4]);
            sum_dt = ((a.v[0] + a.v[1]) + (a.v[2] + a.v[3])) + ((b2.v[0] + b2.v[1]) + (b2.v[2] + b2.v[3]));
        }
        if (p.x_ptr && ((t_end & 2047) == 0 || t_end == L) && live) {
            float *xr = reinterpret_cast<float *>(p.x_ptr) + (((int64_t)b * p.dim + d) * p.n_chunks + (t_end - 1) / 2048) * (2 * kN) + 2 * ns0;
#pragma unroll
            for (int k = 0; k < kNL; k += 2) {
                const f32x4 v = {{fast_exp2(A2[k] * sum_dt), h[k], fast_exp2(A2[k + 1] * sum_dt), h[k + 1]}};
                *reinterpret_cast<f32x4 *>(xr + 2 * k) = v;
            }
        }

        // ---- epilogue: re-read y in the coalesced layout, gate, store -------------------------------------------
        if constexpr (kVec) {
            if (t0 + lcol < L) {
                if constexpr (kHasZ && kLean) {
                    const int col = col_of(t0);
#pragma unroll
                    for (int i = 0; i < kNPc; ++i) rz[i] = ld4<T>(piece(z_base, z_ds, i, col));
                }
#pragma unroll
                for (int i = 0; i < kNPc; ++i) {
                    const int row = i * 8 + lrow;
                    if (kFull || row < nd) {
                        f32x4 y4 = *reinterpret_cast<const f32x4 *>(&tileU[stile_off(row, lc4)]);
                        if (has_out) st4<T>(at(out_base + i * 8 * out_ds, (unsigned)(lrow * out_ds + t0 + lcol)), y4);
                        if constexpr (kHasZ) {
                            const f32x4 z4 = widen(rz[i]);
#pragma unroll
                            for (int s = 0; s < 4; ++s) y4.v[s] *= z4.v[s] * sigmoidf_fast(z4.v[s]);
                            st4_out_z<T>(oz_base + i * 8 * oz_ds, oz_planes ? oz_planes + i * 8 * oz_ds : nullptr, p.out_z_lo_offset, (unsigned)(lrow * oz_ds + t0 + lcol), y4);
                        }
                    }
                }
            }
        } else {
            for (int i = 0; i < kSC * kST / kWave; ++i) {
                const int idx = i * kWave + lane, row = idx / kST, col = idx & (kST - 1);
                if (row < nd && t0 + col < L) {
                    const float yv = tileU[stile_off(row, col >> 2) + (col & 3)];
                    if (out_base) out_base[(unsigned)(row * out_ds + t0 + col)] = from_f32<T>(yv);
                    if constexpr (kHasZ) {
                        const float zv = to_f32<T>(z_base[(unsigned)(row * z_ds + t0 + col)]);
                        oz_base[(unsigned)(row * oz_ds + t0 + col)] = from_f32<T>(yv * zv * sigmoidf_fast(zv));
                    }
                }
            }
        }
    }
}

// ---- launcher: explicitly instantiated per I/O dtype in ssm_scan_fwd_split_{f32,f16,bf16}.hip ---------------------------------
template <typename T, int kN, int kSP>
void ssm_scan_fwd_launch_split(const ssm_args_t &p, hipStream_t stream, int tiles, bool vec, bool full) {
    const dim3 grid(tiles), block(kWave);
    const hipEvent_t ev0 = reinterpret_cast<hipEvent_t>(p.timing_start_event), ev1 = reinterpret_cast<hipEvent_t>(p.timing_stop_event);
#define DIMSUM_LAUNCH(HASZ, VEC, FULL)                                                                                               \
    do {                                                                                                                              \
        if (p.ckpt_ptr) DIMSUM_LAUNCH_EV((ssm_scan_fwd_split_kernel<T, kN, kSP, HASZ, VEC, FULL, true>), grid, block, stream, ev0, ev1, p); \
        else DIMSUM_LAUNCH_EV((ssm_scan_fwd_split_kernel<T, kN, kSP, HASZ, VEC, FULL, false>), grid, block, stream, ev0, ev1, p);         \
    } while (0)
    DIMSUM_Z_VEC_FULL_LADDER(DIMSUM_LAUNCH, p.z_ptr, vec, full);
#undef DIMSUM_LAUNCH
}

#define DIMSUM_INSTANTIATE_FWD_SPLIT(T)                                                                                   \
    template void ssm_scan_fwd_launch_split<T, 4, 2>(const ssm_args_t &, hipStream_t, int, bool, bool);           \
    template void ssm_scan_fwd_launch_split<T, 8, 2>(const ssm_args_t &, hipStream_t, int, bool, bool);           \
    template void ssm_scan_fwd_launch_split<T, 16, 2>(const ssm_args_t &, hipStream_t, int, bool, bool);          \
    template void ssm_scan_fwd_launch_split<T, 32, 2>(const ssm_args_t &, hipStream_t, int, bool, bool);          \
    template void ssm_scan_fwd_launch_split<T, 8, 4>(const ssm_args_t &, hipStream_t, int, bool, bool);           \
    template void ssm_scan_fwd_launch_split<T, 16, 4>(const ssm_args_t &, hipStream_t, int, bool, bool);          \
    template void ssm_scan_fwd_launch_split<T, 32, 4>(const ssm_args_t &, hipStream_t, int, bool, bool);

}  // namespace dimsum
