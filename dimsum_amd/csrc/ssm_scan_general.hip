// ssm_scan_general.hip -- the general selective scan for gfx950: everything selective_scan_cuda takes that the tuned kernels
// (ssm_scan_fwd*.hip, ssm_scan_bwd.hip: real A, input-dependent B / C, dstate in {4, 8, 16, 32}) do not: any dstate in 1..256, constant
// (dim, dstate) B and / or C, complex A (mamba/csrc/selective_scan/selective_scan.cpp:226-492, selective_scan_fwd_kernel.cuh,
// selective_scan_bwd_kernel.cuh). Plain HIP C++.
//
//   dt = softplus(delta + delta_bias)      h_t = exp(dt A) h_{t-1} + dt B_t u_t      y_t = sum_n C_t h_t  (complex: 2 Re sum_n C_t h_t)
//   out = y + D u                          out_z = out silu(z)
//
// Layout. Lane = channel: a wave owns 64 channels of one (batch, group); a workgroup is W = ceil(dstate / kNB) such
// waves over the SAME channels, wave w owning the states [w kNB, (w + 1) kNB) in registers (kNB = 16: W <= 4 up to 64 states, <= 16 above). The
// sequence is walked ONCE, in tiles of kT = 64 / (kNB reals per state) steps: a tile of input-dependent B (or C) of one wave is exactly 64
// values -- one load instruction (kNB row pieces of 16 - 32 bytes), lane l holding (state l / row, step l % row), read back with v_readlane as a scalar operand. Constant B / C
// are per-lane registers. Every wave reads u and delta itself (the same lines: L1 / L2 hits after the first wave). The per-wave partial sums
// over states -- y in the forward, du and ddelta in the backward -- go through LDS and are added by wave 0 in wave order (fixed order),
// which also applies D, z, delta's softplus and writes the (batch, dim, seqlen) outputs.
// The backward is one kernel: a forward sweep stores the state before every tile into the caller's workspace (each lane reads back only
// what it wrote itself), then the tiles are walked from the last to the first: the tile's kT states are rebuilt from the saved one and the
// adjoint recurrence runs backwards over them. Sums over a group's channels (input-dependent dB / dC: a DPP wave reduction per value) and
// over the batch (dA, constant dB / dC, dD, ddelta_bias) are fp32 atomics into zero-filled outputs: not bit-repeatable.
// A carried state (dimsum_ssm_scan_carry_fwd, forward only) is a load before the walk and a store after it: the states live in registers, each
// (channel, state) in exactly one lane, so that lane reads its h0 element, walks the sequence and writes its hT element -- hT may be h0.
// Packed rows (dimsum_ssm_scan_varlen_fwd / _bwd, kVarlen; real A, input-dependent B / C): a per-token sequence id rides along. Once per tile
// a wave reads the tile's kT ids and the one before them -- the row is the workgroup's, so the addresses and the resulting kT-bit reset
// mask are wave-uniform and every wave of the workgroup forms the same mask -- and at a set bit the step starts from h = 0 (a select on
// h_{t-1}, so nothing of the previous segment survives, not even a NaN). The backward masks a_t h_{t-1} and the adjoint hand-over the same way.
// Per-segment states (dimsum_ssm_scan_varlen_states_fwd, kEmit on top of kVarlen): a second int32 row, end_slots, rides next to the ids and is
// read the same way (uniform addresses, a kT-bit wave-uniform mask). After a step whose bit is set every lane stores the h[j] it has just
// computed -- the value the next step would read -- to pool[slot, d, n0 + j]: one lane per (channel, state), as for hT. The stores sit
// behind a uniform branch inside the statically unrolled tile loop; kEmit = false compiles to the kernels as they were.
// Resumed segments (dimsum_ssm_scan_varlen_resume_fwd, kStart on top of kEmit): a third int32 row, start_slots, read like end_slots. Before a
// step whose bit is set every lane loads its h[j] from init[slot, d, n0 + j] -- in place of the 0 a boundary puts in, and at t = 0, where
// there is no boundary bit -- behind the same kind of uniform branch. init may be the pool: the lane that loads an element at a segment's
// first step is the lane that stores it at the segment's end, in its own program order, provided no OTHER segment of the launch reads a
// slot this launch stores. kStart = false compiles to the kernels as they were.
#include "common.hpp"

#include <type_traits>

namespace dimsum {

// the carried state of dimsum_ssm_scan_carry_fwd: both pointers NULL for every other entry point
struct gen_carry_t {
    const void *h0_ptr;
    void *hT_ptr;
    int64_t h0_batch_stride, h0_d_stride, h0_dstate_stride, hT_batch_stride, hT_d_stride, hT_dstate_stride;
    int32_t f32;                           // the state is float (pairs, with complex A); else of the I/O type
};

struct gen_args_t {
    dimsum_ssm_general_params_t f;
    dimsum_ssm_general_bwd_params_t b;     // b.fwd is not used (f is)
    gen_carry_t c;                         // forward only
    int32_t cblocks;                       // 64-channel blocks per group
    int64_t dpad;                          // padded channel count of the saved states: n_groups * cblocks * 64
    const int32_t *seq_idx;                // packed rows (kVarlen): (batch, seqlen) ids, rows seq_batch_stride apart; else NULL
    int64_t seq_batch_stride;
};

// the kernel argument of the kEmit kernels: the plain one + where the per-segment states go
struct gen_emit_args_t : gen_args_t {
    const int32_t *end_slots;              // (batch, seqlen) int32, rows end_batch_stride apart: >= 0 = store the state after this position into that slot
    int64_t end_batch_stride;
    void *pool;                            // (num_slots, dim, dstate), three free element strides
    int64_t pool_slot_stride, pool_d_stride, pool_dstate_stride;
    int32_t pool_f32;                      // the pool is float; else of the I/O type
};

// the kernel argument of the kStart kernels: the kEmit one + where a segment's first state comes from
struct gen_start_args_t : gen_emit_args_t {
    const int32_t *start_slots;            // (batch, seqlen) int32, rows start_batch_stride apart: >= 0 (a segment's first position) = enter it with that row of init
    int64_t start_batch_stride;
    const void *init;                      // (n_init, dim, dstate), three free element strides; may be the pool
    int64_t init_slot_stride, init_d_stride, init_dstate_stride;
    int32_t init_f32;                      // init is float; else of the I/O type
};

constexpr int kGenChunk = 2048;            // selective_scan.cpp:307

template <bool kCplx, int kNB> struct GenCfg {
    static constexpr int kK = kCplx ? 2 : 1;            // reals per state
    static constexpr int kRow = 64 / kNB;               // reals of one state's row in a 64-value tile of B / C
    static constexpr int kT = kRow / kK;                // steps per tile
};

// sum over the 64 lanes, in every lane, on the VALU (the pattern of wave_allmax)
__device__ __forceinline__ float wave_allsum(float v) {
    v += dpp_mov<0xB1>(v);
    v += dpp_mov<0x4E>(v);
    v += dpp_mov<0x141>(v);
    v += dpp_mov<0x140>(v);
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

__device__ __forceinline__ float lane_value(float v, int lane) {      // lane: a compile-time constant after unrolling
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

// what a (wave, tile) shares: where the block sits
struct gen_pos_t {
    int b, g, d, n0, lane, wave;
    bool live;           // d < the group's last channel
};

template <typename T> __device__ __forceinline__ float ld_f32(const void *base, int64_t off) { return to_f32<T>(reinterpret_cast<const T *>(base)[off]); }

// the wave's 64-value tile of an input-dependent B / C: rows of kRow reals (kT steps) of kNB states
template <typename T, bool kCplx, int kNB>
__device__ __forceinline__ float load_bc_tile(const void *ptr, int64_t batch_stride, int64_t group_stride, int64_t dstate_stride, const gen_pos_t &q, int dstate,
                                              int seqlen, int t0) {
    using Cfg = GenCfg<kCplx, kNB>;
    const int j = q.lane / Cfg::kRow, i = q.lane % Cfg::kRow;
    const int n = q.n0 + j;
    const int64_t col = (int64_t)t0 * Cfg::kK + i;
    if (n >= dstate || col >= (int64_t)seqlen * Cfg::kK) return 0.f;
    return ld_f32<T>(ptr, q.b * batch_stride + q.g * group_stride + n * dstate_stride + col);
}

// per-lane constants of the wave's states: A (and constant B / C) rows of channel d; states beyond dstate read as 0 (a = 1, h stays 0)
template <bool kCplx, int kNB>
__device__ __forceinline__ void load_weight_rows(const void *ptr, int64_t d_stride, int64_t n_stride, const gen_pos_t &q, int dstate, float (&w)[kNB * (kCplx ? 2 : 1)]) {
    constexpr int kK = kCplx ? 2 : 1;
    const float *p = reinterpret_cast<const float *>(ptr);
#pragma unroll
    for (int j = 0; j < kNB; ++j) {
        const bool ok = q.live && q.n0 + j < dstate;
        const int64_t off = ((int64_t)q.d * d_stride + (int64_t)(q.n0 + j) * n_stride) * kK;
#pragma unroll
        for (int c = 0; c < kK; ++c) w[j * kK + c] = ok ? p[off + c] : 0.f;
    }
}

template <bool kCplx> __device__ __forceinline__ void decay(float dt, float ar, float ai, float &pr, float &pi) {      // exp(dt A)
    const float m = fast_exp(dt * ar);
    if constexpr (kCplx) {
        float s, c;
        sincosf(dt * ai, &s, &c);
        pr = m * c;
        pi = m * s;
    } else {
        pr = m;
        pi = 0.f;
    }
}

__device__ __forceinline__ float delta_of(float raw, float bias, bool softplus) {
    const float x = raw + bias;
    return softplus ? softplus_ref(x) : x;
}

// the reset mask of one tile of a packed row: bit i = position t0 + i is a boundary (its id differs from the one before it; position 0 and
// the positions beyond the row never are). `ids` is the workgroup's row: uniform addresses, a scalar result.
template <int kT> __device__ __forceinline__ unsigned reset_mask(const int32_t *ids, int t0, int L) {
    unsigned m = 0;
    int prev = ids[t0 > 0 ? t0 - 1 : 0];
#pragma unroll
    for (int i = 0; i < kT; ++i) {
        const int t = t0 + i;
        const int cur = ids[t < L ? t : L - 1];
        if (t > 0 && t < L && cur != prev) m |= 1u << i;
        prev = cur;
    }
    return (unsigned)__builtin_amdgcn_readfirstlane((int)m);
}

// the slots of one tile of end_slots and their mask: bit i = the state after position t0 + i is stored into slot[i] (>= 0; positions beyond
// the row never store). The row is the workgroup's, as for reset_mask: uniform addresses, scalar results. start_slots is read by the same
// function: bit i = the state entering position t0 + i is loaded from slot[i].
template <int kT> __device__ __forceinline__ unsigned emit_mask(const int32_t *ends, int t0, int L, int (&slot)[kT]) {
    unsigned m = 0;
#pragma unroll
    for (int i = 0; i < kT; ++i) {
        const int t = t0 + i;
        const int s = __builtin_amdgcn_readfirstlane(ends[t < L ? t : L - 1]);
        slot[i] = s;
        if (t < L && s >= 0) m |= 1u << i;
    }
    return (unsigned)__builtin_amdgcn_readfirstlane((int)m);
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------------------
template <typename T, bool kCplx, bool kVarB, bool kVarC, int kNB, int kMaxThreads, bool kVarlen, bool kEmit = false, bool kStart = false>
__global__ __launch_bounds__(kMaxThreads) void ssm_scan_general_fwd_kernel(
    const std::conditional_t<kStart, gen_start_args_t, std::conditional_t<kEmit, gen_emit_args_t, gen_args_t>> a) {
    static_assert(!kVarlen || (!kCplx && kVarB && kVarC), "packed rows: real A with input-dependent B and C");
    static_assert(!kEmit || kVarlen, "per-segment states belong to packed rows");
    static_assert(!kStart || kEmit, "resumed segments ride on the per-segment-states kernels");
    using Cfg = GenCfg<kCplx, kNB>;
    constexpr int kK = Cfg::kK, kT = Cfg::kT, kRow = Cfg::kRow;
    extern __shared__ float red[];                      // [wave][step][lane]
    const dimsum_ssm_general_params_t &p = a.f;
    gen_pos_t q;
    q.lane = threadIdx.x & 63;
    q.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    q.b = blockIdx.y;
    q.g = blockIdx.x / a.cblocks;
    const int dpg = p.dim / p.n_groups;
    const int dg = (blockIdx.x % a.cblocks) * 64 + q.lane;
    q.live = dg < dpg;
    q.d = q.g * dpg + (q.live ? dg : 0);
    q.n0 = q.wave * kNB;
    const int W = blockDim.x >> 6, L = p.seqlen, N = p.dstate;

    float A[kNB * kK], Bc[kNB * kK], Cc[kNB * kK], h[kNB * kK];
    load_weight_rows<kCplx, kNB>(p.A_ptr, p.A_d_stride, p.A_dstate_stride, q, N, A);
    if constexpr (!kVarB) load_weight_rows<kCplx, kNB>(p.B_ptr, p.B_d_stride, p.B_dstate_stride, q, N, Bc);
    if constexpr (!kVarC) load_weight_rows<kCplx, kNB>(p.C_ptr, p.C_d_stride, p.C_dstate_stride, q, N, Cc);
    // the carried state: this lane's own elements, read before the walk and written after it (hT may be h0: no other lane touches them);
    // states beyond dstate and masked channels stay 0
#pragma unroll
    for (int j = 0; j < kNB; ++j) {
        const bool ok = a.c.h0_ptr && q.live && q.n0 + j < N;
        const int64_t off = q.b * a.c.h0_batch_stride + q.d * a.c.h0_d_stride + (q.n0 + j) * a.c.h0_dstate_stride;
#pragma unroll
        for (int c = 0; c < kK; ++c) h[j * kK + c] = !ok ? 0.f : (kCplx || a.c.f32) ? ld_f32<float>(a.c.h0_ptr, off * kK + c) : ld_f32<T>(a.c.h0_ptr, off);
    }
    const float bias = (p.delta_bias_ptr && q.live) ? reinterpret_cast<const float *>(p.delta_bias_ptr)[q.d] : 0.f;
    const float Dd = (p.D_ptr && q.live) ? reinterpret_cast<const float *>(p.D_ptr)[q.d] : 0.f;
    const bool sp = p.delta_softplus != 0;
    const int64_t u_row = q.b * p.u_batch_stride + q.d * p.u_d_stride, dl_row = q.b * p.delta_batch_stride + q.d * p.delta_d_stride;
    float sumdt = 0.f, sumdt_lo = 0.f;                  // x's running product = exp(A sum dt); compensated: the phase of a complex product is A.im sum dt
    const int32_t *ids = kVarlen ? a.seq_idx + (int64_t)q.b * a.seq_batch_stride : nullptr;
    bool cut = false;                                   // kVarlen: a boundary lies behind: the running product is 0 from there on
    const int32_t *ends = nullptr;                      // kEmit: the row's end_slots
    if constexpr (kEmit) ends = a.end_slots + (int64_t)q.b * a.end_batch_stride;
    const int32_t *starts = nullptr;                    // kStart: the row's start_slots
    if constexpr (kStart) starts = a.start_slots + (int64_t)q.b * a.start_batch_stride;

    for (int t0 = 0; t0 < L; t0 += kT) {
        unsigned rm = 0;
        if constexpr (kVarlen) {
            rm = reset_mask<kT>(ids, t0, L);
            cut = cut || rm != 0;
        }
        unsigned em = 0;
        int eslot[kT];
        if constexpr (kEmit) em = emit_mask<kT>(ends, t0, L, eslot);
        unsigned sm = 0;
        int sslot[kT];
        if constexpr (kStart) {
            sm = emit_mask<kT>(starts, t0, L, sslot);
            rm &= ~sm;                                  // the loaded state takes the place of the boundary's 0
        }
        float uv[kT], dt[kT], y[kT];
#pragma unroll
        for (int i = 0; i < kT; ++i) {
            const bool ok = q.live && t0 + i < L;
            uv[i] = ok ? ld_f32<T>(p.u_ptr, u_row + t0 + i) : 0.f;
            dt[i] = ok ? delta_of(ld_f32<T>(p.delta_ptr, dl_row + t0 + i), bias, sp) : 0.f;
            y[i] = 0.f;
        }
        float bt = 0.f, ct = 0.f;
        if constexpr (kVarB) bt = load_bc_tile<T, kCplx, kNB>(p.B_ptr, p.B_batch_stride, p.B_group_stride, p.B_dstate_stride, q, N, L, t0);
        if constexpr (kVarC) ct = load_bc_tile<T, kCplx, kNB>(p.C_ptr, p.C_batch_stride, p.C_group_stride, p.C_dstate_stride, q, N, L, t0);
#pragma unroll
        for (int i = 0; i < kT; ++i) {
            const float dtu = dt[i] * uv[i];
            {
                const float yk = dt[i] - sumdt_lo, tk = sumdt + yk;      // Kahan
                sumdt_lo = (tk - sumdt) - yk;
                sumdt = tk;
            }
            if constexpr (kStart) {
                if ((sm >> i) & 1u) {                   // wave-uniform: a resumed segment begins at t0 + i; this lane's states, as h0 reads them
                    const int64_t base = (int64_t)sslot[i] * a.init_slot_stride + (int64_t)q.d * a.init_d_stride;
                    if (a.init_f32) {
#pragma unroll
                        for (int j = 0; j < kNB; ++j)
                            h[j] = q.live && q.n0 + j < N ? ld_f32<float>(a.init, base + (int64_t)(q.n0 + j) * a.init_dstate_stride) : 0.f;
                    } else {
#pragma unroll
                        for (int j = 0; j < kNB; ++j)
                            h[j] = q.live && q.n0 + j < N ? ld_f32<T>(a.init, base + (int64_t)(q.n0 + j) * a.init_dstate_stride) : 0.f;
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < kNB; ++j) {
                float pr, pi;
                decay<kCplx>(dt[i], A[j * kK], kCplx ? A[j * kK + kK - 1] : 0.f, pr, pi);
                if constexpr (kCplx) {
                    const float br = kVarB ? lane_value(bt, j * kRow + 2 * i) : Bc[2 * j], bi = kVarB ? lane_value(bt, j * kRow + 2 * i + 1) : Bc[2 * j + 1];
                    const float cr = kVarC ? lane_value(ct, j * kRow + 2 * i) : Cc[2 * j], ci = kVarC ? lane_value(ct, j * kRow + 2 * i + 1) : Cc[2 * j + 1];
                    const float hr = h[2 * j], hi = h[2 * j + 1];
                    h[2 * j] = fmaf(pr, hr, fmaf(-pi, hi, dtu * br));
                    h[2 * j + 1] = fmaf(pr, hi, fmaf(pi, hr, dtu * bi));
                    y[i] += 2.f * (cr * h[2 * j] - ci * h[2 * j + 1]);          // 2 Re(C h): selective_scan_fwd_kernel.cuh, selective_scan_ref :163-164
                } else {
                    const float bv = kVarB ? lane_value(bt, j * kRow + i) : Bc[j], cv = kVarC ? lane_value(ct, j * kRow + i) : Cc[j];
                    h[j] = fmaf(pr, kVarlen && ((rm >> i) & 1u) ? 0.f : h[j], dtu * bv);
                    y[i] = fmaf(h[j], cv, y[i]);
                }
            }
            if constexpr (kEmit) {
                if ((em >> i) & 1u) {                   // wave-uniform: a segment ends at t0 + i; this lane's states, as hT writes them
                    const int64_t base = (int64_t)eslot[i] * a.pool_slot_stride + (int64_t)q.d * a.pool_d_stride;
#pragma unroll
                    for (int j = 0; j < kNB; ++j) {
                        if (!q.live || q.n0 + j >= N) continue;
                        const int64_t off = base + (int64_t)(q.n0 + j) * a.pool_dstate_stride;
                        if (a.pool_f32) reinterpret_cast<float *>(a.pool)[off] = h[j];
                        else reinterpret_cast<T *>(a.pool)[off] = from_f32<T>(h[j]);
                    }
                }
            }
        }
        // chunk-end states (selective_scan_fwd_kernel.cuh:239-254): running product and state interleaved. kT divides the chunk, so a chunk ends
        // with a tile; the steps of the last tile beyond seqlen leave h and sum dt as they are
        const bool chunk_end = (t0 + kT) % kGenChunk == 0 || t0 + kT >= L;
        if (p.x_ptr && chunk_end && q.live) {
            float *xr = reinterpret_cast<float *>(p.x_ptr) + (((int64_t)q.b * p.dim + q.d) * p.n_chunks + t0 / kGenChunk) * 2 * N * kK;
#pragma unroll
            for (int j = 0; j < kNB; ++j) {
                float pr, pi;
                decay<kCplx>(sumdt, A[j * kK], kCplx ? A[j * kK + kK - 1] : 0.f, pr, pi);
                if (q.n0 + j < N) {
                    float *e = xr + (int64_t)(q.n0 + j) * 2 * kK;
                    e[0] = kVarlen && cut ? 0.f : pr;
                    if constexpr (kCplx) { e[1] = pi; e[2] = h[2 * j]; e[3] = h[2 * j + 1]; }
                    else e[1] = h[j];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < kT; ++i) red[(q.wave * kT + i) * 64 + q.lane] = y[i];
        __syncthreads();
        if (q.wave == 0) {
#pragma unroll
            for (int i = 0; i < kT; ++i) {
                float acc = 0.f;
                for (int w = 0; w < W; ++w) acc += red[(w * kT + i) * 64 + q.lane];
                if (q.live && t0 + i < L) {
                    acc = fmaf(Dd, uv[i], acc);
                    if (p.out_ptr) reinterpret_cast<T *>(p.out_ptr)[q.b * p.out_batch_stride + q.d * p.out_d_stride + t0 + i] = from_f32<T>(acc);
                    if (p.z_ptr) {
                        const float z = ld_f32<T>(p.z_ptr, q.b * p.z_batch_stride + q.d * p.z_d_stride + t0 + i);
                        reinterpret_cast<T *>(p.out_z_ptr)[q.b * p.out_z_batch_stride + q.d * p.out_z_d_stride + t0 + i] = from_f32<T>(acc * z * sigmoidf_fast(z));
                    }
                }
            }
        }
        __syncthreads();
    }
    if (a.c.hT_ptr && q.live) {
#pragma unroll
        for (int j = 0; j < kNB; ++j) {
            if (q.n0 + j >= N) continue;
            const int64_t off = q.b * a.c.hT_batch_stride + q.d * a.c.hT_d_stride + (q.n0 + j) * a.c.hT_dstate_stride;
            if constexpr (kCplx) {
                reinterpret_cast<float *>(a.c.hT_ptr)[off * 2] = h[2 * j];
                reinterpret_cast<float *>(a.c.hT_ptr)[off * 2 + 1] = h[2 * j + 1];
            } else if (a.c.f32) {
                reinterpret_cast<float *>(a.c.hT_ptr)[off] = h[j];
            } else {
                reinterpret_cast<T *>(a.c.hT_ptr)[off] = from_f32<T>(h[j]);
            }
        }
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------------------------
// gradients follow torch.autograd's convention for complex leaves: grad = dL/dRe + i dL/dIm, propagated with conjugates
template <typename T, bool kCplx, bool kVarB, bool kVarC, int kNB, int kMaxThreads, bool kVarlen>
__global__ __launch_bounds__(kMaxThreads) void ssm_scan_general_bwd_kernel(const gen_args_t a) {
    static_assert(!kVarlen || (!kCplx && kVarB && kVarC), "packed rows: real A with input-dependent B and C");
    using Cfg = GenCfg<kCplx, kNB>;
    constexpr int kK = Cfg::kK, kT = Cfg::kT, kRow = Cfg::kRow, kS = kNB * kK;
    extern __shared__ float red[];                      // [wave][du | ddelta][step][lane]
    const dimsum_ssm_general_params_t &p = a.f;
    const dimsum_ssm_general_bwd_params_t &r = a.b;
    gen_pos_t q;
    q.lane = threadIdx.x & 63;
    q.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    q.b = blockIdx.y;
    q.g = blockIdx.x / a.cblocks;
    const int dpg = p.dim / p.n_groups;
    const int dg = (blockIdx.x % a.cblocks) * 64 + q.lane;
    q.live = dg < dpg;
    q.d = q.g * dpg + (q.live ? dg : 0);
    q.n0 = q.wave * kNB;
    const int W = blockDim.x >> 6, L = p.seqlen, N = p.dstate;
    const int ntiles = (L + kT - 1) / kT;

    float A[kS], Bc[kS], Cc[kS], h[kS];
    load_weight_rows<kCplx, kNB>(p.A_ptr, p.A_d_stride, p.A_dstate_stride, q, N, A);
    if constexpr (!kVarB) load_weight_rows<kCplx, kNB>(p.B_ptr, p.B_d_stride, p.B_dstate_stride, q, N, Bc);
    if constexpr (!kVarC) load_weight_rows<kCplx, kNB>(p.C_ptr, p.C_d_stride, p.C_dstate_stride, q, N, Cc);
    const float bias = (p.delta_bias_ptr && q.live) ? reinterpret_cast<const float *>(p.delta_bias_ptr)[q.d] : 0.f;
    const float Dd = (p.D_ptr && q.live) ? reinterpret_cast<const float *>(p.D_ptr)[q.d] : 0.f;
    const bool sp = p.delta_softplus != 0;
    const int64_t u_row = q.b * p.u_batch_stride + q.d * p.u_d_stride, dl_row = q.b * p.delta_batch_stride + q.d * p.delta_d_stride;
    const int64_t do_row = q.b * r.dout_batch_stride + q.d * r.dout_d_stride, z_row = q.b * p.z_batch_stride + q.d * p.z_d_stride;
    // saved states: (batch, tile, state real, padded channel) f32; this lane's column
    float *ck = reinterpret_cast<float *>(r.workspace_ptr) + ((int64_t)q.b * ntiles * N * kK) * a.dpad + (int64_t)blockIdx.x * 64 + q.lane;

    const int32_t *ids = kVarlen ? a.seq_idx + (int64_t)q.b * a.seq_batch_stride : nullptr;

    // 1. forward sweep: the state before every tile
#pragma unroll
    for (int j = 0; j < kS; ++j) h[j] = 0.f;
    for (int tile = 0; tile < ntiles; ++tile) {
        const int t0 = tile * kT;
#pragma unroll
        for (int j = 0; j < kNB; ++j)
            if (q.n0 + j < N) {
#pragma unroll
                for (int c = 0; c < kK; ++c) ck[((int64_t)tile * N * kK + (q.n0 + j) * kK + c) * a.dpad] = h[j * kK + c];
            }
        if (tile == ntiles - 1) break;
        unsigned rm = 0;
        if constexpr (kVarlen) rm = reset_mask<kT>(ids, t0, L);
        float bt = 0.f;
        if constexpr (kVarB) bt = load_bc_tile<T, kCplx, kNB>(p.B_ptr, p.B_batch_stride, p.B_group_stride, p.B_dstate_stride, q, N, L, t0);
#pragma unroll
        for (int i = 0; i < kT; ++i) {
            const bool ok = q.live && t0 + i < L;
            const float uv = ok ? ld_f32<T>(p.u_ptr, u_row + t0 + i) : 0.f;
            const float dt = ok ? delta_of(ld_f32<T>(p.delta_ptr, dl_row + t0 + i), bias, sp) : 0.f;
            const float dtu = dt * uv;
#pragma unroll
            for (int j = 0; j < kNB; ++j) {
                float pr, pi;
                decay<kCplx>(dt, A[j * kK], kCplx ? A[j * kK + kK - 1] : 0.f, pr, pi);
                if constexpr (kCplx) {
                    const float br = kVarB ? lane_value(bt, j * kRow + 2 * i) : Bc[2 * j], bi = kVarB ? lane_value(bt, j * kRow + 2 * i + 1) : Bc[2 * j + 1];
                    const float hr = h[2 * j], hi = h[2 * j + 1];
                    h[2 * j] = fmaf(pr, hr, fmaf(-pi, hi, dtu * br));
                    h[2 * j + 1] = fmaf(pr, hi, fmaf(pi, hr, dtu * bi));
                } else {
                    const float bv = kVarB ? lane_value(bt, j * kRow + i) : Bc[j];
                    h[j] = fmaf(pr, kVarlen && ((rm >> i) & 1u) ? 0.f : h[j], dtu * bv);
                }
            }
        }
    }

    // 2. the tiles from the last to the first
    float gc[kS], dA[kS], dBc[kS], dCc[kS];             // gc = conj(a_{t+1}) g_{t+1}: what the later steps hand to step t
#pragma unroll
    for (int j = 0; j < kS; ++j) gc[j] = dA[j] = dBc[j] = dCc[j] = 0.f;
    float dD = 0.f, dbias = 0.f;
    for (int tile = ntiles - 1; tile >= 0; --tile) {
        const int t0 = tile * kT;
        unsigned rm = 0;
        if constexpr (kVarlen) rm = reset_mask<kT>(ids, t0, L);
        float uv[kT], dt[kT], dy[kT], du[kT], ddt[kT], hs[kT][kS];
#pragma unroll
        for (int i = 0; i < kT; ++i) {
            const bool ok = q.live && t0 + i < L;
            uv[i] = ok ? ld_f32<T>(p.u_ptr, u_row + t0 + i) : 0.f;
            dt[i] = ok ? delta_of(ld_f32<T>(p.delta_ptr, dl_row + t0 + i), bias, sp) : 0.f;
            dy[i] = ok ? ld_f32<T>(r.dout_ptr, do_row + t0 + i) : 0.f;
            if (p.z_ptr && ok) {
                const float z = ld_f32<T>(p.z_ptr, z_row + t0 + i);
                dy[i] *= z * sigmoidf_fast(z);
            }
            du[i] = ddt[i] = 0.f;
        }
        float bt = 0.f, ct = 0.f;
        if constexpr (kVarB) bt = load_bc_tile<T, kCplx, kNB>(p.B_ptr, p.B_batch_stride, p.B_group_stride, p.B_dstate_stride, q, N, L, t0);
        if constexpr (kVarC) ct = load_bc_tile<T, kCplx, kNB>(p.C_ptr, p.C_batch_stride, p.C_group_stride, p.C_dstate_stride, q, N, L, t0);
#pragma unroll
        for (int j = 0; j < kNB; ++j) {
#pragma unroll
            for (int c = 0; c < kK; ++c) h[j * kK + c] = (q.n0 + j < N) ? ck[((int64_t)tile * N * kK + (q.n0 + j) * kK + c) * a.dpad] : 0.f;
        }
        // the tile's states
#pragma unroll
        for (int i = 0; i < kT; ++i) {
            const float dtu = dt[i] * uv[i];
#pragma unroll
            for (int j = 0; j < kNB; ++j) {
                float pr, pi;
                decay<kCplx>(dt[i], A[j * kK], kCplx ? A[j * kK + kK - 1] : 0.f, pr, pi);
                if constexpr (kCplx) {
                    const float br = kVarB ? lane_value(bt, j * kRow + 2 * i) : Bc[2 * j], bi = kVarB ? lane_value(bt, j * kRow + 2 * i + 1) : Bc[2 * j + 1];
                    const float hr = h[2 * j], hi = h[2 * j + 1];
                    h[2 * j] = fmaf(pr, hr, fmaf(-pi, hi, dtu * br));
                    h[2 * j + 1] = fmaf(pr, hi, fmaf(pi, hr, dtu * bi));
                    hs[i][2 * j] = h[2 * j];
                    hs[i][2 * j + 1] = h[2 * j + 1];
                } else {
                    const float bv = kVarB ? lane_value(bt, j * kRow + i) : Bc[j];
                    h[j] = fmaf(pr, kVarlen && ((rm >> i) & 1u) ? 0.f : h[j], dtu * bv);
                    hs[i][j] = h[j];
                }
            }
        }
        // the adjoint recurrence, backwards
        float dBt = 0.f, dCt = 0.f;                      // this lane's element of the tile's dB / dC (input-dependent B / C)
#pragma unroll
        for (int i = kT - 1; i >= 0; --i) {
            const float dtu = dt[i] * uv[i];
#pragma unroll
            for (int j = 0; j < kNB; ++j) {
                float pr, pi;
                decay<kCplx>(dt[i], A[j * kK], kCplx ? A[j * kK + kK - 1] : 0.f, pr, pi);
                if constexpr (kCplx) {
                    const float br = kVarB ? lane_value(bt, j * kRow + 2 * i) : Bc[2 * j], bi = kVarB ? lane_value(bt, j * kRow + 2 * i + 1) : Bc[2 * j + 1];
                    const float cr = kVarC ? lane_value(ct, j * kRow + 2 * i) : Cc[2 * j], ci = kVarC ? lane_value(ct, j * kRow + 2 * i + 1) : Cc[2 * j + 1];
                    const float hr = hs[i][2 * j], hi = hs[i][2 * j + 1];
                    // y = 2 Re(C h): g = 2 conj(C) dy + carry;  dC = 2 conj(h) dy
                    const float gr = fmaf(2.f * cr, dy[i], gc[2 * j]), gi = fmaf(-2.f * ci, dy[i], gc[2 * j + 1]);
                    const float dcr = 2.f * hr * dy[i], dci = -2.f * hi * dy[i];
                    // a h_{t-1} = h_t - dt u B; at the row's first step h_{-1} = 0: 0 by definition, not the rounding of dt u B left by the difference
                    const bool first = t0 + i == 0;
                    const float ahr = first ? 0.f : fmaf(-dtu, br, hr), ahi = first ? 0.f : fmaf(-dtu, bi, hi);
                    // conj(B) g, conj(a h_{t-1}) g
                    const float bgr = br * gr + bi * gi;
                    const float qr = ahr * gr + ahi * gi, qi = ahr * gi - ahi * gr;
                    du[i] = fmaf(dt[i], bgr, du[i]);
                    // d dt: Re(conj(B u) g) + Re(conj(A) conj(a h_{t-1}) g)
                    ddt[i] += uv[i] * bgr + (A[2 * j] * qr + A[2 * j + 1] * qi);
                    dA[2 * j] = fmaf(dt[i], qr, dA[2 * j]);
                    dA[2 * j + 1] = fmaf(dt[i], qi, dA[2 * j + 1]);
                    const float dbr = dtu * gr, dbi = dtu * gi;
                    if constexpr (kVarB) {
                        const float s0 = wave_allsum(dbr), s1 = wave_allsum(dbi);
                        dBt = q.lane == j * kRow + 2 * i ? s0 : (q.lane == j * kRow + 2 * i + 1 ? s1 : dBt);
                    } else {
                        dBc[2 * j] += dbr;
                        dBc[2 * j + 1] += dbi;
                    }
                    if constexpr (kVarC) {
                        const float s0 = wave_allsum(dcr), s1 = wave_allsum(dci);
                        dCt = q.lane == j * kRow + 2 * i ? s0 : (q.lane == j * kRow + 2 * i + 1 ? s1 : dCt);
                    } else {
                        dCc[2 * j] += dcr;
                        dCc[2 * j + 1] += dci;
                    }
                    gc[2 * j] = pr * gr + pi * gi;       // conj(a) g
                    gc[2 * j + 1] = pr * gi - pi * gr;
                } else {
                    const float bv = kVarB ? lane_value(bt, j * kRow + i) : Bc[j], cv = kVarC ? lane_value(ct, j * kRow + i) : Cc[j];
                    const float hv = hs[i][j];
                    const float g = fmaf(cv, dy[i], gc[j]);
                    // a boundary, or the row's first step (h_{-1} = 0): a_t h_{t-1} is 0 by definition, not by cancellation
                    const bool rst = (kVarlen && ((rm >> i) & 1u)) || t0 + i == 0;
                    const float ah = rst ? 0.f : fmaf(-dtu, bv, hv);
                    const float bg = bv * g, qg = ah * g;
                    du[i] = fmaf(dt[i], bg, du[i]);
                    ddt[i] += uv[i] * bg + A[j] * qg;
                    dA[j] = fmaf(dt[i], qg, dA[j]);
                    const float db = dtu * g, dc = hv * dy[i];
                    if constexpr (kVarB) {
                        const float s = wave_allsum(db);
                        dBt = q.lane == j * kRow + i ? s : dBt;
                    } else {
                        dBc[j] += db;
                    }
                    if constexpr (kVarC) {
                        const float s = wave_allsum(dc);
                        dCt = q.lane == j * kRow + i ? s : dCt;
                    } else {
                        dCc[j] += dc;
                    }
                    gc[j] = rst ? 0.f : pr * g;                             // nothing is handed to the previous segment
                }
            }
        }
        if constexpr (kVarB || kVarC) {
            const int j = q.lane / kRow, i = q.lane % kRow;
            const int64_t col = (int64_t)t0 * kK + i;
            if (q.n0 + j < N && col < (int64_t)L * kK) {
                if constexpr (kVarB)
                    unsafeAtomicAdd(reinterpret_cast<float *>(r.dB_ptr) + q.b * r.dB_batch_stride + q.g * r.dB_group_stride + (q.n0 + j) * r.dB_dstate_stride + col, dBt);
                if constexpr (kVarC)
                    unsafeAtomicAdd(reinterpret_cast<float *>(r.dC_ptr) + q.b * r.dC_batch_stride + q.g * r.dC_group_stride + (q.n0 + j) * r.dC_dstate_stride + col, dCt);
            }
        }
#pragma unroll
        for (int i = 0; i < kT; ++i) {
            red[((q.wave * 2 + 0) * kT + i) * 64 + q.lane] = du[i];
            red[((q.wave * 2 + 1) * kT + i) * 64 + q.lane] = ddt[i];
        }
        __syncthreads();
        if (q.wave == 0) {
#pragma unroll
            for (int i = 0; i < kT; ++i) {
                float su = 0.f, sd = 0.f;
                for (int w = 0; w < W; ++w) {
                    su += red[((w * 2 + 0) * kT + i) * 64 + q.lane];
                    sd += red[((w * 2 + 1) * kT + i) * 64 + q.lane];
                }
                if (q.live && t0 + i < L) {
                    const int t = t0 + i;
                    su = fmaf(Dd, dy[i], su);
                    dD = fmaf(dy[i], uv[i], dD);
                    if (sp) {                             // d softplus(x) = sigmoid(x) below the threshold (selective_scan_bwd_kernel.cuh)
                        const float x = ld_f32<T>(p.delta_ptr, dl_row + t) + bias;
                        sd = x <= 20.f ? sd * sigmoidf_fast(x) : sd;
                    }
                    dbias += sd;
                    reinterpret_cast<T *>(r.du_ptr)[q.b * r.du_batch_stride + q.d * r.du_d_stride + t] = from_f32<T>(su);
                    reinterpret_cast<T *>(r.ddelta_ptr)[q.b * r.ddelta_batch_stride + q.d * r.ddelta_d_stride + t] = from_f32<T>(sd);
                    if (p.z_ptr) {
                        const float z = ld_f32<T>(p.z_ptr, z_row + t), s = sigmoidf_fast(z);
                        const float o = ld_f32<T>(p.out_ptr, q.b * p.out_batch_stride + q.d * p.out_d_stride + t);
                        const float dout = ld_f32<T>(r.dout_ptr, do_row + t);
                        reinterpret_cast<T *>(r.dz_ptr)[q.b * r.dz_batch_stride + q.d * r.dz_d_stride + t] = from_f32<T>(dout * o * s * (1.f + z * (1.f - s)));
                    }
                }
            }
        }
        __syncthreads();
    }

    // 3. the sums over time: added across the batch with atomics
    if (q.live) {
        float *dAp = reinterpret_cast<float *>(r.dA_ptr);
#pragma unroll
        for (int j = 0; j < kNB; ++j) {
            if (q.n0 + j < N) {
#pragma unroll
                for (int c = 0; c < kK; ++c) {
                    unsafeAtomicAdd(dAp + ((int64_t)q.d * r.dA_d_stride + (int64_t)(q.n0 + j) * r.dA_dstate_stride) * kK + c, dA[j * kK + c]);
                    if constexpr (!kVarB)
                        unsafeAtomicAdd(reinterpret_cast<float *>(r.dB_ptr) + ((int64_t)q.d * r.dB_d_stride + (int64_t)(q.n0 + j) * r.dB_dstate_stride) * kK + c, dBc[j * kK + c]);
                    if constexpr (!kVarC)
                        unsafeAtomicAdd(reinterpret_cast<float *>(r.dC_ptr) + ((int64_t)q.d * r.dC_d_stride + (int64_t)(q.n0 + j) * r.dC_dstate_stride) * kK + c, dCc[j * kK + c]);
                }
            }
        }
        if (q.wave == 0) {
            if (r.dD_ptr) unsafeAtomicAdd(reinterpret_cast<float *>(r.dD_ptr) + q.d, dD);
            if (r.ddelta_bias_ptr) unsafeAtomicAdd(reinterpret_cast<float *>(r.ddelta_bias_ptr) + q.d, dbias);
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------
// One check (gen_check; an entry's own fields around it), one fill (gen_fill), one launch (gen_run -> gen_launch). DESIGN.md section 3.14a.
constexpr int kGenNB = 16;                  // states per wave: <= 4 waves up to 64 states (256 work-items: the whole register file), else <= 16
static int gen_tile_steps(bool cplx) { return 64 / kGenNB / (cplx ? 2 : 1); }

static int64_t gen_ckpt_bytes(int32_t batch, int32_t dim, int32_t seqlen, int32_t dstate, int32_t n_groups, bool cplx) {
    const int kT = gen_tile_steps(cplx);
    const int64_t ntiles = (seqlen + kT - 1) / kT, cblocks = (dim / n_groups + 63) / 64;
    return (int64_t)batch * ntiles * dstate * (cplx ? 2 : 1) * (n_groups * cblocks * 64) * (int64_t)sizeof(float);
}

static bool gen_shape_ok(int32_t batch, int32_t dim, int32_t seqlen, int32_t dstate, int32_t n_groups) {
    return batch >= 1 && batch <= 65535 && dim >= 1 && seqlen >= 1 && dstate >= 1 && dstate <= 256 && n_groups >= 1 && dim % n_groups == 0;
}

struct gen_ids_t {                          // the seq_idx of a packed-row entry, as its struct names it
    const void *ptr;
    int64_t batch_stride;
};

// a (batch, seqlen) int32 row operand (seq_idx, end_slots): a batch stride that lets rows overlap
static bool gen_row_stride_bad(int64_t batch_stride, const dimsum_ssm_general_params_t &p) { return batch_stride < 0 || (p.batch > 1 && batch_stride < p.seqlen); }

// packed rows, behind the general checks: the ids (NULL, then their batch stride), then what has no kVarlen instantiation
static int gen_varlen_check(const dimsum_ssm_general_params_t &p, const gen_ids_t &ids) {
    if (!ids.ptr) return DIMSUM_ERR_NULL;
    if (gen_row_stride_bad(ids.batch_stride, p)) return DIMSUM_ERR_STRIDE;
    if (p.is_complex || !p.is_variable_B || !p.is_variable_C) return DIMSUM_ERR_UNSUPPORTED;
    return DIMSUM_OK;
}

// THE check of every entry point, behind its own NULL / struct_size test, in this order: required pointers, shape, dtype, strides; then, where
// the entry has ids and nothing of its own in between, gen_varlen_check
static int gen_check(const dimsum_ssm_general_params_t &p, bool forward, const gen_ids_t *ids = nullptr) {
    if (!p.A_ptr || !p.B_ptr || !p.C_ptr || !p.u_ptr || !p.delta_ptr) return DIMSUM_ERR_NULL;
    if (forward && p.z_ptr && !p.out_z_ptr) return DIMSUM_ERR_NULL;
    if (!gen_shape_ok(p.batch, p.dim, p.seqlen, p.dstate, p.n_groups)) return DIMSUM_ERR_SHAPE;
    if (p.n_chunks != (p.seqlen + kGenChunk - 1) / kGenChunk) return DIMSUM_ERR_SHAPE;
    if (!p.is_variable_B && !p.is_variable_C && p.n_groups != 1) return DIMSUM_ERR_SHAPE;      // groups belong to input-dependent B / C
    if (p.dtype < DIMSUM_F32 || p.dtype > DIMSUM_BF16) return DIMSUM_ERR_DTYPE;
    if (any_negative({p.A_d_stride, p.A_dstate_stride, p.B_batch_stride, p.B_d_stride, p.B_group_stride, p.B_dstate_stride, p.C_batch_stride, p.C_d_stride,
                      p.C_group_stride, p.C_dstate_stride, p.u_batch_stride, p.u_d_stride, p.delta_batch_stride, p.delta_d_stride, p.z_batch_stride,
                      p.z_d_stride, p.out_batch_stride, p.out_d_stride, p.out_z_batch_stride, p.out_z_d_stride}))
        return DIMSUM_ERR_STRIDE;
    if (p.x_ptr && !aligned_to<float>(p.x_ptr, 8)) return DIMSUM_ERR_STRIDE;
    return ids ? gen_varlen_check(p, *ids) : DIMSUM_OK;
}

// THE fill: the kernel argument of an entry -- zeroed, the scan's struct, the ids where it has them; what else an entry has it sets itself
template <typename Args> static Args gen_fill(const dimsum_ssm_general_params_t &f, const gen_ids_t *ids = nullptr) {
    Args a;
    memset(&a, 0, sizeof(a));
    a.f = f;
    if (ids) a.seq_idx = reinterpret_cast<const int32_t *>(ids->ptr), a.seq_batch_stride = ids->batch_stride;
    return a;
}

// THE launch: kFwd / kVarlen / kEmit / kStart pick the kernel family, Args (gen_args_t; gen_emit_args_t with kEmit; gen_start_args_t with kStart)
// is its argument. One launch shape for all.
template <typename T, bool kCplx, bool kVarB, bool kVarC, bool kFwd, bool kVarlen, bool kEmit, bool kStart, typename Args>
static int gen_launch(const Args &a, hipStream_t s) {
    const dimsum_ssm_general_params_t &p = a.f;
    const int W = (p.dstate + kGenNB - 1) / kGenNB, kT = gen_tile_steps(kCplx);
    const dim3 grid((unsigned)(p.n_groups * a.cblocks), (unsigned)p.batch), block((unsigned)(64 * W));
    const size_t lds = (size_t)W * kT * 64 * sizeof(float) * (kFwd ? 1 : 2);
    auto launch = [&](auto max_threads) {
        constexpr int kMax = decltype(max_threads)::value;
        if constexpr (kFwd) hipLaunchKernelGGL((ssm_scan_general_fwd_kernel<T, kCplx, kVarB, kVarC, kGenNB, kMax, kVarlen, kEmit, kStart>), grid, block, lds, s, a);
        else hipLaunchKernelGGL((ssm_scan_general_bwd_kernel<T, kCplx, kVarB, kVarC, kGenNB, kMax, kVarlen>), grid, block, lds, s, a);
    };
    // up to 64 states a workgroup is at most 4 waves, one per SIMD: the kernel may use the whole register file (512 per lane); above, up to
    // 16 waves share it (128 each)
    if (W <= 4) launch(std::integral_constant<int, 256>{});
    else launch(std::integral_constant<int, 1024>{});
    return launch_status();
}

// THE run of every entry point, behind its checks: the padded channel counts, the element type, the (complex, varB, varC) case. Packed rows
// (kVarlen, and kEmit and kStart on top of it) exist for real A with input-dependent B / C alone: gen_varlen_check lets nothing else through.
template <bool kFwd, bool kVarlen, bool kEmit = false, bool kStart = false, typename Args> static int gen_run(Args &a, void *stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    a.cblocks = (a.f.dim / a.f.n_groups + 63) / 64;
    a.dpad = (int64_t)a.f.n_groups * a.cblocks * 64;
    return dispatch_dtype(a.f.dtype, [&](auto t) {
        using T = decltype(t);
        if constexpr (kVarlen) {
            return gen_launch<T, false, true, true, kFwd, true, kEmit, kStart>(a, s);
        } else {
            const bool c = a.f.is_complex != 0, vb = a.f.is_variable_B != 0, vc = a.f.is_variable_C != 0;
#define DIMSUM_GEN_CASE(C, VB, VC) \
    if (c == C && vb == VB && vc == VC) return gen_launch<T, C, VB, VC, kFwd, false, false, false>(a, s)
            DIMSUM_GEN_CASE(false, true, true);
            DIMSUM_GEN_CASE(false, true, false);
            DIMSUM_GEN_CASE(false, false, true);
            DIMSUM_GEN_CASE(false, false, false);
            DIMSUM_GEN_CASE(true, true, true);
            DIMSUM_GEN_CASE(true, true, false);
            DIMSUM_GEN_CASE(true, false, true);
#undef DIMSUM_GEN_CASE
            return gen_launch<T, true, false, false, kFwd, false, false, false>(a, s);      // the eighth of eight
        }
    });
}

// the backward's checks behind NULL / struct_size and its launch; ids != NULL: packed rows
static int gen_bwd(const dimsum_ssm_general_bwd_params_t *p, const gen_ids_t *ids, void *stream) {
    const dimsum_ssm_general_params_t &f = p->fwd;
    const int rc = gen_check(f, false);
    if (rc == DIMSUM_ERR_NULL) return rc;
    if (!p->dout_ptr || !p->dA_ptr || !p->dB_ptr || !p->dC_ptr || !p->du_ptr || !p->ddelta_ptr || !p->workspace_ptr) return DIMSUM_ERR_NULL;
    if (f.z_ptr && (!p->dz_ptr || !f.out_ptr)) return DIMSUM_ERR_NULL;
    if (rc != DIMSUM_OK) return rc;
    if (any_negative({p->dout_batch_stride, p->dout_d_stride, p->dA_d_stride, p->dA_dstate_stride, p->dB_batch_stride, p->dB_d_stride, p->dB_group_stride,
                      p->dB_dstate_stride, p->dC_batch_stride, p->dC_d_stride, p->dC_group_stride, p->dC_dstate_stride, p->du_batch_stride, p->du_d_stride,
                      p->dz_batch_stride, p->dz_d_stride, p->ddelta_batch_stride, p->ddelta_d_stride}))
        return DIMSUM_ERR_STRIDE;
    if (!aligned_to<float>(p->workspace_ptr, 16)) return DIMSUM_ERR_STRIDE;
    if (p->workspace_bytes < gen_ckpt_bytes(f.batch, f.dim, f.seqlen, f.dstate, f.n_groups, f.is_complex != 0)) return DIMSUM_ERR_SHAPE;
    if (ids)
        if (const int rc_ids = gen_varlen_check(f, *ids)) return rc_ids;
    gen_args_t a = gen_fill<gen_args_t>(f, ids);
    a.b = *p;
    return ids ? gen_run<false, true>(a, stream) : gen_run<false, false>(a, stream);
}

// dimsum_ssm_scan_varlen_states_fwd behind NULL / struct_size: its own fields, then the packed-row checks; the resume entry runs the same
static int gen_states_check(const dimsum_ssm_varlen_states_params_t &p) {
    if (p.num_slots < 1) return DIMSUM_ERR_SHAPE;
    if (!p.end_slots_ptr || !p.state_ptr) return DIMSUM_ERR_NULL;
    const dimsum_ssm_general_params_t &f = p.varlen.scan;
    if (gen_row_stride_bad(p.end_slots_batch_stride, f) || any_negative({p.state_slot_stride, p.state_d_stride, p.state_dstate_stride})) return DIMSUM_ERR_STRIDE;
    const gen_ids_t ids{p.varlen.seq_idx_ptr, p.varlen.seq_idx_batch_stride};
    return gen_check(f, true, &ids);
}

// ... and its fill: the ids, end_slots and the pool
template <typename Args> static Args gen_states_fill(const dimsum_ssm_varlen_states_params_t &p) {
    const dimsum_ssm_general_params_t &f = p.varlen.scan;
    const gen_ids_t ids{p.varlen.seq_idx_ptr, p.varlen.seq_idx_batch_stride};
    Args e = gen_fill<Args>(f, &ids);
    e.end_slots = reinterpret_cast<const int32_t *>(p.end_slots_ptr);
    e.end_batch_stride = p.end_slots_batch_stride;
    e.pool = p.state_ptr;
    e.pool_slot_stride = p.state_slot_stride, e.pool_d_stride = p.state_d_stride, e.pool_dstate_stride = p.state_dstate_stride;
    e.pool_f32 = p.state_f32 != 0 || f.dtype == DIMSUM_F32;
    return e;
}

}  // namespace dimsum

extern "C" int dimsum_ssm_scan_general_fwd(const dimsum_ssm_general_params_t *p, void *stream) {
    using namespace dimsum;
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_ssm_general_params_t)) return DIMSUM_ERR_ABI;
    if (const int rc = gen_check(*p, true)) return rc;
    gen_args_t a = gen_fill<gen_args_t>(*p);
    return gen_run<true, false>(a, stream);
}

extern "C" int dimsum_ssm_scan_carry_fwd(const dimsum_ssm_carry_params_t *p, void *stream) {
    using namespace dimsum;
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_ssm_carry_params_t)) return DIMSUM_ERR_ABI;
    const bool carried = p->h0_ptr || p->hT_ptr;
    const int rc = gen_check(p->scan, true);
    // gen_check stops at its first failure, in the documented order: the state's dtype belongs right after the scan's, before any stride
    if (rc != DIMSUM_OK && rc != DIMSUM_ERR_STRIDE) return rc;
    if (carried && p->state_dtype != DIMSUM_F32 && (p->scan.is_complex || p->state_dtype != p->scan.dtype)) return DIMSUM_ERR_DTYPE;
    if (rc != DIMSUM_OK) return rc;
    if (carried && any_negative({p->h0_batch_stride, p->h0_d_stride, p->h0_dstate_stride, p->hT_batch_stride, p->hT_d_stride, p->hT_dstate_stride}))
        return DIMSUM_ERR_STRIDE;
    gen_args_t a = gen_fill<gen_args_t>(p->scan);
    a.c = {p->h0_ptr, p->hT_ptr, p->h0_batch_stride, p->h0_d_stride, p->h0_dstate_stride, p->hT_batch_stride, p->hT_d_stride, p->hT_dstate_stride,
           p->state_dtype == DIMSUM_F32};
    return gen_run<true, false>(a, stream);
}

extern "C" int64_t dimsum_ssm_scan_general_bwd_workspace_bytes(int32_t batch, int32_t dim, int32_t seqlen, int32_t dstate, int32_t n_groups, int32_t is_complex) {
    using namespace dimsum;
    if (!gen_shape_ok(batch, dim, seqlen, dstate, n_groups)) return -1;
    return gen_ckpt_bytes(batch, dim, seqlen, dstate, n_groups, is_complex != 0);
}

extern "C" int dimsum_ssm_scan_general_bwd(const dimsum_ssm_general_bwd_params_t *p, void *stream) {
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_ssm_general_bwd_params_t)) return DIMSUM_ERR_ABI;
    return dimsum::gen_bwd(p, nullptr, stream);
}

extern "C" int dimsum_ssm_scan_varlen_bwd(const dimsum_ssm_varlen_bwd_params_t *p, void *stream) {
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_ssm_varlen_bwd_params_t)) return DIMSUM_ERR_ABI;
    const dimsum::gen_ids_t ids{p->seq_idx_ptr, p->seq_idx_batch_stride};
    return dimsum::gen_bwd(&p->bwd, &ids, stream);
}

extern "C" int dimsum_ssm_scan_varlen_fwd(const dimsum_ssm_varlen_params_t *p, void *stream) {
    using namespace dimsum;
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_ssm_varlen_params_t)) return DIMSUM_ERR_ABI;
    const gen_ids_t ids{p->seq_idx_ptr, p->seq_idx_batch_stride};
    if (const int rc = gen_check(p->scan, true, &ids)) return rc;
    gen_args_t a = gen_fill<gen_args_t>(p->scan, &ids);
    return gen_run<true, true>(a, stream);
}

extern "C" int dimsum_ssm_scan_varlen_states_fwd(const dimsum_ssm_varlen_states_params_t *p, void *stream) {
    using namespace dimsum;
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_ssm_varlen_states_params_t)) return DIMSUM_ERR_ABI;
    if (const int rc = gen_states_check(*p)) return rc;
    gen_emit_args_t e = gen_states_fill<gen_emit_args_t>(*p);
    return gen_run<true, true, true>(e, stream);
}

extern "C" int dimsum_ssm_scan_varlen_resume_fwd(const dimsum_ssm_varlen_resume_params_t *p, void *stream) {
    using namespace dimsum;
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_ssm_varlen_resume_params_t)) return DIMSUM_ERR_ABI;
    if (p->n_init < 1) return DIMSUM_ERR_SHAPE;
    if (!p->start_slots_ptr || !p->init_ptr) return DIMSUM_ERR_NULL;
    const dimsum_ssm_general_params_t &f = p->states.varlen.scan;
    if (gen_row_stride_bad(p->start_slots_batch_stride, f) || any_negative({p->init_slot_stride, p->init_d_stride, p->init_dstate_stride})) return DIMSUM_ERR_STRIDE;
    if (const int rc = gen_states_check(p->states)) return rc;
    gen_start_args_t e = gen_states_fill<gen_start_args_t>(p->states);
    e.start_slots = reinterpret_cast<const int32_t *>(p->start_slots_ptr);
    e.start_batch_stride = p->start_slots_batch_stride;
    e.init = p->init_ptr;
    e.init_slot_stride = p->init_slot_stride, e.init_d_stride = p->init_d_stride, e.init_dstate_stride = p->init_dstate_stride;
    e.init_f32 = p->init_f32 != 0 || f.dtype == DIMSUM_F32;
    return gen_run<true, true, true, true>(e, stream);
}
