// moe.hip -- the row passes of the top-1 mixture-of-experts layer (SwitchMLP: dimsum/switch_mlp.py:69-99, expert dimsum/mlp.py:7-46) around the
// per-expert GEMMs the host runs over contiguous row slices:
//   route_fwd   : router dot products + sigmoid / softmax + first-argmax per token, then a stable counting sort of the tokens by expert
//                 (three launches: route + per-block counts, scan of the counts, placement). No atomic decides a position.
//   permute     : xp[j] = x[perm[j]]                                  combine_fwd : out[perm[j]] = prob[perm[j]] y[j] (every token written once)
//   (the experts' activation between the two GEMMs, dimsum_moe_act_fwd / _bwd, is one of the activation row passes of act_rows.hip)
//   combine_bwd : dy[j] = prob[t] dout[t], dprob[t] = <dout[t], y[j]>   route_bwd : dx = dxp[inv] + dlogit W_r, dW_r, db_r
// All fp32 rows with width % 4 == 0 and 16-byte accesses; 1 <= E <= 64. HBM-bound: bytes per element are listed in DESIGN.md section 3.15.
#include "common.hpp"

namespace dimsum {
namespace {

constexpr int kBlk = 64;          // tokens per workgroup of the route pass = per wave of the placement pass: the unit of the counting sort
constexpr int kXr = 8;            // 16-byte pieces of a token's row a lane keeps in registers across the experts (rows up to 2048 columns)
constexpr int kRows = 64;         // tokens per tile of the router's backward (their dlogit values sit in LDS)
constexpr int kEG = 8;            // experts per register group of the router's backward

__device__ __forceinline__ float wave_allsum(float v) {        // butterfly: every lane ends with the same bits
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float dot4(const float4 &a, const float4 &b, float acc) {
    return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, fmaf(a.x, b.x, acc))));
}

// ---- pass a: one wave per token, 16 tokens per wave, kBlk tokens per workgroup. The E dot products of a token run through the same loop and the
// same butterfly, so identical router rows give identical logits. Lane e ends up holding logit e.
template <bool kSigmoid>
__global__ __launch_bounds__(256) void moe_route_kernel(const float *x, const float *w, const float *b, float *prob, int *expert, float *logits,
                                                        int *counts, int64_t T, int64_t H, int E) {
    __shared__ int cnt[64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x < 64) cnt[threadIdx.x] = 0;
    __syncthreads();
    const int64_t t0 = (int64_t)blockIdx.x * kBlk + wv * (kBlk / 4);
    for (int i = 0; i < kBlk / 4; ++i) {
        const int64_t t = t0 + i;
        if (t >= T) break;                                   // (wave-uniform)
        const float *xr = x + t * H;
        float4 xv[kXr];
#pragma unroll
        for (int k = 0; k < kXr; ++k) {
            const int64_t c = ((int64_t)k * 64 + lane) * 4;
            xv[k] = c < H ? ldf4(xr + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        float mine = -INFINITY;
        for (int e = 0; e < E; ++e) {
            const float *wr = w + (int64_t)e * H;
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < kXr; ++k) {
                const int64_t c = ((int64_t)k * 64 + lane) * 4;
                if (c < H) acc = dot4(xv[k], ldf4(wr + c), acc);
            }
            for (int64_t c = ((int64_t)kXr * 64 + lane) * 4; c < H; c += 256) acc = dot4(ldf4(xr + c), ldf4(wr + c), acc);
            acc = wave_allsum(acc);
            if (lane == e) mine = acc + (b ? b[e] : 0.f);
        }
        float p;
        if constexpr (kSigmoid) {
            p = lane < E ? 1.0f / (1.0f + expf(-mine)) : -INFINITY;
        } else {
            const float m = wave_allmax(mine);
            const float ex = lane < E ? expf(mine - m) : 0.f;
            const float s = wave_allsum(ex);
            p = lane < E ? ex / s : -INFINITY;
        }
        const float best = wave_allmax(p);
        const unsigned long long hit = __ballot(lane < E && p == best);
        const int es = hit ? __ffsll(hit) - 1 : 0;          // first maximum; a row of NaNs goes to expert 0
        if (lane < E) logits[t * E + lane] = mine;
        if (lane == es) {
            prob[t] = p;
            expert[t] = es;
            atomicAdd(&cnt[es], 1);                          // (a count: the order of the adds decides nothing)
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < E) counts[(int64_t)blockIdx.x * E + threadIdx.x] = cnt[threadIdx.x];
}

// ---- pass b, first half: counts (nblk, E) -> offsets (E + 1) and, in place, base[blk][e] = offsets[e] + the tokens of expert e in earlier blocks.
// One workgroup; wave w takes the experts w, w + 4, ..; a lane sums a contiguous run of blocks, the wave scans the lane sums.
__global__ __launch_bounds__(256) void moe_scan_kernel(int *counts, int *offsets, int nblk, int E) {
    __shared__ int total[64];
    __shared__ int off[65];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int seg = (nblk + 63) / 64;
    const int b0 = min(lane * seg, nblk), b1 = min(b0 + seg, nblk);
    for (int e = wv; e < E; e += 4) {
        int s = 0;
        for (int bk = b0; bk < b1; ++bk) s += counts[(int64_t)bk * E + e];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) total[e] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int a = 0;
        for (int e = 0; e < E; ++e) { off[e] = a; a += total[e]; }
        off[E] = a;
    }
    __syncthreads();
    if ((int)threadIdx.x <= E) offsets[threadIdx.x] = off[threadIdx.x];
    for (int e = wv; e < E; e += 4) {
        int s = 0;
        for (int bk = b0; bk < b1; ++bk) s += counts[(int64_t)bk * E + e];
        int inc = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(inc, o, 64);
            if (lane >= o) inc += v;
        }
        int run = off[e] + inc - s;
        for (int bk = b0; bk < b1; ++bk) {
            const int c = counts[(int64_t)bk * E + e];
            counts[(int64_t)bk * E + e] = run;
            run += c;
        }
    }
}

// ---- pass b, second half: one wave per block of kBlk tokens. A token's place = its block's base for its expert + the number of earlier lanes
// with the same expert (six ballots match the lanes bit by bit): stable in token order.
__global__ __launch_bounds__(64) void moe_place_kernel(const int *expert, const int *bases, int *perm, int *inv, int *row_expert, int64_t T, int E) {
    const int lane = threadIdx.x;
    const int64_t t = (int64_t)blockIdx.x * kBlk + lane;
    const bool valid = t < T;
    const int e = valid ? expert[t] : 0;
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 6; ++bit) {
        const bool on = (e >> bit) & 1;
        const unsigned long long bm = __ballot(on);
        peers &= on ? bm : ~bm;
    }
    if (valid) {
        const int rank = __popcll(peers & ((1ull << lane) - 1ull));
        const int64_t pos = (int64_t)bases[(int64_t)blockIdx.x * E + e] + rank;
        if (pos >= 0 && pos < T) {
            perm[pos] = (int)t;
            inv[t] = (int)pos;
            row_expert[pos] = e;
        }
    }
}

// ---- passes c and e (forward): rows moved through the sort's table. One thread = one 16-byte piece, 4 independent pieces in flight a grid stride
// apart (the flat mapping of act_rows.hip's forward). kScatter: dst[perm[j]] = prob[perm[j]] src[j], else dst[j] = src[perm[j]].
template <bool kScatter>
__global__ __launch_bounds__(256) void moe_rows_kernel(const float *src, const int *perm, const float *prob, float *dst, int64_t rows, int64_t H) {
    const int64_t q = H / 4, total = rows * q;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x; i0 < total; i0 += 4 * stride) {
        float4 a[4];
        float s[4];
        int64_t rr[4], cc[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = min(i0 + k * stride, total - 1);
            const int64_t j = i / q;
            cc[k] = (i - j * q) * 4;
            const int64_t t = perm[j];
            if constexpr (kScatter) { a[k] = ldf4(src + j * H + cc[k]); s[k] = prob[t]; rr[k] = t; }
            else { a[k] = ldf4(src + t * H + cc[k]); s[k] = 1.f; rr[k] = j; }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k * stride >= total) break;
            if constexpr (kScatter) stf4(dst + rr[k] * H + cc[k], make_float4(s[k] * a[k].x, s[k] * a[k].y, s[k] * a[k].z, s[k] * a[k].w));
            else stf4(dst + rr[k] * H + cc[k], a[k]);
        }
    }
}

// ---- pass c with the result as a scaled-fp16 operand image (common.hpp, f16s): one wave per sorted row j, the row x[perm[j]] held in registers
// (kXr pieces per lane: rows up to 2048 columns; wider rows read their tail twice) between the exact row maximum and the store. The image is
// rows_f16s_kernel's of the permuted rows, bit for bit: the same maximum, f16s_scales and f16s_pack4.
__global__ __launch_bounds__(256) void moe_permute_f16s_kernel(const float *src, const int *perm, __half *dst, float *inv_scale, int64_t rows, int64_t H) {
    const int lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= rows) return;                                   // (wave-uniform)
    const float *xr = src + (int64_t)perm[j] * H;
    float4 xv[kXr];
    float m = 0.f;
#pragma unroll
    for (int k = 0; k < kXr; ++k) {
        const int64_t c = ((int64_t)k * 64 + lane) * 4;
        xv[k] = c < H ? ldf4(xr + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        m = fmaxf(fmaxf(m, fmaxf(fabsf(xv[k].x), fabsf(xv[k].y))), fmaxf(fabsf(xv[k].z), fabsf(xv[k].w)));
    }
    for (int64_t c = ((int64_t)kXr * 64 + lane) * 4; c < H; c += 256) {
        const float4 v = ldf4(xr + c);
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
    m = wave_allmax(m);
    float sc, inv;
    f16s_scales(m, sc, inv);
    if (lane == 0) inv_scale[j] = inv;
    __half *row = dst + j * H;
#pragma unroll
    for (int k = 0; k < kXr; ++k) {
        const int64_t c = ((int64_t)k * 64 + lane) * 4;
        if (c < H) *reinterpret_cast<uint2 *>(row + c) = f16s_pack4(f32x4{{xv[k].x, xv[k].y, xv[k].z, xv[k].w}}, sc);
    }
    for (int64_t c = ((int64_t)kXr * 64 + lane) * 4; c < H; c += 256) {
        const float4 v = ldf4(xr + c);
        *reinterpret_cast<uint2 *>(row + c) = f16s_pack4(f32x4{{v.x, v.y, v.z, v.w}}, sc);
    }
}

// ---- pass e (backward): one wave per permuted row j, t = perm[j]: dy[j] = prob[t] dout[t], dprob[t] = <dout[t], y[j]>; 8 loads in flight per lane
__global__ __launch_bounds__(256) void moe_combine_bwd_kernel(const float *dout, const float *y, const int *perm, const float *prob, float *dy,
                                                              float *dprob, int64_t rows, int64_t H) {
    const int lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= rows) return;
    const int64_t t = perm[j];
    const float p = prob[t];
    float acc = 0.f;
    for (int64_t c0 = (int64_t)lane * 4; c0 < H; c0 += 1024) {
        float4 d[4], v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t c = c0 + k * 256;
            if (c < H) { d[k] = ldf4(dout + t * H + c); v[k] = ldf4(y + j * H + c); }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t c = c0 + k * 256;
            if (c < H) {
                stf4(dy + j * H + c, make_float4(p * d[k].x, p * d[k].y, p * d[k].z, p * d[k].w));
                acc = dot4(d[k], v[k], acc);
            }
        }
    }
    acc = wave_allsum(acc);
    if (lane == 0) dprob[t] = acc;
}

// ---- pass f: the router's adjoint. One workgroup = a strip of 1024 columns x rows_per_wg tokens, walked in tiles of kRows rows whose dlogit
// values (from the saved logits: p_e = exp(l_e - l_e*) p_e*) sit in LDS for a group of kEG experts; a thread keeps its 4 columns of the group's
// W_r rows and of their gradient sums in registers. dx = dxp[inv[t]] + sum_e dlogit W_r[e] (groups after the first add to what the first wrote),
// dW_r and db_r leave with one atomic per element per workgroup and group.
template <bool kSigmoid>
__global__ __launch_bounds__(256) void moe_route_bwd_kernel(const float *x, const float *w, const float *logits, const float *prob, const int *expert,
                                                            const float *dprob, const float *dxp, const int *inv, float *dx, float *dw, float *db,
                                                            int64_t T, int64_t H, int E, int rows_per_wg) {
    __shared__ float dl[kRows][kEG];
    const int tid = threadIdx.x;
    const int64_t c = ((int64_t)blockIdx.x * 256 + tid) * 4;
    const bool active = c < H;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_wg, r1 = min(T, r0 + rows_per_wg);
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int g0 = 0; g0 < E; g0 += kEG) {
        const int ne = min(kEG, E - g0);
        float4 wr[kEG];
        f32x4 acc[kEG];
#pragma unroll
        for (int k = 0; k < kEG; ++k) {
            wr[k] = (active && k < ne) ? ldf4(w + (int64_t)(g0 + k) * H + c) : zero;
            acc[k] = f32x4{{0.f, 0.f, 0.f, 0.f}};
        }
        float dbs = 0.f;
        for (int64_t s0 = r0; s0 < r1; s0 += kRows) {
            const int n = (int)min((int64_t)kRows, r1 - s0);
            __syncthreads();                                  // the previous tile has been read
            for (int idx = tid; idx < n * kEG; idx += 256) {
                const int r = idx / kEG, k = idx % kEG;
                float v = 0.f;
                if (k < ne) {
                    const int64_t t = s0 + r;
                    const int e = g0 + k, es = expert[t];
                    const float p = prob[t], dp = dprob[t];
                    if constexpr (kSigmoid) {
                        v = e == es ? dp * p * (1.0f - p) : 0.f;
                    } else {
                        const float pe = e == es ? p : expf(logits[t * E + e] - logits[t * E + es]) * p;
                        v = dp * p * ((e == es ? 1.0f : 0.f) - pe);
                    }
                }
                dl[r][k] = v;
            }
            __syncthreads();
            if (blockIdx.x == 0 && tid < ne)
                for (int r = 0; r < n; ++r) dbs += dl[r][tid];
            if (active) {
#pragma unroll 2
                for (int r = 0; r < n; ++r) {
                    const int64_t t = s0 + r;
                    const float4 x4 = ldf4(x + t * H + c);
                    float4 d = g0 == 0 ? ldf4(dxp + (int64_t)inv[t] * H + c) : ldf4(dx + t * H + c);
#pragma unroll
                    for (int k = 0; k < kEG; ++k) {
                        const float s = dl[r][k];
                        acc[k].v[0] = fmaf(s, x4.x, acc[k].v[0]); acc[k].v[1] = fmaf(s, x4.y, acc[k].v[1]);
                        acc[k].v[2] = fmaf(s, x4.z, acc[k].v[2]); acc[k].v[3] = fmaf(s, x4.w, acc[k].v[3]);
                        d.x = fmaf(s, wr[k].x, d.x); d.y = fmaf(s, wr[k].y, d.y); d.z = fmaf(s, wr[k].z, d.z); d.w = fmaf(s, wr[k].w, d.w);
                    }
                    stf4(dx + t * H + c, d);
                }
            }
        }
        if (active) {
#pragma unroll
            for (int k = 0; k < kEG; ++k) {
                if (k < ne) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) atomicAdd(dw + (int64_t)(g0 + k) * H + c + e, acc[k].v[e]);
                }
            }
        }
        if (blockIdx.x == 0 && tid < ne) atomicAdd(db + g0 + tid, dbs);
    }
}

inline bool al16(const void *p) { return aligned_to<char>(p, 16); }
inline bool al4(const void *p) { return aligned_to<char>(p, 4); }

// (every check below: struct sizes, then shapes, then -- for a call with rows -- pointers and alignment; an empty call needs no row pointers)
int route_params_ok(const dimsum_moe_route_params_t *p, bool bwd) {
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_moe_route_params_t)) return DIMSUM_ERR_ABI;
    dimsum_moe_ext_t e;
    if (const int rc = ext_from<dimsum_moe_ext_t>(p->ext, e)) return rc;
    if (p->mode != DIMSUM_MOE_ROUTE_SOFTMAX && p->mode != DIMSUM_MOE_ROUTE_SIGMOID) return DIMSUM_ERR_UNSUPPORTED;
    if (p->tokens < 0 || p->tokens >= ((int64_t)1 << 31) - kBlk || p->hidden <= 0 || p->hidden % 4 != 0 || p->num_experts < 1 || p->num_experts > 64)
        return DIMSUM_ERR_SHAPE;
    if (!bwd && (!p->offsets_ptr || !p->work_ptr)) return DIMSUM_ERR_NULL;          // (written even for zero tokens: E + 1 zeros)
    if (!bwd && p->work_bytes < dimsum_moe_route_work_bytes(p->tokens, p->num_experts)) return DIMSUM_ERR_SHAPE;
    if (!al4(p->offsets_ptr) || !al4(p->work_ptr)) return DIMSUM_ERR_STRIDE;
    if (p->tokens == 0) return DIMSUM_OK;
    if (!p->x_ptr || !p->w_ptr || !p->prob_ptr || !p->expert_ptr || !p->logits_ptr || !p->inv_ptr) return DIMSUM_ERR_NULL;
    if (!bwd && (!p->perm_ptr || !p->row_expert_ptr)) return DIMSUM_ERR_NULL;
    if (bwd && (!p->dprob_ptr || !p->dxp_ptr || !p->dx_ptr || !p->dw_ptr || !p->db_ptr)) return DIMSUM_ERR_NULL;
    if (!al16(p->x_ptr) || !al16(p->w_ptr) || !al4(p->b_ptr) || !al4(p->prob_ptr) || !al4(p->expert_ptr) || !al4(p->logits_ptr) || !al4(p->inv_ptr) ||
        !al4(p->perm_ptr) || !al4(p->row_expert_ptr) || !al4(p->dprob_ptr) || !al16(p->dxp_ptr) || !al16(p->dx_ptr) || !al4(p->dw_ptr) || !al4(p->db_ptr))
        return DIMSUM_ERR_STRIDE;
    return DIMSUM_OK;
}

int rows_params_ok(const dimsum_moe_rows_params_t *p, bool need_prob, bool bwd) {
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_moe_rows_params_t)) return DIMSUM_ERR_ABI;
    dimsum_moe_ext_t e;
    if (const int rc = ext_from<dimsum_moe_ext_t>(p->ext, e)) return rc;
    if (p->rows < 0 || p->rows >= ((int64_t)1 << 31) || p->hidden <= 0 || p->hidden % 4 != 0) return DIMSUM_ERR_SHAPE;
    if (p->rows == 0) return DIMSUM_OK;
    if (!p->src_ptr || !p->perm_ptr || !p->dst_ptr || (need_prob && !p->prob_ptr) || (bwd && (!p->y_ptr || !p->dprob_ptr))) return DIMSUM_ERR_NULL;
    if (!al16(p->src_ptr) || !al16(p->dst_ptr) || !al16(p->y_ptr) || !al4(p->perm_ptr) || !al4(p->prob_ptr) || !al4(p->dprob_ptr)) return DIMSUM_ERR_STRIDE;
    return DIMSUM_OK;
}

}  // namespace
}  // namespace dimsum

extern "C" int64_t dimsum_moe_route_work_bytes(int64_t tokens, int32_t num_experts) {
    if (tokens < 0 || num_experts < 1) return 0;
    return ((tokens + dimsum::kBlk - 1) / dimsum::kBlk) * num_experts * (int64_t)sizeof(int32_t);
}

extern "C" int dimsum_moe_route_fwd(const dimsum_moe_route_params_t *p, void *stream) {
    using namespace dimsum;
    if (const int rc = route_params_ok(p, false)) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int64_t T = p->tokens;
    const int E = p->num_experts;
    const int nblk = (int)((T + kBlk - 1) / kBlk);
    const float *x = reinterpret_cast<const float *>(p->x_ptr), *w = reinterpret_cast<const float *>(p->w_ptr);
    const float *b = reinterpret_cast<const float *>(p->b_ptr);
    float *prob = reinterpret_cast<float *>(p->prob_ptr), *logits = reinterpret_cast<float *>(p->logits_ptr);
    int *expert = reinterpret_cast<int *>(p->expert_ptr), *counts = reinterpret_cast<int *>(p->work_ptr);
    if (nblk > 0) {
        if (p->mode == DIMSUM_MOE_ROUTE_SIGMOID)
            hipLaunchKernelGGL(moe_route_kernel<true>, dim3(nblk), dim3(256), 0, s, x, w, b, prob, expert, logits, counts, T, p->hidden, E);
        else
            hipLaunchKernelGGL(moe_route_kernel<false>, dim3(nblk), dim3(256), 0, s, x, w, b, prob, expert, logits, counts, T, p->hidden, E);
    }
    hipLaunchKernelGGL(moe_scan_kernel, dim3(1), dim3(256), 0, s, counts, reinterpret_cast<int *>(p->offsets_ptr), nblk, E);
    if (nblk > 0)
        hipLaunchKernelGGL(moe_place_kernel, dim3(nblk), dim3(64), 0, s, expert, counts, reinterpret_cast<int *>(p->perm_ptr),
                           reinterpret_cast<int *>(p->inv_ptr), reinterpret_cast<int *>(p->row_expert_ptr), T, E);
    return launch_status();
}

extern "C" int dimsum_moe_route_bwd(const dimsum_moe_route_params_t *p, void *stream) {
    using namespace dimsum;
    if (const int rc = route_params_ok(p, true)) return rc;
    if (p->tokens == 0) return DIMSUM_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // one round of ~512 row groups whatever the token count (fewer atomics per element of dW_r), whole tiles of kRows rows
    int64_t rpw = (p->tokens + 511) / 512;
    rpw = (rpw + kRows - 1) / kRows * kRows;
    const dim3 grid((unsigned)((p->hidden / 4 + 255) / 256), (unsigned)((p->tokens + rpw - 1) / rpw));
#define DIMSUM_MRB(SIG)                                                                                                                                \
    hipLaunchKernelGGL(moe_route_bwd_kernel<SIG>, grid, dim3(256), 0, s, reinterpret_cast<const float *>(p->x_ptr), reinterpret_cast<const float *>(p->w_ptr), \
                       reinterpret_cast<const float *>(p->logits_ptr), reinterpret_cast<const float *>(p->prob_ptr),                                   \
                       reinterpret_cast<const int *>(p->expert_ptr), reinterpret_cast<const float *>(p->dprob_ptr),                                    \
                       reinterpret_cast<const float *>(p->dxp_ptr), reinterpret_cast<const int *>(p->inv_ptr), reinterpret_cast<float *>(p->dx_ptr),   \
                       reinterpret_cast<float *>(p->dw_ptr), reinterpret_cast<float *>(p->db_ptr), p->tokens, p->hidden, (int)p->num_experts, (int)rpw)
    if (p->mode == DIMSUM_MOE_ROUTE_SIGMOID) DIMSUM_MRB(true);
    else DIMSUM_MRB(false);
#undef DIMSUM_MRB
    return launch_status();
}

extern "C" int dimsum_moe_permute(const dimsum_moe_rows_params_t *p, void *stream) {
    using namespace dimsum;
    if (const int rc = rows_params_ok(p, false, false)) return rc;
    if (p->rows == 0) return DIMSUM_OK;
    dim3 grid;
    if (!flat_grid(p->rows * (p->hidden / 4), grid)) return DIMSUM_ERR_SHAPE;
    hipLaunchKernelGGL(moe_rows_kernel<false>, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const float *>(p->src_ptr),
                       reinterpret_cast<const int *>(p->perm_ptr), (const float *)nullptr, reinterpret_cast<float *>(p->dst_ptr), p->rows, p->hidden);
    return launch_status();
}

extern "C" int dimsum_moe_permute_f16s(const dimsum_moe_permute_f16s_params_t *p, void *stream) {
    using namespace dimsum;
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_moe_permute_f16s_params_t)) return DIMSUM_ERR_ABI;
    dimsum_moe_ext_t e;
    if (const int rc = ext_from<dimsum_moe_ext_t>(p->ext, e)) return rc;
    if (p->rows < 0 || p->rows >= ((int64_t)1 << 31) || p->hidden <= 0 || p->hidden % 4 != 0) return DIMSUM_ERR_SHAPE;
    if (p->rows == 0) return DIMSUM_OK;
    if (!p->src_ptr || !p->perm_ptr || !p->dst_ptr || !p->inv_scale_ptr) return DIMSUM_ERR_NULL;
    if (!al16(p->src_ptr) || !aligned_to<char>(p->dst_ptr, 8) || !al4(p->perm_ptr) || !al4(p->inv_scale_ptr)) return DIMSUM_ERR_STRIDE;
    hipLaunchKernelGGL(moe_permute_f16s_kernel, dim3((unsigned)((p->rows + 3) / 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const float *>(p->src_ptr), reinterpret_cast<const int *>(p->perm_ptr), reinterpret_cast<__half *>(p->dst_ptr),
                       reinterpret_cast<float *>(p->inv_scale_ptr), p->rows, p->hidden);
    return launch_status();
}

extern "C" int dimsum_moe_combine_fwd(const dimsum_moe_rows_params_t *p, void *stream) {
    using namespace dimsum;
    if (const int rc = rows_params_ok(p, true, false)) return rc;
    if (p->rows == 0) return DIMSUM_OK;
    dim3 grid;
    if (!flat_grid(p->rows * (p->hidden / 4), grid)) return DIMSUM_ERR_SHAPE;
    hipLaunchKernelGGL(moe_rows_kernel<true>, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const float *>(p->src_ptr),
                       reinterpret_cast<const int *>(p->perm_ptr), reinterpret_cast<const float *>(p->prob_ptr), reinterpret_cast<float *>(p->dst_ptr),
                       p->rows, p->hidden);
    return launch_status();
}

extern "C" int dimsum_moe_combine_bwd(const dimsum_moe_rows_params_t *p, void *stream) {
    using namespace dimsum;
    if (const int rc = rows_params_ok(p, true, true)) return rc;
    if (p->rows == 0) return DIMSUM_OK;
    hipLaunchKernelGGL(moe_combine_bwd_kernel, dim3((unsigned)((p->rows + 3) / 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const float *>(p->src_ptr), reinterpret_cast<const float *>(p->y_ptr), reinterpret_cast<const int *>(p->perm_ptr),
                       reinterpret_cast<const float *>(p->prob_ptr), reinterpret_cast<float *>(p->dst_ptr), reinterpret_cast<float *>(p->dprob_ptr),
                       p->rows, p->hidden);
    return launch_status();
}
