// pos_embed.hip -- the rope and cpe positional encodings of the embed pass (see include/dimsum_hip.h):
//   pos_rope_kernel       y = x cos + rotate_half(x) sin over channel pairs, or the transpose of that map (the backward, the inverse rotation)
//   pos_cpe_fwd_kernel    v = x + bias + depthwise 3x3 conv(x) on the token grid, LayerNorm over the channels, affine, modulate -- one pass
//   pos_cpe_bwd_row_kernel  v again from x, the modulation / LayerNorm backward -> dv, and every parameter gradient
//   pos_cpe_bwd_conv_kernel dx = dv + conv^T(dv)
// fp32. (batch, tokens, channels) with the channels contiguous; a lane owns 4 adjacent channels (one 16-byte access per row and operand), a
// workgroup owns a run of consecutive token rows of ONE batch element: the 36 conv weights, gamma, beta, scale and shift of a lane's channels
// are loaded once per workgroup, and the backward's per-channel sums live in registers until the workgroup's last row.
#include "common.hpp"

namespace dimsum {
namespace {

constexpr int kRopeBlock = 256;
constexpr int kCpeMaxBlock = 512;                 // one lane per 4 channels: channels <= 2048
constexpr int kCpeMaxChannels = 4 * kCpeMaxBlock;

__device__ __forceinline__ f32x4 ldv(const float *q) { return widen(ld4<float>(q)); }
__device__ __forceinline__ f32x4 zero4() { return {{0.f, 0.f, 0.f, 0.f}}; }

// ---- rope ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRopeBlock) void pos_rope_kernel(const dimsum_pos_rope_params_t p, const int64_t n4) {
    const int64_t i = (int64_t)blockIdx.x * kRopeBlock + threadIdx.x;
    if (i >= n4) return;
    const int cq = p.channels >> 2;
    const int64_t row = i / cq;
    const int c = (int)(i - row * cq) * 4;
    const int64_t b = row / p.tokens, l = row - b * p.tokens;
    const f32x4 x = ldv(static_cast<const float *>(p.x) + b * p.x_batch_stride + l * p.x_token_stride + c);
    const f32x4 s = ldv(static_cast<const float *>(p.sin) + l * p.channels + c), k = ldv(static_cast<const float *>(p.cos) + l * p.channels + c);
    f32x4 y;
#pragma unroll
    for (int j = 0; j < 4; j += 2) {
        if (!p.inverse) {
            y.v[j] = x.v[j] * k.v[j] - x.v[j + 1] * s.v[j];
            y.v[j + 1] = x.v[j + 1] * k.v[j + 1] + x.v[j] * s.v[j + 1];
        } else {
            y.v[j] = x.v[j] * k.v[j] + x.v[j + 1] * s.v[j + 1];
            y.v[j + 1] = x.v[j + 1] * k.v[j + 1] - x.v[j] * s.v[j];
        }
    }
    st4<float>(static_cast<float *>(p.y) + b * p.y_batch_stride + l * p.y_token_stride + c, y);
}

// ---- cpe ----------------------------------------------------------------------------------------------------------------------------------
// sum of (a, b) over the workgroup, in every lane; lanes without channels bring zeros. red: 2 * (kCpeMaxBlock / kWave) floats of LDS
__device__ __forceinline__ void block_sum2(float &a, float &b, float *red) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, kWave);
        b += __shfl_xor(b, o, kWave);
    }
    const int nw = blockDim.x / kWave;
    if (nw == 1) return;
    __syncthreads();                                    // the previous use of `red` has been read by every wave
    if ((threadIdx.x & (kWave - 1)) == 0) {
        red[2 * (threadIdx.x / kWave)] = a;
        red[2 * (threadIdx.x / kWave) + 1] = b;
    }
    __syncthreads();
    a = 0.f, b = 0.f;
    for (int w = 0; w < nw; ++w) {
        a += red[2 * w];
        b += red[2 * w + 1];
    }
}

// the 36 weights of a lane's 4 channels: w[t].v[e] = weight[c + e][t], t = 3 i + j
__device__ __forceinline__ void load_taps(const float *weight, int c, f32x4 (&w)[9]) {
    float flat[36];
#pragma unroll
    for (int q = 0; q < 9; ++q) {
        const f32x4 t = ldv(weight + (int64_t)c * 9 + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) flat[4 * q + e] = t.v[e];
    }
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) w[t].v[e] = flat[e * 9 + t];
}

// the rows [first, last) of batch element blockIdx.y that this workgroup owns
__device__ __forceinline__ void row_range(int tokens, int &first, int &last) {
    const int per = (tokens + (int)gridDim.x - 1) / (int)gridDim.x;
    first = (int)blockIdx.x * per;
    last = min(tokens, first + per);
}

// the up-to-9 rows around token (h, w): nb[t] = x[b, (h + i - 1) G + (w + j - 1), c .. c + 3], zeros off the grid (a workgroup-uniform test)
__device__ __forceinline__ void load_window(const float *xb, int64_t token_stride, int G, int h, int w, int c, bool active, f32x4 (&nb)[9]) {
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int hh = h + t / 3 - 1, ww = w + t % 3 - 1;
        nb[t] = zero4();
        if (active && hh >= 0 && hh < G && ww >= 0 && ww < G) nb[t] = ldv(xb + (int64_t)(hh * G + ww) * token_stride + c);
    }
}

__device__ __forceinline__ f32x4 conv_row(const f32x4 (&nb)[9], const f32x4 (&w)[9], const f32x4 &bias) {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float acc = nb[4].v[e] + bias.v[e];                // the centre tap's row is x itself
#pragma unroll
        for (int t = 0; t < 9; ++t) acc = fmaf(w[t].v[e], nb[t].v[e], acc);
        v.v[e] = acc;
    }
    return v;
}

__global__ __launch_bounds__(kCpeMaxBlock) void pos_cpe_fwd_kernel(const dimsum_pos_cpe_params_t p) {
    __shared__ float red[2 * (kCpeMaxBlock / kWave)];
    const int C = p.channels, G = p.grid, L = G * G, b = blockIdx.y, c = threadIdx.x * 4;
    const bool active = c < C;
    const float *xb = static_cast<const float *>(p.x) + (int64_t)b * p.x_batch_stride;
    float *yb = static_cast<float *>(p.y) + (int64_t)b * p.y_batch_stride;
    f32x4 w[9], bias = zero4(), gamma = zero4(), beta = zero4(), scale = zero4(), shift = zero4();
#pragma unroll
    for (int t = 0; t < 9; ++t) w[t] = zero4();
    if (active) {
        load_taps(static_cast<const float *>(p.weight), c, w);
        bias = ldv(static_cast<const float *>(p.conv_bias) + c);
        gamma = ldv(static_cast<const float *>(p.gamma) + c);
        beta = ldv(static_cast<const float *>(p.beta) + c);
        scale = ldv(static_cast<const float *>(p.scale) + (int64_t)b * p.mod_batch_stride + c);
        shift = ldv(static_cast<const float *>(p.shift) + (int64_t)b * p.mod_batch_stride + c);
    }
    int first, last;
    row_range(L, first, last);
    const float inv_c = 1.f / (float)C;
    for (int l = first; l < last; ++l) {
        const int h = l / G, wcol = l - h * G;
        f32x4 nb[9];
        load_window(xb, p.x_token_stride, G, h, wcol, c, active, nb);
        const f32x4 v = conv_row(nb, w, bias);             // (lanes without channels: all zeros)
        float s = (v.v[0] + v.v[1]) + (v.v[2] + v.v[3]), unused = 0.f;
        block_sum2(s, unused, red);
        const float mean = s * inv_c;
        float q = 0.f;
        if (active) {
#pragma unroll
            for (int e = 0; e < 4; ++e) q = fmaf(v.v[e] - mean, v.v[e] - mean, q);
        }
        block_sum2(q, unused, red);
        const float rstd = 1.f / sqrtf(q * inv_c + p.eps);
        if (active) {
            f32x4 y;
#pragma unroll
            for (int e = 0; e < 4; ++e) y.v[e] = fmaf(fmaf((v.v[e] - mean) * rstd, gamma.v[e], beta.v[e]), 1.f + scale.v[e], shift.v[e]);
            st4<float>(yb + (int64_t)l * p.y_token_stride + c, y);
            if (p.v) st4<float>(static_cast<float *>(p.v) + ((int64_t)b * L + l) * C + c, v);
        }
        if (threadIdx.x == 0 && p.mean) {
            static_cast<float *>(p.mean)[(int64_t)b * L + l] = mean;
            static_cast<float *>(p.rstd)[(int64_t)b * L + l] = rstd;
        }
    }
}

__device__ __forceinline__ void atomic_add4(float *dst, const f32x4 &a) {
#pragma unroll
    for (int e = 0; e < 4; ++e) atomicAdd(dst + e, a.v[e]);
}

__global__ __launch_bounds__(kCpeMaxBlock) void pos_cpe_bwd_row_kernel(const dimsum_pos_cpe_bwd_params_t p) {
    __shared__ float red[2 * (kCpeMaxBlock / kWave)];
    const dimsum_pos_cpe_params_t &f = p.fwd;
    const int C = f.channels, G = f.grid, L = G * G, b = blockIdx.y, c = threadIdx.x * 4;
    const bool active = c < C;
    const float *xb = static_cast<const float *>(f.x) + (int64_t)b * f.x_batch_stride;
    const float *dyb = static_cast<const float *>(p.dy) + (int64_t)b * p.dy_batch_stride;
    float *dvb = static_cast<float *>(p.dv) + (int64_t)b * L * C;
    f32x4 w[9], bias = zero4(), gamma = zero4(), beta = zero4(), scale = zero4();
#pragma unroll
    for (int t = 0; t < 9; ++t) w[t] = zero4();
    if (active) {
        load_taps(static_cast<const float *>(f.weight), c, w);
        bias = ldv(static_cast<const float *>(f.conv_bias) + c);
        gamma = ldv(static_cast<const float *>(f.gamma) + c);
        beta = ldv(static_cast<const float *>(f.beta) + c);
        scale = ldv(static_cast<const float *>(f.scale) + (int64_t)b * f.mod_batch_stride + c);
    }
    f32x4 dw[9], dbias = zero4(), dgamma = zero4(), dbeta = zero4(), dshift = zero4(), dscale = zero4();
#pragma unroll
    for (int t = 0; t < 9; ++t) dw[t] = zero4();
    int first, last;
    row_range(L, first, last);
    const float inv_c = 1.f / (float)C;
    for (int l = first; l < last; ++l) {
        const int h = l / G, wcol = l - h * G;
        f32x4 nb[9];
        load_window(xb, f.x_token_stride, G, h, wcol, c, active, nb);
        const f32x4 v = conv_row(nb, w, bias);
        const float mean = static_cast<const float *>(f.mean)[(int64_t)b * L + l], rstd = static_cast<const float *>(f.rstd)[(int64_t)b * L + l];
        f32x4 dy = zero4(), xhat, wdy;
        if (active) dy = ldv(dyb + (int64_t)l * p.dy_token_stride + c);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            xhat.v[e] = active ? (v.v[e] - mean) * rstd : 0.f;
            const float g = dy.v[e] * (1.f + scale.v[e]);             // d (LayerNorm's output)
            dshift.v[e] += dy.v[e];
            dscale.v[e] = fmaf(dy.v[e], fmaf(xhat.v[e], gamma.v[e], beta.v[e]), dscale.v[e]);
            dgamma.v[e] = fmaf(g, xhat.v[e], dgamma.v[e]);
            dbeta.v[e] += g;
            wdy.v[e] = g * gamma.v[e];
            s1 = fmaf(xhat.v[e], wdy.v[e], s1);
            s2 += wdy.v[e];
        }
        block_sum2(s1, s2, red);
        const float c1 = s1 * inv_c, c2 = s2 * inv_c;
        if (active) {
            f32x4 dv;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                dv.v[e] = (wdy.v[e] - xhat.v[e] * c1 - c2) * rstd;
                dbias.v[e] += dv.v[e];
#pragma unroll
                for (int t = 0; t < 9; ++t) dw[t].v[e] = fmaf(dv.v[e], nb[t].v[e], dw[t].v[e]);
            }
            st4<float>(dvb + (int64_t)l * C + c, dv);
        }
    }
    if (!active || first >= last) return;
    float *dwp = static_cast<float *>(p.dweight) + (int64_t)c * 9;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) atomicAdd(dwp + e * 9 + t, dw[t].v[e]);
    atomic_add4(static_cast<float *>(p.dconv_bias) + c, dbias);
    atomic_add4(static_cast<float *>(p.dgamma) + c, dgamma);
    atomic_add4(static_cast<float *>(p.dbeta) + c, dbeta);
    atomic_add4(static_cast<float *>(p.dshift) + (int64_t)b * p.dmod_batch_stride + c, dshift);
    atomic_add4(static_cast<float *>(p.dscale) + (int64_t)b * p.dmod_batch_stride + c, dscale);
}

// dx[h, w] = dv[h, w] + sum_{i, j} weight[i, j] dv[h - (i - 1), w - (j - 1)]: the window of dv read through the mirrored taps
__global__ __launch_bounds__(kCpeMaxBlock) void pos_cpe_bwd_conv_kernel(const dimsum_pos_cpe_bwd_params_t p) {
    const dimsum_pos_cpe_params_t &f = p.fwd;
    const int C = f.channels, G = f.grid, L = G * G, b = blockIdx.y, c = threadIdx.x * 4;
    if (c >= C) return;                                    // (no workgroup-wide step below)
    const float *dvb = static_cast<const float *>(p.dv) + (int64_t)b * L * C;
    float *dxb = static_cast<float *>(p.dx) + (int64_t)b * L * C;
    f32x4 w[9];
    load_taps(static_cast<const float *>(f.weight), c, w);
    int first, last;
    row_range(L, first, last);
    for (int l = first; l < last; ++l) {
        const int h = l / G, wcol = l - h * G;
        f32x4 nb[9], dx;
        load_window(dvb, C, G, h, wcol, c, true, nb);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float acc = nb[4].v[e];
#pragma unroll
            for (int t = 0; t < 9; ++t) acc = fmaf(w[8 - t].v[e], nb[t].v[e], acc);      // the row at offset (di, dj) meets the tap (-di, -dj)
            dx.v[e] = acc;
        }
        st4<float>(dxb + (int64_t)l * C + c, dx);
    }
}

inline bool ok16(const void *q) { return aligned_to<float>(q, 16); }
inline bool stride_ok(int64_t s) { return s >= 0 && s % 4 == 0; }

int check_cpe(const dimsum_pos_cpe_params_t &f, bool bwd) {
    if (!f.x || !f.weight || !f.conv_bias || !f.gamma || !f.beta || !f.shift || !f.scale) return DIMSUM_ERR_NULL;
    if (bwd ? (!f.mean || !f.rstd) : (!f.y || (f.mean == nullptr) != (f.rstd == nullptr))) return DIMSUM_ERR_NULL;
    if (f.batch <= 0 || f.batch > 65535 || f.grid <= 0 || f.grid > 32768 || f.channels < 4 || f.channels % 4 || f.channels > kCpeMaxChannels) return DIMSUM_ERR_SHAPE;
    const int64_t L = (int64_t)f.grid * f.grid;
    if (L * f.channels >= ((int64_t)1 << 31)) return DIMSUM_ERR_SHAPE;
    if (!stride_ok(f.x_batch_stride) || !stride_ok(f.x_token_stride) || !stride_ok(f.mod_batch_stride) || f.x_token_stride < f.channels) return DIMSUM_ERR_STRIDE;
    if (!bwd && (!stride_ok(f.y_batch_stride) || !stride_ok(f.y_token_stride) || f.y_token_stride < f.channels || !ok16(f.y))) return DIMSUM_ERR_STRIDE;
    if (!bwd && !ok16(f.v)) return DIMSUM_ERR_STRIDE;
    if (!ok16(f.x) || !ok16(f.weight) || !ok16(f.conv_bias) || !ok16(f.gamma) || !ok16(f.beta) || !ok16(f.shift) || !ok16(f.scale)) return DIMSUM_ERR_STRIDE;
    return DIMSUM_OK;
}

// a workgroup takes at least 4 rows where the batch element has them, and the launch stays near 1024 workgroups: the backward's atomics
// are one per channel, sum and workgroup
inline dim3 cpe_grid(const dimsum_pos_cpe_params_t &f) {
    const int64_t L = (int64_t)f.grid * f.grid;
    const int64_t chunks = std::max<int64_t>(1, std::min<int64_t>((L + 3) / 4, std::max<int64_t>(1, 1024 / f.batch)));
    return dim3((unsigned)chunks, (unsigned)f.batch);
}
inline dim3 cpe_block(const dimsum_pos_cpe_params_t &f) { return dim3((unsigned)((f.channels / 4 + kWave - 1) / kWave * kWave)); }

}  // namespace
}  // namespace dimsum

extern "C" int dimsum_pos_rope(const dimsum_pos_rope_params_t *p, void *stream) {
    using namespace dimsum;
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_pos_rope_params_t)) return DIMSUM_ERR_ABI;
    if (!p->x || !p->sin || !p->cos || !p->y) return DIMSUM_ERR_NULL;
    if (p->batch <= 0 || p->tokens <= 0 || p->channels < 4 || p->channels % 4) return DIMSUM_ERR_SHAPE;
    if (!stride_ok(p->x_batch_stride) || !stride_ok(p->x_token_stride) || !stride_ok(p->y_batch_stride) || !stride_ok(p->y_token_stride)
        || p->x_token_stride < p->channels || p->y_token_stride < p->channels || !ok16(p->x) || !ok16(p->sin) || !ok16(p->cos) || !ok16(p->y))
        return DIMSUM_ERR_STRIDE;
    const int64_t n4 = (int64_t)p->batch * p->tokens * (p->channels / 4), blocks = (n4 + kRopeBlock - 1) / kRopeBlock;
    if (blocks >= ((int64_t)1 << 31)) return DIMSUM_ERR_SHAPE;
    hipLaunchKernelGGL(pos_rope_kernel, dim3((unsigned)blocks), dim3(kRopeBlock), 0, reinterpret_cast<hipStream_t>(stream), *p, n4);
    return launch_status();
}

extern "C" int dimsum_pos_cpe_fwd(const dimsum_pos_cpe_params_t *p, void *stream) {
    using namespace dimsum;
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_pos_cpe_params_t)) return DIMSUM_ERR_ABI;
    if (const int st = check_cpe(*p, false)) return st;
    hipLaunchKernelGGL(pos_cpe_fwd_kernel, cpe_grid(*p), cpe_block(*p), 0, reinterpret_cast<hipStream_t>(stream), *p);
    return launch_status();
}

extern "C" int dimsum_pos_cpe_bwd(const dimsum_pos_cpe_bwd_params_t *p, void *stream) {
    using namespace dimsum;
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_pos_cpe_bwd_params_t)) return DIMSUM_ERR_ABI;
    if (const int st = check_cpe(p->fwd, true)) return st;
    if (!p->dy || !p->dv || !p->dx || !p->dweight || !p->dconv_bias || !p->dgamma || !p->dbeta || !p->dshift || !p->dscale) return DIMSUM_ERR_NULL;
    if (!stride_ok(p->dy_batch_stride) || !stride_ok(p->dy_token_stride) || p->dy_token_stride < p->fwd.channels || p->dmod_batch_stride < 0
        || !ok16(p->dy) || !ok16(p->dv) || !ok16(p->dx))
        return DIMSUM_ERR_STRIDE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(pos_cpe_bwd_row_kernel, cpe_grid(p->fwd), cpe_block(p->fwd), 0, s, *p);
    if (const int st = launch_status()) return st;
    hipLaunchKernelGGL(pos_cpe_bwd_conv_kernel, cpe_grid(p->fwd), cpe_block(p->fwd), 0, s, *p);
    return launch_status();
}
