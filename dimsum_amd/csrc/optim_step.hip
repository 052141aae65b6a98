// optim_step.hip -- the tail of a training step as two launches over a LIST of fp32 tensors (see include/dimsum_hip.h):
//   optim_sumsq_kernel   sum of squares of all gradients -> one partial per workgroup; advances the per-tensor step counters
//   optim_step_kernel    every workgroup sums the partials (one fixed order) -> clip factor; AdamW + EMA, one read and one write per stream
// Work is cut into chunks of DIMSUM_OPTIM_CHUNK elements of one tensor; a workgroup takes chunk blockIdx.x, + gridDim.x, ... Inside a chunk,
// lane l owns the elements [1024 k + 4 l, + 4), k = 0 .. 3 -- ALWAYS, whether they arrive as one 16-byte load (every pointer of the tensor
// 16-byte aligned) or as four 4-byte loads (a gradient that is a view at an odd offset) and whether the chunk is whole or a tensor's tail. Sums
// therefore depend on the tables only, never on addresses: equal gradients give bit-equal norms (no float atomics anywhere).
#include "common.hpp"

namespace dimsum {
namespace {

constexpr int kChunk = DIMSUM_OPTIM_CHUNK;
constexpr int kBlock = 256;
constexpr int kPass = kBlock * 4;                      // elements per pass of a workgroup
static_assert(kChunk % kPass == 0, "a chunk is a whole number of passes");

// every tensor lives in device memory: telling the compiler so (address space 1) turns the flat loads and stores of pointers that were themselves
// loaded from a table into global ones
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) const float cgfloat;
typedef float gfloat4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ gfloat *as_global(float *q) { return (gfloat *)q; }
__device__ __forceinline__ cgfloat *as_global(const float *q) { return (cgfloat *)q; }

// elements [0, 4) at q; `n` of them exist (n >= 1), the rest read as 0. kVec: q is 16-byte aligned
template <bool kVec> __device__ __forceinline__ f32x4 load4(cgfloat *q, int n) {
    if (kVec && n >= 4) {
        const gfloat4 r = *(const __attribute__((address_space(1))) gfloat4 *)q;
        return {{r.x, r.y, r.z, r.w}};
    }
    f32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r.v[j] = j < n ? q[j] : 0.f;
    return r;
}
template <bool kVec> __device__ __forceinline__ void store4(gfloat *q, int n, const f32x4 &a) {
    if (kVec && n >= 4) {
        *(__attribute__((address_space(1))) gfloat4 *)q = gfloat4{a.v[0], a.v[1], a.v[2], a.v[3]};
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < n) q[j] = a.v[j];
}

__device__ __forceinline__ bool aligned16(const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

struct Chunk {
    int tensor;
    int64_t offset;     // first element
    int count;          // 1 .. kChunk elements
};
__device__ __forceinline__ Chunk chunk_at(const dimsum_optim_params_t &p, int c) {
    const int2 e = static_cast<const int2 *>(p.chunk_table)[c];
    const int64_t off = (int64_t)e.y * kChunk, left = static_cast<const int64_t *>(p.numel)[e.x] - off;
    return {e.x, off, (int)(left < kChunk ? left : kChunk)};
}

template <bool kVec> __device__ __forceinline__ float sumsq_chunk(cgfloat *g, int count, int tid, float acc) {
    for (int i = tid * 4; i < count; i += kPass) {
        const f32x4 r = load4<kVec>(g + i, count - i);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = fmaf(r.v[j], r.v[j], acc);         // the padding adds +0
    }
    return acc;
}

__global__ __launch_bounds__(kBlock) void optim_sumsq_kernel(const dimsum_optim_params_t p) {
    const int tid = threadIdx.x;
    const float *const *g_ptrs = static_cast<const float *const *>(p.g_ptrs);
    // one lane per tensor advances its counter; the step kernel (the next launch) only reads them
    float *const *step_ptrs = static_cast<float *const *>(p.step_ptrs);
    for (int t = blockIdx.x * kBlock + tid; t < p.n_tensors; t += gridDim.x * kBlock)
        if (g_ptrs[t]) {
            gfloat *s = as_global(step_ptrs[t]);
            *s = *s + 1.f;
        }
    if (!p.partials) return;

    float acc = 0.f;
    for (int c = blockIdx.x; c < p.n_chunks; c += gridDim.x) {
        const Chunk ch = chunk_at(p, c);
        if (!g_ptrs[ch.tensor]) continue;
        cgfloat *g = as_global(g_ptrs[ch.tensor]) + ch.offset;
        if (!aligned16((const void *)g)) {
            acc = sumsq_chunk<false>(g, ch.count, tid, acc);
        } else if (ch.count != kChunk) {
            acc = sumsq_chunk<true>(g, ch.count, tid, acc);
        } else {                                         // whole chunk: four independent 16-byte loads in flight, the same sums in the same order
            gfloat4 r[kChunk / kPass];
#pragma unroll
            for (int k = 0; k < kChunk / kPass; ++k) r[k] = *(const __attribute__((address_space(1))) gfloat4 *)(g + k * kPass + tid * 4);
#pragma unroll
            for (int k = 0; k < kChunk / kPass; ++k) {
                acc = fmaf(r[k].x, r[k].x, acc);
                acc = fmaf(r[k].y, r[k].y, acc);
                acc = fmaf(r[k].z, r[k].z, acc);
                acc = fmaf(r[k].w, r[k].w, acc);
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, kWave);
    __shared__ float red[kBlock / kWave];
    if ((tid & (kWave - 1)) == 0) red[tid / kWave] = acc;
    __syncthreads();
    if (tid == 0) *as_global(static_cast<float *>(p.partials) + blockIdx.x) = (red[0] + red[1]) + (red[2] + red[3]);
}

// b^n for a whole n >= 0 held in a float (the step counters), by squaring: a handful of fp64 products per chunk instead of pow()
__device__ __forceinline__ double pow_count(double b, float n) {
    double r = 1.0;
    for (unsigned long long k = (unsigned long long)n; k; k >>= 1, b *= b)
        if (k & 1) r *= b;
    return r;
}

struct StepConsts {
    float clip, b1, w1, b2, w2, eps, keep, d, wd;      // w1 = 1 - beta1, w2 = 1 - beta2, keep = 1 - lr weight_decay, wd = 1 - ema_decay
};

// no gradient: the parameter and its state stay as they are, the EMA follows
template <bool kVec> __device__ __forceinline__ void ema_chunk(cgfloat *w, gfloat *e, int count, int tid, const StepConsts &k) {
    for (int i = tid * 4; i < count; i += kPass) {
        const int n = count - i;
        const f32x4 pw = load4<kVec>(w + i, n);
        f32x4 pe = load4<kVec>(e + i, n);
#pragma unroll
        for (int j = 0; j < 4; ++j) pe.v[j] = fmaf(k.wd, pw.v[j], k.d * pe.v[j]);
        store4<kVec>(e + i, n, pe);
    }
}

template <bool kVec, bool kEma>
__device__ __forceinline__ void adamw_chunk(cgfloat *g, gfloat *w, gfloat *m, gfloat *v, gfloat *e, int count, int tid, const StepConsts &k,
                                            float step_size, float bc2_sqrt) {
    for (int i = tid * 4; i < count; i += kPass) {
        const int n = count - i;
        const f32x4 pg = load4<kVec>(g + i, n);
        f32x4 pw = load4<kVec>(w + i, n), pm = load4<kVec>(m + i, n), pv = load4<kVec>(v + i, n), pe;
        if (kEma) pe = load4<kVec>(e + i, n);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float gc = k.clip * pg.v[j];
            pm.v[j] = fmaf(k.b1, pm.v[j], k.w1 * gc);
            pv.v[j] = fmaf(k.b2, pv.v[j], k.w2 * gc * gc);
            const float denom = sqrtf(pv.v[j]) / bc2_sqrt + k.eps;
            pw.v[j] = fmaf(-step_size, pm.v[j] / denom, pw.v[j] * k.keep);
            if (kEma) pe.v[j] = fmaf(k.wd, pw.v[j], k.d * pe.v[j]);                  // the NEW parameter
        }
        store4<kVec>(w + i, n, pw);
        store4<kVec>(m + i, n, pm);
        store4<kVec>(v + i, n, pv);
        if (kEma) store4<kVec>(e + i, n, pe);
    }
}

__global__ __launch_bounds__(kBlock) void optim_step_kernel(const dimsum_optim_params_t p) {
    const int tid = threadIdx.x;
    StepConsts k;
    k.clip = 1.f;
    if (p.partials) {
        // <= 2048 floats out of L2, summed in fp64 in an order that is the same in every workgroup
        cgfloat *partials = as_global(static_cast<const float *>(p.partials));
        double s = 0.0;
        for (int j = tid; j < p.n_partials; j += kBlock) s += (double)partials[j];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, kWave);
        __shared__ double red[kBlock / kWave];
        if ((tid & (kWave - 1)) == 0) red[tid / kWave] = s;
        __syncthreads();
        const float total_norm = (float)sqrt((red[0] + red[1]) + (red[2] + red[3]));
        if (blockIdx.x == 0 && tid == 0 && p.total_norm) *as_global(static_cast<float *>(p.total_norm)) = total_norm;
        if (p.max_norm > 0.0) {
            const float c = (float)p.max_norm / (total_norm + 1e-6f);
            k.clip = c > 1.f ? 1.f : c;                  // a NaN norm stays NaN, like torch's clamp(max=1)
        }
    }
    k.b1 = (float)p.beta1, k.w1 = (float)(1.0 - p.beta1), k.b2 = (float)p.beta2, k.w2 = (float)(1.0 - p.beta2), k.eps = (float)p.eps;
    k.keep = (float)(1.0 - p.lr * p.weight_decay), k.d = (float)p.ema_decay, k.wd = (float)(1.0 - p.ema_decay);
    float *const *p_ptrs = static_cast<float *const *>(p.p_ptrs), *const *m_ptrs = static_cast<float *const *>(p.m_ptrs);
    float *const *v_ptrs = static_cast<float *const *>(p.v_ptrs), *const *ema_ptrs = static_cast<float *const *>(p.ema_ptrs);
    const float *const *g_ptrs = static_cast<const float *const *>(p.g_ptrs), *const *step_ptrs = static_cast<const float *const *>(p.step_ptrs);

    for (int c = blockIdx.x; c < p.n_chunks; c += gridDim.x) {
        const Chunk ch = chunk_at(p, c);
        const bool has_g = g_ptrs[ch.tensor] != nullptr, has_e = ema_ptrs && ema_ptrs[ch.tensor];
        if (!has_g && !has_e) continue;
        gfloat *w = as_global(p_ptrs[ch.tensor]) + ch.offset;
        gfloat *e = has_e ? as_global(ema_ptrs[ch.tensor]) + ch.offset : nullptr;
        bool vec = aligned16((const void *)w) && aligned16((const void *)e);
        if (!has_g) {
            if (vec) ema_chunk<true>(w, e, ch.count, tid, k);
            else ema_chunk<false>(w, e, ch.count, tid, k);
            continue;
        }
        cgfloat *g = as_global(g_ptrs[ch.tensor]) + ch.offset;
        gfloat *m = as_global(m_ptrs[ch.tensor]) + ch.offset, *v = as_global(v_ptrs[ch.tensor]) + ch.offset;
        vec = vec && aligned16((const void *)g) && aligned16((const void *)m) && aligned16((const void *)v);
        // bias corrections once per chunk, in fp64 like torch's host arithmetic, rounded to the fp32 factors the update uses
        const float count = *as_global(step_ptrs[ch.tensor]);
        const float step_size = (float)(p.lr / (1.0 - pow_count(p.beta1, count)));
        const float bc2_sqrt = (float)sqrt(1.0 - pow_count(p.beta2, count));
        if (vec && has_e) adamw_chunk<true, true>(g, w, m, v, e, ch.count, tid, k, step_size, bc2_sqrt);
        else if (vec) adamw_chunk<true, false>(g, w, m, v, e, ch.count, tid, k, step_size, bc2_sqrt);
        else if (has_e) adamw_chunk<false, true>(g, w, m, v, e, ch.count, tid, k, step_size, bc2_sqrt);
        else adamw_chunk<false, false>(g, w, m, v, e, ch.count, tid, k, step_size, bc2_sqrt);
    }
}

struct PtrBatch { const void *v[DIMSUM_OPTIM_PTRS_PER_LAUNCH]; };
static_assert(sizeof(PtrBatch) + 16 <= 4096, "the batch travels as kernel arguments");

__global__ __launch_bounds__(kBlock) void optim_write_ptrs_kernel(const void **dst, const PtrBatch b, const int count) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < count) dst[i] = b.v[i];
}

int check(const dimsum_optim_params_t *p) {
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_optim_params_t)) return DIMSUM_ERR_ABI;
    if (!p->p_ptrs || !p->g_ptrs || !p->m_ptrs || !p->v_ptrs || !p->step_ptrs || !p->numel || !p->chunk_table) return DIMSUM_ERR_NULL;
    if (p->n_tensors <= 0 || p->n_chunks <= 0) return DIMSUM_ERR_SHAPE;
    if (p->partials && (p->n_partials < 1 || p->n_partials > DIMSUM_OPTIM_MAX_PARTIALS)) return DIMSUM_ERR_SHAPE;
    return DIMSUM_OK;
}

}  // namespace
}  // namespace dimsum

extern "C" int dimsum_optim_grad_sumsq(const dimsum_optim_params_t *p, void *stream) {
    using namespace dimsum;
    if (const int st = check(p)) return st;
    // one partial per workgroup: the caller's n_partials IS the grid, so the order of the sum is the caller's to keep fixed
    const int blocks = p->partials ? p->n_partials : (p->n_tensors + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(optim_sumsq_kernel, dim3(blocks), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream), *p);
    return hipGetLastError() == hipSuccess ? DIMSUM_OK : DIMSUM_ERR_LAUNCH;
}

extern "C" int dimsum_optim_adamw_ema_step(const dimsum_optim_params_t *p, void *stream) {
    using namespace dimsum;
    if (const int st = check(p)) return st;
    if (p->max_norm > 0.0 && !p->partials) return DIMSUM_ERR_NULL;
    // memory-bound: 8 workgroups per CU x 256 CUs, grid-striding the rest
    const int blocks = p->n_chunks < 2048 ? p->n_chunks : 2048;
    hipLaunchKernelGGL(optim_step_kernel, dim3(blocks), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream), *p);
    return hipGetLastError() == hipSuccess ? DIMSUM_OK : DIMSUM_ERR_LAUNCH;
}

extern "C" int dimsum_optim_write_ptrs(void *dst_table, int64_t first, const void *const *src, int32_t count, void *stream) {
    using namespace dimsum;
    if (!dst_table || (!src && count > 0)) return DIMSUM_ERR_NULL;
    if (first < 0 || count < 0) return DIMSUM_ERR_SHAPE;
    for (int32_t done = 0; done < count; done += DIMSUM_OPTIM_PTRS_PER_LAUNCH) {
        const int n = count - done < DIMSUM_OPTIM_PTRS_PER_LAUNCH ? count - done : DIMSUM_OPTIM_PTRS_PER_LAUNCH;
        PtrBatch b = {};
        memcpy(b.v, src + done, sizeof(void *) * n);
        hipLaunchKernelGGL(optim_write_ptrs_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream),
                           static_cast<const void **>(dst_table) + first + done, b, n);
        if (hipGetLastError() != hipSuccess) return DIMSUM_ERR_LAUNCH;
    }
    return DIMSUM_OK;
}
