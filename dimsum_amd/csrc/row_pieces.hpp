// row_pieces.hpp -- a row of f32 / f16 / bf16 elements walked in 16-byte PIECES (4 fp32 / 8 16-bit elements), as the row passes over logits
// do (cross_entropy.hip, sample_logits.hip): one 16-byte access where the row starts 16-byte aligned and the piece is whole, element
// accesses otherwise, with the same values either way.
#pragma once
#include "common.hpp"

namespace dimsum {

typedef unsigned int ce_u32x4 __attribute__((ext_vector_type(4)));

template <typename T> struct CePiece { static constexpr int kElems = 16 / sizeof(T); };

template <typename T> __device__ __forceinline__ void ce_unpack(const ce_u32x4 &v, float *f);
template <> __device__ __forceinline__ void ce_unpack<float>(const ce_u32x4 &v, float *f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) f[i] = __uint_as_float(v[i]);
}
template <> __device__ __forceinline__ void ce_unpack<__half>(const ce_u32x4 &v, float *f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned u = v[i];
        const float2 t = __half22float2(*reinterpret_cast<const __half2 *>(&u));
        f[2 * i] = t.x;
        f[2 * i + 1] = t.y;
    }
}
template <> __device__ __forceinline__ void ce_unpack<__hip_bfloat16>(const ce_u32x4 &v, float *f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = __uint_as_float(v[i] << 16);
        f[2 * i + 1] = __uint_as_float(v[i] & 0xffff0000u);
    }
}

template <typename T> __device__ __forceinline__ ce_u32x4 ce_pack(const float *f);
template <> __device__ __forceinline__ ce_u32x4 ce_pack<float>(const float *f) {
    return ce_u32x4{__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3])};
}
template <> __device__ __forceinline__ ce_u32x4 ce_pack<__half>(const float *f) {
    ce_u32x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const __half2 h = __floats2half2_rn(f[2 * i], f[2 * i + 1]);
        r[i] = *reinterpret_cast<const unsigned *>(&h);
    }
    return r;
}
template <> __device__ __forceinline__ ce_u32x4 ce_pack<__hip_bfloat16>(const float *f) {
    ce_u32x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const __hip_bfloat16 t[2] = {__float2bfloat16(f[2 * i]), __float2bfloat16(f[2 * i + 1])};
        r[i] = *reinterpret_cast<const unsigned *>(t);
    }
    return r;
}

// piece `pc` of a row of V elements as E floats; elements at or beyond V read as `fill`. vec: the row starts 16-byte aligned
template <typename T> __device__ __forceinline__ void ce_load_piece(const T *row, int pc, int V, bool vec, float fill, float *f) {
    constexpr int E = CePiece<T>::kElems;
    const int c0 = pc * E;
    if (vec && c0 + E <= V) {
        ce_unpack<T>(*reinterpret_cast<const ce_u32x4 *>(row + c0), f);
    } else {
#pragma unroll
        for (int e = 0; e < E; ++e) f[e] = c0 + e < V ? to_f32<T>(row[c0 + e]) : fill;
    }
}
template <typename T> __device__ __forceinline__ void ce_store_piece(T *row, int pc, int V, bool vec, const float *f) {
    constexpr int E = CePiece<T>::kElems;
    const int c0 = pc * E;
    if (vec && c0 + E <= V) {
        *reinterpret_cast<ce_u32x4 *>(row + c0) = ce_pack<T>(f);
    } else {
#pragma unroll
        for (int e = 0; e < E; ++e)
            if (c0 + e < V) row[c0 + e] = from_f32<T>(f[e]);
    }
}

template <typename T> static bool ce_rows_aligned(const void *ptr, int64_t rows, int64_t row_stride) {
    return aligned_to<T>(ptr, 16) && (rows == 1 || (row_stride * (int64_t)sizeof(T)) % 16 == 0);
}

static bool ce_ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

}  // namespace dimsum
