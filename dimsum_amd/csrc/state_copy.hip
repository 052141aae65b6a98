// state_copy.hip -- dimsum_state_copy_slots: duplicate slots of a state pool across every tensor of the pool in ONE launch (include/dimsum_hip.h;
// DESIGN.md section 3.22). A streaming copy of a few MB: the work is flattened over (pair, tensor, chunk of the row), the pairs and the pool's
// table are read on the device, the data moves through plain vector loads and stores. No atomics, no host read: capturable.
#include "common.hpp"

namespace dimsum {
namespace {

constexpr int kBlock = 256;
constexpr int kInFlight = 4;                                    // pieces a lane loads before it stores the first
static_assert(kBlock * kInFlight * 16 == DIMSUM_STATE_COPY_CHUNK_BYTES, "one round of a workgroup on the 16-byte path");

struct PoolEntry { int64_t base, slot_stride, row_bytes; };      // one row of the device table, as the header lays it out
static_assert(sizeof(PoolEntry) == 24, "three int64 per tensor");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
#define DIMSUM_GLOBAL __attribute__((address_space(1)))          // the table's pointers are global memory: global_load / global_store, not flat

// pieces first, first + step, ... of a row, kInFlight loads ahead of their stores; consecutive lanes move consecutive pieces
template <typename Piece> __device__ __forceinline__ void copy_row(const char *src, char *dst, int64_t pieces, int64_t first, int64_t step) {
    const DIMSUM_GLOBAL Piece *s = (const DIMSUM_GLOBAL Piece *)src;
    DIMSUM_GLOBAL Piece *d = (DIMSUM_GLOBAL Piece *)dst;
    for (int64_t i = first; i < pieces; i += kInFlight * step) {
        const int64_t i1 = i + step, i2 = i + 2 * step, i3 = i + 3 * step;
        const Piece zero = {};
        const Piece v0 = s[i], v1 = i1 < pieces ? s[i1] : zero, v2 = i2 < pieces ? s[i2] : zero, v3 = i3 < pieces ? s[i3] : zero;
        d[i] = v0;
        if (i1 < pieces) d[i1] = v1;
        if (i2 < pieces) d[i2] = v2;
        if (i3 < pieces) d[i3] = v3;
    }
}
static_assert(kInFlight == 4, "copy_row is written out for four pieces");

__global__ __launch_bounds__(kBlock) void state_copy_slots_kernel(const PoolEntry *__restrict__ table, const int32_t *__restrict__ pairs,
                                                                  const int64_t pairs_stride, const int num_slots, const int n_tensors,
                                                                  const int chunks) {
    const unsigned chunk = blockIdx.x % (unsigned)chunks, pt = blockIdx.x / (unsigned)chunks;
    const unsigned tensor = pt % (unsigned)n_tensors, pair = pt / (unsigned)n_tensors;
    const int src = pairs[(int64_t)pair * pairs_stride], dst = pairs[(int64_t)pair * pairs_stride + 1];
    // padding, out of range, or nothing to move: no address is formed
    if (src < 0 || dst < 0 || src >= num_slots || dst >= num_slots || src == dst) return;
    const PoolEntry e = table[tensor];
    const char *s = reinterpret_cast<const char *>(e.base) + (int64_t)src * e.slot_stride;
    char *d = reinterpret_cast<char *>(e.base) + (int64_t)dst * e.slot_stride;
    const int64_t first = (int64_t)chunk * kBlock + threadIdx.x, step = (int64_t)chunks * kBlock;
    const int64_t all = e.base | e.slot_stride | e.row_bytes;    // a piece size divides all three or is not used
    if ((all & 15) == 0) copy_row<u32x4>(s, d, e.row_bytes >> 4, first, step);
    else if ((all & 3) == 0) copy_row<uint32_t>(s, d, e.row_bytes >> 2, first, step);
    else if ((all & 1) == 0) copy_row<uint16_t>(s, d, e.row_bytes >> 1, first, step);
    else copy_row<uint8_t>(s, d, e.row_bytes, first, step);
}

}  // namespace
}  // namespace dimsum

extern "C" int dimsum_state_copy_slots(const dimsum_state_copy_params_t *p, void *stream) {
    using namespace dimsum;
    if (!p) return DIMSUM_ERR_NULL;
    if (p->struct_size != sizeof(dimsum_state_copy_params_t)) return DIMSUM_ERR_ABI;
    if (!p->table_ptr || !p->pairs_ptr) return DIMSUM_ERR_NULL;
    if (p->num_slots < 1 || p->n_tensors < 0 || p->n_pairs < 0 || p->max_row_bytes < 0) return DIMSUM_ERR_SHAPE;
    const int64_t chunks = (p->max_row_bytes + DIMSUM_STATE_COPY_CHUNK_BYTES - 1) / DIMSUM_STATE_COPY_CHUNK_BYTES;
    if (chunks > 0x7fffffff || (int64_t)p->n_pairs * p->n_tensors > 0x7fffffff / (chunks > 0 ? chunks : 1)) return DIMSUM_ERR_SHAPE;
    if (p->pairs_stride < 2) return DIMSUM_ERR_STRIDE;
    const int64_t blocks = (int64_t)p->n_pairs * p->n_tensors * chunks;
    if (blocks == 0) return DIMSUM_OK;
    hipLaunchKernelGGL(state_copy_slots_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, reinterpret_cast<hipStream_t>(stream),
                       static_cast<const PoolEntry *>(p->table_ptr), static_cast<const int32_t *>(p->pairs_ptr), p->pairs_stride, p->num_slots,
                       p->n_tensors, (int)chunks);
    return launch_status();
}
