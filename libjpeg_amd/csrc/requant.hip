// requant.hip -- requant_list_kernel (requant.hpp).
//
// One launch requantises the planes of every picture of a transcode pass, whatever their shapes, precisions and sources.  A
// workgroup owns REQUANT_WG_BLOCKS consecutive blocks of one component's destination plane; it finds its (picture, component) in the
// prefix table of first workgroups (wave-uniform loads, a binary search: what tile_enter_ragged, the ragged forward kernels and
// resample_list_kernel do).  A lane owns one row of one block: 16 bytes in, 16 bytes out, and row j of the tables a, b and m as
// 16-byte vectors (the eight lanes of a block read the whole table between them, every block's lanes the same 512 bytes: they stay in
// the cache).  The kernel waits for memory: the arithmetic of a coefficient is two multiplications and a handful of integer
// operations (requant_value), no division.  A destination block without a source block -- the destination frame pads to its own
// MCU grid -- is written as zero.  A lane that had to clamp a value stores 1 into its picture's flag word; nobody else touches it.
#include <hip/hip_runtime.h>

#include "requant.hpp"

namespace mij {

struct alignas(16) Row16 { int16_t v[8]; };
struct alignas(16) Row16u { uint16_t v[8]; };
struct alignas(16) Row32u { uint32_t v[4]; };

__global__ __launch_bounds__(REQUANT_GROUP) void requant_list_kernel(RequantArgs a)
{
  const unsigned wg = blockIdx.x;
  const uint32_t *__restrict__ first = a.first_wg;
  unsigned lo = 0, hi = a.items; // first[lo] <= wg < first[hi]
  while (hi - lo > 1) {
    const unsigned mid = (lo + hi) >> 1;
    if (first[mid] <= wg) lo = mid;
    else hi = mid;
  }
  const unsigned it = a.item[lo], pic = it >> 2, c = it & 3u;
  const RequantPicture *__restrict__ p = a.pics + pic;
  const unsigned dbw = (unsigned)p->dst_bw[c], dblocks = dbw * (unsigned)p->dst_bh[c];
  const unsigned blk = (wg - first[lo]) * REQUANT_WG_BLOCKS + (threadIdx.x >> 3), row = threadIdx.x & 7u;
  if (blk >= dblocks) return;
  const unsigned by = blk / dbw, bx = blk - by * dbw;
  Row16 out = {{0, 0, 0, 0, 0, 0, 0, 0}};
  bool beyond = false;
  if (bx < (unsigned)p->src_bw[c] && by < (unsigned)p->src_bh[c]) {
    const uint64_t sblk = (uint64_t)by * (unsigned)p->src_bw[c] + bx;
    const Row16 in = *reinterpret_cast<const Row16 *>(p->src + p->src_off[c] + (int64_t)(sblk * 64 + row * 8));
    const RequantTables *__restrict__ t = &p->t[c];
    const Row16u qa = *reinterpret_cast<const Row16u *>(t->a + row * 8), qb = *reinterpret_cast<const Row16u *>(t->b + row * 8);
    const Row32u m0 = *reinterpret_cast<const Row32u *>(t->m + row * 8), m1 = *reinterpret_cast<const Row32u *>(t->m + row * 8 + 4);
    const int ac = p->range.ac_max;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const bool dc = row == 0 && j == 0;
      out.v[j] = (int16_t)requant_value(in.v[j], qa.v[j], qb.v[j], j < 4 ? m0.v[j] : m1.v[j - 4], dc ? p->range.dc_min : -ac, dc ? p->range.dc_max : ac, beyond);
    }
  }
  *reinterpret_cast<Row16 *>(p->dst + p->dst_off[c] + (int64_t)((uint64_t)blk * 64 + row * 8)) = out;
  if (beyond) a.flags[pic] = 1u;
}

int launch_requant_list(const RequantArgs &a, unsigned grid, hipStream_t stream)
{
  if (!grid) return 0;
  hipLaunchKernelGGL(requant_list_kernel, dim3(grid), dim3(REQUANT_GROUP), 0, stream, a);
  return (int)hipGetLastError();
}

} // namespace mij
