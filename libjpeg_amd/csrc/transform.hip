// transform.hip -- transform_list_kernel (transform.hpp).
//
// One launch flips, transposes or rotates the planes of every transformed picture of a transcode pass and requantises them on the
// way.  Work list, ownership and the range flag are requant_list_kernel's (requant.hip): a workgroup owns REQUANT_WG_BLOCKS
// consecutive blocks of one component's destination plane, a lane one row of one block -- 16 bytes stored, row j of the tables a, b
// and m (made in destination order on the host) as 16-byte vectors.  What differs is where the row comes from.  Without T it is row
// j of the mirrored source block: one 16-byte load.  With T it is column j of source block (by, bx): the block's eight lanes load
// its eight rows, 16 bytes each -- exactly its one 128-byte line -- and exchange them through LDS as an 8 x 4 matrix of dwords
// (pairs of coefficients): lane j writes dword k of its row to [k][j], a ds_write_b32 each, and reads line j / 2 back as two 16-byte
// vectors, the dwords of the eight source rows that hold its column, of which it keeps the low or the high half.  A block's image is
// 32 dwords; at a pitch of 40 the four blocks of a 32-lane write group lie on 32 different banks (TRANSFORM_LDS_PITCH).  The
// pictures of a workgroup are one picture, so T is uniform in it and the barrier between the writes and the reads is met by all.
#include <hip/hip_runtime.h>

#include "transform.hpp"

namespace mij {

struct alignas(16) TRow16 { int16_t v[8]; };
struct alignas(16) TRow16u { uint16_t v[8]; };
struct alignas(16) TRow32u { uint32_t v[4]; };

__global__ __launch_bounds__(REQUANT_GROUP) void transform_list_kernel(TransformArgs a)
{
  __shared__ TRow32u tile[REQUANT_WG_BLOCKS * TRANSFORM_LDS_PITCH / 4];
  const unsigned wg = blockIdx.x;
  const uint32_t *__restrict__ first = a.list.first_wg;
  unsigned lo = 0, hi = a.list.items; // first[lo] <= wg < first[hi]
  while (hi - lo > 1) {
    const unsigned mid = (lo + hi) >> 1;
    if (first[mid] <= wg) lo = mid;
    else hi = mid;
  }
  const unsigned it = a.list.item[lo], pic = it >> 2, c = it & 3u;
  const RequantPicture *__restrict__ p = a.list.pics + pic;
  const unsigned bits = a.bits[pic];
  const unsigned dbw = (unsigned)p->dst_bw[c], dbh = (unsigned)p->dst_bh[c], dblocks = dbw * dbh;
  const unsigned slot = threadIdx.x >> 3, row = threadIdx.x & 7u;
  const unsigned blk = (wg - first[lo]) * REQUANT_WG_BLOCKS + slot;
  const bool live = blk < dblocks;
  bool has = false;
  TRow32u in = {{0u, 0u, 0u, 0u}};
  if (live) {
    const unsigned by = blk / dbw, bx = blk - by * dbw;
    unsigned sbx, sby;
    transform_source_block(bits, bx, by, dbw, dbh, sbx, sby);
    has = sbx < (unsigned)p->src_bw[c] && sby < (unsigned)p->src_bh[c];
    if (has) {
      const uint64_t sblk = (uint64_t)sby * (unsigned)p->src_bw[c] + sbx;
      in = *reinterpret_cast<const TRow32u *>(p->src + p->src_off[c] + (int64_t)(sblk * 64 + row * 8));
    }
  }
  if (bits & TRANSFORM_T) { // (uniform in the workgroup: one picture)
    uint32_t *mine = reinterpret_cast<uint32_t *>(tile) + slot * TRANSFORM_LDS_PITCH;
#pragma unroll
    for (int k = 0; k < 4; k++) mine[k * 8 + row] = in.v[k];
    __syncthreads();
    const TRow32u d0 = tile[(slot * TRANSFORM_LDS_PITCH + (row >> 1) * 8) / 4], d1 = tile[(slot * TRANSFORM_LDS_PITCH + (row >> 1) * 8) / 4 + 1];
    const unsigned sh = (row & 1u) * 16;
#pragma unroll
    for (int k = 0; k < 2; k++) {
      in.v[k] = ((d0.v[2 * k] >> sh) & 0xffffu) | ((d0.v[2 * k + 1] >> sh) << 16);
      in.v[k + 2] = ((d1.v[2 * k] >> sh) & 0xffffu) | ((d1.v[2 * k + 1] >> sh) << 16);
    }
  }
  if (!live) return;
  TRow16 out = {{0, 0, 0, 0, 0, 0, 0, 0}};
  bool beyond = false;
  if (has) {
    const RequantTables *__restrict__ t = &p->t[c];
    const TRow16u qa = *reinterpret_cast<const TRow16u *>(t->a + row * 8), qb = *reinterpret_cast<const TRow16u *>(t->b + row * 8);
    const TRow32u m0 = *reinterpret_cast<const TRow32u *>(t->m + row * 8), m1 = *reinterpret_cast<const TRow32u *>(t->m + row * 8 + 4);
    const int ac = p->range.ac_max;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const bool dc = row == 0 && j == 0;
      const int v = (int)(int16_t)(in.v[j >> 1] >> ((j & 1) * 16));
      out.v[j] = (int16_t)requant_value(transform_negates(bits, (unsigned)j, row) ? -v : v, qa.v[j], qb.v[j], j < 4 ? m0.v[j] : m1.v[j - 4], dc ? p->range.dc_min : -ac,
                                        dc ? p->range.dc_max : ac, beyond);
    }
  }
  *reinterpret_cast<TRow16 *>(p->dst + p->dst_off[c] + (int64_t)((uint64_t)blk * 64 + row * 8)) = out;
  if (beyond) a.list.flags[pic] = 1u;
}

int launch_transform_list(const TransformArgs &a, unsigned grid, hipStream_t stream)
{
  if (!grid) return 0;
  hipLaunchKernelGGL(transform_list_kernel, dim3(grid), dim3(REQUANT_GROUP), 0, stream, a);
  return (int)hipGetLastError();
}

} // namespace mij
