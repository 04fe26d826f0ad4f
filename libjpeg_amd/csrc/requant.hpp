// requant.hpp -- requantisation of coefficient planes (requant.hip; include/mijpeg.h): the rule in integers, the coding
// range it clamps into, the kernel's descriptors and their builder, and the rule over blocks in host memory (mijpeg_requantize).  The
// rule stands here once: requant_list_kernel, the host twin and tests/cxx/transcode_tables.cpp all call requant_value.  Calls nothing
// of the HIP runtime.
//
// The rule, for coefficient c at position k of a block (natural order), source table entry a = q_old[k], target entry b = q_new[k]:
//   v = c * a                                       exact: |v| <= 32768 * 65535 < 2^31
//   r = sign(v) * floor((|v| + floor(b / 2)) / b)   to nearest, halves away from zero; |v| + floor(b / 2) < 2^32
// so that b == a gives r == c for every c.  The division is a multiplication by m = floor(2^32 / b) (2^32 - 1 for b = 1), made on
// the host, and one correction: with n < 2^32, n * m / 2^32 > n / b - 1, so the high word q of n * m is floor(n / b) or one below it,
// and n - q * b >= b tells which.
// r is clamped into what a frame of precision P codes -- DC in [-2^(P+2), 2^(P+2) - 1], |AC| <= 2^(P+2) - 1: DC differences then stay
// in category P + 3 and AC coefficients in category P + 2, the widest HencTables index -- and a value that had to be clamped is
// reported: it is the picture's refusal, the clamp only keeps the coder away from symbols without a code.
#ifndef MIJ_REQUANT_HPP
#define MIJ_REQUANT_HPP
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <string.h>

#include "../../include/mijpeg.h"

#ifdef __HIPCC__
#define MIJ_REQUANT_HD __host__ __device__ __forceinline__
#else
#define MIJ_REQUANT_HD inline
#endif

namespace mij {

constexpr unsigned REQUANT_GROUP = 256;                    // lanes of a workgroup: one row of a block each
constexpr unsigned REQUANT_WG_BLOCKS = REQUANT_GROUP / 8;  // destination blocks of a workgroup

// the multiplier of the division by b (b >= 1)
inline uint32_t requant_reciprocal(uint32_t b) { return b <= 1 ? 0xffffffffu : (uint32_t)(0x100000000ull / b); }

// The rule for one coefficient.  lo, hi: the coding range at its position (lo <= 0 <= hi); beyond: set where r lies outside it (never
// cleared).  -> r, clamped
MIJ_REQUANT_HD int requant_value(int c, uint32_t a, uint32_t b, uint32_t m, int lo, int hi, bool &beyond)
{
  const int v = c * (int)a;
  const uint32_t n = (uint32_t)(v < 0 ? -v : v) + (b >> 1);
  uint32_t q = (uint32_t)(((uint64_t)n * m) >> 32);
  if (n - q * b >= b) q++;
  const uint32_t limit = v < 0 ? (uint32_t)-lo : (uint32_t)hi;
  if (q > limit) {
    beyond = true;
    q = limit;
  }
  return v < 0 ? -(int)q : (int)q;
}

// the coding range of precision P (8 or 12)
struct RequantRange { int32_t dc_min, dc_max, ac_max; };
inline RequantRange requant_range(int precision)
{
  const int32_t top = 1 << (precision + 2);
  return RequantRange{-top, top - 1, top - 1};
}

// per component: source and target entries and the multipliers, natural order.  A lane reads row j of each as 16-byte vectors.
struct alignas(16) RequantTables {
  uint16_t a[64], b[64];
  uint32_t m[64];
};
inline void requant_tables_of(RequantTables &t, const uint16_t a[64], const uint16_t b[64])
{
  for (int k = 0; k < 64; k++) {
    t.a[k] = a[k];
    t.b[k] = b[k];
    t.m[k] = requant_reciprocal(b[k]);
  }
}

// One picture of a launch.  Work is block-addressed: block (bx, by) of component c of the destination is made of block (bx, by) of
// the source where the source has one (bx < src_bw, by < src_bh) and is zero otherwise; the pitches may differ.
struct alignas(16) RequantPicture {
  const int16_t *src;                       // device: the object's coefficient store at the picture's base, or a child's planes
  int16_t *dst;                             // device: the pass's coefficient store at the picture's base
  int64_t src_off[4], dst_off[4];           // int16 elements from the bases to the component's plane
  int32_t src_bw[4], src_bh[4], dst_bw[4], dst_bh[4]; // blocks
  RequantRange range;
  int32_t ncomp;
  RequantTables t[4];
};
static_assert(sizeof(RequantPicture) % 16 == 0, "an array of them keeps the tables on 16-byte boundaries");

// workgroups of component c of a picture with this destination frame
inline uint64_t requant_workgroups(const mijpeg_info &out, int c)
{
  return ((uint64_t)out.blocks_w[c] * (uint64_t)out.blocks_h[c] + REQUANT_WG_BLOCKS - 1) / REQUANT_WG_BLOCKS;
}

// The descriptor of a picture: planes of frame `in` at src -> planes of frame `out` (same components; its tables the target) at dst
inline void requant_picture_of(RequantPicture &p, const mijpeg_info &in, const int16_t *src, const mijpeg_info &out, int16_t *dst)
{
  memset(&p, 0, sizeof(p));
  p.src = src;
  p.dst = dst;
  p.range = requant_range(out.precision);
  p.ncomp = out.components;
  for (int c = 0; c < out.components; c++) {
    p.src_off[c] = in.coef_offset[c];
    p.dst_off[c] = out.coef_offset[c];
    p.src_bw[c] = in.blocks_w[c];
    p.src_bh[c] = in.blocks_h[c];
    p.dst_bw[c] = out.blocks_w[c];
    p.dst_bh[c] = out.blocks_h[c];
    requant_tables_of(p.t[c], in.quant[in.quant_index[c]], out.quant[out.quant_index[c]]);
  }
}

struct RequantArgs {
  const RequantPicture *pics; // device
  const uint32_t *first_wg;   // device: first workgroup of item k, the grid behind the last (items + 1 entries)
  const uint32_t *item;       // device: picture * 4 + component
  uint32_t items;
  uint32_t *flags;            // device: one word per picture, zero before the launch; 1 where a value of the picture was clamped
};

// ONE launch of `grid` workgroups on `stream` for all pictures of a pass; 0 or a hipError_t
int launch_requant_list(const RequantArgs &a, unsigned grid, hipStream_t stream);

// The rule over n blocks in host memory (mijpeg_requantize): src -> dst (may be the same), -> coefficients that were clamped
inline int64_t requantize_blocks(const int16_t *src, int16_t *dst, int64_t n, const uint16_t a[64], const uint16_t b[64], int precision)
{
  RequantTables t;
  requant_tables_of(t, a, b);
  const RequantRange r = requant_range(precision);
  int64_t clamped = 0;
  for (int64_t i = 0; i < n; i++)
    for (int k = 0; k < 64; k++) {
      bool beyond = false;
      dst[i * 64 + k] = (int16_t)requant_value(src[i * 64 + k], t.a[k], t.b[k], t.m[k], k ? -r.ac_max : r.dc_min, k ? r.ac_max : r.dc_max, beyond);
      clamped += beyond;
    }
  return clamped;
}

} // namespace mij
#endif
