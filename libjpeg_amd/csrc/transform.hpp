// transform.hpp -- lossless flips, transposes and rotations of coefficient planes (transform.hip; include/mijpeg.h): the
// rule, the kernel's arguments, and the rule over one component's plane in host memory (mijpeg_transform_blocks).  The rule stands
// here once: transform_list_kernel, the host twin and tests/cxx/transform_tables.cpp all call transform_source_block,
// transform_negates and requant_value (requant.hpp).  Calls nothing of the HIP runtime.
//
// The rule.  Each of the eight transforms (numbered as jpegtran's JXFORM_CODE) is "transpose first (T), then mirror horizontally
// (MH) and / or vertically (MV)".  Per component, blocks in natural order, coef[v * 8 + u] with u the horizontal frequency:
//   T    destination block (bx, by) is source block (by, bx); inside the block dst[v][u] = src[u][v]; the component's sampling
//        factors swap, the frame is H x W, every quantiser table is transposed
//   MH   destination block bx is block bw - 1 - bx of the frame after T, coefficients with odd u are negated; bw: the component's
//        width in blocks, which is the destination's own: a mirrored axis is a whole number of MCUs (the plan refuses or trims)
//   MV   the same in v, by and bh
// Requantisation composes: a is the (transposed) source entry at the destination position, b and m the target's, requant_value as
// ever.  It is odd in c and DC is never negated, so negating before it or behind it is the same; kept tables give r == c.
// Trimming drops the partial MCU column or row at the source's far edge, so the source block origin is always (0, 0).
#ifndef MIJ_TRANSFORM_HPP
#define MIJ_TRANSFORM_HPP
#include "requant.hpp"

namespace mij {

constexpr uint32_t TRANSFORM_T = 1, TRANSFORM_MH = 2, TRANSFORM_MV = 4;

// a code of include/mijpeg.h (with or without MIJPEG_TRANSFORM_TRIM) is one of the eight
inline bool transform_in_order(int32_t code) { return (code & ~MIJPEG_TRANSFORM_TRIM) >= 0 && (code & ~MIJPEG_TRANSFORM_TRIM) <= MIJPEG_TRANSFORM_ROT_270; }
// its T / MH / MV bits
inline uint32_t transform_bits(int32_t code)
{
  static const uint8_t bits[8] = {0, TRANSFORM_MH, TRANSFORM_MV, TRANSFORM_T, TRANSFORM_T | TRANSFORM_MH | TRANSFORM_MV, TRANSFORM_T | TRANSFORM_MH,
                                  TRANSFORM_MH | TRANSFORM_MV, TRANSFORM_T | TRANSFORM_MV};
  return bits[code & 7];
}

// destination block (bx, by) of a component of dbw x dbh blocks -> its source block
MIJ_REQUANT_HD void transform_source_block(uint32_t bits, uint32_t bx, uint32_t by, uint32_t dbw, uint32_t dbh, uint32_t &sbx, uint32_t &sby)
{
  const uint32_t mx = bits & TRANSFORM_MH ? dbw - 1 - bx : bx, my = bits & TRANSFORM_MV ? dbh - 1 - by : by;
  sbx = bits & TRANSFORM_T ? my : mx;
  sby = bits & TRANSFORM_T ? mx : my;
}
// the coefficient at (u, v) of a destination block changes its sign
MIJ_REQUANT_HD bool transform_negates(uint32_t bits, uint32_t u, uint32_t v) { return (((bits >> 1) & u) ^ ((bits >> 2) & v)) & 1u; }

// a quantiser table as the destination sees it
inline void transform_table(uint32_t bits, const uint16_t q[64], uint16_t out[64])
{
  for (int v = 0; v < 8; v++)
    for (int u = 0; u < 8; u++) out[v * 8 + u] = bits & TRANSFORM_T ? q[u * 8 + v] : q[v * 8 + u];
}

// The descriptor of a transformed picture: requant_picture_of with the source's tables in destination order
inline void transform_picture_of(RequantPicture &p, const mijpeg_info &in, const int16_t *src, const mijpeg_info &out, int16_t *dst, uint32_t bits)
{
  requant_picture_of(p, in, src, out, dst);
  for (int c = 0; c < out.components; c++) {
    uint16_t a[64];
    transform_table(bits, in.quant[in.quant_index[c]], a);
    requant_tables_of(p.t[c], a, out.quant[out.quant_index[c]]);
  }
}

// LDS of transform_list_kernel: a block's 8 x 8 exchange takes 32 dwords; 40 keep the eight blocks of a wave on banks of their own
constexpr unsigned TRANSFORM_LDS_PITCH = 40;

struct TransformArgs {
  RequantArgs list;     // the transformed pictures' work list over the pass's descriptors and flags
  const uint32_t *bits; // device: T / MH / MV per picture of the pass
};

// ONE launch of `grid` workgroups on `stream` for the transformed pictures of a pass; 0 or a hipError_t
int launch_transform_list(const TransformArgs &a, unsigned grid, hipStream_t stream);

// The rule over one component's plane in host memory (mijpeg_transform_blocks): src (sbw x sbh blocks, table a in ITS order) ->
// dst (dbw x dbh blocks, table b), -> coefficients that were clamped.  A destination block without a source block is zero.
inline int64_t transform_blocks(const int16_t *src, int32_t sbw, int32_t sbh, int16_t *dst, int32_t dbw, int32_t dbh, uint32_t bits, const uint16_t a[64],
                                const uint16_t b[64], int precision)
{
  uint16_t at[64];
  transform_table(bits, a, at);
  RequantTables t;
  requant_tables_of(t, at, b);
  const RequantRange r = requant_range(precision);
  int64_t clamped = 0;
  for (uint32_t by = 0; by < (uint32_t)dbh; by++)
    for (uint32_t bx = 0; bx < (uint32_t)dbw; bx++) {
      int16_t *out = dst + ((int64_t)by * dbw + bx) * 64;
      uint32_t sbx, sby;
      transform_source_block(bits, bx, by, (uint32_t)dbw, (uint32_t)dbh, sbx, sby);
      if (sbx >= (uint32_t)sbw || sby >= (uint32_t)sbh) {
        memset(out, 0, 64 * sizeof(int16_t));
        continue;
      }
      const int16_t *in = src + ((int64_t)sby * sbw + sbx) * 64;
      for (uint32_t v = 0; v < 8; v++)
        for (uint32_t u = 0; u < 8; u++) {
          const uint32_t k = v * 8 + u;
          const int c = bits & TRANSFORM_T ? in[u * 8 + v] : in[k];
          bool beyond = false;
          out[k] = (int16_t)requant_value(transform_negates(bits, u, v) ? -c : c, t.a[k], t.b[k], t.m[k], k ? -r.ac_max : r.dc_min, k ? r.ac_max : r.dc_max, beyond);
          clamped += beyond;
        }
    }
  return clamped;
}

} // namespace mij
#endif
