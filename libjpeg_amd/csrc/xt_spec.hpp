// xt_spec.hpp -- the pure part of the JPEG XT merging specification (HostDecoder::finish_xt, xt_finish.cpp): big-endian fields,
// the sub-box walk over a superbox payload, the non-linear point transformations with their scaled tables, the registry of the
// tables and matrices a specification can name, and the parsed specification itself.  Functions of bytes and small structs:
// no HIP, no HostDecoder (tests/cxx/xt_spec.cpp runs them as a program of its own).
#ifndef MIJ_XT_SPEC_HPP
#define MIJ_XT_SPEC_HPP

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/mijpeg.h"

namespace mij {

static inline int rd16(const uint8_t *p) { return (p[0] << 8) | p[1]; }
static inline uint32_t rd32(const uint8_t *p) { return ((uint32_t)rd16(p) << 16) | (uint32_t)rd16(p + 2); }
static inline uint32_t boxid(char a, char b, char c, char d)
{
  return ((uint32_t)(uint8_t)a << 24) | ((uint32_t)(uint8_t)b << 16) | ((uint32_t)(uint8_t)c << 8) | (uint32_t)(uint8_t)d;
}

// The sub-boxes of a superbox payload, LBox(4) TBox(4) payload each, read leniently: `while (w.next())` yields type, payload and
// its length (0: a box without payload).  An LBox below 8 or beyond the end stops the walk with `broken` set: what that means
// is the caller's business (the form check of the walk, check_merging_spec, has thrown such a box out where it matters).
struct SubBoxWalk {
  const uint8_t *d;
  size_t size, j = 0;
  uint32_t type = 0;
  const uint8_t *payload = nullptr;
  size_t len = 0;
  bool broken = false;
  SubBoxWalk(const uint8_t *data, size_t bytes) : d(data), size(bytes) {}
  bool next()
  {
    if (j + 8 > size) return false;
    const uint32_t l = rd32(d + j);
    if (l < 8 || j + l > size) { broken = true; return false; }
    type = rd32(d + j + 4);
    payload = d + j + 8;
    len = l - 8;
    j += l;
    return true;
  }
};

// Non-linear point transformations a merging specification can name: explicit tables (TONE, boxes/inversetonemappingbox.cpp)
// and parametric curves (CURV, boxes/parametrictonemappingbox.cpp), looked up by table index (boxes/namespace.cpp:60-91).
struct XtNlt {
  int kind = 0; // 0: none, 1: TONE, 2: CURV
  int entries = 0, resbits = 0;
  std::vector<int32_t> lut;
  int type = 0, e = 0;
  float p[4] = {0, 0, 0, 0};
};

inline float ieee_decode(uint32_t bits) // tools/numerics.cpp:56-89
{
  if (((bits >> 23) & 0xff) == 0xff) return (bits >> 31) ? -HUGE_VALF : HUGE_VALF;
  float f;
  memcpy(&f, &bits, 4);
  return f;
}

// ParametricToneMappingBox::TableValue (:199-272).  The reference is an x87 / -ffast-math build: the arithmetic of an expression
// stays in 80-bit registers, only pow / exp / log go through doubles -- long double around double calls reproduces its tables
// (pinned by tests/test_xt_general.py against the reference binary).
inline long double curve_value(const XtNlt &t, double v, bool &bad)
{
  const long double p1 = t.p[0], p2 = t.p[1], p3 = t.p[2], p4 = t.p[3];
  switch (t.type) {
  case 0: return 0.0L;
  case 1: return 1.0L;
  case 2: return v;
  case 4:
    return v >= p1 ? (long double)pow((double)((v + p3) / (1.0L + p3)), (double)p2)
                   : (long double)pow((double)((p1 + p3) / (1.0L + p3)), (double)p2) * v / p1;
  case 5: if (t.p[1] >= t.p[0]) return v * (p2 - p1) + p1; bad = true; return 0.0L;
  case 6: if (t.p[1] > t.p[0]) return p3 * (long double)exp((double)(v * (p2 - p1) + p1)) + p4; bad = true; return 0.0L;
  case 7:
    if (p1 > 0.0L) return (v > 0.0 || (p3 > 0.0L && v >= 0.0)) ? (long double)log((double)((long double)pow((double)(p1 * v), (double)p2) + p3)) + p4 : -HUGE_VALL;
    return (v > 0.0 || (p3 > 0.0L && v >= 0.0)) ? -(long double)log((double)((long double)pow((double)(-p1 * v), (double)p2) + p3)) + p4 : HUGE_VALL;
  case 8: return v > 0.0 ? (p2 - p1) * (long double)pow(v, (double)p3) + p1 : p1;
  }
  return 0.0L;
}

// ToneMapperBox::ScaledTableOf for the integer path: 2^(inbits + infract) entries.  0 or the reference's error code.
inline int scaled_table(const XtNlt &t, int inbits, int outbits, int infract, int outfract, std::vector<int32_t> &tab)
{
  if (t.kind == 1) { // inversetonemappingbox.cpp:192-212: the table as it is, if it fits
    if (outbits + outfract != 8 + t.resbits || inbits > 16 || (1u << inbits) != (uint32_t)t.entries || infract != 0) return MIJPEG_ERR_INVALID_PARAMETER;
    tab = t.lut;
    return 0;
  }
  const uint32_t max = 1u << (inbits + infract); // parametrictonemappingbox.cpp:387-430
  tab.resize(max);
  const double inscale = inbits > 1 ? 1.0 / (double)(((1u << inbits) - (uint32_t)t.e) << infract) : 1.0 / (double)(1 << infract);
  const double outscale = outbits > 1 ? 1.0 * (double)(((1u << outbits) - (uint32_t)t.e) << outfract) : 1.0 * (double)(1 << outfract);
  bool bad = false;
  for (uint32_t i = 0; i < max; i++) {
    const double w = floor((double)((long double)outscale * curve_value(t, i * inscale, bad) + 0.5L));
    tab[i] = (w >= -2147483648.0 && w < 2147483648.0) ? (int32_t)w : INT32_MIN; // LONG(double) of an out-of-range value on x86
  }
  return bad ? MIJPEG_ERR_INVALID_PARAMETER : 0;
}

struct XtVerdict { // 0, or the reference's error code with its message
  int code = 0;
  const char *message = nullptr;
};

// The tables and matrices a specification's indices resolve to.  First definition of an index wins: the specification's own
// boxes are searched before the file's (namespace.cpp:60-125).
struct XtTables {
  XtNlt nlt[16];
  int32_t mtx[16][9];
  bool have_mtx[16] = {false};

  XtVerdict register_box(uint32_t type, const uint8_t *d, size_t len)
  {
    const int bad = MIJPEG_ERR_MALFORMED_STREAM;
    if (type == boxid('T', 'O', 'N', 'E')) { // inversetonemappingbox.cpp:72-118
      if (len < 1 + 512 || !(len & 1)) return {bad, "number of table entries in the inverse tone mapping box is invalid"};
      const int idx = d[0] >> 4;
      const bool wide = (d[0] & 15) > 8;
      const size_t n = (len - 1) >> (wide ? 2 : 1);
      if ((wide && ((len - 1) & 3)) || (n & (n - 1))) return {bad, "number of table entries in the inverse tone mapping box must be a power of two"};
      if (nlt[idx].kind) return {};
      nlt[idx].kind = 1; nlt[idx].entries = (int)n; nlt[idx].resbits = d[0] & 15;
      nlt[idx].lut.resize(n);
      for (size_t i = 0; i < n; i++) nlt[idx].lut[i] = wide ? (int32_t)rd32(d + 1 + 4 * i) : rd16(d + 1 + 2 * i);
    } else if (type == boxid('C', 'U', 'R', 'V')) { // parametrictonemappingbox.cpp:84-149
      if (len != 2 + 16) return {bad, "Malformed JPEG file, CURV box size is invalid"};
      const int idx = d[0] >> 4, ty = d[0] & 15;
      if (ty == 3 || ty > 8) return {bad, "Malformed JPEG file, curve type in CURV box is invalid"};
      if ((d[1] & 15) || (d[1] >> 4) > 1) return {bad, "Malformed JPEG file, the r and e parameters of the CURV box are invalid"};
      if (nlt[idx].kind) return {};
      nlt[idx].kind = 2; nlt[idx].type = ty; nlt[idx].e = d[1] >> 4;
      for (int i = 0; i < 4; i++) nlt[idx].p[i] = ieee_decode(rd32(d + 2 + 4 * i));
    } else if (type == boxid('M', 'T', 'R', 'X')) { // lineartransformationbox.cpp:62-99
      if (len != 1 + 18) return {bad, "malformed JPEG stream, size of the linear transformation box is inccorrect"};
      const int id = d[0] >> 4;
      if (id < 5) return {bad, "malformed JPEG stream, the M value of a linear transformation box is out of range"};
      if ((d[0] & 15) != 13) return {bad, "malformed JPEG stream, the t value of a linear transformation box is invalid"};
      if (have_mtx[id]) return {};
      have_mtx[id] = true;
      for (int i = 0; i < 9; i++) mtx[id][i] = (int16_t)rd16(d + 1 + 2 * i);
    }
    return {};
  }
};

// A merging specification as its boxes state it (255 / -1: not stated), and what the stages of finish_xt resolve from it
struct XtSpec {
  int ltrafo = 255, rtrafo = 255, ctrafo = 255, ocon = -1, rdct = 0;
  int lidx[4] = {255, 255, 255, 255}, qidx[4] = {255, 255, 255, 255}, r2idx[4] = {255, 255, 255, 255};
  int hidden_l = 0, hidden_r = 0; // coefficient bits carried by hidden refinement scans (FINE / RFIN boxes)
  int outbits = 0, rbits = 4;     // bits of the output; fractional bits of the residual path
  bool clamping = false, lossless = false;
};

} // namespace mij
#endif
