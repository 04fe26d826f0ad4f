// xt_spec.cpp -- the pure part of the JPEG XT merging specification (libjpeg_amd/csrc/xt_spec.hpp) as a program of its own, for the
// sanitizers: the sub-box walk at its framing edges, the registry of tables and matrices, scaled tables, ieee_decode.  Every
// input lies in a heap buffer of exactly its size.  No device, nothing of the library is linked.
// (tests/test_xt_spec_cpu.py builds it with -fsanitize=address,undefined and runs it.)
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "xt_spec.hpp"

using namespace mij;

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      failures++;                                                          \
      fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond);     \
    }                                                                      \
  } while (0)

typedef std::vector<uint8_t> Bytes;

static void put32(Bytes &b, uint32_t v)
{
  for (int s = 24; s >= 0; s -= 8) b.push_back((uint8_t)(v >> s));
}
static void put_box(Bytes &b, uint32_t lbox, const char *type, const Bytes &payload)
{
  put32(b, lbox);
  put32(b, boxid(type[0], type[1], type[2], type[3]));
  b.insert(b.end(), payload.begin(), payload.end());
}
// the walk over a copy of exactly b.size() bytes on the heap: "TYPE:len:first payload byte," per box, "!" behind a framing break
static std::string walk(const Bytes &b)
{
  uint8_t *heap = b.empty() ? nullptr : new uint8_t[b.size()];
  if (heap) memcpy(heap, b.data(), b.size());
  std::string out;
  SubBoxWalk w(heap, b.size());
  while (w.next()) {
    for (int s = 24; s >= 0; s -= 8) out += (char)(w.type >> s);
    out += ":" + std::to_string(w.len) + ":" + (w.len ? std::to_string(w.payload[0] + w.payload[w.len - 1]) : "-") + ",";
  }
  if (w.broken) out += "!";
  delete[] heap;
  return out;
}
static XtVerdict reg(XtTables &t, const char *type, const Bytes &payload)
{
  const Bytes exact(payload); // (a copy has no capacity beyond its size)
  return t.register_box(boxid(type[0], type[1], type[2], type[3]), exact.data(), exact.size());
}
static bool says(const XtVerdict &v, int code, const char *message) { return v.code == code && v.message && !strcmp(v.message, message); }

static void test_walk()
{
  CHECK(walk({}) == "");
  CHECK(walk({0, 0, 0, 8, 'L', 'T', 'R'}) == ""); // seven bytes: no box header fits, and nothing is broken
  Bytes b;
  put_box(b, 8, "LDCT", {});
  put_box(b, 11, "OCON", {5, 6, 7});
  CHECK(walk(b) == "LDCT:0:-,OCON:3:12,"); // ... whose last box ends exactly at the end
  b.clear();
  put_box(b, 9, "LTRF", {0x20});
  put_box(b, 7, "RTRF", {});
  CHECK(walk(b) == "LTRF:1:64,!");
  b.clear();
  put_box(b, 9, "LTRF", {0x20});
  put_box(b, 11, "RTRF", {1, 2}); // one byte longer than what is left
  CHECK(walk(b) == "LTRF:1:64,!");
  b.clear();
  put_box(b, 0xffffffffu, "RTRF", {1});
  CHECK(walk(b) == "!");
}

static void test_registry()
{
  static const char *const tone_count = "number of table entries in the inverse tone mapping box is invalid";
  static const char *const tone_power = "number of table entries in the inverse tone mapping box must be a power of two";
  const int bad = MIJPEG_ERR_MALFORMED_STREAM;
  XtTables t;
  Bytes tone(1 + 512);
  tone[0] = 0x38; // index 3, eight extra bits
  for (int i = 0; i < 256; i++) { tone[1 + 2 * i] = (uint8_t)(0x80 | i); tone[2 + 2 * i] = (uint8_t)(255 - i); }
  CHECK(reg(t, "TONE", tone).code == 0);
  CHECK(t.nlt[3].kind == 1 && t.nlt[3].entries == 256 && t.nlt[3].resbits == 8 && t.nlt[3].lut.size() == 256);
  CHECK(t.nlt[3].lut[0] == 0x80ff && t.nlt[3].lut[255] == 0xff00);
  Bytes wide(1 + 1024);
  wide[0] = 0x59; // index 5, a depth nibble above 8: 32-bit entries
  for (int i = 0; i < 256; i++) { wide[1 + 4 * i] = 0xff; wide[2 + 4 * i] = 0xfe; wide[3 + 4 * i] = (uint8_t)i; wide[4 + 4 * i] = 7; }
  CHECK(reg(t, "TONE", wide).code == 0);
  CHECK(t.nlt[5].kind == 1 && t.nlt[5].entries == 256 && t.nlt[5].resbits == 9 && t.nlt[5].lut.size() == 256);
  CHECK(t.nlt[5].lut[0] == (int32_t)0xfffe0007u && t.nlt[5].lut[255] == (int32_t)0xfffeff07u);
  CHECK(says(reg(t, "TONE", Bytes(512, 0x10)), bad, tone_count));
  CHECK(says(reg(t, "TONE", Bytes(1 + 513, 0x10)), bad, tone_count)); // an even length
  CHECK(says(reg(t, "TONE", Bytes(1 + 768, 0x10)), bad, tone_power)); // 384 entries
  CHECK(says(reg(t, "TONE", Bytes(1 + 1026, 0x19)), bad, tone_power)); // wide entries, and not a multiple of four bytes
  CHECK(!t.nlt[1].kind);
  // a second definition of index 3 -- a curve, then another table -- leaves the first in place
  Bytes curv(18, 0);
  curv[0] = 0x34; // index 3, type 4
  curv[1] = 0x10; // e = 1
  curv[2] = 0x3f; curv[3] = 0x80; // p1 = 1.0f
  CHECK(reg(t, "CURV", curv).code == 0 && t.nlt[3].kind == 1 && t.nlt[3].type == 0);
  tone[1] = 0;
  CHECK(reg(t, "TONE", tone).code == 0 && t.nlt[3].lut[0] == 0x80ff);
  curv[0] = 0x74;
  CHECK(reg(t, "CURV", curv).code == 0);
  CHECK(t.nlt[7].kind == 2 && t.nlt[7].type == 4 && t.nlt[7].e == 1 && t.nlt[7].p[0] == 1.0f && t.nlt[7].p[1] == 0.0f);
  curv[0] = 0x83;
  CHECK(says(reg(t, "CURV", curv), bad, "Malformed JPEG file, curve type in CURV box is invalid"));
  curv[0] = 0x89;
  CHECK(says(reg(t, "CURV", curv), bad, "Malformed JPEG file, curve type in CURV box is invalid"));
  curv[0] = 0x82; curv[1] = 0x20;
  CHECK(says(reg(t, "CURV", curv), bad, "Malformed JPEG file, the r and e parameters of the CURV box are invalid"));
  CHECK(says(reg(t, "CURV", Bytes(17, 0x82)), bad, "Malformed JPEG file, CURV box size is invalid"));
  CHECK(!t.nlt[8].kind);
  Bytes mtrx(19, 0);
  mtrx[0] = 0x6d; // id 6, t = 13
  mtrx[1] = 0x20; mtrx[3] = 0xff; mtrx[4] = 0xfe; mtrx[17] = 0x80;
  CHECK(reg(t, "MTRX", mtrx).code == 0);
  CHECK(t.have_mtx[6] && t.mtx[6][0] == 8192 && t.mtx[6][1] == -2 && t.mtx[6][8] == -32768);
  mtrx[1] = 0x10;
  CHECK(reg(t, "MTRX", mtrx).code == 0 && t.mtx[6][0] == 8192); // (the first definition again)
  mtrx[0] = 0x4d;
  CHECK(says(reg(t, "MTRX", mtrx), bad, "malformed JPEG stream, the M value of a linear transformation box is out of range"));
  mtrx[0] = 0x6c;
  CHECK(says(reg(t, "MTRX", mtrx), bad, "malformed JPEG stream, the t value of a linear transformation box is invalid"));
  CHECK(says(reg(t, "MTRX", Bytes(20, 0x6d)), bad, "malformed JPEG stream, size of the linear transformation box is inccorrect"));
  CHECK(!t.have_mtx[4] && !t.have_mtx[5]);
  CHECK(reg(t, "OCON", {0x82}).code == 0 && reg(t, "LCHK", {}).code == 0); // (not the registry's business)
}

static void test_scaled_table()
{
  std::vector<int32_t> tab;
  XtNlt id;
  id.kind = 2; id.type = 2; id.e = 1;
  CHECK(scaled_table(id, 8, 16, 0, 0, tab) == 0 && tab.size() == 256);
  bool same = tab.size() == 256;
  for (int i = 0; same && i < 256; i++) same = tab[i] == 257 * i;
  CHECK(same);
  id.e = 0;
  CHECK(scaled_table(id, 8, 8, 4, 4, tab) == 0 && tab.size() == 4096);
  same = tab.size() == 4096;
  for (int i = 0; same && i < 4096; i++) same = tab[i] == i;
  CHECK(same);
  XtNlt tone;
  tone.kind = 1; tone.entries = 256; tone.resbits = 8;
  tone.lut.assign(256, 77);
  CHECK(scaled_table(tone, 8, 16, 0, 0, tab) == 0 && tab.size() == 256 && tab[255] == 77);
  CHECK(scaled_table(tone, 8, 12, 0, 0, tab) == MIJPEG_ERR_INVALID_PARAMETER); // another output depth
  CHECK(scaled_table(tone, 9, 16, 0, 0, tab) == MIJPEG_ERR_INVALID_PARAMETER); // more entries than it has
  CHECK(scaled_table(tone, 8, 12, 4, 4, tab) == MIJPEG_ERR_INVALID_PARAMETER); // fractional bits in
  XtNlt lin;
  lin.kind = 2; lin.type = 5; lin.p[0] = 0.75f; lin.p[1] = 0.25f;
  CHECK(scaled_table(lin, 8, 8, 0, 0, tab) == MIJPEG_ERR_INVALID_PARAMETER);
  lin.p[1] = 0.75f; // p2 == p1 is a (constant) curve
  CHECK(scaled_table(lin, 8, 8, 0, 0, tab) == 0 && tab[0] == 192 && tab[255] == 192);
  XtNlt lg;
  lg.kind = 2; lg.type = 7; lg.p[0] = 1.0f; lg.p[1] = 1.0f; lg.p[2] = 0.0f; lg.p[3] = 1.0f;
  CHECK(scaled_table(lg, 8, 8, 0, 0, tab) == 0 && tab.size() == 256);
  CHECK(tab[0] == INT32_MIN && tab[255] == 255); // log(0) at input 0; floor(256 * (log(255 / 256) + 1) + 0.5) = floor(255.498) at the other end
  lg.p[0] = -1.0f; // ... and the mirrored branch: plus infinity does not fit either
  CHECK(scaled_table(lg, 8, 8, 0, 0, tab) == 0 && tab[0] == INT32_MIN);
}

int main()
{
  test_walk();
  test_registry();
  test_scaled_table();
  CHECK(ieee_decode(0x7f800000u) == HUGE_VALF && ieee_decode(0xff800000u) == -HUGE_VALF);
  CHECK(ieee_decode(0x7fc00000u) == HUGE_VALF); // (every pattern with all exponent bits set: no NaN leaves)
  CHECK(ieee_decode(0x3f800000u) == 1.0f && ieee_decode(0xc0200000u) == -2.5f);
  if (failures) {
    fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  printf("OK xt_spec\n");
  return 0;
}
