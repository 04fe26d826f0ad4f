// resample_mirror.cpp -- the mirrored tables of the normalised resized call (libjpeg_amd/csrc/resample_taps.hpp) as a
// program of its own, for the sanitizers: the tables of a list whose members are mirrored and of the same list without the flags,
// each filled into a heap buffer of exactly the layout's size; column x of a mirrored picture's x table must carry first, count and
// every weight of column m - 1 - x of the unmirrored one, its y table, its descriptor and the unmirrored members must be untouched.
// No device, nothing of the library is linked.
// (tests/test_ragged_normalized_cpu.py builds it with -fsanitize=address,undefined and runs it.)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "resample_taps.hpp"

using namespace mij;

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      failures++;                                                          \
      fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond);     \
    }                                                                      \
  } while (0)

// One list: every picture n_x x n_y samples (the axes under test on x, another pair on y), to m_x x m_y; picture 1 and 2 mirrored
static void check_pair(int32_t nx, int32_t mx, int32_t ny, int32_t my)
{
  const int n = 4;
  std::vector<ResampleItem> plain((size_t)n), flagged;
  for (int i = 0; i < n; i++) {
    ResampleItem &it = plain[(size_t)i];
    it.slot = i;
    it.served = i != 3; // (a refused member rides along)
    it.src_w = nx; it.src_h = ny; it.comps = i == 2 ? 1 : 3;
  }
  CHECK(!plain[0].mirror); // (the default)
  flagged = plain;
  flagged[1].mirror = flagged[2].mirror = flagged[3].mirror = true;
  const ResampleLayout L = resample_layout(plain.data(), n, mx, my), M = resample_layout(flagged.data(), n, mx, my);
  CHECK(L.per.size() == 3 && M.per.size() == 3 && L.table_bytes == M.table_bytes && L.arena_bytes == M.arena_bytes && L.workgroups == M.workgroups);
  if (L.per.size() != 3 || M.per.size() != 3 || L.table_bytes != M.table_bytes) return;
  uint8_t *a = (uint8_t *)malloc(L.table_bytes), *b = (uint8_t *)malloc(M.table_bytes); // (exactly: the sanitizer sees a byte too many)
  memset(a, 0xEE, L.table_bytes);
  memset(b, 0xEE, M.table_bytes);
  for (size_t k = 0; k < 3; k++) {
    CHECK(resample_fill(a, L, k, plain.data(), mx, my, 4096));
    CHECK(resample_fill(b, M, k, flagged.data(), mx, my, 4096));
  }
  resample_fill_first(a, L);
  resample_fill_first(b, M);
  // descriptors and prefix table: the flag is not in them
  CHECK(!memcmp(a + L.pictures, b + M.pictures, 3 * sizeof(ResamplePicture)));
  CHECK(!memcmp(a + L.first, b + M.first, 4 * sizeof(uint32_t)));
  for (size_t k = 0; k < 3; k++) {
    const ResampleLayout::Per &p = L.per[k], &q = M.per[k];
    CHECK(p.xtab == q.xtab && p.ytab == q.ytab && p.xcap == q.xcap && p.ycap == q.ycap);
    const int32_t cap = p.xcap;
    const int32_t *pf = (const int32_t *)(a + p.xtab), *pc = pf + mx, *qf = (const int32_t *)(b + q.xtab), *qc = qf + mx;
    const int16_t *pw = (const int16_t *)(pf + 2 * (size_t)mx), *qw = (const int16_t *)(qf + 2 * (size_t)mx);
    // the y table is untouched, mirrored or not
    CHECK(!memcmp(a + p.ytab, b + q.ytab, resample_axis_bytes(my, p.ycap)));
    if (!flagged[(size_t)q.item].mirror) {
      CHECK(!memcmp(a + p.xtab, b + q.xtab, resample_axis_bytes(mx, cap)));
      continue;
    }
    for (int32_t x = 0; x < mx; x++) {
      const int32_t r = mx - 1 - x;
      CHECK(qf[x] == pf[r] && qc[x] == pc[r]);
      CHECK(!memcmp(qw + (size_t)x * (size_t)cap, pw + (size_t)r * (size_t)cap, (size_t)cap * 2));
      CHECK(qf[x] >= 0 && qc[x] >= 1 && qf[x] + qc[x] <= nx); // (every tap the kernel reads lies inside the crop)
    }
    // the padding behind the weights is nobody's
    const size_t used = (size_t)mx * 8 + (size_t)mx * (size_t)cap * 2;
    for (size_t at = used; at < resample_axis_bytes(mx, cap); at++) CHECK(b[q.xtab + at] == 0xEE);
  }
  free(a);
  free(b);
}

int main()
{
  // n -> m on x: one sample either way, a reduction by a hair, many taps, tile edges, an enlargement, an odd reduction
  const int32_t axes[7][2] = {{1, 1}, {1, 64}, {65, 64}, {300, 1}, {300, 65}, {17, 224}, {270, 37}};
  for (int i = 0; i < 7; i++) check_pair(axes[i][0], axes[i][1], axes[(i + 3) % 7][0], axes[(i + 3) % 7][1]);
  // mirroring twice is the identity
  {
    const int32_t n = 270, m = 37, cap = resample_taps(n, m, nullptr, nullptr, nullptr, 0);
    std::vector<int32_t> f((size_t)m), c((size_t)m), f0, c0;
    std::vector<int16_t> w((size_t)m * (size_t)cap), w0;
    CHECK(resample_taps(n, m, f.data(), c.data(), w.data(), cap) == cap);
    f0 = f; c0 = c; w0 = w;
    resample_mirror_axis(f.data(), c.data(), w.data(), m, cap);
    CHECK(f != f0);
    resample_mirror_axis(f.data(), c.data(), w.data(), m, cap);
    CHECK(f == f0 && c == c0 && w == w0);
  }
  if (failures) {
    printf("FAILED %d checks\n", failures);
    return 1;
  }
  printf("OK mirrored resample tables\n");
  return 0;
}
