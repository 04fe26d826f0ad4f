// resample_taps.cpp -- the host half of the resized call (libjpeg_amd/csrc/resample_taps.hpp) as a program of its own, for the
// sanitizers: the taps of single axes into heap arrays of exactly their sizes, checked against the filter's definition evaluated here
// once more, and the tables of a list with refused members laid out and filled into a heap buffer of exactly the layout's size, every
// field read back.  No device, nothing of the library is linked.
// (tests/test_ragged_resized_cpu.py builds it with -fsanitize=address,undefined and runs it.)
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

// One axis against the definition: runs, bound, sum and sign of the weights, the remainder's place, zero padding
static void check_axis(int32_t n, int32_t m)
{
  const int32_t cap = resample_taps(n, m, nullptr, nullptr, nullptr, 0);
  CHECK(cap >= 1 && cap <= resample_taps_bound(n, m));
  if (cap < 1) return;
  int32_t *first = (int32_t *)malloc((size_t)m * 4), *count = (int32_t *)malloc((size_t)m * 4);
  int16_t *k = (int16_t *)malloc((size_t)m * (size_t)cap * 2);
  CHECK(resample_taps(n, m, first, count, k, cap - 1) == 0); // (a capacity below the axis's count: refused, the arrays undefined)
  CHECK(resample_taps(n, m, first, count, k, cap) == cap);
  const __int128 S = 2 * (__int128)(n > m ? n : m);
  int32_t most = 0;
  for (int32_t o = 0; o < m; o++) {
    const int32_t f = first[o], c = count[o];
    const int16_t *ko = k + (size_t)o * (size_t)cap;
    CHECK(f >= 0 && c >= 1 && f + c <= n && c <= cap);
    if (c > most) most = c;
    auto w = [&](int64_t i) {
      __int128 d = (2 * (__int128)i + 1) * m - (2 * (__int128)o + 1) * n;
      if (d < 0) d = -d;
      return S - d;
    };
    // the run is exactly where w > 0
    CHECK(f == 0 || w(f - 1) <= 0);
    CHECK(f + c == n || w(f + c) <= 0);
    __int128 W = 0, best = 0;
    int32_t at = 0;
    for (int32_t t = 0; t < c; t++) {
      CHECK(w(f + t) > 0);
      W += w(f + t);
      if (w(f + t) > best) { best = w(f + t); at = t; }
    }
    int32_t sum = 0, plain = 0;
    for (int32_t t = 0; t < c; t++) {
      const int32_t q = (int32_t)((w(f + t) * RESAMPLE_ONE + W / 2) / W);
      CHECK(ko[t] >= 0 && (t == at || ko[t] == q));
      sum += ko[t];
      plain += q;
    }
    CHECK(sum == RESAMPLE_ONE);
    CHECK(ko[at] == (int32_t)((w(f + at) * RESAMPLE_ONE + W / 2) / W) + RESAMPLE_ONE - plain);
    for (int32_t t = c; t < cap; t++) CHECK(ko[t] == 0);
    if (m == n) CHECK(f == o && c == 1 && ko[0] == RESAMPLE_ONE);
  }
  CHECK(most == cap);
  free(first); free(count); free(k);
}

// A list of seven pictures, three of them refused: layout and fill
static void check_layout()
{
  const int n = 7, out_w = 37, out_h = 5;
  const int64_t image_stride = 1000;
  std::vector<ResampleItem> items((size_t)n);
  const int32_t shapes[7][3] = {{300, 270, 3}, {0, 0, 0}, {1, 1, 1}, {16, 16, 3}, {0, 0, 0}, {257, 40, 1}, {0, 0, 0}};
  for (int i = 0; i < n; i++) {
    items[(size_t)i].slot = i;
    items[(size_t)i].served = shapes[i][0] > 0;
    items[(size_t)i].src_w = shapes[i][0]; items[(size_t)i].src_h = shapes[i][1]; items[(size_t)i].comps = shapes[i][2];
  }
  const ResampleLayout L = resample_layout(items.data(), n, out_w, out_h);
  CHECK(L.per.size() == 4);
  if (L.per.size() != 4) return;
  const uint64_t tiles = resample_tiles(out_w, out_h);
  CHECK(tiles == 1 && L.workgroups == 4 * tiles);
  CHECK(resample_tiles(224, 224) == 4 * 14 && resample_tiles(64, 16) == 1 && resample_tiles(65, 17) == 4);
  CHECK(L.pictures == 0 && L.first == 4 * sizeof(ResamplePicture) && L.first % 16 == 0);
  uint8_t *host = (uint8_t *)malloc(L.table_bytes); // (exactly: the sanitizer sees a byte too many)
  memset(host, 0xEE, L.table_bytes);
  for (size_t k = 0; k < L.per.size(); k++) CHECK(resample_fill(host, L, k, items.data(), out_w, out_h, image_stride));
  resample_fill_first(host, L);
  const ResamplePicture *pics = (const ResamplePicture *)(host + L.pictures);
  const uint32_t *first = (const uint32_t *)(host + L.first);
  const int served[4] = {0, 2, 3, 5};
  size_t at = L.first + 32, src = 0; // (five prefix entries, padded to 16 bytes)
  for (size_t k = 0; k < 4; k++) {
    const ResampleItem &it = items[(size_t)served[k]];
    const ResamplePicture &p = pics[k];
    CHECK(L.per[k].item == served[k]);
    CHECK(first[k] == k * tiles);
    CHECK(p.src_off == src && p.src_off % 16 == 0);
    CHECK(p.dst_off == (uint64_t)served[k] * (uint64_t)image_stride);
    CHECK(p.src_w == it.src_w && p.src_h == it.src_h && p.comps == it.comps && p.tiles_x == 1);
    CHECK(p.xcap == resample_taps(it.src_w, out_w, nullptr, nullptr, nullptr, 0) && p.ycap == resample_taps(it.src_h, out_h, nullptr, nullptr, nullptr, 0));
    CHECK(p.xtab == at && p.xtab % 16 == 0);
    at += resample_axis_bytes(out_w, p.xcap);
    CHECK(p.ytab == at && p.ytab % 16 == 0);
    at += resample_axis_bytes(out_h, p.ycap);
    src += resample_crop_bytes(it.src_w, it.src_h, it.comps);
    // the tables are the single axes' tables
    std::vector<int32_t> f((size_t)out_w), c((size_t)out_w);
    std::vector<int16_t> w((size_t)out_w * (size_t)p.xcap);
    CHECK(resample_taps(it.src_w, out_w, f.data(), c.data(), w.data(), p.xcap) == p.xcap);
    const int32_t *xt = (const int32_t *)(host + p.xtab);
    CHECK(!memcmp(xt, f.data(), (size_t)out_w * 4) && !memcmp(xt + out_w, c.data(), (size_t)out_w * 4) && !memcmp(xt + 2 * out_w, w.data(), w.size() * 2));
    f.assign((size_t)out_h, 0); c.assign((size_t)out_h, 0); w.assign((size_t)out_h * (size_t)p.ycap, 0);
    CHECK(resample_taps(it.src_h, out_h, f.data(), c.data(), w.data(), p.ycap) == p.ycap);
    const int32_t *yt = (const int32_t *)(host + p.ytab);
    CHECK(!memcmp(yt, f.data(), (size_t)out_h * 4) && !memcmp(yt + out_h, c.data(), (size_t)out_h * 4) && !memcmp(yt + 2 * out_h, w.data(), w.size() * 2));
    // every tap the kernel reads lies inside the crop
    for (int o = 0; o < out_w; o++) CHECK(xt[o] >= 0 && xt[o] + xt[out_w + o] <= it.src_w);
    for (int o = 0; o < out_h; o++) CHECK(yt[o] >= 0 && yt[o] + yt[out_h + o] <= it.src_h);
  }
  CHECK(first[4] == 4 * tiles);
  CHECK(at == L.table_bytes && src == L.arena_bytes);
  free(host);
  // a list without a served member
  std::vector<ResampleItem> none(3);
  const ResampleLayout E = resample_layout(none.data(), 3, 8, 8);
  CHECK(E.per.empty() && E.workgroups == 0 && E.arena_bytes == 0);
}

int main()
{
  const int32_t sizes[] = {1, 2, 3, 7, 8, 9, 16, 127, 128, 129, 300};
  for (int32_t n : sizes)
    for (int32_t m : sizes) check_axis(n, m);
  check_axis(65535, 224);
  check_axis(224, 65535);
  check_axis(65535, 1);
  check_axis(1, 65535);
  check_axis(65535, 65535);
  check_axis(65535, 65534);
  CHECK(resample_taps(0, 5, nullptr, nullptr, nullptr, 0) == 0 && resample_taps(5, 0, nullptr, nullptr, nullptr, 0) == 0);
  CHECK(resample_taps(65536, 5, nullptr, nullptr, nullptr, 0) == 0 && resample_taps(5, 65536, nullptr, nullptr, nullptr, 0) == 0);
  check_layout();
  if (failures) {
    printf("FAILED %d checks\n", failures);
    return 1;
  }
  printf("OK resample taps and tables\n");
  return 0;
}
