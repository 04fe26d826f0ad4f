// fused_window_tables.cpp -- the host half of the WINDOW launches (libjpeg_amd/csrc/fused_list.hpp: the crop windows of a list) as a
// program of its own, for the sanitizers: hand-made frames with crop rectangles are grouped into launches, their tables laid out and
// filled into a heap buffer of exactly the layout's size, and read back -- offsets and alignment, first[] as the prefix of the
// WINDOW's tiles, every listed tile against its rectangle by brute force, and the biased base: base + the offset the kernels form
// for pixel (min_x, min_y) is the caller's pointer.  No device, nothing of the library is linked.
// (tests/test_ragged_rect_cpu.py builds it with -fsanitize=address,undefined and runs it.)
#include <stdio.h>
#include <stdlib.h>

#include "fused_list.hpp"

using namespace mij;

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      failures++;                                                          \
      fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond);     \
    }                                                                      \
  } while (0)

static mijpeg_info frame(int w, int h, int components, int hs, int vs)
{
  mijpeg_info f;
  memset(&f, 0, sizeof(f));
  f.width = w; f.height = h; f.components = components; f.precision = 8; f.ycbcr = 1; f.fast_arith = 1; f.sample_bytes = 1;
  f.mcus_x = (w + 8 * hs - 1) / (8 * hs); f.mcus_y = (h + 8 * vs - 1) / (8 * vs);
  int64_t at = 0;
  for (int c = 0; c < components; c++) {
    f.hsamp[c] = c ? 1 : hs; f.vsamp[c] = c ? 1 : vs;
    f.subx[c] = c ? hs : 1; f.suby[c] = c ? vs : 1;
    f.quant_index[c] = c ? 1 : 0;
    f.blocks_w[c] = f.mcus_x * f.hsamp[c]; f.blocks_h[c] = f.mcus_y * f.vsamp[c];
    f.coef_offset[c] = at;
    at += (int64_t)f.blocks_w[c] * f.blocks_h[c] * 64;
  }
  f.coef_count = at;
  for (int t = 0; t < 4; t++)
    for (int z = 0; z < 64; z++) f.quant[t][z] = (uint16_t)(1 + 100 * t + z);
  return f;
}

static ReconPlan plan(Recon k, Sampling s)
{
  ReconPlan p{};
  p.kernel = k; p.sampling = s; p.fast = true;
  return p;
}

// does tile (tx, ty) hold a pixel of w?  (brute force over the tile's 128 x 128 pixels' bounds)
static bool tile_meets(int tx, int ty, const mijpeg_rect &w)
{
  for (int y = ty * 128; y < ty * 128 + 128; y++)
    if (y >= w.min_y && y <= w.max_y)
      for (int x = tx * 128; x < tx * 128 + 128; x++)
        if (x >= w.min_x && x <= w.max_x) return true;
  return false;
}

static void check_tables(const uint8_t *host, const FusedListTable &t, const FusedListLaunch &l, const FusedListItem *items, bool planar)
{
  const size_t m = l.members.size();
  CHECK(t.frames % 16 == 0 && t.first % 16 == 0 && t.deltas % 16 == 0 && t.planes % 16 == 0 && t.windows % 16 == 0 && t.end % 16 == 0);
  CHECK(t.first == t.frames + m * 96 && t.deltas == t.first + ((m + 1) * 4 + 15) / 16 * 16 && t.planes == t.deltas + m * 1024);
  CHECK(t.windows == t.planes + (planar ? m * 16 : 0) && t.end == t.windows + m * 32); // (the kernels find the windows behind the planes)
  const RaggedFrame *fr = (const RaggedFrame *)(host + t.frames);
  const uint32_t *first = (const uint32_t *)(host + t.first);
  const PlanarFrame *pl = (const PlanarFrame *)(host + t.planes);
  const WindowFrame *win = (const WindowFrame *)(host + t.windows);
  uint32_t at = 0;
  for (size_t k = 0; k < m; k++) {
    const FusedListItem &it = items[l.members[k]];
    const mijpeg_info &f = *it.info;
    const mijpeg_rect &w = *it.window;
    const RaggedFrame &x = fr[k];
    const WindowFrame &v = win[k];
    // the frame's geometry is the PICTURE's
    CHECK(x.width == f.width && x.height == f.height && x.tiles_x == (f.width + 127) / 128 && x.tiles_y == (f.height + 127) / 128);
    CHECK(x.coef_base == it.coef_base && x.row_stride == it.row_stride && x.qframe == (int32_t)k);
    CHECK(v.min_x == w.min_x && v.min_y == w.min_y && v.max_x == w.max_x && v.max_y == w.max_y);
    CHECK(first[k] == at);
    // every tile the frame's workgroups map to meets the rectangle, and no tile of the picture that meets it is missing
    const uint32_t count = (uint32_t)(v.wtiles_x * v.wtiles_y);
    std::vector<char> listed((size_t)(x.tiles_x * x.tiles_y), 0);
    for (uint32_t local = 0; local < count; local++) {
      const int tx = v.tile_x0 + (int)(local % (uint32_t)v.wtiles_x), ty = v.tile_y0 + (int)(local / (uint32_t)v.wtiles_x);
      CHECK(tx >= 0 && tx < x.tiles_x && ty >= 0 && ty < x.tiles_y);
      CHECK(tile_meets(tx, ty, w));
      if (tx >= 0 && tx < x.tiles_x && ty >= 0 && ty < x.tiles_y) {
        CHECK(!listed[(size_t)(ty * x.tiles_x + tx)]);
        listed[(size_t)(ty * x.tiles_x + tx)] = 1;
      }
    }
    for (int ty = 0; ty < x.tiles_y; ty++)
      for (int tx = 0; tx < x.tiles_x; tx++) CHECK((listed[(size_t)(ty * x.tiles_x + tx)] != 0) == tile_meets(tx, ty, w));
    at += count;
    // the biased base: what the kernels add for pixel (min_x, min_y) -- Y * row_stride + X * bytes per pixel, 32 bits -- leads to
    // the caller's pointer (integers: the base itself may lie in front of every object)
    const int bpp = planar ? 1 : f.components;
    const uint32_t off = (uint32_t)w.min_y * (uint32_t)it.row_stride + (uint32_t)w.min_x * (uint32_t)bpp;
    CHECK((uintptr_t)x.out + off == (uintptr_t)it.out[0]);
    if (planar) CHECK((uintptr_t)pl[k].g + off == (uintptr_t)it.out[1] && (uintptr_t)pl[k].b + off == (uintptr_t)it.out[2]);
  }
  CHECK(first[m] == at && at == l.grid);
}

int main()
{
  std::vector<mijpeg_info> infos;
  infos.push_back(frame(300, 270, 3, 2, 2)); // 0  3 x 3 tiles
  infos.push_back(frame(300, 270, 3, 2, 2)); // 1
  infos.push_back(frame(129, 131, 3, 2, 2)); // 2
  infos.push_back(frame(16, 16, 1, 1, 1));   // 3  grey
  infos.push_back(frame(257, 40, 1, 1, 1));  // 4
  infos.push_back(frame(1000, 700, 3, 2, 2)); // 5  8 x 6 tiles
  infos.push_back(frame(300, 270, 3, 2, 2)); // 6
  // rectangles as a caller writes them, and what clipping leaves
  const mijpeg_rect asked[] = {{0, 0, INT32_MAX, INT32_MAX}, {130, 129, 299, 269}, {127, 0, 128, 130}, {9, 10, 14, 13}, {128, 39, 5000, 39},
                               {383, 255, 640, 384}, {299, 269, 299, 269}};
  const mijpeg_rect want[] = {{0, 0, 299, 269}, {130, 129, 299, 269}, {127, 0, 128, 130}, {9, 10, 14, 13}, {128, 39, 256, 39}, {383, 255, 640, 384}, {299, 269, 299, 269}};
  const uint64_t tiles[] = {9, 4, 4, 1, 2, 4 * 3, 1};
  std::vector<mijpeg_rect> clipped(infos.size());
  for (size_t i = 0; i < infos.size(); i++) {
    CHECK(fused_window_clip(asked[i], infos[i].width, infos[i].height, clipped[i]));
    CHECK(clipped[i].min_x == want[i].min_x && clipped[i].min_y == want[i].min_y && clipped[i].max_x == want[i].max_x && clipped[i].max_y == want[i].max_y);
    CHECK(fused_list_tiles(infos[i], &clipped[i]) == tiles[i]);
    CHECK(fused_list_tiles(infos[i], nullptr) == fused_list_tiles(infos[i]));
  }
  // what the calls refuse
  mijpeg_rect r;
  CHECK(!fused_window_clip(mijpeg_rect{-1, 0, 5, 5}, 16, 16, r) && !fused_window_clip(mijpeg_rect{0, -1, 5, 5}, 16, 16, r));
  CHECK(!fused_window_clip(mijpeg_rect{16, 0, 20, 5}, 16, 16, r) && !fused_window_clip(mijpeg_rect{0, 16, 5, 20}, 16, 16, r));
  CHECK(!fused_window_clip(mijpeg_rect{5, 0, 4, 5}, 16, 16, r) && !fused_window_clip(mijpeg_rect{0, 5, 5, 4}, 16, 16, r));
  CHECK(!fused_window_clip(mijpeg_rect{0, 0, -1, -1}, 16, 16, r) && !fused_window_clip(mijpeg_rect{0, 0, 0, 0}, 0, 16, r));
  CHECK(fused_window_clip(mijpeg_rect{15, 15, 15, 15}, 16, 16, r) && r.max_x == 15 && r.max_y == 15);

  // destinations: heap blocks of exactly a crop's bytes (line padding included), at odd addresses; nothing is written through them
  std::vector<uint8_t *> blocks;
  std::vector<FusedListItem> items;
  std::vector<FusedListLaunch> launches;
  const ReconPlan p420 = plan(Recon::FUSED420P, Sampling::S420), pgrey = plan(Recon::FUSED1, Sampling::GREY);
  int64_t base = 0;
  for (size_t i = 0; i < infos.size(); i++) {
    const mijpeg_info &f = infos[i];
    const mijpeg_rect &w = clipped[i];
    const int64_t stride = (int64_t)(w.max_x - w.min_x + 1) * f.components + 5;
    const size_t bytes = (size_t)(stride * (w.max_y - w.min_y + 1)) + 3;
    uint8_t *b0 = (uint8_t *)malloc(bytes), *b1 = (uint8_t *)malloc(bytes), *b2 = (uint8_t *)malloc(bytes);
    if (!b0 || !b1 || !b2) return 2;
    blocks.push_back(b0); blocks.push_back(b1); blocks.push_back(b2);
    fused_list_add(launches, f.components == 1 ? pgrey : p420, (int)i, f, &w);
    items.push_back(FusedListItem{&f, base, {b0 + (i & 3), b1 + (i & 3), b2 + (i & 3)}, stride, nullptr, &w});
    base += f.coef_count;
  }
  CHECK(launches.size() == 2);
  CHECK(launches[0].members == std::vector<int>({0, 1, 2, 5, 6}) && launches[0].grid == 9 + 4 + 4 + 12 + 1);
  CHECK(launches[1].members == std::vector<int>({3, 4}) && launches[1].grid == 1 + 2);
  size_t total = 0;
  for (int planar = 0; planar < 2; planar++) {
    const std::vector<FusedListTable> tables = fused_list_layout(launches, planar != 0, true);
    CHECK(tables.size() == 2 && tables[0].frames == 0 && tables[1].frames == tables[0].end);
    const size_t bytes = tables.back().end;
    uint8_t *host = (uint8_t *)malloc(bytes); // (exactly the layout: a byte further is the sanitizer's)
    if (!host) return 2;
    memset(host, 0xA5, bytes);
    for (size_t l = 0; l < launches.size(); l++) fused_list_fill(host, tables[l], launches[l], items.data(), planar != 0, true);
    // (a planar call's grey launch is its own plane: bytes per pixel are 1 either way, its PlanarFrame entries are nobody's)
    check_tables(host, tables[0], launches[0], items.data(), planar != 0);
    {
      const FusedListTable &t = tables[1];
      const RaggedFrame *fr = (const RaggedFrame *)(host + t.frames);
      const WindowFrame *win = (const WindowFrame *)(host + t.windows);
      for (size_t k = 0; k < 2; k++) {
        const FusedListItem &it = items[launches[1].members[k]];
        const uint32_t off = (uint32_t)it.window->min_y * (uint32_t)it.row_stride + (uint32_t)it.window->min_x;
        CHECK((uintptr_t)fr[k].out + off == (uintptr_t)it.out[0]);
        CHECK(win[k].tile_x0 == it.window->min_x >> 7 && win[k].tile_y0 == it.window->min_y >> 7);
      }
      CHECK(t.end == t.windows + 2 * 32);
    }
    total += bytes;
    free(host);
  }
  // a window launch without windows is the launch of before: same layout, same bytes
  {
    const std::vector<FusedListTable> a = fused_list_layout(launches, false), b = fused_list_layout(launches, false, false);
    CHECK(a.back().end == b.back().end && a[0].windows == a[0].end && a[0].planes == a[0].end);
  }
  for (uint8_t *b : blocks) free(b);
  if (failures) return 1;
  printf("OK %zu bytes of tables, %zu launches\n", total, launches.size());
  return 0;
}
