// transcode_tables.cpp -- the device-free half of the ragged transcode (libjpeg_amd/csrc/requant.hpp, encode_list.hpp) as a
// program of its own, for the sanitizers: the rule against 64-bit arithmetic, then lists of decoded pictures -- group members and
// children whose planes have other pitches and an MCU row more, both precisions, kept and requantised, with and without tables of their
// own, cut into passes -- through the real plan, pass layout and fill, into heap buffers of exactly up_bytes and host_bytes.  The
// device arena is a heap buffer of exactly dev_bytes and every source a heap buffer of exactly its frame's coefficients: the work
// list is then walked on the host the way requant_list_kernel addresses it, lane by lane, so that an offset outside a store is the
// sanitizer's to find, and what arrives in the pass's coefficient store is compared with requantize_blocks.  No device; of the
// library only encoder.cpp.  (tests/test_ragged_transcode_cpu.py builds it with -fsanitize=address,undefined and runs it.)
#include <stdio.h>
#include <stdlib.h>

#include <functional>
#include <memory>

#include "encode_list.hpp"

using namespace mij;

// what encoder.cpp's coder and header writer ask of worker_pool.cpp and host_decoder.cpp; nothing here calls them
namespace mij {
int default_threads() { return 1; }
void parallel_for(int n, const std::function<void(int)> &fn) { for (int i = 0; i < n; i++) fn(i); }
const uint8_t *scan_order()
{
  static uint8_t zz[64];
  for (int k = 0, x = 0, y = 0; k < 64; k++) { // the zig-zag walk
    zz[k] = (uint8_t)(y * 8 + x);
    if ((x + y) & 1) { if (y == 7) x++; else if (x == 0) y++; else { x--; y++; } }
    else { if (x == 7) y++; else if (y == 0) x++; else { x++; y--; } }
  }
  return zz;
}
} // namespace mij

static int failures = 0;
static const char *list_name = "";
#define CHECK(cond)                                                                     \
  do {                                                                                  \
    if (!(cond)) {                                                                      \
      failures++;                                                                       \
      fprintf(stderr, "line %d (%s): %s does not hold\n", __LINE__, list_name, #cond); \
    }                                                                                   \
  } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd()
{
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 24);
}

// ---- the rule -----------------------------------------------------------------------------------------------------------
static int64_t exact(int64_t c, int64_t a, int64_t b)
{
  const int64_t v = c * a, q = ((v < 0 ? -v : v) + b / 2) / b;
  return v < 0 ? -q : q;
}
static void check_rule()
{
  list_name = "rule";
  const int cs[] = {0, 1, -1, 2, -2, 1023, -1023, -1024, 1024, 16383, -16383, -16384, 16384, 32767, -32767, -32768};
  const uint32_t qs[] = {1, 2, 3, 4, 5, 7, 16, 17, 99, 254, 255, 256, 257, 1000, 4095, 4096, 32766, 32767, 32768, 65534, 65535};
  long checked = 0;
  auto one = [&](int c, uint32_t a, uint32_t b) {
    bool beyond = false;
    const int wide = requant_value(c, a, b, requant_reciprocal(b), -(1 << 30), 1 << 30, beyond); // (no frame has this range: the division alone)
    const int64_t want = exact(c, a, b);
    if (want >= -(1 << 30) && want <= (1 << 30)) CHECK(!beyond && wide == want);
    for (int precision : {8, 12}) {
      const RequantRange r = requant_range(precision);
      for (int dc = 0; dc < 2; dc++) {
        const int lo = dc ? r.dc_min : -r.ac_max, hi = dc ? r.dc_max : r.ac_max;
        beyond = false;
        const int got = requant_value(c, a, b, requant_reciprocal(b), lo, hi, beyond);
        CHECK(beyond == (want < lo || want > hi) && got == (want < lo ? lo : want > hi ? hi : want));
      }
    }
    checked++;
  };
  for (int c : cs)
    for (uint32_t a : qs)
      for (uint32_t b : qs) one(c, a, b);
  for (uint32_t b : qs) // halves of both signs, one below and one above them: c * 1 = k * b + b / 2 (+-1)
    for (int k = 0; k < 6; k++)
      for (int d = -1; d <= 1; d++) {
        const int64_t v = (int64_t)k * b + b / 2 + d;
        if (v > 32767) continue;
        one((int)v, 1, b);
        one((int)-v, 1, b);
      }
  for (int i = 0; i < 200000; i++) one((int)(rnd() & 0xffff) - 32768, (rnd() & 0xffff) | (i & 1), (rnd() % 65535) + 1);
  for (int c = -32768; c <= 32767; c++) one(c, 65535, 1), one(c, 65535, 65535), one(c, 1, 2);
  CHECK(requant_range(8).dc_min == -1024 && requant_range(8).dc_max == 1023 && requant_range(8).ac_max == 1023);
  CHECK(requant_range(12).dc_min == -16384 && requant_range(12).dc_max == 16383 && requant_range(12).ac_max == 16383);
  CHECK(checked > 300000);
}

// ---- decoded pictures -----------------------------------------------------------------------------------------------------
struct Decoded { int w, h, nc, hs, vs, precision, quality, ri; bool extra_row; int spec_quality, spec_ri; };

// the frame a decoder reports: two tables in use; extra_row: the planes hold an MCU row more than the frame's grid (what a DNL
// frame's do), so the source's plane sizes and offsets differ from every output's
static mijpeg_info decoded_info(const Decoded &s)
{
  mijpeg_info f;
  int32_t hs[4] = {s.hs, 1, 1, 1}, vs[4] = {s.vs, 1, 1, 1};
  if (picture_info_of(s.w, s.h, s.nc, hs, vs, s.quality, f, s.precision)) exit(2);
  for (int c = 1; c < s.nc; c++) f.quant_index[c] = 1;
  f.restart_interval = s.ri;
  if (s.extra_row) {
    int64_t off = 0;
    for (int c = 0; c < s.nc; c++) {
      f.blocks_h[c] += f.vsamp[c];
      f.coef_offset[c] = off;
      off += (int64_t)f.blocks_w[c] * f.blocks_h[c] * 64;
    }
    f.coef_count = off;
    f.dnl = 1;
  }
  return f;
}

// requant_list_kernel's addressing on the host: every workgroup of the grid, every lane
static void walk_work_list(const RequantArgs &a, uint32_t grid, uint32_t n)
{
  for (uint32_t wg = 0; wg < grid; wg++) {
    uint32_t lo = 0, hi = a.items;
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (a.first_wg[mid] <= wg) lo = mid;
      else hi = mid;
    }
    CHECK(a.first_wg[lo] <= wg && wg < a.first_wg[lo + 1]);
    const uint32_t it = a.item[lo], pic = it >> 2, c = it & 3;
    CHECK(pic < n);
    if (pic >= n) return;
    const RequantPicture &p = a.pics[pic];
    CHECK((int)c < p.ncomp);
    const uint32_t dbw = (uint32_t)p.dst_bw[c], dblocks = dbw * (uint32_t)p.dst_bh[c];
    for (uint32_t lane = 0; lane < REQUANT_GROUP; lane++) {
      const uint32_t blk = (wg - a.first_wg[lo]) * REQUANT_WG_BLOCKS + (lane >> 3), row = lane & 7;
      if (blk >= dblocks) continue;
      const uint32_t by = blk / dbw, bx = blk - by * dbw;
      int16_t out[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      bool beyond = false;
      if (bx < (uint32_t)p.src_bw[c] && by < (uint32_t)p.src_bh[c]) {
        const int16_t *in = p.src + p.src_off[c] + (int64_t)(((uint64_t)by * (uint32_t)p.src_bw[c] + bx) * 64 + row * 8);
        const RequantTables &t = p.t[c];
        for (int j = 0; j < 8; j++) {
          const bool dc = row == 0 && j == 0;
          out[j] = (int16_t)requant_value(in[j], t.a[row * 8 + j], t.b[row * 8 + j], t.m[row * 8 + j], dc ? p.range.dc_min : -p.range.ac_max,
                                          dc ? p.range.dc_max : p.range.ac_max, beyond);
        }
      }
      memcpy(p.dst + p.dst_off[c] + (int64_t)((uint64_t)blk * 64 + row * 8), out, sizeof(out));
      if (beyond) a.flags[pic] = 1;
    }
  }
}

static int run_list(const char *name, const std::vector<Decoded> &list, int optimize, uint32_t pass_blocks, int want_passes)
{
  list_name = name;
  const int n = (int)list.size();
  std::vector<mijpeg_info> infos;
  std::vector<std::unique_ptr<int16_t[]>> stores; // every source: exactly its frame's coefficients
  std::vector<mijpeg_encode_frame> frames;
  std::vector<mijpeg_encode_ragged_item> items;
  std::vector<RequantSource> sources;
  std::vector<char> kept;
  mijpeg_encode_ragged_totals totals;
  memset(&totals, 0, sizeof(totals));
  PassCutter cut{pass_blocks ? pass_blocks : PASS_BLOCKS_DEFAULT};
  for (int i = 0; i < n; i++) {
    const Decoded &s = list[(size_t)i];
    infos.push_back(decoded_info(s));
    const mijpeg_info &f = infos.back();
    stores.emplace_back(new int16_t[(size_t)f.coef_count]);
    const RequantRange r = requant_range(f.precision);
    for (int64_t k = 0; k < f.coef_count; k++) // (inside the coding range; one picture in seven carries a value outside it)
      stores.back()[(size_t)k] = (k & 63) ? (int16_t)((int)(rnd() % (2u * (uint32_t)r.ac_max + 1)) - r.ac_max) : (int16_t)((int)(rnd() % (2u * (uint32_t)r.dc_max + 2)) + r.dc_min);
    if (i % 7 == 3) stores.back()[65] = (int16_t)(r.ac_max + 1);
    mijpeg_encode_ragged_item it;
    memset(&it, 0, sizeof(it));
    int ri = -1;
    bool keeps = false;
    const mijpeg_transcode_spec spec{s.spec_quality, s.spec_ri};
    CHECK(transcode_spec_in_order(spec));
    CHECK(transcode_plan_one(f, spec, it.info, ri, keeps, it.blocks, it.intervals) == MIJPEG_OK);
    CHECK(keeps == (s.spec_quality == 0) && ri == (s.spec_ri < 0 ? s.ri : s.spec_ri));
    CHECK(it.info.width == f.width && it.info.height == f.height && it.info.precision == f.precision && it.info.components == f.components && !it.info.dnl);
    for (int c = 0; c < f.components; c++) {
      CHECK(it.info.hsamp[c] == (f.components == 1 ? 1 : f.hsamp[c]) && it.info.quant_index[c] == (keeps ? f.quant_index[c] : 0));
      if (keeps) CHECK(memcmp(it.info.quant[it.info.quant_index[c]], f.quant[f.quant_index[c]], 128) == 0);
    }
    mijpeg_encode_frame e;
    memset(&e, 0, sizeof(e));
    e.width = f.width; e.height = f.height; e.components = f.components;
    for (int c = 0; c < 4; c++) { e.hsamp[c] = it.info.hsamp[c]; e.vsamp[c] = it.info.vsamp[c]; }
    e.restart_interval = ri;
    cut.place(it, &totals);
    frames.push_back(e);
    items.push_back(it);
    sources.push_back(RequantSource{f, stores.back().get()});
    kept.push_back(keeps);
  }
  CHECK(cut.pass + 1 == want_passes);
  int passes = 0;
  for (int p0 = 0; p0 < n;) {
    int p1 = p0 + 1;
    while (p1 < n && items[(size_t)p1].pass == items[(size_t)p0].pass) p1++;
    const EncodePassLayout L(frames.data(), items.data(), p0, p1, optimize, nullptr, sources.data());
    CHECK(L.error == MIJPEG_OK);
    if (L.error) return passes;
    const uint32_t m = L.n;
    // the regions: the forward lists and the ForwardArgs are empty, the requant regions follow the plane table's place in order
    CHECK(L.fargs_at == 0 && L.hargs_at == 0 && L.n_planar == 0);
    for (int l = 0; l < FORWARD_RAGGED_LISTS; l++) CHECK(L.lists[l].item.empty() && L.lists[l].first.empty());
    CHECK(L.rq_pics_at % 256 == 0 && L.rq_pics_at >= L.std_tables_at + sizeof(HencTables) && L.rq_first_at >= L.rq_pics_at + m * sizeof(RequantPicture));
    CHECK(L.rq_item_at >= L.rq_first_at + L.requant.first.size() * 4 && L.rq_flags_at >= L.rq_item_at + L.requant.item.size() * 4 && L.up_bytes >= L.rq_flags_at + m * 4);
    CHECK(L.rq_first_at % 256 == 0 && L.rq_item_at % 256 == 0 && L.rq_flags_at % 256 == 0 && L.up_bytes % 256 == 0);
    CHECK(L.h_flags >= L.h_ffstart + (m + 1) * 8 && L.host_bytes >= L.h_flags + m * 4 && L.d_first_chunk >= L.up_bytes && L.h_first_chunk >= L.up_bytes);
    CHECK(L.coef_at + (size_t)L.coef_total * 2 <= L.dev_bytes);
    uint32_t own = 0;
    for (uint32_t p = 0; p < m; p++) own += optimize || items[(size_t)p0 + p].info.precision == 12;
    CHECK(L.n_own == own);
    uint8_t *dev = (uint8_t *)aligned_alloc(256, L.dev_bytes), *only_up = (uint8_t *)malloc(L.up_bytes), *host = (uint8_t *)malloc(L.host_bytes);
    if (!dev || !only_up || !host) exit(2);
    memset(only_up, 0xA5, L.up_bytes);
    memset(host, 0xA5, L.host_bytes);
    memset(dev + L.coef_at, 0x5A, (size_t)L.coef_total * 2);
    EncTables std_tabs;
    enc_standard_tables(std_tabs);
    (void)fill_upload(only_up, dev, L, std_tabs);
    const EncodePassArgs a = fill_upload(host, dev, L, std_tabs);
    CHECK(memcmp(only_up, host, L.up_bytes) == 0);
    free(only_up);
    for (size_t i = L.up_bytes; i < L.host_bytes; i++)
      if (host[i] != 0xA5) { CHECK(!"fill_upload wrote behind the uploaded part"); break; }
    memcpy(dev, host, L.up_bytes); // (the one upload)
    CHECK((const uint8_t *)a.requant.pics == dev + L.rq_pics_at && (const uint8_t *)a.requant.first_wg == dev + L.rq_first_at);
    CHECK((const uint8_t *)a.requant.item == dev + L.rq_item_at && (uint8_t *)a.requant.flags == dev + L.rq_flags_at && a.requant.items == L.requant.item.size());
    CHECK(a.requant_grid == a.requant.first_wg[a.requant.items] && a.requant.first_wg[0] == 0 && a.requant_grid <= 0x7fffffffu);
    for (int l = 0; l < FORWARD_RAGGED_LISTS; l++) CHECK(a.forward.grid[l] == 0 && a.forward.launch[l].items == 0);
    uint32_t item = 0;
    for (uint32_t p = 0; p < m; p++) {
      const mijpeg_encode_ragged_item &it = items[(size_t)p0 + p];
      const RequantPicture &q = a.requant.pics[p];
      const HencArgs &h = ((const HencArgs *)(dev + L.hargs_at))[p];
      CHECK(q.src == sources[(size_t)p0 + p].planes && q.dst == (int16_t *)(dev + L.coef_at) + it.coef_base && (const int16_t *)h.coef == q.dst);
      CHECK((uintptr_t)q.dst % 256 == 0 && (uintptr_t)&q.t[0] % 16 == 0 && q.ncomp == it.info.components && a.requant.flags[p] == 0);
      CHECK(h.total_blocks == it.blocks && h.n_intervals == it.intervals && h.ri == (frames[(size_t)p0 + p].restart_interval ? frames[(size_t)p0 + p].restart_interval : h.total_mcus));
      for (int c = 0; c < q.ncomp; c++, item++) {
        CHECK(a.requant.item[item] == p * 4 + (uint32_t)c);
        CHECK(a.requant.first_wg[item + 1] - a.requant.first_wg[item] == ((uint32_t)(q.dst_bw[c] * q.dst_bh[c]) + REQUANT_WG_BLOCKS - 1) / REQUANT_WG_BLOCKS);
        CHECK(q.dst_off[c] + (int64_t)q.dst_bw[c] * q.dst_bh[c] * 64 <= it.info.coef_count);
      }
    }
    CHECK(item == a.requant.items);
    walk_work_list(a.requant, a.requant_grid, m);
    // what arrived: every destination block from its source block by the rule over blocks, zero where the source has none
    for (uint32_t p = 0; p < m; p++) {
      const mijpeg_info &f = infos[(size_t)p0 + p], &o = items[(size_t)p0 + p].info;
      const int16_t *src = sources[(size_t)p0 + p].planes, *dst = (const int16_t *)(dev + L.coef_at) + items[(size_t)p0 + p].coef_base;
      int64_t clamped = 0;
      bool same = true;
      for (int c = 0; c < o.components; c++)
        for (int by = 0; by < o.blocks_h[c]; by++)
          for (int bx = 0; bx < o.blocks_w[c]; bx++) {
            int16_t want[64] = {0};
            if (bx < f.blocks_w[c] && by < f.blocks_h[c])
              clamped += requantize_blocks(src + f.coef_offset[c] + ((int64_t)by * f.blocks_w[c] + bx) * 64, want, 1, f.quant[f.quant_index[c]], o.quant[o.quant_index[c]], o.precision);
            same = same && memcmp(want, dst + o.coef_offset[c] + ((int64_t)by * o.blocks_w[c] + bx) * 64, sizeof(want)) == 0;
          }
      CHECK(same);
      CHECK((a.requant.flags[p] != 0) == (clamped != 0));
      if (kept[(size_t)p0 + p] && !list[(size_t)p0 + p].extra_row && list[(size_t)p0 + p].nc == 3 && !clamped) CHECK(memcmp(src, dst, (size_t)f.coef_count * 2) == 0);
    }
    free(host);
    free(dev);
    passes++;
    p0 = p1;
  }
  CHECK(passes == want_passes);
  return passes;
}

int main()
{
  check_rule();
  // group members and children of both precisions; kept (quality 0) and requantised; restart intervals kept, dropped and set
  const std::vector<Decoded> mixed = {
      {131, 77, 3, 2, 1, 8, 75, 0, false, 0, -1},  {80, 48, 3, 1, 1, 8, 90, 5, false, 50, 0},   {70, 40, 1, 1, 1, 8, 60, 0, false, 95, 1},
      {9, 9, 3, 2, 2, 8, 30, 0, false, 100, -1},   {1, 1, 3, 1, 1, 8, 85, 0, false, 0, -1},     {120, 90, 3, 2, 2, 12, 75, 3, false, 0, -1},
      {64, 48, 3, 1, 1, 12, 2, 0, false, 30, 7},   {97, 61, 3, 1, 2, 8, 75, 0, true, 75, -1},   {97, 61, 3, 4, 1, 8, 75, 0, false, 0, 2},
      {23, 50, 1, 2, 1, 8, 50, 0, false, 0, -1},   {136, 136, 3, 2, 2, 8, 75, 8, true, 0, -1},  {33, 7, 1, 1, 1, 12, 75, 0, true, 2, 0}};
  int passes = run_list("one pass", mixed, 0, 0, 1);
  passes += run_list("own tables", mixed, 1, 0, 1);
  passes += run_list("cut", mixed, 0, 1024, 4); // (padded blocks 512 256 256 | 256 256 512 | 256 256 256 256 | 512 256)
  // refusals of the plan
  list_name = "refusals";
  {
    mijpeg_info f = decoded_info(mixed[0]), out;
    int ri;
    bool keeps;
    uint32_t b, iv;
    const mijpeg_transcode_spec keep{0, -1}, q50{50, -1};
    mijpeg_info x = f; x.xt = 1;
    CHECK(transcode_plan_one(x, keep, out, ri, keeps, b, iv) == MIJPEG_ERR_NOT_IMPLEMENTED && out.width == 0);
    x = f; x.coef_wide = 1;
    CHECK(transcode_plan_one(x, q50, out, ri, keeps, b, iv) == MIJPEG_ERR_NOT_IMPLEMENTED);
    x = f; x.components = 4;
    CHECK(transcode_plan_one(x, q50, out, ri, keeps, b, iv) == MIJPEG_ERR_NOT_IMPLEMENTED);
    x = f; x.quant[1][63] = 256;
    CHECK(transcode_plan_one(x, keep, out, ri, keeps, b, iv) == MIJPEG_ERR_NOT_IMPLEMENTED && transcode_plan_one(x, q50, out, ri, keeps, b, iv) == MIJPEG_OK);
    x = f; x.quant[0][5] = 0;
    CHECK(transcode_plan_one(x, q50, out, ri, keeps, b, iv) == MIJPEG_ERR_NOT_IMPLEMENTED);
    CHECK(!transcode_spec_in_order(mijpeg_transcode_spec{101, 0}) && !transcode_spec_in_order(mijpeg_transcode_spec{-2, 0}) && !transcode_spec_in_order(mijpeg_transcode_spec{50, 65536}) &&
          !transcode_spec_in_order(mijpeg_transcode_spec{50, -2}) && transcode_spec_in_order(mijpeg_transcode_spec{-1, 65535}));
  }
  if (failures) return 1;
  printf("OK %d passes of 3 lists\n", passes);
  return 0;
}
