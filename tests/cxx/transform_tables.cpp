// transform_tables.cpp -- the device-free half of the ragged transcode's transforms (libjpeg_amd/csrc/transform.hpp, encode_list.hpp;
// DESIGN 4.3e) as a program of its own, for the sanitizers: lists of decoded pictures, transformed and not, trimmed, both precisions,
// kept and requantised, children whose planes hold an MCU row more -- through the real plan, pass layout and fill, into heap buffers
// of exactly up_bytes and host_bytes.  The device arena is a heap buffer of exactly dev_bytes and every source a heap buffer of exactly
// its frame's coefficients: both work lists are then walked on the host the way requant_list_kernel and transform_list_kernel
// address them, lane by lane (a block's eight 16-byte row loads from the mirrored or transposed source block, the 8 x 8 exchange, the
// 16-byte store), so that an offset outside a store is the sanitizer's to find, and what arrives in the pass's coefficient store is
// compared with transform_blocks.  A pass without transforms is laid out through the old signatures as well: every offset is the
// same.  No device; of the library only encoder.cpp.  (tests/test_ragged_transform_cpu.py builds and runs it.)
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

struct Decoded { int w, h, nc, hs, vs, precision, quality, ri; bool extra_row; int spec_quality, spec_ri, transform; };

// the frame a decoder reports: two tables in use, without symmetry; extra_row: the planes hold an MCU row more than the frame's grid
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

// the binary search both kernels make
static uint32_t find_item(const RequantArgs &a, uint32_t wg)
{
  uint32_t lo = 0, hi = a.items;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a.first_wg[mid] <= wg) lo = mid;
    else hi = mid;
  }
  CHECK(a.first_wg[lo] <= wg && wg < a.first_wg[lo + 1]);
  return lo;
}

static void finish_row(const RequantPicture &p, uint32_t c, uint32_t bits, uint32_t row, const int16_t in[8], int16_t out[8], bool &beyond)
{
  const RequantTables &t = p.t[c];
  for (uint32_t j = 0; j < 8; j++) {
    const bool dc = row == 0 && j == 0;
    const int v = in[j];
    out[j] = (int16_t)requant_value(transform_negates(bits, j, row) ? -v : v, t.a[row * 8 + j], t.b[row * 8 + j], t.m[row * 8 + j], dc ? p.range.dc_min : -p.range.ac_max,
                                    dc ? p.range.dc_max : p.range.ac_max, beyond);
  }
}

// requant_list_kernel's addressing (bits 0) and transform_list_kernel's on the host: every workgroup of the grid, every lane; the
// pictures of a list are those with or without a transform, never both
static void walk_work_list(const RequantArgs &a, const uint32_t *bits_of, uint32_t grid, uint32_t n)
{
  for (uint32_t wg = 0; wg < grid; wg++) {
    const uint32_t lo = find_item(a, wg), it = a.item[lo], pic = it >> 2, c = it & 3;
    CHECK(pic < n);
    if (pic >= n) return;
    const RequantPicture &p = a.pics[pic];
    const uint32_t bits = bits_of ? bits_of[pic] : 0;
    CHECK((int)c < p.ncomp && (bits_of ? bits != 0 && bits < 8 : true));
    const uint32_t dbw = (uint32_t)p.dst_bw[c], dbh = (uint32_t)p.dst_bh[c], dblocks = dbw * dbh;
    for (uint32_t slot = 0; slot < REQUANT_WG_BLOCKS; slot++) {
      const uint32_t blk = (wg - a.first_wg[lo]) * REQUANT_WG_BLOCKS + slot;
      if (blk >= dblocks) continue;
      const uint32_t by = blk / dbw, bx = blk - by * dbw;
      uint32_t sbx, sby;
      transform_source_block(bits, bx, by, dbw, dbh, sbx, sby);
      const bool has = sbx < (uint32_t)p.src_bw[c] && sby < (uint32_t)p.src_bh[c];
      int16_t rows[8][8]; // what the block's eight lanes load: 16 bytes each
      memset(rows, 0, sizeof(rows));
      for (uint32_t row = 0; has && row < 8; row++)
        memcpy(rows[row], p.src + p.src_off[c] + (int64_t)(((uint64_t)sby * (uint32_t)p.src_bw[c] + sbx) * 64 + row * 8), 16);
      if (bits & TRANSFORM_T) { // the exchange: lane j writes dword k of its row to [k][j], reads line j / 2 and keeps its half
        uint32_t image[4][8];
        for (uint32_t j = 0; j < 8; j++)
          for (uint32_t k = 0; k < 4; k++) memcpy(&image[k][j], &rows[j][2 * k], 4);
        for (uint32_t j = 0; j < 8; j++)
          for (uint32_t u = 0; u < 8; u++) rows[j][u] = (int16_t)(uint16_t)(image[j >> 1][u] >> ((j & 1) * 16));
      }
      for (uint32_t row = 0; row < 8; row++) {
        int16_t out[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        bool beyond = false;
        if (has) finish_row(p, c, bits, row, rows[row], out, beyond);
        memcpy(p.dst + p.dst_off[c] + (int64_t)((uint64_t)blk * 64 + row * 8), out, sizeof(out));
        if (beyond) a.flags[pic] = 1;
      }
    }
  }
}

static bool same_layout(const EncodePassLayout &a, const EncodePassLayout &b)
{
  bool same = a.n == b.n && a.N == b.N && a.I == b.I && a.coef_total == b.coef_total && a.n_own == b.n_own && a.fargs_at == b.fargs_at && a.hargs_at == b.hargs_at &&
              a.first_block_at == b.first_block_at && a.first_interval_at == b.first_interval_at && a.std_tables_at == b.std_tables_at && a.planes_at == b.planes_at &&
              a.up_bytes == b.up_bytes && a.d_first_chunk == b.d_first_chunk && a.d_tables == b.d_tables && a.d_hist == b.d_hist && a.d_gather == b.d_gather &&
              a.coder_at == b.coder_at && a.coef_at == b.coef_at && a.dev_bytes == b.dev_bytes && a.h_first_chunk == b.h_first_chunk && a.h_tables == b.h_tables &&
              a.h_hist == b.h_hist && a.h_istart == b.h_istart && a.h_ffstart == b.h_ffstart && a.host_bytes == b.host_bytes && a.rq_pics_at == b.rq_pics_at &&
              a.rq_first_at == b.rq_first_at && a.rq_item_at == b.rq_item_at && a.rq_flags_at == b.rq_flags_at && a.h_flags == b.h_flags && a.requant.first == b.requant.first &&
              a.requant.item == b.requant.item;
  for (int l = 0; l < FORWARD_RAGGED_LISTS; l++) same = same && a.wl_first_at[l] == b.wl_first_at[l] && a.wl_item_at[l] == b.wl_item_at[l];
  return same;
}

static int run_list(const char *name, const std::vector<Decoded> &list, int optimize, uint32_t pass_blocks, int want_passes)
{
  list_name = name;
  const int n = (int)list.size();
  std::vector<mijpeg_info> infos;
  std::vector<std::unique_ptr<int16_t[]>> stores; // every source: exactly its frame's coefficients
  std::vector<mijpeg_encode_frame> frames;
  std::vector<mijpeg_encode_ragged_item> items;
  std::vector<RequantSource> sources, plain_sources;
  mijpeg_encode_ragged_totals totals;
  memset(&totals, 0, sizeof(totals));
  PassCutter cut{pass_blocks ? pass_blocks : PASS_BLOCKS_DEFAULT};
  bool any = false;
  for (int i = 0; i < n; i++) {
    const Decoded &s = list[(size_t)i];
    infos.push_back(decoded_info(s));
    const mijpeg_info &f = infos.back();
    stores.emplace_back(new int16_t[(size_t)f.coef_count]);
    const RequantRange r = requant_range(f.precision);
    for (int64_t k = 0; k < f.coef_count; k++) // (inside the coding range; one picture in five carries a value outside it)
      stores.back()[(size_t)k] = (k & 63) ? (int16_t)((int)(rnd() % (2u * (uint32_t)r.ac_max + 1)) - r.ac_max) : (int16_t)((int)(rnd() % (2u * (uint32_t)r.dc_max + 2)) + r.dc_min);
    if (i % 5 == 2) stores.back()[65] = (int16_t)(r.ac_max + 1);
    mijpeg_encode_ragged_item it;
    memset(&it, 0, sizeof(it));
    int ri = -1;
    bool keeps = false;
    TransformPlan how;
    const mijpeg_transcode_spec spec{s.spec_quality, s.spec_ri};
    CHECK(transform_in_order(s.transform));
    CHECK(transcode_plan_one(f, spec, it.info, ri, keeps, it.blocks, it.intervals, s.transform, &how) == MIJPEG_OK);
    CHECK(how.bits == transform_bits(s.transform) && !how.geometry && keeps == (s.spec_quality == 0));
    const bool T = how.bits & TRANSFORM_T;
    CHECK(it.info.width <= (T ? f.height : f.width) && it.info.height <= (T ? f.width : f.height) && how.trimmed == (it.info.width != (T ? f.height : f.width) || it.info.height != (T ? f.width : f.height)));
    if (how.bits & TRANSFORM_MH) CHECK(it.info.width == it.info.mcus_x * 8 * (f.components == 1 ? 1 : it.info.hsamp[0]));
    if (how.bits & TRANSFORM_MV) CHECK(it.info.height == it.info.mcus_y * 8 * (f.components == 1 ? 1 : it.info.vsamp[0]));
    for (int c = 0; c < f.components; c++) {
      CHECK(it.info.hsamp[c] == (f.components == 1 ? 1 : T ? f.vsamp[c] : f.hsamp[c]) && it.info.vsamp[c] == (f.components == 1 ? 1 : T ? f.hsamp[c] : f.vsamp[c]));
      uint16_t want[64];
      transform_table(how.bits, f.quant[f.quant_index[c]], want);
      if (keeps) CHECK(memcmp(it.info.quant[it.info.quant_index[c]], want, 128) == 0);
    }
    if (!s.transform) { // the old signature plans the same frame
      mijpeg_info old;
      int ri2 = -1;
      bool keeps2 = false;
      uint32_t b2 = 0, i2 = 0;
      CHECK(transcode_plan_one(f, spec, old, ri2, keeps2, b2, i2) == MIJPEG_OK && memcmp(&old, &it.info, sizeof(old)) == 0 && ri2 == ri && b2 == it.blocks && i2 == it.intervals);
    }
    mijpeg_encode_frame e;
    memset(&e, 0, sizeof(e));
    e.width = it.info.width; e.height = it.info.height; e.components = it.info.components;
    for (int c = 0; c < 4; c++) { e.hsamp[c] = it.info.hsamp[c]; e.vsamp[c] = it.info.vsamp[c]; }
    e.restart_interval = ri;
    cut.place(it, &totals);
    frames.push_back(e);
    items.push_back(it);
    sources.push_back(RequantSource{f, stores.back().get(), how.bits});
    plain_sources.push_back(RequantSource{f, stores.back().get()});
    any = any || how.bits;
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
    uint32_t transformed = 0;
    for (uint32_t p = 0; p < m; p++) transformed += sources[(size_t)p0 + p].transform != 0;
    if (!any) { // a list without transforms: what the old signatures lay out, offset for offset, and no region of the new ones
      const EncodePassLayout old(frames.data(), items.data(), p0, p1, optimize, nullptr, plain_sources.data());
      CHECK(same_layout(L, old));
    }
    if (!transformed) CHECK(L.transform.item.empty() && L.transform.first.empty() && L.tf_first_at == L.up_bytes && L.tf_item_at == L.up_bytes && L.tf_bits_at == L.up_bytes);
    else CHECK(L.tf_first_at >= L.rq_flags_at + m * 4 && L.tf_item_at >= L.tf_first_at + L.transform.first.size() * 4 && L.tf_bits_at >= L.tf_item_at + L.transform.item.size() * 4 &&
               L.up_bytes >= L.tf_bits_at + m * 4 && L.tf_first_at % 256 == 0 && L.tf_item_at % 256 == 0 && L.tf_bits_at % 256 == 0);
    CHECK(L.up_bytes % 256 == 0 && L.d_first_chunk >= L.up_bytes && L.h_first_chunk >= L.up_bytes && L.coef_at + (size_t)L.coef_total * 2 <= L.dev_bytes);
    uint8_t *dev = (uint8_t *)aligned_alloc(256, L.dev_bytes), *host = (uint8_t *)malloc(L.host_bytes);
    if (!dev || !host) exit(2);
    memset(host, 0xA5, L.host_bytes);
    memset(dev + L.coef_at, 0x5A, (size_t)L.coef_total * 2);
    EncTables std_tabs;
    enc_standard_tables(std_tabs);
    const EncodePassArgs a = fill_upload(host, dev, L, std_tabs);
    for (size_t i = L.up_bytes; i < L.host_bytes; i++)
      if (host[i] != 0xA5) { CHECK(!"fill_upload wrote behind the uploaded part"); break; }
    memcpy(dev, host, L.up_bytes); // (the one upload)
    // both lists between them hold every component of every picture once, each picture in the list of its kind
    CHECK((a.requant_grid != 0) == (transformed < m) && (a.transform_grid != 0) == (transformed > 0));
    CHECK(a.requant.items + a.transform.list.items == L.requant.item.size() + L.transform.item.size());
    if (transformed) {
      CHECK((const uint8_t *)a.transform.list.pics == dev + L.rq_pics_at && (uint8_t *)a.transform.list.flags == dev + L.rq_flags_at);
      CHECK((const uint8_t *)a.transform.list.first_wg == dev + L.tf_first_at && (const uint8_t *)a.transform.list.item == dev + L.tf_item_at && (const uint8_t *)a.transform.bits == dev + L.tf_bits_at);
      CHECK(a.transform_grid == a.transform.list.first_wg[a.transform.list.items] && a.transform.list.first_wg[0] == 0);
      for (uint32_t p = 0; p < m; p++) CHECK(a.transform.bits[p] == sources[(size_t)p0 + p].transform);
    }
    uint32_t in_requant = 0, in_transform = 0;
    for (uint32_t p = 0; p < m; p++) {
      const mijpeg_encode_ragged_item &it = items[(size_t)p0 + p];
      const bool tf = sources[(size_t)p0 + p].transform != 0;
      const RequantArgs &l = tf ? a.transform.list : a.requant;
      uint32_t &at = tf ? in_transform : in_requant;
      const RequantPicture &q = a.requant.pics ? a.requant.pics[p] : a.transform.list.pics[p];
      CHECK(q.dst == (int16_t *)(dev + L.coef_at) + it.coef_base && q.src == sources[(size_t)p0 + p].planes && (uintptr_t)&q.t[0] % 16 == 0 && q.ncomp == it.info.components);
      for (int c = 0; c < it.info.components; c++, at++) {
        CHECK(at < l.items && l.item[at] == p * 4 + (uint32_t)c);
        CHECK(l.first_wg[at + 1] - l.first_wg[at] == ((uint32_t)(q.dst_bw[c] * q.dst_bh[c]) + REQUANT_WG_BLOCKS - 1) / REQUANT_WG_BLOCKS);
        CHECK(q.dst_off[c] + (int64_t)q.dst_bw[c] * q.dst_bh[c] * 64 <= it.info.coef_count);
      }
    }
    CHECK(in_requant == a.requant.items && in_transform == a.transform.list.items);
    walk_work_list(a.requant, nullptr, a.requant_grid, m);
    walk_work_list(a.transform.list, a.transform.bits, a.transform_grid, m);
    // what arrived: every component by the rule over planes in host memory
    for (uint32_t p = 0; p < m; p++) {
      const mijpeg_info &f = infos[(size_t)p0 + p], &o = items[(size_t)p0 + p].info;
      const int16_t *src = sources[(size_t)p0 + p].planes, *dst = (const int16_t *)(dev + L.coef_at) + items[(size_t)p0 + p].coef_base;
      int64_t clamped = 0;
      for (int c = 0; c < o.components; c++) {
        const size_t count = (size_t)o.blocks_w[c] * o.blocks_h[c] * 64;
        std::unique_ptr<int16_t[]> want(new int16_t[count]);
        clamped += transform_blocks(src + f.coef_offset[c], f.blocks_w[c], f.blocks_h[c], want.get(), o.blocks_w[c], o.blocks_h[c], sources[(size_t)p0 + p].transform,
                                    f.quant[f.quant_index[c]], o.quant[o.quant_index[c]], o.precision);
        CHECK(memcmp(want.get(), dst + o.coef_offset[c], count * 2) == 0);
      }
      CHECK((((const uint32_t *)(dev + L.rq_flags_at))[p] != 0) == (clamped != 0));
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
  // the rule's pieces: every code's bits, the source block of every destination block, the signs
  list_name = "rule";
  const uint32_t want_bits[8] = {0, 2, 4, 1, 7, 3, 6, 5};
  for (int code = 0; code < 8; code++) {
    CHECK(transform_bits(code) == want_bits[code] && transform_bits(code | MIJPEG_TRANSFORM_TRIM) == want_bits[code] && transform_in_order(code) && transform_in_order(code | MIJPEG_TRANSFORM_TRIM));
    const uint32_t bits = transform_bits(code), dbw = 5, dbh = 3;
    bool seen[5][5] = {};
    for (uint32_t by = 0; by < dbh; by++)
      for (uint32_t bx = 0; bx < dbw; bx++) {
        uint32_t sx, sy;
        transform_source_block(bits, bx, by, dbw, dbh, sx, sy);
        CHECK(sx < (bits & 1 ? dbh : dbw) && sy < (bits & 1 ? dbw : dbh) && !seen[sy][sx]);
        seen[sy][sx] = true;
      }
    for (uint32_t v = 0; v < 8; v++)
      for (uint32_t u = 0; u < 8; u++) CHECK(transform_negates(bits, u, v) == ((((bits & 2) && (u & 1)) ? 1 : 0) != (((bits & 4) && (v & 1)) ? 1 : 0)));
  }
  CHECK(!transform_in_order(8) && !transform_in_order(-1) && !transform_in_order(0x200) && !transform_in_order(8 | MIJPEG_TRANSFORM_TRIM));
  const int TRIM = MIJPEG_TRANSFORM_TRIM;
  // group members and children of both precisions, every transform, kept (quality 0) and requantised, whole MCUs and trimmed ones;
  // 72 x 56 4:4:4 is 63 blocks a component: a workgroup's ragged end
  const std::vector<Decoded> mixed = {
      {48, 32, 3, 2, 2, 8, 75, 0, false, 0, -1, 5},        {32, 16, 3, 2, 1, 8, 90, 5, false, 50, 0, 3},       {72, 56, 3, 1, 1, 8, 60, 0, false, 0, 1, 7},
      {8, 24, 1, 1, 1, 8, 30, 0, false, 0, -1, 4},         {50, 35, 3, 2, 2, 8, 85, 0, false, 0, -1, 5 | TRIM}, {32, 32, 3, 2, 2, 12, 75, 3, false, 0, -1, 6},
      {64, 48, 3, 1, 1, 12, 2, 0, false, 30, 7, 0},        {96, 64, 3, 1, 2, 8, 75, 0, true, 75, -1, 1},        {97, 61, 3, 4, 1, 8, 75, 0, false, 0, 2, 3},
      {23, 50, 1, 2, 1, 8, 50, 0, false, 0, -1, 2 | TRIM}, {136, 136, 3, 2, 2, 8, 75, 8, true, 0, -1, 0},       {33, 7, 1, 1, 1, 12, 75, 0, true, 2, 0, 1 | TRIM},
      {50, 35, 3, 2, 2, 8, 85, 0, false, 95, -1, 4 | TRIM}, {131, 77, 3, 2, 1, 8, 75, 0, false, 0, -1, 3},      {40, 24, 3, 2, 1, 8, 75, 0, false, 50, -1, 6 | TRIM}};
  int passes = run_list("mixed", mixed, 0, 0, 1);
  passes += run_list("mixed, own tables", mixed, 1, 0, 1);
  std::vector<Decoded> all = mixed, none = mixed;
  for (Decoded &s : all) if (!s.transform) s.transform = 5 | TRIM; // (no picture is left for the requant launch)
  for (Decoded &s : none) s.transform = 0;
  passes += run_list("all transformed", all, 0, 0, 1);
  passes += run_list("none transformed", none, 0, 0, 1);
  passes += run_list("none transformed, own tables", none, 1, 0, 1);
  passes += run_list("cut", mixed, 0, 1024, 5);
  // the geometry's refusals, behind the existing ones
  list_name = "refusals";
  {
    mijpeg_info f = decoded_info(Decoded{50, 35, 3, 2, 2, 8, 75, 0, false, 0, -1, 0}), out;
    int ri;
    bool keeps;
    uint32_t b, iv;
    TransformPlan how;
    const mijpeg_transcode_spec keep{0, -1}, q50{50, -1};
    CHECK(transcode_plan_one(f, keep, out, ri, keeps, b, iv, MIJPEG_TRANSFORM_FLIP_H, &how) == MIJPEG_ERR_NOT_AVAILABLE && how.geometry && out.width == 0);
    CHECK(transcode_plan_one(f, q50, out, ri, keeps, b, iv, MIJPEG_TRANSFORM_ROT_90, &how) == MIJPEG_ERR_NOT_AVAILABLE && how.geometry);
    CHECK(transcode_plan_one(f, keep, out, ri, keeps, b, iv, MIJPEG_TRANSFORM_TRANSPOSE, &how) == MIJPEG_OK && !how.geometry && !how.trimmed && out.width == 35 && out.height == 50);
    CHECK(transcode_plan_one(f, keep, out, ri, keeps, b, iv, MIJPEG_TRANSFORM_ROT_90 | TRIM, &how) == MIJPEG_OK && how.trimmed && out.width == 32 && out.height == 50);
    mijpeg_info x = f; x.xt = 1;
    CHECK(transcode_plan_one(x, keep, out, ri, keeps, b, iv, MIJPEG_TRANSFORM_FLIP_H, &how) == MIJPEG_ERR_NOT_IMPLEMENTED && out.width == 0);
    x = f; x.quant[0][5] = 0;
    CHECK(transcode_plan_one(x, q50, out, ri, keeps, b, iv, MIJPEG_TRANSFORM_FLIP_H, &how) == MIJPEG_ERR_NOT_IMPLEMENTED);
    x = decoded_info(Decoded{15, 40, 3, 2, 2, 8, 75, 0, false, 0, -1, 0});
    CHECK(transcode_plan_one(x, keep, out, ri, keeps, b, iv, MIJPEG_TRANSFORM_FLIP_H | TRIM, &how) == MIJPEG_ERR_NOT_AVAILABLE && how.geometry);
  }
  if (failures) return 1;
  printf("OK %d passes of 6 lists\n", passes);
  return 0;
}
