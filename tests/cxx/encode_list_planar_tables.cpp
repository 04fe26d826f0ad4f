// encode_list_planar_tables.cpp -- the host half of the ragged encode with PLANAR input (libjpeg_amd/csrc/encode_list.hpp)
// as a program of its own, for the sanitizers: lists whose pictures came as component planes -- every routing: tiles, tiles with
// strips, below a tile, the four interior layouts, 3x factors, planes off their dword boundaries, an odd pitch, grey pictures (their
// own plane) and 12-bit colour pictures (interleaved first: they reach the layout as interleaved pictures) -- go through the real
// planner, every pass through the real layout and fill into heap buffers of exactly up_bytes and host_bytes; the device arena is an
// address range nobody dereferences.  Every plane-table entry, prefix table and work list is read back, and every planar picture's
// work items are compared with those of its interleaved twin, laid out beside it.  No device; of the library only encoder.cpp.
// (tests/test_planar_encode_cpu.py builds it with -fsanitize=address,undefined and runs it.)
#include <stdio.h>
#include <stdlib.h>

#include <functional>
#include <map>

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

// skew: what is added to the address of plane 1 and to the pitch -- 0: the fast condition holds
struct Picture { int w, h, components, hs, vs, precision, plane_skew, pitch_skew; };
static const Picture ROUTINGS[] = {
    {128, 128, 3, 2, 2, 8, 0, 0},  // one tile
    {136, 130, 3, 2, 2, 8, 0, 0},  // a tile with strips
    {127, 127, 3, 2, 2, 8, 0, 0},  // below a tile: interior <1,1> and <2,2>
    {40, 24, 3, 1, 1, 8, 0, 0},    // 4:4:4
    {48, 24, 3, 2, 1, 8, 0, 0},    // 4:2:2
    {48, 24, 3, 1, 2, 8, 0, 0},    // 4:4:0
    {33, 17, 3, 4, 1, 8, 0, 0},    // 4:1:1: the per-block kernel alone
    {136, 130, 3, 2, 2, 8, 1, 0},  // plane 1 at an odd address: the per-block kernel alone
    {136, 130, 3, 2, 2, 8, 2, 0},  // ... two bytes off
    {97, 61, 3, 2, 1, 8, 0, 1},    // an odd pitch
    {33, 7, 1, 1, 1, 8, 0, 0},     // grey: its own plane
    {70, 50, 1, 1, 1, 12, 0, 0},   // grey at 12 bits
    {130, 200, 3, 2, 2, 12, 0, 0}, // 12-bit colour: interleaved first
    {1, 1, 3, 2, 2, 8, 0, 0},
};
constexpr int ROUTING_COUNT = (int)(sizeof(ROUTINGS) / sizeof(ROUTINGS[0]));

static bool planar_picture(const Picture &s) { return s.components == 3 && s.precision == 8; }

// The description a pass is laid out with.  planar: plane 0 in `pixels`, the planes' pitch in `row_stride`, *entry = planes 1 and 2;
// otherwise an interleaved picture with lines on dword boundaries (what a planar picture's twin is, and what the entry point makes
// of a grey or a 12-bit colour picture), *entry = nulls.  Addresses are made up.
static mijpeg_encode_frame frame(const Picture &s, int restart_interval, int index, bool planar, ForwardPlanes *entry)
{
  mijpeg_encode_frame e;
  memset(&e, 0, sizeof(e));
  e.width = s.w; e.height = s.h; e.components = s.components;
  for (int c = 0; c < 4; c++) e.hsamp[c] = e.vsamp[c] = 1;
  e.hsamp[0] = s.hs; e.vsamp[0] = s.vs;
  e.quality = 30 + 10 * (index % 7);
  e.restart_interval = restart_interval;
  const uintptr_t base = (uintptr_t)0x7000000000ull + ((uintptr_t)index << 24);
  e.pixels = (const uint8_t *)base;
  if (planar) {
    e.row_stride = (((int64_t)s.w + 3) & ~(int64_t)3) + s.pitch_skew;
    // planes in reversed memory order, far apart
    *entry = ForwardPlanes{(const uint8_t *)(base - 0x100000 + (uintptr_t)s.plane_skew), (const uint8_t *)(base - 0x200000)};
  } else {
    e.row_stride = ((int64_t)s.w * s.components * (s.precision == 12 ? 2 : 1) + 3) & ~(int64_t)3;
    *entry = ForwardPlanes{nullptr, nullptr};
  }
  return e;
}

// the work items of picture p in the six lists from `first_list` on: (family, component) -> workgroups, read from where the
// launches will read them
typedef std::map<std::pair<int, int>, uint32_t> Items;
static Items items_of(const EncodePassArgs &a, const uint8_t *host, const uint8_t *dev, uint32_t p, int first_list)
{
  Items out;
  for (int family = 0; family < FORWARD_RAGGED_LAUNCHES; family++) {
    const ForwardRaggedArgs &r = a.forward.launch[first_list + family];
    if (!r.items) continue;
    const uint32_t *first = (const uint32_t *)(host + ((const uint8_t *)r.first_wg - dev)), *item = (const uint32_t *)(host + ((const uint8_t *)r.item - dev));
    for (uint32_t k = 0; k < r.items; k++)
      if (item[k] >> 2 == p) {
        CHECK(!out.count({family, (int)(item[k] & 3)}));
        out[{family, (int)(item[k] & 3)}] = first[k + 1] - first[k];
      }
  }
  return out;
}

struct Filled {
  EncodePassArgs a;
  uint8_t *host, *dev;
};
// layout -> fill into exactly up_bytes and into the pinned arena's twin; both must agree, nothing behind the upload is written
static Filled fill(const EncodePassLayout &L)
{
  uint8_t *dev = (uint8_t *)aligned_alloc(256, L.dev_bytes ? L.dev_bytes : 256), *only_up = (uint8_t *)malloc(L.up_bytes), *host = (uint8_t *)malloc(L.host_bytes);
  if (!dev || !only_up || !host) exit(2);
  memset(only_up, 0xA5, L.up_bytes);
  memset(host, 0xA5, L.host_bytes);
  EncTables std_tabs;
  enc_standard_tables(std_tabs);
  (void)fill_upload(only_up, dev, L, std_tabs);
  Filled f{fill_upload(host, dev, L, std_tabs), host, dev};
  CHECK(memcmp(only_up, host, L.up_bytes) == 0);
  free(only_up);
  for (size_t i = L.up_bytes; i < L.host_bytes; i++)
    if (host[i] != 0xA5) { CHECK(!"fill_upload wrote behind the uploaded part"); break; }
  return f;
}

// One pass [p0, p1): the planar layout against the layout of the interleaved twins
static void check_pass(const std::vector<Picture> &pics, const std::vector<mijpeg_encode_frame> &frames, const std::vector<ForwardPlanes> &table,
                       const std::vector<mijpeg_encode_frame> &twins, const mijpeg_encode_ragged_item *items, int p0, int p1, int optimize)
{
  const EncodePassLayout L(frames.data(), items, p0, p1, optimize, table.data()), T(twins.data(), items, p0, p1, optimize);
  CHECK(L.error == MIJPEG_OK && T.error == MIJPEG_OK);
  if (L.error || T.error) return;
  const uint32_t n = L.n;
  uint32_t want_planar = 0, want_own = 0;
  for (uint32_t p = 0; p < n; p++) {
    want_planar += planar_picture(pics[(size_t)p0 + p]);
    want_own += optimize || pics[(size_t)p0 + p].precision == 12;
    CHECK(L.planar(p) == planar_picture(pics[(size_t)p0 + p]) && !T.planar(p));
  }
  CHECK(L.n_planar == want_planar && T.n_planar == 0 && L.n_own == want_own && T.n_own == want_own && L.planes == table.data() + p0 && !T.planes);
  // ---- the plane table: behind the standard tables, the last region of the upload; empty without planar pictures
  CHECK(L.planes_at % 256 == 0 && L.planes_at >= L.std_tables_at + sizeof(HencTables) && L.up_bytes % 256 == 0);
  CHECK(L.planes_at + (want_planar ? (size_t)n * sizeof(ForwardPlanes) : 0) <= L.up_bytes && L.up_bytes - L.planes_at < (want_planar ? (size_t)n * sizeof(ForwardPlanes) : 0) + 256);
  CHECK(T.planes_at == T.up_bytes);
  // (everything in front of it lies where it lies without planes; what follows the upload moves by the table's size alone)
  CHECK(L.fargs_at == T.fargs_at && L.hargs_at == T.hargs_at && L.first_block_at == T.first_block_at && L.first_interval_at == T.first_interval_at);
  CHECK(L.N == T.N && L.I == T.I && L.coef_total == T.coef_total && L.d_first_chunk >= L.up_bytes && L.h_first_chunk >= L.up_bytes);
  CHECK(L.dev_bytes - L.up_bytes == T.dev_bytes - T.up_bytes && L.host_bytes - L.up_bytes == T.host_bytes - T.up_bytes);
  Filled f = fill(L), t = fill(T);
  if (want_planar) {
    CHECK((const uint8_t *)f.a.forward.planes == f.dev + L.planes_at);
    const ForwardPlanes *up = (const ForwardPlanes *)(f.host + L.planes_at);
    for (uint32_t p = 0; p < n; p++) {
      CHECK(up[p].p1 == table[(size_t)p0 + p].p1 && up[p].p2 == table[(size_t)p0 + p].p2);
      CHECK((up[p].p1 != nullptr) == planar_picture(pics[(size_t)p0 + p]) && (up[p].p2 != nullptr) == (up[p].p1 != nullptr));
    }
  } else
    CHECK(f.a.forward.planes == nullptr);
  CHECK(t.a.forward.planes == nullptr);
  // ---- ForwardArgs and prefix tables, read back
  const ForwardArgs *hf = (const ForwardArgs *)(f.host + L.fargs_at), *tf = (const ForwardArgs *)(t.host + T.fargs_at);
  const uint32_t *first_block = (const uint32_t *)(f.host + L.first_block_at), *first_interval = (const uint32_t *)(f.host + L.first_interval_at);
  for (uint32_t p = 0; p < n; p++) {
    const Picture &s = pics[(size_t)p0 + p];
    const mijpeg_encode_frame &e = frames[(size_t)p0 + p];
    CHECK(hf[p].pixels == e.pixels && hf[p].pixel_row_stride == e.row_stride && hf[p].width == s.w && hf[p].height == s.h && hf[p].ncomp == s.components);
    CHECK(hf[p].coef == (int16_t *)(f.dev + L.coef_at) + items[p0 + p].coef_base && (const uint8_t *)(hf[p].coef + items[p0 + p].info.coef_count) <= f.dev + L.dev_bytes);
    CHECK(first_block[p] == items[p0 + p].first_block && first_interval[p] == items[p0 + p].first_interval);
    // the routing: the fast condition of a planar picture is that of its three plane addresses and its pitch
    const bool aligned = s.plane_skew % 4 == 0 && s.pitch_skew % 4 == 0;
    for (int c = 0; c < s.components; c++) {
      if (planar_picture(s)) CHECK(hf[p].fast[c] == (aligned && tf[p].fast[c]));
      else CHECK(hf[p].fast[c] == tf[p].fast[c]);
      CHECK(hf[p].fast_nbx[c] == tf[p].fast_nbx[c] && hf[p].fast_nby[c] == tf[p].fast_nby[c] && hf[p].bw[c] == tf[p].bw[c] && hf[p].coef_off[c] == tf[p].coef_off[c]);
    }
    if (planar_picture(s)) CHECK(hf[p].tiled420 == (aligned && tf[p].tiled420));
    else CHECK(hf[p].tiled420 == tf[p].tiled420);
    CHECK(memcmp(hf[p].invq, tf[p].invq, sizeof(hf[p].invq)) == 0 && memcmp(hf[p].first_block, tf[p].first_block, sizeof(hf[p].first_block)) == 0);
    // the work items: a planar picture's on the planar lists and nowhere else, exactly its twin's; unaligned: the per-block list only
    const Items mine8 = items_of(f.a, f.host, f.dev, p, 0), mine12 = items_of(f.a, f.host, f.dev, p, FORWARD_RAGGED_LAUNCHES),
                mine_planar = items_of(f.a, f.host, f.dev, p, 2 * FORWARD_RAGGED_LAUNCHES);
    const Items twin8 = items_of(t.a, t.host, t.dev, p, 0), twin12 = items_of(t.a, t.host, t.dev, p, FORWARD_RAGGED_LAUNCHES);
    CHECK(items_of(t.a, t.host, t.dev, p, 2 * FORWARD_RAGGED_LAUNCHES).empty());
    if (planar_picture(s)) {
      CHECK(mine8.empty() && mine12.empty() && twin12.empty() && !twin8.empty());
      if (aligned) CHECK(mine_planar == twin8);
      else CHECK(mine_planar.size() == 1 && mine_planar.count({5, 0}) && mine_planar.at({5, 0}) == twin8.at({5, 0}));
      if (s.w >= 128 && s.h >= 128 && s.hs == 2 && s.vs == 2) CHECK(twin8.count({0, 0}) == 1 && twin8.at({0, 0}) == (uint32_t)((s.w >> 7) * (s.h >> 7)));
    } else {
      CHECK(mine_planar.empty() && mine8 == twin8 && mine12 == twin12 && (s.precision == 12 ? mine8.empty() && !mine12.empty() : mine12.empty() && !mine8.empty()));
    }
  }
  CHECK(first_block[n] == L.N && first_interval[n] == L.I);
  // ---- the work lists as such: strictly ascending items, whole workgroups, the grid behind the last
  for (int l = 0; l < FORWARD_RAGGED_LISTS; l++) {
    const ForwardRaggedArgs &r = f.a.forward.launch[l];
    CHECK(r.items == L.lists[l].item.size());
    if (!r.items) { CHECK(f.a.forward.grid[l] == 0 && !r.pics && !r.first_wg && !r.item); continue; }
    CHECK((const uint8_t *)r.pics == f.dev + L.fargs_at && (const uint8_t *)r.first_wg == f.dev + L.wl_first_at[l] && (const uint8_t *)r.item == f.dev + L.wl_item_at[l]);
    CHECK(L.wl_item_at[l] + r.items * 4 <= L.std_tables_at && L.wl_first_at[l] + (r.items + 1) * 4 <= L.wl_item_at[l]);
    const uint32_t *first = (const uint32_t *)(f.host + L.wl_first_at[l]), *item = (const uint32_t *)(f.host + L.wl_item_at[l]);
    CHECK(first[0] == 0 && f.a.forward.grid[l] == first[r.items]);
    for (uint32_t k = 0; k < r.items; k++) {
      CHECK(first[k + 1] > first[k] && (item[k] >> 2) < n && (k == 0 || item[k] > item[k - 1]));
      if ((item[k] >> 2) < n) CHECK(L.planar(item[k] >> 2) == (l >= 2 * FORWARD_RAGGED_LAUNCHES)); // a workgroup never spans flavours
    }
  }
  // ---- own tables with made-up statistics: the slots of the table arena do not move with the plane table in front
  if (want_own) {
    uint32_t(*hist)[256] = (uint32_t(*)[256])(f.host + L.h_hist);
    memset(hist, 0, L.hist_bytes);
    for (uint32_t o = 0; o < want_own; o++)
      for (int tb = 0; tb < 4; tb++)
        for (int i = 0; i < 12; i++) hist[(size_t)o * 4 + tb][tb < 2 ? i : (i == 0 ? 0 : (i % 10) + 1 + 16 * (i / 10))] = 1 + (uint32_t)((i * 5 + o + tb) % 11);
    std::vector<EncTables> tabs;
    own_tables(f.host, f.dev, L, tabs);
    CHECK(tabs.size() == want_own);
    const HencArgs *hh = (const HencArgs *)(f.host + L.hargs_at);
    for (uint32_t p = 0; p < n; p++)
      if (L.own(p)) CHECK(hh[p].tables == (const HencTables *)(f.dev + L.d_tables) + L.own_index[p] && (const uint8_t *)(hh[p].tables + 1) <= f.dev + L.d_hist);
      else CHECK((const uint8_t *)hh[p].tables == f.dev + L.std_tables_at);
  }
  free(f.host); free(f.dev); free(t.host); free(t.dev);
}

// plan, cut into passes, check every pass
static int run_list(const char *name, const std::vector<Picture> &pics, int optimize, uint32_t pass_blocks, int want_passes)
{
  list_name = name;
  const int n = (int)pics.size();
  std::vector<mijpeg_encode_frame> frames, twins;
  std::vector<ForwardPlanes> table((size_t)n), none((size_t)n);
  std::vector<int32_t> precision;
  for (int i = 0; i < n; i++) {
    frames.push_back(frame(pics[(size_t)i], i & 1 ? 1 : 0, i, planar_picture(pics[(size_t)i]), &table[(size_t)i]));
    twins.push_back(frame(pics[(size_t)i], i & 1 ? 1 : 0, i, false, &none[(size_t)i]));
    precision.push_back(pics[(size_t)i].precision);
  }
  std::vector<mijpeg_encode_ragged_item> items((size_t)n);
  mijpeg_encode_ragged_totals totals;
  CHECK(plan_list(frames.data(), precision.data(), n, pass_blocks, items.data(), &totals) == MIJPEG_OK);
  CHECK(want_passes == 1 ? totals.passes == 1 : totals.passes >= want_passes); // (cut lists: at least so many)
  if (failures) return 0;
  int passes = 0;
  for (int p0 = 0; p0 < n;) {
    int p1 = p0 + 1;
    while (p1 < n && items[(size_t)p1].pass == items[(size_t)p0].pass) p1++;
    check_pass(pics, frames, table, twins, items.data(), p0, p1, optimize);
    passes++;
    p0 = p1;
  }
  CHECK(passes == totals.passes);
  return passes;
}

int main()
{
  static_assert(sizeof(ForwardPlanes) == 16, "16-byte entries");
  static_assert(FORWARD_RAGGED_LISTS == 18, "three flavours of six lists");
  int passes = 0;
  const std::vector<Picture> all(ROUTINGS, ROUTINGS + ROUTING_COUNT);
  // (a) every routing in one pass, without and with tables of their own for the 8-bit pictures
  passes += run_list("a", all, 0, 0, 1);
  passes += run_list("b", all, 1, 0, 1);
  // (c) the same list twice over, cut into passes: a pass's plane table starts at its first picture
  std::vector<Picture> twice = all;
  twice.insert(twice.end(), all.begin(), all.end());
  passes += run_list("c", twice, 0, 1536, 3);
  passes += run_list("d", twice, 1, 1536, 3);
  // (e) one planar picture alone; (f) a list without a planar picture (grey and 12-bit colour): no table goes up
  passes += run_list("e", {ROUTINGS[1]}, 0, 0, 1);
  passes += run_list("f", {ROUTINGS[10], ROUTINGS[12], ROUTINGS[11]}, 0, 0, 1);
  // (g) 8-bit planar pictures only: nothing on the interleaved lists
  passes += run_list("g", {ROUTINGS[0], ROUTINGS[3], ROUTINGS[7], ROUTINGS[13]}, 1, 0, 1);
  // ---- the list index of a flavour
  list_name = "lists";
  for (int w = 0; w < FORWARD_RAGGED_LAUNCHES; w++)
    CHECK(forward_ragged_list(w, 8) == w && forward_ragged_list(w, 12) == 6 + w && forward_ragged_list(w, 8, true) == 12 + w && forward_ragged_list(w, 8, false) == w);
  // ---- a planar entry on a picture that has no planar kernel is refused by the layout, not launched
  {
    list_name = "refusal";
    ForwardPlanes entry;
    mijpeg_encode_frame e = frame(ROUTINGS[12], 0, 0, true, &entry);
    const int32_t twelve = 12;
    mijpeg_encode_ragged_item item;
    mijpeg_encode_ragged_totals totals;
    CHECK(plan_list(&e, &twelve, 1, 0, &item, &totals) == MIJPEG_OK);
    const EncodePassLayout L(&e, &item, 0, 1, 0, &entry);
    CHECK(L.error == MIJPEG_ERR_INVALID_PARAMETER && L.why);
  }
  if (failures) return 1;
  printf("OK %d passes of 7 lists\n", passes);
  return 0;
}
