// encode_list_tables.cpp -- the host half of the ragged encode (libjpeg_amd/csrc/encode_list.hpp) as a program of its own, for the
// sanitizers: lists of picture descriptions go through the real planner, every pass through the real layout and fill, into heap
// buffers of exactly up_bytes and host_bytes; the device arena is an address range of dev_bytes that nobody dereferences.  Every
// region, pointer, prefix table and work list is read back, the plain buffer is laid out from made-up sizes, and every picture's
// piece is cut out of a fake output arena built the way hencode.hpp describes it.  No device; of the library only encoder.cpp.
// (tests/test_ragged_twin_cpu.py builds it with -fsanitize=address,undefined and runs it.)
#include <stdio.h>
#include <stdlib.h>

#include <functional>

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
#define CHECK(cond)                                                                     \
  do {                                                                                  \
    if (!(cond)) {                                                                      \
      failures++;                                                                       \
      fprintf(stderr, "line %d (%s): %s does not hold\n", __LINE__, list_name, #cond); \
    }                                                                                   \
  } while (0)
static const char *list_name = "";

struct Picture { int w, h, components, hs, vs; };
// list (b): 4:4:4; 4:2:0 of one MCU; 4:2:0 below a tile; exactly one tile; a tile with edge strips; 4:2:2; 1 x 2; grey
static const Picture MIXED[8] = {{8, 8, 3, 1, 1}, {16, 16, 3, 2, 2}, {127, 127, 3, 2, 2}, {128, 128, 3, 2, 2}, {136, 130, 3, 2, 2}, {17, 9, 3, 2, 1}, {9, 17, 3, 1, 2}, {33, 7, 1, 1, 1}};

// a description with pixels at a made-up device address, lines on dword boundaries (what the tile and interior kernels ask for)
static mijpeg_encode_frame frame(const Picture &s, int precision, int restart_interval, int index)
{
  mijpeg_encode_frame e;
  memset(&e, 0, sizeof(e));
  e.width = s.w; e.height = s.h; e.components = s.components;
  for (int c = 0; c < 4; c++) e.hsamp[c] = e.vsamp[c] = 1;
  e.hsamp[0] = s.hs; e.vsamp[0] = s.vs;
  e.quality = 30 + 10 * (index % 7);
  e.restart_interval = restart_interval;
  e.row_stride = ((int64_t)s.w * s.components * (precision == 12 ? 2 : 1) + 3) & ~(int64_t)3;
  e.pixels = (const uint8_t *)((uintptr_t)0x7000000000ull + ((uintptr_t)index << 24));
  return e;
}

struct Region { size_t at, bytes; };
// every region on a 256-byte boundary, in the order it was carved none reaches into the next (empty ones included), none past the arena
static void check_regions(const std::vector<Region> &r, size_t arena)
{
  for (size_t i = 0; i < r.size(); i++) {
    CHECK(r[i].at % 256 == 0);
    CHECK(r[i].at + r[i].bytes <= (i + 1 < r.size() ? r[i + 1].at : arena));
  }
  CHECK(arena % 256 == 0);
}

static uint32_t plain_size_of(uint32_t p) { static const uint32_t s[7] = {1, 63, 64, 65, 5000, 128, 3217}; return s[p % 7]; }
static uint32_t ff_count_of(uint32_t p) { static const uint32_t s[5] = {0, 3, 1, 40, 7}; return s[p % 5]; }

// One pass [p0, p1) of a planned list: layout, fill, own tables, plain buffer, pieces
static void check_pass(const mijpeg_encode_frame *frames, const mijpeg_encode_ragged_item *items, int p0, int p1, int optimize, uint32_t want_own)
{
  const EncodePassLayout L(frames, items, p0, p1, optimize);
  CHECK(L.error == MIJPEG_OK && L.why == nullptr);
  if (L.error) return;
  const uint32_t n = L.n;
  const mijpeg_encode_ragged_item *it = items + p0;
  CHECK(n == (uint32_t)(p1 - p0) && L.items == it && L.frames == frames + p0);
  CHECK(L.N == it[n - 1].first_block + pad256(it[n - 1].blocks) && L.I == it[n - 1].first_interval + it[n - 1].intervals);
  CHECK(L.coef_total == it[n - 1].coef_base + ((it[n - 1].info.coef_count + 127) & ~(int64_t)127));
  CHECK(it[0].first_block == 0 && it[0].first_interval == 0 && it[0].coef_base == 0); // (every pass starts its index spaces again)
  // ---- own_index: compact, in picture order
  CHECK(L.n_own == want_own && L.own_index.size() == n);
  uint32_t own = 0;
  for (uint32_t p = 0; p < n; p++) {
    const bool wants = optimize || it[p].info.precision == 12;
    CHECK(L.own(p) == wants && L.own_index[p] == (wants ? own : UINT32_MAX));
    own += wants;
  }
  CHECK(own == L.n_own && L.hist_bytes == (size_t)own * 4096);
  // ---- regions of the three arenas
  const CoderLayout cl = coder_layout(L.N, L.I);
  CHECK(L.coder.end == cl.end && L.coder.N == L.N && L.coder.I == L.I);
  std::vector<Region> up = {{L.fargs_at, n * sizeof(ForwardArgs)}, {L.hargs_at, n * sizeof(HencArgs)}, {L.first_block_at, (n + 1) * 4}, {L.first_interval_at, (n + 1) * 4}};
  for (int l = 0; l < FORWARD_RAGGED_LISTS; l++) {
    CHECK(L.lists[l].first.size() == (L.lists[l].item.empty() ? 0 : L.lists[l].item.size() + 1));
    up.push_back({L.wl_first_at[l], L.lists[l].first.size() * 4});
    up.push_back({L.wl_item_at[l], L.lists[l].item.size() * 4});
  }
  up.push_back({L.std_tables_at, sizeof(HencTables)});
  CHECK(L.fargs_at == 0);
  check_regions(up, L.up_bytes);
  std::vector<Region> dv = up, hp = up; // (the uploaded part: the same offsets in both arenas, everything else behind it)
  dv.insert(dv.end(), {{L.d_first_chunk, (n + 1) * 4}, {L.d_tables, own * sizeof(HencTables)}, {L.d_hist, own * HENC_HIST_BYTES}, {L.d_gather, (n + 1) * 8},
                       {L.coder_at, cl.end}, {L.coef_at, (size_t)L.coef_total * 2}});
  hp.insert(hp.end(), {{L.h_first_chunk, (n + 1) * 4}, {L.h_tables, own * sizeof(HencTables)}, {L.h_hist, own * HENC_HIST_BYTES}, {L.h_istart, (n + 1) * 8},
                       {L.h_ffstart, (n + 1) * 8}});
  check_regions(dv, L.dev_bytes);
  check_regions(hp, L.host_bytes);
  CHECK(L.d_first_chunk >= L.up_bytes && L.h_first_chunk >= L.up_bytes && L.up_bytes <= L.host_bytes && L.up_bytes <= L.dev_bytes);
  // ---- fill: once into exactly up_bytes, once into the pinned arena's twin; the device arena is addresses only
  uint8_t *dev = (uint8_t *)aligned_alloc(256, L.dev_bytes), *only_up = (uint8_t *)malloc(L.up_bytes), *host = (uint8_t *)malloc(L.host_bytes);
  if (!dev || !only_up || !host) exit(2);
  memset(only_up, 0xA5, L.up_bytes);
  memset(host, 0xA5, L.host_bytes);
  EncTables std_tabs;
  enc_standard_tables(std_tabs);
  (void)fill_upload(only_up, dev, L, std_tabs);
  const EncodePassArgs a = fill_upload(host, dev, L, std_tabs);
  CHECK(memcmp(only_up, host, L.up_bytes) == 0);
  free(only_up);
  for (size_t i = L.up_bytes; i < L.host_bytes; i++)
    if (host[i] != 0xA5) { CHECK(!"fill_upload wrote behind the uploaded part"); break; }
  HencTables std_packed;
  henc_pack_tables(&std_packed, std_tabs);
  CHECK(memcmp(host + L.std_tables_at, &std_packed, sizeof(std_packed)) == 0);
  // (what the device is told lies where the host wrote it: same offsets)
  CHECK((const uint8_t *)a.coder.pics == dev + L.hargs_at && (const uint8_t *)a.coder.first_block == dev + L.first_block_at);
  CHECK((const uint8_t *)a.coder.first_interval == dev + L.first_interval_at && (const uint8_t *)a.coder.first_chunk == dev + L.d_first_chunk);
  CHECK(a.coder.n == n && a.coder.total_blocks == L.N && a.coder.total_intervals == L.I && a.coder.total_chunks == 0 && !a.coder.out && !a.coder.plain);
  // ---- ForwardArgs, HencArgs, prefix tables
  const ForwardArgs *hf = (const ForwardArgs *)(host + L.fargs_at);
  HencArgs *hh = (HencArgs *)(host + L.hargs_at);
  const uint32_t *first_block = (const uint32_t *)(host + L.first_block_at), *first_interval = (const uint32_t *)(host + L.first_interval_at);
  uint8_t *coder = dev + L.coder_at;
  const int16_t *coef = (const int16_t *)(dev + L.coef_at);
  for (uint32_t p = 0; p < n; p++) {
    const mijpeg_info &f = it[p].info;
    const HencArgs &h = hh[p];
    CHECK(h.bits == (uint32_t *)(coder + cl.bits) + it[p].first_block && h.bitpos == (const uint64_t *)(coder + cl.bitpos) + it[p].first_block);
    CHECK(h.ibytes == (uint32_t *)(coder + cl.ibytes) + it[p].first_interval && h.istart == (const uint64_t *)(coder + cl.istart) + it[p].first_interval);
    CHECK((const uint8_t *)(h.bits + pad256(it[p].blocks)) <= coder + cl.bitpos && (const uint8_t *)(h.istart + it[p].intervals + 1) <= coder + cl.scratch);
    CHECK(h.coef == coef + it[p].coef_base && (uintptr_t)h.coef % 256 == 0 && (const uint8_t *)(h.coef + f.coef_count) <= dev + L.dev_bytes);
    CHECK(hf[p].coef == h.coef && hf[p].pixels == frames[p0 + p].pixels && hf[p].pixel_row_stride == frames[p0 + p].row_stride && hf[p].frames == 1);
    CHECK(hf[p].width == f.width && hf[p].height == f.height && hf[p].ncomp == f.components && hf[p].coef_frame_stride == f.coef_count);
    CHECK((h.hist == nullptr) == !L.own(p));
    if (L.own(p)) CHECK(h.hist == (uint32_t *)(dev + L.d_hist) + (size_t)L.own_index[p] * 1024 && (const uint8_t *)(h.hist + 1024) <= dev + L.d_gather);
    CHECK((const uint8_t *)h.tables == dev + L.std_tables_at);
    CHECK(h.total_blocks == it[p].blocks && h.n_intervals == it[p].intervals && h.ncomp == f.components && h.mcus_x == f.mcus_x);
    CHECK((uint32_t)h.total_mcus * (uint32_t)h.blocks_per_mcu == it[p].blocks && h.ri == (frames[p0 + p].restart_interval ? frames[p0 + p].restart_interval : h.total_mcus));
    CHECK(!h.plain && !h.ffcount && !h.ffstart && !h.out && h.plain_bytes == 0);
    CHECK(first_block[p] == it[p].first_block && first_block[p] % 256 == 0 && first_interval[p] == it[p].first_interval);
    CHECK(first_block[p + 1] >= first_block[p] + it[p].blocks && first_interval[p + 1] == first_interval[p] + it[p].intervals); // (n + 1 entries)
  }
  CHECK(first_block[n] == L.N && L.N % 256 == 0 && first_interval[n] == L.I);
  // ---- work lists, read from where the launches will read them
  std::vector<int> in_block_list(n, 0);
  for (int l = 0; l < FORWARD_RAGGED_LISTS; l++) {
    const ForwardRaggedArgs &r = a.forward.launch[l];
    CHECK(r.items == L.lists[l].item.size());
    if (!r.items) { CHECK(a.forward.grid[l] == 0 && !r.pics && !r.first_wg && !r.item); continue; }
    CHECK((const uint8_t *)r.pics == dev + L.fargs_at && (const uint8_t *)r.first_wg == dev + L.wl_first_at[l] && (const uint8_t *)r.item == dev + L.wl_item_at[l]);
    const uint32_t *first = (const uint32_t *)(host + ((const uint8_t *)r.first_wg - dev)), *item = (const uint32_t *)(host + ((const uint8_t *)r.item - dev));
    CHECK(first[0] == 0 && a.forward.grid[l] == first[r.items] && a.forward.grid[l] <= 0x7fffffffu);
    for (uint32_t k = 0; k < r.items; k++) {
      const uint32_t p = item[k] >> 2, comp = item[k] & 3;
      CHECK(first[k + 1] > first[k] && p < n && (k == 0 || item[k] > item[k - 1]));
      if (p >= n) continue;
      CHECK((int)comp < it[p].info.components && (it[p].info.precision == 12) == (l >= FORWARD_RAGGED_LAUNCHES));
      const int family = l % FORWARD_RAGGED_LAUNCHES;
      if (family == 0) CHECK(comp == 0 && hf[p].tiled420 && first[k + 1] - first[k] == (uint32_t)((hf[p].width >> 7) * (hf[p].height >> 7)));
      if (family == 5) { CHECK(comp == 0 && first[k + 1] - first[k] == (hf[p].first_block[hf[p].ncomp] + 255) / 256); in_block_list[p]++; }
      if (family >= 1 && family <= 4) CHECK(hf[p].fast[comp] && first[k + 1] - first[k] == ((uint32_t)(hf[p].fast_nbx[comp] * hf[p].fast_nby[comp]) + 255) / 256);
    }
  }
  for (uint32_t p = 0; p < n; p++) {
    CHECK(in_block_list[p] == 1); // (the per-block kernel takes every picture once)
    CHECK(hf[p].tiled420 == (it[p].info.components == 3 && it[p].info.hsamp[0] == 2 && it[p].info.vsamp[0] == 2 && it[p].info.width >= 128 && it[p].info.height >= 128));
  }
  // ---- own tables: made-up statistics in the pinned arena (a grey picture's second pair stays empty)
  std::vector<EncTables> tabs;
  if (own) {
    uint32_t(*hist)[256] = (uint32_t(*)[256])(host + L.h_hist);
    memset(hist, 0, L.hist_bytes);
    for (uint32_t p = 0; p < n; p++) {
      if (!L.own(p)) continue;
      uint32_t(*x)[256] = hist + (size_t)L.own_index[p] * 4;
      for (int t = 0; t < (it[p].info.components > 1 ? 2 : 1); t++) {
        for (int i = 0; i <= (it[p].info.precision == 12 ? 15 : 11); i++) x[t][i] = 1 + (uint32_t)((i * 7 + p + t) % 13);
        for (int i = 0; i < 256; i++) x[2 + t][i] = (i & 15) >= 1 && (i & 15) <= 10 && (i >> 4) < 4 ? 1 + (uint32_t)((i + 3 * p + t) % 29) : 0;
        x[2 + t][0] = 50 + p; // EOB
      }
    }
  }
  own_tables(host, dev, L, tabs);
  CHECK(tabs.size() == own);
  for (uint32_t p = 0; p < n; p++) {
    if (!L.own(p)) { CHECK((const uint8_t *)hh[p].tables == dev + L.std_tables_at); continue; }
    const uint32_t o = L.own_index[p];
    CHECK(hh[p].tables == (const HencTables *)(dev + L.d_tables) + o && (const uint8_t *)(hh[p].tables + 1) <= dev + L.d_hist);
    HencTables packed;
    henc_pack_tables(&packed, tabs[o]);
    const HencTables *up_tab = (const HencTables *)(host + L.h_tables) + o;
    CHECK(memcmp(up_tab, &packed, sizeof(packed)) == 0);
    CHECK(up_tab->dc_len[0][it[p].info.precision == 12 ? 15 : 11] > 0 && up_tab->ac_len[0][0] > 0 && up_tab->ac_len[0][0x3a] > 0 && up_tab->ac_len[0][0x4a] == 0);
    if (it[p].info.components == 1) CHECK(memcmp(up_tab->ac_len[1], std_packed.ac_len[1], 256) == 0 && memcmp(up_tab->dc_code[1], std_packed.dc_code[1], 32) == 0);
    else CHECK(up_tab->dc_len[1][0] > 0 && up_tab->ac_len[1][0x3a] > 0 && up_tab->ac_len[1][0x4a] == 0);
  }
  // ---- the plain buffer from made-up plain sizes
  uint64_t *istart = (uint64_t *)(host + L.h_istart), *ffs = (uint64_t *)(host + L.h_ffstart);
  istart[0] = ffs[0] = 0;
  for (uint32_t p = 0; p < n; p++) {
    istart[p + 1] = istart[p] + plain_size_of(p);
    ffs[p + 1] = ffs[p] + ff_count_of(p);
  }
  CHECK(chunk_layout(host, L));
  const uint32_t *first_chunk = (const uint32_t *)(host + L.h_first_chunk);
  CHECK(first_chunk[0] == 0 && chunks_of(host, L) == first_chunk[n]);
  for (uint32_t p = 0; p < n; p++) CHECK(first_chunk[p + 1] - first_chunk[p] == (plain_size_of(p) + 63) / 64 && first_chunk[p + 1] > first_chunk[p]);
  // ---- pieces: `out` as the comment on HencBatchArgs lays it out, built without the layout's formulas -- the plain layout with
  // the stuffing bytes and markers of everything in front added
  const size_t arena = arena_bytes(host, L);
  uint8_t *out = (uint8_t *)calloc(arena ? arena : 1, 1);
  if (!out) exit(2);
  size_t added = 0, last_end = 0; // stuffing bytes and marker bytes of the pictures in front
  std::vector<size_t> begin(n), length(n);
  for (uint32_t p = 0; p < n; p++) {
    begin[p] = (size_t)first_chunk[p] * 64 + added;
    length[p] = plain_size_of(p) + ff_count_of(p) + 2 * ((size_t)it[p].intervals - 1);
    CHECK(begin[p] + length[p] <= arena);
    if (begin[p] + length[p] > arena) continue;
    memset(out + begin[p], (int)(p % 200) + 1, length[p]);
    for (uint32_t k = 0; k + 1 < it[p].intervals; k++) { // (two marker bytes per boundary; where in the piece does not matter here)
      out[begin[p] + length[p] - 2 * k - 2] = 0xff;
      out[begin[p] + length[p] - 2 * k - 1] = (uint8_t)(0xd0 + (k & 7));
    }
    added += ff_count_of(p) + 2 * ((size_t)it[p].intervals - 1);
  }
  CHECK((size_t)first_chunk[n] * 64 + added == arena);
  for (uint32_t p = 0; p < n; p++) {
    const StreamPiece piece = stream_piece(host, L, p);
    CHECK(piece.at == begin[p] && piece.ecs == length[p] && piece.at >= last_end && piece.at + piece.ecs <= arena);
    if (piece.at + piece.ecs > arena) continue;
    size_t mine = 0, markers = 0;
    for (size_t i = 0; i < piece.ecs; i++) {
      mine += out[piece.at + i] == (uint8_t)(p % 200 + 1);
      markers += out[piece.at + i] == 0xff || (out[piece.at + i] & 0xf8) == 0xd0;
    }
    CHECK(mine == (size_t)plain_size_of(p) + ff_count_of(p) && markers == 2 * ((size_t)it[p].intervals - 1));
    if (piece.at > last_end) CHECK(out[piece.at - 1] == 0 && out[last_end] == 0); // (chunk padding: nobody's)
    last_end = piece.at + piece.ecs;
  }
  CHECK(last_end <= arena);
  // ---- a plain stream of 2^30 chunks is refused
  istart[n] = istart[n - 1] + ((uint64_t)PASS_BLOCKS_MAX - first_chunk[n - 1]) * 64;
  CHECK(!chunk_layout(host, L));
  istart[n] -= 64;
  CHECK(chunk_layout(host, L) && chunks_of(host, L) == PASS_BLOCKS_MAX - 1);
  free(out);
  free(host);
  free(dev);
}

// plan, cut into passes, check every pass; want_own: pictures with tables of their own per pass
static int run_list(const char *name, const std::vector<mijpeg_encode_frame> &frames, const std::vector<int32_t> &precision, int optimize, uint32_t pass_blocks,
                    const std::vector<uint32_t> &want_own)
{
  list_name = name;
  const int n = (int)frames.size();
  std::vector<mijpeg_encode_ragged_item> items((size_t)n);
  mijpeg_encode_ragged_totals totals;
  CHECK(plan_list(frames.data(), precision.empty() ? nullptr : precision.data(), n, pass_blocks, items.data(), &totals) == MIJPEG_OK);
  CHECK(totals.passes == (int)want_own.size());
  if (failures) return 0;
  int passes = 0;
  for (int p0 = 0; p0 < n;) {
    int p1 = p0 + 1;
    while (p1 < n && items[(size_t)p1].pass == items[(size_t)p0].pass) p1++;
    check_pass(frames.data(), items.data(), p0, p1, optimize, want_own[(size_t)passes]);
    passes++;
    p0 = p1;
  }
  CHECK(passes == totals.passes);
  return passes;
}

static std::vector<mijpeg_encode_frame> mixed_list(const std::vector<int32_t> &precision, bool restarts, int count = 8)
{
  std::vector<mijpeg_encode_frame> frames;
  for (int i = 0; i < count; i++) frames.push_back(frame(MIXED[i % 8], precision.empty() ? 8 : precision[(size_t)i], restarts && (i & 1) ? 1 : 0, i));
  return frames;
}

int main()
{
  int passes = 0;
  // (a) one 1 x 1 grey picture alone
  passes += run_list("a", {frame(Picture{1, 1, 1, 1, 1}, 8, 0, 0)}, {}, 0, 0, {0});
  // (b) the mixed list; (c) with a restart interval of one MCU on every second picture: intervals outnumber the pictures by far
  passes += run_list("b", mixed_list({}, false), {}, 0, 0, {0});
  passes += run_list("c", mixed_list({}, true), {}, 0, 0, {0});
  {
    list_name = "c";
    const std::vector<mijpeg_encode_frame> frames = mixed_list({}, true);
    std::vector<mijpeg_encode_ragged_item> items(8);
    mijpeg_encode_ragged_totals totals;
    CHECK(plan_list(frames.data(), nullptr, 8, 0, items.data(), &totals) == MIJPEG_OK && totals.intervals == 4 + 1 + 64 + 4 + 5 && totals.intervals > 8 * 8);
  }
  // (d) precisions alternate: only the 12-bit pictures have tables of their own
  const std::vector<int32_t> alternating = {8, 12, 8, 12, 8, 12, 8, 12};
  passes += run_list("d", mixed_list(alternating, false), alternating, 0, 0, {4});
  // (e) all 8-bit: every picture with `optimize`, none without (b: empty table and histogram arenas)
  passes += run_list("e", mixed_list({}, false), {}, 1, 0, {8});
  // (f) twelve pictures cut into three passes
  const std::vector<int32_t> twelve = {8, 12, 8, 12, 8, 12, 8, 12, 8, 12, 8, 12};
  passes += run_list("f", mixed_list(twelve, true, 12), twelve, 0, 1536, {2, 2, 2});
  // ---- the work-list appender at the grid's limit, with made-up counts
  list_name = "appender";
  ForwardWorkList w;
  CHECK(work_list_append(w, 0, 0x7ffffff0u) && work_list_append(w, 5, 0xf) && w.first.back() == 0x7fffffffu);
  CHECK(!work_list_append(w, 6, 1) && w.first.size() == 3 && w.item == std::vector<uint32_t>({0, 5}) && w.first[0] == 0 && w.first[1] == 0x7ffffff0u);
  ForwardWorkList big;
  CHECK(!work_list_append(big, 0, 0x80000000ull) && big.item.empty() && work_list_append(big, 0, 0x7fffffffull) && !work_list_append(big, 1, 1));
  if (failures) return 1;
  printf("OK %d passes of 6 lists\n", passes);
  return 0;
}
