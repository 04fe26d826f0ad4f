// fused_list_tables.cpp -- the host half of the fused list launches (libjpeg_amd/csrc/fused_list.hpp) as a program of its own, for
// the sanitizers: hand-made frame descriptions are grouped into launches, their tables laid out and filled into a heap buffer of
// exactly the layout's size, and every field is read back.  No device, nothing of the library is linked.
// (tests/test_ragged_twin_cpu.py builds it with -fsanitize=address,undefined and runs it.)
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

// A frame description as the parser leaves it: three components with chroma subsampled hs x vs, or one component
static mijpeg_info frame(int w, int h, int components, int hs, int vs, int salt)
{
  mijpeg_info f;
  memset(&f, 0, sizeof(f));
  f.width = w; f.height = h; f.components = components; f.precision = 8; f.ycbcr = 1; f.fast_arith = 1; f.sample_bytes = 1;
  f.mcus_x = (w + 8 * hs - 1) / (8 * hs); f.mcus_y = (h + 8 * vs - 1) / (8 * vs);
  int64_t at = 0;
  for (int c = 0; c < components; c++) {
    f.hsamp[c] = c ? 1 : hs; f.vsamp[c] = c ? 1 : vs;
    f.subx[c] = c ? hs : 1; f.suby[c] = c ? vs : 1;
    f.quant_index[c] = c ? 1 + (c & 1) : 3; // (tables 3, 2, 1: not the identity)
    f.blocks_w[c] = f.mcus_x * f.hsamp[c]; f.blocks_h[c] = f.mcus_y * f.vsamp[c];
    f.coef_offset[c] = at;
    at += (int64_t)f.blocks_w[c] * f.blocks_h[c] * 64;
  }
  f.coef_count = at;
  for (int t = 0; t < 4; t++)
    for (int z = 0; z < 64; z++) f.quant[t][z] = (uint16_t)(1 + salt + 300 * t + z);
  return f;
}

static ReconPlan plan(Recon k, Sampling s, bool fast = true, bool wide = false, bool narrow12 = false)
{
  ReconPlan p{};
  p.kernel = k; p.sampling = s; p.fast = fast; p.wide = wide; p.narrow12 = narrow12;
  return p;
}

// What launch l's tables must hold, field by field, read from host + t
static void check_tables(const uint8_t *host, const FusedListTable &t, const FusedListLaunch &l, const FusedListItem *items, bool planar)
{
  const size_t m = l.members.size();
  CHECK(t.frames % 16 == 0 && t.first % 16 == 0 && t.deltas % 16 == 0 && t.planes % 16 == 0 && t.end % 16 == 0);
  CHECK(t.first == t.frames + m * 96 && t.deltas == t.first + ((m + 1) * 4 + 15) / 16 * 16 && t.planes == t.deltas + m * 1024);
  CHECK(t.end == t.planes + (planar ? m * 16 : 0));
  const RaggedFrame *fr = (const RaggedFrame *)(host + t.frames);
  const uint32_t *first = (const uint32_t *)(host + t.first);
  const int32_t *q = (const int32_t *)(host + t.deltas);
  const PlanarFrame *pl = (const PlanarFrame *)(host + t.planes);
  uint32_t at = 0;
  for (size_t k = 0; k < m; k++) {
    const FusedListItem &it = items[l.members[k]];
    const mijpeg_info &f = *it.info;
    const RaggedFrame &x = fr[k];
    const bool colour = f.components == 3;
    CHECK(x.coef_base == it.coef_base && x.out == it.out[0] && x.row_stride == it.row_stride && x.qframe == (int32_t)k && x.reserved == 0);
    CHECK(x.width == f.width && x.height == f.height);
    CHECK(x.off_y == f.coef_offset[0] && x.off_cb == (colour ? f.coef_offset[1] : 0) && x.off_cr == (colour ? f.coef_offset[2] : 0));
    CHECK(x.bw_y == f.blocks_w[0] && x.bh_y == f.blocks_h[0] && x.bw_c == (colour ? f.blocks_w[1] : 0) && x.bh_c == (colour ? f.blocks_h[1] : 0));
    CHECK(x.cw == (f.width + 1) / 2 && x.ch == (l.p.sampling == Sampling::S422 ? f.height : (f.height + 1) / 2));
    CHECK(x.tiles_x == (f.width + 127) / 128 && x.tiles_y == (f.height + 127) / 128);
    CHECK(first[k] == at);
    at += (uint32_t)(x.tiles_x * x.tiles_y);
    int wrong_deltas = 0;
    for (int c = 0; c < 4; c++)
      for (int z = 0; z < 64; z++) {
        const int32_t want = c >= f.components ? 16 : it.own_deltas ? (int32_t)it.own_deltas[c * 64 + z] << 4 : (int32_t)f.quant[f.quant_index[c]][z] << 4;
        wrong_deltas += q[(k * 4 + (size_t)c) * 64 + (size_t)z] != want;
      }
    CHECK(wrong_deltas == 0);
    if (planar) CHECK(pl[k].g == it.out[1] && pl[k].b == it.out[2]);
  }
  CHECK(first[m] == at && at == l.grid);
  for (const uint8_t *pad = (const uint8_t *)(first + m + 1); pad < host + t.deltas; pad++) CHECK(*pad == 0xA5); // (nobody's: left alone)
}

int main()
{
  // ---- frames: 1 x 1; two tiles each way; grey; one with tables of its own; a launch of three
  std::vector<mijpeg_info> infos;
  infos.push_back(frame(1, 1, 3, 2, 2, 0));      // 0  4:2:0
  infos.push_back(frame(129, 1, 3, 2, 2, 7));    // 1
  infos.push_back(frame(40, 30, 1, 1, 1, 11));   // 2  grey
  infos.push_back(frame(1, 129, 3, 2, 2, 13));   // 3
  infos.push_back(frame(200, 120, 3, 2, 2, 17)); // 4  own_deltas
  infos.push_back(frame(16, 16, 3, 1, 1, 19));   // 5  4:4:4
  infos.push_back(frame(300, 129, 3, 1, 1, 23)); // 6
  infos.push_back(frame(127, 128, 3, 1, 1, 29)); // 7
  uint16_t own[4 * 64];
  for (int i = 0; i < 4 * 64; i++) own[i] = (uint16_t)(2047 - i);
  static uint8_t pixels[8 * 3]; // (addresses only: nothing is written through them)
  const ReconPlan p420 = plan(Recon::FUSED420P, Sampling::S420), pgrey = plan(Recon::FUSED1, Sampling::GREY), p444 = plan(Recon::FUSED444, Sampling::S444);
  std::vector<FusedListItem> items;
  std::vector<FusedListLaunch> launches;
  int64_t base = 0;
  for (size_t i = 0; i < infos.size(); i++) {
    const mijpeg_info &f = infos[i];
    fused_list_add(launches, f.components == 1 ? pgrey : f.hsamp[0] == 2 ? p420 : p444, (int)i, f);
    items.push_back(FusedListItem{&f, base, {pixels + 3 * i, pixels + 3 * i + 1, pixels + 3 * i + 2}, 1000 + (int64_t)i, i == 4 ? own : nullptr});
    base += f.coef_count;
  }
  CHECK(launches.size() == 3);
  CHECK(launches[0].p.kernel == Recon::FUSED420P && launches[0].members == std::vector<int>({0, 1, 3, 4}) && launches[0].grid == 1 + 2 + 2 + 2);
  CHECK(launches[1].p.kernel == Recon::FUSED1 && launches[1].members == std::vector<int>({2}) && launches[1].grid == 1);
  CHECK(launches[2].p.kernel == Recon::FUSED444 && launches[2].members == std::vector<int>({5, 6, 7}) && launches[2].grid == 1 + 6 + 1);
  // ---- the interleaved launches (m = 4, 1, 3) and, behind them, the 4:4:4 one once more with planes out
  std::vector<FusedListTable> tables = fused_list_layout(launches, false);
  CHECK(tables.size() == 3 && tables[0].frames == 0 && tables[1].frames == tables[0].end && tables[2].frames == tables[1].end);
  CHECK(tables[0].deltas - tables[0].first == 32 && tables[1].deltas - tables[1].first == 16 && tables[2].deltas - tables[2].first == 16);
  CHECK(tables[0].end == 4 * 96 + 32 + 4 * 1024 && tables[0].planes == tables[0].end);
  const FusedListTable planar(tables.back().end, launches[2].members.size(), true);
  CHECK(planar.frames == tables[2].end && planar.end == planar.planes + 3 * 16);
  const size_t bytes = planar.end;
  uint8_t *host = (uint8_t *)malloc(bytes); // (exactly the layout: a byte further is the sanitizer's)
  if (!host) return 2;
  memset(host, 0xA5, bytes);
  for (size_t l = 0; l < launches.size(); l++) fused_list_fill(host, tables[l], launches[l], items.data(), false);
  fused_list_fill(host, planar, launches[2], items.data(), true);
  for (size_t l = 0; l < launches.size(); l++) check_tables(host, tables[l], launches[l], items.data(), false);
  check_tables(host, planar, launches[2], items.data(), true);
  // the grey frame: no chroma planes, deltas of 16 for the components it does not have (check_tables saw them; once more by hand)
  const RaggedFrame &grey = *(const RaggedFrame *)(host + tables[1].frames);
  CHECK(grey.off_cb == 0 && grey.off_cr == 0 && grey.bw_c == 0 && grey.bh_c == 0);
  const int32_t *gq = (const int32_t *)(host + tables[1].deltas);
  CHECK(gq[0] == (int32_t)infos[2].quant[3][0] << 4 && gq[64] == 16 && gq[128 + 63] == 16 && gq[192 + 63] == 16);
  // the frame with its own tables, fourth of launch 0: component c takes own[c * 64 ...], not info's
  const int32_t *oq = (const int32_t *)(host + tables[0].deltas) + 3 * 4 * 64;
  CHECK(oq[0] == 2047 << 4 && oq[64] == (2047 - 64) << 4 && oq[2 * 64 + 63] == (2047 - 191) << 4 && oq[3 * 64] == 16);
  free(host);
  // ---- a launch per flavour; a full grid opens the next launch (nothing is allocated per tile)
  const mijpeg_info huge = frame(65535, 65535, 3, 2, 2, 0);
  CHECK(fused_list_tiles(huge) == 512 * 512);
  std::vector<FusedListLaunch> big;
  for (int i = 0; i < 8192; i++) fused_list_add(big, p420, i, huge);
  CHECK(big.size() == 2 && big[0].members.size() == 8191 && big[0].grid == 8191ull * 512 * 512 && big[0].grid <= 0x7fffffffull);
  CHECK(big[1].members == std::vector<int>({8191}) && big[1].grid == 512 * 512);
  fused_list_add(big, p420, 8192, infos[0]); // (one tile more fits the first)
  CHECK(big.size() == 2 && big[0].members.back() == 8192 && big[0].grid == 8191ull * 512 * 512 + 1);
  fused_list_add(big, plan(Recon::FUSED420, Sampling::S420), 8193, infos[0]);
  fused_list_add(big, plan(Recon::FUSED420, Sampling::S420, false), 8194, infos[0]);
  fused_list_add(big, plan(Recon::FUSED422, Sampling::S422, true, true), 8195, infos[0]);
  fused_list_add(big, plan(Recon::FUSED422, Sampling::S422), 8196, infos[0]);
  fused_list_add(big, plan(Recon::FUSED420_12, Sampling::S420, true, false, true), 8197, infos[0]);
  fused_list_add(big, plan(Recon::FUSED420_12, Sampling::S420), 8198, infos[0]);
  fused_list_add(big, plan(Recon::FUSED420, Sampling::S420, false), 8199, infos[0]);
  CHECK(big.size() == 8 && big[3].members == std::vector<int>({8194, 8199}) && big[3].grid == 2);
  if (failures) return 1;
  printf("OK %zu bytes of tables, %zu + 1 launches\n", bytes, launches.size());
  return 0;
}
