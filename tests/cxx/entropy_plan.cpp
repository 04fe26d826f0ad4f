// entropy_plan.cpp -- the device-free half of the on-device entropy decoders (libjpeg_amd/csrc/entropy_plan.hpp) as a program of
// its own, for the sanitizers: the plan of a multiscan decode (levels, table slots, lanes, workgroups, stream slots, the cut, the
// refusals) on hand-made scan lists, its staging read back field by field from a heap buffer of exactly plan.end bytes; the plan
// of the device walk (subsequence size, lanes, group lists, tiles, rounds, the refusals) and its staging in a buffer of exactly
// o_up_end bytes.  Every expected value is written out from the rules, none comes from a run of the code.  No device.
// (tests/test_entropy_plan_cpu.py builds it with -fsanitize=address,undefined and the library's plain-C++ units -- HuffTable::build
// is host_decoder.cpp's -- and runs it.)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>
#include <vector>

#include "entropy_plan.hpp"

using namespace mij;

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      failures++;                                                          \
      fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond);     \
    }                                                                      \
  } while (0)

static const char TOO_LARGE[] = "file too large for one device decode", TOO_FEW[] = "too few restart intervals to occupy the device";
static bool says(const char *got, const char *want) { return got && !strcmp(got, want); }
static size_t r16(size_t x) { return (x + 15) & ~(size_t)15; }
constexpr size_t MiB = (size_t)1 << 20;

// A Huffman code of its own per seed: the lengths of the Annex K luminance tables (the AC one has codes of up to 16 bits, which
// fill second-level tables), values that differ from seed to seed
static HuffTable table(bool ac, int seed)
{
  static const uint8_t dc_counts[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
  static const uint8_t ac_counts[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
  HuffTable t;
  memcpy(t.counts, ac ? ac_counts : dc_counts, 16);
  const int n = ac ? 162 : 12;
  for (int k = 0; k < n; k++) t.values[k] = ac ? (uint8_t)(k * 7 + seed) : (uint8_t)((k + seed) % 12);
  t.defined = true;
  t.built = t.build();
  CHECK(t.built);
  return t;
}

// Scan number `id` of a test: components `comps` of the frame, its band and bits, its MCU grid and restart interval, the size of
// its entropy coded data.  Tables with seeds of its own where the rules give it a slot; `with_intervals`: interval lists for a fill.
static Scan scan(int id, std::initializer_list<int> comps, int ss, int se, int ah, int al, int mcus_x, int mcus_y, int restart_interval, size_t usize,
                 bool with_intervals = false)
{
  Scan s;
  for (int c : comps) {
    s.sc[s.ncomp].comp = c;
    s.dc[s.ncomp] = table(false, 16 * id + s.ncomp);
    s.ac[s.ncomp] = table(true, 16 * id + s.ncomp + 8);
    s.ncomp++;
  }
  s.ss = ss; s.se = se; s.ah = ah; s.al = al;
  s.refinement = ah > 0;
  s.progressive_run = se > 0 && id % 2 == 1;
  s.mcus_x = mcus_x;
  s.mcus_y = mcus_y;
  s.restart_interval = restart_interval;
  s.unstuffed_size = usize;
  if (with_intervals) {
    const int64_t mcus = (int64_t)mcus_x * mcus_y, nint = restart_interval > 0 ? (mcus + restart_interval - 1) / restart_interval : 1;
    for (int64_t k = 0; k < nint; k++) {
      s.interval_ubegin.push_back((uint32_t)(1000 * id + k));
      s.interval_uend.push_back((uint32_t)(1000 * id + k + 500));
    }
  }
  return s;
}

// a 4:2:0 frame of 64 x 48 pixels: 4 x 3 MCUs, luma 8 x 6 blocks, chroma 4 x 3
static mijpeg_info frame420(bool wide)
{
  mijpeg_info f;
  memset(&f, 0, sizeof(f));
  f.width = 64; f.height = 48; f.components = 3; f.precision = 8;
  const int hs[3] = {2, 1, 1}, bw[3] = {8, 4, 4}, bh[3] = {6, 3, 3};
  int64_t off = 0;
  for (int c = 0; c < 3; c++) {
    f.hsamp[c] = f.vsamp[c] = hs[c];
    f.blocks_w[c] = bw[c];
    f.blocks_h[c] = bh[c];
    f.coef_offset[c] = off;
    off += (int64_t)bw[c] * bh[c] * 64 * (wide ? 2 : 1);
  }
  f.coef_count = off;
  f.coef_wide = wide ? 1 : 0;
  return f;
}

// the rules for stream slots, whatever the script: on 16-byte boundaries, as large as the data and its pad, ordered by level and
// then by item, none into the next; level_end non-decreasing, each where its level's last slot ends, the last one stream_bytes
static void check_slots(const MultiscanPlan &p, const FrameScans *frames)
{
  size_t at = 0;
  for (int lv = 0; lv < p.levels(); lv++) {
    for (const MultiscanPlan::Item &it : p.items) {
      if (it.level != lv) continue;
      CHECK(it.stream_off % 16 == 0);
      CHECK(it.stream_off == at);
      at = r16(it.stream_off + (*frames[it.frame].scans)[it.scan].unstuffed_size + HUFF_STREAM_PAD);
    }
    CHECK(p.level_end[(size_t)lv] == at);
    CHECK(lv == 0 || p.level_end[(size_t)lv] >= p.level_end[(size_t)lv - 1]);
  }
  CHECK(p.stream_bytes == at);
  for (const MultiscanPlan::Item &it : p.items) CHECK(it.level >= 0 && it.level < p.levels());
}

// the staging of a plan in a heap buffer of exactly plan.end bytes, every field read back.  The descriptors are compared with the
// plan's items, not with literals: a caller asserts the items (level, intervals, slots, offsets) against hand-written numbers FIRST,
// as test_level_chain and test_two_frames do -- without that this check only says that plan and fill agree.
static void check_fill(const MultiscanPlan &p, const FrameScans *frames, const std::vector<std::vector<uint32_t>> &want_groups)
{
  uint8_t *hp = new uint8_t[p.end];
  memset(hp, 0xcd, p.end);
  fill_multiscan(p, frames, hp);
  const uint32_t *ib = (const uint32_t *)(hp + p.ibegin), *ie = (const uint32_t *)(hp + p.iend);
  const ProgScanDev *sd = (const ProgScanDev *)(hp + p.scans);
  HuffDevTable *scratch = new HuffDevTable;
  for (size_t ii = 0; ii < p.items.size(); ii++) {
    const MultiscanPlan::Item &it = p.items[ii];
    const mijpeg_info &f = *frames[it.frame].info;
    const Scan &s = (*frames[it.frame].scans)[it.scan];
    const ProgScanDev &o = sd[ii];
    const int64_t mcus = (int64_t)s.mcus_x * s.mcus_y;
    CHECK(o.stream_off == it.stream_off && o.first_interval == it.first && o.n_intervals == it.nint);
    CHECK(o.total_mcus == mcus && o.mcus_x == s.mcus_x);
    CHECK(o.restart_interval == (s.restart_interval > 0 ? s.restart_interval : mcus));
    CHECK(o.ncomp == s.ncomp && o.ntables == it.ntab && o.table_off == it.table_off);
    CHECK(o.ss == s.ss && o.se == s.se && o.ah == s.ah && o.al == s.al);
    CHECK(o.runs_legal == (s.progressive_run ? 1 : 0) && o.reserved == 0);
    for (int k = 0; k < 4; k++) {
      if (k >= s.ncomp) { // (the descriptor starts out as zeros)
        CHECK(o.comp[k] == 0 && o.hs[k] == 0 && o.vs[k] == 0 && o.bw[k] == 0 && o.coef_off[k] == 0 && o.dc_tab[k] == 0 && o.ac_tab[k] == 0);
        continue;
      }
      const int c = s.sc[k].comp;
      CHECK(o.comp[k] == c);
      CHECK(o.hs[k] == (s.ncomp > 1 ? f.hsamp[c] : 1) && o.vs[k] == (s.ncomp > 1 ? f.vsamp[c] : 1));
      CHECK(o.bw[k] == f.blocks_w[c]);
      CHECK(o.coef_off[k] == (f.coef_wide ? f.coef_offset[c] / 2 : f.coef_offset[c]));
      CHECK(o.dc_tab[k] == it.dc_tab[k] && o.ac_tab[k] == it.ac_tab[k]);
      // the slot a scan component names holds the table built from that component's code
      const HuffDevTable *tabs = (const HuffDevTable *)(hp + p.tables + o.table_off);
      if (s.ss == 0 && s.ah == 0) {
        build_dev_table(*scratch, s.dc[k], 0);
        CHECK(o.dc_tab[k] < o.ntables && !memcmp(&tabs[o.dc_tab[k]], scratch, sizeof(HuffDevTable)));
      }
      if (s.se > 0) {
        build_dev_table(*scratch, s.ac[k], 2);
        CHECK(o.ac_tab[k] < o.ntables && !memcmp(&tabs[o.ac_tab[k]], scratch, sizeof(HuffDevTable)));
      }
    }
    for (int64_t k = 0; k < it.nint; k++) {
      CHECK(ib[it.first + k] == s.interval_ubegin[(size_t)k]);
      CHECK(ie[it.first + k] == s.interval_uend[(size_t)k]);
    }
  }
  // the workgroups: launch by launch {scan, first interval}, as many as the plan counts
  const ProgGroup *groups = (const ProgGroup *)(hp + p.groups);
  CHECK(want_groups.size() == p.launches.size());
  int64_t g = 0;
  for (size_t l = 0; l < p.launches.size() && l < want_groups.size(); l++) {
    CHECK(p.launches[l].g0 == g && p.launches[l].groups * 2 == (int64_t)want_groups[l].size());
    for (size_t k = 0; k + 1 < want_groups[l].size() && g < p.n_groups; k += 2, g++)
      CHECK(groups[g].scan == want_groups[l][k] && groups[g].first_interval == want_groups[l][k + 1]);
  }
  CHECK(g == p.n_groups);
  // the status words are the device's: the fill leaves them alone
  for (size_t k = p.status; k < p.end; k++) CHECK(hp[k] == 0xcd);
  delete scratch;
  delete[] hp;
}

static void check_tail_layout(const MultiscanPlan &p, int nframes)
{
  size_t at = 0;
  CHECK(p.ibegin == at); at = r16(at + (size_t)p.total_intervals * 4);
  CHECK(p.iend == at);   at = r16(at + (size_t)p.total_intervals * 4);
  CHECK(p.tables == at); at = r16(at + p.table_bytes);
  CHECK(p.scans == at);  at = r16(at + p.items.size() * sizeof(ProgScanDev));
  CHECK(p.groups == at); at = r16(at + (size_t)p.n_groups * sizeof(ProgGroup));
  CHECK(p.status == at && p.status_bytes == (size_t)nframes * 32);
  CHECK(p.end == at + (size_t)nframes * 32);
}

// DC first pass interleaved; AC Y 1..5; AC Cb 1..63; AC Cr 1..63; AC Y 6..63; AC Y refinement; DC refinement interleaved
static void test_level_chain()
{
  const mijpeg_info f = frame420(false);
  // single-component scans: luma 8 x 6 MCUs, chroma 4 x 3
  const std::vector<Scan> scans = {scan(0, {0, 1, 2}, 0, 0, 0, 1, 4, 3, 1, 100, true), scan(1, {0}, 1, 5, 0, 2, 8, 6, 8, 37, true),
                                   scan(2, {1}, 1, 63, 0, 1, 4, 3, 0, 16, true),       scan(3, {2}, 1, 63, 0, 1, 4, 3, 0, 0, true),
                                   scan(4, {0}, 6, 63, 0, 2, 8, 6, 5, 1000, true),     scan(5, {0}, 1, 5, 1, 0, 8, 6, 8, 5, true),
                                   scan(6, {0, 1, 2}, 0, 0, 1, 0, 4, 3, 5, 1, true)};
  const FrameScans fr{&f, &scans};
  MultiscanPlan p;
  CHECK(plan_multiscan(&fr, 1, 12, p) == nullptr); // (the widest launch: level 0's 12 intervals)
  CHECK(says(plan_multiscan(&fr, 1, 13, p), TOO_FEW));
  CHECK(plan_multiscan(&fr, 1, 1, p) == nullptr);
  const int level[7] = {0, 1, 1, 1, 2, 3, 4}, ntab[7] = {3, 1, 1, 1, 1, 1, 0};
  const int64_t nint[7] = {12, 6, 1, 1, 10, 6, 3}, first[7] = {0, 12, 18, 19, 20, 30, 36}; // ceil(MCUs / restart interval), or 1
  const size_t tables_in_front[7] = {0, 3, 4, 5, 6, 7, 8};
  // slots of size + 256 rounded to 16, level by level: 368 | 304, 272, 256 | 1264 | 272 | 272
  const size_t stream_off[7] = {0, 368, 672, 944, 1200, 2464, 2736};
  CHECK(p.items.size() == 7);
  for (size_t j = 0; j < 7 && j < p.items.size(); j++) {
    const MultiscanPlan::Item &it = p.items[j];
    CHECK(it.frame == 0 && it.scan == j);
    CHECK(it.level == level[j]);
    CHECK(it.ntab == ntab[j]);
    CHECK(it.table_off == tables_in_front[j] * sizeof(HuffDevTable));
    CHECK(it.nint == nint[j] && it.first == first[j]);
    CHECK(it.stream_off == stream_off[j]);
  }
  // a DC slot per component of the first DC pass, an AC slot for the AC scans, none for the DC refinement
  CHECK(p.items[0].dc_tab[0] == 0 && p.items[0].dc_tab[1] == 1 && p.items[0].dc_tab[2] == 2);
  for (int j = 1; j <= 5; j++) CHECK(p.items[(size_t)j].ac_tab[0] == 0);
  CHECK(p.max_tables == 3 && p.table_bytes == 8 * sizeof(HuffDevTable));
  CHECK(p.levels() == 5 && p.frame_levels.size() == 1 && p.frame_levels[0] == 5);
  CHECK(p.total_intervals == 39 && p.widest == 12);
  const size_t level_end[5] = {368, 1200, 2464, 2736, 3008};
  for (int lv = 0; lv < 5 && lv < p.levels(); lv++) CHECK(p.level_end[(size_t)lv] == level_end[lv]);
  CHECK(p.stream_bytes == 3008);
  CHECK(p.cut == 2); // 368 * 4 < 3008 <= 1200 * 4
  // every launch has few intervals: one lane per wave, four intervals per workgroup
  CHECK(p.level_lanes.size() == 1 && p.level_lanes[0] == std::vector<int>({1, 1, 1, 1, 1}));
  CHECK(p.n_groups == 13);
  check_slots(p, &fr);
  check_tail_layout(p, 1);
  check_fill(p, &fr, {{0, 0, 0, 4, 0, 8}, {1, 0, 1, 4, 2, 0, 3, 0}, {4, 0, 4, 4, 4, 8}, {5, 0, 5, 4}, {6, 0}});
}

// a JPEG XT pair: levels are counted per frame, launches are ordered frame, level, scan; the second frame's planes are wide
static void test_two_frames()
{
  const mijpeg_info fa = frame420(false), fb = frame420(true);
  const std::vector<Scan> a = {scan(0, {0, 1, 2}, 0, 0, 0, 0, 4, 3, 2, 300, true), scan(1, {0}, 1, 63, 0, 0, 8, 6, 0, 40, true),
                               scan(2, {1}, 1, 63, 0, 0, 4, 3, 4, 50, true)};
  const std::vector<Scan> b = {scan(3, {0, 1, 2}, 0, 63, 0, 1, 4, 3, 1, 70, true), scan(4, {0}, 1, 63, 1, 0, 8, 6, 6, 9, true)};
  const FrameScans fr[2] = {{&fa, &a}, {&fb, &b}};
  MultiscanPlan p;
  CHECK(plan_multiscan(fr, 2, 1, p) == nullptr);
  const int frame[5] = {0, 0, 0, 1, 1}, level[5] = {0, 1, 1, 0, 1}, ntab[5] = {3, 1, 1, 6, 1};
  const size_t scan_of[5] = {0, 1, 2, 0, 1}, tables_in_front[5] = {0, 3, 4, 5, 11};
  const int64_t nint[5] = {6, 1, 3, 12, 8}, first[5] = {0, 6, 7, 10, 22};
  // level 0: frame 0's scan 0 (560 bytes), frame 1's scan 0 (336); level 1: 304, 320, 272
  const size_t stream_off[5] = {0, 896, 1200, 560, 1520};
  CHECK(p.items.size() == 5);
  for (size_t j = 0; j < 5 && j < p.items.size(); j++) {
    const MultiscanPlan::Item &it = p.items[j];
    CHECK(it.frame == frame[j] && it.scan == scan_of[j] && it.level == level[j] && it.ntab == ntab[j]);
    CHECK(it.table_off == tables_in_front[j] * sizeof(HuffDevTable));
    CHECK(it.nint == nint[j] && it.first == first[j]);
    CHECK(it.stream_off == stream_off[j]);
  }
  // a sequential scan over three components: DC and AC slot per component, in turn
  for (int k = 0; k < 3; k++) CHECK(p.items[3].dc_tab[k] == 2 * k && p.items[3].ac_tab[k] == 2 * k + 1);
  CHECK(p.max_tables == 6 && p.table_bytes == 12 * sizeof(HuffDevTable));
  CHECK(p.frame_levels == std::vector<int>({2, 2}) && p.levels() == 2);
  CHECK(p.level_end == std::vector<size_t>({896, 1792}) && p.stream_bytes == 1792);
  CHECK(p.cut == 1);
  CHECK(p.widest == 12 && p.total_intervals == 30 && p.n_groups == 2 + 1 + 1 + 3 + 2);
  CHECK(p.launches.size() == 4);
  const int lframe[4] = {0, 0, 1, 1}, llevel[4] = {0, 1, 0, 1};
  for (size_t l = 0; l < 4 && l < p.launches.size(); l++) CHECK(p.launches[l].frame == lframe[l] && p.launches[l].level == llevel[l]);
  check_slots(p, fr);
  check_tail_layout(p, 2);
  check_fill(p, fr, {{0, 0, 0, 4}, {1, 0, 2, 0}, {3, 0, 3, 4, 3, 8}, {4, 0, 4, 4}});
}

// one grey scan of `intervals` restart intervals of one MCU (plan only: it has no interval lists)
static std::vector<Scan> grey(int64_t intervals, size_t usize = 64) { return {scan(0, {0}, 0, 63, 0, 0, (int)intervals, 1, 1, usize)}; }

static void test_lanes_and_groups()
{
  mijpeg_info f;
  memset(&f, 0, sizeof(f));
  // 64 lanes halved while intervals / lanes < 768; groups = ceil(intervals / (lanes * 4))
  const int64_t intervals[4] = {1535, 1536, 49151, 49152}, groups[4] = {384, 192, 384, 192};
  const int lanes[4] = {1, 2, 32, 64};
  for (int t = 0; t < 4; t++) {
    const std::vector<Scan> s = grey(intervals[t]);
    const FrameScans fr{&f, &s};
    MultiscanPlan p;
    CHECK(plan_multiscan(&fr, 1, 1, p) == nullptr);
    CHECK(p.level_lanes.size() == 1 && p.level_lanes[0] == std::vector<int>({lanes[t]}));
    CHECK(p.n_groups == groups[t] && p.launches.size() == 1 && p.launches[0].groups == groups[t] && p.launches[0].g0 == 0);
    CHECK(p.widest == intervals[t] && p.total_intervals == intervals[t]);
    CHECK(p.levels() == 1 && p.cut == 1); // a one-level frame: nothing to cut
  }
  // the lanes of a launch come from the SUM of its intervals: 768 + 768 side by side decode with two lanes, each alone with one
  const std::vector<Scan> two = {scan(0, {0}, 1, 63, 0, 0, 768, 1, 1, 10), scan(1, {1}, 1, 63, 0, 0, 768, 1, 1, 10)};
  const FrameScans fr{&f, &two};
  MultiscanPlan p;
  CHECK(plan_multiscan(&fr, 1, 1, p) == nullptr);
  CHECK(p.levels() == 1 && p.level_lanes[0] == std::vector<int>({2}) && p.n_groups == 96 + 96 && p.widest == 1536);
  setenv("MIJPEG_HUFF_LANES", "16", 1);
  CHECK(lanes_for(5) == 16 && lanes_for(1 << 20) == 16);
  setenv("MIJPEG_HUFF_LANES", "24", 1); // (no power of two: not taken)
  CHECK(lanes_for(5) == 1);
  unsetenv("MIJPEG_HUFF_LANES");
}

static void test_cut()
{
  mijpeg_info f;
  memset(&f, 0, sizeof(f));
  MultiscanPlan p;
  // level 0 holds half of the bytes (1264 of 2528): the first upload is level 0 alone
  const std::vector<Scan> half = {scan(0, {0}, 0, 0, 0, 0, 4, 3, 1, 1000), scan(1, {0}, 1, 63, 0, 0, 4, 3, 1, 1000)};
  const FrameScans fh{&f, &half};
  CHECK(plan_multiscan(&fh, 1, 1, p) == nullptr);
  CHECK(p.levels() == 2 && p.level_end == std::vector<size_t>({1264, 2528}) && p.cut == 1);
  // 256, 512 of 4768 bytes: no level in front of the last brings a quarter, so everything goes up in one go
  const std::vector<Scan> late = {scan(0, {0}, 0, 0, 0, 0, 4, 3, 1, 0), scan(1, {0}, 1, 5, 0, 0, 4, 3, 1, 0), scan(2, {0}, 6, 63, 0, 0, 4, 3, 1, 4000)};
  const FrameScans fl{&f, &late};
  CHECK(plan_multiscan(&fl, 1, 1, p) == nullptr);
  CHECK(p.levels() == 3 && p.level_end == std::vector<size_t>({256, 512, 4768}) && p.cut == 3);
  // exactly a quarter counts: 1024 of 4096 (sizes 768, 2816 -> slots 1024, 3072)
  const std::vector<Scan> quarter = {scan(0, {0}, 0, 0, 0, 0, 4, 3, 1, 768), scan(1, {0}, 1, 63, 0, 0, 4, 3, 1, 2816)};
  const FrameScans fq{&f, &quarter};
  CHECK(plan_multiscan(&fq, 1, 1, p) == nullptr);
  CHECK(p.level_end == std::vector<size_t>({1024, 4096}) && p.cut == 1);
}

static void test_multiscan_refusals()
{
  mijpeg_info f;
  memset(&f, 0, sizeof(f));
  MultiscanPlan p;
  for (int min_intervals : {0, -5}) { // (not positive: 2048)
    const std::vector<Scan> few = grey(2047), enough = grey(2048);
    const FrameScans ff{&f, &few}, fe{&f, &enough};
    CHECK(says(plan_multiscan(&ff, 1, min_intervals, p), TOO_FEW));
    CHECK(plan_multiscan(&fe, 1, min_intervals, p) == nullptr);
  }
  // 2^31 - 1 intervals are planned, 2^31 are too many -- also where the launch is too narrow for the caller as well: two levels of
  // 2^30 intervals each, and a caller that asks for 2^31 - 1 in one launch
  {
    const std::vector<Scan> most = grey(0x7fffffff), two = {scan(0, {0}, 0, 0, 0, 0, 1 << 15, 1 << 15, 1, 64), scan(1, {0}, 1, 63, 0, 0, 1 << 15, 1 << 15, 1, 64)};
    const FrameScans fm{&f, &most}, ft{&f, &two};
    CHECK(plan_multiscan(&fm, 1, 0, p) == nullptr && p.total_intervals == 0x7fffffff);
    CHECK(says(plan_multiscan(&ft, 1, 0x7fffffff, p), TOO_LARGE));
  }
  // stream bytes: a slot that ends at 0xfffffff0 is planned, one byte more is too large -- with its one interval, which is too few
  // as well
  {
    const std::vector<Scan> fits = {scan(0, {0}, 0, 63, 0, 0, 4, 3, 0, 0xfffffff0ull - 256)}, over = {scan(0, {0}, 0, 63, 0, 0, 4, 3, 0, 0xfffffff0ull - 255)};
    const FrameScans ff{&f, &fits}, fo{&f, &over};
    CHECK(plan_multiscan(&ff, 1, 1, p) == nullptr && p.stream_bytes == 0xfffffff0ull);
    CHECK(says(plan_multiscan(&ff, 1, 0, p), TOO_FEW));
    CHECK(says(plan_multiscan(&fo, 1, 0, p), TOO_LARGE));
    CHECK(says(plan_multiscan(&fo, 1, 1, p), TOO_LARGE));
  }
}

// ---- the device walk ----
static WalkImage walked(size_t bytes, int64_t first_interval = 0, int64_t n_intervals = 1, int mcus_per_interval = 1, int64_t total_mcus = 1)
{
  return WalkImage{true, false, mcus_per_interval, bytes, first_interval, n_intervals, total_mcus};
}
static const char TOO_LONG[] = "stream too long for the device walk", TOO_MANY_BLOCKS[] = "too many blocks per MCU for the device walk";

static void test_walk_sizes()
{
  WalkPlan p;
  // 128 up to 8 MiB of walked bytes, 256 up to 32 MiB, else 512; deferred rounds 40, 24, 16
  const size_t bytes[4] = {8 * MiB, 8 * MiB + 1, 32 * MiB, 32 * MiB + 1};
  const uint32_t sub[4] = {128, 256, 256, 512}, nsub[4] = {65536, 32769, 131072, 65537};
  const int rounds[4] = {40, 24, 24, 16}, lanes[4] = {32, 16, 64, 32}, tiles[4] = {64, 33, 128, 65};
  for (int t = 0; t < 4; t++) {
    const WalkImage im = walked(bytes[t]);
    CHECK(plan_walk(&im, 1, false, 6, p) == nullptr);
    CHECK(p.sub_bytes == sub[t] && p.defer_rounds == rounds[t]);
    CHECK(p.nsub_total == nsub[t] && p.img_nsub[0] == nsub[t] && p.lanes == lanes[t] && p.tiles == tiles[t]);
    CHECK(p.nblk_mcu == 6 && p.n == 1 && !p.per_image && !p.any_fit);
  }
  // the bytes of all walked images count, those of the others do not
  const WalkImage both[2] = {walked(4 * MiB), walked(4 * MiB + 1)};
  CHECK(plan_walk(both, 2, false, 6, p) == nullptr && p.sub_bytes == 256);
  WalkImage mixed[2] = {walked(8 * MiB), walked(8 * MiB)};
  mixed[1].device_walked = false;
  CHECK(plan_walk(mixed, 2, false, 6, p) == nullptr && p.sub_bytes == 128 && p.img_nsub[1] == 0 && p.nsub_total == 65536);
  // one long image: doubled while below 1024 and longest / sub_bytes > 2^20.  512 MiB are 2^20 subsequences of 512 bytes and 1024
  // tiles; up to 511 bytes more are one subsequence and one tile too many; from 512 more on the subsequences have 1024 bytes
  const WalkImage at = walked(512 * MiB), over = walked(512 * MiB + 511), doubled = walked(512 * MiB + 512), last = walked(1024 * MiB), longest = walked(1024 * MiB + 1);
  CHECK(plan_walk(&at, 1, false, 6, p) == nullptr && p.sub_bytes == 512 && p.nsub_total == (1u << 20) && p.tiles == 1024);
  CHECK(says(plan_walk(&over, 1, false, 6, p), TOO_LONG) && p.sub_bytes == 512);
  CHECK(plan_walk(&doubled, 1, false, 6, p) == nullptr && p.sub_bytes == 1024 && p.nsub_total == (1u << 19) + 1 && p.tiles == 513 && p.defer_rounds == 16);
  CHECK(plan_walk(&last, 1, false, 6, p) == nullptr && p.sub_bytes == 1024 && p.tiles == 1024);
  CHECK(says(plan_walk(&longest, 1, false, 6, p), TOO_LONG));
  // blocks per MCU
  const WalkImage small = walked(5000);
  CHECK(plan_walk(&small, 1, false, 64, p) == nullptr && p.nblk_mcu == 64);
  CHECK(says(plan_walk(&small, 1, false, 65, p), TOO_MANY_BLOCKS));
  // MIJPEG_WALK_SUB, clamped to 32 .. 4096
  setenv("MIJPEG_WALK_SUB", "8", 1);
  CHECK(plan_walk(&small, 1, false, 6, p) == nullptr && p.sub_bytes == 32 && p.nsub_total == 157 && p.defer_rounds == 40);
  setenv("MIJPEG_WALK_SUB", "100000", 1);
  CHECK(plan_walk(&small, 1, false, 6, p) == nullptr && p.sub_bytes == 4096 && p.nsub_total == 2 && p.defer_rounds == 16);
  unsetenv("MIJPEG_WALK_SUB");
}

static void test_walk_lanes()
{
  // 64 lanes halved while subsequences / lanes < 2048 (128-byte subsequences up to 8 MiB, 256-byte ones up to 32 MiB)
  const uint32_t nsub[4] = {4095, 4096, 131071, 131072}, sub[4] = {128, 128, 256, 256};
  const int lanes[4] = {1, 2, 32, 64};
  WalkPlan p;
  for (int t = 0; t < 4; t++) {
    const WalkImage im = walked((size_t)nsub[t] * sub[t]);
    CHECK(plan_walk(&im, 1, false, 3, p) == nullptr);
    CHECK(p.sub_bytes == sub[t] && p.nsub_total == nsub[t] && p.lanes == lanes[t]);
    const size_t per_group = (size_t)lanes[t] * 4;
    CHECK(p.sub_image.size() == (nsub[t] + per_group - 1) / per_group && p.sub_first.size() == p.sub_image.size());
    CHECK(p.sub_first.back() == (p.sub_first.size() - 1) * per_group && p.sub_image.back() == 0);
  }
}

static void check_walk_layout(const WalkPlan &p, bool per_image, bool any_fit)
{
  const size_t G = p.sub_image.size(), S = p.nsub_total, N = (size_t)p.n;
  size_t at = 0;
  CHECK(p.o_simg == at);   at = r16(at + G * 4);
  CHECK(p.o_sfirst == at); at = r16(at + G * 4);
  CHECK(p.o_isub0 == at);  at = r16(at + N * 4);
  CHECK(p.o_insub == at);  at = r16(at + N * 4);
  CHECK(p.o_e0 == at);     at = r16(at + N * 4);
  CHECK(p.o_e1 == at);     at = r16(at + N * 4);
  CHECK(p.o_int0 == at);   at = r16(at + N * 4);
  CHECK(p.o_state == at);  at = r16(at + S * 8);
  CHECK(p.o_every == at);  at = r16(at + (per_image ? N * 4 : 0));
  CHECK(p.o_blocks == at); at = r16(at + (per_image ? N * 4 : 0));
  CHECK(p.o_fit == at);    at = r16(at + (any_fit ? N * 4 : 0));
  CHECK(p.o_up_end == at);
  CHECK(p.o_flags == at);  at = r16(at + 49 * 4 + N * 4); // changed[0 .. 48], a status word per image
  CHECK(p.o_stamp == at);  at = r16(at + S * 4);
  CHECK(p.o_zero_end == at);
  CHECK(p.o_nblk == at);   at = r16(at + S * 4);
  CHECK(p.o_dcsum == at);  at = r16(at + S * 16);
  CHECK(p.o_fblk == at);   at = r16(at + S * 4);
  CHECK(p.o_fpred == at);  at = r16(at + S * 16);
  CHECK(p.o_tiles == at);  at = r16(at + N * (size_t)p.tiles * 40);
  CHECK(p.end == at);
  CHECK(p.flags_bytes() == r16(49 * 4 + N * 4));
}

// walked and not-walked images side by side: a ragged launch with one image that is walked behind its search, and the same
// images in a uniform launch without one
static void test_walk_mixed_launch()
{
  // {walked, searched walk, MCUs per interval, bytes, first interval, intervals, MCUs}
  WalkImage images[4] = {{true, false, 3, 1000, 0, 40, 120}, {false, false, 7, 5000, 40, 1, 7}, {true, true, 2, 129, 41, 11, 22}, {true, false, 5, 128 * 9, 52, 4, 20}};
  for (int ragged = 1; ragged >= 0; ragged--) {
    if (!ragged) images[2].searched_walk = false;
    WalkPlan p;
    CHECK(plan_walk(images, 4, ragged != 0, 6, p) == nullptr);
    CHECK(p.sub_bytes == 128 && p.lanes == 1 && p.tiles == 1 && p.nsub_total == 19 && p.any_fit == (ragged != 0) && p.per_image == (ragged != 0));
    CHECK(p.img_nsub == std::vector<uint32_t>({8, 0, 2, 9}));
    CHECK(p.img_sub0 == std::vector<uint32_t>({0, 8, 8, 10}));
    CHECK(p.img_e0 == std::vector<uint32_t>({0, 0, 0, 0}));
    CHECK(p.img_e1 == std::vector<uint32_t>({1000, 5000, 129, 1152}));
    CHECK(p.img_int0 == std::vector<uint32_t>({0, 40, 41, 52}));
    // four subsequences per workgroup; the image that is not walked has none
    CHECK(p.sub_image == std::vector<uint32_t>({0, 0, 2, 3, 3, 3}));
    CHECK(p.sub_first == std::vector<uint32_t>({0, 4, 0, 0, 4, 8}));
    check_walk_layout(p, ragged != 0, ragged != 0);
    uint8_t *wh = new uint8_t[p.o_up_end];
    memset(wh, 0xcd, p.o_up_end);
    fill_walk(p, images, wh);
    auto words = [&](size_t off, size_t n) { return std::vector<uint32_t>((const uint32_t *)(wh + off), (const uint32_t *)(wh + off) + n); };
    CHECK(words(p.o_simg, 6) == p.sub_image && words(p.o_sfirst, 6) == p.sub_first);
    CHECK(words(p.o_isub0, 4) == p.img_sub0 && words(p.o_insub, 4) == p.img_nsub && words(p.o_e0, 4) == p.img_e0 && words(p.o_e1, 4) == p.img_e1);
    CHECK(words(p.o_int0, 4) == p.img_int0);
    // the initial states: subsequence k of its image starts at byte k * 128, no bits to skip, first block of an MCU
    const uint64_t *st = (const uint64_t *)(wh + p.o_state);
    const uint64_t want[19] = {0, 128, 256, 384, 512, 640, 768, 896, 0, 128, 0, 128, 256, 384, 512, 640, 768, 896, 1024};
    for (int k = 0; k < 19; k++) CHECK(st[k] == want[k]);
    if (ragged) {
      // blocks per virtual interval (one MCU's for an image that is not walked) and blocks in all, six blocks to the MCU
      CHECK(words(p.o_every, 4) == std::vector<uint32_t>({18, 6, 12, 30}));
      CHECK(words(p.o_blocks, 4) == std::vector<uint32_t>({720, 42, 132, 120}));
      // the fit step's virtual intervals: of the image that is walked behind its search
      CHECK(words(p.o_fit, 4) == std::vector<uint32_t>({0, 0, 11, 0}));
    } else {
      CHECK(p.o_every == p.o_up_end && p.o_blocks == p.o_up_end && p.o_fit == p.o_up_end); // (no such regions: nothing to write)
    }
    delete[] wh;
  }
  // a ragged launch without a searched walk has the per-image blocks and no fit counts
  WalkPlan p;
  CHECK(plan_walk(images, 4, true, 6, p) == nullptr && !p.any_fit && p.o_blocks > p.o_every && p.o_fit == p.o_up_end);
  uint8_t *wh = new uint8_t[p.o_up_end];
  fill_walk(p, images, wh);
  CHECK(((const uint32_t *)(wh + p.o_blocks))[3] == 120);
  delete[] wh;
}

int main()
{
  for (const char *name : {"MIJPEG_HUFF_LANES", "MIJPEG_WALK_SUB", "MIJPEG_HUFF_NO_SUBTABLES"}) unsetenv(name);
  test_level_chain();
  test_two_frames();
  test_lanes_and_groups();
  test_cut();
  test_multiscan_refusals();
  test_walk_sizes();
  test_walk_lanes();
  test_walk_mixed_launch();
  if (failures) {
    fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  printf("OK entropy_plan\n");
  return 0;
}
