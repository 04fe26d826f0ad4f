// entropy_plan.hpp -- on-device entropy decoding (entropy_device.cpp), the host half that needs no device: what the sequential,
// progressive and walk paths share (packed-buffer regions, lanes per wave, blocks per MCU, Huffman tables in the device's form),
// and plan + fill of the two paths whose drivers are stages over a plan: all scans of a file level by level (plan_multiscan,
// fill_multiscan -> device_entropy_multiscan) and the walk that finds the restart points of streams without restart markers
// (plan_walk, fill_walk -> device_walk_images).  Plain functions over Scan, mijpeg_info and integers; calls nothing of the HIP
// runtime: a plain host compiler builds tests/cxx/entropy_plan.cpp around it.  Private to libmijpeg.so.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/mijpeg.h"
#include "host_decoder.hpp"
#include "huffman_dev.hpp"

namespace mij {

// Workgroups of the Huffman kernels hold four waves, one per SIMD: with two-wave workgroups (which round 1 chose for the LDS
// they leave to others) the same eight waves per CU decode 37 % slower (0.60 against 0.38 ms per 32 4K frames; 3, 5, 6 waves:
// 0.55, 0.58, 0.48) -- the waves of a workgroup go to the SIMDs in cyclic order, and only a multiple of four loads them evenly
constexpr int WAVES_PER_GROUP = 4;

// The regions of a packed buffer: offsets handed out in order, each region starting on a 16-byte boundary.
struct Layout {
  size_t end = 0;
  size_t take(size_t bytes) { const size_t at = end; end = (at + bytes + 15) & ~(size_t)15; return at; }
};

// Decoding lanes per wave for a launch of `intervals` restart intervals: about a thousand waves (one per SIMD) are what a small
// launch wants -- fewer lanes per wave mean more waves that each issue the same instructions for less, fuller waves mean longer
// steps (the slowest lane's block).  Measured with the bit-addressed reader and four-wave workgroups on one 8K 4:2:0 frame with
// 16200 intervals (tools/gpu_huff_lanes.sh): 1 lane 0.81 ms, 2: 0.52, 4: 0.33, 8: 0.26, 16: 0.26, 32: 0.27.
// MIJPEG_HUFF_LANES (a power of two up to 64) overrides the choice.
inline int lanes_for(int64_t intervals)
{
  int lanes = 64;
  while (lanes > 1 && intervals / lanes < 768) lanes >>= 1;
  if (const char *e = getenv("MIJPEG_HUFF_LANES")) {
    const int l = atoi(e);
    if (l >= 1 && l <= 64 && (l & (l - 1)) == 0) lanes = l;
  }
  return lanes;
}

// Blocks of scan component k in one MCU: an interleaved scan uses the frame's sampling factors, a single-component scan 1 x 1
struct McuBlocks { int h, v; };
inline McuBlocks mcu_blocks(const mijpeg_info &f, const Scan &s, int k)
{
  const int c = s.sc[k].comp;
  return s.ncomp > 1 ? McuBlocks{f.hsamp[c], f.vsamp[c]} : McuBlocks{1, 1};
}

// Where component c's plane starts inside its frame's coefficient store, in coefficients (coef_offset counts int16 slots, two to a
// coefficient of a wide store)
inline int64_t plane_offset(const mijpeg_info &f, int c) { return f.coef_offset[c] / (f.coef_wide ? 2 : 1); }

// Second-level tables of a device Huffman table: every code longer than the direct table's ten bits, grouped by its first
// ten bits, in a 64-entry table indexed by the six bits that follow (entries as in the direct table: huff_dev_entry).  Codes
// whose prefix finds no table left keep the direct entry HUFF_DEV_SUB | HUFF_DEV_NO_SUB: the kernels walk the canonical arrays
// for those.
inline void fill_second_level(HuffDevTable &dst, const HuffTable &h, int ac)
{
  int prefix_of[HUFF_DEV_SUBTABLES], used = 0;
  int code = 0, k = 0;
  for (int l = 1; l <= 16; l++) {
    for (int i = 0; i < h.counts[l - 1]; i++, code++, k++) {
      if (l <= HUFF_DEV_LOOKAHEAD || k >= 256) continue;
      if (code >= (1 << l)) return; // over-subscribed lengths: the host refuses such tables anyway
      const int prefix = code >> (l - HUFF_DEV_LOOKAHEAD), rest = l - HUFF_DEV_LOOKAHEAD; // 1..6 bits behind the prefix
      int t = 0;
      while (t < used && prefix_of[t] != prefix) t++;
      if (t == used) {
        if (used == HUFF_DEV_SUBTABLES) continue;
        prefix_of[used++] = prefix;
        dst.fast[prefix] = (uint16_t)(HUFF_DEV_SUB | t);
      }
      const uint16_t e = (uint16_t)huff_dev_entry(l, h.values[k], ac);
      const int first = (code & ((1 << rest) - 1)) << (6 - rest);
      for (int j = 0; j < (1 << (6 - rest)); j++) dst.sub[t][first + j] = e;
    }
    code <<= 1;
  }
}

// The host's decoder table in the device's form (huffman_dev.hpp): direct entries, second-level tables, the canonical arrays.
// mode: 0 DC, 1 AC of a sequential scan, 2 AC of a progressive / refinement scan (huff_dev_entry).
inline void build_dev_table(HuffDevTable &dst, const HuffTable &src, int mode)
{
  memset(&dst, 0, sizeof(dst));
  // the host's direct table ((length << 8) | symbol, 0 = a longer code or none) in the device's entry format
  for (int x = 0; x < (1 << HUFF_DEV_LOOKAHEAD); x++) {
    const uint16_t he = src.fast[x];
    dst.fast[x] = he ? (uint16_t)huff_dev_entry(he >> 8, he & 0xffu, mode) : (uint16_t)(HUFF_DEV_SUB | HUFF_DEV_NO_SUB);
  }
  static const bool no_sub = getenv("MIJPEG_HUFF_NO_SUBTABLES") != nullptr; // A-B measurements: long codes walk the canonical arrays
  if (!no_sub) fill_second_level(dst, src, mode);
  memcpy(dst.maxcode, src.maxcode, sizeof(dst.maxcode));
  memcpy(dst.valoff, src.valoff, sizeof(dst.valoff));
  memcpy(dst.values, src.values, sizeof(dst.values));
}

// ------------------------------------------------------------------------------------------------
// All scans of a file's frames (device_entropy_multiscan): the plan and the staging behind the streams
// ------------------------------------------------------------------------------------------------
// What plan and fill read of one frame (a MultiScanFrame's decoder: its info and its scans)
struct FrameScans {
  const mijpeg_info *info;
  const std::vector<Scan> *scans;
};

struct MultiscanPlan {
  // One scan of one frame: its level (scans of one level of one frame are launched side by side), its restart intervals and
  // where they begin in the interval tables, its tables (slot per scan component; table_off: bytes from the table region), its slot
  // in the stream buffer
  struct Item { int frame; size_t scan; int level; int64_t nint; size_t stream_off; size_t table_off; int ntab; int dc_tab[4], ac_tab[4]; int64_t first; };
  // The scans of one level of one frame: its workgroups are groups[g0 .. g0 + groups)
  struct Launch { int frame, level; int64_t g0, groups; };
  std::vector<Item> items;                  // frame by frame, scan by scan
  std::vector<int> frame_levels;            // levels per frame
  std::vector<size_t> level_end;            // end of level l's bytes in the stream buffer
  std::vector<std::vector<int>> level_lanes; // [frame][level]: decoding lanes per wave
  std::vector<Launch> launches;             // in launch order: frame, level (groups inside: scan)
  int64_t n_groups = 0, widest = 0, total_intervals = 0; // widest: intervals of the largest launch
  int max_tables = 1;
  size_t table_bytes = 0, stream_bytes = 0;
  int cut = 0; // levels [0, cut) are gathered and uploaded first, [cut, levels) while those run
  // behind the streams: [ibegin][iend][tables][scans][groups][status: 8 dwords per frame]; the same offsets in pinned staging
  size_t ibegin = 0, iend = 0, tables = 0, scans = 0, groups = 0, status = 0, status_bytes = 0, end = 0;
  int levels() const { return (int)level_end.size(); }
};

// The items of a plan: level, restart intervals and table slots of every scan, the levels of every frame
inline void multiscan_items(const FrameScans *frames, int nframes, MultiscanPlan &p)
{
  p.frame_levels.assign((size_t)nframes, 0);
  for (int fi = 0; fi < nframes; fi++) {
    const std::vector<Scan> &scans = *frames[fi].scans;
    std::vector<int> level(scans.size(), 0);
    for (size_t j = 0; j < scans.size(); j++) {
      const Scan &b = scans[j];
      // (a scan of the AC kind writes whole blocks back: two scans that share a component never run side by side)
      for (size_t i = 0; i < j; i++) {
        const Scan &a = scans[i];
        bool common = false;
        for (int ka = 0; ka < a.ncomp; ka++)
          for (int kb = 0; kb < b.ncomp; kb++) common |= a.sc[ka].comp == b.sc[kb].comp;
        if (common) level[j] = std::max(level[j], level[i] + 1);
      }
      MultiscanPlan::Item it;
      memset(&it, 0, sizeof(it));
      it.frame = fi;
      it.scan = j;
      it.level = level[j];
      const int64_t total_mcus = (int64_t)b.mcus_x * b.mcus_y;
      it.nint = b.restart_interval > 0 ? (total_mcus + b.restart_interval - 1) / b.restart_interval : 1;
      it.table_off = p.table_bytes;
      for (int k = 0; k < b.ncomp; k++) {
        it.dc_tab[k] = it.ac_tab[k] = 0;
        if (b.ss == 0 && b.ah == 0) it.dc_tab[k] = it.ntab++;
        if (b.se > 0) it.ac_tab[k] = it.ntab++;
      }
      p.table_bytes += (size_t)it.ntab * sizeof(HuffDevTable);
      p.max_tables = std::max(p.max_tables, it.ntab);
      it.first = p.total_intervals;
      p.total_intervals += it.nint;
      p.frame_levels[(size_t)fi] = std::max(p.frame_levels[(size_t)fi], level[j] + 1);
      p.items.push_back(it);
    }
  }
}

// nullptr, or why the frames are not decoded on the device.  min_intervals <= 0: 2048.
inline const char *plan_multiscan(const FrameScans *frames, int nframes, int min_intervals, MultiscanPlan &p)
{
  p = MultiscanPlan();
  multiscan_items(frames, nframes, p);
  // The entropy coded data lies in the upload level by level: what the first launches read goes up first, and the rest is
  // gathered and uploaded while they run (level_end[l]: end of level l's bytes).
  int n_levels = 0;
  for (int fi = 0; fi < nframes; fi++) n_levels = std::max(n_levels, p.frame_levels[(size_t)fi]);
  p.level_end.assign((size_t)n_levels, 0);
  Layout streams;
  for (int lv = 0; lv < n_levels; lv++) {
    for (MultiscanPlan::Item &it : p.items)
      if (it.level == lv) it.stream_off = streams.take((*frames[it.frame].scans)[it.scan].unstuffed_size + HUFF_STREAM_PAD);
    p.level_end[(size_t)lv] = streams.end;
  }
  p.stream_bytes = streams.end;
  if (p.stream_bytes > 0xfffffff0ull || p.total_intervals > 0x7fffffff) return "file too large for one device decode";
  // the largest launch decides whether the device is worth the trip ("auto"); every launch -- the scans of one level of one
  // frame -- picks how many lanes of a wave decode by its own number of intervals: fewer lanes = more waves, less divergence.
  // Its groups in launch order: frame, level, scan
  p.level_lanes.resize((size_t)nframes);
  for (int fi = 0; fi < nframes; fi++)
    for (int lv = 0; lv < p.frame_levels[(size_t)fi]; lv++) {
      int64_t n = 0;
      for (const MultiscanPlan::Item &it : p.items)
        if (it.frame == fi && it.level == lv) n += it.nint;
      p.widest = std::max(p.widest, n);
      const int lanes = lanes_for(n), per_group = lanes * WAVES_PER_GROUP;
      p.level_lanes[(size_t)fi].push_back(lanes);
      const int64_t g0 = p.n_groups;
      for (const MultiscanPlan::Item &it : p.items)
        if (it.frame == fi && it.level == lv) p.n_groups += (it.nint + per_group - 1) / per_group;
      if (p.n_groups > g0) p.launches.push_back(MultiscanPlan::Launch{fi, lv, g0, p.n_groups - g0});
    }
  if (min_intervals <= 0) min_intervals = 2048;
  if (p.widest < min_intervals) return "too few restart intervals to occupy the device";
  // where to cut: behind the first level that brings a quarter of the bytes (a progressive frame's DC scan alone is over before
  // anything could hide behind it); no cut when that is the last level
  p.cut = n_levels;
  for (int lv = 0; lv + 1 < n_levels; lv++)
    if (p.level_end[(size_t)lv] * 4 >= p.stream_bytes) { p.cut = lv + 1; break; }
  Layout L;
  p.ibegin = L.take((size_t)p.total_intervals * 4);
  p.iend = L.take((size_t)p.total_intervals * 4);
  p.tables = L.take(p.table_bytes);
  p.scans = L.take(p.items.size() * sizeof(ProgScanDev));
  p.groups = L.take((size_t)p.n_groups * sizeof(ProgGroup));
  p.status_bytes = (size_t)nframes * 32;
  p.status = L.take(p.status_bytes);
  p.end = L.end;
  return nullptr;
}

// Interval tables, Huffman tables, scan descriptors and workgroup lists into hp: plan.end bytes (the status words at their end are
// the device's to write)
inline void fill_multiscan(const MultiscanPlan &p, const FrameScans *frames, uint8_t *hp)
{
  uint32_t *ib = (uint32_t *)(hp + p.ibegin), *ie = (uint32_t *)(hp + p.iend);
  ProgScanDev *sd = (ProgScanDev *)(hp + p.scans);
  ProgGroup *groups = (ProgGroup *)(hp + p.groups);
  for (const MultiscanPlan::Launch &l : p.launches) {
    const int per_group = p.level_lanes[(size_t)l.frame][(size_t)l.level] * WAVES_PER_GROUP;
    int64_t g = l.g0;
    for (size_t ii = 0; ii < p.items.size(); ii++) {
      const MultiscanPlan::Item &it = p.items[ii];
      if (it.frame != l.frame || it.level != l.level) continue;
      for (int64_t k = 0; k < it.nint; k += per_group) groups[g++] = ProgGroup{(uint32_t)ii, (uint32_t)k};
    }
  }
  for (size_t ii = 0; ii < p.items.size(); ii++) {
    const MultiscanPlan::Item &it = p.items[ii];
    const mijpeg_info &f = *frames[it.frame].info;
    const Scan &s = (*frames[it.frame].scans)[it.scan];
    ProgScanDev &o = sd[ii];
    memset(&o, 0, sizeof(o));
    o.stream_off = (uint32_t)it.stream_off;
    o.first_interval = (uint32_t)it.first;
    o.n_intervals = (int32_t)it.nint;
    o.total_mcus = s.mcus_x * s.mcus_y;
    o.restart_interval = s.restart_interval > 0 ? s.restart_interval : o.total_mcus;
    o.mcus_x = s.mcus_x;
    o.ncomp = s.ncomp;
    o.ntables = it.ntab;
    o.table_off = (uint32_t)it.table_off;
    o.ss = s.ss; o.se = s.se; o.ah = s.ah; o.al = s.al;
    o.runs_legal = s.progressive_run ? 1 : 0;
    HuffDevTable *tabs = (HuffDevTable *)(hp + p.tables + it.table_off);
    for (int k = 0; k < s.ncomp; k++) {
      const int c = s.sc[k].comp;
      o.comp[k] = c;
      const McuBlocks b = mcu_blocks(f, s, k);
      o.hs[k] = b.h;
      o.vs[k] = b.v;
      o.bw[k] = f.blocks_w[c];
      o.coef_off[k] = plane_offset(f, c);
      o.dc_tab[k] = it.dc_tab[k];
      o.ac_tab[k] = it.ac_tab[k];
      if (s.ss == 0 && s.ah == 0) build_dev_table(tabs[it.dc_tab[k]], s.dc[k], 0);
      if (s.se > 0) build_dev_table(tabs[it.ac_tab[k]], s.ac[k], 2);
    }
    memcpy(ib + it.first, s.interval_ubegin.data(), (size_t)it.nint * sizeof(uint32_t)); // (multiscan_obstacle: both lists hold nint entries at least)
    memcpy(ie + it.first, s.interval_uend.data(), (size_t)it.nint * sizeof(uint32_t));
  }
}

// ------------------------------------------------------------------------------------------------
// Streams without restart markers (device_walk_images): the plan of the walk and its staging
// ------------------------------------------------------------------------------------------------
constexpr int WALK_MAX_ROUNDS = 48;

// What plan and fill read of one image of the launch (device_entropy_batch's ImagePlan and the image's MCU grid)
struct WalkImage {
  bool device_walked;     // its intervals come from this walk (the others of the launch bring no subsequences)
  bool searched_walk;     // ... behind its marker search: copy_bytes is a bound, and the fit step reads n_intervals
  int mcus_per_interval;  // MCUs per virtual interval
  size_t copy_bytes;      // the device's copy of its entropy coded data (searched_walk: the raw segment, which is no shorter)
  int64_t first_interval, n_intervals; // its entries in the launch's interval tables
  int64_t total_mcus;
};

struct WalkPlan {
  int n = 0;
  bool per_image = false; // images of different sizes: interval sizes and block counts image by image
  uint32_t sub_bytes = 0; // bytes per subsequence
  int nblk_mcu = 0;
  std::vector<uint32_t> img_sub0, img_nsub, img_e0, img_e1, img_int0; // per image: its subsequences, its segment, its first interval
  uint32_t nsub_total = 0;
  int lanes = 0;
  std::vector<uint32_t> sub_image, sub_first; // per workgroup: image and first subsequence
  int tiles = 0;         // prefix-sum tiles per image
  bool any_fit = false;  // some image is walked behind its search: the fit step runs in front of the first round
  int defer_rounds = 0;  // rounds launched in one go when nobody looks at the flags in between
  // One device buffer: [per group: image, first][per image: sub0, nsub, e0, e1, int0][per subsequence: state][per image, ragged
  // launches: blocks per interval, blocks][per image, the fit step: virtual intervals] (the host fills these; nsub and e1 of a
  // searched_walk image are bounds the fit step replaces) | up_end [changed flag per round, status per image][per subsequence: stamp]
  // (start out as zero) | zero_end [per subsequence: nblocks, dcsum, first_block, first_pred][prefix-sum tiles]
  size_t o_simg = 0, o_sfirst = 0, o_isub0 = 0, o_insub = 0, o_e0 = 0, o_e1 = 0, o_int0 = 0, o_state = 0, o_every = 0, o_blocks = 0, o_fit = 0, o_up_end = 0;
  size_t o_flags = 0, o_stamp = 0, o_zero_end = 0, o_nblk = 0, o_dcsum = 0, o_fblk = 0, o_fpred = 0, o_tiles = 0, end = 0;
  size_t flags_bytes() const { return o_stamp - o_flags; } // changed[], walk_status[]
};

// nullptr, or why the launch is not walked on the device.  nblk_mcu: blocks per MCU of the scan the images share.
inline const char *plan_walk(const WalkImage *images, int n, bool per_image, int nblk_mcu, WalkPlan &p)
{
  p = WalkPlan();
  p.n = n;
  p.per_image = per_image;
  if (nblk_mcu > 64) return "too many blocks per MCU for the device walk";
  p.nblk_mcu = nblk_mcu;
  // subsequence size.  One image: the launch is latency-bound, its serial part is (distance the decoder needs to
  // synchronise + two subsequences), so small ones.  Batches are throughput-bound and every round re-walks whole
  // subsequences, so fewer rounds over larger ones (measured on 1, 4 and 16 8K frames: 128, 256, 512 bytes win).
  size_t longest = 0, all_bytes = 0;
  for (int i = 0; i < n; i++)
    if (images[i].device_walked) {
      longest = std::max(longest, images[i].copy_bytes);
      all_bytes += images[i].copy_bytes;
    }
  uint32_t sub_bytes = all_bytes <= ((size_t)8 << 20) ? 128 : all_bytes <= ((size_t)32 << 20) ? 256 : 512;
  while (sub_bytes < 1024 && longest / sub_bytes > ((size_t)1 << 20)) sub_bytes <<= 1; // bounds the prefix-sum tiles
  if (const char *e = getenv("MIJPEG_WALK_SUB")) sub_bytes = (uint32_t)std::max(32, std::min(4096, atoi(e))); // experiments
  p.sub_bytes = sub_bytes;
  // per image: its subsequences; per workgroup: image and first subsequence
  for (std::vector<uint32_t> *v : {&p.img_sub0, &p.img_nsub, &p.img_e0, &p.img_e1, &p.img_int0}) v->assign((size_t)n, 0);
  uint32_t most = 0;
  for (int i = 0; i < n; i++) {
    p.img_e1[(size_t)i] = (uint32_t)images[i].copy_bytes;
    p.img_int0[(size_t)i] = (uint32_t)images[i].first_interval;
    p.img_sub0[(size_t)i] = p.nsub_total;
    if (images[i].device_walked) {
      p.img_nsub[(size_t)i] = (uint32_t)((images[i].copy_bytes + sub_bytes - 1) / sub_bytes);
      p.nsub_total += p.img_nsub[(size_t)i];
    }
    most = std::max(most, p.img_nsub[(size_t)i]);
    p.any_fit |= images[i].searched_walk;
  }
  p.lanes = 64;
  while (p.lanes > 1 && p.nsub_total / (uint32_t)p.lanes < 2048) p.lanes >>= 1;
  const uint32_t per_group = (uint32_t)(p.lanes * WAVES_PER_GROUP);
  for (int i = 0; i < n; i++)
    for (uint32_t k = 0; k < p.img_nsub[(size_t)i]; k += per_group) { p.sub_image.push_back((uint32_t)i); p.sub_first.push_back(k); }
  p.tiles = (int)((most + HUFF_WALK_TILE - 1) / HUFF_WALK_TILE);
  if (p.tiles > HUFF_WALK_TILE) return "stream too long for the device walk";
  // Enough rounds for the states to settle, where they are launched in one go (device_walk_images)
  p.defer_rounds = std::min(WALK_MAX_ROUNDS, sub_bytes >= 512 ? 16 : sub_bytes >= 256 ? 24 : 40);
  const size_t G = p.sub_image.size(), S = p.nsub_total, N = (size_t)n;
  Layout L;
  p.o_simg = L.take(G * 4);
  p.o_sfirst = L.take(G * 4);
  p.o_isub0 = L.take(N * 4);
  p.o_insub = L.take(N * 4);
  p.o_e0 = L.take(N * 4);
  p.o_e1 = L.take(N * 4);
  p.o_int0 = L.take(N * 4);
  p.o_state = L.take(S * 8);
  p.o_every = L.take(per_image ? N * 4 : 0);
  p.o_blocks = L.take(per_image ? N * 4 : 0);
  p.o_fit = L.take(p.any_fit ? N * 4 : 0);
  p.o_up_end = L.end;
  p.o_flags = L.take((size_t)(WALK_MAX_ROUNDS + 1) * 4 + N * 4);
  p.o_stamp = L.take(S * 4);
  p.o_zero_end = L.end;
  p.o_nblk = L.take(S * 4);
  p.o_dcsum = L.take(S * 16);
  p.o_fblk = L.take(S * 4);
  p.o_fpred = L.take(S * 16);
  p.o_tiles = L.take(N * (size_t)p.tiles * HUFF_WALK_SUMS_BYTES);
  p.end = L.end;
  return nullptr;
}

// What the host fills of the walk's buffer, into wh: plan.o_up_end bytes
inline void fill_walk(const WalkPlan &p, const WalkImage *images, uint8_t *wh)
{
  const size_t G = p.sub_image.size(), N = (size_t)p.n;
  memcpy(wh + p.o_simg, p.sub_image.data(), G * 4);
  memcpy(wh + p.o_sfirst, p.sub_first.data(), G * 4);
  memcpy(wh + p.o_isub0, p.img_sub0.data(), N * 4);
  memcpy(wh + p.o_insub, p.img_nsub.data(), N * 4);
  memcpy(wh + p.o_e0, p.img_e0.data(), N * 4);
  memcpy(wh + p.o_e1, p.img_e1.data(), N * 4);
  memcpy(wh + p.o_int0, p.img_int0.data(), N * 4);
  if (p.per_image) {
    uint32_t *every = (uint32_t *)(wh + p.o_every), *blocks = (uint32_t *)(wh + p.o_blocks);
    for (int i = 0; i < p.n; i++) {
      every[i] = (uint32_t)(std::max(1, images[i].device_walked ? images[i].mcus_per_interval : 0) * p.nblk_mcu);
      blocks[i] = (uint32_t)(images[i].total_mcus * p.nblk_mcu);
    }
  }
  // the initial guess: every subsequence starts at its boundary (behind a stuffed zero if it falls on one) with the
  // first block of an MCU; for the first subsequence of an image that is no guess
  // (positions in the device's copy, which has no byte stuffing: nothing of the stream is looked at here)
  uint64_t *st = (uint64_t *)(wh + p.o_state);
  for (int i = 0; i < p.n; i++)
    for (uint32_t k = 0; k < p.img_nsub[(size_t)i]; k++) st[p.img_sub0[(size_t)i] + k] = (uint64_t)k * p.sub_bytes;
  if (p.any_fit) {
    uint32_t *fit = (uint32_t *)(wh + p.o_fit);
    for (int i = 0; i < p.n; i++) fit[i] = images[i].searched_walk ? (uint32_t)images[i].n_intervals : 0u;
  }
}

} // namespace mij
