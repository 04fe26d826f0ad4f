// speculative_decode.cpp -- HostDecoder::decode_scan_speculative: a scan without restart markers decoded in parallel by
// self-synchronisation, and the virtual restart intervals the device decoder takes from the same walk.  Entered once per scan.
#include "block_decode.hpp"

#include <algorithm>
#include <atomic>

namespace mij {

// ------------------------------------------------------------------------------------------------
// Scans WITHOUT restart markers: self-synchronising parallel decoding.
//
// Huffman-coded JPEG data re-synchronises: a decoder started at an arbitrary bit of the stream soon reads the same
// symbols as the true one (Klein & Wiseman 2003; Weissenberger & Schmidt, "Massively Parallel Huffman Decoding on
// GPUs", ICPP 2018 / "Accelerating JPEG Decompression on GPUs", 2021).  The entropy coded segment is cut into byte
// ranges; pass 1 lets one worker per range walk its range WITHOUT storing coefficients, from a guessed state (block
// start, first block of an MCU), and log every block start as (position in the unstuffed stream, index of the block
// inside the MCU, DC difference); each worker then runs on into the next range until one of its block starts coincides
// with a logged one in position and MCU phase -- from there on the next worker's log is the truth.  A short sequential
// pass strings the valid pieces together (block numbers, DC predictors by prefix sums), and pass 2 decodes every piece
// for real, straight into the coefficient planes.  Anything unexpected (no synchronisation, a decoding error on the
// true path, a block count that does not fit) returns "not handled" and the ordinary sequential decoder takes over,
// so malformed streams keep their diagnostics.
// ------------------------------------------------------------------------------------------------
std::atomic<int64_t> g_speculative_scans{0}, g_speculative_pieces{0};

// Bytes of entropy coded data per speculative range (MIJPEG_SPEC_SEGMENT_BYTES overrides; tests use tiny ranges).
size_t spec_segment_bytes()
{
  const char *e = getenv("MIJPEG_SPEC_SEGMENT_BYTES");
  const long v = e ? atol(e) : 0;
  return v > 0 ? (size_t)v : (size_t)32 << 10;
}

struct SpecRecord {
  uint64_t pos;     // first bit of the block, in bits of the unstuffed entropy coded segment
  uint32_t raw;     // reader state at that point: offset of the next unread byte ...
  uint8_t n;        // ... and bits still buffered in front of it
  uint8_t j;        // index of the block inside its MCU (as this worker believes)
  int16_t dcdiff;
};

// One block in "walk" mode: no stores.  Returns 0, or nonzero when the data cannot be a block (speculation went wrong).
static inline int walk_block(BitReader &b, const HuffTable &dc, const HuffTable &ac, int &dcdiff)
{
  if (b.n < 32) b.refill();
  int s = decode_symbol(b, dc);
  if (s < 0 || s > 15) return 1;
  dcdiff = s ? receive_extend(b, s) : 0;
  int k = 1;
  do {
    if (b.n < 32) b.refill();
    const int rs = decode_symbol(b, ac);
    if (rs < 0) return 1;
    const int r = rs >> 4;
    s = rs & 15;
    if (s == 0) {
      if (r == 15) { k += 16; continue; }
      if (r == 0) break;
      return 1;
    }
    k += r;
    b.skip(s);
    if (k >= 64) return 1;
    k++;
  } while (k <= 63);
  return 0;
}

// A reader positioned where `rec` was logged: step back over the bytes whose bits were still buffered (a zero byte
// behind 0xFF is always a stuffed one inside entropy coded data), then drop the bits that had been consumed.
static inline BitReader reader_at(const uint8_t *base, const uint8_t *lo, const uint8_t *end, uint32_t raw, int n)
{
  const uint8_t *q = base + raw;
  const int back = (n + 7) >> 3;
  for (int i = 0; i < back; i++) {
    q--;
    if (q > lo && q[0] == 0x00 && q[-1] == 0xff) q--;
  }
  BitReader b(q, end);
  b.refill();
  b.skip(8 * back - n);
  return b;
}

template <class T>
int HostDecoder::decode_scan_speculative(T *coef, const Scan &s, int threads, uint32_t (&qmax_out)[MIJPEG_MAX_COMPONENTS],
                                         VirtualIntervals *plan_only, bool first_pass)
{
  const uint8_t *base = s.base ? s.base : data_;
  const uint8_t *lo = base + s.ecs_begin, *hi = base + s.ecs_end;
  const int64_t total_mcus = (int64_t)s.mcus_x * s.mcus_y;
  // blocks of one MCU: component (scan index) and offset inside the MCU
  int B = 0, bk[64], bbx[64], bby[64]; // up to four components of 4 x 4 blocks
  for (int k = 0; k < s.ncomp; k++) {
    const int c = s.sc[k].comp;
    const int h = s.ncomp > 1 ? info.hsamp[c] : 1, v = s.ncomp > 1 ? info.vsamp[c] : 1;
    for (int by = 0; by < v; by++)
      for (int bx = 0; bx < h; bx++) {
        if (B == 64) return 1;
        bk[B] = k; bbx[B] = bx; bby[B] = by;
        B++;
      }
  }
  const int64_t total_blocks = total_mcus * B;
  const size_t seg_bytes = spec_segment_bytes();
  const size_t len = (size_t)(hi - lo);
  int G = (int)std::min<size_t>((size_t)threads * 4, len / std::max<size_t>(seg_bytes, 64));
  if (G < 2) return 1;
  // range starts; never between 0xFF and its stuffed zero
  std::vector<const uint8_t *> start((size_t)G + 1);
  for (int i = 0; i <= G; i++) {
    const uint8_t *q = lo + len * (size_t)i / (size_t)G;
    if (i > 0 && i < G && q[-1] == 0xff && q[0] == 0x00) q++;
    start[(size_t)i] = q;
  }
  start[(size_t)G] = hi;
  // stuffed zeros in front of every range: positions are counted in the unstuffed stream
  std::vector<uint64_t> stuffed_before((size_t)G + 1, 0);
  {
    std::vector<uint64_t> cnt((size_t)G, 0);
    parallel_for(std::min(G, threads), [&](int w) {
      for (int i = w; i < G; i += std::min(G, threads)) {
        uint64_t c = 0;
        const uint8_t *q = start[(size_t)i], *e = start[(size_t)i + 1];
        while (q < e && (q = (const uint8_t *)memchr(q, 0xff, (size_t)(e - q)))) {
          if (q + 1 < hi && q[1] == 0x00) { c++; q += 2; }
          else q++;
        }
        cnt[(size_t)i] = c;
      }
    });
    for (int i = 0; i < G; i++) stuffed_before[(size_t)i + 1] = stuffed_before[(size_t)i] + cnt[(size_t)i];
  }
  auto position = [&](const BitReader &b, int seg_of_reader_start) -> uint64_t {
    // unstuffed bytes in front of b.p, minus the stream bits still buffered
    const uint64_t bytes = (uint64_t)(b.p - lo) - (stuffed_before[(size_t)seg_of_reader_start] + b.stuffed);
    return bytes * 8 - (uint64_t)b.real_bits();
  };
  struct Segment {
    std::vector<SpecRecord> rec;  // own range
    std::vector<SpecRecord> over; // blocks walked beyond the own range until the next log was met
    BitReader tail{nullptr, nullptr};
    int tail_j = 0;
    bool tail_ok = false; // walked to the end of the own range
    int sync_seg = -1;    // first following range whose log was met ...
    int64_t sync_idx = -1; // ... at this record
    bool reached_end = false; // the walk ran into the end of the data
  };
  std::vector<Segment> seg((size_t)G);
  const int workers = std::min(G, threads);

  // ---- pass 1a: walk the own range
  parallel_for(workers, [&](int w) {
    for (int i = w; i < G; i += workers) {
      Segment &sg = seg[(size_t)i];
      sg.rec.reserve((size_t)(start[(size_t)i + 1] - start[(size_t)i]) / 6 + 16);
      BitReader b(start[(size_t)i], hi);
      const uint64_t limit = ((uint64_t)(start[(size_t)i + 1] - lo) - stuffed_before[(size_t)i + 1]) * 8;
      int j = 0;
      for (;;) {
        if (b.n < 32) b.refill();
        const uint64_t pos = position(b, i);
        if (pos >= limit || (b.parked && b.real_bits() <= 0)) break;
        SpecRecord r;
        r.pos = pos;
        r.raw = (uint32_t)(b.p - base);
        r.n = (uint8_t)b.n;
        r.j = (uint8_t)j;
        int dcdiff = 0;
        const int bad = walk_block(b, s.dc[bk[j]], s.ac[bk[j]], dcdiff);
        if (b.parked && b.real_bits() < 0) { sg.reached_end = true; break; } // ran over the end of the data inside a block
        if (bad) { // not a block: move on by one bit and guess again
          if (b.n < 8) b.refill();
          b.skip(1);
          j = 0;
          continue;
        }
        r.dcdiff = (int16_t)dcdiff;
        if (dcdiff != r.dcdiff) { j = 0; continue; }
        sg.rec.push_back(r);
        j = j + 1 == B ? 0 : j + 1;
      }
      sg.tail = b;
      sg.tail_j = j;
      sg.tail_ok = true;
    }
  });

  // ---- pass 1b: walk on into the following ranges until a logged block start is met
  parallel_for(workers, [&](int w) {
    for (int i = w; i + 1 < G; i += workers) {
      Segment &sg = seg[(size_t)i];
      if (sg.reached_end) continue;
      BitReader b = sg.tail;
      int j = sg.tail_j;
      int t = i + 1;
      size_t ti = 0;
      for (;;) {
        if (b.n < 32) b.refill();
        if (b.parked && b.real_bits() <= 0) { sg.reached_end = true; break; }
        const uint64_t pos = position(b, i);
        // the range this position lies in
        while (t < G) {
          const uint64_t tl = ((uint64_t)(start[(size_t)t + 1] - lo) - stuffed_before[(size_t)t + 1]) * 8;
          if (pos < tl) break;
          t++;
          ti = 0;
        }
        if (t == G) { sg.reached_end = true; break; }
        const std::vector<SpecRecord> &tr = seg[(size_t)t].rec;
        while (ti < tr.size() && tr[ti].pos < pos) ti++;
        if (ti < tr.size() && tr[ti].pos == pos && tr[ti].j == j) {
          sg.sync_seg = t;
          sg.sync_idx = (int64_t)ti;
          break;
        }
        SpecRecord r;
        r.pos = pos;
        r.raw = (uint32_t)(b.p - base);
        r.n = (uint8_t)b.n;
        r.j = (uint8_t)j;
        int dcdiff = 0;
        if (walk_block(b, s.dc[bk[j]], s.ac[bk[j]], dcdiff) || (b.parked && b.real_bits() < 0)) { sg.reached_end = true; break; }
        r.dcdiff = (int16_t)dcdiff;
        if (dcdiff != r.dcdiff) { sg.reached_end = true; break; }
        sg.over.push_back(r);
        j = j + 1 == B ? 0 : j + 1;
      }
    }
  });

  // ---- stitch: the true path starts with range 0 and hops along the synchronisation points
  struct Piece {
    int seg;
    int64_t first;      // first valid record of the range's own log
    int64_t nblocks;    // own records from `first` + overflow records
    int64_t g0;         // global number of its first block
    int pred[MIJPEG_MAX_COMPONENTS];
  };
  std::vector<Piece> pieces;
  {
    int cur = 0;
    int64_t first = 0, g = 0;
    while (g < total_blocks) {
      const Segment &sg = seg[(size_t)cur];
      if (cur != 0 && (first >= (int64_t)sg.rec.size() || sg.rec[(size_t)first].j != (uint8_t)(g % B))) return 1; // MCU phase must agree with the block count
      Piece pc;
      pc.seg = cur;
      pc.first = first;
      pc.nblocks = (int64_t)sg.rec.size() - first + (int64_t)sg.over.size();
      pc.g0 = g;
      memset(pc.pred, 0, sizeof(pc.pred));
      pieces.push_back(pc);
      g += pc.nblocks;
      if (g >= total_blocks) break;
      if (sg.sync_seg < 0) return 1; // neither synchronised nor complete
      cur = sg.sync_seg;
      first = sg.sync_idx;
    }
    if (g < total_blocks) return 1;
    pieces.back().nblocks -= g - total_blocks; // the last piece may have walked into the padding / following marker
    if (pieces.back().nblocks <= 0) return 1;
  }
  auto record_of = [&](const Piece &pc, int64_t i) -> const SpecRecord & {
    const Segment &sg = seg[(size_t)pc.seg];
    const int64_t own = (int64_t)sg.rec.size() - pc.first;
    return i < own ? sg.rec[(size_t)(pc.first + i)] : sg.over[(size_t)(i - own)];
  };
  // DC predictors at the start of every piece: per-piece sums of the differences, then a prefix sum
  {
    std::vector<std::array<int64_t, MIJPEG_MAX_COMPONENTS>> sums(pieces.size());
    const int np = (int)pieces.size();
    parallel_for(std::min(np, threads), [&](int w) {
      for (int pi = w; pi < np; pi += std::min(np, threads)) {
        const Piece &pc = pieces[(size_t)pi];
        std::array<int64_t, MIJPEG_MAX_COMPONENTS> a{};
        for (int64_t i = 0; i < pc.nblocks; i++) {
          const SpecRecord &r = record_of(pc, i);
          a[(size_t)bk[r.j]] += r.dcdiff;
        }
        sums[(size_t)pi] = a;
      }
    });
    int64_t run[MIJPEG_MAX_COMPONENTS] = {0, 0, 0, 0};
    for (size_t pi = 0; pi < pieces.size(); pi++) {
      for (int k = 0; k < MIJPEG_MAX_COMPONENTS; k++) {
        if (run[k] != (int)run[k]) return 1;
        pieces[pi].pred[k] = (int)run[k];
        run[k] += sums[pi][(size_t)k];
      }
    }
  }

  if (plan_only) {
    // ---- instead of pass 2: restart points every mcus_per_interval MCUs for the device decoder
    const int64_t per = (int64_t)plan_only->mcus_per_interval * B;
    if (per <= 0) return 1;
    const int64_t nint = (total_blocks + per - 1) / per;
    plan_only->byte_off.assign((size_t)nint, 0);
    plan_only->bit_skip.assign((size_t)nint, 0);
    plan_only->pred.assign((size_t)nint * 4, 0);
    std::atomic<int> bad{0};
    const int np = (int)pieces.size(), nw = std::min(np, threads);
    parallel_for(nw, [&](int w) {
      for (int pi = w; pi < np; pi += nw) {
        const Piece &pc = pieces[(size_t)pi];
        int64_t run[MIJPEG_MAX_COMPONENTS];
        for (int k = 0; k < MIJPEG_MAX_COMPONENTS; k++) run[k] = pc.pred[k];
        for (int64_t i = 0; i < pc.nblocks; i++) {
          const int64_t g = pc.g0 + i;
          const SpecRecord &r = record_of(pc, i);
          if (g % per == 0) {
            const size_t idx = (size_t)(g / per);
            if (g == 0) {
              plan_only->byte_off[idx] = (uint32_t)s.ecs_begin;
            } else { // step back over the bytes whose bits were still buffered (see reader_at)
              const uint8_t *q = base + r.raw;
              const int back = (r.n + 7) >> 3;
              for (int b = 0; b < back; b++) {
                q--;
                if (q > lo && q[0] == 0x00 && q[-1] == 0xff) q--;
              }
              plan_only->byte_off[idx] = (uint32_t)(q - base);
              plan_only->bit_skip[idx] = (uint8_t)(8 * back - r.n);
            }
            for (int k = 0; k < MIJPEG_MAX_COMPONENTS; k++) {
              if (run[k] != (int16_t)run[k]) bad.store(1);
              plan_only->pred[idx * 4 + (size_t)k] = (int16_t)run[k];
            }
          }
          run[bk[r.j]] += r.dcdiff;
        }
      }
    });
    return bad.load() ? 1 : 0;
  }

  // ---- pass 2: decode every piece for real
  const uint8_t *zz = scan_order();
  std::atomic<int> failed{0};
  std::atomic<uint32_t> qm[MIJPEG_MAX_COMPONENTS];
  for (auto &q : qm) q.store(0);
  const int np = (int)pieces.size();
  std::atomic<int> next{0};
  parallel_for(std::min(np, threads), [&](int) {
    uint32_t qmax[MIJPEG_MAX_COMPONENTS] = {0, 0, 0, 0};
    for (;;) {
      const int pi = next.fetch_add(1);
      if (pi >= np || failed.load(std::memory_order_relaxed)) break;
      const Piece &pc = pieces[(size_t)pi];
      const SpecRecord &r0 = record_of(pc, 0);
      BitReader b = (pc.seg == 0 && pc.first == 0) ? BitReader(lo, hi) : reader_at(base, lo, hi, r0.raw, r0.n);
      int pred[MIJPEG_MAX_COMPONENTS];
      for (int k = 0; k < MIJPEG_MAX_COMPONENTS; k++) pred[k] = pc.pred[k];
      int64_t m = pc.g0 / B;
      int j = (int)(pc.g0 - m * B);
      int my = (int)(m / s.mcus_x), mx = (int)(m - (int64_t)my * s.mcus_x);
      for (int64_t i = 0; i < pc.nblocks; i++) {
        const int k = bk[j], c = s.sc[k].comp;
        const int h = s.ncomp > 1 ? info.hsamp[c] : 1, v = s.ncomp > 1 ? info.vsamp[c] : 1;
        T *blk = coef + plane_offset_[c] + ((int64_t)(my * v + bby[j]) * info.blocks_w[c] + (mx * h + bbx[j])) * 64;
        int bad;
        if (first_pass) { // a full-band first pass of a frame whose scans accumulate (point transform s.al): see FrameDecode::first_full_band_pass
          int eob_run = 0;
          memset(blk, 0, 64 * sizeof(T));
          bad = decode_block_first<T>(b, s.dc[k], s.ac[k], pred[k], blk, zz, 0, 63, s.al, eob_run) || eob_run;
        } else
          bad = decode_block_seq(b, s.dc[k], s.ac[k], pred[k], blk, info.quant[info.quant_index[c]], zz, qmax[c]);
        if (bad) {
          failed.store(1);
          break;
        }
        if (++j == B) {
          j = 0;
          if (++mx == s.mcus_x) { mx = 0; my++; }
        }
      }
      if (b.n < b.phantom) failed.store(1); // decoded only by reading beyond the data: the sequential walk decides
    }
    for (int c = 0; c < MIJPEG_MAX_COMPONENTS; c++) {
      uint32_t cur = qm[c].load(std::memory_order_relaxed);
      while (qmax[c] > cur && !qm[c].compare_exchange_weak(cur, qmax[c], std::memory_order_relaxed)) {}
    }
  });
  if (failed.load()) return 1; // the sequential decoder finds and reports what is wrong
  for (int c = 0; c < MIJPEG_MAX_COMPONENTS; c++) qmax_out[c] = std::max(qmax_out[c], qm[c].load());
  g_speculative_scans.fetch_add(1);
  g_speculative_pieces.fetch_add((int64_t)pieces.size());
  return 0;
}
// (host_decoder.cpp's scan loop calls both)
template int HostDecoder::decode_scan_speculative<int16_t>(int16_t *, const Scan &, int, uint32_t (&)[MIJPEG_MAX_COMPONENTS], VirtualIntervals *, bool);
template int HostDecoder::decode_scan_speculative<int32_t>(int32_t *, const Scan &, int, uint32_t (&)[MIJPEG_MAX_COMPONENTS], VirtualIntervals *, bool);

int HostDecoder::plan_virtual_intervals(size_t scan, int mcus_per_interval, int threads, VirtualIntervals &out)
{
  if (scan >= scans.size() || info.progressive || has_hidden_scans() || mcus_per_interval < 1) return 1;
  const Scan &s = scans[scan];
  if (s.ss != 0 || s.se != 63 || s.ah != 0 || s.al != 0) return 1;
  if (threads <= 0) threads = default_threads();
  out.mcus_per_interval = mcus_per_interval;
  uint32_t qm[MIJPEG_MAX_COMPONENTS] = {0, 0, 0, 0};
  return decode_scan_speculative<int16_t>(nullptr, s, std::max(2, threads), qm, &out);
}

} // namespace mij
