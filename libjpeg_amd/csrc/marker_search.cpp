// marker_search.cpp -- HostDecoder's search of an entropy coded segment for its markers (AVX2 where the CPU has it): the restart
// intervals of a scan, the end of a segment, and the copy of the data without its byte stuffing that the device decoder reads.
// Called once per scan or per piece, never from a block loop.
#include "host_decoder.hpp"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace mij {

// Markers inside [a, b) of the stream: RSTn positions/codes in order; `term` = position of the first marker that ends
// the entropy coded segment (or the stream size when the data runs out), SIZE_MAX if the range holds none.
// Along the way: stuffed pairs (FF 00) and the first fill byte (an FF in front of another FF: the bit reader stops there) since
// the previous event -- what unstuffed_layout needs to know how many bytes every interval keeps.
struct MarkerEvents {
  struct Rst {
    size_t first;  // position of the marker's FF
    uint8_t second; // its code
    uint32_t pairs; // stuffed pairs since the previous marker (or the start of the range) ...
    size_t cut;     // ... and the first fill byte there (SIZE_MAX: none); pairs behind it are not counted
    Rst() {} // (nothing: RstAppender opens the list to its capacity and writes what counts)
    Rst(size_t f, uint8_t s, uint32_t p, size_t c) : first(f), second(s), pairs(p), cut(c) {}
  };
  std::vector<Rst> rst;
  size_t term = SIZE_MAX;
  uint32_t tail_pairs = 0; // behind the last marker of the range
  size_t tail_cut = SIZE_MAX;
};

// Copy [src, lim) to dst up to (not including) the first 0xFF; returns the number of bytes copied.  dst may be written up to 31
// bytes beyond what counts (the callers' destinations have that slack: a slot is as large as its stream plus the pad, and the
// copy never gets ahead of the source); nothing is read beyond `readable`.
#if defined(__x86_64__)
__attribute__((target("avx2"))) static size_t copy_until_ff_avx2(const uint8_t *src, const uint8_t *lim, const uint8_t *readable, uint8_t *dst)
{
  const __m256i ff = _mm256_set1_epi8((char)0xff);
  size_t i = 0;
  const size_t n = (size_t)(lim - src), safe = (size_t)(readable - src);
  while (i + 32 <= safe && i < n) {
    const __m256i v = _mm256_loadu_si256((const __m256i *)(src + i));
    const unsigned m = (unsigned)_mm256_movemask_epi8(_mm256_cmpeq_epi8(v, ff));
    _mm256_storeu_si256((__m256i *)(dst + i), v);
    if (m) {
      i += (size_t)__builtin_ctz(m);
      return i < n ? i : n;
    }
    i += 32;
  }
  if (i > n) return n;
  while (i < n && src[i] != 0xff) { dst[i] = src[i]; i++; }
  return i;
}
#endif
static size_t copy_until_ff(const uint8_t *src, const uint8_t *lim, const uint8_t *readable, uint8_t *dst)
{
#if defined(__x86_64__)
  static const bool avx2 = __builtin_cpu_supports("avx2");
  if (avx2) return copy_until_ff_avx2(src, lim, readable, dst);
#endif
  (void)readable;
  const uint8_t *f = (const uint8_t *)memchr(src, 0xff, (size_t)(lim - src));
  const size_t n = f ? (size_t)(f - src) : (size_t)(lim - src);
  memcpy(dst, src, n);
  return n;
}

#if defined(__x86_64__)
// The search without a sink on 32 bytes at a time: every 0xFF of the range is an event -- a stuffed pair, a fill byte, a restart
// marker or the marker that ends the segment, by the byte behind it -- and with restart intervals of a few blocks (the
// refinement scans of `-z 8` files: a marker every twenty bytes) a library call per event is what the search costs.  Returns the
// position it stopped at (b, or short of it: the scalar loop takes the rest), or SIZE_MAX when the range is finished.
// Events appended through a plain pointer: a push_back per marker on a vector behind a reference reloads and stores the
// vector's own three pointers every time (the stores into the list may alias them, for all the compiler knows) -- measured on the
// merge of these lists, where it was most of 6-15 ns per marker.  The vector is opened to its capacity, written, and closed at
// the number of entries when the appender goes.
struct RstAppender {
  std::vector<MarkerEvents::Rst> &v;
  MarkerEvents::Rst *w, *lim;
  explicit RstAppender(std::vector<MarkerEvents::Rst> &vec) : v(vec)
  {
    const size_t n = v.size();
    if (v.capacity() < n + 64) v.reserve(std::max<size_t>(2 * v.capacity(), n + 64));
    v.resize(v.capacity());
    w = v.data() + n;
    lim = v.data() + v.size();
  }
  ~RstAppender() { v.resize((size_t)(w - v.data())); }
  inline void push(const MarkerEvents::Rst &r)
  {
    if (__builtin_expect(w == lim, 0)) {
      const size_t n = (size_t)(w - v.data());
      v.resize(2 * v.size());
      w = v.data() + n;
      lim = v.data() + v.size();
    }
    *w++ = r;
  }
};

__attribute__((target("avx2"))) static size_t scan_markers_avx2(const uint8_t *base, size_t size, size_t a, size_t b, MarkerEvents &out, uint32_t &pairs_io,
                                                                size_t &cut_io)
{
  const __m256i ff = _mm256_set1_epi8((char)0xff);
  size_t i = a;
  RstAppender app(out.rst);
  uint32_t pairs = pairs_io; // (in registers while the loop runs)
  size_t cut = cut_io;
  while (i + 32 <= b && i + 33 <= size) {
    unsigned m = (unsigned)_mm256_movemask_epi8(_mm256_cmpeq_epi8(_mm256_loadu_si256((const __m256i *)(base + i)), ff));
    while (m) {
      const size_t pos = i + (size_t)__builtin_ctz(m);
      m &= m - 1;
      const uint8_t nx = base[pos + 1];
      if (nx == 0x00) {
        if (cut == SIZE_MAX) pairs++;
      } else if (nx == 0xff) {
        if (cut == SIZE_MAX) cut = pos;
      } else if (nx >= 0xd0 && nx <= 0xd7) {
        app.push(MarkerEvents::Rst{pos, nx, pairs, cut});
        pairs = 0;
        cut = SIZE_MAX;
      } else {
        out.term = pos;
        pairs_io = pairs;
        cut_io = cut;
        return SIZE_MAX;
      }
    }
    i += 32;
  }
  pairs_io = pairs;
  cut_io = cut;
  return i;
}
#endif

#if defined(__x86_64__)
// ... and the search WITH a sink (a batch's workers: one stream each, the device's copy of the entropy coded data written on the way):
// 32 bytes are copied and looked at per step, an event is handled where it is found -- no call per run between two 0xFF bytes.
// A 4K frame with restart intervals of 8 MCUs has one every 150 bytes, and under a container's CPU quota the cycles of these
// workers are what a pipeline of batches waits for (config 4, profiles/r06/batch4k_host.txt).  Stops at the first fill byte
// (an FF in front of an FF: rare) or 32 bytes in front of the range's end; returns the position, `o` moved along.
__attribute__((target("avx2"))) static size_t scan_copy_avx2(const uint8_t *base, size_t size, size_t a, size_t b, MarkerEvents &out, uint32_t &pairs_io,
                                                             uint8_t *&o)
{
  const __m256i ff = _mm256_set1_epi8((char)0xff);
  size_t p = a;
  uint8_t *d = o;
  RstAppender app(out.rst);
  uint32_t pairs = pairs_io;
  while (p + 32 <= b && p + 33 <= size) {
    const __m256i v = _mm256_loadu_si256((const __m256i *)(base + p));
    _mm256_storeu_si256((__m256i *)d, v);
    const unsigned m = (unsigned)_mm256_movemask_epi8(_mm256_cmpeq_epi8(v, ff));
    if (!m) {
      p += 32;
      d += 32;
      continue;
    }
    const unsigned j = (unsigned)__builtin_ctz(m);
    p += j;
    d += j; // (the bytes in front of the FF are in place; what the store wrote behind them is overwritten by the next one)
    const uint8_t nx = base[p + 1];
    if (nx == 0x00) {
      pairs++;
      *d++ = 0xff;
      p += 2;
    } else if (nx >= 0xd0 && nx <= 0xd7) {
      app.push(MarkerEvents::Rst{p, nx, pairs, SIZE_MAX});
      pairs = 0;
      p += 2;
    } else
      break; // a fill byte or the marker that ends the segment: the caller's loop knows what to do
  }
  o = d;
  pairs_io = pairs;
  return p;
}
#endif

// Where the entropy coded segment that starts at `from` ends: the position of the first 0xFF that is followed by neither 0x00
// (stuffing), 0xFF (it is a fill byte then) nor RSTn -- or `size`.  Nothing is recorded: this is what a planning walk needs to
// know to go on behind a scan, the restart markers of the scan are searched for later, side by side with the other scans'
// (progressive frames: HostDecoder::run_deferred_searches).
#if defined(__x86_64__)
__attribute__((target("avx2"))) static size_t segment_end_avx2(const uint8_t *base, size_t size, size_t from)
{
  const __m256i ff = _mm256_set1_epi8((char)0xff);
  size_t i = from;
  while (i + 33 <= size) {
    unsigned m = (unsigned)_mm256_movemask_epi8(_mm256_cmpeq_epi8(_mm256_loadu_si256((const __m256i *)(base + i)), ff));
    while (m) {
      const size_t pos = i + (size_t)__builtin_ctz(m);
      m &= m - 1;
      const uint8_t nx = base[pos + 1];
      if (nx != 0x00 && nx != 0xff && !(nx >= 0xd0 && nx <= 0xd7)) return pos;
    }
    i += 32;
  }
  return i;
}
#endif
static size_t find_segment_end(const uint8_t *base, size_t size, size_t from)
{
  size_t p = from;
#if defined(__x86_64__)
  static const bool avx2 = __builtin_cpu_supports("avx2");
  if (avx2) {
    p = segment_end_avx2(base, size, from);
    if (p + 33 <= size) return p; // (found inside the vector loop)
  }
#endif
  while (p < size) {
    const uint8_t *f = (const uint8_t *)memchr(base + p, 0xff, size - p);
    if (!f) return size;
    p = (size_t)(f - base);
    if (p + 1 >= size) return size; // a lone FF in front of the end: no marker, the data ran out
    const uint8_t nx = base[p + 1];
    if (nx != 0x00 && nx != 0xff && !(nx >= 0xd0 && nx <= 0xd7)) return p;
    p += nx == 0xff ? 1 : 2;
  }
  return size;
}

// Where the entropy coded segment that starts at `from` ends, for the planning walk over a progressive frame (one call per scan,
// each of which walks its scan's bytes on the calling thread): in a large file the FIRST call has the pool look at everything
// from there to the end of the file once -- every 0xFF whose next byte says "marker that ends a segment" is noted, whatever it
// stands in, a handful per file -- and the calls are look-ups in that list from then on (what lies in front of a scan's first
// byte is never asked for).  MIJPEG_NO_TERM_INDEX=1: every call walks (A-B comparisons).
size_t HostDecoder::segment_end(const uint8_t *base, size_t size, size_t from)
{
  static const bool off = getenv("MIJPEG_NO_TERM_INDEX") != nullptr;
  const int lanes = std::min(default_threads(), 16);
  if (term_base_ != base || term_size_ != size || from < term_from_) {
    if (off || lanes < 2 || size - from < ((size_t)2 << 20)) return find_segment_end(base, size, from);
    term_base_ = base;
    term_size_ = size;
    term_from_ = from;
    const size_t span = (size - from + (size_t)lanes - 1) / (size_t)lanes;
    std::vector<std::vector<size_t>> found((size_t)lanes);
    parallel_for(lanes, [&](int i) {
      const size_t a = from + (size_t)i * span, b = std::min(size, a + span);
      std::vector<size_t> &out = found[(size_t)i];
      const size_t lim = std::min(size, b + 1); // (the byte behind the chunk's last one says what an FF there is)
      for (size_t p = a; p < b;) {
        const size_t q = find_segment_end(base, lim, p);
        if (q >= b) break;
        out.push_back(q);
        p = q + 1;
      }
    });
    term_pos_.clear();
    for (const auto &v : found) term_pos_.insert(term_pos_.end(), v.begin(), v.end());
  }
  const auto it = std::lower_bound(term_pos_.begin(), term_pos_.end(), from);
  return it == term_pos_.end() ? size : *it;
}

// With `sink`: the entropy coded data without stuffing and markers is written there along the way (what unstuff_run produces).
static void scan_markers(const uint8_t *base, size_t size, size_t a, size_t b, MarkerEvents &out, uint8_t *sink = nullptr)
{
  const uint8_t *end = base + size, *lim = base + b, *p = base + a;
  uint32_t pairs = 0;
  size_t cut = SIZE_MAX;
#if defined(__x86_64__)
  static const bool avx2 = __builtin_cpu_supports("avx2");
  if (!sink && avx2) {
    const size_t at = scan_markers_avx2(base, size, a, b, out, pairs, cut);
    if (at == SIZE_MAX) {
      out.tail_pairs = pairs;
      out.tail_cut = cut;
      return;
    }
    p = base + at;
  }
#endif
  if (sink) { // the same walk, copying the runs between the FFs (one worker, the whole segment)
    uint8_t *o = sink;
#if defined(__x86_64__)
    if (avx2) p = base + scan_copy_avx2(base, size, a, b, out, pairs, o);
#endif
    while (p < lim) {
      if (cut == SIZE_MAX) { // copy up to the next FF
        const size_t k = copy_until_ff(p, lim, end, o);
        o += k;
        p += k;
        if (p >= lim) break;
      } else { // behind a fill byte nothing counts until the next marker
        p = (const uint8_t *)memchr(p, 0xff, (size_t)(lim - p));
        if (!p) break;
      }
      if (p + 1 >= end) {
        out.term = size;
        if (cut == SIZE_MAX) cut = (size_t)(p - base);
        break;
      }
      const uint8_t m = p[1];
      if (m == 0x00) {
        if (cut == SIZE_MAX) { pairs++; *o++ = 0xff; }
        p += 2;
      } else if (m == 0xff) {
        if (cut == SIZE_MAX) cut = (size_t)(p - base);
        p += 1;
      } else if (m >= 0xd0 && m <= 0xd7) {
        out.rst.push_back(MarkerEvents::Rst{(size_t)(p - base), m, pairs, cut});
        pairs = 0;
        cut = SIZE_MAX;
        p += 2;
      } else {
        out.term = (size_t)(p - base);
        break;
      }
    }
    out.tail_pairs = pairs;
    out.tail_cut = cut;
    return;
  }
  while (p < lim) {
    p = (const uint8_t *)memchr(p, 0xff, (size_t)(lim - p));
    if (!p) break;
    if (p + 1 >= end) {
      out.term = size;
      if (cut == SIZE_MAX) cut = (size_t)(p - base); // a lone FF in front of the end: no data byte either
      break;
    }
    const uint8_t m = p[1];
    if (m == 0x00) {
      if (cut == SIZE_MAX) pairs++;
      p += 2;
      continue;
    }
    if (m == 0xff) { // fill byte: the marker (if any) starts at the last FF
      if (cut == SIZE_MAX) cut = (size_t)(p - base);
      p += 1;
      continue;
    }
    if (m >= 0xd0 && m <= 0xd7) {
      out.rst.push_back(MarkerEvents::Rst{(size_t)(p - base), m, pairs, cut});
      pairs = 0;
      cut = SIZE_MAX;
      p += 2;
      continue;
    }
    out.term = (size_t)(p - base); // some other marker: end of the scan
    break;
  }
  out.tail_pairs = pairs;
  out.tail_cut = cut;
}

void HostDecoder::find_intervals(Scan &s)
{
  find_intervals_in(s, data_, size_, interval_end_, rst_code_, true);
}

// (no member of the object is written: the hidden refinement scans of a frame are searched side by side, add_hidden_scans)
void HostDecoder::find_intervals_in(Scan &s, const uint8_t *data, size_t size, std::vector<size_t> &interval_end_out, std::vector<uint8_t> &rst_code_out,
                                    bool may_sink)
{
  // The lists grow in vectors of THIS thread's frame and change places with the scan's when the search is through: the scans of
  // a file are searched side by side (run_deferred_searches), their Scan objects and the entries of scan_interval_end_ /
  // scan_rst_code_ lie next to one another, and a push_back per marker into them is a write to a cache line that the thread
  // of the next scan writes as well -- 15-27 ns per marker measured on the GPU box's host (65 000 markers in a scan of an 8K
  // progressive picture: the searches took 2 ms of a 3 ms parse, the search proper 0.25 ms of them).
  std::vector<size_t> ibegin, interval_end;
  std::vector<uint32_t> iulen;
  std::vector<uint8_t> rst_code;
  std::vector<Scan::StuffCheckpoint> ckpt;
  ibegin.swap(s.interval_begin); // (what they hold from an earlier search is kept as capacity)
  iulen.swap(s.interval_ulen);
  ckpt.swap(s.stuff_ckpt);
  interval_end.swap(interval_end_out);
  rst_code.swap(rst_code_out);
  // Entropy coded segment: runs to the first marker that is neither a stuffed FF00, a fill FF nor RSTn.  An interval
  // ends where the marker (incl. leading fill bytes) starts: the bit reader stops at any FF that is not followed by
  // 00 anyway.  Large streams are searched in rounds of parallel chunks (a byte pair is only ever interpreted from
  // its FF, so chunks can be cut anywhere); the search of a round that lies beyond the end of the scan is wasted.
  ibegin.clear();
  iulen.clear();
  ckpt.clear();
  interval_end.clear();
  rst_code.clear();
  // (the scan header says how many restart intervals to expect: no vector grows while the markers come in)
  size_t expect = 1;
  if (s.restart_interval > 0) expect = (size_t)std::min<int64_t>(((int64_t)s.mcus_x * s.mcus_y + s.restart_interval - 1) / s.restart_interval, (int64_t)(size / 2 + 1));
  ibegin.reserve(expect + 1);
  iulen.reserve(expect + 1);
  interval_end.reserve(expect + 1);
  rst_code.reserve(expect + 1);
  ibegin.push_back(s.ecs_begin);
  uint32_t acc_pairs = 0;    // stuffed pairs of the open interval so far ...
  size_t acc_cut = SIZE_MAX; // ... and its first fill byte
  auto close_interval = [&](size_t end_pos) { // the open interval ends at end_pos (a marker, or the end of the data)
    const size_t eff = std::min(acc_cut, end_pos);
    iulen.push_back((uint32_t)(eff - ibegin.back() - acc_pairs));
    acc_pairs = 0;
    acc_cut = SIZE_MAX;
  };
  // 16 searchers at most (waking more costs more than it saves: 0.53 ms serial, 0.10 ms with 16 on an 8K frame),
  // one round for typical frames, chunks of at most 1 MiB so that little is wasted beyond the end of a short scan
  // (MIJPEG_MARKER_CHUNK: tests make the chunks tiny so that small streams exercise the seams)
  static const size_t chunk_env = getenv("MIJPEG_MARKER_CHUNK") ? (size_t)std::max(16, atoi(getenv("MIJPEG_MARKER_CHUNK"))) : 0;
  const size_t min_chunk = chunk_env ? chunk_env : (size_t)256 << 10, max_chunk = chunk_env ? chunk_env : (size_t)1 << 20;
  int lanes = size - s.ecs_begin >= 4 * min_chunk ? std::min(std::max(default_threads(), chunk_env ? 4 : 1), 16) : 1;
  // a batch's worker walks its stream alone and writes the device's copy as it goes (set_unstuff_sink)
  uint8_t *sink = nullptr;
  s.unstuffed_at = nullptr;
  if (may_sink && active_sink_ && scans.size() == 1 && &s == &scans[0] && active_cap_ >= size - s.ecs_begin && !chunk_env) {
    sink = active_sink_;
    lanes = 1;
  }
  if (may_sink) active_sink_ = nullptr; // one parse, one scan
  size_t from = s.ecs_begin, ecs_end = size;
  // A file of many scans (progressive frames, the codestreams of JPEG XT boxes): what a round searches beyond the end of its scan
  // is searched again for the next scan -- ten scans, five times the file.  There the rounds start at a megabyte and double, so
  // that a scan costs at most twice its own length; the single scan of a sequential frame is searched to the end of the file
  // in one round as before.
  const bool many_scans = (progressive_ || scans.size() > 1) && !chunk_env;
  size_t round_bytes = many_scans ? (size_t)1 << 20 : SIZE_MAX;
  // (the chunks' event lists are this thread's and are kept: hundreds of kilobytes per chunk that would be mapped, touched and
  // unmapped for every scan otherwise)
  static thread_local std::vector<MarkerEvents> tl_events;
  std::vector<MarkerEvents> &ev = tl_events; // (the chunk workers below must see THIS thread's list, not their own)
  for (bool done = false; !done && from < size;) {
    const size_t left = size - from, reach = std::min(left, round_bytes);
    const size_t span = lanes > 1 ? std::min(max_chunk, std::max(many_scans ? (size_t)64 << 10 : min_chunk, (reach + lanes - 1) / lanes)) : left;
    const int n = (int)std::min<size_t>((size_t)lanes, (reach + span - 1) / span);
    if (round_bytes < SIZE_MAX / 2) round_bytes *= 2;
    if (ev.size() < (size_t)n) ev.resize((size_t)n);
    for (int i = 0; i < n; i++) {
      MarkerEvents &e = ev[(size_t)i];
      e.rst.clear();
      e.term = SIZE_MAX;
      e.tail_pairs = 0;
      e.tail_cut = SIZE_MAX;
      if (e.rst.capacity() < expect / (size_t)n + 16 && e.rst.capacity() < 4096) e.rst.reserve(std::min<size_t>(expect / (size_t)n + 16, 4096));
    }
    static const bool trace_search = getenv("MIJPEG_SEARCH_TIMES") != nullptr; // diagnostics
    const auto ts0 = std::chrono::steady_clock::now();
    parallel_for(n, [&](int i) {
      const size_t a = from + (size_t)i * span;
      scan_markers(data, size, a, std::min(size, a + span), ev[(size_t)i], sink);
    });
    if (trace_search) {
      size_t nm = 0;
      for (int i = 0; i < n; i++) nm += ev[(size_t)i].rst.size();
      fprintf(stderr, "   search round: %d chunks of %zu bytes, %zu markers, %.3f ms\n", n, span, nm,
              std::chrono::duration<double>(std::chrono::steady_clock::now() - ts0).count() * 1e3);
    }
    const auto tm0 = std::chrono::steady_clock::now();
    // (the lists take the round's markers in one piece and are written through plain pointers: four stores per marker)
    size_t add = 0;
    for (int i = 0; i < n; i++) {
      add += ev[(size_t)i].rst.size();
      if (ev[(size_t)i].term != SIZE_MAX) break;
    }
    size_t closed = iulen.size(), open_begin = ibegin.back();
    ibegin.resize(ibegin.size() + add);
    iulen.resize(iulen.size() + add);
    interval_end.resize(interval_end.size() + add);
    rst_code.resize(rst_code.size() + add);
    size_t *pb = ibegin.data() + closed + 1, *pe = interval_end.data() + closed;
    uint32_t *pu = iulen.data() + closed;
    uint8_t *pr = rst_code.data() + closed;
    for (int i = 0; i < n && !done; i++) {
      const size_t a = from + (size_t)i * span;
      if (a > open_begin && acc_cut == SIZE_MAX) // inside an interval: a place where a parallel copy may start
        ckpt.push_back(Scan::StuffCheckpoint{a, (uint32_t)closed, acc_pairs});
      for (const auto &m : ev[(size_t)i].rst) {
        if (acc_cut == SIZE_MAX) { acc_pairs += m.pairs; acc_cut = m.cut; }
        *pu++ = (uint32_t)(std::min(acc_cut, m.first) - open_begin - acc_pairs); // (close_interval)
        acc_pairs = 0;
        acc_cut = SIZE_MAX;
        *pe++ = m.first;
        *pr++ = m.second;
        open_begin = m.first + 2;
        *pb++ = open_begin;
        closed++;
      }
      if (acc_cut == SIZE_MAX) { acc_pairs += ev[(size_t)i].tail_pairs; acc_cut = ev[(size_t)i].tail_cut; }
      if (ev[(size_t)i].term != SIZE_MAX) {
        ecs_end = ev[(size_t)i].term;
        done = true;
      }
    }
    from += (size_t)n * span;
    if (trace_search) fprintf(stderr, "   ... merged in %.3f ms\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - tm0).count() * 1e3);
  }
  s.ecs_end = ecs_end;
  close_interval(s.ecs_end);
  interval_end.push_back(s.ecs_end);
  // where the intervals lie in the copy without stuffing and markers: back to back
  const size_t n = iulen.size();
  s.interval_ubegin.resize(n);
  s.interval_uend.resize(n);
  size_t off = 0;
  for (size_t k = 0; k < n; k++) {
    s.interval_ubegin[k] = (uint32_t)off;
    off += iulen[k];
    s.interval_uend[k] = (uint32_t)off;
  }
  s.unstuffed_size = off;
  s.unstuffed_at = sink;
  ibegin.swap(s.interval_begin);
  iulen.swap(s.interval_ulen);
  ckpt.swap(s.stuff_ckpt);
  interval_end.swap(interval_end_out);
  rst_code.swap(rst_code_out);
}

// ------------------------------------------------------------------------------------------------
// the entropy coded data without its byte stuffing (what the device decoder reads)
// ------------------------------------------------------------------------------------------------
// [src, end) -> dst: bytes up to the first FF that is not followed by 00, FF 00 as FF.  Returns the bytes written.
static size_t unstuff_copy(const uint8_t *src, const uint8_t *end, uint8_t *dst)
{
  uint8_t *o = dst;
  while (src < end) {
    const uint8_t *f = (const uint8_t *)memchr(src, 0xff, (size_t)(end - src));
    if (!f) {
      memcpy(o, src, (size_t)(end - src));
      o += end - src;
      break;
    }
    if (f + 1 >= end || f[1] != 0x00) { // marker, fill byte, or an FF the data ends with: not data
      memcpy(o, src, (size_t)(f - src));
      o += f - src;
      break;
    }
    memcpy(o, src, (size_t)(f + 1 - src)); // ... FF
    o += f + 1 - src;
    src = f + 2;                           // the stuffed zero stays behind
  }
  return (size_t)(o - dst);
}

// A run of whole restart intervals [src, end): what lies between them are their RSTn markers (with fill bytes in front, may
// be); the intervals are back to back in the copy, so the run is one sweep: FF 00 -> FF, everything else that starts with
// FF (fill bytes, the two bytes of a marker) leaves.  A fill byte inside the data of an interval ends that interval's data
// (the bit reader stops there): what follows up to the next marker leaves as well.
#if defined(__x86_64__)
// ... 32 bytes at a time: with restart intervals of a few blocks (a marker every twenty bytes) the two library calls per event
// of the loop below are what the copy costs.  A step stores all 32 bytes and moves on by those in front of the first 0xFF;
// what it wrote beyond them is overwritten by the steps that follow -- so a step is only taken where 32 bytes still fit in
// front of `dst_end`, the end of what this run produces (the neighbouring piece's bytes lie behind it, written by another thread).
__attribute__((target("avx2"))) static size_t unstuff_run_avx2(const uint8_t *src, const uint8_t *end, uint8_t *dst, const uint8_t *dst_end)
{
  const __m256i ff = _mm256_set1_epi8((char)0xff);
  uint8_t *o = dst;
  bool dead = false;
  while (src < end) {
    if (!dead && end - src >= 32 && dst_end - o >= 32) {
      const __m256i v = _mm256_loadu_si256((const __m256i *)src);
      const unsigned m = (unsigned)_mm256_movemask_epi8(_mm256_cmpeq_epi8(v, ff));
      _mm256_storeu_si256((__m256i *)o, v);
      if (!m) { src += 32; o += 32; continue; }
      const int p = __builtin_ctz(m);
      src += p;
      o += p;
    } else {
      const uint8_t *f = (const uint8_t *)memchr(src, 0xff, (size_t)(end - src));
      if (!f) f = end;
      if (!dead) {
        memcpy(o, src, (size_t)(f - src));
        o += f - src;
      }
      src = f;
      if (src >= end) break;
    }
    const uint8_t m = src + 1 < end ? src[1] : 0x01; // (an FF the run ends with is no data)
    if (m == 0x00) {
      if (!dead) *o++ = 0xff;
      src += 2;
    } else if (m >= 0xd0 && m <= 0xd7) {
      dead = false;
      src += 2;
    } else {
      dead = true; // fill byte (or the marker that ends the scan)
      src += 1;
    }
  }
  return (size_t)(o - dst);
}
#endif
static size_t unstuff_run(const uint8_t *src, const uint8_t *end, uint8_t *dst, const uint8_t *dst_end)
{
#if defined(__x86_64__)
  static const bool avx2 = __builtin_cpu_supports("avx2");
  if (avx2) return unstuff_run_avx2(src, end, dst, dst_end);
#endif
  (void)dst_end;
  uint8_t *o = dst;
  bool dead = false; // behind a fill byte: nothing counts until the next marker
  while (src < end) {
    const uint8_t *f = (const uint8_t *)memchr(src, 0xff, (size_t)(end - src));
    if (!f) f = end;
    if (!dead) {
      memcpy(o, src, (size_t)(f - src));
      o += f - src;
    }
    if (f >= end) break;
    const uint8_t m = f + 1 < end ? f[1] : 0x01; // (an FF the run ends with is no data)
    if (m == 0x00) {
      if (!dead) *o++ = 0xff;
      src = f + 2;
    } else if (m >= 0xd0 && m <= 0xd7) {
      dead = false;
      src = f + 2;
    } else {
      dead = true; // fill byte (or the marker that ends the scan)
      src = f + 1;
    }
  }
  return (size_t)(o - dst);
}

void HostDecoder::unstuff_pieces(size_t scan, size_t piece_bytes, std::vector<UnstuffPiece> &out) const
{
  const Scan &s = scans[scan];
  const std::vector<size_t> &iend = scan_interval_end_[scan];
  const size_t n = s.interval_ulen.size();
  size_t ck = 0;
  for (size_t k = 0; k < n;) {
    const size_t len = iend[k] - s.interval_begin[k];
    if (len <= piece_bytes) { // a run of whole intervals
      size_t k1 = k + 1;
      while (k1 < n && iend[k1] - s.interval_begin[k] <= piece_bytes) k1++;
      out.push_back(UnstuffPiece{(uint32_t)k, (uint32_t)k1, 0, SIZE_MAX, s.interval_ubegin[k]});
      k = k1;
      continue;
    }
    // a long interval: cut at the checkpoints the marker search left inside it
    size_t a = s.interval_begin[k];
    uint32_t pairs_a = 0;
    while (ck < s.stuff_ckpt.size() && s.stuff_ckpt[ck].interval < k) ck++;
    for (; ck < s.stuff_ckpt.size() && s.stuff_ckpt[ck].interval == k; ck++) {
      const Scan::StuffCheckpoint &c = s.stuff_ckpt[ck];
      out.push_back(UnstuffPiece{(uint32_t)k, (uint32_t)k + 1, a, c.pos, s.interval_ubegin[k] + (a - s.interval_begin[k]) - pairs_a});
      a = c.pos;
      pairs_a = c.pairs;
    }
    out.push_back(UnstuffPiece{(uint32_t)k, (uint32_t)k + 1, a, SIZE_MAX, s.interval_ubegin[k] + (a - s.interval_begin[k]) - pairs_a});
    k++;
  }
}

void HostDecoder::unstuff_piece(size_t scan, const UnstuffPiece &p, uint8_t *dst) const
{
  const Scan &s = scans[scan];
  const std::vector<size_t> &iend = scan_interval_end_[scan];
  const uint8_t *base = s.base ? s.base : data_;
  if (p.k1 - p.k0 > 1 || (p.src0 == 0 && p.src1 == SIZE_MAX)) {
    unstuff_run(base + s.interval_begin[p.k0], base + iend[p.k1 - 1], dst + p.dst, dst + s.interval_uend[p.k1 - 1]);
    return;
  }
  // a piece of one long interval.  A piece that starts on the zero of a stuffed pair leaves it to its predecessor (the pair
  // was counted where its FF is); one that ends between an FF and its zero looks at the zero all the same.
  const size_t b = s.interval_begin[p.k0], e = iend[p.k0];
  size_t a = std::max(p.src0, b), at = p.dst;
  const size_t z = std::min(p.src1, e);
  if (a > b && base[a] == 0x00 && base[a - 1] == 0xff) { a++; at++; } // (p.dst took that zero for one in front of the piece)
  if (a >= z) return;
  size_t stop = z;
  if (stop < e && base[stop - 1] == 0xff) stop++; // let unstuff_copy see what follows the FF (the next piece skips the zero)
  unstuff_copy(base + a, base + stop, dst + at);
}

// The restart marker searches the planning walk put off (the hidden refinement scans of a frame, the scans of a progressive frame),
// every scan's search on a thread of its own -- a search that is handed to a pool thread runs its chunks in order -- and what
// RefWalker::scan checks behind a search: exactly the restart markers the MCU count asks for, in sequence (anything else
// resynchronises: the sequential walk's business).
bool HostDecoder::defer_progressive_scans()
{
  static const bool off = getenv("MIJPEG_NO_DEFERRED_SEARCH") != nullptr; // A-B comparisons
  return !off;
}

void HostDecoder::run_deferred_searches(std::vector<DeferredSearch> &searches)
{
  if (searches.empty()) return;
  // (small ones: not worth waking anybody -- like the searches of small streams, which stay on the calling thread)
  size_t bytes = 0;
  for (const DeferredSearch &ds : searches) bytes += ds.size > scans[ds.scan].ecs_begin ? ds.size - scans[ds.scan].ecs_begin : 0;
  const int workers = bytes < ((size_t)1 << 20) ? 1 : (int)std::min<size_t>(searches.size(), (size_t)std::max(1, default_threads()));
  std::atomic<size_t> next{0};
  static const bool trace = getenv("MIJPEG_SEARCH_TIMES") != nullptr; // diagnostics
  const auto t0 = std::chrono::steady_clock::now();
  std::atomic<bool> irregular{false};
  parallel_for(workers, [&](int w) {
    for (size_t k = next.fetch_add(1); k < searches.size(); k = next.fetch_add(1)) {
      const DeferredSearch &ds = searches[k];
      const auto ta = std::chrono::steady_clock::now();
      find_intervals_in(scans[ds.scan], ds.data, ds.size, scan_interval_end_[ds.scan], scan_rst_code_[ds.scan], false);
      // (what RefWalker::scan checks behind a search, by the thread that made the lists)
      const Scan &ps = scans[ds.scan];
      const std::vector<uint8_t> &rst = scan_rst_code_[ds.scan];
      const int64_t total_mcus = (int64_t)ps.mcus_x * ps.mcus_y;
      const int64_t ri = ps.restart_interval ? ps.restart_interval : total_mcus;
      const int64_t nint = (total_mcus + ri - 1) / ri;
      bool bad = (int64_t)ps.interval_begin.size() != nint;
      for (int64_t i = 0; !bad && i + 1 < nint; i++) bad = rst[(size_t)i] != 0xd0 + (i & 7);
      if (bad) irregular.store(true, std::memory_order_relaxed);
      if (trace)
        fprintf(stderr, "   deferred search %zu on worker %d: starts at %.3f ms, takes %.3f ms\n", k, w, std::chrono::duration<double>(ta - t0).count() * 1e3,
                std::chrono::duration<double>(std::chrono::steady_clock::now() - ta).count() * 1e3);
    }
  });
  if (trace) fprintf(stderr, "   deferred searches: %zu on %d workers, %.3f ms\n", searches.size(), workers, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3);
  if (irregular.load()) needs_sequential_ = true;
  searches.clear();
}

} // namespace mij
