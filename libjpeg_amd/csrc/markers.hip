// markers.hip -- restart marker search and unstuffing of entropy coded segments on the device (contract: markers.hpp).
//
// Two passes over the raw bytes, 16 per lane, 4096 per workgroup ("chunk"), all images of a batch in one launch each:
//   pass 1   classify; kept bytes and markers per chunk; atomicMin of the first terminator into the image's `term`
//   scans    exclusive prefix sums of both counts over the launch's chunks (exclusive_scan_u32 of the encoder side); a chunk's
//            prefix inside its image is the difference to the image's first chunk
//   pass 2   classify again, mask everything at or beyond term, write kept bytes and table entries
// The counts of pass 1 do not know term yet.  That is sound because the scans are exclusive: chunks in front of the one that
// holds term are unaffected, that chunk masks in pass 2, and the ones behind it write nothing.  The chunk that holds term
// knows the image's totals and writes them, the COUNT / NO_END flags, the last table entry and the zeros behind the data.
// A byte is classified from itself, the byte in front and the byte behind: the pairs FF 00 / FF Dn are interpreted from their
// FF, and their second byte (never FF) is dropped by whoever holds it because the byte in front of it is FF.
#include <hip/hip_runtime.h>

#include "hencode.hpp"
#include "markers.hpp"

namespace mij {
namespace {

constexpr int GROUP = (int)MARKERS_GROUP, LANE_BYTES = (int)MARKERS_LANE_BYTES;
constexpr uint32_t NO_BYTE = 0x100; // "no byte there": in front of the segment, behind its end

// The 16 bytes of a lane at p0 (< size), the byte in front (NO_BYTE at p0 = 0) and the byte behind (NO_BYTE at the end).
struct LaneBytes {
  uint32_t w[4];
  uint32_t prev, next, n; // n: bytes of the lane inside the segment
  __device__ uint32_t at(int j) const { return (w[j >> 2] >> ((j & 3) * 8)) & 0xffu; }
};

__device__ inline LaneBytes load_lane(const uint8_t *seg, uint32_t size, uint32_t p0)
{
  LaneBytes b;
  b.w[0] = b.w[1] = b.w[2] = b.w[3] = 0;
  b.prev = b.next = NO_BYTE;
  b.n = 0;
  if (p0 >= size) return b;
  b.n = min((uint32_t)LANE_BYTES, size - p0);
  const uint8_t *p = seg + p0;
  if (b.n == (uint32_t)LANE_BYTES && ((uintptr_t)p & 15u) == 0) {
    const uint4 v = *(const uint4 *)p;
    b.w[0] = v.x; b.w[1] = v.y; b.w[2] = v.z; b.w[3] = v.w;
  } else {
    for (uint32_t j = 0; j < b.n; j++) b.w[j >> 2] |= (uint32_t)p[j] << ((j & 3) * 8);
  }
  if (p0 > 0) b.prev = p[-1];
  if (p0 + (uint32_t)LANE_BYTES < size) b.next = p[LANE_BYTES];
  return b;
}

enum Kind : uint32_t { DROP = 0, KEEP = 1, MARKER = 2, FILL = 3, TERM = 4 };

// what byte `cur` is, given its neighbours (FILL and a lone FF at the end count as kept: a flag is set for them anyway)
__device__ inline uint32_t classify(uint32_t before, uint32_t cur, uint32_t after)
{
  if (cur == 0xffu) {
    if (after == NO_BYTE || after == 0x00u) return KEEP;
    if (after == 0xffu) return FILL;
    if (after >= 0xd0u && after <= 0xd7u) return MARKER;
    return TERM;
  }
  if (before == 0xffu && (cur == 0x00u || (cur >= 0xd0u && cur <= 0xd7u))) return DROP;
  return KEEP;
}

// f(j, kind, byte, follower) for the lane's bytes at positions p0 + j < limit
template <class F>
__device__ inline void for_each_byte(const LaneBytes &b, uint32_t p0, uint32_t limit, F f)
{
  uint32_t before = b.prev;
#pragma unroll
  for (int j = 0; j < LANE_BYTES; j++) {
    const uint32_t cur = b.at(j);
    const uint32_t after = j + 1 < LANE_BYTES ? ((uint32_t)(j + 1) < b.n ? b.at(j + 1) : NO_BYTE) : b.next;
    if ((uint32_t)j < b.n && p0 + (uint32_t)j < limit) f(j, classify(before, cur, after), cur, after);
    before = cur;
  }
}

// inclusive prefix sum over the workgroup's lanes; *total: the workgroup's sum
__device__ inline uint32_t group_inclusive(uint32_t v, uint32_t *wave_tot, uint32_t *total)
{
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  if (lane == 63) wave_tot[wv] = v;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < GROUP / 64; k++) {
    const uint32_t t = wave_tot[k];
    if (k < wv) before += t;
    all += t;
  }
  *total = all;
  return before + v;
}

__global__ __launch_bounds__(GROUP) void marker_count_kernel(MarkerArgs a)
{
  __shared__ uint32_t wave_tot[GROUP / 64];
  if (blockIdx.x >= a.n_chunks) return;
  const uint32_t c = a.chunk0 + blockIdx.x;
  const MarkerChunk ch = a.chunks[c];
  const MarkerImage im = a.images[ch.image];
  const uint32_t p0 = ch.index * MARKERS_CHUNK + threadIdx.x * MARKERS_LANE_BYTES;
  const LaneBytes b = load_lane(a.raw + im.raw_off, im.size, p0);
  uint32_t kept = 0, marks = 0, term = 0xffffffffu;
  for_each_byte(b, p0, im.size, [&](int j, uint32_t kind, uint32_t, uint32_t) {
    kept += (kind == KEEP || kind == FILL) ? 1u : 0u;
    marks += kind == MARKER ? 1u : 0u;
    if (kind == TERM) term = min(term, p0 + (uint32_t)j);
  });
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) term = min(term, (uint32_t)__shfl_down(term, d, 64));
  if ((threadIdx.x & 63) == 0 && term != 0xffffffffu) atomicMin(&a.results[ch.image].term, term);
  uint32_t total;
  group_inclusive(kept | (marks << 16), wave_tot, &total); // (4096 bytes, 2048 markers at most: both fit their halves)
  if (threadIdx.x == 0) {
    a.kept[c] = total & 0xffffu;
    a.marks[c] = total >> 16;
  }
}

__global__ __launch_bounds__(GROUP) void marker_write_kernel(MarkerArgs a)
{
  __shared__ uint32_t wave_tot[GROUP / 64];
  if (blockIdx.x >= a.n_chunks) return;
  const uint32_t c = a.chunk0 + blockIdx.x;
  const MarkerChunk ch = a.chunks[c];
  const MarkerImage im = a.images[ch.image];
  MarkerResult *res = a.results + ch.image;
  const uint32_t term = min(res->term, im.size);
  const uint32_t term_chunk = min(term / MARKERS_CHUNK, im.n_chunks - 1);
  if (ch.index > term_chunk) return; // everything here lies behind term
  const uint32_t p0 = ch.index * MARKERS_CHUNK + threadIdx.x * MARKERS_LANE_BYTES;
  const LaneBytes b = load_lane(a.raw + im.raw_off, im.size, p0);
  uint32_t kept = 0, marks = 0, flags = 0;
  for_each_byte(b, p0, term, [&](int, uint32_t kind, uint32_t, uint32_t) {
    kept += (kind == KEEP || kind == FILL) ? 1u : 0u;
    marks += kind == MARKER ? 1u : 0u;
    if (kind == FILL) flags |= MARKERS_FILL;
  });
  uint32_t total;
  const uint32_t packed = kept | (marks << 16);
  const uint32_t mine = group_inclusive(packed, wave_tot, &total) - packed;
  const uint32_t kept0 = (uint32_t)(a.kept_at[c] - a.kept_at[im.first_chunk]), marks0 = (uint32_t)(a.marks_at[c] - a.marks_at[im.first_chunk]);
  uint32_t at = kept0 + (mine & 0xffffu), k = marks0 + (mine >> 16);
  uint8_t *out = a.dst + im.dst_off;
  uint32_t *ib = a.ibegin + im.first_interval, *ie = a.iend + im.first_interval;
  for_each_byte(b, p0, term, [&](int, uint32_t kind, uint32_t cur, uint32_t after) {
    if (kind == KEEP || kind == FILL) {
      if (at < im.dst_cap) out[at] = (uint8_t)cur; // (kept bytes <= size <= dst_cap: the guard costs nothing and holds whatever the host says)
      at++;
    } else if (kind == MARKER) {
      if (after != 0xd0u + (k & 7u)) flags |= MARKERS_SEQUENCE;
      if (k + 1 < im.expect) { // markers beyond the ones the frame header asks for have no table entry
        ie[k] = at;
        ib[k + 1] = at;
      }
      k++;
    }
  });
  if (flags) atomicOr(&res->flags, flags);
  if (ch.index == 0 && threadIdx.x == 0 && im.expect > 0) ib[0] = 0;
  if (ch.index != term_chunk) return;
  // the chunk that holds term: the image's totals, the flags that need them, the last table entry, the zeros behind the data
  const uint32_t all_kept = kept0 + (total & 0xffffu), all_marks = marks0 + (total >> 16);
  if (threadIdx.x == 0) {
    res->total = all_kept;
    res->markers = all_marks;
    const uint32_t late = (all_marks + 1 != im.expect ? MARKERS_COUNT : 0u) | (term >= im.size ? MARKERS_NO_END : 0u);
    if (late) atomicOr(&res->flags, late);
    if (im.expect > 0) ie[im.expect - 1] = all_kept;
  }
  for (uint32_t z = all_kept + threadIdx.x; z < im.dst_cap; z += (uint32_t)GROUP) out[z] = 0;
}

// One wave per image, behind pass 2 (contract: MarkerFitArgs)
__global__ __launch_bounds__(64) void marker_fit_kernel(MarkerFitArgs a)
{
  const uint32_t i = blockIdx.x;
  if (i >= a.n_images) return;
  const uint32_t nint = a.fit_intervals[i];
  if (nint == 0) return;
  const MarkerImage im = a.images[i];
  const MarkerResult r = a.results[i];
  const bool good = r.flags == 0 && im.size >= 2 && r.term == im.size - 2 && r.total > 0 && r.total <= im.size;
  const uint32_t total = good ? r.total : 0;
  if (threadIdx.x == 0) {
    const uint32_t bound = a.img_nsub[i]; // the host's, from the raw size
    a.img_e1[i] = total;
    a.img_nsub[i] = min((total + a.sub_bytes - 1) / a.sub_bytes, bound);
    if (!good) a.walk_status[i] = HUFF_WALK_NOT_SEARCHED;
  }
  for (uint32_t k = threadIdx.x; k < nint; k += 64) a.iend[im.first_interval + k] = total;
}

} // namespace

int launch_marker_fit(const MarkerFitArgs &a, hipStream_t stream)
{
  if (a.n_images == 0) return 0;
  hipLaunchKernelGGL(marker_fit_kernel, dim3(a.n_images), dim3(64), 0, stream, a);
  return (int)hipGetLastError();
}

MarkerScratch markers_scratch(uint32_t n_chunks)
{
  auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
  MarkerScratch s;
  const size_t C = n_chunks;
  s.kept = 0;
  s.marks = up(s.kept + C * 4);
  s.kept_at = up(s.marks + C * 4);
  s.marks_at = up(s.kept_at + (C + 1) * 8);
  s.scan = up(s.marks_at + (C + 1) * 8);
  s.scan_words = scan_scratch_words(C);
  s.end = up(s.scan + s.scan_words * 8);
  return s;
}

int launch_marker_search(const MarkerArgs &a, uint64_t *scan_scratch, size_t scan_words, hipStream_t stream)
{
  if (a.n_chunks == 0) return 0;
  hipLaunchKernelGGL(marker_count_kernel, dim3(a.n_chunks), dim3(GROUP), 0, stream, a);
  if (const int rc = (int)hipGetLastError()) return rc;
  // (a chunk's prefix inside its image is a difference of two entries: where the sums start does not matter)
  if (const int rc = exclusive_scan_u32(a.kept + a.chunk0, (uint64_t *)a.kept_at + a.chunk0, a.n_chunks, scan_scratch, scan_words, stream)) return rc;
  if (const int rc = exclusive_scan_u32(a.marks + a.chunk0, (uint64_t *)a.marks_at + a.chunk0, a.n_chunks, scan_scratch, scan_words, stream)) return rc;
  hipLaunchKernelGGL(marker_write_kernel, dim3(a.n_chunks), dim3(GROUP), 0, stream, a);
  return (int)hipGetLastError();
}

} // namespace mij
