// resample_taps.hpp -- the host half of the resized crop call (include/mijpeg.h): the filter's taps for one axis, in
// integers only, and the layout of the tables one call uploads.  resample.hip reads what stands in them; ragged_reconstruct.cpp uploads and
// launches.  Calls nothing of the HIP runtime and nothing of the library: a plain host compiler builds tests/cxx/resample_taps.cpp
// around it.  Private to libmijpeg.so.
//
// The filter (normative: tests/resample_model.py restates it in numpy).  One axis, n source samples -> m output samples, a triangle
// whose support grows with the reduction; for output o and source i
//   S = 2 max(n, m)    D(i) = |(2i + 1) m - (2o + 1) n|    w(i) = max(0, S - D(i))
// the taps of o are the run of i in [0, n) with w(i) > 0 (never empty, at most min(n, 2 ceil(max(n, m) / m) + 1) long), and with
// W = sum w(i) their weights are k(i) = floor((w(i) 2^14 + floor(W / 2)) / W); what is missing to sum k = 2^14 goes to the tap
// with the largest w (the lowest such index).  out = min(255, (sum k(i) p(i) + 2^13) >> 14), first along x, then along y.
#ifndef MIJ_RESAMPLE_TAPS_HPP
#define MIJ_RESAMPLE_TAPS_HPP
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace mij {

constexpr int RESAMPLE_BITS = 14;
constexpr int32_t RESAMPLE_ONE = 1 << RESAMPLE_BITS;
constexpr int32_t RESAMPLE_MAX_AXIS = 65535;      // what a JPEG frame header can say
constexpr int RESAMPLE_TILE_W = 64, RESAMPLE_TILE_H = 16; // output pixels of a workgroup (resample.hip)

// the bound of the tap count the filter's definition gives
inline int32_t resample_taps_bound(int32_t n, int32_t m)
{
  const int64_t big = n > m ? n : m, b = 2 * ((big + m - 1) / m) + 1;
  return (int32_t)(b < n ? b : n);
}

// w(i) of output o (64-bit: (2i + 1) m passes 32 bits for 65535-sample axes)
inline int64_t resample_w(int64_t n, int64_t m, int64_t o, int64_t i)
{
  const int64_t S = 2 * (n > m ? n : m), d = (2 * i + 1) * m - (2 * o + 1) * n;
  return S - (d < 0 ? -d : d);
}

// The run of output o: its first tap and their number
inline void resample_run(int32_t n, int32_t m, int32_t o, int32_t &first, int32_t &count)
{
  // w(i) > 0 <=> (2o + 1) n - S < (2i + 1) m: an estimate from below, then the exact edge
  const int64_t S = 2 * (int64_t)(n > m ? n : m), lo = (2 * (int64_t)o + 1) * n - S;
  int64_t i = lo > 0 ? lo / (2 * (int64_t)m) - 1 : 0;
  if (i < 0) i = 0;
  while (i < n - 1 && resample_w(n, m, o, i) <= 0) i++;
  int64_t e = i;
  while (e < n && resample_w(n, m, o, e) > 0) e++;
  first = (int32_t)i;
  count = (int32_t)(e - i);
}

// The taps of one axis: first[m], count[m], and the weights of output o at weights[o * capacity_per_output ...], zero behind its
// count.  -> the maximal tap count of the axis; with a NULL array only that.  0: n or m outside [1, RESAMPLE_MAX_AXIS], a capacity
// below the maximal count, or -- what the definition excludes -- an empty run or weights that do not sum to 2^14 (nothing is then
// defined).
inline int32_t resample_taps(int32_t n, int32_t m, int32_t *first, int32_t *count, int16_t *weights, int32_t capacity_per_output)
{
  if (n < 1 || m < 1 || n > RESAMPLE_MAX_AXIS || m > RESAMPLE_MAX_AXIS) return 0;
  const bool fill = first && count && weights;
  if (fill && capacity_per_output < 1) return 0;
  int32_t most = 0;
  for (int32_t o = 0; o < m; o++) {
    int32_t f, c;
    resample_run(n, m, o, f, c);
    if (c < 1) return 0;
    if (c > most) most = c;
    if (!fill) continue;
    if (c > capacity_per_output) return 0;
    first[o] = f;
    count[o] = c;
    int16_t *k = weights + (size_t)o * (size_t)capacity_per_output;
    int64_t W = 0, best = 0;
    int32_t at = 0;
    for (int32_t t = 0; t < c; t++) {
      const int64_t w = resample_w(n, m, o, f + t);
      W += w;
      if (w > best) { best = w; at = t; }
    }
    int32_t sum = 0;
    const bool narrow = W < ((int64_t)1 << 30); // (w < 2^17: w 2^14 + W / 2 then fits 32 bits, and so does the division)
    for (int32_t t = 0; t < c; t++) {
      const int64_t w = resample_w(n, m, o, f + t);
      const int32_t q = narrow ? (int32_t)(((uint32_t)w * (uint32_t)RESAMPLE_ONE + (uint32_t)W / 2) / (uint32_t)W) : (int32_t)((w * RESAMPLE_ONE + W / 2) / W);
      k[t] = (int16_t)q;
      sum += q;
    }
    const int32_t fixed = k[at] + (RESAMPLE_ONE - sum);
    if (fixed < 0 || fixed > RESAMPLE_ONE) return 0;
    k[at] = (int16_t)fixed;
    for (int32_t t = c; t < capacity_per_output; t++) k[t] = 0;
  }
  return most <= resample_taps_bound(n, m) ? most : 0;
}

// ---- the tables of one call ----------------------------------------------------------------------------------------------------
// One served picture as the kernel reads it (device memory)
struct ResamplePicture {
  uint64_t src_off;        // its crop in the arena: bytes from the arena's base, a multiple of 16; lines src_w * comps bytes apart
  uint64_t dst_off;        // its slot: bytes from the destination's base
  int32_t src_w, src_h;    // the clipped crop
  int32_t comps;           // 1 or 3, interleaved
  int32_t tiles_x;         // workgroups per row of tiles of the output picture
  uint32_t xtab, ytab;     // its two axis tables: bytes from the tables' base
  int32_t xcap, ycap;      // weights per output sample in them
};
static_assert(sizeof(ResamplePicture) == 48, "the kernel and the host agree on the descriptor");

// An axis table of m outputs with `cap` weights each: int32 first[m], int32 count[m], int16 weights[m * cap], padded to 16 bytes
inline size_t resample_axis_bytes(int32_t m, int32_t cap) { return ((size_t)m * 8 + (size_t)m * (size_t)cap * 2 + 15) / 16 * 16; }
inline size_t resample_crop_bytes(int32_t w, int32_t h, int32_t comps) { return ((size_t)w * (size_t)h * (size_t)comps + 15) / 16 * 16; }

// One picture of the list as the call sees it: served or not, its clipped crop
struct ResampleItem {
  bool served = false;
  int32_t slot = 0;          // its index in the list = its slot in the destination
  int32_t src_w = 0, src_h = 0, comps = 0;
  int32_t xcap = 0, ycap = 0; // the axes' maximal tap counts where the caller has them (resample_item_caps: one picture per worker); 0: resample_layout counts
  bool mirror = false;       // its slot holds the lines reversed (resize, then flip): resample_fill reverses the x table's columns
};
inline void resample_item_caps(ResampleItem &it, int32_t out_w, int32_t out_h)
{
  it.xcap = resample_taps(it.src_w, out_w, nullptr, nullptr, nullptr, 0);
  it.ycap = resample_taps(it.src_h, out_h, nullptr, nullptr, nullptr, 0);
}

// Where everything lies, in bytes from 16-byte aligned bases: the tables [pictures][first, one more than pictures][axis tables], and
// the arena of the crops.  per[k] belongs to the k-th SERVED picture.
struct ResampleLayout {
  struct Per { int32_t item; size_t xtab, ytab, src_off; int32_t xcap, ycap; uint32_t first_workgroup; };
  std::vector<Per> per;
  size_t pictures = 0, first = 0, table_bytes = 0, arena_bytes = 0;
  uint64_t workgroups = 0;
};

inline uint64_t resample_tiles(int32_t out_w, int32_t out_h)
{
  return (uint64_t)((out_w + RESAMPLE_TILE_W - 1) / RESAMPLE_TILE_W) * (uint64_t)((out_h + RESAMPLE_TILE_H - 1) / RESAMPLE_TILE_H);
}

inline ResampleLayout resample_layout(const ResampleItem *items, int n, int32_t out_w, int32_t out_h)
{
  ResampleLayout L;
  for (int i = 0; i < n; i++)
    if (items[i].served) L.per.push_back(ResampleLayout::Per{i, 0, 0, 0, 0, 0, 0});
  const size_t served = L.per.size();
  L.pictures = 0;
  L.first = (served * sizeof(ResamplePicture) + 15) / 16 * 16;
  size_t at = L.first + ((served + 1) * sizeof(uint32_t) + 15) / 16 * 16, src = 0;
  const uint64_t tiles = resample_tiles(out_w, out_h);
  for (ResampleLayout::Per &p : L.per) {
    const ResampleItem &it = items[p.item];
    p.xcap = it.xcap ? it.xcap : resample_taps(it.src_w, out_w, nullptr, nullptr, nullptr, 0);
    p.ycap = it.ycap ? it.ycap : resample_taps(it.src_h, out_h, nullptr, nullptr, nullptr, 0);
    p.xtab = at;
    at += resample_axis_bytes(out_w, p.xcap);
    p.ytab = at;
    at += resample_axis_bytes(out_h, p.ycap);
    p.src_off = src;
    src += resample_crop_bytes(it.src_w, it.src_h, it.comps);
    p.first_workgroup = (uint32_t)L.workgroups;
    L.workgroups += tiles;
  }
  L.table_bytes = at;
  L.arena_bytes = src;
  return L;
}

// An axis table's columns in reverse order: output o carries first, count and the weights of output m - 1 - o.  The kernel reads a
// column's run as it stands and stores along x as ever, so a picture filled this way comes out mirrored without the kernel knowing.
inline void resample_mirror_axis(int32_t *first, int32_t *count, int16_t *weights, int32_t m, int32_t cap)
{
  for (int32_t o = 0, r = m - 1; o < r; o++, r--) {
    const int32_t f = first[o], c = count[o];
    first[o] = first[r]; count[o] = count[r];
    first[r] = f; count[r] = c;
    int16_t *a = weights + (size_t)o * (size_t)cap, *b = weights + (size_t)r * (size_t)cap;
    for (int32_t t = 0; t < cap; t++) { const int16_t k = a[t]; a[t] = b[t]; b[t] = k; }
  }
}

// The tables of served picture k into host (table_bytes of it); k == 0 also writes nothing else: resample_fill_first closes the prefix
// table.  A mirrored item's x table is filled in reverse; its y table is what it would be without the flag.  false where an axis has
// no taps (sizes resample_taps refuses)
inline bool resample_fill(uint8_t *host, const ResampleLayout &L, size_t k, const ResampleItem *items, int32_t out_w, int32_t out_h, int64_t image_stride)
{
  const ResampleLayout::Per &p = L.per[k];
  const ResampleItem &it = items[p.item];
  ResamplePicture &d = ((ResamplePicture *)(host + L.pictures))[k];
  d.src_off = p.src_off;
  d.dst_off = (uint64_t)it.slot * (uint64_t)image_stride;
  d.src_w = it.src_w; d.src_h = it.src_h; d.comps = it.comps;
  d.tiles_x = (out_w + RESAMPLE_TILE_W - 1) / RESAMPLE_TILE_W;
  d.xtab = (uint32_t)p.xtab; d.ytab = (uint32_t)p.ytab;
  d.xcap = p.xcap; d.ycap = p.ycap;
  ((uint32_t *)(host + L.first))[k] = p.first_workgroup;
  int32_t *xt = (int32_t *)(host + p.xtab), *yt = (int32_t *)(host + p.ytab);
  if (!(resample_taps(it.src_w, out_w, xt, xt + out_w, (int16_t *)(xt + 2 * (size_t)out_w), p.xcap) == p.xcap && p.xcap > 0 &&
        resample_taps(it.src_h, out_h, yt, yt + out_h, (int16_t *)(yt + 2 * (size_t)out_h), p.ycap) == p.ycap && p.ycap > 0))
    return false;
  if (it.mirror) resample_mirror_axis(xt, xt + out_w, (int16_t *)(xt + 2 * (size_t)out_w), out_w, p.xcap);
  return true;
}
inline void resample_fill_first(uint8_t *host, const ResampleLayout &L) { ((uint32_t *)(host + L.first))[L.per.size()] = (uint32_t)L.workgroups; }

} // namespace mij
#endif
