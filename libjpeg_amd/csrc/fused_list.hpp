// fused_list.hpp -- lists of differently shaped frames through the ragged flavours of the fused kernels, the
// host half that needs no device: which frames share a launch, where a launch's tables lie in the one upload of a call, what
// stands in them.  launch_fused_lists (reconstruct_device.cpp) uploads and launches.  Calls nothing of the HIP runtime: a plain
// host compiler builds tests/cxx/fused_list_tables.cpp around it.  Private to libmijpeg.so.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "kernels.hpp"
#include "reconstruct.hpp"

// One frame of a list: its description, where its coefficients lie and where its pixels go
struct FusedListItem {
  const mijpeg_info *info;
  int64_t coef_base;                    // int16 index of its coefficient store from the object's coef_dev
  void *out[3];                         // device: the first pixel (interleaved output: out[0] alone), or the first sample of each plane
  int64_t row_stride;                   // bytes per line (of every plane)
  const uint16_t *own_deltas = nullptr; // host, [4][64] per COMPONENT: the frame's own tables in a batch that has them (else info's)
  // A window launch: the crop rectangle on the frame's canvas, inclusive and clipped to it (fused_window_clip); `out`
  // is then where pixel (min_x, min_y) goes.  Null in every other launch.
  const mijpeg_rect *window = nullptr;
};

// A crop rectangle as the rect calls take it -> the rectangle inside a w x h picture: max beyond the picture is clipped to the last
// column / line; false where min lies outside the picture or nothing is left (min > max)
inline bool fused_window_clip(const mijpeg_rect &r, int32_t w, int32_t h, mijpeg_rect &clipped)
{
  if (w < 1 || h < 1 || r.min_x < 0 || r.min_y < 0 || r.min_x >= w || r.min_y >= h) return false;
  clipped.min_x = r.min_x; clipped.min_y = r.min_y;
  clipped.max_x = r.max_x < w - 1 ? r.max_x : w - 1;
  clipped.max_y = r.max_y < h - 1 ? r.max_y : h - 1;
  return clipped.min_x <= clipped.max_x && clipped.min_y <= clipped.max_y;
}
// The 128 x 128 tiles a clipped window touches: first tile column and row, tiles per window row, window rows
inline mij::WindowFrame fused_window_tiles(const mijpeg_rect &w)
{
  mij::WindowFrame t;
  t.tile_x0 = w.min_x >> 7; t.tile_y0 = w.min_y >> 7;
  t.wtiles_x = (w.max_x >> 7) - t.tile_x0 + 1; t.wtiles_y = (w.max_y >> 7) - t.tile_y0 + 1;
  t.min_x = w.min_x; t.min_y = w.min_y; t.max_x = w.max_x; t.max_y = w.max_y;
  return t;
}

// The frames that share a launch: those that agree on kernel and arithmetic flavour, as many as a grid holds
struct FusedListLaunch {
  mij::ReconPlan p;
  std::vector<int> members; // indices into the items
  uint64_t grid;            // workgroups: one per 128 x 128 tile of every member (a window launch: per tile of every member's window)
};

inline uint64_t fused_list_tiles(const mijpeg_info &f) { return (uint64_t)((f.width + 127) / 128) * (uint64_t)((f.height + 127) / 128); }
// ... of which a window launch runs those of the window
inline uint64_t fused_list_tiles(const mijpeg_info &f, const mijpeg_rect *window)
{
  if (!window) return fused_list_tiles(f);
  const mij::WindowFrame t = fused_window_tiles(*window);
  return (uint64_t)t.wtiles_x * (uint64_t)t.wtiles_y;
}

// Item `item` (frame f, planned as p) into the launch of its kernel and flavour, a new one where there is none or the grid is
// full (2^31 - 1 workgroups).  One outlier beyond the fast gates runs the SAFE flavour alone instead of taking a launch along.
inline void fused_list_add(std::vector<FusedListLaunch> &launches, const mij::ReconPlan &p, int item, const mijpeg_info &f, const mijpeg_rect *window = nullptr)
{
  const uint64_t tiles = fused_list_tiles(f, window);
  size_t l = 0;
  while (l < launches.size() && !(launches[l].p.kernel == p.kernel && launches[l].p.fast == p.fast && launches[l].p.wide == p.wide &&
                                  launches[l].p.narrow12 == p.narrow12 && launches[l].grid + tiles <= 0x7fffffffull))
    l++;
  if (l == launches.size()) launches.push_back(FusedListLaunch{p, {}, 0});
  launches[l].members.push_back(item);
  launches[l].grid += tiles;
}

// The tables of a launch of m frames, `at` bytes into the upload: [RaggedFrame x m][first workgroups, m + 1 of them, padded to 16
// bytes][deltas << 4, per frame 4 x 64] and, for planar launches, [PlanarFrame x m], for window launches [WindowFrame x m] (behind
// the planes: the kernels find it there): where its parts begin and where it ends.  Every part is 16-byte aligned where `at` is.
struct FusedListTable {
  size_t frames, first, deltas, planes, windows, end;
  FusedListTable(size_t at, size_t m, bool planar, bool window = false)
      : frames(at), first(frames + m * sizeof(mij::RaggedFrame)), deltas(first + ((m + 1) * 4 + 15) / 16 * 16), planes(deltas + m * 4 * 64 * sizeof(int32_t)),
        windows(planes + (planar ? m * sizeof(mij::PlanarFrame) : 0)), end(windows + (window ? m * sizeof(mij::WindowFrame) : 0)) {}
};

// The tables of all launches, one behind the other from offset 0
inline std::vector<FusedListTable> fused_list_layout(const std::vector<FusedListLaunch> &launches, bool planar, bool window = false)
{
  std::vector<FusedListTable> tables;
  for (const FusedListLaunch &l : launches) tables.emplace_back(tables.empty() ? 0 : tables.back().end, l.members.size(), planar, window);
  return tables;
}

// Launch l's tables into host memory (t: its place there): the frames in member order, frame k with the workgroups
// [first[k], first[k + 1]) -- first[m] is the grid -- and with table k of the deltas, 16 for a component it does not have.
// window: every item has one; frame k's workgroups are its window's tiles, and its `out` (its planes) are biased -- the address canvas
// pixel (0, 0) would have, min_y lines and min_x pixels in front of the caller's pointer: the kernels add the offsets of picture
// coordinates to it, and those of the window's pixels -- the only ones they store to -- land in the caller's memory.  (8-bit samples:
// a pixel is `components` bytes, one byte in a plane.  The address may lie in front of the allocation; it is never dereferenced.)
inline uint8_t *fused_window_bias(void *p, const mijpeg_rect &w, int64_t row_stride, int bytes_per_pixel)
{
  return (uint8_t *)((uintptr_t)p - (uintptr_t)((int64_t)w.min_y * row_stride + (int64_t)w.min_x * bytes_per_pixel));
}
inline void fused_list_fill(uint8_t *host, const FusedListTable &t, const FusedListLaunch &l, const FusedListItem *items, bool planar, bool window = false)
{
  const size_t m = l.members.size();
  mij::RaggedFrame *fr = (mij::RaggedFrame *)(host + t.frames);
  uint32_t *first = (uint32_t *)(host + t.first);
  int32_t *q = (int32_t *)(host + t.deltas);
  mij::PlanarFrame *pl = (mij::PlanarFrame *)(host + t.planes);
  mij::WindowFrame *win = (mij::WindowFrame *)(host + t.windows);
  uint32_t at = 0;
  for (size_t k = 0; k < m; k++) {
    const FusedListItem &it = items[l.members[k]];
    const mijpeg_info &f = *it.info;
    mij::RaggedFrame &x = fr[k];
    memset(&x, 0, sizeof(x));
    fused_geometry(f, l.p.sampling, x);
    x.coef_base = it.coef_base;
    x.out = (uint8_t *)it.out[0];
    x.row_stride = it.row_stride;
    x.qframe = (int32_t)k;
    if (planar) {
      pl[k].g = (uint8_t *)it.out[1];
      pl[k].b = (uint8_t *)it.out[2];
    }
    if (window) {
      const int bpp = planar ? 1 : f.components;
      win[k] = fused_window_tiles(*it.window);
      x.out = fused_window_bias(it.out[0], *it.window, it.row_stride, bpp);
      if (planar) {
        pl[k].g = fused_window_bias(it.out[1], *it.window, it.row_stride, bpp);
        pl[k].b = fused_window_bias(it.out[2], *it.window, it.row_stride, bpp);
      }
    }
    first[k] = at;
    at += (uint32_t)fused_list_tiles(f, window ? it.window : nullptr);
    for (int c = 0; c < 4; c++)
      for (int z = 0; z < 64; z++) {
        const uint16_t delta = c >= f.components ? 1 : it.own_deltas ? it.own_deltas[c * 64 + z] : f.quant[f.quant_index[c]][z];
        q[(k * 4 + (size_t)c) * 64 + (size_t)z] = (int32_t)delta << 4;
      }
  }
  first[m] = at;
}
