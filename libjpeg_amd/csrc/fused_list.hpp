// fused_list.hpp -- lists of differently shaped frames through the ragged flavours of the fused kernels, the
// host half that needs no device: which frames share a launch, where a launch's tables lie in the one upload of a call, what
// stands in them.  launch_fused_lists (reconstruct_device.cpp) uploads and launches.  Calls nothing of the HIP runtime: a plain
// host compiler builds tests/cxx/fused_list_tables.cpp around it.  Private to libmijpeg.so.
#pragma once
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
};

// The frames that share a launch: those that agree on kernel and arithmetic flavour, as many as a grid holds
struct FusedListLaunch {
  mij::ReconPlan p;
  std::vector<int> members; // indices into the items
  uint64_t grid;            // workgroups: one per 128 x 128 tile of every member
};

inline uint64_t fused_list_tiles(const mijpeg_info &f) { return (uint64_t)((f.width + 127) / 128) * (uint64_t)((f.height + 127) / 128); }

// Item `item` (frame f, planned as p) into the launch of its kernel and flavour, a new one where there is none or the grid is
// full (2^31 - 1 workgroups).  One outlier beyond the fast gates runs the SAFE flavour alone instead of taking a launch along.
inline void fused_list_add(std::vector<FusedListLaunch> &launches, const mij::ReconPlan &p, int item, const mijpeg_info &f)
{
  const uint64_t tiles = fused_list_tiles(f);
  size_t l = 0;
  while (l < launches.size() && !(launches[l].p.kernel == p.kernel && launches[l].p.fast == p.fast && launches[l].p.wide == p.wide &&
                                  launches[l].p.narrow12 == p.narrow12 && launches[l].grid + tiles <= 0x7fffffffull))
    l++;
  if (l == launches.size()) launches.push_back(FusedListLaunch{p, {}, 0});
  launches[l].members.push_back(item);
  launches[l].grid += tiles;
}

// The tables of a launch of m frames, `at` bytes into the upload: [RaggedFrame x m][first workgroups, m + 1 of them, padded to 16
// bytes][deltas << 4, per frame 4 x 64] and, for planar launches, [PlanarFrame x m]: where its parts begin and where it ends.
// Every part is 16-byte aligned where `at` is.
struct FusedListTable {
  size_t frames, first, deltas, planes, end;
  FusedListTable(size_t at, size_t m, bool planar)
      : frames(at), first(frames + m * sizeof(mij::RaggedFrame)), deltas(first + ((m + 1) * 4 + 15) / 16 * 16), planes(deltas + m * 4 * 64 * sizeof(int32_t)),
        end(planes + (planar ? m * sizeof(mij::PlanarFrame) : 0)) {}
};

// The tables of all launches, one behind the other from offset 0
inline std::vector<FusedListTable> fused_list_layout(const std::vector<FusedListLaunch> &launches, bool planar)
{
  std::vector<FusedListTable> tables;
  for (const FusedListLaunch &l : launches) tables.emplace_back(tables.empty() ? 0 : tables.back().end, l.members.size(), planar);
  return tables;
}

// Launch l's tables into host memory (t: its place there): the frames in member order, frame k with the workgroups
// [first[k], first[k + 1]) -- first[m] is the grid -- and with table k of the deltas, 16 for a component it does not have
inline void fused_list_fill(uint8_t *host, const FusedListTable &t, const FusedListLaunch &l, const FusedListItem *items, bool planar)
{
  const size_t m = l.members.size();
  mij::RaggedFrame *fr = (mij::RaggedFrame *)(host + t.frames);
  uint32_t *first = (uint32_t *)(host + t.first);
  int32_t *q = (int32_t *)(host + t.deltas);
  mij::PlanarFrame *pl = (mij::PlanarFrame *)(host + t.planes);
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
    first[k] = at;
    at += (uint32_t)fused_list_tiles(f);
    for (int c = 0; c < 4; c++)
      for (int z = 0; z < 64; z++) {
        const uint16_t delta = c >= f.components ? 1 : it.own_deltas ? it.own_deltas[c * 64 + z] : f.quant[f.quant_index[c]][z];
        q[(k * 4 + (size_t)c) * 64 + (size_t)z] = (int32_t)delta << 4;
      }
  }
  first[m] = at;
}
