// rect_request.hpp -- the rectangle service (rect_service.cpp: mijpeg_reconstruct_rect, mijpeg_display_rect), the host half that
// needs no device: the frame a request is reconstructed as, what of it the client's bitmaps take, the planes of a launch that does
// not show the plain picture with their row maps and filter windows, the copy into a strided bitmap, the bands and slabs of the
// cached frame's way to the host.  Plain functions over mijpeg_info, RequestPlan and integers; calls nothing of the HIP runtime: a
// plain host compiler builds tests/cxx/rect_request_tables.cpp around it.  Private to libmijpeg.so.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "../../include/mijpeg.h"
#include "kernels.hpp"
#include "request_model.hpp"

// The frame as the reconstruction sees it: the whole picture, or -- without upsampling -- one component at its own
// resolution, which is a single-component identity-transformed frame over that component's coefficient plane
// (BlockBitmapRequester::ReconstructUnsampled with rr_bUpsampling = false: control/blockbitmaprequester.cpp:1013-1074,
// control/bitmapctrl.cpp:273-294; the colour transformation is off then, codestream/rectanglerequest.cpp:157-159).
inline mijpeg_info view_of(const mijpeg_info &f, int comp)
{
  if (comp < 0) return f;
  mijpeg_info v = f;
  v.components = 1;
  v.width = (f.width + f.subx[comp] - 1) / f.subx[comp];
  v.height = (f.height + f.suby[comp] - 1) / f.suby[comp];
  v.hsamp[0] = v.vsamp[0] = v.subx[0] = v.suby[0] = 1;
  v.quant_index[0] = f.quant_index[comp];
  v.blocks_w[0] = f.blocks_w[comp];
  v.blocks_h[0] = f.blocks_h[comp];
  v.mcus_x = v.blocks_w[0];
  v.mcus_y = v.blocks_h[0];
  v.coef_offset[0] = 0;
  v.coef_count = (int64_t)v.blocks_w[0] * v.blocks_h[0] * 64;
  v.range_max[0] = f.range_max[comp];
  v.ycbcr = 0;
  return v;
}

// Frame description for a request that does not show the plain picture: the whole picture, or -- without upsampling --
// the grid of component `view` with every component of the frame on it (the ones that were not asked for are zeros; only
// a colour transformer left over from earlier upsampled requests makes them matter).
inline mijpeg_info request_frame(const mijpeg_info &f, int view, bool all_components)
{
  if (view < 0) return f;
  if (!all_components) return view_of(f, view);
  mijpeg_info v = f;
  v.width = (f.width + f.subx[view] - 1) / f.subx[view];
  v.height = (f.height + f.suby[view] - 1) / f.suby[view];
  for (int c = 0; c < f.components; c++) {
    v.hsamp[c] = v.vsamp[c] = v.subx[c] = v.suby[c] = 1;
    v.blocks_w[c] = f.blocks_w[view];
    v.blocks_h[c] = f.blocks_h[view];
    v.coef_offset[c] = f.coef_offset[view]; // read only where the row map says so: component `view`
    v.quant_index[c] = f.quant_index[view];
    v.range_max[c] = f.range_max[view];
  }
  v.mcus_x = v.blocks_w[0];
  v.mcus_y = v.blocks_h[0];
  return v;
}

// ---- what the bitmaps take: BitmapCtrl::ExtractBitmap (interface/imagebitmap.cpp:58-129) ----
// A block whose corner lies outside the bitmap the hook described is blank -- nothing of it is written; one that starts inside is
// written in full.  -> the last sample of [lo, hi] in a block whose (8-aligned; the first block's: lo) corner is below extent,
// lo - 1 where there is none.
inline int32_t last_inside(int32_t lo, int32_t hi, uint32_t extent)
{
  if ((uint32_t)lo >= extent) return lo - 1;
  const int64_t last_block = ((int64_t)extent - 1) >> 3; // the last block whose (aligned) corner is inside
  return (int32_t)std::min<int64_t>(hi, std::max<int64_t>(last_block, lo >> 3) * 8 + 7);
}

// Per component the last column and line of the plan's region that its bitmap takes
inline void writable_extents(const mij::RequestPlan &p, const uint32_t *bm_w, const uint32_t *bm_h, int ncomp, int32_t *cx1, int32_t *cy1)
{
  for (int c = 0; c < ncomp; c++) {
    cx1[c] = last_inside(p.min_x, p.max_x, bm_w[c]);
    cy1[c] = last_inside(p.min_y, p.max_y, bm_h[c]);
  }
}

// Components with the same writable extent go out together (all of them, normally: one interleaved copy): the last component of
// the run that starts at c, within [c, last]
inline int extent_run_end(const int32_t *cx1, const int32_t *cy1, int c, int last)
{
  int e = c;
  while (e + 1 <= last && cx1[e + 1] == cx1[c] && cy1[e + 1] == cy1[c]) e++;
  return e;
}

// ---- the launch of a request that does not show the plain picture ----
// What such a request adds to a launch (request_model.hpp; GenericArgs::rowmap ...)
struct RequestExtra {
  const int32_t *rowmap_dev;
  int32_t rowmap_stride;
  int32_t corner_x, corner_y, y_base, y_count;
  int32_t wstart[mij::MAXP], wlimit[mij::MAXP]; // per plane (JPEG XT: legacy planes, then residual planes)
  int32_t ycc;
};

// Plane k of that launch: the plan and the component of it that stand behind the plane
struct RequestPlane {
  const mij::RequestPlan *plan;
  int comp;
  bool present;       // false: the component was not asked for -- zeros in every row
  bool identity;      // the plan says nothing about the plane (the residual image of a JPEG XT frame without residual): every row its own
  bool windowed;      // the plane goes through an upsampler in this request: the plan's filter window holds, else [0, lines)
  int32_t lines;      // ... the lines the filter may read off the upsampling path
};

// A plain frame's planes: the components of the request frame g, which without upsampling (view >= 0) all stand for component
// `view` of the frame -- the one plane alone, or (all_on_view) as many planes as the frame has components
inline int plain_planes(const mij::RequestPlan &p, const mijpeg_info &g, bool all_on_view, RequestPlane *planes)
{
  const int vc = p.view;
  for (int c = 0; c < g.components; c++) {
    const int pc = vc >= 0 ? (all_on_view ? c : vc) : c; // component of the frame behind plane c of the request frame
    RequestPlane &k = planes[c];
    k.plan = &p;
    k.comp = pc;
    k.present = p.requested[pc];
    k.identity = false;
    k.windowed = vc < 0 && p.upsampling_path && p.upsampler[pc] && p.requested[pc];
    k.lines = (g.dnl && g.suby[c] > 1) ? g.blocks_h[c] * 8 : (g.height + g.suby[c] - 1) / g.suby[c];
  }
  return g.components;
}

// A JPEG XT frame's planes: three of the legacy image f (plan pl), three of the residual image r (plan pr; identity where the frame
// has no residual).  All three components are asked for (the contract of mijpeg_display_rect).
inline int xt_planes(const mij::RequestPlan &pl, const mij::RequestPlan &pr, const mijpeg_info &f, const mijpeg_info &r, bool no_residual,
                     RequestPlane *planes)
{
  for (int pn = 0; pn < 6; pn++) {
    const mij::RequestPlan &p = pn < 3 ? pl : pr;
    const mijpeg_info &g = pn < 3 ? f : r;
    const int c = pn % 3;
    RequestPlane &k = planes[pn];
    k.plan = &p;
    k.comp = c;
    k.present = true;
    k.identity = pn >= 3 && no_residual;
    k.windowed = p.upsampling_path && p.upsampler[c] && !k.identity;
    k.lines = (f.height + g.suby[c] - 1) / std::max(1, g.suby[c]);
  }
  return 6;
}

// Row maps, `stride` entries per plane into out[n * stride]: identity outside what the plan defines; planes that are not present
// are zeros (-1).  (A component that appears in no scan carries coefficients that transform to zeros in every row: host_decoder.cpp.)
// *all_zero: no colour transformation and no row of the plans that is not zeros -- every sample the request shows is 0.
inline void fill_rowmaps(const RequestPlane *planes, int n, int stride, bool ycc, int32_t *out, bool *all_zero)
{
  *all_zero = !ycc;
  for (int k = 0; k < n; k++) {
    const RequestPlane &pn = planes[k];
    const mij::RequestPlan &p = *pn.plan;
    const int c = pn.comp;
    int32_t *m = out + (size_t)k * stride;
    for (int g = 0; g < stride; g++) m[g] = pn.present ? g : -1;
    if (!pn.present || pn.identity) continue;
    for (int g = p.g0[c]; g <= p.g1[c] && g < stride && g < (int)p.rowmap[c].size(); g++) {
      m[g] = p.rowmap[c][(size_t)g];
      if (m[g] >= 0) *all_zero = false;
    }
  }
}

// ... and the rest of what the launch takes (rowmap_dev: the caller's, once the maps are on the device); p: the plan that places
// the request (the legacy image's)
inline RequestExtra request_extra(const RequestPlane *planes, int n, const mij::RequestPlan &p, int stride, int y_count, bool ycc)
{
  RequestExtra rx;
  memset(&rx, 0, sizeof(rx));
  rx.rowmap_stride = stride;
  rx.corner_x = p.corner_x;
  rx.corner_y = p.corner_y;
  rx.y_base = p.min_y;
  rx.y_count = y_count;
  rx.ycc = ycc ? 1 : 0;
  for (int k = 0; k < n; k++) {
    rx.wstart[k] = planes[k].windowed ? planes[k].plan->wstart[planes[k].comp] : 0;
    rx.wlimit[k] = planes[k].windowed ? planes[k].plan->wlimit[planes[k].comp] : planes[k].lines;
  }
  return rx;
}

// ---- the interleaved image a frame or a request is reconstructed into, and its way into the bitmaps ----
struct RequestImage {
  int nc, sb;                             // samples per pixel, bytes per sample
  size_t row, padded;                     // bytes per line (8-byte aligned: wide stores in the kernel), bytes in all
  int plane_of[MIJPEG_MAX_COMPONENTS];    // the sample of a pixel that holds component c of the client's bitmaps
};

// g: the frame as reconstructed; sb_default: bytes per sample where the frame does not say; view, all_on_view: as request_frame
inline RequestImage request_image(const mijpeg_info &g, int sb_default, int view = -1, bool all_on_view = false)
{
  RequestImage im;
  im.nc = g.components;
  im.sb = g.sample_bytes > 0 ? g.sample_bytes : sb_default;
  im.row = ((size_t)g.width * im.nc * im.sb + 7) & ~(size_t)7;
  im.padded = im.row * g.height;
  for (int c = 0; c < MIJPEG_MAX_COMPONENTS; c++) im.plane_of[c] = view >= 0 ? (all_on_view ? c : 0) : c;
  return im;
}

// Columns [x0, x1], lines [y0, y1] of samples [p0, p1] of the image at src, for launch_scatter_rect; the bitmaps: scatter_plane
inline mij::ScatterArgs scatter_args(const uint8_t *src, const RequestImage &im, int x0, int y0, int x1, int y1, int p0, int p1)
{
  mij::ScatterArgs a;
  memset(&a, 0, sizeof(a));
  a.src = src;
  a.src_row = (int64_t)im.row;
  a.ncomp = im.nc;
  a.sample_bytes = im.sb;
  a.x0 = x0;
  a.y0 = y0;
  a.w = x1 - x0 + 1;
  a.h = y1 - y0 + 1;
  a.c0 = p0;
  a.c1 = p1;
  return a;
}
inline void scatter_plane(mij::ScatterArgs &a, int plane, void *dst, int32_t bytes_per_pixel, int32_t bytes_per_row)
{
  a.dst[plane] = (uint8_t *)dst;
  a.bytes_per_pixel[plane] = bytes_per_pixel;
  a.bytes_per_row[plane] = bytes_per_row;
}

// The same on the host: sample `plane` of columns [x0, x1], lines [y0, y1] of the image at img into a bitmap described like the
// reference's ImageBitMap (dst: canvas pixel (0, 0))
inline void copy_plane_rect(const uint8_t *img, const RequestImage &im, int plane, int x0, int y0, int x1, int y1, void *dst, int32_t bpp,
                            int32_t bpr)
{
  const int n = x1 - x0 + 1, nc = im.nc;
  for (int y = y0; y <= y1; y++) {
    const uint8_t *src = img + (size_t)y * im.row + ((size_t)x0 * nc + plane) * im.sb;
    uint8_t *out = (uint8_t *)dst + (ptrdiff_t)y * bpr + (ptrdiff_t)x0 * bpp;
    if (im.sb == 1) {
      if (nc == 1 && bpp == 1) memcpy(out, src, (size_t)n);
      else
        for (int x = 0; x < n; x++) out[(ptrdiff_t)x * bpp] = src[(size_t)x * nc];
    } else {
      for (int x = 0; x < n; x++) memcpy(out + (ptrdiff_t)x * bpp, src + (size_t)x * nc * 2, 2);
    }
  }
}

// ---- the cached frame's way to the host: bands of lines, one event each; big copies in slabs over the worker pool ----
// Bands of about band_mib MiB (at least 8 lines, a multiple of 8); band_mib <= 0: one band
inline int band_lines(long band_mib, size_t row, int height)
{
  return band_mib <= 0 ? height : (int)std::max<size_t>(8, (((size_t)band_mib << 20) / std::max<size_t>(row, 1) + 7) & ~(size_t)7);
}
inline int band_count(int height, int lines) { return (height + lines - 1) / lines; }
inline int band_of(int line, int lines) { return line / lines; }

// Workers for a copy of `lines` lines of line_bytes: one per 4 MiB, at most 16 and what the pool has (<= 1: the caller copies)
inline int copy_parts(size_t line_bytes, int lines, int threads)
{
  return (int)std::min<size_t>((size_t)std::min(threads, 16), line_bytes * lines / (4u << 20));
}
// ... which copy slab k while the bands of slab k + 1 are still arriving: up to four slabs of at least eight bands
inline int slab_count(int lines, int band) { return std::min(4, std::max(1, lines / (8 * band))); }
// Slab k of `slabs` over the lines from min_y: [*s0, *s1)
inline void slab_bounds(int min_y, int lines, int slabs, int k, int *s0, int *s1)
{
  *s0 = min_y + (int)((int64_t)lines * k / slabs);
  *s1 = min_y + (int)((int64_t)lines * (k + 1) / slabs);
}
// Worker i of `parts` in the slab [s0, s1): [*y0, *y1)
inline void worker_lines(int s0, int s1, int parts, int i, int *y0, int *y1)
{
  *y0 = s0 + (int)((int64_t)(s1 - s0) * i / parts);
  *y1 = s0 + (int)((int64_t)(s1 - s0) * (i + 1) / parts);
}
