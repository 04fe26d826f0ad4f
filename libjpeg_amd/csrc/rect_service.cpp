// rect_service.cpp -- the rectangle service of the decoder object: mijpeg_reconstruct_rect (every request answered from the plain
// picture, reconstructed once and cached) and mijpeg_display_rect (JPEG::DisplayRectangle as a sequence of calls:
// request_model.hpp plans, this serves), with the diagnostics mijpeg_display_plan / mijpeg_display_cursor.  The arithmetic that
// needs no device is in rect_request.hpp.  Private to libmijpeg.so.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "../../include/mijpeg.h"
#include "decoder.hpp"
#include "kernels.hpp"
#include "reconstruct.hpp"
#include "rect_request.hpp"

using namespace mij;
using clk = std::chrono::steady_clock;

namespace {
// The client's bitmaps, taken apart (mijpeg_bitmap; the ImageBitMap of the reference's hook)
struct Bitmaps {
  void *dst[MIJPEG_MAX_COMPONENTS];
  int32_t bpp[MIJPEG_MAX_COMPONENTS], bpr[MIJPEG_MAX_COMPONENTS];
};
struct Rect { int32_t x0, y0, x1, y1; }; // inclusive
} // namespace

// ------------------------------------------------------------------------------------------------
// the plain picture: reconstructed once per (stream, flags, view), served rectangle by rectangle
// ------------------------------------------------------------------------------------------------
// d->img_dev holds the frame f (image im) for (flags, view), or does when this returns
static int ensure_frame(mijpeg_decoder *d, const RequestImage &im, int view, uint32_t flags, bool to_device)
{
  if (d->img_valid && d->img_flags == flags && d->img_view == view) return MIJPEG_OK;
  HIP_TRY(d, hipSetDevice(d->device));
  int rc = ensure_dev(d, (void **)&d->img_dev, &d->img_dev_cap, im.padded);
  if (rc) return rc;
  auto t0 = clk::now();
  HIP_TRY(d, hipStreamSynchronize(d->stream)); // uploads complete
  auto t1 = clk::now();
  rc = reconstruct_view(d, view, d->img_dev, (int64_t)im.row, flags, to_device ? 1 : 0); // host requests: the copy follows in stream order
  if (rc) return rc;
  d->timing[1] = std::chrono::duration<double>(t1 - t0).count();
  d->timing[2] = std::chrono::duration<double>(clk::now() - t1).count();
  d->timing[3] = 0;
  d->img_valid = true;
  d->img_host_valid = false;
  d->img_flags = flags;
  d->img_view = view;
  return MIJPEG_OK;
}

// The frame's copy in d->img_host: bands of about 4 MiB, all of them enqueued now and waited for as they are asked for
static int enqueue_bands(mijpeg_decoder *d, const RequestImage &im, int height)
{
  HIP_TRY(d, hipSetDevice(d->device));
  if (const int prc = ensure_cached(d, true, (void **)&d->img_host, &d->img_host_cap, im.padded)) return prc;
  static const long band_mib = getenv("MIJPEG_RECT_BAND_MIB") ? atol(getenv("MIJPEG_RECT_BAND_MIB")) : 4; // tuning; <= 0: one band
  d->band_lines = band_lines(band_mib, im.row, height);
  d->bands = band_count(height, d->band_lines);
  while ((int)d->band_events.size() < d->bands) {
    hipEvent_t e;
    HIP_TRY(d, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    d->band_events.push_back(e);
  }
  for (int b = 0; b < d->bands; b++) {
    const size_t y0 = (size_t)b * d->band_lines, y1 = std::min<size_t>(height, y0 + d->band_lines);
    HIP_TRY(d, hipMemcpyAsync(d->img_host + y0 * im.row, d->img_dev + y0 * im.row, (y1 - y0) * im.row, hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(d, hipEventRecord(d->band_events[(size_t)b], d->stream));
  }
  d->bands_waited = 0;
  d->img_host_valid = true;
  return MIJPEG_OK;
}

// bands [0, upto] of the host copy have arrived when this returns
static int wait_bands(mijpeg_decoder *d, int upto)
{
  auto t2 = clk::now();
  for (; d->bands_waited <= upto && d->bands_waited < d->bands; d->bands_waited++)
    HIP_TRY(d, hipEventSynchronize(d->band_events[(size_t)d->bands_waited]));
  d->timing[3] += std::chrono::duration<double>(clk::now() - t2).count();
  return MIJPEG_OK;
}

static int launch_scatter(mijpeg_decoder *d, const ScatterArgs &a)
{
  if (launch_scatter_rect(a, d->stream)) return hip_fail(d, hipGetLastError(), "scatter_rect_kernel launch");
  return MIJPEG_OK;
}

static int scatter_frame(mijpeg_decoder *d, const RequestImage &im, const Rect &r, int c0, int c1, const Bitmaps &bm)
{
  ScatterArgs a = scatter_args(d->img_dev, im, r.x0, r.y0, r.x1, r.y1, c0, c1);
  for (int c = 0; c < im.nc; c++) scatter_plane(a, c, bm.dst[c], bm.bpp[c], bm.bpr[c]);
  HIP_TRY(d, hipSetDevice(d->device));
  if (const int rc = launch_scatter(d, a)) return rc;
  HIP_TRY(d, hipStreamSynchronize(d->stream));
  return MIJPEG_OK;
}

// interleaved destination (the layout cmd/bitmaphook.cpp hands out): whole lines at once
static bool interleaved_bitmaps(const RequestImage &im, int c0, int c1, const Bitmaps &bm)
{
  bool interleaved = c0 == 0 && c1 == im.nc - 1 && bm.dst[0];
  for (int c = 0; c < im.nc && interleaved; c++)
    interleaved = bm.dst[c] == (uint8_t *)bm.dst[0] + c * im.sb && bm.bpp[c] == im.nc * im.sb && bm.bpr[c] == bm.bpr[0];
  return interleaved;
}

static int copy_interleaved(mijpeg_decoder *d, const RequestImage &im, const Rect &r, const Bitmaps &bm)
{
  const size_t px = (size_t)im.nc * im.sb, line = (size_t)(r.x1 - r.x0 + 1) * px;
  const int lines = r.y1 - r.y0 + 1;
  auto copy_lines = [&](int y0, int y1) {
    for (int y = y0; y < y1; y++)
      memcpy((uint8_t *)bm.dst[0] + (ptrdiff_t)y * bm.bpr[0] + (ptrdiff_t)r.x0 * px, d->img_host + (size_t)y * im.row + (size_t)r.x0 * px, line);
  };
  // big rectangles (whole frames) are copied by the worker pool, one memcpy stream per worker, in a few slabs: the
  // workers copy slab k while the bands of slab k + 1 are still arriving
  const int parts = copy_parts(line, lines, default_threads());
  if (parts <= 1) {
    if (const int rc = wait_bands(d, band_of(r.y1, d->band_lines))) return rc;
    copy_lines(r.y0, r.y1 + 1);
    return MIJPEG_OK;
  }
  const int slabs = slab_count(lines, d->band_lines);
  for (int k = 0; k < slabs; k++) {
    int s0, s1;
    slab_bounds(r.y0, lines, slabs, k, &s0, &s1);
    if (const int rc = wait_bands(d, band_of(s1 - 1, d->band_lines))) return rc;
    parallel_for(parts, [&](int i) {
      int y0, y1;
      worker_lines(s0, s1, parts, i, &y0, &y1);
      copy_lines(y0, y1);
    });
  }
  return MIJPEG_OK;
}

static int copy_strided(mijpeg_decoder *d, const RequestImage &im, const Rect &r, int c0, int c1, const Bitmaps &bm)
{
  if (const int rc = wait_bands(d, band_of(r.y1, d->band_lines))) return rc;
  for (int c = c0; c <= c1; c++)
    if (bm.dst[c]) copy_plane_rect(d->img_host, im, c, r.x0, r.y0, r.x1, r.y1, bm.dst[c], bm.bpp[c], bm.bpr[c]);
  return MIJPEG_OK;
}

// The rectangle r (on the grid of `view`: the canvas, or a component's own samples) of the plain picture, components
// [min_comp, max_comp] of the view, into the bitmaps.  The whole frame is reconstructed once per (stream, flags, view) and then
// served rectangle by rectangle, which is what the stripe loop of cmd/reconstruct.cpp:334-342 asks for.
static int serve_rect(mijpeg_decoder *d, int view, uint32_t flags, bool to_device, Rect r, int32_t min_comp, int32_t max_comp, const Bitmaps &bm)
{
  const mijpeg_info f = view_of(d->host.info, view);
  const RequestImage im = request_image(f, 1);
  if (const int rc = ensure_frame(d, im, view, flags, to_device)) return rc;
  if (!to_device && !d->img_host_valid)
    if (const int rc = enqueue_bands(d, im, f.height)) return rc;
  r.x0 = std::max(r.x0, 0);
  r.y0 = std::max(r.y0, 0);
  if (r.x1 >= f.width) r.x1 = f.width - 1;
  if (r.y1 >= f.height) r.y1 = f.height - 1;
  if (min_comp < 0) min_comp = 0;
  if (max_comp >= im.nc) max_comp = im.nc - 1;
  // an empty request after clipping is served by doing nothing (codestream/rectanglerequest.cpp clips alike)
  if (r.x0 > r.x1 || r.y0 > r.y1 || min_comp > max_comp) return MIJPEG_OK;
  if (to_device) return scatter_frame(d, im, r, min_comp, max_comp, bm);
  if (interleaved_bitmaps(im, min_comp, max_comp, bm)) return copy_interleaved(d, im, r, bm);
  return copy_strided(d, im, r, min_comp, max_comp, bm);
}

// mijpeg_reconstruct_rect behind its NULL checks: the flags taken apart, the view of a request without upsampling
static int reconstruct_rect(mijpeg_decoder *d, Rect r, int32_t min_comp, int32_t max_comp, uint32_t flags, const Bitmaps &bm)
{
  if (d->device < 0) return set_error(d, MIJPEG_ERR_DEVICE, "decoder was created without a device: no reconstruction path");
  if (!d->uploaded) return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "no decoded coefficients: call mijpeg_decode_coefficients first");
  const bool to_device = (flags & MIJPEG_FLAG_DEVICE_OUTPUT) != 0;
  const bool unsampled = (flags & MIJPEG_FLAG_NO_UPSAMPLING) != 0;
  flags &= ~(MIJPEG_FLAG_DEVICE_OUTPUT | MIJPEG_FLAG_NO_UPSAMPLING);
  if (!unsampled) return serve_rect(d, -1, flags, to_device, r, min_comp, max_comp, bm);
  // control/bitmapctrl.cpp:273-294: one component at a time, no colour transformation, and the rectangle (given
  // on the canvas) shrinks to the component's grid
  if (min_comp < 0) min_comp = 0;
  if (max_comp >= d->host.info.components) max_comp = d->host.info.components - 1;
  if (min_comp != max_comp)
    return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "if upsampling is disabled, components can only be reconstructed one by one");
  if (d->host.is_xt())
    return set_error(d, MIJPEG_ERR_OPERATION_UNIMPLEMENTED, "JPEG XT frames are not reconstructed without upsampling (the reference merges the component with residual scratch buffers it never initialised)");
  const int view = min_comp; // component whose own sample grid is reconstructed
  const int sx = d->host.info.subx[view], sy = d->host.info.suby[view];
  r = Rect{(std::max(r.x0, 0) + sx - 1) / sx, (std::max(r.y0, 0) + sy - 1) / sy, (r.x1 + sx) / sx - 1, (r.y1 + sy) / sy - 1};
  Bitmaps v = bm; // the view has one component, number 0
  v.dst[0] = bm.dst[view];
  v.bpp[0] = bm.bpp[view];
  v.bpr[0] = bm.bpr[view];
  return serve_rect(d, view, flags | MIJPEG_FLAG_NO_COLOR_TRANSFORM, to_device, r, 0, 0, v);
}

// ------------------------------------------------------------------------------------------------
// JPEG::DisplayRectangle as a sequence of calls
// ------------------------------------------------------------------------------------------------
// The request models of a decoded image start with its first DisplayRectangle call (every decode resets them): one for a plain
// frame; two for a JPEG XT frame -- legacy and residual image share m_bSubsampling (request_model.hpp)
static void ensure_request_models(mijpeg_decoder *d)
{
  if (d->model_valid) return;
  const mijpeg_info &f = d->host.info;
  if (d->host.is_xt() && f.components == 3) {
    const mijpeg_info &r = d->host.xt.residual;
    bool lsub = false, rsub = false;
    for (int c = 0; c < 3; c++) {
      lsub = lsub || f.subx[c] > 1 || f.suby[c] > 1;
      rsub = rsub || r.subx[c] > 1 || r.suby[c] > 1;
    }
    d->model.reset(3, f.width, f.height, f.subx, f.suby, true, false, nullptr, nullptr, rsub);
    d->rmodel.reset(3, f.width, f.height, r.subx, r.suby, true, false, nullptr, nullptr, lsub);
  } else
    d->model.reset(f.components, f.width, f.height, f.subx, f.suby, f.ycbcr != 0, f.dnl != 0, f.rows, f.blocks_h);
  d->model_valid = true;
}

namespace {
// One mijpeg_display_rect call on its way through the stages below
struct DisplayRequest {
  mijpeg_decoder *d;
  Rect r;
  int32_t min_comp, max_comp; // clipped to the frame
  uint32_t flags;             // as given
  bool to_device, upsample, ctrafo;
  uint32_t pass;              // the flags that reach the kernel selection
  Bitmaps bm;
  uint32_t bm_w[MIJPEG_MAX_COMPONENTS], bm_h[MIJPEG_MAX_COMPONENTS];
  bool xt;                    // a JPEG XT frame inside the contract: both images follow the request
  RequestPlan p, pr;          // the plan (XT: of the legacy image; pr: of the residual image, p again where there is none)
  int32_t cx1[MIJPEG_MAX_COMPONENTS], cy1[MIJPEG_MAX_COMPONENTS]; // writable extents
  // a request that is not the plain picture: the frame the generic kernels see, its planes, the image they write
  mijpeg_info frame;
  const int16_t *coef;
  uint32_t launch_flags;
  bool ycc;
  RequestPlane planes[MAXP];
  int nplanes, stride, y_count;
  RequestImage im;
};
} // namespace

static void take_request(DisplayRequest &q, mijpeg_decoder *d, const Rect &r, int32_t min_comp, int32_t max_comp, uint32_t flags,
                         const mijpeg_bitmap *bitmaps)
{
  q.d = d;
  q.r = r;
  q.flags = flags;
  q.to_device = (flags & MIJPEG_FLAG_DEVICE_OUTPUT) != 0;
  q.upsample = !(flags & MIJPEG_FLAG_NO_UPSAMPLING);
  q.ctrafo = !(flags & MIJPEG_FLAG_NO_COLOR_TRANSFORM);
  q.pass = flags & (MIJPEG_FLAG_FORCE_GENERIC | MIJPEG_FLAG_FORCE_SAFE);
  q.min_comp = std::max(min_comp, 0);
  q.max_comp = max_comp >= d->host.info.components ? d->host.info.components - 1 : max_comp;
  for (int c = 0; c < MIJPEG_MAX_COMPONENTS; c++) {
    q.bm.dst[c] = bitmaps[c].data;
    q.bm.bpp[c] = bitmaps[c].bytes_per_pixel;
    q.bm.bpr[c] = bitmaps[c].bytes_per_row;
    q.bm_w[c] = bitmaps[c].width;
    q.bm_h[c] = bitmaps[c].height;
  }
}

// JPEG XT outside the contract -- a component subset merges with whatever m_ppDTemp holds from the block before, a request without
// the transformation builds another transformer --: served as the plain picture, the block rows the bitmaps' heights allow
static int xt_plain_picture(DisplayRequest &q)
{
  uint32_t maxmcu = 0xffffffffu;
  for (int c = q.min_comp; c <= q.max_comp; c++) maxmcu = std::min(maxmcu, (q.bm_h[c] >> 3) - 1u);
  if (maxmcu != 0xffffffffu && (int64_t)q.r.y1 > (int64_t)maxmcu * 8 + 7) q.r.y1 = (int32_t)(maxmcu * 8 + 7);
  if (q.r.y1 < q.r.y0) return MIJPEG_OK;
  return mijpeg_reconstruct_rect(q.d, q.r.x0, q.r.y0, q.r.x1, q.r.y1, q.min_comp, q.max_comp, q.flags, q.bm.dst, q.bm.bpp, q.bm.bpr);
}

// The request through the model, or -- JPEG XT: the residual image has row cursors and upsamplers of its own beside the legacy
// image's (control/blockbitmaprequester.cpp:228-232, 356-372, 1118-1146, 1197-1222) -- through one model per image, fed the same
// request.  -> nothing is shown
static bool plan_request(DisplayRequest &q)
{
  mijpeg_decoder *d = q.d;
  ensure_request_models(d);
  if (!q.xt) {
    q.p = d->model.request(q.r.x0, q.r.y0, q.r.x1, q.r.y1, q.min_comp, q.max_comp, q.upsample, q.ctrafo, q.bm_h);
    return q.p.nothing;
  }
  q.p = d->model.request(q.r.x0, q.r.y0, q.r.x1, q.r.y1, 0, 2, true, true, q.bm_h);
  q.pr = d->host.xt.no_residual ? q.p : d->rmodel.request(q.r.x0, q.r.y0, q.r.x1, q.r.y1, 0, 2, true, true, q.bm_h);
  q.p.plain = q.p.plain && (d->host.xt.no_residual || q.pr.plain);
  return q.p.nothing;
}

// JPEG XT: a residual component without an upsampler whose cursor stands behind its last row: `rrow->BlockAt(x)` on a NULL row
// (:1057-1058, :1201-1202) -- the reference does not survive this request
static int refuse_null_residual_row(const DisplayRequest &q)
{
  if (!q.xt || q.d->host.xt.no_residual) return MIJPEG_OK;
  const RequestPlan &pr = q.pr;
  for (int c = 0; c < 3; c++)
    if (!(pr.upsampling_path && pr.upsampler[c]))
      for (int g = pr.g0[c]; g <= pr.g1[c]; g++)
        if (g >= (int)pr.rowmap[c].size() || pr.rowmap[c][(size_t)g] < 0)
          return set_error(q.d, MIJPEG_ERR_OBJECT_DOESNT_EXIST,
                           "the request walks the residual image's row cursor behind its last row (the reference dereferences a NULL row here)");
  return MIJPEG_OK;
}

// One run [c, e] of components with the same writable extent out of the cached plain picture.  A JPEG XT frame goes through
// mijpeg_reconstruct_rect with the request's own flags; a plain frame with the transformer the model says is in force, without
// upsampling as the view of its one component.
static int serve_plain_run(DisplayRequest &q, int c, int e)
{
  mijpeg_decoder *d = q.d;
  const RequestPlan &p = q.p;
  const Rect r{p.min_x, p.min_y, q.cx1[c], q.cy1[c]};
  if (q.xt) return mijpeg_reconstruct_rect(d, r.x0, r.y0, r.x1, r.y1, c, e, q.flags, q.bm.dst, q.bm.bpp, q.bm.bpr);
  const int vc = p.view; // without upsampling the single component of the view is number 0 there
  const uint32_t fl = q.pass | (p.ycc || !d->host.info.ycbcr ? 0u : MIJPEG_FLAG_NO_COLOR_TRANSFORM) | (vc >= 0 ? MIJPEG_FLAG_NO_COLOR_TRANSFORM : 0u);
  if (vc < 0) return serve_rect(d, -1, fl, q.to_device, r, c, e, q.bm);
  const Bitmaps v{{q.bm.dst[vc], nullptr, nullptr, nullptr}, {q.bm.bpp[vc], 0, 0, 0}, {q.bm.bpr[vc], 0, 0, 0}};
  return serve_rect(d, vc, fl, q.to_device, r, 0, 0, v);
}

static int serve_plain_picture(DisplayRequest &q)
{
  const int last = q.xt ? 2 : q.max_comp;
  for (int c = q.xt ? 0 : q.min_comp, e; c <= last; c = e + 1) {
    e = extent_run_end(q.cx1, q.cy1, c, last);
    if (q.cx1[c] < q.p.min_x || q.cy1[c] < q.p.min_y) continue;
    if (const int rc = serve_plain_run(q, c, e)) return rc;
  }
  return MIJPEG_OK;
}

// ---- not the plain picture: row maps, zeros, displaced upsampler output -> the generic kernels on this request's lines ----
// The frame the kernels see, its planes, the image they write.  JPEG XT: both images, 16-bit samples unless the frame says otherwise.
static void build_planes(DisplayRequest &q)
{
  const mijpeg_info &f = q.d->host.info;
  const int vc = q.xt ? -1 : q.p.view;
  const bool all_on_view = vc >= 0 && q.p.ycc;
  q.frame = request_frame(f, vc, all_on_view);
  q.ycc = q.xt || q.p.ycc;
  q.stride = 1;
  if (q.xt) {
    const mijpeg_info &r = q.d->host.xt.residual;
    q.nplanes = xt_planes(q.p, q.pr, f, r, q.d->host.xt.no_residual, q.planes);
    for (int c = 0; c < 3; c++) q.stride = std::max(q.stride, std::max(f.blocks_h[c], r.blocks_h[c]));
    q.launch_flags = q.pass | MIJPEG_FLAG_FORCE_GENERIC;
  } else {
    q.frame.ycbcr = q.p.ycc ? 1 : 0;
    q.nplanes = plain_planes(q.p, q.frame, all_on_view, q.planes);
    for (int c = 0; c < q.nplanes; c++) q.stride = std::max(q.stride, q.frame.blocks_h[c]);
    q.launch_flags = q.pass | MIJPEG_FLAG_FORCE_GENERIC | (q.p.ycc ? 0u : MIJPEG_FLAG_NO_COLOR_TRANSFORM);
  }
  q.coef = q.d->coef_dev + (vc >= 0 && !all_on_view ? f.coef_offset[vc] : 0);
  q.im = request_image(q.frame, q.xt ? 2 : 1, vc, all_on_view);
  q.y_count = q.p.max_y - q.p.min_y + 1;
}

// The request's lines into d->req_dev: the row maps to the device and the generic kernels over them
static int launch_request(DisplayRequest &q, const std::vector<int32_t> &maps)
{
  mijpeg_decoder *d = q.d;
  const int rc = ensure_dev(d, (void **)&d->rowmap_dev, &d->rowmap_cap, maps.size() * sizeof(int32_t));
  if (rc) return rc;
  HIP_TRY(d, hipMemcpyAsync(d->rowmap_dev, maps.data(), maps.size() * sizeof(int32_t), hipMemcpyHostToDevice, d->stream));
  HIP_TRY(d, hipStreamSynchronize(d->stream)); // `maps` is pageable and leaves scope; uploads of the coefficients are complete too
  mijpeg_batch b = batch_of(q.frame, q.coef, d->req_dev, (int64_t)q.im.row, (int64_t)q.im.padded, 1, q.launch_flags);
  if (q.xt) b.xt = &d->host.xt;
  RequestExtra rx = request_extra(q.planes, q.nplanes, q.p, q.stride, q.y_count, q.ycc);
  rx.rowmap_dev = d->rowmap_dev;
  return reconstruct_on(d, b, &rx, "request");
}

static int reconstruct_request(DisplayRequest &q)
{
  mijpeg_decoder *d = q.d;
  if (const int rc = ensure_dev(d, (void **)&d->req_dev, &d->req_dev_cap, q.im.padded)) return rc;
  std::vector<int32_t> maps((size_t)q.nplanes * q.stride);
  bool all_zero;
  fill_rowmaps(q.planes, q.nplanes, q.stride, q.ycc, maps.data(), &all_zero);
  if (!all_zero) return launch_request(q, maps);
  // every sample the request shows is the transform of "no row": 0 through the filters and the identity transformation
  HIP_TRY(d, hipMemsetAsync(d->req_dev + (size_t)q.p.min_y * q.im.row, 0, (size_t)q.y_count * q.im.row, d->stream));
  return MIJPEG_OK;
}

// does component c's bitmap take anything of the request?
static bool takes(const DisplayRequest &q, int c) { return q.bm.dst[c] && q.cx1[c] >= q.p.min_x && q.cy1[c] >= q.p.min_y; }

// The lines the request reconstructed into d->req_dev go out to the client's bitmaps: columns [min_x, cx1[c]], lines
// [min_y, cy1[c]] of component c
static int hand_out_device(DisplayRequest &q, int c0, int c1)
{
  mijpeg_decoder *d = q.d;
  for (int c = c0; c <= c1; c++) {
    if (!takes(q, c)) continue;
    const int plane = q.im.plane_of[c];
    ScatterArgs a = scatter_args(d->req_dev, q.im, q.p.min_x, q.p.min_y, q.cx1[c], q.cy1[c], plane, plane);
    scatter_plane(a, plane, q.bm.dst[c], q.bm.bpp[c], q.bm.bpr[c]);
    if (const int rc = launch_scatter(d, a)) return rc;
  }
  HIP_TRY(d, hipStreamSynchronize(d->stream));
  return MIJPEG_OK;
}

static int hand_out_host(DisplayRequest &q, int c0, int c1)
{
  mijpeg_decoder *d = q.d;
  const RequestPlan &p = q.p;
  if (const int prc = ensure_pinned(d, &d->req_host, &d->req_host_cap, q.im.padded)) return prc;
  HIP_TRY(d, hipMemcpyAsync(d->req_host + (size_t)p.min_y * q.im.row, d->req_dev + (size_t)p.min_y * q.im.row, (size_t)q.y_count * q.im.row,
                            hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(d, hipStreamSynchronize(d->stream));
  for (int c = c0; c <= c1; c++)
    if (takes(q, c)) copy_plane_rect(d->req_host, q.im, q.im.plane_of[c], p.min_x, p.min_y, q.cx1[c], q.cy1[c], q.bm.dst[c], q.bm.bpp[c], q.bm.bpr[c]);
  return MIJPEG_OK;
}

static int serve_request(DisplayRequest &q)
{
  HIP_TRY(q.d, hipSetDevice(q.d->device));
  build_planes(q);
  if (const int rc = reconstruct_request(q)) return rc;
  const int c0 = q.xt ? 0 : q.min_comp, c1 = q.xt ? 2 : q.max_comp;
  return q.to_device ? hand_out_device(q, c0, c1) : hand_out_host(q, c0, c1);
}

extern "C" {

int mijpeg_reconstruct_rect(mijpeg_decoder *d, int32_t min_x, int32_t min_y, int32_t max_x, int32_t max_y, int32_t min_comp,
                            int32_t max_comp, uint32_t flags, void *const dst[MIJPEG_MAX_COMPONENTS],
                            const int32_t bytes_per_pixel[MIJPEG_MAX_COMPONENTS],
                            const int32_t bytes_per_row[MIJPEG_MAX_COMPONENTS])
try {
  if (!d || !dst || !bytes_per_pixel || !bytes_per_row) return MIJPEG_ERR_INVALID_PARAMETER;
  Bitmaps bm;
  for (int c = 0; c < MIJPEG_MAX_COMPONENTS; c++) {
    bm.dst[c] = dst[c];
    bm.bpp[c] = bytes_per_pixel[c];
    bm.bpr[c] = bytes_per_row[c];
  }
  return reconstruct_rect(d, Rect{min_x, min_y, max_x, max_y}, min_comp, max_comp, flags, bm);
} catch (...) { return boundary_catch(d, "mijpeg_reconstruct_rect"); }

int mijpeg_display_rect(mijpeg_decoder *d, int32_t min_x, int32_t min_y, int32_t max_x, int32_t max_y, int32_t min_comp, int32_t max_comp,
                        uint32_t flags, const mijpeg_bitmap bitmaps[MIJPEG_MAX_COMPONENTS])
try {
  if (!d || !bitmaps) return MIJPEG_ERR_INVALID_PARAMETER;
  if (d->device < 0) return set_error(d, MIJPEG_ERR_DEVICE, "decoder was created without a device: no reconstruction path");
  if (!d->uploaded) return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "no decoded coefficients: call mijpeg_decode_coefficients first");
  DisplayRequest q;
  take_request(q, d, Rect{min_x, min_y, max_x, max_y}, min_comp, max_comp, flags, bitmaps);
  if (!q.upsample && q.min_comp != q.max_comp && q.min_comp <= q.max_comp)
    return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "if upsampling is disabled, components can only be reconstructed one by one");
  // JPEG XT, in the contract: what the reference's command line asks for -- all three components, upsampling and colour
  // transformation on -- with any order and size of rectangles
  q.xt = d->host.is_xt();
  if (q.xt && (!q.upsample || !q.ctrafo || q.min_comp != 0 || q.max_comp != 2 || d->host.info.components != 3)) return xt_plain_picture(q);
  if (plan_request(q)) return MIJPEG_OK;
  if (const int rc = refuse_null_residual_row(q)) return rc;
  writable_extents(q.p, q.bm_w, q.bm_h, q.xt ? 3 : d->host.info.components, q.cx1, q.cy1);
  return q.p.plain ? serve_plain_picture(q) : serve_request(q);
} catch (...) { return boundary_catch(d, "mijpeg_display_rect"); }

int mijpeg_display_plan(mijpeg_decoder *d, int32_t min_x, int32_t min_y, int32_t max_x, int32_t max_y, int32_t min_comp, int32_t max_comp,
                        uint32_t flags, const uint32_t bm_height[MIJPEG_MAX_COMPONENTS], int32_t out[8 + 6 * MIJPEG_MAX_COMPONENTS])
try {
  if (!d || !bm_height || !out) return MIJPEG_ERR_INVALID_PARAMETER;
  if (d->host.info.components < 1 || d->host.info.width < 1) return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "no parsed stream: call mijpeg_read_header first");
  const mijpeg_info &f = d->host.info;
  ensure_request_models(d);
  const RequestPlan p = d->model.request(min_x, min_y, max_x, max_y, min_comp, max_comp, !(flags & MIJPEG_FLAG_NO_UPSAMPLING),
                                         !(flags & MIJPEG_FLAG_NO_COLOR_TRANSFORM), bm_height);
  bool rplain = true;
  if (d->host.is_xt() && f.components == 3 && !d->host.xt.no_residual) // (the residual image: cursors through mijpeg_display_cursor(4 + c))
    rplain = d->rmodel.request(min_x, min_y, max_x, max_y, min_comp, max_comp, !(flags & MIJPEG_FLAG_NO_UPSAMPLING),
                               !(flags & MIJPEG_FLAG_NO_COLOR_TRANSFORM), bm_height).plain;
  out[0] = p.nothing; out[1] = p.plain && rplain; out[2] = p.ycc; out[3] = p.view;
  out[4] = p.min_x; out[5] = p.min_y; out[6] = p.max_x; out[7] = p.max_y;
  for (int c = 0; c < MIJPEG_MAX_COMPONENTS; c++) {
    int32_t *o = out + 8 + 6 * c;
    o[0] = d->model.cursor(c); o[1] = p.g0[c]; o[2] = p.g1[c]; o[3] = p.wstart[c]; o[4] = p.wlimit[c];
    int zeros = 0;
    for (int g = p.g0[c]; g <= p.g1[c] && g < (int)p.rowmap[c].size(); g++) zeros += p.rowmap[c][(size_t)g] < 0;
    o[5] = zeros;
  }
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_display_plan"); }

int mijpeg_display_cursor(mijpeg_decoder *d, int component)
try {
  if (!d || component < 0 || component >= 2 * MIJPEG_MAX_COMPONENTS || !d->model_valid) return 0;
  return component >= MIJPEG_MAX_COMPONENTS ? d->rmodel.cursor(component - MIJPEG_MAX_COMPONENTS) : d->model.cursor(component);
} catch (...) { return boundary_catch(d, "mijpeg_display_cursor"); }

} // extern "C"
