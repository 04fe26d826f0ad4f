// ragged_reconstruct.cpp -- what reconstructs the list that ragged_decode.cpp decoded (include/mijpeg.h): the full
// pictures, interleaved or as planes, their crop windows, and the crops resized into one batch tensor.  Every call has the same
// stages: refuse before anything is launched, written or counted; route every wanted picture (a list launch, a launch of its own, the
// child object that decoded it); launch; the pictures outside the list launches; the children; finish.  Private to libmijpeg.so.
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "fused_list.hpp"
#include "reconstruct.hpp"
#include "resample.hpp"

using namespace mij;

typedef mijpeg_decoder::RaggedImage RaggedImage;
constexpr uint32_t INTERLEAVED_FLAGS = ~(uint32_t)(MIJPEG_FLAG_DEVICE_OUTPUT | MIJPEG_FLAG_NO_UPSAMPLING | MIJPEG_FLAG_SPECULATIVE); // what the interleaved calls take

// What every call starts with: MIJPEG_ERR_INVALID_PARAMETER for a NULL argument (args: all others are there) without touching the
// object, then the object without a device, then the one without a decoded list
static int ragged_call_refused(mijpeg_decoder *d, bool args)
{
  if (!d || !args) return MIJPEG_ERR_INVALID_PARAMETER;
  if (d->device < 0) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "decoder was created without a device");
  if (d->ragged_n < 1) return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "no decoded ragged batch: call mijpeg_decode_ragged_device first");
  return MIJPEG_OK;
}

// The images of the single-image route, on their own objects (which wait for their kernels themselves): step(i, r) reconstructs
// wanted image i on r.child and returns the child's code, which is noted with the child's message
template <class Wanted, class Step> static void reconstruct_children(mijpeg_decoder *d, RaggedFailures &failures, Wanted wanted, Step step)
{
  for (int i = 0; i < d->ragged_n; i++) {
    RaggedImage &r = d->ragged[(size_t)i];
    if (!r.child || !wanted(i)) continue;
    const int rc = step(i, r);
    if (!rc) continue;
    const char *msg = nullptr;
    (void)mijpeg_last_error(r.child, &msg);
    failures.note(i, rc, msg ? msg : "");
  }
}

static int finish_call(mijpeg_decoder *d, const RaggedFailures &failures, int sync)
{
  if (sync) HIP_TRY(d, hipStreamSynchronize(d->stream));
  return failures.finish(d);
}

extern "C" { // (to the end of the file: the calls of include/mijpeg.h, their bodies between them)

int mijpeg_reconstruct_ragged_device(mijpeg_decoder *d, void *const *dst_device, const int64_t *row_strides, uint32_t flags, int sync)
try {
  if (const int rc = ragged_call_refused(d, dst_device && row_strides)) return rc;
  HIP_TRY(d, hipSetDevice(d->device));
  flags &= INTERLEAVED_FLAGS;
  d->ragged_stats.recon_launches = d->ragged_stats.recon_single = 0;
  auto wanted = [&](int i) { return !d->ragged[(size_t)i].status && dst_device[i] != nullptr; };
  // Which kernel every group image takes, from ITS range check: images of a group that agree on kernel and arithmetic flavour
  // share a launch -- one outlier beyond the fast gates runs the SAFE flavour alone instead of taking the group along.  12-bit
  // groups: kernel and narrow12, i.e. at most two launches per three-component group; an image beyond the 12-bit gates or without the
  // YCbCr transformation gets no fused kernel from the planner and is reconstructed by a launch of its own.
  std::vector<FusedListItem> items;
  std::vector<FusedListLaunch> launches;
  std::vector<int> singles;
  for (int i = 0; i < d->ragged_n; i++) {
    const RaggedImage &r = d->ragged[(size_t)i];
    if (!wanted(i) || r.group < 0) continue;
    const ReconPlan p = plan_list_member(r.info, d->coef_dev + r.coef_base, dst_device[i], row_strides[i], flags);
    if (!ragged_twin(p)) { singles.push_back(i); continue; } // (a ragged kernel is its layout group's: tests/test_ragged_twin_cpu.py)
    fused_list_add(launches, p, (int)items.size(), r.info);
    items.push_back(FusedListItem{&r.info, r.coef_base, {dst_device[i], nullptr, nullptr}, row_strides[i]});
  }
  // descriptor tables of all launches in one upload, then the launches
  const int made = launch_fused_lists(d, items.data(), launches, false);
  if (made < 0) return made;
  d->ragged_stats.recon_launches = made;
  RaggedFailures failures;
  // group images no ragged flavour fits (ranges beyond the fused kernels' gates, no colour transformation, ...): the existing kernels
  for (int i : singles) {
    const RaggedImage &r = d->ragged[(size_t)i];
    mijpeg_batch b = batch_of(r.info, d->coef_dev + r.coef_base, dst_device[i], row_strides[i], 0, 1, flags);
    const int rc = reconstruct_on(d, b, nullptr, nullptr); // (no noun: this call reports the first failure)
    if (!rc) d->ragged_stats.recon_single++;
    failures.note(i, rc);
  }
  reconstruct_children(d, failures, wanted, [&](int i, RaggedImage &r) { return mijpeg_reconstruct_device(r.child, dst_device[i], row_strides[i], flags, 1); });
  return finish_call(d, failures, sync);
} catch (...) { return boundary_catch(d, "mijpeg_reconstruct_ragged_device"); }

// The planar twin: the group images are the items of one reconstruct_planar_items call on this object (one fused planar launch per
// kernel and flavour across ALL layout groups' 8-bit colour members; the rest in two passes), the images of the single-image
// route are lists of one on their own objects.
int mijpeg_reconstruct_ragged_planar_device(mijpeg_decoder *d, void *const *planes, const int64_t *row_strides, uint32_t flags, int sync)
try {
  if (const int rc = ragged_call_refused(d, planes && row_strides)) return rc;
  const int n = d->ragged_n;
  flags &= PLANAR_FLAGS;
  auto dest = [&](int i) { return planes + (size_t)i * MIJPEG_MAX_COMPONENTS; };
  auto wanted = [&](int i) { return !d->ragged[(size_t)i].status && dest(i)[0] != nullptr; };
  for (int i = 0; i < n; i++) // every destination, before anything is launched
    if (wanted(i) && planar_check(d->ragged[(size_t)i].info, dest(i), row_strides[i]))
      return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "planar destination of image " + std::to_string(i) + ": a plane pointer is NULL or the row stride is smaller than a line of samples");
  HIP_TRY(d, hipSetDevice(d->device));
  d->planar_stats = mijpeg_planar_stats{};
  std::vector<PlanarItem> items;
  std::vector<int> item_image;
  for (int i = 0; i < n; i++) {
    const RaggedImage &r = d->ragged[(size_t)i];
    if (!wanted(i) || r.group < 0) continue;
    PlanarItem it;
    it.info = &r.info;
    it.coef_dev = d->coef_dev + r.coef_base;
    for (int c = 0; c < MIJPEG_MAX_COMPONENTS; c++) it.planes[c] = c < r.info.components ? dest(i)[c] : nullptr;
    it.row_stride = row_strides[i];
    items.push_back(it);
    item_image.push_back(i);
  }
  RaggedFailures failures;
  if (!items.empty()) {
    const int rc = reconstruct_planar_items(d, items.data(), (int)items.size(), flags, failures, item_image.data());
    if (rc && !failures.code) return rc; // (a group launch or the tables' memory: the device's failure ends the call)
    d->planar_stats.images = d->planar_stats.fused + d->planar_stats.two_pass;
  }
  reconstruct_children(d, failures, wanted, [&](int i, RaggedImage &r) {
    const int rc = mijpeg_reconstruct_planar_device(r.child, dest(i), row_strides[i], flags, 1);
    if (rc) return rc;
    const mijpeg_planar_stats &s = r.child->planar_stats;
    d->planar_stats.images += s.images; d->planar_stats.fused += s.fused; d->planar_stats.two_pass += s.two_pass;
    d->planar_stats.fused_launches += s.fused_launches; d->planar_stats.two_pass_launches += s.two_pass_launches;
    return MIJPEG_OK;
  });
  return finish_call(d, failures, sync);
} catch (...) { return boundary_catch(d, "mijpeg_reconstruct_ragged_planar_device"); }

// ------------------------------------------------------------------------------------------------
// crop windows
// ------------------------------------------------------------------------------------------------
// The two crop calls' body.  planar: ptrs holds MIJPEG_MAX_COMPONENTS entries per picture, else one.
static int reconstruct_ragged_rect(mijpeg_decoder *d, const mijpeg_rect *rects, void *const *ptrs, const int64_t *row_strides, uint32_t flags, int sync, bool planar)
{
  if (const int rc = ragged_call_refused(d, rects && ptrs && row_strides)) return rc;
  const int n = d->ragged_n;
  flags &= planar ? PLANAR_FLAGS : INTERLEAVED_FLAGS;
  auto dest = [&](int i) { return ptrs + (size_t)i * (planar ? MIJPEG_MAX_COMPONENTS : 1); };
  auto wanted = [&](int i) { return !d->ragged[(size_t)i].status && dest(i)[0] != nullptr; };
  // validate and clip: every rectangle and every destination, before anything is launched, written or counted
  std::vector<mijpeg_rect> win((size_t)n);
  bool children = false;
  for (int i = 0; i < n; i++) {
    if (!wanted(i)) continue;
    const RaggedImage &r = d->ragged[(size_t)i];
    const mijpeg_info &f = r.info;
    mijpeg_rect &w = win[(size_t)i];
    if (!fused_window_clip(rects[i], f.width, f.height, w))
      return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "crop of image " + std::to_string(i) + ": min_x / min_y lie outside the picture, or min > max");
    const int64_t crop_line = (int64_t)(w.max_x - w.min_x + 1) * sample_bytes_of(f) * (planar ? 1 : f.components);
    bool ok = f.components >= 1 && f.components <= MIJPEG_MAX_COMPONENTS && row_strides[i] >= crop_line;
    for (int c = 0; planar && ok && c < f.components; c++) ok = dest(i)[c] != nullptr;
    if (!ok)
      return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "crop destination of image " + std::to_string(i) + ": the row stride is smaller than a line of the crop, or a plane pointer is NULL");
    children |= r.group < 0 && r.child;
  }
  HIP_TRY(d, hipSetDevice(d->device));
  d->rect_stats = mijpeg_ragged_rect_stats{};
  // route: group pictures whose plan has a window flavour (plan_list_member with the crop's stride: fits32 is the kernels' 32-bit
  // offsets from canvas pixel (0, 0)) share one window launch per kernel and arithmetic flavour, as the full calls' launches do
  std::vector<FusedListItem> items;
  std::vector<FusedListLaunch> launches;
  std::vector<int> copies; // group pictures of the copy route
  size_t staging = 0;
  for (int i = 0; i < n; i++) {
    const RaggedImage &r = d->ragged[(size_t)i];
    if (!wanted(i) || r.group < 0) continue;
    void *const *p = dest(i);
    const bool planes = planar && r.info.components == 3;
    const ReconPlan plan = plan_list_member(r.info, d->coef_dev + r.coef_base, p[0], row_strides[i], flags);
    if (!window_twin(plan, planes)) {
      copies.push_back(i);
      staging = std::max(staging, picture_bytes(r.info));
      continue;
    }
    fused_list_add(launches, plan, (int)items.size(), r.info, &win[(size_t)i]);
    items.push_back(FusedListItem{&r.info, r.coef_base, {p[0], planes ? p[1] : nullptr, planes ? p[2] : nullptr}, row_strides[i], nullptr, &win[(size_t)i]});
    d->rect_stats.workgroups_full += (int64_t)fused_list_tiles(r.info);
  }
  // launch.  (A child reconstructs into its own buffer on its own stream, and this object's stream copies from there: the copies an
  // earlier call without sync left on this stream are done before a child's buffer is written again)
  if (children) HIP_TRY(d, hipStreamSynchronize(d->stream));
  const int made = launch_fused_lists(d, items.data(), launches, planar, true);
  if (made < 0) return made;
  d->rect_stats.launches = made;
  d->rect_stats.fused = (int32_t)items.size();
  for (const FusedListLaunch &l : launches) d->rect_stats.workgroups += (int64_t)l.grid;
  // copy route: the staged second pass through a buffer of the object
  if (const int rc = ensure_dev(d, (void **)&d->rect_tmp_dev, &d->rect_tmp_cap, staging)) return rc; // (no copies: nothing to grow)
  RaggedFailures failures;
  for (int i : copies) {
    const RaggedImage &r = d->ragged[(size_t)i];
    mijpeg_batch b = batch_of(r.info, d->coef_dev + r.coef_base, nullptr, 0, 0, 1, flags);
    const int rc = reconstruct_staged(d, b, d->rect_tmp_dev, win[(size_t)i], dest(i), row_strides[i], planar);
    if (!rc) d->rect_stats.copied++;
    failures.note(i, rc);
  }
  // children: the full picture into the child's buffer, its second pass on this object's stream
  reconstruct_children(d, failures, wanted, [&](int i, RaggedImage &r) {
    mijpeg_decoder *c = r.child;
    const int64_t line = (int64_t)r.info.width * r.info.components * sample_bytes_of(r.info);
    int rc = ensure_dev(c, (void **)&c->rect_tmp_dev, &c->rect_tmp_cap, (size_t)(line * r.info.height));
    if (!rc) rc = mijpeg_reconstruct_device(c, c->rect_tmp_dev, line, flags, 1); // (waits: the copy below is on another stream)
    if (rc) return rc;
    rc = staged_rect_out(d, c->rect_tmp_dev, r.info, win[(size_t)i], dest(i), row_strides[i], planar);
    if (!rc) d->rect_stats.copied++;
    failures.note(i, rc); // (this object's copy: no message of the child's)
    return MIJPEG_OK;
  });
  d->rect_stats.images = d->rect_stats.fused + d->rect_stats.copied;
  return finish_call(d, failures, sync);
}

int mijpeg_reconstruct_ragged_rect_device(mijpeg_decoder *d, const mijpeg_rect *rects, void *const *dst_device, const int64_t *row_strides, uint32_t flags, int sync)
try {
  return reconstruct_ragged_rect(d, rects, dst_device, row_strides, flags, sync, false);
} catch (...) { return boundary_catch(d, "mijpeg_reconstruct_ragged_rect_device"); }

int mijpeg_reconstruct_ragged_rect_planar_device(mijpeg_decoder *d, const mijpeg_rect *rects, void *const *planes, const int64_t *row_strides, uint32_t flags, int sync)
try {
  return reconstruct_ragged_rect(d, rects, planes, row_strides, flags, sync, true);
} catch (...) { return boundary_catch(d, "mijpeg_reconstruct_ragged_rect_planar_device"); }

int mijpeg_ragged_rect_stats_get(mijpeg_decoder *d, mijpeg_ragged_rect_stats *out)
try {
  if (!d || !out) return MIJPEG_ERR_INVALID_PARAMETER;
  *out = d->rect_stats;
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_ragged_rect_stats_get"); }

int mijpeg_ragged_rect_plan(const mijpeg_info *infos, const mijpeg_rect *rects, int n, int32_t *tile_x0, int32_t *tile_y0, int32_t *tiles_x, int32_t *tiles_y)
try {
  if (!infos || !rects || !tile_x0 || !tile_y0 || !tiles_x || !tiles_y || n < 1) return MIJPEG_ERR_INVALID_PARAMETER;
  for (int i = 0; i < n; i++) {
    mijpeg_rect w;
    if (!fused_window_clip(rects[i], infos[i].width, infos[i].height, w)) return MIJPEG_ERR_INVALID_PARAMETER;
    const WindowFrame t = fused_window_tiles(w);
    tile_x0[i] = t.tile_x0; tile_y0[i] = t.tile_y0; tiles_x[i] = t.wtiles_x; tiles_y[i] = t.wtiles_y;
  }
  return MIJPEG_OK;
} catch (...) { return boundary_catch(nullptr, "mijpeg_ragged_rect_plan"); }

// ------------------------------------------------------------------------------------------------
// crops resized into one batch tensor, and the same as a normalised float batch, mirrored per picture:
// one driver, the resized call is its {uint8 samples, nobody mirrored}
// ------------------------------------------------------------------------------------------------
static_assert(MIJPEG_SAMPLE_U8 == RESAMPLE_U8 && MIJPEG_SAMPLE_F32 == RESAMPLE_F32 && MIJPEG_SAMPLE_F16 == RESAMPLE_F16 && MIJPEG_SAMPLE_BF16 == RESAMPLE_BF16,
              "the header's sample types are the kernels'");

// Why the resized call does not serve a decoded picture, or 0
static int resized_refusal(const mijpeg_info &f, int32_t channels)
{
  const bool served = sample_bytes_of(f) == 1 && (f.components == 1 || (f.components == 3 && channels != 1));
  return served ? 0 : MIJPEG_ERR_NOT_IMPLEMENTED;
}

// What the call's parameters have against them (MIJPEG_ERR_INVALID_PARAMETER with this text), or nullptr.  Needs no device and no list.
static const char *resized_parameters_refused(int32_t out_w, int32_t out_h, int32_t channels, const mijpeg_batch_format &format, const void *dst, int64_t image_stride,
                                              int64_t plane_stride, int64_t row_stride)
{
  static const char *const spans = "resized call: a stride is smaller than the data it spans, or a slot spans 4 GiB or more";
  if (out_w < 1 || out_h < 1 || out_w > RESAMPLE_MAX_AXIS || out_h > RESAMPLE_MAX_AXIS) return "resized call: out_width and out_height are 1 .. 65535";
  if (channels != 1 && channels != 3) return "resized call: channels is 1 or 3";
  if (format.sample < MIJPEG_SAMPLE_U8 || format.sample > MIJPEG_SAMPLE_BF16 || format.reserved != 0) return "normalised call: sample is a MIJPEG_SAMPLE_*, reserved is 0";
  if (format.sample != MIJPEG_SAMPLE_U8)
    for (int c = 0; c < channels; c++)
      if (!std::isfinite(format.scale[c]) || !std::isfinite(format.bias[c])) return "normalised call: scale and bias are finite";
  const int64_t es = (int64_t)resample_sample_bytes(format.sample); // (every stride is in bytes)
  if ((uintptr_t)dst % (uintptr_t)es || image_stride % es || plane_stride % es || row_stride % es) return "normalised call: dst_device and the strides are multiples of the element size";
  const bool planar = plane_stride != 0;
  if (row_stride < 1 || row_stride > 0xffffffffll || plane_stride < 0 || plane_stride > 0xffffffffll) return spans; // (what follows then stays inside 64 bits)
  const int64_t line = (int64_t)out_w * (planar ? 1 : channels) * es, plane = (int64_t)(out_h - 1) * row_stride + line;
  const int64_t slot = planar ? (int64_t)(channels - 1) * plane_stride + plane : plane;
  if (row_stride < line || (planar && plane_stride < plane) || image_stride < slot || slot > 0xffffffffll) return spans;
  return nullptr;
}

// Stage 2: the tables of the served pictures in one pinned upload, and the one launch
static int launch_resample(mijpeg_decoder *d, const ResampleItem *items, const ResampleLayout &L, int32_t out_w, int32_t out_h, int32_t channels,
                           const mijpeg_batch_format &format, void *dst, int64_t image_stride, int64_t plane_stride, int64_t row_stride)
{
  PinnedUpload &u = d->resample_tables;
  if (const int rc = pinned_upload_reserve(d, u, L.table_bytes)) return rc;
  const int served = (int)L.per.size(), workers = std::min(served, default_threads());
  std::vector<char> bad((size_t)workers, 0);
  parallel_for(workers, [&](int w) { // (a division per tap: a list of 256 pictures has half a million)
    for (int k = w; k < served; k += workers)
      if (!resample_fill(u.host, L, (size_t)k, items, out_w, out_h, image_stride)) bad[(size_t)w] = 1;
  });
  resample_fill_first(u.host, L);
  for (char b : bad)
    if (b) return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "the resample filter has no taps for these sizes");
  if (const int rc = pinned_upload_send(d, u, L.table_bytes)) return rc;
  ResampleArgs a;
  memset(&a, 0, sizeof(a));
  a.src = d->resized_arena_dev; a.dst = (uint8_t *)dst;
  a.tables = u.dev;
  a.pictures = (const ResamplePicture *)(u.dev + L.pictures);
  a.first = (const uint32_t *)(u.dev + L.first);
  a.served = served;
  a.out_w = out_w; a.out_h = out_h; a.channels = channels;
  a.plane_stride = (uint32_t)plane_stride; a.row_stride = (uint32_t)row_stride;
  if (format.sample != MIJPEG_SAMPLE_U8)
    for (int c = 0; c < channels; c++) { a.scale[c] = format.scale[c]; a.bias[c] = format.bias[c]; }
  if (launch_resample_list(a, format.sample, (unsigned)L.workgroups, d->stream))
    return set_error(d, MIJPEG_ERR_DEVICE, std::string("kernel launch failed: ") + hipGetErrorString(hipGetLastError()));
  return MIJPEG_OK;
}

static int reconstruct_ragged_resized(mijpeg_decoder *d, const mijpeg_rect *rects, int32_t out_w, int32_t out_h, int32_t channels, const mijpeg_batch_format *format,
                                      void *dst, int64_t image_stride, int64_t plane_stride, int64_t row_stride, uint32_t flags, int32_t *status, int sync)
{
  if (d && dst && !format) return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "normalised call: format is NULL");
  if (const int rc = ragged_call_refused(d, dst != nullptr)) return rc;
  const int n = d->ragged_n;
  // every parameter, before anything is launched, written or counted
  if (const char *why = resized_parameters_refused(out_w, out_h, channels, *format, dst, image_stride, plane_stride, row_stride))
    return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, why);
  const mijpeg_rect whole{0, 0, INT32_MAX, INT32_MAX};
  std::vector<mijpeg_rect> asked((size_t)n, whole), win((size_t)n);
  // the crop of every decoded picture; who is served, and where everything lies
  std::vector<ResampleItem> items((size_t)n);
  std::vector<int32_t> st((size_t)n, 0);
  for (int i = 0; i < n; i++) {
    const RaggedImage &r = d->ragged[(size_t)i];
    ResampleItem &it = items[(size_t)i];
    it.slot = i;
    if ((st[(size_t)i] = r.status)) continue;
    if (rects) asked[(size_t)i] = rects[i];
    if (!fused_window_clip(asked[(size_t)i], r.info.width, r.info.height, win[(size_t)i]))
      return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "crop of image " + std::to_string(i) + ": min_x / min_y lie outside the picture, or min > max");
    if ((st[(size_t)i] = resized_refusal(r.info, channels))) continue;
    it.src_w = win[(size_t)i].max_x - win[(size_t)i].min_x + 1;
    it.src_h = win[(size_t)i].max_y - win[(size_t)i].min_y + 1;
    it.comps = r.info.components;
    it.mirror = format->mirror && format->mirror[i];
    if ((uint64_t)it.src_w * (uint64_t)it.src_h * (uint64_t)it.comps > 0xffffffffull) { st[(size_t)i] = MIJPEG_ERR_NOT_IMPLEMENTED; continue; } // (the kernel's 32-bit offsets)
    it.served = true;
  }
  const int workers = std::min(n, default_threads());
  parallel_for(workers, [&](int w) { // (a pass over every output sample of both axes: one picture per worker)
    for (int i = w; i < n; i += workers)
      if (items[(size_t)i].served) resample_item_caps(items[(size_t)i], out_w, out_h);
  });
  const ResampleLayout L = resample_layout(items.data(), n, out_w, out_h);
  if (L.table_bytes > 0xffffffffull || L.workgroups > 0x7fffffffull)
    return set_error(d, MIJPEG_ERR_OVERFLOW_PARAMETER, "resized call: the list's tap tables pass 4 GiB or its tiles a grid of 2^31 - 1 workgroups");
  HIP_TRY(d, hipSetDevice(d->device));
  mijpeg_ragged_resized_stats stats{};
  stats.images = n;
  stats.resampled = (int32_t)L.per.size();
  stats.refused = n - stats.resampled;
  stats.arena_bytes = (int64_t)L.arena_bytes;
  mijpeg_ragged_normalized_stats nstats{};
  nstats.sample = format->sample;
  for (const ResampleLayout::Per &p : L.per) nstats.mirrored += items[(size_t)p.item].mirror ? 1 : 0;
  if (!L.per.empty()) {
    // stage 1: the crop call's body, destinations in the arena (its statistics stay the last crop call's)
    if (const int rc = ensure_dev(d, (void **)&d->resized_arena_dev, &d->resized_arena_cap, L.arena_bytes + RESAMPLE_ARENA_SPARE)) return rc;
    std::vector<void *> ptrs((size_t)n, nullptr);
    std::vector<int64_t> rows((size_t)n, 0);
    for (const ResampleLayout::Per &p : L.per) {
      ptrs[(size_t)p.item] = d->resized_arena_dev + p.src_off;
      rows[(size_t)p.item] = (int64_t)items[(size_t)p.item].src_w * items[(size_t)p.item].comps;
    }
    const mijpeg_ragged_rect_stats kept = d->rect_stats;
    const int rc1 = reconstruct_ragged_rect(d, asked.data(), ptrs.data(), rows.data(), flags, 0, false);
    stats.window_launches = d->rect_stats.launches;
    d->rect_stats = kept;
    if (rc1) return rc1;
    // stage 2: one launch for the list
    if (const int rc2 = launch_resample(d, items.data(), L, out_w, out_h, channels, *format, dst, image_stride, plane_stride, row_stride)) return rc2;
    stats.resample_launches = 1;
  }
  d->resized_stats = stats;
  d->normalized_stats = nstats;
  if (status)
    for (int i = 0; i < n; i++) status[i] = st[(size_t)i];
  if (sync) HIP_TRY(d, hipStreamSynchronize(d->stream));
  return MIJPEG_OK;
}

int mijpeg_reconstruct_ragged_resized_device(mijpeg_decoder *d, const mijpeg_rect *rects, int32_t out_width, int32_t out_height, int32_t channels, void *dst_device,
                                             int64_t image_stride, int64_t plane_stride, int64_t row_stride, uint32_t flags, int32_t *status, int sync)
try {
  static const mijpeg_batch_format plain = {MIJPEG_SAMPLE_U8, 0, {0, 0, 0}, {0, 0, 0}, nullptr};
  return reconstruct_ragged_resized(d, rects, out_width, out_height, channels, &plain, dst_device, image_stride, plane_stride, row_stride, flags, status, sync);
} catch (...) { return boundary_catch(d, "mijpeg_reconstruct_ragged_resized_device"); }

int mijpeg_reconstruct_ragged_normalized_device(mijpeg_decoder *d, const mijpeg_rect *rects, int32_t out_width, int32_t out_height, int32_t channels,
                                                const mijpeg_batch_format *format, void *dst_device, int64_t image_stride, int64_t plane_stride, int64_t row_stride,
                                                uint32_t flags, int32_t *status, int sync)
try {
  return reconstruct_ragged_resized(d, rects, out_width, out_height, channels, format, dst_device, image_stride, plane_stride, row_stride, flags, status, sync);
} catch (...) { return boundary_catch(d, "mijpeg_reconstruct_ragged_normalized_device"); }

int mijpeg_ragged_normalized_stats_get(mijpeg_decoder *d, mijpeg_ragged_normalized_stats *out)
try {
  if (!d || !out) return MIJPEG_ERR_INVALID_PARAMETER;
  *out = d->normalized_stats;
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_ragged_normalized_stats_get"); }

int mijpeg_ragged_resized_stats_get(mijpeg_decoder *d, mijpeg_ragged_resized_stats *out)
try {
  if (!d || !out) return MIJPEG_ERR_INVALID_PARAMETER;
  *out = d->resized_stats;
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_ragged_resized_stats_get"); }

int32_t mijpeg_resample_taps(int32_t n, int32_t m, int32_t *first, int32_t *count, int16_t *weights, int32_t capacity_per_output)
try {
  return resample_taps(n, m, first, count, weights, capacity_per_output);
} catch (...) { (void)boundary_catch(nullptr, "mijpeg_resample_taps"); return 0; }

} // extern "C"
