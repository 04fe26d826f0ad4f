// ragged_decode.cpp -- ragged batches: streams of any shapes in one device pass (include/mijpeg.h): the planner, the
// decode (a Huffman launch per layout group, the single-image route for the rest) and the reconstruction.  Private to libmijpeg.so.
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "fused_list.hpp"
#include "reconstruct.hpp"
#include "resample.hpp"

using namespace mij;

// The layout group of a frame description, or -1: 8-bit plain sequential frames in the four layouts whose fused kernels have a
// ragged flavour, every plane inside the kernels' 32-bit offsets.  with12 (the ...16 calls): 12-bit ones as well, in the groups
// MIJPEG_RAGGED_420_12 ... of the same layouts (MIJPEG_RAGGED_GROUPS further on)
static int ragged_group_of(const mijpeg_info &f, bool with12)
{
  if ((f.precision != 8 && !(with12 && f.precision == 12)) || f.xt || f.progressive || f.coef_wide || f.dnl || f.width < 1 || f.height < 1 || f.coef_count < 64) return -1;
  if (f.components != 1 && f.components != 3) return -1;
  for (int c = 0; c < f.components; c++)
    if ((unsigned)f.quant_index[c] >= 4 || f.blocks_w[c] < 1 || f.blocks_h[c] < 1 || (uint64_t)f.blocks_w[c] * (uint64_t)f.blocks_h[c] * 128u > 0xffffffffull) return -1;
  const int p12 = f.precision == 12 ? MIJPEG_RAGGED_GROUPS : 0;
  switch (sampling_of(f)) {
  case Sampling::S420: return MIJPEG_RAGGED_420 + p12;
  case Sampling::S422: return MIJPEG_RAGGED_422 + p12;
  case Sampling::S444: return MIJPEG_RAGGED_444 + p12;
  case Sampling::GREY: return f.hsamp[0] == 1 && f.vsamp[0] == 1 ? MIJPEG_RAGGED_GREY + p12 : -1; // (sampling factors on a single component: MCU padding nobody decodes)
  default: return -1;
  }
}
static_assert(MIJPEG_RAGGED_420_12 == MIJPEG_RAGGED_420 + MIJPEG_RAGGED_GROUPS && MIJPEG_RAGGED_GREY_12 == MIJPEG_RAGGED_GREY + MIJPEG_RAGGED_GROUPS &&
              MIJPEG_RAGGED_GROUPS16 == 2 * MIJPEG_RAGGED_GROUPS, "the 12-bit groups follow the 8-bit ones, layout by layout");

// Grouping, workgroup ranges and coefficient bases of n frames; excluded[i] != 0 (optional) keeps frame i out of the groups.
// with12: the planner of the ...16 calls -- group_workgroups holds MIJPEG_RAGGED_GROUPS16 grids, MIJPEG_RAGGED_GROUPS without it.
static int ragged_plan(const mijpeg_info *infos, int n, const char *excluded, bool with12, int32_t *group, mijpeg_ragged_frame *frames, int32_t *group_workgroups, int64_t *coef_total)
{
  int64_t base = 0;
  uint64_t grid[MIJPEG_RAGGED_GROUPS16] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < n; i++) {
    const mijpeg_info &f = infos[i];
    mijpeg_ragged_frame &r = frames[i];
    memset(&r, 0, sizeof(r));
    int g = excluded && excluded[i] ? -1 : ragged_group_of(f, with12);
    if (g >= 0) fused_geometry(f, sampling_of(f), r); // (what the uniform launches of the same kernels get)
    const uint64_t tiles = (uint64_t)r.tiles_x * (uint64_t)r.tiles_y;
    if (g >= 0 && grid[g] + tiles > 0x7fffffffull) { // (a grid holds 2^31 - 1 workgroups)
      g = -1;
      memset(&r, 0, sizeof(r));
    }
    group[i] = g;
    if (g < 0) continue;
    r.coef_base = base;
    base += f.coef_count;
    r.first_workgroup = (int32_t)grid[g];
    grid[g] += tiles;
  }
  for (int g = 0; g < (with12 ? MIJPEG_RAGGED_GROUPS16 : MIJPEG_RAGGED_GROUPS); g++) group_workgroups[g] = (int32_t)grid[g];
  *coef_total = base;
  return MIJPEG_OK;
}

// Image i through the single-image route, on a decoder object of its own (kept from call to call)
static void ragged_single_image(mijpeg_decoder *d, int i, int k, const uint8_t *data, size_t size, int min_intervals)
{
  mijpeg_decoder::RaggedImage &r = d->ragged[(size_t)i];
  r.group = -1;
  r.child = nullptr;
  if ((size_t)k >= d->ragged_children.size()) {
    mijpeg_decoder *c = nullptr;
    const int rc = mijpeg_create(&c, d->device);
    if (rc) { r.status = rc; return; }
    d->ragged_children.push_back(c);
  }
  mijpeg_decoder *c = d->ragged_children[(size_t)k];
  r.child = c;
  if (data) c->own_input.assign(data, data + size);
  else c->own_input.clear();
  int rc = mijpeg_set_input(c, data ? c->own_input.data() : nullptr, data ? size : 0);
  if (!rc) {
    rc = mijpeg_decode_coefficients_device(c, min_intervals);
    if (rc == MIJPEG_ERR_NOT_AVAILABLE) rc = mijpeg_decode_coefficients(c, 0);
  }
  if (!rc) rc = mijpeg_get_info(c, &r.info);
  r.status = rc;
}

// The two decode calls' body.  with12: mijpeg_decode_ragged_device16 -- plain 12-bit frames pass the entropy obstacle and have layout
// groups of their own (a Huffman launch decodes one precision: plan_batch), everything else is the same call
static int decode_ragged(mijpeg_decoder *d, const uint8_t *const *streams, const size_t *sizes, int n, int min_intervals, int32_t *status, bool with12)
{
  if (!d || !streams || !sizes || !status || n < 1) return MIJPEG_ERR_INVALID_PARAMETER;
  if (d->device < 0) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "decoder was created without a device");
  HIP_TRY(d, hipSetDevice(d->device));
  if (d->spec_active) (void)settle_speculation(d); // (an unvalidated batch of the uniform calls is abandoned here)
  if (const int prc = settle_pending(d)) return prc;
  d->batch_frames = 0;
  d->ragged_n = 0;
  d->img_valid = d->model_valid = d->uploaded = d->decoded = false;
  d->ragged_stats = mijpeg_ragged_stats{};
  if (d->batch_hosts.size() < (size_t)n) d->batch_hosts.resize((size_t)n);
  for (auto &h : d->batch_hosts)
    if (!h) h.reset(new HostDecoder());
  d->ragged.assign((size_t)n, mijpeg_decoder::RaggedImage{});
  // headers and restart markers of all streams, one stream per worker.  mijpeg_set_device_markers: headers only where the parse
  // can leave the search to the device (HostDecoder::set_skip_search; Scan::search_skipped tells) -- such members are searched
  // inside their layout group's launch, beside members that were searched here
  const bool markers = d->device_markers == 1;
  std::vector<int> rcs((size_t)n, 0);
  const int workers = std::min(n, default_threads());
  parallel_for(workers, [&](int w) {
    for (int i = w; i < n; i += workers) {
      if (!streams[i] || !sizes[i]) { rcs[(size_t)i] = MIJPEG_ERR_STREAM_EMPTY; continue; }
      if (markers) d->batch_hosts[(size_t)i]->set_skip_search(); // (armed for the parse that follows)
      rcs[(size_t)i] = d->batch_hosts[(size_t)i]->parse(streams[i], sizes[i], false);
    }
  });
  auto skipped = [&](int i) { return !rcs[(size_t)i] && !d->batch_hosts[(size_t)i]->scans.empty() && d->batch_hosts[(size_t)i]->scans[0].search_skipped; };
  int64_t searched = 0;
  // what the batch kernels cover goes into the layout groups
  std::vector<char> excluded((size_t)n, 0);
  std::vector<mijpeg_info> infos((size_t)n);
  for (int i = 0; i < n; i++) {
    const char *why = rcs[(size_t)i] ? "the stream does not parse as the batch decoder reads it" : ragged_entropy_obstacle(*d->batch_hosts[(size_t)i], sizes[i], with12);
    excluded[(size_t)i] = why != nullptr;
    if (why) d->ragged[(size_t)i].why_single = why;
    if (excluded[(size_t)i]) memset(&infos[(size_t)i], 0, sizeof(mijpeg_info));
    else infos[(size_t)i] = d->batch_hosts[(size_t)i]->info;
  }
  std::vector<int32_t> group((size_t)n);
  std::vector<mijpeg_ragged_frame> frames((size_t)n);
  int32_t grids[MIJPEG_RAGGED_GROUPS16];
  int64_t coef_total = 0;
  ragged_plan(infos.data(), n, excluded.data(), with12, group.data(), frames.data(), grids, &coef_total);
  for (int i = 0; i < n; i++)
    if (group[(size_t)i] < 0 && !excluded[(size_t)i])
      d->ragged[(size_t)i].why_single = with12 ? "no layout group for this frame: 8-bit and 12-bit sequential 4:2:0, 4:2:2, 4:4:4 and grey frames have one"
                                               : "no layout group for this frame: 8-bit sequential 4:2:0, 4:2:2, 4:4:4 and grey frames have one";
  if (coef_total > 0) {
    const int rc = ensure_coef_store(d, (size_t)coef_total, false);
    if (rc) return rc;
  }
  // one launch of the Huffman kernel per group (the walk in front of it where streams have no restart markers)
  for (int g = 0; g < (with12 ? MIJPEG_RAGGED_GROUPS16 : MIJPEG_RAGGED_GROUPS); g++) {
    std::vector<int> members;
    for (int i = 0; i < n; i++)
      if (group[(size_t)i] == g) members.push_back(i);
    if (members.empty()) continue;
    const size_t m = members.size();
    std::vector<HostDecoder *> hosts(m);
    std::vector<const uint8_t *> datas(m);
    std::vector<size_t> gsizes(m);
    std::vector<int64_t> bases(m);
    std::vector<int> verdict(m, 1);
    for (size_t k = 0; k < m; k++) {
      const int i = members[k];
      hosts[k] = d->batch_hosts[(size_t)i].get();
      datas[k] = streams[i];
      gsizes[k] = sizes[i];
      bases[k] = frames[(size_t)i].coef_base;
    }
    int scan_launches = 0, walk_launches = 0;
    const RaggedEntropy re{bases.data(), verdict.data(), &scan_launches, &walk_launches};
    EntropyBatchOptions opt;
    opt.ragged = &re;
    opt.plain12 = g >= MIJPEG_RAGGED_GROUPS;
    for (size_t k = 0; k < m; k++) opt.markers |= skipped(members[k]);
    const int rc = device_entropy_batch(d, hosts.data(), datas.data(), gsizes.data(), (int)m, 1, d->coef_dev, 0, opt);
    d->ragged_stats.entropy_launches += scan_launches;
    d->ragged_stats.walk_launches += walk_launches;
    if (rc && rc != MIJPEG_ERR_NOT_AVAILABLE) return rc; // (the device, memory: not a verdict on a stream)
    // What is left to refuse a whole group once every member passed ragged_entropy_obstacle: its device walk did not settle
    // or has more subsequences than its prefix sums hold, the launch outgrew 32-bit offsets.  Every member then takes the
    // single-image route, with the launch's message as the reason (mijpeg_ragged_route).
    const std::string group_refusal = rc ? "the layout group's launch was refused: " + d->err_msg : std::string();
    for (size_t k = 0; k < m; k++) {
      const int i = members[k];
      if (rc || verdict[k]) { // damaged: the single-image route decides
        group[(size_t)i] = -1;
        d->ragged[(size_t)i].why_single = rc                 ? group_refusal
                                          : verdict[k] == 2 ? std::string("device marker search: the segment is not the plain case; the host searches it")
                                                            : std::string("the device decoder found the entropy coded data damaged");
        if (!rc && skipped(i)) searched++; // (the device searched it, whatever it found)
        continue;
      }
      if (skipped(i)) searched++;
      mijpeg_decoder::RaggedImage &r = d->ragged[(size_t)i];
      r.group = g;
      r.info = hosts[k]->info;
      r.coef_base = frames[(size_t)i].coef_base;
      d->ragged_stats.ragged++;
    }
  }
  // everything else: the single-image route, stream by stream
  int children = 0;
  for (int i = 0; i < n; i++) {
    if (group[(size_t)i] >= 0) continue;
    ragged_single_image(d, i, children++, streams[i], sizes[i], min_intervals);
    d->ragged_stats.fallbacks++;
    if (d->ragged[(size_t)i].status) d->ragged_stats.errors++;
  }
  for (int i = 0; i < n; i++) status[i] = d->ragged[(size_t)i].status;
  if (markers) { // mijpeg_device_markers_stats: members the device searched, and all the others
    d->markers_searched += searched;
    d->markers_declined += n - searched;
  }
  d->ragged_stats.images = n;
  d->ragged_n = n;
  d->err_code = 0;
  d->err_msg.clear();
  return MIJPEG_OK;
}

extern "C" {

int mijpeg_ragged_plan(const mijpeg_info *infos, int n, int32_t *group, mijpeg_ragged_frame *frames, int32_t group_workgroups[MIJPEG_RAGGED_GROUPS], int64_t *coef_total)
try {
  if (!infos || !group || !frames || !group_workgroups || !coef_total || n < 1) return MIJPEG_ERR_INVALID_PARAMETER;
  return ragged_plan(infos, n, nullptr, false, group, frames, group_workgroups, coef_total);
} catch (...) { return boundary_catch(nullptr, "mijpeg_ragged_plan"); }

int mijpeg_ragged_plan16(const mijpeg_info *infos, int n, int32_t *group, mijpeg_ragged_frame *frames, int32_t group_workgroups[MIJPEG_RAGGED_GROUPS16], int64_t *coef_total)
try {
  if (!infos || !group || !frames || !group_workgroups || !coef_total || n < 1) return MIJPEG_ERR_INVALID_PARAMETER;
  return ragged_plan(infos, n, nullptr, true, group, frames, group_workgroups, coef_total);
} catch (...) { return boundary_catch(nullptr, "mijpeg_ragged_plan16"); }

int mijpeg_decode_ragged_device(mijpeg_decoder *d, const uint8_t *const *streams, const size_t *sizes, int n, int min_intervals, int32_t *status)
try {
  return decode_ragged(d, streams, sizes, n, min_intervals, status, false);
} catch (...) { return boundary_catch(d, "mijpeg_decode_ragged_device"); }

int mijpeg_decode_ragged_device16(mijpeg_decoder *d, const uint8_t *const *streams, const size_t *sizes, int n, int min_intervals, int32_t *status)
try {
  return decode_ragged(d, streams, sizes, n, min_intervals, status, true);
} catch (...) { return boundary_catch(d, "mijpeg_decode_ragged_device16"); }


int mijpeg_ragged_info(mijpeg_decoder *d, int i, mijpeg_info *info)
try {
  if (!d || !info || i < 0) return MIJPEG_ERR_INVALID_PARAMETER;
  if (i >= d->ragged_n) return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "no such image: call mijpeg_decode_ragged_device first");
  const mijpeg_decoder::RaggedImage &r = d->ragged[(size_t)i];
  if (r.status) {
    const char *msg = nullptr;
    if (r.child) (void)mijpeg_last_error(r.child, &msg);
    return set_error(d, r.status, msg ? msg : "the stream could not be decoded");
  }
  *info = r.info;
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_ragged_info"); }

int mijpeg_ragged_warning(mijpeg_decoder *d, int i, const char **message)
try {
  if (message) *message = nullptr;
  if (!d || i < 0 || i >= d->ragged_n) return 0;
  const mijpeg_decoder::RaggedImage &r = d->ragged[(size_t)i];
  return r.child && !r.status ? mijpeg_last_warning(r.child, message) : 0;
} catch (...) { return boundary_catch(d, "mijpeg_ragged_warning"); }

int mijpeg_ragged_route(mijpeg_decoder *d, int i, const char **why)
try {
  if (why) *why = nullptr;
  if (!d || i < 0) return MIJPEG_ERR_INVALID_PARAMETER;
  if (i >= d->ragged_n) return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "no such image: call mijpeg_decode_ragged_device first");
  const mijpeg_decoder::RaggedImage &r = d->ragged[(size_t)i];
  if (r.group >= 0) return 0;
  if (why) *why = r.why_single.c_str();
  return 1;
} catch (...) { return boundary_catch(d, "mijpeg_ragged_route"); }

int mijpeg_ragged_get_stats(mijpeg_decoder *d, mijpeg_ragged_stats *out)
try {
  if (!d || !out) return MIJPEG_ERR_INVALID_PARAMETER;
  *out = d->ragged_stats;
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_ragged_get_stats"); }

int mijpeg_reconstruct_ragged_device(mijpeg_decoder *d, void *const *dst_device, const int64_t *row_strides, uint32_t flags, int sync)
try {
  if (!d || !dst_device || !row_strides) return MIJPEG_ERR_INVALID_PARAMETER;
  if (d->device < 0) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "decoder was created without a device");
  if (d->ragged_n < 1) return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "no decoded ragged batch: call mijpeg_decode_ragged_device first");
  HIP_TRY(d, hipSetDevice(d->device));
  const int n = d->ragged_n;
  flags &= ~(uint32_t)(MIJPEG_FLAG_DEVICE_OUTPUT | MIJPEG_FLAG_NO_UPSAMPLING | MIJPEG_FLAG_SPECULATIVE);
  d->ragged_stats.recon_launches = d->ragged_stats.recon_single = 0;
  // Which kernel every group image takes, from ITS range check: images of a group that agree on kernel and arithmetic flavour
  // share a launch -- one outlier beyond the fast gates runs the SAFE flavour alone instead of taking the group along.
  // (quant_dev is only tested by the planner: the ragged launches read per-frame tables.)  12-bit groups: kernel and narrow12, i.e.
  // at most two launches per three-component group; an image beyond the 12-bit gates or without the YCbCr transformation gets
  // no fused kernel from the planner and is reconstructed by a launch of its own.
  static const uint16_t per_frame_tables = 0;
  auto describe = [&](int i, bool own_tables) {
    const mijpeg_decoder::RaggedImage &r = d->ragged[(size_t)i];
    mijpeg_batch b = batch_of(r.info, d->coef_dev + r.coef_base, dst_device[i], row_strides[i], 0, 1, flags);
    b.quant_dev = own_tables ? &per_frame_tables : nullptr;
    return b;
  };
  std::vector<FusedListItem> items;
  std::vector<FusedListLaunch> launches;
  std::vector<int> singles;
  for (int i = 0; i < n; i++) {
    const mijpeg_decoder::RaggedImage &r = d->ragged[(size_t)i];
    if (r.status || r.group < 0 || !dst_device[i]) continue;
    const mijpeg_batch b = describe(i, true);
    const ReconPlan p = plan_reconstruct(&b);
    if (!ragged_twin(p)) { singles.push_back(i); continue; } // (a ragged kernel is its layout group's: tests/test_ragged_twin_cpu.py)
    fused_list_add(launches, p, (int)items.size(), r.info);
    items.push_back(FusedListItem{&r.info, r.coef_base, {dst_device[i], nullptr, nullptr}, row_strides[i]});
  }
  // descriptor tables of all launches in one upload, then the launches
  const int made = launch_fused_lists(d, items.data(), launches, false);
  if (made < 0) return made;
  d->ragged_stats.recon_launches = made;
  // One image whose reconstruction fails does not stop the others, whichever route it takes: the call works through the list
  // and then returns the first such code, with a message that names the image.  (A launch of a whole group that fails, or
  // memory that cannot be had for the tables, is the device's failure and ends the call at once; what was enqueued stays
  // ordered on the object's stream, and the next call waits for the descriptor upload as usual.)
  int failed = MIJPEG_OK;
  std::string failed_msg;
  // group images no ragged flavour fits (ranges beyond the fused kernels' gates, no colour transformation, ...): the existing kernels
  for (int i : singles) {
    mijpeg_batch b = describe(i, false);
    const int rc = reconstruct_on(d, b, nullptr, nullptr); // (no noun: this call reports the first failure, below)
    if (!rc) d->ragged_stats.recon_single++;
    else if (!failed) {
      failed = rc;
      failed_msg = "image " + std::to_string(i) + " of the ragged batch was not reconstructed";
    }
  }
  // images of the single-image route, on their own objects (which wait for their kernels themselves)
  for (int i = 0; i < n; i++) {
    mijpeg_decoder::RaggedImage &r = d->ragged[(size_t)i];
    if (!r.child || r.status || !dst_device[i]) continue;
    const int rc = mijpeg_reconstruct_device(r.child, dst_device[i], row_strides[i], flags, 1);
    if (rc && !failed) {
      const char *msg = nullptr;
      (void)mijpeg_last_error(r.child, &msg);
      failed = rc;
      failed_msg = "image " + std::to_string(i) + " of the ragged batch was not reconstructed: " + (msg ? msg : "");
    }
  }
  if (sync) HIP_TRY(d, hipStreamSynchronize(d->stream));
  if (failed) return set_error(d, failed, failed_msg);
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_reconstruct_ragged_device"); }

// The planar twin: the group images are the items of one reconstruct_planar_items call on this object (one fused planar launch per
// kernel and flavour across ALL layout groups' 8-bit colour members; the rest in two passes), the images of the single-image
// route are lists of one on their own objects.
int mijpeg_reconstruct_ragged_planar_device(mijpeg_decoder *d, void *const *planes, const int64_t *row_strides, uint32_t flags, int sync)
try {
  if (!d || !planes || !row_strides) return MIJPEG_ERR_INVALID_PARAMETER;
  if (d->device < 0) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "decoder was created without a device");
  if (d->ragged_n < 1) return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "no decoded ragged batch: call mijpeg_decode_ragged_device first");
  const int n = d->ragged_n;
  flags &= PLANAR_FLAGS;
  auto wanted = [&](int i) { return !d->ragged[(size_t)i].status && planes[(size_t)i * MIJPEG_MAX_COMPONENTS] != nullptr; };
  for (int i = 0; i < n; i++) // every destination, before anything is launched
    if (wanted(i) && planar_check(d->ragged[(size_t)i].info, planes + (size_t)i * MIJPEG_MAX_COMPONENTS, row_strides[i]))
      return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "planar destination of image " + std::to_string(i) + ": a plane pointer is NULL or the row stride is smaller than a line of samples");
  HIP_TRY(d, hipSetDevice(d->device));
  d->planar_stats = mijpeg_planar_stats{};
  std::vector<PlanarItem> items;
  std::vector<int> item_image;
  for (int i = 0; i < n; i++) {
    const mijpeg_decoder::RaggedImage &r = d->ragged[(size_t)i];
    if (!wanted(i) || r.group < 0) continue;
    PlanarItem it;
    it.info = &r.info;
    it.coef_dev = d->coef_dev + r.coef_base;
    for (int c = 0; c < MIJPEG_MAX_COMPONENTS; c++) it.planes[c] = c < r.info.components ? planes[(size_t)i * MIJPEG_MAX_COMPONENTS + c] : nullptr;
    it.row_stride = row_strides[i];
    items.push_back(it);
    item_image.push_back(i);
  }
  int failed = MIJPEG_OK, failed_item = -1;
  std::string failed_msg;
  if (!items.empty()) {
    failed = reconstruct_planar_items(d, items.data(), (int)items.size(), flags, &failed_item);
    if (failed && failed_item < 0) return failed; // (a group launch or the tables' memory: the device's failure ends the call)
    if (failed) failed_msg = "image " + std::to_string(item_image[(size_t)failed_item]) + " of the ragged batch was not reconstructed";
    d->planar_stats.images = d->planar_stats.fused + d->planar_stats.two_pass;
  }
  // images of the single-image route, on their own objects (which wait for their kernels themselves)
  for (int i = 0; i < n; i++) {
    mijpeg_decoder::RaggedImage &r = d->ragged[(size_t)i];
    if (!r.child || !wanted(i)) continue;
    const int rc = mijpeg_reconstruct_planar_device(r.child, planes + (size_t)i * MIJPEG_MAX_COMPONENTS, row_strides[i], flags, 1);
    if (!rc) {
      const mijpeg_planar_stats &s = r.child->planar_stats;
      d->planar_stats.images += s.images; d->planar_stats.fused += s.fused; d->planar_stats.two_pass += s.two_pass;
      d->planar_stats.fused_launches += s.fused_launches; d->planar_stats.two_pass_launches += s.two_pass_launches;
    } else if (!failed) {
      const char *msg = nullptr;
      (void)mijpeg_last_error(r.child, &msg);
      failed = rc;
      failed_msg = "image " + std::to_string(i) + " of the ragged batch was not reconstructed: " + (msg ? msg : "");
    }
  }
  if (sync) HIP_TRY(d, hipStreamSynchronize(d->stream));
  if (failed) return set_error(d, failed, failed_msg);
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_reconstruct_ragged_planar_device"); }

} // extern "C"

// ------------------------------------------------------------------------------------------------
// crop windows (include/mijpeg.h)
// ------------------------------------------------------------------------------------------------
// The rectangle w of the full picture at `full` (interleaved, tightly packed lines) to the caller's memory on the object's stream:
// a strided device copy, or -- planar -- deinterleave_kernel with an offset source
static int copy_rect_out(mijpeg_decoder *d, const uint8_t *full, const mijpeg_info &f, const mijpeg_rect &w, void *const *ptrs, int64_t row_stride, bool planar)
{
  const int sb = sample_bytes_of(f);
  const int64_t bpp = (int64_t)f.components * sb, line = (int64_t)f.width * bpp;
  const int32_t cw = w.max_x - w.min_x + 1, ch = w.max_y - w.min_y + 1;
  const uint8_t *src = full + (int64_t)w.min_y * line + (int64_t)w.min_x * bpp;
  if (!planar) {
    HIP_TRY(d, hipMemcpy2DAsync(ptrs[0], (size_t)row_stride, src, (size_t)line, (size_t)(cw * bpp), (size_t)ch, hipMemcpyDeviceToDevice, d->stream));
    return MIJPEG_OK;
  }
  DeinterleaveArgs a;
  memset(&a, 0, sizeof(a));
  a.src = src;
  a.src_row = line;
  a.ncomp = f.components; a.sample_bytes = sb;
  a.width = cw; a.height = ch;
  for (int c = 0; c < f.components; c++) a.dst[c] = (uint8_t *)ptrs[c];
  a.dst_row = row_stride;
  return launch_deinterleave(a, d->stream) ? MIJPEG_ERR_DEVICE : MIJPEG_OK;
}

// The two crop calls' body.  planar: ptrs holds MIJPEG_MAX_COMPONENTS entries per picture, else one.
static int reconstruct_ragged_rect(mijpeg_decoder *d, const mijpeg_rect *rects, void *const *ptrs, const int64_t *row_strides, uint32_t flags, int sync, bool planar)
{
  if (!d || !rects || !ptrs || !row_strides) return MIJPEG_ERR_INVALID_PARAMETER;
  if (d->device < 0) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "decoder was created without a device");
  if (d->ragged_n < 1) return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "no decoded ragged batch: call mijpeg_decode_ragged_device first");
  const int n = d->ragged_n;
  const size_t per = planar ? MIJPEG_MAX_COMPONENTS : 1;
  flags &= planar ? PLANAR_FLAGS : ~(uint32_t)(MIJPEG_FLAG_DEVICE_OUTPUT | MIJPEG_FLAG_NO_UPSAMPLING | MIJPEG_FLAG_SPECULATIVE);
  auto wanted = [&](int i) { return !d->ragged[(size_t)i].status && ptrs[(size_t)i * per] != nullptr; };
  // every rectangle and every destination, before anything is launched, written or counted
  std::vector<mijpeg_rect> win((size_t)n);
  for (int i = 0; i < n; i++) {
    if (!wanted(i)) continue;
    const mijpeg_info &f = d->ragged[(size_t)i].info;
    if (!fused_window_clip(rects[i], f.width, f.height, win[(size_t)i]))
      return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "crop of image " + std::to_string(i) + ": min_x / min_y lie outside the picture, or min > max");
    const int64_t crop_line = (int64_t)(win[(size_t)i].max_x - win[(size_t)i].min_x + 1) * sample_bytes_of(f) * (planar ? 1 : f.components);
    bool ok = f.components >= 1 && f.components <= MIJPEG_MAX_COMPONENTS && row_strides[i] >= crop_line;
    for (int c = 0; planar && ok && c < f.components; c++) ok = ptrs[(size_t)i * per + (size_t)c] != nullptr;
    if (!ok)
      return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "crop destination of image " + std::to_string(i) + ": the row stride is smaller than a line of the crop, or a plane pointer is NULL");
  }
  HIP_TRY(d, hipSetDevice(d->device));
  d->rect_stats = mijpeg_ragged_rect_stats{};
  // Group pictures whose plan has a window flavour (plan_reconstruct with the crop's stride: fits32 is the kernels' 32-bit offsets
  // from canvas pixel (0, 0)) share one window launch per kernel and arithmetic flavour, as the full calls' launches do
  static const uint16_t per_frame_tables = 0; // (the planner only asks whether a batch brings per-frame tables: the list launches do)
  std::vector<FusedListItem> items;
  std::vector<FusedListLaunch> launches;
  std::vector<int> copies; // group pictures of the copy route
  bool children = false;
  size_t staging = 0;
  for (int i = 0; i < n; i++) {
    const mijpeg_decoder::RaggedImage &r = d->ragged[(size_t)i];
    if (!wanted(i)) continue;
    if (r.group < 0) { children |= r.child != nullptr; continue; }
    void *const *p = ptrs + (size_t)i * per;
    mijpeg_batch b = batch_of(r.info, d->coef_dev + r.coef_base, p[0], row_strides[i], 0, 1, flags);
    b.quant_dev = &per_frame_tables;
    const ReconPlan plan = plan_reconstruct(&b);
    if (!window_twin(plan, planar && r.info.components == 3)) {
      copies.push_back(i);
      staging = std::max(staging, (size_t)r.info.height * (size_t)r.info.width * (size_t)r.info.components * (size_t)sample_bytes_of(r.info));
      continue;
    }
    fused_list_add(launches, plan, (int)items.size(), r.info, &win[(size_t)i]);
    const bool planes = planar && r.info.components == 3;
    items.push_back(FusedListItem{&r.info, r.coef_base, {p[0], planes ? p[1] : nullptr, planes ? p[2] : nullptr}, row_strides[i], nullptr, &win[(size_t)i]});
    d->rect_stats.workgroups_full += (int64_t)fused_list_tiles(r.info);
  }
  // (a child reconstructs into its own buffer on its own stream, and this object's stream copies from there: the copies an earlier
  // call without sync left on this stream are done before a child's buffer is written again)
  if (children) HIP_TRY(d, hipStreamSynchronize(d->stream));
  const int made = launch_fused_lists(d, items.data(), launches, planar, true);
  if (made < 0) return made;
  d->rect_stats.launches = made;
  d->rect_stats.fused = (int32_t)items.size();
  for (const FusedListLaunch &l : launches) d->rect_stats.workgroups += (int64_t)l.grid;
  // The copy route: the picture in full, as the full calls reconstruct it, into a buffer of the object (one after the other: the
  // stream orders them), and its rectangle to the caller.  One picture that fails does not stop the others (the full calls' rule).
  if (staging) {
    const int rc = ensure_dev(d, (void **)&d->rect_tmp_dev, &d->rect_tmp_cap, staging);
    if (rc) return rc;
  }
  int failed = MIJPEG_OK;
  std::string failed_msg;
  auto fail = [&](int i, int rc, const char *msg) {
    if (failed) return;
    failed = rc;
    failed_msg = "image " + std::to_string(i) + " of the ragged batch was not reconstructed" + (msg ? std::string(": ") + msg : std::string());
  };
  for (int i : copies) {
    const mijpeg_decoder::RaggedImage &r = d->ragged[(size_t)i];
    const int64_t line = (int64_t)r.info.width * r.info.components * sample_bytes_of(r.info);
    mijpeg_batch b = batch_of(r.info, d->coef_dev + r.coef_base, d->rect_tmp_dev, line, line * r.info.height, 1, flags);
    int rc = reconstruct_on(d, b, nullptr, nullptr);
    if (!rc) rc = copy_rect_out(d, d->rect_tmp_dev, r.info, win[(size_t)i], ptrs + (size_t)i * per, row_strides[i], planar);
    if (rc) fail(i, rc, nullptr);
    else d->rect_stats.copied++;
  }
  for (int i = 0; i < n; i++) {
    mijpeg_decoder::RaggedImage &r = d->ragged[(size_t)i];
    if (!r.child || !wanted(i)) continue;
    mijpeg_decoder *c = r.child;
    const int64_t line = (int64_t)r.info.width * r.info.components * sample_bytes_of(r.info);
    int rc = ensure_dev(c, (void **)&c->rect_tmp_dev, &c->rect_tmp_cap, (size_t)(line * r.info.height));
    if (!rc) rc = mijpeg_reconstruct_device(c, c->rect_tmp_dev, line, flags, 1); // (waits: the copy below is on another stream)
    if (rc) {
      const char *msg = nullptr;
      (void)mijpeg_last_error(c, &msg);
      fail(i, rc, msg ? msg : "");
      continue;
    }
    rc = copy_rect_out(d, c->rect_tmp_dev, r.info, win[(size_t)i], ptrs + (size_t)i * per, row_strides[i], planar);
    if (rc) fail(i, rc, nullptr);
    else d->rect_stats.copied++;
  }
  d->rect_stats.images = d->rect_stats.fused + d->rect_stats.copied;
  if (sync) HIP_TRY(d, hipStreamSynchronize(d->stream));
  if (failed) return set_error(d, failed, failed_msg);
  return MIJPEG_OK;
}

extern "C" {

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

} // extern "C"

// ------------------------------------------------------------------------------------------------
// crops resized into one batch tensor (include/mijpeg.h), and the same as a normalised float batch, mirrored per
// picture: one driver, the resized call is its {uint8 samples, nobody mirrored}
// ------------------------------------------------------------------------------------------------
static_assert(MIJPEG_SAMPLE_U8 == RESAMPLE_U8 && MIJPEG_SAMPLE_F32 == RESAMPLE_F32 && MIJPEG_SAMPLE_F16 == RESAMPLE_F16 && MIJPEG_SAMPLE_BF16 == RESAMPLE_BF16,
              "the header's sample types are the kernels'");

// Why the resized call does not serve a decoded picture, or 0
static int resized_refusal(const mijpeg_info &f, int32_t channels)
{
  if (sample_bytes_of(f) != 1) return MIJPEG_ERR_NOT_IMPLEMENTED;
  if (f.components != 1 && f.components != 3) return MIJPEG_ERR_NOT_IMPLEMENTED;
  if (f.components == 3 && channels == 1) return MIJPEG_ERR_NOT_IMPLEMENTED;
  return 0;
}

// Stage 2: the tables of the served pictures in one pinned upload, and the one launch
static int launch_resample(mijpeg_decoder *d, const ResampleItem *items, const ResampleLayout &L, int32_t out_w, int32_t out_h, int32_t channels,
                           const mijpeg_batch_format &format, void *dst, int64_t image_stride, int64_t plane_stride, int64_t row_stride)
{
  int rc = ensure_dev(d, (void **)&d->resized_desc_dev, &d->resized_desc_cap, L.table_bytes);
  if (rc) return rc;
  if (d->resized_upload_pending) { // (the pinned copy travels asynchronously: the last call's must have left)
    HIP_TRY(d, hipEventSynchronize(d->resized_uploaded));
    d->resized_upload_pending = false;
  }
  if ((rc = ensure_pinned(d, &d->resized_desc_host, &d->resized_desc_host_cap, L.table_bytes))) return rc;
  const int served = (int)L.per.size(), workers = std::min(served, default_threads());
  std::vector<char> bad((size_t)workers, 0);
  parallel_for(workers, [&](int w) { // (a division per tap: a list of 256 pictures has half a million)
    for (int k = w; k < served; k += workers)
      if (!resample_fill(d->resized_desc_host, L, (size_t)k, items, out_w, out_h, image_stride)) bad[(size_t)w] = 1;
  });
  resample_fill_first(d->resized_desc_host, L);
  for (char b : bad)
    if (b) return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "the resample filter has no taps for these sizes");
  HIP_TRY(d, hipMemcpyAsync(d->resized_desc_dev, d->resized_desc_host, L.table_bytes, hipMemcpyHostToDevice, d->stream));
  if (!d->resized_uploaded) HIP_TRY(d, hipEventCreateWithFlags(&d->resized_uploaded, hipEventDisableTiming));
  HIP_TRY(d, hipEventRecord(d->resized_uploaded, d->stream));
  d->resized_upload_pending = true;
  ResampleArgs a;
  memset(&a, 0, sizeof(a));
  a.src = d->resized_arena_dev;
  a.dst = (uint8_t *)dst;
  a.tables = d->resized_desc_dev;
  a.pictures = (const ResamplePicture *)(d->resized_desc_dev + L.pictures);
  a.first = (const uint32_t *)(d->resized_desc_dev + L.first);
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
  if (!d || !dst) return MIJPEG_ERR_INVALID_PARAMETER;
  if (!format) return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "normalised call: format is NULL");
  if (d->device < 0) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "decoder was created without a device");
  if (d->ragged_n < 1) return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "no decoded ragged batch: call mijpeg_decode_ragged_device first");
  const int n = d->ragged_n;
  // every parameter, before anything is launched, written or counted
  if (out_w < 1 || out_h < 1 || out_w > RESAMPLE_MAX_AXIS || out_h > RESAMPLE_MAX_AXIS) return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "resized call: out_width and out_height are 1 .. 65535");
  if (channels != 1 && channels != 3) return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "resized call: channels is 1 or 3");
  if (format->sample < MIJPEG_SAMPLE_U8 || format->sample > MIJPEG_SAMPLE_BF16 || format->reserved != 0)
    return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "normalised call: sample is a MIJPEG_SAMPLE_*, reserved is 0");
  if (format->sample != MIJPEG_SAMPLE_U8)
    for (int c = 0; c < channels; c++)
      if (!std::isfinite(format->scale[c]) || !std::isfinite(format->bias[c])) return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "normalised call: scale and bias are finite");
  const int64_t es = (int64_t)resample_sample_bytes(format->sample); // (every stride is in bytes)
  if ((uintptr_t)dst % (uintptr_t)es || image_stride % es || plane_stride % es || row_stride % es)
    return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "normalised call: dst_device and the strides are multiples of the element size");
  const bool planar = plane_stride != 0;
  if (row_stride < 1 || row_stride > 0xffffffffll || plane_stride < 0 || plane_stride > 0xffffffffll) // (what follows then stays inside 64 bits)
    return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "resized call: a stride is smaller than the data it spans, or a slot spans 4 GiB or more");
  const int64_t line = (int64_t)out_w * (planar ? 1 : channels) * es, plane = (int64_t)(out_h - 1) * row_stride + line;
  const int64_t slot = planar ? (int64_t)(channels - 1) * plane_stride + plane : plane;
  if (row_stride < line || (planar && plane_stride < plane) || image_stride < slot || slot > 0xffffffffll)
    return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "resized call: a stride is smaller than the data it spans, or a slot spans 4 GiB or more");
  const mijpeg_rect whole{0, 0, INT32_MAX, INT32_MAX};
  std::vector<mijpeg_rect> asked((size_t)n, whole), win((size_t)n);
  for (int i = 0; i < n; i++) {
    const mijpeg_decoder::RaggedImage &r = d->ragged[(size_t)i];
    if (r.status) continue;
    if (rects) asked[(size_t)i] = rects[i];
    if (!fused_window_clip(asked[(size_t)i], r.info.width, r.info.height, win[(size_t)i]))
      return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "crop of image " + std::to_string(i) + ": min_x / min_y lie outside the picture, or min > max");
  }
  // who is served, and where everything lies
  std::vector<ResampleItem> items((size_t)n);
  std::vector<int32_t> st((size_t)n, 0);
  for (int i = 0; i < n; i++) {
    const mijpeg_decoder::RaggedImage &r = d->ragged[(size_t)i];
    ResampleItem &it = items[(size_t)i];
    it.slot = i;
    st[(size_t)i] = r.status ? r.status : resized_refusal(r.info, channels);
    if (st[(size_t)i]) continue;
    it.src_w = win[(size_t)i].max_x - win[(size_t)i].min_x + 1;
    it.src_h = win[(size_t)i].max_y - win[(size_t)i].min_y + 1;
    it.comps = r.info.components;
    it.mirror = format->mirror && format->mirror[i];
    if ((uint64_t)it.src_w * (uint64_t)it.src_h * (uint64_t)it.comps > 0xffffffffull) { st[(size_t)i] = MIJPEG_ERR_NOT_IMPLEMENTED; continue; } // (the kernel's 32-bit offsets)
    it.served = true;
  }
  {
    const int workers = std::min(n, default_threads());
    parallel_for(workers, [&](int w) { // (a pass over every output sample of both axes: one picture per worker)
      for (int i = w; i < n; i += workers)
        if (items[(size_t)i].served) resample_item_caps(items[(size_t)i], out_w, out_h);
    });
  }
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
    const int rc = ensure_dev(d, (void **)&d->resized_arena_dev, &d->resized_arena_cap, L.arena_bytes + RESAMPLE_ARENA_SPARE);
    if (rc) return rc;
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
    const int rc2 = launch_resample(d, items.data(), L, out_w, out_h, channels, *format, dst, image_stride, plane_stride, row_stride);
    if (rc2) return rc2;
    stats.resample_launches = 1;
  }
  d->resized_stats = stats;
  d->normalized_stats = nstats;
  if (status)
    for (int i = 0; i < n; i++) status[i] = st[(size_t)i];
  if (sync) HIP_TRY(d, hipStreamSynchronize(d->stream));
  return MIJPEG_OK;
}

extern "C" {

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
