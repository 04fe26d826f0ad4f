// ragged_decode.cpp -- ragged batches: streams of any shapes in one device pass (include/mijpeg.h): the planner, the
// decode (a Huffman launch per layout group, the single-image route for the rest).  What reconstructs the decoded list:
// ragged_reconstruct.cpp.  Private to libmijpeg.so.
#include <string.h>

#include <algorithm>
#include <string>

#include "reconstruct.hpp"

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
  d->ragged.assign((size_t)n, mijpeg_decoder::RaggedImage{});
  // headers and restart markers of all streams, one stream per worker.  mijpeg_set_device_markers: headers only where the parse
  // can leave the search to the device (HostDecoder::set_skip_search; Scan::search_skipped tells) -- such members are searched
  // inside their layout group's launch, beside members that were searched here
  const bool markers = d->device_markers == 1;
  std::vector<int> rcs;
  parse_stream_headers(d, streams, sizes, n, rcs, [&](HostDecoder &h, int i) {
    if (!streams[i] || !sizes[i]) return (int)MIJPEG_ERR_STREAM_EMPTY; // (nothing to parse)
    if (markers) h.set_skip_search(); // (armed for the parse that follows)
    return 0;
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

} // extern "C"
