// batch_decode.cpp -- uniform batches of the C ABI (include/mijpeg.h): n streams of one geometry -> n coefficient stores -> n frames, two
// kernel launches in all.  The header pass over a list of streams (ragged_decode.cpp runs it too), submit_batch and finish_batch as
// named stages, the speculative reconstruction and its validation, the host half alone (mijpeg_prepare_batch_host), and the marker
// route option (mijpeg_set_device_markers) with its queries.  The decoder object itself: capi.cpp.  Private to libmijpeg.so.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <mutex>
#include <string>

#include "reconstruct.hpp"

using namespace mij;

// The marker route of a call (mijpeg_set_device_markers) is an attempt: it ends well, or the call runs the ordinary route as if
// the option were off -- error state included (whatever the attempt reported is taken back).  Counts the images either way.
int with_device_markers(mijpeg_decoder *d, int images, const std::function<int(bool)> &attempt)
{
  if (d->device_markers == 1) {
    const int keep_code = d->err_code;
    const std::string keep_msg = d->err_msg;
    d->markers_retry = false;
    d->markers_staged.clear();
    if (attempt(true) == MIJPEG_OK) {
      d->markers_searched += images;
      return MIJPEG_OK;
    }
    d->markers_staged.clear();
    d->markers_declined += images;
    d->err_code = keep_code;
    d->err_msg = keep_msg;
  }
  return attempt(false);
}

// ------------------------------------------------------------------------------------------------
// the header pass: headers (and, unless the device searches, restart markers) of all streams of a list, one stream per worker
// ------------------------------------------------------------------------------------------------
void parse_stream_headers(mijpeg_decoder *d, const uint8_t *const *streams, const size_t *sizes, int n, std::vector<int> &rcs, const StreamArm &arm,
                          const StreamAfter &after)
{
  if (d->batch_hosts.size() < (size_t)n) d->batch_hosts.resize((size_t)n); // never shrinks: a pipeline's chunks differ in size, and
  for (auto &h : d->batch_hosts)                                         // a parser that is thrown away takes its grown vectors along
    if (!h) h.reset(new HostDecoder());
  rcs.assign((size_t)n, 0);
  const int workers = std::min(n, default_threads());
  parallel_for(workers, [&](int w) {
    for (int i = w; i < n; i += workers) {
      HostDecoder &h = *d->batch_hosts[(size_t)i];
      if ((rcs[(size_t)i] = arm(h, i)) != 0) continue;
      rcs[(size_t)i] = h.parse(streams[i], sizes[i], false);
      if (after) after(h, i, rcs[(size_t)i]);
    }
  });
}

std::vector<HostDecoder *> batch_host_list(mijpeg_decoder *d, int n)
{
  std::vector<HostDecoder *> hosts((size_t)n);
  for (int i = 0; i < n; i++) hosts[(size_t)i] = d->batch_hosts[(size_t)i].get();
  return hosts;
}

// What the header pass of a uniform call reports: the first stream that failed, with its parser's message
static int first_failure(mijpeg_decoder *d, const std::vector<int> &rcs)
{
  for (size_t i = 0; i < rcs.size(); i++)
    if (rcs[i]) return set_error(d, rcs[i], d->batch_hosts[i]->error.message);
  return MIJPEG_OK;
}

// What the last finished batch of shared tables reported, for the speculative launch of the next one (MIJPEG_FLAG_SPECULATIVE):
// frame geometry, tables, and the range check that selected its kernel.  Process-wide: the decoder objects of a pipeline work
// on chunks of the same material.  (extern "C" as when they stood inside capi.cpp's block: the compiler gives such functions C names
// that the library exports, unnamed namespace or not, and the export list is compared from commit to commit -- it stays what it was.)
extern "C" {
namespace {
struct SpecHint {
  std::mutex m;
  bool valid = false;
  mijpeg_info info{};
};
SpecHint *spec_hint()
{
  static SpecHint *h = new SpecHint;
  return h;
}
// an assumed range just below the next gate selects the kernel the hint's batch ran on and holds for every batch that stays
// below that gate
int32_t next_gate_below(int32_t range)
{
  for (int32_t g : RANGE_GATES)
    if (range < g) return g - 1;
  return -1;
}
bool same_shape_and_tables(const mijpeg_info &a, const mijpeg_info &b)
{
  if (a.width != b.width || a.height != b.height || a.components != b.components || a.precision != b.precision || a.ycbcr != b.ycbcr || a.xt != b.xt ||
      a.dnl != b.dnl || a.coef_count != b.coef_count)
    return false;
  for (int c = 0; c < a.components; c++) {
    if (a.hsamp[c] != b.hsamp[c] || a.vsamp[c] != b.vsamp[c]) return false;
    if (memcmp(a.quant[a.quant_index[c]], b.quant[b.quant_index[c]], sizeof(a.quant[0]))) return false;
  }
  return true;
}
} // namespace
} // extern "C"

// ------------------------------------------------------------------------------------------------
// submit: parse, gather, enqueue upload + Huffman kernel
// ------------------------------------------------------------------------------------------------
static int finish_batch(mijpeg_decoder *d);

namespace {
using clk = std::chrono::steady_clock;
// One submit_batch: the call's arguments and what travels between its stages, which run in the order they stand in
struct BatchSubmit {
  mijpeg_decoder *d;
  const uint8_t *const *streams;
  const size_t *sizes;
  int n, min_intervals;
  bool defer, markers;
  clk::time_point t0 = clk::now(), t_parsed{};
  std::vector<HostDecoder *> hosts{};
  bool own_tables = false;

  // what is outstanding on the object is settled, and the object holds no batch
  int settle()
  {
    if (d->spec_active) { // a speculative reconstruction nobody validated (mijpeg_finish_batch_device): its verdict comes first
      const int src = settle_speculation(d);
      if (src) return src;
    }
    if (const int prc = settle_pending(d)) return prc; // a submitted batch nobody waited for: its staging buffers are about to be reused
    d->batch_frames = 0;
    d->ragged_n = 0; // (a ragged batch's coefficient stores are about to be overwritten)
    return MIJPEG_OK;
  }
  // headers and restart markers of all streams, one stream per worker -- which writes the device's copy of the entropy
  // coded data (no byte stuffing, no markers) into the stream's slot of the pinned gathering area while it is at it
  int headers()
  {
    std::vector<size_t> slot;
    const size_t total = stream_slots(sizes, n, slot);
    const int src = ensure_pinned(d, &d->stage_host, &d->stage_cap, total);
    if (src) return src;
    // (a worker walks ~3 GB/s this way: good for the many small streams of a batch; a large stream is searched in
    // parallel chunks and gathered in parallel pieces instead -- device_entropy_batch sees which it was)
    const bool sink_all = n >= default_threads();
    std::vector<int> rcs;
    parse_stream_headers(d, streams, sizes, n, rcs, [&](HostDecoder &h, int i) {
      if (markers) h.set_skip_search(); // (headers only: the device searches the segments)
      else if (sizes[i] <= ((size_t)2 << 20) || sink_all) h.set_unstuff_sink(d->stage_host + slot[(size_t)i], sizes[i]);
      return 0;
    });
    if (const int rc = first_failure(d, rcs)) return rc;
    t_parsed = clk::now();
    hosts = batch_host_list(d, n);
    return MIJPEG_OK;
  }
  // what keeps a stream off the route the call takes
  int obstacles() const
  {
    for (int i = 0; i < n; i++)
      if (const char *why = markers ? device_markers_obstacle(*hosts[(size_t)i], sizes[i]) : device_entropy_obstacle(*hosts[(size_t)i], sizes[i]))
        return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, why);
    return MIJPEG_OK;
  }
  // one reconstruction launch serves the batch; images with tables of their own (motion JPEG under rate control) make it
  // read per-frame tables from device memory instead of the kernel arguments
  void test_own_tables()
  {
    const mijpeg_info &f0 = hosts[0]->info;
    for (int i = 1; i < n && !own_tables; i++) {
      const mijpeg_info &f = hosts[(size_t)i]->info;
      for (int c = 0; c < f.components; c++)
        if (memcmp(f.quant[f.quant_index[c]], f0.quant[f0.quant_index[c]], sizeof(f.quant[0]))) own_tables = true;
    }
  }
  // the coefficient stores of the n frames; only with them in hand does the object let go of what it held
  int store()
  {
    const int rc = ensure_coef_store(d, (size_t)hosts[0]->info.coef_count * (size_t)n, false);
    if (rc) return rc;
    d->img_valid = d->model_valid = false;
    d->uploaded = false;
    d->decoded = false;
    d->pend_n = 0;
    return MIJPEG_OK;
  }
  // upload + Huffman kernel (enqueued only where defer); the marker route notes where each raw segment was staged
  int launch()
  {
    EntropyBatchOptions opt;
    opt.defer = defer;
    opt.markers = markers;
    const int rc = device_entropy_batch(d, hosts.data(), streams, sizes, n, min_intervals, d->coef_dev, hosts[0]->info.coef_count, opt);
    if (!rc && markers) {
      std::vector<size_t> slot;
      stream_slots(sizes, n, slot);
      for (int i = 0; i < n; i++) d->markers_staged.emplace_back(slot[(size_t)i], sizes[i] - hosts[(size_t)i]->scans[0].ecs_begin);
    }
    return rc;
  }
  // the call's timings; the batch is the object's, decoded or on its way -- rc: what launch() returned
  int hand_over(int rc)
  {
    d->timing[0] = std::chrono::duration<double>(clk::now() - t0).count();
    d->timing[1] = std::chrono::duration<double>(t_parsed - t0).count();
    d->timing[2] = d->phase_prepare;
    d->timing[3] = d->phase_device;
    if (rc) { // (device_entropy_batch has waited for whatever it enqueued before the failure)
      d->pend_n = 0;
      return rc;
    }
    d->batch_own_tables = own_tables;
    d->batch_frames = -n; // decoded (or on its way) but not aggregated yet
    if (d->pend_n) return MIJPEG_OK; // deferred: finish_batch() waits
    return finish_batch(d);
  }
};
} // namespace

static int submit_batch(mijpeg_decoder *d, const uint8_t *const *streams, const size_t *sizes, int n, int min_intervals, bool defer, bool markers)
{
  if (!d || !streams || !sizes || n < 1) return MIJPEG_ERR_INVALID_PARAMETER;
  if (d->device < 0) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "decoder was created without a device");
  HIP_TRY(d, hipSetDevice(d->device));
  BatchSubmit s{d, streams, sizes, n, min_intervals, defer, markers};
  int rc = s.settle();
  if (!rc) rc = s.headers();
  if (!rc) rc = s.obstacles();
  if (rc) return rc;
  s.test_own_tables();
  rc = s.store();
  if (rc) return rc;
  return s.hand_over(s.launch());
}

// ------------------------------------------------------------------------------------------------
// finish: the verdicts of the submitted work, then the aggregation over the images of the decoded batch -- what one
// reconstruction launch for all of them needs to know
// ------------------------------------------------------------------------------------------------
// The upload and the Huffman kernel of the submitted batch are through
static int wait_for_submitted(mijpeg_decoder *d)
{
  // The pipeline's one wait on the device.  hipStreamSynchronize blocks on an interrupt after a short spin, and how long the wake-up
  // takes is the host's business (idle states of the core that takes the interrupt): on some boxes 0.3 ms per wait for seconds
  // on end -- sixteen chunks of a batch, five milliseconds (profiles/r05/batch4k_stall.txt).  A submitted batch is a
  // millisecond from done when somebody asks for it: poll the stream for that long, block only beyond.
  static const bool no_spin = getenv("MIJPEG_NO_SPIN_WAIT") != nullptr; // A-B measurements
  const auto t_spin = std::chrono::steady_clock::now();
  hipError_t q = hipSuccess;
  while (!no_spin && (q = hipStreamQuery(d->stream)) == hipErrorNotReady) {
    if (std::chrono::steady_clock::now() - t_spin > std::chrono::milliseconds(4)) break;
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
  }
  // hipErrorNotReady is not an error: drop it -- and only it; anything else the query saw (a failed launch of the work it waits
  // for) is the batch's verdict
  if (q == hipErrorNotReady) (void)hipGetLastError();
  else if (q != hipSuccess) HIP_TRY(d, q);
  HIP_TRY(d, hipStreamSynchronize(d->stream));
  d->phase_device += std::chrono::duration<double>(std::chrono::steady_clock::now() - d->pend_t0).count();
  return MIJPEG_OK;
}

// What the submitted work of pn images reported: the marker search, the walk, the Huffman kernel's status words
static int submitted_verdicts(mijpeg_decoder *d, HostDecoder *const *hosts, int pn)
{
  // the device searched the segments: is every search good?  (The bytes are gone: the caller's fallback takes over.)  Asked first:
  // the walk of a stream without restart markers follows its search, and has walked nothing behind one that is not good
  if (d->pend_markers) {
    const uint32_t *results = d->pend_markers;
    d->pend_markers = nullptr;
    if (!device_markers_good(results, d->markers_want_term.data(), pn)) {
      d->markers_searched -= pn;
      d->markers_declined += pn;
      d->pend_walk_round = 0;
      return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "device marker search: a segment is not the plain case; the host searches such streams (mijpeg_decode_batch_device)");
    }
  }
  if (d->pend_walk_round > 0) { // streams without restart markers: did the walk settle within the rounds it was given?
    const int rounds = d->pend_walk_round;
    d->pend_walk_round = 0;
    if (d->pend_walk_flags[rounds]) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "speculative decoding did not settle in the rounds a submitted batch gets: decode it with mijpeg_decode_batch_device");
    d->walk_rounds = walk_rounds_needed(d->pend_walk_flags, rounds);
    if (d->pend_walk_status)
      if (const int wrc = walk_verdict(d, d->pend_walk_status, pn)) return wrc;
  }
  return evaluate_entropy_status(d, hosts, pn, d->pend_status);
}

// A batch whose images bring their own tables: the batch's info carries, per COMPONENT, the largest delta any image has at each
// position -- what the range gates of the kernel selection look at; the frames' tables go to the device
static int aggregate_own_tables(mijpeg_decoder *d, const std::vector<HostDecoder *> &hosts)
{
  const size_t n = hosts.size();
  const mijpeg_info &f0 = hosts[0]->info;
  d->batch_quant_host.assign(n * 4 * 64, 1);
  mijpeg_info &bi = d->batch_info;
  for (int c = 0; c < f0.components; c++) {
    bi.quant_index[c] = (uint8_t)c;
    for (int k = 0; k < 64; k++) bi.quant[c][k] = 0;
  }
  for (size_t i = 0; i < n; i++) {
    const mijpeg_info &f = hosts[i]->info;
    for (int c = 0; c < f.components; c++)
      for (int k = 0; k < 64; k++) {
        const uint16_t q = f.quant[f.quant_index[c]][k];
        d->batch_quant_host[(i * 4 + c) * 64 + k] = q;
        bi.quant[c][k] = std::max(bi.quant[c][k], q);
      }
  }
  const size_t bytes = d->batch_quant_host.size() * sizeof(uint16_t);
  if (const int rc = ensure_dev(d, (void **)&d->batch_quant_dev, &d->batch_quant_cap, bytes)) return rc;
  HIP_TRY(d, hipMemcpyAsync(d->batch_quant_dev, d->batch_quant_host.data(), bytes, hipMemcpyHostToDevice, d->stream));
  return MIJPEG_OK;
}

// the batch is as fast as its most demanding image
static void aggregate_ranges(mijpeg_decoder *d, const std::vector<HostDecoder *> &hosts)
{
  d->batch_info.fast_arith = 1;
  for (const HostDecoder *h : hosts) {
    const mijpeg_info &f = h->info;
    if (!f.fast_arith) d->batch_info.fast_arith = 0;
    for (int c = 0; c < f.components; c++) d->batch_info.range_max[c] = std::max(d->batch_info.range_max[c], f.range_max[c]);
  }
}

// the next batch of this shape may launch its reconstruction on this range check
static void leave_speculation_hint(const mijpeg_decoder *d)
{
  if (d->batch_own_tables || d->batch_info.xt) return;
  SpecHint &h = *spec_hint();
  std::lock_guard<std::mutex> lock(h.m);
  h.info = d->batch_info;
  h.valid = true;
}

static int finish_batch(mijpeg_decoder *d)
{
  const int n = d->batch_frames < 0 ? -d->batch_frames : 0;
  if (n == 0) return d->batch_frames > 0 ? MIJPEG_OK : set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "no batch has been submitted");
  d->batch_frames = 0; // (a finish that fails leaves no batch)
  const std::vector<HostDecoder *> hosts = batch_host_list(d, n);
  if (d->pend_n) { // wait for the upload and the Huffman kernel of the submitted batch, then look at what it reported
    const int pn = d->pend_n;
    d->pend_n = 0;
    if (const int rc = wait_for_submitted(d)) return rc;
    if (const int rc = submitted_verdicts(d, hosts.data(), pn)) return rc;
  }
  d->batch_info = hosts[0]->info;
  if (d->batch_own_tables)
    if (const int rc = aggregate_own_tables(d, hosts)) return rc;
  aggregate_ranges(d, hosts);
  d->batch_frames = n;
  leave_speculation_hint(d);
  return MIJPEG_OK;
}

// A speculative launch is validated: the batch is finished the ordinary way (wait, errors, range check), and where the range
// check is not the one the launch assumed the reconstruction runs again with the kernel the real one selects.
int settle_speculation(mijpeg_decoder *d)
{
  if (!d->spec_active) return MIJPEG_OK;
  d->spec_active = false;
  d->spec_redone = false;
  if (d->batch_frames == 0) return MIJPEG_OK; // (the batch was abandoned: another stream was set on the object)
  if (d->batch_frames < 0) {
    const int rc = finish_batch(d);
    if (rc) return rc; // (the stream is damaged, the walk had not settled ...: nothing of the speculative pixels counts)
  }
  bool holds = d->batch_info.fast_arith != 0;
  for (int c = 0; c < d->batch_info.components; c++) holds = holds && d->batch_info.range_max[c] <= d->spec_assumed[c];
  if (holds) return MIJPEG_OK;
  d->spec_redone = true;
  d->spec_redone_count++;
  return mijpeg_reconstruct_batch_device(d, d->spec_dst, d->spec_frame_stride, d->spec_row_stride, d->spec_flags & ~MIJPEG_FLAG_SPECULATIVE, 1);
}

// The submitted batch is awaited here: a speculative launch on it is validated (which finishes the batch), any other is finished
static int await_batch(mijpeg_decoder *d) { return d->spec_active ? settle_speculation(d) : finish_batch(d); }

// The host half of a submit alone: headers, and the streams' entropy coded data in their slots of the gathering area (pinned where
// the object has a device) -- unstuffed by the parse, or (the marker route) the raw segment as the device would search it
static int prepare_batch_host(mijpeg_decoder *d, const uint8_t *const *streams, const size_t *sizes, int n, bool markers)
{
  if (const int prc = settle_pending(d)) return prc;
  d->batch_frames = 0;
  std::vector<size_t> slot;
  const size_t total = stream_slots(sizes, n, slot);
  uint8_t *stage;
  if (d->device >= 0) {
    HIP_TRY(d, hipSetDevice(d->device));
    if (const int src = ensure_pinned(d, &d->stage_host, &d->stage_cap, total)) return src;
    stage = d->stage_host;
  } else {
    if (d->host_stage.size() < total) d->host_stage.resize(total);
    stage = d->host_stage.data();
  }
  std::vector<int> rcs;
  parse_stream_headers(
      d, streams, sizes, n, rcs,
      [&](HostDecoder &h, int i) {
        if (markers) h.set_skip_search(); // (the host half of the marker route: headers, and one memcpy of the raw segment)
        else h.set_unstuff_sink(stage + slot[(size_t)i], sizes[i]);
        return 0;
      },
      [&](HostDecoder &h, int i, int rc) {
        if (markers && !rc && !h.scans.empty() && h.scans[0].search_skipped)
          memcpy(stage + slot[(size_t)i], streams[i] + h.scans[0].ecs_begin, sizes[i] - h.scans[0].ecs_begin);
      });
  if (const int rc = first_failure(d, rcs)) return rc;
  for (int i = 0; i < n && markers; i++)
    if (const char *why = device_markers_obstacle(*d->batch_hosts[(size_t)i], sizes[i])) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, why);
  for (int i = 0; i < n && markers; i++) d->markers_staged.emplace_back(slot[(size_t)i], sizes[i] - d->batch_hosts[(size_t)i]->scans[0].ecs_begin);
  return MIJPEG_OK;
}

// A submitted batch whose Huffman kernel may still be running: the reconstruction can be launched behind it on the range check the
// last batch of this shape and these tables reported (rounded up to the selection's next gate) instead of waiting for this
// one's.  The pipeline's host thread never blocks on the device; mijpeg_finish_batch_device validates.  -> whether, and the
// frame description to launch on
static bool speculation_possible(mijpeg_decoder *d, uint32_t flags, int sync, mijpeg_info &assumed)
{
  if (!(d->batch_frames < 0 && (flags & MIJPEG_FLAG_SPECULATIVE) && !sync && d->pend_n && !d->pend_walk_round && !d->batch_own_tables && !d->spec_active)) return false;
  const mijpeg_info &f0 = d->batch_hosts[0]->info;
  SpecHint &h = *spec_hint();
  std::lock_guard<std::mutex> lock(h.m);
  if (!h.valid || !h.info.fast_arith || !same_shape_and_tables(h.info, f0)) return false;
  assumed = f0;
  assumed.fast_arith = 1;
  bool speculate = true;
  for (int c = 0; c < f0.components; c++) {
    assumed.range_max[c] = next_gate_below(h.info.range_max[c]);
    if (assumed.range_max[c] < 0) speculate = false;
  }
  return speculate;
}

extern "C" {

int mijpeg_decode_batch_device(mijpeg_decoder *d, const uint8_t *const *streams, const size_t *sizes, int n, int min_intervals)
try {
  if (!d || !streams || !sizes || n < 1) return MIJPEG_ERR_INVALID_PARAMETER;
  return with_device_markers(d, n, [&](bool markers) { return submit_batch(d, streams, sizes, n, min_intervals, false, markers); });
} catch (...) { return boundary_catch(d, "mijpeg_decode_batch_device"); }

int mijpeg_prepare_batch_host(mijpeg_decoder *d, const uint8_t *const *streams, const size_t *sizes, int n)
try {
  if (!d || !streams || !sizes || n < 1) return MIJPEG_ERR_INVALID_PARAMETER;
  return with_device_markers(d, n, [&](bool markers) { return prepare_batch_host(d, streams, sizes, n, markers); });
} catch (...) { return boundary_catch(d, "mijpeg_prepare_batch_host"); }

int mijpeg_set_device_markers(mijpeg_decoder *d, int on)
try {
  if (!d) return MIJPEG_ERR_INVALID_PARAMETER;
  if (on != 0 && on != 1) return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "mijpeg_set_device_markers: on must be 0 or 1");
  d->device_markers = on;
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_set_device_markers"); }

int mijpeg_device_markers_stats(mijpeg_decoder *d, int64_t *searched, int64_t *declined)
try {
  if (!d) return MIJPEG_ERR_INVALID_PARAMETER;
  if (searched) *searched = d->markers_searched;
  if (declined) *declined = d->markers_declined;
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_device_markers_stats"); }

const uint8_t *mijpeg_device_markers_staging(mijpeg_decoder *d, int image, size_t *bytes)
{
  if (!d || image < 0 || (size_t)image >= d->markers_staged.size()) return nullptr;
  const uint8_t *stage = d->device >= 0 ? d->stage_host : d->host_stage.data();
  if (!stage) return nullptr;
  if (bytes) *bytes = d->markers_staged[(size_t)image].second;
  return stage + d->markers_staged[(size_t)image].first;
}

int64_t mijpeg_device_marker_search(mijpeg_decoder *d, const uint8_t *segment, size_t size, int32_t expect, uint8_t *dst, size_t capacity,
                                    uint32_t *begin, uint32_t *end, uint32_t *term, uint32_t *flags)
try {
  if (!d) return MIJPEG_ERR_INVALID_PARAMETER;
  if (expect > (1 << 26)) return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "mijpeg_device_marker_search: expect");
  return device_marker_search(d, segment, size, expect, dst, capacity, begin, end, term, flags);
} catch (...) { return boundary_catch(d, "mijpeg_device_marker_search"); }

int mijpeg_submit_batch_device(mijpeg_decoder *d, const uint8_t *const *streams, const size_t *sizes, int n, int min_intervals)
try {
  if (!d || !streams || !sizes || n < 1) return MIJPEG_ERR_INVALID_PARAMETER;
  return with_device_markers(d, n, [&](bool markers) { return submit_batch(d, streams, sizes, n, min_intervals, true, markers); });
} catch (...) { return boundary_catch(d, "mijpeg_submit_batch_device"); }

int mijpeg_finish_batch_device(mijpeg_decoder *d)
try {
  if (!d) return MIJPEG_ERR_INVALID_PARAMETER;
  if (d->device >= 0) HIP_TRY(d, hipSetDevice(d->device));
  return await_batch(d);
} catch (...) { return boundary_catch(d, "mijpeg_finish_batch_device"); }

int mijpeg_batch_speculation(mijpeg_decoder *d, int64_t *launched, int64_t *redone)
try {
  if (!d) return MIJPEG_ERR_INVALID_PARAMETER;
  if (launched) *launched = d->spec_launched;
  if (redone) *redone = d->spec_redone_count;
  return d->spec_redone ? 1 : 0;
} catch (...) { return boundary_catch(d, "mijpeg_batch_speculation"); }

int mijpeg_reconstruct_batch_device(mijpeg_decoder *d, void *dst_device, int64_t frame_stride, int64_t row_stride, uint32_t flags, int sync)
try {
  if (!d || !dst_device) return MIJPEG_ERR_INVALID_PARAMETER;
  if (d->device >= 0) HIP_TRY(d, hipSetDevice(d->device));
  mijpeg_info assumed;
  const bool speculate = speculation_possible(d, flags, sync, assumed);
  if (d->batch_frames < 0 && !speculate) // submitted with mijpeg_submit_batch_device: wait for it now
    if (const int rc = await_batch(d)) return rc;
  if (d->batch_frames < 1 && !speculate) return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "no decoded batch: call mijpeg_decode_batch_device first");
  mijpeg_batch b = batch_of(speculate ? assumed : d->batch_info, d->coef_dev, dst_device, row_stride, frame_stride, speculate ? -d->batch_frames : d->batch_frames,
                            flags & ~(MIJPEG_FLAG_DEVICE_OUTPUT | MIJPEG_FLAG_NO_UPSAMPLING | MIJPEG_FLAG_SPECULATIVE));
  b.quant_dev = d->batch_own_tables ? d->batch_quant_dev : nullptr;
  if (const int rc = reconstruct_on(d, b, nullptr, "batch")) return rc;
  if (speculate) {
    d->spec_active = true;
    d->spec_redone = false;
    d->spec_dst = dst_device;
    d->spec_frame_stride = frame_stride;
    d->spec_row_stride = row_stride;
    d->spec_flags = flags;
    for (int c = 0; c < MIJPEG_MAX_COMPONENTS; c++) d->spec_assumed[c] = assumed.range_max[c];
    d->spec_launched++;
    return MIJPEG_OK;
  }
  if (sync) HIP_TRY(d, hipStreamSynchronize(d->stream));
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_reconstruct_batch_device"); }

int mijpeg_reconstruct_batch_planar_device(mijpeg_decoder *d, void *dst_device, int64_t frame_stride, int64_t plane_stride, int64_t row_stride, uint32_t flags,
                                           int sync)
try {
  if (!d || !dst_device) return MIJPEG_ERR_INVALID_PARAMETER;
  if (d->device >= 0) HIP_TRY(d, hipSetDevice(d->device));
  if (d->batch_frames < 0) // submitted with mijpeg_submit_batch_device: wait for it now
    if (const int rc = await_batch(d)) return rc;
  if (d->batch_frames < 1) return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "no decoded batch: call mijpeg_decode_batch_device first");
  const mijpeg_info &f = d->batch_info;
  void *first[MIJPEG_MAX_COMPONENTS] = {dst_device, dst_device, dst_device, dst_device};
  if (planar_check(f, first, row_stride) || plane_stride < row_stride * f.height || frame_stride < plane_stride * f.components)
    return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "planar destination: the strides do not hold a line, a plane or a frame");
  d->planar_stats = mijpeg_planar_stats{};
  std::vector<PlanarItem> items((size_t)d->batch_frames);
  for (int i = 0; i < d->batch_frames; i++) {
    PlanarItem &it = items[(size_t)i];
    it.info = &d->batch_info;
    it.coef_dev = d->coef_dev + (int64_t)i * f.coef_count;
    for (int c = 0; c < f.components; c++) it.planes[c] = (uint8_t *)dst_device + i * frame_stride + c * plane_stride;
    for (int c = f.components; c < MIJPEG_MAX_COMPONENTS; c++) it.planes[c] = nullptr;
    it.row_stride = row_stride;
    if (d->batch_own_tables) {
      it.own_deltas = d->batch_quant_host.data() + (size_t)i * 4 * 64;
      it.own_deltas_dev = d->batch_quant_dev + (size_t)i * 4 * 64;
    }
  }
  RaggedFailures failures;
  const int rc = reconstruct_planar_items(d, items.data(), d->batch_frames, flags & PLANAR_FLAGS, failures);
  if (rc) return set_error(d, rc, rc == MIJPEG_ERR_DEVICE ? "planar reconstruction: a kernel launch failed" : "planar reconstruction not available for this batch");
  d->planar_stats.images = d->batch_frames;
  if (sync) HIP_TRY(d, hipStreamSynchronize(d->stream));
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_reconstruct_batch_planar_device"); }

} // extern "C"
