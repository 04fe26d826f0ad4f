// decoder.hpp -- the decoder object of the C ABI and what its translation units share: capi.cpp (the object, single images),
// batch_decode.cpp (uniform batches, the header pass of a list, the marker route option), rect_service.cpp (rectangles),
// entropy_device.cpp (with entropy_plan.hpp), reconstruct_device.cpp (with reconstruct.hpp), ragged_decode.cpp, ragged_reconstruct.cpp and encode_device.cpp.
// Private to libmijpeg.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <chrono>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../../include/mijpeg.h"
#include "host_decoder.hpp"
#include "request_model.hpp"

// Tables that travel to the device through a pinned copy, once per call, on the object's stream (pinned_upload_reserve / _send /
// _release below): the device buffer, the pinned one, and the event behind the last upload, which frees the pinned copy for the next
struct PinnedUpload {
  uint8_t *dev = nullptr, *host = nullptr;
  size_t dev_cap = 0, host_cap = 0;
  hipEvent_t left = nullptr;
  bool pending = false;
};

struct mijpeg_decoder {
  int device = -1;
  mij::HostDecoder host;
  const uint8_t *data = nullptr;
  size_t size = 0;
  bool parsed = false, decoded = false, uploaded = false;
  bool parse_fresh = false; // host holds a full parse of (data, size) that nothing has touched since: mijpeg_decode_coefficients_device
                            // found the stream not to qualify, the host decode that follows need not parse again
  // coefficient store: pinned when a device is attached
  int16_t *coef_host = nullptr;
  size_t coef_host_cap = 0; // int16 units
  int16_t *coef_dev = nullptr;
  size_t coef_dev_cap = 0;
  // reconstruction cache for the rectangle service (rect_service.cpp)
  uint8_t *img_dev = nullptr;
  size_t img_dev_cap = 0;
  uint8_t *img_host = nullptr; // pinned
  size_t img_host_cap = 0;
  bool img_valid = false;      // img_dev holds the reconstructed frame for img_flags
  bool img_host_valid = false; // ... and img_host its copy (being filled band by band, see band_events)
  // the device-to-host copy of the reconstructed frame travels in bands of lines, one event each: a rectangle request
  // waits for the bands it touches only, so the first stripes of a frame are served while the rest is still on its way
  std::vector<hipEvent_t> band_events;
  int band_lines = 0, bands = 0, bands_waited = 0;
  uint32_t img_flags = 0;
  int img_view = -1;           // component of a non-upsampled reconstruction, -1: the whole picture
  // mijpeg_display_rect: the reference's state between DisplayRectangle calls (request_model.hpp) and the buffers of the
  // requests that do not show the plain picture
  mij::RequestModel model, rmodel; // (rmodel: the residual image of a JPEG XT frame)
  bool model_valid = false;
  uint8_t *req_dev = nullptr, *req_host = nullptr; // frame-sized interleaved image (device; pinned host)
  size_t req_dev_cap = 0, req_host_cap = 0;
  int32_t *rowmap_dev = nullptr;
  size_t rowmap_cap = 0;
  int32_t *ws_dev = nullptr;
  size_t ws_cap = 0; // bytes
  // on-device entropy decoding: stream bytes, interval offsets, tables, status word
  uint8_t *ent_dev = nullptr;
  size_t ent_cap = 0;
  uint8_t *ent_host = nullptr; // pinned staging for offsets + tables + status
  size_t ent_host_cap = 0;
  bool host_planes_stale = false; // coefficients live on the device only
  double phase_prepare = 0, phase_device = 0; // last device entropy decode: host tables / upload + kernel
  mijpeg_decoder *xt_helper = nullptr; // JPEG XT: second context that entropy-decodes the residual codestream concurrently
  // JPEG XT alpha channel: an image of its own (ALFA box), decoded by a decoder object of its own that this one owns
  // (mijpeg_alpha_channel); its codestream is copied here because every parse of the file rebuilds the boxes
  mijpeg_decoder *alpha = nullptr;
  bool alpha_ready = false;
  int alpha_refusal = 0;          // the alpha image reads, its transformer would not build (or this path declines it): the code
  std::string alpha_refusal_msg;
  std::vector<uint8_t> alpha_data;
  uint8_t *enc_dev = nullptr; // encoder direction: pixels + coefficients of one picture
  size_t enc_cap = 0;
  uint8_t *henc_dev[2] = {nullptr, nullptr}, *henc_out_dev[2] = {nullptr, nullptr}; // device entropy coder, two jobs: arrays; streams
  size_t henc_cap[2] = {0, 0}, henc_out_cap[2] = {0, 0};
  uint64_t *henc_host = nullptr; // pinned: byte counts read back from the device, code tables on their way up
  uint8_t *walk_dev = nullptr, *walk_host = nullptr; // state of the device walk over streams without restart markers
  size_t walk_cap = 0, walk_host_cap = 0;
  int walk_rounds = 0;
  uint32_t *walk_status_dev = nullptr;
  hipStream_t copy_stream = nullptr;          // uploads of a batch's streams, ahead of the kernels that decode them
  hipEvent_t ent_free = nullptr;              // behind the last kernel / copy that reads ent_dev
  bool ent_free_valid = false;
  std::vector<hipEvent_t> copy_events;
  uint8_t *stage_host = nullptr;  // pinned gathering area for the streams of a batch
  std::vector<uint8_t> host_stage; // the same for host-only objects (mijpeg_prepare_batch_host)
  size_t stage_cap = 0;
  // batches (mijpeg_decode_batch_device): one parsed decoder per stream, frame 0's info with the batch's worst range
  std::vector<std::unique_ptr<mij::HostDecoder>> batch_hosts;
  mijpeg_info batch_info{};
  int batch_frames = 0;
  // a submitted batch whose device work has not been waited for yet (mijpeg_submit_batch_device)
  int pend_n = 0;
  const uint32_t *pend_status = nullptr;
  int pend_walk_round = 0;                       // > 0: the batch went through the device walk with this many rounds, unchecked
  const uint32_t *pend_walk_flags = nullptr;     // "something changed" per round (pinned)
  const uint32_t *pend_walk_status = nullptr;    // per image (pinned)
  std::chrono::steady_clock::time_point pend_t0;
  // mijpeg_set_device_markers: the restart marker search and the unstuffing of qualifying batches run on the device (markers.hip).
  // markers_retry: the marker route declined inside a synchronous call, which then runs the host route; pend_markers: the
  // result words (flags, term, total, markers per image, pinned) of a submitted batch, markers_want_term the `term` of a good one
  int device_markers = 0;
  int64_t markers_searched = 0, markers_declined = 0; // images
  bool markers_retry = false;
  const uint32_t *pend_markers = nullptr;
  std::vector<uint32_t> markers_want_term;
  std::vector<std::pair<size_t, size_t>> markers_staged; // the last call that took the marker route: slot offset and raw bytes per image
  // batches whose images bring different quantisation tables: [frames][4][64] deltas per component, on the device
  uint16_t *batch_quant_dev = nullptr;
  size_t batch_quant_cap = 0;
  bool batch_own_tables = false;
  std::vector<uint16_t> batch_quant_host;
  // MIJPEG_FLAG_SPECULATIVE: the reconstruction of a submitted batch was launched on an ASSUMED range check (spec_assumed:
  // what the last batch of this shape reported, rounded up to the kernel selection's next gate) behind the Huffman kernel,
  // without the host waiting for what that kernel reports; finish_batch validates and launches again where the assumption
  // did not hold (settle_speculation)
  bool spec_active = false, spec_redone = false;
  void *spec_dst = nullptr;
  int64_t spec_frame_stride = 0, spec_row_stride = 0;
  uint32_t spec_flags = 0;
  int32_t spec_assumed[MIJPEG_MAX_COMPONENTS] = {0, 0, 0, 0};
  int64_t spec_launched = 0, spec_redone_count = 0; // diagnostics (mijpeg_batch_speculation)
  // ragged batches (mijpeg_decode_ragged_device): per image where its coefficients lie, or the decoder object of its own that
  // took it through the single-image route; the launches of the last call
  struct RaggedImage {
    mijpeg_info info{};
    int64_t coef_base = 0;     // int16 index in coef_dev
    int group = -1;            // layout group, -1: single-image route (child) or in error (status)
    int status = 0;
    mijpeg_decoder *child = nullptr;
    std::string why_single;    // why it left (or never entered) the layout groups
  };
  std::vector<RaggedImage> ragged;
  std::vector<mijpeg_decoder *> ragged_children; // kept from call to call
  std::vector<uint8_t> own_input;                // a child's copy of its stream (the caller's bytes are only read during the call)
  int ragged_n = 0;
  mijpeg_ragged_stats ragged_stats{};
  PinnedUpload list_tables; // launch_fused_lists (reconstruct_device.cpp) alone writes these: the tables of a list call's launches (fused_list.hpp)
  // planar calls (reconstruct_planar_items): the interleaved picture of the two-pass route; what the last call did
  uint8_t *planar_tmp_dev = nullptr;
  size_t planar_tmp_cap = 0;
  mijpeg_planar_stats planar_stats{};
  // crop calls (mijpeg_reconstruct_ragged_rect_device and its planar twin, ragged_reconstruct.cpp): the full picture of the copy route
  // (a child's own: its reconstruction runs on the child's stream); what the last call did
  uint8_t *rect_tmp_dev = nullptr;
  size_t rect_tmp_cap = 0;
  mijpeg_ragged_rect_stats rect_stats{};
  // resized call (mijpeg_reconstruct_ragged_resized_device, ragged_reconstruct.cpp): the arena of the crops and the call's tables
  // (resample_taps.hpp; of their own: a crop call inside the resized call fills list_tables while these wait); what the last call did
  uint8_t *resized_arena_dev = nullptr;
  size_t resized_arena_cap = 0;
  PinnedUpload resample_tables;
  mijpeg_ragged_resized_stats resized_stats{};
  mijpeg_ragged_normalized_stats normalized_stats{}; // (the normalised call's sample type and mirrored pictures: set wherever resized_stats is)
  // ragged encode (encode_device.cpp): descriptors, coder arrays and coefficient store of a pass; plain stream and output arena;
  // pinned: descriptors on their way up and counts read back; the downloaded arena
  uint8_t *eragged_dev = nullptr, *eragged_out_dev = nullptr, *eragged_host = nullptr, *eragged_down = nullptr;
  size_t eragged_cap = 0, eragged_out_cap = 0, eragged_host_cap = 0, eragged_down_cap = 0;
  mijpeg_encode_ragged_stats eragged_stats{};
  // planar input (mijpeg_encode_ragged_planar_device16): what the last call did; the interleaved pictures of its two-pass route
  // lie in enc_dev
  mijpeg_encode_planar_stats eplanar_stats{};
  mijpeg_transcode_transform_stats transform_stats{}; // ... and what its transforms did
  mijpeg_transcode_ragged_stats transcode_stats{}; // ragged transcode (encode_device.cpp; its passes use the eragged_ buffers): what the last call did
  double eragged_forward_s = 0; // MIJPEG_ENCODE_RAGGED_TIME_FORWARD: device time of the last ragged encode's forward stages (0: not timed)
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t chain_ev = nullptr; // mijpeg_stream_wait
  hipEvent_t ms_ready = nullptr, ms_done = nullptr; // device_entropy_multiscan (MultiscanRun): the second frame's stream
  hipStream_t ms_stream = nullptr;
  int err_code = 0;
  std::string err_msg;
  double timing[4] = {0, 0, 0, 0};
};

inline int set_error(mijpeg_decoder *d, int code, const std::string &msg)
{
  d->err_code = code;
  d->err_msg = msg;
  return code;
}

inline int hip_fail(mijpeg_decoder *d, hipError_t e, const char *what)
{
  return set_error(d, MIJPEG_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

#define HIP_TRY(d, call)                                  \
  do {                                                    \
    hipError_t e_ = (call);                               \
    if (e_ != hipSuccess) return hip_fail(d, e_, #call);  \
  } while (0)

// everything this object has enqueued is done (before one of its buffers changes hands while the object lives on: rare, a
// buffer only grows when a larger picture arrives)
inline void quiesce(mijpeg_decoder *d)
{
  if (d->device < 0) return;
  if (d->stream) (void)hipStreamSynchronize(d->stream);
  if (d->copy_stream) (void)hipStreamSynchronize(d->copy_stream);
  if (d->ms_stream) (void)hipStreamSynchronize(d->ms_stream);
}

// Device buffers that grow through the buffer cache (capi.cpp): what this object has enqueued finishes before the old buffer goes
int ensure_dev(mijpeg_decoder *d, void **ptr, size_t *cap, size_t bytes);
// ... and the same for either kind the cache keeps: device memory, or (pinned) host memory -- the coefficient store, the frame
int ensure_cached(mijpeg_decoder *d, bool pinned, void **ptr, size_t *cap, size_t bytes);

// capi.cpp: the coefficient store for `count` int16 (device mirror; pinned host planes where need_host); a batch that was submitted
// and not waited for is settled before its staging buffers are rewritten
int ensure_coef_store(mijpeg_decoder *d, size_t count, bool need_host = true);
int settle_pending(mijpeg_decoder *d);

// ---- batch_decode.cpp: uniform batches ----
// a speculative launch (MIJPEG_FLAG_SPECULATIVE) is validated
int settle_speculation(mijpeg_decoder *d);
// The marker route of a call over `images` images (mijpeg_set_device_markers): attempt(true) where the option is on, and
// attempt(false) -- the ordinary route, as if it were off -- where that declines or the option is off
int with_device_markers(mijpeg_decoder *d, int images, const std::function<int(bool)> &attempt);
// The header pass of a list call: d->batch_hosts grows to n parsers (and never shrinks), stream i is parsed by batch_hosts[i] on
// worker i mod min(n, default_threads()), its code goes to rcs[i].  The caller's steps, once per stream on that worker: arm(h, i)
// before the parse (skip-search, the unstuff sink; a code other than 0 is the stream's, and it is not parsed), after(h, i, rc)
// behind it (optional)
using StreamArm = std::function<int(mij::HostDecoder &, int)>;
using StreamAfter = std::function<void(mij::HostDecoder &, int, int)>;
void parse_stream_headers(mijpeg_decoder *d, const uint8_t *const *streams, const size_t *sizes, int n, std::vector<int> &rcs, const StreamArm &arm,
                          const StreamAfter &after = nullptr);
// ... and the first n of those parsers as device_entropy_batch takes them
std::vector<mij::HostDecoder *> batch_host_list(mijpeg_decoder *d, int n);

// ... and ensure_dev's pinned counterpart, for staging buffers that are not handed to the buffer cache
inline int ensure_pinned(mijpeg_decoder *d, uint8_t **ptr, size_t *cap, size_t bytes)
{
  if (*cap >= bytes) return MIJPEG_OK;
  quiesce(d);
  if (*ptr) (void)hipHostFree(*ptr);
  *ptr = nullptr;
  *cap = 0;
  HIP_TRY(d, hipHostMalloc((void **)ptr, bytes, hipHostMallocDefault));
  *cap = bytes;
  return MIJPEG_OK;
}

// `bytes` of u's pinned copy to fill, once the last call's upload has left it (the copy travels asynchronously); grows both buffers
inline int pinned_upload_reserve(mijpeg_decoder *d, PinnedUpload &u, size_t bytes)
{
  if (const int rc = ensure_dev(d, (void **)&u.dev, &u.dev_cap, bytes)) return rc;
  if (u.pending) HIP_TRY(d, hipEventSynchronize(u.left));
  u.pending = false;
  return ensure_pinned(d, &u.host, &u.host_cap, bytes);
}
// ... and on their way: u.host -> u.dev on the object's stream, the event behind it (nothing is waited for)
inline int pinned_upload_send(mijpeg_decoder *d, PinnedUpload &u, size_t bytes)
{
  HIP_TRY(d, hipMemcpyAsync(u.dev, u.host, bytes, hipMemcpyHostToDevice, d->stream));
  if (!u.left) HIP_TRY(d, hipEventCreateWithFlags(&u.left, hipEventDisableTiming));
  HIP_TRY(d, hipEventRecord(u.left, d->stream));
  u.pending = true;
  return MIJPEG_OK;
}
inline void pinned_upload_release(PinnedUpload &u) // (mijpeg_destroy)
{
  if (u.dev) (void)hipFree(u.dev);
  if (u.host) (void)hipHostFree(u.host);
  if (u.left) (void)hipEventDestroy(u.left);
}

// MIJPEG_TRACE_SUBMIT (diagnostics): the host time of the steps of a device decode, since t0, on stderr
struct TraceMarks {
  const char *who;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  static bool on() { static const bool e = getenv("MIJPEG_TRACE_SUBMIT") != nullptr; return e; }
  void operator()(const char *what) const
  {
    if (on()) fprintf(stderr, "[%s] %-28s %8.3f ms\n", who, what, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3);
  }
};

// The boundary of the C ABI (capi.cpp): the handler of every extern "C" function-try-block
int boundary_catch(mijpeg_decoder *d, const char *where) noexcept;

// ---- entropy_device.cpp: on-device entropy decoding ----
// One frame of a file: its decoder, the element type of its planes, where they start in the object's coefficient store.
struct MultiScanFrame {
  mij::HostDecoder *h;
  bool wide;        // int32 coefficients (JPEG XT residual frames with hidden bits)
  int64_t base16;   // offset of the frame's planes in coef_dev, in int16 units
};

// Images of different sizes in one launch of device_entropy_batch (they share components and sampling factors)
struct RaggedEntropy {
  const int64_t *coef_base; // per image: int16 index of its coefficient store in coef_dev
  int *verdict;             // out, per image: 0 decoded (info carries its range check), 1 damaged: the single-image route decides,
                            // 2 (the marker route) the device's search of its segment is not good: the same
  int *entropy_launches, *walk_launches; // counted up per launch of huffman_scan_kernel / huffman_walk_kernel (rounds and emitting pass)
};

// plain12: plain 12-bit frames (SOF1, P = 12) pass as well -- mijpeg_decode_ragged_device16 alone asks with it
const char *device_entropy_obstacle(const mij::HostDecoder &h, size_t size, bool xt_part = false, bool plain12 = false);
const char *ragged_entropy_obstacle(const mij::HostDecoder &h, size_t size, bool plain12 = false);
const char *multiscan_obstacle(const mij::HostDecoder &h, bool xt_part, bool residual_frame);
size_t stream_slots(const size_t *sizes, int n, std::vector<size_t> &stream_off);
// How device_entropy_batch is asked to work: a caller names what it sets
struct EntropyBatchOptions {
  bool xt_part = false;                  // the stream is one of the two codestreams of a JPEG XT file
  bool defer = false;                    // enqueue only: mijpeg_finish_batch_device waits and looks at the status words
  bool markers = false;                  // the marker route: the streams were parsed without a marker search, the device searches them
                                         // (a ragged launch: those of its members whose Scan::search_skipped says so, the others as always)
  const RaggedEntropy *ragged = nullptr; // images of different sizes
  bool plain12 = false;                  // ... which may be plain 12-bit frames (all of a launch or none: one precision per launch)
};
int device_entropy_batch(mijpeg_decoder *d, mij::HostDecoder *const *hosts, const uint8_t *const *datas, const size_t *sizes, int n,
                         int min_intervals, int16_t *coef_dev, int64_t frame_stride, const EntropyBatchOptions &opt);
// the marker route: why a stream parsed with HostDecoder::set_skip_search stays on the host route (nullptr: it qualifies; ragged: as
// a member of a ragged launch, where a stream without restart markers that is too small for a walk is one interval); what
// the result words of n images say (true: every search is good)
const char *device_markers_obstacle(const mij::HostDecoder &h, size_t size, bool ragged = false);
bool device_markers_good(const uint32_t *results, const uint32_t *want_term, int n);
// mijpeg_device_marker_search's body (include/mijpeg.h)
int64_t device_marker_search(mijpeg_decoder *d, const uint8_t *segment, size_t size, int32_t expect, uint8_t *dst, size_t capacity,
                             uint32_t *begin, uint32_t *end, uint32_t *term, uint32_t *flags);
int device_entropy_multiscan(mijpeg_decoder *d, const MultiScanFrame *frames, int nframes, int min_intervals);
int evaluate_entropy_status(mijpeg_decoder *d, mij::HostDecoder *const *hosts, int n, const uint32_t *status_host);
int walk_rounds_needed(const uint32_t *changed, int rounds);
int walk_verdict(mijpeg_decoder *d, const uint32_t *walk_status, int n);
