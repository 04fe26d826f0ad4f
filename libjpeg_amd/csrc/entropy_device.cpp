// entropy_device.cpp -- entropy decoding on the device: which streams qualify, the upload of their entropy coded data and
// tables, the launches of the Huffman kernels (huffman.hip) and what their status words say.  Host code only, compiled with
// hipcc like capi.cpp, whose extern "C" bodies call it.  What needs no device -- the helpers the paths share, plan and staging of
// the multiscan and walk paths -- is entropy_plan.hpp.
#include <string.h>

#include <algorithm>

#include "decoder.hpp"
#include "entropy_plan.hpp"
#include "huffman_dev.hpp"
#include "kernels.hpp"
#include "markers.hpp"

using namespace mij;

// ------------------------------------------------------------------------------------------------
// on-device entropy decoding
// ------------------------------------------------------------------------------------------------
// What keeps a parsed stream from every device path, sequential or not: damage, a JPEG XT stream that is not decoded as one of its
// file's two codestreams, a missing EOI, a verdict that is the host decoder's.  `sequential_only`: progressive frames as well
// (asked where the sequential path always asked it: behind the damage).
static const char *stream_obstacle(const HostDecoder &h, bool xt_part, bool sequential_only)
{
  const mijpeg_info &f = h.info;
  if (h.needs_sequential())
    return "on-device entropy decoding: the stream is damaged; the host decoder walks it with the reference's resynchronisation (entropyparser.cpp:117-201)";
  if (sequential_only && f.progressive) return "on-device entropy decoding: progressive frames are decoded on the host";
  if (f.xt && !xt_part) return "on-device entropy decoding: not for this JPEG XT stream";
  if (!h.residual_merged()) return "on-device entropy decoding: the legacy codestream has no EOI marker (the host decoder decides what is merged)";
  // (a RESI box without a merging specification, a residual codestream header that does not match, tables looked up at the first
  // request: what the reference reports behind the legacy frame's decode -- HostDecoder::decode reports it, this path would not)
  if (h.verdict_pending()) return "on-device entropy decoding: the file's verdict is the host decoder's (residual codestream header / tables looked up at the first request)";
  return nullptr;
}

static const char *sampling_obstacle(const mijpeg_info &f)
{
  for (int c = 0; c < f.components; c++)
    if (f.hsamp[c] > 4 || f.vsamp[c] > 4) return "on-device entropy decoding: MCUs of more than 4 x 4 blocks of a component are decoded on the host";
  return nullptr;
}

// Why a parsed stream cannot be entropy-decoded on the device (nullptr: it can).  `xt_part`: the stream is one of the
// two codestreams of a JPEG XT profile C file (8-bit legacy or 12-bit residual frame without hidden refinement scans).
const char *device_entropy_obstacle(const HostDecoder &h, size_t size, bool xt_part, bool plain12)
{
  const mijpeg_info &f = h.info;
  // one Huffman sequential scan over all components (or a single-component frame)
  if (const char *why = stream_obstacle(h, xt_part, true)) return why;
  // (plain12: the ragged call with 12-bit groups.  The kernel is the one that decodes the residual frames: DC categories to 15,
  // AC categories to 15 into the int16 store, code + value bits <= 31, a DC prediction beyond int16 is HUFF_ERR_OVERFLOW.)
  if (f.precision != 8 && !((xt_part || plain12) && f.precision == 12)) return "on-device entropy decoding: 8-bit frames (12-bit residual frames of JPEG XT) only";
  if (h.scans.size() != 1 || h.hidden_bits()) return "on-device entropy decoding: the frame has more than one scan";
  const Scan &s = h.scans[0];
  if (s.ncomp != f.components) return "on-device entropy decoding: the scan does not cover all components";
  if (size > 0xfffffff0ull) return "on-device entropy decoding: stream too long";
  return sampling_obstacle(f);
}

// Why the restart markers of scan `si` of a parsed stream keep it from the device (nullptr: they do not, or it has none): the
// intervals the kernel decodes side by side must all be there, in sequence.
static const char *restart_markers_obstacle(const HostDecoder &h, size_t si)
{
  static const char MISSING[] = "restart markers missing: the host decoder resynchronises like the reference (entropyparser.cpp:117-201)";
  const Scan &s = h.scans[si];
  if (s.restart_interval <= 0) return nullptr;
  const int64_t total_mcus = (int64_t)s.mcus_x * s.mcus_y;
  const int64_t nint = (total_mcus + s.restart_interval - 1) / s.restart_interval;
  if (nint > 0x7fffffff) return "too many restart intervals";
  if ((int64_t)s.interval_begin.size() < nint) return MISSING;
  const std::vector<uint8_t> &rst = h.restart_codes(si);
  if ((int64_t)rst.size() + 1 < nint) return MISSING;
  for (int64_t k = 0; k + 1 < nint; k++)
    if (rst[(size_t)k] != 0xd0 + (k & 7))
      return "restart markers out of sequence: the host decoder resynchronises like the reference (entropyparser.cpp:117-201)";
  return nullptr;
}

// ... and the device's copy of its entropy coded data (no byte stuffing, no markers): inside the kernels' bit addresses, no
// larger than the stream it came from.  *code: what the refusal is (a copy larger than its stream is the caller's mistake).
static const char *stream_copy_obstacle(const HostDecoder &h, size_t size, int *code)
{
  const size_t usize = h.scans[0].unstuffed_size;
  *code = MIJPEG_ERR_NOT_AVAILABLE;
  if (usize >= ((size_t)1 << 28)) return "entropy coded segment too large for the device decoder's bit addresses";
  if (usize > size) { *code = MIJPEG_ERR_INVALID_PARAMETER; return "entropy coded segment larger than its stream"; }
  return nullptr;
}

// Everything device_entropy_batch would refuse ONE parsed stream for, whatever its neighbours in the launch are (the same
// checks, asked stream by stream before the groups are formed): what mijpeg_decode_ragged_device sends to the single-image
// route, so that only the odd member leaves its layout group.  The scan must list the components in frame order -- a launch
// shares the order, and this is the one every group can share.
const char *ragged_entropy_obstacle(const HostDecoder &h, size_t size, bool plain12)
{
  int code;
  if (const char *why = device_entropy_obstacle(h, size, false, plain12)) return why;
  const Scan &s = h.scans[0];
  if (s.search_skipped) { // (the marker route: the device searches the segment, and the launch's verdict says what it found)
    if (const char *why = device_markers_obstacle(h, size, true)) return why;
  } else {
    if (const char *why = restart_markers_obstacle(h, 0)) return why;
    if (const char *why = stream_copy_obstacle(h, size, &code)) return why;
    if (s.restart_interval > 0 && s.interval_ubegin.size() < s.interval_begin.size()) return "restart intervals missing";
  }
  for (int k = 0; k < s.ncomp; k++)
    if (s.sc[k].comp != k) return "the scan lists its components out of frame order";
  return nullptr;
}

// The marker route (mijpeg_set_device_markers, markers.hip): what keeps one stream, parsed with HostDecoder::set_skip_search, on the
// host route.  What the parse itself asks for -- a plain 8-bit Huffman sequential frame, one scan over all components, FF D9 as
// the last two bytes -- shows in Scan::search_skipped.  A stream without restart markers is searched with one expected interval
// and then walked on the device (huffman_walk_kernel), so it must be large enough for a walk, and the walk must not be switched
// off (MIJPEG_DEVICE_WALK=0: the host plans the restart points, which needs the host's search).
static bool too_small_for_a_walk(const Scan &s) { return (int64_t)s.mcus_x * s.mcus_y < 256 || s.ecs_end - s.ecs_begin < 4096; }
static bool device_walk_enabled() { return !(getenv("MIJPEG_DEVICE_WALK") && atoi(getenv("MIJPEG_DEVICE_WALK")) == 0); }
static const char TOO_SMALL_FOR_A_WALK[] = "stream without restart markers is too small for speculative decoding";

const char *device_markers_obstacle(const HostDecoder &h, size_t size, bool ragged)
{
  if (const char *why = device_entropy_obstacle(h, size, false)) return why;
  const Scan &s = h.scans[0];
  if (!s.search_skipped) return "device marker search: not a plain 8-bit sequential stream that ends in EOI";
  if (h.info.xt || h.is_xt() || h.info.dnl || h.info.precision != 8) return "device marker search: plain 8-bit frames only";
  if (size < s.ecs_begin + 2) return "device marker search: no room for the closing EOI";
  if (size - s.ecs_begin >= MARKERS_MAX_SEGMENT) return "entropy coded segment too large for the device decoder's bit addresses";
  const int64_t total_mcus = (int64_t)s.mcus_x * s.mcus_y;
  if (s.restart_interval <= 0) {
    if (too_small_for_a_walk(s)) return ragged ? nullptr : TOO_SMALL_FOR_A_WALK; // (a ragged launch decodes it as one interval)
    if (!device_walk_enabled()) return "device marker search: streams without restart markers need the device walk";
    return nullptr;
  }
  if ((total_mcus + s.restart_interval - 1) / s.restart_interval > 0x7fffffff) return "too many restart intervals";
  return nullptr;
}

// Good: no flag, and the segment ends at the FF of the EOI the stream closes with
bool device_markers_good(const uint32_t *results, const uint32_t *want_term, int n)
{
  for (int i = 0; i < n; i++) {
    const MarkerResult &r = ((const MarkerResult *)results)[i];
    if (r.flags != 0 || r.term != want_term[i]) return false;
  }
  return true;
}

namespace { // steps the sequential, progressive and walk paths share

const char DC_OVERFLOW[] = "on-device entropy decoding: a DC coefficient leaves the 16 bit coefficient store (damaged stream); the host decoder keeps 32-bit coefficients for it";

// The buffer of one device decode: on the device [streams][tables, intervals ...][status words][what only the device keeps:
// `device_extra` bytes]; in pinned staging (ent_host) everything behind the streams up to the status words, at the same offsets
// less stream_bytes.  The staging part goes up in one copy, and the status words come back into its end.
int ensure_entropy_buffers(mijpeg_decoder *d, size_t stream_bytes, size_t tail_bytes, size_t device_extra = 0)
{
  const int rc = ensure_dev(d, (void **)&d->ent_dev, &d->ent_cap, stream_bytes + tail_bytes + device_extra);
  return rc ? rc : ensure_pinned(d, &d->ent_host, &d->ent_host_cap, tail_bytes);
}

// One image of a marker search in staging: its descriptor, its chunks (at chunks[im.first_chunk]) and a fresh result
void stage_marker_image(MarkerImage &im, MarkerChunk *chunks, MarkerResult &res, uint32_t image, const MarkerImage &desc)
{
  im = desc;
  im.n_chunks = markers_chunks(im.size);
  for (uint32_t k = 0; k < im.n_chunks; k++) chunks[im.first_chunk + k] = MarkerChunk{image, k};
  res.flags = 0;
  res.term = im.size;
  res.total = res.markers = 0;
}

// The argument block of a search over device memory (chunk0 / n_chunks: the caller's launch)
MarkerArgs marker_args(const uint8_t *raw, uint8_t *dst, uint32_t *ibegin, uint32_t *iend, const MarkerImage *images, const MarkerChunk *chunks,
                       MarkerResult *results, uint8_t *scratch, const MarkerScratch &ms)
{
  MarkerArgs a;
  memset(&a, 0, sizeof(a));
  a.raw = raw;
  a.dst = dst;
  a.ibegin = ibegin;
  a.iend = iend;
  a.images = images;
  a.chunks = chunks;
  a.kept = (uint32_t *)(scratch + ms.kept);
  a.marks = (uint32_t *)(scratch + ms.marks);
  a.kept_at = (const uint64_t *)(scratch + ms.kept_at);
  a.marks_at = (const uint64_t *)(scratch + ms.marks_at);
  a.results = results;
  return a;
}

// The unstuffing gather: the device's copy of scans' entropy coded data (no byte stuffing, no markers: HostDecoder::unstuff_piece)
// written into pinned staging by the pool, in pieces of ~256 KiB of source.
struct Gather {
  struct Job { const HostDecoder *h; size_t scan; HostDecoder::UnstuffPiece piece; uint8_t *dst; };
  std::vector<Job> jobs;
  std::vector<HostDecoder::UnstuffPiece> pieces;
  void add(const HostDecoder *h, size_t scan, uint8_t *dst)
  {
    pieces.clear();
    h->unstuff_pieces(scan, (size_t)256 << 10, pieces);
    for (const auto &p : pieces) jobs.push_back(Job{h, scan, p, dst});
  }
  void run()
  {
    if (jobs.empty()) return;
    // (the sweep runs at about half of memcpy's rate: twice the workers the plain copy had)
    const int workers = std::max(1, std::min<int>((int)jobs.size(), std::min(default_threads(), 32)));
    parallel_for(workers, [&](int w) {
      for (size_t k = (size_t)w; k < jobs.size(); k += (size_t)workers) jobs[k].h->unstuff_piece(jobs[k].scan, jobs[k].piece, jobs[k].dst);
    });
    jobs.clear();
  }
};

// The copy stream, with at least `events` events for its uploads.  It must not overtake work that still reads the entropy
// buffer from an earlier call: the Huffman kernels and the status copy of the previous decode (ent_free, recorded behind them).
// NOT everything on d->stream: the reconstruction kernel of a previous batch does not touch this buffer, and an upload that
// waits for it leaves the link idle for the length of that kernel in every round of a pipeline (profiles/r03/batch4k_timeline.txt)
int prepare_copy_stream(mijpeg_decoder *d, size_t events)
{
  if (!d->copy_stream) HIP_TRY(d, hipStreamCreateWithFlags(&d->copy_stream, hipStreamNonBlocking));
  while (d->copy_events.size() < events) {
    hipEvent_t e = nullptr;
    HIP_TRY(d, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    d->copy_events.push_back(e);
  }
  if (d->ent_free_valid) HIP_TRY(d, hipStreamWaitEvent(d->copy_stream, d->ent_free, 0));
  return MIJPEG_OK;
}

// The status words back into pinned staging, and ent_free behind them: from there on nothing enqueued so far reads the entropy buffer
int read_back_status(mijpeg_decoder *d, uint32_t *status_host, const uint8_t *status_dev, size_t bytes)
{
  HIP_TRY(d, hipMemcpyAsync(status_host, status_dev, bytes, hipMemcpyDeviceToHost, d->stream));
  if (!d->ent_free) HIP_TRY(d, hipEventCreateWithFlags(&d->ent_free, hipEventDisableTiming));
  HIP_TRY(d, hipEventRecord(d->ent_free, d->stream));
  d->ent_free_valid = true;
  return MIJPEG_OK;
}

// Once a device decode has put work on its streams, an exit with an error code or an exception waits for all of it: the caller
// goes on to the host decoder, which reuses the staging buffers and coef_dev.  Success disarms the guard (a deferred batch is
// waited for by finish_batch).
struct QuiesceOnError {
  mijpeg_decoder *d;
  bool armed = false;
  ~QuiesceOnError() { if (armed) quiesce(d); }
};

// Where the restart intervals of one image of a launch come from: what device_entropy_batch's stages switch on
enum class IntervalSource {
  RestartMarkers, // found by the host's marker search (Scan::interval_ubegin / interval_uend)
  HostWalk,       // no markers: the host's self-synchronising walk plans exact restart points (MIJPEG_DEVICE_WALK=0)
  DeviceWalk,     // no markers: huffman_walk_kernel finds them in front of the decode; their number is known already
  WholeScan,      // no markers, a small member of a ragged launch: ONE interval, one lane -- every MCU in sequence, as a host thread would
  MarkerSearch,   // the raw segment goes up; the search kernels (markers.hip) write the copy and the interval tables
  SearchedWalk,   // no markers, the raw segment goes up: searched with ONE expected interval, fitted (marker_fit_kernel), then walked like DeviceWalk
  SearchedWhole,  // WholeScan whose raw segment goes up: searched with one expected interval, which writes its copy and the end of its one interval
};

struct ImagePlan {
  IntervalSource source = IntervalSource::RestartMarkers;
  int64_t n_intervals = 0, first_interval = 0; // its entries in the launch's interval tables
  int mcus_per_interval = 0;                   // the restart interval, or MCUs per virtual interval
  size_t copy_bytes = 0; // the device's copy of its entropy coded data (MarkerSearch: the raw segment, terminator included -- the copy is no longer)
  size_t slot_off = 0;   // its slot in the stream buffer (stream_slots)
  std::unique_ptr<VirtualIntervals> walked; // HostWalk: the restart points
  bool device_walked() const { return source == IntervalSource::DeviceWalk || source == IntervalSource::SearchedWalk; }
  bool searched() const { return source == IntervalSource::MarkerSearch || source == IntervalSource::SearchedWalk || source == IntervalSource::SearchedWhole; }
  bool virtual_intervals() const { return source == IntervalSource::HostWalk || device_walked(); }
};

struct BatchPlan {
  std::vector<ImagePlan> images;
  int64_t total_intervals = 0, n_groups = 0;
  int lanes = 0, per_group = 0; // decoding lanes per wave; intervals of one workgroup
  size_t stream_bytes = 0;      // all slots
  uint32_t marker_chunks = 0;
  bool any_virtual = false; // some image has virtual intervals: the launch carries bit skips and DC predictors per interval
  bool any_dwalk = false;   // ... found by the device walk
  bool needs_clear = false; // some scan leaves blocks of its planes unwritten: the planes are cleared first
  int n() const { return (int)images.size(); }
  int64_t groups_of(int i) const { return (images[(size_t)i].n_intervals + per_group - 1) / per_group; }
  size_t slot_end(int i) const { return i + 1 < n() ? images[(size_t)i + 1].slot_off : stream_bytes; }
};

} // namespace

// Where the device's copy of image i's entropy coded data goes inside the launch's stream buffer (and inside the pinned
// gathering area): a slot of the stream's own size -- known before the stream is parsed, so a batch's workers can write the
// copy while they search it for markers -- rounded to 16 bytes, plus the pad the kernels' prefetch may run into.
size_t stream_slots(const size_t *sizes, int n, std::vector<size_t> &stream_off)
{
  stream_off.resize((size_t)n);
  Layout slots;
  for (int i = 0; i < n; i++) stream_off[(size_t)i] = slots.take(sizes[i] + HUFF_STREAM_PAD);
  return slots.end;
}

// "Something changed" flags of walk rounds 1..rounds: the rounds that were needed -- the last one that changed something, and
// one to see it
int walk_rounds_needed(const uint32_t *changed, int rounds)
{
  int needed = 1;
  for (int r = 1; r <= rounds; r++)
    if (changed[r]) needed = r + 1;
  return needed;
}

// What the walk's status words of n images say about the restart points it settled on
int walk_verdict(mijpeg_decoder *d, const uint32_t *walk_status, int n)
{
  for (int i = 0; i < n; i++) {
    if (walk_status[i] & 2) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, DC_OVERFLOW);
    if (walk_status[i]) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "speculative decoding settled on something that is not a decode of the image");
  }
  return MIJPEG_OK;
}

// Streams without restart markers: find their virtual restart intervals on the device.  Rounds of huffman_walk_kernel
// until the hand-over states between neighbouring subsequences stop changing, prefix sums over the subsequences
// (block numbers, DC predictors: huffman_walk_scan_kernel), and one EMIT walk that writes the interval tables the
// decode kernel reads.  The host only looks at the per-round "something changed" flags.
// The images of `plan` whose source is the device walk are walked; `scan` is the argument block of the decode that follows (its
// data, images and tables are the walk's), `intervals` the tables the EMIT walk writes.
// Images whose source is SearchedWalk (the marker route, `search` its argument block): everything here is sized from the raw
// segment, an upper bound of the copy the search writes, and the fit step (launch_marker_fit) puts what the search found --
// the copy's size, the subsequences it really has, the end of every virtual interval -- where the walk kernels read it.
// Plan and staging are entropy_plan.hpp's (plan_walk, fill_walk); the stages here bring the plan to the device.
struct DeviceIntervals { uint32_t *ibegin, *iend; uint8_t *iskip; int16_t *ipred; };

namespace {

// What the walk's plan reads of the images of a launch
std::vector<WalkImage> walk_images(HostDecoder *const *hosts, const BatchPlan &plan)
{
  std::vector<WalkImage> images((size_t)plan.n());
  for (int i = 0; i < plan.n(); i++) {
    const ImagePlan &p = plan.images[(size_t)i];
    const Scan &s = hosts[i]->scans[0];
    images[(size_t)i] = WalkImage{p.device_walked(), p.source == IntervalSource::SearchedWalk, p.mcus_per_interval, p.copy_bytes,
                                  p.first_interval, p.n_intervals, (int64_t)s.mcus_x * s.mcus_y};
  }
  return images;
}

// device_walk_images' stages: the plan's buffer on the device (walk_dev) and what the host fills of it in pinned staging
// (walk_host), the argument block of the walk kernels, everything enqueued on the object's stream
struct WalkRun {
  mijpeg_decoder *d;
  const WalkPlan &p;
  int *walk_launches; // (a ragged launch counts them)
  HuffWalkArgs w;

  uint32_t *flags_host() const { return (uint32_t *)(d->walk_host + p.o_up_end); }

  // pinned: what the host fills, then room for the flags (and the status words, read back to the start)
  int ensure()
  {
    const int rc = ensure_dev(d, (void **)&d->walk_dev, &d->walk_cap, p.end);
    return rc ? rc : ensure_pinned(d, &d->walk_host, &d->walk_host_cap, p.o_up_end + p.flags_bytes());
  }

  int upload_and_clear()
  {
    HIP_TRY(d, hipMemcpyAsync(d->walk_dev, d->walk_host, p.o_up_end, hipMemcpyHostToDevice, d->stream));
    HIP_TRY(d, hipMemsetAsync(d->walk_dev + p.o_flags, 0, p.o_zero_end - p.o_flags, d->stream));
    return MIJPEG_OK;
  }

  // (behind the search on this stream, behind the upload and the cleared status words, in front of the first round)
  int fit_step(const MarkerArgs &search, const DeviceIntervals &intervals)
  {
    uint8_t *const wd = d->walk_dev;
    MarkerFitArgs fit;
    memset(&fit, 0, sizeof(fit));
    fit.images = search.images;
    fit.results = search.results;
    fit.fit_intervals = (const uint32_t *)(wd + p.o_fit);
    fit.img_e1 = (uint32_t *)(wd + p.o_e1);
    fit.img_nsub = (uint32_t *)(wd + p.o_insub);
    fit.walk_status = (uint32_t *)(wd + p.o_flags) + WALK_MAX_ROUNDS + 1;
    fit.iend = intervals.iend;
    fit.sub_bytes = p.sub_bytes;
    fit.n_images = (uint32_t)p.n;
    if (launch_marker_fit(fit, d->stream)) return hip_fail(d, hipGetLastError(), "marker_fit_kernel launch");
    return MIJPEG_OK;
  }

  // `scan`: the argument block of the decode that follows (its data, images, tables and MCU are the walk's)
  void arguments(const HuffScanArgs &scan, const DeviceIntervals &intervals, const WalkImage *images)
  {
    uint8_t *const wd = d->walk_dev;
    memset(&w, 0, sizeof(w));
    w.ncomp = scan.ncomp;
    for (int k = 0; k < scan.ncomp; k++) {
      w.hs[k] = scan.hs[k];
      w.vs[k] = scan.vs[k];
    }
    w.nblk_mcu = p.nblk_mcu;
    w.ntables = scan.ntables;
    w.sub_bytes = p.sub_bytes;
    w.lanes = p.lanes;
    w.waves_per_group = WAVES_PER_GROUP;
    w.n_groups = (int32_t)p.sub_image.size();
    w.data = scan.data;
    w.images = scan.images;
    w.tables = scan.tables;
    w.sub_image = (const uint32_t *)(wd + p.o_simg);
    w.sub_first = (const uint32_t *)(wd + p.o_sfirst);
    w.img_sub0 = (const uint32_t *)(wd + p.o_isub0);
    w.img_nsub = (const uint32_t *)(wd + p.o_insub);
    w.img_e0 = (const uint32_t *)(wd + p.o_e0);
    w.img_e1 = (const uint32_t *)(wd + p.o_e1);
    w.img_int0 = (const uint32_t *)(wd + p.o_int0);
    w.state = (uint64_t *)(wd + p.o_state);
    w.stamp = (uint32_t *)(wd + p.o_stamp);
    w.changed = (uint32_t *)(wd + p.o_flags);
    w.walk_status = w.changed + WALK_MAX_ROUNDS + 1;
    w.nblocks = (uint32_t *)(wd + p.o_nblk);
    w.dcsum = (int32_t *)(wd + p.o_dcsum);
    w.first_block = (uint32_t *)(wd + p.o_fblk);
    w.first_pred = (int32_t *)(wd + p.o_fpred);
    w.tile_sums = (WalkSums *)(wd + p.o_tiles);
    w.tiles_per_image = p.tiles;
    w.ibegin = intervals.ibegin;
    w.iskip = intervals.iskip;
    w.ipred = intervals.ipred;
    if (p.per_image) {
      w.img_emit_every = (const uint32_t *)(wd + p.o_every);
      w.img_total_blocks = (const uint32_t *)(wd + p.o_blocks);
    } else {
      // one interval size and one block count for the launch: the images share their geometry, hence their MCUs per virtual interval
      int per = 0;
      for (int i = 0; i < p.n; i++)
        if (images[i].device_walked) per = images[i].mcus_per_interval;
      w.emit_every = (uint32_t)(per * p.nblk_mcu);
      w.total_blocks = (uint32_t)(images[0].total_mcus * p.nblk_mcu);
    }
  }

  int read_flags()
  {
    HIP_TRY(d, hipMemcpyAsync(flags_host(), d->walk_dev + p.o_flags, (size_t)(WALK_MAX_ROUNDS + 1) * 4, hipMemcpyDeviceToHost, d->stream));
    return MIJPEG_OK;
  }

  // mijpeg_submit_batch_device: nobody looks at the flags between the rounds.  Enough rounds for the states to settle are
  // launched in one go -- a round in which no lane is dirty costs a few microseconds (its workgroups leave before they
  // load their tables) -- and whoever waits for the batch checks that the last one changed nothing (finish_batch).
  int rounds_in_one_go()
  {
    int round = 0;
    while (round < p.defer_rounds) {
      w.round = (uint32_t)++round;
      if (launch_huffman_walk(w, false, d->stream)) return hip_fail(d, hipGetLastError(), "huffman_walk_kernel launch");
    }
    if (const int rc = read_flags()) return rc;
    d->pend_walk_round = round;
    d->pend_walk_flags = flags_host();
    d->walk_rounds = 1;
    return MIJPEG_OK;
  }

  // rounds, launched back to back in bunches; between bunches the host looks at the flags: a round that changed no
  // hand-over state means the states are the fixed point (and the counts of the lanes' last walks belong to it)
  int rounds_until_settled()
  {
    constexpr int FIRST_BUNCH = 8;
    int round = 0;
    for (;;) {
      const int upto = round == 0 ? FIRST_BUNCH : std::min(WALK_MAX_ROUNDS, round + 4);
      while (round < upto) {
        w.round = (uint32_t)++round;
        if (launch_huffman_walk(w, false, d->stream)) return hip_fail(d, hipGetLastError(), "huffman_walk_kernel launch");
        if (walk_launches) ++*walk_launches;
      }
      if (const int rc = read_flags()) return rc;
      HIP_TRY(d, hipStreamSynchronize(d->stream));
      if (!flags_host()[round]) break;
      if (round == WALK_MAX_ROUNDS) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "speculative decoding did not settle");
    }
    d->walk_rounds = walk_rounds_needed(flags_host(), round);
    return MIJPEG_OK;
  }

  // prefix sums over the subsequences, and the EMIT walk that writes the interval tables
  int sums_and_emit()
  {
    if (launch_huffman_walk_scan(w, p.n, d->stream)) return hip_fail(d, hipGetLastError(), "huffman_walk_scan_kernel launch");
    if (launch_huffman_walk(w, true, d->stream)) return hip_fail(d, hipGetLastError(), "huffman_walk_kernel launch");
    if (walk_launches) ++*walk_launches;
    d->walk_status_dev = w.walk_status;
    return MIJPEG_OK;
  }
};

} // namespace

static int device_walk_images(mijpeg_decoder *d, HostDecoder *const *hosts, const BatchPlan &plan, const EntropyBatchOptions &opt, const HuffScanArgs &scan,
                              const DeviceIntervals &intervals, const MarkerArgs &search)
{
  // (the MCU of the decode that follows -- scan_args filled hs / vs with mcu_blocks of hosts[0]'s scan, and the walk must step through
  // the same blocks: it reads them there instead of deriving them a second time)
  int nblk_mcu = 0;
  for (int k = 0; k < scan.ncomp; k++) nblk_mcu += scan.hs[k] * scan.vs[k];
  const std::vector<WalkImage> images = walk_images(hosts, plan);
  WalkPlan wp;
  if (const char *why = plan_walk(images.data(), plan.n(), opt.ragged != nullptr, nblk_mcu, wp)) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, why);
  WalkRun run{d, wp, opt.ragged ? opt.ragged->walk_launches : nullptr, HuffWalkArgs()};
  int rc;
  if ((rc = run.ensure())) return rc;
  fill_walk(wp, images.data(), d->walk_host);
  if ((rc = run.upload_and_clear())) return rc;
  if (wp.any_fit && (rc = run.fit_step(search, intervals))) return rc;
  run.arguments(scan, intervals, images.data());
  if ((rc = opt.defer ? run.rounds_in_one_go() : run.rounds_until_settled())) return rc;
  return run.sums_and_emit();
}

// What the Huffman kernel left in the status words of n images: errors, and per image the range check that selects the
// arithmetic flavour of the reconstruction (fast_arith / range_max).
int evaluate_entropy_status(mijpeg_decoder *d, HostDecoder *const *hosts, int n, const uint32_t *status_host)
{
  for (int i = 0; i < n; i++) {
    const uint32_t *st = status_host + 8 * i;
    // A DC prediction that leaves the 16-bit store (only damaged streams get there): the host decoder keeps 32-bit planes
    if (st[0] == HUFF_ERR_OVERFLOW) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, DC_OVERFLOW);
    // Damaged entropy coded data: which error the reference reports (or whether it decodes on after a resynchronisation)
    // depends on its sequential walk; the host decoder restates that walk, the device decoder does not try to
    if (st[0]) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "the entropy coded data is damaged: the host decoder walks such streams like the reference does (DESIGN 4.0)");
    mijpeg_info &f = hosts[i]->info;
    f.fast_arith = 1;
    for (int c = 0; c < f.components; c++) {
      f.range_max[c] = (int32_t)std::min<uint32_t>(st[1 + c], 0x7fffffffu);
      if (f.range_max[c] >= 16384) f.fast_arith = 0;
    }
    if (f.precision != 8) f.fast_arith = 0; // (as HostDecoder::decode has it: the fast flavour is derived for 8-bit frames; 12-bit kernels gate on range_max)
  }
  return MIJPEG_OK;
}

// ------------------------------------------------------------------------------------------------
// device_entropy_batch and its stages: qualify and count, table slots, layout, fill staging, kernel arguments, enqueue, read back
// and verdict
// ------------------------------------------------------------------------------------------------
namespace {

// Qualify and count: what keeps image i from the device, what the images of a launch must share, where each image's intervals come
// from and how many they are, the `min_intervals` gate; then the device copies and their slots.  Nothing has been touched when this
// refuses.
int plan_batch(mijpeg_decoder *d, HostDecoder *const *hosts, const size_t *sizes, int n, int min_intervals, const EntropyBatchOptions &opt, BatchPlan &plan)
{
  const bool ragged = opt.ragged != nullptr;
  const mijpeg_info &f0 = hosts[0]->info;
  const Scan &s0 = hosts[0]->scans[0];
  plan.images.resize((size_t)n);
  d->walk_rounds = 0;
  const bool device_walk = device_walk_enabled();
  for (int i = 0; i < n; i++) {
    // the marker route: every image of a uniform call; of a ragged launch the members whose parse left the search to the device
    const bool searched = opt.markers && (!ragged || (!hosts[i]->scans.empty() && hosts[i]->scans[0].search_skipped));
    const char *why = searched ? device_markers_obstacle(*hosts[i], sizes[i], ragged) : device_entropy_obstacle(*hosts[i], sizes[i], opt.xt_part, ragged && opt.plain12);
    if (why) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, why);
    const mijpeg_info &f = hosts[i]->info;
    const Scan &s = hosts[i]->scans[0];
    if (((f.width != f0.width || f.height != f0.height) && !ragged) || f.components != f0.components || memcmp(f.hsamp, f0.hsamp, sizeof(f.hsamp)) ||
        memcmp(f.vsamp, f0.vsamp, sizeof(f.vsamp)))
      return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "the images of a batch must share width, height and sampling factors");
    // ... and what the one reconstruction launch applies to all of them: the colour transformation (an Adobe marker may
    // switch it off per image), the sample precision, being a JPEG XT stream or not
    // (a ragged launch is followed by reconstruction launches that look at every image's own colour transformation)
    if ((f.ycbcr != f0.ycbcr && !ragged) || f.precision != f0.precision || f.xt != f0.xt)
      return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "the images of a batch must share colour transformation and precision");
    for (int k = 0; k < s.ncomp; k++)
      if (s.sc[k].comp != s0.sc[k].comp) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "the images of a batch must share the component order of their scan");
    ImagePlan &p = plan.images[(size_t)i];
    const int64_t total_mcus = (int64_t)s.mcus_x * s.mcus_y;
    const bool small = too_small_for_a_walk(s);
    if (s.restart_interval > 0) {
      p.source = searched ? IntervalSource::MarkerSearch : IntervalSource::RestartMarkers;
      p.mcus_per_interval = s.restart_interval;
      p.n_intervals = (total_mcus + s.restart_interval - 1) / s.restart_interval;
      if (!searched)
        if (const char *bad = restart_markers_obstacle(*hosts[i], 0)) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, bad);
    } else if (ragged && small) {
      p.source = searched ? IntervalSource::SearchedWhole : IntervalSource::WholeScan;
      p.mcus_per_interval = s.mcus_x * s.mcus_y;
      p.n_intervals = 1;
    } else {
      // no restart markers: the decode starts from exact restart points ("virtual intervals"), about 16 K of them
      const int per = (int)std::min<int64_t>(64, std::max<int64_t>(1, total_mcus / 16384));
      if (small) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, TOO_SMALL_FOR_A_WALK);
      if (device_walk || searched) { // (the marker route: device_markers_obstacle asked for the device walk)
        p.source = searched ? IntervalSource::SearchedWalk : IntervalSource::DeviceWalk;
        p.mcus_per_interval = per;
        p.n_intervals = (total_mcus + per - 1) / per;
      } else {
        p.source = IntervalSource::HostWalk;
        p.walked.reset(new VirtualIntervals());
        if (hosts[i]->plan_virtual_intervals(0, per, 0, *p.walked))
          return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "stream without restart markers did not lend itself to speculative decoding");
        p.mcus_per_interval = p.walked->mcus_per_interval;
        p.n_intervals = (int64_t)p.walked->byte_off.size();
      }
    }
    plan.total_intervals += p.n_intervals;
  }
  if (min_intervals <= 0) min_intervals = 2048; // below this the device runs mostly idle
  if ((plan.total_intervals < min_intervals && !ragged) || plan.total_intervals > 0x7fffffff)
    return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "too few restart intervals to occupy the device");
  plan.lanes = lanes_for(plan.total_intervals);
  plan.per_group = plan.lanes * WAVES_PER_GROUP;
  // What travels to the device is the entropy coded data of every image WITHOUT its byte stuffing and without the markers,
  // one restart interval behind the other (HostDecoder::unstuff_piece; the marker search counted what leaves): the kernels
  // address it by plain bit positions (huffman.hip, DevBits).
  std::vector<size_t> stream_off;
  plan.stream_bytes = stream_slots(sizes, n, stream_off);
  for (int i = 0; i < n; i++) {
    ImagePlan &p = plan.images[(size_t)i];
    const mijpeg_info &f = hosts[i]->info;
    const Scan &s = hosts[i]->scans[0];
    p.slot_off = stream_off[(size_t)i];
    p.first_interval = i ? plan.images[(size_t)i - 1].first_interval + plan.images[(size_t)i - 1].n_intervals : 0;
    if (p.searched()) {
      p.copy_bytes = sizes[i] - s.ecs_begin;
      plan.marker_chunks += markers_chunks(p.copy_bytes);
    } else {
      p.copy_bytes = s.unstuffed_size;
      int why_code;
      if (const char *why = stream_copy_obstacle(*hosts[i], sizes[i], &why_code)) return set_error(d, why_code, why);
    }
    if (p.source == IntervalSource::RestartMarkers && (int64_t)s.interval_ubegin.size() < p.n_intervals)
      return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "restart intervals missing");
    plan.n_groups += plan.groups_of(i);
    plan.any_virtual |= p.virtual_intervals();
    plan.any_dwalk |= p.device_walked();
    // an interleaved scan writes every block of every plane; a single-component scan of a frame whose only component
    // has sampling factors > 1 leaves the MCU padding blocks untouched (they must read as zero)
    if (s.ncomp == 1 && (s.mcus_x != f.blocks_w[s.sc[0].comp] || s.mcus_y != f.blocks_h[s.sc[0].comp])) plan.needs_clear = true;
  }
  // (the stores of a ragged launch lie between those of other launches: nothing to clear in one sweep, and no layout group holds such frames)
  if (plan.needs_clear && ragged) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "single components with sampling factors are not decoded in a ragged launch");
  return MIJPEG_OK;
}

// Table slots.  Tables in LDS: components that bring the same Huffman code (Cb and Cr practically always do) share one copy -- the
// workgroup's LDS footprint decides how many of them a CU holds.  The sharing pattern is that of image 0 and must hold
// for every image of the launch; the device walk indexes its tables by component and keeps one per component.
struct TableSlots {
  int slot[MIJPEG_MAX_COMPONENTS][2]; // per scan component: DC, AC
  int ntab = 0;
  size_t blob_bytes() const { return (size_t)ntab * sizeof(HuffDevTable) + sizeof(HuffDevAux); } // one image's tables
};
TableSlots share_table_slots(HostDecoder *const *hosts, int n, bool any_dwalk)
{
  const Scan &s0 = hosts[0]->scans[0];
  TableSlots t;
  bool share = !any_dwalk;
  for (int pass = 0; pass < 2; pass++) {
    t.ntab = 0;
    for (int k = 0; k < s0.ncomp; k++)
      for (int x = 0; x < 2; x++) {
        t.slot[k][x] = -1;
        for (int j = 0; j < k && share && t.slot[k][x] < 0; j++)
          if ((x ? s0.ac[k].same_code(s0.ac[j]) : s0.dc[k].same_code(s0.dc[j]))) t.slot[k][x] = t.slot[j][x];
        if (t.slot[k][x] < 0) t.slot[k][x] = t.ntab++;
      }
    if (!share) break;
    bool holds = true; // ... in every image?
    for (int i = 1; i < n && holds; i++) {
      const Scan &s = hosts[i]->scans[0];
      for (int k = 0; k < s.ncomp && holds; k++)
        for (int j = 0; j < k && holds; j++) {
          if (t.slot[k][0] == t.slot[j][0] && !s.dc[k].same_code(s.dc[j])) holds = false;
          if (t.slot[k][1] == t.slot[j][1] && !s.ac[k].same_code(s.ac[j])) holds = false;
        }
    }
    if (holds) break;
    share = false;
  }
  return t;
}

// Layout.  The device buffer is [streams, each padded] and behind them, at these offsets,
//   [ibegin][iend][iskip][ipred][tables of every image][images][groups][planes][marker images][marker chunks][marker results][status]
//   | [marker scratch][raw segments, slots as in front]
// Pinned staging (ent_host) holds the part in front of the bar at the same offsets; it goes up as far as the status words, and
// the marker results and the status words come back in one copy.  What is behind the bar exists on the device only.
struct BatchLayout {
  bool markers; // the launch has the marker route's regions (some of its images are searched on the device)
  size_t stream_bytes;
  size_t ibegin, iend, iskip, ipred, tables, images, groups, planes, mimages, mchunks, mresults, status;
  size_t status_bytes, tail_bytes; // tail_bytes: everything in front of the bar
  MarkerScratch scratch;
  size_t mscratch, raw, end;
  size_t upload_bytes() const { return status; }
  size_t read_back_bytes() const { return status + status_bytes - mresults; }
  size_t device_extra() const { return end - tail_bytes; }
};
// nullptr, or why the launch does not fit its 32-bit offsets
const char *batch_layout(const BatchPlan &plan, size_t table_blob, const EntropyBatchOptions &opt, BatchLayout &l)
{
  static_assert(sizeof(MarkerResult) == 16, "the result words end where the status words begin");
  const size_t n = (size_t)plan.n(), T = (size_t)plan.total_intervals;
  Layout L;
  l.markers = opt.markers;
  l.stream_bytes = plan.stream_bytes;
  l.ibegin = L.take(T * 4);
  l.iend = L.take(T * 4);
  l.iskip = L.take(plan.any_virtual ? T : 0);
  l.ipred = L.take(plan.any_virtual ? T * 8 : 0);
  l.tables = L.take(n * table_blob);
  l.images = L.take(n * sizeof(HuffImage));
  l.groups = L.take((size_t)plan.n_groups * sizeof(HuffGroup));
  l.planes = L.take(opt.ragged ? n * sizeof(HuffPlanes) : 0);
  l.mimages = L.take(opt.markers ? n * sizeof(MarkerImage) : 0);
  l.mchunks = L.take(opt.markers ? (size_t)plan.marker_chunks * sizeof(MarkerChunk) : 0);
  l.mresults = L.take(opt.markers ? n * sizeof(MarkerResult) : 0);
  l.status_bytes = n * 32;
  l.status = L.take(l.status_bytes);
  l.tail_bytes = L.end;
  l.scratch = markers_scratch(plan.marker_chunks);
  l.mscratch = L.take(opt.markers ? l.scratch.end : 0);
  l.raw = L.take(opt.markers ? plan.stream_bytes : 0);
  l.end = L.end;
  if (plan.stream_bytes > 0xfffffff0ull || plan.n_groups > 0x7fffffff || (opt.markers && plan.stream_bytes + l.end > 0xfffffff0ull)) return "batch too large for one launch";
  return nullptr;
}

// Fill staging: the pinned copy (at hp) of everything the layout places behind the streams, image by image
struct Staging {
  const BatchPlan &plan;
  const BatchLayout &l;
  uint8_t *hp;

  // image i: its entries in the interval tables
  void intervals(int i, const Scan &s, const uint8_t *data) const
  {
    const ImagePlan &p = plan.images[(size_t)i];
    const int64_t first = p.first_interval, nint = p.n_intervals;
    uint32_t *ib = (uint32_t *)(hp + l.ibegin) + first, *ie = (uint32_t *)(hp + l.iend) + first;
    // (iskip and ipred exist where some image of the launch has virtual intervals)
    uint8_t *isk = plan.any_virtual ? hp + l.iskip + first : nullptr;
    int16_t *ipr = plan.any_virtual ? (int16_t *)(hp + l.ipred) + first * 4 : nullptr;
    // the marker route: the image's descriptor, its chunks and a fresh result for a search that expects `expect` intervals
    auto stage_search = [&](uint32_t expect) {
      MarkerImage *mi = (MarkerImage *)(hp + l.mimages);
      const uint32_t chunk_at = i ? mi[i - 1].first_chunk + mi[i - 1].n_chunks : 0;
      // {raw_off, size, dst_off, dst_cap, first_interval, expect, first_chunk}
      stage_marker_image(mi[i], (MarkerChunk *)(hp + l.mchunks), ((MarkerResult *)(hp + l.mresults))[i], (uint32_t)i,
                         MarkerImage{(uint32_t)p.slot_off, (uint32_t)p.copy_bytes, (uint32_t)p.slot_off, (uint32_t)(plan.slot_end(i) - p.slot_off), (uint32_t)first,
                                     expect, chunk_at, 0});
    };
    if (l.markers && !p.searched()) { // a marker launch's image that is not searched: no chunks, a result that reads as good
      MarkerImage *mi = (MarkerImage *)(hp + l.mimages);
      memset(&mi[i], 0, sizeof(MarkerImage));
      mi[i].first_chunk = i ? mi[i - 1].first_chunk + mi[i - 1].n_chunks : 0;
      memset(&((MarkerResult *)(hp + l.mresults))[i], 0, sizeof(MarkerResult));
    }
    switch (p.source) {
    case IntervalSource::SearchedWhole: // the search's begin[0] = 0 and end[0] = total are the one interval
      ib[0] = ie[0] = 0;
      if (isk) isk[0] = 0;
      stage_search(1);
      break;
    case IntervalSource::SearchedWalk:
      // begin by the EMIT walk, end by the fit step behind the search (the search's own begin[0] = 0 and end[0] = total agree with
      // both); zeroed like MarkerSearch's, so that a search that is not good leaves every interval empty at offset 0 of the slot
      memset(ib, 0, (size_t)nint * 4);
      memset(ie, 0, (size_t)nint * 4);
      memset(isk, 0, (size_t)nint);
      memset(ipr, 0, (size_t)nint * 8);
      stage_search(1);
      break;
    case IntervalSource::DeviceWalk: // filled in by the EMIT walk on the device
      for (int64_t k = 0; k < nint; k++) { ib[k] = 0; ie[k] = (uint32_t)p.copy_bytes; }
      memset(isk, 0, (size_t)nint);
      memset(ipr, 0, (size_t)nint * 8);
      break;
    case IntervalSource::HostWalk: {
      // the host's walk reports stream offsets: into the copy's (stuffed pairs in front of each, counted as the offsets go up)
      const VirtualIntervals &vi = *p.walked;
      const uint8_t *base = s.base ? s.base : data;
      size_t at = s.ecs_begin, pairs = 0;
      for (int64_t k = 0; k < nint; k++) {
        const size_t pos = vi.byte_off[(size_t)k];
        while (at < pos) {
          const uint8_t *q = (const uint8_t *)memchr(base + at, 0xff, pos - at);
          if (!q) break;
          at = (size_t)(q - base);
          if (base[at + 1] == 0x00) { pairs++; at += 2; }
          else at++;
        }
        at = std::max(at, pos);
        ib[k] = (uint32_t)(pos - s.ecs_begin - pairs);
        ie[k] = (uint32_t)p.copy_bytes;
        isk[k] = vi.bit_skip[(size_t)k];
        memcpy(ipr + k * 4, &vi.pred[(size_t)k * 4], 8);
      }
      break;
    }
    case IntervalSource::MarkerSearch: {
      // written by the search kernels; entries they leave alone (a search that is not good) must not send the Huffman kernel anywhere
      memset(ib, 0, (size_t)nint * 4);
      memset(ie, 0, (size_t)nint * 4);
      if (isk) memset(isk, 0, (size_t)nint);
      stage_search((uint32_t)nint);
      break;
    }
    case IntervalSource::WholeScan:
      ib[0] = 0;
      ie[0] = (uint32_t)p.copy_bytes;
      if (isk) isk[0] = 0;
      break;
    case IntervalSource::RestartMarkers:
      memcpy(ib, s.interval_ubegin.data(), (size_t)nint * 4);
      memcpy(ie, s.interval_uend.data(), (size_t)nint * 4);
      if (isk) memset(isk, 0, (size_t)nint);
      break;
    }
  }

  // ... its Huffman tables and dequantisation words; returns where they lie in the table region.  Images that bring the tables of the
  // image in front of them (every frame of a camera or an encoder run does) share its blob, at `table_off_in_front`: nothing to build,
  // and the workgroups of both read the same lines
  uint32_t tables(HostDecoder *const *hosts, int i, const TableSlots &slots, uint32_t table_off_in_front) const
  {
    const mijpeg_info &f = hosts[i]->info;
    const Scan &s = hosts[i]->scans[0];
    HuffDevTable *tabs = (HuffDevTable *)(hp + l.tables + (size_t)i * slots.blob_bytes());
    HuffDevAux *aux = (HuffDevAux *)(tabs + slots.ntab);
    bool same_tables = i > 0;
    if (same_tables) {
      const mijpeg_info &fp = hosts[i - 1]->info;
      const Scan &sp = hosts[i - 1]->scans[0];
      for (int k = 0; k < s.ncomp && same_tables; k++) {
        const int c = s.sc[k].comp;
        same_tables = s.dc[k].same_code(sp.dc[k]) && s.ac[k].same_code(sp.ac[k]) &&
                      !memcmp(f.quant[f.quant_index[c]], fp.quant[fp.quant_index[c]], sizeof(f.quant[0]));
      }
    }
    memset(aux, 0, sizeof(*aux));
    if (same_tables) return table_off_in_front;
    for (int k = 0; k < s.ncomp; k++) {
      build_dev_table(tabs[slots.slot[k][0]], s.dc[k], 0);
      build_dev_table(tabs[slots.slot[k][1]], s.ac[k], 1);
      const int c = s.sc[k].comp;
      const uint16_t *delta = f.quant[f.quant_index[c]];
      for (int z = 0; z < 80; z++) {
        const uint32_t pos = scan_order()[z];
        aux->zq[k][z] = ((uint32_t)delta[pos] << 16) | (pos * 2);
      }
    }
    return (uint32_t)((size_t)i * slots.blob_bytes());
  }

  // ... and its descriptor, its plane geometry (ragged launches) and its workgroups, from groups[g] on
  void descriptors(int i, const mijpeg_info &f, const Scan &s, uint32_t table_off, int64_t coef_base, bool ragged, int64_t &g) const
  {
    const ImagePlan &p = plan.images[(size_t)i];
    HuffImage &im = ((HuffImage *)(hp + l.images))[i];
    im.stream_off = (uint32_t)p.slot_off;
    im.first_interval = (uint32_t)p.first_interval;
    im.n_intervals = (int32_t)p.n_intervals;
    im.restart_interval = p.mcus_per_interval;
    im.virt = p.virtual_intervals() ? 1u : 0u;
    im.reserved = 0;
    im.total_mcus = s.mcus_x * s.mcus_y;
    im.mcus_x = s.mcus_x;
    im.coef_base = coef_base;
    im.table_off = table_off;
    im.status_off = (uint32_t)(i * 8);
    if (ragged) {
      HuffPlanes &pl = ((HuffPlanes *)(hp + l.planes))[i];
      memset(&pl, 0, sizeof(pl));
      for (int k = 0; k < s.ncomp; k++) {
        pl.bw[k] = (uint32_t)f.blocks_w[s.sc[k].comp];
        pl.base[k] = (uint32_t)(f.coef_offset[s.sc[k].comp] >> 6);
      }
    }
    HuffGroup *groups = (HuffGroup *)(hp + l.groups);
    for (int64_t k = 0; k < p.n_intervals; k += plan.per_group) {
      groups[g].image = (uint32_t)i;
      groups[g].first_interval = (uint32_t)k;
      g++;
    }
  }
};

// Kernel arguments of the scan kernel: the regions of the layout in the object's buffer, the geometry the images share (image 0's)
HuffScanArgs scan_args(const mijpeg_decoder *d, const HostDecoder &h0, const BatchPlan &plan, const TableSlots &slots, const BatchLayout &l, int16_t *coef_dev, bool ragged)
{
  const mijpeg_info &f0 = h0.info;
  const Scan &s0 = h0.scans[0];
  uint8_t *const dp = d->ent_dev + l.stream_bytes;
  HuffScanArgs a;
  memset(&a, 0, sizeof(a));
  a.lanes = plan.lanes;
  a.waves_per_group = WAVES_PER_GROUP;
  for (int k = 0; k < s0.ncomp; k++) {
    const int c = s0.sc[k].comp;
    a.comp_of[k] = c;
    const McuBlocks b = mcu_blocks(f0, s0, k);
    a.hs[k] = b.h;
    a.vs[k] = b.v;
    a.bw[k] = f0.blocks_w[c];
    a.coef_off[k] = f0.coef_offset[c];
    a.dc_tab[k] = slots.slot[k][0];
    a.ac_tab[k] = slots.slot[k][1];
  }
  a.data = d->ent_dev;
  a.ibegin = (const uint32_t *)(dp + l.ibegin);
  a.iend = (const uint32_t *)(dp + l.iend);
  a.iskip = dp + l.iskip;
  a.ipred = (const int16_t *)(dp + l.ipred);
  a.images = (const HuffImage *)(dp + l.images);
  a.groups = (const HuffGroup *)(dp + l.groups);
  a.n_groups = (int32_t)plan.n_groups;
  a.ncomp = s0.ncomp;
  a.ntables = slots.ntab;
  a.tables = dp + l.tables;
  a.coef = coef_dev;
  a.status = (uint32_t *)(dp + l.status);
  a.planes = ragged ? (const HuffPlanes *)(dp + l.planes) : nullptr;
  return a;
}

// Enqueue: the streams of the images go up and the kernels are launched behind them, on d->stream and d->copy_stream
struct Enqueue {
  mijpeg_decoder *d;
  HostDecoder *const *hosts;
  const uint8_t *const *datas;
  const BatchPlan &plan;
  const BatchLayout &l;
  const HuffScanArgs &scan;
  const MarkerArgs &search; // (the marker route)
  const EntropyBatchOptions &opt;
  const TraceMarks &mark;
  Gather gather;

  uint8_t *tail_dev() const { return d->ent_dev + l.stream_bytes; }

  // the unstuffing gather of images [g0, g1) into the pinned area (images whose marker search wrote the copy already -- a
  // batch's workers do, set_unstuff_sink -- have nothing left to do)
  void gather_images(int g0, int g1)
  {
    if (opt.markers) { // one memcpy per searched image: the raw segment into its slot
      auto copy = [&](int i) {
        const ImagePlan &p = plan.images[(size_t)i];
        if (p.searched()) memcpy(d->stage_host + p.slot_off, datas[i] + hosts[i]->scans[0].ecs_begin, p.copy_bytes);
      };
      if (g1 - g0 > 1) parallel_for(g1 - g0, [&](int k) { copy(g0 + k); });
      else copy(g0);
    }
    for (int i = g0; i < g1; i++) {
      uint8_t *const slot = d->stage_host + plan.images[(size_t)i].slot_off;
      if (!plan.images[(size_t)i].searched() && hosts[i]->scans[0].unstuffed_at != slot) gather.add(hosts[i], 0, slot);
    }
    gather.run();
  }

  // the upload of images [g0, g1) from the pinned area.  Without `done`: on the object's stream, image by image, only what the
  // copies occupy (a slot is as large as its stream, headers and all).  With it: their slots in one copy on the copy stream,
  // `done` recorded behind it, and the object's stream waits for that.
  int upload_images(int g0, int g1, hipEvent_t done = nullptr)
  {
    // (the marker route: a searched image's raw segment goes beside the slots, the search writes the copy into its slot)
    auto dst_of = [&](int i) { return plan.images[(size_t)i].searched() ? tail_dev() + l.raw : d->ent_dev; };
    if (done) {
      // images that go to the same place travel in one copy (a uniform launch: all of them)
      for (int i0 = g0; i0 < g1;) {
        int i1 = i0 + 1;
        while (i1 < g1 && dst_of(i1) == dst_of(i0)) i1++;
        const size_t b0 = plan.images[(size_t)i0].slot_off, b1 = plan.slot_end(i1 - 1);
        HIP_TRY(d, hipMemcpyAsync(dst_of(i0) + b0, d->stage_host + b0, b1 - b0, hipMemcpyHostToDevice, d->copy_stream));
        i0 = i1;
      }
      HIP_TRY(d, hipEventRecord(done, d->copy_stream));
      HIP_TRY(d, hipStreamWaitEvent(d->stream, done, 0));
      return MIJPEG_OK;
    }
    for (int i = g0; i < g1; i++) {
      const ImagePlan &p = plan.images[(size_t)i];
      const size_t bytes = p.searched() ? p.copy_bytes : ((p.copy_bytes + 15) & ~(size_t)15) + HUFF_STREAM_PAD;
      if (bytes) HIP_TRY(d, hipMemcpyAsync(dst_of(i) + p.slot_off, d->stage_host + p.slot_off, bytes, hipMemcpyHostToDevice, d->stream));
    }
    return MIJPEG_OK;
  }

  // the marker search of images [g0, g1) on the object's stream, behind their upload
  int search_images(int g0, int g1)
  {
    const MarkerImage *mi = (const MarkerImage *)(d->ent_host + l.mimages);
    MarkerArgs part = search;
    part.chunk0 = mi[g0].first_chunk;
    part.n_chunks = mi[g1 - 1].first_chunk + mi[g1 - 1].n_chunks - part.chunk0;
    if (launch_marker_search(part, (uint64_t *)(tail_dev() + l.mscratch + l.scratch.scan), l.scratch.scan_words, d->stream))
      return hip_fail(d, hipGetLastError(), "marker search launch");
    return MIJPEG_OK;
  }

  // the scan kernel for workgroups [wg0, wg1) of the launch
  int launch_scan(int64_t wg0, int64_t wg1)
  {
    HuffScanArgs part = scan;
    part.groups = scan.groups + wg0;
    part.n_groups = (int32_t)(wg1 - wg0);
    if (launch_huffman_scan(part, d->stream)) return hip_fail(d, hipGetLastError(), "huffman_scan_kernel launch");
    if (opt.ragged) ++*opt.ragged->entropy_launches;
    return MIJPEG_OK;
  }

  // every image in one launch; streams without restart markers: the walk finds the intervals of every image first
  int decode_all()
  {
    if (plan.any_dwalk) {
      uint8_t *const dp = tail_dev();
      const int rc = device_walk_images(d, hosts, plan, opt, scan,
                                        DeviceIntervals{(uint32_t *)(dp + l.ibegin), (uint32_t *)(dp + l.iend), dp + l.iskip, (int16_t *)(dp + l.ipred)}, search);
      if (rc) return rc;
      mark("device walk enqueued");
    }
    return launch_scan(0, plan.n_groups);
  }

  int run()
  {
    const int n = plan.n();
    int rc;
    // (a deferred batch always goes through the pinned gathering area: the caller's bytes are only read during the call)
    const bool small = !opt.defer && (n == 1 || plan.stream_bytes < ((size_t)8 << 20));
    if ((rc = ensure_pinned(d, &d->stage_host, &d->stage_cap, plan.stream_bytes))) return rc;
    if (small) {
      gather_images(0, n);
      if ((rc = upload_images(0, n))) return rc;
      if (opt.markers && (rc = search_images(0, n))) return rc;
      return decode_all();
    }
    // large batches, in up to eight groups of images: the pool threads gather a group's streams into pinned memory, its
    // DMA runs on a copy stream while the next group is gathered and while the kernel decodes the previous one
    mark("staging buffer ready");
    // Images per upload + launch.  A launch is latency-bound (the serial symbol chain of its longest restart interval,
    // ~0.3 ms) until it holds several waves per SIMD: ~128 K restart intervals; more, smaller launches only pay when the
    // batch is so large that the upload of one part hides behind the decode of another (profiles/r02/batch4k_*.txt:
    // 32 x 4K frames in one launch 0.80 ms, in eight launches of four 8 x 0.39 ms).
    const int64_t per_image = std::max<int64_t>(1, plan.total_intervals / n);
    const int groups_of = (int)std::max<int64_t>(std::max(4, (n + 7) / 8), (131072 + per_image - 1) / per_image);
    if ((rc = prepare_copy_stream(d, (size_t)((n + groups_of - 1) / groups_of)))) return rc;
    // the walk covers all images at once; a ragged group is one launch by contract
    const bool launch_per_group = !plan.any_dwalk && !opt.ragged;
    int64_t wg0 = 0;
    for (int gi = 0, g0 = 0; g0 < n; g0 += groups_of, gi++) {
      const int g1 = std::min(n, g0 + groups_of);
      gather_images(g0, g1);
      if ((rc = upload_images(g0, g1, d->copy_events[(size_t)gi]))) return rc;
      if (opt.markers && (rc = search_images(g0, g1))) return rc;
      if (!launch_per_group) continue;
      int64_t wg1 = wg0;
      for (int i = g0; i < g1; i++) wg1 += plan.groups_of(i);
      if ((rc = launch_scan(wg0, wg1))) return rc; // the workgroups of this group's images
      wg0 = wg1;
    }
    mark("groups gathered + enqueued");
    return launch_per_group ? MIJPEG_OK : decode_all();
  }
};

// Read back: the walk's status words, the marker results and the status words (pinned); the deferred hand-over or the verdict
struct ReadBack {
  uint32_t *status, *walk_status; // walk_status: null without a device walk
  const uint32_t *markers;        // null off the marker route
};
int read_back(mijpeg_decoder *d, const BatchPlan &plan, const BatchLayout &l, const EntropyBatchOptions &opt, ReadBack &back)
{
  uint8_t *const hp = d->ent_host, *const dp = d->ent_dev + l.stream_bytes;
  const int n = plan.n();
  back.status = (uint32_t *)(hp + l.status);
  back.walk_status = plan.any_dwalk ? (uint32_t *)d->walk_host : nullptr; // the walk's staging buffer is free again
  back.markers = opt.markers ? (const uint32_t *)(hp + l.mresults) : nullptr;
  if (plan.any_dwalk) HIP_TRY(d, hipMemcpyAsync(back.walk_status, d->walk_status_dev, (size_t)n * 4, hipMemcpyDeviceToHost, d->stream));
  // (the marker route's result words lie right in front of the status words: one copy)
  if (const int rc = read_back_status(d, (uint32_t *)(hp + l.mresults), dp + l.mresults, l.read_back_bytes())) return rc;
  d->pend_markers = nullptr;
  if (opt.markers) {
    d->markers_want_term.resize((size_t)n);
    for (int i = 0; i < n; i++) // (an image of the launch that is not searched: its result was staged as zeros and stays so)
      d->markers_want_term[(size_t)i] = plan.images[(size_t)i].searched() ? (uint32_t)plan.images[(size_t)i].copy_bytes - 2u : 0u;
  }
  return MIJPEG_OK;
}

// mijpeg_submit_batch_device: the caller waits later (finish_batch)
void hand_over(mijpeg_decoder *d, int n, const ReadBack &back, std::chrono::steady_clock::time_point t0)
{
  d->pend_n = n;
  d->pend_status = back.status;
  d->pend_walk_status = back.walk_status;
  d->pend_markers = back.markers;
  d->pend_t0 = t0;
}

// What the words that came back say, once the stream is idle
int verdict(mijpeg_decoder *d, HostDecoder *const *hosts, int n, const ReadBack &back, const EntropyBatchOptions &opt)
{
  if (opt.ragged) {
    // image by image: one that the walk or the kernel found damaged goes to the single-image route, the others stand
    for (int i = 0; i < n; i++) {
      HostDecoder *h = hosts[i];
      const bool bad = (back.walk_status && back.walk_status[i]) || evaluate_entropy_status(d, &h, 1, back.status + 8 * i) != MIJPEG_OK;
      opt.ragged->verdict[i] = bad ? 1 : 0;
      if (!opt.markers || !h->scans[0].search_skipped) continue;
      // a member the device searched: the search's verdict comes first
      if (!device_markers_good(back.markers + 4 * i, d->markers_want_term.data() + i, 1)) opt.ragged->verdict[i] = 2;
      else h->scans[0].unstuffed_size = ((const MarkerResult *)back.markers)[i].total;
    }
    return MIJPEG_OK;
  }
  if (opt.markers) {
    if (!device_markers_good(back.markers, d->markers_want_term.data(), n)) {
      d->markers_retry = true;
      return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "device marker search: the segment is not the plain case; the host searches it");
    }
    for (int i = 0; i < n; i++) hosts[i]->scans[0].unstuffed_size = ((const MarkerResult *)back.markers)[i].total;
  }
  if (back.walk_status)
    if (const int rc = walk_verdict(d, back.walk_status, n)) return rc;
  return evaluate_entropy_status(d, hosts, n, back.status);
}

} // namespace

// Entropy-decode n parsed images on the device with one launch of huffman_scan_kernel (large uniform batches: one per upload
// group).  Without opt.ragged: images of identical frame geometry, image i into coef_dev + i * frame_stride.  With it: images that
// share components and sampling factors but not their size, image i into coef_dev + ragged->coef_base[i], plane geometry per
// image; a damaged image is reported in ragged->verdict[i] instead of failing the call.
// opt.markers: the streams were parsed without a marker search (device_markers_obstacle holds for each): their raw segments go up,
// and the search kernels write the copies and the interval tables in front of the Huffman launch.  A ragged launch: those of its
// members whose Scan::search_skipped says so, side by side with members that are not; ragged->verdict[i] = 2 for a search that is not good.  On a search that is not
// good the call answers MIJPEG_ERR_NOT_AVAILABLE with d->markers_retry set (deferred: mijpeg_finish_batch_device looks).
// hosts[i]->info receives fast_arith / range_max.  Returns MIJPEG_OK, MIJPEG_ERR_NOT_AVAILABLE (nothing touched) or an error.
int device_entropy_batch(mijpeg_decoder *d, HostDecoder *const *hosts, const uint8_t *const *datas, const size_t *sizes, int n,
                         int min_intervals, int16_t *coef_dev, int64_t frame_stride, const EntropyBatchOptions &opt)
{
  if (opt.markers && opt.xt_part) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "device marker search: plain streams only");
  const auto tb0 = std::chrono::steady_clock::now();
  int rc;
  BatchPlan plan;
  if ((rc = plan_batch(d, hosts, sizes, n, min_intervals, opt, plan))) return rc;
  const TableSlots slots = share_table_slots(hosts, n, plan.any_dwalk);
  BatchLayout l;
  if (const char *why = batch_layout(plan, slots.blob_bytes(), opt, l)) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, why);
  if ((rc = ensure_entropy_buffers(d, l.stream_bytes, l.tail_bytes, l.device_extra()))) return rc;
  uint8_t *const hp = d->ent_host, *const dp = d->ent_dev + l.stream_bytes;
  const Staging staging{plan, l, hp};
  int64_t g = 0;
  uint32_t table_off = 0;
  for (int i = 0; i < n; i++) {
    const Scan &s = hosts[i]->scans[0];
    staging.intervals(i, s, datas[i]);
    table_off = staging.tables(hosts, i, slots, table_off);
    staging.descriptors(i, hosts[i]->info, s, table_off, opt.ragged ? opt.ragged->coef_base[i] : (int64_t)i * frame_stride, opt.ragged != nullptr, g);
  }
  const HuffScanArgs scan = scan_args(d, *hosts[0], plan, slots, l, coef_dev, opt.ragged != nullptr);
  MarkerArgs search;
  memset(&search, 0, sizeof(search));
  if (opt.markers)
    search = marker_args(dp + l.raw, d->ent_dev, (uint32_t *)(dp + l.ibegin), (uint32_t *)(dp + l.iend), (const MarkerImage *)(dp + l.mimages),
                         (const MarkerChunk *)(dp + l.mchunks), (MarkerResult *)(dp + l.mresults), dp + l.mscratch, l.scratch);
  const TraceMarks mark{"mijpeg"};
  const auto tb1 = mark.t0;
  QuiesceOnError guard{d};
  guard.armed = true;
  HIP_TRY(d, hipMemcpyAsync(dp, hp, l.upload_bytes(), hipMemcpyHostToDevice, d->stream));
  HIP_TRY(d, hipMemsetAsync(dp + l.status, 0, l.status_bytes, d->stream));
  if (plan.needs_clear) HIP_TRY(d, hipMemsetAsync(coef_dev, 0, (size_t)n * (size_t)frame_stride * sizeof(int16_t), d->stream));
  Enqueue enqueue{d, hosts, datas, plan, l, scan, search, opt, mark, Gather{}};
  if ((rc = enqueue.run())) return rc;
  ReadBack back;
  if ((rc = read_back(d, plan, l, opt, back))) return rc;
  d->phase_prepare = std::chrono::duration<double>(tb1 - tb0).count(); // interval tables, Huffman tables
  mark("status copies enqueued");
  if (!plan.any_dwalk) d->pend_walk_round = 0;
  if (opt.defer) {
    guard.armed = false;
    hand_over(d, n, back, tb1);
    d->phase_device = std::chrono::duration<double>(std::chrono::steady_clock::now() - tb1).count(); // so far: gathering + enqueueing
    return MIJPEG_OK;
  }
  HIP_TRY(d, hipStreamSynchronize(d->stream));
  guard.armed = false; // (everything of this call is behind the stream's last copy)
  d->phase_device = std::chrono::duration<double>(std::chrono::steady_clock::now() - tb1).count();  // upload + kernel + status
  return verdict(d, hosts, n, back, opt);
}

// ------------------------------------------------------------------------------------------------
// Progressive frames and frames with hidden refinement scans on the device (huffman_prog_kernel)
// ------------------------------------------------------------------------------------------------
// nullptr: every scan of the frame can be decoded one restart interval per lane.
const char *multiscan_obstacle(const HostDecoder &h, bool xt_part, bool residual_frame)
{
  const mijpeg_info &f = h.info;
  if (const char *why = stream_obstacle(h, xt_part, false)) return why;
  if (f.dnl) return "on-device entropy decoding: frames whose height arrives in a DNL marker are decoded on the host";
  // (12-bit frames: the same int16 store as the host decoder's, a coefficient beyond it sends the frame there like everywhere)
  if (f.precision < 8 || f.precision > 12 || (xt_part && !residual_frame && f.precision != 8))
    return "on-device entropy decoding: frames of 8 to 12 bits (JPEG XT: an 8-bit legacy frame)";
  if (h.scans.empty() || h.scans.size() > 4096) return "on-device entropy decoding: no scans, or more than the device path plans for";
  if (!h.every_component_seen()) return "on-device entropy decoding: a component appears in no scan (the host decoder supplies its stand-in)";
  if (const char *why = sampling_obstacle(f)) return why;
  for (size_t si = 0; si < h.scans.size(); si++) {
    const Scan &s = h.scans[si];
    if (s.residual) return "on-device entropy decoding: the residual scan types of part 8 are decoded on the host";
    if (s.ncomp < 1 || (s.se > 0 && s.ss > 0 && s.ncomp != 1)) return "on-device entropy decoding: scan layout";
    if (s.ah > 0 && !s.refinement) return "on-device entropy decoding: scan layout";
    if (s.unstuffed_size >= ((size_t)1 << 28)) return "on-device entropy decoding: entropy coded segment too large for the device decoder's bit addresses";
    const int64_t total_mcus = (int64_t)s.mcus_x * s.mcus_y;
    if (total_mcus < 1 || total_mcus > 0x7fffffff) return "on-device entropy decoding: scan layout";
    if (s.restart_interval > 0) {
      const int64_t nint = (total_mcus + s.restart_interval - 1) / s.restart_interval;
      if ((int64_t)s.interval_ubegin.size() < nint) // (the copy's interval table is the one that goes up)
        return "restart markers missing: the host decoder resynchronises like the reference (entropyparser.cpp:117-201)";
      if (const char *why = restart_markers_obstacle(h, si)) return why;
    } else {
      // One interval: one lane decodes the whole scan.  First passes could be cut into pieces that fall into step with the real
      // decoder; an AC refinement scan cannot -- the bits a block takes depend on which block it is -- so scans
      // without restart markers are left to the host's pipeline of scans unless they are small
      if (s.interval_ubegin.empty()) return "on-device entropy decoding: scan without data";
      if (s.unstuffed_size > ((size_t)24 << 10))
        return "on-device entropy decoding: progressive / refinement scans without restart markers are serial by construction (refinementscan.cpp:584-700): host";
    }
    for (int k = 0; k < s.ncomp; k++) {
      if (s.ss == 0 && s.ah == 0 && !s.dc[k].built) return "on-device entropy decoding: a Huffman table the scan names does not exist";
      if (s.se > 0 && !s.ac[k].built) return "on-device entropy decoding: a Huffman table the scan names does not exist";
    }
  }
  return nullptr;
}

namespace {

// The range pass over one frame's finished planes
CoefRangeArgs coef_range_args(const mijpeg_decoder *d, const MultiScanFrame &fr, uint32_t *status)
{
  const mijpeg_info &f = fr.h->info;
  CoefRangeArgs r;
  memset(&r, 0, sizeof(r));
  r.coef = (const void *)(d->coef_dev + fr.base16);
  r.wide = fr.wide ? 1 : 0;
  r.ncomp = f.components;
  for (int c = 0; c < f.components; c++) {
    r.coef_off[c] = plane_offset(f, c);
    r.nblocks[c] = (int64_t)f.blocks_w[c] * f.blocks_h[c];
    memcpy(r.q[c], f.quant[f.quant_index[c]], sizeof(r.q[c]));
  }
  r.status = status;
  return r;
}

// device_entropy_multiscan's stages behind plan and staging (entropy_plan.hpp).  The entropy coded data of every scan without its
// stuffing is gathered by the pool in two goes: what the first launches read, then the rest -- while the copy engine brings up the
// first part and the first launches run.  Uploads on the copy stream, one event per level; the frames' launches wait for their
// level's event.
struct MultiscanRun {
  mijpeg_decoder *d;
  const MultiScanFrame *frames;
  int nframes;
  const MultiscanPlan &p;
  hipStream_t second; // the two frames of a JPEG XT file share nothing: the second one's launches go to a stream of their own
  ProgArgs a;
  Gather gather;

  uint8_t *tail_dev() const { return d->ent_dev + p.stream_bytes; }
  uint32_t *status_dev(int fi) const { return (uint32_t *)(tail_dev() + p.status) + 8 * fi; }
  hipStream_t stream_of(int fi) const { return fi == 0 ? d->stream : second; }

  int prepare_second_stream()
  {
    second = d->stream;
    if (nframes > 1) {
      if (!d->ms_stream) HIP_TRY(d, hipStreamCreateWithFlags(&d->ms_stream, hipStreamNonBlocking));
      if (!d->ms_ready) HIP_TRY(d, hipEventCreateWithFlags(&d->ms_ready, hipEventDisableTiming));
      if (!d->ms_done) HIP_TRY(d, hipEventCreateWithFlags(&d->ms_done, hipEventDisableTiming));
      second = d->ms_stream;
    }
    return MIJPEG_OK;
  }

  // what every launch shares (launch_levels: its workgroups, lanes, frame)
  void arguments()
  {
    uint8_t *const dp = tail_dev();
    memset(&a, 0, sizeof(a));
    a.data = d->ent_dev;
    a.ibegin = (const uint32_t *)(dp + p.ibegin);
    a.iend = (const uint32_t *)(dp + p.iend);
    a.scans = (const ProgScanDev *)(dp + p.scans);
    a.waves_per_group = WAVES_PER_GROUP;
    a.max_tables = p.max_tables;
    a.tables = dp + p.tables;
  }

  void gather_levels(int lv0, int lv1)
  {
    for (const MultiscanPlan::Item &it : p.items)
      if (it.level >= lv0 && it.level < lv1) gather.add(frames[it.frame].h, it.scan, d->stage_host + it.stream_off);
    gather.run();
  }

  // (tables, intervals, descriptors and groups travel in front of level 0's bytes)
  int upload_levels(int lv0, int lv1)
  {
    for (int lv = lv0; lv < lv1; lv++) {
      const size_t b0 = lv ? p.level_end[(size_t)lv - 1] : 0, b1 = p.level_end[(size_t)lv];
      if (lv == 0) HIP_TRY(d, hipMemcpyAsync(tail_dev(), d->ent_host, p.status, hipMemcpyHostToDevice, d->copy_stream));
      if (b1 > b0) HIP_TRY(d, hipMemcpyAsync(d->ent_dev + b0, d->stage_host + b0, b1 - b0, hipMemcpyHostToDevice, d->copy_stream));
      HIP_TRY(d, hipEventRecord(d->copy_events[(size_t)lv], d->copy_stream));
    }
    return MIJPEG_OK;
  }

  int clear_status_and_planes()
  {
    HIP_TRY(d, hipMemsetAsync(tail_dev() + p.status, 0, p.status_bytes, d->stream));
    if (nframes > 1) { // (behind whatever the object's stream still does with the planes, and the cleared status words)
      HIP_TRY(d, hipEventRecord(d->ms_ready, d->stream));
      HIP_TRY(d, hipStreamWaitEvent(second, d->ms_ready, 0));
    }
    // coefficients accumulate over the scans: the planes start out as zeros (coding/blockrow.cpp:77-87)
    for (int fi = 0; fi < nframes; fi++) {
      const mijpeg_info &f = frames[fi].h->info;
      int64_t count = 0;
      for (int c = 0; c < f.components; c++) count += (int64_t)f.blocks_w[c] * f.blocks_h[c] * 64;
      HIP_TRY(d, hipMemsetAsync(d->coef_dev + frames[fi].base16, 0, (size_t)count * (frames[fi].wide ? 4 : 2), stream_of(fi)));
    }
    return MIJPEG_OK;
  }

  int launch_levels(int lv0, int lv1)
  {
    for (const MultiscanPlan::Launch &l : p.launches) {
      const int fi = l.frame, lv = l.level;
      if (lv < lv0 || lv >= lv1) continue;
      HIP_TRY(d, hipStreamWaitEvent(stream_of(fi), d->copy_events[(size_t)lv], 0));
      a.groups = (const ProgGroup *)(tail_dev() + p.groups) + l.g0;
      a.n_groups = (int32_t)l.groups;
      a.lanes = p.level_lanes[(size_t)fi][(size_t)lv];
      a.wide = frames[fi].wide ? 1 : 0;
      a.coef = (void *)(d->coef_dev + frames[fi].base16);
      a.status = status_dev(fi);
      if (launch_huffman_prog(a, stream_of(fi))) return hip_fail(d, hipGetLastError(), "huffman_prog_kernel launch");
    }
    return MIJPEG_OK;
  }

  int join_second_stream()
  {
    if (second == d->stream) return MIJPEG_OK;
    HIP_TRY(d, hipEventRecord(d->ms_done, second));
    HIP_TRY(d, hipStreamWaitEvent(d->stream, d->ms_done, 0));
    return MIJPEG_OK;
  }

  int range_pass()
  {
    for (int fi = 0; fi < nframes; fi++)
      if (launch_coef_range(coef_range_args(d, frames[fi], status_dev(fi)), d->stream)) return hip_fail(d, hipGetLastError(), "coef_range_kernel launch");
    return MIJPEG_OK;
  }
};

} // namespace

// All scans of the given frames (one file: a progressive picture, or the two frames of a JPEG XT file): upload of the entropy
// coded data without its stuffing, planes cleared, the scans launched level by level (scans that share a component one after
// the other, the rest side by side), range pass.  MIJPEG_ERR_NOT_AVAILABLE: the host decoder's.
int device_entropy_multiscan(mijpeg_decoder *d, const MultiScanFrame *frames, int nframes, int min_intervals)
{
  const TraceMarks mark{"mijpeg multiscan"};
  std::vector<FrameScans> views;
  for (int fi = 0; fi < nframes; fi++) views.push_back(FrameScans{&frames[fi].h->info, &frames[fi].h->scans});
  MultiscanPlan plan;
  if (const char *why = plan_multiscan(views.data(), nframes, min_intervals, plan)) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, why);
  int rc;
  if ((rc = ensure_entropy_buffers(d, plan.stream_bytes, plan.end))) return rc;
  if ((rc = ensure_pinned(d, &d->stage_host, &d->stage_cap, plan.stream_bytes))) return rc;
  fill_multiscan(plan, views.data(), d->ent_host);
  mark("tables + intervals");
  QuiesceOnError guard{d};
  guard.armed = true;
  if ((rc = prepare_copy_stream(d, (size_t)plan.levels()))) return rc;
  MultiscanRun run{d, frames, nframes, plan, d->stream, ProgArgs(), Gather{}};
  if ((rc = run.prepare_second_stream())) return rc;
  run.arguments();
  run.gather_levels(0, plan.cut);
  mark("first levels gathered");
  if ((rc = run.upload_levels(0, plan.cut))) return rc;
  if ((rc = run.clear_status_and_planes())) return rc;
  if ((rc = run.launch_levels(0, plan.cut))) return rc;
  if (plan.cut < plan.levels()) {
    run.gather_levels(plan.cut, plan.levels());
    mark("other levels gathered");
    if ((rc = run.upload_levels(plan.cut, plan.levels()))) return rc;
    if ((rc = run.launch_levels(plan.cut, plan.levels()))) return rc;
  }
  if ((rc = run.join_second_stream())) return rc;
  if ((rc = run.range_pass())) return rc;
  uint32_t *status_host = (uint32_t *)(d->ent_host + plan.status);
  if ((rc = read_back_status(d, status_host, run.tail_dev() + plan.status, plan.status_bytes))) return rc;
  mark("launches enqueued");
  HIP_TRY(d, hipStreamSynchronize(d->stream));
  guard.armed = false; // (the second frame's stream and the copy stream are behind it)
  mark("device done");
  std::vector<HostDecoder *> hosts((size_t)nframes);
  for (int fi = 0; fi < nframes; fi++) hosts[(size_t)fi] = frames[fi].h;
  return evaluate_entropy_status(d, hosts.data(), nframes, status_host);
}

// ------------------------------------------------------------------------------------------------
// mijpeg_device_marker_search: the search kernels on one segment of the caller's, with guard bytes around the device copies of
// everything they write
// ------------------------------------------------------------------------------------------------
int64_t device_marker_search(mijpeg_decoder *d, const uint8_t *segment, size_t size, int32_t expect, uint8_t *dst, size_t capacity,
                             uint32_t *begin, uint32_t *end, uint32_t *term, uint32_t *flags)
{
  if ((!segment && size) || expect < 1 || (!dst && capacity) || !term || !flags) return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "mijpeg_device_marker_search: arguments");
  if (d->device < 0) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "decoder was created without a device");
  if (size >= MARKERS_MAX_SEGMENT || capacity >= ((size_t)1 << 30))
    return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "entropy coded segment too large for the device decoder's bit addresses");
  if (capacity < size) return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "mijpeg_device_marker_search: the destination needs the segment's size");
  HIP_TRY(d, hipSetDevice(d->device));
  if (const int prc = settle_pending(d)) return prc;
  quiesce(d); // (the entropy buffers change hands)
  constexpr size_t GUARD = 64;
  constexpr uint8_t PATTERN = 0xa5;
  const uint32_t C = markers_chunks(size);
  const size_t E = (size_t)expect;
  // [raw][guard dst guard begin guard end guard][image, chunks, result] go up, everything from the first guard on comes back
  Layout L;
  const size_t o_raw = L.take(size), o_g0 = L.take(GUARD), o_dst = L.take(capacity), o_g1 = L.take(GUARD), o_begin = L.take(E * 4), o_g2 = L.take(GUARD);
  const size_t o_end = L.take(E * 4), o_g3 = L.take(GUARD), o_img = L.take(sizeof(MarkerImage)), o_chunk = L.take((size_t)C * sizeof(MarkerChunk));
  const size_t o_res = L.take(sizeof(MarkerResult)), o_up_end = L.end;
  const MarkerScratch ms = markers_scratch(C);
  const size_t o_scratch = L.take(ms.end);
  int rc = ensure_dev(d, (void **)&d->ent_dev, &d->ent_cap, L.end);
  if (!rc) rc = ensure_pinned(d, &d->ent_host, &d->ent_host_cap, o_up_end);
  if (rc) return rc;
  uint8_t *const hp = d->ent_host, *const dp = d->ent_dev;
  memset(hp, PATTERN, o_up_end); // (the regions the kernels write start out as the pattern too: what they leave alone shows)
  if (size) memcpy(hp + o_raw, segment, size);
  MarkerResult &res = *(MarkerResult *)(hp + o_res);
  // {raw_off, size, dst_off, dst_cap, first_interval, expect, first_chunk}
  stage_marker_image(*(MarkerImage *)(hp + o_img), (MarkerChunk *)(hp + o_chunk), res, 0,
                     MarkerImage{(uint32_t)o_raw, (uint32_t)size, (uint32_t)o_dst, (uint32_t)capacity, 0, (uint32_t)expect, 0, 0});
  MarkerArgs a = marker_args(dp, dp, (uint32_t *)(dp + o_begin), (uint32_t *)(dp + o_end), (const MarkerImage *)(dp + o_img), (const MarkerChunk *)(dp + o_chunk),
                             (MarkerResult *)(dp + o_res), dp + o_scratch, ms);
  a.chunk0 = 0;
  a.n_chunks = C;
  QuiesceOnError guard{d};
  guard.armed = true;
  HIP_TRY(d, hipMemcpyAsync(dp, hp, o_up_end, hipMemcpyHostToDevice, d->stream));
  if (launch_marker_search(a, (uint64_t *)(dp + o_scratch + ms.scan), ms.scan_words, d->stream)) return hip_fail(d, hipGetLastError(), "marker search launch");
  HIP_TRY(d, hipMemcpyAsync(hp + o_g0, dp + o_g0, o_up_end - o_g0, hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(d, hipStreamSynchronize(d->stream));
  guard.armed = false;
  const size_t guards[4] = {o_g0, o_g1, o_g2, o_g3};
  for (size_t g : guards)
    for (size_t k = 0; k < GUARD; k++)
      if (hp[g + k] != PATTERN) return set_error(d, MIJPEG_ERR_PHASE_ERROR, "device marker search: bytes outside the buffers handed in were written");
  // (the pads between a region's last byte and the next 16-byte boundary belong to the guards)
  const size_t region_end[3] = {o_dst + capacity, o_begin + E * 4, o_end + E * 4}, next[3] = {o_g1, o_g2, o_g3};
  for (int r = 0; r < 3; r++)
    for (size_t k = region_end[r]; k < next[r]; k++)
      if (hp[k] != PATTERN) return set_error(d, MIJPEG_ERR_PHASE_ERROR, "device marker search: bytes outside the buffers handed in were written");
  if (capacity) memcpy(dst, hp + o_dst, capacity);
  if (begin) memcpy(begin, hp + o_begin, E * 4);
  if (end) memcpy(end, hp + o_end, E * 4);
  *term = res.term;
  *flags = res.flags;
  return (int64_t)res.total;
}
