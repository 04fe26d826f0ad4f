// encode_device.cpp -- the encoder direction on the device: the device entropy coder's two host drivers, the per-frame coder
// (HencJob: mijpeg_encode_image(_ex|16), mijpeg_encode_coefficients_device, mijpeg_encode_batch_device) and the RAGGED ENCODE, lists
// of pictures of any shapes through one device pass (EncodePass: mijpeg_encode_ragged_plan / _device / mijpeg_encode_ragged and their
// ...16 flavours with a precision per picture), and the entry points of both.  Only what touches the device, its
// buffers on the decoder object and the stream stands here.  Frame layout and quality tables, the planner, the argument blocks of
// the forward kernels and of the coder, and a pass's arenas, tables and piece arithmetic are encode_list.hpp, which needs no device.
// What the two drivers share is stated once: the buffers are coder_layout() and output_layout() of hencode.hpp, the launches
// coder_stage_one / coder_stage_two over either argument type, the table rule codes_with_own_tables / tables_from_statistics.
// The entropy coder on the host is encoder.cpp.  Private to libmijpeg.so.
//
// A pass of the ragged encode (EncodePassLayout and the stages of EncodePass):
//   plan        per picture: frame layout, block and interval counts, its place in the pass's index spaces, its coefficient store
//   upload      ONE copy of the descriptor tables: a ForwardArgs and a HencArgs per picture, the prefix tables, the work lists
//   forward     at most six launches per precision present (forward.hip, ragged flavours) whatever the number of pictures; a list
//               that came as planes (mijpeg_encode_ragged_planar_device16): six more for its 8-bit colour pictures, whose
//               plane table goes up with the descriptors, and in front of them one interleave launch per 12-bit colour picture
//   coder       count [statistics first, for the pictures that get tables of their own -- all with `optimize`, the 12-bit ones
//               always: one read-back of their histograms, the table sets built on the host, one upload], prefix
//               sums, interval bytes, prefix sums -> read-back of the plain sizes (sync) -> layout of the plain buffer, emit,
//               0xFF counts, prefix sums -> read-back (sync) -> stuffing -> ONE download of the output arena (sync)
//   assembly    headers in front of every picture's piece, EOI behind it
// The RAGGED TRANSCODE (mijpeg_transcode_ragged_device) is the same pass with another first stage: the pictures are those
// of the object's decoded ragged batch, `forward` is ONE launch of requant_list_kernel (requant.hip) from the decode's stores into the
// pass's coefficient store, its range flags come back with the plain sizes, and a flagged picture's piece is dropped at assembly.
// Pictures that are flipped, transposed or rotated on the way (mijpeg_transcode_ragged_transformed_device) leave that launch
// for ONE of transform_list_kernel (transform.hip) over the same descriptors and flags.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>

#include "decoder.hpp"
#include "encode_list.hpp"

using namespace mij;

// ------------------------------------------------------------------------------------------------
// helpers
// ------------------------------------------------------------------------------------------------
namespace {

// A call that failed leaves nothing behind: what it produced is freed, pointers null, sizes 0 ...
void drop_streams(uint8_t **streams, size_t *sizes, int n)
{
  if (!streams || !sizes) return;
  for (int i = 0; i < n; i++) { free(streams[i]); streams[i] = nullptr; sizes[i] = 0; }
}
// ... and mijpeg_last_timing of the calls that have no phases to tell apart: the whole call
void whole_call_timing(mijpeg_decoder *d, std::chrono::steady_clock::time_point t_begin)
{
  d->timing[0] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
  d->timing[1] = d->timing[2] = d->timing[3] = 0;
}

// A finished stream in memory the client frees: headers, `ecs` bytes of entropy coded data, EOI.  ecs_src null: the caller puts
// the data there itself (a download from the device: no copy on the host in between).
int assemble_stream(const std::vector<uint8_t> &head, const uint8_t *ecs_src, size_t ecs, uint8_t **out, size_t *size)
{
  const size_t hs = head.size();
  uint8_t *s = (uint8_t *)malloc(hs + ecs + 2);
  if (!s) return MIJPEG_ERR_OUT_OF_MEMORY;
  memcpy(s, head.data(), hs);
  if (ecs_src) memcpy(s + hs, ecs_src, ecs);
  s[hs + ecs] = 0xff;
  s[hs + ecs + 1] = 0xd9;
  *out = s;
  *size = hs + ecs + 2;
  return MIJPEG_OK;
}

// ------------------------------------------------------------------------------------------------
// the device entropy coder's host side, shared by the per-frame coder (HencArgs) and the passes of a list (HencBatchArgs)
// ------------------------------------------------------------------------------------------------
// the widest categories a frame codes (encoder.cpp code_block): DC differences and AC coefficients, at precision 8 and at 12
constexpr int DC_CATEGORY_MAX_8 = 11, AC_CATEGORY_MAX_8 = 10, DC_CATEGORY_MAX_12 = 15, AC_CATEGORY_MAX_12 = 14;

// where the coefficients are a caller's: does a henc_survey histogram hold a category a frame of this precision cannot code?
bool beyond_coding_range(const uint32_t hist[4][256], int precision)
{
  const int dc_max = precision == 12 ? DC_CATEGORY_MAX_12 : DC_CATEGORY_MAX_8, ac_max = precision == 12 ? AC_CATEGORY_MAX_12 : AC_CATEGORY_MAX_8;
  bool beyond = false;
  for (int t = 0; t < 2; t++)
    for (int i = 0; i < 256; i++) beyond |= (hist[t][i] && i > dc_max) || (hist[2 + t][i] && (i & 15) > ac_max);
  return beyond;
}

// a launch of the coder: its failure under its name, or `count` more launches where a driver keeps count (`counter`, may be null)
#define LAUNCHED(d, call, what, count, counter)                          \
  do {                                                                   \
    if (const int e_ = (call)) return hip_fail(d, (hipError_t)e_, what); \
    if (counter) *(counter) += (count);                                  \
  } while (0)
struct ScanNames { const char *blocks, *intervals, *chunks; }; // what a driver calls its three scans when one fails
constexpr ScanNames FRAME_SCANS{"scan over the blocks", "scan over the intervals", "scan over the chunks"}, PASS_SCANS{"scan launch", "scan launch", "scan launch"};

// Stage one: code lengths per block, their prefix sums, bytes per interval, their prefix sums -- istart[I] is the plain stream's size.
template <class Args>
int coder_stage_one(mijpeg_decoder *d, const Args &args, uint8_t *base, const CoderLayout &l, hipStream_t stream, const ScanNames &scans, int32_t *launches)
{
  uint64_t *bitpos = (uint64_t *)(base + l.bitpos), *istart = (uint64_t *)(base + l.istart), *scratch = (uint64_t *)(base + l.scratch);
  LAUNCHED(d, henc_count(args, false, stream), "henc_count_kernel launch", 1, launches);
  LAUNCHED(d, exclusive_scan_u32((uint32_t *)(base + l.bits), bitpos, l.N, scratch, l.scratch_words, stream), scans.blocks, scan_layout(l.N).launches, launches);
  LAUNCHED(d, henc_interval_bytes(args, stream), "henc_interval_bytes_kernel launch", 1, launches);
  LAUNCHED(d, exclusive_scan_u32((uint32_t *)(base + l.ibytes), istart, l.I, scratch, l.scratch_words, stream), scans.intervals, scan_layout(l.I).launches, launches);
  return MIJPEG_OK;
}

// Stage two, once the plain sizes are known and `args` point into the arena: the zeroed plain stream, the code words into it, 0xFF
// bytes per chunk, their prefix sums -- ffstart[chunks] is what the stuffing adds --, then the stuffed stream with its markers.
// before_stuff: what a driver enqueues between the last scan and the stuffing kernel.
template <class Args, class BeforeStuff>
int coder_stage_two(mijpeg_decoder *d, const Args &args, uint8_t *base, const OutputLayout &l, hipStream_t stream, const ScanNames &scans, int32_t *launches,
                    BeforeStuff before_stuff)
{
  HIP_TRY(d, hipMemsetAsync(base + l.plain, 0, l.zeroed, stream));
  LAUNCHED(d, henc_emit(args, stream), "henc_emit_kernel launch", 1, launches);
  LAUNCHED(d, henc_count_ff(args, stream), "henc_count_ff_kernel launch", 1, launches);
  LAUNCHED(d, exclusive_scan_u32(args.ffcount, (uint64_t *)args.ffstart, l.chunks, (uint64_t *)(base + l.scratch), l.scratch_words, stream), scans.chunks,
           scan_layout(l.chunks).launches, launches);
  if (const int rc = before_stuff()) return rc;
  LAUNCHED(d, henc_stuff(args, stream), "henc_stuff_kernel launch", 1, launches);
  return MIJPEG_OK;
}

// The per-frame coder: entropy coding of one frame's coefficient planes on the device (hencode.hip) and download of the finished stream, as a
// job of three stages with a host synchronisation in front of the second and the third (the byte counts the next stage
// sizes its buffers and copies with come from the device).  Two jobs on two streams with two sets of buffers overlap:
// mijpeg_encode_batch_device keeps the next frame's first stage in flight while it waits for the current frame.
struct HencJob {
  mijpeg_decoder *d = nullptr;
  const mijpeg_info *f = nullptr;
  int slot = 0, restart_interval = 0;
  hipStream_t stream = nullptr;
  HencArgs a;
  EncTables tabs;
  uint64_t *readback = nullptr; // pinned: [0] plain bytes, [1] 0xFF bytes
  HencTables *packed = nullptr; // pinned: the slot's tables on their way up
  uint32_t chunks = 0;
  uint8_t *result = nullptr;
  size_t result_size = 0;
  std::vector<uint8_t> head;

  // geometry, buffers, tables (the picture's own cost a synchronisation of their own), then stage one.
  // check_range: the coefficients are the caller's own (mijpeg_encode_coefficients_device), not the forward kernels': the symbol
  // statistics are always taken, by the survey kernel that is safe for any int16 content, and what beyond_coding_range() finds is
  // refused before any kernel looks a code up.  One launch and one synchronisation more where the tables are the standard ones.
  int stage_a(mijpeg_decoder *dec, const mijpeg_info &info, const int16_t *coef_dev, int ri, int optimize, int slot_, hipStream_t st,
              bool check_range = false)
  {
    d = dec; f = &info; slot = slot_; stream = st; restart_interval = ri;
    memset(&a, 0, sizeof(a));
    a.coef = coef_dev;
    if (!henc_frame_geometry(a, info, ri)) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "too many blocks per MCU for the device entropy coder");
    const uint64_t nblocks = (uint64_t)a.total_mcus * (uint64_t)a.blocks_per_mcu;
    if (nblocks > HENC_SCAN_MAX) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "frame too large for the device entropy coder"); // (2^30 - 1025 blocks)
    a.total_blocks = (uint32_t)nblocks;
    a.n_intervals = (uint32_t)((a.total_mcus + a.ri - 1) / a.ri);
    // arena 1: tables, statistics, the arrays over blocks and intervals
    const CoderLayout l = coder_layout(a.total_blocks, a.n_intervals);
    Carver ar;
    const size_t o_tab = ar.take(sizeof(HencTables)), o_hist = ar.take(HENC_HIST_BYTES), o_coder = ar.take(l.end);
    int rc = ensure_dev(d, (void **)&d->henc_dev[slot], &d->henc_cap[slot], ar.at);
    if (rc) return rc;
    if (!d->henc_host) HIP_TRY(d, hipHostMalloc((void **)&d->henc_host, 64 + 2 * sizeof(HencTables), hipHostMallocDefault));
    readback = d->henc_host + 2 * slot;
    packed = (HencTables *)((uint8_t *)d->henc_host + 64 + (size_t)slot * sizeof(HencTables));
    uint8_t *base = d->henc_dev[slot];
    a.tables = (const HencTables *)(base + o_tab);
    a.hist = (uint32_t *)(base + o_hist);
    point_into(a, base + o_coder, l);
    enc_standard_tables(tabs);
    henc_pack_tables(packed, tabs);
    HIP_TRY(d, hipMemcpyAsync((void *)a.tables, packed, sizeof(*packed), hipMemcpyHostToDevice, stream));
    const bool own_tables = codes_with_own_tables(info, optimize);
    if (own_tables || check_range) { // symbol statistics first, tables from them
      HIP_TRY(d, hipMemsetAsync(a.hist, 0, HENC_HIST_BYTES, stream));
      if (const int e = check_range ? henc_survey(a, stream) : henc_count(a, true, stream)) return hip_fail(d, (hipError_t)e, "statistics kernel launch");
      uint32_t hist[4][256];
      HIP_TRY(d, hipMemcpyAsync(hist, a.hist, sizeof(hist), hipMemcpyDeviceToHost, stream));
      HIP_TRY(d, hipStreamSynchronize(stream));
      if (check_range && beyond_coding_range(hist, info.precision))
        return set_error(d, MIJPEG_ERR_OVERFLOW_PARAMETER, "coefficients outside what a frame of this precision can hold");
      if (own_tables) {
        tables_from_statistics(hist, info.components, tabs, packed);
        HIP_TRY(d, hipMemcpyAsync((void *)a.tables, packed, sizeof(*packed), hipMemcpyHostToDevice, stream));
      }
    }
    if ((rc = coder_stage_one(d, a, base + o_coder, l, stream, FRAME_SCANS, nullptr))) return rc;
    HIP_TRY(d, hipMemcpyAsync(&readback[0], a.istart + a.n_intervals, 8, hipMemcpyDeviceToHost, stream));
    return MIJPEG_OK;
  }

  // the plain size is there: arena 2, stage two
  int stage_b()
  {
    HIP_TRY(d, hipStreamSynchronize(stream));
    a.plain_bytes = readback[0];
    chunks = (uint32_t)((a.plain_bytes + HENC_STUFF_CHUNK - 1) / HENC_STUFF_CHUNK);
    const OutputLayout l = output_layout(chunks, a.n_intervals);
    int rc = ensure_dev(d, (void **)&d->henc_out_dev[slot], &d->henc_out_cap[slot], l.end);
    if (rc) return rc;
    point_into(a, d->henc_out_dev[slot], l);
    if ((rc = coder_stage_two(d, a, d->henc_out_dev[slot], l, stream, FRAME_SCANS, nullptr, [] { return MIJPEG_OK; }))) return rc;
    HIP_TRY(d, hipMemcpyAsync(&readback[1], a.ffstart + chunks, 8, hipMemcpyDeviceToHost, stream));
    return MIJPEG_OK;
  }

  // headers on the host, download of the entropy coded data straight into the stream, behind them
  int stage_c()
  {
    HIP_TRY(d, hipStreamSynchronize(stream));
    const size_t ecs = (size_t)a.plain_bytes + (size_t)readback[1] + (size_t)(a.n_intervals - 1) * 2;
    head.clear();
    enc_write_headers(head, *f, tabs, restart_interval);
    if (assemble_stream(head, nullptr, ecs, &result, &result_size)) return set_error(d, MIJPEG_ERR_OUT_OF_MEMORY, "out of memory for the stream");
    const hipError_t e = hipMemcpyAsync(result + head.size(), a.out, ecs, hipMemcpyDeviceToHost, stream);
    if (e != hipSuccess) { free(result); result = nullptr; return hip_fail(d, e, "download of the stream"); }
    return MIJPEG_OK;
  }

  int finish(uint8_t **out_stream, size_t *out_size)
  {
    const hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess) { free(result); result = nullptr; return hip_fail(d, e, "download of the stream"); }
    *out_stream = result;
    *out_size = result_size;
    result = nullptr;
    return MIJPEG_OK;
  }
};

int device_entropy_code(mijpeg_decoder *d, const mijpeg_info &f, const int16_t *coef_dev, int restart_interval, int optimize,
                               uint8_t **stream, size_t *size, bool check_range = false)
{
  HencJob job;
  int rc = job.stage_a(d, f, coef_dev, restart_interval, optimize, 0, d->stream, check_range);
  if (!rc) rc = job.stage_b();
  if (!rc) rc = job.stage_c();
  if (!rc) rc = job.finish(stream, size);
  return rc;
}

// ------------------------------------------------------------------------------------------------
// ragged encode: one pass on the device
// ------------------------------------------------------------------------------------------------
int sync_counted(mijpeg_decoder *d)
{
  HIP_TRY(d, hipStreamSynchronize(d->stream));
  d->eragged_stats.host_syncs++;
  return MIJPEG_OK;
}

// One pass of a list on the device, stage by stage (encode_pass): what is enqueued, where the host waits, what is counted.  Every
// offset, table and piece is the layout's (encode_list.hpp); only these stages touch d->eragged_* and the stream.
struct EncodePass {
  mijpeg_decoder *d;
  const EncodePassLayout &L;
  uint8_t **streams; // of the pass's first picture
  size_t *sizes;
  hipStream_t stream = d->stream;
  int32_t *launches = &d->eragged_stats.coder_launches;
  uint8_t *dev = nullptr, *host = nullptr; // the device and the pinned arena
  EncodePassArgs a;
  EncTables std_tabs; // Annex K.3: what the 8-bit pictures code with unless their tables are optimised
  std::vector<EncTables> tabs; // of the pictures with tables of their own
  std::vector<std::vector<uint8_t>> heads;
  bool timed = false; // MIJPEG_ENCODE_RAGGED_TIME_FORWARD: an event behind the forward launches (encode_passes has one in front)
  int32_t *status = nullptr; // a transcode pass: of the pass's first picture (a picture refused by its range flag gets no stream)

  // arena 1 and its pinned twin; the descriptor tables, one upload
  int descriptors_up()
  {
    int rc = ensure_dev(d, (void **)&d->eragged_dev, &d->eragged_cap, L.dev_bytes);
    if (!rc) rc = ensure_pinned(d, &d->eragged_host, &d->eragged_host_cap, L.host_bytes);
    if (rc) return rc;
    dev = d->eragged_dev;
    host = d->eragged_host;
    enc_standard_tables(std_tabs);
    a = fill_upload(host, dev, L, std_tabs);
    HIP_TRY(d, hipMemcpyAsync(dev, host, L.up_bytes, hipMemcpyHostToDevice, stream));
    return MIJPEG_OK;
  }

  int forward()
  {
    if (launch_forward_ragged(a.forward, stream, &d->eragged_stats.forward_launches)) return hip_fail(d, hipGetLastError(), "ragged forward kernel launch");
    if (timed) HIP_TRY(d, hipEventRecord(d->ev1, stream));
    return MIJPEG_OK;
  }

  // a transcode pass's first stage: the planes of all its pictures requantised (or copied, where the tables are kept) into the
  // pass's coefficient store, range-checked, ONE launch -- and ONE more for the pictures that are flipped, transposed or rotated on
  // the way; a list of them alone has no requant launch
  int requant()
  {
    if (a.requant_grid) {
      if (const int e = launch_requant_list(a.requant, a.requant_grid, stream)) return hip_fail(d, (hipError_t)e, "requant_list_kernel launch");
      d->transcode_stats.requant_launches++;
    }
    if (a.transform_grid) {
      if (const int e = launch_transform_list(a.transform, a.transform_grid, stream)) return hip_fail(d, (hipError_t)e, "transform_list_kernel launch");
      d->transform_stats.transform_launches++;
    }
    return MIJPEG_OK;
  }

  // statistics of the pictures with tables of their own, read back (sync); their tables and the repointed HencArgs up
  // (the statistics launch runs over the pass; workgroups of pictures without a histogram leave at once)
  int own_tables_up()
  {
    HIP_TRY(d, hipMemsetAsync(dev + L.d_hist, 0, L.hist_bytes, stream));
    LAUNCHED(d, henc_count(a.coder, true, stream), "henc_count_kernel launch", 1, launches);
    HIP_TRY(d, hipMemcpyAsync(host + L.h_hist, dev + L.d_hist, L.hist_bytes, hipMemcpyDeviceToHost, stream));
    if (const int rc = sync_counted(d)) return rc;
    own_tables(host, dev, L, tabs);
    HIP_TRY(d, hipMemcpyAsync(dev + L.d_tables, host + L.h_tables, (size_t)L.n_own * sizeof(HencTables), hipMemcpyHostToDevice, stream));
    HIP_TRY(d, hipMemcpyAsync(dev + L.hargs_at, host + L.hargs_at, (size_t)L.n * sizeof(HencArgs), hipMemcpyHostToDevice, stream)); // (tables now the pictures' own)
    return MIJPEG_OK;
  }

  // count, prefix sums, interval bytes, prefix sums; where every picture's plain stream begins, read back (sync)
  int plain_sizes()
  {
    if (const int rc = coder_stage_one(d, a.coder, dev + L.coder_at, L.coder, stream, PASS_SCANS, launches)) return rc;
    LAUNCHED(d, henc_gather((const uint64_t *)(dev + L.coder_at + L.coder.istart), a.coder.first_interval, (uint64_t *)(dev + L.d_gather), L.n + 1, stream),
             "henc_gather_kernel launch", 1, launches);
    HIP_TRY(d, hipMemcpyAsync(host + L.h_istart, dev + L.d_gather, ((size_t)L.n + 1) * 8, hipMemcpyDeviceToHost, stream));
    if (L.sources) // (a transcode pass: the range flags of its requant launch come back with the same wait)
      HIP_TRY(d, hipMemcpyAsync(host + L.h_flags, dev + L.rq_flags_at, (size_t)L.n * 4, hipMemcpyDeviceToHost, stream));
    return sync_counted(d);
  }

  // the plain buffer laid out, the output arena, emit to stuffing; the 0xFF bytes in front of every picture, read back (sync)
  int stuffed_sizes()
  {
    if (!chunk_layout(host, L)) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "pass too large for the device entropy coder's output arena");
    const OutputLayout ol = output_layout(chunks_of(host, L), L.I);
    int rc = ensure_dev(d, (void **)&d->eragged_out_dev, &d->eragged_out_cap, ol.end);
    if (rc) return rc;
    a.coder.total_chunks = ol.chunks;
    point_into(a.coder, d->eragged_out_dev, ol);
    HIP_TRY(d, hipMemcpyAsync(dev + L.d_first_chunk, host + L.h_first_chunk, ((size_t)L.n + 1) * 4, hipMemcpyHostToDevice, stream));
    rc = coder_stage_two(d, a.coder, d->eragged_out_dev, ol, stream, PASS_SCANS, launches, [&]() -> int { // (where every picture's piece of `out` lies)
      LAUNCHED(d, henc_gather(a.coder.ffstart, a.coder.first_chunk, (uint64_t *)(dev + L.d_gather), L.n + 1, stream), "henc_gather_kernel launch", 1, launches);
      return MIJPEG_OK;
    });
    if (rc) return rc;
    HIP_TRY(d, hipMemcpyAsync(host + L.h_ffstart, dev + L.d_gather, ((size_t)L.n + 1) * 8, hipMemcpyDeviceToHost, stream));
    return sync_counted(d);
  }

  // one download of the arena (sync); the headers are written while the copy runs
  int download()
  {
    const size_t arena = arena_bytes(host, L);
    const int rc = ensure_pinned(d, &d->eragged_down, &d->eragged_down_cap, arena + 16);
    if (rc) return rc;
    HIP_TRY(d, hipMemcpyAsync(d->eragged_down, a.coder.out, arena, hipMemcpyDeviceToHost, stream));
    heads.resize(L.n);
    for (uint32_t p = 0; p < L.n; p++)
      enc_write_headers(heads[p], L.items[p].info, L.own(p) ? tabs[L.own_index[p]] : std_tabs,
                        L.frames[p].restart_interval); // (SOF0 and 8-bit DQT, or SOF1 and the DQT width the entries need: from info)
    if (const int rc2 = sync_counted(d)) return rc2;
    d->eragged_stats.bytes_downloaded += (int64_t)arena;
    return MIJPEG_OK;
  }

  // headers in front of every picture's piece, EOI behind it
  int assemble()
  {
    for (uint32_t p = 0; p < L.n; p++) {
      if (L.sources && ((const uint32_t *)(host + L.h_flags))[p]) { // (a value outside the coding range: the clamped planes' piece is dropped)
        status[p] = MIJPEG_ERR_OVERFLOW_PARAMETER;
        continue;
      }
      const StreamPiece piece = stream_piece(host, L, p);
      if (assemble_stream(heads[p], d->eragged_down + piece.at, piece.ecs, &streams[p], &sizes[p]))
        return set_error(d, MIJPEG_ERR_OUT_OF_MEMORY, "out of memory for the stream");
    }
    return MIJPEG_OK;
  }
};

// pictures [p0, p1) of the list: one pass.  frames[i].pixels are device addresses; planes: the list's plane table where its pictures
// came as planes (PlanarList), one entry per picture
int encode_pass(mijpeg_decoder *d, const mijpeg_encode_frame *frames, const mijpeg_encode_ragged_item *items, int p0, int p1, int optimize,
                uint8_t **streams, size_t *sizes, const ForwardPlanes *planes = nullptr, bool timed = false, const RequantSource *sources = nullptr,
                int32_t *status = nullptr)
{
  const EncodePassLayout layout(frames, items, p0, p1, optimize, planes, sources);
  if (layout.error) return set_error(d, layout.error, layout.why);
  EncodePass pass{d, layout, streams + p0, sizes + p0};
  pass.timed = timed;
  pass.status = status ? status + p0 : nullptr;
  int rc = pass.descriptors_up();
  if (!rc) rc = sources ? pass.requant() : pass.forward();
  if (!rc && layout.n_own) rc = pass.own_tables_up();
  if (!rc) rc = pass.plain_sizes();
  if (!rc) rc = pass.stuffed_sizes();
  if (!rc) rc = pass.download();
  if (!rc) rc = pass.assemble();
  return rc;
}

uint32_t pass_blocks_setting()
{
  const char *e = getenv("MIJPEG_ENCODE_RAGGED_PASS_BLOCKS"); // (testing: cut small lists into several passes)
  if (!e) return 0;
  const unsigned long long v = strtoull(e, nullptr, 10);
  return (uint32_t)std::min<unsigned long long>(std::max<unsigned long long>(v, 256), PASS_BLOCKS_MAX);
}

// A list whose pictures came as component planes (mijpeg_encode_ragged_planar_device16), as the one driver takes it: per picture the
// frame its pass is laid out with and its entry of the plane table.
//   own_plane  one component: the plane is the interleaved picture
//   fused      8 bit, three components: plane 0 and the planes' pitch in the frame, planes 1 and 2 in the table
//   two_pass   12 bit, three components: the interleaved copy in d->enc_dev, made in front of the picture's pass (interleave_pass)
struct PlanarList {
  const void *const *planes; // the caller's, MIJPEG_MAX_COMPONENTS per picture
  std::vector<mijpeg_encode_frame> frames;
  std::vector<ForwardPlanes> table;

  PlanarList(const mijpeg_encode_frame *caller, const void *const *planes_, int n)
      : planes(planes_), frames(caller, caller + n), table((size_t)n, ForwardPlanes{nullptr, nullptr})
  {
    for (int i = 0; i < n; i++) frames[(size_t)i].pixels = (const uint8_t *)plane(i, 0);
  }
  const void *plane(int i, int c) const { return planes[(size_t)i * MIJPEG_MAX_COMPONENTS + c]; }
};

// what picture i of a planar list needs: its planes, a pitch that holds a line; 16-bit samples on 2-byte boundaries
bool planes_in_order(const mijpeg_encode_frame &e, int precision, const void *const *planes)
{
  const int sb = precision == 12 ? 2 : 1;
  if (e.row_stride < (int64_t)e.width * sb) return false;
  uintptr_t bits = (uintptr_t)e.row_stride;
  for (int c = 0; c < e.components; c++) {
    if (!planes[c]) return false;
    bits |= (uintptr_t)planes[c];
  }
  return sb == 1 || (bits & 1) == 0;
}

// the routes of the pictures [p0, p1) of a planar list; the two-pass pictures interleaved into d->enc_dev, ONE launch per picture, on
// the stream the pass's forward launches follow on (lines of the copy on dword boundaries: the tile and interior kernels).
// MIJPEG_ENCODE_PLANAR_TWO_PASS (testing, tools/planar_encode_bench.py): the 8-bit colour pictures take that route as well -- the
// route their planar kernels replace.
int interleave_pass(mijpeg_decoder *d, PlanarList &pl, const mijpeg_encode_ragged_item *items, int p0, int p1)
{
  const bool all_two_pass = getenv("MIJPEG_ENCODE_PLANAR_TWO_PASS") != nullptr;
  auto two_pass = [&](const mijpeg_info &f) { return f.components == 3 && (f.precision == 12 || all_two_pass); };
  auto line_of = [](const mijpeg_info &f) { return ((size_t)f.width * 3 * (f.precision == 12 ? 2 : 1) + 3) & ~(size_t)3; };
  std::vector<size_t> at((size_t)(p1 - p0), 0);
  size_t total = 0;
  for (int i = p0; i < p1; i++) {
    const mijpeg_info &f = items[(size_t)i].info;
    if (!two_pass(f)) continue;
    at[(size_t)(i - p0)] = total;
    total += (line_of(f) * (size_t)f.height + 255) & ~(size_t)255;
  }
  if (total)
    if (const int rc = ensure_dev(d, (void **)&d->enc_dev, &d->enc_cap, total)) return rc;
  for (int i = p0; i < p1; i++) {
    const mijpeg_info &f = items[(size_t)i].info;
    mijpeg_encode_frame &e = pl.frames[(size_t)i];
    if (f.components == 1) {
      d->eplanar_stats.own_plane++;
    } else if (!two_pass(f)) {
      pl.table[(size_t)i] = ForwardPlanes{(const uint8_t *)pl.plane(i, 1), (const uint8_t *)pl.plane(i, 2)};
      d->eplanar_stats.fused++;
    } else {
      InterleaveArgs a;
      memset(&a, 0, sizeof(a));
      for (int c = 0; c < 3; c++) a.src[c] = (const uint8_t *)pl.plane(i, c);
      a.src_row = e.row_stride;
      a.ncomp = 3; a.sample_bytes = f.precision == 12 ? 2 : 1;
      a.width = f.width; a.height = f.height;
      a.dst = d->enc_dev + at[(size_t)(i - p0)];
      a.dst_row = (int64_t)line_of(f);
      if (launch_interleave(a, d->stream)) return hip_fail(d, hipGetLastError(), "interleave_kernel launch");
      e.pixels = a.dst;
      e.row_stride = a.dst_row;
      d->eplanar_stats.two_pass++;
      d->eplanar_stats.interleave_launches++;
    }
  }
  return MIJPEG_OK;
}

// a planned list, pass by pass; pixels in device memory, or -- planar -- planes
int encode_passes(mijpeg_decoder *d, const mijpeg_encode_frame *frames, const mijpeg_encode_ragged_item *items, int n, int optimize, uint8_t **streams,
                  size_t *sizes, PlanarList *planar = nullptr)
{
  int rc = MIJPEG_OK;
  d->eragged_stats.pictures = n;
  // MIJPEG_ENCODE_RAGGED_TIME_FORWARD (testing, tools/planar_encode_bench.py): the device time from the first thing a pass enqueues
  // -- the interleave launches of a planar list, the upload of the descriptors -- to the end of its forward launches, between two
  // events, summed over the passes: mijpeg_last_timing [1].  Unset: no event is recorded.
  const bool timed = getenv("MIJPEG_ENCODE_RAGGED_TIME_FORWARD") != nullptr;
  d->eragged_forward_s = 0;
  for (int p0 = 0; p0 < n && !rc;) {
    int p1 = p0 + 1;
    while (p1 < n && items[(size_t)p1].pass == items[(size_t)p0].pass) p1++;
    if (timed) HIP_TRY(d, hipEventRecord(d->ev0, d->stream));
    if (planar) rc = interleave_pass(d, *planar, items, p0, p1);
    if (!rc) rc = encode_pass(d, planar ? planar->frames.data() : frames, items, p0, p1, optimize, streams, sizes, planar ? planar->table.data() : nullptr, timed);
    if (timed && !rc) { // (the pass has waited for its download: both events are behind us)
      float ms = 0;
      HIP_TRY(d, hipEventElapsedTime(&ms, d->ev0, d->ev1));
      d->eragged_forward_s += ms * 1e-3;
    }
    d->eragged_stats.passes++;
    p0 = p1;
  }
  return rc;
}

// the list, pass by pass; pixels in device memory
int encode_list(mijpeg_decoder *d, const mijpeg_encode_frame *frames, const int32_t *precision, int n, int optimize, uint8_t **streams, size_t *sizes)
{
  std::vector<mijpeg_encode_ragged_item> items((size_t)n);
  mijpeg_encode_ragged_totals totals;
  const int rc = plan_list(frames, precision, n, pass_blocks_setting(), items.data(), &totals);
  if (rc) return set_error(d, rc, "invalid picture description in the list");
  for (int i = 0; i < n; i++)
    if (!pixels_in_order(frames[i], items[(size_t)i].info.precision))
      return set_error(d, MIJPEG_ERR_INVALID_PARAMETER,
                       "picture without pixels, with a row stride below its width, or with 16-bit samples off their 2-byte boundaries");
  return encode_passes(d, frames, items.data(), n, optimize, streams, sizes);
}

// the planar entry: everything is checked for every picture before anything is launched, written or counted
int encode_planar_entry(mijpeg_decoder *d, const mijpeg_encode_frame *frames, const void *const *planes, const int32_t *precision, int n, int optimize,
                        uint32_t flags, uint8_t **streams, size_t *sizes)
{
  if (streams && sizes)
    for (int i = 0; i < n; i++) { streams[i] = nullptr; sizes[i] = 0; }
  if (!d || !frames || !planes || !streams || !sizes || n < 1 || flags != 0) return MIJPEG_ERR_INVALID_PARAMETER;
  std::vector<mijpeg_encode_ragged_item> items((size_t)n);
  mijpeg_encode_ragged_totals totals;
  if (const int rc = plan_list(frames, precision, n, pass_blocks_setting(), items.data(), &totals)) return set_error(d, rc, "invalid picture description in the list");
  for (int i = 0; i < n; i++)
    if (!planes_in_order(frames[i], items[(size_t)i].info.precision, planes + (size_t)i * MIJPEG_MAX_COMPONENTS))
      return set_error(d, MIJPEG_ERR_INVALID_PARAMETER,
                       "picture without one of its planes, with a pitch below its width, or with 16-bit samples off their 2-byte boundaries");
  if (d->device < 0) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "decoder was created without a device");
  HIP_TRY(d, hipSetDevice(d->device));
  const auto t_begin = std::chrono::steady_clock::now();
  d->eragged_stats = mijpeg_encode_ragged_stats{};
  d->eragged_forward_s = 0;
  d->eplanar_stats = mijpeg_encode_planar_stats{};
  d->eplanar_stats.pictures = n;
  PlanarList list(frames, planes, n);
  const int rc = encode_passes(d, frames, items.data(), n, optimize, streams, sizes, &list);
  if (rc) {
    (void)hipStreamSynchronize(d->stream);
    drop_streams(streams, sizes, n);
  }
  whole_call_timing(d, t_begin);
  d->timing[1] = d->eragged_forward_s;
  return rc;
}

int encode_entry(mijpeg_decoder *d, const mijpeg_encode_frame *frames, const int32_t *precision, int n, int optimize, uint32_t flags, uint8_t **streams,
                 size_t *sizes, bool host_pixels)
{
  if (!d || !frames || !streams || !sizes || n < 1 || flags != 0) return MIJPEG_ERR_INVALID_PARAMETER;
  for (int i = 0; i < n; i++) { streams[i] = nullptr; sizes[i] = 0; }
  if (d->device < 0) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "decoder was created without a device");
  HIP_TRY(d, hipSetDevice(d->device));
  const auto t_begin = std::chrono::steady_clock::now();
  d->eragged_stats = mijpeg_encode_ragged_stats{};
  d->eragged_forward_s = 0;
  int rc = MIJPEG_OK;
  std::vector<mijpeg_encode_frame> on_device;
  if (host_pixels) {
    // gather into pinned staging (the workers share the pictures), one upload, then the device path on the copies
    quiesce(d); // (a batch that was submitted and not waited for may still read the staging area)
    std::vector<size_t> off((size_t)n + 1, 0);
    for (int i = 0; i < n && !rc; i++) {
      const mijpeg_encode_frame &e = frames[i];
      const int pr = precision_of(precision, i);
      if (!shape_in_order(pr, e.components, e.width, e.height) || !pixels_in_order(e, pr))
        rc = set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "invalid picture description in the list");
      else
        off[(size_t)i + 1] = (off[(size_t)i] + (size_t)e.row_stride * (size_t)e.height + 255) & ~(size_t)255;
    }
    const size_t total = off[(size_t)n];
    if (!rc) rc = ensure_dev(d, (void **)&d->enc_dev, &d->enc_cap, total + 256);
    if (!rc) rc = ensure_pinned(d, &d->stage_host, &d->stage_cap, total + 256);
    if (!rc) {
      const int workers = std::max(1, std::min(std::min(default_threads(), 16), n));
      parallel_for(workers, [&](int w) {
        for (int i = w; i < n; i += workers) memcpy(d->stage_host + off[(size_t)i], frames[i].pixels, (size_t)frames[i].row_stride * (size_t)frames[i].height);
      });
      const hipError_t e = hipMemcpyAsync(d->enc_dev, d->stage_host, total, hipMemcpyHostToDevice, d->stream);
      if (e != hipSuccess) rc = hip_fail(d, e, "upload of the pictures");
      on_device.assign(frames, frames + n);
      for (int i = 0; i < n; i++) on_device[(size_t)i].pixels = d->enc_dev + off[(size_t)i]; // (256-byte aligned: 16-bit samples stay on their boundaries)
      frames = on_device.data();
    }
  }
  if (!rc) rc = encode_list(d, frames, precision, n, optimize, streams, sizes);
  if (rc) {
    (void)hipStreamSynchronize(d->stream);
    drop_streams(streams, sizes, n);
  }
  whole_call_timing(d, t_begin);
  d->timing[1] = d->eragged_forward_s;
  return rc;
}

// ------------------------------------------------------------------------------------------------
// ragged transcode (include/mijpeg.h): the pictures of the object's decoded ragged batch, coded again from their planes
// ------------------------------------------------------------------------------------------------
// The planes of a picture of the single-image route, on the device and at rest: the child decoded on its own stream (a host decode
// sent its planes up behind it), and this object's stream is about to read them.  Per child: a wait, and the upload where none was made
int child_planes(mijpeg_decoder *d, mijpeg_decoder *c, const mijpeg_info &f, const int16_t **planes)
{
  if (!c->uploaded) {
    int rc = ensure_coef_store(c, (size_t)f.coef_count, true);
    if (!rc && hipMemcpyAsync(c->coef_dev, c->coef_host, (size_t)f.coef_count * sizeof(int16_t), hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = MIJPEG_ERR_DEVICE;
    if (rc) return set_error(d, rc, "upload of a child's coefficient planes");
    c->uploaded = true;
  }
  if (!c->host_planes_stale) d->transcode_stats.child_uploads++;
  quiesce(c);
  *planes = c->coef_dev;
  return MIJPEG_OK;
}

int transcode_entry(mijpeg_decoder *d, const mijpeg_transcode_spec *specs, const int32_t *transforms, int optimize, uint32_t flags, uint8_t **streams, size_t *sizes,
                    int32_t *status)
{
  if (!d || !streams || !sizes || !status || flags != 0) return MIJPEG_ERR_INVALID_PARAMETER;
  const int n = d->ragged_n;
  for (int i = 0; i < n; i++) { streams[i] = nullptr; sizes[i] = 0; status[i] = MIJPEG_OK; }
  for (int i = 0; transforms && i < n; i++)
    if (!transform_in_order(transforms[i]))
      return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "transform " + std::to_string(i) + ": one of MIJPEG_TRANSFORM_NONE .. ROT_270, with or without MIJPEG_TRANSFORM_TRIM");
  for (int i = 0; specs && i < n; i++)
    if (!transcode_spec_in_order(specs[i]))
      return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "transcode spec " + std::to_string(i) + ": quality is 1 .. 100, KEEP or SKIP, restart_interval 0 .. 65535 or -1");
  if (d->device < 0) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "decoder was created without a device");
  if (n < 1) return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "no decoded ragged batch: call mijpeg_decode_ragged_device first");
  HIP_TRY(d, hipSetDevice(d->device));
  const auto t_begin = std::chrono::steady_clock::now();
  mijpeg_transcode_ragged_stats &stats = d->transcode_stats;
  stats = mijpeg_transcode_ragged_stats{};
  stats.pictures = n;
  mijpeg_transcode_transform_stats &tstats = d->transform_stats;
  tstats = mijpeg_transcode_transform_stats{};
  // the plan: who is served, every served picture's output frame and its place in the passes
  const mijpeg_transcode_spec keep{MIJPEG_TRANSCODE_KEEP, -1};
  std::vector<int> picture; // of served slot k
  std::vector<mijpeg_encode_frame> frames;
  std::vector<mijpeg_encode_ragged_item> items;
  std::vector<RequantSource> sources;
  std::vector<char> kept, trimmed;
  mijpeg_encode_ragged_totals totals;
  memset(&totals, 0, sizeof(totals));
  const uint32_t pass_blocks = pass_blocks_setting();
  PassCutter cut{pass_blocks ? pass_blocks : PASS_BLOCKS_DEFAULT};
  int rc = MIJPEG_OK;
  for (int i = 0; i < n && !rc; i++) {
    const mijpeg_decoder::RaggedImage &r = d->ragged[(size_t)i];
    const mijpeg_transcode_spec &spec = specs ? specs[i] : keep;
    if (r.status) { status[i] = r.status; continue; }
    if (spec.quality == MIJPEG_TRANSCODE_SKIP) continue;
    if (r.group < 0 && !(r.child && r.child->decoded)) { status[i] = MIJPEG_ERR_NOT_AVAILABLE; continue; }
    mijpeg_encode_ragged_item it;
    memset(&it, 0, sizeof(it));
    int ri = 0;
    bool keeps = false;
    TransformPlan how;
    if ((status[i] = transcode_plan_one(r.info, spec, it.info, ri, keeps, it.blocks, it.intervals, transforms ? transforms[i] : MIJPEG_TRANSFORM_NONE, &how))) {
      tstats.geometry_refusals += how.geometry;
      continue;
    }
    RequantSource src{r.info, d->coef_dev + r.coef_base, how.bits};
    if (r.group < 0) {
      if ((rc = child_planes(d, r.child, r.info, &src.planes))) break;
      stats.children++;
    }
    mijpeg_encode_frame e;
    memset(&e, 0, sizeof(e));
    e.width = it.info.width; e.height = it.info.height; e.components = it.info.components;
    for (int c = 0; c < MIJPEG_MAX_COMPONENTS; c++) { e.hsamp[c] = it.info.hsamp[c]; e.vsamp[c] = it.info.vsamp[c]; }
    e.quality = spec.quality;
    e.restart_interval = ri;
    cut.place(it, &totals);
    picture.push_back(i);
    frames.push_back(e);
    items.push_back(it);
    sources.push_back(src);
    kept.push_back(keeps);
    trimmed.push_back(how.trimmed);
  }
  // the passes: an encode pass each, its first stage the requant launch (the counters of the last ragged encode stay that call's)
  const int m = (int)picture.size();
  std::vector<uint8_t *> out((size_t)m, nullptr);
  std::vector<size_t> out_size((size_t)m, 0);
  std::vector<int32_t> out_status((size_t)m, MIJPEG_OK);
  const mijpeg_encode_ragged_stats encode_stats = d->eragged_stats;
  d->eragged_stats = mijpeg_encode_ragged_stats{};
  for (int p0 = 0; p0 < m && !rc;) {
    int p1 = p0 + 1;
    while (p1 < m && items[(size_t)p1].pass == items[(size_t)p0].pass) p1++;
    rc = encode_pass(d, frames.data(), items.data(), p0, p1, optimize, out.data(), out_size.data(), nullptr, false, sources.data(), out_status.data());
    stats.passes++;
    p0 = p1;
  }
  stats.coder_launches = d->eragged_stats.coder_launches;
  stats.host_syncs = d->eragged_stats.host_syncs;
  stats.bytes_downloaded = d->eragged_stats.bytes_downloaded;
  d->eragged_stats = encode_stats;
  if (rc) {
    (void)hipStreamSynchronize(d->stream);
    drop_streams(out.data(), out_size.data(), m);
    for (int i = 0; i < n; i++) status[i] = MIJPEG_OK;
  } else {
    for (int k = 0; k < m; k++) {
      const int i = picture[(size_t)k];
      streams[i] = out[(size_t)k];
      sizes[i] = out_size[(size_t)k];
      status[i] = out_status[(size_t)k];
      if (streams[i]) {
        stats.served++;
        stats.kept += kept[(size_t)k];
        tstats.transformed += sources[(size_t)k].transform != 0;
        tstats.trimmed += trimmed[(size_t)k];
      }
    }
    for (int i = 0; i < n; i++) stats.refused += status[i] != MIJPEG_OK;
  }
  whole_call_timing(d, t_begin);
  return rc;
}

} // namespace

extern "C" {

int mijpeg_transcode_ragged_device(mijpeg_decoder *d, const mijpeg_transcode_spec *specs, int optimize, uint32_t flags, uint8_t **streams, size_t *sizes,
                                   int32_t *status)
try {
  return transcode_entry(d, specs, nullptr, optimize, flags, streams, sizes, status);
} catch (...) {
  if (d) drop_streams(streams, sizes, d->ragged_n);
  return boundary_catch(d, "mijpeg_transcode_ragged_device");
}

int mijpeg_transcode_ragged_transformed_device(mijpeg_decoder *d, const mijpeg_transcode_spec *specs, const int32_t *transforms, int optimize, uint32_t flags,
                                               uint8_t **streams, size_t *sizes, int32_t *status)
try {
  return transcode_entry(d, specs, transforms, optimize, flags, streams, sizes, status);
} catch (...) {
  if (d) drop_streams(streams, sizes, d->ragged_n);
  return boundary_catch(d, "mijpeg_transcode_ragged_transformed_device");
}

int mijpeg_transcode_transform_stats_get(mijpeg_decoder *d, mijpeg_transcode_transform_stats *out)
try {
  if (!d || !out) return MIJPEG_ERR_INVALID_PARAMETER;
  *out = d->transform_stats;
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_transcode_transform_stats_get"); }

int mijpeg_transcode_plan_transformed(const mijpeg_info *source, const mijpeg_transcode_spec *spec, int32_t transform, mijpeg_info *out, int32_t *restart_interval,
                                      int32_t *kept)
try {
  if (out) memset(out, 0, sizeof(*out));
  if (restart_interval) *restart_interval = 0;
  if (kept) *kept = 0;
  if (!source || !spec || !out || !restart_interval || !kept || !transcode_spec_in_order(*spec) || !transform_in_order(transform)) return MIJPEG_ERR_INVALID_PARAMETER;
  if (spec->quality == MIJPEG_TRANSCODE_SKIP) return MIJPEG_OK;
  int ri = 0;
  bool keeps = false;
  uint32_t blocks = 0, intervals = 0;
  const int rc = transcode_plan_one(*source, *spec, *out, ri, keeps, blocks, intervals, transform);
  if (rc) return rc;
  *restart_interval = ri;
  *kept = keeps;
  return MIJPEG_OK;
} catch (...) { return boundary_catch(nullptr, "mijpeg_transcode_plan_transformed"); }

int64_t mijpeg_transform_blocks(const int16_t *src, int32_t src_bw, int32_t src_bh, int16_t *dst, int32_t dst_bw, int32_t dst_bh, int32_t transform,
                                const uint16_t q_old[64], const uint16_t q_new[64], int precision)
try {
  if (!src || !dst || src == dst || src_bw < 1 || src_bh < 1 || dst_bw < 1 || dst_bh < 1 || transform < 0 || transform > MIJPEG_TRANSFORM_ROT_270 || !q_old || !q_new ||
      (precision != 8 && precision != 12))
    return MIJPEG_ERR_INVALID_PARAMETER;
  for (int k = 0; k < 64; k++)
    if (!q_old[k] || !q_new[k]) return MIJPEG_ERR_INVALID_PARAMETER;
  return transform_blocks(src, src_bw, src_bh, dst, dst_bw, dst_bh, transform_bits(transform), q_old, q_new, precision);
} catch (...) { return boundary_catch(nullptr, "mijpeg_transform_blocks"); }

int mijpeg_transcode_ragged_stats_get(mijpeg_decoder *d, mijpeg_transcode_ragged_stats *out)
try {
  if (!d || !out) return MIJPEG_ERR_INVALID_PARAMETER;
  *out = d->transcode_stats;
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_transcode_ragged_stats_get"); }

int mijpeg_transcode_plan(const mijpeg_info *source, const mijpeg_transcode_spec *spec, mijpeg_info *out, int32_t *restart_interval, int32_t *kept)
try {
  if (out) memset(out, 0, sizeof(*out));
  if (restart_interval) *restart_interval = 0;
  if (kept) *kept = 0;
  if (!source || !spec || !out || !restart_interval || !kept || !transcode_spec_in_order(*spec)) return MIJPEG_ERR_INVALID_PARAMETER;
  if (spec->quality == MIJPEG_TRANSCODE_SKIP) return MIJPEG_OK;
  int ri = 0;
  bool keeps = false;
  uint32_t blocks = 0, intervals = 0;
  const int rc = transcode_plan_one(*source, *spec, *out, ri, keeps, blocks, intervals);
  if (rc) return rc;
  *restart_interval = ri;
  *kept = keeps;
  return MIJPEG_OK;
} catch (...) { return boundary_catch(nullptr, "mijpeg_transcode_plan"); }

int64_t mijpeg_requantize(const int16_t *src, int16_t *dst, int64_t n, const uint16_t q_old[64], const uint16_t q_new[64], int precision)
try {
  if (!src || !dst || n < 0 || !q_old || !q_new || (precision != 8 && precision != 12)) return MIJPEG_ERR_INVALID_PARAMETER;
  for (int k = 0; k < 64; k++)
    if (!q_old[k] || !q_new[k]) return MIJPEG_ERR_INVALID_PARAMETER;
  return requantize_blocks(src, dst, n, q_old, q_new, precision);
} catch (...) { return boundary_catch(nullptr, "mijpeg_requantize"); }

int mijpeg_frame_layout(mijpeg_info *f)
try {
  return frame_layout_of(f);
} catch (...) { return boundary_catch(nullptr, "mijpeg_frame_layout"); }

int mijpeg_launch_forward(const mijpeg_forward_batch *b, void *stream)
try {
  ForwardArgs a;
  if (const int rc = forward_args_of(b, a)) return rc;
  return launch_forward(a, b->info.precision, (hipStream_t)stream) ? MIJPEG_ERR_DEVICE : MIJPEG_OK;
} catch (...) { return boundary_catch(nullptr, "mijpeg_launch_forward"); }

void mijpeg_quality_tables(int quality, uint16_t luma[64], uint16_t chroma[64])
try {
  quality_tables_of(quality, 255, luma, chroma);
} catch (...) { (void)boundary_catch(nullptr, "mijpeg_quality_tables"); }

int mijpeg_encode_batch_device(mijpeg_decoder *d, const mijpeg_forward_batch *b, int restart_interval, int optimize, uint8_t **streams, size_t *sizes)
try {
  if (!d || !b || !streams || !sizes || b->frames < 1 || restart_interval < 0 || restart_interval > 65535) return MIJPEG_ERR_INVALID_PARAMETER;
  if (d->device < 0) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "decoder was created without a device");
  HIP_TRY(d, hipSetDevice(d->device));
  for (int f = 0; f < b->frames; f++) { streams[f] = nullptr; sizes[f] = 0; }
  const auto t_begin = std::chrono::steady_clock::now();
  int rc = mijpeg_launch_forward(b, d->stream);
  if (rc) return set_error(d, rc, "forward kernel launch failed");
  // frame f on stream f & 1 with buffer set f & 1: while the host waits for one frame's byte counts and download, the
  // other frame's kernels run
  if (!d->copy_stream) HIP_TRY(d, hipStreamCreateWithFlags(&d->copy_stream, hipStreamNonBlocking));
  HIP_TRY(d, hipEventRecord(d->ev0, d->stream));
  HIP_TRY(d, hipStreamWaitEvent(d->copy_stream, d->ev0, 0));
  hipStream_t st[2] = {d->stream, d->copy_stream};
  HencJob jobs[2];
  auto coef_of = [&](int f) { return b->coef_dev + (int64_t)f * b->coef_frame_stride; };
  rc = jobs[0].stage_a(d, b->info, coef_of(0), restart_interval, optimize, 0, st[0]);
  for (int f = 0; f < b->frames && !rc; f++) {
    HencJob &cur = jobs[f & 1], &nxt = jobs[(f + 1) & 1];
    if (f + 1 < b->frames) rc = nxt.stage_a(d, b->info, coef_of(f + 1), restart_interval, optimize, (f + 1) & 1, st[(f + 1) & 1]);
    if (!rc) rc = cur.stage_b();
    if (!rc) rc = cur.stage_c();
    if (!rc) rc = cur.finish(&streams[f], &sizes[f]);
  }
  (void)hipStreamSynchronize(d->copy_stream);
  (void)hipStreamSynchronize(d->stream);
  if (rc) drop_streams(streams, sizes, b->frames);
  whole_call_timing(d, t_begin);
  return rc;
} catch (...) { return boundary_catch(d, "mijpeg_encode_batch_device"); }

int mijpeg_encode_coefficients_device(mijpeg_decoder *d, const mijpeg_info *info, const int16_t *coef_dev, int restart_interval, int optimize,
                                      uint8_t **stream, size_t *size)
try {
  // (the checks and codes of mijpeg_encode_coefficients, then HencJob::stage_a's, before anything touches a device)
  if (!d || !info || !coef_dev || !stream || !size || restart_interval < 0 || restart_interval > 65535) return MIJPEG_ERR_INVALID_PARAMETER;
  *stream = nullptr;
  *size = 0;
  const mijpeg_info &f = *info;
  if ((f.precision != 8 && f.precision != 12) || (f.components != 1 && f.components != 3))
    return set_error(d, MIJPEG_ERR_OPERATION_UNIMPLEMENTED, "the entropy coder takes 8-bit and 12-bit frames of one or three components");
  // (a zeroed or hand-built info: the geometry helper divides by subx / suby and multiplies the MCU counts as ints)
  bool laid_out = f.mcus_x >= 1 && f.mcus_y >= 1 && (int64_t)f.mcus_x * f.mcus_y <= INT32_MAX;
  for (int c = 0; c < f.components; c++) laid_out = laid_out && f.subx[c] >= 1 && f.suby[c] >= 1 && f.hsamp[c] >= 1 && f.vsamp[c] >= 1 && f.blocks_w[c] >= 1;
  if (!laid_out) return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "frame without a layout (mijpeg_frame_layout)");
  HencArgs geometry;
  memset(&geometry, 0, sizeof(geometry));
  if (!henc_frame_geometry(geometry, f, restart_interval)) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "too many blocks per MCU for the device entropy coder");
  if ((uint64_t)geometry.total_mcus * (uint64_t)geometry.blocks_per_mcu > HENC_SCAN_MAX) // (2^30 blocks or more, and the 1024 counts below)
    return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "frame too large for the device entropy coder");
  if (d->device < 0) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "decoder was created without a device");
  HIP_TRY(d, hipSetDevice(d->device));
  const auto t_begin = std::chrono::steady_clock::now();
  int rc = device_entropy_code(d, f, coef_dev, restart_interval, optimize, stream, size, true);
  if (rc) {
    (void)hipStreamSynchronize(d->stream);
    drop_streams(stream, size, 1);
  }
  whole_call_timing(d, t_begin);
  return rc;
} catch (...) { return boundary_catch(d, "mijpeg_encode_coefficients_device"); }

int mijpeg_encode_image(mijpeg_decoder *d, const uint8_t *pixels, int32_t width, int32_t height, int32_t components, int64_t row_stride,
                        int quality, const int32_t *hsamp, const int32_t *vsamp, int restart_interval, int optimize, uint8_t **stream, size_t *size)
try {
  return mijpeg_encode_image_ex(d, pixels, width, height, components, row_stride, quality, hsamp, vsamp, restart_interval, optimize, 0, stream, size);
} catch (...) { return boundary_catch(d, "mijpeg_encode_image"); }

// the body of mijpeg_encode_image_ex and mijpeg_encode_image16: `pixels` are 8-bit samples or, precision 12, uint16_t samples
static int encode_image_of(mijpeg_decoder *d, const uint8_t *pixels, int32_t width, int32_t height, int32_t components, int64_t row_stride,
                           int precision, int quality, const int32_t *hsamp, const int32_t *vsamp, int restart_interval, int optimize, uint32_t flags,
                           uint8_t **stream, size_t *size)
{
  using clk = std::chrono::steady_clock;
  const auto t_begin = clk::now();
  // (width and height are mijpeg_frame_layout's to refuse, below and under its own message)
  if (!d || !pixels || !stream || !size || (components != 1 && components != 3) || !line_fits(precision, components, width, row_stride)) return MIJPEG_ERR_INVALID_PARAMETER;
  if (d->device < 0) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "decoder was created without a device");
  HIP_TRY(d, hipSetDevice(d->device));
  mijpeg_forward_batch b;
  memset(&b, 0, sizeof(b));
  mijpeg_info &f = b.info;
  int rc = picture_info_of(width, height, components, hsamp, vsamp, quality, f, precision);
  if (rc) return set_error(d, rc, "invalid frame layout for encoding");
  const size_t px_bytes = (size_t)row_stride * (size_t)height, coef_bytes = (size_t)f.coef_count * sizeof(int16_t);
  rc = ensure_dev(d, (void **)&d->enc_dev, &d->enc_cap, px_bytes + 256 + coef_bytes);
  if (rc) return rc;
  int16_t *coef_dev = (int16_t *)(d->enc_dev + ((px_bytes + 255) & ~(size_t)255));
  // pinned staging: [pixels][coefficients].  The picture goes up in bands, each gathered into pinned memory by the pool
  // threads while the DMA of the previous band runs; the coefficients come down into pinned memory the coder reads.
  const size_t stage_bytes = ((px_bytes + 255) & ~(size_t)255) + coef_bytes;
  rc = ensure_pinned(d, &d->stage_host, &d->stage_cap, stage_bytes);
  if (rc) return rc;
  int16_t *coef_host = (int16_t *)(d->stage_host + ((px_bytes + 255) & ~(size_t)255));
  {
    const size_t band = std::max<size_t>((size_t)8 << 20, (px_bytes + 7) / 8) & ~(size_t)255;
    for (size_t b0 = 0; b0 < px_bytes; b0 += band) {
      const size_t len = std::min(band, px_bytes - b0);
      const size_t pieces = (len + ((size_t)1 << 20) - 1) >> 20;
      const int workers = (int)std::min<size_t>(pieces, (size_t)std::min(default_threads(), 16));
      parallel_for(workers, [&](int w) {
        for (size_t k = (size_t)w; k < pieces; k += (size_t)workers) {
          const size_t o = b0 + (k << 20), n = std::min<size_t>((size_t)1 << 20, b0 + len - o);
          memcpy(d->stage_host + o, pixels + o, n);
        }
      });
      HIP_TRY(d, hipMemcpyAsync(d->enc_dev + b0, d->stage_host + b0, len, hipMemcpyHostToDevice, d->stream));
    }
  }
  b.pixels_dev = d->enc_dev;
  b.pixel_row_stride = row_stride;
  b.pixel_frame_stride = (int64_t)px_bytes;
  b.coef_dev = coef_dev;
  b.coef_frame_stride = f.coef_count;
  b.frames = 1;
  const auto t_up = clk::now(); // uploads enqueued (the gathering is synchronous)
  rc = mijpeg_launch_forward(&b, d->stream);
  if (rc) return set_error(d, rc, "forward kernel launch failed");
  static const bool env_host_coder = getenv("MIJPEG_ENTROPY_CODER") && !strcmp(getenv("MIJPEG_ENTROPY_CODER"), "host");
  if (!(flags & MIJPEG_ENCODE_HOST_CODER) && !env_host_coder) {
    if (restart_interval < 0 || restart_interval > 65535) return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "invalid restart interval");
    rc = device_entropy_code(d, f, coef_dev, restart_interval, optimize, stream, size);
    d->timing[0] = std::chrono::duration<double>(t_up - t_begin).count();
    d->timing[1] = std::chrono::duration<double>(clk::now() - t_up).count(); // kernels, entropy coder and download of the stream
    d->timing[2] = d->timing[3] = 0;
    if (rc != MIJPEG_ERR_NOT_AVAILABLE) return rc;
  }
  HIP_TRY(d, hipStreamSynchronize(d->stream));
  const auto t_kernel = clk::now();
  HIP_TRY(d, hipMemcpyAsync(coef_host, coef_dev, coef_bytes, hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(d, hipStreamSynchronize(d->stream));
  const auto t_down = clk::now();
  rc = mijpeg_encode_coefficients(&f, coef_host, restart_interval, optimize, 0, stream, size);
  // mijpeg_last_timing: gather + upload, kernels (incl. the rest of the upload), download, entropy coder
  d->timing[0] = std::chrono::duration<double>(t_up - t_begin).count();
  d->timing[1] = std::chrono::duration<double>(t_kernel - t_up).count();
  d->timing[2] = std::chrono::duration<double>(t_down - t_kernel).count();
  d->timing[3] = std::chrono::duration<double>(clk::now() - t_down).count();
  if (rc) return set_error(d, rc, "entropy coding failed");
  return MIJPEG_OK;
}

int mijpeg_encode_image_ex(mijpeg_decoder *d, const uint8_t *pixels, int32_t width, int32_t height, int32_t components, int64_t row_stride,
                           int quality, const int32_t *hsamp, const int32_t *vsamp, int restart_interval, int optimize, uint32_t flags,
                           uint8_t **stream, size_t *size)
try {
  return encode_image_of(d, pixels, width, height, components, row_stride, 8, quality, hsamp, vsamp, restart_interval, optimize, flags, stream, size);
} catch (...) { return boundary_catch(d, "mijpeg_encode_image_ex"); }

int mijpeg_encode_image16(mijpeg_decoder *d, const uint16_t *pixels, int32_t width, int32_t height, int32_t components, int64_t row_stride,
                          int precision, int quality, const int32_t *hsamp, const int32_t *vsamp, int restart_interval, uint32_t flags,
                          uint8_t **stream, size_t *size)
try {
  if (precision != 12 || (row_stride & 1) || ((uintptr_t)pixels & 1) || (flags & ~MIJPEG_ENCODE_HOST_CODER)) return MIJPEG_ERR_INVALID_PARAMETER;
  return encode_image_of(d, (const uint8_t *)pixels, width, height, components, row_stride, 12, quality, hsamp, vsamp, restart_interval, 1, flags, stream, size);
} catch (...) { return boundary_catch(d, "mijpeg_encode_image16"); }

int mijpeg_encode_ragged_plan16(const mijpeg_encode_frame *frames, const int32_t *precision, int n, uint32_t pass_blocks,
                                mijpeg_encode_ragged_item *items, mijpeg_encode_ragged_totals *totals)
try {
  return plan_list(frames, precision, n, pass_blocks, items, totals);
} catch (...) { return boundary_catch(nullptr, "mijpeg_encode_ragged_plan16"); }

int mijpeg_encode_ragged_device16(mijpeg_decoder *d, const mijpeg_encode_frame *frames, const int32_t *precision, int n, int optimize, uint32_t flags,
                                  uint8_t **streams, size_t *sizes)
try {
  return encode_entry(d, frames, precision, n, optimize, flags, streams, sizes, false);
} catch (...) {
  drop_streams(streams, sizes, n);
  return boundary_catch(d, "mijpeg_encode_ragged_device16");
}

int mijpeg_encode_ragged16(mijpeg_decoder *d, const mijpeg_encode_frame *frames, const int32_t *precision, int n, int optimize, uint32_t flags,
                           uint8_t **streams, size_t *sizes)
try {
  return encode_entry(d, frames, precision, n, optimize, flags, streams, sizes, true);
} catch (...) {
  drop_streams(streams, sizes, n);
  return boundary_catch(d, "mijpeg_encode_ragged16");
}

int mijpeg_encode_ragged_planar_device16(mijpeg_decoder *d, const mijpeg_encode_frame *frames, const void *const *planes, const int32_t *precision, int n,
                                         int optimize, uint32_t flags, uint8_t **streams, size_t *sizes)
try {
  return encode_planar_entry(d, frames, planes, precision, n, optimize, flags, streams, sizes);
} catch (...) {
  drop_streams(streams, sizes, n);
  return boundary_catch(d, "mijpeg_encode_ragged_planar_device16");
}

int mijpeg_encode_planar_stats_get(mijpeg_decoder *d, mijpeg_encode_planar_stats *out)
try {
  if (!d || !out) return MIJPEG_ERR_INVALID_PARAMETER;
  *out = d->eplanar_stats;
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_encode_planar_stats_get"); }

int mijpeg_interleave_device(mijpeg_decoder *d, const void *const planes[MIJPEG_MAX_COMPONENTS], int64_t plane_row_stride, int32_t width, int32_t height,
                             int32_t components, int32_t sample_bytes, void *dst_device, int64_t dst_row_stride, int sync)
try {
  if (!d || !dst_device || !planes || width < 1 || height < 1 || components < 1 || components > MIJPEG_MAX_COMPONENTS || (sample_bytes != 1 && sample_bytes != 2))
    return MIJPEG_ERR_INVALID_PARAMETER;
  for (int c = 0; c < components; c++)
    if (!planes[c]) return MIJPEG_ERR_INVALID_PARAMETER;
  if (plane_row_stride < (int64_t)width * sample_bytes || dst_row_stride < (int64_t)width * sample_bytes * components) return MIJPEG_ERR_INVALID_PARAMETER;
  if (d->device < 0) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "decoder was created without a device");
  HIP_TRY(d, hipSetDevice(d->device));
  InterleaveArgs a;
  memset(&a, 0, sizeof(a));
  for (int c = 0; c < components; c++) a.src[c] = (const uint8_t *)planes[c];
  a.src_row = plane_row_stride;
  a.ncomp = components; a.sample_bytes = sample_bytes;
  a.width = width; a.height = height;
  a.dst = (uint8_t *)dst_device;
  a.dst_row = dst_row_stride;
  if (launch_interleave(a, d->stream)) return hip_fail(d, hipGetLastError(), "interleave_kernel launch");
  if (sync) HIP_TRY(d, hipStreamSynchronize(d->stream));
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_interleave_device"); }

// the 8-bit entry points: the same calls without a precision array
int mijpeg_encode_ragged_plan(const mijpeg_encode_frame *frames, int n, uint32_t pass_blocks, mijpeg_encode_ragged_item *items,
                              mijpeg_encode_ragged_totals *totals)
{
  return mijpeg_encode_ragged_plan16(frames, nullptr, n, pass_blocks, items, totals);
}

int mijpeg_encode_ragged_device(mijpeg_decoder *d, const mijpeg_encode_frame *frames, int n, int optimize, uint32_t flags, uint8_t **streams,
                                size_t *sizes)
{
  return mijpeg_encode_ragged_device16(d, frames, nullptr, n, optimize, flags, streams, sizes);
}

int mijpeg_encode_ragged(mijpeg_decoder *d, const mijpeg_encode_frame *frames, int n, int optimize, uint32_t flags, uint8_t **streams, size_t *sizes)
{
  return mijpeg_encode_ragged16(d, frames, nullptr, n, optimize, flags, streams, sizes);
}

int mijpeg_encode_ragged_get_stats(mijpeg_decoder *d, mijpeg_encode_ragged_stats *out)
try {
  if (!d || !out) return MIJPEG_ERR_INVALID_PARAMETER;
  *out = d->eragged_stats;
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_encode_ragged_get_stats"); }

} // extern "C"
