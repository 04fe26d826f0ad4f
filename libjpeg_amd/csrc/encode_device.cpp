// encode_device.cpp -- the encoder direction on the device: frame layout and quality tables, the argument blocks of the forward
// kernels and of the device entropy coder, and that coder's two host drivers: the per-frame coder (HencJob: mijpeg_encode_image(_ex|16),
// mijpeg_encode_coefficients_device, mijpeg_encode_batch_device) and the RAGGED ENCODE, lists of pictures of any shapes through one
// device pass (mijpeg_encode_ragged_plan / _device / mijpeg_encode_ragged and their ...16 flavours with a precision per picture;
// DESIGN 4.3b).  What the two drivers share is stated once: the buffers are coder_layout() and output_layout() of hencode.hpp, the
// launches coder_stage_one / coder_stage_two over either argument type, the table rule codes_with_own_tables / tables_from_statistics.
// The entropy coder on the host is encoder.cpp.  Private to libmijpeg.so.
//
// A pass of the ragged encode:
//   plan        per picture: frame layout, block and interval counts, its place in the pass's index spaces, its coefficient store
//   upload      ONE copy of the descriptor tables: a ForwardArgs and a HencArgs per picture, the prefix tables, the work lists
//   forward     at most six launches per precision present (forward.hip, ragged flavours) whatever the number of pictures
//   coder       count [statistics first, for the pictures that get tables of their own -- all with `optimize`, the 12-bit ones
//               always: one read-back of their histograms, the table sets built on the host, one upload], prefix
//               sums, interval bytes, prefix sums -> read-back of the plain sizes (sync) -> layout of the plain buffer, emit,
//               0xFF counts, prefix sums -> read-back (sync) -> stuffing -> ONE download of the output arena (sync)
//   assembly    headers in front of every picture's piece, EOI behind it
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>

#include "decoder.hpp"
#include "encoder.hpp"
#include "forward.hpp"
#include "hencode.hpp"

using namespace mij;

// ------------------------------------------------------------------------------------------------
// argument blocks
// ------------------------------------------------------------------------------------------------
// the forward kernels' argument block for a batch (geometry, routing, quantiser multipliers): MIJPEG_OK or the refusal
static int forward_args_of(const mijpeg_forward_batch *b, ForwardArgs &a)
{
  if (!b || !b->pixels_dev || !b->coef_dev || b->frames < 1) return MIJPEG_ERR_INVALID_PARAMETER;
  const mijpeg_info &f = b->info;
  if ((f.precision != 8 && f.precision != 12) || (f.components != 1 && f.components != 3) || f.xt) return MIJPEG_ERR_OPERATION_UNIMPLEMENTED;
  // precision 12: 16-bit samples, every line on a 2-byte boundary
  if (f.precision == 12 && (((uintptr_t)b->pixels_dev | (uintptr_t)b->pixel_frame_stride | (uintptr_t)b->pixel_row_stride) & 1)) return MIJPEG_ERR_INVALID_PARAMETER;
  memset(&a, 0, sizeof(a));
  a.pixels = b->pixels_dev;
  a.pixel_frame_stride = b->pixel_frame_stride;
  a.pixel_row_stride = b->pixel_row_stride;
  a.coef = b->coef_dev;
  a.coef_frame_stride = b->coef_frame_stride;
  a.width = f.width;
  a.height = f.height;
  a.ncomp = f.components;
  a.ycbcr = f.ycbcr;
  a.frames = b->frames;
  // (the interior and tile kernels read lines as dwords, 16 bytes at a time at precision 12: with 2-byte samples too the
  // condition is that every line starts on a dword boundary -- a block's first pixel is 24 or 48 bytes into its line)
  const bool dword_lines = (((uintptr_t)b->pixels_dev | (uintptr_t)b->pixel_frame_stride | (uintptr_t)b->pixel_row_stride) & 3) == 0;
  uint64_t blocks = 0;
  for (int c = 0; c < f.components; c++) {
    if (f.subx[c] < 1 || f.suby[c] < 1 || f.blocks_w[c] < 1 || f.blocks_h[c] < 1) return MIJPEG_ERR_INVALID_PARAMETER;
    a.subx[c] = f.subx[c];
    a.suby[c] = f.suby[c];
    a.bw[c] = f.blocks_w[c];
    a.bh[c] = f.blocks_h[c];
    a.nbx[c] = ((f.width + f.subx[c] - 1) / f.subx[c] + 7) >> 3;
    a.nby[c] = ((f.height + f.suby[c] - 1) / f.suby[c] + 7) >> 3;
    a.coef_off[c] = f.coef_offset[c];
    a.fast[c] = dword_lines && f.components == 3 && f.ycbcr && f.subx[c] <= 2 && f.suby[c] <= 2 && !getenv("MIJPEG_FORWARD_SLOW");
    a.fast_nbx[c] = f.width / (8 * f.subx[c]);
    a.fast_nby[c] = f.height / (8 * f.suby[c]);
    a.first_block[c] = (uint32_t)blocks;
    blocks += (uint64_t)f.blocks_w[c] * f.blocks_h[c];
    for (int i = 0; i < 64; i++) {
      const uint16_t delta = f.quant[f.quant_index[c]][i];
      if (delta == 0) return MIJPEG_ERR_INVALID_PARAMETER;
      // LONG(FLOAT(1L << QUANTIZER_BITS) / delta + 0.5), dct/idct.cpp:106: a single precision quotient
      volatile float q = (float)(1L << 30) / (float)delta;
      a.invq[c][i] = (int32_t)((double)q + 0.5);
    }
  }
  if (blocks > 0xffffffffull) return MIJPEG_ERR_INVALID_PARAMETER;
  a.first_block[f.components] = (uint32_t)blocks;
  if (a.fast[0] && a.fast[1] && a.fast[2] && f.subx[0] == 1 && f.suby[0] == 1 && f.subx[1] == 2 && f.suby[1] == 2 && f.subx[2] == 2 && f.suby[2] == 2 &&
      f.width >= 128 && f.height >= 128 && !getenv("MIJPEG_FORWARD_NO_TILES")) {
    a.tiled420 = 1;
    const int tx = f.width >> 7, ty = f.height >> 7;
    a.tile_nbx[0] = tx * 16; a.tile_nby[0] = ty * 16;
    for (int c = 1; c < 3; c++) { a.tile_nbx[c] = tx * 8; a.tile_nby[c] = ty * 8; }
  }
  return MIJPEG_OK;
}

// MCU structure and plane geometry of a frame for the device entropy coder (ri: MCUs per interval, 0 = none); false: more than
// 64 blocks per MCU
static bool henc_frame_geometry(HencArgs &a, const mijpeg_info &info, int ri)
{
  const int nc = info.components;
  a.ncomp = nc;
  a.mcus_x = info.mcus_x;
  a.total_mcus = info.mcus_x * info.mcus_y;
  a.ri = ri ? ri : a.total_mcus;
  int B = 0;
  for (int c = 0; c < nc; c++) {
    a.hs[c] = nc > 1 ? info.hsamp[c] : 1;
    a.vs[c] = nc > 1 ? info.vsamp[c] : 1;
    a.bw[c] = info.blocks_w[c];
    a.nbx[c] = ((info.width + info.subx[c] - 1) / info.subx[c] + 7) >> 3;
    a.nby[c] = ((info.height + info.suby[c] - 1) / info.suby[c] + 7) >> 3;
    a.coef_off[c] = info.coef_offset[c];
    for (int by = 0; by < a.vs[c]; by++)
      for (int bx = 0; bx < a.hs[c]; bx++) {
        if (B >= 64) return false;
        a.blk_comp[B] = (uint8_t)c;
        a.blk_bx[B] = (uint8_t)bx;
        a.blk_by[B] = (uint8_t)by;
        B++;
      }
  }
  a.blocks_per_mcu = B;
  return true;
}

static void henc_pack_tables(HencTables *h, const EncTables &t)
{
  memset(h, 0, sizeof(*h));
  for (int k = 0; k < 2; k++) {
    for (int i = 0; i < 16; i++) { h->dc_code[k][i] = t.dc[k].code[i]; h->dc_len[k][i] = t.dc[k].len[i]; }
    for (int i = 0; i < 256; i++) { h->ac_code[k][i] = t.ac[k].code[i]; h->ac_len[k][i] = t.ac[k].len[i]; }
  }
}

// ------------------------------------------------------------------------------------------------
// helpers
// ------------------------------------------------------------------------------------------------
namespace {

struct Carver { // lays regions out in a buffer, 256-byte aligned
  size_t at = 0;
  size_t take(size_t bytes)
  {
    const size_t o = at;
    at += henc_aligned(bytes);
    return o;
  }
};

// What the entry points ask of a picture before they look further: 8 or 12 bits, one or three components, width and height in
// 1..65535 ...
bool shape_in_order(int precision, int components, int64_t width, int64_t height)
{
  return (precision == 8 || precision == 12) && (components == 1 || components == 3) && width >= 1 && width <= 65535 && height >= 1 && height <= 65535;
}
// ... and a row stride (bytes) that holds a line of it
bool line_fits(int precision, int components, int64_t width, int64_t row_stride) { return row_stride >= width * components * (precision == 12 ? 2 : 1); }

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

// The frame of a picture to encode: its layout and the tables of its quality (hsamp, vsamp: null = 1 x 1 throughout).  What
// mijpeg_frame_layout says to it.
// Quantization::InitDefaultTables (marker/quantization.cpp:275-466) with the default (Annex K) matrices, natural order: entries
// limited to `limit` -- 255 in 8-bit frames (:456-459: "the table entries shall be byte-sized"), 32767 at precision 12 (:446-447),
// where low qualities give 16-bit DQT entries (tests/golden/enc12: q 2)
void quality_tables_of(int quality, int limit, uint16_t luma[64], uint16_t chroma[64])
{
  // ISO/IEC 10918-1 Annex K.1 / K.2 matrices, natural order
  static const uint8_t K1[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
                                 14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
  static const uint8_t K2[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
  quality = std::min(100, std::max(1, quality));
  const int scale = quality < 50 ? 5000 / quality : 200 - quality * 2; // quantization.cpp:296-299
  for (int j = 0; j < 64; j++) {
    luma[j] = (uint16_t)std::min(limit, std::max(1, (K1[j] * scale + 50) / 100)); // :411, :443-466
    chroma[j] = (uint16_t)std::min(limit, std::max(1, (K2[j] * scale + 50) / 100));
  }
}

int picture_info_of(int32_t width, int32_t height, int32_t components, const int32_t *hsamp, const int32_t *vsamp, int quality, mijpeg_info &f,
                    int precision = 8)
{
  memset(&f, 0, sizeof(f));
  f.width = width;
  f.height = height;
  f.components = components;
  f.precision = precision;
  f.ycbcr = components == 3 ? 1 : 0;
  for (int c = 0; c < components; c++) {
    f.hsamp[c] = hsamp ? hsamp[c] : 1;
    f.vsamp[c] = vsamp ? vsamp[c] : 1;
    // the reference encoder defines a luma and a chroma table but its frame header selects table 0 for every component
    // (what its own files show: tests/test_encoder.py::test_quality_tables_are_the_reference_encoders), so that is
    // what reproduces its coefficients
    f.quant_index[c] = 0;
  }
  quality_tables_of(quality, precision == 12 ? 32767 : 255, f.quant[0], f.quant[1]);
  return mijpeg_frame_layout(&f);
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
constexpr size_t HENC_HIST_BYTES = 4 * 256 * sizeof(uint32_t); // a picture's symbol statistics: HencArgs::hist
// the widest categories a frame codes (encoder.cpp code_block): DC differences and AC coefficients, at precision 8 and at 12
constexpr int DC_CATEGORY_MAX_8 = 11, AC_CATEGORY_MAX_8 = 10, DC_CATEGORY_MAX_12 = 15, AC_CATEGORY_MAX_12 = 14;

// Huffman tables from the picture's own statistics: with `optimize`, and always at precision 12, where the Annex K.3 tables have
// no codes for categories 12..15.  (Coefficients the forward kernels make of 8-bit pixels always have a code in the standard
// tables, at most 11 / 10 bits, the host coder's check; of 12-bit pixels at most 15 / 14 bits, which tables of their own cover.)
bool codes_with_own_tables(const mijpeg_info &f, int optimize) { return optimize || f.precision == 12; }

// ... and where the coefficients are a caller's: does a henc_survey histogram hold a category a frame of this precision cannot code?
bool beyond_coding_range(const uint32_t hist[4][256], int precision)
{
  const int dc_max = precision == 12 ? DC_CATEGORY_MAX_12 : DC_CATEGORY_MAX_8, ac_max = precision == 12 ? AC_CATEGORY_MAX_12 : AC_CATEGORY_MAX_8;
  bool beyond = false;
  for (int t = 0; t < 2; t++)
    for (int i = 0; i < 256; i++) beyond |= (hist[t][i] && i > dc_max) || (hist[2 + t][i] && (i & 15) > ac_max);
  return beyond;
}

// histogram of a picture -> its tables (Annex K.2; a single component: one pair) -> as the kernels read them
void tables_from_statistics(const uint32_t hist[4][256], int components, EncTables &t, HencTables *packed)
{
  enc_standard_tables(t);
  enc_optimal_tables(t, hist, hist + 2, components > 1 ? 2 : 1);
  henc_pack_tables(packed, t);
}

// a picture's view of the arrays of coder_layout() at `base`: from its first block and first interval
void point_into(HencArgs &a, uint8_t *base, const CoderLayout &l, uint32_t first_block = 0, uint32_t first_interval = 0)
{
  a.bits = (uint32_t *)(base + l.bits) + first_block;
  a.bitpos = (const uint64_t *)(base + l.bitpos) + first_block;
  a.ibytes = (uint32_t *)(base + l.ibytes) + first_interval;
  a.istart = (const uint64_t *)(base + l.istart) + first_interval;
}
// the arena of output_layout() at `base`: a frame's or a pass's
template <class Args> void point_into(Args &a, uint8_t *base, const OutputLayout &l)
{
  a.plain = (uint32_t *)(base + l.plain);
  a.ffcount = (uint32_t *)(base + l.ffcount);
  a.ffstart = (const uint64_t *)(base + l.ffstart);
  a.out = base + l.out;
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
// ragged encode: the planner
// ------------------------------------------------------------------------------------------------
constexpr uint32_t PASS_BLOCKS_DEFAULT = 1u << 24; // 2 GiB of coefficients at most
constexpr uint32_t PASS_BLOCKS_MAX = 1u << 30;     // exclusive_scan_u32's reach

uint32_t pad256(uint32_t x) { return (x + 255u) & ~255u; }

// one picture's description -> its frame (layout, tables of its quality at its precision), blocks and intervals; MIJPEG_OK or
// INVALID_PARAMETER
int plan_one(const mijpeg_encode_frame &e, int precision, mijpeg_info &f, uint32_t &blocks, uint32_t &intervals)
{
  if (!shape_in_order(precision, e.components, e.width, e.height) || e.restart_interval < 0 || e.restart_interval > 65535) return MIJPEG_ERR_INVALID_PARAMETER;
  int per_mcu = 0;
  for (int c = 0; c < e.components; c++) {
    if (e.hsamp[c] < 1 || e.hsamp[c] > 4 || e.vsamp[c] < 1 || e.vsamp[c] > 4) return MIJPEG_ERR_INVALID_PARAMETER;
    per_mcu += e.components > 1 ? e.hsamp[c] * e.vsamp[c] : 1;
  }
  if (per_mcu > 64) return MIJPEG_ERR_INVALID_PARAMETER;
  if (picture_info_of(e.width, e.height, e.components, e.hsamp, e.vsamp, e.quality, f, precision)) return MIJPEG_ERR_INVALID_PARAMETER;
  const uint64_t mcus = (uint64_t)f.mcus_x * (uint64_t)f.mcus_y, nb = mcus * (uint64_t)per_mcu;
  if (nb >= PASS_BLOCKS_MAX) return MIJPEG_ERR_INVALID_PARAMETER;
  blocks = (uint32_t)nb;
  const uint64_t ri = e.restart_interval ? (uint64_t)e.restart_interval : mcus;
  intervals = (uint32_t)((mcus + ri - 1) / ri);
  return MIJPEG_OK;
}

// precision of picture i of a list: the array's entry, 8 without an array
int precision_of(const int32_t *precision, int i) { return precision ? precision[i] : 8; }

// (blocks, intervals, index spaces, pass cuts and coefficient bases do not depend on the precision: coefficients are int16 either way)
int plan_list(const mijpeg_encode_frame *frames, const int32_t *precision, int n, uint32_t pass_blocks, mijpeg_encode_ragged_item *items,
              mijpeg_encode_ragged_totals *totals)
{
  if (!frames || !items || !totals || n < 1 || pass_blocks > PASS_BLOCKS_MAX) return MIJPEG_ERR_INVALID_PARAMETER;
  if (pass_blocks == 0) pass_blocks = PASS_BLOCKS_DEFAULT;
  memset(totals, 0, sizeof(*totals));
  int pass = 0;
  uint64_t at_block = 0, at_interval = 0;
  int64_t at_coef = 0;
  for (int i = 0; i < n; i++) {
    mijpeg_encode_ragged_item &it = items[i];
    memset(&it, 0, sizeof(it));
    if (const int rc = plan_one(frames[i], precision_of(precision, i), it.info, it.blocks, it.intervals)) return rc;
    const uint32_t padded = pad256(it.blocks);
    if (at_block > 0 && at_block + padded > pass_blocks) { // (a picture beyond the limit is a pass of its own)
      pass++;
      at_block = at_interval = 0;
      at_coef = 0;
    }
    it.pass = pass;
    it.first_block = (uint32_t)at_block;
    it.first_interval = (uint32_t)at_interval;
    it.coef_base = at_coef;
    at_block += padded;
    at_interval += it.intervals;
    at_coef += (it.info.coef_count + 127) & ~(int64_t)127; // stores start on 256-byte boundaries
    totals->blocks += padded;
    totals->intervals += it.intervals;
    totals->coef_count = std::max(totals->coef_count, at_coef);
  }
  totals->passes = pass + 1;
  return MIJPEG_OK;
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

// pictures [p0, p1) of the list: one pass.  frames[i].pixels are device addresses.
int encode_pass(mijpeg_decoder *d, const mijpeg_encode_frame *frames, const mijpeg_encode_ragged_item *items, int p0, int p1, int optimize,
                uint8_t **streams, size_t *sizes)
{
  const uint32_t n = (uint32_t)(p1 - p0);
  const mijpeg_encode_ragged_item &last = items[p1 - 1];
  const uint32_t N = last.first_block + pad256(last.blocks), I = last.first_interval + last.intervals;
  const int64_t coef_total = last.coef_base + ((last.info.coef_count + 127) & ~(int64_t)127);
  hipStream_t stream = d->stream;

  // ---- the forward kernels' work lists (routing: launch_forward's, per picture)
  std::vector<ForwardArgs> fargs(n);
  std::vector<uint32_t> wl_first[FORWARD_RAGGED_LISTS], wl_item[FORWARD_RAGGED_LISTS]; // per precision and kernel family
  // own_index: the place of a picture that codes with tables of its own in the histogram and table arenas
  std::vector<uint32_t> own_index(n, UINT32_MAX);
  uint32_t n_own = 0;
  for (uint32_t p = 0; p < n; p++) {
    if (codes_with_own_tables(items[p0 + p].info, optimize)) own_index[p] = n_own++;
    const mijpeg_encode_frame &e = frames[p0 + p];
    mijpeg_forward_batch b;
    memset(&b, 0, sizeof(b));
    b.info = items[p0 + p].info;
    b.pixels_dev = e.pixels;
    b.pixel_row_stride = e.row_stride;
    b.pixel_frame_stride = e.row_stride * (int64_t)e.height;
    b.coef_dev = (int16_t *)16; // (placed below, once the store's address is known)
    b.coef_frame_stride = b.info.coef_count;
    b.frames = 1;
    if (const int rc = forward_args_of(&b, fargs[p])) return set_error(d, rc, "invalid frame for the forward kernels");
    int which[5], comp[5];
    uint32_t wgs[5];
    const int k = forward_ragged_items(fargs[p], which, wgs, comp);
    for (int j = 0; j < k; j++) {
      const int l = forward_ragged_list(which[j], b.info.precision);
      std::vector<uint32_t> &first = wl_first[l];
      const uint64_t at = first.empty() ? 0 : first.back();
      if (first.empty()) first.push_back(0);
      if (at + wgs[j] > 0x7fffffffull) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "pass too large for one forward launch");
      first.push_back((uint32_t)(at + wgs[j])); // (entry k: first workgroup of item k; the grid behind the last)
      wl_item[l].push_back(p * 4u + (uint32_t)comp[j]);
    }
  }

  // ---- arena 1: descriptor tables (one upload), coder arrays, coefficient store
  Carver up; // the part that is uploaded in one piece: same offsets in the pinned buffer and on the device
  const size_t o_fargs = up.take((size_t)n * sizeof(ForwardArgs));
  const size_t o_hargs = up.take((size_t)n * sizeof(HencArgs));
  const size_t o_fblock = up.take(((size_t)n + 1) * 4);
  const size_t o_fint = up.take(((size_t)n + 1) * 4);
  size_t o_wl_first[FORWARD_RAGGED_LISTS], o_wl_item[FORWARD_RAGGED_LISTS];
  for (int l = 0; l < FORWARD_RAGGED_LISTS; l++) {
    o_wl_first[l] = up.take(wl_first[l].size() * 4);
    o_wl_item[l] = up.take(wl_item[l].size() * 4);
  }
  const size_t o_stdtab = up.take(sizeof(HencTables));
  const size_t up_bytes = up.at;
  Carver dv = up; // device only (or uploaded / read back later)
  const size_t o_fchunk = dv.take(((size_t)n + 1) * 4);
  const size_t hist_bytes = (size_t)n_own * HENC_HIST_BYTES; // (the arenas hold the pictures that use them)
  const size_t o_tabs = dv.take((size_t)n_own * sizeof(HencTables));
  const size_t o_hist = dv.take(hist_bytes);
  const size_t o_gather = dv.take(((size_t)n + 1) * 8);
  const CoderLayout cl = coder_layout(N, I);
  const size_t o_coder = dv.take(cl.end);
  const size_t o_coef = dv.take((size_t)coef_total * sizeof(int16_t));
  int rc = ensure_dev(d, (void **)&d->eragged_dev, &d->eragged_cap, dv.at);
  if (rc) return rc;
  // pinned: the upload, then what comes back or goes up later
  Carver hp = up;
  const size_t h_fchunk = hp.take(((size_t)n + 1) * 4);
  const size_t h_tabs = hp.take((size_t)n_own * sizeof(HencTables));
  const size_t h_hist = hp.take(hist_bytes);
  const size_t h_istart = hp.take(((size_t)n + 1) * 8);
  const size_t h_ffs = hp.take(((size_t)n + 1) * 8);
  rc = ensure_pinned(d, &d->eragged_host, &d->eragged_host_cap, hp.at);
  if (rc) return rc;
  uint8_t *dev = d->eragged_dev, *host = d->eragged_host;
  int16_t *coef = (int16_t *)(dev + o_coef);

  // ---- fill the tables
  EncTables std_tabs; // Annex K.3: what the 8-bit pictures code with unless their tables are optimised
  std::vector<EncTables> tabs(n_own);
  enc_standard_tables(std_tabs);
  henc_pack_tables((HencTables *)(host + o_stdtab), std_tabs);
  ForwardArgs *hf = (ForwardArgs *)(host + o_fargs);
  HencArgs *hh = (HencArgs *)(host + o_hargs);
  uint32_t *h_first_block = (uint32_t *)(host + o_fblock), *h_first_int = (uint32_t *)(host + o_fint);
  for (uint32_t p = 0; p < n; p++) {
    const mijpeg_encode_ragged_item &it = items[p0 + p];
    fargs[p].coef = coef + it.coef_base;
    hf[p] = fargs[p];
    HencArgs &a = hh[p];
    memset(&a, 0, sizeof(a));
    if (!henc_frame_geometry(a, it.info, frames[p0 + p].restart_interval)) return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "too many blocks per MCU");
    a.coef = coef + it.coef_base;
    // statistics are counted with the standard tables' lengths (any would do), the real pass with the picture's own
    a.tables = (const HencTables *)(dev + o_stdtab);
    a.total_blocks = it.blocks;
    a.n_intervals = it.intervals;
    point_into(a, dev + o_coder, cl, it.first_block, it.first_interval);
    a.hist = own_index[p] != UINT32_MAX ? (uint32_t *)(dev + o_hist) + (size_t)own_index[p] * 4 * 256 : nullptr;
    h_first_block[p] = it.first_block;
    h_first_int[p] = it.first_interval;
  }
  h_first_block[n] = N;
  h_first_int[n] = I;
  ForwardRaggedPlan plan;
  memset(&plan, 0, sizeof(plan));
  for (int l = 0; l < FORWARD_RAGGED_LISTS; l++) {
    if (wl_item[l].empty()) continue;
    memcpy(host + o_wl_first[l], wl_first[l].data(), wl_first[l].size() * 4);
    memcpy(host + o_wl_item[l], wl_item[l].data(), wl_item[l].size() * 4);
    plan.launch[l].pics = (const ForwardArgs *)(dev + o_fargs);
    plan.launch[l].first_wg = (const uint32_t *)(dev + o_wl_first[l]);
    plan.launch[l].item = (const uint32_t *)(dev + o_wl_item[l]);
    plan.launch[l].items = (uint32_t)wl_item[l].size();
    plan.grid[l] = wl_first[l].back();
  }
  HIP_TRY(d, hipMemcpyAsync(dev, host, up_bytes, hipMemcpyHostToDevice, stream));

  // ---- forward kernels
  if (launch_forward_ragged(plan, stream, &d->eragged_stats.forward_launches)) return hip_fail(d, hipGetLastError(), "ragged forward kernel launch");

  // ---- coder: count, prefix sums, plain sizes
  HencBatchArgs b;
  memset(&b, 0, sizeof(b));
  b.pics = (const HencArgs *)(dev + o_hargs);
  b.first_block = (const uint32_t *)(dev + o_fblock);
  b.first_interval = (const uint32_t *)(dev + o_fint);
  b.first_chunk = (const uint32_t *)(dev + o_fchunk);
  b.n = n;
  b.total_blocks = N;
  b.total_intervals = I;
  int32_t *launches = &d->eragged_stats.coder_launches;
  if (n_own) { // (the statistics launch runs over the pass; workgroups of pictures without a histogram leave at once)
    HIP_TRY(d, hipMemsetAsync(dev + o_hist, 0, hist_bytes, stream));
    LAUNCHED(d, henc_count(b, true, stream), "henc_count_kernel launch", 1, launches);
    HIP_TRY(d, hipMemcpyAsync(host + h_hist, dev + o_hist, hist_bytes, hipMemcpyDeviceToHost, stream));
    if ((rc = sync_counted(d))) return rc;
    HencTables *ht = (HencTables *)(host + h_tabs);
    for (uint32_t p = 0; p < n; p++) {
      const uint32_t o = own_index[p];
      if (o == UINT32_MAX) continue;
      tables_from_statistics((const uint32_t(*)[256])(host + h_hist) + (size_t)o * 4, items[p0 + p].info.components, tabs[o], ht + o);
      hh[p].tables = (const HencTables *)(dev + o_tabs) + o;
    }
    HIP_TRY(d, hipMemcpyAsync(dev + o_tabs, ht, (size_t)n_own * sizeof(HencTables), hipMemcpyHostToDevice, stream));
    HIP_TRY(d, hipMemcpyAsync(dev + o_hargs, hh, (size_t)n * sizeof(HencArgs), hipMemcpyHostToDevice, stream)); // (tables now the pictures' own)
  }
  if ((rc = coder_stage_one(d, b, dev + o_coder, cl, stream, PASS_SCANS, launches))) return rc;
  LAUNCHED(d, henc_gather((const uint64_t *)(dev + o_coder + cl.istart), b.first_interval, (uint64_t *)(dev + o_gather), n + 1, stream), "henc_gather_kernel launch", 1, launches);
  HIP_TRY(d, hipMemcpyAsync(host + h_istart, dev + o_gather, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, stream));
  if ((rc = sync_counted(d))) return rc;

  // ---- layout of the plain buffer: every picture on a chunk boundary
  const uint64_t *g_istart = (const uint64_t *)(host + h_istart);
  uint32_t *h_first_chunk = (uint32_t *)(host + h_fchunk);
  uint64_t chunks = 0;
  for (uint32_t p = 0; p < n; p++) {
    h_first_chunk[p] = (uint32_t)chunks;
    chunks += (g_istart[p + 1] - g_istart[p] + HENC_STUFF_CHUNK - 1) / HENC_STUFF_CHUNK;
    if (chunks >= PASS_BLOCKS_MAX) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "pass too large for the device entropy coder's output arena");
  }
  h_first_chunk[n] = (uint32_t)chunks;
  const size_t plain_total = (size_t)chunks * HENC_STUFF_CHUNK;
  const OutputLayout ol = output_layout((uint32_t)chunks, I);
  rc = ensure_dev(d, (void **)&d->eragged_out_dev, &d->eragged_out_cap, ol.end);
  if (rc) return rc;
  b.total_chunks = ol.chunks;
  point_into(b, d->eragged_out_dev, ol);
  HIP_TRY(d, hipMemcpyAsync(dev + o_fchunk, h_first_chunk, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, stream));
  rc = coder_stage_two(d, b, d->eragged_out_dev, ol, stream, PASS_SCANS, launches, [&]() -> int { // (where every picture's piece of `out` lies)
    LAUNCHED(d, henc_gather(b.ffstart, b.first_chunk, (uint64_t *)(dev + o_gather), n + 1, stream), "henc_gather_kernel launch", 1, launches);
    return MIJPEG_OK;
  });
  if (rc) return rc;
  HIP_TRY(d, hipMemcpyAsync(host + h_ffs, dev + o_gather, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, stream));
  if ((rc = sync_counted(d))) return rc;

  // ---- one download of the arena, then the streams
  const uint64_t *g_ffs = (const uint64_t *)(host + h_ffs);
  const size_t arena = plain_total + (size_t)g_ffs[n] + 2 * ((size_t)I - n);
  rc = ensure_pinned(d, &d->eragged_down, &d->eragged_down_cap, arena + 16);
  if (rc) return rc;
  HIP_TRY(d, hipMemcpyAsync(d->eragged_down, b.out, arena, hipMemcpyDeviceToHost, stream));
  std::vector<std::vector<uint8_t>> heads(n); // (the headers are written while the copy runs)
  for (uint32_t p = 0; p < n; p++)
    enc_write_headers(heads[p], items[p0 + p].info, own_index[p] != UINT32_MAX ? tabs[own_index[p]] : std_tabs,
                      frames[p0 + p].restart_interval); // (SOF0 and 8-bit DQT, or SOF1 and the DQT width the entries need: from info)
  if ((rc = sync_counted(d))) return rc;
  d->eragged_stats.bytes_downloaded += (int64_t)arena;
  for (uint32_t p = 0; p < n; p++) {
    const mijpeg_encode_ragged_item &it = items[p0 + p];
    const size_t at = (size_t)h_first_chunk[p] * HENC_STUFF_CHUNK + (size_t)g_ffs[p] + 2 * ((size_t)it.first_interval - p);
    const size_t ecs = (size_t)(g_istart[p + 1] - g_istart[p]) + (size_t)(g_ffs[p + 1] - g_ffs[p]) + 2 * ((size_t)it.intervals - 1);
    if (assemble_stream(heads[p], d->eragged_down + at, ecs, &streams[p0 + p], &sizes[p0 + p]))
      return set_error(d, MIJPEG_ERR_OUT_OF_MEMORY, "out of memory for the stream");
  }
  return MIJPEG_OK;
}

uint32_t pass_blocks_setting()
{
  const char *e = getenv("MIJPEG_ENCODE_RAGGED_PASS_BLOCKS"); // (testing: cut small lists into several passes)
  if (!e) return 0;
  const unsigned long long v = strtoull(e, nullptr, 10);
  return (uint32_t)std::min<unsigned long long>(std::max<unsigned long long>(v, 256), PASS_BLOCKS_MAX);
}

// pixels, and a row stride that holds a line; 16-bit samples: address and stride on 2-byte boundaries
bool pixels_in_order(const mijpeg_encode_frame &e, int precision)
{
  if (!e.pixels || !line_fits(precision, e.components, e.width, e.row_stride)) return false;
  return precision != 12 || (((uintptr_t)e.pixels | (uintptr_t)e.row_stride) & 1) == 0;
}

// the list, pass by pass; pixels in device memory
int encode_list(mijpeg_decoder *d, const mijpeg_encode_frame *frames, const int32_t *precision, int n, int optimize, uint8_t **streams, size_t *sizes)
{
  std::vector<mijpeg_encode_ragged_item> items((size_t)n);
  mijpeg_encode_ragged_totals totals;
  int rc = plan_list(frames, precision, n, pass_blocks_setting(), items.data(), &totals);
  if (rc) return set_error(d, rc, "invalid picture description in the list");
  for (int i = 0; i < n; i++)
    if (!pixels_in_order(frames[i], items[(size_t)i].info.precision))
      return set_error(d, MIJPEG_ERR_INVALID_PARAMETER,
                       "picture without pixels, with a row stride below its width, or with 16-bit samples off their 2-byte boundaries");
  d->eragged_stats.pictures = n;
  for (int p0 = 0; p0 < n && !rc;) {
    int p1 = p0 + 1;
    while (p1 < n && items[(size_t)p1].pass == items[(size_t)p0].pass) p1++;
    rc = encode_pass(d, frames, items.data(), p0, p1, optimize, streams, sizes);
    d->eragged_stats.passes++;
    p0 = p1;
  }
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
  return rc;
}

} // namespace

extern "C" {

int mijpeg_frame_layout(mijpeg_info *f)
try {
  if (!f || f->width < 1 || f->height < 1 || f->width > 65535 || f->height > 65535 || f->components < 1 || f->components > MIJPEG_MAX_COMPONENTS ||
      (f->precision != 8 && f->precision != 12))
    return MIJPEG_ERR_INVALID_PARAMETER;
  int hmax = 1, vmax = 1;
  for (int c = 0; c < f->components; c++) {
    if (f->hsamp[c] < 1 || f->hsamp[c] > 4 || f->vsamp[c] < 1 || f->vsamp[c] > 4 || f->quant_index[c] < 0 || f->quant_index[c] > 3)
      return MIJPEG_ERR_INVALID_PARAMETER;
    hmax = std::max(hmax, f->hsamp[c]);
    vmax = std::max(vmax, f->vsamp[c]);
  }
  f->mcus_x = (f->width + 8 * hmax - 1) / (8 * hmax);
  f->mcus_y = (f->height + 8 * vmax - 1) / (8 * vmax);
  int64_t off = 0;
  for (int c = 0; c < f->components; c++) {
    if (hmax % f->hsamp[c] || vmax % f->vsamp[c]) return MIJPEG_ERR_INVALID_PARAMETER; // fractional subsampling factors
    f->subx[c] = hmax / f->hsamp[c];
    f->suby[c] = vmax / f->vsamp[c];
    f->blocks_w[c] = f->mcus_x * f->hsamp[c];
    f->blocks_h[c] = f->mcus_y * f->vsamp[c];
    f->coef_offset[c] = off;
    off += (int64_t)f->blocks_w[c] * f->blocks_h[c] * 64;
  }
  f->coef_count = off;
  f->sample_bytes = f->precision == 12 ? 2 : 1;
  return MIJPEG_OK;
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
