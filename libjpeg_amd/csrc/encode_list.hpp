// encode_list.hpp -- the encoder direction's host half that needs no device: the frame of a picture to encode (layout,
// tables of its quality), the planner of the ragged encode, the argument blocks of the forward kernels and of the device entropy
// coder, and a pass of a list as plain data: what is in it (EncodePassLayout: index spaces, work lists, every offset of its three
// arenas), what the one upload holds (fill_upload), the tables the pictures' own statistics give (own_tables), where the pictures
// lie in the plain buffer (chunk_layout) and in the downloaded arena (arena_bytes, stream_piece).  A list that came as component
// planes adds a plane table to the pass and a third set of work lists, through defaulted arguments; tests/cxx/
// encode_list_planar_tables.cpp is their program.  A pass of the ragged transcode is the same pass with another first
// stage: transcode_plan_one makes a decoded picture's output frame, and a layout built with `sources` carries the requant work list,
// descriptors and range flags (requant.hpp) in place of the forward lists; tests/cxx/transcode_tables.cpp.  Pictures with a flip,
// transpose or rotation (transform.hpp) get their output frame from the same planner and a second work list in the same
// layout; tests/cxx/transform_tables.cpp.  encode_device.cpp enqueues, waits
// and copies.  Calls nothing of the HIP runtime: a plain host compiler builds tests/cxx/encode_list_tables.cpp around it and
// encoder.cpp.  Private to libmijpeg.so.
#pragma once
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "encoder.hpp"
#include "forward.hpp"
#include "hencode.hpp"
#include "requant.hpp"
#include "transform.hpp"

namespace mij {

// ------------------------------------------------------------------------------------------------
// the frame of a picture to encode
// ------------------------------------------------------------------------------------------------
// What the entry points ask of a picture before they look further: 8 or 12 bits, one or three components, width and height in
// 1..65535 ...
inline bool shape_in_order(int precision, int components, int64_t width, int64_t height)
{
  return (precision == 8 || precision == 12) && (components == 1 || components == 3) && width >= 1 && width <= 65535 && height >= 1 && height <= 65535;
}
// ... and a row stride (bytes) that holds a line of it
inline bool line_fits(int precision, int components, int64_t width, int64_t row_stride) { return row_stride >= width * components * (precision == 12 ? 2 : 1); }

// pixels, and a row stride that holds a line; 16-bit samples: address and stride on 2-byte boundaries
inline bool pixels_in_order(const mijpeg_encode_frame &e, int precision)
{
  if (!e.pixels || !line_fits(precision, e.components, e.width, e.row_stride)) return false;
  return precision != 12 || (((uintptr_t)e.pixels | (uintptr_t)e.row_stride) & 1) == 0;
}

// mijpeg_frame_layout without its firewall
inline int frame_layout_of(mijpeg_info *f)
{
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
}

// The frame of a picture to encode: its layout and the tables of its quality (hsamp, vsamp: null = 1 x 1 throughout).  What
// mijpeg_frame_layout says to it.
// Quantization::InitDefaultTables (marker/quantization.cpp:275-466) with the default (Annex K) matrices, natural order: entries
// limited to `limit` -- 255 in 8-bit frames (:456-459: "the table entries shall be byte-sized"), 32767 at precision 12 (:446-447),
// where low qualities give 16-bit DQT entries (tests/golden/enc12: q 2)
inline void quality_tables_of(int quality, int limit, uint16_t luma[64], uint16_t chroma[64])
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

inline int picture_info_of(int32_t width, int32_t height, int32_t components, const int32_t *hsamp, const int32_t *vsamp, int quality, mijpeg_info &f,
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
  return frame_layout_of(&f);
}

// ------------------------------------------------------------------------------------------------
// ragged encode: the planner
// ------------------------------------------------------------------------------------------------
constexpr uint32_t PASS_BLOCKS_DEFAULT = 1u << 24; // 2 GiB of coefficients at most
constexpr uint32_t PASS_BLOCKS_MAX = 1u << 30;     // exclusive_scan_u32's reach

inline uint32_t pad256(uint32_t x) { return (x + 255u) & ~255u; }

// one picture's description -> its frame (layout, tables of its quality at its precision), blocks and intervals; MIJPEG_OK or
// INVALID_PARAMETER
inline int plan_one(const mijpeg_encode_frame &e, int precision, mijpeg_info &f, uint32_t &blocks, uint32_t &intervals)
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
inline int precision_of(const int32_t *precision, int i) { return precision ? precision[i] : 8; }

// Where the pictures of a list lie in their passes, one after the other: a picture whose frame, blocks and intervals are known gets
// its pass, its place in the pass's index spaces and its coefficient base; the totals grow.  The ragged encode and the ragged
// transcode cut their lists with it.
struct PassCutter {
  uint32_t pass_blocks; // (not 0)
  int pass = 0;
  uint64_t at_block = 0, at_interval = 0;
  int64_t at_coef = 0;
  void place(mijpeg_encode_ragged_item &it, mijpeg_encode_ragged_totals *totals)
  {
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
};

// (blocks, intervals, index spaces, pass cuts and coefficient bases do not depend on the precision: coefficients are int16 either way)
inline int plan_list(const mijpeg_encode_frame *frames, const int32_t *precision, int n, uint32_t pass_blocks, mijpeg_encode_ragged_item *items,
                     mijpeg_encode_ragged_totals *totals)
{
  if (!frames || !items || !totals || n < 1 || pass_blocks > PASS_BLOCKS_MAX) return MIJPEG_ERR_INVALID_PARAMETER;
  if (pass_blocks == 0) pass_blocks = PASS_BLOCKS_DEFAULT;
  memset(totals, 0, sizeof(*totals));
  PassCutter cut{pass_blocks};
  for (int i = 0; i < n; i++) {
    mijpeg_encode_ragged_item &it = items[i];
    memset(&it, 0, sizeof(it));
    if (const int rc = plan_one(frames[i], precision_of(precision, i), it.info, it.blocks, it.intervals)) return rc;
    cut.place(it, totals);
  }
  totals->passes = cut.pass + 1;
  return MIJPEG_OK;
}

// ------------------------------------------------------------------------------------------------
// ragged transcode: the plan of a picture
// ------------------------------------------------------------------------------------------------
inline bool transcode_spec_in_order(const mijpeg_transcode_spec &s)
{
  return s.quality >= MIJPEG_TRANSCODE_SKIP && s.quality <= 100 && s.restart_interval >= -1 && s.restart_interval <= 65535;
}

inline bool henc_frame_geometry(HencArgs &a, const mijpeg_info &info, int ri); // (below, with the argument blocks)

// A decoded picture's frame + spec (not SKIP, in order) -> the frame of its output, its restart interval, kept or not, the blocks
// and intervals of its scan; MIJPEG_OK or the picture's refusal, `out` zeroed.
//   a quality   what picture_info_of completes for the source's shape, sampling and precision: every component on table 0
//   kept        the same layout with the source's tables and quant_index, which enc_write_headers writes generally
// A one-component scan is not interleaved, so its output has sampling factors 1 x 1: the coders walk info.mcus_x * mcus_y blocks.
// transform (a code of mijpeg.h in order): under T width and height and every component's sampling factors swap and kept
// tables are transposed; a mirrored axis that is no whole number of the output's MCUs is trimmed to one (TRIM) or refuses the
// picture -- after the refusals above, with MIJPEG_ERR_NOT_AVAILABLE.  how: what became of the transform.
struct TransformPlan {
  uint32_t bits = 0;     // T / MH / MV
  bool trimmed = false;  // a partial MCU column or row was dropped
  bool geometry = false; // refused: a mirrored axis is no whole number of MCUs, or nothing is left of it
};
inline int transcode_plan_one(const mijpeg_info &src, const mijpeg_transcode_spec &spec, mijpeg_info &out, int &ri, bool &kept, uint32_t &blocks, uint32_t &intervals,
                              int32_t transform = MIJPEG_TRANSFORM_NONE, TransformPlan *how = nullptr)
{
  TransformPlan local;
  TransformPlan &tp = how ? *how : local;
  tp = TransformPlan{};
  tp.bits = transform_bits(transform);
  const bool T = tp.bits & TRANSFORM_T;
  auto refuse = [&](int code) { memset(&out, 0, sizeof(out)); return code; };
  kept = spec.quality == MIJPEG_TRANSCODE_KEEP;
  ri = spec.restart_interval < 0 ? src.restart_interval : spec.restart_interval;
  if (src.xt || (src.components != 1 && src.components != 3) || src.coef_wide || (src.precision != 8 && src.precision != 12) || ri < 0 || ri > 65535)
    return refuse(MIJPEG_ERR_NOT_IMPLEMENTED);
  int32_t hs[MIJPEG_MAX_COMPONENTS] = {1, 1, 1, 1}, vs[MIJPEG_MAX_COMPONENTS] = {1, 1, 1, 1};
  int per_mcu = 1;
  if (src.components == 3) {
    per_mcu = 0;
    for (int c = 0; c < 3; c++) {
      hs[c] = T ? src.vsamp[c] : src.hsamp[c];
      vs[c] = T ? src.hsamp[c] : src.vsamp[c];
      per_mcu += hs[c] * vs[c];
    }
  }
  // the frame after T, and its mirrored axes in whole MCUs (sampling factors out of order are picture_info_of's to refuse)
  int32_t width = T ? src.height : src.width, height = T ? src.width : src.height;
  auto mcu_of = [](const int32_t *s) { return 8 * std::min(4, std::max(1, std::max(s[0], std::max(s[1], s[2])))); }; // (1 .. 4 whatever the source says)
  const int mcu_w = mcu_of(hs), mcu_h = mcu_of(vs);
  auto whole = [&](uint32_t mirrored, int32_t &extent, int mcu) {
    if (!(tp.bits & mirrored) || extent < 1 || extent % mcu == 0) return;
    if ((transform & MIJPEG_TRANSFORM_TRIM) && extent > mcu) {
      extent -= extent % mcu;
      tp.trimmed = true;
    } else {
      tp.geometry = true;
    }
  };
  whole(TRANSFORM_MH, width, mcu_w);
  whole(TRANSFORM_MV, height, mcu_h);
  if (picture_info_of(width, height, src.components, hs, vs, kept ? 50 : spec.quality, out, src.precision)) return refuse(MIJPEG_ERR_NOT_IMPLEMENTED);
  for (int c = 0; c < src.components; c++) {
    if ((unsigned)src.quant_index[c] >= 4 || src.blocks_w[c] < 1 || src.blocks_h[c] < 1) return refuse(MIJPEG_ERR_NOT_IMPLEMENTED);
    for (int k = 0; k < 64; k++) {
      const uint16_t a = src.quant[src.quant_index[c]][k];
      if (a == 0 || (kept && src.precision == 8 && a > 255)) return refuse(MIJPEG_ERR_NOT_IMPLEMENTED); // (no division by it; no baseline DQT holds it)
    }
  }
  if (tp.geometry) return refuse(MIJPEG_ERR_NOT_AVAILABLE);
  if (kept) {
    for (int t = 0; t < 4; t++) transform_table(tp.bits, src.quant[t], out.quant[t]);
    for (int c = 0; c < src.components; c++) out.quant_index[c] = src.quant_index[c];
  }
  HencArgs geometry;
  memset(&geometry, 0, sizeof(geometry));
  const uint64_t mcus = (uint64_t)out.mcus_x * (uint64_t)out.mcus_y, nb = mcus * (uint64_t)per_mcu;
  if (!henc_frame_geometry(geometry, out, ri) || nb >= PASS_BLOCKS_MAX) return refuse(MIJPEG_ERR_NOT_AVAILABLE);
  blocks = (uint32_t)nb;
  const uint64_t per = ri ? (uint64_t)ri : mcus;
  intervals = (uint32_t)((mcus + per - 1) / per);
  return MIJPEG_OK;
}

// What a transcode pass reads of a picture beside its item: the decoded frame and where its planes lie in device memory
struct RequantSource {
  mijpeg_info info;
  const int16_t *planes;
  uint32_t transform = 0; // T / MH / MV (transform.hpp); not 0: the picture is transform_list_kernel's
};

// ------------------------------------------------------------------------------------------------
// argument blocks
// ------------------------------------------------------------------------------------------------
// the forward kernels' argument block for a batch (geometry, routing, quantiser multipliers): MIJPEG_OK or the refusal.
// planes: the picture is planar -- b->pixels_dev is its plane 0, b->pixel_row_stride the pitch of all three, *planes its
// planes 1 and 2; the fast condition then asks all three plane addresses and the pitch to be multiples of 4
inline int forward_args_of(const mijpeg_forward_batch *b, ForwardArgs &a, const ForwardPlanes *planes = nullptr)
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
  const bool dword_lines = (((uintptr_t)b->pixels_dev | (uintptr_t)b->pixel_frame_stride | (uintptr_t)b->pixel_row_stride |
                             (planes ? (uintptr_t)planes->p1 | (uintptr_t)planes->p2 : 0)) & 3) == 0;
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
inline bool henc_frame_geometry(HencArgs &a, const mijpeg_info &info, int ri)
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

inline void henc_pack_tables(HencTables *h, const EncTables &t)
{
  memset(h, 0, sizeof(*h));
  for (int k = 0; k < 2; k++) {
    for (int i = 0; i < 16; i++) { h->dc_code[k][i] = t.dc[k].code[i]; h->dc_len[k][i] = t.dc[k].len[i]; }
    for (int i = 0; i < 256; i++) { h->ac_code[k][i] = t.ac[k].code[i]; h->ac_len[k][i] = t.ac[k].len[i]; }
  }
}

struct Carver { // lays regions out in a buffer, 256-byte aligned
  size_t at = 0;
  size_t take(size_t bytes)
  {
    const size_t o = at;
    at += henc_aligned(bytes);
    return o;
  }
};

constexpr size_t HENC_HIST_BYTES = 4 * 256 * sizeof(uint32_t); // a picture's symbol statistics: HencArgs::hist

// Huffman tables from the picture's own statistics: with `optimize`, and always at precision 12, where the Annex K.3 tables have
// no codes for categories 12..15.  (Coefficients the forward kernels make of 8-bit pixels always have a code in the standard
// tables, at most 11 / 10 bits, the host coder's check; of 12-bit pixels at most 15 / 14 bits, which tables of their own cover.)
inline bool codes_with_own_tables(const mijpeg_info &f, int optimize) { return optimize || f.precision == 12; }

// histogram of a picture -> its tables (Annex K.2; a single component: one pair) -> as the kernels read them
inline void tables_from_statistics(const uint32_t hist[4][256], int components, EncTables &t, HencTables *packed)
{
  enc_standard_tables(t);
  enc_optimal_tables(t, hist, hist + 2, components > 1 ? 2 : 1);
  henc_pack_tables(packed, t);
}

// a picture's view of the arrays of coder_layout() at `base`: from its first block and first interval
inline void point_into(HencArgs &a, uint8_t *base, const CoderLayout &l, uint32_t first_block = 0, uint32_t first_interval = 0)
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

// ------------------------------------------------------------------------------------------------
// ragged encode: one pass as data
// ------------------------------------------------------------------------------------------------
// A work list of the forward kernels: first[k] is the first workgroup of item k, the grid behind the last (empty: no launch)
struct ForwardWorkList { std::vector<uint32_t> first, item; };

// `item` (picture * 4 + component) with `wgs` workgroups behind the list's last; false: the grid would pass 2^31 - 1
inline bool work_list_append(ForwardWorkList &l, uint32_t item, uint64_t wgs)
{
  const uint64_t at = l.first.empty() ? 0 : l.first.back();
  if (at + wgs > 0x7fffffffull) return false;
  if (l.first.empty()) l.first.push_back(0);
  l.first.push_back((uint32_t)(at + wgs));
  l.item.push_back(item);
  return true;
}

// Pictures [p0, p1) of a planned list, one pass (frames[i].pixels are device addresses): index spaces, routing, and the three
// arenas.  Offsets are bytes from an arena's start, every region 256-byte aligned.  The part that goes up in one copy is laid
// out first: its offsets hold in the pinned arena and in the device arena alike.
struct EncodePassLayout {
  int error = MIJPEG_OK;                  // a refusal (`why`): nothing below is complete, nothing was enqueued
  const char *why = nullptr;
  const mijpeg_encode_frame *frames;      // the pass's first
  const mijpeg_encode_ragged_item *items; // the pass's first
  uint32_t n, N, I;                       // pictures, blocks (every picture padded to 256), intervals
  int64_t coef_total;                     // int16 elements of the coefficient store
  std::vector<uint32_t> own_index;        // the place of a picture that codes with tables of its own in the histogram and table
  uint32_t n_own = 0;                     // arenas, which hold the pictures that use them; UINT32_MAX: the standard tables
  std::vector<ForwardArgs> fargs;         // per picture (routing: launch_forward's); coef is fill_upload's
  std::vector<HencArgs> hargs;            // per picture, the geometry alone
  ForwardWorkList lists[FORWARD_RAGGED_LISTS]; // per flavour (8 bit, 12 bit, planar 8 bit) and kernel family
  const ForwardPlanes *planes;            // the pass's first, or null: planes 1 and 2 of the planar pictures (p1 set), nulls for the others
  uint32_t n_planar = 0;                  // planar pictures of the pass; none: no plane table goes up
  CoderLayout coder;                      // coder_layout(N, I), at `coder_at` of the device arena
  // uploaded in one piece (pinned and device): descriptors, prefix tables (n + 1 entries), work lists, the standard tables
  size_t fargs_at, hargs_at, first_block_at, first_interval_at, wl_first_at[FORWARD_RAGGED_LISTS], wl_item_at[FORWARD_RAGGED_LISTS], std_tables_at, up_bytes;
  size_t planes_at;                       // the plane table, n entries behind the standard tables (empty without planar pictures)
  // device only, behind them: first_chunk[n + 1], own tables and histograms, the gathered prefix sums, coder arrays, coefficients
  size_t d_first_chunk, d_tables, d_hist, d_gather, coder_at, coef_at, dev_bytes;
  // pinned, behind the upload: what goes up later (first_chunk, own tables) and what comes back (histograms, gathered sums)
  size_t h_first_chunk, h_tables, h_hist, h_istart, h_ffstart, host_bytes;
  size_t hist_bytes;
  // A pass's first stage is the forward work lists above or, in a transcode pass, the requant work list: `sources` set,
  // no ForwardArgs are made and no forward list is filled (frames[i] then hold the shape and the restart interval, no pixels).
  // Its regions are empty in an encode pass, whose offsets and sizes are what they were
  const RequantSource *sources;           // the pass's first, or null
  ForwardWorkList requant;                // items (picture * 4 + component) of requant_list_kernel
  size_t rq_pics_at, rq_first_at, rq_item_at, rq_flags_at; // uploaded: a RequantPicture per picture, the work list, the zeroed range flags (n words)
  size_t h_flags;                         // pinned: the flags read back
  // The transformed pictures of a transcode pass have a work list of their own, transform_list_kernel's, over the same
  // descriptors and flags, and the pass a word of T / MH / MV bits per picture.  Without such pictures the regions are empty and
  // every offset and size is what it was
  ForwardWorkList transform;
  size_t tf_first_at, tf_item_at, tf_bits_at;

  // all_planes: one entry per picture of the list; a planar picture's frame holds plane 0 in `pixels` and the planes' pitch in
  // `row_stride`, its entry planes 1 and 2 (only 8-bit pictures of three components are planar here)
  EncodePassLayout(const mijpeg_encode_frame *all_frames, const mijpeg_encode_ragged_item *all_items, int p0, int p1, int optimize,
                   const ForwardPlanes *all_planes = nullptr, const RequantSource *all_sources = nullptr)
      : frames(all_frames + p0), items(all_items + p0), n((uint32_t)(p1 - p0)), own_index(n, UINT32_MAX), fargs(n), hargs(n),
        planes(all_planes ? all_planes + p0 : nullptr), sources(all_sources ? all_sources + p0 : nullptr)
  {
    const mijpeg_encode_ragged_item &last = items[n - 1];
    N = last.first_block + pad256(last.blocks);
    I = last.first_interval + last.intervals;
    coef_total = last.coef_base + ((last.info.coef_count + 127) & ~(int64_t)127);
    route(optimize);
    Carver up;
    fargs_at = up.take(sources ? 0 : (size_t)n * sizeof(ForwardArgs));
    hargs_at = up.take((size_t)n * sizeof(HencArgs));
    first_block_at = up.take(((size_t)n + 1) * 4);
    first_interval_at = up.take(((size_t)n + 1) * 4);
    for (int l = 0; l < FORWARD_RAGGED_LISTS; l++) {
      wl_first_at[l] = up.take(lists[l].first.size() * 4);
      wl_item_at[l] = up.take(lists[l].item.size() * 4);
    }
    std_tables_at = up.take(sizeof(HencTables));
    planes_at = up.take(n_planar ? (size_t)n * sizeof(ForwardPlanes) : 0);
    rq_pics_at = up.take(sources ? (size_t)n * sizeof(RequantPicture) : 0);
    rq_first_at = up.take(requant.first.size() * 4);
    rq_item_at = up.take(requant.item.size() * 4);
    rq_flags_at = up.take(sources ? (size_t)n * 4 : 0);
    tf_first_at = up.take(transform.first.size() * 4);
    tf_item_at = up.take(transform.item.size() * 4);
    tf_bits_at = up.take(transform.item.empty() ? 0 : (size_t)n * 4);
    up_bytes = up.at;
    hist_bytes = (size_t)n_own * HENC_HIST_BYTES;
    coder = coder_layout(N, I);
    Carver dv = up;
    d_first_chunk = dv.take(((size_t)n + 1) * 4);
    d_tables = dv.take((size_t)n_own * sizeof(HencTables));
    d_hist = dv.take(hist_bytes);
    d_gather = dv.take(((size_t)n + 1) * 8);
    coder_at = dv.take(coder.end);
    coef_at = dv.take((size_t)coef_total * sizeof(int16_t));
    dev_bytes = dv.at;
    Carver hp = up;
    h_first_chunk = hp.take(((size_t)n + 1) * 4);
    h_tables = hp.take((size_t)n_own * sizeof(HencTables));
    h_hist = hp.take(hist_bytes);
    h_istart = hp.take(((size_t)n + 1) * 8);
    h_ffstart = hp.take(((size_t)n + 1) * 8);
    h_flags = hp.take(sources ? (size_t)n * 4 : 0);
    host_bytes = hp.at;
  }
  // per picture: tables of its own or not, its ForwardArgs and its items in the work lists, its coder geometry
  void route(int optimize)
  {
    for (uint32_t p = 0; p < n; p++) {
      if (codes_with_own_tables(items[p].info, optimize)) own_index[p] = n_own++;
      const mijpeg_encode_frame &e = frames[p];
      if (sources) { // a transcode pass: the picture's components in the requant work list, its coder geometry
        for (int c = 0; c < items[p].info.components; c++)
          if (!work_list_append(sources[p].transform ? transform : requant, p * 4u + (uint32_t)c, requant_workgroups(items[p].info, c)))
            return refuse(MIJPEG_ERR_NOT_AVAILABLE, "pass too large for one requant launch");
        memset(&hargs[p], 0, sizeof(HencArgs));
        if (!henc_frame_geometry(hargs[p], items[p].info, e.restart_interval)) return refuse(MIJPEG_ERR_NOT_AVAILABLE, "too many blocks per MCU");
        continue;
      }
      mijpeg_forward_batch b;
      memset(&b, 0, sizeof(b));
      b.info = items[p].info;
      b.pixels_dev = e.pixels;
      b.pixel_row_stride = e.row_stride;
      b.pixel_frame_stride = e.row_stride * (int64_t)e.height;
      b.coef_dev = (int16_t *)16; // (placed by fill_upload, once the store's address is known)
      b.coef_frame_stride = b.info.coef_count;
      b.frames = 1;
      if (planar(p) && (b.info.precision != 8 || b.info.components != 3)) return refuse(MIJPEG_ERR_INVALID_PARAMETER, "planar picture without a planar kernel");
      if (const int rc = forward_args_of(&b, fargs[p], planar(p) ? planes + p : nullptr)) return refuse(rc, "invalid frame for the forward kernels");
      n_planar += planar(p);
      int which[5], comp[5];
      uint32_t wgs[5];
      const int k = forward_ragged_items(fargs[p], which, wgs, comp);
      for (int j = 0; j < k; j++)
        if (!work_list_append(lists[forward_ragged_list(which[j], b.info.precision, planar(p))], p * 4u + (uint32_t)comp[j], wgs[j]))
          return refuse(MIJPEG_ERR_NOT_AVAILABLE, "pass too large for one forward launch");
      memset(&hargs[p], 0, sizeof(HencArgs));
      if (!henc_frame_geometry(hargs[p], items[p].info, e.restart_interval)) return refuse(MIJPEG_ERR_INVALID_PARAMETER, "too many blocks per MCU");
    }
  }
  void refuse(int code, const char *message) { error = code; why = message; }
  bool own(uint32_t p) const { return own_index[p] != UINT32_MAX; }
  bool planar(uint32_t p) const { return planes && planes[p].p1; }
};

// What the kernels of a pass are launched with
struct EncodePassArgs {
  ForwardRaggedPlan forward;
  HencBatchArgs coder; // (plain, ffcount, ffstart, out, total_chunks: once the output arena is there)
  RequantArgs requant; // a transcode pass: its first stage, and its grid
  uint32_t requant_grid;
  TransformArgs transform; // ... and the first stage of its transformed pictures
  uint32_t transform_grid;
};

// The uploaded part into `host` (up_bytes of it), with the addresses it will have at `dev`: a ForwardArgs and a HencArgs per
// picture, first_block and first_interval, the work lists, the standard tables (std_tabs, packed), the plane table of a pass with planar pictures.  Statistics are counted with
// the standard tables' lengths (any would do), the real pass with the picture's own (own_tables).
inline EncodePassArgs fill_upload(uint8_t *host, uint8_t *dev, const EncodePassLayout &L, const EncTables &std_tabs)
{
  henc_pack_tables((HencTables *)(host + L.std_tables_at), std_tabs);
  ForwardArgs *hf = (ForwardArgs *)(host + L.fargs_at);
  HencArgs *hh = (HencArgs *)(host + L.hargs_at);
  uint32_t *first_block = (uint32_t *)(host + L.first_block_at), *first_interval = (uint32_t *)(host + L.first_interval_at);
  int16_t *coef = (int16_t *)(dev + L.coef_at);
  for (uint32_t p = 0; p < L.n; p++) {
    const mijpeg_encode_ragged_item &it = L.items[p];
    if (L.sources) {
      if (L.sources[p].transform) transform_picture_of(((RequantPicture *)(host + L.rq_pics_at))[p], L.sources[p].info, L.sources[p].planes, it.info, coef + it.coef_base, L.sources[p].transform);
      else requant_picture_of(((RequantPicture *)(host + L.rq_pics_at))[p], L.sources[p].info, L.sources[p].planes, it.info, coef + it.coef_base);
      if (!L.transform.item.empty()) ((uint32_t *)(host + L.tf_bits_at))[p] = L.sources[p].transform;
      ((uint32_t *)(host + L.rq_flags_at))[p] = 0;
    } else {
      hf[p] = L.fargs[p];
      hf[p].coef = coef + it.coef_base;
    }
    HencArgs &a = hh[p];
    a = L.hargs[p];
    a.coef = coef + it.coef_base;
    a.tables = (const HencTables *)(dev + L.std_tables_at);
    a.total_blocks = it.blocks;
    a.n_intervals = it.intervals;
    point_into(a, dev + L.coder_at, L.coder, it.first_block, it.first_interval);
    a.hist = L.own(p) ? (uint32_t *)(dev + L.d_hist) + (size_t)L.own_index[p] * 4 * 256 : nullptr;
    first_block[p] = it.first_block;
    first_interval[p] = it.first_interval;
  }
  first_block[L.n] = L.N;
  first_interval[L.n] = L.I;
  EncodePassArgs a;
  memset(&a, 0, sizeof(a));
  for (int l = 0; l < FORWARD_RAGGED_LISTS; l++) {
    const ForwardWorkList &w = L.lists[l];
    if (w.item.empty()) continue;
    memcpy(host + L.wl_first_at[l], w.first.data(), w.first.size() * 4);
    memcpy(host + L.wl_item_at[l], w.item.data(), w.item.size() * 4);
    a.forward.launch[l].pics = (const ForwardArgs *)(dev + L.fargs_at);
    a.forward.launch[l].first_wg = (const uint32_t *)(dev + L.wl_first_at[l]);
    a.forward.launch[l].item = (const uint32_t *)(dev + L.wl_item_at[l]);
    a.forward.launch[l].items = (uint32_t)w.item.size();
    a.forward.grid[l] = w.first.back();
  }
  if (L.n_planar) {
    memcpy(host + L.planes_at, L.planes, (size_t)L.n * sizeof(ForwardPlanes));
    a.forward.planes = (const ForwardPlanes *)(dev + L.planes_at);
  }
  if (L.sources) {
    if (!L.requant.item.empty()) { // (every picture of the pass may be transformed)
      memcpy(host + L.rq_first_at, L.requant.first.data(), L.requant.first.size() * 4);
      memcpy(host + L.rq_item_at, L.requant.item.data(), L.requant.item.size() * 4);
    }
    a.requant.pics = (const RequantPicture *)(dev + L.rq_pics_at);
    a.requant.first_wg = (const uint32_t *)(dev + L.rq_first_at);
    a.requant.item = (const uint32_t *)(dev + L.rq_item_at);
    a.requant.items = (uint32_t)L.requant.item.size();
    a.requant.flags = (uint32_t *)(dev + L.rq_flags_at);
    a.requant_grid = L.requant.first.empty() ? 0 : L.requant.first.back();
  }
  if (!L.transform.item.empty()) {
    memcpy(host + L.tf_first_at, L.transform.first.data(), L.transform.first.size() * 4);
    memcpy(host + L.tf_item_at, L.transform.item.data(), L.transform.item.size() * 4);
    a.transform.list = a.requant;
    a.transform.list.first_wg = (const uint32_t *)(dev + L.tf_first_at);
    a.transform.list.item = (const uint32_t *)(dev + L.tf_item_at);
    a.transform.list.items = (uint32_t)L.transform.item.size();
    a.transform.bits = (const uint32_t *)(dev + L.tf_bits_at);
    a.transform_grid = L.transform.first.back();
  }
  a.coder.pics = (const HencArgs *)(dev + L.hargs_at);
  a.coder.first_block = (const uint32_t *)(dev + L.first_block_at);
  a.coder.first_interval = (const uint32_t *)(dev + L.first_interval_at);
  a.coder.first_chunk = (const uint32_t *)(dev + L.d_first_chunk);
  a.coder.n = L.n;
  a.coder.total_blocks = L.N;
  a.coder.total_intervals = L.I;
  return a;
}

// The histograms have come back (h_hist): every own picture's tables (tabs[own_index], n_own of them), packed at h_tables, and its
// HencArgs in `host` repointed at its slot of the device's table arena
inline void own_tables(uint8_t *host, uint8_t *dev, const EncodePassLayout &L, std::vector<EncTables> &tabs)
{
  tabs.resize(L.n_own);
  HencTables *ht = (HencTables *)(host + L.h_tables);
  HencArgs *hh = (HencArgs *)(host + L.hargs_at);
  for (uint32_t p = 0; p < L.n; p++) {
    const uint32_t o = L.own_index[p];
    if (o == UINT32_MAX) continue;
    tables_from_statistics((const uint32_t(*)[256])(host + L.h_hist) + (size_t)o * 4, L.items[p].info.components, tabs[o], ht + o);
    hh[p].tables = (const HencTables *)(dev + L.d_tables) + o;
  }
}

// The gathered istart have come back (h_istart: where every picture's plain stream begins, n + 1 entries): every picture on a
// chunk boundary of the plain buffer, first_chunk[n + 1] at h_first_chunk.  false: 2^30 chunks or more
inline bool chunk_layout(uint8_t *host, const EncodePassLayout &L)
{
  const uint64_t *istart = (const uint64_t *)(host + L.h_istart);
  uint32_t *first_chunk = (uint32_t *)(host + L.h_first_chunk);
  uint64_t chunks = 0;
  for (uint32_t p = 0; p < L.n; p++) {
    first_chunk[p] = (uint32_t)chunks;
    chunks += (istart[p + 1] - istart[p] + HENC_STUFF_CHUNK - 1) / HENC_STUFF_CHUNK;
    if (chunks >= PASS_BLOCKS_MAX) return false;
  }
  first_chunk[L.n] = (uint32_t)chunks;
  return true;
}
inline uint32_t chunks_of(const uint8_t *host, const EncodePassLayout &L) { return ((const uint32_t *)(host + L.h_first_chunk))[L.n]; }

// The gathered ffstart have come back too (h_ffstart: 0xFF bytes in front of every picture): what of `out` the pass has written
// (HencBatchArgs in hencode.hpp) ...
inline size_t arena_bytes(const uint8_t *host, const EncodePassLayout &L)
{
  return (size_t)chunks_of(host, L) * HENC_STUFF_CHUNK + (size_t)((const uint64_t *)(host + L.h_ffstart))[L.n] + 2 * ((size_t)L.I - L.n);
}
// ... and picture p's entropy coded segment in it: the plain bytes, a stuffing byte per 0xFF, a marker between two intervals
struct StreamPiece { size_t at, ecs; };
inline StreamPiece stream_piece(const uint8_t *host, const EncodePassLayout &L, uint32_t p)
{
  const uint64_t *istart = (const uint64_t *)(host + L.h_istart), *ffs = (const uint64_t *)(host + L.h_ffstart);
  const mijpeg_encode_ragged_item &it = L.items[p];
  return StreamPiece{(size_t)((const uint32_t *)(host + L.h_first_chunk))[p] * HENC_STUFF_CHUNK + (size_t)ffs[p] + 2 * ((size_t)it.first_interval - p),
                     (size_t)(istart[p + 1] - istart[p]) + (size_t)(ffs[p + 1] - ffs[p]) + 2 * ((size_t)it.intervals - 1)};
}

} // namespace mij
