// codestream_walk.cpp -- HostDecoder::parse and the RefWalker state machine behind it: the reference's walk over a codestream's
// markers, tables, frame and scan headers and JPEG XT boxes, restated with what it does with damaged streams; the boxes' byte
// stores, their hidden refinement scans and the file's checksum.
#include "codestream_walk.hpp"

#include "encoder.hpp"
#include "xt_spec.hpp"

#include <limits.h>
#include <stdio.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>

namespace mij {

// ------------------------------------------------------------------------------------------------
// The codestream state machine of the reference, including what it does with damaged streams
// ------------------------------------------------------------------------------------------------
// interface/jpeg.cpp:244-354 (JPEG::ReadInternal) drives: SOI (codestream/decoder.cpp:77-108), the tables/misc
// segments one at a time (Tables::ParseTablesIncremental, codestream/tables.cpp:1003-1418), the frame header
// (codestream/image.cpp:616-650, marker/frame.cpp:111-208, marker/component.cpp:86-111), then per scan
// Frame::StartParseScan / ScanForScanHeader (marker/frame.cpp:796-899), Scan::ParseMarker (marker/scan.cpp:163-315), the
// MCUs, Frame::ParseTrailer (marker/frame.cpp:1016-1123) and Image::ParseTrailer (codestream/image.cpp:1408-1497).
// Conditions the reference throws on end the decode with its error code; conditions it only warns about
// (JPG_WARN) are decoded through the way it does: stray markers and garbage between segments are skipped, a missing
// EOI is accepted, restart markers that are not where the entropy decoder expects them make it resynchronise
// (EntropyParser::ParseRestartMarker, codestream/entropyparser.cpp:117-201) and lost restart intervals come out grey.
//
// The walker runs in two modes.  PLAN (HostDecoder::parse): at a scan header the entropy coded segment is only
// searched for its markers, the scan is recorded for the parallel decoders and the walk continues behind it -- valid
// when the segment is well-formed, which the search and, later, the parallel decoders check; everything else sets
// needs_sequential_.  DECODE (HostDecoder::decode_sequential): the scans are decoded MCU by MCU in stream order with a
// literal restatement of the reference's bit reader, exactly as the reference does it.
namespace {

// io/bitstream.hpp:106-210 + io/bitstream.cpp:56-137, byte-stuffing flavour, literally: in front of a marker Fill() adds
// EIGHT zero bits per call, at the end of the data it pads the window; a read that still finds too few bits throws.
struct RefBits {
  ByteCursor *io = nullptr;
  uint32_t b = 0;
  int bits = 0;
  bool marker = false, eof = false;
  void open(ByteCursor *s) { io = s; b = 0; bits = 0; marker = eof = false; }
  void fill()
  {
    do {
      const long dt = io->get();
      if (dt == 0xff) {
        io->lastundo();
        if (io->peekword() == 0xff00) {
          io->getword();
          b |= (uint32_t)0xff << (24 - bits);
          bits += 8;
        } else {
          marker = true;
          bits += 8;
          break;
        }
      } else if (dt == ByteCursor::END) {
        eof = true;
        bits += 8;
      } else {
        b |= (uint32_t)dt << (24 - bits);
        bits += 8;
      }
    } while (bits <= 24);
  }
  [[noreturn]] void report_error() const
  {
    if (eof) wthrow(MIJPEG_ERR_UNEXPECTED_EOF, "invalid stream, found EOF within entropy coded segment");
    if (marker) wthrow(MIJPEG_ERR_UNEXPECTED_EOF, "invalid stream, found marker in entropy coded segment");
    wthrow(MIJPEG_ERR_MALFORMED_STREAM, "invalid stream, found invalid huffman code in entropy coded segment");
  }
  uint32_t get(int k)
  {
    if (k > bits) {
      fill();
      if (k > bits) report_error();
    }
    const uint32_t v = b >> (32 - k);
    b <<= k;
    bits -= k;
    return v;
  }
  uint32_t peekword()
  {
    if (bits < 16) fill();
    return b >> 16;
  }
  void skipbits(int k)
  {
    if (k > bits) report_error();
    b <<= k;
    bits -= k;
  }
};

// HuffmanDecoder::Get, coding/huffmandecoder.hpp:103-124: an unassigned code has length 0xff in the reference's table
inline int ref_symbol(RefBits &s, const HuffTable &h)
{
  const uint32_t data = s.peekword();
  const uint16_t e = h.fast[data >> (16 - HuffTable::LOOKAHEAD)];
  if (e) {
    s.skipbits(e >> 8);
    return e & 0xff;
  }
  for (int l = HuffTable::LOOKAHEAD + 1; l <= 16; l++) {
    const int32_t code = (int32_t)(data >> (16 - l));
    if (code <= h.maxcode[l]) {
      s.skipbits(l);
      return h.values[(code + h.valoff[l]) & 0xff];
    }
  }
  s.skipbits(0xff);
  return 0;
}
} // namespace

// Quantization::ParseMarker, marker/quantization.cpp:474-537
void RefWalker::parse_dqt(ByteCursor &s)
{
  long len = s.getword();
  if (len < 2) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "DQT marker must be at least two bytes long");
  len -= 2;
  while (len > 2) {
    uint16_t deltas[64];
    const uint8_t *zz = scan_order();
    long type = s.get();
    if (type == ByteCursor::END) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "DQT marker run out of data");
    const long target = type & 15;
    type >>= 4;
    if (type != 0 && type != 1) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "DQT marker entry type must be either 0 or 1");
    if (target > 3) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "DQT marker target table must be between 0 and 3");
    len -= 1;
    if (len < 64 * (type + 1)) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "DQT marker contains insufficient data");
    for (int i = 0; i < 64; i++) {
      const long v = type ? s.getword() : s.get();
      if (v == ByteCursor::END) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "DQT marker run out of data");
      deltas[zz[i]] = (uint16_t)v;
    }
    len -= 64 * (type + 1);
    memcpy(hd.quant_[target], deltas, sizeof(deltas));
    hd.quant_defined_[target] = true;
  }
  hd.have_quant_ = true; // the table set exists as soon as a DQT marker was seen (tables.cpp:1007-1009)
  if (len != 0) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "DQT marker size corrupt");
}

// HuffmanTable::ParseMarker, marker/huffmantable.cpp:127-169 + HuffmanTemplate::ParseMarker, coding/huffmantemplate.cpp:878-905.
// The decoder of a table is only built when a scan uses it (huffmantemplate.cpp:802-874), a damaged table nobody
// uses is not an error.
void RefWalker::parse_dht(ByteCursor &s)
{
  long len = s.getword();
  if (len < 2) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Huffman table length must be at least two bytes long");
  len -= 2;
  while (len > 0) {
    const long t = s.get();
    const size_t p = s.pos;
    if (t == ByteCursor::END) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Huffman table marker run out of data");
    len--;
    if ((t >> 4) > 1) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "undefined Huffman table type");
    if ((t & 15) > 3) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "invalid Huffman table destination, must be between 0 and 3");
    HuffTable &h = (t >> 4) ? hd.ac_[t & 3] : hd.dc_[t & 3];
    h.defined = false;
    h.built = false;
    h.oversize = false;
    int total = 0;
    for (int i = 0; i < 16; i++) {
      const long cnt = s.get();
      if (cnt == ByteCursor::END) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Huffman table marker run out of data");
      h.counts[i] = (uint8_t)cnt;
      total += (int)cnt;
    }
    if ((long)(16 + total) > len) {
      // the reference reads the values first and notices then; reading may run into the end of the stream
      if ((size_t)total > s.n - s.pos) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Huffman table marker run out of data");
      wthrow(MIJPEG_ERR_MALFORMED_STREAM, "huffman table size corrupt");
    }
    // the reference takes as many values as the counts add up to (up to 4080); this decoder keeps 256 and refuses the
    // table only when a scan wants to use it
    memset(h.values, 0, sizeof(h.values));
    for (int i = 0; i < total; i++) {
      const uint8_t v = (uint8_t)s.get();
      if (i < 256) h.values[i] = v;
    }
    h.oversize = total > 256;
    h.defined = true;
    len -= (long)(s.pos - p);
  }
  hd.have_huff_ = true;
}

// The FORM of a merging specification, checked where its box completes -- in front of everything that follows in the file:
// SuperBox::ParseBoxContent (boxes/superbox.cpp:93-206) frames the sub-boxes, MergingSpecBox::CreateBox / AcknowledgeBox
// (boxes/mergingspecbox.cpp:108-256) allow one box of each kind and one curve / matrix per index, and each sub-box parses its
// own payload (outputconversionbox.cpp:93-127, colortrafobox.cpp:62-79, nonlineartrafobox.cpp:62-80, dctbox.cpp:61-90,
// refinementspecbox.cpp:58-82, parametrictonemappingbox.cpp:85-149, lineartransformationbox.cpp:62-99).  What the boxes MEAN
// is the colour transformer's business (HostDecoder::finish_xt).  `announced`: the box length its segments added up to (a file
// that ends inside the box leaves fewer bytes: reads beyond them find EOF).
// is_alpha: the box is the ALPHA merging specification (ASPC), where the compositing box AMUL belongs (boxes/alphabox.cpp:60-90).
static void check_merging_spec(const uint8_t *d, size_t have, uint64_t announced, bool is_alpha = false)
{
  static const char *const incomplete = "found incomplete box header within a superbox";
  static const char *const too_short = "box size within super box is inconsistent and too short";
  auto id = [](char a, char b, char c, char e) { return ((uint32_t)(uint8_t)a << 24) | ((uint32_t)(uint8_t)b << 16) | ((uint32_t)(uint8_t)c << 8) | (uint32_t)(uint8_t)e; };
  const uint32_t once[] = {id('R', 'S', 'P', 'C'), id('O', 'C', 'O', 'N'), id('L', 'D', 'C', 'T'), id('R', 'D', 'C', 'T'), id('L', 'T', 'R', 'F'),
                           id('C', 'T', 'R', 'F'), id('R', 'T', 'R', 'F'), id('D', 'T', 'R', 'F'), id('S', 'T', 'R', 'F'), id('L', 'P', 'T', 'S'),
                           id('Q', 'P', 'T', 'S'), id('C', 'P', 'T', 'S'), id('R', 'P', 'T', 'S'), id('S', 'P', 'T', 'S'), id('P', 'P', 'T', 'S'),
                           id('D', 'P', 'T', 'S')};
  bool seen[sizeof(once) / sizeof(once[0])] = {false};
  bool curve[16] = {false}, matrix[16] = {false}, amul = false;
  uint64_t j = 0;
  while (j < announced) {
    const uint64_t left = announced - j;
    if (left < 8) wthrow(MIJPEG_ERR_MALFORMED_STREAM, incomplete);
    if (j + 8 > have) wthrow(MIJPEG_ERR_UNEXPECTED_EOF, "run into an EOF while parsing a box header in a superbox");
    const uint32_t lbox = rd32(d + j), tbox = rd32(d + j + 4);
    uint64_t xl = lbox, overhead = 8;
    if (lbox == 1) {
      if (left < 16) wthrow(MIJPEG_ERR_MALFORMED_STREAM, incomplete);
      if (j + 16 > have) wthrow(MIJPEG_ERR_UNEXPECTED_EOF, "run into an EOF while parsing a box header in a superbox");
      xl = 0;
      for (int k = 0; k < 8; k++) xl = (xl << 8) | d[j + 8 + k];
      if (xl < 16) wthrow(MIJPEG_ERR_MALFORMED_STREAM, too_short);
      overhead = 16;
    } else if (lbox == 0)
      wthrow(MIJPEG_ERR_MALFORMED_STREAM, "found a box size of zero within a superbox");
    else if (lbox < 8)
      wthrow(MIJPEG_ERR_MALFORMED_STREAM, too_short);
    if (left < xl) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "incomplete super box, super box does not provide enough data for body of sub-box");
    const uint64_t len = xl - overhead;
    const uint8_t *pl = d + j + overhead;
    auto byte = [&](uint64_t k) -> long { return j + overhead + k < have ? (long)pl[k] : -1; }; // ByteStream::Get at the end: EOF
    for (size_t k = 0; k < sizeof(once) / sizeof(once[0]); k++)
      if (tbox == once[k]) {
        if (seen[k]) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG stream - found a box of the merging specification twice");
        seen[k] = true;
      }
    if (tbox == id('R', 'S', 'P', 'C')) {
      if (len != 1) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG stream - the size of the refinement spec box is incorrect");
      const long v = byte(0);
      if ((v >> 4) > 4) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG stream - the number of refinement scans must be smaller or equal than four");
      if ((v & 15) > 4) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG stream - the number of residual refinement scans must be smaller or equal than four");
    } else if (tbox == id('O', 'C', 'O', 'N')) {
      if (len != 3) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG stream, Output Conversion box size is invalid");
      const long v = byte(0) & 0xff; // (UBYTE v = stream->Get())
      if ((v >> 4) > 8) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG stream, bit depths cannot be larger than 16");
      if (!(v & 1) && (byte(1) < 0 || byte(2) < 0 || byte(1) != 0 || byte(2) != 0))
        wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG stream, output conversion is disabled, but lookup information is not zero");
    } else if (tbox == id('L', 'D', 'C', 'T') || tbox == id('R', 'D', 'C', 'T')) {
      if (len != 1) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG stream - size of the DCT box is incorrect");
      const long v = byte(0);
      const int t = (int)((v >> 4) & 0xff), ns = (int)(v & 15);
      if (t != 0 && t != 2 && t != 3) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG stream - invalid DCT specified");
      if (ns > 1) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG stream - invalid noise shaping specified");
      if (ns && t != 3) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG stream - cannot enable noise shaping without bypassing the DCT");
    } else if (tbox == id('L', 'T', 'R', 'F') || tbox == id('C', 'T', 'R', 'F') || tbox == id('R', 'T', 'R', 'F') || tbox == id('D', 'T', 'R', 'F') ||
               tbox == id('S', 'T', 'R', 'F')) {
      if (len != 1) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG stream - size of the color transformation box is invalid");
      if (byte(0) & 15) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG stream - the reserved field is not zero");
    } else if (tbox == id('L', 'P', 'T', 'S') || tbox == id('Q', 'P', 'T', 'S') || tbox == id('C', 'P', 'T', 'S') || tbox == id('R', 'P', 'T', 'S') ||
               tbox == id('S', 'P', 'T', 'S') || tbox == id('P', 'P', 'T', 'S') || tbox == id('D', 'P', 'T', 'S')) {
      if (len != 2) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG stream - the size of a non-linear transformation box is incorrect");
    } else if (tbox == id('C', 'U', 'R', 'V')) {
      if (len != 2 + 16) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG file, CURV box size is invalid");
      const int m = (int)(byte(0) & 0xff), ty = m & 15, e = (int)(byte(1) & 0xff);
      if (ty == 3 || ty > 8) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG file, curve type in CURV box is invalid");
      if (e & 15) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG file, the r parameter of the CURV box must be zero");
      if ((e >> 4) > 1) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG file, rounding parameter e must be zero or one");
      if (curve[m >> 4]) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG stream - found an double parametric curve box for the same index");
      curve[m >> 4] = true;
    } else if (tbox == id('M', 'T', 'R', 'X')) {
      if (len != 1 + 18) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "malformed JPEG stream, size of the linear transformation box is inccorrect");
      const long b = byte(0);
      if (b < 0) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "malformed JPEG stream, unexpected EOF while parsing the linear transformation box");
      if ((b >> 4) < 5) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "malformed JPEG stream, the M value of a linear transformation box is out of range");
      if ((b & 15) != 13) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "malformed JPEG stream, the t value of a linear transformation box is invalid");
      if (j + overhead + len > have) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "malformed JPEG stream, unexpected EOF while parsing the linear transformation box");
      if (matrix[b >> 4]) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG stream - found an double linear transformation for the same index");
      matrix[b >> 4] = true;
    } else if (tbox == id('A', 'M', 'U', 'L')) {
      if (amul) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG stream - found a double alpha channel composition box");
      if (!is_alpha)
        wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG stream - found an alpha channel composition box outside of the alpha channel merging specification box");
      amul = true;
      if (len != 2 + 4 * 2) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG stream, the alpha channel composition box size is invalid");
      if ((byte(0) >> 4) > 3) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG stream, the alpha composition method is invalid");
      if ((byte(0) & 15) || byte(1) != 0) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG stream, found invalid values for reserved fields");
    }
    j += xl;
  }
}

// Box::ParseBoxMarker, boxes/box.cpp:93-200: the framing of one APP11 segment; ftyp boxes are checked when complete
// (boxes/filetypebox.cpp:71-120), boxes of unknown type are skipped unseen (Box::CreateBox, box.cpp:391-428).
void RefWalker::box_marker(ByteCursor &s, long length)
{
  long overhead = 2 + 2 + 2 + 4 + 4 + 4;
  if (length <= overhead) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "JPEG stream is malformed, APP11 extended box marker size is too short.");
  const uint16_t en = (uint16_t)s.getword();
  s.getword();
  s.getword(); // sequence number: the segments of a box arrive in order
  uint64_t lbox = (uint64_t)(uint32_t)((unsigned long)s.getword() << 16); // (a -1 at the end of the data shifts like the reference's LONG does)
  lbox |= (uint64_t)(s.getword() & 0xffff);
  long blen = length - overhead;
  if (lbox != 1 && lbox < 8) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "JPEG stream is malformed, box length field is invalid");
  uint32_t tbox = (uint32_t)((unsigned long)s.getword() << 16);
  long dt = s.getword();
  if (dt == ByteCursor::END) wthrow(MIJPEG_ERR_UNEXPECTED_EOF, "JPEG stream is malformed, unexpected end of file while parsing an APP11 marker");
  tbox |= (uint32_t)dt;
  if (lbox == 1) {
    overhead += 8;
    if (length <= overhead) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "JPEG stream is malformed, APP11 extended box marker size is too short.");
    lbox = (uint64_t)(s.getword() & 0xffff) << 48;
    lbox |= (uint64_t)(s.getword() & 0xffff) << 32;
    lbox |= (uint64_t)(s.getword() & 0xffff) << 16;
    dt = s.getword();
    if (dt == ByteCursor::END) wthrow(MIJPEG_ERR_UNEXPECTED_EOF, "JPEG stream is malformed, unexpected end of file while parsing an APP11 marker");
    if (lbox < 8 + 8) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "JPEG stream is malformed, box length field is invalid");
    lbox |= (uint64_t)dt;
    blen -= 8;
    lbox -= 8;
  }
  lbox -= 8;
  switch (tbox) {
  case 0x52455349u: case 0x46494e45u: case 0x5246494eu: case 0x414c4641u: case 0x4146494eu: case 0x41524553u: case 0x41525246u: // RESI FINE RFIN ALFA AFIN ARES ARRF
  case 0x53504543u: case 0x41535043u:                   // SPEC ASPC
  case 0x544f4e45u: case 0x46544f4eu: case 0x43555256u: // TONE FTON CURV
  case 0x4d545258u: case 0x4c43484bu: case 0x66747970u: // MTRX LCHK ftyp
    break;
  default:
    s.skip(blen);
    return;
  }
  XtBox *box = nullptr;
  for (auto &b : hd.boxes_)
    if (b.type == tbox && b.en == en) box = &b;
  if (box) {
    if (box->boxsize != lbox) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "JPEG stream is malformed, box size is not consistent across APP11 markers");
    if (box->complete) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "JPEG stream is malformed, received box data beyond box length");
  } else {
    hd.boxes_.emplace_back();
    box = &hd.boxes_.back();
    box->type = tbox;
    box->en = en;
    box->boxsize = lbox;
    // a box of many segments: room for all of it at once -- as much as the file can still hold -- in the store a box of the
    // last parse left behind where one is big enough (the smallest such)
    // (... as long as all boxes together are promised no more than the file is long: a crafted file of a thousand boxes that
    // each announce what is left of it grows its vectors segment by segment, as before)
    const size_t want = (size_t)std::min<uint64_t>(lbox, (uint64_t)(s.n - s.pos));
    // (a codestream box of many segments is copied when the walk is through, XtBox::pieces; the spare stores keep their old
    // size so that taking one over fills nothing)
    const char *nodefer = getenv("MIJPEG_NO_DEFERRED_BOXES"); // A-B comparisons (read per box: a file has a handful)
    box->deferred = !(nodefer && atoi(nodefer)) && lbox > (uint64_t)blen && (tbox == 0x52455349u || tbox == 0x46494e45u || tbox == 0x5246494eu || tbox == 0x414c4641u ||
                                               tbox == 0x4146494eu || tbox == 0x41524553u || tbox == 0x41525246u);
    if (lbox > (uint64_t)blen && hd.box_bytes_promised_ + want <= s.n) {
      hd.box_bytes_promised_ += want;
      size_t best = SIZE_MAX;
      for (size_t k = 0; k < hd.box_spares_.size(); k++)
        if (hd.box_spares_[k].capacity() >= want && (best == SIZE_MAX || hd.box_spares_[k].capacity() < hd.box_spares_[best].capacity())) best = k;
      if (best != SIZE_MAX) {
        box->data = std::move(hd.box_spares_[best]);
        hd.box_spares_.erase(hd.box_spares_.begin() + (long)best);
        if (!box->deferred) box->data.clear(); // (a box that is filled segment by segment starts empty)
      } else {
        box->data.reserve(want);
        if (box->deferred) box->data.resize(want); // (touched here once; materialize_boxes finds its size in place from then on)
      }
    }
  }
  box->parsed += (uint64_t)blen; // (box.cpp:183-184: what the segment announces -- a file that ends inside the last segment completes the box)
  // ... and DecoderStream::Append (io/decoderstream.cpp:136-158) fills what the stream no longer had with ZEROS (and warns): the
  // box holds every byte it was promised -- a merging specification cut short is "found a box size of zero within a superbox"
  const size_t promised = (size_t)blen;
  if ((size_t)blen > s.n - s.pos) { blen = (long)(s.n - s.pos); warn(); }
  if (box->deferred) {
    box->pieces.push_back(XtBox::Piece{s.d + s.pos, (size_t)blen, promised - (size_t)blen});
    box->pending += promised;
  } else {
    box->data.insert(box->data.end(), s.d + s.pos, s.d + s.pos + blen);
    box->data.resize(box->data.size() + (promised - (size_t)blen), 0);
  }
  s.pos += (size_t)blen;
  if (box->parsed > box->boxsize)
    wthrow(MIJPEG_ERR_MALFORMED_STREAM, "JPEG stream is invalid, more data in the application marker than indicated and required by the box contained within.");
  if (box->parsed == box->boxsize) {
    box->complete = true;
    if (tbox == 0x53504543u) check_merging_spec(box->data.data(), box->data.size(), box->boxsize);
    if (tbox == 0x41535043u) check_merging_spec(box->data.data(), box->data.size(), box->boxsize, true); // ASPC: the alpha channel's
    // Tables and matrices of the file's own list parse where they complete (inversetonemappingbox.cpp:72-118,
    // parametrictonemappingbox.cpp:85-149, lineartransformationbox.cpp:62-99), and a table index / matrix id may be taken once
    // (Tables::ParseTablesIncremental, codestream/tables.cpp:1247-1266; NameSpace::isUniqueNonlinearity counts TONE, FTON and CURV)
    if (tbox == 0x544f4e45u || tbox == 0x43555256u || tbox == 0x4d545258u) {
      const uint64_t n = box->boxsize;
      const std::vector<uint8_t> &d = box->data;
      auto byte = [&](size_t k) -> long { return k < d.size() ? (long)d[k] : -1; };
      if (tbox == 0x544f4e45u) {
        if (n > 65536u * 2 + 1) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG stream, inverse tone mapping box is too large");
        if (!(n & 1) || n < 512) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG stream, number of table entries in the inverse tone mapping box is invalid");
        const uint64_t entries = (n - 1) >> 1;
        if (entries & (entries - 1)) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG stream, number of table entries in the inverse tone mapping box must be a power of two");
      } else if (tbox == 0x43555256u) {
        if (n != 2 + 16) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG file, CURV box size is invalid");
        const int ty = (int)(byte(0) & 15), e = (int)(byte(1) & 0xff);
        if (ty == 3 || ty > 8) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG file, curve type in CURV box is invalid");
        if (e & 15) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG file, the r parameter of the CURV box must be zero");
        if ((e >> 4) > 1) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG file, rounding parameter e must be zero or one");
      } else {
        if (n != 1 + 18) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "malformed JPEG stream, size of the linear transformation box is inccorrect");
        const long b = byte(0);
        if (b < 0 || d.size() < n) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "malformed JPEG stream, unexpected EOF while parsing the linear transformation box");
        if ((b >> 4) < 5) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "malformed JPEG stream, the M value of a linear transformation box is out of range");
        if ((b & 15) != 13) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "malformed JPEG stream, the t value of a linear transformation box is invalid");
      }
      if (tbox != 0x43555256u && !d.empty()) { // (a curve that completes is not checked; it counts when a table does)
        int same = 0;
        for (const auto &o : hd.boxes_) {
          if (!o.complete || o.data.empty() || (o.data[0] >> 4) != (d[0] >> 4)) continue;
          if (tbox == 0x4d545258u ? o.type == 0x4d545258u : (o.type == 0x544f4e45u || o.type == 0x43555256u)) same++;
        }
        if (same > 1)
          wthrow(MIJPEG_ERR_MALFORMED_STREAM, tbox == 0x4d545258u ? "Malformed JPEG stream - found a doubly used table destination for a matrix box"
                                                                   : "Malformed JPEG stream - found a doubly used table destination for a nonlinearity box");
      }
    }
    if (tbox == 0x66747970u) {
      if (box->boxsize < 8) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG stream - file type box is too short to contain brand and minor version");
      if (box->data.size() < 4 || memcmp(box->data.data(), "jpxt", 4) != 0)
        wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG stream - file is not compatible to JPEG XT and cannot be read by this software");
      if ((box->boxsize - 8) & 3)
        wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG stream - number of compatibilities is corrupted, box size is not divisible by entry size");
    }
  }
}

// Tables::ParseTablesIncremental, codestream/tables.cpp:1003-1418.  false: the next marker is not part of the tables/misc
// section (SOFn, SOS, EOI, DHP) or the stream ended.
bool RefWalker::tables_incremental(ByteCursor &s)
{
  const long marker = s.peekword();
  switch (marker) {
  case 0xffdb: s.getword(); parse_dqt(s); break;
  case 0xffc4: s.getword(); parse_dht(s); break;
  case 0xffcc: { // DAC: marker/actable.cpp:119-149, coding/actemplate.cpp:71-107 -- checked, irrelevant to Huffman scans
    s.getword();
    long len = s.getword();
    if (len < 2) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "AC conditioning table length must be at least two bytes long");
    len -= 2;
    while (len > 0) {
      const long t = s.get();
      if (t == ByteCursor::END) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "AC conditioning table marker run out of data");
      len--;
      if ((t >> 4) > 1) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "undefined conditioning table type");
      const long v = s.get();
      if (v == ByteCursor::END) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "unexpected EOF while parsing off the AC conditioning parameters");
      if ((t >> 4) == 1) {
        if (v < 1 || v > 63) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "AC conditoning parameter must be between 1 and 63");
      } else if ((v >> 4) < (v & 0x0f))
        wthrow(MIJPEG_ERR_MALFORMED_STREAM, "upper DC conditioning parameter must be larger or equal to the lower one");
      len--;
    }
    break;
  }
  case 0xffdd: { // marker/restartintervalmarker.cpp:80-102.  The marker object is made where the first DRI stands
    // (codestream/tables.cpp:1045-1047) -- with the JPEG LS lengths, five and six bytes for 24 and 32 bit intervals, when that is
    // the header part of the file (see the LSE marker below) -- and stays
    s.getword();
    if (!dri_seen) { dri_seen = true; dri_extended = header_part; }
    long len = s.getword(), upper = 0;
    if (len < 4 || len > (dri_extended ? 6 : 4)) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "DRI restart interval definition marker size is invalid");
    if (len == 6) upper = s.getword();
    else if (len == 5) upper = s.get();
    len = s.getword();
    if (len == ByteCursor::END) wthrow(MIJPEG_ERR_UNEXPECTED_EOF, "DRI restart interval definition marker run out of data");
    if (upper != 0) wthrow(MIJPEG_ERR_OPERATION_UNIMPLEMENTED, "restart intervals beyond 16 bits are not on the accelerated path");
    hd.restart_interval_ = (int)(len & 0xffff);
    break;
  }
  case 0xfffe: {
    s.getword();
    const long size = s.getword();
    if (size == ByteCursor::END) wthrow(MIJPEG_ERR_UNEXPECTED_EOF, "COM marker incomplete, stream truncated");
    if (size <= 2) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "COM marker size out of range");
    s.skip(size - 2);
    break;
  }
  case 0xfff8: {
    // LSE, the JPEG LS extensions marker.  The header part of the file in front of the frame header is parsed with `isls` TRUE
    // (Decoder::ParseHeaderIncremental, codestream/decoder.cpp:85: the frame type is not known yet): the marker is read there
    // (codestream/tables.cpp:1073-1110, marker/thresholds.cpp:84-94, marker/lscolortrafo.cpp:120-169) and means nothing to a DCT
    // frame; behind the frame header, and in the codestreams of boxes, it is "outside of a JPEG LS stream".
    if (!header_part) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "found LSE marker outside of JPEG LS stream");
    s.getword();
    long len = s.getword();
    if (len > 3) {
      const int id = (int)(s.get() & 0xff);
      if (id == 1) { // thresholds
        if (len != 13) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "LSE marker length is invalid");
        for (int k = 0; k < 5; k++) s.getword();
        break;
      } else if (id == 2 || id == 3) {
        wthrow(MIJPEG_ERR_OPERATION_UNIMPLEMENTED, "JPEG LS mapping tables are not implemented by this code, sorry");
      } else if (id == 4) {
        wthrow(MIJPEG_ERR_OPERATION_UNIMPLEMENTED, "JPEG LS size extensions are not implemented by this code, sorry");
      } else if (id == 0x0d) { // the LS colour transformation
        if (ls_trafo_seen) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "found duplicate JPEG LS color transformation specification");
        ls_trafo_seen = true;
        if (len < 6) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "length of the LSE color transformation marker is invalid, must be at least six bytes long");
        s.getword();
        const int depth = (int)(s.get() & 0xff);
        len -= 6;
        if (len != 2 * depth * depth) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "length of the LSE color transformation marker is invalid");
        if (depth == 0) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "number of components in the LSE color transformation marker must not be zero");
        for (int k = 0; k < depth; k++) s.get();
        for (int k = 0; k < depth; k++) {
          const int v = (int)(s.get() & 0xff);
          if ((v & 0x7f) > 32) wthrow(MIJPEG_ERR_OVERFLOW_PARAMETER, "LSE color transformation marker shift value is too large, must be < 32");
          for (int j = 0; j + 1 < depth; j++) s.getword();
        }
        break;
      } else {
        warn(); // "skipping over unknown JPEG LS extensions marker"
        len--;
      }
    }
    if (len <= 2) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "marker size out of range");
    s.skip(len - 2);
    break;
  }
  case 0xffe0: { // APP0: a JFIF marker is checked (marker/jfifmarker.cpp:103-129)
    s.getword();
    long len = s.getword();
    if (len >= 2 + 5 + 2 + 1 + 2 + 2 + 1 + 1) {
      const char *id = "JFIF";
      while (*id) { len--; if (s.get() != *id) break; id++; }
      if (*id == 0) {
        len--;
        if (s.get() == 0) {
          long l = (len + 5) & 0xffff;
          if (l < 2 + 5 + 2 + 1 + 2 + 2 + 1 + 1) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "malformed JFIF marker");
          s.get();
          s.get();
          if ((s.get() & 0xff) > 2) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "JFIF specified unit is invalid");
          s.getword();
          s.getword();
          l -= 2 + 5 + 2 + 1 + 2 + 2;
          s.skip(l);
          break;
        }
      }
    }
    if (len <= 2) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "marker size out of range");
    s.skip(len - 2);
    break;
  }
  case 0xffe1: { // APP1: the Exif header is checked (marker/exifmarker.cpp:117-128)
    s.getword();
    long len = s.getword();
    if (len >= 2 + 4 + 2 + 2 + 2 + 4 + 2) {
      const char *id = "Exif";
      while (*id) { len--; if (s.get() != *id) break; id++; }
      if (*id == 0) {
        len -= 2;
        if (s.getword() == 0) {
          long l = (len + 4 + 2) & 0xffff;
          if (l < 2 + 4 + 2 + 2 + 2 + 4 + 2 + 4) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "malformed EXIF marker");
          s.skip(l - (2 + 4 + 2));
          break;
        }
      }
    }
    if (len < 2) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "marker size out of range");
    s.skip(len - 2);
    break;
  }
  case 0xffeb: { // APP11: JPEG XT boxes
    s.getword();
    const long len = s.getword();
    if (len >= 2 + 2 + 2 + 4 + 4 + 4 && s.peekword() == 0x4a50) {
      s.getword();
      if (hd.nested_) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Found a box in the residual codestream.");
      box_marker(s, len & 0xffff);
      break;
    }
    if (len < 2) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "marker size out of range");
    s.skip(len - 2);
    break;
  }
  case 0xffee: { // APP14: Adobe, only at its exact size (marker/adobemarker.cpp:96-117)
    s.getword();
    long len = s.getword();
    if (len == 2 + 5 + 2 + 2 + 2 + 1) {
      const char *id = "Adobe";
      while (*id) { len--; if (s.get() != *id) break; id++; }
      if (*id == 0) {
        const long version = s.getword() & 0xffff;
        if (version != 100 && version != 101) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Adobe marker version unrecognized");
        s.getword();
        s.getword();
        const long color = s.get();
        if (color < 0 || color > 2) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Adobe color information unrecognized");
        hd.adobe_transform_ = (int)color;
        break;
      }
    }
    if (len < 2) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "marker size out of range");
    s.skip(len - 2);
    break;
  }
  case 0xffdf: wthrow(MIJPEG_ERR_MALFORMED_STREAM, "found an EXP marker outside a hierarchical process");
  case 0xffc8: {
    s.getword();
    const long len = s.getword();
    if (len < 2) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "marker size out of range");
    s.skip(len - 2);
    break;
  }
  case 0xffc0: case 0xffc1: case 0xffc2: case 0xffc3: case 0xffc5: case 0xffc6: case 0xffc7: case 0xffc9: case 0xffca:
  case 0xffcb: case 0xffcd: case 0xffce: case 0xffcf: case 0xffb1: case 0xffb2: case 0xffb3: case 0xffb9: case 0xffba:
  case 0xffbb: case 0xffd9: case 0xffda: case 0xffde: case 0xfff7:
    return false;
  case 0xffff: s.get(); break; // a filler byte
  case 0xffd0: case 0xffd1: case 0xffd2: case 0xffd3: case 0xffd4: case 0xffd5: case 0xffd6: case 0xffd7:
    s.getword();
    warn(); // stray restart marker
    break;
  default:
    if (marker >= 0xffc0 && (marker < 0xffd0 || marker >= 0xffd8) && marker < 0xfff0) {
      s.getword();
      const long size = s.getword();
      if (size == ByteCursor::END) wthrow(MIJPEG_ERR_UNEXPECTED_EOF, "marker incomplete, stream truncated");
      if (size <= 2) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "marker size out of range");
      s.skip(size - 2);
    } else {
      warn(); // "found invalid marker, probably a marker size is out of range": on to the next FF
      s.get();
      long dt;
      do dt = s.get(); while (dt != 0xff && dt != ByteCursor::END);
      if (dt == 0xff) s.lastundo();
      else return false;
    }
  }
  return true;
}

// Image::ParseFrameHeader / CreateFrameBuffer (codestream/image.cpp:616-650, 480-607), Frame::ParseMarker
// (marker/frame.cpp:111-208), Component::ParseMarker (marker/component.cpp:86-111)
void RefWalker::frame_header(ByteCursor &s)
{
  mijpeg_info &f = hd.info;
  long marker = s.peekword();
  if (marker == ByteCursor::END) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "unexpected EOF while parsing the image");
  if (marker == 0xffd9) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "unexpected EOI marker while parsing the image");
  marker = s.getword();
  int type = -1;
  switch (marker) {
  case 0xffc0: type = 0; break;
  case 0xffc1: type = 1; break;
  case 0xffc2: type = 2; break;
  // residual sequential (part 8: what the reference's encoder puts into the RESI box for -ro / -Q 100): a frame type inside a
  // residual codestream only
  case 0xffb1: if (hd.nested_) type = 3; break;
  // residual progressive (`-rv` beside `-ro` / `-Q 100`): the same scans with spectral bands, successive approximation and EOB runs
  case 0xffb2: if (hd.nested_) type = 4; break;
  case 0xffc5: case 0xffc6: case 0xffc7: case 0xffcd: case 0xffce: case 0xffcf:
    // Image::CreateFrameBuffer, codestream/image.cpp:487-500, in front of everything else: the header is not even read (and a DHP
    // marker, the only way into a hierarchical process, is declined below)
    wthrow(MIJPEG_ERR_MALFORMED_STREAM, "found a differential frame outside a hierarchical image process");
  case 0xffc3: case 0xffc9: case 0xffca: case 0xffcb:
  case 0xffb3: case 0xffb9: case 0xffba: case 0xffbb: case 0xfff7: case 0xffde:
    break;
  default: wthrow(MIJPEG_ERR_MALFORMED_STREAM, "unexpected marker while parsing the image, decoder out of sync");
  }
  if (hd.have_frame_) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "found a double frame header");
  // A frame type outside the accelerated path is declined -- behind the checks Frame::ParseMarker makes on every header
  // (marker/frame.cpp:111-208): a damaged byte that happens to spell such a marker in front of garbage is the reference's
  // "frame header marker size is invalid", not a coding process this library does not know.
  const bool declined_type = type < 0;
  const bool lossless_kind = marker == 0xffc3 || marker == 0xffc7 || marker == 0xffcb || marker == 0xffcf || marker == 0xfff7;
  const bool residual_kind = marker == 0xffb1 || marker == 0xffb2 || marker == 0xffb3 || marker == 0xffb9 || marker == 0xffba || marker == 0xffbb;
  if (declined_type) type = residual_kind ? 3 : lossless_kind ? -2 : (marker == 0xffca || marker == 0xffce) ? 2 : 1; // (marker/frame.cpp:163-170: four components at most for these two)
  hd.frame_type_ = type;
  hd.progressive_ = type == 2;
  long len = s.getword();
  if (len < 8) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "start of frame marker size invalid");
  f.precision = (int)(s.get() & 0xff);
  if (type == -2) { // marker/frame.cpp:122-131
    if (f.precision < 2 || f.precision > 16) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "frame precision in lossless mode must be between 2 and 16");
  } else if (type >= 3) { // marker/frame.cpp:132-140
    if (f.precision < 2 || f.precision > 17) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "frame precision in residual mode must be between 2 and 17");
  } else if (type == 0 ? f.precision != 8 : (f.precision != 8 && f.precision != 12))
    wthrow(MIJPEG_ERR_MALFORMED_STREAM, type == 0 ? "frame precision in baseline mode must be 8" : "frame precision in lossy mode must be 8 or 12");
  f.sample_bytes = f.precision > 8 ? 2 : 1;
  long data = s.getword();
  if (data == ByteCursor::END) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "frame marker run out of data");
  f.height = (int)data;
  data = s.getword();
  if (data == ByteCursor::END) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "frame marker run out of data");
  if (data == 0) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "image width must not be zero");
  f.width = (int)data;
  data = s.get();
  if (data == ByteCursor::END) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "frame marker run out of data");
  if (data <= 0 || data > (type == 2 ? 4 : 255))
    wthrow(MIJPEG_ERR_MALFORMED_STREAM, type == 2 ? "number of components must be between 1 and 4 for progressive mode" : "number of components must be between 1 and 255");
  len -= 8;
  if (len != 3 * data) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "frame header marker size is invalid");
  if (declined_type)
    wthrow(MIJPEG_ERR_OPERATION_UNIMPLEMENTED, "only Huffman sequential and progressive frames (SOF0/SOF1/SOF2) are on the accelerated path");
  // (Tables::LTrafoTypeOf, codestream/tables.cpp:2024-2028: an LSE colour transformation in the header part becomes the colour
  // transformation of a three component frame, DCT or not)
  if (ls_trafo_seen && data == 3) wthrow(MIJPEG_ERR_OPERATION_UNIMPLEMENTED, "the JPEG LS colour transformation is not on the accelerated path");
  if (data > MIJPEG_MAX_COMPONENTS) wthrow(MIJPEG_ERR_OPERATION_UNIMPLEMENTED, "frames of more than four components are not on the accelerated path");
  f.components = (int)data;
  int hmax = 0, vmax = 0;
  for (int c = 0; c < f.components; c++) {
    data = s.get();
    if (data == ByteCursor::END) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "frame marker incomplete, no component identifier found");
    hd.comp_id_[c] = (int)data;
    data = s.get();
    if (data == ByteCursor::END) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "frame marker incomplete, subsamling information missing");
    f.hsamp[c] = (int)(data >> 4);
    f.vsamp[c] = (int)(data & 15);
    if (f.hsamp[c] == 0 || f.vsamp[c] == 0) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "frame marker corrupt, MCU size cannot be 0");
    data = s.get();
    if (data < 0 || data > 3) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "quantization table identifier corrupt, must be >= 0 and <= 3");
    f.quant_index[c] = (int)data;
    hmax = std::max(hmax, f.hsamp[c]);
    vmax = std::max(vmax, f.vsamp[c]);
  }
  for (int c = 0; c < f.components; c++)
    if (hmax % f.hsamp[c] || vmax % f.vsamp[c])
      wthrow(MIJPEG_ERR_OPERATION_UNIMPLEMENTED, "non-integer subsampling factors are not supported by this implementation, sorry");
  hd.need_dnl_ = f.height == 0; // the number of lines follows the first scan in a DNL marker (entropyparser.cpp:204-249)
  f.dnl = hd.need_dnl_ ? 1 : 0;
  const int rc = hd.frame_geometry();
  if (rc) wthrow(rc, "frame dimensions require an unreasonably large coefficient store");
  // Image::CreateFrameBuffer ends with PrepareForDecoding (image.cpp:604-607): upsamplers exist for factors up to 4
  for (int c = 0; c < f.components; c++) {
    if (f.subx[c] > 4 || f.suby[c] > 4) wthrow(MIJPEG_ERR_OPERATION_UNIMPLEMENTED, "subsampling factors larger than 4x4 are not supported, sorry");
  }
  hd.have_frame_ = true;
}

// Frame::ScanForScanHeader, marker/frame.cpp:863-899
bool RefWalker::scan_for_scan_header(ByteCursor &s)
{
  long data = s.getword();
  if (data != 0xffda) {
    warn(); // "Start of Scan SOS marker missing"
    if (data == ByteCursor::END) return false;
    do {
      s.lastundo();
      do data = s.get(); while (data != 0xff && data != ByteCursor::END);
      if (data == ByteCursor::END) break;
      s.lastundo();
      data = s.getword();
      if (data == ByteCursor::END) break;
    } while (data != 0xffda);
  }
  return data == 0xffda;
}

// Frame::ParseTrailer, marker/frame.cpp:1016-1123.  true: another scan follows.
bool RefWalker::frame_trailer(ByteCursor &s)
{
  // The residual codestream at its end: Image::InputStreamOf (codestream/image.cpp:978-996) hands out the LEGACY stream instead,
  // and that one stands at its EOI (it stays in the buffer while the residual codestream is read, image.cpp:1416-1431).  A
  // residual frame whose data simply ends is therefore at "its" EOI, and its hidden refinement scans are read.
  if (hd.nested_ && !legacy_eoi_gone && s.peekword() == ByteCursor::END) {
    frame_eoi = true;
    // (... which hangs on where the scan's decoder stopped, to the byte: one whose data went wrong -- a byte too many in it --
    // is through with its blocks a byte or two in front of the end, finds garbage here instead of the end, and the frame
    // has no EOI.  The planning walk only knows where the segment ends; a residual codestream without an EOI marker is no
    // encoder's work anyway: the sequential walk decides.  tools/xt_gpu_damage_campaign.py, seed 2001.)
    if (mode == PLAN) hd.needs_sequential_ = true;
    return false;
  }
  for (;;) {
    long marker = s.peekword();
    switch (marker) {
    case 0xffb1: case 0xffb2: case 0xffb3: case 0xffb9: case 0xffba: case 0xffbb: case 0xffc0: case 0xffc1: case 0xffc2:
    case 0xffc3: case 0xffc9: case 0xffca: case 0xffcb: case 0xfff7: case 0xffde: case 0xffc5: case 0xffc6: case 0xffc7:
    case 0xffcd: case 0xffce: case 0xffcf:
      warn();
      return false;
    case 0xffda: return true;
    case 0xffd9: frame_eoi = true; return false;
    case 0xffff: s.get(); break;
    case 0xffd0: case 0xffd1: case 0xffd2: case 0xffd3: case 0xffd4: case 0xffd5: case 0xffd6: case 0xffd7:
      s.getword();
      warn();
      break;
    case ByteCursor::END: warn(); return false; // "missing an EOI marker at the end of the stream"
    default:
      if (marker < 0xff00) {
        warn(); // "expecting a marker or marker segment - stream is out of sync"
        s.get();
        do marker = s.get(); while (marker != 0xff && marker != ByteCursor::END);
        if (marker == ByteCursor::END) { warn(); return false; }
        s.lastundo();
      } else {
        while (tables_incremental(s)) {}
      }
    }
  }
}

// Image::ParseTrailer, codestream/image.cpp:1408-1497.  true: something that is not the end follows.
bool RefWalker::image_trailer(ByteCursor &s)
{
  for (bool first = true;; first = false) {
    long marker = s.peekword();
    if (marker == 0xffd9) { image_eoi = true; s.getword(); return false; }
    if (marker == 0xffff) { s.get(); continue; }
    if (marker == ByteCursor::END) { if (!(hd.nested_ && first && !legacy_eoi_gone)) warn(); return false; } // (image.cpp:1320-1323: a residual codestream may simply end)
    if (marker >= 0xff00) return true;
    warn();
    s.get();
    do marker = s.get(); while (marker != 0xff && marker != ByteCursor::END);
    if (marker == ByteCursor::END) { warn(); return false; }
    s.lastundo();
  }
}

void RefWalker::run()
{
  ByteCursor &s = io;
  if (s.getword() != 0xffd8) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "stream does not contain a JPEG file, SOI marker missing");
  header_part = !hd.nested_ && !hd.alpha_child_;
  while (tables_incremental(s)) {}
  header_part = false;
  for (;;) {
    frame_header(s);
    for (;;) {
      while (tables_incremental(s)) {}
      // (a residual codestream that is through here: the search for a scan header works on the legacy stream -- InputStreamOf, see
      // frame_trailer -- and takes its EOI away: one warning like at the end of this stream, but the trailers that follow find
      // the end of the file, not an EOI)
      if (hd.nested_ && s.peekword() == ByteCursor::END) legacy_eoi_gone = true;
      if (scan_for_scan_header(s)) {
        scan(s, false);
        if (mode == HEADER) return;
        if (frame_trailer(s)) continue;
        if (!image_trailer(s)) return;
        // The residual codestream: Image::ParseResidualStream (codestream/image.cpp:1318-1331) hands the SAME frame back when its
        // image trailer finds a marker (the parent's m_pCurrent, m_bReceivedFrameHeader set): no frame header is read, the frame
        // goes on looking for scans
        // (... and Image::ParseAlphaChannel, image.cpp:1386-1397, does the same for the alpha channel's codestream)
        if (hd.nested_ || hd.alpha_child_) continue;
        break; // a second frame header follows: it throws
      }
      if (frame_trailer(s)) continue;
      if (!image_trailer(s)) return;
      if (hd.nested_ || hd.alpha_child_) continue;
      wthrow(MIJPEG_ERR_MALFORMED_STREAM, "no scan found in front of the next frame"); // the reference dereferences a NULL frame here
    }
  }
}

void RefWalker::run_hidden(const uint8_t *box, size_t size)
{
  ByteCursor s(box, size);
  s.in_memory = true;
  scan_base = box;
  while (tables_incremental(s)) {}
  if (scan_for_scan_header(s)) scan(s, true);
  scan_base = nullptr;
}

// Scan::ParseMarker (marker/scan.cpp:163-315), Scan::CreateParser / StartParseScan (:355-470, 985-994),
// SequentialScan::StartParseScan (codestream/sequentialscan.cpp:112-141), BlockBuffer::ResetToStartOfScan
// (control/blockbuffer.cpp:177-208).  hidden: the scan comes from a FINE / RFIN box
// (Scan::StartParseHiddenRefinementScan, marker/scan.cpp:899-980).
void RefWalker::scan(ByteCursor &s, bool hidden)
{
  mijpeg_info &f = hd.info;
  Scan sc;
  // (the hidden scans of a frame of the residual kind are parsed as residual progressive scans and refine from position 0 on:
  // RefinementScan(.., residual), marker/scan.cpp:941-953)
  const bool residual_frame = hd.frame_type_ == 3 || hd.frame_type_ == 4;
  const int type = hidden ? (residual_frame ? 4 : 2) : hd.frame_type_;
  const long len = s.getword();
  if (len < 8) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "marker length of the SOS marker invalid, must be at least 8 bytes long");
  long data = s.get();
  if (data < 1 || data > 4) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "number of components in scan is invalid, must be between 1 and 4");
  sc.ncomp = (int)data;
  if (len != sc.ncomp * 2 + 6) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "length of the SOS marker is invalid");
  int id[MIJPEG_MAX_COMPONENTS];
  for (int i = 0; i < sc.ncomp; i++) {
    data = s.get();
    if (data == ByteCursor::END) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "SOS marker run out of data");
    id[i] = (int)data;
    for (int j = 0; j < i; j++)
      if (id[j] == id[i]) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "SOS includes the same component twice");
    data = s.get();
    if (data == ByteCursor::END) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "SOS marker run out of data");
    sc.sc[i].td = (int)(data >> 4);
    sc.sc[i].ta = (int)(data & 15);
    if (sc.sc[i].td > 3) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "DC table index in SOS marker is out of range, must be at most 4");
    if (sc.sc[i].ta > 3) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "AC table index in SOS marker is out of range, must be at most 4");
  }
  data = s.get();
  if (data == ByteCursor::END) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "SOS marker run out of data");
  if (data > 63) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "start of scan index is out of range, must be between 0 and 63");
  sc.ss = (int)data;
  data = s.get();
  if (data == ByteCursor::END) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "SOS marker run out of data");
  if (data > 63) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "end of scan index is out of range, must be between 0 and 63");
  sc.se = (int)data;
  data = s.get();
  if (data == ByteCursor::END) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "SOS marker run out of data");
  sc.ah = (int)(data >> 4);
  sc.al = (int)(data & 15);
  if (sc.ah > 13) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "SOS high bit approximation is out of range, must be < 13");
  if (type == 2) {
    if (sc.ah && sc.ah != sc.al + 1) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "SOS high bit is invalid, successive approximation must refine by one bit per scan");
    if (sc.se < sc.ss) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "end of scan is lower than start of scan");
    if (sc.ss == 0 && sc.se != 0) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "DC component must be in a separate scan in the progressive mode");
    if (sc.ss && sc.ncomp != 1) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "AC scans in progressive mode must only contain a single component");
  } else if (type == 3 || type == 4) {
    // marker/scan.cpp:262-272; Scan::CreateParser: Residual -> SequentialScan(.., differential, residual) whatever Ah says (:483-489),
    // ResidualProgressive -> that for Ah = 0, RefinementScan(.., residual) behind it (:411-424): no DC scans, bands start at 0
    if (sc.ah && sc.ah != sc.al + 1) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "SOS high bit is invalid, successive approximation must refine by one bit per scan");
    if (sc.se < sc.ss) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "end of scan is lower than start of scan");
    sc.residual = true;
    hd.needs_sequential_ = true; // (the walk decodes these: no DC part, symbol 0x10 -- not the parallel block decoders' business)
  } else {
    if (sc.se != 63 || sc.ss != 0) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "scan start must be zero and scan stop must be 63 for the sequential operating modes");
    if (sc.ah != 0) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "successive approximation parameters must be zero for the sequential operating modes");
  }
  if (hidden && sc.ah != sc.al + 1) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "SOS high bit is invalid, hidden refinement must refine by one bit per scan");
  const bool refinement = hidden || ((type == 2 || type == 4) && sc.ah != 0);
  // the sequential parser decodes a point transform as well: Al is not checked for sequential frames and moves the
  // coefficients up; EOB runs become legal then (m_bProgressive, sequentialscan.cpp:84-87)
  const int lowbit = hidden ? sc.al : sc.al + hd.hidden_;
  const bool progressive_run = sc.ss > 0 || sc.se < 63 || lowbit > hd.hidden_;
  // Scan::CreateParser: every component of the scan must exist (Frame::FindComponent)
  for (int i = 0; i < sc.ncomp; i++) {
    int c = 0;
    while (c < f.components && hd.comp_id_[c] != id[i]) c++;
    if (c == f.components) wthrow(MIJPEG_ERR_OBJECT_DOESNT_EXIST, "found a component ID that does not exist");
    sc.sc[i].comp = c;
  }
  // Huffman decoders: Tables::FindDC/ACHuffmanTable (tables.cpp:1423-1452); a table no DHT marker defined is one of the
  // reference's default tables (marker/huffmantable.cpp:186-228) -- for 8-bit sequential frames the Annex K.3 tables
  auto table_for = [&](HuffTable &h, bool ac, int idx) -> const HuffTable & {
    if (!hd.have_huff_) wthrow(MIJPEG_ERR_OBJECT_DOESNT_EXIST, "DHT marker missing for Huffman encoded scan");
    if (!h.defined) {
      if (type == 2 || f.precision != 8)
        wthrow(MIJPEG_ERR_OPERATION_UNIMPLEMENTED, "scan selects a Huffman table the stream does not define (default tables of this frame type are not on the accelerated path)");
      EncTables std_tabs;
      enc_standard_tables(std_tabs);
      const EncTable &t = ac ? std_tabs.ac[idx != 0] : std_tabs.dc[idx != 0];
      memcpy(h.counts, t.counts, 16);
      memcpy(h.values, t.values, 256);
      h.defined = true;
      h.built = false;
      h.oversize = false;
    }
    if (h.oversize) wthrow(MIJPEG_ERR_INVALID_HUFFMAN, "Huffman table with more than 256 code words is not on the accelerated path");
    if (!h.built) {
      if (!h.build()) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "Huffman table corrupt - entry depends on more bits than available for the bit length");
      h.built = true;
    }
    return h;
  };
  for (int i = 0; i < sc.ncomp; i++) {
    if (sc.ss == 0 && !refinement && !sc.residual) sc.dc[i] = table_for(hd.dc_[sc.sc[i].td], false, sc.sc[i].td);
    if (sc.se || (sc.residual && refinement)) sc.ac[i] = table_for(hd.ac_[sc.sc[i].ta], true, sc.sc[i].ta); // (refinementscan.cpp:104)
  }
  // the transform of a component is built, with the quantiser table in force NOW, when the component first appears
  // in a scan (control/blockbuffer.cpp:177-208, codestream/tables.cpp:1741-1750)
  for (int i = 0; i < sc.ncomp; i++) {
    const int c = sc.sc[i].comp;
    if (!hd.comp_seen_[c]) {
      const int tq = f.quant_index[c];
      if (hd.nested_ && (!hd.have_quant_ || !hd.quant_defined_[tq])) {
        // The RESIDUAL image's transforms are not built at the start of a scan: ResidualBlockHelper::AllocateBuffers builds them (and
        // looks the quantiser tables up, codestream/tables.cpp:1481-1494, 1750) when the first block is dequantised -- at the first
        // request for pixels.  Whatever stops either codestream, and what the colour transformer refuses, comes first.
        hd.late_quant_missing_ = hd.have_quant_ ? "requested quantization matrix not defined" : "DQT marker missing, no quantization table defined";
        memset(hd.comp_quant_[c], 0, sizeof(hd.comp_quant_[c]));
        hd.comp_seen_[c] = true;
        continue;
      }
      if (!hd.have_quant_) wthrow(MIJPEG_ERR_OBJECT_DOESNT_EXIST, "DQT marker missing, no quantization table defined");
      if (!hd.quant_defined_[tq]) wthrow(MIJPEG_ERR_OBJECT_DOESNT_EXIST, "requested quantization matrix not defined");
      memcpy(hd.comp_quant_[c], hd.quant_[tq], sizeof(hd.comp_quant_[c]));
      hd.comp_seen_[c] = true;
    }
  }
  if (!hidden) f.progressive = hd.progressive_ ? 1 : 0;
  sc.restart_interval = hd.restart_interval_;
  f.restart_interval = hd.restart_interval_;
  scan_for_dnl = hd.need_dnl_; // EntropyParser::EntropyParser, codestream/entropyparser.cpp:79
  if (hd.need_dnl_) {
    // The frame header carried zero lines: the height follows this scan in a DNL marker, and the reference finds it WHILE it
    // decodes -- it looks at the byte stream in front of every MCU, where its bit reader's prefetch happens to stand
    // (decode_scan below).  What it makes of the scan MCU by MCU is the literal walk's business, not the parallel decoders'.
    hd.needs_sequential_ = true;
    if (hd.dnl_height_ == 0) {
      // first walk of this stream: decode the scan once without keeping anything, for the height it comes to (or the error)
      // and the block rows it makes
      ByteCursor t = s;
      Scan probe = sc;
      probe.mcus_x = sc.ncomp > 1 ? f.mcus_x : (((f.width + f.subx[sc.sc[0].comp] - 1) / f.subx[sc.sc[0].comp]) + 7) >> 3;
      discover = true;
      decode_scan<int32_t>(t, probe, refinement, progressive_run, lowbit); // (int32: what the coefficients hold is not the question here)
      discover = false;
      // (decode_scan has set the height and the geometry when it met the marker; it throws when it does not meet one)
    } else {
      f.height = hd.dnl_height_;
      const int grc = hd.frame_geometry();
      if (grc) wthrow(grc, "frame dimensions require an unreasonably large coefficient store");
      hd.need_dnl_ = false;
    }
  }
  if (sc.ncomp > 1) {
    sc.mcus_x = f.mcus_x;
    sc.mcus_y = f.mcus_y;
  } else {
    // single component scan: 1x1 MCUs over the component's own block grid (sequentialscan.cpp:396-397)
    const int c = sc.sc[0].comp;
    const int cw = (f.width + f.subx[c] - 1) / f.subx[c], ch = (f.height + f.suby[c] - 1) / f.suby[c];
    sc.mcus_x = (cw + 7) >> 3;
    sc.mcus_y = (ch + 7) >> 3;
  }
  sc.ecs_begin = s.pos;
  sc.base = scan_base;
  sc.refinement = refinement;
  sc.progressive_run = progressive_run;
  sc.lowbit = lowbit;
  if (mode == HEADER) return;
  if (mode == DECODE) {
    const size_t begin = s.pos;
    const bool dnl_scan_now = scan_for_dnl;
    if (wide) decode_scan<int32_t>(s, sc, refinement, progressive_run, lowbit);
    else decode_scan<int16_t>(s, sc, refinement, progressive_run, lowbit);
    // (a DNL frame's first scan is walked twice -- once to find the height: the walk that keeps the coefficients counts)
    // (... and the scan that brings the DNL marker starts as many MCU rows as it takes to find it: one more than the frame has
    // where the marker only shows at the first MCU of the next row, EntropyParser::BeginReadMCU, entropyparser.hpp:147-160)
    if (!discover) hd.walked_scans_.push_back(HostDecoder::WalkedScan{begin, s.pos, sc.mcus_x, dnl_scan_now ? rows_entered : sc.mcus_y, scan_base != nullptr});
    return;
  }
  // PLAN: find the restart intervals; the walk goes on behind the segment as it does behind a well-formed one
  hd.scans.push_back(std::move(sc));
  Scan &ps = hd.scans.back();
  if (hidden && hd.deferred_hidden_) {
    // the boxes of a frame's hidden scans hold nothing behind their one scan: the searches for their restart markers -- with
    // restart intervals of a few blocks one marker every few dozen bytes, megabytes of them -- run side by side when all boxes
    // have been looked at (add_hidden_scans), and so does what is checked behind them
    hd.deferred_hidden_->push_back(HostDecoder::DeferredSearch{hd.scans.size() - 1, s.d, s.n, type, hidden});
    hd.scan_interval_end_.emplace_back();
    hd.scan_rst_code_.emplace_back();
    s.pos = s.n;
    s.at_eof = false;
    return;
  }
  if (!hidden && hd.progressive_ && !hd.need_dnl_ && hd.defer_progressive_scans()) {
    // The scans of a progressive frame: the walk only needs to know where a scan's data ends to go on; the searches for the restart
    // markers of all scans -- with restart intervals of a few blocks the larger part of the parse -- run side by side when the walk
    // is through (HostDecoder::run_deferred_searches), and what is checked behind a search is checked there.  Whatever the walk
    // meets behind a scan that turns out to be ill-formed is the sequential walk's business, as it always was (parse()).
    const size_t term = hd.segment_end(s.d, s.n, ps.ecs_begin);
    hd.deferred_scans_.push_back(HostDecoder::DeferredSearch{hd.scans.size() - 1, s.d, term, type, false});
    hd.scan_interval_end_.emplace_back();
    hd.scan_rst_code_.emplace_back();
    ps.ecs_end = term;
    s.pos = term;
    s.at_eof = false;
    return;
  }
  if (hd.active_skip_ && !hidden && hd.scans.size() == 1 && (type == 0 || type == 1) && f.precision == 8 && !hd.need_dnl_ && !hd.needs_sequential_ &&
      !hd.nested_ && !hd.alpha_child_ && hd.boxes_.empty() && ps.al == 0 && ps.ncomp == f.components && s.d == hd.data_ &&
      s.n == hd.size_ && s.n >= ps.ecs_begin + 2 && s.d[s.n - 2] == 0xff && s.d[s.n - 1] == 0xd9) {
    // The device searches this segment (set_skip_search).  The walk goes on at the EOI the stream ends in; whether the segment
    // really runs up to there, with the markers the MCU count asks for in sequence, is the device's verdict (markers.hpp), and a
    // caller that gets another one parses again the ordinary way.
    hd.active_skip_ = false;
    ps.search_skipped = true;
    ps.ecs_end = s.n - 2;
    hd.scan_interval_end_.emplace_back();
    hd.scan_rst_code_.emplace_back();
    s.pos = ps.ecs_end;
    s.at_eof = false;
    return;
  }
  {
    const uint8_t *keep_d = hd.data_;
    const size_t keep_n = hd.size_;
    hd.data_ = s.d;
    hd.size_ = s.n;
    hd.find_intervals(ps);
    hd.data_ = keep_d;
    hd.size_ = keep_n;
  }
  hd.scan_interval_end_.push_back(hd.interval_end_);
  hd.scan_rst_code_.push_back(hd.rst_code_);
  // well-formed: exactly the restart markers the MCU count asks for, in sequence (anything else resynchronises)
  const int64_t total_mcus = (int64_t)ps.mcus_x * ps.mcus_y;
  const int64_t ri = ps.restart_interval ? ps.restart_interval : total_mcus;
  const int64_t nint = (total_mcus + ri - 1) / ri;
  if ((int64_t)ps.interval_begin.size() != nint) hd.needs_sequential_ = true;
  else
    for (int64_t i = 0; i + 1 < nint; i++)
      if (hd.rst_code_[(size_t)i] != 0xd0 + (i & 7)) hd.needs_sequential_ = true;
  // a point transform in a sequential frame (no encoder writes one; a flipped byte does): the reference's sequential parser
  // applies it and accepts EOB runs then (sequentialscan.cpp:84-87) -- the walk's business, not the block decoders'
  if (type != 2 && !hidden && hd.hidden_ == 0 && ps.al != 0) hd.needs_sequential_ = true;
  s.pos = ps.ecs_end;
  s.at_eof = false;
  if (hd.needs_sequential_ && !hidden) throw WalkError{0, "damaged scan"}; // nothing behind it can be planned
}

// The MCU loop of JPEG::ReadInternal (interface/jpeg.cpp:318-348) with SequentialScan::ParseMCU / DecodeBlock
// (codestream/sequentialscan.cpp:381-428, 678-773), RefinementScan::ParseMCU / DecodeBlock
// (codestream/refinementscan.cpp:305-345, 584-700), EntropyParser::BeginReadMCU / ParseRestartMarker
// (codestream/entropyparser.hpp:147-160, entropyparser.cpp:117-201) and the Restart() methods.
template <class T>
void RefWalker::decode_scan(ByteCursor &s, const Scan &sc, bool refinement, bool progressive_run, int lowbit)
{
  const mijpeg_info &f = hd.info;
  const uint8_t *zz = scan_order();
  T *store = (T *)coef;
  RefBits bits;
  bits.open(&s);
  int32_t pred[MIJPEG_MAX_COMPONENTS] = {0, 0, 0, 0};
  int skip[MIJPEG_MAX_COMPONENTS] = {0, 0, 0, 0};
  const uint32_t ri = (uint32_t)sc.restart_interval;
  uint32_t togo = ri;
  long next_rst = 0xffd0;
  bool valid = true;
  const int ss = sc.ss, se = sc.se;
  const bool residual = sc.residual; // m_bResidual: no DC part, the band starts at position 0, symbol 0x10 (sequentialscan.cpp:682, 709, 727-736)

  const bool log_spans = mode == DECODE && !discover && scan_base == nullptr;
  size_t span_from = s.pos;
  auto restart = [&]() { // (the caller has just taken the marker it recognised: two bytes that do not count)
    if (log_spans) { spans.emplace_back(span_from, s.pos - 2); span_from = s.pos; }
    for (int i = 0; i < sc.ncomp; i++) { pred[i] = 0; skip[i] = 0; }
    bits.open(&s);
    next_rst = (next_rst + 1) & 0xfff7;
    togo = ri;
    valid = true;
  };
  auto lose_segment = [&]() {
    valid = false;
    next_rst = (next_rst + 1) & 0xfff7;
    togo = ri;
  };
  auto parse_restart_marker = [&]() {
    long dt = s.peekword();
    while (dt == 0xffff) { s.get(); dt = s.peekword(); }
    if (dt == next_rst) { s.getword(); restart(); return; }
    warn(); // "entropy coder is out of sync, trying to advance to the next marker"
    for (;;) {
      dt = s.get();
      if (dt == ByteCursor::END) wthrow(MIJPEG_ERR_UNEXPECTED_EOF, "run into end of file while trying to resync the entropy parser");
      if (dt != 0xff) continue;
      s.lastundo();
      dt = s.peekword();
      if (dt >= 0xffd0 && dt < 0xffd8) {
        if (dt == next_rst) { s.getword(); restart(); return; } // the decoder was behind and is in step again
        if (((dt - next_rst) & 7) >= 4) s.getword();              // a marker it already passed: drop it, look on
        else { lose_segment(); return; }                          // the marker is ahead: this interval is lost, the marker stays
      } else if (dt >= 0xffc0 && dt < 0xfff0) {
        lose_segment(); // some other marker: the scan is over, the rest is lost
        return;
      } else {
        s.get(); // garbage, FF00, or a lone FF in front of the end
      }
    }
  };
  auto store_coef = [&](T *blk, int pos, int32_t v) {
    if (v != (T)v) {
      hd.left_16bit_store_ = true; // (what the callers that retry with 32-bit planes ask for: not the message's wording)
      wthrow(MIJPEG_ERR_OVERFLOW_PARAMETER, "coefficient exceeds the coefficient store of the accelerated path");
    }
    blk[pos] = (T)v;
  };
  auto decode_block = [&](T *blk, const HuffTable &dc, const HuffTable &ac, int32_t &prevdc, int &skp) {
    if (ss == 0 && !residual) {
      int32_t diff = 0;
      const int value = ref_symbol(bits, dc);
      if (value > 0) {
        if (value > 15) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "DC coefficient decoding out of sync");
        diff = (int32_t)bits.get(value);
        if (diff < (1 << (value - 1))) diff += (int32_t)((~0u) << value) + 1;
      }
      prevdc = (int32_t)((uint32_t)prevdc + (uint32_t)diff);
      store_coef(blk, 0, (int32_t)((uint32_t)prevdc << lowbit));
    }
    if (se) {
      if (skp > 0) { skp--; return; }
      int k = ss ? ss : (residual ? 0 : 1);
      do {
        const int rs = ref_symbol(bits, ac);
        const int r = rs >> 4, sz = rs & 15;
        if (sz == 0) {
          if (r == 15) { k += 16; continue; }
          if (r == 0 || progressive_run) {
            skp = 1 << r;
            if (r) skp |= (int)bits.get(r);
            skp = (skp - 1) & 0xffff;
            break;
          }
          if (residual && rs == 0x10) { // the value -0x8000 has no magnitude category: four bits of run follow
            k += (int)bits.get(4);
            if (k >= 64) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "AC coefficient decoding out of sync");
            store_coef(blk, zz[k], (int32_t)((uint32_t)(-0x8000) << lowbit));
            k++;
            continue;
          }
          wthrow(MIJPEG_ERR_MALFORMED_STREAM, "AC coefficient decoding out of sync");
        }
        k += r;
        int32_t diff = (int32_t)bits.get(sz);
        if (diff < (1 << (sz - 1))) diff += (int32_t)((~0u) << sz) + 1;
        if (k >= 64) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "AC coefficient decoding out of sync");
        store_coef(blk, zz[k], (int32_t)((uint32_t)diff << lowbit));
        k++;
      } while (k <= se);
    }
  };
  auto decode_block_refine = [&](T *blk, const HuffTable &ac, int &skp) {
    if (ss == 0 && !residual) store_coef(blk, 0, (int32_t)(blk[0] | (int32_t)(bits.get(1) << lowbit)));
    if (!se && !residual) return; // (refinementscan.cpp:594: `if (m_ucScanStop || m_bResidual)`)
    int k = ss, run = 0;
    int32_t sv = 0;
    bool at_start = false;
    if (skp > 0) { run = (se - ss + 1) & 0xff; skp--; }
    else { k--; at_start = true; }
    do {
      if (!at_start) {
        const int32_t dv = blk[zz[k]];
        if (dv) {
          if (bits.get(1)) store_coef(blk, zz[k], dv + (dv > 0 ? (1 << lowbit) : -(1 << lowbit)));
          continue;
        }
        if (run) { run--; continue; }
        store_coef(blk, zz[k], (int32_t)((uint32_t)sv << lowbit));
        if (k == se) break;
      }
      at_start = false;
      const int rs = ref_symbol(bits, ac), r = rs >> 4;
      sv = rs & 15;
      if (sv == 0) {
        if (r == 15) run = r;
        else {
          skp = 1 << r;
          if (r) skp |= (int)bits.get(r);
          skp = (skp - 1) & 0xffff;
          run = (se - k + 1) & 0xff;
        }
      } else if (sv != 1) {
        warn(); // refinementscan.cpp:667: "unexpected Huffman symbol in refinement coding": leave the block unrefined
        run = 0;
        sv = 0;
      } else {
        if (bits.get(1) == 0) sv = -sv;
        run = r;
      }
    } while (++k <= se);
  };

  // EntropyParser::ParseDNLMarker, codestream/entropyparser.cpp:204-249.  It looks at the BYTE stream, and that stands where the
  // bit reader's prefetch stopped -- up to four bytes ahead of the bits in use (io/bitstream.cpp:56-118): the marker is "found",
  // and every later MCU of the scan skipped, while the last MCUs' bits still wait in the window.
  bool dnl_found = false;
  auto parse_dnl_marker = [&]() -> bool {
    if (dnl_found) return true;
    long dt = s.peekword();
    while (dt == 0xffff) { s.get(); dt = s.peekword(); }
    if (dt != 0xffdc) return false;
    s.getword();
    dt = s.getword();
    if (dt != 4) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "DNL marker size is out of range, must be exactly four bytes long");
    dt = s.getword();
    if (dt == ByteCursor::END) wthrow(MIJPEG_ERR_UNEXPECTED_EOF, "stream is truncated, could not read the DNL marker");
    if (dt == 0) wthrow(MIJPEG_ERR_MALFORMED_STREAM, "frame height as indicated by the DNL marker is corrupt, must be > 0");
    if (hd.need_dnl_) { // Frame::PostImageHeight, marker/frame.cpp:1241-1258
      hd.info.height = (int32_t)dt;
      hd.dnl_height_ = (int)dt;
      const int grc = hd.frame_geometry();
      if (grc) wthrow(grc, "frame dimensions require an unreasonably large coefficient store");
      hd.need_dnl_ = false;
    } else if (dt != f.height)
      wthrow(MIJPEG_ERR_OPERATION_UNIMPLEMENTED, "DNL marker is not the one the first walk of the stream found");
    dnl_found = true;
    return true;
  };
  // BlockBuffer::StartMCUQuantizerRow (control/blockbuffer.cpp:212-265) while m_ulPixelHeight is 0: every MCU row gets all its
  // block rows and nothing bounds their number until the marker delivered the height; from then on rows end at ceil(ch / 8).
  // info.rows[] = what exists afterwards; later scans reach rows below ceil(ch / 8) through the list (`if (q) q = q->NextOf()`,
  // sequentialscan.cpp:423) iff the first scan created them.
  const bool dnl_scan = scan_for_dnl;
  int rows_made[MIJPEG_MAX_COMPONENTS] = {0, 0, 0, 0};
  for (int my = 0; dnl_scan || my < sc.mcus_y; my++) {
    if (dnl_scan) {
      bool more = true;
      for (int i = 0; i < sc.ncomp; i++) {
        const int c = sc.sc[i].comp;
        const int h = sc.ncomp > 1 ? f.vsamp[c] : 1;
        const int ch = (f.height + f.suby[c] - 1) / f.suby[c];
        int ymin = my * h * 8, ymax = ymin + h * 8;
        if (dnl_found) {
          ymin = std::min(ymin, ch); // m_pulY stopped at the clipped end of the previous row
          ymax = std::min(ymax, ch);
        }
        if (ymin < ymax) rows_made[c] = std::max(rows_made[c], my * h + ((ymax - ymin + 7) >> 3));
        else more = false;
      }
      if (!more) break;
      // (a scan that never comes to its DNL marker goes on until the reference runs out of memory)
      if (my > 65536 / 8 + 8) wthrow(MIJPEG_ERR_OPERATION_UNIMPLEMENTED, "frame height is zero and the first scan does not come to a DNL marker");
    }
    rows_entered = my + 1;
    for (int mx = 0; mx < sc.mcus_x; mx++) {
      bool mcu_valid;
      // EntropyParser::BeginReadMCU, entropyparser.hpp:147-160
      if (dnl_scan && parse_dnl_marker()) mcu_valid = false;
      else {
        if (ri) {
          if (togo == 0) {
            long dt = s.peekword();
            while (dt == 0xffff) { s.get(); dt = s.peekword(); }
            if (dt == 0xffdc && dnl_scan) parse_dnl_marker(); // entropyparser.cpp:127-128: no restart, the counter stays at 0
            else parse_restart_marker();
          }
          togo--;
        }
        mcu_valid = valid;
      }
      for (int i = 0; i < sc.ncomp; i++) {
        const int c = sc.sc[i].comp;
        const int w = sc.ncomp > 1 ? f.hsamp[c] : 1, h = sc.ncomp > 1 ? f.vsamp[c] : 1;
        T *plane = store + hd.plane_offset_[c];
        for (int by = 0; by < h; by++)
          for (int bx = 0; bx < w; bx++) {
            T dummy[64];
            const int X = mx * w + bx, Y = my * h + by;
            // (while the first scan of a DNL frame runs, every row it is at exists; later scans reach a row below ceil(ch / 8)
            // iff the first one made it)
            T *blk = (!discover && X < f.blocks_w[c] && Y < f.blocks_h[c] && (!f.dnl || dnl_scan || Y < f.rows[c])) ? plane + ((int64_t)Y * f.blocks_w[c] + X) * 64 : dummy;
            if (blk == dummy) memset(dummy, 0, sizeof(dummy));
            if (mcu_valid) {
              if (refinement) decode_block_refine(blk, sc.ac[i], skip[i]);
              else decode_block(blk, sc.dc[i], sc.ac[i], pred[i], skip[i]);
            } else if (!refinement) {
              for (int k = ss; k <= se; k++) blk[k] = 0; // sequentialscan.cpp:416-420: natural positions ss..se, not zigzag
            }
          }
      }
    }
  }
  if (log_spans) spans.emplace_back(span_from, s.pos);
  if (dnl_scan) {
    for (int i = 0; i < sc.ncomp; i++) {
      const int c = sc.sc[i].comp;
      hd.info.rows[c] = rows_made[c];
      if (discover) hd.dnl_rows_made_[c] = rows_made[c];
    }
    if (discover) { // the store keeps every row the scan made (frame_geometry)
      const int grc = hd.frame_geometry();
      if (grc) wthrow(grc, "frame dimensions require an unreasonably large coefficient store");
      for (int i = 0; i < sc.ncomp; i++) hd.info.rows[sc.sc[i].comp] = rows_made[sc.sc[i].comp];
    }
  }
}

void HostDecoder::reset_stream_state()
{
  scans.clear();
  term_base_ = nullptr; // (the same address may hold another file by now)
  // (walked_ / walked_scans_ are decode_sequential's: it clears them itself -- this function runs inside its walk as well)
  term_pos_.clear();
  box_bytes_promised_ = 0;
  for (auto &b : boxes_)
    if (b.data.capacity() >= (64u << 10) && box_spares_.size() < 64) box_spares_.push_back(std::move(b.data)); // (size and all: materialize_boxes)
  boxes_.clear();
  scan_interval_end_.clear();
  scan_rst_code_.clear();
  for (auto &t : dc_) t.defined = t.built = false;
  for (auto &t : ac_) t.defined = t.built = false;
  memset(quant_defined_, 0, sizeof(quant_defined_));
  memset(comp_seen_, 0, sizeof(comp_seen_));
  have_quant_ = have_huff_ = false;
  restart_interval_ = 0;
  adobe_transform_ = -1;
  have_frame_ = false;
  need_dnl_ = false;
  progressive_ = false;
  frame_type_ = 0;
  needs_sequential_ = false;
  warnings_ = 0;
}

// The tables the kernels read: component c uses info.quant[info.quant_index[c]].  Normally that is the stream's own
// assignment; when a table was redefined between the first scans of two components that share its index, or a
// component appears in no scan (it then reconstructs as sample value 0: a table of ones and a DC of -2^(P+2) in every
// block give exactly that, see fill_unseen_components), every component gets a table slot of its own.
void HostDecoder::publish_tables(bool header_only)
{
  if (header_only) { // only the first scan header was seen: the tables as they stand
    for (int c = 0; c < info.components; c++)
      if (quant_defined_[info.quant_index[c]]) memcpy(info.quant[info.quant_index[c]], quant_[info.quant_index[c]], sizeof(quant_[0]));
    return;
  }
  bool own_slots = false;
  for (int c = 0; c < info.components; c++) {
    if (!comp_seen_[c]) { own_slots = true; continue; }
    for (int e = 0; e < c; e++)
      if (comp_seen_[e] && info.quant_index[e] == info.quant_index[c] && memcmp(comp_quant_[e], comp_quant_[c], sizeof(comp_quant_[c])))
        own_slots = true;
  }
  for (int c = 0; c < info.components; c++) {
    if (own_slots) info.quant_index[c] = c;
    uint16_t *q = info.quant[info.quant_index[c]];
    if (comp_seen_[c]) memcpy(q, comp_quant_[c], sizeof(comp_quant_[c]));
    else
      for (int k = 0; k < 64; k++) q[k] = 1;
  }
}

int HostDecoder::parse(const uint8_t *data, size_t size, bool header_only)
{
  // a sink is good for this parse only: a parse that fails before it reaches the scan must not leave it to the next one
  active_sink_ = header_only ? nullptr : sink_;
  active_cap_ = sink_cap_;
  sink_ = nullptr;
  active_skip_ = !header_only && skip_search_;
  skip_search_ = false;
  scan_order();
  data_ = data;
  size_ = size;
  drop_residual();
  lonly_ = false;
  walked_ = false;
  walked_scans_.clear();
  memset(&xt, 0, sizeof(xt));
  error = StreamError();
  transformer_refused_ = false;
  late_quant_missing_ = nullptr;
  verdict_hidden_l_ = verdict_hidden_r_ = 0;
  memset(&info, 0, sizeof(info));
  reset_stream_state();
  dnl_height_ = 0;
  memset(dnl_rows_made_, 0, sizeof(dnl_rows_made_));
  spec_ltrafo_ = 255;
  hidden_src_.clear();
  residual_error_ = StreamError();
  parsed_ = false;
  hidden_ = 0;
  deferred_scans_.clear();
  RefWalker walker(*this, header_only ? RefWalker::HEADER : RefWalker::PLAN);
  eoi_frame_ = eoi_image_ = true; // (until a walk that got to the trailers says otherwise)
  static const bool trace = getenv("MIJPEG_READ_TIMES") != nullptr; // diagnostics
  using clk = std::chrono::steady_clock;
  const auto t_begin = clk::now();
  try {
    walker.run();
    // (the ALPHA image's residual codestream is read whichever way its own codestream ended: the outer image's trailer turns to it
    // when Image::ParseAlphaChannel has no more scans to give, codestream/image.cpp:1440-1462)
    if (!header_only) { eoi_frame_ = walker.frame_eoi; eoi_image_ = walker.image_eoi || alpha_child_; }
  } catch (const WalkError &e) {
    // Behind the first scan the planning walk is only as good as its assumption that the entropy coded segments are
    // well-formed: where the reference stands after a damaged scan depends on how the decode went.  An error from
    // there on is not reported here; the sequential walk of decode() finds what the reference finds.
    if (e.code != 0 && (header_only || scans.empty())) return fail(e.code, e.msg);
    needs_sequential_ = true; // (code 0: the walk stopped itself at a damaged scan)
  }
  materialize_boxes();
  run_deferred_searches(deferred_scans_);
  warnings_ = walker.warnings;
  if (!have_frame_) return fail(MIJPEG_ERR_MALFORMED_STREAM, "no frame header found");
  // a frame that announced a DNL marker and never met one keeps zero lines: the reference reads it without complaint and fails
  // at the first request for pixels (codestream/rectanglerequest.cpp:119-121; cmd/reconstruct.cpp:334-342 asks for MaxY = -1)
  if (info.height == 0) return fail(MIJPEG_ERR_OVERFLOW_PARAMETER, "Rectangle MaxY underflow, must be >= 0");
  info.ycbcr = (info.components == 3 && adobe_transform_ != 0) ? 1 : 0;
  publish_tables(header_only);
  parsed_ = !header_only;
  // an alpha channel's codestream: its boxes are the file's (the alpha kinds under their image counterparts' names, alpha_boxes)
  if (alpha_child_) boxes_ = preset_boxes_;
  const auto t_walked = clk::now();
  const int xrc = finish_xt(header_only);
  if (trace && !header_only)
    fprintf(stderr, "parse%s: %zu bytes, planning walk %.2f ms, boxes and their codestreams %.2f ms\n", nested_ ? " [residual]" : alpha_child_ ? " [alpha]" : "", size,
            std::chrono::duration<double>(t_walked - t_begin).count() * 1e3, std::chrono::duration<double>(clk::now() - t_walked).count() * 1e3);
  return xrc > 0 ? late_verdict() : xrc;
}


// ------------------------------------------------------------------------------------------------
// JPEG XT: the collected boxes' bytes, their hidden refinement scans and the file's checksum (what the boxes MEAN: xt_finish.cpp)
// ------------------------------------------------------------------------------------------------

// The codestream boxes the walk only took note of (XtBox::pieces): their bytes, copied by the pool -- sixteen megabytes in
// sixty-four kilobyte segments for a 4K file with hidden bit planes, a millisecond of one thread's memcpy on the walk's path before.
void HostDecoder::materialize_boxes()
{
  struct Job { uint8_t *dst; const uint8_t *src; size_t len, pad; };
  std::vector<Job> jobs;
  size_t bytes = 0;
  for (auto &b : boxes_) {
    if (!b.deferred) continue;
    b.data.resize(b.pending);
    size_t off = 0;
    for (const XtBox::Piece &pc : b.pieces) {
      jobs.push_back(Job{b.data.data() + off, pc.src, pc.len, pc.pad});
      off += pc.len + pc.pad;
      bytes += pc.len;
    }
    b.pieces.clear();
    b.pieces.shrink_to_fit();
    b.pending = 0;
    b.deferred = false; // (what arrives for it later -- nothing does: the walk is over -- would be appended the plain way)
  }
  if (jobs.empty()) return;
  const int workers = bytes < ((size_t)1 << 20) ? 1 : (int)std::min<size_t>(jobs.size(), (size_t)std::max(1, std::min(default_threads(), 16)));
  auto work = [&](int w) {
    for (size_t k = (size_t)w; k < jobs.size(); k += (size_t)workers) {
      memcpy(jobs[k].dst, jobs[k].src, jobs[k].len);
      if (jobs[k].pad) memset(jobs[k].dst + jobs[k].len, 0, jobs[k].pad);
    }
  };
  if (workers > 1) parallel_for(workers, work);
  else work(0);
}


// Hidden refinement scans of this frame: box number 0, 1, ... of `type` holds tables and exactly one scan
// (Frame::StartParseScan, marker/frame.cpp:805-818; Scan::StartParseHiddenRefinementScan, marker/scan.cpp:899-980).
// The visible scans move up by `hidden` bits (marker/scan.cpp:353-437).
int HostDecoder::add_hidden_scans(uint32_t type, const std::vector<XtBox> &boxes, int hidden)
{
  hidden_src_.clear(); // (decode_sequential walks them again: the boxes themselves stay put for the object's life time)
  for (auto &s : scans) {
    s.al += hidden;
    s.lowbit += hidden;
  }
  std::vector<DeferredSearch> searches;
  struct Undefer { // (whatever way this function is left)
    HostDecoder &h;
    ~Undefer() { h.deferred_hidden_ = nullptr; }
  } undefer{*this};
  deferred_hidden_ = &searches;
  for (int en = 0;; en++) {
    const XtBox *bx = nullptr;
    for (const auto &b : boxes)
      if (b.type == type && b.en == en && b.complete) bx = &b; // Tables::RefinementDataOf, codestream/tables.cpp:872-891
    if (!bx) break;
    hidden_src_.push_back(bx);
    // A frame whose visible scans are damaged, or whose trailer never stands at an EOI, is walked the reference's way by
    // decode(): the walk takes the hidden scans from hidden_src_ if and when the reference gets to them; nothing to plan
    if (needs_sequential_ || !eoi_frame_) continue;
    // the box payload is a little codestream of its own (tables, then one scan): offsets of its scan refer to it
    const size_t before = scans.size();
    RefWalker walker(*this, RefWalker::PLAN);
    // A box without a scan header is skipped with a warning and the frame turns to the next one (marker/frame.cpp:805-822,
    // 857-860); what is wrong inside a box is reported when the reference gets there, behind the visible scans: both are the
    // sequential walk's business (decode_sequential runs the boxes of hidden_src_ again)
    try {
      walker.run_hidden(bx->data.data(), bx->data.size());
    } catch (const WalkError &) {
      needs_sequential_ = true;
      continue;
    }
    if (scans.size() == before) needs_sequential_ = true;
  }
  deferred_hidden_ = nullptr;
  run_deferred_searches(searches);
  // A component that no visible scan names appears in a hidden one first (a residual codestream whose scan header is damaged,
  // with its RFIN boxes intact: xt_gpu_damage_campaign, seed 72): its transform is built THERE, with the table in force there
  // (RefWalker::scan took it) -- parse() published the stand-in of an unseen component before this function ran.
  publish_tables(false);
  return 0;
}

// The checksum of a JPEG XT file (LCHK box): tools/checksum.hpp:104-126 is a Fletcher sum modulo 255 over the bytes the scans of
// the LEGACY codestream read through their ChecksumAdapter -- the entropy coded data as stored (stuffed bytes included),
// without the restart markers, without headers and tables (Tables::ChecksumTables() is false) and without the hidden
// refinement scans, which live in boxes.  With c1 = sum b_j and c2 = sum (N - j) b_j (mod 255) it is computed range by range.
int HostDecoder::last_warning(const char **msg)
{
  if (msg) *msg = nullptr;
  if (have_lchk_ && checksum_state_ < 0) {
    uint64_t c1 = 0, c2 = 0;
    // the byte ranges the legacy scans read: from the plan of a well-formed stream, or -- a damaged one, walked the reference's
    // way -- as the walk logged them
    std::vector<std::pair<size_t, size_t>> ranges;
    if (needs_sequential_) ranges = seq_spans_;
    else
      for (size_t si = 0; si < scans.size(); si++) {
        const Scan &s = scans[si];
        if (s.base) continue; // a hidden scan out of a FINE box
        const std::vector<size_t> &iend = scan_interval_end_[si];
        for (size_t k = 0; k < s.interval_begin.size() && k < iend.size(); k++) ranges.emplace_back(s.interval_begin[k], iend[k]);
      }
    {
      for (const auto &rg : ranges) {
        size_t a = rg.first;
        const size_t b = std::min(rg.second, size_);
        while (a < b) { // blocks short enough for 64-bit partial sums
          const size_t n = std::min<size_t>(b - a, (size_t)1 << 20);
          uint64_t sum = 0, wsum = 0;
          for (size_t j = 0; j < n; j++) {
            sum += data_[a + j];
            wsum += (uint64_t)(n - j) * data_[a + j];
          }
          c2 = (c2 + (uint64_t)(n % 255) * c1 + wsum) % 255;
          c1 = (c1 + sum) % 255;
          a += n;
        }
      }
    }
    checksum_state_ = (((uint32_t)c1 | ((uint32_t)c2 << 8)) == lchk_value_) ? 0 : 1; // the box value is compared as 32 bits (interface/jpeg.cpp:231): upper bits that are not zero always warn
  }
  if (checksum_state_ == 1) {
    if (msg) *msg = "Found a mismatching checksum of the legacy stream, HDR reconstructed image may be wrong";
    return MIJPEG_ERR_PHASE_ERROR;
  }
  if (warnings_ > 0) {
    if (msg) *msg = "the codestream is damaged: the decoder skipped or resynchronised over parts of it like the reference does";
    return MIJPEG_ERR_MALFORMED_STREAM;
  }
  return 0;
}

} // namespace mij
