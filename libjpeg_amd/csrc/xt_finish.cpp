// xt_finish.cpp -- JPEG XT: interpret the collected boxes (codestream/tables.cpp:1172-1277, boxes/mergingspecbox.cpp,
// colortrafo/colortransformerfactory.cpp:206-594) and set up the decoder of the residual codestream
// (codestream/image.cpp:1264-1300).  Only the profile C subset named in include/mijpeg.h is accepted.  HostDecoder::finish_xt
// as named stages; what is a function of bytes alone lives in xt_spec.hpp.
#include "host_decoder.hpp"
#include "xt_spec.hpp"

#include <stdio.h>
#include <stdlib.h>

#include <chrono>

namespace mij {

// A merging specification box in a file that has no residual codestream: what the reference's encoder writes for `-c`
// (SPEC{OCON, LTRF = identity}, codestream/tables.cpp:625-632) and for grey scale pictures.  Tables::LTrafoTypeOf
// (codestream/tables.cpp:1994-2021) takes the L transformation from the box BEFORE it looks at the Adobe marker or the number
// of components; the colour transformer is the Extended flavour without anything to merge
// (colortransformerfactory.cpp:232-236, 275-279): identity L tables and C transformation, clamp to 2^P - 1
// (colortrafo/ycbcrtrafo.cpp:861-878, 921-936) -- the plain picture with the box's transformation.  Accepted: LTRF undefined /
// identity / YCbCr (three components), an output conversion that clamps and changes nothing else: 0, the plain picture on the
// plain kernels.  Tables, hidden bits, free-form matrices, more output bits, float output: 1 -- finish_xt builds the whole L chain
// (ColorTransformerFactory::BuildColorTransformer with R transformation "zero", colortransformerfactory.cpp:262-283).
int HostDecoder::spec_without_residual(const XtBox &spec)
{
  int ltrafo = 255, ctrafo = 255, ocon = -1;
  bool beyond = false, have_mtx[16] = {false};
  SubBoxWalk w(spec.data.data(), spec.data.size());
  while (w.next()) {
    if (!w.len) continue; // (a box without payload: nothing to read; the form check has thrown it out where it matters)
    const uint8_t *pl = w.payload;
    const uint32_t t = w.type;
    if (t == boxid('L', 'T', 'R', 'F')) ltrafo = pl[0] >> 4;
    else if (t == boxid('C', 'T', 'R', 'F')) ctrafo = pl[0] >> 4;
    else if (t == boxid('O', 'C', 'O', 'N')) ocon = pl[0];
    else if (t == boxid('R', 'S', 'P', 'C')) beyond = beyond || pl[0] != 0;
    else if (t == boxid('L', 'D', 'C', 'T')) beyond = beyond || pl[0] != 0;
    else if (t == boxid('R', 'T', 'R', 'F') || t == boxid('R', 'D', 'C', 'T')) {} // about a residual that is not there
    else if (t == boxid('M', 'T', 'R', 'X')) have_mtx[pl[0] >> 4] = true; // (a matrix or a curve nobody names changes nothing)
    else if (t == boxid('F', 'T', 'R', 'X') || (t & 0xffffffu) == (boxid(0, 'P', 'T', 'S')) || t == boxid('D', 'T', 'R', 'F') || t == boxid('S', 'T', 'R', 'F'))
      beyond = true; // point transformations, float matrices, transformations of the other profiles
    // (a type MergingSpecBox::CreateBox does not know is skipped, boxes/superbox.cpp:161-176)
  }
  if (w.broken) return fail(MIJPEG_ERR_OPERATION_UNIMPLEMENTED, "malformed box inside a merging specification box without a residual codestream");
  for (const auto &b : boxes_)
    if (b.type == boxid('M', 'T', 'R', 'X') && b.complete && !b.data.empty()) have_mtx[b.data[0] >> 4] = true;
  if (info.components == 1 && ltrafo != 255)
    return fail(MIJPEG_ERR_MALFORMED_STREAM, "Base transformation box exists even though the number of components is one");
  if (ltrafo == 0 || ltrafo == 3 || ltrafo == 4)
    return fail(MIJPEG_ERR_MALFORMED_STREAM, "Found an invalid base transformation, must be YCbCr, identity or free-form");
  if (ltrafo != 255 && ltrafo >= 5 && !have_mtx[ltrafo]) // colortransformerfactory.cpp:379-383
    return fail(MIJPEG_ERR_OBJECT_DOESNT_EXIST, "the base transformation specified in the codestream does not exist");
  if (beyond || (ctrafo != 255 && ctrafo != 1) || (ltrafo != 255 && ltrafo >= 5) || (ltrafo == 2 && info.components != 3) ||
      // (the lossless flag changes the residual's side only, the output lookup indices are never used by the decoder: finish_xt)
      (ocon >= 0 && ((ocon >> 4) != 0 || (ocon & 0x04) || !(ocon & 0x02))))
    return 1; // more than the plain picture: the L chain of finish_xt
  spec_ltrafo_ = ltrafo;
  if (ltrafo == 2) info.ycbcr = 1;
  else if (ltrafo == 1) info.ycbcr = 0;
  return 0;
}

// The alpha channel of a JPEG XT file is an image of its own in the ALFA box (Image::ParseAlphaChannel, codestream/image.cpp:
// 1337-1404): SOI, tables, a one-component frame, scans -- with the alpha merging specification ASPC in the role of SPEC
// (Tables::ResidualSpecsOf, codestream/tables.hpp:451-460), ARES / AFIN / ARRF in the roles of RESI / FINE / RFIN
// (boxes/databox.hpp:90-96, codestream/tables.cpp:752-775, 850-903) and the file's TONE / CURV / MTRX boxes behind the
// specification's own (Tables::AlphaNamespace, codestream/tables.cpp:109, 2115-2125).  A second decoder object decodes it
// (capi.cpp: mijpeg_alpha_channel) from these boxes instead of what its own walk collects.
bool HostDecoder::alpha_stream(const uint8_t **data, size_t *size) const
{
  for (const auto &b : boxes_)
    if (b.complete && b.type == boxid('A', 'L', 'F', 'A')) {
      *data = b.data.data();
      *size = b.data.size();
      return true;
    }
  return false;
}

std::vector<XtBox> HostDecoder::alpha_boxes() const
{
  std::vector<XtBox> out;
  for (const auto &b : boxes_) {
    if (!b.complete) continue;
    uint32_t t = b.type;
    if (t == boxid('A', 'S', 'P', 'C')) t = boxid('S', 'P', 'E', 'C');
    else if (t == boxid('A', 'R', 'E', 'S')) t = boxid('R', 'E', 'S', 'I');
    else if (t == boxid('A', 'F', 'I', 'N')) t = boxid('F', 'I', 'N', 'E');
    else if (t == boxid('A', 'R', 'R', 'F')) t = boxid('R', 'F', 'I', 'N');
    else if (t != boxid('T', 'O', 'N', 'E') && t != boxid('C', 'U', 'R', 'V') && t != boxid('M', 'T', 'R', 'X')) continue;
    out.push_back(b);
    out.back().type = t;
  }
  return out;
}

// One call of finish_xt: what its stages hand on.  A stage that ends the call says `return stop(code)` (or fail / late / late_r,
// which do) and finish_xt returns `rc`; a stage that returns false leaves the call to the next one.
struct HostDecoder::XtFinish {
  HostDecoder &h;
  const bool header_only;
  const XtBox *spec = nullptr, *resi = nullptr;
  bool lonly = false; // a specification and no residual codestream: the legacy picture through the whole L chain
  int nc = 0, rc = 0;
  XtSpec s;
  XtTables tables;
  std::chrono::steady_clock::time_point t_xt0, t_xt1, t_xt2; // (MIJPEG_READ_TIMES)

  XtFinish(HostDecoder &decoder, bool headers) : h(decoder), header_only(headers) {}
  bool stop(int code) { rc = code; return true; }
  bool fail(int code, const char *msg) { return stop(h.fail(code, msg)); }
  // what the reference's colour transformer finds when the first request builds it (Tables::ColorTrafoOf, codestream/tables.cpp:
  // 1517-1555; colortrafo/colortransformerfactory.cpp:206-594): reported behind what stops either codestream (late_verdict)
  bool late(int code, const char *msg)
  {
    if (header_only) return fail(code, msg); // (nothing will be decoded: say it now)
    h.late_error_.code = code;
    h.late_error_.message = msg;
    return stop(1);
  }
  bool late_r(int code, const char *msg) // ... about the residual's side (Q, R2)
  {
    h.late_residual_only_ = true;
    return late(code, msg);
  }
  int legacy_hidden_scans(int hidden) { return h.add_hidden_scans(boxid('F', 'I', 'N', 'E'), h.boxes_, hidden); }

  void reset_state()
  {
    h.late_error_ = StreamError();
    h.late_residual_only_ = false;
    h.have_lchk_ = false;
    h.checksum_state_ = -1;
    h.residual_unspecified_ = false;
    h.have_alpha_ = false;
    h.alpha_mode_ = -1;
    h.alpha_matte_[0] = h.alpha_matte_[1] = h.alpha_matte_[2] = 0;
  }

  bool survey_boxes()
  {
    for (const auto &b : h.boxes_) {
      if (!b.complete) continue; // a box that never filled up stays in the reference's list unparsed: nobody looks at it
      if (b.type == boxid('L', 'C', 'H', 'K') && b.data.size() >= 4) { // boxes/checksumbox.cpp: 32 bits, the low 16 are used
        h.have_lchk_ = true;
        h.lchk_value_ = rd32(&b.data[0]);
      }
      if (b.type == boxid('S', 'P', 'E', 'C')) spec = &b;
      else if (b.type == boxid('R', 'E', 'S', 'I')) resi = &b;
      else if (b.type == boxid('A', 'L', 'F', 'A') && !h.nested_ && !h.alpha_child_) h.have_alpha_ = true;
      else if (b.type == boxid('A', 'S', 'P', 'C') && !h.nested_ && !h.alpha_child_) {
        // the compositing box inside the alpha merging specification (boxes/alphabox.cpp:60-90): what GetInformation reports
        SubBoxWalk w(b.data.data(), b.data.size());
        while (w.next()) // (a framing break ends the search and nothing else)
          if (w.type == boxid('A', 'M', 'U', 'L') && w.len == 10) {
            h.alpha_mode_ = w.payload[0] >> 4;
            for (int k = 0; k < 3; k++) h.alpha_matte_[k] = rd16(w.payload + 2 + 2 * k);
          }
      } else if (b.type == boxid('F', 'T', 'O', 'N') || b.type == boxid('F', 'T', 'R', 'X'))
        return fail(MIJPEG_ERR_OPERATION_UNIMPLEMENTED, "floating point tables and transformations (profiles A and B) are not on the accelerated path");
    }
    if (h.ignore_residual_ && spec) resi = nullptr; // (late_verdict: the legacy codestream has no EOI, the residual one is never looked at)
    return false;
  }

  // Parses the residual codestream with `r` and gives the verdict on its headers (h.residual_error_); true: they are refused.
  // Image::ParseResidualStream (codestream/image.cpp:1289-1299) compares right behind the residual FRAME HEADER: a residual
  // codestream that brings its height in a DNL marker (the reference's own encoder writes that for -n) still says 0 there.
  // The reference gets to the residual codestream behind the legacy codestream's EOI (codestream/image.cpp:1416-1431): what is
  // wrong with it is reported when the legacy frame has been decoded -- whatever stops that one comes first (decode_t).
  bool residual_header(HostDecoder &r, bool headers_alone)
  {
    r.nested_ = true;
    t_xt0 = std::chrono::steady_clock::now();
    const int prc = r.parse(resi->data.data(), resi->data.size(), headers_alone);
    t_xt1 = std::chrono::steady_clock::now();
    StreamError &e = h.residual_error_;
    e = StreamError();
    if (prc) { e.code = prc; e.message = r.error.message; }
    else if (r.info.width != h.info.width || r.info.height != h.info.height || r.info.dnl) {
      e.code = MIJPEG_ERR_MALFORMED_STREAM;
      e.message = "Malformed stream - residual image dimensions do not match the dimensions of the legacy image";
    } else if (r.info.components != h.info.components) {
      e.code = MIJPEG_ERR_MALFORMED_STREAM;
      e.message = "Malformed stream - number of components differ between residual and legacy image";
    }
    return e.code != 0;
  }

  bool residual_without_spec()
  {
    if (spec || !resi) return false;
    // A residual codestream and no merging specification (its APP11 segment damaged, its box never complete).  The reference's
    // command line reads the whole file (cmd/reconstruct.cpp:119-121) and builds the colour transformer at the first request:
    // no specification -> R transformation "zero" (codestream/tables.cpp:2070-2071), for which, with a residual frame, no
    // transformer exists (colortransformerfactory.cpp:277-291).  What is wrong with either codestream comes first (decode_t);
    // without an EOI behind the legacy codestream the residual frame never comes to be and the file is a plain JPEG.
    HostDecoder r;
    h.residual_unspecified_ = true;
    if (!residual_header(r, true)) {
      h.residual_error_.code = MIJPEG_ERR_INVALID_PARAMETER;
      h.residual_error_.message = "The combination of L and R transformation is non-standard and not supported";
    }
    if (header_only) return fail(h.residual_error_.code, h.residual_error_.message.c_str()); // (nothing will be decoded: say it now)
    return stop(legacy_hidden_scans(0));
  }

  bool without_residual()
  {
    // Refinement boxes are read behind the frame's last visible scan whoever else is there (marker/frame.cpp:1063-1070): without a
    // specification that names hidden bits the scans in them refine the bits the visible scans left as they are
    if (!spec) return stop(header_only ? 0 : legacy_hidden_scans(0)); // plain JPEG (ftyp / LCHK boxes alone change nothing)
    // A merging specification and no residual codestream: the plain picture where the specification only names the L
    // transformation (`jpeg -c`, grey scale files), else the legacy picture through the whole L chain -- what the reference's encoder
    // writes for `-R n` without `-r` from a picture of more than eight bits: hidden refinement scans, an L table from 8 + n bits to
    // the output's depth, an output conversion.  The transformer is the Extended flavour with R transformation "zero"
    // (colortransformerfactory.cpp:262-283): L transformation, L tables, C transformation, clamp or cast to half float, nothing
    // merged (rr = m_lOutDCShift, colortrafo/ycbcrtrafo.cpp:744-746, 861-878); InstallIntegerParameters (:300-594) looks at the
    // L tables and the L and C transformations only.
    if (!resi) {
      const int src = h.spec_without_residual(*spec);
      if (src != 1) return stop(src || header_only ? src : legacy_hidden_scans(0));
      lonly = true;
      if (h.info.precision != 8)
        return fail(MIJPEG_ERR_OPERATION_UNIMPLEMENTED, "a merging specification with tables on a frame of more than 8 bits is not on the accelerated path");
    }
    if (h.info.precision != 8)
      return late(MIJPEG_ERR_MALFORMED_STREAM, "Residual or refinement coding requires a coding precision of 8 bits per sample");
    // three components, or one: a grey scale picture with a residual (`jpeg -r .. in.pgm`) -- every transformation is the identity then
    if (h.info.components != 3 && h.info.components != 1)
      return fail(MIJPEG_ERR_OPERATION_UNIMPLEMENTED, "JPEG XT with two or four components is not on the accelerated path");
    nc = h.info.components;
    return false;
  }

  // The specification's own boxes, in their order: a failure -- of a value, of a table registered from inside the box, of the
  // framing -- is the first one the walk comes to.
  bool read_spec()
  {
    auto indices = [](const uint8_t *pl, int (&idx)[4]) { idx[0] = pl[0] >> 4; idx[1] = pl[0] & 15; idx[2] = pl[1] >> 4; idx[3] = pl[1] & 15; };
    SubBoxWalk w(spec->data.data(), spec->data.size()); // superbox: LBox(4) TBox(4) payload
    while (w.next()) {
      if (!w.len) continue; // (a box without payload: nothing to read; the form check has thrown it out where it matters)
      const uint8_t *pl = w.payload;
      const uint32_t t = w.type;
      if (t == boxid('L', 'T', 'R', 'F')) s.ltrafo = pl[0] >> 4;
      else if (t == boxid('R', 'T', 'R', 'F')) s.rtrafo = pl[0] >> 4;
      else if (t == boxid('C', 'T', 'R', 'F')) s.ctrafo = pl[0] >> 4;
      else if (t == boxid('L', 'P', 'T', 'S') && w.len >= 2) indices(pl, s.lidx);
      else if (t == boxid('Q', 'P', 'T', 'S') && w.len >= 2) indices(pl, s.qidx);
      else if (t == boxid('R', 'P', 'T', 'S') && w.len >= 2) indices(pl, s.r2idx);
      else if (t == boxid('O', 'C', 'O', 'N')) s.ocon = pl[0];
      else if (t == boxid('R', 'S', 'P', 'C')) { // boxes/refinementspecbox.cpp:57-83
        s.hidden_l = pl[0] >> 4;
        s.hidden_r = pl[0] & 15;
        h.verdict_hidden_l_ = s.hidden_l; // (late_verdict: the codestreams' verdict includes their hidden refinement scans)
        h.verdict_hidden_r_ = s.hidden_r;
        if (s.hidden_l > 4) return fail(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG stream - the number of refinement scans must be smaller or equal than four");
        if (s.hidden_r > 4) return fail(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG stream - the number of residual refinement scans must be smaller or equal than four");
      } else if (t == boxid('L', 'D', 'C', 'T')) {
        if ((pl[0] >> 4) != 0 || (pl[0] & 15)) return fail(MIJPEG_ERR_OPERATION_UNIMPLEMENTED, "only the fixpoint DCT is on the accelerated path for the base layer");
      } else if (t == boxid('R', 'D', 'C', 'T')) { // boxes/dctbox.cpp:60-92: 0 fixpoint DCT, 2 integer DCT (lossless coding), 3 bypass
        const int rdct = s.rdct = pl[0];
        if ((rdct >> 4) == 2) return fail(MIJPEG_ERR_OPERATION_UNIMPLEMENTED, "only the fixpoint DCT is on the accelerated path");
        if ((rdct >> 4) != 0 && (rdct >> 4) != 3) return fail(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG stream - invalid DCT specified");
        if ((rdct & 15) > 1) return fail(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG stream - invalid noise shaping specified");
        if ((rdct & 15) && (rdct >> 4) != 3) return fail(MIJPEG_ERR_MALFORMED_STREAM, "Malformed JPEG stream - cannot enable noise shaping without bypassing the DCT");
      } else if (t == boxid('T', 'O', 'N', 'E') || t == boxid('C', 'U', 'R', 'V') || t == boxid('M', 'T', 'R', 'X')) {
        if (const XtVerdict v = tables.register_box(t, pl, w.len); v.code) return fail(v.code, v.message);
      } else if (t == boxid('C', 'P', 'T', 'S') || t == boxid('D', 'P', 'T', 'S') || t == boxid('S', 'P', 'T', 'S') || t == boxid('P', 'P', 'T', 'S') ||
                 t == boxid('D', 'T', 'R', 'F') || t == boxid('S', 'T', 'R', 'F') || t == boxid('F', 'T', 'R', 'X'))
        return fail(MIJPEG_ERR_OPERATION_UNIMPLEMENTED, "merging specification uses tables or transformations outside profile C (secondary base, intermediate residual, pre/post scaling)");
      // (any other type: MergingSpecBox::CreateBox knows no such box and the superbox skips it, boxes/superbox.cpp:161-176)
    }
    return w.broken && fail(MIJPEG_ERR_MALFORMED_STREAM, "malformed box inside the merging specification box");
  }

  bool register_file_boxes()
  {
    for (const auto &b : h.boxes_)
      if (b.complete)
        if (const XtVerdict v = tables.register_box(b.type, b.data.data(), b.data.size()); v.code) return fail(v.code, v.message);
    // A TONE box that never completes stays in the reference's list as an object that was constructed and never parsed: no entries,
    // and a table index nobody initialised (boxes/tonemapperbox.hpp:64-76) -- in practice the zero of fresh heap memory.  A
    // specification that names table 0 finds it (namespace.cpp:60-91) and its ScaledTableOf refuses: "does not fit to the input bit
    // precision", -1024 (inversetonemappingbox.cpp:192-212) -- not "does not exist".  Restated as the table with no entries.
    XtNlt &t0 = tables.nlt[0];
    if (!t0.kind)
      for (const auto &b : h.boxes_)
        if (!b.complete && b.type == boxid('T', 'O', 'N', 'E')) { t0.kind = 1; t0.entries = 0; t0.resbits = 0; t0.lut.clear(); }
    return false;
  }

  bool apply_defaults()
  {
    if (nc == 1) {
      // codestream/tables.cpp:2003-2005, 2079-2081: these two boxes must not exist with one component; the residual transformation
      // defaults to the identity (:2055-2060), and only that has a transformer (colortransformerfactory.cpp:681-757)
      if (s.ltrafo != 255) return late(MIJPEG_ERR_MALFORMED_STREAM, "Base transformation box exists even though the number of components is one");
      if (s.ctrafo != 255) return late(MIJPEG_ERR_MALFORMED_STREAM, "Color transformation box exists even though the number of components is one");
      if (!lonly && s.rtrafo != 255 && s.rtrafo != 1) return fail(MIJPEG_ERR_OPERATION_UNIMPLEMENTED, "a residual transformation on one component is not on the accelerated path");
      s.ltrafo = 1;
      if (!lonly) s.rtrafo = 1;
    }
    // codestream/tables.cpp:1994-2031: undefined -> the rule of plain JPEG: three components and no Adobe marker that says "none"
    if (s.ltrafo == 255) s.ltrafo = (nc == 3 && h.adobe_transform_ != 0) ? 2 : 1;
    // Tables::RTrafoTypeOf (codestream/tables.cpp:2040-2075) is asked with or without a residual: zero and JPEG_LS are invalid;
    // any other value is never used without one
    if (lonly && (s.rtrafo == 0 || s.rtrafo == 3)) return late(MIJPEG_ERR_MALFORMED_STREAM, "Found an invalid residual transformation");
    if (s.rtrafo == 255 || lonly) s.rtrafo = 2;
    return false;
  }

  bool verdicts()
  {
    const int ltrafo = s.ltrafo, rtrafo = s.rtrafo, ctrafo = s.ctrafo;
    int &ocon = s.ocon;
    // colortransformerfactory.cpp:355-400, 528-566: which values the L / C / R transformations may take
    if (ltrafo == 0 || ltrafo == 3 || ltrafo == 4) return late(MIJPEG_ERR_MALFORMED_STREAM, "the base transformation specified in the codestream is invalid");
    if (rtrafo == 3) return late_r(MIJPEG_ERR_MALFORMED_STREAM, "the residual transformation specified in the codestream is invalid");
    if (rtrafo == 0) return fail(MIJPEG_ERR_OPERATION_UNIMPLEMENTED, "an R transformation \"zero\" beside a residual codestream is not on the accelerated path");
    if (rtrafo == 4 && nc != 3) return fail(MIJPEG_ERR_OPERATION_UNIMPLEMENTED, "the RCT on one component is not on the accelerated path");
    if (ctrafo != 255 && ctrafo != 1 && ctrafo < 5) return late(MIJPEG_ERR_MALFORMED_STREAM, "the color transformation specified in the codestream is invalid");
    // output conversion (boxes/outputconversionbox.cpp:91-127): 8 + extra range bits of output, clamped, no lookup, not lossless;
    // the cast to half float wants the full 16 bits.  Integer JPEG XT of an 8-bit picture (`jpeg -r -q .. -Q ..` on a PPM) has 8.
    if (ocon < 0 && lonly) ocon = 0x02; // no output conversion box: no extra bits, clipping (boxes/mergingspecbox.cpp:323-331, 648-656)
    // the lossless flag only changes the residual's side (codestream/tables.cpp:1643, 1687; marker/frame.cpp:595), the output
    // lookup indices are read and never used by the decoder: without a residual neither matters
    if (lonly) ocon &= ~0x09;
    // (... the lookup flag with a residual as well: MergingSpecBox::OutputConversionLookupOf has no caller; the reference's encoder
    // sets it for alpha channels that have a residual)
    if (ocon >= 0) ocon &= ~0x01;
    s.outbits = ocon < 0 ? 0 : 8 + (ocon >> 4);
    // without a residual only the clamping flavours of the transformer exist (colortransformerfactory.cpp:698-725, 850-885)
    if (lonly && !(ocon & 0x09) && !(ocon & 0x02))
      return late(MIJPEG_ERR_INVALID_PARAMETER, "The combination of L and R transformation is non-standard and not supported");
    if (ocon < 0 || s.outbits > 16 || ((ocon & 0x04) && s.outbits != 16))
      return fail(MIJPEG_ERR_OPERATION_UNIMPLEMENTED, "output conversion outside the subset of the accelerated path (half float output at 16 bits)");
    s.clamping = (ocon & 0x02) != 0;
    s.lossless = (ocon & 0x08) != 0;
    // Which transformers exist beside a residual (colortransformerfactory.cpp:681-757, 793-995): R = YCbCr / free-form has the
    // clamping flavours only, R = RCT the ones without, R = identity all four
    if (!lonly && ((rtrafo == 4 && s.clamping) || (rtrafo != 4 && rtrafo != 1 && !s.clamping)))
      return late(MIJPEG_ERR_INVALID_PARAMETER, "The combination of L and R transformation is non-standard and not supported");
    // ... and only a transformer that exists gets its parameters (InstallIntegerParameters, colortransformerfactory.cpp:283-286)
    const bool(&have_mtx)[16] = tables.have_mtx;
    if (ltrafo >= 5 && !have_mtx[ltrafo]) return late(MIJPEG_ERR_OBJECT_DOESNT_EXIST, "the base transformation specified in the codestream does not exist");
    if (ctrafo != 255 && ctrafo >= 5 && !have_mtx[ctrafo]) return late(MIJPEG_ERR_OBJECT_DOESNT_EXIST, "the color transformation specified in the codestream does not exist");
    if (rtrafo >= 5 && !have_mtx[rtrafo]) return late_r(MIJPEG_ERR_OBJECT_DOESNT_EXIST, "the residual transformation specified in the codestream does not exist");
    // fractional bits of the residual path (Tables::FractionalColorBitsOf, codestream/tables.cpp:1621-1660): the RCT has one (a
    // precision bit really), the identity none when the lossless flag is set, everything else four
    s.rbits = rtrafo == 4 ? 1 : (rtrafo == 1 && s.lossless) ? 0 : 4;
    if (!lonly && s.rbits == 0 && s.clamping)
      return fail(MIJPEG_ERR_OPERATION_UNIMPLEMENTED, "a lossless identity R transformation with clamping is not on the accelerated path");
    if (!lonly && s.rbits != 4 && (s.rdct >> 4) != 3)
      return fail(MIJPEG_ERR_OPERATION_UNIMPLEMENTED, "only the fixpoint DCT is on the accelerated path (a residual DCT with one or no fractional bit: lossless coding)");
    return false;
  }

  void fill_params()
  {
    static const int32_t std_ycc[9] = {8192, 0, 11485, 8192, -2819, -5850, 8192, 14516, 0}; // colortransformerfactory.cpp:136-138, TO_FIX at 13 bits
    static const int32_t std_id[9] = {8192, 0, 0, 0, 8192, 0, 0, 0, 8192};
    const int ltrafo = s.ltrafo, rtrafo = s.rtrafo, ctrafo = s.ctrafo;
    mijpeg_xt_params &xt = h.xt;
    // free-form matrices run through the YCbCr branches of the transformer
    xt.ltrafo_ycbcr = ltrafo != 1;
    xt.ltrafo_standard = ltrafo == 2; // MergingSpecBox::YCbCr: what a request without colour transformation turns into the identity
    xt.rtrafo_ycbcr = rtrafo != 1 && rtrafo != 4;
    xt.rct = rtrafo == 4 ? 1 : 0;
    xt.rbits = s.rbits;
    memcpy(xt.lmat, ltrafo >= 5 ? tables.mtx[ltrafo] : ltrafo == 2 ? std_ycc : std_id, sizeof(xt.lmat));
    memcpy(xt.rmat, rtrafo >= 5 ? tables.mtx[rtrafo] : (rtrafo == 2 || rtrafo == 4) ? std_ycc : std_id, sizeof(xt.rmat));
    memcpy(xt.cmat, (ctrafo != 255 && ctrafo >= 5) ? tables.mtx[ctrafo] : std_id, sizeof(xt.cmat));
    xt.rdct_bypass = (s.rdct >> 4) == 3;
    xt.noise_shaping = s.rdct & 1;
    xt.out_max = (1 << s.outbits) - 1;
    xt.out_shift = (xt.out_max + 1) >> 1;
    xt.is_float = (s.ocon & 0x04) ? 1 : 0;
    xt.clamp = s.clamping ? 1 : 0;
    xt.hidden_bits = s.hidden_l;
    xt.residual_hidden_bits = s.hidden_r;
  }

  bool build_l_tables()
  {
    // the L tables are indexed with the legacy samples at 8 + hidden bits (codestream/tables.cpp:549, 1531-1534)
    const int entries = 256 << s.hidden_l;
    h.xt.ltable_entries = entries;
    XtNlt id1; // the default: the identity with e = 1 (e = 0 for Q and R2), colortransformerfactory.cpp:95-108
    id1.kind = 2; id1.type = 2; id1.e = 1;
    for (int c = 0; c < nc; c++) {
      const XtNlt &t = s.lidx[c] == 255 ? id1 : tables.nlt[s.lidx[c]];
      if (!t.kind) return late(MIJPEG_ERR_OBJECT_DOESNT_EXIST, "the L lookup table specified in the codestream does not exist");
      std::vector<int32_t> tab;
      if (const int trc = scaled_table(t, 8 + s.hidden_l, s.outbits, 0, 0, tab))
        return late(trc, "Codestream is requesting a tone mapping that does not fit to the output bit precision.");
      memcpy(h.xt.ltable[c], tab.data(), (size_t)entries * sizeof(int32_t));
    }
    return false;
  }

  // nothing to merge: no residual frame, no Q / R2 tables (looked up beside a residual frame only, :452, :496).  xt.residual
  // describes a frame without components (sampling factors 1, so that nobody divides by zero)
  int lonly_exit()
  {
    mijpeg_xt_params &xt = h.xt;
    memset(&xt.residual, 0, sizeof(xt.residual));
    for (int c = 0; c < MIJPEG_MAX_COMPONENTS; c++) {
      xt.residual.subx[c] = xt.residual.suby[c] = xt.residual.hsamp[c] = xt.residual.vsamp[c] = 1;
      h.xt_q_[c < 3 ? c : 0].clear();
      h.xt_r2_[c < 3 ? c : 0].clear();
    }
    xt.residual.width = h.info.width;
    xt.residual.height = h.info.height;
    xt.no_residual = 1;
    xt.residual_hidden_bits = 0; // (whatever the RSPC box says about a residual that is not there)
    // free-form matrices and outputs of at most eight bits (bytes out) are the general kernel's
    xt.general = (s.ltrafo >= 5 || (s.ctrafo != 255 && s.ctrafo >= 5) || s.outbits <= 8) ? 1 : 0;
    xt.qtable_entries = 16;
    for (int c = 0; c < 3; c++) xt.qtable[c] = xt.r2table[c] = nullptr;
    xt.rdct_bypass = xt.noise_shaping = xt.residual_wide = 0;
    if (!header_only)
      if (const int rc2 = legacy_hidden_scans(s.hidden_l)) return rc2;
    h.hidden_ = s.hidden_l;
    h.lonly_ = true;
    publish();
    return 0;
  }

  bool parse_residual()
  {
    HostDecoder *const res = h.residual_ = new HostDecoder();
    res->refine_scratch_ = std::move(h.spare_scratch_);
    res->refine_scratch_cap_ = h.spare_scratch_cap_;
    h.spare_scratch_cap_ = 0;
    if (residual_header(*res, header_only)) {
      if (header_only) return fail(h.residual_error_.code, h.residual_error_.message.c_str()); // (nothing will be decoded: say it now)
      // the legacy frame alone is what decode() works on; its verdict, or this one behind it (decode_t).  Where the legacy
      // codestream turns out to have no EOI the reference never looks at the residual codestream: the legacy picture through
      // the L chain, nothing merged -- the frame is set up for that
      h.drop_residual();
      return stop(lonly_exit());
    }
    const mijpeg_info &r = res->info;
    const bool residual_type = res->frame_type_ >= 3; // SOF 0xffb1, 0xffb2
    if (residual_type ? (r.precision + s.hidden_r - (s.rbits == 1) > 16 || s.rbits == 4) : (r.precision < 8 || r.precision > 12))
      return fail(MIJPEG_ERR_OPERATION_UNIMPLEMENTED, "residual codestreams of 8 to 12 bits (DCT) or up to 16 + 1 bits (residual scan type, no DCT) are on the accelerated path");
    return false;
  }

  // The Q or the R2 table of component c, named by idx[c] (255: the default, an identity).  The kernels' arithmetic identities (a
  // shift by 16 - Pr; (x + 8) >> 4) are those of a 16-bit output: at another depth the default identities are real tables as well
  // -- 2^(Pr + 4) and 2^(outbits + 4) entries, small ones (... and of four fractional bits; the flavours without clamping index
  // their Q tables with the samples as they are, colortrafo/ycbcrtrafo.cpp:752-766, 797-801, 820-822: always real tables there)
  bool residual_table(int c, const int (&idx)[4], int inbits, int infract, int outfract, std::vector<int32_t> (&store)[3], const int32_t *(&table)[3], const char *missing)
  {
    XtNlt ident;
    ident.kind = 2; ident.type = 2; ident.e = 0;
    const bool own_depth = s.outbits != 16 || s.rbits != 4 || !s.clamping;
    if (idx[c] == 255 && !own_depth) return false;
    const XtNlt &t = idx[c] != 255 ? tables.nlt[idx[c]] : ident;
    if (!t.kind) return late_r(MIJPEG_ERR_OBJECT_DOESNT_EXIST, missing);
    // (components that name the same table share one copy: a curve with a transcendental function costs ~50 ms per 2^20 entries)
    int same = -1;
    for (int j = 0; j < c; j++)
      if (idx[j] == idx[c]) same = j;
    if (same >= 0) { table[c] = table[same]; return false; }
    if (const int trc = scaled_table(t, inbits, s.outbits, infract, outfract, store[c]))
      return late_r(trc, t.kind == 1 ? "Codestream is requesting a lookup table in a path that requires fractional bits" : "Parametric tone mapping definition is invalid");
    if (own_depth || !(t.kind == 2 && t.type == 2 && t.e == 0)) table[c] = store[c].data(); // an explicit identity curve stays arithmetic
    return false;
  }

  // Q: ScaledTableOf(Pr + hidden bits, 16, 4, 4), R2: ScaledTableOf(16, 16, 4, 0) (colortransformerfactory.cpp:435-474, 486-520).
  // The identities the encoder leaves in place are evaluated arithmetically by the kernels (a shift, a rounding shift).
  // (the RCT's extra bit is a precision bit, not a fractional one: colortransformerfactory.cpp:441-446)
  bool build_residual_tables()
  {
    mijpeg_xt_params &xt = h.xt;
    const int qbits = h.residual_->info.precision + s.hidden_r - (s.rbits == 1);
    xt.qtable_entries = 1 << (qbits + s.rbits);
    for (int c = 0; c < nc; c++) {
      h.xt_q_[c].clear();
      h.xt_r2_[c].clear();
      xt.qtable[c] = xt.r2table[c] = nullptr;
      if (residual_table(c, s.qidx, qbits, s.rbits, s.rbits, h.xt_q_, xt.qtable, "the r lookup table specified in the codestream does not exist")) return true;
      // (R2 tables exist with clipping only, colortransformerfactory.cpp:481)
      if (s.clamping && residual_table(c, s.r2idx, s.outbits, 4, 0, h.xt_r2_, xt.r2table, "the R lookup table specified in the codestream does not exist")) return true;
    }
    xt.general = (s.ltrafo >= 5 || s.rtrafo >= 5 || s.rtrafo == 4 || !s.clamping || (s.ctrafo != 255 && s.ctrafo >= 5) || xt.rdct_bypass || xt.qtable[0] || xt.qtable[1] || xt.qtable[2] ||
                  xt.r2table[0] || xt.r2table[1] || xt.r2table[2]) ? 1 : 0;
    t_xt2 = std::chrono::steady_clock::now();
    return false;
  }

  // hidden bits: the visible scans of either frame address the bits above them, the boxes FINE (legacy) and RFIN
  // (residual) hold one refinement scan each, read in box order behind the visible ones (marker/frame.cpp:805-818)
  bool attach_hidden_scans()
  {
    static const bool trace_xt = getenv("MIJPEG_READ_TIMES") != nullptr; // diagnostics
    HostDecoder &res = *h.residual_;
    if (!header_only) {
      int rc2 = legacy_hidden_scans(s.hidden_l);
      if (rc2) return stop(rc2);
      rc2 = res.add_hidden_scans(boxid('R', 'F', 'I', 'N'), h.boxes_, s.hidden_r);
      if (rc2) return fail(rc2, res.error.message.c_str());
    }
    if (trace_xt && !header_only)
      fprintf(stderr, "finish_xt: residual codestream %.2f ms, tables %.2f ms, hidden scans %.2f ms\n", std::chrono::duration<double>(t_xt1 - t_xt0).count() * 1e3,
              std::chrono::duration<double>(t_xt2 - t_xt1).count() * 1e3, std::chrono::duration<double>(std::chrono::steady_clock::now() - t_xt2).count() * 1e3);
    h.hidden_ = s.hidden_l;
    res.hidden_ = s.hidden_r;
    // 12 + hidden bits do not fit the 16-bit store: such a residual frame keeps 32-bit coefficients (two slots each)
    // ... and so does a residual frame of the residual scan type beyond 12 bits (its coefficients are samples: up to 17 bits)
    const mijpeg_info &r = res.info;
    h.xt.residual_wide = (s.hidden_r > 0 || r.precision > 12) ? 1 : 0;
    const int slots = h.xt.residual_wide ? 2 : 1;
    h.xt.residual = r;
    for (int c = 0; c < r.components; c++) h.xt.residual.coef_offset[c] = h.info.coef_count + r.coef_offset[c] * slots;
    h.info.coef_count += r.coef_count * slots;
    return false;
  }

  void publish()
  {
    h.info.ycbcr = h.xt.ltrafo_ycbcr;
    h.info.xt = 1;
    h.info.is_float = h.xt.is_float;
    h.info.sample_bytes = s.outbits > 8 ? 2 : 1; // (the pixel type a client of the reference would pick for JPGTAG_IMAGE_PRECISION = outbits)
  }
};

// Every verdict the reference's colour-transformer factory gives, in the reference's order, then the parameters every config-5
// kernel consumes (mijpeg_xt_params).  A stage that ends the call -- a refusal, the plain picture, a late verdict -- leaves its
// code in f.rc.
int HostDecoder::finish_xt(bool header_only)
{
  if (plain_only_) return 0;
  XtFinish f(*this, header_only);
  f.reset_state();
  if (f.survey_boxes()) return f.rc;          // LCHK, SPEC, RESI, ALFA, ASPC / AMUL; FTON / FTRX refused
  if (f.residual_without_spec()) return f.rc; // a residual codestream nobody specifies
  if (f.without_residual()) return f.rc;      // plain JPEG; a specification alone (spec_without_residual); the frame's depth and components
  if (f.read_spec()) return f.rc;             // the SPEC box's own sub-boxes, tables inside it included
  if (f.register_file_boxes()) return f.rc;   // the file's TONE / CURV / MTRX boxes, the stand-in of an incomplete TONE box
  if (f.apply_defaults()) return f.rc;        // one component; L, R and C where the boxes are silent
  if (f.verdicts()) return f.rc;              // which transformations and conversions are valid, exist and are on this path
  f.fill_params();
  if (f.build_l_tables()) return f.rc;
  if (f.lonly) return f.lonly_exit();
  if (f.parse_residual()) return f.rc;        // its header's verdict; a refused one leaves through lonly_exit
  if (f.build_residual_tables()) return f.rc; // Q and R2
  if (f.attach_hidden_scans()) return f.rc;   // FINE and RFIN
  f.publish();
  return 0;
}

} // namespace mij
