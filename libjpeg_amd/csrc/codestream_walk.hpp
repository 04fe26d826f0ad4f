// codestream_walk.hpp -- RefWalker, the codestream state machine of the reference (codestream_walk.cpp has its description and
// its members), as far as the two files see it that run one: codestream_walk.cpp (parse, add_hidden_scans) and host_decoder.cpp
// (decode_sequential).  Included by those two only.
#ifndef MIJ_CODESTREAM_WALK_HPP
#define MIJ_CODESTREAM_WALK_HPP

#include "host_decoder.hpp"

#include <utility>

namespace mij {

struct WalkError {
  int code;
  const char *msg;
};
[[noreturn]] inline void wthrow(int code, const char *msg) { throw WalkError{code, msg}; }

// io/bytestream.hpp over memory.  Get() beyond the end: EOF; PeekWord() needs two bytes and does not move; LastUnDo()
// takes back the last byte unless the last Get() hit the end (bytestream.hpp:229-236, iostream.cpp:132-197); SkipBytes()
// beyond the end does not fail with a seekable hook (iostream.cpp:327-365 caches the seek), later reads return EOF.
struct ByteCursor {
  const uint8_t *d = nullptr;
  size_t n = 0, pos = 0;
  bool at_eof = false;
  static constexpr long END = -1;
  ByteCursor(const uint8_t *data, size_t size) : d(data), n(size) {}
  long get()
  {
    if (pos >= n) { at_eof = true; return END; }
    at_eof = false;
    return d[pos++];
  }
  long peekword() const { return pos + 2 > n ? END : ((long)d[pos] << 8) | d[pos + 1]; }
  long getword()
  {
    const long a = get();
    if (a == END) return END;
    const long b = get();
    return b == END ? END : (a << 8) | b;
  }
  void lastundo() { if (!at_eof && pos > 0) pos--; }
  // the memory stream of a box (the residual codestream, a refinement scan) throws where the file caches the seek:
  // io/bytestream.cpp:231-276 through io/decoderstream.hpp:212-216
  bool in_memory = false;
  void skip(long k)
  {
    if (k <= 0) return;
    if ((size_t)k > n - pos) {
      pos = n;
      if (in_memory) wthrow(MIJPEG_ERR_UNEXPECTED_EOF, "unexpectedly hit the end of the stream while skipping bytes");
    } else
      pos += (size_t)k;
  }
};

class RefWalker {
public:
  enum Mode { PLAN, HEADER, DECODE };
  RefWalker(HostDecoder &h, Mode m) : hd(h), mode(m), io(h.data_, h.size_) { io.in_memory = h.nested_ || h.alpha_child_; }
  void run();
  // one hidden refinement scan from a FINE / RFIN box (Frame::StartParseScan, marker/frame.cpp:805-822)
  void run_hidden(const uint8_t *box, size_t size);
  // DECODE mode: where the coefficients go
  void *coef = nullptr;
  bool wide = false; // int32 store
  int warnings = 0;

private:
  HostDecoder &hd;
  Mode mode;
  ByteCursor io;
  const uint8_t *scan_base = nullptr; // hidden scans: the box the offsets refer to
  bool scan_for_dnl = false;          // m_bScanForDNL of the scan at hand: the frame height was unknown when its parser was built
  bool header_part = false;           // the tables in front of the first frame header of the file itself: an LSE marker may stand there
  bool ls_trafo_seen = false;
  bool dri_seen = false, dri_extended = false;
  bool discover = false;              // decode_scan keeps no coefficients: it only finds out where the scan's DNL marker takes the frame
  int rows_entered = 0;               // MCU rows the last decode_scan started (a scan that brings the DNL marker may start one more than the frame has)
public:
  // The frame trailer / the image trailer stood at an EOI marker.  Only there does the reference turn to a frame's hidden
  // refinement scans (marker/frame.cpp:1063-1070) and to the residual codestream (codestream/image.cpp:1416-1431): a JPEG XT
  // file whose legacy codestream runs out without one -- truncated, or a marker where none belongs -- is decoded without them.
  bool frame_eoi = false, image_eoi = false;
  // nested: the residual codestream ran dry in front of a scan header and the search for one took the legacy stream's EOI (run())
  bool legacy_eoi_gone = false;
  // DECODE mode: what the scans of the codestream read of their entropy coded data, restart markers that were recognised left
  // out -- the bytes the LCHK checksum of a JPEG XT file runs over (HostDecoder::last_warning)
  std::vector<std::pair<size_t, size_t>> spans;
private:

  void warn() { warnings++; }
  bool tables_incremental(ByteCursor &s);
  void parse_dqt(ByteCursor &s);
  void parse_dht(ByteCursor &s);
  void box_marker(ByteCursor &s, long length);
  void frame_header(ByteCursor &s);
  bool scan_for_scan_header(ByteCursor &s);
  bool frame_trailer(ByteCursor &s);
  bool image_trailer(ByteCursor &s);
  void scan(ByteCursor &s, bool hidden);
  template <class T> void decode_scan(ByteCursor &s, const Scan &sc, bool refinement, bool progressive_run, int lowbit);
};

} // namespace mij
#endif
