// markers.hpp -- restart marker search and unstuffing of entropy coded segments on the device (markers.hip).
//
// The contract is HostDecoder::find_intervals_in's, restricted to the well-formed case.  A byte pair is only ever interpreted
// from its FF:
//   term   position of the first FF whose follower is none of 00, FF, D0..D7.  Nothing at or behind it is interpreted, kept or
//          counted.  No such FF (the data runs out; a lone FF as last byte included): term = size and MARKERS_NO_END.
//   in front of term:  FF 00  keep the FF, drop the 00
//                      FF Dn  drop both; it is the k-th restart marker (k from 0)
//                      FF FF  MARKERS_FILL
//   MARKERS_SEQUENCE   marker k's code is not 0xD0 + (k & 7)
//   MARKERS_COUNT      markers + 1 != expect
// With flags == 0: the kept bytes back to back in the destination slot, begin[0] = 0, begin[k + 1] = end[k] = kept bytes in
// front of marker k, end[expect - 1] = total, zeros from total to the end of the slot (the Huffman kernels read up to
// HUFF_STREAM_PAD beyond the data and rely on zero bits there).  With any flag set only flags and term are defined; nothing
// outside the slot and the image's `expect` table entries is ever written.
#ifndef MIJ_MARKERS_HPP
#define MIJ_MARKERS_HPP
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace mij {

constexpr uint32_t MARKERS_FILL = 1, MARKERS_SEQUENCE = 2, MARKERS_COUNT = 4, MARKERS_NO_END = 8;
constexpr uint32_t MARKERS_LANE_BYTES = 16;  // bytes a lane classifies
constexpr uint32_t MARKERS_GROUP = 256;      // lanes of a workgroup
constexpr uint32_t MARKERS_CHUNK = MARKERS_LANE_BYTES * MARKERS_GROUP; // bytes of one workgroup
constexpr size_t MARKERS_MAX_SEGMENT = (size_t)1 << 28; // segments of this size or more are refused on the host

// chunks of a segment of `size` bytes: at least one, so that an empty segment still has a workgroup that reports it
constexpr uint32_t markers_chunks(size_t size) { return size ? (uint32_t)((size + MARKERS_CHUNK - 1) / MARKERS_CHUNK) : 1u; }

// One image of a launch (device memory).
struct MarkerImage {
  uint32_t raw_off;        // byte offset of the raw segment in `raw`
  uint32_t size;           // its bytes, terminator and whatever follows included
  uint32_t dst_off;        // byte offset of the destination slot in `dst` ...
  uint32_t dst_cap;        // ... and its bytes (>= size): zero from `total` up to here
  uint32_t first_interval; // the image's first entry in ibegin / iend
  uint32_t expect;         // restart intervals the frame header asks for (>= 1)
  uint32_t first_chunk;    // its first chunk in `chunks`
  uint32_t n_chunks;       // markers_chunks(size)
};
// A workgroup works on one chunk of one image.
struct MarkerChunk {
  uint32_t image, index;
};
// What comes back per image.  The host sets term = size and the rest to zero before the first pass.
struct MarkerResult {
  uint32_t flags, term, total, markers;
};

struct MarkerArgs {
  const uint8_t *raw;          // device: the raw segments
  uint8_t *dst;                // device: the destination slots
  uint32_t *ibegin, *iend;     // device: the interval tables
  const MarkerImage *images;   // device
  const MarkerChunk *chunks;   // device: one per workgroup
  uint32_t chunk0, n_chunks;   // the chunks of this launch: [chunk0, chunk0 + n_chunks) of the arrays below (whole images)
  uint32_t *kept, *marks;      // device, per chunk: kept bytes and markers of the chunk (pass 1 writes them)
  const uint64_t *kept_at, *marks_at; // device, one more than chunks: their exclusive prefix sums over the launch's chunks
  MarkerResult *results;       // device, per image
};

// The scratch of a launch behind its descriptors, in bytes from a 16-byte aligned base: kept[C], marks[C], kept_at[C + 1],
// marks_at[C + 1] and the scratch of one exclusive_scan_u32 over C elements (hencode.hpp), used by both scans in turn.
struct MarkerScratch { size_t kept, marks, kept_at, marks_at, scan, scan_words, end; };
MarkerScratch markers_scratch(uint32_t n_chunks);

// pass 1, the two scans and pass 2 on `stream`; the argument block's kept / marks / kept_at / marks_at must point into a
// scratch laid out by markers_scratch, `scan_scratch` at its scan part.  0 or a hipError_t.
int launch_marker_search(const MarkerArgs &a, uint64_t *scan_scratch, size_t scan_words, hipStream_t stream);

// The fit step: streams without restart markers are searched with expect = 1 and then walked (huffman_walk_kernel), and only the
// search knows how many bytes the copy holds.  The host sized the walk from the raw segment -- an upper bound; behind pass 2 one
// wave per image writes what the walk really reads: img_e1 = total, img_nsub = ceil(total / sub_bytes) (never more than the
// host's bound, which it finds in img_nsub) and iend = total for each of the image's virtual intervals.  A search that is not
// good (a flag, or term not at the FF of the closing EOI) or that kept nothing: img_nsub = 0, so that no lane walks, and
// HUFF_WALK_NOT_SEARCHED in the image's walk status.
constexpr uint32_t HUFF_WALK_NOT_SEARCHED = 8; // (beside the walk's own status bits 1, 2, 4: huffman_dev.hpp)
struct MarkerFitArgs {
  const MarkerImage *images;    // device: size, first_interval
  const MarkerResult *results;  // device: what pass 2 left
  const uint32_t *fit_intervals; // device, per image: its virtual intervals, 0 = not an image the walk follows the search for
  uint32_t *img_e1, *img_nsub;  // device, per image: the walk's (HuffWalkArgs)
  uint32_t *walk_status;        // device, per image
  uint32_t *iend;               // device: the interval table
  uint32_t sub_bytes, n_images;
};
int launch_marker_fit(const MarkerFitArgs &a, hipStream_t stream);

} // namespace mij
#endif
