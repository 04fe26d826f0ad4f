// hencode.hpp -- argument blocks of the on-device entropy coder (hencode.hip); internal to libmijpeg.so.
#ifndef MIJ_HENCODE_HPP
#define MIJ_HENCODE_HPP
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

namespace mij {

// code word and length per symbol of the four tables of a scan (DC/AC for the first component, DC/AC for the others); DC categories
// 0..15 and every AC run/size symbol have a place, so the tables serve 12-bit frames (categories to 15 / 14) as they are
struct HencTables {
  uint16_t dc_code[2][16];
  uint16_t ac_code[2][256];
  uint8_t dc_len[2][16];
  uint8_t ac_len[2][256];
};
static_assert(sizeof(HencTables) % 16 == 0, "copied to LDS in dwords");

constexpr int HENC_STUFF_CHUNK = 64; // bytes of the plain stream one lane of the stuffing kernels handles

struct HencArgs {
  const int16_t *coef;          // coefficient planes of the frame (decoder layout)
  const HencTables *tables;     // device
  int32_t ncomp, mcus_x, total_mcus, ri, blocks_per_mcu; // ri: MCUs per restart interval (= total_mcus without restart markers)
  int32_t hs[4], vs[4], bw[4], nbx[4], nby[4];
  int64_t coef_off[4];
  uint8_t blk_comp[64], blk_bx[64], blk_by[64]; // block j of an MCU: component, position inside the MCU
  uint32_t total_blocks, n_intervals;
  uint32_t *bits;               // per block in scan order: length of its code in bits
  const uint64_t *bitpos;       // exclusive prefix sums of bits (total_blocks + 1 entries)
  uint32_t *ibytes;             // per interval: bytes of its entropy coded segment before stuffing
  const uint64_t *istart;       // exclusive prefix sums of ibytes (n_intervals + 1 entries): byte offsets in the plain stream
  uint32_t *plain;              // plain (unstuffed) stream as big-endian 32-bit words, zeroed
  uint64_t plain_bytes;
  uint32_t *ffcount;            // per HENC_STUFF_CHUNK bytes of the plain stream: 0xFF bytes in them
  const uint64_t *ffstart;      // exclusive prefix sums of ffcount (chunks + 1 entries)
  uint8_t *out;                 // entropy coded data with stuffing and RSTn markers
  uint32_t *hist;               // optional statistics: [2][256] DC symbol counts, [2][256] AC symbol counts (null in a list: the
                                // picture takes no part in the statistics launch)
};

// Batch-wide flavour (encode_device.cpp): ONE launch of every pass over all pictures of a list.  Every picture has an argument
// block of its own in device memory whose bits / bitpos / ibytes / istart point at the picture's own first block and first
// interval inside arrays that run over the whole pass (the kernels only ever look at differences of bitpos and istart, so the
// picture's entries of the pass-wide prefix sums serve as they are) and whose coef / tables / hist are the picture's.  plain,
// ffcount, ffstart and out of those blocks are not read: they are the pass's, below.
//   blocks     padded per picture to a multiple of 256: a workgroup belongs to one picture, padding lanes write bits = 0
//   intervals  the pictures' lists one behind the other; every picture starts a new interval
//   plain      picture p from byte first_chunk[p] * HENC_STUFF_CHUNK of a common zeroed buffer: no word and no chunk is shared
//   out        the plain layout with the stuffing bytes and markers of everything in front added: picture p's entropy coded
//              segment starts at first_chunk[p] * HENC_STUFF_CHUNK + ffstart[first_chunk[p]] + 2 * (first_interval[p] - p)
struct HencBatchArgs {
  const HencArgs *pics;           // device, n entries
  const uint32_t *first_block;    // n + 1 entries, multiples of 256
  const uint32_t *first_interval; // n + 1 entries
  const uint32_t *first_chunk;    // n + 1 entries (known once the plain sizes are: henc_emit and later)
  uint32_t n, total_blocks, total_intervals, total_chunks;
  uint32_t *plain;
  uint32_t *ffcount;
  const uint64_t *ffstart;
  uint8_t *out;
};

// where the categories of henc_survey saturate: above every category a frame can code (DC 11 / 15, AC 10 / 14), small enough for
// (run << 4) | category to stay an AC symbol and for the DC category to stay inside its row of hist[]
constexpr int HENC_SURVEY_DC_CAT = 17, HENC_SURVEY_AC_CAT = 15;

int henc_count(const HencArgs &a, bool statistics, hipStream_t stream);      // bits[] (and hist[])
int henc_survey(const HencArgs &a, hipStream_t stream);                      // hist[] alone, safe for any int16 content
int henc_interval_bytes(const HencArgs &a, hipStream_t stream);              // ibytes[] from bitpos[]
int henc_emit(const HencArgs &a, hipStream_t stream);                        // plain[]
int henc_count_ff(const HencArgs &a, hipStream_t stream);                    // ffcount[]
int henc_stuff(const HencArgs &a, hipStream_t stream);                       // out[]
int henc_count(const HencBatchArgs &b, bool statistics, hipStream_t stream);
int henc_interval_bytes(const HencBatchArgs &b, hipStream_t stream);
int henc_emit(const HencBatchArgs &b, hipStream_t stream);
int henc_count_ff(const HencBatchArgs &b, hipStream_t stream); // (the one-frame kernel over the common plain buffer)
int henc_stuff(const HencBatchArgs &b, hipStream_t stream);
// dst[i] = src[idx[i]], i < n: the entries of a pass-wide prefix sum the host lays the pictures out with
int henc_gather(const uint64_t *src, const uint32_t *idx, uint64_t *dst, uint32_t n, hipStream_t stream);
// ---- exclusive prefix sums (hencode.hip): tiles of HENC_SCAN_TILE, recursively -------------------------------------
// The scratch of an exclusive_scan_u32 over n elements, in uint64 words; this is its only statement: the scan takes its pointers
// from it and its callers their buffer sizes.
//   level 0   the n elements in tiles1 = n / TILE + 1 tiles (the last one holds out[n]); one tile: one launch, no scratch
//   level 1   sums1[tiles1]: the tiles' sums (and one spare word); off1[tiles1 + 1]: their exclusive prefix sums.  Up to TILE - 1
//             of them are scanned by one workgroup: three launches
//   level 2   beyond that sums1 is scanned in tiles2 = tiles1 / TILE + 1 tiles of its own: sums2[tiles2] (and a spare word),
//             off2[tiles2 + 1]: five launches.  One workgroup scans sums2, so tiles2 <= TILE: n <= HENC_SCAN_MAX
constexpr uint32_t HENC_SCAN_TILE = 1024;
struct ScanLayout {
  uint32_t tiles1, tiles2;
  int launches;                     // 1, 3 or 5
  uint64_t sums1, off1, sums2, off2; // first word of each array
  uint64_t end1, end2;              // behind off1, behind off2 (0 where the level does not exist)
  uint64_t words;                   // all of it
  bool in_reach;                    // n <= HENC_SCAN_MAX
};
constexpr ScanLayout scan_layout(uint32_t n)
{
  ScanLayout l{};
  l.tiles1 = n / HENC_SCAN_TILE + 1;
  l.tiles2 = l.tiles1 / HENC_SCAN_TILE + 1;
  l.in_reach = l.tiles2 <= HENC_SCAN_TILE;
  l.launches = 1;
  if (l.tiles1 == 1) return l;
  l.sums1 = 0;
  l.off1 = l.sums1 + l.tiles1 + 1;
  l.end1 = l.off1 + l.tiles1 + 1;
  l.words = l.end1;
  l.launches = 3;
  if (l.tiles2 == 1) return l;
  l.sums2 = l.end1;
  l.off2 = l.sums2 + l.tiles2 + 1;
  l.end2 = l.off2 + l.tiles2 + 1;
  l.words = l.end2;
  l.launches = 5;
  return l;
}
constexpr uint32_t HENC_SCAN_MAX = (HENC_SCAN_TILE * HENC_SCAN_TILE - 1) * HENC_SCAN_TILE - 1; // 2^30 - 1025
constexpr bool scan_layout_consistent(uint32_t n)
{
  const ScanLayout l = scan_layout(n);
  const bool one = l.launches == 1 && l.tiles1 == 1 && l.words == 0;
  const bool three = l.launches == 3 && l.tiles1 > 1 && l.tiles2 == 1 && l.off1 == (uint64_t)l.tiles1 + 1 && l.end1 == 2 * ((uint64_t)l.tiles1 + 1) && l.words == l.end1;
  const bool five = l.launches == 5 && l.tiles2 > 1 && l.sums2 == l.end1 && l.end1 == 2 * ((uint64_t)l.tiles1 + 1) &&
                    l.end2 == l.end1 + 2 * ((uint64_t)l.tiles2 + 1) && l.words == l.end2;
  return one || three || five;
}
static_assert(scan_layout_consistent(0) && scan_layout(0).launches == 1, "one tile");
static_assert(scan_layout_consistent(1023) && scan_layout(1023).launches == 1, "one tile: 1023 elements and the total");
static_assert(scan_layout_consistent(1024) && scan_layout(1024).launches == 3 && scan_layout(1024).words == 6, "two tiles");
static_assert(scan_layout_consistent((1u << 20) - 1025) && scan_layout((1u << 20) - 1025).launches == 3 && scan_layout((1u << 20) - 1025).words == 2 * 1024,
              "1023 tile sums: the last count one workgroup scans");
static_assert(scan_layout_consistent((1u << 20) - 1024) && scan_layout((1u << 20) - 1024).launches == 5 && scan_layout((1u << 20) - 1024).words == 2 * 1025 + 2 * 3,
              "1024 tile sums: the second level");
static_assert(scan_layout_consistent(1u << 20) && scan_layout(1u << 20).launches == 5 && scan_layout(1u << 20).words == 2 * 1026 + 2 * 3, "second level");
static_assert(scan_layout_consistent((1u << 30) - 1) && scan_layout((1u << 30) - 1).launches == 5 && scan_layout((1u << 30) - 1).words == 2 * ((1u << 20) + 1) + 2 * 1026,
              "the layout arithmetic holds past the scan's reach");
static_assert(scan_layout(HENC_SCAN_MAX).in_reach && !scan_layout(HENC_SCAN_MAX + 1).in_reach && !scan_layout((1u << 30) - 1).in_reach, "the scan's reach");

// ---- the coder's buffers (encode_device.cpp) ------------------------------------------------------------------------
// Their only statement, for one frame and for a pass of a list alike: the host drivers take offsets, sizes, the extent to zero and
// the scans' capacity from here.  Offsets are bytes from the start of a 256-byte aligned region; every array starts on such a boundary.
constexpr size_t henc_aligned(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
// words of scratch for an exclusive_scan_u32 over n elements, some to spare (n beyond the scan's reach: the scan refuses whatever it gets)
constexpr size_t scan_scratch_words(size_t n) { return (size_t)scan_layout((uint32_t)(n < HENC_SCAN_MAX ? n : HENC_SCAN_MAX)).words + 32; }

// the arrays over N blocks and I intervals: bits[N], bitpos[N + 1], ibytes[I], istart[I + 1], ONE scratch for the scan over the
// blocks and then the one over the intervals
struct CoderLayout { uint32_t N, I; size_t bits, bitpos, ibytes, istart, scratch, end, scratch_words; };
constexpr CoderLayout coder_layout(uint32_t N, uint32_t I)
{
  CoderLayout l{N, I};
  l.bitpos = l.bits + henc_aligned((size_t)N * 4);
  l.ibytes = l.bitpos + henc_aligned(((size_t)N + 1) * 8);
  l.istart = l.ibytes + henc_aligned((size_t)I * 4);
  l.scratch = l.istart + henc_aligned(((size_t)I + 1) * 8);
  l.scratch_words = scan_scratch_words(N > I ? N : I);
  l.end = l.scratch + henc_aligned(l.scratch_words * 8);
  return l;
}
// the output arena of a plain stream of `chunks` times HENC_STUFF_CHUNK bytes in I intervals: the plain stream (`zeroed` bytes of
// it are cleared before henc_emit), ffcount[chunks + 1], ffstart[chunks + 1], out (every byte stuffed and a marker per interval at
// the most), and a scratch for the scan over the CHUNKS, which may outnumber the blocks
struct OutputLayout { uint32_t chunks; size_t plain, ffcount, ffstart, out, scratch, end, zeroed, scratch_words; };
constexpr OutputLayout output_layout(uint32_t chunks, uint32_t I)
{
  OutputLayout l{chunks};
  l.zeroed = (size_t)chunks * HENC_STUFF_CHUNK + 16;
  l.ffcount = l.plain + henc_aligned(l.zeroed);
  l.ffstart = l.ffcount + henc_aligned(((size_t)chunks + 1) * 4);
  l.out = l.ffstart + henc_aligned(((size_t)chunks + 1) * 8);
  l.scratch = l.out + henc_aligned((size_t)chunks * HENC_STUFF_CHUNK * 2 + (size_t)I * 2 + 16);
  l.scratch_words = scan_scratch_words(chunks);
  l.end = l.scratch + henc_aligned(l.scratch_words * 8);
  return l;
}
// every region starts at or behind the end of the one before it, and a scratch holds what scan_layout() says its scans take
constexpr bool coder_layout_consistent(uint32_t N, uint32_t I)
{
  const CoderLayout l = coder_layout(N, I);
  return l.bitpos >= l.bits + (size_t)N * 4 && l.ibytes >= l.bitpos + ((size_t)N + 1) * 8 && l.istart >= l.ibytes + (size_t)I * 4 && l.scratch >= l.istart + ((size_t)I + 1) * 8 &&
         l.end >= l.scratch + l.scratch_words * 8 && l.scratch_words >= scan_layout(N).words && l.scratch_words >= scan_layout(I).words;
}
constexpr bool output_layout_consistent(uint32_t chunks, uint32_t I)
{
  const OutputLayout l = output_layout(chunks, I);
  const size_t plain_bytes = (size_t)chunks * HENC_STUFF_CHUNK;
  return l.zeroed >= plain_bytes && l.ffcount >= l.plain + l.zeroed && l.ffstart >= l.ffcount + ((size_t)chunks + 1) * 4 && l.out >= l.ffstart + ((size_t)chunks + 1) * 8 &&
         l.scratch >= l.out + 2 * plain_bytes + 2 * (size_t)I + 16 && l.end >= l.scratch + l.scratch_words * 8 && l.scratch_words >= scan_layout(chunks).words;
}
static_assert(coder_layout_consistent(0, 0) && coder_layout_consistent(1023, 1023) && coder_layout_consistent(1024, 1) && coder_layout_consistent(1024, 1024) &&
                  coder_layout_consistent((1u << 20) - 1025, 1) && coder_layout_consistent((1u << 20) - 1024, (1u << 20) - 1024) &&
                  coder_layout_consistent(HENC_SCAN_MAX, 1) && coder_layout_consistent(HENC_SCAN_MAX, HENC_SCAN_MAX),
              "the arrays over blocks and intervals do not overlap and their scratch holds either scan");
static_assert(output_layout_consistent(0, 1) && output_layout_consistent(1023, 1) && output_layout_consistent(1024, 1024) && output_layout_consistent((1u << 20) - 1025, 1) &&
                  output_layout_consistent((1u << 20) - 1024, 65536) && output_layout_consistent(HENC_SCAN_MAX, 1),
              "the regions of the output arena do not overlap; the zeroed extent reaches the last chunk's end and stops in front of ffcount");
static_assert(coder_layout(1u << 22, 1).scratch_words < scan_layout(1u << 23).words && output_layout(1u << 23, 1).scratch_words >= scan_layout(1u << 23).words,
              "the scan over the chunks has a scratch sized from the chunks: 2^22 blocks of 128 bytes each are 2^23 chunks, past the blocks' scratch");

// out[i] = sum of in[0..i) for i = 0..n (n + 1 entries); scratch: scratch_words uint64, at least scan_layout(n).words of them.
// hipErrorInvalidValue, before anything is launched, where the scratch is smaller or n is beyond HENC_SCAN_MAX
int exclusive_scan_u32(const uint32_t *in, uint64_t *out, uint32_t n, uint64_t *scratch, size_t scratch_words, hipStream_t stream);

} // namespace mij
#endif
