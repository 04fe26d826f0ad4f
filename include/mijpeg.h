/*
 * mijpeg.h -- C ABI of the MI355X-native JPEG block-decode path (libjpeg_amd/libmijpeg.so).
 *
 * This is the drop-in boundary for the hot path of thorfdbg/libjpeg:
 *
 *      JPEG::Read            (interface/jpeg.cpp:205-354)   -> mijpeg_set_input + mijpeg_read_header
 *                                                              + mijpeg_decode_coefficients (+ upload)
 *      JPEG::GetInformation  (interface/jpeg.cpp:822-957)   -> mijpeg_info (filled by read_header)
 *      JPEG::DisplayRectangle(interface/jpeg.cpp:694-722)   -> mijpeg_reconstruct_rect
 *          = Image::ReconstructRegion (codestream/image.cpp:1087-1123)
 *          = BlockBitmapRequester::ReconstructRegion (control/blockbitmaprequester.cpp:1249-1272)
 *      JPEG::LastError       (interface/jpeg.cpp:959-968)   -> mijpeg_last_error
 *
 * The reference has no C ABI (it exports the C++ class JPEG); the source-compatible class JPEG in
 * libjpeg_amd/csrc/interface/ is implemented on top of these entry points, see INTEGRATION.md.
 *
 * Conventions: extern "C", plain pointers and sizes, int return codes (0 = ok, negative = the
 * reference's JPGERR_* value, interface/parameters.hpp:1156-1228), no exceptions cross the
 * boundary, the library never takes ownership of pixel memory.  hipStream_t is passed as void*.
 */
#ifndef MIJPEG_H
#define MIJPEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIJPEG_MAX_COMPONENTS 4

/* Error codes: numeric values of the reference's JPGERR_* (interface/parameters.hpp:1156-1228). */
#define MIJPEG_OK 0
#define MIJPEG_ERR_INVALID_PARAMETER (-1024)
#define MIJPEG_ERR_UNEXPECTED_EOF (-1025)
#define MIJPEG_ERR_UNEXPECTED_EOB (-1026)
#define MIJPEG_ERR_STREAM_EMPTY (-1027)
#define MIJPEG_ERR_OVERFLOW_PARAMETER (-1028)
#define MIJPEG_ERR_NOT_AVAILABLE (-1029)
#define MIJPEG_ERR_OBJECT_EXISTS (-1030)
#define MIJPEG_ERR_OBJECT_DOESNT_EXIST (-1031)
#define MIJPEG_ERR_MISSING_PARAMETER (-1032)
#define MIJPEG_ERR_BAD_STREAM (-1033)
#define MIJPEG_ERR_OPERATION_UNIMPLEMENTED (-1034)
#define MIJPEG_ERR_PHASE_ERROR (-1035)
#define MIJPEG_ERR_NO_JPG (-1036)
#define MIJPEG_ERR_DOUBLE_MARKER (-1037)
#define MIJPEG_ERR_MALFORMED_STREAM (-1038)
#define MIJPEG_ERR_NOT_IN_PROFILE (-1040)
#define MIJPEG_ERR_THREAD_ABORTED (-1041)
#define MIJPEG_ERR_INVALID_HUFFMAN (-1042)
#define MIJPEG_ERR_OUT_OF_MEMORY (-2048)
#define MIJPEG_ERR_DEVICE (-8191) /* HIP runtime failure (no reference equivalent) */

/* flags for the reconstruct calls */
#define MIJPEG_FLAG_NO_COLOR_TRANSFORM 1u /* JPGTAG_MATRIX_LTRAFO = JPGFLAG_MATRIX_COLORTRANSFORMATION_NONE (CLI -c) */
#define MIJPEG_FLAG_FORCE_GENERIC 2u      /* use the unfused generic kernels even where a fused one exists (testing) */
#define MIJPEG_FLAG_FORCE_SAFE 4u         /* use the 32/64-bit "safe" arithmetic flavour even if the range check passed */
#define MIJPEG_FLAG_NO_UPSAMPLING 16u      /* mijpeg_reconstruct_rect: JPGTAG_DECODER_UPSAMPLE = false -- one component on its own sample grid */
#define MIJPEG_FLAG_DEVICE_OUTPUT 8u      /* mijpeg_reconstruct_rect: dst[] are DEVICE pointers; nothing crosses PCIe */
#define MIJPEG_FLAG_FORCE_DOT2 64u        /* (testing) the 16-bit second pass of the packed 4:2:0 kernel whatever the range check says */
#define MIJPEG_FLAG_SPECULATIVE 32u       /* mijpeg_reconstruct_batch_device with sync = 0 on a SUBMITTED batch: launch the reconstruction
                                             behind the Huffman kernel without waiting for that kernel's report (see there) */

typedef struct mijpeg_decoder mijpeg_decoder;

/* Frame geometry, as JPEG::GetInformation reports it plus the coefficient-plane layout. */
typedef struct mijpeg_info {
  int32_t width, height;     /* JPGTAG_IMAGE_WIDTH / HEIGHT                                     */
  int32_t components;        /* JPGTAG_IMAGE_DEPTH                                              */
  int32_t precision;         /* JPGTAG_IMAGE_PRECISION: 8 or 12 (16 for JPEG XT)                */
  int32_t hsamp[MIJPEG_MAX_COMPONENTS], vsamp[MIJPEG_MAX_COMPONENTS]; /* SOF Hi, Vi              */
  int32_t subx[MIJPEG_MAX_COMPONENTS], suby[MIJPEG_MAX_COMPONENTS];   /* JPGTAG_IMAGE_SUBX/SUBY  */
  int32_t quant_index[MIJPEG_MAX_COMPONENTS];                         /* SOF Tqi                 */
  int32_t mcus_x, mcus_y;    /* interleaved MCU grid                                            */
  int32_t blocks_w[MIJPEG_MAX_COMPONENTS], blocks_h[MIJPEG_MAX_COMPONENTS]; /* plane size, blocks */
  int32_t restart_interval;  /* DRI                                                             */
  int32_t ycbcr;             /* 1 = L-transformation is YCbCr->RGB (codestream/tables.cpp:2021-2030) */
  int32_t fast_arith;        /* set by decode_coefficients: 1 = every block passed the range check */
  int64_t coef_offset[MIJPEG_MAX_COMPONENTS]; /* start of each component plane, in int16 units   */
  int64_t coef_count;        /* total int16 coefficients of one frame (all planes)              */
  uint16_t quant[4][64];     /* DQT deltas in natural order, index = Tq                          */
  int32_t range_max[MIJPEG_MAX_COMPONENTS]; /* set by decode_coefficients: max over the component's blocks of
                                sum_k |c_k| * q_k (bounds every IDCT output by 4 * range_max) */
  int32_t sample_bytes;      /* bytes per output sample: 1 (precision 8), 2 (precision 12, JPEG XT)          */
  int32_t xt;                /* 1 = JPEG XT profile C stream (three components or one): see mijpeg_xt_params     */
  int32_t is_float;          /* JPGTAG_IMAGE_IS_FLOAT: the 16-bit codes are half-float bit patterns          */
  int32_t progressive;       /* 1 = progressive frame (SOF2): informational, the reconstruction is the same         */
  int32_t coef_wide;         /* 1 = the planes hold int32 coefficients, two int16 slots each (coef_offset[] and coef_count
                                stay in int16 units and count both slots).  Set by mijpeg_decode_coefficients for the
                                streams -- damaged ones -- whose DC prediction or point transform leaves the 16-bit range:
                                the reference keeps LONG coefficients (coding/blockrow.hpp) and so does this frame; it is
                                reconstructed by the unfused kernels with the reference's 32-bit transform          */
  int32_t dnl;               /* 1 = the frame header carried zero lines and the height arrived in a DNL marker behind the first
                                scan.  The reference has set up its buffers by then and the traces stay in the picture
                                (DESIGN.md "DNL frames"): block rows are created MCU row by MCU row without a bound until
                                the marker is seen (control/blockbuffer.cpp:212-265), and the upsamplers never learn the
                                height (control/blockbitmaprequester.cpp:298-322, upsampling/upsamplerbase.cpp:61-75): their
                                line buffers have no bottom edge.  For such frames blocks_h[] counts one MCU row more than
                                mcus_y * vsamp[] -- the row the first scan creates behind the picture when it meets the marker
                                only there -- and rows[] below tells how far the scans really got                        */
  int32_t rows[MIJPEG_MAX_COMPONENTS]; /* set by decode_coefficients for dnl frames: block rows of the component the scans created;
                                a row below that reads as NULL and transforms to sample value 0 (dct/idct.cpp:336-338)    */
} mijpeg_info;

/* JPEG XT (ISO/IEC 18477-7) profile C parameters of the loaded stream, valid when info.xt != 0:
 * what ColorTransformerFactory::InstallIntegerParameters (colortrafo/colortransformerfactory.cpp:300-594)
 * installs into YCbCrTrafo<UWORD,3,Residual|Extended|ClampFlag|Float,...>.  Supported: explicit (TONE box), parametric
 * (CURV box) or identity L tables, parametric or identity Q and R2 tables, standard or free-form (MTRX box) L, R and C
 * transformations, residual codestream = Huffman sequential / progressive 8..12 bit with the fixpoint DCT or the DCT
 * bypass, hidden refinement scans (-R / -rR of the reference encoder: FINE / RFIN boxes, up to four bits each); merging
 * specifications WITHOUT a residual codestream (the L chain alone: no_residual); the lossless / near-lossless files of part 8 that
 * need no integer DCT (-ro, -Q 100: residual scan types FFB1 / FFB2, RCT, no clamping; rct, rbits, clamp below); alpha channels
 * (mijpeg_alpha_channel).
 * Not supported (JPGERR_NOT_IMPLEMENTED): the integer (lifting) DCT of part 8 (-l, -rl), profiles A / B (float tables, pre/post
 * scaling), arithmetic coding. */
typedef struct mijpeg_xt_params {
  mijpeg_info residual;      /* residual codestream: geometry and quantiser tables; its coef_offset[] are offsets
                                into the SAME per-frame coefficient buffer, behind the legacy planes            */
  int32_t ltable[3][4096];   /* L lookup tables per component: 8 + hidden_bits in, 16 bit out (ltable_entries used)  */
  int32_t ltable_entries;    /* 256 << hidden_bits                                                               */
  int32_t hidden_bits;       /* RSPC: low bits of the legacy coefficients that arrived in hidden refinement scans
                                (FINE boxes); the legacy frame reconstructs at precision 8 + hidden_bits         */
  int32_t residual_hidden_bits; /* ... of the residual coefficients (RFIN boxes): precision 12 + residual_hidden_bits */
  int32_t residual_wide;     /* 1: the residual planes hold int32 coefficients (two int16 slots each)           */
  int32_t ltrafo_ycbcr;      /* L transformation: 1 = YCbCr -> RGB, 0 = identity                                */
  int32_t rtrafo_ycbcr;      /* R transformation                                                                */
  int32_t out_max;           /* 2^(8 + extra range bits) - 1: 65535 (half-float codes, 16-bit integers) or 255              */
  int32_t out_shift;         /* (out_max + 1) / 2                                                               */
  int32_t is_float, clamp;   /* output conversion box: cast to float, clamping                                  */
  /* Beyond what the reference's encoder writes by default (all of it decodes like the reference, bit for bit):
   * free-form L / R / C transformations (MTRX boxes, the encoder's -xyz / -cxyz), parametric curves (CURV boxes) as L, Q
   * or R2 tables, a residual DCT bypass (RDCT box).  `general` != 0 when any of these is in use: the reconstruction
   * then runs the unfused kernels with the literal 64-bit merge and table gathers. */
  int32_t general;
  int32_t lmat[9], rmat[9], cmat[9]; /* 13 fractional bits (ColorTrafo::FIX_BITS); the standard matrices when not free-form */
  int32_t rdct_bypass;       /* RDCT box: no residual DCT, samples = coefficient * (delta[63] << 4) + 2^(Pr-1)
                                (control/residualblockhelper.cpp:203-231) */
  int32_t noise_shaping;     /* ... with the 2x2 averaging of that function                                         */
  int32_t qtable_entries;    /* 2^(residual precision + hidden bits + 4)                                             */
  const int32_t *qtable[3];  /* HOST memory, owned by the decoder object: Q table per component, qtable_entries each;
                                NULL = the identity (a shift)                                                        */
  const int32_t *r2table[3]; /* HOST memory: R2 table per component, (out_max + 1) << 4 entries (2^20 at 16 bits of output);
                                NULL = the identity (x + 8) >> 4                                                     */
  int32_t no_residual;       /* 1: nothing is merged (rr = m_lOutDCShift, colortrafo/ycbcrtrafo.cpp:744-746), the legacy picture goes
                                through the L chain alone.  Either the legacy codestream never came to an EOI marker and the
                                reference has not parsed the residual codestream (codestream/image.cpp:1416-1431): the residual
                                planes are zeros and the merge ignores them.  Or the file has a merging specification and NO
                                residual codestream (`jpeg -R n` without `-r` from HDR / 16-bit input; the transformer with R
                                transformation "zero", colortrafo/colortransformerfactory.cpp:262-283): residual.components is 0,
                                the coefficient store ends behind the legacy planes                                            */
  int32_t ltrafo_standard;   /* 1: the L transformation is the STANDARD YCbCr one (not a free-form matrix): the one a request without
                                colour transformation (MIJPEG_FLAG_NO_COLOR_TRANSFORM, the command line's -c) replaces by the
                                identity -- and nothing else of the merge (colortrafo/colortransformerfactory.cpp:231-232)          */
  /* Lossless / near-lossless coding (part 8: the reference encoder's -ro and -Q 100): the residual codestream is of the residual scan
   * type (SOF 0xffb1, no DCT: rdct_bypass), merged through the reversible colour transformation and without clamping */
  int32_t rct;               /* R transformation = RCT (colortrafo/ycbcrtrafo.cpp:752-766); rtrafo_ycbcr is 0 then                     */
  int32_t rbits;             /* fractional bits of the residual path: 4; 1 with the RCT (a precision bit: Q tables of 2^Pr entries); 0 for
                                the identity under the lossless flag (Tables::FractionalColorBitsOf, codestream/tables.cpp:1621-1660)  */
} mijpeg_xt_params;

/* ---- decoder object (one image at a time; one object = one host thread at a time) ---------- */

/* device >= 0: HIP device ordinal, coefficient store is pinned host memory + a device mirror.
 * device  < 0: host-only object (header parsing and entropy decoding, no GPU needed). */
int mijpeg_create(mijpeg_decoder **out, int device);
void mijpeg_destroy(mijpeg_decoder *d);

/* The byte range is borrowed until the next set_input / destroy. */
int mijpeg_set_input(mijpeg_decoder *d, const uint8_t *data, size_t size);

/* SOI .. first SOS: tables, frame header.  Replaces Decoder::ParseHeaderIncremental +
 * Image::StartParseFrame (codestream/decoder.cpp:77, codestream/image.cpp:660). */
int mijpeg_read_header(mijpeg_decoder *d, mijpeg_info *info);

/* Entropy-decode all scans into the planar int16 coefficient store (natural order, quantised):
 * replaces the Scan::ParseMCU loop of JPEG::ReadInternal (interface/jpeg.cpp:300-340) =
 * SequentialScan::ParseMCU/DecodeBlock (codestream/sequentialscan.cpp:381-428, 678-773).
 * threads <= 0: one per host core.  Restart intervals decode in parallel.  With a device, MCU-row
 * bands are hipMemcpyAsync'ed to the GPU while later bands are still being decoded. */
int mijpeg_decode_coefficients(mijpeg_decoder *d, int threads);

/* The same on the GPU: the host only parses the headers and locates the restart markers, the compressed
 * bytes are uploaded (a few MB instead of ~100 MB of coefficients) and one device thread decodes one restart interval.
 * Available for single-scan Huffman sequential 8-bit frames with a restart interval and at least min_intervals
 * restart intervals (<= 0: library default, below which the host decoder is the faster one); otherwise -- and for every
 * stream that turns out to be damaged (irregular restart markers, an error inside an interval, a virtual interval that does
 * not end where the next begins): the reference's behaviour on those is that of its sequential walk, which the host decoder
 * restates -- it returns MIJPEG_ERR_NOT_AVAILABLE and the caller uses mijpeg_decode_coefficients on the same object.
 * After it, mijpeg_coefficients() downloads the planes on first use. */
int mijpeg_decode_coefficients_device(mijpeg_decoder *d, int min_intervals);

/* Batches (SURVEY config 4: many frames of one shape).  n codestreams of identical width, height and
 * sampling, each qualifying for mijpeg_decode_coefficients_device, are parsed on the host in parallel, uploaded
 * and entropy-decoded by ONE kernel launch (every workgroup works on one image; the restart intervals of all images fill
 * the device, which a single image rarely does), into n coefficient stores that mijpeg_reconstruct_batch_device turns
 * into n frames (`frame_stride` bytes apart, interleaved samples, `row_stride` bytes per line) with ONE launch of the
 * reconstruction kernel.  Nothing but the compressed bytes crosses PCIe.  MIJPEG_ERR_NOT_AVAILABLE when the streams do
 * not form such a batch.  The stream bytes are only read during the call.
 * Images may bring quantisation tables of their own (motion JPEG under rate control): the reconstruction launch then
 * reads per-frame tables from device memory (mijpeg_batch.quant_dev below) and mijpeg_get_info reports, per component,
 * the largest delta of any image.
 * Streams: every call of a decoder object works on the object's own non-blocking stream.  Device memory handed to it
 * (dst_device, device bitmaps, pixels to encode) must not have work pending on other streams when the call is made, and
 * is complete when a call returns with sync != 0. */
int mijpeg_decode_batch_device(mijpeg_decoder *d, const uint8_t *const *streams, const size_t *sizes, int n, int min_intervals);
/* The same in two halves, for pipelines that keep several decoder objects in flight from one thread: submit parses the headers,
 * gathers the streams into pinned memory and ENQUEUES upload and Huffman kernel on the object's stream, then returns (the stream
 * bytes are only read during the call); finish waits for them and evaluates what the kernel reported (errors, range check).
 * mijpeg_reconstruct_batch_device and mijpeg_get_info finish a submitted batch themselves.  While one object's batch is on the
 * device the host prepares the next one with another object: see libjpeg_amd/batch.py (BASELINE config 4).  Batches of streams
 * without restart markers get a fixed, generous number of device-walk rounds (rounds in which nothing changes cost
 * microseconds); finish answers MIJPEG_ERR_NOT_AVAILABLE in the unlikely case that the walk had not settled by then, and
 * mijpeg_decode_batch_device, which looks at the walk between its rounds, decodes such a batch. */
int mijpeg_submit_batch_device(mijpeg_decoder *d, const uint8_t *const *streams, const size_t *sizes, int n, int min_intervals);
int mijpeg_finish_batch_device(mijpeg_decoder *d);
/* Pipelines that never block on the device: mijpeg_reconstruct_batch_device(.., flags | MIJPEG_FLAG_SPECULATIVE, sync = 0) on a batch
 * that was only SUBMITTED launches the reconstruction right behind the Huffman kernel, on the range check (the kernel selection's
 * input, which the Huffman kernel reports) of the last finished batch of the same frame shape and tables, rounded up to the next
 * gate of the selection -- instead of waiting for this batch's.  mijpeg_finish_batch_device then VALIDATES: it waits, evaluates what
 * the Huffman kernel reported (damaged streams: the usual MIJPEG_ERR_NOT_AVAILABLE) and, should the real range check lie beyond the
 * assumed one, runs the reconstruction again with the kernel it selects (synchronously, into the same destination).  Until it has
 * returned MIJPEG_OK the destination's pixels do not count; mijpeg_synchronize and the next mijpeg_submit_batch_device validate as
 * well (and report the batch's error).  Without a finished batch of this shape to go by, with per-image tables, or for streams
 * without restart markers the call behaves as without the flag.  mijpeg_batch_speculation: diagnostics -- returns 1 when the last
 * validation had to reconstruct again; *launched / *redone count the object's speculative launches and the ones redone. */
int mijpeg_batch_speculation(mijpeg_decoder *d, int64_t *launched, int64_t *redone);
/* BASELINE config 4 as ONE call (round 6; libjpeg_amd/csrc/batch_pipeline.cpp -- until then a Python loop): `decoder_objects`
 * decoder objects on `device`, driven round-robin by the calling thread over chunks of `chunk_frames` streams (ramp != 0:
 * smaller chunks at both ends of the batch): submit of chunk i + 1 (host: parse, marker search, gather) while chunk i's upload,
 * Huffman kernel and fused kernel run.  run: n streams of one shape, bytes in host memory -> frame i at dst_device + i *
 * frame_stride (device memory, `row_stride` bytes per line); returns when every frame is there.  download_host != NULL: the
 * frames also travel to that (pinned) host buffer, same strides, each chunk as soon as its reconstruction is through, on a
 * stream of the pipeline's own; run returns when the last one has arrived.  A chunk the device path declines
 * (MIJPEG_ERR_NOT_AVAILABLE) is decoded by mijpeg_decode_batch_device, failing that stream by stream on the host; any other
 * error ends the run with its code (mijpeg_batch_pipeline_last_error).  stats: chunks of the last run, how many fell back, host
 * milliseconds of every submit.  schedule: the chunk boundaries run would use.  decoder: object k (diagnostics: mijpeg_get_info,
 * mijpeg_last_timing of its last chunk). */
typedef struct mijpeg_batch_pipeline mijpeg_batch_pipeline;
int mijpeg_batch_pipeline_create(mijpeg_batch_pipeline **out, int device, int chunk_frames, int decoder_objects, int ramp);
void mijpeg_batch_pipeline_destroy(mijpeg_batch_pipeline *p);
int mijpeg_batch_pipeline_run(mijpeg_batch_pipeline *p, const uint8_t *const *streams, const size_t *sizes, int n, void *dst_device,
                              int64_t frame_stride, int64_t row_stride, void *download_host);
int mijpeg_batch_pipeline_schedule(int n, int chunk_frames, int ramp, int32_t *first, int32_t *end, int capacity);
int mijpeg_batch_pipeline_stats(mijpeg_batch_pipeline *p, int32_t *chunks, int32_t *fallbacks, float *submit_ms, int capacity);
int mijpeg_batch_pipeline_last_error(mijpeg_batch_pipeline *p, const char **message);
/* on = 1 / 0: launch the reconstructions speculatively (MIJPEG_FLAG_SPECULATIVE above; off by default), on < 0: leave as is.
 * Returns how many chunks of the last run were reconstructed again by their validation. */
int mijpeg_batch_pipeline_speculation(mijpeg_batch_pipeline *p, int on);
mijpeg_decoder *mijpeg_batch_pipeline_decoder(mijpeg_batch_pipeline *p, int k);
/* Capacity planning / diagnostics: the HOST half of mijpeg_submit_batch_device alone -- header parse, restart marker search
 * and the copy of the entropy coded data without its byte stuffing into the staging area, one stream per pool worker -- with
 * no device involved (works on host-only objects).  This is what a rank's cores do per chunk of a batch; `bench.py
 * --emulate-world N` runs it in neighbour processes to load the host the way the other ranks of a node would. */
int mijpeg_prepare_batch_host(mijpeg_decoder *d, const uint8_t *const *streams, const size_t *sizes, int n);
/* Opt-in: search the restart markers and strip the byte stuffing on the DEVICE (on = 1; off, 0, by default; anything else is
 * MIJPEG_ERR_INVALID_PARAMETER).  With it on, mijpeg_decode_coefficients_device, mijpeg_decode_batch_device,
 * mijpeg_submit_batch_device / mijpeg_finish_batch_device and mijpeg_prepare_batch_host (its host half) parse the headers only,
 * copy the raw entropy coded segment into the staging slot with one memcpy, and two kernel passes in front of the Huffman
 * launch write the copy without stuffing and markers and the interval tables where that launch reads them.  Every image of the
 * call must qualify -- plain (no JPEG XT, no DNL) 8-bit Huffman sequential, one scan over all components, FF D9 as the last two
 * bytes of the stream -- else the whole call takes the ordinary route.  Streams with restart markers (DRI > 0) and without may
 * share a batch.  A stream without restart markers is searched with one expected interval (no marker at all), a small fit step puts
 * the size of its copy where the device walk reads it, and the walk finds its virtual restart intervals as it does with the
 * option off; in the batch calls it must be large enough for a walk (256 MCUs, 4096 bytes) as it must be there, and
 * mijpeg_decode_coefficients_device, the single-image call, keeps the host's search for such a stream.  The search
 * must come out plain as well: no fill byte, exactly the markers the MCU count asks for, in sequence, and the segment ending at the
 * FF of that closing EOI.  Where it does not, the synchronous calls run the ordinary route inside the same call (the caller sees
 * what it would have seen with the option off); mijpeg_finish_batch_device, which no longer has the bytes, answers
 * MIJPEG_ERR_NOT_AVAILABLE as it does for damaged streams.  The ragged calls (mijpeg_decode_ragged_device / ...16) honour the option
 * member by member: a member whose parse could leave the search to the device is searched inside its layout group's one launch,
 * beside members that were searched on the host (bytes behind EOI, the 12-bit groups); a small stream without restart markers is
 * searched as its one interval; a member whose search or decode is not good takes the single-image route, with its reason in
 * mijpeg_ragged_route, and the other members keep their result.  Multi-scan / progressive / JPEG XT / DNL / 12-bit streams, the
 * single-image route of the ragged calls, class JPEG and the command line ignore the option.  stats: images of this object that
 * went through the device search, and images of calls that took the ordinary route although the option was on -- in a ragged
 * call, every member the device did not search (either pointer may be NULL). */
int mijpeg_set_device_markers(mijpeg_decoder *d, int on);
int mijpeg_device_markers_stats(mijpeg_decoder *d, int64_t *searched, int64_t *declined);
/* ... for every decoder object of a pipeline (on < 0: leave as is).  Returns the setting. */
int mijpeg_batch_pipeline_device_markers(mijpeg_batch_pipeline *p, int on);
/* Diagnostics: where the last mijpeg_prepare_batch_host / batch submit with the option on put the raw segment of image i (host
 * memory, valid until the object's next call) and its size in *bytes; NULL when that call took the ordinary route. */
const uint8_t *mijpeg_device_markers_staging(mijpeg_decoder *d, int image, size_t *bytes);
/* Wait for everything the object has enqueued on its stream (e.g. a reconstruction launched with sync = 0). */
int mijpeg_synchronize(mijpeg_decoder *d);
/* ... or let a stream of the CLIENT's wait for it instead of the host: everything the object has enqueued so far (uploads, entropy
 * kernels, a reconstruction launched with sync = 0) happens before whatever the client enqueues on `client_stream` (a hipStream_t;
 * NULL = the null stream) after this call.  The host does not block.  What config 4's other half uses: the download of a chunk's
 * pixels waits for that chunk's reconstruction kernel and for nothing else, so PCIe carries pixels down while the next chunks'
 * bytes go up (libjpeg_amd/batch.py, `download_to`). */
int mijpeg_stream_wait(mijpeg_decoder *d, void *client_stream);
int mijpeg_reconstruct_batch_device(mijpeg_decoder *d, void *dst_device, int64_t frame_stride, int64_t row_stride, uint32_t flags,
                                    int sync);

/* Current frame information (after mijpeg_decode_coefficients it includes fast_arith). */
int mijpeg_get_info(mijpeg_decoder *d, mijpeg_info *info);

/* JPEG XT parameters of the loaded stream (MIJPEG_ERR_OBJECT_DOESNT_EXIST if it is a plain JPEG). */
int mijpeg_get_xt_params(mijpeg_decoder *d, mijpeg_xt_params *xt);

/* Host view of a decoded component plane: blocks_h x blocks_w x 64 int16 (NULL for a frame with info.coef_wide). */
const int16_t *mijpeg_coefficients(mijpeg_decoder *d, int component);
/* ... of a frame with info.coef_wide: blocks_h x blocks_w x 64 int32 (NULL for every other frame). */
const int32_t *mijpeg_coefficients32(mijpeg_decoder *d, int component);

/* Device pointer of the uploaded frame (coef_count int16) or NULL. */
const int16_t *mijpeg_device_coefficients(mijpeg_decoder *d);

/* Reconstruct the whole frame on the GPU into DEVICE memory: interleaved 8-bit samples,
 * `components * sample_bytes` bytes per pixel, `row_stride` bytes per line.  Asynchronous on the decoder's stream
 * unless `sync` is non-zero. */
int mijpeg_reconstruct_device(mijpeg_decoder *d, void *dst_device, int64_t row_stride, uint32_t flags,
                              int sync);

/* Reconstruct the whole frame into HOST memory (interleaved samples, `row_stride` bytes per line) with the
 * device-to-host copy landing directly in `dst_host`: no staging copy when the memory is pinned
 * (mijpeg_host_alloc, hipHostMalloc, hipHostRegister); pageable memory works too, only slower. Synchronous. */
int mijpeg_reconstruct_host(mijpeg_decoder *d, void *dst_host, int64_t row_stride, uint32_t flags);

/* Pinned host memory for frame buffers (hipHostMalloc / hipHostFree). */
void *mijpeg_host_alloc(size_t bytes);
void mijpeg_host_free(void *p);

/* Reconstruct a rectangle into HOST memory described like the reference's ImageBitMap
 * (interface/imagebitmap.hpp): for component c, dst[c] is the address of canvas pixel (0,0),
 * bytes_per_pixel[c] / bytes_per_row[c] the strides.  Rectangle and component range are inclusive,
 * as in JPGTAG_DECODER_MINX..MAXY / MINCOMPONENT..MAXCOMPONENT (codestream/rectanglerequest.cpp:92-152).
 * With MIJPEG_FLAG_NO_UPSAMPLING (min_comp == max_comp required) the component is delivered at its own resolution
 * without colour transformation; the rectangle is still given on the canvas and shrinks by the subsampling factors
 * (control/bitmapctrl.cpp:273-294), dst[c] addresses the component's sample (0,0).  JPEG XT frames return
 * MIJPEG_ERR_OPERATION_UNIMPLEMENTED for it: the reference merges the one requested component with whatever its scratch
 * buffers hold for the residuals of the OTHER two -- heap memory it never initialised during the first component's pass
 * (control/blockbitmaprequester.cpp:379-388, 1054-1061; `MALLOC_PERTURB_=165 jpeg -U xt.jpg out.pgx` writes other planes
 * than `jpeg -U xt.jpg out.pgx`), so there is no output to equal.
 * With MIJPEG_FLAG_DEVICE_OUTPUT the bitmaps live in device memory of the decoder's GPU and the pixels never leave
 * HBM ("device-side output"); the call returns when they are written. */
int mijpeg_reconstruct_rect(mijpeg_decoder *d, int32_t min_x, int32_t min_y, int32_t max_x, int32_t max_y,
                            int32_t min_comp, int32_t max_comp, uint32_t flags,
                            void *const dst[MIJPEG_MAX_COMPONENTS],
                            const int32_t bytes_per_pixel[MIJPEG_MAX_COMPONENTS],
                            const int32_t bytes_per_row[MIJPEG_MAX_COMPONENTS]);

/* JPEG::DisplayRectangle AS THE REFERENCE RUNS IT: one call of a sequence.  mijpeg_reconstruct_rect above answers every
 * request from the plain picture; the reference does not -- BlockBitmapRequester::ReconstructRegion
 * (control/blockbitmaprequester.cpp:1013-1272) walks row cursors that never rewind and upsampler line buffers
 * (upsampling/upsamplerbase.cpp:138-327) that persist between calls, so a request shows what the calls before it left:
 * on the upsampling path every call moves the cursor of every unsubsampled component, requested or not (:1214-1223 -- the
 * reference's own PGX loop, cmd/reconstruct.cpp:272-303, therefore writes planes of zeros for the later unsubsampled
 * components of a two- or four-component frame with mixed sampling); components outside the requested range enter the colour
 * transformation as zeros; the colour transformer of the first request stays (colortrafo/colortransformerfactory.cpp:220-221);
 * rectangles whose corner is off the 8-pixel grid see subsampled components displaced (upsampling/upsampler.cpp:85-86 against
 * colortrafo/ycbcrtrafo.cpp:683-686); stripes that are skipped or repeated read the rows the cursors stand at.  This entry
 * point keeps that state per decoder object (reset by every decode) and reproduces all of it; top-down requests of whole
 * component sets -- every sane client -- are recognised as the plain picture and served from the cached frame.
 * bitmaps[c] describes what the bitmap hook returned for component c (requested components only are read): address of canvas
 * pixel (0,0), strides in bytes, BIO_WIDTH / BIO_HEIGHT (the height bounds the block rows that are reconstructed, :1229-1244;
 * blocks that start outside the extent are not written, interface/imagebitmap.cpp:58-129).  data == NULL: nothing is
 * written for that component but the state advances.  flags: MIJPEG_FLAG_NO_UPSAMPLING, _NO_COLOR_TRANSFORM, _DEVICE_OUTPUT.
 * JPEG XT frames: the residual image has cursors and upsamplers of its own beside the legacy image's (:228-232, 356-372,
 * 1118-1146, 1197-1222) and both follow every request -- reproduced for what the reference's command line asks for (all three
 * components, upsampling and colour transformation on) with any order and size of rectangles; a request that walks the
 * residual cursor of a component without upsampler behind its last row makes the reference dereference a NULL row
 * (:1057-1058, :1201-1202): MIJPEG_ERR_OBJECT_DOESNT_EXIST here.  Component subsets of an XT frame (they merge with what a
 * scratch buffer holds from the block before) are served as the plain picture, XT requests without colour transformation as
 * the plain picture with the identity in place of the standard YCbCr L transformation (what the reference's transformer
 * does, mijpeg_xt_params.ltrafo_standard), XT requests without upsampling fail (see mijpeg_reconstruct_rect).  Not modelled either: rectangles narrower than the frame that move sideways between calls read line-buffer
 * memory the reference never initialised. */
typedef struct mijpeg_bitmap {
  void *data;
  int32_t bytes_per_pixel, bytes_per_row;
  uint32_t width, height;
} mijpeg_bitmap;
int mijpeg_display_rect(mijpeg_decoder *d, int32_t min_x, int32_t min_y, int32_t max_x, int32_t max_y, int32_t min_comp, int32_t max_comp,
                        uint32_t flags, const mijpeg_bitmap bitmaps[MIJPEG_MAX_COMPONENTS]);
/* Diagnostics, no device needed (mijpeg_read_header is enough): advance the request state exactly like mijpeg_display_rect
 * would and report the plan instead of pixels -- out[0..7] = nothing shown, plain picture, YCbCr transformer, view component,
 * region min_x, min_y, max_x, max_y; then per component: cursor after the call, first / last block row with a row map, upsampler
 * window start / end (lines), number of mapped block rows that are zeros. */
int mijpeg_display_plan(mijpeg_decoder *d, int32_t min_x, int32_t min_y, int32_t max_x, int32_t max_y, int32_t min_comp, int32_t max_comp,
                        uint32_t flags, const uint32_t bm_height[MIJPEG_MAX_COMPONENTS], int32_t out[8 + 6 * MIJPEG_MAX_COMPONENTS]);
/* Diagnostics: coefficient row the cursor of `component` stands at after the mijpeg_display_rect calls so far (JPEG XT:
 * 4 + c = component c of the residual image, which has cursors of its own, control/blockbitmaprequester.cpp:228-232). */
int mijpeg_display_cursor(mijpeg_decoder *d, int component);

/* The scans of the decoded frame in codestream order: first_byte[k] = offset (in the input of mijpeg_set_input) of the first
 * entropy coded byte of scan k, i.e. where the reference stands when JPEG::Read returns with JPGFLAG_DECODER_STOP_SCAN
 * (interface/jpeg.cpp:310-353), end_byte[k] = offset of the marker that follows the scan's data.  JPEG XT scans that live in
 * boxes come last: first_byte = the marker behind the codestream's last scan (where the reference's input stands while it
 * parses them from memory), end_byte = 0 -- the legacy frame's refinement scans, the residual codestream's scans, then the
 * alpha channel's codestreams in the same order (Image::ParseAlphaChannel, codestream/image.cpp:1337-1404).  A frame that
 * was decoded by the sequential walk (a height from a DNL marker, the residual scan types of part 8, damaged streams) is
 * listed by the scans that walk met.  Either array may be NULL.  Returns the number of scans (also when capacity is
 * smaller) or a negative error. */
int mijpeg_scan_offsets(mijpeg_decoder *d, uint64_t *first_byte, uint64_t *end_byte, int capacity);
/* ... and their MCU grids, same order: mcus_y[k] rows of mcus_x[k] MCUs (a single-component scan walks its component's own blocks,
 * codestream/sequentialscan.cpp:396-397).  What JPEG::Read with JPGFLAG_DECODER_STOP_ROW / _MCU counts its returns by: one at the
 * start of every MCU row, one behind every MCU of a row but the last (interface/jpeg.cpp:326-350).  (The scan that brings a DNL
 * marker: as many rows as the reference starts to find it.)  Returns the number of scans. */
int mijpeg_scan_grids(mijpeg_decoder *d, int32_t *mcus_x, int32_t *mcus_y, int capacity);

/* JPEG XT alpha channel (the reference: Image::ParseAlphaChannel, codestream/image.cpp:1337-1404; JPEG::GetInformation's
 * JPGTAG_ALPHA_MODE / JPGTAG_ALPHA_TAGLIST / JPGTAG_ALPHA_MATTE, interface/jpeg.cpp:870-945; JPEG::DisplayRectangle with
 * JPGTAG_BIH_ALPHAHOOK and JPGTAG_DECODER_INCLUDE_ALPHA, codestream/image.cpp:1087-1123, cmd/reconstruct.cpp:154-217, 268-319).
 * The alpha channel is an image of its own -- one component, its own tables, optionally its own residual codestream and hidden
 * refinement scans, its own merging specification -- that the reference decodes inside JPEG::Read behind the picture's
 * codestreams: mijpeg_decode_coefficients (host or device) decodes it as well, and what is wrong with it fails that call like it
 * fails JPEG::Read.  The decoder does not composite: the plane is handed out beside the picture.
 * mijpeg_alpha_channel: the decoder object of the alpha image, owned by `d` and valid until `d` decodes again or is destroyed; every
 * call that works on a decoded object works on it (mijpeg_get_info, mijpeg_get_xt_params, mijpeg_reconstruct_rect,
 * mijpeg_display_rect with cursors of its own, mijpeg_coefficients).  NULL (and MIJPEG_ERR_OBJECT_DOESNT_EXIST on `d`) when the
 * decoded file has none -- no complete ALFA box, or a legacy codestream that never came to its EOI.
 * mijpeg_alpha_info: *mode = the compositing method of the AMUL box (0 opaque, 1 regular, 2 premultiplied, 3 matte removal;
 * -1: the alpha merging specification has no such box and JPEG::GetInformation reports no alpha channel), matte = its colour. */
mijpeg_decoder *mijpeg_alpha_channel(mijpeg_decoder *d);
/* 1 when mijpeg_alpha_channel(d) would hand out a decoder, 0 otherwise; never records an error (JPEG::GetInformation asks on every file,
 * interface/jpeg.cpp:919-951, and must not leave "no alpha channel" behind as the object's last error). */
int mijpeg_has_alpha(mijpeg_decoder *d);
int mijpeg_alpha_info(mijpeg_decoder *d, int32_t *mode, int32_t matte[3]);

/* Error of the last failing call on this object (JPEG::LastError). Returns the code, 0 if none. */
int mijpeg_last_error(mijpeg_decoder *d, const char **message);

/* JPEG::LastWarning (interface/jpeg.cpp:970-979): 0, or the code of what the reference warns about at the loaded stream --
 * MIJPEG_ERR_PHASE_ERROR: the LCHK checksum box of a JPEG XT file does not fit its legacy codestream (interface/jpeg.cpp:222-238;
 * computed when first asked for), MIJPEG_ERR_MALFORMED_STREAM: a damaged codestream that was decoded with resynchronisation. */
int mijpeg_last_warning(mijpeg_decoder *d, const char **message);

/* Diagnostics: the entropy coded data of the first scan of the parsed stream (mijpeg_read_header is not enough:
 * mijpeg_decode_coefficients or a device decode must have parsed it) the way the device decoder receives it -- without the
 * byte stuffing and without the markers, restart interval k at begin[k] (n_begin entries are filled at most), copied in
 * pieces of at most piece_bytes source bytes like the parallel gather does (piece_bytes = 1: the stream is parsed again and the
 * marker search writes the copy while it walks the segment, as a batch's workers do; capacity >= stream size + 64 then).  Returns the number of bytes (also when dst is
 * NULL or too small: nothing is copied then), or a negative error code.  *n_intervals (may be NULL): restart intervals. */
int64_t mijpeg_unstuffed_scan(mijpeg_decoder *d, uint8_t *dst, size_t capacity, uint32_t *begin, size_t n_begin, size_t piece_bytes,
                              int32_t *n_intervals);

/* Diagnostics, the device twin of mijpeg_unstuffed_scan: the segment-level primitive behind mijpeg_set_device_markers on `size`
 * raw bytes as they lie in the file from the first entropy coded byte on (terminator and whatever follows included), for a frame
 * whose header asks for `expect` restart intervals.  A byte pair is only ever interpreted from its FF.  *term: position of the
 * first FF whose follower is none of 00, FF, D0..D7 -- nothing at or behind it is interpreted, kept or counted -- or `size` with
 * flag 8 (NO_END) when there is none (a lone FF as last byte included; size = 0 is legal).  In front of it FF 00 keeps the FF and
 * drops the 00, FF Dn drops both and is restart marker k = 0, 1, ..., FF FF sets flag 1 (FILL).  Flag 2 (SEQUENCE): a marker's
 * code is not 0xD0 + (k & 7); flag 4 (COUNT): markers + 1 != expect.  With *flags == 0: dst holds the kept bytes back to back and
 * zeros from there to `capacity` (>= size), begin[0] = 0, begin[k + 1] = end[k] = kept bytes in front of marker k,
 * end[expect - 1] = the return value (`expect` entries each; either may be NULL).  With a flag set only *flags and *term are
 * defined.  The call uploads, runs the kernels, checks that nothing outside the device copies of dst / begin / end was written
 * (MIJPEG_ERR_PHASE_ERROR otherwise) and downloads.  Returns the number of kept bytes or a negative error code; segments of
 * 2^28 bytes or more are MIJPEG_ERR_NOT_AVAILABLE. */
int64_t mijpeg_device_marker_search(mijpeg_decoder *d, const uint8_t *segment, size_t size, int32_t expect, uint8_t *dst, size_t capacity,
                                    uint32_t *begin, uint32_t *end, uint32_t *term, uint32_t *flags);

/* Diagnostics: number of scans without restart markers that the host decoder decoded in parallel (self-synchronising
 * speculative decoding) since the library was loaded; *pieces (may be NULL) = ranges they were stitched from. */
int64_t mijpeg_speculative_scans(int64_t *pieces);

/* Diagnostics: rounds the on-device self-synchronising walk needed in the last device entropy decode of streams
 * without restart markers (0: no such walk took place, e.g. the streams had restart markers). */
int mijpeg_device_walk_rounds(mijpeg_decoder *d);

/* Seconds spent in the phases of the last decode (huffman, h2d, kernel, d2h) -- diagnostics. */
int mijpeg_last_timing(mijpeg_decoder *d, double out_seconds[4]);

/* ---- ragged batches: n streams of ANY shapes in one device pass ---------------------------------------------------
 * A folder of photographs instead of a film: the streams differ in width, height and sampling.  mijpeg_decode_ragged_device
 * parses them in parallel and sorts the ones the batch kernels cover -- 8-bit Huffman sequential, one interleaved scan (or one
 * component), intact, plain JPEG, in the layouts 4:2:0, 4:2:2, 4:4:4 and grey -- into one LAYOUT GROUP per layout.  Each group
 * is entropy-decoded by ONE launch of the Huffman kernel (streams without restart markers: the device walk in front of it; too
 * small for the walk: one interval, one lane) into coefficient stores packed back to back in the object's store, and
 * mijpeg_reconstruct_ragged_device turns each group into pixels with one launch of the ragged flavour of its fused kernel per
 * arithmetic flavour the range checks select, image i at dst_device[i] with row_strides[i] bytes per line.
 * Every other stream -- progressive, 12 bit, other layouts, CMYK, DNL, JPEG XT, damaged -- takes the single-image route inside
 * the same calls (a decoder object of its own that this one owns; its bytes are copied), so the caller gets all n pictures.
 * status[i]: MIJPEG_OK or the JPGERR_* code of stream i; a stream in error does not stop the others, and the calls return
 * MIJPEG_OK when they could work through the list.  min_intervals is handed to the single-image route (0: its default).
 * What sends a stream to the single-image route is a property of that stream alone, with one exception: where a whole group's
 * launch is refused -- its device walk does not settle within its rounds, or the group outgrows the launch's 32-bit offsets --
 * every member of that group takes the single-image route (same pictures, counted as fallbacks).
 * mijpeg_ragged_info: geometry and range check of image i after the decode (the caller sizes dst_device[i] from it);
 * mijpeg_ragged_warning: the warning the single-image route left for image i, or NULL;
 * mijpeg_ragged_route: 0 = image i was decoded by its group's launch, 1 = by the single-image route, *why says for what reason.
 * Any other decode call on the object ends the ragged batch: its coefficient stores are reused. */
int mijpeg_decode_ragged_device(mijpeg_decoder *d, const uint8_t *const *streams, const size_t *sizes, int n, int min_intervals, int32_t *status);
int mijpeg_ragged_info(mijpeg_decoder *d, int i, mijpeg_info *info);
int mijpeg_ragged_warning(mijpeg_decoder *d, int i, const char **message);
int mijpeg_ragged_route(mijpeg_decoder *d, int i, const char **why);
/* dst_device and row_strides hold one entry per stream of the decode call; dst_device[i] == NULL (and images in error) are
 * skipped.  An image whose own reconstruction fails (the single-image route, or a group image reconstructed by a launch of its
 * own) does not stop the others: the call then returns the first such code, and mijpeg_last_error names the image.  A group
 * launch that fails is the device's failure and ends the call. */
int mijpeg_reconstruct_ragged_device(mijpeg_decoder *d, void *const *dst_device, const int64_t *row_strides, uint32_t flags, int sync);
/* What the last mijpeg_decode_ragged_device + mijpeg_reconstruct_ragged_device of the object did. */
typedef struct mijpeg_ragged_stats {
  int32_t images;            /* streams of the call                                                          */
  int32_t ragged;            /* ... entropy-decoded by a layout group's launch                                */
  int32_t fallbacks;         /* ... that took the single-image route (those in error included)                */
  int32_t errors;            /* ... whose status is an error                                                  */
  int32_t entropy_launches;  /* launches of the Huffman kernel for the groups                                  */
  int32_t walk_launches;     /* launches of the walk kernel (its rounds and the emitting pass), all groups     */
  int32_t recon_launches;    /* ragged reconstruction launches (one per group and arithmetic flavour)          */
  int32_t recon_single;      /* group images reconstructed by a launch of their own (no ragged flavour fits)   */
} mijpeg_ragged_stats;
int mijpeg_ragged_get_stats(mijpeg_decoder *d, mijpeg_ragged_stats *out);
/* The planner behind the two calls, on its own (no device, no decoder object): n frame descriptions (as mijpeg_read_header or
 * mijpeg_frame_layout fill them) -> group[i] (MIJPEG_RAGGED_420 ... _GREY, or -1: the single-image route) and, for group members,
 * frames[i]: the frame's entry of the descriptor table.  Members of a group follow each other in list order; frame i occupies
 * the workgroups [first_workgroup, first_workgroup + tiles_x * tiles_y) of its group's launch -- tiles of 128 x 128 pixels, row
 * by row, no padding -- and coef_count coefficients from coef_base in the store, whose size *coef_total receives.
 * group_workgroups[g]: the grid of group g.  (Where the range checks split a group into arithmetic flavours, each launch numbers
 * its own frames the same way.)  MIJPEG_ERR_INVALID_PARAMETER for n < 1 or NULL lists. */
#define MIJPEG_RAGGED_420 0
#define MIJPEG_RAGGED_422 1
#define MIJPEG_RAGGED_444 2
#define MIJPEG_RAGGED_GREY 3
#define MIJPEG_RAGGED_GROUPS 4
typedef struct mijpeg_ragged_frame {
  int64_t coef_base;               /* int16 index of the frame's coefficient store                       */
  int64_t off_y, off_cb, off_cr;   /* its planes inside that store                                        */
  int32_t first_workgroup;
  int32_t tiles_x, tiles_y;
  int32_t width, height;
  int32_t bw_y, bh_y, bw_c, bh_c;  /* plane sizes in blocks (MCU padded)                                  */
  int32_t cw, ch;                  /* valid chroma samples                                                */
  int32_t reserved;
} mijpeg_ragged_frame;
int mijpeg_ragged_plan(const mijpeg_info *infos, int n, int32_t *group, mijpeg_ragged_frame *frames, int32_t group_workgroups[MIJPEG_RAGGED_GROUPS],
                       int64_t *coef_total);
/* Lists that mix 8-bit and 12-bit pictures (the decoder's counterpart of mijpeg_encode_ragged_device16).  The calls
 * above keep 12-bit frames out of the layout groups; these give a plain 12-bit Huffman sequential frame (SOF1, P = 12, one
 * interleaved scan or one component) the 12-bit group of its layout -- 4:2:0, 4:2:2, 4:4:4 or grey 1 x 1 -- and are the calls
 * above on everything else.  mijpeg_ragged_plan16: groups 0..3 as ever, 4..7 for the 12-bit frames; geometry, workgroup ranges
 * and stores as above, the stores packed back to back in list order across both precisions (int16 coefficients either way).
 * mijpeg_decode_ragged_device16: one Huffman launch per layout and precision present, at most eight.
 * mijpeg_reconstruct_ragged_device serves whichever decode call filled the object: the images of a 12-bit group that agree on
 * kernel and colour-stage flavour (mijpeg_kernel_name: "/narrow" or not) share a launch -- at most two per three-component group,
 * one for grey -- and an image beyond the 12-bit kernels' gates, or without the YCbCr transformation, is reconstructed by a
 * launch of its own (recon_single).  A 12-bit picture's destination holds 16-bit samples: row_strides[i] is in bytes, as
 * mijpeg_reconstruct_device takes it for such a frame.  The other mijpeg_ragged_* calls read either call's batch. */
#define MIJPEG_RAGGED_420_12 4
#define MIJPEG_RAGGED_422_12 5
#define MIJPEG_RAGGED_444_12 6
#define MIJPEG_RAGGED_GREY_12 7
#define MIJPEG_RAGGED_GROUPS16 8
int mijpeg_ragged_plan16(const mijpeg_info *infos, int n, int32_t *group, mijpeg_ragged_frame *frames, int32_t group_workgroups[MIJPEG_RAGGED_GROUPS16],
                         int64_t *coef_total);
int mijpeg_decode_ragged_device16(mijpeg_decoder *d, const uint8_t *const *streams, const size_t *sizes, int n, int min_intervals, int32_t *status);

/* ---- planar output: component planes (C, H, W) instead of interleaved pixels -------------------------
 * The planar twins of mijpeg_reconstruct_device, mijpeg_reconstruct_batch_device and mijpeg_reconstruct_ragged_device: same
 * objects, same streams, same `sync`, same error codes (and the ragged call's per-image error rule); every picture those calls
 * reconstruct comes back planar.  Component c of a picture goes to its own plane: sample (x, y) at plane + y * row_stride +
 * x * sample_bytes (1, or 2 for 12-bit and JPEG XT frames: native-endian 16-bit samples), row_stride >= width * sample_bytes,
 * any plane address, any stride.  Which kernel reconstructs a picture is decided as for the interleaved calls; an 8-bit
 * three-component picture whose kernel is the fused 4:2:0 (packed, fast or safe), 4:2:2 (packed or wide) or 4:4:4 one is
 * written to its planes by the planar flavour of that kernel's ragged launch -- one launch per kernel and flavour for all such
 * pictures of the call, the pixel bytes cross HBM once -- a one-component picture is its own plane, and everything else (12 bit,
 * JPEG XT, 4:4:0, 4:1:1, CMYK, no colour transformation, frames beyond the fused gates, MIJPEG_FLAG_FORCE_GENERIC) is
 * reconstructed interleaved into a buffer of the object and taken apart by a second kernel.
 * flags: MIJPEG_FLAG_FORCE_SAFE, MIJPEG_FLAG_FORCE_GENERIC (forces the two-pass route), MIJPEG_FLAG_NO_COLOR_TRANSFORM; others are
 * ignored.  MIJPEG_ERR_INVALID_PARAMETER -- before anything is launched -- for NULL arguments, a row_stride below a line of
 * samples, or a NULL plane of a component the picture has.
 * planes[c]: first sample of component c; row_stride: bytes per plane line. */
int mijpeg_reconstruct_planar_device(mijpeg_decoder *d, void *const planes[MIJPEG_MAX_COMPONENTS], int64_t row_stride, uint32_t flags, int sync);
/* a decoded uniform batch as (N, C, H, W): frame f, component c at dst_device + f * frame_stride + c * plane_stride (bytes;
 * plane_stride >= height * row_stride, frame_stride >= components * plane_stride).  A submitted batch is waited for
 * (MIJPEG_FLAG_SPECULATIVE has no planar form). */
int mijpeg_reconstruct_batch_planar_device(mijpeg_decoder *d, void *dst_device, int64_t frame_stride, int64_t plane_stride, int64_t row_stride,
                                           uint32_t flags, int sync);
/* after mijpeg_decode_ragged_device / ...16: image i, component c at planes[i * MIJPEG_MAX_COMPONENTS + c], its lines
 * row_strides[i] bytes apart; planes[i * MIJPEG_MAX_COMPONENTS] == NULL (and images in error) are skipped. */
int mijpeg_reconstruct_ragged_planar_device(mijpeg_decoder *d, void *const *planes, const int64_t *row_strides, uint32_t flags, int sync);
/* What the object's last planar call did: pictures it wrote; of those, in one pass (a fused planar launch, or a one-component
 * picture's own kernel) and in two; launches of the fused planar kernels, and of the kernel that takes interleaved pictures apart. */
typedef struct mijpeg_planar_stats {
  int32_t images, fused, two_pass, fused_launches, two_pass_launches;
} mijpeg_planar_stats;
int mijpeg_planar_stats_get(mijpeg_decoder *d, mijpeg_planar_stats *out);
/* The second pass of the two-pass route on its own, on the object's stream (no wait): an interleaved picture in device memory
 * (components x sample_bytes per pixel, src_row_stride bytes per line) -> its planes.  components 1..4, sample_bytes 1 or 2.
 * (tools/planar_bench.py times it behind the interleaved launch; a client that holds interleaved pictures may use it as well.) */
int mijpeg_deinterleave_device(mijpeg_decoder *d, const void *src_device, int64_t src_row_stride, int32_t width, int32_t height, int32_t components,
                               int32_t sample_bytes, void *const planes[MIJPEG_MAX_COMPONENTS], int64_t row_stride);

/* ---- crop windows of a ragged batch: only their tiles are reconstructed --------------------------------
 * What a data loader asks of a folder of photographs: a crop of every picture, a different one per picture.  The calls follow
 * mijpeg_decode_ragged_device / ...16 exactly as mijpeg_reconstruct_ragged_device and its planar twin do -- same object, same
 * `flags`, same `sync`, same per-image error rule, the coefficient stores valid until the next decode call, so one decode serves any
 * number of crop calls -- and write, per picture, the rectangle rects[i] of what those calls write, byte for byte (the stateless rule
 * of mijpeg_reconstruct_rect: every request is answered from the plain picture).
 * rects[i] is on picture i's canvas, inclusive (JPGTAG_DECODER_MINX .. MAXY).  max_x / max_y beyond the picture are clipped to its
 * last column / line (INT32_MAX: "to the edge").  MIJPEG_ERR_INVALID_PARAMETER for the call, BEFORE anything is launched or written
 * (and with the statistics of the last call left alone): NULL arguments, a min_x / min_y below 0 or beyond the picture, min > max
 * after clipping, a row_strides[i] below one line of the crop, a NULL plane of a component the picture has.
 * Pixel (min_x, min_y) lands at dst_device[i] (sample c of it at planes[i * MIJPEG_MAX_COMPONENTS + c]), lines row_strides[i] bytes
 * apart; any base address, any stride; nothing but the crop's own bytes is written -- not the padding of a line, not a byte in
 * front of or behind the buffer.  dst_device[i] == NULL (planes[i * MIJPEG_MAX_COMPONENTS] == NULL) and pictures in error are skipped.
 * An 8-bit group picture whose kernel has a ragged flavour (planar: a planar twin; grey is its own plane) is written by the WINDOW
 * flavour of that kernel: the launch holds only the 128 x 128 tiles the window touches and stores only the window's pixels.  Every
 * other picture -- 12-bit groups, group pictures reconstructed by a launch of their own, the single-image route (progressive, JPEG
 * XT, CMYK, 4:4:0, 4:1:1, DNL, ...), a crop whose offsets do not fit 32 bits -- is reconstructed in full into a buffer of the object
 * and its rectangle copied out on the object's stream (`copied`): the caller gets all n crops whatever the stream is. */
typedef struct mijpeg_rect { int32_t min_x, min_y, max_x, max_y; } mijpeg_rect;   /* inclusive, as JPGTAG_DECODER_MINX..MAXY */
int mijpeg_reconstruct_ragged_rect_device(mijpeg_decoder *d, const mijpeg_rect *rects, void *const *dst_device, const int64_t *row_strides,
                                          uint32_t flags, int sync);
int mijpeg_reconstruct_ragged_rect_planar_device(mijpeg_decoder *d, const mijpeg_rect *rects, void *const *planes, const int64_t *row_strides,
                                                 uint32_t flags, int sync);
/* What the object's last crop call did. */
typedef struct mijpeg_ragged_rect_stats {
  int32_t images, fused, copied;        /* pictures written; by a window launch; by full reconstruction + rectangle copy */
  int32_t launches;                     /* window launches of the fused kernels                                         */
  int64_t workgroups, workgroups_full;  /* tiles those launches ran; tiles the same pictures have in all                 */
} mijpeg_ragged_rect_stats;
int mijpeg_ragged_rect_stats_get(mijpeg_decoder *d, mijpeg_ragged_rect_stats *out);
/* The planner on its own, no device: per picture the clipped window in tiles of 128 x 128 -- first tile column and row, tiles per
 * window row, window rows; picture i runs tiles_x[i] * tiles_y[i] workgroups.  Only width and height of infos[i] are read.
 * MIJPEG_ERR_INVALID_PARAMETER for NULL lists, n < 1 or a rectangle the calls above refuse (nothing is then defined). */
int mijpeg_ragged_rect_plan(const mijpeg_info *infos, const mijpeg_rect *rects, int n, int32_t *tile_x0, int32_t *tile_y0, int32_t *tiles_x,
                            int32_t *tiles_y);

/* ---- crops of a ragged batch resized into ONE batch tensor, one resample launch for the list ------------
 * What a loader does between the decoder and a training batch: a window of a different size from every picture (RandomResizedCrop,
 * resize + centre crop), all of them out_width x out_height afterwards, in the slots of one (N, C, H, W) or (N, H, W, C) tensor.  The
 * call follows mijpeg_decode_ragged_device / ...16 exactly as the crop calls above do (same object, the coefficient stores stay valid,
 * same `flags` masking, same `sync`).  Stage 1 is the crop call's own body with destinations in an arena of the object -- so window
 * launches, the copy route and child objects all deliver --, stage 2 ONE launch of the resample kernel on the object's stream, for
 * any n.
 * The filter is defined in integers, so that host, kernel and a model in numpy cannot disagree: a separable triangle filter whose
 * support grows with the reduction (Pillow's BILINEAR, antialias=True elsewhere), horizontally first, rounded to 8 bits, then
 * vertically.  One axis, n source samples (the clipped crop's extent), m output samples, output o, source i:
 *   S = 2 max(n, m),  D(i) = |(2i + 1) m - (2o + 1) n|,  w(i) = max(0, S - D(i));  the taps of o: the run of i in [0, n) with w(i) > 0;
 *   W = sum w(i),  k(i) = floor((w(i) 2^14 + floor(W / 2)) / W);  2^14 - sum k(i) is added to k at the tap with the largest w (the
 *   lowest such i);  out = min(255, (sum k(i) p(i) + 2^13) >> 14).            m == n is the identity: the crop call's bytes.
 * rects[i]: as the crop calls take and clip it; rects == NULL: whole pictures.  Slot i of the destination belongs to picture i:
 * dst_device + i * image_stride, channel c at + c * plane_stride (plane_stride != 0: planar) or interleaved in the pixel
 * (plane_stride == 0), lines row_stride bytes apart.  channels is 1 or 3; a one-component picture in a 3-channel batch is written to
 * all three channels.  Nothing but the served slots' own out_height lines of out_width pixels is written.
 * MIJPEG_ERR_INVALID_PARAMETER for the call, before anything is launched, written or counted: NULL d or dst_device, out_width or
 * out_height below 1 (or above 65535), channels not 1 or 3, a rectangle the crop calls refuse, a row_stride below a line, a
 * plane_stride below a plane's lines, an image_stride below a slot's data, a slot that spans 4 GiB or more.
 * Per picture, status[i] (n entries, may be NULL): 0 = served; the decode status of a picture in error; MIJPEG_ERR_NOT_IMPLEMENTED for
 * 16-bit samples (12 bit, JPEG XT), two or four components, three components into channels == 1, and a crop of 4 GiB or more.  Such a
 * picture's slot is not written, the others are served. */
#define MIJPEG_ERR_NOT_IMPLEMENTED MIJPEG_ERR_OPERATION_UNIMPLEMENTED
int mijpeg_reconstruct_ragged_resized_device(mijpeg_decoder *d, const mijpeg_rect *rects /* NULL: whole pictures */, int32_t out_width,
                                             int32_t out_height, int32_t channels, void *dst_device, int64_t image_stride,
                                             int64_t plane_stride /* 0: interleaved */, int64_t row_stride, uint32_t flags,
                                             int32_t *status /* n, may be NULL */, int sync);
/* What the object's last resized call did. */
typedef struct mijpeg_ragged_resized_stats {
  int32_t images, resampled, refused;   /* pictures of the list; served; not served (status[i] != 0)                      */
  int32_t window_launches;              /* stage 1: what the crop call reports as `launches` for the same rectangles      */
  int32_t resample_launches;            /* stage 2: 1 whenever resampled > 0                                              */
  int32_t reserved;
  int64_t arena_bytes;                  /* the crops of this call, each padded to 16 bytes                                */
} mijpeg_ragged_resized_stats;
int mijpeg_ragged_resized_stats_get(mijpeg_decoder *d, mijpeg_ragged_resized_stats *out);
/* The filter's taps for one axis, no device: first[m], count[m] and the weights of output o at weights[o * capacity_per_output ...]
 * (zero behind its count).  -> the axis's maximal tap count (<= min(n, 2 ceil(max(n, m) / m) + 1)); with a NULL array only that.
 * 0: n or m outside 1 .. 65535, or a capacity below the maximal count. */
int32_t mijpeg_resample_taps(int32_t n, int32_t m, int32_t *first, int32_t *count, int16_t *weights, int32_t capacity_per_output);

/* ---- ... as a normalised float batch, mirrored per picture, still one resample launch -------------------
 * What a training step does to the resized batch -- flip a random half of the pictures, x / 255, subtract a mean, divide by a
 * deviation, cast --, in the resample launch's store epilogue.  Everything the resized call says holds here too: the object, `flags`,
 * `sync`, clipping, refusals and status[i], the arena and stage 1, "nothing but the served slots' own lines is written" and "invalid
 * parameters are refused before anything is launched, written or counted".  Every stride is in BYTES.
 * Let v be the sample the resized call writes for a pixel and picture component (an integer 0 .. 255).  For output channel c
 *   y = fl32(fl32((float)v * scale[c]) + bias[c])
 * two IEEE binary32 operations, each rounded to nearest-even -- NOT a fused multiply-add.  A one-component picture in a 3-channel
 * batch uses the same v with each channel's own scale[c], bias[c].  The stored element:
 *   MIJPEG_SAMPLE_F32   y
 *   MIJPEG_SAMPLE_F16   binary16 of y, to nearest-even
 *   MIJPEG_SAMPLE_BF16  the upper 16 bits of bits(y) + 0x7fff + ((bits(y) >> 16) & 1): to nearest-even for every finite y
 *   MIJPEG_SAMPLE_U8    v (scale and bias are not read)
 * A result that is subnormal in the stored type is outside the contract: it may be flushed to zero.
 * mirror[i] != 0: slot i holds the lines of the unmirrored slot reversed -- column x is column out_width - 1 - x of what the call
 * writes without the flag.  Resize, then flip; not flip, then resize (the two differ where the filter's remainder goes to "the lowest
 * such i").
 * MIJPEG_ERR_INVALID_PARAMETER, besides the resized call's cases and as early: format == NULL, sample outside 0 .. 3, reserved != 0,
 * for float samples a scale[c] or bias[c] with c < channels that is not finite, and dst_device, image_stride, plane_stride or
 * row_stride that is no multiple of the element size (1, 4, 2, 2 bytes).  The resized call's stride checks apply with lines, planes
 * and slots in bytes of that element; a slot still spans less than 4 GiB. */
#define MIJPEG_SAMPLE_U8   0
#define MIJPEG_SAMPLE_F32  1
#define MIJPEG_SAMPLE_F16  2
#define MIJPEG_SAMPLE_BF16 3
typedef struct mijpeg_batch_format {
  int32_t sample;            /* MIJPEG_SAMPLE_*                                                  */
  int32_t reserved;          /* 0                                                                */
  float scale[3], bias[3];   /* per OUTPUT channel; ignored for MIJPEG_SAMPLE_U8                 */
  const uint8_t *mirror;     /* n flags (0 / non-0), host memory, read before the call returns; NULL: none mirrored */
} mijpeg_batch_format;
int mijpeg_reconstruct_ragged_normalized_device(mijpeg_decoder *d, const mijpeg_rect *rects /* NULL: whole pictures */, int32_t out_width,
                                                int32_t out_height, int32_t channels, const mijpeg_batch_format *format, void *dst_device,
                                                int64_t image_stride, int64_t plane_stride /* 0: interleaved */, int64_t row_stride,
                                                uint32_t flags, int32_t *status /* n, may be NULL */, int sync);
/* What the last resized or normalised call of the object stored: mijpeg_ragged_resized_stats keeps its members and meanings for both
 * calls (resample_launches is 1 for any n); this is beside it.  The resized call sets {MIJPEG_SAMPLE_U8, 0}. */
typedef struct mijpeg_ragged_normalized_stats {
  int32_t sample;            /* MIJPEG_SAMPLE_* of the call                                      */
  int32_t mirrored;          /* served pictures written mirrored                                 */
  int32_t reserved[2];
} mijpeg_ragged_normalized_stats;
int mijpeg_ragged_normalized_stats_get(mijpeg_decoder *d, mijpeg_ragged_normalized_stats *out);

/* ---- stateless device entry points (inputs and outputs resident in HBM) -------------------- */

/* Describes a batch of equally shaped frames whose coefficient planes are already on the device. */
typedef struct mijpeg_batch {
  mijpeg_info info;            /* geometry + quantiser tables (shared by the batch unless quant_dev: then the
                                  element-wise maxima over the frames, which the kernel selection looks at,
                                  and range_max / fast_arith of the most demanding frame) */
  const int16_t *coef_dev;     /* frame f starts at coef_dev + f * coef_frame_stride (int16 units) */
  int64_t coef_frame_stride;
  const uint16_t *quant_dev;   /* optional: per-frame tables [frames][4][64] u16 on the device: deltas of
                                  COMPONENT c of frame f, natural order; plain JPEG only.  They are expanded
                                  into the workspace (see mijpeg_workspace_bytes) by a small kernel in front */
  uint8_t *out_dev;            /* frame f pixels at out_dev + f * out_frame_stride (bytes)          */
  int64_t out_frame_stride;
  int64_t out_row_stride;      /* bytes per line                                                  */
  int32_t frames;
  uint32_t flags;
  void *workspace;             /* device scratch for the unfused path, see mijpeg_workspace_bytes     */
  size_t workspace_bytes;
  const mijpeg_xt_params *xt;  /* required when info.xt != 0 (host memory)                            */
} mijpeg_batch;

/* Device scratch the batch needs (0 for the fused kernels of plain JPEG; the L tables for the fused JPEG XT kernel;
 * tables + int32 sample planes for the generic kernels; plus frames x 1 KiB of expanded tables with quant_dev). */
size_t mijpeg_workspace_bytes(const mijpeg_batch *batch);

/* dequant + IDCT + upsample + colour transform + interleaved store for `frames` frames in one
 * launch on `stream` (hipStream_t).  Asynchronous.  This is what bench.py times. */
int mijpeg_launch_reconstruct(const mijpeg_batch *batch, void *stream);

/* Name of the kernel the batch would run ("fused420", "generic", ...) -- for profiling scripts. */
const char *mijpeg_kernel_name(const mijpeg_batch *batch);

/* ---- encoder direction of the block pipeline -----------------------------------------------------
 * What BlockBitmapRequester::PullSourceData / AdvanceQRows (control/blockbitmaprequester.cpp:505-576, 708-846) do
 * per block in front of the entropy coder: forward L transformation (colortrafo/ycbcrtrafo.cpp:85-242), box
 * downsampling (upsampling/downsampler.cpp:70-139), forward DCT + quantisation (dct/idct.cpp:114-222), for frames
 * resident in HBM.  Entropy coding and marker writing are not part of it. */

/* Completes *info from width, height, components (1 or 3), precision (8, or 12: an extended sequential frame), hsamp[], vsamp[],
 * quant_index[] and quant[][]: MCU grid, subsampling factors, plane sizes, coef_offset[] and coef_count, as a frame header with
 * these values would produce (marker/frame.cpp, marker/component.cpp).  Returns MIJPEG_OK or MIJPEG_ERR_INVALID_PARAMETER
 * (any other precision included). */
int mijpeg_frame_layout(mijpeg_info *info);

typedef struct mijpeg_forward_batch {
  mijpeg_info info;            /* completed by mijpeg_frame_layout; ycbcr = 1: RGB in, YCbCr coded; 0: identity   */
  const uint8_t *pixels_dev;   /* interleaved 8-bit samples, `components` per pixel; frame f at + f * pixel_frame_stride.
                                  info.precision == 12: the address of native-endian uint16_t samples, 0..4095, on a 2-byte
                                  boundary; the strides stay in bytes and are even                                    */
  int64_t pixel_frame_stride;  /* bytes                                                                            */
  int64_t pixel_row_stride;    /* bytes per line                                                                   */
  int16_t *coef_dev;           /* out: quantised coefficients in the layout the decoder reads (natural order inside a
                                  block, blocks row-major, planes at info.coef_offset[]); MCU padding blocks are zero */
  int64_t coef_frame_stride;   /* int16 units                                                                      */
  int32_t frames;
  uint32_t flags;              /* 0                                                                                */
} mijpeg_forward_batch;

/* One launch on `stream` (hipStream_t) for all frames of the batch.  Asynchronous. */
int mijpeg_launch_forward(const mijpeg_forward_batch *batch, void *stream);

/* Entropy coder + stream writer for what mijpeg_launch_forward produced (after a device-to-host copy): quantised
 * coefficient planes in HOST memory, the layout of *info, -> a baseline (SOF0) JPEG stream with one interleaved
 * Huffman-sequential scan (codestream/sequentialscan.cpp:430-676 WriteMCU / EncodeBlock; segment syntax: marker/ directory).
 * restart_interval: MCUs per restart interval, 0 = none (the intervals are coded in parallel on `threads` threads,
 * <= 0: default); optimize != 0: Huffman tables optimised for the picture (Annex K.2) instead of the Annex K.3 tables.
 * MCU padding blocks are coded as "same DC, no AC".  *stream is malloc'ed: release it with mijpeg_free.
 * info->precision == 12: an extended sequential (SOF1, P = 12) stream; DC differences up to category 15 and AC coefficients up to
 * category 14 are coded (8 bits: 11 and 10), anything beyond is MIJPEG_ERR_OVERFLOW_PARAMETER.  The Annex K.3 tables have no codes
 * for categories 12..15, so at precision 12 the Huffman tables are ALWAYS built from the picture's statistics and `optimize` is
 * ignored -- here, in mijpeg_encode_image16 and in mijpeg_encode_batch_device, on the host and on the device coder alike. */
int mijpeg_encode_coefficients(const mijpeg_info *info, const int16_t *coef, int restart_interval, int optimize, int threads,
                               uint8_t **stream, size_t *size);
void mijpeg_free(void *p);

/* The device twin of mijpeg_encode_coefficients: the planes are in DEVICE memory (coef_dev, the layout of *info: what
 * mijpeg_launch_forward writes and what mijpeg_device_coefficients returns), the device entropy coder (hencode.hip) codes them,
 * and only the finished stream comes down -- byte for byte the stream mijpeg_encode_coefficients writes for the same planes,
 * restart interval and `optimize` (precision 12: the tables are always the picture's own).  So a stream that was entropy-decoded on
 * the device can be coded again with another restart interval or with optimised tables without its coefficients leaving HBM.
 * The caller wrote the coefficients, so they are checked as the host coder checks them: a DC difference beyond category 11 (15 at
 * precision 12) or an AC coefficient beyond category 10 (14) is MIJPEG_ERR_OVERFLOW_PARAMETER and no stream, whatever int16
 * values stand there; the object serves the next call as usual.  The check takes the symbol statistics in a launch of its own,
 * which with `optimize` (or precision 12) are the statistics the tables are built from anyway; with the standard tables it costs
 * one launch and one host synchronisation more than the pixel entry points spend.  Arguments are checked before a device is
 * touched: null pointers, a restart interval outside 0..65535 (INVALID_PARAMETER), a precision other than 8 or 12 or a
 * component count other than 1 or 3 (OPERATION_UNIMPLEMENTED), more than 64 blocks per MCU or more than 2^30 - 1025 blocks
 * (NOT_AVAILABLE), an object without a device (NOT_AVAILABLE).  coef_dev must not have work pending on other streams.
 * *stream is malloc'ed (mijpeg_free).  mijpeg_last_timing: [0] the whole call. */
int mijpeg_encode_coefficients_device(mijpeg_decoder *d, const mijpeg_info *info, const int16_t *coef_dev, int restart_interval,
                                      int optimize, uint8_t **stream, size_t *size);

/* The quantiser tables the reference encoder derives from `-q quality` with its default (Annex K) matrices:
 * Quantization::InitDefaultTables, marker/quantization.cpp:275-466, for 8-bit frames -- natural order. */
void mijpeg_quality_tables(int quality, uint16_t luma[64], uint16_t chroma[64]);

/* Whole encoder-direction pipeline for one picture in HOST memory on the decoder object's device: upload, forward kernel,
 * download of the coefficients, entropy coding (`jpeg -bl -q quality -s ... -z restart_interval [-h] in.ppm out.jpg` of the
 * reference CLI, cmd/encodec.cpp; here: Annex K.3 or optimised Huffman tables, one interleaved baseline scan).
 * pixels: interleaved 8-bit, `components` (1 or 3) per pixel, row_stride bytes per line; hsamp/vsamp: sampling factors
 * per component (NULL: 1x1 everywhere); RGB input is coded as YCbCr.  *stream is malloc'ed (mijpeg_free). */
int mijpeg_encode_image(mijpeg_decoder *d, const uint8_t *pixels, int32_t width, int32_t height, int32_t components, int64_t row_stride,
                        int quality, const int32_t *hsamp, const int32_t *vsamp, int restart_interval, int optimize,
                        uint8_t **stream, size_t *size);
/* The same with flags.  By default the entropy coder runs on the device too (hencode.hip: the coefficients never leave
 * HBM, only the finished stream comes down); MIJPEG_ENCODE_HOST_CODER downloads the coefficients and codes them with
 * mijpeg_encode_coefficients.  Both write the same bytes. */
#define MIJPEG_ENCODE_HOST_CODER 1u
int mijpeg_encode_image_ex(mijpeg_decoder *d, const uint8_t *pixels, int32_t width, int32_t height, int32_t components, int64_t row_stride,
                           int quality, const int32_t *hsamp, const int32_t *vsamp, int restart_interval, int optimize, uint32_t flags,
                           uint8_t **stream, size_t *size);

/* The same for a picture of 16-bit samples: interleaved native-endian uint16_t, 0..4095, `components` (1 or 3) per pixel,
 * row_stride_bytes (even) bytes per line -> an extended sequential stream (SOF1, P = 12: what `jpeg -q quality -s ... -z
 * restart_interval -h in.ppm out.jpg` of the reference writes for a PNM with maxval 4095, coefficient for coefficient and
 * quantiser table for table; the Huffman tables are the picture's own, see mijpeg_encode_coefficients).  precision: 12 -- anything
 * else is MIJPEG_ERR_INVALID_PARAMETER.  The quantiser tables of `quality` are the reference's for 12-bit frames: not limited to
 * 255 as mijpeg_quality_tables' are, so low qualities write 16-bit DQT entries.  flags: as mijpeg_encode_image_ex. */
int mijpeg_encode_image16(mijpeg_decoder *d, const uint16_t *pixels, int32_t width, int32_t height, int32_t components, int64_t row_stride_bytes,
                          int precision, int quality, const int32_t *hsamp, const int32_t *vsamp, int restart_interval, uint32_t flags,
                          uint8_t **stream, size_t *size);

/* Frames that are already in device memory (a renderer's or a video pipeline's output): forward kernels for the whole batch in
 * one launch, then the device entropy coder frame by frame; only the finished streams cross PCIe.  batch->coef_dev is
 * scratch for the coefficient planes (frames * coef_frame_stride int16).  streams[f] is malloc'ed (mijpeg_free).
 * batch->info.precision == 12: frames of 16-bit samples (mijpeg_forward_batch), streams as mijpeg_encode_image16 writes them. */
int mijpeg_encode_batch_device(mijpeg_decoder *d, const mijpeg_forward_batch *batch, int restart_interval, int optimize,
                               uint8_t **streams, size_t *sizes);

/* ---- ragged encode: n pictures of ANY shapes in one device pass ------------------------------------------------------
 * The encoder's counterpart of mijpeg_decode_ragged_device: a list of pictures that differ in size, sampling, quality and
 * restart interval -> n baseline streams, stream i byte for byte what mijpeg_encode_image_ex writes for picture i.  The forward
 * kernels run once per kernel family over all pictures (ragged flavours: a workgroup looks its picture up), the five passes of the
 * device entropy coder once over all pictures: the number of launches and of host synchronisations does not grow
 * with n.  Lists of equally shaped frames are served by mijpeg_encode_batch_device as well.  Which of the two is faster for them
 * HAS NOT BEEN MEASURED (profiles/ragged_encode.txt, section 3): until it has, uniform lists are better served by the uniform
 * call, whose cost is known. */
/* mijpeg_encode_frame has no precision field and its layout is not touched: the calls above take 8-bit pictures, and lists with
 * 12-bit pictures in them go through the ...16 flavours below, which take the precision of every picture in a parallel array. */
typedef struct mijpeg_encode_frame {
  const uint8_t *pixels;     /* interleaved 8-bit samples, `components` per pixel: device memory for mijpeg_encode_ragged_device,
                                host memory for mijpeg_encode_ragged; the planner does not look at it.  A 12-bit picture of the
                                ...16 calls: native-endian uint16_t samples 0..4095 at an even address                          */
  int64_t row_stride;        /* bytes per line, >= width * components (12-bit picture: even, >= width * components * 2)         */
  int32_t width, height;     /* 1 .. 65535                                                                                      */
  int32_t components;        /* 1 (grey) or 3 (RGB in, YCbCr coded)                                                             */
  int32_t hsamp[MIJPEG_MAX_COMPONENTS], vsamp[MIJPEG_MAX_COMPONENTS]; /* sampling factors per component, 1 .. 4                 */
  int32_t quality;           /* as mijpeg_quality_tables takes it                                                               */
  int32_t restart_interval;  /* MCUs per restart interval, 0 = none; 0 .. 65535                                                 */
} mijpeg_encode_frame;

/* What the planner decides for picture i.  A list is cut into PASSES where it would exceed the coder's limits (pass_blocks
 * below); the index spaces start again in every pass. */
typedef struct mijpeg_encode_ragged_item {
  mijpeg_info info;          /* the frame as mijpeg_frame_layout completes it at the picture's precision, the tables of `quality`
                                in quant[0], quant[1]                                                                            */
  int64_t coef_base;         /* int16 index of its coefficient store in the pass's packed scratch store                         */
  uint32_t blocks;           /* blocks of its scan (MCUs * blocks per MCU)                                                       */
  uint32_t intervals;        /* restart intervals of its scan (1 without restart markers)                                        */
  uint32_t first_block;      /* in the pass's block index space: a multiple of 256, the picture owns whole workgroups            */
  uint32_t first_interval;   /* in the pass's concatenated interval list                                                         */
  int32_t pass;
  int32_t reserved;
} mijpeg_encode_ragged_item;
typedef struct mijpeg_encode_ragged_totals {
  int64_t coef_count;        /* int16 elements of the largest pass's coefficient store                                           */
  uint64_t blocks;           /* index space of all passes together (every picture padded to a multiple of 256)                   */
  uint64_t intervals;        /* all pictures                                                                                     */
  int32_t passes;
  int32_t reserved;
} mijpeg_encode_ragged_totals;
/* The planner on its own (no device, no decoder object).  pass_blocks: most blocks (padded) of a pass, 0 = the default (2^24; at
 * most 2^30, what the coder's prefix sums take; a picture larger than the limit is a pass of its own).  MIJPEG_ERR_INVALID_PARAMETER
 * for n < 1, NULL lists and any description outside the ranges above, fractional subsampling factors included. */
int mijpeg_encode_ragged_plan(const mijpeg_encode_frame *frames, int n, uint32_t pass_blocks, mijpeg_encode_ragged_item *items,
                              mijpeg_encode_ragged_totals *totals);

/* Pictures resident in DEVICE memory -> streams[i] / sizes[i] in host memory (malloc'ed: mijpeg_free).  optimize != 0: Huffman
 * tables optimised per picture.  flags: 0.  On any failure every stream already allocated is freed, all streams[i] are NULL and
 * all sizes[i] are 0.  Scratch (coefficients, bit counts, plain stream, output arena) belongs to the decoder object.  The
 * environment variable MIJPEG_ENCODE_RAGGED_PASS_BLOCKS overrides pass_blocks (testing).  Passes are cut by blocks alone: one
 * whose plain stream would reach 2^30 stuffing chunks (64 GiB -- out of reach below 2^28 blocks a pass, sixteen times the default)
 * is refused with MIJPEG_ERR_NOT_AVAILABLE instead of being cut again. */
int mijpeg_encode_ragged_device(mijpeg_decoder *d, const mijpeg_encode_frame *frames, int n, int optimize, uint32_t flags,
                                uint8_t **streams, size_t *sizes);
/* The same for pictures in HOST memory: gathered into pinned staging, uploaded in one piece, then the device path. */
int mijpeg_encode_ragged(mijpeg_decoder *d, const mijpeg_encode_frame *frames, int n, int optimize, uint32_t flags,
                         uint8_t **streams, size_t *sizes);
/* What the last ragged encode of the object did. */
typedef struct mijpeg_encode_ragged_stats {
  int32_t pictures;
  int32_t passes;
  int32_t forward_launches;  /* ragged forward kernels, at most six per pass for each flavour of picture present -- 8-bit
                                interleaved, 12-bit interleaved, 8-bit planar: at most twelve per pass of an interleaved call,
                                at most eighteen per pass of a planar one (mijpeg_encode_ragged_planar_device16)                 */
  int32_t coder_launches;    /* count, prefix-sum, interval, gather, emit and stuffing kernels, summed (a prefix sum takes one,
                                three or five launches with the SIZE of its input)                                               */
  int32_t host_syncs;        /* host waits for the device: per pass one for the plain sizes, one for the 0xFF counts, one for the
                                download, one more for the statistics in a pass with optimize or with a 12-bit picture in it (an
                                8-bit pass without optimize stays at three; buffers that grow wait as well: not counted)         */
  int32_t reserved;
  int64_t bytes_downloaded;  /* the output arenas                                                                                */
} mijpeg_encode_ragged_stats;
int mijpeg_encode_ragged_get_stats(mijpeg_decoder *d, mijpeg_encode_ragged_stats *out);

/* The same three calls for lists in which every picture is 8-bit or 12-bit, freely mixed.  precision: NULL = 8 for every picture
 * (the calls above are these with NULL), otherwise precision[i] is 8 or 12 -- anything else is MIJPEG_ERR_INVALID_PARAMETER.  For a
 * 12-bit picture frames[i].pixels addresses interleaved native-endian uint16_t samples, 0..4095, on a 2-byte boundary, and
 * row_stride (still bytes) is even and at least width * components * 2; a violation is MIJPEG_ERR_INVALID_PARAMETER with all
 * outputs cleared as above.  Stream i is byte for byte what mijpeg_encode_image16 (flags 0) writes for a 12-bit picture -- an
 * extended sequential frame, SOF1 with P = 12, the reference's quantiser tables for 12-bit frames (16-bit DQT entries at low
 * qualities) -- and what mijpeg_encode_image_ex writes for an 8-bit one.  12-bit pictures always get Huffman tables from their
 * own statistics, as everywhere else at precision 12; `optimize` speaks for the 8-bit pictures of the list only, which keep the
 * Annex K.3 tables without it.  Blocks, intervals, index spaces, pass cuts and coef_base of the plan do not depend on precision. */
int mijpeg_encode_ragged_plan16(const mijpeg_encode_frame *frames, const int32_t *precision, int n, uint32_t pass_blocks,
                                mijpeg_encode_ragged_item *items, mijpeg_encode_ragged_totals *totals);
int mijpeg_encode_ragged_device16(mijpeg_decoder *d, const mijpeg_encode_frame *frames, const int32_t *precision, int n,
                                  int optimize, uint32_t flags, uint8_t **streams, size_t *sizes);
int mijpeg_encode_ragged16(mijpeg_decoder *d, const mijpeg_encode_frame *frames, const int32_t *precision, int n,
                           int optimize, uint32_t flags, uint8_t **streams, size_t *sizes);

/* ---- planar (CHW) input for the ragged encode ----------------------------------------------------------
 * mijpeg_encode_ragged_device16 for pictures whose samples lie in component planes, as mijpeg_reconstruct_ragged_planar_device
 * writes them: planes[i * MIJPEG_MAX_COMPONENTS + c] is the device address of plane c of picture i, c < frames[i].components (a
 * grey picture has one plane); frames[i].pixels is ignored; frames[i].row_stride is the line pitch in bytes of every plane of
 * picture i, at least width * sample_bytes; sample (x, y) of component c is at plane[c] + y * row_stride + x * sample_bytes.
 * Planes may lie anywhere, in any order, in separate allocations.  precision: as above, NULL = 8; a 12-bit picture's planes hold
 * native-endian uint16_t samples 0..4095 at even addresses with an even pitch.
 * Stream i is byte for byte what mijpeg_encode_ragged_device16 writes for the interleaved picture with the same samples and the same
 * description, precision and `optimize`; the call takes what that call takes -- 1 or 3 components, any sampling factors, 8 or 12 bit,
 * any sizes, any alignment -- and the route only decides the speed:
 *   fused      8-bit pictures of three components: read by the planar-input flavours of the ragged forward kernels.  Planes and
 *              pitch on dword boundaries: the tile and interior kernels where the interleaved picture takes them; otherwise the
 *              per-block kernel alone, byte by byte
 *   two_pass   12-bit pictures of three components: interleaved into scratch of the object first, ONE launch per picture, in front
 *              of the forward launches of the picture's pass and on the same stream; then the 12-bit interleaved work lists
 *   own_plane  one-component pictures of either precision: their plane is the interleaved picture
 * All arguments are checked for every picture before anything is launched, written or counted (the statistics of the last call
 * stay): MIJPEG_ERR_INVALID_PARAMETER for NULL lists, n < 1, flags != 0, a description mijpeg_encode_ragged_plan16 refuses, a NULL
 * plane that a picture needs, a pitch below one line, an odd address or pitch at 12 bit, a precision other than 8 or 12.  An object
 * without a device: MIJPEG_ERR_NOT_AVAILABLE.  On any failure all streams[i] are NULL and all sizes[i] are 0.
 * It adds to a pass of the interleaved call the plane table in the pass's one upload, at most six forward launches and the
 * interleave launches; no host wait.  mijpeg_encode_ragged_get_stats speaks of a planar call as of any other. */
int mijpeg_encode_ragged_planar_device16(mijpeg_decoder *d, const mijpeg_encode_frame *frames, const void *const *planes,
                                         const int32_t *precision, int n, int optimize, uint32_t flags, uint8_t **streams, size_t *sizes);
/* What the object's last planar encode did. */
typedef struct mijpeg_encode_planar_stats {
  int32_t pictures;
  int32_t fused;               /* read by the planar-input forward flavours                                    */
  int32_t two_pass;            /* interleaved first                                                            */
  int32_t own_plane;           /* one-component pictures                                                       */
  int32_t interleave_launches; /* one per two_pass picture                                                     */
  int32_t reserved;
} mijpeg_encode_planar_stats;
int mijpeg_encode_planar_stats_get(mijpeg_decoder *d, mijpeg_encode_planar_stats *out);
/* The first pass of the two-pass route on its own, the mirror image of mijpeg_deinterleave_device: `components` planes in device
 * memory (plane_row_stride bytes per line of each) -> an interleaved picture (components x sample_bytes per pixel, dst_row_stride
 * bytes per line), on the object's stream; sync != 0 waits for it.  components 1..4, sample_bytes 1 or 2; any addresses and
 * pitches that hold a line.  Nothing but the lines' own bytes is written. */
int mijpeg_interleave_device(mijpeg_decoder *d, const void *const planes[MIJPEG_MAX_COMPONENTS], int64_t plane_row_stride, int32_t width,
                             int32_t height, int32_t components, int32_t sample_bytes, void *dst_device, int64_t dst_row_stride, int sync);

/* ---- ragged transcode: decoded lists recoded from their coefficients in HBM -------------------------------
 * The pictures of the object's last mijpeg_decode_ragged_device / ...16 call, coded again as baseline (8 bit) or extended sequential
 * (12 bit) Huffman streams from the quantised planes the decode left in device memory: no inverse transform, no pixels, no second
 * generation of DCT loss.  Per picture the source's quantiser tables are kept -- the recode is lossless: the output decodes to the
 * source's coefficients -- or replaced by those of a quality, the planes requantised in the coefficient domain by ONE launch per pass
 * of requant_list_kernel.  The rule, in integers, for coefficient c at position k with source entry a and target entry b:
 *   v = c * a;  r = sign(v) * floor((|v| + floor(b / 2)) / b)            (to nearest, halves away from zero; b == a gives r == c)
 * r outside what a frame of the picture's precision P codes -- DC in [-2^(P+2), 2^(P+2) - 1], |AC| <= 2^(P+2) - 1 -- refuses the
 * picture with MIJPEG_ERR_OVERFLOW_PARAMETER; kept pictures pass the same check (a crafted stream's own planes may lie outside).
 * The passes are those of the ragged encode with the requant launch in place of the forward launches: launches and host waits do
 * not grow with the list, MIJPEG_ENCODE_RAGGED_PASS_BLOCKS cuts them, 12-bit pictures always get Huffman tables of their own and
 * `optimize` speaks for the 8-bit ones.  The outputs carry the headers every encoder call here writes (DQT, SOF0 / SOF1, DHT, DRI,
 * SOS): APPn, COM and ICC segments of the source are NOT carried across.  Sampling and size change only under a transform (below); the output is never
 * progressive or arithmetic coded (a progressive source comes out sequential).
 * Served: members of the layout groups, and pictures of the single-image route whose object holds int16 planes of a plain Huffman
 * frame of 8 or 12 bits with 1 or 3 components (progressive, SOF1, DNL, 4:4:0, 4:1:1, ...).  A one-component output has sampling
 * factors 1 x 1 whatever the source's header said.  status[i] per picture, the others are served:
 *   MIJPEG_ERR_NOT_IMPLEMENTED      JPEG XT, 2 or 4 components, 32-bit planes (coef_wide), a table entry of 0, or a kept 8-bit picture with
 *                                   a table entry above 255 (no baseline DQT holds it)
 *   MIJPEG_ERR_NOT_AVAILABLE        more blocks per MCU than the device entropy coder takes, or 2^30 blocks or more
 *   MIJPEG_ERR_OVERFLOW_PARAMETER   a requantised (or kept) value outside the coding range
 *   the decode's status             where the decode of the picture failed
 * streams[i] / sizes[i]: malloc'ed (mijpeg_free); NULL / 0 for a picture that is refused or skipped.  The decode's stores stay as
 * they are: reconstruction calls may precede or follow.  Arguments are checked before a device is touched: NULL lists or flags != 0,
 * a quality outside -1 .. 100 or a restart interval outside -1 .. 65535 are MIJPEG_ERR_INVALID_PARAMETER; an object without a device
 * MIJPEG_ERR_NOT_AVAILABLE; without a decoded ragged batch MIJPEG_ERR_OBJECT_DOESNT_EXIST.  On a failure of the call all streams[i]
 * are NULL and all sizes[i] 0. */
#define MIJPEG_TRANSCODE_KEEP 0     /* quality: the source's quantiser tables (lossless recode) */
#define MIJPEG_TRANSCODE_SKIP (-1)  /* quality: no stream for this picture, status MIJPEG_OK    */
typedef struct mijpeg_transcode_spec {
  int32_t quality;           /* 1..100 as mijpeg_quality_tables takes it (at precision 12: entries to 32767), KEEP or SKIP */
  int32_t restart_interval;  /* MCUs per restart interval 0..65535, or -1: the source's                                    */
} mijpeg_transcode_spec;
/* specs: one per picture of the decoded batch, or NULL: keep everything (tables and restart intervals). */
int mijpeg_transcode_ragged_device(mijpeg_decoder *d, const mijpeg_transcode_spec *specs, int optimize, uint32_t flags, uint8_t **streams,
                                   size_t *sizes, int32_t *status);
/* What the object's last transcode call did. */
typedef struct mijpeg_transcode_ragged_stats {
  int32_t pictures;          /* of the decoded batch                                                                           */
  int32_t served;            /* pictures with a stream                                                                         */
  int32_t kept;              /* ... of them with the source's tables                                                           */
  int32_t refused;           /* pictures with a status: the decode's, a refusal of the plan, the range check                   */
  int32_t children;          /* served pictures of the single-image route                                                      */
  int32_t passes;
  int32_t requant_launches;  /* one per pass                                                                                   */
  int32_t coder_launches;    /* as mijpeg_encode_ragged_stats counts them                                                      */
  int32_t host_syncs;        /* per pass: plain sizes (the range flags travel with them), 0xFF counts, download, one more for the
                                statistics of pictures with tables of their own.  Waiting for a child's own stream, once per child
                                in front of the first pass, is not counted                                                     */
  int32_t child_uploads;     /* children whose planes were decoded on the host and travelled to the device for this            */
  int64_t bytes_downloaded;  /* the output arenas                                                                              */
} mijpeg_transcode_ragged_stats;
int mijpeg_transcode_ragged_stats_get(mijpeg_decoder *d, mijpeg_transcode_ragged_stats *out);
/* The plan of one picture, no device and no object: source frame + spec -> the output frame (layout, tables, quant_index), its
 * restart interval, kept (1: the source's tables).  Returns the picture's status as above (MIJPEG_OK for SKIP: *out zeroed);
 * MIJPEG_ERR_INVALID_PARAMETER for NULL arguments and a spec outside its ranges.  *out is zeroed on every refusal. */
int mijpeg_transcode_plan(const mijpeg_info *source, const mijpeg_transcode_spec *spec, mijpeg_info *out, int32_t *restart_interval, int32_t *kept);
/* The rule over n blocks (64 coefficients each, natural order) in host memory: src -> dst (may be the same) with source table
 * q_old and target table q_new (no entry 0), clamped into the coding range of `precision` (8 or 12).  Returns the number of
 * coefficients that were clamped, or MIJPEG_ERR_INVALID_PARAMETER.  The kernel's host twin: one header states the rule for both. */
int64_t mijpeg_requantize(const int16_t *src, int16_t *dst, int64_t n, const uint16_t q_old[64], const uint16_t q_new[64], int precision);

/* ---- ragged transcode: lossless flips, transposes and rotations -------------------------------------------
 * What jpegtran -flip / -transpose / -transverse / -rotate does, in the pass of the ragged transcode and on the planes in device
 * memory: a permutation of blocks, a transposition inside each block, sign changes on odd frequencies -- no pixels, no DCT loss --
 * by ONE launch per pass of transform_list_kernel for the pictures that have a transform; the others stay with
 * requant_list_kernel, so a pass has at most two first-stage launches and a list without transforms exactly the launches, waits,
 * bytes and statistics of mijpeg_transcode_ragged_device.  The codes are jpegtran's JXFORM_CODE; each is "transpose first (T), then
 * mirror horizontally (MH) and / or vertically (MV)":
 *   NONE -   FLIP_H MH   FLIP_V MV   TRANSPOSE T   TRANSVERSE T MH MV   ROT_90 T MH (clockwise)   ROT_180 MH MV   ROT_270 T MV
 * T swaps width and height and every component's sampling factors (4:2:2 becomes 4:4:0) and transposes the quantiser tables; with a
 * quality the (transposed) source entry at the destination position is the rule's a.  A mirrored axis must be a whole number of MCUs
 * of the frame after T: otherwise the picture is refused with MIJPEG_ERR_NOT_AVAILABLE (jpegtran -perfect), or, with
 * MIJPEG_TRANSFORM_TRIM OR-ed in, the partial MCU column or row at the source's far edge is dropped and width or height shrink to the
 * multiple (a picture that would shrink to nothing is refused).  Axes that are not mirrored keep their partial MCUs.  A
 * one-component output is 1 x 1 sampled: its MCU is one block. */
#define MIJPEG_TRANSFORM_NONE 0
#define MIJPEG_TRANSFORM_FLIP_H 1
#define MIJPEG_TRANSFORM_FLIP_V 2
#define MIJPEG_TRANSFORM_TRANSPOSE 3
#define MIJPEG_TRANSFORM_TRANSVERSE 4
#define MIJPEG_TRANSFORM_ROT_90 5    /* clockwise */
#define MIJPEG_TRANSFORM_ROT_180 6
#define MIJPEG_TRANSFORM_ROT_270 7
#define MIJPEG_TRANSFORM_TRIM 0x100  /* OR-ed in: drop partial MCUs of a mirrored axis instead of refusing the picture */
/* mijpeg_transcode_ragged_device with one transform per picture of the decoded batch (NULL: none, the existing call).  A code outside
 * the eight (with or without TRIM) is MIJPEG_ERR_INVALID_PARAMETER, returned before a device is touched; everything else as there. */
int mijpeg_transcode_ragged_transformed_device(mijpeg_decoder *d, const mijpeg_transcode_spec *specs, const int32_t *transforms, int optimize,
                                               uint32_t flags, uint8_t **streams, size_t *sizes, int32_t *status);
/* mijpeg_transcode_plan under a transform: the output frame with its width, height, sampling and (kept: transposed) tables.  The
 * refusals of mijpeg_transcode_plan come first; then the geometry's MIJPEG_ERR_NOT_AVAILABLE.  A bad code: INVALID_PARAMETER. */
int mijpeg_transcode_plan_transformed(const mijpeg_info *source, const mijpeg_transcode_spec *spec, int32_t transform, mijpeg_info *out,
                                      int32_t *restart_interval, int32_t *kept);
/* The kernel's host twin over ONE component's plane in host memory (blocks of 64 coefficients, natural order): src, src_bw x src_bh
 * blocks, under table q_old (in the SOURCE's order) -> dst (another buffer), dst_bw x dst_bh blocks, under q_new (the destination's
 * order).  transform: one of the eight codes (TRIM is the plan's matter: it shows in dst_bw / dst_bh).  A destination block
 * without a source block is zero.  Returns the number of clamped coefficients, or MIJPEG_ERR_INVALID_PARAMETER. */
int64_t mijpeg_transform_blocks(const int16_t *src, int32_t src_bw, int32_t src_bh, int16_t *dst, int32_t dst_bw, int32_t dst_bh, int32_t transform,
                                const uint16_t q_old[64], const uint16_t q_new[64], int precision);
/* What the transforms of the object's last transcode call did (beside mijpeg_transcode_ragged_stats). */
typedef struct mijpeg_transcode_transform_stats {
  int32_t transformed;         /* served pictures with a transform other than NONE                       */
  int32_t trimmed;             /* ... of them that lost a partial MCU column or row                      */
  int32_t geometry_refusals;   /* pictures refused because a mirrored axis is no whole number of MCUs    */
  int32_t transform_launches;  /* one per pass that holds a transformed picture                          */
} mijpeg_transcode_transform_stats;
int mijpeg_transcode_transform_stats_get(mijpeg_decoder *d, mijpeg_transcode_transform_stats *out);

/* Worker threads mijpeg_decode_coefficients uses for threads <= 0 (MIJPEG_THREADS overrides; default min(cores, 64)). */
int mijpeg_default_threads(void);

/* The large buffers of destroyed decoder objects (pinned coefficient store and frame, their device mirrors) wait in a process-wide
 * cache for the next object on the same device -- a client that constructs a JPEG object per picture would otherwise pin and
 * unpin ~200 MB per 8K picture.  At most four buffers per kind and MIJPEG_BUFFER_CACHE_MB megabytes in all (environment,
 * default 2048, 0 = keep nothing) are kept; a buffer enters the cache only after the device has gone idle, so kernels a client
 * launched on its own streams against mijpeg_device_coefficients() / a mijpeg_batch never race with the next owner.
 * mijpeg_trim_cache() hands everything the cache holds back to the runtime and returns the number of bytes freed. */
size_t mijpeg_trim_cache(void);

/* Library / build identification. */
const char *mijpeg_version(void);

#ifdef __cplusplus
}
#endif
#endif
