// capi.cpp -- the C ABI of include/mijpeg.h: decoder object (host entropy decoding + streaming upload +
// GPU reconstruction + rectangle service) and the stateless batch launch.  Compiled with hipcc (host side
// only uses the HIP runtime API).  There is NO CPU fallback for the reconstruction: without a device the
// reconstruct calls fail with MIJPEG_ERR_DEVICE.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <new>
#include <memory>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>

#include "../../include/mijpeg.h"
#include "decoder.hpp"
#include "huffman_dev.hpp"
#include "encoder.hpp"
#include "forward.hpp"
#include "hencode.hpp"
#include "kernels.hpp"

using namespace mij;

// The boundary lets no C++ exception through (the reference turns everything into an error code at JPEG::Read /
// DisplayRectangle, interface/jpeg.cpp:205-220, tools/environment.hpp:752-784): every extern "C" body is a function-try-block
// whose handler lands here.  Out of memory is the reference's JPGERR_OUT_OF_MEMORY; anything else is a defect of this library
// and reported as such, not as a verdict on the stream.
int boundary_catch(mijpeg_decoder *d, const char *where) noexcept
{
  int code = MIJPEG_ERR_PHASE_ERROR;
  const char *what = "unexpected exception";
  char buf[160];
  try {
    throw;
  } catch (const std::bad_alloc &) {
    code = MIJPEG_ERR_OUT_OF_MEMORY;
    what = "out of memory";
  } catch (const std::length_error &) { // (a container asked for more than max_size: memory all the same)
    code = MIJPEG_ERR_OUT_OF_MEMORY;
    what = "out of memory (container size)";
  } catch (const std::exception &e) {
    snprintf(buf, sizeof(buf), "%s", e.what());
    what = buf;
  } catch (...) {
  }
  if (d) {
    d->err_code = code;
    try {
      d->err_msg = std::string(where) + ": " + what;
    } catch (...) {
      d->err_msg.clear(); // (no memory for the message either: the code stands)
    }
  }
  return code;
}

// The large buffers of destroyed decoder objects -- pinned coefficient store and frame, their device mirrors -- wait here for
// the next object on the same device: a client that constructs a JPEG object per picture (cmd/reconstruct.cpp does) would
// otherwise pin ~200 MB of pages per 8K picture, 17 ms of the 24 ms such a decode took from Construct to Destruct.  At most
// four buffers per kind and 2 GiB in all are kept; a request takes the smallest buffer that fits and is at most twice as large.
namespace {
struct BufferCache {
  struct Entry { void *p; size_t bytes; int device; bool pinned; };
  std::mutex m;
  std::vector<Entry> kept;
  void *take(int device, bool pinned, size_t bytes, size_t *got)
  {
    std::lock_guard<std::mutex> lock(m);
    int best = -1;
    for (int i = 0; i < (int)kept.size(); i++)
      if (kept[(size_t)i].device == device && kept[(size_t)i].pinned == pinned && kept[(size_t)i].bytes >= bytes && kept[(size_t)i].bytes <= 2 * bytes &&
          (best < 0 || kept[(size_t)i].bytes < kept[(size_t)best].bytes))
        best = i;
    if (best < 0) return nullptr;
    void *p = kept[(size_t)best].p;
    *got = kept[(size_t)best].bytes;
    kept.erase(kept.begin() + best);
    return p;
  }
  // would give() keep a buffer like this one right now?
  bool has_room(int device, bool pinned, size_t bytes)
  {
    static const bool off = getenv("MIJPEG_NO_BUFFER_CACHE") != nullptr; // A-B measurements
    if (off || bytes < ((size_t)1 << 20)) return false;
    std::lock_guard<std::mutex> lock(m);
    return room_locked(device, pinned, bytes);
  }
  // false: not kept, the caller frees it
  bool give(int device, bool pinned, void *p, size_t bytes)
  {
    std::lock_guard<std::mutex> lock(m);
    if (!room_locked(device, pinned, bytes)) return false;
    kept.push_back(Entry{p, bytes, device, pinned});
    return true;
  }
  bool room_locked(int device, bool pinned, size_t bytes) const
  {
    size_t total = bytes, same = 0;
    for (const Entry &e : kept) {
      total += e.bytes;
      same += e.device == device && e.pinned == pinned;
    }
    return same < 4 && total <= limit_bytes();
  }
  // MIJPEG_BUFFER_CACHE_MB: what the cache may hold in all (default 2048, 0 = keep nothing)
  static size_t limit_bytes()
  {
    static const size_t lim = [] {
      const char *e = getenv("MIJPEG_BUFFER_CACHE_MB");
      return e ? (size_t)strtoull(e, nullptr, 10) << 20 : (size_t)2 << 30;
    }();
    return lim;
  }
  // mijpeg_trim_cache: hand everything back to the runtime
  size_t trim()
  {
    std::vector<Entry> gone;
    {
      std::lock_guard<std::mutex> lock(m);
      gone.swap(kept);
    }
    size_t bytes = 0;
    for (const Entry &e : gone) {
      bytes += e.bytes;
      if (e.pinned) (void)hipHostFree(e.p);
      else {
        int cur = 0;
        (void)hipGetDevice(&cur);
        (void)hipSetDevice(e.device);
        (void)hipFree(e.p);
        (void)hipSetDevice(cur);
      }
    }
    return bytes;
  }
};
BufferCache &buffer_cache()
{
  static BufferCache *c = new BufferCache; // (never destroyed: the HIP runtime may be gone when static destructors run)
  return *c;
}
} // namespace
static void release_big(int device, bool pinned, void *p, size_t bytes)
{
  if (!p) return;
  // hipFree / hipHostFree wait for the device before they take the memory away, and the buffers were handed to clients
  // (mijpeg_device_coefficients, mijpeg_batch: kernels on the client's own streams may still read them).  A buffer that changes
  // hands through the cache instead gets the same guarantee: nothing on the device is in flight when the next owner writes it.
  // Only a buffer that actually enters the cache needs it spelled out (and only its own device has to be idle): growing a
  // workspace in the middle of a pipeline must not stall every stream of the process for a buffer that is freed anyway.
  if (buffer_cache().has_room(device, pinned, bytes)) {
    if (device >= 0) {
      int cur = -1;
      (void)hipGetDevice(&cur);
      if (cur != device) (void)hipSetDevice(device);
      (void)hipDeviceSynchronize();
      if (cur >= 0 && cur != device) (void)hipSetDevice(cur);
    }
    if (buffer_cache().give(device, pinned, p, bytes)) return; // (another thread may have filled the room meanwhile: freed then)
  }
  if (pinned) (void)hipHostFree(p);
  else (void)hipFree(p);
}

// A buffer that grows through the buffer cache: device memory, or pinned host memory (the coefficient store and the frame)
static int ensure_cached(mijpeg_decoder *d, bool pinned, void **ptr, size_t *cap, size_t bytes)
{
  if (*cap >= bytes) return MIJPEG_OK;
  quiesce(d); // (the buffer may go to another object: nothing of this one may still read or write it)
  release_big(d->device, pinned, *ptr, *cap);
  *ptr = nullptr;
  *cap = 0;
  size_t got = 0;
  if (void *p = buffer_cache().take(d->device, pinned, bytes, &got)) {
    *ptr = p;
    *cap = got;
    return MIJPEG_OK;
  }
  HIP_TRY(d, pinned ? hipHostMalloc(ptr, bytes, hipHostMallocDefault) : hipMalloc(ptr, bytes));
  *cap = bytes;
  return MIJPEG_OK;
}

int ensure_dev(mijpeg_decoder *d, void **ptr, size_t *cap, size_t bytes) { return ensure_cached(d, false, ptr, cap, bytes); }

// A batch that was submitted (mijpeg_submit_batch_device) and not waited for still reads the pinned staging buffers
// (ent_host, stage_host, status words) from its asynchronous uploads: every entry point that rewrites them settles it first.
static int settle_pending(mijpeg_decoder *d)
{
  if (!d->pend_n) return MIJPEG_OK;
  d->pend_n = 0;
  if (d->device >= 0) {
    HIP_TRY(d, hipSetDevice(d->device));
    HIP_TRY(d, hipStreamSynchronize(d->stream));
    if (d->copy_stream) HIP_TRY(d, hipStreamSynchronize(d->copy_stream));
  }
  return MIJPEG_OK;
}

extern "C" {

const char *mijpeg_version(void) { return "libjpeg_amd/mijpeg 0.1 (gfx950)"; }

int mijpeg_default_threads(void) { return default_threads(); }

size_t mijpeg_trim_cache(void)
try {
  return buffer_cache().trim();
} catch (...) { (void)boundary_catch(nullptr, "mijpeg_trim_cache"); return 0; }

int mijpeg_create(mijpeg_decoder **out, int device)
try {
  if (!out) return MIJPEG_ERR_INVALID_PARAMETER;
  *out = nullptr;
  mijpeg_decoder *d = new (std::nothrow) mijpeg_decoder();
  if (!d) return MIJPEG_ERR_OUT_OF_MEMORY;
  d->device = device;
  if (device >= 0) {
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&d->ev0);
    if (e == hipSuccess) e = hipEventCreate(&d->ev1);
    if (e != hipSuccess) {
      delete d;
      return MIJPEG_ERR_DEVICE;
    }
  }
  *out = d;
  return MIJPEG_OK;
} catch (...) { return boundary_catch(nullptr, "mijpeg_create"); }

void mijpeg_destroy(mijpeg_decoder *d)
try {
  if (!d) return;
  if (d->device >= 0) {
    (void)hipSetDevice(d->device);
    quiesce(d); // (the buffers below may go to another object)
    release_big(d->device, true, d->coef_host, d->coef_host_cap * sizeof(int16_t));
    release_big(d->device, true, d->img_host, d->img_host_cap);
    release_big(d->device, false, d->coef_dev, d->coef_dev_cap * sizeof(int16_t));
    release_big(d->device, false, d->img_dev, d->img_dev_cap);
    if (d->ws_dev) (void)hipFree(d->ws_dev);
    if (d->batch_quant_dev) (void)hipFree(d->batch_quant_dev);
    if (d->ent_dev) (void)hipFree(d->ent_dev);
    if (d->ent_host) (void)hipHostFree(d->ent_host);
    if (d->stage_host) (void)hipHostFree(d->stage_host);
    if (d->walk_dev) (void)hipFree(d->walk_dev);
    if (d->xt_helper) mijpeg_destroy(d->xt_helper);
    if (d->ragged_desc_dev) (void)hipFree(d->ragged_desc_dev);
    if (d->ragged_desc_host) (void)hipHostFree(d->ragged_desc_host);
    if (d->ragged_uploaded) (void)hipEventDestroy(d->ragged_uploaded);
    if (d->enc_dev) (void)hipFree(d->enc_dev);
    for (int k = 0; k < 2; k++) {
      if (d->henc_dev[k]) (void)hipFree(d->henc_dev[k]);
      if (d->henc_out_dev[k]) (void)hipFree(d->henc_out_dev[k]);
    }
    if (d->henc_host) (void)hipHostFree(d->henc_host);
    if (d->eragged_dev) (void)hipFree(d->eragged_dev);
    if (d->eragged_out_dev) (void)hipFree(d->eragged_out_dev);
    if (d->eragged_host) (void)hipHostFree(d->eragged_host);
    if (d->eragged_down) (void)hipHostFree(d->eragged_down);
    if (d->walk_host) (void)hipHostFree(d->walk_host);
    if (d->req_dev) (void)hipFree(d->req_dev);
    if (d->req_host) (void)hipHostFree(d->req_host);
    if (d->rowmap_dev) (void)hipFree(d->rowmap_dev);
    if (d->ent_free) (void)hipEventDestroy(d->ent_free);
    for (hipEvent_t e : d->copy_events) (void)hipEventDestroy(e);
    for (hipEvent_t e : d->band_events) (void)hipEventDestroy(e);
    if (d->copy_stream) (void)hipStreamDestroy(d->copy_stream);
    if (d->ev0) (void)hipEventDestroy(d->ev0);
    if (d->ev1) (void)hipEventDestroy(d->ev1);
    if (d->chain_ev) (void)hipEventDestroy(d->chain_ev);
    if (d->ms_ready) (void)hipEventDestroy(d->ms_ready);
    if (d->ms_done) (void)hipEventDestroy(d->ms_done);
    if (d->ms_stream) (void)hipStreamDestroy(d->ms_stream);
    if (d->stream) (void)hipStreamDestroy(d->stream);
  } else {
    free(d->coef_host);
  }
  if (d->alpha) mijpeg_destroy(d->alpha);
  for (mijpeg_decoder *c : d->ragged_children) mijpeg_destroy(c);
  delete d;
} catch (...) { (void)boundary_catch(d, "mijpeg_destroy"); }

int mijpeg_set_input(mijpeg_decoder *d, const uint8_t *data, size_t size)
try {
  if (!d) return MIJPEG_ERR_INVALID_PARAMETER;
  if (!data) return set_error(d, MIJPEG_ERR_STREAM_EMPTY, "empty input stream");
  // a stream of no bytes: the reference's first GetWord meets the end of file, which is its SOI error (codestream/decoder.cpp:92-96)
  if (!size) return set_error(d, MIJPEG_ERR_MALFORMED_STREAM, "stream does not contain a JPEG file, SOI marker missing");
  d->data = data;
  d->size = size;
  d->parsed = d->decoded = d->uploaded = d->img_valid = d->model_valid = false;
  d->parse_fresh = false;
  d->ragged_n = 0; // (the coefficient store is about to be this stream's)
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_set_input"); }

int mijpeg_read_header(mijpeg_decoder *d, mijpeg_info *info)
try {
  if (!d) return MIJPEG_ERR_INVALID_PARAMETER;
  if (!d->data) return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "no input stream has been set");
  d->parse_fresh = false;
  const int rc = d->host.parse(d->data, d->size, true);
  if (rc) return set_error(d, rc, d->host.error.message);
  if (info) *info = d->host.info;
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_read_header"); }

static int ensure_coef_store(mijpeg_decoder *d, size_t count, bool need_host = true)
{
  if (d->device < 0) {
    if (need_host && d->coef_host_cap < count) {
      free(d->coef_host);
      d->coef_host = (int16_t *)malloc(count * sizeof(int16_t));
      if (!d->coef_host) return set_error(d, MIJPEG_ERR_OUT_OF_MEMORY, "out of memory for the coefficient store");
      d->coef_host_cap = count;
    }
    return MIJPEG_OK;
  }
  size_t host = d->coef_host_cap * sizeof(int16_t), dev = d->coef_dev_cap * sizeof(int16_t); // (the caps count int16)
  int rc = need_host ? ensure_cached(d, true, (void **)&d->coef_host, &host, count * sizeof(int16_t)) : MIJPEG_OK;
  if (!rc) rc = ensure_cached(d, false, (void **)&d->coef_dev, &dev, count * sizeof(int16_t));
  d->coef_host_cap = host / sizeof(int16_t);
  d->coef_dev_cap = dev / sizeof(int16_t);
  return rc;
}

// The alpha channel of a JPEG XT file: the reference turns to the ALFA box behind the legacy codestream's EOI (and the residual
// codestream), inside JPEG::Read (Image::ParseTrailer, codestream/image.cpp:1430-1460): what is wrong with it fails the read,
// whether or not the client will ask for alpha.  Here a decoder object of its own -- same device, the file's boxes under the
// names an image's decoder looks for (HostDecoder::alpha_boxes) -- decodes it right behind the picture's codestreams.
static int decode_alpha_channel(mijpeg_decoder *d, int threads)
{
  d->alpha_ready = false;
  d->alpha_refusal = 0;
  if (!d->host.has_alpha()) return MIJPEG_OK;
  const uint8_t *p = nullptr;
  size_t n = 0;
  if (!d->host.alpha_stream(&p, &n)) return MIJPEG_OK;
  if (!d->alpha && mijpeg_create(&d->alpha, d->device) != MIJPEG_OK)
    return set_error(d, MIJPEG_ERR_OUT_OF_MEMORY, "no decoder object for the alpha channel");
  d->alpha_data.assign(p, p + n);
  d->alpha->host.preset_boxes(d->host.alpha_boxes());
  int rc = n ? mijpeg_set_input(d->alpha, d->alpha_data.data(), n)
             : set_error(d->alpha, MIJPEG_ERR_MALFORMED_STREAM, "Alpha channel codestream is invalid, SOI marker missing.");
  if (!rc) {
    // Image::ParseAlphaChannel compares the dimensions right behind the alpha FRAME HEADER (codestream/image.cpp:1366-1380), before
    // any of its scans is looked at (a frame header whose width byte is damaged: -1038, whatever its entropy coded data would do
    // to a frame of that size).  A height that arrives in a DNL marker still says 0 there.
    d->alpha->host.parse(d->alpha_data.data(), n, true); // (headers only; what it returns is the decode's to report)
    const mijpeg_info &a = d->alpha->host.info, &f = d->host.info;
    if (a.width > 0 && (a.width != f.width || a.height != f.height || a.dnl))
      rc = set_error(d->alpha, MIJPEG_ERR_MALFORMED_STREAM, "Malformed stream - residual image dimensions do not match the dimensions of the legacy image");
    else if (a.width > 0 && a.components != 1)
      rc = set_error(d->alpha, MIJPEG_ERR_MALFORMED_STREAM, "Malformed stream - the alpha channel may only consist of a single component");
  }
  if (!rc) rc = mijpeg_decode_coefficients(d->alpha, threads);
  if (!rc) {
    const mijpeg_info &a = d->alpha->host.info, &f = d->host.info;
    if (a.width != f.width || a.height != f.height) // codestream/image.cpp:1370-1380
      rc = set_error(d->alpha, MIJPEG_ERR_MALFORMED_STREAM, "Malformed stream - residual image dimensions do not match the dimensions of the legacy image");
    else if (a.components != 1)
      rc = set_error(d->alpha, MIJPEG_ERR_MALFORMED_STREAM, "Malformed stream - the alpha channel may only consist of a single component");
  }
  d->alpha_refusal = 0;
  if (rc == MIJPEG_ERR_OPERATION_UNIMPLEMENTED) {
    // (what this path declines does not fail the read -- but what stops the alpha image's codestreams does, and the reference has
    // read them whatever their specification says)
    const int v = d->alpha->host.declined_verdict();
    if (v && v != MIJPEG_ERR_OPERATION_UNIMPLEMENTED) rc = set_error(d->alpha, v, d->alpha->host.error.message.c_str());
  }
  if (rc) {
    const char *m = nullptr;
    mijpeg_last_error(d->alpha, &m);
    // What the alpha image's colour transformer would refuse (a table that does not exist ...) the reference only finds when
    // alpha pixels are asked for (Tables::ColorTrafoOf at the first request); what this path declines (-1034) is no reason to
    // withhold the picture either: the file reads, mijpeg_alpha_channel reports why there is no alpha.
    if (rc == MIJPEG_ERR_OPERATION_UNIMPLEMENTED || d->alpha->host.transformer_refused()) {
      d->alpha_refusal = rc;
      d->alpha_refusal_msg = m ? m : "";
      return MIJPEG_OK;
    }
    d->decoded = false; // the read has failed: no picture either (JPEG::Read returns false)
    return set_error(d, rc, m ? m : "the alpha channel does not decode");
  }
  d->alpha_ready = true;
  return MIJPEG_OK;
}

int mijpeg_decode_coefficients(mijpeg_decoder *d, int threads)
try {
  if (!d) return MIJPEG_ERR_INVALID_PARAMETER;
  if (!d->data) return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "no input stream has been set");
  if (d->device >= 0) HIP_TRY(d, hipSetDevice(d->device));
  if (const int prc = settle_pending(d)) return prc;
  d->batch_frames = 0;
  static const bool trace = getenv("MIJPEG_READ_TIMES") != nullptr; // diagnostics: where a read spends its time
  const auto t_begin = std::chrono::steady_clock::now();
  const bool parsed_already = d->parse_fresh; // (by mijpeg_decode_coefficients_device a moment ago)
  d->parse_fresh = false;
  int rc = parsed_already ? 0 : d->host.parse(d->data, d->size, false);
  if (rc) return set_error(d, rc, d->host.error.message);
  d->parsed = true;
  const mijpeg_info &f = d->host.info;
  const auto t_parsed = std::chrono::steady_clock::now();
  rc = ensure_coef_store(d, (size_t)f.coef_count);
  if (rc) return rc;
  const auto t_store = std::chrono::steady_clock::now();
  d->img_valid = d->model_valid = false;
  d->uploaded = false;
  d->host_planes_stale = false;
  d->batch_frames = 0;

  hipError_t copy_err = hipSuccess;
  std::function<void(int, int)> cb;
  if (d->device >= 0) {
    // stream finished MCU-row bands to the device while the workers decode the rest
    (void)hipEventRecord(d->ev0, d->stream);
    cb = [&](int r0, int r1) {
      for (int c = 0; c < f.components; c++) {
        const size_t row = (size_t)f.blocks_w[c] * 64 * f.vsamp[c]; // int16 per MCU row of this component
        const size_t off = (size_t)f.coef_offset[c] + row * r0, cnt = row * (r1 - r0);
        hipError_t e = hipMemcpyAsync(d->coef_dev + off, d->coef_host + off, cnt * sizeof(int16_t), hipMemcpyHostToDevice, d->stream);
        if (e != hipSuccess) copy_err = e;
      }
    };
  }
  // ... and the residual planes of a JPEG XT frame with hidden bits as the last refinement window finishes them (a worker thread
  // calls: its own device binding, its own error slot)
  std::atomic<int> rcopy_err{(int)hipSuccess};
  if (d->device >= 0 && d->host.residual()) {
    d->host.set_residual_rows_callback([&, d](int c, int y0, int y1) {
      (void)hipSetDevice(d->device);
      const mijpeg_xt_params &x = d->host.xt;
      const size_t row = (size_t)x.residual.blocks_w[c] * 64 * (x.residual_wide ? 2 : 1); // int16 units per block row
      const size_t off = (size_t)x.residual.coef_offset[c] + row * (size_t)y0;
      const hipError_t e = hipMemcpyAsync(d->coef_dev + off, d->coef_host + off, row * (size_t)(y1 - y0) * sizeof(int16_t), hipMemcpyHostToDevice, d->stream);
      if (e != hipSuccess) rcopy_err.store((int)e);
    });
  }
  rc = d->host.decode(d->coef_host, threads, cb);
  d->host.set_residual_rows_callback(nullptr);
  if (rcopy_err.load() != (int)hipSuccess && copy_err == hipSuccess) copy_err = (hipError_t)rcopy_err.load();
  d->timing[0] = d->host.huffman_seconds;
  if (trace) {
    const auto ms = [](auto a, auto b) { return std::chrono::duration<double>(b - a).count() * 1e3; };
    fprintf(stderr, "read: parse %.2f ms, coefficient store %.2f ms, decode %.2f ms (entropy decoders %.2f)\n", ms(t_begin, t_parsed), ms(t_parsed, t_store),
            ms(t_store, std::chrono::steady_clock::now()), d->host.huffman_seconds * 1e3);
  }
  if (rc == MIJPEG_ERR_OVERFLOW_PARAMETER && !d->host.is_xt()) {
    // A coefficient beyond the 16-bit store -- only damaged streams get there: a DC prediction that runs away, a point
    // transform on garbage.  The reference keeps LONG coefficients and reconstructs what they hold; so does this frame,
    // in int32 planes (info.coef_wide) that the unfused kernels transform with the reference's 32-bit arithmetic.
    if (d->device >= 0) HIP_TRY(d, hipStreamSynchronize(d->stream)); // band uploads of the first attempt read coef_host
    d->parse_fresh = false;
    rc = d->host.parse(d->data, d->size, false);
    if (rc) return set_error(d, rc, d->host.error.message);
    rc = ensure_coef_store(d, (size_t)f.coef_count * 2);
    if (rc) return rc;
    rc = d->host.decode_wide((int32_t *)d->coef_host, threads);
    d->timing[0] += d->host.huffman_seconds;
    // (a frame with hidden refinement scans has no 32-bit planes on this path: declined, not the stream's fault)
    if (rc == MIJPEG_ERR_OVERFLOW_PARAMETER && d->host.left_16bit_store())
      return set_error(d, MIJPEG_ERR_OPERATION_UNIMPLEMENTED, "frame with hidden refinement scans and coefficients beyond the 16-bit store (a damaged scan) is not on the accelerated path");
    if (rc) return set_error(d, rc, d->host.error.message);
    if (d->device >= 0 && copy_err == hipSuccess)
      copy_err = hipMemcpyAsync(d->coef_dev, d->coef_host, (size_t)f.coef_count * sizeof(int16_t), hipMemcpyHostToDevice, d->stream);
  }
  // (a JPEG XT frame whose damaged scans leave the 16-bit store: the reference goes on in LONG coefficients, this path has no
  // int32 planes for merged frames -- declined like every other subset it does not take, not reported as the stream's fault)
  if (rc == MIJPEG_ERR_OVERFLOW_PARAMETER && d->host.is_xt() && d->host.left_16bit_store())
    return set_error(d, MIJPEG_ERR_OPERATION_UNIMPLEMENTED, "JPEG XT frame with coefficients beyond the 16-bit store (a damaged scan) is not on the accelerated path");
  if (rc) return set_error(d, rc, d->host.error.message);
  if (d->device >= 0 && d->host.residual() && copy_err == hipSuccess) {
    // the residual codestream's planes sit behind the legacy planes in the same buffer
    const mijpeg_xt_params &x = d->host.xt;
    bool some = false;
    for (int c = 0; c < x.residual.components; c++) some |= d->host.residual_rows_reported(c) > 0;
    if (!some) {
      const size_t off = (size_t)x.residual.coef_offset[0], cnt = (size_t)f.coef_count - off;
      copy_err = hipMemcpyAsync(d->coef_dev + off, d->coef_host + off, cnt * sizeof(int16_t), hipMemcpyHostToDevice, d->stream);
    } else // (rows the decode has sent on their way already: the rest of each plane)
      for (int c = 0; c < x.residual.components && copy_err == hipSuccess; c++) {
        const int y0 = d->host.residual_rows_reported(c), y1 = x.residual.blocks_h[c];
        if (y0 >= y1) continue;
        const size_t row = (size_t)x.residual.blocks_w[c] * 64 * (x.residual_wide ? 2 : 1);
        const size_t off = (size_t)x.residual.coef_offset[c] + row * (size_t)y0;
        copy_err = hipMemcpyAsync(d->coef_dev + off, d->coef_host + off, row * (size_t)(y1 - y0) * sizeof(int16_t), hipMemcpyHostToDevice, d->stream);
      }
  }
  if (copy_err != hipSuccess) return hip_fail(d, copy_err, "hipMemcpyAsync(coefficients)");
  d->decoded = true;
  if (d->device >= 0) {
    (void)hipEventRecord(d->ev1, d->stream);
    d->uploaded = true;
  }
  return decode_alpha_channel(d, threads);
} catch (...) { return boundary_catch(d, "mijpeg_decode_coefficients"); }

int64_t mijpeg_unstuffed_scan(mijpeg_decoder *d, uint8_t *dst, size_t capacity, uint32_t *begin, size_t n_begin, size_t piece_bytes,
                              int32_t *n_intervals)
{
  if (!d) return MIJPEG_ERR_INVALID_PARAMETER;
  if (!d->parsed || d->host.scans.empty()) return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "no parsed stream");
  if (const int prc = settle_pending(d)) return prc;
  if (piece_bytes == 1 && dst) { // the other producer: the marker search writes the copy itself (what a batch's workers do)
    if (capacity < d->size + 64) return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "the sink needs the stream's size (+ 64 bytes of slack)");
    d->host.set_unstuff_sink(dst, d->size);
    d->parse_fresh = false;
    const int rc = d->host.parse(d->data, d->size, false);
    if (rc) return set_error(d, rc, d->host.error.message);
    if (d->host.scans.empty() || d->host.scans[0].unstuffed_at != dst) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "the marker search did not write the copy");
    if (n_intervals) *n_intervals = (int32_t)d->host.scans[0].interval_ubegin.size();
    for (size_t k = 0; k < d->host.scans[0].interval_ubegin.size() && k < n_begin && begin; k++) begin[k] = d->host.scans[0].interval_ubegin[k];
    return (int64_t)d->host.scans[0].unstuffed_size;
  }
  const std::vector<uint32_t> &b = d->host.scans[0].interval_ubegin;
  const size_t total = d->host.scans[0].unstuffed_size;
  if (n_intervals) *n_intervals = (int32_t)b.size();
  for (size_t k = 0; k < b.size() && k < n_begin && begin; k++) begin[k] = b[k];
  if (dst && capacity >= total) {
    std::vector<HostDecoder::UnstuffPiece> pieces;
    d->host.unstuff_pieces(0, piece_bytes ? piece_bytes : ((size_t)1 << 20), pieces);
    for (const auto &p : pieces) d->host.unstuff_piece(0, p, dst);
  }
  return (int64_t)total;
}

int64_t mijpeg_speculative_scans(int64_t *pieces)
{
  if (pieces) *pieces = g_speculative_pieces.load();
  return g_speculative_scans.load();
}

int mijpeg_device_walk_rounds(mijpeg_decoder *d) { return d ? d->walk_rounds : 0; }

int mijpeg_get_info(mijpeg_decoder *d, mijpeg_info *info)
try {
  if (!d || !info) return MIJPEG_ERR_INVALID_PARAMETER;
  if (d->batch_frames < 0) { // a submitted batch: the range check is known once its Huffman kernel is through
    const int rc = mijpeg_finish_batch_device(d);
    if (rc) return rc;
  }
  if (d->batch_frames > 0) { // frame shape of the batch, range check of its most demanding image
    *info = d->batch_info;
    return MIJPEG_OK;
  }
  if (!d->data) return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "no input stream has been set");
  *info = d->host.info;
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_get_info"); }

int mijpeg_get_xt_params(mijpeg_decoder *d, mijpeg_xt_params *xt)
try {
  if (!d || !xt) return MIJPEG_ERR_INVALID_PARAMETER;
  if (!d->data || !d->host.is_xt()) return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "the loaded stream is not a JPEG XT stream");
  *xt = d->host.xt;
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_get_xt_params"); }

const int32_t *mijpeg_coefficients32(mijpeg_decoder *d, int component)
{
  if (!d || !d->decoded || component < 0 || component >= d->host.info.components || !d->host.info.coef_wide) return nullptr;
  return (const int32_t *)(d->coef_host + d->host.info.coef_offset[component]); // wide frames are decoded on the host
}

const int16_t *mijpeg_coefficients(mijpeg_decoder *d, int component)
{
  if (!d || !d->decoded || component < 0 || component >= d->host.info.components) return nullptr;
  if (d->host.info.coef_wide) {
    set_error(d, MIJPEG_ERR_OVERFLOW_PARAMETER, "the frame holds 32-bit coefficients (info.coef_wide): mijpeg_coefficients32");
    return nullptr;
  }
  if (d->host_planes_stale) { // decoded on the device: fetch once
    if (hipSetDevice(d->device) != hipSuccess) return nullptr;
    if (ensure_coef_store(d, (size_t)d->host.info.coef_count, true)) return nullptr;
    if (hipMemcpyAsync(d->coef_host, d->coef_dev, (size_t)d->host.info.coef_count * sizeof(int16_t), hipMemcpyDeviceToHost, d->stream) != hipSuccess ||
        hipStreamSynchronize(d->stream) != hipSuccess)
      return nullptr;
    d->host_planes_stale = false;
  }
  return d->coef_host + d->host.info.coef_offset[component];
}

int mijpeg_decode_coefficients_device(mijpeg_decoder *d, int min_intervals)
try {
  if (!d) return MIJPEG_ERR_INVALID_PARAMETER;
  if (!d->data) return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "no input stream has been set");
  if (d->device < 0) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "decoder was created without a device");
  HIP_TRY(d, hipSetDevice(d->device));
  if (const int prc = settle_pending(d)) return prc;
  using clk = std::chrono::steady_clock;
  const auto t0 = clk::now();
  d->parse_fresh = false;
  int rc = d->host.parse(d->data, d->size, false);
  if (rc) return set_error(d, rc, d->host.error.message);
  d->parsed = true;
  d->batch_frames = 0;
  const auto t_parsed = clk::now();
  HostDecoder *h = &d->host, *res = d->host.residual();
  // (a stream that does not qualify: the parse is as good as the one mijpeg_decode_coefficients would make next)
  d->parse_fresh = true;
  // progressive frames and frames with hidden refinement scans: every scan one restart interval per lane (huffman_prog_kernel)
  auto many_scans = [](const HostDecoder &x) { return x.info.progressive != 0 || x.has_hidden_scans() || x.scans.size() != 1; };
  static const bool no_multiscan = getenv("MIJPEG_NO_DEVICE_MULTISCAN") != nullptr; // A-B comparisons
  // (... and 12-bit frames, whose single scan the sequential kernel's path declines: round 6)
  const bool multiscan = !no_multiscan && (many_scans(d->host) || (res && many_scans(*res)) || (!res && d->host.info.precision != 8));
  if (multiscan) {
    if (const char *why = multiscan_obstacle(d->host, res != nullptr, false)) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, why);
    if (res)
      if (const char *why = multiscan_obstacle(*res, true, true)) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, why);
  } else {
    if (const char *why = device_entropy_obstacle(d->host, d->size, res != nullptr)) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, why);
    if (res) {
      if (const char *why = device_entropy_obstacle(*res, res->stream_size(), true)) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, why);
      if (d->host.xt.residual_wide) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "32-bit residual coefficients are decoded on the host");
    }
  }
  d->parse_fresh = false;
  rc = ensure_coef_store(d, (size_t)d->host.info.coef_count, false);
  if (rc) return rc;
  d->img_valid = d->model_valid = false;
  d->uploaded = false;
  d->decoded = false;
  // JPEG XT: the planes of the residual frame follow those of the legacy frame in the same store
  int64_t own_count = 0;
  for (int c = 0; c < d->host.info.components; c++) own_count += (int64_t)d->host.info.blocks_w[c] * d->host.info.blocks_h[c] * 64;
  const bool trace_read = TraceMarks::on();
  if (trace_read)
    fprintf(stderr, "[mijpeg device read] parse %.3f ms, checks + coefficient store %.3f ms\n", std::chrono::duration<double>(t_parsed - t0).count() * 1e3,
            std::chrono::duration<double>(clk::now() - t_parsed).count() * 1e3);
  if (multiscan) {
    MultiScanFrame fr[2] = {{h, false, 0}, {res, res && d->host.xt.residual_wide != 0, own_count}};
    rc = device_entropy_multiscan(d, fr, res ? 2 : 1, min_intervals);
  } else if (!res) {
    rc = device_entropy_batch(d, &h, &d->data, &d->size, 1, min_intervals, d->coef_dev, own_count, false);
  } else {
    // JPEG XT: the two codestreams are independent, so the residual one is decoded at the same time by a helper object
    // (own stream, own buffers) on a thread of its own, straight into the planes behind the legacy frame's
    if (!d->xt_helper && mijpeg_create(&d->xt_helper, d->device) != MIJPEG_OK) return set_error(d, MIJPEG_ERR_OUT_OF_MEMORY, "no helper decoder for the residual codestream");
    const uint8_t *rdata = res->stream_base();
    const size_t rsize = res->stream_size();
    int rc2 = MIJPEG_OK;
    std::thread helper([&]() {
      try {
        if (hipSetDevice(d->device) != hipSuccess) { rc2 = MIJPEG_ERR_DEVICE; return; }
        rc2 = device_entropy_batch(d->xt_helper, &res, &rdata, &rsize, 1, min_intervals, d->coef_dev + own_count, res->info.coef_count, true);
      } catch (...) { // (nothing may leave a thread's function)
        rc2 = boundary_catch(d->xt_helper, "residual codestream, device entropy decoding");
      }
    });
    struct Joiner { // (an exception on this thread must not meet a joinable thread object)
      std::thread &t;
      ~Joiner() { if (t.joinable()) t.join(); }
    } joiner{helper};
    rc = device_entropy_batch(d, &h, &d->data, &d->size, 1, min_intervals, d->coef_dev, own_count, true);
    helper.join();
    if (!rc && rc2) {
      const char *m = nullptr;
      mijpeg_last_error(d->xt_helper, &m);
      rc = set_error(d, rc2, m ? m : "residual codestream: device entropy decoding failed");
    }
  }
  if (!rc && res) {
    for (int c = 0; c < MIJPEG_MAX_COMPONENTS; c++) d->host.xt.residual.range_max[c] = res->info.range_max[c];
    d->host.info.fast_arith = 0; // as HostDecoder::decode has it: the fast flavours are chosen per kernel for XT
  }
  d->timing[0] = std::chrono::duration<double>(clk::now() - t0).count();
  d->timing[1] = std::chrono::duration<double>(t_parsed - t0).count(); // header parse + restart marker search
  d->timing[2] = d->timing[3] = 0;
  if (trace_read) fprintf(stderr, "[mijpeg device read] whole call %.3f ms\n", d->timing[0] * 1e3);
  if (rc) return rc;
  d->decoded = true;
  d->uploaded = true;
  d->host_planes_stale = true;
  return decode_alpha_channel(d, 0);
} catch (...) { return boundary_catch(d, "mijpeg_decode_coefficients_device"); }

// ------------------------------------------------------------------------------------------------
// batches: n streams of one geometry -> n coefficient stores -> n frames, two kernel launches in all
// ------------------------------------------------------------------------------------------------
// Aggregation over the images of a decoded batch: what one reconstruction launch for all of them needs to know.
static int finish_batch(mijpeg_decoder *d);

// The range gates of the kernel selection (plan_reconstruct): a kernel or flavour is admitted where mijpeg_info::range_max
// (sum |c| q of a block) is below its gate
constexpr int32_t GATE_DOT2 = 1477;          // fused420p_kernel's second pass on v_dot2 (idct_columns_dot2: sum |c| q <= 1476)
constexpr int32_t GATE_PACKED = 2047;        // chroma filtered as int16 pairs (packed 4:2:0, 4:2:2, 4:4:0)
constexpr int32_t GATE_INT16_SAMPLES = 7600; // int16 sample planes of the kernel pair; int16 luma of fusedxtw420_kernel<true>
constexpr int32_t GATE_FUSED8 = 8190;        // chroma of the 8-bit fused 4:2:2 / 4:4:0 / 4:1:1 / 4:4:4 kernels, fused1_kernel
constexpr int32_t GATE_XT_LEGACY = 16384;    // legacy frame of the JPEG XT kernels (fused, and the merge's 32-bit colour stage)
constexpr int32_t GATE_12_CHROMA = 45056;    // 12-bit fused kernels: chroma (every component of fused_tile_kernel's fast12)
constexpr int32_t GATE_12_LUMA = 49152;      // 12-bit fused kernels: luma
constexpr int32_t GATE_XT_RESIDUAL = 65536;  // residual frame of the fused JPEG XT kernels
constexpr int32_t RANGE_GATES[] = { // (ascending)
    GATE_DOT2, GATE_PACKED, GATE_INT16_SAMPLES, GATE_FUSED8, GATE_XT_LEGACY, GATE_12_CHROMA, GATE_12_LUMA, GATE_XT_RESIDUAL};

// What the last finished batch of shared tables reported, for the speculative launch of the next one (MIJPEG_FLAG_SPECULATIVE):
// frame geometry, tables, and the range check that selected its kernel.  Process-wide: the decoder objects of a pipeline work
// on chunks of the same material.
namespace {
struct SpecHint {
  std::mutex m;
  bool valid = false;
  mijpeg_info info{};
};
SpecHint *spec_hint()
{
  static SpecHint *h = new SpecHint;
  return h;
}
// an assumed range just below the next gate selects the kernel the hint's batch ran on and holds for every batch that stays
// below that gate
int32_t next_gate_below(int32_t range)
{
  for (int32_t g : RANGE_GATES)
    if (range < g) return g - 1;
  return -1;
}
bool same_shape_and_tables(const mijpeg_info &a, const mijpeg_info &b)
{
  if (a.width != b.width || a.height != b.height || a.components != b.components || a.precision != b.precision || a.ycbcr != b.ycbcr || a.xt != b.xt ||
      a.dnl != b.dnl || a.coef_count != b.coef_count)
    return false;
  for (int c = 0; c < a.components; c++) {
    if (a.hsamp[c] != b.hsamp[c] || a.vsamp[c] != b.vsamp[c]) return false;
    if (memcmp(a.quant[a.quant_index[c]], b.quant[b.quant_index[c]], sizeof(a.quant[0]))) return false;
  }
  return true;
}
} // namespace
static int settle_speculation(mijpeg_decoder *d);

static int submit_batch(mijpeg_decoder *d, const uint8_t *const *streams, const size_t *sizes, int n, int min_intervals, bool defer)
{
  if (!d || !streams || !sizes || n < 1) return MIJPEG_ERR_INVALID_PARAMETER;
  if (d->device < 0) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "decoder was created without a device");
  HIP_TRY(d, hipSetDevice(d->device));
  using clk = std::chrono::steady_clock;
  const auto t0 = clk::now();
  if (d->spec_active) { // a speculative reconstruction nobody validated (mijpeg_finish_batch_device): its verdict comes first
    const int src = settle_speculation(d);
    if (src) return src;
  }
  if (const int prc = settle_pending(d)) return prc; // a submitted batch nobody waited for: its staging buffers are about to be reused
  d->batch_frames = 0;
  d->ragged_n = 0; // (a ragged batch's coefficient stores are about to be overwritten)
  if (d->batch_hosts.size() < (size_t)n) d->batch_hosts.resize((size_t)n); // never shrinks: a pipeline's chunks differ in size, and
  for (auto &h : d->batch_hosts)                                         // a parser that is thrown away takes its grown vectors along
    if (!h) h.reset(new HostDecoder());
  // headers and restart markers of all streams, one stream per worker -- which writes the device's copy of the entropy
  // coded data (no byte stuffing, no markers) into the stream's slot of the pinned gathering area while it is at it
  std::vector<int> rcs((size_t)n, 0);
  {
    std::vector<size_t> slot;
    const size_t total = stream_slots(sizes, n, slot);
    const int src = ensure_pinned(d, &d->stage_host, &d->stage_cap, total);
    if (src) return src;
    parallel_for(std::min(n, default_threads()), [&](int w) {
      for (int i = w; i < n; i += std::min(n, default_threads())) {
        // (a worker walks ~3 GB/s this way: good for the many small streams of a batch; a large stream is searched in
        // parallel chunks and gathered in parallel pieces instead -- device_entropy_batch sees which it was)
        if (sizes[i] <= ((size_t)2 << 20) || n >= default_threads()) d->batch_hosts[(size_t)i]->set_unstuff_sink(d->stage_host + slot[(size_t)i], sizes[i]);
        rcs[(size_t)i] = d->batch_hosts[(size_t)i]->parse(streams[i], sizes[i], false);
      }
    });
  }
  for (int i = 0; i < n; i++)
    if (rcs[(size_t)i]) return set_error(d, rcs[(size_t)i], d->batch_hosts[(size_t)i]->error.message);
  const auto t_parsed = clk::now();
  std::vector<HostDecoder *> hosts((size_t)n);
  for (int i = 0; i < n; i++) hosts[(size_t)i] = d->batch_hosts[(size_t)i].get();
  for (int i = 0; i < n; i++)
    if (const char *why = device_entropy_obstacle(*hosts[(size_t)i], sizes[i])) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, why);
  const mijpeg_info &f0 = hosts[0]->info;
  // one reconstruction launch serves the batch; images with tables of their own (motion JPEG under rate control) make it
  // read per-frame tables from device memory instead of the kernel arguments
  bool own_tables = false;
  for (int i = 1; i < n && !own_tables; i++) {
    const mijpeg_info &f = hosts[(size_t)i]->info;
    for (int c = 0; c < f.components; c++)
      if (memcmp(f.quant[f.quant_index[c]], f0.quant[f0.quant_index[c]], sizeof(f.quant[0]))) own_tables = true;
  }
  int rc = ensure_coef_store(d, (size_t)f0.coef_count * (size_t)n, false);
  if (rc) return rc;
  d->img_valid = d->model_valid = false;
  d->uploaded = false;
  d->decoded = false;
  d->pend_n = 0;
  rc = device_entropy_batch(d, hosts.data(), streams, sizes, n, min_intervals, d->coef_dev, f0.coef_count, false, defer);
  d->timing[0] = std::chrono::duration<double>(clk::now() - t0).count();
  d->timing[1] = std::chrono::duration<double>(t_parsed - t0).count();
  d->timing[2] = d->phase_prepare;
  d->timing[3] = d->phase_device;
  if (rc) { // (device_entropy_batch has waited for whatever it enqueued before the failure)
    d->pend_n = 0;
    return rc;
  }
  d->batch_own_tables = own_tables;
  d->batch_frames = -n; // decoded (or on its way) but not aggregated yet
  if (d->pend_n) return MIJPEG_OK; // deferred: finish_batch() waits
  return finish_batch(d);
}

static int finish_batch(mijpeg_decoder *d)
{
  const int n = d->batch_frames < 0 ? -d->batch_frames : 0;
  if (n == 0) return d->batch_frames > 0 ? MIJPEG_OK : set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "no batch has been submitted");
  d->batch_frames = 0;
  std::vector<HostDecoder *> hosts((size_t)n);
  for (int i = 0; i < n; i++) hosts[(size_t)i] = d->batch_hosts[(size_t)i].get();
  if (d->pend_n) { // wait for the upload and the Huffman kernel of the submitted batch, then look at what it reported
    const int pn = d->pend_n;
    d->pend_n = 0;
    // The pipeline's one wait on the device.  hipStreamSynchronize blocks on an interrupt after a short spin, and how long the wake-up
    // takes is the host's business (idle states of the core that takes the interrupt): on some boxes 0.3 ms per wait for seconds
    // on end -- sixteen chunks of a batch, five milliseconds (profiles/r05/batch4k_stall.txt).  A submitted batch is a
    // millisecond from done when somebody asks for it: poll the stream for that long, block only beyond.
    {
      static const bool no_spin = getenv("MIJPEG_NO_SPIN_WAIT") != nullptr; // A-B measurements
      const auto t_spin = std::chrono::steady_clock::now();
      hipError_t q = hipSuccess;
      while (!no_spin && (q = hipStreamQuery(d->stream)) == hipErrorNotReady) {
        if (std::chrono::steady_clock::now() - t_spin > std::chrono::milliseconds(4)) break;
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
      }
      // hipErrorNotReady is not an error: drop it -- and only it; anything else the query saw (a failed launch of the work it waits
      // for) is the batch's verdict
      if (q == hipErrorNotReady) (void)hipGetLastError();
      else if (q != hipSuccess) HIP_TRY(d, q);
    }
    HIP_TRY(d, hipStreamSynchronize(d->stream));
    d->phase_device += std::chrono::duration<double>(std::chrono::steady_clock::now() - d->pend_t0).count();
    if (d->pend_walk_round > 0) { // streams without restart markers: did the walk settle within the rounds it was given?
      const int rounds = d->pend_walk_round;
      d->pend_walk_round = 0;
      if (d->pend_walk_flags[rounds]) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "speculative decoding did not settle in the rounds a submitted batch gets: decode it with mijpeg_decode_batch_device");
      d->walk_rounds = walk_rounds_needed(d->pend_walk_flags, rounds);
      if (d->pend_walk_status)
        if (const int wrc = walk_verdict(d, d->pend_walk_status, pn)) return wrc;
    }
    const int rc = evaluate_entropy_status(d, hosts.data(), pn, d->pend_status);
    if (rc) return rc;
  }
  const mijpeg_info &f0 = hosts[0]->info;
  const bool own_tables = d->batch_own_tables;
  int rc = MIJPEG_OK;
  d->batch_info = f0;
  d->batch_own_tables = own_tables;
  if (own_tables) {
    // the batch's info then carries, per COMPONENT, the largest delta any image has at each position: what the range
    // gates of the kernel selection look at
    d->batch_quant_host.assign((size_t)n * 4 * 64, 1);
    mijpeg_info &bi = d->batch_info;
    for (int c = 0; c < f0.components; c++) {
      bi.quant_index[c] = (uint8_t)c;
      for (int k = 0; k < 64; k++) bi.quant[c][k] = 0;
    }
    for (int i = 0; i < n; i++) {
      const mijpeg_info &f = hosts[(size_t)i]->info;
      for (int c = 0; c < f.components; c++)
        for (int k = 0; k < 64; k++) {
          const uint16_t q = f.quant[f.quant_index[c]][k];
          d->batch_quant_host[((size_t)i * 4 + c) * 64 + k] = q;
          bi.quant[c][k] = std::max(bi.quant[c][k], q);
        }
    }
    const size_t bytes = d->batch_quant_host.size() * sizeof(uint16_t);
    rc = ensure_dev(d, (void **)&d->batch_quant_dev, &d->batch_quant_cap, bytes);
    if (rc) return rc;
    HIP_TRY(d, hipMemcpyAsync(d->batch_quant_dev, d->batch_quant_host.data(), bytes, hipMemcpyHostToDevice, d->stream));
  }
  d->batch_info.fast_arith = 1;
  for (int i = 0; i < n; i++) { // the batch is as fast as its most demanding image
    const mijpeg_info &f = hosts[(size_t)i]->info;
    if (!f.fast_arith) d->batch_info.fast_arith = 0;
    for (int c = 0; c < f.components; c++) d->batch_info.range_max[c] = std::max(d->batch_info.range_max[c], f.range_max[c]);
  }
  d->batch_frames = n;
  if (!own_tables && !d->batch_info.xt) { // the next batch of this shape may launch its reconstruction on this range check
    SpecHint &h = *spec_hint();
    std::lock_guard<std::mutex> lock(h.m);
    h.info = d->batch_info;
    h.valid = true;
  }
  return MIJPEG_OK;
}

// A speculative launch is validated: the batch is finished the ordinary way (wait, errors, range check), and where the range
// check is not the one the launch assumed the reconstruction runs again with the kernel the real one selects.
static int settle_speculation(mijpeg_decoder *d)
{
  if (!d->spec_active) return MIJPEG_OK;
  d->spec_active = false;
  d->spec_redone = false;
  if (d->batch_frames == 0) return MIJPEG_OK; // (the batch was abandoned: another stream was set on the object)
  if (d->batch_frames < 0) {
    const int rc = finish_batch(d);
    if (rc) return rc; // (the stream is damaged, the walk had not settled ...: nothing of the speculative pixels counts)
  }
  bool holds = d->batch_info.fast_arith != 0;
  for (int c = 0; c < d->batch_info.components; c++) holds = holds && d->batch_info.range_max[c] <= d->spec_assumed[c];
  if (holds) return MIJPEG_OK;
  d->spec_redone = true;
  d->spec_redone_count++;
  return mijpeg_reconstruct_batch_device(d, d->spec_dst, d->spec_frame_stride, d->spec_row_stride, d->spec_flags & ~MIJPEG_FLAG_SPECULATIVE, 1);
}

int mijpeg_decode_batch_device(mijpeg_decoder *d, const uint8_t *const *streams, const size_t *sizes, int n, int min_intervals)
try {
  return submit_batch(d, streams, sizes, n, min_intervals, false);
} catch (...) { return boundary_catch(d, "mijpeg_decode_batch_device"); }

int mijpeg_prepare_batch_host(mijpeg_decoder *d, const uint8_t *const *streams, const size_t *sizes, int n)
try {
  if (!d || !streams || !sizes || n < 1) return MIJPEG_ERR_INVALID_PARAMETER;
  if (const int prc = settle_pending(d)) return prc;
  d->batch_frames = 0;
  if (d->batch_hosts.size() < (size_t)n) d->batch_hosts.resize((size_t)n); // never shrinks: a pipeline's chunks differ in size, and
  for (auto &h : d->batch_hosts)                                         // a parser that is thrown away takes its grown vectors along
    if (!h) h.reset(new HostDecoder());
  std::vector<size_t> slot;
  const size_t total = stream_slots(sizes, n, slot);
  uint8_t *stage;
  if (d->device >= 0) {
    HIP_TRY(d, hipSetDevice(d->device));
    if (const int src = ensure_pinned(d, &d->stage_host, &d->stage_cap, total)) return src;
    stage = d->stage_host;
  } else {
    if (d->host_stage.size() < total) d->host_stage.resize(total);
    stage = d->host_stage.data();
  }
  std::vector<int> rcs((size_t)n, 0);
  const int workers = std::min(n, default_threads());
  parallel_for(workers, [&](int w) {
    for (int i = w; i < n; i += workers) {
      d->batch_hosts[(size_t)i]->set_unstuff_sink(stage + slot[(size_t)i], sizes[i]);
      rcs[(size_t)i] = d->batch_hosts[(size_t)i]->parse(streams[i], sizes[i], false);
    }
  });
  for (int i = 0; i < n; i++)
    if (rcs[(size_t)i]) return set_error(d, rcs[(size_t)i], d->batch_hosts[(size_t)i]->error.message);
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_prepare_batch_host"); }

int mijpeg_submit_batch_device(mijpeg_decoder *d, const uint8_t *const *streams, const size_t *sizes, int n, int min_intervals)
try {
  return submit_batch(d, streams, sizes, n, min_intervals, true);
} catch (...) { return boundary_catch(d, "mijpeg_submit_batch_device"); }

int mijpeg_synchronize(mijpeg_decoder *d)
try {
  if (!d) return MIJPEG_ERR_INVALID_PARAMETER;
  if (d->device < 0 || !d->stream) return MIJPEG_OK;
  HIP_TRY(d, hipSetDevice(d->device));
  HIP_TRY(d, hipStreamSynchronize(d->stream));
  if (d->spec_active) return settle_speculation(d); // (pixels of a speculative launch count once it is validated)
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_synchronize"); }

int mijpeg_stream_wait(mijpeg_decoder *d, void *client_stream)
try {
  if (!d) return MIJPEG_ERR_INVALID_PARAMETER;
  if (d->device < 0 || !d->stream) return MIJPEG_OK;
  HIP_TRY(d, hipSetDevice(d->device));
  if (!d->chain_ev) HIP_TRY(d, hipEventCreateWithFlags(&d->chain_ev, hipEventDisableTiming));
  HIP_TRY(d, hipEventRecord(d->chain_ev, d->stream));
  HIP_TRY(d, hipStreamWaitEvent((hipStream_t)client_stream, d->chain_ev, 0));
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_stream_wait"); }

int mijpeg_finish_batch_device(mijpeg_decoder *d)
try {
  if (!d) return MIJPEG_ERR_INVALID_PARAMETER;
  if (d->device >= 0) HIP_TRY(d, hipSetDevice(d->device));
  if (d->spec_active) return settle_speculation(d);
  return finish_batch(d);
} catch (...) { return boundary_catch(d, "mijpeg_finish_batch_device"); }

int mijpeg_batch_speculation(mijpeg_decoder *d, int64_t *launched, int64_t *redone)
try {
  if (!d) return MIJPEG_ERR_INVALID_PARAMETER;
  if (launched) *launched = d->spec_launched;
  if (redone) *redone = d->spec_redone_count;
  return d->spec_redone ? 1 : 0;
} catch (...) { return boundary_catch(d, "mijpeg_batch_speculation"); }

int mijpeg_reconstruct_batch_device(mijpeg_decoder *d, void *dst_device, int64_t frame_stride, int64_t row_stride, uint32_t flags, int sync)
try {
  if (!d || !dst_device) return MIJPEG_ERR_INVALID_PARAMETER;
  if (d->device >= 0) HIP_TRY(d, hipSetDevice(d->device));
  bool speculate = false;
  mijpeg_info assumed;
  if (d->batch_frames < 0 && (flags & MIJPEG_FLAG_SPECULATIVE) && !sync && d->pend_n && !d->pend_walk_round && !d->batch_own_tables && !d->spec_active) {
    // A submitted batch whose Huffman kernel may still be running: launch the reconstruction behind it on the range check the
    // last batch of this shape and these tables reported (rounded up to the selection's next gate) instead of waiting for this
    // one's.  The pipeline's host thread never blocks on the device; mijpeg_finish_batch_device validates.
    const mijpeg_info &f0 = d->batch_hosts[0]->info;
    SpecHint &h = *spec_hint();
    std::lock_guard<std::mutex> lock(h.m);
    if (h.valid && h.info.fast_arith && same_shape_and_tables(h.info, f0)) {
      assumed = f0;
      assumed.fast_arith = 1;
      speculate = true;
      for (int c = 0; c < f0.components; c++) {
        assumed.range_max[c] = next_gate_below(h.info.range_max[c]);
        if (assumed.range_max[c] < 0) speculate = false;
      }
    }
  }
  if (d->batch_frames < 0 && !speculate) { // submitted with mijpeg_submit_batch_device: wait for it now
    const int rc = d->spec_active ? settle_speculation(d) : finish_batch(d);
    if (rc) return rc;
  }
  if (d->batch_frames < 1 && !speculate) return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "no decoded batch: call mijpeg_decode_batch_device first");
  mijpeg_batch b;
  memset(&b, 0, sizeof(b));
  b.info = speculate ? assumed : d->batch_info;
  b.coef_dev = d->coef_dev;
  b.coef_frame_stride = b.info.coef_count;
  b.out_dev = (uint8_t *)dst_device;
  b.out_row_stride = row_stride;
  b.out_frame_stride = frame_stride;
  b.frames = speculate ? -d->batch_frames : d->batch_frames;
  b.quant_dev = d->batch_own_tables ? d->batch_quant_dev : nullptr;
  b.flags = flags & ~(MIJPEG_FLAG_DEVICE_OUTPUT | MIJPEG_FLAG_NO_UPSAMPLING | MIJPEG_FLAG_SPECULATIVE);
  const size_t ws = mijpeg_workspace_bytes(&b);
  if (ws) {
    const int rc = ensure_dev(d, (void **)&d->ws_dev, &d->ws_cap, ws);
    if (rc) return rc;
    b.workspace = d->ws_dev;
    b.workspace_bytes = d->ws_cap;
  }
  const int rc = mijpeg_launch_reconstruct(&b, d->stream);
  if (rc) return set_error(d, rc, rc == MIJPEG_ERR_DEVICE ? std::string("kernel launch failed: ") + hipGetErrorString(hipGetLastError())
                                                           : std::string("reconstruction not available for this batch"));
  if (speculate) {
    d->spec_active = true;
    d->spec_redone = false;
    d->spec_dst = dst_device;
    d->spec_frame_stride = frame_stride;
    d->spec_row_stride = row_stride;
    d->spec_flags = flags;
    for (int c = 0; c < MIJPEG_MAX_COMPONENTS; c++) d->spec_assumed[c] = assumed.range_max[c];
    d->spec_launched++;
    return MIJPEG_OK;
  }
  if (sync) HIP_TRY(d, hipStreamSynchronize(d->stream));
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_reconstruct_batch_device"); }

const int16_t *mijpeg_device_coefficients(mijpeg_decoder *d) { return (d && d->uploaded) ? d->coef_dev : nullptr; }

int mijpeg_last_error(mijpeg_decoder *d, const char **message)
try {
  if (!d) return MIJPEG_ERR_INVALID_PARAMETER;
  if (message) *message = d->err_code ? d->err_msg.c_str() : nullptr;
  return d->err_code;
} catch (...) { return boundary_catch(d, "mijpeg_last_error"); }

mijpeg_decoder *mijpeg_alpha_channel(mijpeg_decoder *d)
try {
  if (!d) return nullptr;
  if (d->decoded && !d->alpha_ready && d->alpha_refusal) { // (what the reference reports at the first request for alpha pixels)
    set_error(d, d->alpha_refusal, d->alpha_refusal_msg);
    return nullptr;
  }
  if (!d->decoded || !d->alpha_ready) {
    set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "the decoded stream has no alpha channel");
    return nullptr;
  }
  return d->alpha;
} catch (...) { (void)boundary_catch(d, "mijpeg_alpha_channel"); return nullptr; }

int mijpeg_has_alpha(mijpeg_decoder *d)
try {
  return d && d->decoded && d->alpha_ready ? 1 : 0; // (a query: leaves the object's last error alone)
} catch (...) { return boundary_catch(d, "mijpeg_has_alpha"); }

int mijpeg_alpha_info(mijpeg_decoder *d, int32_t *mode, int32_t matte[3])
try {
  if (!d) return MIJPEG_ERR_INVALID_PARAMETER;
  if (!d->decoded || !d->alpha_ready) return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "the decoded stream has no alpha channel");
  if (mode) *mode = d->host.alpha_mode();
  for (int k = 0; k < 3 && matte; k++) matte[k] = (int32_t)d->host.alpha_matte()[k];
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_alpha_info"); }

int mijpeg_last_warning(mijpeg_decoder *d, const char **message)
try {
  if (message) *message = nullptr;
  if (!d || !d->data) return 0;
  return d->host.last_warning(message);
} catch (...) { return boundary_catch(d, "mijpeg_last_warning"); }

int mijpeg_last_timing(mijpeg_decoder *d, double out_seconds[4])
try {
  if (!d || !out_seconds) return MIJPEG_ERR_INVALID_PARAMETER;
  for (int i = 0; i < 4; i++) out_seconds[i] = d->timing[i];
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_last_timing"); }

// ------------------------------------------------------------------------------------------------
// stateless batch launch
// ------------------------------------------------------------------------------------------------
static Sampling sampling_of(const mijpeg_info &f)
{
  if (f.components == 1) return Sampling::GREY;
  if (f.components != 3 || f.hsamp[1] != 1 || f.vsamp[1] != 1 || f.hsamp[2] != 1 || f.vsamp[2] != 1) return Sampling::OTHER;
  const int h = f.hsamp[0], v = f.vsamp[0];
  return h == 2 && v == 2 ? Sampling::S420 : h == 2 && v == 1 ? Sampling::S422 : h == 1 && v == 2 ? Sampling::S440
         : h == 4 && v == 1 ? Sampling::S411 : h == 1 && v == 1 ? Sampling::S444 : Sampling::OTHER;
}

// The fused kernels address inside a frame with 32-bit byte offsets (planes and pixels; frames are 64 bits apart): frames
// beyond that -- a 65535 x 65535 picture has 8.6 GB of luma coefficients and 12.9 GB of pixels -- take the generic kernels,
// whose addressing is 64 bits wide throughout.
// DNL frames (mijpeg_info::dnl): the vertical filter of a subsampled component reads the line below the picture's last one,
// and when the picture ends on a block row boundary that line belongs to the block row the first scan creates behind the
// picture -- unless it met the marker before it got there.  Then the row does not exist, the reference reads NULL and
// transforms it to samples of value 0 (control/blockbitmaprequester.cpp:1097-1108, dct/idct.cpp:336-338): no coefficients
// give that, the unfused kernels write the zeros themselves (GenericArgs::zero_from).
static bool dnl_row_missing(const mijpeg_info &f)
{
  if (!f.dnl) return false;
  for (int c = 0; c < f.components && c < MIJPEG_MAX_COMPONENTS; c++) {
    const int ch = (f.height + f.suby[c] - 1) / f.suby[c];
    if (f.suby[c] > 1 && (ch & 7) == 0 && f.rows[c] <= (ch >> 3)) return true;
  }
  return false;
}

static bool fits32(const mijpeg_batch *b)
{
  const mijpeg_info &f = b->info;
  const uint64_t lim = 0xffffffffull;
  if (f.coef_wide) return false; // int32 coefficients (damaged stream): the unfused kernels' business
  if (dnl_row_missing(f)) return false; // (the fused kernels have no way to say "this block row is NULL")
  for (int c = 0; c < f.components; c++)
    if ((uint64_t)f.blocks_w[c] * (uint64_t)f.blocks_h[c] * 128u > lim) return false;
  if (f.xt && b->xt)
    for (int c = 0; c < b->xt->residual.components; c++)
      if ((uint64_t)b->xt->residual.blocks_w[c] * (uint64_t)b->xt->residual.blocks_h[c] * 128u > lim) return false;
  if (b->out_row_stride < 0) return false; // bottom-up bitmaps: the offsets are unsigned
  // (a batch description without strides -- mijpeg_kernel_name, mijpeg_workspace_bytes asked ahead of time -- is taken to
  // have tightly packed lines)
  const uint64_t line = (uint64_t)f.width * (uint64_t)f.components * (f.xt ? (uint64_t)(f.sample_bytes > 1 ? 2 : 1) : f.precision > 8 ? 2u : 1u);
  const uint64_t rs = b->out_row_stride ? (uint64_t)b->out_row_stride : line;
  return (uint64_t)f.height * rs + line <= lim;
}

// every delta << 4 a signed 16-bit operand (the fast transforms)
static bool deltas_fit16(const mijpeg_info &f)
{
  if (f.components > MIJPEG_MAX_COMPONENTS) return false;
  for (int c = 0; c < f.components; c++) {
    if ((unsigned)f.quant_index[c] >= 4) return false;
    for (int i = 0; i < 64; i++)
      if (f.quant[f.quant_index[c]][i] > 2047) return false;
  }
  return true;
}

// The 12-bit kernels' colour stage in one 32-bit sum per channel (colour12<true>, kernels.hip): the luma sample times 16 is at most
// 4.02 * range_max[0] + 2 in magnitude, a chroma sample behind the upsampling filters 4.02 * range_max[c] + 4 (the bounds of
// the 12-bit gate of plan_reconstruct; the filters are convex combinations plus a rounding), so (|y'| + 32776) * 8192 + 14516 |c| --
// 14516 is the largest weight a channel puts on chroma, 2819 + 5850 the green one's -- stays below 2^31 where this holds.  Monotone
// in every range: a speculative launch that assumed larger ranges and selected the flavour holds for the smaller ones.
static bool narrow12_colour(const mijpeg_info &f)
{
  if (f.precision != 12 || f.components != 3) return false;
  const int64_t ry = f.range_max[0], rc = std::max(f.range_max[1], f.range_max[2]);
  if (ry <= 0 || rc < 0) return false;
  const int64_t sum = ((402 * ry + 99) / 100 + 2 + 32776) * 8192 + 14516 * ((402 * rc + 99) / 100 + 4);
  return sum < ((int64_t)1 << 31);
}

// JPEG XT: the L transformation in force for this launch.  A request without colour transformation (the command line's -c)
// replaces the STANDARD YCbCr transformation by the identity and leaves everything else of the merge alone
// (colortrafo/colortransformerfactory.cpp:231-232: `if (ltrafo == YCbCr && disabletorgb) ltrafo = Identity`)
static bool xt_ltrafo_ycbcr(const mijpeg_batch *b)
{
  const mijpeg_xt_params &x = *b->xt;
  return x.ltrafo_ycbcr && !((b->flags & MIJPEG_FLAG_NO_COLOR_TRANSFORM) && x.ltrafo_standard);
}

// JPEG XT profile C in the shape the fused kernels cover (the legacy frame's part is plan_reconstruct's): 12-bit 4:4:4
// residual frame of the legacy frame's size, L transformation on, the residual frame within the range the fast transforms
// are exact for
static bool fused_xt_shape(const mijpeg_batch *b)
{
  const mijpeg_xt_params &x = *b->xt;
  const mijpeg_info &r = x.residual;
  if (x.general) return false; // free-form matrices, table gathers, DCT bypass: xt_merge_general_kernel
  if (x.no_residual) return false; // (a legacy codestream without its EOI: the unfused merge kernels know how to merge nothing)
  // hidden bits in the RESIDUAL frame (-rR n: 13..16-bit samples, int32 coefficients) have a kernel of their own
  // (fusedxtw420_kernel); hidden bits in the legacy frame change its precision and stay on the three-kernel path
  if (x.hidden_bits || x.residual_hidden_bits < 0 || x.residual_hidden_bits > 4 || (x.residual_wide != 0) != (x.residual_hidden_bits > 0) ||
      x.ltable_entries != 256 || !xt_ltrafo_ycbcr(b) || r.precision != 12 || r.components != 3 || x.out_max != 65535 || x.out_shift != 32768)
    return false;
  for (int c = 0; c < 3; c++)
    if (r.subx[c] != 1 || r.suby[c] != 1 || r.blocks_w[c] != r.blocks_w[0] || r.blocks_h[c] != r.blocks_h[0] || r.range_max[c] >= GATE_XT_RESIDUAL)
      return false;
  return deltas_fit16(r) && r.width == b->info.width && r.height == b->info.height;
}

// Which kernel reconstructs a batch, and in which flavour: the one place that decides it (mijpeg_kernel_name,
// mijpeg_workspace_bytes and launch_reconstruct_ex each ask once).  Safe on any batch description, a JPEG XT frame without
// its parameter block and a batch without strides included.  (A rectangle request needs MIJPEG_FLAG_FORCE_GENERIC, which
// alone rules out the fused, flat and tile kernels.)
static ReconPlan plan_reconstruct(const mijpeg_batch *b)
{
  const mijpeg_info &f = b->info;
  const int32_t *r = f.range_max;
  const bool generic = b->flags & MIJPEG_FLAG_FORCE_GENERIC, safe = b->flags & MIJPEG_FLAG_FORCE_SAFE;
  const bool ycc = f.ycbcr && !(b->flags & MIJPEG_FLAG_NO_COLOR_TRANSFORM); // (the fused three-component kernels transform colour)
  const bool deltas16 = deltas_fit16(f); // (false for more components than a frame can have)
  const auto chroma_below = [&](int32_t gate) { return r[1] < gate && r[2] < gate; };
  ReconPlan p{};
  p.sampling = sampling_of(f);
  p.fast = f.fast_arith && !safe && !f.coef_wide && deltas16;
  const auto plan = [&](Recon k) { p.kernel = k; return p; };
  if (f.xt) {
    // (fast_arith itself is never set for XT frames: the generic kernels run SAFE on them; the fused ones check the range here)
    if (b->xt && p.sampling == Sampling::S420 && f.precision == 8 && !generic && !safe && deltas16 && r[0] < GATE_XT_LEGACY &&
        chroma_below(GATE_XT_LEGACY) && fits32(b) && fused_xt_shape(b))
      return plan(b->xt->residual_hidden_bits ? Recon::FUSEDXTW420 : Recon::FUSEDXT420);
    if (f.coef_wide) return plan(Recon::PAIR_LONG);
    if (f.components == 1) return plan(Recon::XT_MERGE1);
    return plan(b->xt && b->xt->general ? Recon::XT_MERGE_GENERAL : Recon::XT_MERGE);
  }
  if (f.coef_wide) return plan(Recon::PAIR_LONG); // int32 coefficients (damaged stream)
  const bool fits = f.components >= 1 && f.components <= MIJPEG_MAX_COMPONENTS && fits32(b); // (no missing DNL row either)
  if (fits && !generic && f.precision == 8) {
    // single components: samples travel as packed int16
    if (p.sampling == Sampling::GREY && p.fast && r[0] < GATE_FUSED8) return plan(Recon::FUSED1);
    // 4:2:0 in any range; the packed flavour filters (Cb, Cr) pairs in 16 bits: every chroma sample * 16 is bounded by
    // 4 * range_max, and the filter sums a + 3 b + r by four times that.  Where the first-pass results of every transform fit
    // 16 bits its second pass runs on v_dot2 as well (MIJPEG_FLAG_FORCE_DOT2, for testing: whatever the range check says).
    if (p.sampling == Sampling::S420 && ycc) {
      if (!p.fast || !chroma_below(GATE_PACKED)) return plan(Recon::FUSED420);
      p.dot2 = !b->quant_dev && ((b->flags & MIJPEG_FLAG_FORCE_DOT2) || (r[0] < GATE_DOT2 && chroma_below(GATE_DOT2)));
      return plan(Recon::FUSED420P);
    }
    // 4:2:2, 4:4:0 (what a losslessly rotated 4:2:2 picture is), 4:1:1, 4:4:4: chroma samples travel through LDS as int16 pairs
    // (4 * range_max < 32768); 4:2:2 and 4:4:0 filter on the pairs below the packed gate, on 32-bit values between the two
    if (p.sampling != Sampling::GREY && p.sampling != Sampling::OTHER && ycc && p.fast && chroma_below(GATE_FUSED8)) {
      const Sampling s = p.sampling;
      p.wide = (s == Sampling::S422 || s == Sampling::S440) && !chroma_below(GATE_PACKED);
      return plan(s == Sampling::S422 ? Recon::FUSED422 : s == Sampling::S440 ? Recon::FUSED440 : s == Sampling::S411 ? Recon::FUSED411 : Recon::FUSED444);
    }
  }
  // 12 bit (SOF1, P = 12): 4:2:0, 4:2:2, 4:4:4 and single components inside the ranges the 12-bit flavours are exact for: every
  // delta << 4 a signed 16-bit operand; sum |c| q < 49152 bounds every butterfly intermediate by 1573 * 16 * 49152 < 2^31 (first
  // pass; the second pass sees at most 22.2 * range_max per column) and every multiplicand by 2^23; chroma sum |c| q < 45056 bounds
  // the chroma samples (times 16) by 4.02 * 45056 + 2 < 181 200 (|basis| <= 1/4 per coefficient, the 9-bit constants and the
  // roundings add < 0.5 %), whose products with the colour constants (11485; 2819 + 5850; 14516 taken as 4 * 3629) fit 32 bits.
  // (The horizontal filter of 4:2:2 weighs samples below 2^18 with 4 in total.)
  if (fits && !generic && f.precision == 12 && !safe && deltas16 && r[0] > 0 && r[0] < GATE_12_LUMA) {
    if (p.sampling == Sampling::GREY) return plan(Recon::FUSED1_12);
    const Sampling s = p.sampling;
    if ((s == Sampling::S420 || s == Sampling::S422 || s == Sampling::S444) && ycc && chroma_below(GATE_12_CHROMA)) {
      p.narrow12 = narrow12_colour(f);
      return plan(s == Sampling::S420 ? Recon::FUSED420_12 : s == Sampling::S422 ? Recon::FUSED422_12 : Recon::FUSED444_12);
    }
  }
  // every component 1 x 1, three or four of them, 8 bit, no colour transformation, fast arithmetic: fused_flat_kernel
  // (CMYK; RGB stored as such -- Adobe transform 0, a merging specification with the identity L transformation, the caller's
  // MIJPEG_FLAG_NO_COLOR_TRANSFORM on a 4:4:4 frame)
  bool flat = f.precision == 8 && !b->quant_dev && !generic && (f.components == 4 || (f.components == 3 && !ycc)) && p.fast && fits;
  for (int c = 0; c < f.components && flat; c++)
    flat = f.subx[c] == 1 && f.suby[c] == 1 && f.blocks_w[c] == f.blocks_w[0] && f.blocks_h[c] == f.blocks_h[0];
  if (flat) return plan(Recon::FLAT);
  // plain JPEG frames of any layout go through LDS in one pass (fused_tile_kernel); the pair with its sample planes in HBM
  // stays for per-frame tables in device memory, MIJPEG_FLAG_FORCE_GENERIC (rectangle requests) and missing DNL rows
  if (b->quant_dev || generic || dnl_row_missing(f)) return plan(Recon::PAIR);
  // 12-bit frames of the tile kernel: the bounds of the 12-bit gate above, the chroma one for every component (the upsampling
  // filters weigh two samples, < 2^18 each with the level shift, with at most 8 in total: far inside the fast flavour's 24-bit
  // operands and 32-bit sums)
  p.fast12 = f.precision == 12 && !safe && deltas16 && r[0] > 0;
  for (int c = 0; c < f.components && p.fast12; c++) p.fast12 = r[c] < GATE_12_CHROMA;
  return plan(Recon::TILE);
}

// per Recon: the name, and that of the flavour (ReconPlan::wide, ReconPlan::narrow12) where the kernel has one
static const char *const RECON_NAMES[][2] = {
    {"fused420p_kernel", nullptr},
    {"fused420_kernel", nullptr},
    {"fused422_kernel", "fused422_kernel<wide>"},
    {"fused440_kernel", "fused440_kernel<wide>"},
    {"fused411_kernel", nullptr},
    {"fused444_kernel", nullptr},
    {"fused1_kernel", nullptr},
    {"fused420_kernel<12>", "fused420_kernel<12>/narrow"},
    {"fused422_12_kernel", "fused422_12_kernel/narrow"},
    {"fused444_12_kernel", "fused444_12_kernel/narrow"},
    {"fused1_kernel<12>", nullptr},
    {"fusedxt420_kernel", nullptr},
    {"fusedxtw420_kernel", nullptr},
    {"fused_flat_kernel", nullptr},
    {"fused_tile_kernel", nullptr},
    {"idct_planes_kernel+upsample_color_kernel", nullptr},
    {"idct_planes_long_kernel+upsample_color_kernel", nullptr},
    {"idct_planes_kernel+xt_merge_kernel", nullptr},
    {"idct_planes_kernel+xt_merge_general_kernel", nullptr},
    {"idct_planes_kernel+xt_merge1_kernel", nullptr},
};
static_assert(sizeof(RECON_NAMES) / sizeof(RECON_NAMES[0]) == (size_t)Recon::XT_MERGE1 + 1, "one name per kernel");

const char *mijpeg_kernel_name(const mijpeg_batch *b)
try {
  if (!b) return "";
  const ReconPlan p = plan_reconstruct(b);
  return RECON_NAMES[(int)p.kernel][p.wide || p.narrow12 ? 1 : 0];
} catch (...) { (void)boundary_catch(nullptr, "mijpeg_kernel_name"); return nullptr; }

static const size_t LUT_BYTES = 3 * 4096 * sizeof(int32_t);

// JPEG XT with real Q / R2 tables (mijpeg_xt_params.general): they travel in the workspace behind everything else
static size_t xt_table_bytes(const mijpeg_batch *b)
{
  if (!b->info.xt || !b->xt || !b->xt->general) return 0;
  size_t n = 0;
  for (int c = 0; c < 3; c++) {
    if (b->xt->qtable[c]) n += (size_t)b->xt->qtable_entries * sizeof(int32_t);
    if (b->xt->r2table[c]) n += ((size_t)(b->xt->out_max + 1) << 4) * sizeof(int32_t);
  }
  return n;
}

// per-frame tables (quant_dev) are expanded to the transforms' operands (deltas << 4, int32) in the workspace
static size_t expanded_tables_bytes(const mijpeg_batch *b) { return b->quant_dev ? (size_t)b->frames * 4 * 64 * sizeof(int32_t) : 0; }

static bool is_fused_xt(Recon k) { return k == Recon::FUSEDXT420 || k == Recon::FUSEDXTW420; }

static size_t workspace_need(const mijpeg_batch *b, const ReconPlan &p)
{
  if (is_fused_xt(p.kernel)) return LUT_BYTES;
  if (p.kernel < Recon::FUSEDXT420) return expanded_tables_bytes(b);
  // [LUT_BYTES: L lookup tables (JPEG XT, up to 3 x 4096 entries)] [per frame: int32 sample planes, one sample per
  // coefficient: coef_count of them, fewer when the residual planes hold 32-bit coefficients] [expanded per-frame tables]
  // [JPEG XT tables]
  return LUT_BYTES + (size_t)b->info.coef_count * sizeof(int32_t) * (size_t)b->frames + expanded_tables_bytes(b) + xt_table_bytes(b);
}

size_t mijpeg_workspace_bytes(const mijpeg_batch *b)
try {
  return b ? workspace_need(b, plan_reconstruct(b)) : 0;
} catch (...) { (void)boundary_catch(nullptr, "mijpeg_workspace_bytes"); return 0; }

// What a rectangle request that does not show the plain picture adds to a launch (request_model.hpp; GenericArgs::rowmap ...)
struct RequestExtra {
  const int32_t *rowmap_dev;
  int32_t rowmap_stride;
  int32_t corner_x, corner_y, y_base, y_count;
  int32_t wstart[MAXP], wlimit[MAXP]; // per plane (JPEG XT: legacy planes, then residual planes)
  int32_t ycc;
};
static int launch_reconstruct_ex(const mijpeg_batch *b, void *stream, const RequestExtra *rx);

int mijpeg_launch_reconstruct(const mijpeg_batch *b, void *stream)
try {
  return launch_reconstruct_ex(b, stream, nullptr);
} catch (...) { return boundary_catch(nullptr, "mijpeg_launch_reconstruct"); }

static int launch_reconstruct_ex(const mijpeg_batch *b, void *stream, const RequestExtra *rx)
{
  if (!b || !b->coef_dev || !b->out_dev || b->frames < 1) return MIJPEG_ERR_INVALID_PARAMETER;
  if (rx && !(b->flags & MIJPEG_FLAG_FORCE_GENERIC)) return MIJPEG_ERR_INVALID_PARAMETER;
  if (b->quant_dev && b->info.xt) return MIJPEG_ERR_OPERATION_UNIMPLEMENTED; // per-frame tables: plain JPEG only
  const mijpeg_info &f = b->info;
  if ((f.precision != 8 && f.precision != 12) || f.components < 1 || f.components > 4) return MIJPEG_ERR_OPERATION_UNIMPLEMENTED;
  if (f.xt && (!b->xt || (f.components != 3 && f.components != 1))) return MIJPEG_ERR_MISSING_PARAMETER; // (one component: grey scale with a residual)
  if (f.coef_wide && (f.xt || b->quant_dev)) return MIJPEG_ERR_INVALID_PARAMETER; // int32 planes: single plain JPEG frames only
  const ReconPlan p = plan_reconstruct(b);
  const size_t need = workspace_need(b, p);
  if (need && (!b->workspace || b->workspace_bytes < need)) return MIJPEG_ERR_MISSING_PARAMETER;
  hipStream_t s = (hipStream_t)stream;
  int rc;
  const int32_t *qdev = nullptr;
  if (b->quant_dev) {
    int32_t *dst = (int32_t *)((char *)b->workspace + (need - expanded_tables_bytes(b) - xt_table_bytes(b)));
    if (launch_expand_deltas(b->quant_dev, dst, b->frames, s)) return MIJPEG_ERR_DEVICE;
    qdev = dst;
  }
  if (p.kernel <= Recon::FUSEDXTW420) {
    FusedXtArgs xa;
    memset(&xa, 0, sizeof(xa));
    Fused420Args &a = xa.base;
    a.coef = b->coef_dev;
    a.coef_frame_stride = b->coef_frame_stride;
    a.off_y = f.coef_offset[0];
    a.off_cb = f.coef_offset[1];
    a.off_cr = f.coef_offset[2];
    a.out = b->out_dev;
    a.out_frame_stride = b->out_frame_stride;
    a.row_stride = b->out_row_stride;
    a.width = f.width;
    a.height = f.height;
    a.bw_y = f.blocks_w[0];
    a.bh_y = f.blocks_h[0];
    a.bw_c = f.blocks_w[1];
    a.bh_c = f.blocks_h[1];
    const bool full_height = p.sampling == Sampling::S422 || p.sampling == Sampling::S411; // (chroma subsampled horizontally only)
    a.cw = p.sampling == Sampling::S440 ? f.width : p.sampling == Sampling::S411 ? (f.width + 3) / 4 : (f.width + 1) / 2;
    a.ch = full_height ? f.height : (f.height + 1) / 2;
    // DNL frames: the reference's upsamplers never learnt the height (upsampling/upsamplerbase.cpp:61-75), their line buffers
    // have no bottom edge: below the last chroma line comes what the block rows hold (the padding of the last one, then the
    // MCU row the first scan created behind the picture: the store has it, include/mijpeg.h) instead of that line again
    if (f.dnl && !full_height && f.components > 1) a.ch = a.bh_c * 8;
    a.tiles_x = (f.width + 127) / 128;
    a.tiles_y = (f.height + 127) / 128;
    a.frames = b->frames;
    for (int c = 0; c < 3; c++)
      fill_deltas(a.q[c], f.quant[f.quant_index[c]]);
    a.qdev = qdev;
    if (is_fused_xt(p.kernel)) {
      const mijpeg_xt_params &x = *b->xt;
      const mijpeg_info &r = x.residual;
      for (int c = 0; c < 3; c++) {
        xa.ext.off_r[c] = r.coef_offset[c];
        for (int i = 0; i < 64; i++) xa.ext.rq[c][i] = (int32_t)r.quant[r.quant_index[c]][i] << 4;
        if (hipMemcpyAsync((int32_t *)b->workspace + (size_t)c * 256, x.ltable[c], 256 * sizeof(int32_t), hipMemcpyHostToDevice, s) != hipSuccess)
          return MIJPEG_ERR_DEVICE;
      }
      xa.ext.bw_r = r.blocks_w[0];
      xa.ext.bh_r = r.blocks_h[0];
      xa.ext.ltable = (const int32_t *)b->workspace;
      xa.ext.rtrafo_ycbcr = x.rtrafo_ycbcr;
      xa.ext.is_float = x.is_float;
      xa.ext.out_max = x.out_max;
      xa.ext.out_shift = x.out_shift;
      xa.ext.rprecision = r.precision + x.residual_hidden_bits;
      // (the two-wave flavour of the hidden-bit kernel keeps the luma block as int16: sample * 16 + 2056 with |sample * 16| <= 4 sum |c| q)
      xa.luma_fits16 = f.range_max[0] < GATE_INT16_SAMPLES ? 1 : 0;
    }
    rc = launch_fused(p, xa, s);
  } else {
    GenericArgs a;
    memset(&a, 0, sizeof(a));
    a.coef = b->coef_dev;
    a.coef_frame_stride = b->coef_frame_stride;
    a.samples = (int32_t *)((char *)b->workspace + LUT_BYTES);
    a.sample_frame_stride = f.coef_count;
    a.out = b->out_dev;
    a.out_frame_stride = b->out_frame_stride;
    a.row_stride = b->out_row_stride;
    a.width = f.width;
    a.height = f.height;
    a.ncomp = f.components;
    a.ycbcr = (f.ycbcr && !(b->flags & MIJPEG_FLAG_NO_COLOR_TRANSFORM)) ? 1 : 0;
    a.frames = b->frames;
    a.qdev = qdev;
    a.nplanes = f.components;
    a.sample_bytes = f.xt ? (b->xt->out_max > 255 ? 2 : 1) : f.precision > 8 ? 2 : 1;
    a.maxval = (1 << f.precision) - 1;
    a.dcshift = (1 << (f.precision - 1)) << 4;
    int64_t sample_off = 0;
    auto plane = [&](int p, const mijpeg_info &g, int c, int precision) {
      a.coef_off[p] = g.coef_offset[c];
      a.sample_off[p] = sample_off;
      sample_off += (int64_t)g.blocks_w[c] * g.blocks_h[c] * 64;
      a.bw[p] = g.blocks_w[c];
      a.bh[p] = g.blocks_h[c];
      a.subx[p] = g.subx[c];
      a.suby[p] = g.suby[c];
      a.cw[p] = (g.width + g.subx[c] - 1) / g.subx[c];
      a.ch[p] = (g.height + g.suby[c] - 1) / g.suby[c];
      if (g.dnl && g.suby[c] > 1) { // no bottom edge, see above; rows nobody created are NULL: zeros
        if ((a.ch[p] & 7) == 0 && g.rows[c] <= (a.ch[p] >> 3)) a.zero_from[p] = g.rows[c];
        a.ch[p] = g.blocks_h[c] * 8;
      }
      a.dcoff[p] = (1 << (precision - 1)) << 7;
      fill_deltas(a.q[p], g.quant[g.quant_index[c]]);
    };
    // JPEG XT frames reconstruct at their precision plus the bits that travelled in hidden refinement scans
    // (Frame::HiddenPrecisionOf, marker/frame.cpp:368-373)
    const int lprec = f.precision + (f.xt ? b->xt->hidden_bits : 0);
    for (int c = 0; c < f.components; c++) plane(c, f, c, lprec);
    if (f.coef_wide) { a.wide_first = 0; a.wide_count = f.components; a.wide_long = 1; }
    // int16 sample planes between the two kernels: |sample * 16| <= 2048 (level shift) + 4 * range_max must fit 16 bits
    a.narrow = p.fast && !f.xt && f.precision == 8;
    for (int c = 0; c < f.components && a.narrow; c++)
      if (f.range_max[c] >= GATE_INT16_SAMPLES) a.narrow = 0;
    a.maxval = (1 << lprec) - 1;
    a.dcshift = (1 << (lprec - 1)) << 4;
    if (f.xt) {
      const mijpeg_xt_params &x = *b->xt;
      const int rprec = x.residual.precision + x.residual_hidden_bits;
      // (a parameter block filled in before the lossless flavours existed has zeros there: with clamping that means four bits)
      const int xrbits = (x.rbits == 0 && x.clamp) ? 4 : x.rbits;
      if (x.hidden_bits < 0 || x.hidden_bits > 4 || x.residual_hidden_bits < 0 || x.residual_hidden_bits > 4 || rprec - (x.rct ? 1 : 0) > 16 ||
          x.ltable_entries != (256 << x.hidden_bits) || (x.residual_wide != 0) != (x.residual_hidden_bits > 0 || x.residual.precision > 12) ||
          (xrbits != 4 && !(x.general && x.rdct_bypass)) || (x.rct && (x.clamp || xrbits != 1)) || (!x.clamp && !x.general))
        return MIJPEG_ERR_INVALID_PARAMETER;
      // the flavours without clamping (RCT, lossless identity) index their Q tables directly: a caller-made block without them is refused
      if ((x.rct || !x.clamp) && !x.no_residual)
        for (int c = 0; c < x.residual.components && c < 3; c++)
          if (!x.qtable[c]) return MIJPEG_ERR_INVALID_PARAMETER;
      for (int c = 0; c < x.residual.components && c < 3; c++) plane(3 + c, x.residual, c, rprec); // (one component: planes 4, 5 stay empty)
      if (!x.residual.components) // (no residual frame at all -- a specification without a residual codestream: the merge reads nothing there)
        for (int pn = 3; pn < 6; pn++) a.subx[pn] = a.suby[pn] = 1;
      // int32 planes: beyond 12 bits (hidden bits included) the reference transforms with IDCT<4,QUAD>, up to 12 with the LONG
      // flavour like every other frame (codestream/tables.cpp:1876-1891) -- the same numbers until a damaged scan leaves a
      // coefficient that overflows 32 bits on the way (an 8-bit alpha residual with one hidden bit and 52 241 in a block:
      // tools/xt_gpu_damage_campaign.py, seed 2002)
      if (x.residual_wide) { a.wide_first = 3; a.wide_count = 3; a.wide_long = rprec <= 12 ? 1 : 0; }
      a.ltable_entries = x.ltable_entries;
      a.nplanes = 6;
      a.xt = 1;
      a.ycbcr = xt_ltrafo_ycbcr(b) ? 1 : 0; // the L transformation of the merging specification, or the identity the -c switch puts in its place
      a.rtrafo_ycbcr = x.rtrafo_ycbcr;
      a.out_shift = x.out_shift;
      a.out_max = x.out_max;
      a.is_float = x.is_float;
      a.rprecision = rprec;
      a.xt_no_residual = x.no_residual;
      a.xt_rct = x.rct;
      a.xt_noclamp = x.clamp ? 0 : 1;
      a.xt_rbits = x.residual.components ? xrbits : 4;
      a.legacy32 = lprec == 8 && f.range_max[0] < GATE_XT_LEGACY && f.range_max[1] < GATE_XT_LEGACY && f.range_max[2] < GATE_XT_LEGACY &&
                   !(b->flags & MIJPEG_FLAG_FORCE_SAFE);
      a.ltable = (const int32_t *)b->workspace;
      for (int c = 0; c < 3; c++)
        if (hipMemcpyAsync((int32_t *)b->workspace + (size_t)c * x.ltable_entries, x.ltable[c], (size_t)x.ltable_entries * sizeof(int32_t),
                           hipMemcpyHostToDevice, s) != hipSuccess)
          return MIJPEG_ERR_DEVICE;
      if (x.general) {
        if (x.residual.components && x.qtable_entries != (1 << (rprec - (xrbits == 1) + xrbits))) return MIJPEG_ERR_INVALID_PARAMETER; // (no residual frame: no Q tables)
        a.xt_general = 1;
        a.rbypass = x.rdct_bypass;
        a.rnoise = x.noise_shaping;
        a.rdcshift = (1 << rprec) >> 1;
        memcpy(a.lmat, x.lmat, sizeof(a.lmat));
        memcpy(a.rmat, x.rmat, sizeof(a.rmat));
        memcpy(a.cmat, x.cmat, sizeof(a.cmat));
        char *tp = (char *)b->workspace + (need - xt_table_bytes(b));
        for (int c = 0; c < 3; c++) {
          // only the highest-frequency delta is used, with the colour bits folded in (residualblockhelper.cpp:351-364)
          // (m_usQuantization is a UWORD: deltas >= 4096 wrap; shifted where the path has more than one fractional bit)
          a.rquant63[c] = xrbits > 1 ? ((int32_t)x.residual.quant[x.residual.quant_index[c]][63] << xrbits) & 0xffff : (int32_t)x.residual.quant[x.residual.quant_index[c]][63];
          // (components that share a table share its copy)
          for (int j = 0; j < c; j++) {
            if (x.qtable[c] && x.qtable[j] == x.qtable[c]) a.qlut[c] = a.qlut[j];
            if (x.r2table[c] && x.r2table[j] == x.r2table[c]) a.r2lut[c] = a.r2lut[j];
          }
          if (x.qtable[c] && !a.qlut[c]) {
            const size_t n = (size_t)x.qtable_entries * sizeof(int32_t);
            if (hipMemcpyAsync(tp, x.qtable[c], n, hipMemcpyHostToDevice, s) != hipSuccess) return MIJPEG_ERR_DEVICE;
            a.qlut[c] = (const int32_t *)tp;
            tp += n;
          }
          if (x.r2table[c] && !a.r2lut[c]) {
            const size_t n = ((size_t)(x.out_max + 1) << 4) * sizeof(int32_t);
            if (hipMemcpyAsync(tp, x.r2table[c], n, hipMemcpyHostToDevice, s) != hipSuccess) return MIJPEG_ERR_DEVICE;
            a.r2lut[c] = (const int32_t *)tp;
            tp += n;
          }
        }
      }
    }
    if (rx) {
      a.rowmap = rx->rowmap_dev;
      a.rowmap_stride = rx->rowmap_stride;
      a.request = 1;
      a.req_x0 = rx->corner_x;
      a.req_y0 = rx->corner_y;
      a.y_base = rx->y_base;
      a.y_count = rx->y_count;
      for (int c = 0; c < a.nplanes && c < MAXP; c++) {
        a.wstart[c] = rx->wstart[c];
        a.wlimit[c] = rx->wlimit[c];
      }
      if (!f.xt) a.ycbcr = rx->ycc; // the colour transformer the first request built (colortransformerfactory.cpp:220-221)
    }
    rc = p.kernel == Recon::FLAT ? launch_fused_flat(a, s) : p.kernel == Recon::TILE ? launch_fused_tile(a, p.fast || p.fast12, s) : -1;
    if (rc == -1) rc = launch_generic(a, p.fast, s); // (also where no tile of fused_tile_kernel fits LDS)
  }
  return rc ? MIJPEG_ERR_DEVICE : MIJPEG_OK;
}


// ------------------------------------------------------------------------------------------------
// ragged batches: streams of any shapes in one device pass (include/mijpeg.h)
// ------------------------------------------------------------------------------------------------
// The layout group of a frame description, or -1: 8-bit plain sequential frames in the four layouts whose fused kernels have a
// ragged flavour, every plane inside the kernels' 32-bit offsets
static int ragged_group_of(const mijpeg_info &f)
{
  if (f.precision != 8 || f.xt || f.progressive || f.coef_wide || f.dnl || f.width < 1 || f.height < 1 || f.coef_count < 64) return -1;
  if (f.components != 1 && f.components != 3) return -1;
  for (int c = 0; c < f.components; c++)
    if ((unsigned)f.quant_index[c] >= 4 || f.blocks_w[c] < 1 || f.blocks_h[c] < 1 || (uint64_t)f.blocks_w[c] * (uint64_t)f.blocks_h[c] * 128u > 0xffffffffull) return -1;
  switch (sampling_of(f)) {
  case Sampling::S420: return MIJPEG_RAGGED_420;
  case Sampling::S422: return MIJPEG_RAGGED_422;
  case Sampling::S444: return MIJPEG_RAGGED_444;
  case Sampling::GREY: return f.hsamp[0] == 1 && f.vsamp[0] == 1 ? MIJPEG_RAGGED_GREY : -1; // (sampling factors on a single component: MCU padding nobody decodes)
  default: return -1;
  }
}

// Grouping, workgroup ranges and coefficient bases of n frames; excluded[i] != 0 (optional) keeps frame i out of the groups
static int ragged_plan(const mijpeg_info *infos, int n, const char *excluded, int32_t *group, mijpeg_ragged_frame *frames, int32_t *group_workgroups, int64_t *coef_total)
{
  int64_t base = 0;
  uint64_t grid[MIJPEG_RAGGED_GROUPS] = {0, 0, 0, 0};
  for (int i = 0; i < n; i++) {
    const mijpeg_info &f = infos[i];
    mijpeg_ragged_frame &r = frames[i];
    memset(&r, 0, sizeof(r));
    int g = excluded && excluded[i] ? -1 : ragged_group_of(f);
    const uint64_t tiles_x = g < 0 ? 0 : ((uint64_t)f.width + 127) / 128, tiles_y = g < 0 ? 0 : ((uint64_t)f.height + 127) / 128;
    if (g >= 0 && grid[g] + tiles_x * tiles_y > 0x7fffffffull) g = -1; // (a grid holds 2^31 - 1 workgroups)
    group[i] = g;
    if (g < 0) continue;
    r.coef_base = base;
    base += f.coef_count;
    r.off_y = f.coef_offset[0];
    r.off_cb = f.components > 1 ? f.coef_offset[1] : 0;
    r.off_cr = f.components > 1 ? f.coef_offset[2] : 0;
    r.first_workgroup = (int32_t)grid[g];
    r.tiles_x = (int32_t)tiles_x;
    r.tiles_y = (int32_t)tiles_y;
    grid[g] += tiles_x * tiles_y;
    r.width = f.width;
    r.height = f.height;
    r.bw_y = f.blocks_w[0];
    r.bh_y = f.blocks_h[0];
    r.bw_c = f.components > 1 ? f.blocks_w[1] : 0;
    r.bh_c = f.components > 1 ? f.blocks_h[1] : 0;
    // valid chroma samples, as launch_reconstruct_ex has them for these layouts
    r.cw = (f.width + 1) / 2;
    r.ch = g == MIJPEG_RAGGED_422 ? f.height : (f.height + 1) / 2;
  }
  for (int g = 0; g < MIJPEG_RAGGED_GROUPS; g++) group_workgroups[g] = (int32_t)grid[g];
  *coef_total = base;
  return MIJPEG_OK;
}

int mijpeg_ragged_plan(const mijpeg_info *infos, int n, int32_t *group, mijpeg_ragged_frame *frames, int32_t group_workgroups[MIJPEG_RAGGED_GROUPS], int64_t *coef_total)
try {
  if (!infos || !group || !frames || !group_workgroups || !coef_total || n < 1) return MIJPEG_ERR_INVALID_PARAMETER;
  return ragged_plan(infos, n, nullptr, group, frames, group_workgroups, coef_total);
} catch (...) { return boundary_catch(nullptr, "mijpeg_ragged_plan"); }

// Image i through the single-image route, on a decoder object of its own (kept from call to call)
static void ragged_single_image(mijpeg_decoder *d, int i, int k, const uint8_t *data, size_t size, int min_intervals)
{
  mijpeg_decoder::RaggedImage &r = d->ragged[(size_t)i];
  r.group = -1;
  r.child = nullptr;
  if ((size_t)k >= d->ragged_children.size()) {
    mijpeg_decoder *c = nullptr;
    const int rc = mijpeg_create(&c, d->device);
    if (rc) { r.status = rc; return; }
    d->ragged_children.push_back(c);
  }
  mijpeg_decoder *c = d->ragged_children[(size_t)k];
  r.child = c;
  if (data) c->own_input.assign(data, data + size);
  else c->own_input.clear();
  int rc = mijpeg_set_input(c, data ? c->own_input.data() : nullptr, data ? size : 0);
  if (!rc) {
    rc = mijpeg_decode_coefficients_device(c, min_intervals);
    if (rc == MIJPEG_ERR_NOT_AVAILABLE) rc = mijpeg_decode_coefficients(c, 0);
  }
  if (!rc) rc = mijpeg_get_info(c, &r.info);
  r.status = rc;
}

int mijpeg_decode_ragged_device(mijpeg_decoder *d, const uint8_t *const *streams, const size_t *sizes, int n, int min_intervals, int32_t *status)
try {
  if (!d || !streams || !sizes || !status || n < 1) return MIJPEG_ERR_INVALID_PARAMETER;
  if (d->device < 0) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "decoder was created without a device");
  HIP_TRY(d, hipSetDevice(d->device));
  if (d->spec_active) (void)settle_speculation(d); // (an unvalidated batch of the uniform calls is abandoned here)
  if (const int prc = settle_pending(d)) return prc;
  d->batch_frames = 0;
  d->ragged_n = 0;
  d->img_valid = d->model_valid = d->uploaded = d->decoded = false;
  d->ragged_stats = mijpeg_ragged_stats{};
  if (d->batch_hosts.size() < (size_t)n) d->batch_hosts.resize((size_t)n);
  for (auto &h : d->batch_hosts)
    if (!h) h.reset(new HostDecoder());
  d->ragged.assign((size_t)n, mijpeg_decoder::RaggedImage{});
  // headers and restart markers of all streams, one stream per worker
  std::vector<int> rcs((size_t)n, 0);
  const int workers = std::min(n, default_threads());
  parallel_for(workers, [&](int w) {
    for (int i = w; i < n; i += workers) rcs[(size_t)i] = streams[i] && sizes[i] ? d->batch_hosts[(size_t)i]->parse(streams[i], sizes[i], false) : MIJPEG_ERR_STREAM_EMPTY;
  });
  // what the batch kernels cover goes into the layout groups
  std::vector<char> excluded((size_t)n, 0);
  std::vector<mijpeg_info> infos((size_t)n);
  for (int i = 0; i < n; i++) {
    const char *why = rcs[(size_t)i] ? "the stream does not parse as the batch decoder reads it" : ragged_entropy_obstacle(*d->batch_hosts[(size_t)i], sizes[i]);
    excluded[(size_t)i] = why != nullptr;
    if (why) d->ragged[(size_t)i].why_single = why;
    if (excluded[(size_t)i]) memset(&infos[(size_t)i], 0, sizeof(mijpeg_info));
    else infos[(size_t)i] = d->batch_hosts[(size_t)i]->info;
  }
  std::vector<int32_t> group((size_t)n);
  std::vector<mijpeg_ragged_frame> frames((size_t)n);
  int32_t grids[MIJPEG_RAGGED_GROUPS];
  int64_t coef_total = 0;
  ragged_plan(infos.data(), n, excluded.data(), group.data(), frames.data(), grids, &coef_total);
  for (int i = 0; i < n; i++)
    if (group[(size_t)i] < 0 && !excluded[(size_t)i]) d->ragged[(size_t)i].why_single = "no layout group for this frame: 8-bit sequential 4:2:0, 4:2:2, 4:4:4 and grey frames have one";
  if (coef_total > 0) {
    const int rc = ensure_coef_store(d, (size_t)coef_total, false);
    if (rc) return rc;
  }
  // one launch of the Huffman kernel per group (the walk in front of it where streams have no restart markers)
  for (int g = 0; g < MIJPEG_RAGGED_GROUPS; g++) {
    std::vector<int> members;
    for (int i = 0; i < n; i++)
      if (group[(size_t)i] == g) members.push_back(i);
    if (members.empty()) continue;
    const size_t m = members.size();
    std::vector<HostDecoder *> hosts(m);
    std::vector<const uint8_t *> datas(m);
    std::vector<size_t> gsizes(m);
    std::vector<int64_t> bases(m);
    std::vector<int> verdict(m, 1);
    for (size_t k = 0; k < m; k++) {
      const int i = members[k];
      hosts[k] = d->batch_hosts[(size_t)i].get();
      datas[k] = streams[i];
      gsizes[k] = sizes[i];
      bases[k] = frames[(size_t)i].coef_base;
    }
    int scan_launches = 0, walk_launches = 0;
    const RaggedEntropy re{bases.data(), verdict.data(), &scan_launches, &walk_launches};
    const int rc = device_entropy_batch(d, hosts.data(), datas.data(), gsizes.data(), (int)m, 1, d->coef_dev, 0, false, false, &re);
    d->ragged_stats.entropy_launches += scan_launches;
    d->ragged_stats.walk_launches += walk_launches;
    if (rc && rc != MIJPEG_ERR_NOT_AVAILABLE) return rc; // (the device, memory: not a verdict on a stream)
    // What is left to refuse a whole group once every member passed ragged_entropy_obstacle: its device walk did not settle
    // or has more subsequences than its prefix sums hold, the launch outgrew 32-bit offsets.  Every member then takes the
    // single-image route, with the launch's message as the reason (mijpeg_ragged_route).
    const std::string group_refusal = rc ? "the layout group's launch was refused: " + d->err_msg : std::string();
    for (size_t k = 0; k < m; k++) {
      const int i = members[k];
      if (rc || verdict[k]) { // damaged: the single-image route decides
        group[(size_t)i] = -1;
        d->ragged[(size_t)i].why_single = rc ? group_refusal : std::string("the device decoder found the entropy coded data damaged");
        continue;
      }
      mijpeg_decoder::RaggedImage &r = d->ragged[(size_t)i];
      r.group = g;
      r.info = hosts[k]->info;
      r.coef_base = frames[(size_t)i].coef_base;
      d->ragged_stats.ragged++;
    }
  }
  // everything else: the single-image route, stream by stream
  int children = 0;
  for (int i = 0; i < n; i++) {
    if (group[(size_t)i] >= 0) continue;
    ragged_single_image(d, i, children++, streams[i], sizes[i], min_intervals);
    d->ragged_stats.fallbacks++;
    if (d->ragged[(size_t)i].status) d->ragged_stats.errors++;
  }
  for (int i = 0; i < n; i++) status[i] = d->ragged[(size_t)i].status;
  d->ragged_stats.images = n;
  d->ragged_n = n;
  d->err_code = 0;
  d->err_msg.clear();
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_decode_ragged_device"); }

int mijpeg_ragged_info(mijpeg_decoder *d, int i, mijpeg_info *info)
try {
  if (!d || !info || i < 0) return MIJPEG_ERR_INVALID_PARAMETER;
  if (i >= d->ragged_n) return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "no such image: call mijpeg_decode_ragged_device first");
  const mijpeg_decoder::RaggedImage &r = d->ragged[(size_t)i];
  if (r.status) {
    const char *msg = nullptr;
    if (r.child) (void)mijpeg_last_error(r.child, &msg);
    return set_error(d, r.status, msg ? msg : "the stream could not be decoded");
  }
  *info = r.info;
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_ragged_info"); }

int mijpeg_ragged_warning(mijpeg_decoder *d, int i, const char **message)
try {
  if (message) *message = nullptr;
  if (!d || i < 0 || i >= d->ragged_n) return 0;
  const mijpeg_decoder::RaggedImage &r = d->ragged[(size_t)i];
  return r.child && !r.status ? mijpeg_last_warning(r.child, message) : 0;
} catch (...) { return boundary_catch(d, "mijpeg_ragged_warning"); }

int mijpeg_ragged_route(mijpeg_decoder *d, int i, const char **why)
try {
  if (why) *why = nullptr;
  if (!d || i < 0) return MIJPEG_ERR_INVALID_PARAMETER;
  if (i >= d->ragged_n) return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "no such image: call mijpeg_decode_ragged_device first");
  const mijpeg_decoder::RaggedImage &r = d->ragged[(size_t)i];
  if (r.group >= 0) return 0;
  if (why) *why = r.why_single.c_str();
  return 1;
} catch (...) { return boundary_catch(d, "mijpeg_ragged_route"); }

int mijpeg_ragged_get_stats(mijpeg_decoder *d, mijpeg_ragged_stats *out)
try {
  if (!d || !out) return MIJPEG_ERR_INVALID_PARAMETER;
  *out = d->ragged_stats;
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_ragged_get_stats"); }

int mijpeg_reconstruct_ragged_device(mijpeg_decoder *d, void *const *dst_device, const int64_t *row_strides, uint32_t flags, int sync)
try {
  if (!d || !dst_device || !row_strides) return MIJPEG_ERR_INVALID_PARAMETER;
  if (d->device < 0) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "decoder was created without a device");
  if (d->ragged_n < 1) return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "no decoded ragged batch: call mijpeg_decode_ragged_device first");
  HIP_TRY(d, hipSetDevice(d->device));
  const int n = d->ragged_n;
  flags &= ~(uint32_t)(MIJPEG_FLAG_DEVICE_OUTPUT | MIJPEG_FLAG_NO_UPSAMPLING | MIJPEG_FLAG_SPECULATIVE);
  d->ragged_stats.recon_launches = d->ragged_stats.recon_single = 0;
  // Which kernel every group image takes, from ITS range check: images of a group that agree on kernel and arithmetic flavour
  // share a launch -- one outlier beyond the fast gates runs the SAFE flavour alone instead of taking the group along.
  // (quant_dev is only tested by the planner: the ragged launches read per-frame tables.)
  static const uint16_t per_frame_tables = 0;
  auto describe = [&](int i, bool own_tables) {
    const mijpeg_decoder::RaggedImage &r = d->ragged[(size_t)i];
    mijpeg_batch b;
    memset(&b, 0, sizeof(b));
    b.info = r.info;
    b.coef_dev = d->coef_dev + r.coef_base;
    b.coef_frame_stride = r.info.coef_count;
    b.quant_dev = own_tables ? &per_frame_tables : nullptr;
    b.out_dev = (uint8_t *)dst_device[i];
    b.out_row_stride = row_strides[i];
    b.out_frame_stride = 0;
    b.frames = 1;
    b.flags = flags;
    return b;
  };
  struct Launch { ReconPlan p; int group; std::vector<int> members; };
  std::vector<Launch> launches;
  std::vector<int> singles;
  for (int i = 0; i < n; i++) {
    const mijpeg_decoder::RaggedImage &r = d->ragged[(size_t)i];
    if (r.status || r.group < 0 || !dst_device[i]) continue;
    const mijpeg_batch b = describe(i, true);
    const ReconPlan p = plan_reconstruct(&b);
    const bool has_flavour = (r.group == MIJPEG_RAGGED_420 && (p.kernel == Recon::FUSED420P || p.kernel == Recon::FUSED420)) ||
                             (r.group == MIJPEG_RAGGED_422 && p.kernel == Recon::FUSED422) || (r.group == MIJPEG_RAGGED_444 && p.kernel == Recon::FUSED444) ||
                             (r.group == MIJPEG_RAGGED_GREY && p.kernel == Recon::FUSED1);
    if (!has_flavour) { singles.push_back(i); continue; }
    size_t l = 0;
    while (l < launches.size() && !(launches[l].group == r.group && launches[l].p.kernel == p.kernel && launches[l].p.fast == p.fast && launches[l].p.wide == p.wide)) l++;
    if (l == launches.size()) launches.push_back(Launch{p, r.group, {}});
    launches[l].members.push_back(i);
  }
  // descriptor tables of all launches in one upload: per launch [frames][first workgroups][deltas << 4, per frame 4 x 64]
  if (!launches.empty()) {
    size_t bytes = 0;
    std::vector<size_t> at(launches.size());
    for (size_t l = 0; l < launches.size(); l++) {
      const size_t m = launches[l].members.size();
      at[l] = bytes;
      bytes += m * sizeof(RaggedFrame) + ((m + 1) * 4 + 15) / 16 * 16 + m * 4 * 64 * sizeof(int32_t);
    }
    int rc = ensure_dev(d, (void **)&d->ragged_desc_dev, &d->ragged_desc_cap, bytes);
    if (rc) return rc;
    if (d->ragged_upload_pending) { // (the pinned copy travels asynchronously: the last call's must have left)
      HIP_TRY(d, hipEventSynchronize(d->ragged_uploaded));
      d->ragged_upload_pending = false;
    }
    if ((rc = ensure_pinned(d, &d->ragged_desc_host, &d->ragged_desc_host_cap, bytes))) return rc;
    std::vector<uint32_t> grid(launches.size());
    for (size_t l = 0; l < launches.size(); l++) {
      const std::vector<int> &mem = launches[l].members;
      const size_t m = mem.size();
      RaggedFrame *fr = (RaggedFrame *)(d->ragged_desc_host + at[l]);
      uint32_t *first = (uint32_t *)(fr + m);
      int32_t *q = (int32_t *)((uint8_t *)first + ((m + 1) * 4 + 15) / 16 * 16);
      // the launch's own frames through the planner: first workgroups, tile grids, plane sizes
      std::vector<mijpeg_info> infos(m);
      std::vector<int32_t> grp(m);
      std::vector<mijpeg_ragged_frame> pf(m);
      int32_t grids[MIJPEG_RAGGED_GROUPS];
      int64_t unused = 0;
      for (size_t k = 0; k < m; k++) infos[k] = d->ragged[(size_t)mem[k]].info;
      ragged_plan(infos.data(), (int)m, nullptr, grp.data(), pf.data(), grids, &unused);
      for (size_t k = 0; k < m; k++) {
        const int i = mem[k];
        const mijpeg_decoder::RaggedImage &r = d->ragged[(size_t)i];
        if (grp[k] != launches[l].group) return set_error(d, MIJPEG_ERR_PHASE_ERROR, "ragged planner disagrees with itself");
        RaggedFrame &x = fr[k];
        memset(&x, 0, sizeof(x));
        x.coef_base = r.coef_base;
        x.off_y = pf[k].off_y; x.off_cb = pf[k].off_cb; x.off_cr = pf[k].off_cr;
        x.out = (uint8_t *)dst_device[i];
        x.row_stride = row_strides[i];
        x.width = pf[k].width; x.height = pf[k].height;
        x.bw_y = pf[k].bw_y; x.bh_y = pf[k].bh_y; x.bw_c = pf[k].bw_c; x.bh_c = pf[k].bh_c;
        x.cw = pf[k].cw; x.ch = pf[k].ch;
        x.tiles_x = pf[k].tiles_x; x.tiles_y = pf[k].tiles_y;
        x.qframe = (int32_t)k;
        first[k] = (uint32_t)pf[k].first_workgroup;
        for (int c = 0; c < 4; c++)
          for (int z = 0; z < 64; z++) q[(k * 4 + (size_t)c) * 64 + (size_t)z] = c < r.info.components ? (int32_t)r.info.quant[r.info.quant_index[c]][z] << 4 : 16;
      }
      grid[l] = (uint32_t)grids[launches[l].group];
      first[m] = grid[l];
    }
    HIP_TRY(d, hipMemcpyAsync(d->ragged_desc_dev, d->ragged_desc_host, bytes, hipMemcpyHostToDevice, d->stream));
    if (!d->ragged_uploaded) HIP_TRY(d, hipEventCreateWithFlags(&d->ragged_uploaded, hipEventDisableTiming));
    HIP_TRY(d, hipEventRecord(d->ragged_uploaded, d->stream));
    d->ragged_upload_pending = true;
    for (size_t l = 0; l < launches.size(); l++) {
      const size_t m = launches[l].members.size();
      Fused420Args a;
      memset(&a, 0, sizeof(a));
      a.coef = d->coef_dev;
      a.frames = (int32_t)m;
      a.ragged = (const RaggedFrame *)(d->ragged_desc_dev + at[l]);
      a.ragged_first = (const uint32_t *)(a.ragged + m);
      a.qdev = (const int32_t *)((const uint8_t *)a.ragged_first + ((m + 1) * 4 + 15) / 16 * 16);
      if (launch_fused_ragged(launches[l].p, a, grid[l], d->stream))
        return set_error(d, MIJPEG_ERR_DEVICE, std::string("kernel launch failed: ") + hipGetErrorString(hipGetLastError()));
      d->ragged_stats.recon_launches++;
    }
  }
  // One image whose reconstruction fails does not stop the others, whichever route it takes: the call works through the list
  // and then returns the first such code, with a message that names the image.  (A launch of a whole group that fails, or
  // memory that cannot be had for the tables, is the device's failure and ends the call at once; what was enqueued stays
  // ordered on the object's stream, and the next call waits for the descriptor upload as usual.)
  int failed = MIJPEG_OK;
  std::string failed_msg;
  // group images no ragged flavour fits (ranges beyond the fused kernels' gates, no colour transformation, ...): the existing kernels
  for (int i : singles) {
    mijpeg_batch b = describe(i, false);
    const size_t ws = mijpeg_workspace_bytes(&b);
    int rc = ws ? ensure_dev(d, (void **)&d->ws_dev, &d->ws_cap, ws) : MIJPEG_OK;
    if (!rc) {
      b.workspace = ws ? d->ws_dev : nullptr;
      b.workspace_bytes = ws ? d->ws_cap : 0;
      rc = mijpeg_launch_reconstruct(&b, d->stream);
    }
    if (rc) {
      if (!failed) {
        failed = rc;
        failed_msg = "image " + std::to_string(i) + " of the ragged batch was not reconstructed";
      }
      continue;
    }
    d->ragged_stats.recon_single++;
  }
  // images of the single-image route, on their own objects (which wait for their kernels themselves)
  for (int i = 0; i < n; i++) {
    mijpeg_decoder::RaggedImage &r = d->ragged[(size_t)i];
    if (!r.child || r.status || !dst_device[i]) continue;
    const int rc = mijpeg_reconstruct_device(r.child, dst_device[i], row_strides[i], flags, 1);
    if (rc && !failed) {
      const char *msg = nullptr;
      (void)mijpeg_last_error(r.child, &msg);
      failed = rc;
      failed_msg = "image " + std::to_string(i) + " of the ragged batch was not reconstructed: " + (msg ? msg : "");
    }
  }
  if (sync) HIP_TRY(d, hipStreamSynchronize(d->stream));
  if (failed) return set_error(d, failed, failed_msg);
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_reconstruct_ragged_device"); }

// ------------------------------------------------------------------------------------------------
// encoder direction of the block pipeline
// ------------------------------------------------------------------------------------------------
int mijpeg_frame_layout(mijpeg_info *f)
try {
  if (!f || f->width < 1 || f->height < 1 || f->width > 65535 || f->height > 65535 || f->components < 1 || f->components > MIJPEG_MAX_COMPONENTS)
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
  f->sample_bytes = 1;
  return MIJPEG_OK;
} catch (...) { return boundary_catch(nullptr, "mijpeg_frame_layout"); }

int mijpeg_launch_forward(const mijpeg_forward_batch *b, void *stream)
try {
  ForwardArgs a;
  if (const int rc = forward_args_of(b, a)) return rc;
  return launch_forward(a, (hipStream_t)stream) ? MIJPEG_ERR_DEVICE : MIJPEG_OK;
} catch (...) { return boundary_catch(nullptr, "mijpeg_launch_forward"); }

void mijpeg_quality_tables(int quality, uint16_t luma[64], uint16_t chroma[64])
try {
  // ISO/IEC 10918-1 Annex K.1 / K.2 matrices, natural order
  static const uint8_t K1[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
                                 14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
  static const uint8_t K2[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
  quality = std::min(100, std::max(1, quality));
  const int scale = quality < 50 ? 5000 / quality : 200 - quality * 2; // quantization.cpp:296-299
  for (int j = 0; j < 64; j++) {
    luma[j] = (uint16_t)std::min(255, std::max(1, (K1[j] * scale + 50) / 100)); // :411, :443-466
    chroma[j] = (uint16_t)std::min(255, std::max(1, (K2[j] * scale + 50) / 100));
  }
} catch (...) { (void)boundary_catch(nullptr, "mijpeg_quality_tables"); }

// Entropy coding of one frame's coefficient planes on the device (hencode.hip) and download of the finished stream, as a
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
  uint64_t *scratch = nullptr;
  uint32_t chunks = 0;
  uint8_t *result = nullptr;
  size_t head_size = 0, ecs = 0;
  std::vector<uint8_t> head;

  static size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

  int upload_tables()
  {
    HencTables *h = (HencTables *)((uint8_t *)d->henc_host + 64 + (size_t)slot * sizeof(HencTables)); // pinned, one per slot
    henc_pack_tables(h, tabs);
    HIP_TRY(d, hipMemcpyAsync((void *)a.tables, h, sizeof(*h), hipMemcpyHostToDevice, stream));
    return MIJPEG_OK;
  }

  // geometry, buffers, tables (optimised ones cost a synchronisation of their own), then count + prefix sums
  int stage_a(mijpeg_decoder *dec, const mijpeg_info &info, const int16_t *coef_dev, int ri, int optimize, int slot_, hipStream_t st)
  {
    d = dec; f = &info; slot = slot_; stream = st; restart_interval = ri;
    const int nc = info.components;
    memset(&a, 0, sizeof(a));
    a.coef = coef_dev;
    if (!henc_frame_geometry(a, info, ri)) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "too many blocks per MCU for the device entropy coder");
    const int B = a.blocks_per_mcu;
    const uint64_t nblocks = (uint64_t)a.total_mcus * (uint64_t)B;
    if (nblocks >= ((uint64_t)1 << 30)) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "frame too large for the device entropy coder");
    a.total_blocks = (uint32_t)nblocks;
    a.n_intervals = (uint32_t)((a.total_mcus + a.ri - 1) / a.ri);
    const uint32_t N = a.total_blocks, I = a.n_intervals;
    // arena 1: tables, statistics, block and interval arrays, scan scratch
    size_t o = 0;
    const size_t o_tab = o; o = al(o + sizeof(HencTables));
    const size_t o_hist = o; o = al(o + 4 * 256 * 4);
    const size_t o_bits = o; o = al(o + (size_t)N * 4);
    const size_t o_bitpos = o; o = al(o + ((size_t)N + 1) * 8);
    const size_t o_ibytes = o; o = al(o + (size_t)I * 4);
    const size_t o_istart = o; o = al(o + ((size_t)I + 1) * 8);
    const size_t scratch_words = ((size_t)N / 1024 + 8) * 2 + 8192;
    const size_t o_scratch = o; o = al(o + scratch_words * 8);
    int rc = ensure_dev(d, (void **)&d->henc_dev[slot], &d->henc_cap[slot], o);
    if (rc) return rc;
    if (!d->henc_host) HIP_TRY(d, hipHostMalloc((void **)&d->henc_host, 64 + 2 * sizeof(HencTables), hipHostMallocDefault));
    readback = d->henc_host + 2 * slot;
    uint8_t *base = d->henc_dev[slot];
    a.tables = (const HencTables *)(base + o_tab);
    a.hist = (uint32_t *)(base + o_hist);
    a.bits = (uint32_t *)(base + o_bits);
    a.bitpos = (const uint64_t *)(base + o_bitpos);
    a.ibytes = (uint32_t *)(base + o_ibytes);
    a.istart = (const uint64_t *)(base + o_istart);
    scratch = (uint64_t *)(base + o_scratch);
    enc_standard_tables(tabs);
    rc = upload_tables();
    if (rc) return rc;
    if (optimize) { // symbol statistics first, tables from them (Annex K.2)
      HIP_TRY(d, hipMemsetAsync(base + o_hist, 0, 4 * 256 * 4, stream));
      if (henc_count(a, true, stream)) return hip_fail(d, hipGetLastError(), "henc_count_kernel launch");
      uint32_t hist[4][256];
      HIP_TRY(d, hipMemcpyAsync(hist, base + o_hist, sizeof(hist), hipMemcpyDeviceToHost, stream));
      HIP_TRY(d, hipStreamSynchronize(stream));
      enc_optimal_tables(tabs, hist, hist + 2, nc > 1 ? 2 : 1);
      rc = upload_tables();
      if (rc) return rc;
    }
    if (henc_count(a, false, stream)) return hip_fail(d, hipGetLastError(), "henc_count_kernel launch");
    if (exclusive_scan_u32(a.bits, (uint64_t *)a.bitpos, N, scratch, stream)) return hip_fail(d, hipGetLastError(), "scan launch");
    if (henc_interval_bytes(a, stream)) return hip_fail(d, hipGetLastError(), "henc_interval_bytes_kernel launch");
    if (exclusive_scan_u32(a.ibytes, (uint64_t *)a.istart, I, scratch, stream)) return hip_fail(d, hipGetLastError(), "scan launch");
    HIP_TRY(d, hipMemcpyAsync(&readback[0], a.istart + I, 8, hipMemcpyDeviceToHost, stream));
    return MIJPEG_OK;
  }

  // plain stream, stuffing
  int stage_b()
  {
    HIP_TRY(d, hipStreamSynchronize(stream));
    const uint64_t plain_bytes = readback[0];
    const uint32_t I = a.n_intervals;
    // (coefficients the forward kernels make of 8-bit pixels always have a code: at most 11 / 10 bits, the host coder's check)
    chunks = (uint32_t)((plain_bytes + HENC_STUFF_CHUNK - 1) / HENC_STUFF_CHUNK);
    size_t q = 0;
    const size_t q_plain = q; q = al(q + (size_t)plain_bytes + 16);
    const size_t q_ffc = q; q = al(q + (size_t)chunks * 4 + 4);
    const size_t q_ffs = q; q = al(q + ((size_t)chunks + 1) * 8);
    const size_t q_out = q; q = al(q + (size_t)plain_bytes * 2 + (size_t)I * 2 + 16);
    const int rc = ensure_dev(d, (void **)&d->henc_out_dev[slot], &d->henc_out_cap[slot], q);
    if (rc) return rc;
    uint8_t *ob = d->henc_out_dev[slot];
    a.plain = (uint32_t *)(ob + q_plain);
    a.plain_bytes = plain_bytes;
    a.ffcount = (uint32_t *)(ob + q_ffc);
    a.ffstart = (const uint64_t *)(ob + q_ffs);
    a.out = ob + q_out;
    HIP_TRY(d, hipMemsetAsync(ob + q_plain, 0, al((size_t)plain_bytes + 16), stream));
    if (henc_emit(a, stream)) return hip_fail(d, hipGetLastError(), "henc_emit_kernel launch");
    if (henc_count_ff(a, stream)) return hip_fail(d, hipGetLastError(), "henc_count_ff_kernel launch");
    if (exclusive_scan_u32(a.ffcount, (uint64_t *)a.ffstart, chunks, scratch, stream)) return hip_fail(d, hipGetLastError(), "scan launch");
    if (henc_stuff(a, stream)) return hip_fail(d, hipGetLastError(), "henc_stuff_kernel launch");
    HIP_TRY(d, hipMemcpyAsync(&readback[1], a.ffstart + chunks, 8, hipMemcpyDeviceToHost, stream));
    return MIJPEG_OK;
  }

  // headers on the host, download of the entropy coded data behind them
  int stage_c()
  {
    HIP_TRY(d, hipStreamSynchronize(stream));
    ecs = (size_t)a.plain_bytes + (size_t)readback[1] + (size_t)(a.n_intervals - 1) * 2;
    head.clear();
    enc_write_headers(head, *f, tabs, restart_interval);
    head_size = head.size();
    result = (uint8_t *)malloc(head_size + ecs + 2);
    if (!result) return set_error(d, MIJPEG_ERR_OUT_OF_MEMORY, "out of memory for the stream");
    memcpy(result, head.data(), head_size);
    const hipError_t e = hipMemcpyAsync(result + head_size, a.out, ecs, hipMemcpyDeviceToHost, stream);
    if (e != hipSuccess) { free(result); result = nullptr; return hip_fail(d, e, "download of the stream"); }
    return MIJPEG_OK;
  }

  int finish(uint8_t **out_stream, size_t *out_size)
  {
    const hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess) { free(result); result = nullptr; return hip_fail(d, e, "download of the stream"); }
    result[head_size + ecs] = 0xff;
    result[head_size + ecs + 1] = 0xd9;
    *out_stream = result;
    *out_size = head_size + ecs + 2;
    result = nullptr;
    return MIJPEG_OK;
  }
};

static int device_entropy_code(mijpeg_decoder *d, const mijpeg_info &f, const int16_t *coef_dev, int restart_interval, int optimize,
                               uint8_t **stream, size_t *size)
{
  HencJob job;
  int rc = job.stage_a(d, f, coef_dev, restart_interval, optimize, 0, d->stream);
  if (!rc) rc = job.stage_b();
  if (!rc) rc = job.stage_c();
  if (!rc) rc = job.finish(stream, size);
  return rc;
}

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
  if (rc)
    for (int f = 0; f < b->frames; f++) { free(streams[f]); streams[f] = nullptr; sizes[f] = 0; }
  d->timing[0] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count(); // mijpeg_last_timing: the whole call
  d->timing[1] = d->timing[2] = d->timing[3] = 0;
  return rc;
} catch (...) { return boundary_catch(d, "mijpeg_encode_batch_device"); }

int mijpeg_encode_image(mijpeg_decoder *d, const uint8_t *pixels, int32_t width, int32_t height, int32_t components, int64_t row_stride,
                        int quality, const int32_t *hsamp, const int32_t *vsamp, int restart_interval, int optimize, uint8_t **stream, size_t *size)
try {
  return mijpeg_encode_image_ex(d, pixels, width, height, components, row_stride, quality, hsamp, vsamp, restart_interval, optimize, 0, stream, size);
} catch (...) { return boundary_catch(d, "mijpeg_encode_image"); }

int mijpeg_encode_image_ex(mijpeg_decoder *d, const uint8_t *pixels, int32_t width, int32_t height, int32_t components, int64_t row_stride,
                           int quality, const int32_t *hsamp, const int32_t *vsamp, int restart_interval, int optimize, uint32_t flags,
                           uint8_t **stream, size_t *size)
try {
  using clk = std::chrono::steady_clock;
  const auto t_begin = clk::now();
  if (!d || !pixels || !stream || !size || (components != 1 && components != 3) || row_stride < (int64_t)width * components)
    return MIJPEG_ERR_INVALID_PARAMETER;
  if (d->device < 0) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "decoder was created without a device");
  HIP_TRY(d, hipSetDevice(d->device));
  mijpeg_forward_batch b;
  memset(&b, 0, sizeof(b));
  mijpeg_info &f = b.info;
  f.width = width;
  f.height = height;
  f.components = components;
  f.precision = 8;
  f.ycbcr = components == 3 ? 1 : 0;
  for (int c = 0; c < components; c++) {
    f.hsamp[c] = hsamp ? hsamp[c] : 1;
    f.vsamp[c] = vsamp ? vsamp[c] : 1;
    // the reference encoder defines a luma and a chroma table but its frame header selects table 0 for every component
    // (what its own files show: tests/test_encoder.py::test_quality_tables_are_the_reference_encoders), so that is
    // what reproduces its coefficients
    f.quant_index[c] = 0;
  }
  mijpeg_quality_tables(quality, f.quant[0], f.quant[1]);
  int rc = mijpeg_frame_layout(&f);
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
} catch (...) { return boundary_catch(d, "mijpeg_encode_image_ex"); }

// ------------------------------------------------------------------------------------------------
// decoder-object reconstruction
// ------------------------------------------------------------------------------------------------
// The frame as the reconstruction sees it: the whole picture, or -- without upsampling -- one component at its own
// resolution, which is a single-component identity-transformed frame over that component's coefficient plane
// (BlockBitmapRequester::ReconstructUnsampled with rr_bUpsampling = false: control/blockbitmaprequester.cpp:1013-1074,
// control/bitmapctrl.cpp:273-294; the colour transformation is off then, codestream/rectanglerequest.cpp:157-159).
static mijpeg_info view_of(const mijpeg_info &f, int comp)
{
  if (comp < 0) return f;
  mijpeg_info v = f;
  v.components = 1;
  v.width = (f.width + f.subx[comp] - 1) / f.subx[comp];
  v.height = (f.height + f.suby[comp] - 1) / f.suby[comp];
  v.hsamp[0] = v.vsamp[0] = v.subx[0] = v.suby[0] = 1;
  v.quant_index[0] = f.quant_index[comp];
  v.blocks_w[0] = f.blocks_w[comp];
  v.blocks_h[0] = f.blocks_h[comp];
  v.mcus_x = v.blocks_w[0];
  v.mcus_y = v.blocks_h[0];
  v.coef_offset[0] = 0;
  v.coef_count = (int64_t)v.blocks_w[0] * v.blocks_h[0] * 64;
  v.range_max[0] = f.range_max[comp];
  v.ycbcr = 0;
  return v;
}

static int reconstruct_view(mijpeg_decoder *d, int comp, void *dst_device, int64_t row_stride, uint32_t flags, int sync)
{
  HIP_TRY(d, hipSetDevice(d->device));
  mijpeg_batch b;
  memset(&b, 0, sizeof(b));
  b.info = view_of(d->host.info, comp);
  b.coef_dev = d->coef_dev + (comp < 0 ? 0 : d->host.info.coef_offset[comp]);
  b.coef_frame_stride = b.info.coef_count;
  b.out_dev = (uint8_t *)dst_device;
  b.out_row_stride = row_stride;
  b.out_frame_stride = row_stride * b.info.height;
  b.frames = 1;
  b.flags = flags;
  b.xt = d->host.is_xt() ? &d->host.xt : nullptr;
  const size_t ws = mijpeg_workspace_bytes(&b);
  if (ws) {
    int rc = ensure_dev(d, (void **)&d->ws_dev, &d->ws_cap, ws);
    if (rc) return rc;
    b.workspace = d->ws_dev;
    b.workspace_bytes = d->ws_cap;
  }
  const int rc = mijpeg_launch_reconstruct(&b, d->stream);
  if (rc) return set_error(d, rc, rc == MIJPEG_ERR_DEVICE ? std::string("kernel launch failed: ") + hipGetErrorString(hipGetLastError())
                                                           : std::string("reconstruction not available for this stream"));
  if (sync) HIP_TRY(d, hipStreamSynchronize(d->stream));
  return MIJPEG_OK;
}

int mijpeg_reconstruct_device(mijpeg_decoder *d, void *dst_device, int64_t row_stride, uint32_t flags, int sync)
try {
  if (!d) return MIJPEG_ERR_INVALID_PARAMETER;
  if (d->device < 0) return set_error(d, MIJPEG_ERR_DEVICE, "decoder was created without a device: no reconstruction path");
  if (!d->uploaded) return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "no decoded coefficients: call mijpeg_decode_coefficients first");
  if (!dst_device) return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "destination pointer is NULL");
  return reconstruct_view(d, -1, dst_device, row_stride, flags & ~(MIJPEG_FLAG_DEVICE_OUTPUT | MIJPEG_FLAG_NO_UPSAMPLING), sync);
} catch (...) { return boundary_catch(d, "mijpeg_reconstruct_device"); }

void *mijpeg_host_alloc(size_t bytes)
try {
  void *p = nullptr;
  return hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess ? p : nullptr;
} catch (...) { (void)boundary_catch(nullptr, "mijpeg_host_alloc"); return nullptr; }

void mijpeg_host_free(void *p)
try {
  if (p) (void)hipHostFree(p);
} catch (...) { (void)boundary_catch(nullptr, "mijpeg_host_free"); }

int mijpeg_reconstruct_host(mijpeg_decoder *d, void *dst_host, int64_t row_stride, uint32_t flags)
try {
  if (!d) return MIJPEG_ERR_INVALID_PARAMETER;
  if (d->device < 0) return set_error(d, MIJPEG_ERR_DEVICE, "decoder was created without a device: no reconstruction path");
  if (!d->uploaded) return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "no decoded coefficients: call mijpeg_decode_coefficients first");
  if (!dst_host) return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "destination pointer is NULL");
  const mijpeg_info &f = d->host.info;
  const size_t line = (size_t)f.width * f.components * (f.sample_bytes > 0 ? f.sample_bytes : 1);
  if (row_stride < (int64_t)line) return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "row stride is smaller than a line of samples");
  HIP_TRY(d, hipSetDevice(d->device));
  const size_t row = (line + 7) & ~(size_t)7; // device image: 8-byte aligned lines -> wide stores in the kernel
  int rc = ensure_dev(d, (void **)&d->img_dev, &d->img_dev_cap, row * f.height);
  if (rc) return rc;
  using clk = std::chrono::steady_clock;
  const auto t0 = clk::now();
  rc = mijpeg_reconstruct_device(d, d->img_dev, (int64_t)row, flags, 0);
  if (rc) return rc;
  if ((size_t)row_stride == row)
    HIP_TRY(d, hipMemcpyAsync(dst_host, d->img_dev, row * f.height, hipMemcpyDeviceToHost, d->stream));
  else
    HIP_TRY(d, hipMemcpy2DAsync(dst_host, (size_t)row_stride, d->img_dev, row, line, (size_t)f.height, hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(d, hipStreamSynchronize(d->stream));
  d->timing[1] = 0;
  d->timing[2] = 0;
  d->timing[3] = std::chrono::duration<double>(clk::now() - t0).count(); // upload tail + kernel + D2H
  d->img_valid = false;
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_reconstruct_host"); }

static int serve_rect(mijpeg_decoder *d, int view, uint32_t flags, bool to_device, int32_t min_x, int32_t min_y, int32_t max_x, int32_t max_y,
                      int32_t min_comp, int32_t max_comp, void *const dst[MIJPEG_MAX_COMPONENTS],
                      const int32_t bytes_per_pixel[MIJPEG_MAX_COMPONENTS], const int32_t bytes_per_row[MIJPEG_MAX_COMPONENTS]);

int mijpeg_reconstruct_rect(mijpeg_decoder *d, int32_t min_x, int32_t min_y, int32_t max_x, int32_t max_y, int32_t min_comp,
                            int32_t max_comp, uint32_t flags, void *const dst[MIJPEG_MAX_COMPONENTS],
                            const int32_t bytes_per_pixel[MIJPEG_MAX_COMPONENTS],
                            const int32_t bytes_per_row[MIJPEG_MAX_COMPONENTS])
try {
  if (!d || !dst || !bytes_per_pixel || !bytes_per_row) return MIJPEG_ERR_INVALID_PARAMETER;
  if (d->device < 0) return set_error(d, MIJPEG_ERR_DEVICE, "decoder was created without a device: no reconstruction path");
  if (!d->uploaded) return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "no decoded coefficients: call mijpeg_decode_coefficients first");
  const bool to_device = (flags & MIJPEG_FLAG_DEVICE_OUTPUT) != 0;
  const bool unsampled = (flags & MIJPEG_FLAG_NO_UPSAMPLING) != 0;
  flags &= ~(MIJPEG_FLAG_DEVICE_OUTPUT | MIJPEG_FLAG_NO_UPSAMPLING);
  int view = -1; // component whose own sample grid is reconstructed, -1: the upsampled picture
  if (unsampled) {
    // control/bitmapctrl.cpp:273-294: one component at a time, no colour transformation, and the rectangle (given
    // on the canvas) shrinks to the component's grid
    if (min_comp < 0) min_comp = 0;
    if (max_comp >= d->host.info.components) max_comp = d->host.info.components - 1;
    if (min_comp != max_comp)
      return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "if upsampling is disabled, components can only be reconstructed one by one");
    if (d->host.is_xt())
      return set_error(d, MIJPEG_ERR_OPERATION_UNIMPLEMENTED, "JPEG XT frames are not reconstructed without upsampling (the reference merges the component with residual scratch buffers it never initialised)");
    view = min_comp;
    flags |= MIJPEG_FLAG_NO_COLOR_TRANSFORM;
    const int sx = d->host.info.subx[view], sy = d->host.info.suby[view];
    min_x = (std::max(min_x, 0) + sx - 1) / sx;
    max_x = (max_x + sx) / sx - 1;
    min_y = (std::max(min_y, 0) + sy - 1) / sy;
    max_y = (max_y + sy) / sy - 1;
  }
  void *vdst[MIJPEG_MAX_COMPONENTS] = {dst[0], dst[1], dst[2], dst[3]};
  int32_t vbpp[MIJPEG_MAX_COMPONENTS] = {bytes_per_pixel[0], bytes_per_pixel[1], bytes_per_pixel[2], bytes_per_pixel[3]};
  int32_t vbpr[MIJPEG_MAX_COMPONENTS] = {bytes_per_row[0], bytes_per_row[1], bytes_per_row[2], bytes_per_row[3]};
  if (view >= 0) { // the view has one component, number 0
    vdst[0] = dst[view];
    vbpp[0] = bytes_per_pixel[view];
    vbpr[0] = bytes_per_row[view];
    min_comp = max_comp = 0;
  }
  return serve_rect(d, view, flags, to_device, min_x, min_y, max_x, max_y, min_comp, max_comp, vdst, vbpp, vbpr);
} catch (...) { return boundary_catch(d, "mijpeg_reconstruct_rect"); }

// The rectangle [min_x, max_x] x [min_y, max_y] (on the grid of `view`: the canvas, or a component's own samples) of the
// plain picture, components [min_comp, max_comp] of the view, into the bitmaps.
static int serve_rect(mijpeg_decoder *d, int view, uint32_t flags, bool to_device, int32_t min_x, int32_t min_y, int32_t max_x, int32_t max_y,
                      int32_t min_comp, int32_t max_comp, void *const dst[MIJPEG_MAX_COMPONENTS],
                      const int32_t bytes_per_pixel[MIJPEG_MAX_COMPONENTS], const int32_t bytes_per_row[MIJPEG_MAX_COMPONENTS])
{
  const mijpeg_info f = view_of(d->host.info, view);
  const int sb = f.sample_bytes > 0 ? f.sample_bytes : 1; // bytes per sample
  const int nc = f.components;
  // the whole frame is reconstructed once per (stream, flags, view) and then served rectangle by rectangle,
  // which is what the stripe loop of cmd/reconstruct.cpp:334-342 asks for
  const size_t row = ((size_t)f.width * nc * sb + 7) & ~(size_t)7;
  const size_t padded = row * f.height;
  using clk = std::chrono::steady_clock;
  if (!d->img_valid || d->img_flags != flags || d->img_view != view) {
    HIP_TRY(d, hipSetDevice(d->device));
    int rc = ensure_dev(d, (void **)&d->img_dev, &d->img_dev_cap, padded);
    if (rc) return rc;
    auto t0 = clk::now();
    HIP_TRY(d, hipStreamSynchronize(d->stream)); // uploads complete
    auto t1 = clk::now();
    rc = reconstruct_view(d, view, d->img_dev, (int64_t)row, flags, to_device ? 1 : 0); // host requests: the copy below follows in stream order
    if (rc) return rc;
    d->timing[1] = std::chrono::duration<double>(t1 - t0).count();
    d->timing[2] = std::chrono::duration<double>(clk::now() - t1).count();
    d->timing[3] = 0;
    d->img_valid = true;
    d->img_host_valid = false;
    d->img_flags = flags;
    d->img_view = view;
  }
  if (!to_device && !d->img_host_valid) {
    HIP_TRY(d, hipSetDevice(d->device));
    if (const int prc = ensure_cached(d, true, (void **)&d->img_host, &d->img_host_cap, padded)) return prc;
    // bands of about 4 MiB (at least 8 lines): enqueue all of them now, wait for them as they are asked for
    static const long band_mib = getenv("MIJPEG_RECT_BAND_MIB") ? atol(getenv("MIJPEG_RECT_BAND_MIB")) : 4; // tuning; <= 0: one band
    d->band_lines = band_mib <= 0 ? f.height : (int)std::max<size_t>(8, (((size_t)band_mib << 20) / std::max<size_t>(row, 1) + 7) & ~(size_t)7);
    d->bands = (f.height + d->band_lines - 1) / d->band_lines;
    while ((int)d->band_events.size() < d->bands) {
      hipEvent_t e;
      HIP_TRY(d, hipEventCreateWithFlags(&e, hipEventDisableTiming));
      d->band_events.push_back(e);
    }
    for (int b = 0; b < d->bands; b++) {
      const size_t y0 = (size_t)b * d->band_lines, y1 = std::min<size_t>(f.height, y0 + d->band_lines);
      HIP_TRY(d, hipMemcpyAsync(d->img_host + y0 * row, d->img_dev + y0 * row, (y1 - y0) * row, hipMemcpyDeviceToHost, d->stream));
      HIP_TRY(d, hipEventRecord(d->band_events[(size_t)b], d->stream));
    }
    d->bands_waited = 0;
    d->img_host_valid = true;
  }
  // bands [0, upto] of the host copy have arrived when this returns
  auto wait_bands = [&](int upto) -> int {
    auto t2 = clk::now();
    for (; d->bands_waited <= upto && d->bands_waited < d->bands; d->bands_waited++)
      HIP_TRY(d, hipEventSynchronize(d->band_events[(size_t)d->bands_waited]));
    d->timing[3] += std::chrono::duration<double>(clk::now() - t2).count();
    return MIJPEG_OK;
  };
  if (min_x < 0) min_x = 0;
  if (min_y < 0) min_y = 0;
  if (max_x >= f.width) max_x = f.width - 1;
  if (max_y >= f.height) max_y = f.height - 1;
  if (min_comp < 0) min_comp = 0;
  if (max_comp >= nc) max_comp = nc - 1;
  // an empty request after clipping is served by doing nothing (codestream/rectanglerequest.cpp clips alike)
  if (min_x > max_x || min_y > max_y || min_comp > max_comp) return MIJPEG_OK;
  if (to_device) {
    ScatterArgs a;
    memset(&a, 0, sizeof(a));
    a.src = d->img_dev;
    a.src_row = (int64_t)row;
    a.ncomp = nc;
    a.sample_bytes = sb;
    a.x0 = min_x;
    a.y0 = min_y;
    a.w = max_x - min_x + 1;
    a.h = max_y - min_y + 1;
    a.c0 = min_comp;
    a.c1 = max_comp;
    for (int c = 0; c < nc; c++) {
      a.dst[c] = (uint8_t *)dst[c];
      a.bytes_per_pixel[c] = bytes_per_pixel[c];
      a.bytes_per_row[c] = bytes_per_row[c];
    }
    HIP_TRY(d, hipSetDevice(d->device));
    if (launch_scatter_rect(a, d->stream)) return hip_fail(d, hipGetLastError(), "scatter_rect_kernel launch");
    HIP_TRY(d, hipStreamSynchronize(d->stream));
    return MIJPEG_OK;
  }
  // interleaved destination (the layout cmd/bitmaphook.cpp hands out): whole lines at once
  bool interleaved = min_comp == 0 && max_comp == nc - 1 && dst[0];
  for (int c = 0; c < nc && interleaved; c++)
    interleaved = dst[c] == (uint8_t *)dst[0] + c * sb && bytes_per_pixel[c] == nc * sb && bytes_per_row[c] == bytes_per_row[0];
  if (interleaved) {
    const size_t line = (size_t)(max_x - min_x + 1) * nc * sb;
    const int lines = max_y - min_y + 1;
    auto copy_lines = [&](int y0, int y1) {
      for (int y = y0; y < y1; y++)
        memcpy((uint8_t *)dst[0] + (ptrdiff_t)y * bytes_per_row[0] + (ptrdiff_t)min_x * nc * sb,
               d->img_host + (size_t)y * row + (size_t)min_x * nc * sb, line);
    };
    // big rectangles (whole frames) are copied by the worker pool, one memcpy stream per worker, in a few slabs: the
    // workers copy slab k while the bands of slab k + 1 are still arriving
    const int parts = (int)std::min<size_t>((size_t)std::min(default_threads(), 16), line * lines / (4u << 20));
    if (parts > 1) {
      const int slabs = std::min(4, std::max(1, lines / (8 * d->band_lines)));
      for (int k = 0; k < slabs; k++) {
        const int s0 = min_y + (int)((int64_t)lines * k / slabs), s1 = min_y + (int)((int64_t)lines * (k + 1) / slabs);
        if (const int rc = wait_bands((s1 - 1) / d->band_lines)) return rc;
        parallel_for(parts, [&](int i) { copy_lines(s0 + (int)((int64_t)(s1 - s0) * i / parts), s0 + (int)((int64_t)(s1 - s0) * (i + 1) / parts)); });
      }
    } else {
      if (const int rc = wait_bands(max_y / d->band_lines)) return rc;
      copy_lines(min_y, max_y + 1);
    }
    return MIJPEG_OK;
  }
  if (const int rc = wait_bands(max_y / d->band_lines)) return rc;
  for (int c = min_comp; c <= max_comp; c++) {
    if (!dst[c]) continue;
    for (int y = min_y; y <= max_y; y++) {
      const uint8_t *src = d->img_host + (size_t)y * row + ((size_t)min_x * nc + c) * sb;
      uint8_t *out = (uint8_t *)dst[c] + (ptrdiff_t)y * bytes_per_row[c] + (ptrdiff_t)min_x * bytes_per_pixel[c];
      const int n = max_x - min_x + 1;
      const int bpp = bytes_per_pixel[c];
      if (sb == 1) {
        if (nc == 1 && bpp == 1) memcpy(out, src, (size_t)n);
        else
          for (int x = 0; x < n; x++) out[(ptrdiff_t)x * bpp] = src[(size_t)x * nc];
      } else {
        for (int x = 0; x < n; x++) memcpy(out + (ptrdiff_t)x * bpp, src + (size_t)x * nc * 2, 2);
      }
    }
  }
  return MIJPEG_OK;
}

// ------------------------------------------------------------------------------------------------
// JPEG::DisplayRectangle as a sequence of calls: request_model.hpp plans, this serves
// ------------------------------------------------------------------------------------------------
// Frame description for a request that does not show the plain picture: the whole picture, or -- without upsampling --
// the grid of component `view` with every component of the frame on it (the ones that were not asked for are zeros; only
// a colour transformer left over from earlier upsampled requests makes them matter).
static mijpeg_info request_frame(const mijpeg_info &f, int view, bool all_components)
{
  if (view < 0) return f;
  if (!all_components) return view_of(f, view);
  mijpeg_info v = f;
  v.width = (f.width + f.subx[view] - 1) / f.subx[view];
  v.height = (f.height + f.suby[view] - 1) / f.suby[view];
  for (int c = 0; c < f.components; c++) {
    v.hsamp[c] = v.vsamp[c] = v.subx[c] = v.suby[c] = 1;
    v.blocks_w[c] = f.blocks_w[view];
    v.blocks_h[c] = f.blocks_h[view];
    v.coef_offset[c] = f.coef_offset[view]; // read only where the row map says so: component `view`
    v.quant_index[c] = f.quant_index[view];
    v.range_max[c] = f.range_max[view];
  }
  v.mcus_x = v.blocks_w[0];
  v.mcus_y = v.blocks_h[0];
  return v;
}

// The request models of a decoded image start with its first DisplayRectangle call (every decode resets them): one for a plain
// frame; two for a JPEG XT frame -- legacy and residual image share m_bSubsampling (request_model.hpp)
static void ensure_request_models(mijpeg_decoder *d)
{
  if (d->model_valid) return;
  const mijpeg_info &f = d->host.info;
  if (d->host.is_xt() && f.components == 3) {
    const mijpeg_info &r = d->host.xt.residual;
    bool lsub = false, rsub = false;
    for (int c = 0; c < 3; c++) {
      lsub = lsub || f.subx[c] > 1 || f.suby[c] > 1;
      rsub = rsub || r.subx[c] > 1 || r.suby[c] > 1;
    }
    d->model.reset(3, f.width, f.height, f.subx, f.suby, true, false, nullptr, nullptr, rsub);
    d->rmodel.reset(3, f.width, f.height, r.subx, r.suby, true, false, nullptr, nullptr, lsub);
  } else
    d->model.reset(f.components, f.width, f.height, f.subx, f.suby, f.ycbcr != 0, f.dnl != 0, f.rows, f.blocks_h);
  d->model_valid = true;
}

// The lines a request reconstructed into d->req_dev (row bytes each, nc interleaved samples of sb bytes) go out to the client's
// bitmaps: columns [min_x, cx1[c]], lines [min_y, cy1[c]] of component c
static int hand_out_request(mijpeg_decoder *d, int min_x, int min_y, int y_count, const int32_t *cx1, const int32_t *cy1, int min_comp, int max_comp,
                            int nc, int sb, size_t row, size_t padded, int vc, bool all_on_view, bool to_device, void *const *dst, const int32_t *bpp,
                            const int32_t *bpr)
{
  // hand the lines out
  for (int c = min_comp; c <= max_comp; c++) {
    if (!dst[c] || cx1[c] < min_x || cy1[c] < min_y) continue;
    const int plane = vc >= 0 ? (all_on_view ? c : 0) : c;
    if (to_device) {
      ScatterArgs a;
      memset(&a, 0, sizeof(a));
      a.src = d->req_dev;
      a.src_row = (int64_t)row;
      a.ncomp = nc;
      a.sample_bytes = sb;
      a.x0 = min_x;
      a.y0 = min_y;
      a.w = cx1[c] - min_x + 1;
      a.h = cy1[c] - min_y + 1;
      a.c0 = a.c1 = plane;
      a.dst[plane] = (uint8_t *)dst[c];
      a.bytes_per_pixel[plane] = bpp[c];
      a.bytes_per_row[plane] = bpr[c];
      if (launch_scatter_rect(a, d->stream)) return hip_fail(d, hipGetLastError(), "scatter_rect_kernel launch");
    }
  }
  if (to_device) {
    HIP_TRY(d, hipStreamSynchronize(d->stream));
    return MIJPEG_OK;
  }
  if (const int prc = ensure_pinned(d, &d->req_host, &d->req_host_cap, padded)) return prc;
  HIP_TRY(d, hipMemcpyAsync(d->req_host + (size_t)min_y * row, d->req_dev + (size_t)min_y * row, (size_t)y_count * row, hipMemcpyDeviceToHost,
                            d->stream));
  HIP_TRY(d, hipStreamSynchronize(d->stream));
  for (int c = min_comp; c <= max_comp; c++) {
    if (!dst[c] || cx1[c] < min_x || cy1[c] < min_y) continue;
    const int plane = vc >= 0 ? (all_on_view ? c : 0) : c;
    const int n = cx1[c] - min_x + 1;
    for (int y = min_y; y <= cy1[c]; y++) {
      const uint8_t *src = d->req_host + (size_t)y * row + ((size_t)min_x * nc + plane) * sb;
      uint8_t *out = (uint8_t *)dst[c] + (ptrdiff_t)y * bpr[c] + (ptrdiff_t)min_x * bpp[c];
      if (sb == 1)
        for (int x = 0; x < n; x++) out[(ptrdiff_t)x * bpp[c]] = src[(size_t)x * nc];
      else
        for (int x = 0; x < n; x++) memcpy(out + (ptrdiff_t)x * bpp[c], src + (size_t)x * nc * 2, 2);
    }
  }
  return MIJPEG_OK;
}

int mijpeg_display_rect(mijpeg_decoder *d, int32_t min_x, int32_t min_y, int32_t max_x, int32_t max_y, int32_t min_comp, int32_t max_comp,
                        uint32_t flags, const mijpeg_bitmap bitmaps[MIJPEG_MAX_COMPONENTS])
try {
  if (!d || !bitmaps) return MIJPEG_ERR_INVALID_PARAMETER;
  if (d->device < 0) return set_error(d, MIJPEG_ERR_DEVICE, "decoder was created without a device: no reconstruction path");
  if (!d->uploaded) return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "no decoded coefficients: call mijpeg_decode_coefficients first");
  const mijpeg_info &f = d->host.info;
  const bool to_device = (flags & MIJPEG_FLAG_DEVICE_OUTPUT) != 0;
  const bool upsample = !(flags & MIJPEG_FLAG_NO_UPSAMPLING);
  const bool ctrafo = !(flags & MIJPEG_FLAG_NO_COLOR_TRANSFORM);
  const uint32_t pass = flags & (MIJPEG_FLAG_FORCE_GENERIC | MIJPEG_FLAG_FORCE_SAFE);
  if (min_comp < 0) min_comp = 0;
  if (max_comp >= f.components) max_comp = f.components - 1;
  if (!upsample && min_comp != max_comp && min_comp <= max_comp)
    return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "if upsampling is disabled, components can only be reconstructed one by one");
  void *dst[MIJPEG_MAX_COMPONENTS];
  int32_t bpp[MIJPEG_MAX_COMPONENTS], bpr[MIJPEG_MAX_COMPONENTS];
  uint32_t bm_h[MIJPEG_MAX_COMPONENTS], bm_w[MIJPEG_MAX_COMPONENTS];
  for (int c = 0; c < MIJPEG_MAX_COMPONENTS; c++) {
    dst[c] = bitmaps[c].data;
    bpp[c] = bitmaps[c].bytes_per_pixel;
    bpr[c] = bitmaps[c].bytes_per_row;
    bm_w[c] = bitmaps[c].width;
    bm_h[c] = bitmaps[c].height;
  }
  if (d->host.is_xt()) {
    // JPEG XT: the residual image has row cursors and upsamplers of its own beside the legacy image's
    // (control/blockbitmaprequester.cpp:228-232, 356-372, 1118-1146, 1197-1222): one request model per image, fed the same
    // requests.  In the contract: what the reference's command line asks for -- all three components, upsampling and colour
    // transformation on -- with any order and size of rectangles.  (A component subset merges with whatever m_ppDTemp holds from
    // the block before, a request without the transformation builds another transformer: served as the plain picture.)
    const mijpeg_xt_params &x = d->host.xt;
    auto plain_picture = [&]() -> int {
      uint32_t maxmcu = 0xffffffffu;
      for (int c = min_comp; c <= max_comp; c++) maxmcu = std::min(maxmcu, (bm_h[c] >> 3) - 1u);
      if (maxmcu != 0xffffffffu && (int64_t)max_y > (int64_t)maxmcu * 8 + 7) max_y = (int32_t)(maxmcu * 8 + 7);
      if (max_y < min_y) return MIJPEG_OK;
      return mijpeg_reconstruct_rect(d, min_x, min_y, max_x, max_y, min_comp, max_comp, flags, dst, bpp, bpr);
    };
    if (!upsample || !ctrafo || min_comp != 0 || max_comp != 2 || f.components != 3) return plain_picture();
    const mijpeg_info &r = x.residual;
    ensure_request_models(d);
    const RequestPlan pl = d->model.request(min_x, min_y, max_x, max_y, 0, 2, true, true, bm_h);
    const RequestPlan pr = x.no_residual ? pl : d->rmodel.request(min_x, min_y, max_x, max_y, 0, 2, true, true, bm_h);
    if (pl.nothing) return MIJPEG_OK;
    // a residual component without an upsampler whose cursor stands behind its last row: `rrow->BlockAt(x)` on a NULL row
    // (:1057-1058, :1201-1202) -- the reference does not survive this request
    if (!x.no_residual)
      for (int c = 0; c < 3; c++)
        if (!(pr.upsampling_path && pr.upsampler[c]))
          for (int g = pr.g0[c]; g <= pr.g1[c]; g++)
            if (g >= (int)pr.rowmap[c].size() || pr.rowmap[c][(size_t)g] < 0)
              return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST,
                               "the request walks the residual image's row cursor behind its last row (the reference dereferences a NULL row here)");
    // BitmapCtrl::ExtractBitmap (interface/imagebitmap.cpp:58-129): blocks whose corner lies outside the bitmap the hook described
    // are not written
    int32_t cx1[MIJPEG_MAX_COMPONENTS], cy1[MIJPEG_MAX_COMPONENTS];
    for (int c = 0; c < 3; c++) {
      auto last_in = [](int32_t lo, int32_t hi, uint32_t extent) -> int32_t {
        if ((uint32_t)lo >= extent) return lo - 1;
        const int64_t last_block = ((int64_t)extent - 1) >> 3;
        return (int32_t)std::min<int64_t>(hi, std::max<int64_t>(last_block, lo >> 3) * 8 + 7);
      };
      cx1[c] = last_in(pl.min_x, pl.max_x, bm_w[c]);
      cy1[c] = last_in(pl.min_y, pl.max_y, bm_h[c]);
    }
    if (pl.plain && (x.no_residual || pr.plain)) {
      for (int c = 0; c <= 2;) { // components with the same writable extent go out together (all of them, normally)
        int e = c;
        while (e + 1 <= 2 && cx1[e + 1] == cx1[c] && cy1[e + 1] == cy1[c]) e++;
        if (cx1[c] >= pl.min_x && cy1[c] >= pl.min_y) {
          const int rc = mijpeg_reconstruct_rect(d, pl.min_x, pl.min_y, cx1[c], cy1[c], c, e, flags, dst, bpp, bpr);
          if (rc) return rc;
        }
        c = e + 1;
      }
      return MIJPEG_OK;
    }
    // ---- not the plain picture: both images through the unfused kernels with their row maps on this request's lines
    HIP_TRY(d, hipSetDevice(d->device));
    mijpeg_batch b;
    memset(&b, 0, sizeof(b));
    b.info = f;
    b.xt = &x;
    const int sb = f.sample_bytes > 0 ? f.sample_bytes : 2;
    const size_t row = ((size_t)f.width * 3 * sb + 7) & ~(size_t)7, padded = row * f.height;
    int rc = ensure_dev(d, (void **)&d->req_dev, &d->req_dev_cap, padded);
    if (rc) return rc;
    int stride = 1;
    for (int c = 0; c < 3; c++) stride = std::max(stride, std::max(f.blocks_h[c], r.blocks_h[c]));
    std::vector<int32_t> maps((size_t)6 * stride);
    for (int pn = 0; pn < 6; pn++) {
      const RequestPlan &p = pn < 3 ? pl : pr;
      const int c = pn % 3;
      int32_t *m = maps.data() + (size_t)pn * stride;
      for (int g = 0; g < stride; g++) m[g] = g;
      if (pn >= 3 && x.no_residual) continue;
      for (int g = p.g0[c]; g <= p.g1[c] && g < stride && g < (int)p.rowmap[c].size(); g++) m[g] = p.rowmap[c][(size_t)g];
    }
    rc = ensure_dev(d, (void **)&d->rowmap_dev, &d->rowmap_cap, maps.size() * sizeof(int32_t));
    if (rc) return rc;
    HIP_TRY(d, hipMemcpyAsync(d->rowmap_dev, maps.data(), maps.size() * sizeof(int32_t), hipMemcpyHostToDevice, d->stream));
    HIP_TRY(d, hipStreamSynchronize(d->stream)); // `maps` is pageable and leaves scope
    b.coef_dev = d->coef_dev;
    b.coef_frame_stride = f.coef_count;
    b.out_dev = d->req_dev;
    b.out_row_stride = (int64_t)row;
    b.out_frame_stride = (int64_t)padded;
    b.frames = 1;
    b.flags = pass | MIJPEG_FLAG_FORCE_GENERIC;
    const size_t ws = mijpeg_workspace_bytes(&b);
    if (ws) {
      rc = ensure_dev(d, (void **)&d->ws_dev, &d->ws_cap, ws);
      if (rc) return rc;
      b.workspace = d->ws_dev;
      b.workspace_bytes = d->ws_cap;
    }
    const int y_count = pl.max_y - pl.min_y + 1;
    RequestExtra rx;
    memset(&rx, 0, sizeof(rx));
    rx.rowmap_dev = d->rowmap_dev;
    rx.rowmap_stride = stride;
    rx.corner_x = pl.corner_x;
    rx.corner_y = pl.corner_y;
    rx.y_base = pl.min_y;
    rx.y_count = y_count;
    rx.ycc = 1;
    for (int pn = 0; pn < 6; pn++) {
      const RequestPlan &p = pn < 3 ? pl : pr;
      const mijpeg_info &g = pn < 3 ? f : r;
      const int c = pn % 3;
      const bool up = p.upsampling_path && p.upsampler[c] && !(pn >= 3 && x.no_residual);
      rx.wstart[pn] = up ? p.wstart[c] : 0;
      rx.wlimit[pn] = up ? p.wlimit[c] : (f.height + g.suby[c] - 1) / std::max(1, g.suby[c]);
    }
    rc = launch_reconstruct_ex(&b, d->stream, &rx);
    if (rc) return set_error(d, rc, rc == MIJPEG_ERR_DEVICE ? std::string("kernel launch failed: ") + hipGetErrorString(hipGetLastError())
                                                             : std::string("reconstruction not available for this request"));
    return hand_out_request(d, pl.min_x, pl.min_y, y_count, cx1, cy1, 0, 2, 3, sb, row, padded, -1, false, to_device, dst, bpp, bpr);
  }
  ensure_request_models(d);
  const RequestPlan p = d->model.request(min_x, min_y, max_x, max_y, min_comp, max_comp, upsample, ctrafo, bm_h);
  if (p.nothing) return MIJPEG_OK;
  // BitmapCtrl::ExtractBitmap (interface/imagebitmap.cpp:58-129): a block whose corner lies outside the bitmap the hook
  // described is blank -- nothing of it is written; one that starts inside is written in full
  int32_t cx1[MIJPEG_MAX_COMPONENTS], cy1[MIJPEG_MAX_COMPONENTS];
  auto last_inside = [](int32_t lo, int32_t hi, uint32_t extent) -> int32_t { // last sample of the blocks whose corner is below extent
    if ((uint32_t)lo >= extent) return lo - 1;
    const int64_t last_block = ((int64_t)extent - 1) >> 3; // the last block whose (aligned) corner is inside
    return (int32_t)std::min<int64_t>(hi, std::max<int64_t>(last_block, lo >> 3) * 8 + 7);
  };
  for (int c = 0; c < f.components; c++) {
    cx1[c] = last_inside(p.min_x, p.max_x, bm_w[c]);
    cy1[c] = last_inside(p.min_y, p.max_y, bm_h[c]);
  }
  const int vc = p.view; // without upsampling the single component of the view is number 0 there
  if (p.plain) {
    const uint32_t fl = pass | (p.ycc || !f.ycbcr ? 0u : MIJPEG_FLAG_NO_COLOR_TRANSFORM) | (vc >= 0 ? MIJPEG_FLAG_NO_COLOR_TRANSFORM : 0u);
    // components with the same writable extent go out together (all of them, normally: one interleaved copy)
    for (int c = min_comp; c <= max_comp;) {
      int e = c;
      while (e + 1 <= max_comp && cx1[e + 1] == cx1[c] && cy1[e + 1] == cy1[c]) e++;
      if (cx1[c] >= p.min_x && cy1[c] >= p.min_y) {
        int rc;
        if (vc >= 0) {
          void *vdst[MIJPEG_MAX_COMPONENTS] = {dst[vc], nullptr, nullptr, nullptr};
          int32_t vbpp[MIJPEG_MAX_COMPONENTS] = {bpp[vc], 0, 0, 0}, vbpr[MIJPEG_MAX_COMPONENTS] = {bpr[vc], 0, 0, 0};
          rc = serve_rect(d, vc, fl, to_device, p.min_x, p.min_y, cx1[c], cy1[c], 0, 0, vdst, vbpp, vbpr);
        } else
          rc = serve_rect(d, -1, fl, to_device, p.min_x, p.min_y, cx1[c], cy1[c], c, e, dst, bpp, bpr);
        if (rc) return rc;
      }
      c = e + 1;
    }
    return MIJPEG_OK;
  }
  // ---- not the plain picture: row maps, zeros, displaced upsampler output -> the generic kernels on this request's lines
  HIP_TRY(d, hipSetDevice(d->device));
  const bool all_on_view = vc >= 0 && p.ycc;
  mijpeg_batch b;
  memset(&b, 0, sizeof(b));
  b.info = request_frame(f, vc, all_on_view);
  b.info.ycbcr = p.ycc ? 1 : 0;
  const mijpeg_info &g = b.info;
  const int nc = g.components, sb = g.sample_bytes > 0 ? g.sample_bytes : 1;
  const size_t row = ((size_t)g.width * nc * sb + 7) & ~(size_t)7, padded = row * g.height;
  int rc = ensure_dev(d, (void **)&d->req_dev, &d->req_dev_cap, padded);
  if (rc) return rc;
  // row maps: identity outside what the plan defines; components that were not asked for are zeros
  int stride = 1;
  for (int c = 0; c < nc; c++) stride = std::max(stride, g.blocks_h[c]);
  std::vector<int32_t> maps((size_t)nc * stride);
  bool all_zero = !p.ycc;
  for (int c = 0; c < nc; c++) {
    const int pc = vc >= 0 ? (all_on_view ? c : vc) : c; // component of the frame behind plane c of the request frame
    int32_t *m = maps.data() + (size_t)c * stride;
    for (int r = 0; r < stride; r++) m[r] = r;
    if (!p.requested[pc]) {
      for (int r = 0; r < stride; r++) m[r] = -1;
      continue;
    }
    // (a component that appears in no scan carries coefficients that transform to zeros in every row: host_decoder.cpp)
    for (int r = p.g0[pc]; r <= p.g1[pc] && r < stride && r < (int)p.rowmap[pc].size(); r++) {
      m[r] = p.rowmap[pc][(size_t)r];
      if (m[r] >= 0) all_zero = false;
    }
  }
  const int y_count = p.max_y - p.min_y + 1;
  if (all_zero) {
    // every sample the request shows is the transform of "no row": 0 through the filters and the identity transformation
    HIP_TRY(d, hipMemsetAsync(d->req_dev + (size_t)p.min_y * row, 0, (size_t)y_count * row, d->stream));
  } else {
    rc = ensure_dev(d, (void **)&d->rowmap_dev, &d->rowmap_cap, maps.size() * sizeof(int32_t));
    if (rc) return rc;
    HIP_TRY(d, hipMemcpyAsync(d->rowmap_dev, maps.data(), maps.size() * sizeof(int32_t), hipMemcpyHostToDevice, d->stream));
    HIP_TRY(d, hipStreamSynchronize(d->stream)); // `maps` is pageable and leaves scope; uploads of the coefficients are complete too
    b.coef_dev = d->coef_dev + (vc >= 0 && !all_on_view ? f.coef_offset[vc] : 0);
    b.coef_frame_stride = g.coef_count;
    b.out_dev = d->req_dev;
    b.out_row_stride = (int64_t)row;
    b.out_frame_stride = (int64_t)padded;
    b.frames = 1;
    b.flags = pass | MIJPEG_FLAG_FORCE_GENERIC | (p.ycc ? 0u : MIJPEG_FLAG_NO_COLOR_TRANSFORM);
    const size_t ws = mijpeg_workspace_bytes(&b);
    if (ws) {
      rc = ensure_dev(d, (void **)&d->ws_dev, &d->ws_cap, ws);
      if (rc) return rc;
      b.workspace = d->ws_dev;
      b.workspace_bytes = d->ws_cap;
    }
    RequestExtra rx;
    memset(&rx, 0, sizeof(rx));
    rx.rowmap_dev = d->rowmap_dev;
    rx.rowmap_stride = stride;
    rx.corner_x = p.corner_x;
    rx.corner_y = p.corner_y;
    rx.y_base = p.min_y;
    rx.y_count = y_count;
    rx.ycc = p.ycc ? 1 : 0;
    for (int c = 0; c < nc; c++) {
      const int pc = vc >= 0 ? vc : c;
      const bool up = vc < 0 && p.upsampling_path && p.upsampler[pc] && p.requested[pc];
      rx.wstart[c] = up ? p.wstart[pc] : 0;
      rx.wlimit[c] = up ? p.wlimit[pc] : (g.dnl && g.suby[c] > 1) ? g.blocks_h[c] * 8 : (g.height + g.suby[c] - 1) / g.suby[c];
    }
    rc = launch_reconstruct_ex(&b, d->stream, &rx);
    if (rc) return set_error(d, rc, rc == MIJPEG_ERR_DEVICE ? std::string("kernel launch failed: ") + hipGetErrorString(hipGetLastError())
                                                             : std::string("reconstruction not available for this request"));
  }
  return hand_out_request(d, p.min_x, p.min_y, y_count, cx1, cy1, min_comp, max_comp, nc, sb, row, padded, vc, all_on_view, to_device, dst, bpp, bpr);
} catch (...) { return boundary_catch(d, "mijpeg_display_rect"); }

// The scans of one codestream in the order the reference meets them: the codestream's own, then the ones that live in its
// refinement boxes.  A frame whose decode went through the sequential walk (damaged streams, DNL frames, the residual scan types of
// part 8) planned no scans: the walk's own record stands in (HostDecoder::walked_scans).
struct ScanStop { uint64_t begin, end; int32_t mcus_x, mcus_y; bool boxed; };
static void scans_of(const HostDecoder &h, bool all_boxed, std::vector<ScanStop> &out)
{
  if (h.walked()) {
    for (const auto &w : h.walked_scans()) out.push_back(ScanStop{(uint64_t)w.begin, (uint64_t)w.end, w.mcus_x, w.mcus_y, all_boxed || w.boxed});
    return;
  }
  for (const Scan &sc : h.scans)
    if (!sc.base) out.push_back(ScanStop{(uint64_t)sc.ecs_begin, (uint64_t)sc.ecs_end, sc.mcus_x, sc.mcus_y, all_boxed});
  for (const Scan &sc : h.scans)
    if (sc.base) out.push_back(ScanStop{0, 0, sc.mcus_x, sc.mcus_y, true});
}
static void all_scans(mijpeg_decoder *d, std::vector<ScanStop> &out)
{
  // scans of the codestream itself first; then -- JPEG XT -- the scans that live in boxes (hidden refinement scans of the legacy
  // frame, the residual codestream and its refinement scans): the reference parses them from memory streams while its input
  // stands at the marker behind the legacy frame's last scan (the EOI); behind them the alpha channel's: its own codestream (ALFA
  // box), that one's refinement boxes, its residual codestream (Image::ParseAlphaChannel / ParseResidualStream of the alpha image,
  // codestream/image.cpp:1337-1404, 1440-1462)
  scans_of(d->host, false, out);
  if (HostDecoder *res = d->host.residual()) scans_of(*res, true, out);
  if (d->alpha && d->alpha_ready) {
    scans_of(d->alpha->host, true, out);
    if (HostDecoder *ares = d->alpha->host.residual()) scans_of(*ares, true, out);
  }
}

int mijpeg_scan_offsets(mijpeg_decoder *d, uint64_t *first_byte, uint64_t *end_byte, int capacity)
try {
  if (!d) return MIJPEG_ERR_INVALID_PARAMETER;
  std::vector<ScanStop> all;
  all_scans(d, all);
  // (boxed scans: the input stands behind the last scan of the codestream itself; end 0 marks them)
  int n = 0;
  uint64_t behind = 0;
  for (const ScanStop &sc : all) {
    if (sc.boxed) continue;
    if (n < capacity) {
      if (first_byte) first_byte[n] = sc.begin;
      if (end_byte) end_byte[n] = sc.end;
    }
    behind = sc.end;
    n++;
  }
  for (const ScanStop &sc : all) {
    if (!sc.boxed) continue;
    if (n < capacity) {
      if (first_byte) first_byte[n] = behind;
      if (end_byte) end_byte[n] = 0;
    }
    n++;
  }
  return n;
} catch (...) { return boundary_catch(d, "mijpeg_scan_offsets"); }

int mijpeg_scan_grids(mijpeg_decoder *d, int32_t *mcus_x, int32_t *mcus_y, int capacity)
try {
  if (!d) return MIJPEG_ERR_INVALID_PARAMETER;
  std::vector<ScanStop> all;
  all_scans(d, all);
  int n = 0;
  for (int boxed = 0; boxed < 2; boxed++) // (the same order as mijpeg_scan_offsets)
    for (const ScanStop &sc : all) {
      if ((int)sc.boxed != boxed) continue;
      if (n < capacity) {
        if (mcus_x) mcus_x[n] = sc.mcus_x;
        if (mcus_y) mcus_y[n] = sc.mcus_y;
      }
      n++;
    }
  return n;
} catch (...) { return boundary_catch(d, "mijpeg_scan_grids"); }

int mijpeg_display_plan(mijpeg_decoder *d, int32_t min_x, int32_t min_y, int32_t max_x, int32_t max_y, int32_t min_comp, int32_t max_comp,
                        uint32_t flags, const uint32_t bm_height[MIJPEG_MAX_COMPONENTS], int32_t out[8 + 6 * MIJPEG_MAX_COMPONENTS])
try {
  if (!d || !bm_height || !out) return MIJPEG_ERR_INVALID_PARAMETER;
  if (d->host.info.components < 1 || d->host.info.width < 1) return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "no parsed stream: call mijpeg_read_header first");
  const mijpeg_info &f = d->host.info;
  ensure_request_models(d);
  const RequestPlan p = d->model.request(min_x, min_y, max_x, max_y, min_comp, max_comp, !(flags & MIJPEG_FLAG_NO_UPSAMPLING),
                                         !(flags & MIJPEG_FLAG_NO_COLOR_TRANSFORM), bm_height);
  bool rplain = true;
  if (d->host.is_xt() && f.components == 3 && !d->host.xt.no_residual) // (the residual image: cursors through mijpeg_display_cursor(4 + c))
    rplain = d->rmodel.request(min_x, min_y, max_x, max_y, min_comp, max_comp, !(flags & MIJPEG_FLAG_NO_UPSAMPLING),
                               !(flags & MIJPEG_FLAG_NO_COLOR_TRANSFORM), bm_height).plain;
  out[0] = p.nothing; out[1] = p.plain && rplain; out[2] = p.ycc; out[3] = p.view;
  out[4] = p.min_x; out[5] = p.min_y; out[6] = p.max_x; out[7] = p.max_y;
  for (int c = 0; c < MIJPEG_MAX_COMPONENTS; c++) {
    int32_t *o = out + 8 + 6 * c;
    o[0] = d->model.cursor(c); o[1] = p.g0[c]; o[2] = p.g1[c]; o[3] = p.wstart[c]; o[4] = p.wlimit[c];
    int zeros = 0;
    for (int g = p.g0[c]; g <= p.g1[c] && g < (int)p.rowmap[c].size(); g++) zeros += p.rowmap[c][(size_t)g] < 0;
    o[5] = zeros;
  }
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_display_plan"); }

int mijpeg_display_cursor(mijpeg_decoder *d, int component)
try {
  if (!d || component < 0 || component >= 2 * MIJPEG_MAX_COMPONENTS || !d->model_valid) return 0;
  return component >= MIJPEG_MAX_COMPONENTS ? d->rmodel.cursor(component - MIJPEG_MAX_COMPONENTS) : d->model.cursor(component);
} catch (...) { return boundary_catch(d, "mijpeg_display_cursor"); }

} // extern "C"
