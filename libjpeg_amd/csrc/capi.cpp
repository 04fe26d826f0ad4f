// capi.cpp -- the C ABI of include/mijpeg.h: decoder object (host entropy decoding + streaming upload +
// GPU reconstruction of whole frames), its buffer cache and its queries.  Uniform batches are in batch_decode.cpp, the kernel
// selection and the launch in reconstruct_device.cpp, the rectangle service in rect_service.cpp, ragged batches in ragged_decode.cpp and
// ragged_reconstruct.cpp, the encoder direction in encode_device.cpp.  Compiled with hipcc (host side only uses the HIP runtime API).  There is NO CPU fallback for the
// reconstruction: without a device the reconstruct calls fail with MIJPEG_ERR_DEVICE.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <memory>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>

#include "../../include/mijpeg.h"
#include "decoder.hpp"
#include "huffman_dev.hpp"
#include "kernels.hpp"
#include "reconstruct.hpp"

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
int ensure_cached(mijpeg_decoder *d, bool pinned, void **ptr, size_t *cap, size_t bytes)
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

// The coefficient store for `count` int16: the device mirror and, where need_host, the (pinned) host planes
int ensure_coef_store(mijpeg_decoder *d, size_t count, bool need_host)
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

// A batch that was submitted (mijpeg_submit_batch_device) and not waited for still reads the pinned staging buffers
// (ent_host, stage_host, status words) from its asynchronous uploads: every entry point that rewrites them settles it first.
int settle_pending(mijpeg_decoder *d)
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
    if (d->planar_tmp_dev) (void)hipFree(d->planar_tmp_dev);
    if (d->rect_tmp_dev) (void)hipFree(d->rect_tmp_dev);
    if (d->batch_quant_dev) (void)hipFree(d->batch_quant_dev);
    if (d->ent_dev) (void)hipFree(d->ent_dev);
    if (d->ent_host) (void)hipHostFree(d->ent_host);
    if (d->stage_host) (void)hipHostFree(d->stage_host);
    if (d->walk_dev) (void)hipFree(d->walk_dev);
    if (d->xt_helper) mijpeg_destroy(d->xt_helper);
    pinned_upload_release(d->list_tables);
    if (d->resized_arena_dev) (void)hipFree(d->resized_arena_dev);
    pinned_upload_release(d->resample_tables);
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

// Block rows [y0, y1) of component c of a JPEG XT frame's residual planes (they sit behind the legacy planes in the same store)
// on their way to the device, on the object's stream
static hipError_t upload_residual_rows(mijpeg_decoder *d, int c, int y0, int y1)
{
  const mijpeg_xt_params &x = d->host.xt;
  const size_t row = (size_t)x.residual.blocks_w[c] * 64 * (x.residual_wide ? 2 : 1); // int16 units per block row
  const size_t off = (size_t)x.residual.coef_offset[c] + row * (size_t)y0;
  return hipMemcpyAsync(d->coef_dev + off, d->coef_host + off, row * (size_t)(y1 - y0) * sizeof(int16_t), hipMemcpyHostToDevice, d->stream);
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
      const hipError_t e = upload_residual_rows(d, c, y0, y1);
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
        if (y0 < y1) copy_err = upload_residual_rows(d, c, y0, y1);
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

static int decode_coefficients_device(mijpeg_decoder *d, int min_intervals, bool markers)
{
  if (d->device < 0) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "decoder was created without a device");
  HIP_TRY(d, hipSetDevice(d->device));
  if (const int prc = settle_pending(d)) return prc;
  using clk = std::chrono::steady_clock;
  const auto t0 = clk::now();
  d->parse_fresh = false;
  if (markers) d->host.set_skip_search(); // (headers only: the device searches the segment)
  int rc = d->host.parse(d->data, d->size, false);
  if (rc) return set_error(d, rc, d->host.error.message);
  d->parsed = true;
  d->batch_frames = 0;
  const auto t_parsed = clk::now();
  HostDecoder *h = &d->host, *res = d->host.residual();
  if (markers) {
    const char *why = res ? "device marker search: plain 8-bit frames only" : device_markers_obstacle(d->host, d->size);
    // This call keeps what it did for a stream without restart markers: the ordinary route, host search included (the batch
    // calls and the ragged calls are where such streams are searched on the device)
    if (!why && d->host.scans[0].restart_interval <= 0) why = "device marker search: the single-image call searches streams without restart markers on the host";
    if (why) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, why);
  }
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
    EntropyBatchOptions opt;
    opt.markers = markers;
    rc = device_entropy_batch(d, &h, &d->data, &d->size, 1, min_intervals, d->coef_dev, own_count, opt);
  } else {
    // JPEG XT: the two codestreams are independent, so the residual one is decoded at the same time by a helper object
    // (own stream, own buffers) on a thread of its own, straight into the planes behind the legacy frame's
    if (!d->xt_helper && mijpeg_create(&d->xt_helper, d->device) != MIJPEG_OK) return set_error(d, MIJPEG_ERR_OUT_OF_MEMORY, "no helper decoder for the residual codestream");
    const uint8_t *rdata = res->stream_base();
    const size_t rsize = res->stream_size();
    EntropyBatchOptions opt;
    opt.xt_part = true;
    int rc2 = MIJPEG_OK;
    std::thread helper([&]() {
      try {
        if (hipSetDevice(d->device) != hipSuccess) { rc2 = MIJPEG_ERR_DEVICE; return; }
        rc2 = device_entropy_batch(d->xt_helper, &res, &rdata, &rsize, 1, min_intervals, d->coef_dev + own_count, res->info.coef_count, opt);
      } catch (...) { // (nothing may leave a thread's function)
        rc2 = boundary_catch(d->xt_helper, "residual codestream, device entropy decoding");
      }
    });
    struct Joiner { // (an exception on this thread must not meet a joinable thread object)
      std::thread &t;
      ~Joiner() { if (t.joinable()) t.join(); }
    } joiner{helper};
    rc = device_entropy_batch(d, &h, &d->data, &d->size, 1, min_intervals, d->coef_dev, own_count, opt);
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
}

int mijpeg_decode_coefficients_device(mijpeg_decoder *d, int min_intervals)
try {
  if (!d) return MIJPEG_ERR_INVALID_PARAMETER;
  if (!d->data) return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "no input stream has been set");
  if (d->device < 0) return set_error(d, MIJPEG_ERR_NOT_AVAILABLE, "decoder was created without a device");
  return with_device_markers(d, 1, [&](bool markers) { return decode_coefficients_device(d, min_intervals, markers); });
} catch (...) { return boundary_catch(d, "mijpeg_decode_coefficients_device"); }

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
// decoder-object reconstruction
// ------------------------------------------------------------------------------------------------
int mijpeg_reconstruct_device(mijpeg_decoder *d, void *dst_device, int64_t row_stride, uint32_t flags, int sync)
try {
  if (!d) return MIJPEG_ERR_INVALID_PARAMETER;
  if (d->device < 0) return set_error(d, MIJPEG_ERR_DEVICE, "decoder was created without a device: no reconstruction path");
  if (!d->uploaded) return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "no decoded coefficients: call mijpeg_decode_coefficients first");
  if (!dst_device) return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "destination pointer is NULL");
  return reconstruct_view(d, -1, dst_device, row_stride, flags & ~(MIJPEG_FLAG_DEVICE_OUTPUT | MIJPEG_FLAG_NO_UPSAMPLING), sync);
} catch (...) { return boundary_catch(d, "mijpeg_reconstruct_device"); }

int mijpeg_reconstruct_planar_device(mijpeg_decoder *d, void *const planes[MIJPEG_MAX_COMPONENTS], int64_t row_stride, uint32_t flags, int sync)
try {
  if (!d || !planes) return MIJPEG_ERR_INVALID_PARAMETER;
  if (d->parsed && planar_check(d->host.info, planes, row_stride))
    return set_error(d, MIJPEG_ERR_INVALID_PARAMETER, "planar destination: a plane pointer is NULL or the row stride is smaller than a line of samples");
  if (d->device < 0) return set_error(d, MIJPEG_ERR_DEVICE, "decoder was created without a device: no reconstruction path");
  if (!d->uploaded) return set_error(d, MIJPEG_ERR_OBJECT_DOESNT_EXIST, "no decoded coefficients: call mijpeg_decode_coefficients first");
  HIP_TRY(d, hipSetDevice(d->device));
  d->planar_stats = mijpeg_planar_stats{};
  PlanarItem it;
  it.info = &d->host.info;
  it.coef_dev = d->coef_dev;
  for (int c = 0; c < MIJPEG_MAX_COMPONENTS; c++) it.planes[c] = c < d->host.info.components ? planes[c] : nullptr;
  it.row_stride = row_stride;
  it.xt = d->host.is_xt() ? &d->host.xt : nullptr;
  RaggedFailures failures;
  const int rc = reconstruct_planar_items(d, &it, 1, flags & PLANAR_FLAGS, failures);
  if (rc) return set_error(d, rc, rc == MIJPEG_ERR_DEVICE ? "planar reconstruction: a kernel launch failed" : "planar reconstruction not available for this stream");
  d->planar_stats.images = 1;
  if (sync) HIP_TRY(d, hipStreamSynchronize(d->stream));
  return MIJPEG_OK;
} catch (...) { return boundary_catch(d, "mijpeg_reconstruct_planar_device"); }

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

} // extern "C"
