// rect_request_tables.cpp -- the device-free half of the rectangle service (libjpeg_amd/csrc/rect_request.hpp) as a program of its
// own, for the sanitizers: the extents rule of BitmapCtrl::ExtractBitmap against its brute-force statement, row maps and filter
// windows of real RequestModel sequences written into heap buffers of exactly their size, the strided host copy into destinations
// that end with the rectangle's last byte, the bands and slabs of the cached frame's download.  No device, nothing of the library
// is linked.  (tests/test_rect_request_cpu.py builds it with -fsanitize=address,undefined and runs it.)
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "rect_request.hpp"

using namespace mij;

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      if (failures++ < 40) fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
    }                                                                      \
  } while (0)

// ------------------------------------------------------------------------------------------------ extents
// oracle/jpeg_oracle.c:2407-2409: a sample is written iff the corner of the block it lies in is below the extent; the first block's
// corner is the request's own (lo), every later one's is 8-aligned
static void check_extents()
{
  std::vector<uint32_t> extents;
  for (uint32_t e = 0; e <= 48; e++) extents.push_back(e);
  extents.push_back(0x7fffffffu);
  for (int lo = 0; lo <= 40; lo++)
    for (int hi = lo; hi <= 47; hi++)
      for (uint32_t extent : extents) {
        int last = lo - 1;
        for (int x = lo; x <= hi; x++) {
          const int corner = (x >> 3) == (lo >> 3) ? lo : (x & ~7);
          if ((uint32_t)corner < extent) last = x;
        }
        CHECK(last_inside(lo, hi, extent) == last);
      }
  RequestPlan p;
  p.min_x = 3; p.max_x = 40; p.min_y = 8; p.max_y = 30;
  const uint32_t bw[4] = {9, 0, 100, 4}, bh[4] = {100, 100, 17, 8};
  int32_t cx1[4], cy1[4];
  writable_extents(p, bw, bh, 4, cx1, cy1);
  CHECK(cx1[0] == 15 && cx1[1] == 2 && cx1[2] == 40 && cx1[3] == 7);
  CHECK(cy1[0] == 30 && cy1[1] == 30 && cy1[2] == 23 && cy1[3] == 7);
  const int32_t ex[4] = {5, 5, 7, 5}, ey[4] = {9, 9, 9, 9};
  CHECK(extent_run_end(ex, ey, 0, 3) == 1 && extent_run_end(ex, ey, 2, 3) == 2 && extent_run_end(ex, ey, 3, 3) == 3 && extent_run_end(ex, ey, 0, 0) == 0);
}

// ------------------------------------------------------------------------------------------------ row maps and windows
// A frame description as the parser leaves it: sampling factors (hs[c], vs[c]) per component
static mijpeg_info frame(int w, int h, int components, const int *hs, const int *vs, bool ycbcr)
{
  mijpeg_info f;
  memset(&f, 0, sizeof(f));
  int hmax = 1, vmax = 1;
  for (int c = 0; c < components; c++) { hmax = std::max(hmax, hs[c]); vmax = std::max(vmax, vs[c]); }
  f.width = w; f.height = h; f.components = components; f.precision = 8; f.ycbcr = ycbcr; f.sample_bytes = 1;
  f.mcus_x = (w + 8 * hmax - 1) / (8 * hmax); f.mcus_y = (h + 8 * vmax - 1) / (8 * vmax);
  int64_t at = 0;
  for (int c = 0; c < components; c++) {
    f.hsamp[c] = hs[c]; f.vsamp[c] = vs[c];
    f.subx[c] = hmax / hs[c]; f.suby[c] = vmax / vs[c];
    f.blocks_w[c] = f.mcus_x * hs[c]; f.blocks_h[c] = f.mcus_y * vs[c];
    f.coef_offset[c] = at;
    at += (int64_t)f.blocks_w[c] * f.blocks_h[c] * 64;
  }
  f.coef_count = at;
  return f;
}

struct Seen { int zeros = 0, absent = 0, all_zero = 0, moved = 0, windowed = 0, identity = 0, requests = 0; };
static Seen seen;

// The maps of the planes into a heap buffer of exactly n * stride entries, and what the launch takes beside them
static void check_launch(const RequestPlane *planes, int n, const RequestPlan &place, int stride, bool ycc)
{
  int32_t *maps = (int32_t *)malloc((size_t)n * stride * sizeof(int32_t));
  bool all_zero = false, any_row = false;
  fill_rowmaps(planes, n, stride, ycc, maps, &all_zero);
  for (int k = 0; k < n; k++) {
    const RequestPlan &p = *planes[k].plan;
    const int c = planes[k].comp;
    for (int g = 0; g < stride; g++) {
      const bool planned = !planes[k].identity && g >= p.g0[c] && g <= p.g1[c] && g < (int)p.rowmap[c].size();
      const int32_t want = !planes[k].present ? -1 : planned ? p.rowmap[c][(size_t)g] : g;
      CHECK(maps[(size_t)k * stride + g] == want);
      if (planes[k].present && planned) {
        any_row = any_row || want >= 0;
        seen.zeros += want < 0;
        seen.moved += want >= 0 && want != g;
      }
    }
    seen.absent += !planes[k].present;
    seen.identity += planes[k].identity;
  }
  CHECK(all_zero == (!any_row && !ycc));
  seen.all_zero += all_zero;
  const int y_count = place.max_y - place.min_y + 1;
  const RequestExtra rx = request_extra(planes, n, place, stride, y_count, ycc);
  CHECK(rx.rowmap_dev == nullptr && rx.rowmap_stride == stride && rx.corner_x == place.corner_x && rx.corner_y == place.corner_y);
  CHECK(rx.y_base == place.min_y && rx.y_count == y_count && rx.ycc == (ycc ? 1 : 0));
  for (int k = 0; k < MAXP; k++) {
    if (k >= n) { CHECK(rx.wstart[k] == 0 && rx.wlimit[k] == 0); continue; }
    const RequestPlan &p = *planes[k].plan;
    CHECK(rx.wstart[k] == (planes[k].windowed ? p.wstart[planes[k].comp] : 0));
    CHECK(rx.wlimit[k] == (planes[k].windowed ? p.wlimit[planes[k].comp] : planes[k].lines));
    seen.windowed += planes[k].windowed && p.wstart[planes[k].comp] > 0;
  }
  free(maps);
  seen.requests++;
}

struct Call { int x0, y0, x1, y1, c0, c1; bool upsample, ctrafo; uint32_t bm_height; };

// One sequence of requests on a plain frame through a fresh model, as mijpeg_display_rect sends it
static void run_plain(const mijpeg_info &f, const std::vector<Call> &calls)
{
  RequestModel model;
  model.reset(f.components, f.width, f.height, f.subx, f.suby, f.ycbcr != 0, f.dnl != 0, f.rows, f.blocks_h);
  for (const Call &q : calls) {
    const uint32_t bm_h[4] = {q.bm_height, q.bm_height, q.bm_height, q.bm_height};
    const RequestPlan p = model.request(q.x0, q.y0, q.x1, q.y1, q.c0, q.c1, q.upsample, q.ctrafo, bm_h);
    if (p.nothing) continue;
    const int vc = p.view;
    const bool all_on_view = vc >= 0 && p.ycc;
    const mijpeg_info g = request_frame(f, vc, all_on_view);
    RequestPlane planes[MAXP];
    const int n = plain_planes(p, g, all_on_view, planes);
    CHECK(n == (vc >= 0 && !all_on_view ? 1 : f.components));
    int stride = 1;
    for (int c = 0; c < n; c++) {
      stride = std::max(stride, g.blocks_h[c]);
      const int pc = vc < 0 ? c : all_on_view ? c : vc;
      CHECK(planes[c].plan == &p && planes[c].comp == pc && planes[c].present == p.requested[pc] && !planes[c].identity);
      CHECK(planes[c].windowed == (vc < 0 && p.upsampling_path && p.upsampler[c] && p.requested[c]));
      // off the upsampling path the filters end with the component: its lines on the canvas, or the view's own
      // (a DNL frame's upsamplers never learnt the height: the block rows of a vertically subsampled component end them)
      CHECK(planes[c].lines == (vc >= 0 ? (f.height + f.suby[vc] - 1) / f.suby[vc] : f.dnl && f.suby[c] > 1 ? f.blocks_h[c] * 8 : (f.height + f.suby[c] - 1) / f.suby[c]));
    }
    const RequestImage im = request_image(g, 1, vc, all_on_view);
    CHECK(im.nc == n && im.sb == 1 && im.row % 8 == 0 && im.row >= (size_t)g.width * n && im.row < (size_t)g.width * n + 8 && im.padded == im.row * g.height);
    for (int c = 0; c < f.components; c++) CHECK(im.plane_of[c] == (vc < 0 || all_on_view ? c : 0));
    check_launch(planes, n, p, stride, p.ycc);
  }
}

// ... and on a JPEG XT frame: one model per image, fed the same requests (all three components, upsampling and transformation on)
static void run_xt(const mijpeg_info &f, const mijpeg_info &r, bool no_residual, const std::vector<Call> &calls)
{
  RequestModel model, rmodel;
  bool lsub = false, rsub = false;
  for (int c = 0; c < 3; c++) {
    lsub = lsub || f.subx[c] > 1 || f.suby[c] > 1;
    rsub = rsub || r.subx[c] > 1 || r.suby[c] > 1;
  }
  model.reset(3, f.width, f.height, f.subx, f.suby, true, false, nullptr, nullptr, rsub);
  rmodel.reset(3, f.width, f.height, r.subx, r.suby, true, false, nullptr, nullptr, lsub);
  for (const Call &q : calls) {
    const uint32_t bm_h[4] = {q.bm_height, q.bm_height, q.bm_height, q.bm_height};
    const RequestPlan pl = model.request(q.x0, q.y0, q.x1, q.y1, 0, 2, true, true, bm_h);
    const RequestPlan pr = no_residual ? pl : rmodel.request(q.x0, q.y0, q.x1, q.y1, 0, 2, true, true, bm_h);
    if (pl.nothing) continue;
    RequestPlane planes[MAXP];
    CHECK(xt_planes(pl, pr, f, r, no_residual, planes) == 6);
    int stride = 1;
    for (int c = 0; c < 3; c++) stride = std::max(stride, std::max(f.blocks_h[c], r.blocks_h[c]));
    for (int k = 0; k < 6; k++) {
      const RequestPlan &p = k < 3 ? pl : pr;
      const mijpeg_info &g = k < 3 ? f : r;
      CHECK(planes[k].plan == &p && planes[k].comp == k % 3 && planes[k].present && planes[k].identity == (k >= 3 && no_residual));
      CHECK(planes[k].windowed == (p.upsampling_path && p.upsampler[k % 3] && !(k >= 3 && no_residual)));
      CHECK(planes[k].lines == (f.height + g.suby[k % 3] - 1) / g.suby[k % 3]);
    }
    check_launch(planes, 6, pl, stride, true);
  }
}

static void check_rowmaps()
{
  const int h11_21[2] = {1, 2}, v11_21[2] = {1, 1};
  const int h420[3] = {2, 1, 1}, v420[3] = {2, 1, 1}, h444[3] = {1, 1, 1}, v444[3] = {1, 1, 1};
  // the PGX loop of the reference's command line over a two-component frame with one subsampled component: the second pass finds
  // the unsubsampled component's cursor behind its last row -- zeros
  const mijpeg_info two = frame(50, 40, 2, h11_21, v11_21, false);
  std::vector<Call> pgx;
  for (int c = 0; c < 2; c++)
    for (int y = 0; y < 40; y += 8) pgx.push_back(Call{0, y, 49, y + 7, c, c, true, true, (uint32_t)y + 8});
  run_plain(two, pgx);
  CHECK(seen.zeros > 0 && seen.all_zero > 0 && seen.absent > 0);
  // 4:2:0: top-down stripes (the plain picture), then stripes out of order, an unaligned corner, one component, views without upsampling
  const mijpeg_info c420 = frame(70, 50, 3, h420, v420, true);
  std::vector<Call> mixed;
  for (int y = 0; y < 50; y += 8) mixed.push_back(Call{0, y, 69, std::min(y + 7, 49), 0, 2, true, true, 50});
  mixed.push_back(Call{0, 16, 69, 31, 0, 2, true, true, 50});
  mixed.push_back(Call{13, 5, 50, 22, 0, 2, true, true, 50});
  mixed.push_back(Call{34, 30, 44, 45, 1, 1, true, true, 50});
  mixed.push_back(Call{28, 35, 43, 42, 2, 2, false, false, 50});
  mixed.push_back(Call{0, 0, 69, 49, 0, 0, false, true, 16});
  run_plain(c420, mixed);
  // ... and a sequence whose first request is without the colour transformation: the views that follow are single planes
  std::vector<Call> noct = {Call{0, 8, 69, 23, 0, 2, true, false, 50}, Call{3, 9, 60, 40, 1, 1, false, false, 50}, Call{0, 0, 69, 49, 0, 2, true, false, 50}};
  run_plain(c420, noct);
  CHECK(seen.moved > 0 && seen.windowed > 0);
  // the same frame with its height in a DNL marker (one more MCU row in the store)
  mijpeg_info dnl = c420;
  dnl.dnl = 1;
  for (int c = 0; c < 3; c++) {
    dnl.rows[c] = c420.blocks_h[c];
    dnl.blocks_h[c] = c420.blocks_h[c] + c420.vsamp[c];
  }
  run_plain(dnl, mixed);
  // JPEG XT: a subsampled legacy image over an unsubsampled residual image and over a subsampled one, with and without residual
  const mijpeg_info r444 = frame(70, 50, 3, h444, v444, true);
  std::vector<Call> xt = {Call{0, 0, 69, 7, 0, 2, true, true, 50}, Call{0, 8, 69, 15, 0, 2, true, true, 50}, Call{13, 21, 50, 38, 0, 2, true, true, 50},
                          Call{0, 40, 69, 49, 0, 2, true, true, 50}};
  for (int no_residual = 0; no_residual < 2; no_residual++) {
    run_xt(c420, r444, no_residual != 0, xt);
    run_xt(c420, c420, no_residual != 0, xt);
    run_xt(r444, c420, no_residual != 0, xt);
  }
  CHECK(seen.identity > 0 && seen.requests > 40);
}

// ------------------------------------------------------------------------------------------------ the host copy
static void check_copy()
{
  const int w = 13, h = 7;
  const int rects[4][4] = {{0, 0, w - 1, h - 1}, {5, 3, w - 1, h - 1}, {w - 1, h - 1, w - 1, h - 1}, {2, 1, 6, 4}};
  for (int nc = 1; nc <= 4; nc++)
    for (int sb = 1; sb <= 2; sb++) {
      const int ones[4] = {1, 1, 1, 1};
      mijpeg_info g = frame(w, h, nc, ones, ones, false);
      g.sample_bytes = sb;
      const RequestImage im = request_image(g, 1);
      uint8_t *img = (uint8_t *)malloc(im.padded);
      for (size_t i = 0; i < im.padded; i++) img[i] = (uint8_t)(i * 37 + 11);
      const int bpps[3] = {sb, nc * sb, nc * sb + 3};
      for (int bpp : bpps)
        for (const int *r : rects)
          for (int plane = 0; plane < nc; plane++) {
            const int bpr = w * bpp + 5;
            // canvas pixel (0, 0) first; the last byte of the buffer is the last byte of the rectangle's last sample
            const size_t bytes = (size_t)r[3] * bpr + (size_t)r[2] * bpp + sb;
            uint8_t *got = (uint8_t *)malloc(bytes), *want = (uint8_t *)malloc(bytes);
            memset(got, 0xAA, bytes);
            memset(want, 0xAA, bytes);
            copy_plane_rect(img, im, plane, r[0], r[1], r[2], r[3], got, bpp, bpr);
            for (int y = r[1]; y <= r[3]; y++)
              for (int x = r[0]; x <= r[2]; x++)
                for (int b = 0; b < sb; b++) want[(size_t)y * bpr + (size_t)x * bpp + b] = img[(size_t)y * im.row + ((size_t)x * nc + plane) * sb + b];
            CHECK(memcmp(got, want, bytes) == 0);
            free(got);
            free(want);
          }
      free(img);
    }
  // the arguments of the device's copy of the same
  RequestImage im;
  im.nc = 3; im.sb = 2; im.row = 64; im.padded = 640;
  ScatterArgs a = scatter_args((const uint8_t *)&im, im, 2, 3, 9, 8, 1, 1);
  uint8_t bitmap[1];
  scatter_plane(a, 1, bitmap, 6, 77);
  CHECK(a.src == (const uint8_t *)&im && a.src_row == 64 && a.ncomp == 3 && a.sample_bytes == 2 && a.x0 == 2 && a.y0 == 3 && a.w == 8 && a.h == 6);
  CHECK(a.c0 == 1 && a.c1 == 1 && a.dst[1] == bitmap && a.bytes_per_pixel[1] == 6 && a.bytes_per_row[1] == 77 && !a.dst[0] && !a.dst[2] && !a.dst[3]);
}

// ------------------------------------------------------------------------------------------------ bands and slabs
static void check_bands()
{
  const size_t rows[] = {1, 7, 64, 4096, (size_t)1 << 20, (size_t)3 << 20, ((size_t)5 << 20) + 8};
  const long mibs[] = {-1, 0, 1, 4};
  int many_slabs = 0, many_bands = 0;
  for (int height = 1; height <= 200; height++)
    for (size_t row : rows)
      for (long mib : mibs) {
        const int bl = band_lines(mib, row, height), bands = band_count(height, bl);
        CHECK(bl >= 1 && (mib <= 0 ? bl == height : (bl >= 8 && bl % 8 == 0)));
        // the bands [b * bl, min(height, (b + 1) * bl)) tile [0, height): none is empty, the last one ends the frame
        CHECK(bands >= 1 && (int64_t)(bands - 1) * bl < height && (int64_t)bands * bl >= height);
        for (int y = 0; y < height; y++) CHECK(band_of(y, bl) >= 0 && band_of(y, bl) < bands && band_of(y, bl) * bl <= y && y < (band_of(y, bl) + 1) * bl);
        many_bands += bands > 1;
        const int tops[3] = {0, height / 3, height - 1};
        for (int min_y : tops) {
          const int ends[3] = {min_y, (min_y + height - 1) / 2, height - 1};
          for (int max_y : ends) {
            const int lines = max_y - min_y + 1, slabs = slab_count(lines, bl);
            CHECK(slabs >= 1 && slabs <= 4);
            many_slabs += slabs > 1;
            int at = min_y;
            for (int k = 0; k < slabs; k++) {
              int s0, s1;
              slab_bounds(min_y, lines, slabs, k, &s0, &s1);
              CHECK(s0 == at && s1 > s0 && band_of(s1 - 1, bl) < bands);
              at = s1;
              const int workers[3] = {2, 3, 16};
              for (int parts : workers) {
                int wat = s0;
                for (int i = 0; i < parts; i++) {
                  int y0, y1;
                  worker_lines(s0, s1, parts, i, &y0, &y1);
                  CHECK(y0 == wat && y1 >= y0);
                  wat = y1;
                }
                CHECK(wat == s1);
              }
            }
            CHECK(at == max_y + 1);
          }
        }
      }
  CHECK(many_slabs > 0 && many_bands > 0);
  CHECK(copy_parts(4u << 20, 1, 8) == 1 && copy_parts(1u << 20, 7, 8) == 1 && copy_parts(1u << 20, 8, 8) == 2 && copy_parts(1u << 20, 4000, 8) == 8);
  CHECK(copy_parts(1u << 20, 4000, 64) == 16 && copy_parts(100, 100, 8) == 0);
}

int main()
{
  check_extents();
  check_rowmaps();
  check_copy();
  check_bands();
  if (failures) {
    fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  printf("OK %d requests: %d rows of zeros, %d rows moved, %d planes not asked for, %d launches of zeros alone, %d identity planes\n", seen.requests,
         seen.zeros, seen.moved, seen.absent, seen.all_zero, seen.identity);
  return 0;
}
