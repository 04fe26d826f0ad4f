// tsan_host.cpp -- the multi-threaded host decoder under ThreadSanitizer ("race detection").
//   tools/tsan_host.sh builds it with the library's plain-C++ units (the Makefile's print-host-srcs) under -fsanitize=thread and
//   runs it on streams that take every parallel path
// What runs concurrently in the product and therefore here: the restart-interval-parallel decode and the speculative
// (self-synchronising) decode of scans without restart markers on the library's worker pool (HostDecoder::decode with
// 8 threads), several decoder objects decoding different streams at the same time from different caller threads (the pool is
// shared process-wide), and damaged streams taking the sequential walk while other objects are in the parallel path.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <thread>
#include <vector>

#include "../libjpeg_amd/csrc/host_decoder.hpp"

static std::vector<uint8_t> slurp(const char *fn)
{
  std::ifstream f(fn, std::ios::binary);
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), {});
}

int main(int argc, char **argv)
{
  std::vector<std::vector<uint8_t>> files;
  for (int a = 1; a < argc; a++) files.push_back(slurp(argv[a]));
  if (files.empty()) return 2;
  long decoded = 0, rejected = 0, mismatched = 0;
  // 1. one object at a time, 8 pool threads, against the single-threaded decode of the same stream
  for (const auto &d : files) {
    mij::HostDecoder a, b;
    if (a.parse(d.data(), d.size(), false) || b.parse(d.data(), d.size(), false)) { rejected++; continue; }
    std::vector<int16_t> ca((size_t)a.info.coef_count + 64), cb((size_t)b.info.coef_count + 64);
    const int ra = a.decode(ca.data(), 8, nullptr), rb = b.decode(cb.data(), 1, nullptr);
    if (ra != rb || (!ra && memcmp(ca.data(), cb.data(), (size_t)a.info.coef_count * 2))) mismatched++;
    (ra ? rejected : decoded)++;
  }
  // 2. four caller threads, each with its own objects, all sharing the pool; every third stream is damaged
  std::vector<std::thread> ts;
  std::vector<long> ok(4, 0);
  for (int t = 0; t < 4; t++)
    ts.emplace_back([&, t] {
      for (size_t i = (size_t)t; i < files.size() * 3; i += 4) {
        std::vector<uint8_t> d = files[i % files.size()];
        if (i % 3 == 2 && d.size() > 600) { d[d.size() / 2] ^= 0x5a; d[d.size() / 2 + 1] = 0xff; d[d.size() / 2 + 2] = 0xd3; }
        mij::HostDecoder h;
        if (h.parse(d.data(), d.size(), false)) continue;
        std::vector<int16_t> c((size_t)h.info.coef_count + 64);
        if (!h.decode(c.data(), 4, nullptr)) ok[(size_t)t]++;
      }
    });
  for (auto &t : ts) t.join();
  // 3. JPEG XT frames with hidden residual bits at 24 threads: the refinement chains on bit masks, the planes updated by the
  // window's spare threads, and the rows of the residual planes handed out while the decode goes on (what the C-ABI layer
  // uploads early): every row once, in order, and FINAL when it is handed out -- the callback copies it right then, from
  // another thread than those still writing the rest (a row that was not final is a data race here, and a mismatch below)
  long early_rows = 0, early_bad = 0;
  for (const auto &d : files) {
    mij::HostDecoder a;
    if (a.parse(d.data(), d.size(), false) || !a.residual() || !a.xt.residual_wide) continue;
    std::vector<int16_t> ca((size_t)a.info.coef_count + 64);
    const mijpeg_info &r = a.xt.residual;
    std::vector<std::vector<int16_t>> snap((size_t)r.components);
    std::vector<int> next((size_t)r.components, 0);
    a.set_residual_rows_callback([&](int c, int y0, int y1) {
      const size_t row = (size_t)r.blocks_w[c] * 64 * 2;
      if (y0 != next[(size_t)c] || y1 <= y0 || y1 > r.blocks_h[c]) early_bad++;
      next[(size_t)c] = y1;
      const int16_t *src = ca.data() + (size_t)r.coef_offset[c] + row * (size_t)y0;
      snap[(size_t)c].insert(snap[(size_t)c].end(), src, src + row * (size_t)(y1 - y0));
      early_rows += y1 - y0;
    });
    if (a.decode(ca.data(), 24, nullptr)) continue;
    a.set_residual_rows_callback(nullptr);
    for (int c = 0; c < r.components; c++) {
      if (a.residual_rows_reported(c) != next[(size_t)c]) early_bad++;
      if (memcmp(snap[(size_t)c].data(), ca.data() + (size_t)r.coef_offset[c], snap[(size_t)c].size() * 2)) early_bad++;
    }
  }
  printf("single: decoded %ld rejected %ld mismatched %ld; concurrent: %ld %ld %ld %ld decoded; residual rows handed out early %ld, wrong %ld\n", decoded, rejected,
         mismatched, ok[0], ok[1], ok[2], ok[3], early_rows, early_bad);
  return mismatched || early_bad ? 1 : 0;
}
