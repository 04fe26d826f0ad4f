// prepare_batch_host_check.cpp -- the host half of the marker route (mijpeg_set_device_markers + mijpeg_prepare_batch_host, DESIGN
// 4.1d) over stream files, as a stand-alone program: meant to be built together with the library's host code under
// -fsanitize=address,undefined (tools/cxx/build_host_check.sh) and run once on a machine without a device.
//
//   prepare_batch_host_check a.jpg b.jpg ...
//
// Every stream alone and all of them as one batch, with the option on and off; for the calls that took the marker route the
// staged bytes must be the raw segment.  Prints the counts; exit code 0 when everything held.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/mijpeg.h"

static std::vector<uint8_t> read_file(const char *path)
{
  std::vector<uint8_t> out;
  FILE *f = fopen(path, "rb");
  if (!f) return out;
  uint8_t buf[65536];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), f)) > 0) out.insert(out.end(), buf, buf + got);
  fclose(f);
  return out;
}

// the raw segment of a stream whose last marker segment in front of the data is SOS: from behind the scan header to the end
static size_t ecs_offset(const std::vector<uint8_t> &s)
{
  size_t p = 2;
  while (p + 4 <= s.size() && s[p] == 0xff) {
    const size_t len = ((size_t)s[p + 2] << 8) | s[p + 3];
    const bool sos = s[p + 1] == 0xda;
    p += 2 + len;
    if (sos) return p;
  }
  return s.size();
}

int main(int argc, char **argv)
{
  if (argc < 2) {
    fprintf(stderr, "usage: %s stream.jpg ...\n", argv[0]);
    return 2;
  }
  std::vector<std::vector<uint8_t>> streams;
  for (int i = 1; i < argc; i++) {
    streams.push_back(read_file(argv[i]));
    if (streams.back().empty()) {
      fprintf(stderr, "%s: cannot read\n", argv[i]);
      return 2;
    }
  }
  mijpeg_decoder *d = nullptr;
  if (mijpeg_create(&d, -1) != MIJPEG_OK) return 2;
  int bad = 0;
  for (int on = 1; on >= 0; on--) {
    if (mijpeg_set_device_markers(d, on) != MIJPEG_OK) bad++;
    // one by one, then all together
    for (size_t first = 0; first <= streams.size(); first++) {
      std::vector<const uint8_t *> ptr;
      std::vector<size_t> size;
      for (size_t i = first < streams.size() ? first : 0; i < (first < streams.size() ? first + 1 : streams.size()); i++) {
        ptr.push_back(streams[i].data());
        size.push_back(streams[i].size());
      }
      const int rc = mijpeg_prepare_batch_host(d, ptr.data(), size.data(), (int)ptr.size());
      for (size_t k = 0; k < ptr.size(); k++) {
        size_t bytes = 0;
        const uint8_t *staged = mijpeg_device_markers_staging(d, (int)k, &bytes);
        if (!staged) continue; // (the call took the ordinary route)
        const std::vector<uint8_t> &s = streams[first < streams.size() ? first : k];
        const size_t at = ecs_offset(s);
        if (rc != MIJPEG_OK || !on || bytes != s.size() - at || memcmp(staged, s.data() + at, bytes)) {
          fprintf(stderr, "stream %zu: the staged bytes are not its raw segment\n", first < streams.size() ? first : k);
          bad++;
        }
      }
    }
  }
  int64_t searched = 0, declined = 0;
  mijpeg_device_markers_stats(d, &searched, &declined);
  printf("%zu streams: %lld images searched, %lld declined, %d mismatches\n", streams.size(), (long long)searched, (long long)declined, bad);
  mijpeg_destroy(d);
  return bad ? 1 : 0;
}
