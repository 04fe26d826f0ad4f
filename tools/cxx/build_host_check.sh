#!/bin/bash
# Builds tools/cxx/prepare_batch_host_check.cpp together with the library's HOST code under AddressSanitizer and
# UndefinedBehaviorSanitizer into a directory of the caller's (default: a temporary one) -- nothing in the tree is touched.
# The kernel translation units (*.hip) keep the ordinary build's objects (libjpeg_amd/csrc/build/, built by `make`): only their
# launch stubs are host code, and the program never launches anything.  Host code alone is instrumented: -Xarch_host on the compile
# lines, -fno-gpu-sanitize on the link line -- no device code object of this build carries a sanitizer.  The program is a stand-alone executable linked with the
# sanitizers' runtimes; run it on a machine without a device, on stream files:
#
#   tools/cxx/build_host_check.sh /tmp/hostcheck && /tmp/hostcheck/prepare_batch_host_check a.jpg b.jpg ...
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/../.." && pwd)"
OUT="${1:-$(mktemp -d)}"
SRC="$ROOT/libjpeg_amd/csrc"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
CXX="${HOSTCXX:-/opt/rocm/lib/llvm/bin/clang++}" # (the compiler hipcc drives: one sanitizer runtime for all objects)
SAN="-fsanitize=address,undefined -fno-omit-frame-pointer -g"
mkdir -p "$OUT"
# The translation units are the Makefile's own lists (libjpeg_amd/csrc/Makefile: `make -s print-objs`, `make -s print-host-srcs`): an
# object with a .hip source is the ordinary build's, a unit of HOST_SRCS and class JPEG are plain C++, every other .cpp is compiled as HIP.
HOST_SRCS=" $(make -s -C "$SRC" print-host-srcs) "
LINK=("$OUT/check.o")
"$CXX" -O1 -std=c++17 -pthread $SAN -c "$ROOT/tools/cxx/prepare_batch_host_check.cpp" -o "$OUT/check.o" &
for obj in $(make -s -C "$SRC" print-objs); do
  f="$(basename "$obj" .o)"
  if [ -f "$SRC/$f.hip" ]; then
    make -s -C "$SRC" "$obj"
    LINK+=("$SRC/$obj")
    continue
  fi
  LINK+=("$OUT/$f.o")
  if [ "$f" = jpeg_class ]; then
    "$CXX" -O1 -std=c++17 -fPIC -pthread $SAN -c "$SRC/interface/jpeg.cpp" -o "$OUT/$f.o" &
  elif [[ "$HOST_SRCS" == *" $f.cpp "* ]]; then
    "$CXX" -O1 -std=c++17 -fPIC -pthread $SAN -c "$SRC/$f.cpp" -o "$OUT/$f.o" &
  else
    "$HIPCC" --offload-arch=gfx950 -O1 -std=c++17 -fPIC -w -Xarch_host "-fsanitize=address,undefined" -Xarch_host -fno-omit-frame-pointer -x hip -c "$SRC/$f.cpp" -o "$OUT/$f.o" &
  fi
done
wait
"$HIPCC" --offload-arch=gfx950 -fsanitize=address,undefined -fno-gpu-sanitize -o "$OUT/prepare_batch_host_check" "${LINK[@]}" -pthread
echo "$OUT/prepare_batch_host_check"
