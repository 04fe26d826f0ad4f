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
make -s -C "$SRC" build/kernels.o build/forward.o build/hencode.o build/huffman.o build/markers.o build/resample.o build/requant.o
for f in capi batch_decode rect_service reconstruct_device ragged_decode ragged_reconstruct entropy_device encode_device batch_pipeline; do
  "$HIPCC" --offload-arch=gfx950 -O1 -std=c++17 -fPIC -w -Xarch_host "-fsanitize=address,undefined" -Xarch_host -fno-omit-frame-pointer -x hip -c "$SRC/$f.cpp" -o "$OUT/$f.o" &
done
"$CXX" -O1 -std=c++17 -fPIC -pthread $SAN -c "$SRC/host_decoder.cpp" -o "$OUT/host_decoder.o" &
"$CXX" -O1 -std=c++17 -fPIC -pthread $SAN -c "$SRC/xt_finish.cpp" -o "$OUT/xt_finish.o" &
"$CXX" -O1 -std=c++17 -fPIC -pthread $SAN -c "$SRC/encoder.cpp" -o "$OUT/encoder.o" &
"$CXX" -O1 -std=c++17 -fPIC -pthread $SAN -c "$SRC/interface/jpeg.cpp" -o "$OUT/jpeg_class.o" &
"$CXX" -O1 -std=c++17 -pthread $SAN -c "$ROOT/tools/cxx/prepare_batch_host_check.cpp" -o "$OUT/check.o" &
wait
"$HIPCC" --offload-arch=gfx950 -fsanitize=address,undefined -fno-gpu-sanitize -o "$OUT/prepare_batch_host_check" "$OUT"/check.o "$OUT"/capi.o "$OUT"/batch_decode.o "$OUT"/rect_service.o "$OUT"/reconstruct_device.o \
  "$OUT"/ragged_decode.o "$OUT"/ragged_reconstruct.o "$OUT"/entropy_device.o "$OUT"/encode_device.o "$OUT"/batch_pipeline.o "$OUT"/host_decoder.o "$OUT"/xt_finish.o "$OUT"/encoder.o "$OUT"/jpeg_class.o \
  "$SRC"/build/kernels.o "$SRC"/build/forward.o "$SRC"/build/hencode.o "$SRC"/build/huffman.o "$SRC"/build/markers.o "$SRC"/build/resample.o "$SRC"/build/requant.o -pthread
echo "$OUT/prepare_batch_host_check"
