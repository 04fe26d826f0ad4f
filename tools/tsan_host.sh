#!/bin/bash
# ThreadSanitizer run of the multi-threaded host decoder (no GPU needed).  Exit code != 0 on a data race or a mismatch.
set -e
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
# a private scratch directory: fixed names under /tmp collide with another user's run of this script
T="$(mktemp -d)"
trap 'rm -rf "$T"' EXIT
# the library's plain-C++ units: the Makefile's list (HOST_SRCS)
SRCS=()
for f in $(make -s -C "$ROOT/libjpeg_amd/csrc" print-host-srcs); do SRCS+=("$ROOT/libjpeg_amd/csrc/$f"); done
g++ -O1 -g -std=c++17 -pthread -fsanitize=thread -I"$ROOT/include" "$ROOT/tools/tsan_host.cpp" "${SRCS[@]}" -o $T/tsan_host
# big enough for the parallel paths: restart intervals, and a scan without restart markers for the speculative decoder
python3 - <<PY
import sys
sys.path.insert(0, "$ROOT")
from libjpeg_amd import synth
open("$T/tsan_dri.jpg", "wb").write(synth.synth_jpeg(1280, 720, 3, 85, "420", 4))
open("$T/tsan_nodri.jpg", "wb").write(synth.synth_jpeg(1280, 720, 4, 90, "420", 0))
open("$T/tsan_prog.jpg", "wb").write(synth.synth_jpeg(640, 480, 5, 85, "420", 8, progressive=True))
# no restart intervals: the scans of the frame run as a pipeline, a scan one MCU row behind the scan it refines
open("$T/tsan_prog_nodri.jpg", "wb").write(synth.synth_jpeg(640, 480, 6, 85, "420", 0, progressive=True))
# a tall JPEG XT frame with four hidden residual bits: rows of its residual planes are handed out a twelfth at a time
# (written by the reference encoder where it is built; tests/golden has small ones otherwise)
# beyond 2 MiB: the segment ends of a progressive file from one pass of the pool, the scans' marker searches side by side
open("$T/tsan_bigprog.jpg", "wb").write(synth.encode_jpeg(synth.synth_image(2048, 1400, 11), 96, "444", restart_mcus=8, progressive=True))
from oracle import oracle as O
if O.have_reference():
    # codestream boxes of more than a megabyte in 64 KiB segments: copied by the pool when the walk is through (materialize_boxes)
    open("$T/tsan_xt_big.jpg", "wb").write(O.reference_encode_hdr(synth.synth_hdr(1280, 960, 6), ["-r", "-q", "90", "-Q", "95", "-h", "-profile", "c", "-r12", "-s", "1x1,2x2,2x2", "-rR", "3", "-z", "4"]))
    open("$T/tsan_xt_rR4.jpg", "wb").write(O.reference_encode_hdr(synth.synth_hdr(192, 1536, 5), ["-r", "-q", "85", "-Q", "90", "-h", "-profile", "c", "-r12", "-s", "1x1,2x2,2x2", "-rR", "4"]))
else:
    import shutil
    shutil.copy("$ROOT/tests/golden/xt_200x120_420_rR4.jpg", "$T/tsan_xt_rR4.jpg")
PY
# ThreadSanitizer's runtime rejects address layouts drawn with more ASLR entropy than it knows ("unexpected memory mapping"):
# the binary runs without randomisation where the kernel allows a process to ask for that
NORAND=""
setarch "$(uname -m)" -R true 2>/dev/null && NORAND="setarch $(uname -m) -R"
TSAN_OPTIONS="halt_on_error=1 exitcode=66" $NORAND $T/tsan_host $T/tsan_dri.jpg $T/tsan_nodri.jpg $T/tsan_prog.jpg "$ROOT"/tests/golden/pil_200x120_420_dri8.jpg "$ROOT"/tests/golden/ref_75x45_420_dri2.jpg "$ROOT"/tests/golden/xt_129x71_420.jpg "$ROOT"/tests/golden/refprog_64x64_444_dri5.jpg $T/tsan_prog_nodri.jpg "$ROOT"/tests/golden/xt_200x120_420_rR4.jpg "$ROOT"/tests/golden/xt_129x71_420_R2_rR3_dri3.jpg $T/tsan_xt_rR4.jpg $T/tsan_bigprog.jpg $( [ -f $T/tsan_xt_big.jpg ] && echo $T/tsan_xt_big.jpg )
