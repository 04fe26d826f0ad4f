#!/bin/bash
# tools/ab/build_variant.sh NAME [compiler flags ...]: the working tree's kernels.hip compiled with the given flags (-D..., -mllvm ...),
# linked with the other objects of the current build -- the Makefile's own list -- into tools/ab/libmijpeg_NAME.so (git-ignored;
# travels to the GPU box).  MIJPEG_LIBRARY selects it at run time.
set -e
ROOT="$(cd "$(dirname "$0")/../.." && pwd)"
NAME="$1"; shift
cd "$ROOT/libjpeg_amd/csrc"
make -s
KOBJ="build/kernels_$NAME.o"
/opt/rocm/bin/hipcc $(make -s print-hipflags) "$@" -c kernels.hip -o "$KOBJ"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$ROOT/tools/ab/libmijpeg_$NAME.so" $(make -s print-objs KERNELS_OBJ="$KOBJ") -pthread
rm -f "$KOBJ".*
echo "built tools/ab/libmijpeg_$NAME.so"
