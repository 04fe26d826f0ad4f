"""mijpeg_reconstruct_ragged_device sends an image of a layout group into a fused list launch where its plan's kernel has a
ragged flavour (ragged_twin, kernels.hip) and asks nothing about the group: that rests on the planner (plan_reconstruct) naming a
kernel of the ragged families only for frames of that family's layout and precision.  Pinned here, without a device, over every
layout the planner tells apart, both precisions, the colour transformation on and off, both arithmetic flavours and every range
gate from both sides.  tests/cxx/fused_list_tables.cpp: the tables of those launches (fused_list.hpp) under the sanitizers;
tests/cxx/encode_list_tables.cpp: the other direction's device-free half, the passes of the ragged encode (encode_list.hpp);
tests/cxx/ragged_failures.cpp: which failing picture a list reconstruction call reports, and in which words (ragged_failures.hpp)."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

from conftest import ROOT
from libjpeg_amd import api
from test_ragged_batch import _flavour

RANGE_GATES = [1477, 2047, 7600, 8190, 16384, 45056, 49152, 65536]  # reconstruct.hpp
LAYOUTS = {"420": ((2, 1, 1), (2, 1, 1)), "422": ((2, 1, 1), (1, 1, 1)), "444": ((1, 1, 1), (1, 1, 1)), "grey": ((1,), (1,)),
           "440": ((1, 1, 1), (2, 1, 1)), "411": ((4, 1, 1), (1, 1, 1)), "grey2x1": ((2,), (1,))}
# the kernels with a ragged flavour (kernel name without its flavour suffix) -> the layout group they reconstruct
FAMILY = {"fused420p_kernel": "420", "fused420_kernel": "420", "fused422_kernel": "422", "fused444_kernel": "444", "fused1_kernel": "grey",
          "fused420_kernel<12>": "420_12", "fused422_12_kernel": "422_12", "fused444_12_kernel": "444_12", "fused1_kernel<12>": "grey_12"}


def test_a_ragged_kernel_is_named_for_its_layout_group_only():
    infos = []
    for (hs, vs), precision, ycbcr, fast in itertools.product(LAYOUTS.values(), (8, 12), (1, 0), (1, 0)):
        for r in [g - k for g in RANGE_GATES for k in (0, 1)]:
            f = api.frame_layout(200, 120, len(hs), hs, vs, [[16] * 64, [17] * 64], ycbcr=ycbcr, precision=precision)
            f.fast_arith = fast
            for c in range(len(hs)):
                f.range_max[c] = r
            infos.append(f)
    group = api.ragged_plan16(infos)[0]
    families, others = set(), set()
    for f, g in zip(infos, group):
        name = _flavour(f)[0]  # (mijpeg_kernel_name with per-frame tables: what the reconstruct call plans with)
        family = name.replace("<wide>", "").replace("/narrow", "")
        if g < 0:
            continue
        if family in FAMILY:
            assert api.RAGGED_GROUPS16[g] == FAMILY[family], (name, api.RAGGED_GROUPS16[g], f.precision, f.ycbcr, f.fast_arith, f.range_max[0])
            families.add(family)
        else:
            others.add(family)
    # the list is not beside the point: every family came up, and so did group members that no ragged kernel takes
    assert families == set(FAMILY) and others, (families, others)
    # 4:4:0, 4:1:1 and sampling factors on a single component have no group
    assert all(g < 0 for f, g in zip(infos, group) if (f.hsamp[0], f.vsamp[0]) in ((1, 2), (4, 1)) or (f.components == 1 and f.hsamp[0] == 2))


def _run_under_sanitizers(tmp_path, name, *more_sources):
    """tests/cxx/<name>.cpp (and library sources that need no device) as a program of its own under AddressSanitizer and UBSan."""
    cxx = "/opt/rocm/lib/llvm/bin/clang++"  # (ROCm's host clang++: a plain host compile, no device code)
    exe = str(tmp_path / name)
    csrc = os.path.join(ROOT, "libjpeg_amd", "csrc")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-isystem", "/opt/rocm/include", "-I", csrc,
                    os.path.join(ROOT, "tests", "cxx", name + ".cpp"), *[os.path.join(csrc, s) for s in more_sources], "-pthread", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK "), (r.stdout[-500:], r.stderr[-3000:])


def test_fused_list_tables_under_sanitizers(tmp_path):
    """tests/cxx/fused_list_tables.cpp, a program of its own around fused_list.hpp: grouping, layout and fill of the list launches'
    tables, every field read back from a heap buffer of exactly the layout's size, under AddressSanitizer and UBSan."""
    _run_under_sanitizers(tmp_path, "fused_list_tables")


def test_encode_list_tables_under_sanitizers(tmp_path):
    """tests/cxx/encode_list_tables.cpp, a program of its own around encode_list.hpp and encoder.cpp: the passes of the ragged
    encode from the real planner, layout and fill -- arenas of exactly their sizes, every pointer, prefix table and work list read
    back, the plain buffer and every picture's piece of a fake output arena -- under AddressSanitizer and UBSan."""
    _run_under_sanitizers(tmp_path, "encode_list_tables", "encoder.cpp")


def test_ragged_failures_under_sanitizers(tmp_path):
    """tests/cxx/ragged_failures.cpp, a program of its own around ragged_failures.hpp: no failure is MIJPEG_OK, the first noted of
    several failures gives code and message, and the message's two forms -- with a child object's text behind ": " (an empty text
    leaves the ": "), without any -- byte for byte, under AddressSanitizer and UBSan."""
    _run_under_sanitizers(tmp_path, "ragged_failures")
