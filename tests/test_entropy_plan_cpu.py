"""The device-free half of the on-device entropy decoders (libjpeg_amd/csrc/entropy_plan.hpp), without a device: what
device_entropy_multiscan and device_walk_images plan and stage before anything is enqueued -- the level schedule of a file's
scans, their table and stream slots, the lanes and workgroups of every launch, where the upload is cut, the walk's subsequences,
group lists and rounds, the refusals of both -- on hand-made scan lists and image lists."""
import os
import subprocess

from conftest import ROOT
from test_ragged_twin_cpu import _run_under_sanitizers


def test_entropy_plan_under_sanitizers(tmp_path):
    """tests/cxx/entropy_plan.cpp, a program of its own around entropy_plan.hpp: plans compared with values written out from the
    rules, the staging of both paths read back field by field from heap buffers of exactly the plans' sizes, under AddressSanitizer
    and UBSan.  Linked with the library's plain-C++ units (the Makefile's list): HuffTable::build is host_decoder.cpp's, which
    needs the others."""
    csrc = os.path.join(ROOT, "libjpeg_amd", "csrc")
    host_srcs = subprocess.run(["make", "-s", "-C", csrc, "print-host-srcs"], check=True, capture_output=True, text=True).stdout.split()
    assert "host_decoder.cpp" in host_srcs
    _run_under_sanitizers(tmp_path, "entropy_plan", *host_srcs)
