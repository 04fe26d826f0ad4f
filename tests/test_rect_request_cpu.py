"""The device-free half of the rectangle service (libjpeg_amd/csrc/rect_request.hpp) under the sanitizers, without a device."""
from test_ragged_twin_cpu import _run_under_sanitizers


def test_rect_request_tables_under_sanitizers(tmp_path):
    """tests/cxx/rect_request_tables.cpp, a program of its own around rect_request.hpp and request_model.hpp: the writable extents
    against the brute-force rule of BitmapCtrl::ExtractBitmap; row maps and filter windows of real request sequences (plain frames,
    views without upsampling, the two images of a JPEG XT frame) in heap buffers of exactly their size; the strided host copy into
    destinations that end with the rectangle; bands, slabs and the workers' lines of the cached frame's download -- under
    AddressSanitizer and UBSan."""
    _run_under_sanitizers(tmp_path, "rect_request_tables")
