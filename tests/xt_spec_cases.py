"""The recorded-verdict cases of the JPEG XT merging specification (tests/golden/xt_spec_verdicts.json): golden files whose SPEC
(or ASPC) box has value bytes of its sub-boxes changed -- bytes that pass the walk's form check, so every case reaches
HostDecoder::finish_xt -- and what a host-only decoder object answers to each.  tests/golden/make_xt_spec_verdicts.py records the
answers of one build, tests/test_xt_spec_cpu.py compares another build's with them."""
import ctypes as C
import os
import random
import zlib

from libjpeg_amd import api

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SPEC_FILES = ["refspec_70x40_gray", "xt_lossless/rgb8_ro", "xt_general/enc_residual8", "xt_lonly/ghdr_R1_seq", "refc_83x47_420", "xt_33x17_422",
              "xt_int8/enc_422_coarse", "xt_general/a_l_curve_inside_spec", "xt_general/a_q_is_tone_box", "xt_general/a_l_gamma_curve",
              "xt_lossless/rgb8_ro_noct", "xt_lonly/hdr_R1_420"]
ALPHA_FILES = ["xt_alpha/a8", "xt_alpha/a16_residual"]
CASES_PER_FILE = 100
DCT_VALUES = [0x00, 0x20, 0x30, 0x31, 0x01, 0x10]


def golden(name):
    with open(os.path.join(GOLDEN_DIR, name + ".jpg"), "rb") as f:
        return f.read()


def sub_boxes(data, box_type):
    """[(type, offset of the payload in the file, its length)] of the sub-boxes with a payload in the file's one box of this type
    (one APP11 segment in front of the first scan: marker, length, "JP", En(2), Z(4), LBox(4), TBox(4), payload)"""
    found, i = [], 2
    while i + 4 <= len(data) and data[i] == 0xFF and data[i + 1] != 0xDA:
        ln = (data[i + 2] << 8) | data[i + 3]
        if data[i + 1] == 0xEB and data[i + 4:i + 6] == b"JP" and data[i + 16:i + 20] == box_type:
            found.append(i)
        i += 2 + ln
    assert len(found) == 1, (box_type, found)
    at = found[0] + 20
    end = found[0] + 12 + int.from_bytes(data[found[0] + 12:found[0] + 16], "big")
    assert end <= found[0] + 2 + ((data[found[0] + 2] << 8) | data[found[0] + 3])  # (the whole box in this segment)
    out = []
    while at + 8 <= end:
        lbox = int.from_bytes(data[at:at + 4], "big")
        assert 8 <= lbox <= end - at
        if lbox > 8:
            out.append((bytes(data[at + 4:at + 8]), at + 8, lbox - 8))
        at += lbox
    return out


def mutate(b, box, rng):
    """one mutation of one sub-box, in place: value bytes only"""
    r = rng.randrange
    t, at, n = box
    if t in (b"LTRF", b"RTRF", b"CTRF"):
        b[at] = r(16) << 4
    elif t[1:] == b"PTS" and n >= 2:
        b[at], b[at + 1] = r(256), r(256)
    elif t == b"RSPC":
        b[at] = (r(6) << 4) | r(6)
    elif t == b"OCON":
        b[at] = (r(10) << 4) | r(16)
    elif t in (b"LDCT", b"RDCT"):
        b[at] = DCT_VALUES[r(len(DCT_VALUES))]
    elif t == b"AMUL" and n >= 8:
        b[at] = r(4) << 4
        for k in range(2, 8):
            b[at + k] = r(256)
    else:  # CURV, MTRX, TONE inside the box
        b[at + r(n)] = r(256)


def streams(name, alpha=False):
    """the CASES_PER_FILE mutated files of one golden: case k carries 1 + (k & 1) mutations"""
    data = golden(name)
    boxes = sub_boxes(data, b"ASPC" if alpha else b"SPEC")
    assert boxes, name
    rng = random.Random(zlib.crc32(name.encode()))
    for k in range(CASES_PER_FILE):
        b = bytearray(data)
        for _ in range(1 + (k & 1)):
            mutate(b, boxes[rng.randrange(len(boxes))], rng)
        yield bytes(b)


def _crc_ints(crc, array):
    return zlib.crc32(bytes(memoryview(array).cast("B")), crc)


def _picture_crc(d, info):
    """CRC-32 over what a successful read published: the info bytes, every scalar and matrix of the transformer's parameters, the L
    tables' entries and the Q / R2 tables that exist (whether each exists is part of it; where it lies is not)"""
    crc = zlib.crc32(bytes(info))
    if not info.xt:
        return crc
    xt = d.xt_params()
    for name, _ in api.MijpegXtParams._fields_:
        if name not in ("ltable", "qtable", "r2table"):
            v = getattr(xt, name)
            crc = zlib.crc32(bytes(v) if isinstance(v, (C.Array, C.Structure)) else int(v).to_bytes(4, "little", signed=True), crc)
    for c in range(3):
        crc = _crc_ints(crc, (C.c_int32 * xt.ltable_entries).from_buffer_copy(xt.ltable[c]))
    # (an R2 table has (out_max + 1) << 4 entries, include/mijpeg.h: the same as qtable_entries at sixteen bits of output only)
    for table, entries in ((xt.qtable, xt.qtable_entries), (xt.r2table, (xt.out_max + 1) << 4)):
        for c in range(3):
            crc = zlib.crc32(b"\1" if table[c] else b"\0", crc)
            if table[c]:
                crc = _crc_ints(crc, (C.c_int32 * entries).from_address(table[c]))
    return crc


def _code_of(call):
    try:
        return 0, b"", call()
    except api.MijpegError as e:
        return e.code, e.message.encode(), None


def record(data, alpha=False):
    """-> [code of read_header, code of read, CRC-32 of their messages, code of last_warning, CRC-32 of what a successful read
    published]; for an alpha file three more: code of alpha_info, CRC-32 of (mode, matte), CRC-32 of what the alpha channel's
    decoder published (0: there is none)"""
    d = api.Decoder(None)
    try:
        hcode, hmsg, _ = _code_of(lambda: d.read_header(data))
        rcode, rmsg, info = _code_of(lambda: d.read(data))
        row = [hcode, rcode, zlib.crc32(hmsg + b"\0" + rmsg), d.last_warning()[0], _picture_crc(d, info) if rcode == 0 else 0]
        if alpha:
            acode, _, answer = _code_of(d.alpha_info)
            child = d.alpha_channel() if rcode == 0 else None
            row += [acode, zlib.crc32(repr(answer).encode()), _picture_crc(child, child.info) if child is not None else 0]
        return row
    finally:
        d.close()


def all_cases():
    """(name, is an alpha file, stream) of every case, in the fixture's order"""
    for names, alpha in ((SPEC_FILES, False), (ALPHA_FILES, True)):
        for name in names:
            for data in streams(name, alpha):
                yield name, alpha, data
