"""Reference model of the device marker search (libjpeg_amd/csrc/markers.hpp) and helpers that craft segments for it.

The contract, stated once: a byte pair is only ever interpreted from its FF.  `term` is the first FF whose follower is none of
00, FF, D0..D7 (nothing at or behind it counts); without one term = size and NO_END.  In front of term FF 00 keeps the FF,
FF Dn is restart marker k (both bytes leave), FF FF sets FILL.  SEQUENCE: marker k is not D0 + (k & 7).  COUNT: markers + 1 !=
expect.  With flags == 0: kept bytes back to back, begin[0] = 0, begin[k + 1] = end[k] = kept bytes in front of marker k,
end[expect - 1] = total.
"""
import numpy as np

FILL, SEQUENCE, COUNT, NO_END = 1, 2, 4, 8


def search(seg: bytes, expect: int) -> dict:
    n, p, term, flags = len(seg), 0, len(seg), 0
    kept, cuts, codes = bytearray(), [], []
    while p < n:
        b = seg[p]
        if b != 0xFF or p + 1 >= n:  # (a lone FF as last byte ends nothing)
            kept.append(b)
            p += 1
        elif seg[p + 1] == 0x00:
            kept.append(0xFF)
            p += 2
        elif seg[p + 1] == 0xFF:
            flags |= FILL
            kept.append(0xFF)
            p += 1
        elif 0xD0 <= seg[p + 1] <= 0xD7:
            cuts.append(len(kept))
            codes.append(seg[p + 1])
            p += 2
        else:
            term = p
            break
    if term == n:
        flags |= NO_END
    if any(c != 0xD0 + (k & 7) for k, c in enumerate(codes)):
        flags |= SEQUENCE
    if len(codes) + 1 != expect:
        flags |= COUNT
    return dict(flags=flags, term=term, total=len(kept), kept=bytes(kept), markers=len(codes),
                begin=[0] + cuts, end=cuts + [len(kept)])


def ecs_offset(jpeg: bytes) -> int:
    """Offset of the first entropy coded byte of the first scan."""
    p = 2
    while True:
        assert jpeg[p] == 0xFF, "marker expected"
        m, ln = jpeg[p + 1], (jpeg[p + 2] << 8) | jpeg[p + 3]
        p += 2 + ln
        if m == 0xDA:
            return p


def wellformed(rng: np.random.Generator, size: int, markers: int, garbage: bytes = b"") -> bytes:
    """A segment of exactly `size` bytes (>= 2 + len(garbage)): entropy coded bytes with stuffed FF 00 pairs and `markers`
    restart markers in sequence, the terminator FF D9, then `garbage`."""
    body = size - 2 - len(garbage)
    assert body >= 2 * markers
    out, k = bytearray(), 0
    # where the markers go: spread over the body, two back to back when there is more than one
    slots = sorted(int(x) for x in rng.integers(0, max(1, body - 2 * markers + 1), markers))
    if markers > 1:
        slots[1] = slots[0]
    plain = body - 2 * markers  # bytes that are no marker
    at = 0
    while at < plain or k < markers:
        while k < markers and slots[k] <= at:
            out += bytes((0xFF, 0xD0 + (k & 7)))
            k += 1
        if at >= plain:
            continue
        if plain - at >= 2 and (k >= markers or slots[k] >= at + 2) and rng.random() < 0.08:
            out += b"\xff\x00"
            at += 2
        else:
            out.append(int(rng.integers(0, 255)))  # never FF
            at += 1
    out += b"\xff\xd9" + garbage
    assert len(out) == size, (len(out), size)
    return bytes(out)
