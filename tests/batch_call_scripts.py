"""Short scripted call sequences over the uniform batch calls of the C ABI (mijpeg_decode_batch_device, _submit_, _finish_,
_reconstruct_batch_device and its planar twin, the marker route option, a ragged call in between), and what each of them lets a
client observe: the return code of every call with its message, info.range_max / fast_arith / batch_frames, batch_speculation(),
device_markers_stats(), a SHA-256 of every output tensor.  tests/golden/make_batch_call_outcomes.py records the observations of one
commit's library; tests/test_batch_calls.py replays the scripts on the library under test and compares.

Tiny pictures: 72 x 48 4:2:0 with a restart interval of 2 MCUs (5 x 3 MCUs, the last column partial), 52 x 36 4:4:4 with 1 MCU
(7 x 5 MCUs, last column and row partial), at most 6 per list."""
import ctypes as C
import hashlib

import numpy as np

from libjpeg_amd import api, synth

W, H = 72, 48
W4, H4 = 52, 36


def s420(seed, quality=85, dri=2):
    return synth.synth_jpeg(W, H, seed, quality, "420", dri)


def s444(seed, quality=85, dri=1):
    return synth.synth_jpeg(W4, H4, seed, quality, "444", dri)


def noise420(seed):
    """Noise in every channel at the tables of s420(): the same shape and tables, a range check far beyond a calm picture's."""
    return synth.encode_jpeg(np.random.default_rng(seed).integers(0, 256, (H, W, 3)).astype(np.uint8), 85, "420", restart_mcus=2)


def damaged(stream):
    """Entropy coded data that cannot be decoded inside an interval (a run of one-bits: no Huffman code is all ones)."""
    bad = bytearray(stream)
    pos = bad.find(b"\xff\xda") + 60
    while any(x == 0xFF for x in bad[pos - 1:pos + 14]):
        pos += 1
    bad[pos:pos + 12] = b"\xff\x00" * 6
    return bytes(bad)


def without_a_marker(stream):
    """One restart marker gone: the host's search sees it at once, a search on the device reports it when the batch is awaited."""
    pos = stream.find(b"\xff\xd1", stream.find(b"\xff\xda"))
    assert pos > 0
    return stream[:pos] + stream[pos + 2:]


class Recorder:
    """One script's decoder objects and the list of what it observed: [label, value ...] rows, JSON as they are."""

    def __init__(self):
        import torch

        self.torch = torch
        self.rows = []
        self.decoders = []

    def decoder(self):
        self.decoders.append(api.Decoder(0))
        return self.decoders[-1]

    def close(self):
        for d in self.decoders:
            d.close()

    def call(self, label, fn, *args, **kw):
        """fn(*args, **kw) -> its result (None where it raised); the row is the call's code and message."""
        try:
            res = fn(*args, **kw)
            self.rows.append([label, 0, None])
            return res
        except api.MijpegError as e:
            self.rows.append([label, e.code, e.message])
            return None

    def info(self, d, label="info"):
        """mijpeg_get_info as the call it is (it awaits a submitted batch), then what it reports of the batch."""
        f = api.MijpegInfo()
        rc = api.lib().mijpeg_get_info(d._h, C.byref(f))
        msg = C.c_char_p()
        if rc:
            api.lib().mijpeg_last_error(d._h, C.byref(msg))
        self.rows.append([label, rc, (msg.value or b"").decode() if rc else None] +
                         ([] if rc else [list(f.range_max)[:f.components], int(f.fast_arith), int(getattr(d, "batch_frames", 0)), f.width, f.height]))
        return None if rc else f

    def state(self, d, label="state"):
        self.rows.append([label, list(d.batch_speculation()), list(d.device_markers_stats())])

    def pixels(self, d, n, w, h, label="pixels", planar=False, **kw):
        """The decoded batch into a zeroed (n, h, w, 3) tensor -- (n, 3, h, w) where planar -- and the tensor's SHA-256 whatever
        the call returned (pending work of a call without sync is waited for first)."""
        out = self.torch.zeros((n, 3, h, w) if planar else (n, h, w * 3), dtype=self.torch.uint8, device="cuda")
        if planar:
            self.call(label, d.reconstruct_batch_planar_device, out.data_ptr(), 3 * h * w, h * w, w, **kw)
        else:
            self.call(label, d.reconstruct_batch_device, out.data_ptr(), h * w * 3, w * 3, **kw)
        return out

    def sha(self, out, label="sha"):
        self.torch.cuda.synchronize()
        self.rows.append([label, hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()])


SCRIPTS = {}


def script(fn):
    SCRIPTS[fn.__name__] = fn
    return fn


def _S(n=5, first=1):
    return [s420(first + i) for i in range(n)]


def _T(n=4):
    return [s444(20 + i) for i in range(n)]


@script
def decode_420(r):
    d = r.decoder()
    r.call("decode", d.decode_batch_device, _S(), 1)
    r.info(d)
    r.sha(r.pixels(d, 5, W, H))
    r.state(d)


@script
def decode_444(r):
    d = r.decoder()
    r.call("decode", d.decode_batch_device, _T(), 1)
    r.info(d)
    r.sha(r.pixels(d, 4, W4, H4))


@script
def submit_finish(r):
    d = r.decoder()
    r.call("submit", d.submit_batch_device, _S(), 1)
    r.call("finish", d.finish_batch_device)
    r.info(d)
    r.sha(r.pixels(d, 5, W, H))


@script
def submit_reconstruct(r):
    d = r.decoder()
    r.call("submit", d.submit_batch_device, _T(), 1)
    r.sha(r.pixels(d, 4, W4, H4))
    r.info(d)
    r.call("finish", d.finish_batch_device)


@script
def submit_get_info(r):
    d = r.decoder()
    r.call("submit", d.submit_batch_device, _S(), 1)
    r.info(d)
    r.sha(r.pixels(d, 5, W, H))


@script
def submit_twice(r):
    d = r.decoder()
    s = _S(6)
    r.call("submit", d.submit_batch_device, s[:2], 1)
    r.call("submit again", d.submit_batch_device, s[2:], 1)
    r.call("finish", d.finish_batch_device)
    r.info(d)
    r.sha(r.pixels(d, 4, W, H))


@script
def finish_with_nothing_submitted(r):
    d = r.decoder()
    r.call("finish", d.finish_batch_device)
    r.info(d)
    r.sha(r.pixels(d, 1, W, H))


@script
def finish_twice(r):
    d = r.decoder()
    r.call("decode", d.decode_batch_device, _S(3), 1)
    r.call("finish", d.finish_batch_device)
    r.call("finish again", d.finish_batch_device)
    r.sha(r.pixels(d, 3, W, H))


@script
def shrinking_and_growing_lists(r):
    d = r.decoder()
    s = _S(5)
    for part in (s, s[3:], s):
        r.call("submit", d.submit_batch_device, part, 1)
        r.sha(r.pixels(d, len(part), W, H))
        r.info(d)


@script
def speculation_holds(r):
    d = r.decoder()
    r.call("hint", d.decode_batch_device, _S(4), 1)
    r.call("submit", d.submit_batch_device, _S(4, 5), 1)
    out = r.pixels(d, 4, W, H, flags=api.FLAG_SPECULATIVE, sync=False)
    r.state(d, "launched")
    r.call("finish", d.finish_batch_device)
    r.state(d)
    r.info(d)
    r.sha(out)


@script
def speculation_redone(r):
    d = r.decoder()
    r.call("hint", d.decode_batch_device, _S(4), 1)
    r.call("submit", d.submit_batch_device, [noise420(i) for i in range(4)], 1)
    out = r.pixels(d, 4, W, H, flags=api.FLAG_SPECULATIVE, sync=False)
    r.call("finish", d.finish_batch_device)
    r.state(d)
    r.info(d)
    r.sha(out)


@script
def speculation_validated_by_synchronize(r):
    d = r.decoder()
    r.call("hint", d.decode_batch_device, _S(4), 1)
    r.call("submit", d.submit_batch_device, _S(4, 9), 1)
    out = r.pixels(d, 4, W, H, flags=api.FLAG_SPECULATIVE, sync=False)
    r.call("synchronize", d.synchronize)
    r.state(d)
    r.sha(out)
    r.call("finish", d.finish_batch_device)


@script
def no_flag_after_a_hint(r):
    d = r.decoder()
    r.call("hint", d.decode_batch_device, _S(4), 1)
    r.call("submit", d.submit_batch_device, _S(4, 5), 1)
    out = r.pixels(d, 4, W, H, sync=False)
    r.state(d)
    r.call("synchronize", d.synchronize)
    r.sha(out)


@script
def flag_with_sync_is_not_speculative(r):
    d = r.decoder()
    r.call("hint", d.decode_batch_device, _S(4), 1)
    r.call("submit", d.submit_batch_device, _S(4, 5), 1)
    r.sha(r.pixels(d, 4, W, H, flags=api.FLAG_SPECULATIVE, sync=True))
    r.state(d)


@script
def flag_without_a_hint_of_this_shape(r):
    d = r.decoder()
    r.call("hint of another shape", d.decode_batch_device, _T(), 1)
    r.call("submit", d.submit_batch_device, _S(3), 1)
    out = r.pixels(d, 3, W, H, flags=api.FLAG_SPECULATIVE, sync=False)
    r.state(d)
    r.call("synchronize", d.synchronize)
    r.sha(out)


@script
def submit_behind_an_unvalidated_speculation(r):
    d = r.decoder()
    r.call("hint", d.decode_batch_device, _S(4), 1)
    r.call("submit", d.submit_batch_device, [noise420(i) for i in range(4)], 1)
    out = r.pixels(d, 4, W, H, flags=api.FLAG_SPECULATIVE, sync=False)
    r.call("submit the next", d.submit_batch_device, _S(2), 1)
    r.state(d)
    r.sha(out)
    r.sha(r.pixels(d, 2, W, H), "sha of the next")


@script
def damaged_member_found_at_finish(r):
    d = r.decoder()
    s = _S(3)
    r.call("submit", d.submit_batch_device, [s[0], damaged(s[1]), s[2]], 1)
    r.call("finish", d.finish_batch_device)
    r.info(d)
    r.sha(r.pixels(d, 3, W, H))
    r.call("finish again", d.finish_batch_device)
    r.call("decode the good ones", d.decode_batch_device, [s[0], s[2]], 1)
    r.sha(r.pixels(d, 2, W, H))


@script
def damaged_member_found_at_reconstruct(r):
    d = r.decoder()
    s = _T(3)
    r.call("submit", d.submit_batch_device, [s[0], s[1], damaged(s[2])], 1)
    r.sha(r.pixels(d, 3, W4, H4))
    r.info(d)


@script
def damaged_member_under_speculation(r):
    d = r.decoder()
    s = _S(3)
    r.call("hint", d.decode_batch_device, s, 1)
    r.call("submit", d.submit_batch_device, [s[0], damaged(s[1]), s[2]], 1)
    r.pixels(d, 3, W, H, flags=api.FLAG_SPECULATIVE, sync=False)
    r.call("finish", d.finish_batch_device)
    r.state(d)
    r.info(d)


@script
def damaged_member_in_the_blocking_call(r):
    d = r.decoder()
    s = _S(2)
    r.call("decode", d.decode_batch_device, [s[0], damaged(s[1])], 1)
    r.info(d)


@script
def not_a_batch(r):
    d = r.decoder()
    r.call("two shapes", d.decode_batch_device, [s420(1), s444(20)], 1)
    sof = s420(2).find(b"\xff\xc0")
    arithmetic = s420(2)[:sof + 1] + b"\xc9" + s420(2)[sof + 2:]
    r.call("two bad streams", d.submit_batch_device, [s420(1), arithmetic, s420(3), b"\xff\xd8 not a jpeg at all"], 1)
    r.call("finish", d.finish_batch_device)


@script
def markers_qualifying(r):
    d = r.decoder()
    d.set_device_markers(1)
    r.call("decode", d.decode_batch_device, _S(), 1)
    r.state(d)
    r.info(d)
    r.sha(r.pixels(d, 5, W, H))


@script
def markers_qualifying_deferred(r):
    d = r.decoder()
    d.set_device_markers(1)
    r.call("submit", d.submit_batch_device, _T(), 1)
    r.state(d, "submitted")
    r.call("finish", d.finish_batch_device)
    r.state(d)
    r.sha(r.pixels(d, 4, W4, H4))


@script
def markers_declining(r):
    d = r.decoder()
    d.set_device_markers(1)
    s = _S(3)
    r.call("decode", d.decode_batch_device, [s[0], s[1] + b"\x00", s[2]], 1)  # (a byte behind EOI: not the plain case)
    r.state(d)
    r.info(d)
    r.sha(r.pixels(d, 3, W, H))


@script
def markers_without_restart_markers(r):
    d = r.decoder()
    d.set_device_markers(1)
    r.call("decode", d.decode_batch_device, [s420(30 + i, dri=0) for i in range(3)], 1)
    r.state(d)
    r.info(d)
    r.sha(r.pixels(d, 3, W, H))


@script
def markers_search_not_good_at_finish(r):
    d = r.decoder()
    d.set_device_markers(1)
    s = _S(3)
    r.call("submit", d.submit_batch_device, [s[0], without_a_marker(s[1]), s[2]], 1)
    r.state(d, "submitted")
    r.call("finish", d.finish_batch_device)
    r.state(d)
    r.info(d)
    r.call("the blocking call", d.decode_batch_device, [s[0], without_a_marker(s[1]), s[2]], 1)
    r.state(d, "blocking")


@script
def ragged_call_abandons_a_submitted_batch(r):
    d = r.decoder()
    r.call("submit", d.submit_batch_device, _S(3), 1)
    st = r.call("ragged", d.decode_ragged_device, [s444(20), s420(1)], 1)
    r.rows.append(["statuses", st])
    r.call("finish", d.finish_batch_device)
    r.sha(r.pixels(d, 3, W, H))
    outs = [r.torch.zeros((H4, W4 * 3), dtype=r.torch.uint8, device="cuda"), r.torch.zeros((H, W * 3), dtype=r.torch.uint8, device="cuda")]
    r.call("ragged pixels", d.reconstruct_ragged_device, [o.data_ptr() for o in outs], [W4 * 3, W * 3])
    for o in outs:
        r.sha(o)


@script
def ragged_call_abandons_a_speculation(r):
    d = r.decoder()
    r.call("hint", d.decode_batch_device, _S(3), 1)
    r.call("submit", d.submit_batch_device, [noise420(i) for i in range(3)], 1)
    r.pixels(d, 3, W, H, flags=api.FLAG_SPECULATIVE, sync=False)
    st = r.call("ragged", d.decode_ragged_device, [s420(1)], 1)
    r.rows.append(["statuses", st])
    r.state(d)
    r.call("finish", d.finish_batch_device)


@script
def single_image_abandons_a_submitted_batch(r):
    d = r.decoder()
    r.call("submit", d.submit_batch_device, _S(3), 1)
    r.call("read", d.read, s420(1))
    r.call("finish", d.finish_batch_device)
    r.sha(r.pixels(d, 3, W, H))


@script
def planar_output(r):
    d = r.decoder()
    r.call("decode", d.decode_batch_device, _S(4), 1)
    r.sha(r.pixels(d, 4, W, H, planar=True))
    r.call("submit", d.submit_batch_device, _T(3), 1)
    r.sha(r.pixels(d, 3, W4, H4, planar=True))
    r.info(d)


@script
def own_tables_then_shared(r):
    d = r.decoder()
    mixed = [s420(1 + i, q) for i, q in enumerate((50, 90, 90, 50))]
    r.call("decode", d.decode_batch_device, mixed, 1)
    f = r.info(d)
    r.rows.append(["quant", [list(f.quant[c]) for c in range(3)] if f else None])
    r.sha(r.pixels(d, 4, W, H))
    r.sha(r.pixels(d, 4, W, H, planar=True), "sha planar")
    r.call("submit shared", d.submit_batch_device, _S(3), 1)
    r.sha(r.pixels(d, 3, W, H))
    r.info(d)


def run(name):
    """-> the rows of script `name` on the library api.lib() loaded."""
    r = Recorder()
    try:
        SCRIPTS[name](r)
    finally:
        r.close()
    return r.rows


def inputs_digest():
    """SHA-256 over the streams the scripts are made of: a record made with another encoder build is no record of these inputs."""
    h = hashlib.sha256()
    for s in _S(6) + _S(4, 9) + _T() + [noise420(i) for i in range(4)] + [s420(30 + i, dri=0) for i in range(3)] + [s420(1, 50), s420(2, 90)]:
        h.update(s)
    return h.hexdigest()
