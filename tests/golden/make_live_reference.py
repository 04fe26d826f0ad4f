#!/usr/bin/env python3
"""Regenerate tests/golden/live_reference/: the cases tests/test_oracle.py compares against the live reference binary, stored for
the machines where it is not built -- each case's stream (`<key>.jpg`) and the sha256 of what the REAL reference decoder makes of
it (manifest.json), or for the encoder cases the stream the reference encoder wrote.

Run in the build container (needs oracle/_ref/jpeg):   python tests/golden/make_live_reference.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_oracle as T  # noqa: E402
from libjpeg_amd import synth  # noqa: E402
from oracle import oracle as O  # noqa: E402

OUT = T.LIVE_DIR


def main():
    O.build(ref=False)
    if not O.have_reference():
        sys.exit("oracle/_ref/jpeg is missing: run `make -C oracle ref` first")
    os.makedirs(OUT, exist_ok=True)
    manifest = {}

    def put(key, data, **ent):
        with open(os.path.join(OUT, key + ".jpg"), "wb") as f:
            f.write(data)
        manifest[key] = ent

    for w, h, q, sub, dri, seed in T._live_cases():
        data = synth.encode_jpeg(synth.synth_image(w, h, seed), q, sub, dri)
        put(f"decode_{seed}", data, pixels_sha256=T.sha256_of(O.reference_decode(data), np.uint8))
    for w, h, sub, dri, scale in T.LIVE_12BIT:
        data = synth.to_12bit(synth.synth_jpeg(w, h, 300 + w, 85, sub, dri), scale)
        rpx, rerr = O.reference_decode_status(data)
        assert rerr == 0
        put(f"decode12_{w}x{h}", data, pixels_sha256=T.sha256_of(np.asarray(rpx).reshape(h, w, 3), "<u2"))
    for w, h, extra in T.LIVE_XT:
        data = T.live_xt_stream(O, w, h, extra)
        put(f"xt_{w}x{h}", data, pixels_sha256=T.sha256_of(O.reference_decode_hdr(data), "<f4"))
    for w, h, args, seed in T.LIVE_FORWARD:
        put(f"forward_{seed}", O.reference_encode(T.live_forward_image(w, h, seed).squeeze(), args), args=args)
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(manifest)} cases -> {OUT}")


if __name__ == "__main__":
    main()
