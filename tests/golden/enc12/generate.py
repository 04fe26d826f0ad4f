#!/usr/bin/env python3
"""Regenerate tests/golden/enc12/: streams the reference encoder writes for 12-bit pictures (16-bit PNMs with maxval 4095 of
tests/enc12_util.py's seeded pictures and checkerboards): plain SOF1 / P = 12 streams, one interleaved scan.  They pin the 12-bit
forward colour transformation, the downsampling and the quantiser tables of `-q n` at 12 bits, which the oracle's oj_forward (8-bit
only) does not.  manifest.json: size, layout, content, seed and switches of every case.

Run in the build container (needs oracle/_ref/jpeg):   python tests/golden/enc12/generate.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import enc12_util as U  # noqa: E402
from oracle import oracle as O  # noqa: E402


def main():
    O.build(ref=False)
    if not O.have_reference():
        sys.exit("oracle/_ref/jpeg is missing: run `make -C oracle ref` first")
    manifest = {}
    for key, (w, h, layout, content, seed, q, extra) in U.CASES.items():
        args = U.case_args(key)
        rc, data, err = U.reference_encode12(U.case_image(key), args)
        assert rc == 0 and data, (key, rc, err)
        with open(os.path.join(U.GOLDEN_DIR, key + ".jpg"), "wb") as f:
            f.write(data)
        manifest[key] = {"width": w, "height": h, "layout": layout, "content": content, "seed": seed, "quality": q, "switches": args,
                         "bytes": len(data)}
    with open(os.path.join(U.GOLDEN_DIR, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(manifest)} cases -> {U.GOLDEN_DIR}")


if __name__ == "__main__":
    main()
