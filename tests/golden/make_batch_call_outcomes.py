#!/usr/bin/env python3
"""Writes tests/golden/batch_call_outcomes.json: what the scripted call sequences of tests/batch_call_scripts.py observe on the
uniform batch calls -- return codes, messages, range checks, speculation and marker route counters, hashes of the pixels.  The
answers are THIS build's: the file is a record of one commit's behaviour, for the commits that move the code behind the calls
(submit_batch, finish_batch) to be compared with.  Run by hand on a machine with the device against a build of the commit to record
(MIJPEG_LIBRARY selects that build's library), with the commit's hash:
    MIJPEG_LIBRARY=/path/to/libmijpeg.so python tests/golden/make_batch_call_outcomes.py <commit> [output file]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import batch_call_scripts as B  # noqa: E402


def main():
    if len(sys.argv) not in (2, 3):
        raise SystemExit(__doc__)
    out = sys.argv[2] if len(sys.argv) == 3 else os.path.join(HERE, "batch_call_outcomes.json")
    rows = {name: B.run(name) for name in B.SCRIPTS}
    with open(out, "w") as f:
        json.dump({"recorded_from": sys.argv[1], "inputs": B.inputs_digest(), "rows": rows}, f, indent=0)
        f.write("\n")
    print(len(rows), "scripts,", sum(len(r) for r in rows.values()), "observations,", sum(1 for r in rows.values() for o in r if len(o) > 2 and isinstance(o[1], int) and o[1] < 0),
          "of them calls that failed")


if __name__ == "__main__":
    main()
