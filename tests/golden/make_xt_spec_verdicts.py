#!/usr/bin/env python3
"""Writes tests/golden/xt_spec_verdicts.json: what the library answers to golden JPEG XT files whose merging specification has
value bytes changed (tests/xt_spec_cases.py has the recipe and what a row holds).  The answers are THIS build's: the file is a
record of one commit's behaviour, for the commits that move the code behind it (HostDecoder::finish_xt) to be compared with.  Run
by hand against a build of the commit to record, with the commit's hash:
    python tests/golden/make_xt_spec_verdicts.py <commit>"""
import collections
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import xt_spec_cases as X  # noqa: E402


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    rows = collections.OrderedDict()
    for name, alpha, data in X.all_cases():
        rows.setdefault(name, []).append(X.record(data, alpha))
    with open(os.path.join(HERE, "xt_spec_verdicts.json"), "w") as f:
        json.dump({"recorded_from": sys.argv[1], "rows": rows}, f, separators=(",", ":"))
        f.write("\n")
    spec = [tuple(r[1:3]) for n in X.SPEC_FILES for r in rows[n]]
    outcomes = collections.Counter(spec)
    print(len(spec), "cases,", len(outcomes), "distinct outcomes,", sum(1 for r in spec if r[0] == 0), "decode, the most frequent outcome covers",
          outcomes.most_common(1)[0][1], "-- and", sum(len(rows[n]) for n in X.ALPHA_FILES), "alpha cases")


if __name__ == "__main__":
    main()
