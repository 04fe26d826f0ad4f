"""The JPEG XT merging specification's module (libjpeg_amd/csrc/xt_spec.hpp, xt_finish.cpp), without a device: the pure
header as a program of its own under the sanitizers, and the recorded verdicts -- what the library answered, at the commit the
fixture names, to golden files whose SPEC / ASPC box has value bytes changed -- answered again row by row."""
import collections
import json
import os

import xt_spec_cases as X
from conftest import GOLDEN_DIR
from test_ragged_twin_cpu import _run_under_sanitizers


def test_xt_spec_under_sanitizers(tmp_path):
    """tests/cxx/xt_spec.cpp, a program of its own around xt_spec.hpp: the sub-box walk at its framing edges, the registry's
    acceptances, refusals and first-definition rule, scaled tables of curves and TONE tables, ieee_decode's infinities, under
    AddressSanitizer and UBSan."""
    _run_under_sanitizers(tmp_path, "xt_spec")


def test_recorded_verdicts():
    """tests/golden/xt_spec_verdicts.json (tests/golden/make_xt_spec_verdicts.py wrote it from the commit it names): codes, messages,
    warnings and published parameters of every case equal the record.  The record itself must not be hollow: many distinct
    outcomes, a fair share of files that decode, no outcome that dominates."""
    with open(os.path.join(GOLDEN_DIR, "xt_spec_verdicts.json")) as f:
        rows = json.load(f)["rows"]
    assert sorted(rows) == sorted(X.SPEC_FILES + X.ALPHA_FILES) and all(len(r) == X.CASES_PER_FILE for r in rows.values())
    spec = [(r[1], r[2]) for n in X.SPEC_FILES for r in rows[n]]  # (code of the read, CRC-32 of the messages)
    outcomes = collections.Counter(spec)
    assert len(outcomes) >= 20, len(outcomes)
    assert sum(1 for code, _ in spec if code == 0) * 20 >= len(spec)
    assert outcomes.most_common(1)[0][1] * 4 <= len(spec), outcomes.most_common(1)
    seen = collections.Counter()
    for name, alpha, data in X.all_cases():
        k = seen[name]
        seen[name] += 1
        assert X.record(data, alpha) == rows[name][k], (name, k)
