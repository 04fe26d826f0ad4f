"""mijpeg_kernel_name and mijpeg_workspace_bytes against the recorded selection table (tests/golden/kernel_selection.json,
written by tests/golden/make_kernel_selection.py): the same case list, the same kernel and the same workspace need for every
case.  Host logic only: no device."""
import importlib.util
import json
import os

from conftest import GOLDEN_DIR

_spec = importlib.util.spec_from_file_location("make_kernel_selection", os.path.join(GOLDEN_DIR, "make_kernel_selection.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


def test_kernel_selection_matches_the_recorded_table():
    with open(os.path.join(GOLDEN_DIR, "kernel_selection.json")) as f:
        table = json.load(f)
    cases = gen.cases()
    assert len(cases) == table["cases"]
    assert gen.case_hash(cases) == table["case_sha256"], "the case list differs from the one the table was recorded for"
    got = gen.answers(cases)
    expected = gen.decode(table)
    diff = [(label, e, g) for (label, _), e, g in zip(cases, expected, got) if e != g]
    assert not diff, f"{len(diff)} of {len(cases)} cases differ, first ones (case, recorded, now): {diff[:5]}"
