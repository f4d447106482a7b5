"""Which kernel variants an MH / HMC handle takes, against the record of the commit before the rule moved into
csrc/mm_path.h: tests/golden/kernel_paths.json, written by tools/record_kernel_paths.py on a checkout of that commit (its hash
is in the file).  Per case -- the shapes listed in the tool's docstring, f32 and f64, MH and HMC -- the library must give
the same default variant (HMC), the same status of set_kernel_variant(v) for every v from -1 to 9 on a fresh handle, and
(HMC) the same value from mmcmc_hmc_kernel_variant after each successful set.  The rule itself is walked exhaustively on the
host in tests/test_path_rule.py."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_kernel_paths as R  # noqa: E402


def _golden():
    with open(R.GOLDEN) as f:
        return json.load(f)


def test_record_covers_every_case_and_names_its_commit():
    doc = _golden()
    assert len(doc["commit"]) == 40 and int(doc["commit"], 16) >= 0
    assert doc["variants"] == R.VARIANTS == list(range(-1, 10))
    assert set(doc["cases"]) == {R.case_id(c) for c in R.CASES} and len(R.CASES) == 54
    for name, rec in doc["cases"].items():
        assert set(rec["status"]) == {str(v) for v in R.VARIANTS}, name
        assert (rec["default"] is None) == name.startswith("mh-"), name
        if rec["default"] is not None:  # the default is a variant the handle accepts, and reports as itself
            assert rec["status"][str(rec["default"])] == 0 and rec["reported"][str(rec["default"])] == rec["default"], name


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_handles_take_the_recorded_variants(case):
    want = _golden()["cases"][R.case_id(case)]
    got = R.observe(case)
    print(R.case_id(case), got)
    assert got["default"] == want["default"]
    assert got["status"] == want["status"]
    assert got["reported"] == want["reported"]
