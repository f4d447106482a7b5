"""Which kernel variants a NUTS handle takes, against the record of the commit before the rule moved into
csrc/mm_nuts_plan.h: tests/golden/nuts_kernel_paths.json, written by tools/record_kernel_paths.py --nuts on a checkout of
that commit (its hash is in the file).  Per case -- the shapes listed at NUTS_CASES in the tool, 64 chains each -- the library
must give the same default variant, the same status of set_kernel_variant(v) for every v from -1 to 9 on a fresh handle and the
same value from mmcmc_nuts_kernel_variant after each successful set.  The toggled cases walk one handle with a diagonal metric,
a dense metric or per-draw statistics switched on (each compiles one unit at run time; the record was taken where the run-time
compiler exists, and says whether the toggle took) and the variant it returns to.  The rule itself is walked exhaustively on
the host in tests/test_nuts_plan_host.py."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_kernel_paths as R  # noqa: E402


def _golden():
    with open(R.NUTS_GOLDEN) as f:
        return json.load(f)


def test_record_covers_every_case_and_names_its_commit():
    doc = _golden()
    assert len(doc["commit"]) == 40 and int(doc["commit"], 16) >= 0
    assert doc["variants"] == R.VARIANTS == list(range(-1, 10))
    assert set(doc["cases"]) == {R.nuts_case_id(c) for c in R.NUTS_CASES} and len(R.NUTS_CASES) == 15
    assert set(doc["toggled"]) == {R.nuts_case_id(c) for c in R.NUTS_TOGGLED} and len(R.NUTS_TOGGLED) == 3
    for name, rec in list(doc["cases"].items()) + list(doc["toggled"].items()):
        assert set(rec["status"]) == {str(v) for v in R.VARIANTS}, name
        # the default is a variant the handle accepts, and reports as itself
        assert rec["status"][str(rec["default"])] == 0 and rec["reported"][str(rec["default"])] == rec["default"], name
    # the shapes the cases were chosen for: pair kernels, lane groups in mode 2 only, a unit at dim 9, none above 32
    d = {k: v["default"] for k, v in doc["cases"].items()}
    assert d["standard_normal_2-0"] == d["rosenbrock_nd_3-1"] == d["rosenbrock_nd_10-2"] == 5
    assert d["gaussian_nd_16-2"] == d["gaussian_nd_32-2"] == 3 and d["gaussian_nd_32-0"] == 0
    assert d["rosenbrock_nd_9-0"] in (6, 7) and d["rosenbrock_nd_40-0"] == 6
    for name, rec in doc["toggled"].items():  # recorded with the run-time compiler present: every toggle took
        assert rec["toggle_status"] == 0 and rec["default"] == 7 and rec["after"] == rec["before"], name


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.NUTS_CASES + R.NUTS_TOGGLED, ids=R.nuts_case_id)
def test_nuts_handles_take_the_recorded_variants(case):
    want = _golden()["cases" if len(case) == 2 else "toggled"][R.nuts_case_id(case)]
    got = R.observe_nuts(case)
    print(R.nuts_case_id(case), got)
    assert got == want
