"""The NUTS host twin against its own recorded bytes (tests/golden/nuts_twin_pins.json, taken from the commit the file names by
tools/experiments/nuts_twin_record.py): the control rules of a transition -- leaf, push, sibling merge, dual averaging, the
step-size search -- are written for the fixed-D path, the pair walk and the run-time-dimension path (the scalar ones once, in
mm_nuts.h), and a change to any of them must not move a sample, a position, an adaptation record or a leapfrog count by a bit.

Every case is one call of O.engine_host_nuts_run on 4-6 chains and at most 12 + 12 transitions, replayed for each of its
`runs` = (mode, pair walk): modes 0, 1, 2 (fixed D) with and without eh_nuts_set_pairs and 4, 5, 6 (generic) at D = 2 .. 5,
generic alone at D = 9 and 17, mode 3 (the grouped twin) at D = 16; run() and run_progress(), n_discard = 0 and > 0,
max_depth 1, 2 and 10; starts far out on RosenbrockND and on a tight Gaussian (the search halves), on a wide one (it doubles),
and starts that are not real (a NaN or infinite coordinate, a density that overflows: the `k > 0` and unchanged-step exits).
Starts and matrices are stored once and named by the cases that share them.  Small outputs are stored whole (the hexadecimal string of their bytes), so a
mismatch names the first chain and row; larger ones as sha256."""
import hashlib
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sample", "pos", "adapt", "nlf")

with open(os.path.join(ROOT, "tests", "golden", "nuts_twin_pins.json")) as _f:
    PINS = json.load(_f)
GROUPS = sorted({c["name"].split("_m")[0] for c in PINS["cases"]})


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _replay(O, case, mode, pairs):
    E = O.engine_host_lib()
    init = np.array(PINS["starts"][case["init"]], dtype=np.uint64).view(np.float64).reshape(-1, case["dim"])
    mat = None if case["matrix"] is None else np.array(PINS["matrices"][case["matrix"]], dtype=np.float64).reshape(case["dim"], case["dim"])
    E.eh_nuts_set_pairs(pairs)
    try:
        return O.engine_host_nuts_run(mode, getattr(O, case["kind"]), case["dim"], case["params"], init, 0.8, case["n_collect"],
                                      case["n_discard"], seed=case["seed"], progress=case["progress"], max_depth=case["max_depth"],
                                      matrix=mat, n_threads=1)
    finally:
        E.eh_nuts_set_pairs(0)


def _check(what, got, want):
    b = _bits(got)
    if isinstance(want, dict):
        assert list(b.shape) == want["shape"], what
        assert hashlib.sha256(b.tobytes()).hexdigest() == want["sha256"], what
        return
    w = np.frombuffer(bytes.fromhex(want), dtype=b.dtype).reshape(b.shape)
    if not np.array_equal(b, w):
        at = np.argwhere(b != w)[0].tolist()  # sample: (chain, row, coordinate); pos, adapt: (chain, field); nlf: (chain,)
        pytest.fail(f"{what}: first difference at {at}: {int(b[tuple(at)]):#x} recorded {int(w[tuple(at)]):#x}")


def test_pins_cover_what_they_claim():
    """the file's own shape: the commit it was taken from, every mode, both walks, the sizes"""
    assert len(PINS["parent_commit"]) >= 7
    runs = {(m, p) for c in PINS["cases"] for m, p in c["runs"]}
    assert {(m, 0) for m in range(7)} <= runs and {(m, 1) for m in (0, 1, 2)} <= runs
    for c in PINS["cases"]:
        assert 4 <= len(PINS["starts"][c["init"]]) // c["dim"] <= 6 and c["n_collect"] <= 12 and c["n_discard"] <= 12, c["name"]
    gen_dims = {c["dim"] for c in PINS["cases"] for m, _ in c["runs"] if m >= 4}
    assert {2, 3, 4, 5, 9, 17} <= gen_dims
    assert {c["max_depth"] for c in PINS["cases"]} >= {1, 2, 10}
    assert any(not c["progress"] and c["n_discard"] == 0 for c in PINS["cases"]) and any(c["progress"] for c in PINS["cases"])


@pytest.mark.parametrize("group", GROUPS)
def test_host_twin_equals_its_recorded_bytes(O, group):
    for case in PINS["cases"]:
        if case["name"].split("_m")[0] != group:
            continue
        for mode, pairs in case["runs"]:
            res = _replay(O, case, mode, pairs)
            for name, a in zip(NAMES, res):
                _check((case["name"], "mode", mode, "pairs", pairs, name), a, case[name])
