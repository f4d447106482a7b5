#!/usr/bin/env python3
"""Retake tests/golden/nuts_twin_pins.json: what the NUTS host twin (oracle/engine_host.cpp over mm_nuts.h and
mm_nuts_generic.h) of a given commit computes on a list of small cases, bit for bit.

    git worktree add /tmp/nuts_parent <commit>           # a scratch copy of the commit the record is taken from
    python3 tools/experiments/nuts_twin_record.py /tmp/nuts_parent <commit hash> [out.json]

Every case is one call of oracle.engine_host_nuts_run, written out in full, with the `runs` -- (mode, pair walk) -- that must
all give the recorded bytes: the fixed-D twin with and without eh_nuts_set_pairs and, at a dimension both have, the generic
twin.  The recorder asserts that they do on the commit it records.  Start positions (f64 bit patterns, so NaN and inf
travel) and matrices are stored once under `starts` / `matrices` and named by the cases that share them.  Outputs of at most
LIMIT bytes are kept whole, as the hexadecimal string of their bytes (a mismatch can name the chain and row), larger ones as
sha256.  tests/test_nuts_twin_pins.py replays the file."""
import hashlib
import json
import os
import sys

import numpy as np

LIMIT = 4096
NAMES = ("sample", "pos", "adapt", "nlf")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def replay(O, doc, case, mode, pairs):
    """the four outputs of one run of `case` of the record `doc`"""
    E = O.engine_host_lib()
    init = np.array(doc["starts"][case["init"]], dtype=np.uint64).view(np.float64).reshape(-1, case["dim"])
    mat = None if case["matrix"] is None else np.array(doc["matrices"][case["matrix"]], dtype=np.float64).reshape(case["dim"], case["dim"])
    E.eh_nuts_set_pairs(pairs)
    try:
        return O.engine_host_nuts_run(mode, getattr(O, case["kind"]), case["dim"], case["params"], init, 0.8, case["n_collect"],
                                      case["n_discard"], seed=case["seed"], progress=case["progress"], max_depth=case["max_depth"],
                                      matrix=mat, n_threads=1)
    finally:
        E.eh_nuts_set_pairs(0)


def packed(a):
    b = bits(a)
    if b.nbytes <= LIMIT:
        return b.tobytes().hex()
    return {"sha256": hashlib.sha256(b.tobytes()).hexdigest(), "shape": list(b.shape)}


def cases(O, N):
    out, starts, matrices = [], {}, {}

    def shared(table, word, values):
        """the name under which `values` is stored in `table` (stored once)"""
        for k, v in table.items():
            if v == values:
                return k
        table[f"{word}{len(table)}"] = values
        return f"{word}{len(table) - 1}"

    def add(name, runs, kind, dim, init, n_collect, n_discard, progress=False, max_depth=10, params=(), matrix=None, seed=5):
        out.append(dict(name=name, runs=[list(r) for r in runs], kind=kind, dim=dim, params=list(params),
                        matrix=None if matrix is None else shared(matrices, "matrix", np.asarray(matrix, dtype=np.float64).ravel().tolist()),
                        init=shared(starts, f"start_d{dim}_", np.ascontiguousarray(init, dtype=np.float64).view(np.uint64).ravel().tolist()),
                        n_collect=n_collect,
                        n_discard=n_discard, progress=progress, max_depth=max_depth, seed=seed))

    def both(tm):  # fixed-D twin without and with the pair walk, and the generic twin
        return [(tm, 0), (tm, 1), (tm + 4, 0)]

    # schedules: (n_collect, n_discard, progress, max_depth) -- the initial row and the N - 1 off-by-one with and without
    # progress, both arms of dual averaging, the cap at the first leaf, after one merge, never
    schedules = [(12, 0, False, 10), (12, 12, False, 10), (8, 4, True, 2), (6, 0, True, 1), (6, 5, False, 2), (6, 3, False, 1),
                 (7, 6, True, 10)]
    for tm in (0, 1, 2):
        for dim in (2, 3, 4):
            init = O.init_with_seed(4, dim, 17 + dim) * 0.8
            for nc, nd, pr, cap in schedules:
                add(f"rosenbrock{dim}_m{tm}_c{nc}_d{nd}_p{int(pr)}_cap{cap}", both(tm), "ROSENBROCK_ND", dim, init, nc, nd, pr, cap)
    # generic only: an odd f64 Box-Muller tail (5; it has a fixed instance too), no compiled instance (9, 17)
    for tm in (0, 1, 2):
        for dim in (5, 9, 17):
            init = O.init_with_seed(4, dim, 17 + dim) * 0.5
            runs = both(tm) if dim == 5 else [(tm + 4, 0)]
            add(f"rosenbrock{dim}_m{tm}_run", runs, "ROSENBROCK_ND", dim, init, 12, 0)
            add(f"rosenbrock{dim}_m{tm}_warm", runs, "ROSENBROCK_ND", dim, init, 10, 12, False, 10 if dim < 17 else 5)
    # the step-size search: halving from far out on Rosenbrock, halving on a tight Gaussian, doubling on a wide one; the
    # first of each pair makes no transition (run(1, 0)), so the adaptation record is the search's result alone
    far = np.array([[30.0, -30.0, 30.0], [-30.0, 30.0, -30.0], [6.0, 5.0, -4.0], [0.3, 0.2, 0.1]])
    gauss = O.init_with_seed(4, 3, 3)
    for tm in (0, 1, 2):
        add(f"far_m{tm}_search", both(tm), "ROSENBROCK_ND", 3, far, 1, 0)
        add(f"far_m{tm}", both(tm), "ROSENBROCK_ND", 3, far, 6, 4)
        for word, std in (("tight", 0.01), ("wide", 100.0)):
            add(f"{word}_m{tm}_search", both(tm), "ISOTROPIC_GAUSSIAN", 3, gauss * std, 1, 0, params=[std])
            add(f"{word}_m{tm}", both(tm), "ISOTROPIC_GAUSSIAN", 3, gauss * std, 6, 6, params=[std])
    # starts that are not real (the inputs of tests/nonfinite_common.py: a NaN, +inf and -inf coordinate, and radii past the
    # edge where the density overflows the tensor type): the `k > 0` and the unchanged-step exits of the search
    for tm in (0, 1, 2):
        dt = np.float32 if tm < 2 else np.float64
        rows, isbad = N.starts(O, dt, 3, n_good=3, bad_at=(1, 4, 5))
        assert isbad.sum() == 3 and np.isnan(rows).any()
        add(f"nonreal_m{tm}", both(tm), "STANDARD_NORMAL", 3, rows.astype(np.float64), 6, 4)
        add(f"nonreal_m{tm}_progress", both(tm), "STANDARD_NORMAL", 3, rows.astype(np.float64), 5, 0, True)
    # mode 3, the grouped twin of the lane-group kernels
    rng = np.random.default_rng(7)
    q, _ = np.linalg.qr(rng.standard_normal((16, 16)))
    A = (q * np.logspace(0.0, 2.0, 16)) @ q.T
    A = (A + A.T) / 2.0
    init = O.init_with_seed(4, 16, 42) * 0.1
    add("grouped16_run", [(3, 0), (3, 1)], "GAUSSIAN_ND", 16, init, 6, 0, matrix=A, seed=42)
    add("grouped16_warm", [(3, 0), (3, 1)], "GAUSSIAN_ND", 16, init, 6, 6, matrix=A, seed=42, max_depth=6)
    return dict(starts=starts, matrices=matrices, cases=out)


def main():
    tree, commit = os.path.abspath(sys.argv[1]), sys.argv[2]
    here = os.path.dirname(os.path.abspath(__file__))
    out_json = sys.argv[3] if len(sys.argv) > 3 else os.path.join(here, "..", "..", "tests", "golden", "nuts_twin_pins.json")
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tests"))
    import nonfinite_common as N
    import oracle as O

    assert os.path.dirname(os.path.abspath(O.__file__)) == os.path.join(tree, "oracle")
    O.lib()
    doc = cases(O, N)
    rec = doc["cases"]
    for case in rec:
        res = [replay(O, doc, case, m, p) for m, p in case["runs"]]
        for r, run in zip(res[1:], case["runs"][1:]):
            for a, b in zip(res[0], r):
                assert a.dtype == b.dtype and np.array_equal(bits(a), bits(b)), (case["name"], run)
        for name, a in zip(NAMES, res[0]):
            case[name] = packed(a)
    # the search cases do what their names say
    by = {c["name"]: c for c in rec}
    for tm in (0, 1, 2):
        eps = lambda n: np.frombuffer(bytes.fromhex(by[n]["adapt"]), dtype=np.float64).reshape(-1, 4)[:, 0]
        assert (eps(f"tight_m{tm}_search") < 1).all() and (eps(f"wide_m{tm}_search") > 1).all() and (eps(f"far_m{tm}_search")[:2] < 1).all()
        assert (np.frombuffer(bytes.fromhex(by[f"nonreal_m{tm}"]["nlf"]), dtype=np.uint64)[[1, 4, 5]] == 9).all()  # every tree stops at its first leaf
    with open(out_json, "w") as f:
        f.write('{"parent_commit": %s,\n"starts": %s,\n"matrices": %s,\n"cases": [\n'
                % (json.dumps(commit), json.dumps(doc["starts"], separators=(",", ":")), json.dumps(doc["matrices"], separators=(",", ":"))))
        f.write(",\n".join(json.dumps(c, separators=(",", ":")) for c in rec))
        f.write("\n]}\n")
    print(len(rec), "cases ->", out_json, os.path.getsize(out_json), "bytes")


if __name__ == "__main__":
    main()
