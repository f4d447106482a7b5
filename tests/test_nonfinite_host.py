"""NUTS from starts whose log-density is not real: the step-size search ends, the chain stays put, its neighbours do not notice.

mm_find_reasonable_epsilon (mm_nuts.h, and its run-time-dimension copy in mm_nuts_generic.h) halves a factor k while the
first leapfrog's log-density and gradient are not real.  The reference's loop (nuts.rs:717) has no other exit, so a start
whose own log-density is not real never leaves it; the engine bounds it by `k > 0`.  Everything here runs the host build of
those headers (oracle/engine_host.cpp) in a CHILD process under a time limit: with the bound taken out, these tests fail by
that limit instead of hanging the test run.  oracle/nuts.c restates the reference, keeps its loop, and is not called here.

Run as a program (`python test_nonfinite_host.py spec.json out.npz`) this file is that child.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "nuts_far_starts.json")
CHILD_TIMEOUT = 30  # seconds per child; a child takes about a second (the interpreter's start included)

N_COLLECT, N_DISCARD = 6, 4
F32_MODES = (0, 1, 4, 5)  # tensor type f32: type modes 0 and 1, and the same through mm_nuts_generic.h (4, 5)
NAMES = ("sample", "pos", "adapt", "nlf")


def _child_main(spec_path, out_path):
    sys.path.insert(0, ROOT)
    import oracle as O

    with open(spec_path) as f:
        runs = json.load(f)
    res = {}
    for i, r in enumerate(runs):
        init = np.array(r["init"], dtype=np.uint64).view(np.float64).reshape(-1, r["dim"])
        mat = None if r["matrix"] is None else np.array(r["matrix"], dtype=np.float64).reshape(r["dim"], r["dim"])
        adapt = None if r.get("adapt") is None else np.array(r["adapt"], dtype=np.uint64).view(np.float64).reshape(-1, 4)
        out = O.engine_host_nuts_run(r["mode"], getattr(O, r["kind"]), r["dim"], r.get("params", []), init, 0.8, r["n_collect"],
                                     r["n_discard"], seed=r["seed"], chain_offset=r["chain_offset"], max_depth=r["max_depth"],
                                     progress=r["progress"], matrix=mat, m0=r.get("m0", 0), adapt=adapt,
                                     n_threads=r.get("n_threads", 1))
        for name, a in zip(NAMES, out):
            res[f"{i}_{name}"] = a
    np.savez(out_path, **res)


def _run_child(tmp_path, runs, tag):
    """Every run of `runs` in one child process; a list of dicts sample / pos / adapt / nlf.  A child that does not return
    within the limit fails the test."""
    spec, out = tmp_path / f"{tag}.json", tmp_path / f"{tag}.npz"
    spec.write_text(json.dumps(runs))
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), str(spec), str(out)], timeout=CHILD_TIMEOUT,
                           capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        pytest.fail(f"{tag}: the host twin did not return within {CHILD_TIMEOUT} s (the step-size search does not end)")
    assert p.returncode == 0, p.stderr[-2000:]
    with np.load(out) as z:
        return [{name: z[f"{i}_{name}"] for name in NAMES} for i in range(len(runs))]


def _run(mode, kind, dim, init, seed=5, chain_offset=0, max_depth=10, progress=False, matrix=None, n_collect=N_COLLECT,
         n_discard=N_DISCARD, params=(), m0=0, adapt=None, n_threads=1):
    """one run of the child; floats travel as their bit patterns (NaN and inf are not JSON)"""
    init = np.ascontiguousarray(init, dtype=np.float64)
    return dict(mode=mode, kind=kind, dim=dim, init=init.view(np.uint64).ravel().tolist(), seed=seed, chain_offset=chain_offset,
                max_depth=max_depth, progress=progress, n_collect=n_collect, n_discard=n_discard, params=list(params), m0=m0,
                adapt=None if adapt is None else np.ascontiguousarray(adapt, dtype=np.float64).view(np.uint64).ravel().tolist(),
                n_threads=n_threads,
                matrix=None if matrix is None else np.asarray(matrix, dtype=np.float64).ravel().tolist())


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _same(a, b):
    return all(a[k].shape == b[k].shape and np.array_equal(_bits(a[k]), _bits(b[k])) for k in NAMES)


def _bad_rows(dim, overflow):
    """(name, start) of the non-real starts: one bad coordinate each, at a different place, the others ordinary"""
    rows = []
    for j, (name, v) in enumerate((("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf), ("overflow", overflow))):
        x = np.linspace(-0.9, 1.1, dim)
        x[(j * 5 + 1) % dim] = v
        rows.append((name, x))
    return rows


def _mixed(O, dim, overflow, seed):
    """healthy and bad starts interleaved: [(is_bad, name, row)]"""
    good = O.init_with_seed(6, dim, seed).astype(np.float64) * 0.7
    bad = _bad_rows(dim, overflow)
    order = [("g", 0), ("b", 0), ("g", 1), ("b", 1), ("b", 2), ("g", 2), ("g", 3), ("b", 3), ("g", 4), ("g", 5)]
    return [(w == "b", bad[i][0] if w == "b" else "good", bad[i][1] if w == "b" else good[i]) for w, i in order]


def _check_mixed(tmp_path, O, mode, kind, dim, overflow, matrix=None, max_depth=10):
    rows = _mixed(O, dim, overflow, 17 + mode)
    init = np.stack([r for _, _, r in rows])
    isbad = np.array([b for b, _, _ in rows])
    runs = [_run(mode, kind, dim, init, matrix=matrix, max_depth=max_depth, progress=pr) for pr in (False, True)]
    # the healthy chains alone, each stretch of them at its chain offset (the stream is a function of the global chain id)
    stretches, c = [], 0
    while c < len(rows):
        if isbad[c]:
            c += 1
            continue
        e = c
        while e < len(rows) and not isbad[e]:
            e += 1
        stretches.append((c, e))
        c = e
    for lo, hi in stretches:
        runs.append(_run(mode, kind, dim, init[lo:hi], chain_offset=lo, matrix=matrix, max_depth=max_depth))
    res = _run_child(tmp_path, runs, f"mixed_m{mode}_{kind}_{dim}")
    tdt = np.float32 if mode in F32_MODES else np.float64
    start = init.astype(tdt)
    for r, pr in zip(res[:2], (False, True)):
        assert r["sample"].dtype == tdt and r["sample"].shape == (len(rows), N_COLLECT, dim)
        for c in np.flatnonzero(isbad):
            what = (mode, rows[c][1], "progress" if pr else "run")
            assert np.array_equal(_bits(r["sample"][c]), np.broadcast_to(_bits(start[c]), (N_COLLECT, dim))), what
            assert np.array_equal(_bits(r["pos"][c]), _bits(start[c])), what
            # one leapfrog per transition: the tree stops at its first leaf (run() makes N - 1 transitions, nuts.rs:163-170)
            assert r["nlf"][c] == N_COLLECT + N_DISCARD - (0 if pr else 1), what
    full = res[0]
    for (lo, hi), alone in zip(stretches, res[2:]):
        part = {k: full[k][lo:hi] for k in NAMES}
        assert _same(part, alone), (mode, lo, hi)
        assert np.isfinite(alone["sample"]).all() and np.isfinite(alone["adapt"]).all() and (alone["adapt"][:, 0] > 0).all()
    return res


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_nuts_nonreal_starts_end_and_stay_put(O, tmp_path, mode):
    """RosenbrockND(3), type modes 0, 1, 2, run() and run_progress(): chains that start at NaN, +inf, -inf or at a finite
    point whose density overflows the tensor type (1e20 in f32, 1e200 in f64) return, keep their start bits in every
    collected row and make one leapfrog per transition; the healthy chains between them equal, bit for bit (samples,
    positions, adaptation, leapfrog counts), the run of those chains alone at their chain offsets."""
    _check_mixed(tmp_path, O, mode, "ROSENBROCK_ND", 3, 1e20 if mode < 2 else 1e200)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_generic_nuts_twin_nonreal_starts(O, tmp_path, mode):
    """The same through mm_nuts_generic.h (modes 4, 5, 6 of the twin, the call test_generic_dim.py uses), at a dimension with
    a fixed instance (3, where both twins must also agree bit for bit) and at one without (11)."""
    over = 1e20 if mode < 2 else 1e200
    gen = _check_mixed(tmp_path, O, mode + 4, "ROSENBROCK_ND", 3, over)
    rows = _mixed(O, 3, over, 17 + mode + 4)
    fixed = _run_child(tmp_path, [_run(mode, "ROSENBROCK_ND", 3, np.stack([r for _, _, r in rows]))], f"fixed_m{mode}")
    assert _same(gen[0], fixed[0])
    _check_mixed(tmp_path, O, mode + 4, "ROSENBROCK_ND", 11, over)


@pytest.mark.parametrize("dim", [16, 32])
def test_grouped_nuts_twin_nonreal_starts(O, tmp_path, dim):
    """Mode 3, the twin of the lane-group kernels (GaussianND, f64, grouped reductions): a NaN or infinite coordinate
    spreads through A x to every coordinate of the gradient, and x^T A x overflows at 1e200."""
    rng = np.random.default_rng(dim)
    B = rng.standard_normal((dim, dim))
    A = B @ B.T / dim + np.eye(dim)
    _check_mixed(tmp_path, O, 3, "GAUSSIAN_ND", dim, 1e200, matrix=A, max_depth=6)


FAR = {"f32": [[30.0, -30.0, 30.0], [-30.0, 30.0, -30.0], [1e6, -1e6, 1e6]],
       "f64": [[30.0, -30.0, 30.0], [-30.0, 30.0, -30.0], [1e40, -1e40, 1e40]]}
FAR_SEEDS = (3, 11)


def _rosen(x, dt):
    """mm_targets.h RosenbrockND logp and gradient in the tensor type, up to the fused roundings (only overflow matters here)"""
    x = np.asarray(x, dtype=dt)
    with np.errstate(all="ignore"):
        t = x[1:] - x[:-1] * x[:-1]
        u = dt(1) - x[:-1]
        lp = -np.sum(dt(100) * t * t + u * u, dtype=dt)
        g = np.zeros_like(x)
        g[:-1] = dt(400) * x[:-1] * t + dt(2) * u
        g[1:] += dt(-200) * t
    return lp, g


def test_far_starts_take_the_first_loop():
    """A condition on the inputs of the next test, from the target alone: at the third start of FAR the first leapfrog of the
    search (step 1) ends at a non-real log-density and gradient whatever the momentum is (|z| < 10 for Box-Muller of 53-bit
    uniforms), while the start itself is real -- so the halving loop is entered and has to end on its own."""
    for name, dt in (("f32", np.float32), ("f64", np.float64)):
        x0 = np.array(FAR[name][2], dtype=dt)
        lp0, g0 = _rosen(x0, dt)
        assert np.isfinite(lp0) and np.isfinite(g0).all()
        for s in range(8):
            z = np.array([10.0 if s >> i & 1 else -10.0 for i in range(3)], dtype=dt)
            with np.errstate(all="ignore"):
                lp1, g1 = _rosen(x0 + (z + dt(0.5) * g0), dt)
            assert not np.isfinite(lp1) and not np.isfinite(g1).all(), (name, s)


def _far_runs():
    runs, keys = [], []
    for mode in (0, 1, 2, 4, 5, 6):
        for seed in FAR_SEEDS:
            runs.append(_run(mode, "ROSENBROCK_ND", 3, FAR["f32" if mode in F32_MODES else "f64"], seed=seed))
            keys.append(f"mode{mode}_seed{seed}")
    return runs, keys


def test_far_but_finite_starts_unchanged(O, tmp_path):
    """Far starts with a real log-density, where the loops of the search are taken and end on their own, give the samples the
    code gave before the loops were bounded: tests/golden/nuts_far_starts.json holds that commit's host-twin output
    (samples, positions, adaptation records, leapfrog counts as integer bit patterns) for two seeds, modes 0, 1, 2 and the
    generic twin's 4, 5, 6."""
    runs, keys = _far_runs()
    res = _run_child(tmp_path, runs, "far")
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert sorted(gold) == sorted(keys)
    for k, r in zip(keys, res):
        for name in NAMES:
            assert _bits(r[name]).ravel().tolist() == gold[k][name], (k, name)
        assert np.isfinite(r["sample"]).all() and (r["adapt"][:, 0] > 0).all(), k
    # the generic twin is the fixed one operation for operation
    for mode in (0, 1, 2):
        for seed in FAR_SEEDS:
            assert gold[f"mode{mode}_seed{seed}"] == gold[f"mode{mode + 4}_seed{seed}"]


if __name__ == "__main__":
    _child_main(sys.argv[1], sys.argv[2])
