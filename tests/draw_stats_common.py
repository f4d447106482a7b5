"""Shared by tests/test_draw_stats_host.py and tests/test_draw_stats_gpu.py: the host twin of NUTS's per-draw records
(tests/cpp/draw_stats_twin.cpp), built once per test session with the host compiler and flags of oracle/Makefile, readers of
what it writes, and the float64 restatement of the per-chain summary."""
import os
import subprocess

import numpy as np

import autodiff_common as A

ROOT = A.ROOT
SRC = os.path.join(ROOT, "tests", "cpp", "draw_stats_twin.cpp")
DRAW = np.dtype([("accept_stat", np.float32), ("step_size", np.float32), ("energy", np.float32), ("tree", np.uint32)])
DIAG = np.array([0.37, 2.9, 11.0])
CHOL = np.array([[0.37, 0.0, 0.0], [-0.8, 2.9, 0.0], [1.5, -2.25, 11.0]])  # the twin's general_factor()
DIVERGENT, DEPTH_CAP, NONE = np.uint32(1 << 24), np.uint32(1 << 25), np.uint32(1 << 31)
_built = {}
_runs = {}


def build_twin(tmp_path_factory, sanitize=False):
    """the twin's executable; sanitize: -fsanitize=address,undefined (a stand-alone program: its runtimes are linked in)"""
    if sanitize not in _built:
        cxx, flags = A.host_flags()
        exe = str(tmp_path_factory.mktemp("draw_stats_twin") / ("draw_stats_twin_san" if sanitize else "draw_stats_twin"))
        extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
        r = subprocess.run([cxx] + flags + extra + [SRC, "-o", exe, "-lm"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        _built[sanitize] = exe
    return _built[sanitize]


def start(n_chains, dim):
    """the twin's fixed start: x0[c][i] = 0.05 * ((7 c + 13 i) mod 17 - 8) + 0.01 i, float64"""
    c = np.arange(n_chains)[:, None]
    i = np.arange(dim)[None, :]
    return 0.05 * (((c * 7 + i * 13) % 17) - 8).astype(np.float64) + 0.01 * i


def _read(path, mode, n_chains, n_collect, dim):
    dtype = np.float64 if mode == 2 else np.float32
    raw = open(path, "rb").read()
    esz = np.dtype(dtype).itemsize
    n_s, n_x = n_chains * n_collect * dim, n_chains * dim
    off = 0
    samples = np.frombuffer(raw, dtype=dtype, count=n_s, offset=off).reshape(n_chains, n_collect, dim)
    off += n_s * esz
    positions = np.frombuffer(raw, dtype=dtype, count=n_x, offset=off).reshape(n_chains, dim)
    off += n_x * esz
    adapt = np.frombuffer(raw, dtype=np.float64, count=4 * n_chains, offset=off).reshape(n_chains, 4)
    off += 32 * n_chains
    nlf = np.frombuffer(raw, dtype=np.uint64, count=n_chains, offset=off)
    off += 8 * n_chains
    hist = np.frombuffer(raw, dtype=np.uint32, count=13, offset=off)
    off += 52
    rec = np.frombuffer(raw, dtype=DRAW, count=n_chains * n_collect, offset=off).reshape(n_chains, n_collect)
    assert off + 16 * n_chains * n_collect == len(raw)
    return samples, positions, adapt, nlf, hist, rec


def twin_nuts(tmp_path_factory, mode, n_chains, n_collect, n_discard, progress, seed, metric="none"):
    """RosenbrockND(3) under the recording policy: (samples, positions, adapt [C, 4] f64, leapfrog counts, depth histogram [13],
    records [C, n_collect]) of the twin's run() (progress False) or run_progress stepping; computed once per argument tuple"""
    key = ("nuts", mode, n_chains, n_collect, n_discard, bool(progress), seed, metric)
    if key not in _runs:
        exe = build_twin(tmp_path_factory)
        path = str(tmp_path_factory.mktemp("draw_stats_run") / "nuts.bin")
        r = subprocess.run([exe, "nuts", str(mode), str(n_chains), str(n_collect), str(n_discard), "1" if progress else "0", str(seed), metric, path],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        _runs[key] = _read(path, mode, n_chains, n_collect, 3)
    return _runs[key]


def twin_gauss(tmp_path_factory, mode, n_chains, rows, eps, seed):
    """Gaussian2D with unit covariance from epsilon = epsilon_bar = eps, run(rows, 0): the same tuple"""
    key = ("gauss", mode, n_chains, rows, float(eps), seed)
    if key not in _runs:
        exe = build_twin(tmp_path_factory)
        path = str(tmp_path_factory.mktemp("draw_stats_run") / "gauss.bin")
        r = subprocess.run([exe, "gauss", str(mode), str(n_chains), str(rows), repr(float(eps)), str(seed), path], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        _runs[key] = _read(path, mode, n_chains, rows, 2)
    return _runs[key]


def summary_f64(rec):
    """The per-chain summary restated in numpy float64, two-pass: a dict of arrays [chains].  ebfmi: differences between
    consecutive rows that both have a transition (the one row without is row 0)."""
    rec = np.asarray(rec)
    n_chains = rec.shape[0]
    out = {k: np.zeros(n_chains, dtype=np.uint32) for k in ("n_transitions", "n_divergent", "n_depth_cap", "max_depth_seen")}
    out["n_leapfrog"] = np.zeros(n_chains, dtype=np.uint64)
    for k in ("mean_accept", "mean_step", "ebfmi"):
        out[k] = np.full(n_chains, np.nan)
    for c in range(n_chains):
        r = rec[c]
        has = (r["tree"] >> np.uint32(31)) == 0
        t = r["tree"][has]
        n = int(has.sum())
        out["n_transitions"][c] = n
        out["n_divergent"][c] = int(((t >> np.uint32(24)) & np.uint32(1)).sum())
        out["n_depth_cap"][c] = int(((t >> np.uint32(25)) & np.uint32(1)).sum())
        out["max_depth_seen"][c] = int(((t >> np.uint32(16)) & np.uint32(15)).max()) if n else 0
        out["n_leapfrog"][c] = int((t & np.uint32(0xFFFF)).astype(np.uint64).sum())
        if n:
            out["mean_accept"][c] = r["accept_stat"][has].astype(np.float64).sum() / n
            out["mean_step"][c] = r["step_size"][has].astype(np.float64).sum() / n
        e = r["energy"].astype(np.float64)
        if n >= 2:
            mean = e[has].sum() / n
            den = ((e[has] - mean) ** 2).sum()
            both = has[1:] & has[:-1]
            num = ((e[1:] - e[:-1])[both] ** 2).sum()
            if den != 0.0:
                out["ebfmi"][c] = num / den
    return out
