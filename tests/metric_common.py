"""Shared by tests/test_metric_host.py and tests/test_metric_gpu.py: the host twin of the diagonal metric
(tests/cpp/metric_twin.cpp), built once per test session with the host compiler and flags of oracle/Makefile, and readers of
what it writes."""
import os
import subprocess

import numpy as np

import autodiff_common as A

ROOT = A.ROOT
SRC = os.path.join(ROOT, "tests", "cpp", "metric_twin.cpp")
_built = {}


def build_twin(tmp_path_factory, sanitize=False):
    """the twin's executable; sanitize: -fsanitize=address,undefined (a stand-alone program: its runtimes are linked in)"""
    if sanitize not in _built:
        cxx, flags = A.host_flags()
        exe = str(tmp_path_factory.mktemp("metric_twin") / ("metric_twin_san" if sanitize else "metric_twin"))
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


def twin_hmc(exe, out_dir, dtype, target, n_chains, n_collect, n_discard, eps, n_leapfrog, seed, scale=None, print_noise=False):
    """(samples, state, accept counts, stdout) of the twin's HMC run; target "rosen3" or "gauss2d" """
    dim = 3 if target == "rosen3" else 2
    path = os.path.join(str(out_dir), f"hmc_{np.dtype(dtype).name}_{target}_{n_chains}_{'m' if scale is not None else 'n'}.bin")
    args = [exe, "hmc", "f64" if dtype == np.float64 else "f32", target, str(n_chains), str(n_collect), str(n_discard), repr(float(eps)),
            str(n_leapfrog), str(seed), path, "1" if print_noise else "0"] + ([repr(float(v)) for v in scale] if scale is not None else [])
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = open(path, "rb").read()
    esz = np.dtype(dtype).itemsize
    n_s, n_x = n_chains * n_collect * dim, n_chains * dim
    assert len(raw) == (n_s + n_x) * esz + 8 * n_chains
    samples = np.frombuffer(raw, dtype=dtype, count=n_s).reshape(n_chains, n_collect, dim)
    state = np.frombuffer(raw, dtype=dtype, count=n_x, offset=n_s * esz).reshape(n_chains, dim)
    accept = np.frombuffer(raw, dtype=np.uint64, count=n_chains, offset=(n_s + n_x) * esz)
    return samples, state, accept, r.stdout


def twin_nuts(exe, out_dir, mode, n_chains, n_collect, n_discard, seed, scale=None):
    """RosenbrockND(3): (samples, positions, adapt [C, 4] f64, leapfrog counts, depth histogram [13]) of the twin's run()"""
    dtype = np.float64 if mode == 2 else np.float32
    path = os.path.join(str(out_dir), f"nuts_{mode}_{n_chains}_{'m' if scale is not None else 'n'}.bin")
    args = [exe, "nuts", str(mode), str(n_chains), str(n_collect), str(n_discard), str(seed), path] + \
           ([repr(float(v)) for v in scale] if scale is not None else [])
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = open(path, "rb").read()
    esz = np.dtype(dtype).itemsize
    n_s, n_x = n_chains * n_collect * 3, n_chains * 3
    off = 0
    samples = np.frombuffer(raw, dtype=dtype, count=n_s, offset=off).reshape(n_chains, n_collect, 3)
    off += n_s * esz
    positions = np.frombuffer(raw, dtype=dtype, count=n_x, offset=off).reshape(n_chains, 3)
    off += n_x * esz
    adapt = np.frombuffer(raw, dtype=np.float64, count=4 * n_chains, offset=off).reshape(n_chains, 4)
    off += 32 * n_chains
    nlf = np.frombuffer(raw, dtype=np.uint64, count=n_chains, offset=off)
    off += 8 * n_chains
    hist = np.frombuffer(raw, dtype=np.uint32, count=13, offset=off)
    assert off + 52 == len(raw)
    return samples, positions, adapt, nlf, hist
