"""Shared by tests/test_dense_metric_host.py and tests/test_dense_metric_gpu.py: the host twin of the dense metric
(tests/cpp/dense_metric_twin.cpp), built once per test session with the host compiler and flags of oracle/Makefile, the
factors the tests use, and readers of what the twin writes."""
import os
import subprocess
import zlib

import numpy as np

import autodiff_common as A
import metric_common as M

ROOT = A.ROOT
SRC = os.path.join(ROOT, "tests", "cpp", "dense_metric_twin.cpp")
start = M.start
_built = {}


def build_twin(tmp_path_factory, sanitize=False):
    """the twin's executable; sanitize: -fsanitize=address,undefined (a stand-alone program: its runtimes are linked in)"""
    if sanitize not in _built:
        cxx, flags = A.host_flags()
        exe = str(tmp_path_factory.mktemp("dense_metric_twin") / ("dense_metric_twin_san" if sanitize else "dense_metric_twin"))
        # -O0 for the instrumented build: it compiles in a sixth of the time, and with -ffp-contract=off the bits do not depend on it
        extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O0"] if sanitize else []
        r = subprocess.run([cxx] + flags + extra + [SRC, "-o", exe, "-lm"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        _built[sanitize] = exe
    return _built[sanitize]


def general_factor(dim):
    """A lower-triangular factor far from the identity: diagonal 0.5 .. 1, off-diagonal entries up to 1.2 / sqrt(dim) in
    magnitude and of both signs, none of them a power of two.  Every entry of the lower triangle is non-zero and no two
    neighbours in the packed order are equal: at dim 32 the last row of L (32 entries) and the last column of L^T are full, so
    a packed index that is off by one reads another value and changes the sample."""
    i, j = np.arange(dim)[:, None], np.arange(dim)[None, :]
    c = 0.6 * (((i * 7 + j * 3) % 5) - 2 + 0.37) / np.sqrt(dim)
    c = np.tril(c, -1)
    c[np.arange(dim), np.arange(dim)] = 0.5 + 0.25 * (np.arange(dim) % 3) + 0.013
    return c


def pow2_scales(dim):
    """2^-3 .. 2^3"""
    return np.ldexp(1.0, (np.arange(dim) * 5 + 3) % 7 - 3)


def _factor_file(out_dir, chol):
    path = os.path.join(str(out_dir), f"factor_{chol.shape[0]}_{zlib.crc32(np.ascontiguousarray(chol, dtype=np.float64).tobytes())}.bin")
    np.ascontiguousarray(chol, dtype=np.float64).tofile(path)
    return path


def twin_hmc(exe, out_dir, dtype, dim, n_chains, n_collect, n_discard, eps, n_leapfrog, seed, chol, print_noise=False):
    """(samples, state, accept counts, stdout) of the twin's HMC run under the factor chol; dim 2: Gaussian2D, else RosenbrockND"""
    path = os.path.join(str(out_dir), f"dense_hmc_{np.dtype(dtype).name}_{dim}_{n_chains}.bin")
    args = [exe, "hmc", "f64" if dtype == np.float64 else "f32", str(dim), str(n_chains), str(n_collect), str(n_discard), repr(float(eps)),
            str(n_leapfrog), str(seed), path, "1" if print_noise else "0", _factor_file(out_dir, chol)]
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


def twin_nuts(exe, out_dir, mode, dim, n_chains, n_collect, n_discard, seed, chol):
    """RosenbrockND(dim): (samples, positions, adapt [C, 4] f64, leapfrog counts, depth histogram [13]) of the twin's run()"""
    dtype = np.float64 if mode == 2 else np.float32
    path = os.path.join(str(out_dir), f"dense_nuts_{mode}_{dim}_{n_chains}.bin")
    args = [exe, "nuts", str(mode), str(dim), str(n_chains), str(n_collect), str(n_discard), str(seed), path, _factor_file(out_dir, chol)]
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
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
    assert off + 52 == len(raw)
    return samples, positions, adapt, nlf, hist
