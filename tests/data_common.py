"""Shared by the tests of targets that carry data (tests/test_data_target_*.py): the two models, their bound arrays, their
sources (tests/cpp/data_cases/), the host program tests/cpp/data_host.cpp built and run once per session, and float64 numpy
restatements.

linreg3  dim 3, 7 rows [x0 x1 x2 y] (data_len 28 > dim^2 = 9), noise sd 2, prior N(0, 2^2): a Gaussian posterior in closed form.
logit9   dim 9, 5 rows [x0 .. x8 y] (data_len 50 < dim^2 = 81), prior N(0, 1), log(1 + e^eta) through mm_softplusT.
Every value is a multiple of 1/8 (exact in f32: the f32 and f64 kinds see the same model), every regressor nonzero.  In both arrays the
last row is unlike the others -- linreg3's has the largest leverage and response, logit9's response is the one fractional y
-- and the last element is that row's response, so an upload short by one element changes every answer."""
import functools
import os
import tempfile

import numpy as np

import autodiff_common as A

ROOT = A.ROOT
CASES = os.path.join(ROOT, "tests", "cpp", "data_cases")
SRC = os.path.join(ROOT, "tests", "cpp", "data_host.cpp")

LINREG3 = np.array([[1.0, 0.5, -0.75, 1.25],
                    [-0.5, 1.25, 0.5, -0.875],
                    [0.75, -1.0, 1.5, 1.5],
                    [-1.25, 0.25, -0.5, -1.0],
                    [0.5, 0.75, 1.0, 0.625],
                    [-1.0, -0.5, 0.25, -0.375],
                    [2.0, -1.5, 1.75, 3.5]])
LINREG3_PARAMS = [0.25, 0.25]  # 1 / sigma^2 (noise sd 2), 1 / tau^2 (prior sd 2); tests/cpp/data_host.cpp has the same


def _logit9():
    a = ((np.arange(50).reshape(5, 10) * 7) % 23 - 11) / 8.0  # multiples of 1/8 in [-11/8, 11/8]
    a[a == 0] = 0.125
    a[:, 0] = 1.0  # intercept
    a[:, 9] = [1.0, 0.0, 1.0, 0.0, 0.75]  # the last response is a proportion: the one row with a weight of its own
    return a


LOGIT9 = _logit9()
MODELS = {"linreg3": (3, LINREG3, LINREG3_PARAMS), "logit9": (9, LOGIT9, [])}


def source(model, flavour):
    """the HIP source of `model` ("linreg3" | "logit9") as `flavour` ("logp": autodiff body | "hand": hand-written gradient)"""
    return open(os.path.join(CASES, f"{model}_{flavour}.inc")).read()


def build_host(out_dir, sanitize=False):
    import subprocess

    cxx, flags = A.host_flags()
    exe = os.path.join(out_dir, "data_host" + ("_san" if sanitize else ""))
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    r = subprocess.run([cxx] + flags + extra + [SRC, "-o", exe, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run_host(exe, out_dir):
    """{(case, "f32" | "f64"): {"x", "value", "value_plain", "grad", ["value_hand", "grad_hand"]}} for the cases linreg3,
    logit9, softplus, softplus_composed, sigmoid (the layout of autodiff_common.run_host)"""
    import subprocess

    data, path = os.path.join(out_dir, "data.bin"), os.path.join(out_dir, os.path.basename(exe) + ".bin")
    np.concatenate([LINREG3.reshape(-1), LOGIT9.reshape(-1)]).astype(np.float64).tofile(data)
    r = subprocess.run([exe, path, data], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    raw = open(path, "rb").read()
    res = {}
    for ln in r.stdout.splitlines():
        name, ty, dim, n, off, hand = ln.split()
        dim, n, off = int(dim), int(n), int(off)
        dt = np.float32 if ty == "f32" else np.float64
        fields = [("x", (n, dim)), ("value", (n,)), ("value_plain", (n,)), ("grad", (n, dim))]
        if hand == "1":
            fields += [("value_hand", (n,)), ("grad_hand", (n, dim))]
        rec = {}
        for key, shape in fields:
            cnt = int(np.prod(shape))
            rec[key] = np.frombuffer(raw, dtype=dt, count=cnt, offset=off).reshape(shape).copy()
            off += cnt * np.dtype(dt).itemsize
        res[(name, ty)] = rec
    return res


@functools.lru_cache(maxsize=None)
def host_results():
    """the host program's output, built with the host twin's flags; computed once and shared (treat as read-only)"""
    d = tempfile.mkdtemp(prefix="data_host_")
    return run_host(build_host(d), d)


def linreg3_posterior(rows=LINREG3):
    """(mean, covariance) of linreg3's Gaussian posterior in float64: (X^T X / sigma^2 + I / tau^2)^-1, and that times X^T y / sigma^2"""
    x, y = rows[:, :3], rows[:, 3]
    prec = LINREG3_PARAMS[0] * x.T @ x + LINREG3_PARAMS[1] * np.eye(3)
    cov = np.linalg.inv(prec)
    return cov @ (LINREG3_PARAMS[0] * x.T @ y), cov


# an isotropic Gaussian random walk as a user proposal (tests/test_autodiff_gpu.py has the same)
ISOTROPIC = r"""
template <class T> struct mmcmc_user_proposal {
    MM_HD static void sample(T sigma, const T *x, const T *z, T *out) {
        for (int i = 0; i < MM_USER_DIM; ++i)
            out[i] = mm_fma(sigma, z[i], x[i]);
    }
    MM_HD static T logp(T sigma, const T *from, const T *to) {
        const T var = sigma * sigma;
        T acc = 0;
        for (int i = 0; i < MM_USER_DIM; ++i) {
            const T d = to[i] - from[i];
            acc += -(d * d) / (T(2) * var);
        }
        return acc;
    }
};
"""
