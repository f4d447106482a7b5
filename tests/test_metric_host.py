"""The diagonal metric of HMC and NUTS without a GPU (include/mmcmc.h: "A diagonal mass matrix").

  * tests/cpp/metric_twin.cpp -- the host build of the kernels' own headers -- checks that a metric of ones gives the bits of
    no metric and the power-of-two identity (its head comment), as built and once more under the address and
    undefined-behaviour sanitizers (a stand-alone program: no preload involved);
  * an independent float64 restatement in numpy of diagonal-metric HMC, with the half-kicks kept apart as hmc.rs:403-429
    writes them, on the noise the twin prints;
  * tests/cpp/metric_host.cpp -- csrc/mm_metric_host.h on its own: the diagonal checks with the device image they produce,
    and the record of the metric both handle types keep --, likewise plain and under the sanitizers;
  * the four entry points refuse a NULL handle;
  * warmup.estimate_scale against numpy float64."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import autodiff_common as A
import metric_common as M


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_twin_ones_metric_is_no_metric_and_power_of_two_identity(tmp_path_factory, sanitize):
    exe = M.build_twin(tmp_path_factory, sanitize)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-4000:])
    m = re.search(r"checks (\d+) failed (\d+)", r.stdout)
    assert m, r.stdout[-1000:]
    checks, failed = map(int, m.groups())
    assert failed == 0
    # not vacuous: (a) 2 targets x 3 L x 2 + 3 modes x 5; (b) 4 dims x (2 dtypes x 3 L x 2 + 3 modes x 2 x 2)
    assert checks == 2 * 3 * 2 + 3 * 5 + 4 * (2 * 3 * 2 + 3 * 2 * 2)


def test_metric_host_header_is_host_only():
    text = open(os.path.join(M.ROOT, "mini_mcmc_amd", "csrc", "mm_metric_host.h")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', text) == ["cmath", "cstddef", "vector"]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_diagonal_checks_and_the_metric_record_on_the_host(tmp_path, sanitize):
    """tests/cpp/metric_host.cpp (its head comment), plain host code with its own main: as built and once more linked with
    the address and undefined-behaviour sanitizers' runtimes, no preload involved"""
    cxx, flags = A.host_flags()
    exe = str(tmp_path / "metric_host")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    r = subprocess.run([cxx] + flags + extra + [os.path.join(M.ROOT, "tests", "cpp", "metric_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-4000:])
    m = re.search(r"checks (\d+) failed (\d+)", r.stdout)
    assert m, r.stdout[-1000:]
    checks, failed = map(int, m.groups())
    assert failed == 0
    # not vacuous.  mm_diag_prepare: placements = the positions of D = 1 and D = 3; two forms (without / with the inverse)
    accepted, placements, forms = 5, 1 + 3, 2
    bad = {"float": 6 + 2, "double": 6}  # NaN, +inf, -inf, 0, -0.0, -1; as float also 1e-60 and 1e60
    diag = sum(accepted * 2 * forms + n * placements * forms + 2 * placements for n in bad.values())
    # the record: 2 starting variants, every sequence of 1 .. 3 out of 5 operations, 4 checks after each operation
    record = 2 * 4 * sum(length * 5 ** length for length in (1, 2, 3))
    assert checks == diag + record


def test_float64_restatement_of_diagonal_metric_hmc_on_the_twins_noise(tmp_path_factory, tmp_path):
    """Gaussian2D in f64, scales (0.37, 2.9), 20 transitions of 4 chains.  The restatement keeps the two half-kicks of every
    leapfrog step apart and uses no fused operation; the engine merges kicks and fuses: two roundings per operation over at
    most 20 * L steps of a well-conditioned target, so states agree to 1e-12 relative and every accept decision is the
    same."""
    exe = M.build_twin(tmp_path_factory)
    n, T, L, eps = 4, 20, 5, 0.4
    s = np.array([0.37, 2.9])
    samples, state, accept, text = M.twin_hmc(exe, tmp_path, np.float64, "gauss2d", n, T, 0, eps, L, 11, scale=s, print_noise=True)
    noise = np.zeros((n, T, 3))
    got_x = np.zeros((n, T, 2))
    got_acc = np.zeros((n, T), dtype=int)
    for line in text.splitlines():
        f = line.split()
        c, t = int(f[1]), int(f[2])
        if f[0] == "noise":
            noise[c, t] = [float.fromhex(v) for v in f[3:6]]
        elif f[0] == "state":
            got_x[c, t] = [float.fromhex(v) for v in f[3:5]]
            got_acc[c, t] = int(f[5])
    assert np.array_equal(got_x, samples) and np.array_equal(got_acc.sum(axis=1), accept.astype(int))
    mean = np.array([0.0, 1.0])
    sinv = np.linalg.inv(np.array([[4.0, 2.0], [2.0, 3.0]]))
    logp = lambda x: -0.5 * (x - mean) @ sinv @ (x - mean)  # noqa: E731 -- the constant cancels in the accept ratio
    grad = lambda x: -0.5 * (sinv + sinv.T) @ (x - mean)  # noqa: E731
    e = eps * s  # M = diag(1 / s^2) in whitened momentum: the step of coordinate i is eps * s_i
    x = M.start(n, 2)
    n_acc = 0
    for c in range(n):
        xc = x[c].copy()
        for t in range(T):
            p = noise[c, t, :2].copy()
            h0 = -logp(xc) + 0.5 * p @ p
            xn = xc.copy()
            for _ in range(L):
                p = p + 0.5 * e * grad(xn)
                xn = xn + e * p
                p = p + 0.5 * e * grad(xn)
            h1 = -logp(xn) + 0.5 * p @ p
            acc = (h0 - h1) >= noise[c, t, 2]
            assert acc == bool(got_acc[c, t]), (c, t, h0 - h1, noise[c, t, 2])
            if acc:
                xc = xn
                n_acc += 1
            assert np.allclose(xc, got_x[c, t], rtol=1e-12, atol=0), (c, t, xc, got_x[c, t])
    assert 0.3 * n * T < n_acc < n * T  # a trajectory that moves, and rejects now and then


def test_metric_entry_points_reject_a_null_handle():
    from mini_mcmc_amd import _lib as L

    lib = L.lib()
    s = (C.c_double * 3)(1.0, 2.0, 3.0)
    for name in ("mmcmc_hmc_set_metric", "mmcmc_hmc_metric", "mmcmc_nuts_set_metric", "mmcmc_nuts_metric"):
        assert getattr(lib, name)(None, s) == L.ERR_INVALID_ARG, name
        assert getattr(lib, name)(None, None) == L.ERR_INVALID_ARG, name
    assert lib.mmcmc_version() == 102


def test_estimate_scale_against_numpy_float64():
    from mini_mcmc_amd.warmup import estimate_scale

    rng = np.random.default_rng(5)
    a = rng.normal(size=(7, 13, 3)) * np.array([1e-2, 1.0, 1e2]) + np.array([3.0, -1.0, 50.0])
    flat = a.reshape(-1, 3).astype(np.float64)
    n = flat.shape[0]
    var = flat.var(axis=0)  # population variance over all chains and draws
    assert np.allclose(estimate_scale(a, regularize=False), np.sqrt(var), rtol=1e-14, atol=0)
    assert np.allclose(estimate_scale(a), np.sqrt(n / (n + 5.0) * var + 1e-3 * 5.0 / (n + 5.0)), rtol=1e-14, atol=0)
    assert np.allclose(estimate_scale(a.astype(np.float32), regularize=False), np.sqrt(a.astype(np.float32).astype(np.float64).reshape(-1, 3).var(axis=0)),
                       rtol=1e-14, atol=0)
    assert estimate_scale(a).dtype == np.float64 and estimate_scale(a).shape == (3,)
    with pytest.raises(ValueError):
        estimate_scale(flat)
