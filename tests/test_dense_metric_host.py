"""The dense metric of HMC and NUTS without a GPU (include/mmcmc.h: "A dense mass matrix from a Cholesky factor").

  * tests/cpp/dense_metric_twin.cpp -- the host build of the kernels' own headers -- checks that an identity factor gives the
    bits of no metric and a power-of-two diagonal factor the bits of the diagonal metric (its head comment), as built and once
    more under the address and undefined-behaviour sanitizers (a stand-alone program: no preload involved; the factors live
    in heap blocks of exactly D (D + 1) / 2 elements);
  * an independent float64 restatement in numpy of HMC with mass matrix M = (L L^T)^-1 in unwhitened momentum, on the noise
    the twin prints;
  * warmup.estimate_chol against numpy float64;
  * the four entry points refuse a NULL handle and are declared in every binding."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dense_metric_common as DM


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_twin_identity_factor_is_no_metric_and_power_of_two_factor_is_the_diagonal_metric(tmp_path_factory, sanitize):
    exe = DM.build_twin(tmp_path_factory, sanitize)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-4000:])
    m = re.search(r"checks (\d+) failed (\d+)", r.stdout)
    assert m, r.stdout[-1000:]
    checks, failed = map(int, m.groups())
    assert failed == 0
    # not vacuous: 4 dims x (HMC: 2 dtypes x (2 L x 2 + 1) + NUTS: 3 modes x (2 walks x 2 + 2))
    assert checks == 4 * (2 * (2 * 2 + 1) + 3 * (2 * 2 + 2))


def test_float64_restatement_of_dense_metric_hmc_in_unwhitened_momentum_on_the_twins_noise(tmp_path_factory, tmp_path):
    """Gaussian2D in f64, L = [[0.8, 0], [1.7, 0.6]] (the off-diagonal entry is the largest: with the products missing, or with
    L and L^T swapped in the kick, nothing below holds), 3 transitions of 4 chains with 5 leapfrog steps of 0.3.

    The restatement never forms a whitened momentum: p = L^-T z, kinetic energy 1/2 p^T M^-1 p with M^-1 = L L^T, drift by
    eps M^-1 p, kicks by eps / 2 grad, the two half-kicks of a step kept apart, numpy's own matrix products.  It equals the
    engine's z-form in exact arithmetic (z = L^T p).  Rounding: a leapfrog step of either form is at most 12 operations per
    coordinate on numbers of magnitude <= `mag` (measured below on the twin's own states and noise), each rounded to
    2^-53 relative; one step amplifies a perturbation of (x, p) by at most (1 + eps sqrt(|Sigma| |H|))^2 (|.| the spectral
    norm, H the target's precision), and a perturbation of x carries from one transition to the next.  Hence
        bound = (T * n_leapfrog) * 12 * 2^-53 * mag * (1 + eps sqrt(|Sigma| |H|))^(2 * n_leapfrog)  ~ 1e-11,
    absolute, against states of order 1; the accept decisions must be the same."""
    exe = DM.build_twin(tmp_path_factory)
    n, T, Lf, eps = 4, 3, 5, 0.3
    chol = np.array([[0.8, 0.0], [1.7, 0.6]])
    samples, state, accept, text = DM.twin_hmc(exe, tmp_path, np.float64, 2, n, T, 0, eps, Lf, 11, chol, print_noise=True)
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
    H = np.linalg.inv(np.array([[4.0, 2.0], [2.0, 3.0]]))
    logp = lambda x: -0.5 * (x - mean) @ H @ (x - mean)  # noqa: E731 -- the constant cancels in the accept ratio
    grad = lambda x: -H @ (x - mean)  # noqa: E731
    Minv = chol @ chol.T  # the mass matrix is M = (L L^T)^-1
    L_invT = np.linalg.inv(chol).T
    mag = max(np.abs(got_x).max(), np.abs(noise[:, :, :2]).max() * np.abs(L_invT).sum(), 1.0)
    bound = T * Lf * 12 * 2.0 ** -53 * mag * (1.0 + eps * np.sqrt(np.linalg.norm(Minv, 2) * np.linalg.norm(H, 2))) ** (2 * Lf)
    assert bound < 1e-10
    x = DM.start(n, 2)
    n_acc = 0
    for c in range(n):
        xc = x[c].copy()
        for t in range(T):
            p = L_invT @ noise[c, t, :2]
            h0 = -logp(xc) + 0.5 * p @ Minv @ p
            xn = xc.copy()
            for _ in range(Lf):
                p = p + 0.5 * eps * grad(xn)
                xn = xn + eps * (Minv @ p)
                p = p + 0.5 * eps * grad(xn)
            h1 = -logp(xn) + 0.5 * p @ Minv @ p
            acc = (h0 - h1) >= noise[c, t, 2]
            assert abs((h0 - h1) - noise[c, t, 2]) > 1e-9, "an accept decision within rounding of its threshold decides nothing"
            assert acc == bool(got_acc[c, t]), (c, t, h0 - h1, noise[c, t, 2])
            if acc:
                xc = xn
                n_acc += 1
            assert np.all(np.abs(xc - got_x[c, t]) <= bound), (c, t, xc, got_x[c, t], bound)
    assert 0 < n_acc  # trajectories that move
    # the factor matters: the same noise without the off-diagonal entry lands elsewhere
    other = DM.twin_hmc(exe, tmp_path, np.float64, 2, n, T, 0, eps, Lf, 11, np.diag(np.diag(chol)))[0]
    assert np.abs(other - samples).max() > 1e-3


def test_estimate_chol_against_numpy_float64():
    import torch

    from mini_mcmc_amd.warmup import estimate_chol

    rng = np.random.default_rng(5)
    mix = rng.normal(size=(5, 5))
    a = rng.normal(size=(7, 11, 5)) @ mix + np.array([3.0, -1.0, 50.0, 0.0, 2.0])
    flat = a.reshape(-1, 5)
    n = flat.shape[0]
    cov = np.cov(flat.T, bias=True)  # divisor N
    want_raw = np.linalg.cholesky(cov)
    want_reg = np.linalg.cholesky(n / (n + 5.0) * cov + 1e-3 * 5.0 / (n + 5.0) * np.eye(5))
    for sample in (a, torch.from_numpy(a), torch.from_numpy(a.astype(np.float32))):
        ref_raw, ref_reg = want_raw, want_reg
        if getattr(sample, "dtype", None) == torch.float32:
            c32 = np.cov(a.astype(np.float32).astype(np.float64).reshape(-1, 5).T, bias=True)
            ref_raw, ref_reg = np.linalg.cholesky(c32), np.linalg.cholesky(n / (n + 5.0) * c32 + 1e-3 * 5.0 / (n + 5.0) * np.eye(5))
        got_raw, got_reg = estimate_chol(sample, regularize=False), estimate_chol(sample)
        # float64 throughout; the two computations differ in summation order only: 77 draws of magnitude <= 60
        assert np.allclose(got_raw, ref_raw, rtol=1e-11, atol=1e-12) and np.allclose(got_reg, ref_reg, rtol=1e-11, atol=1e-12)
        assert got_reg.dtype == np.float64 and got_reg.shape == (5, 5) and np.all(np.triu(got_reg, 1) == 0) and np.all(np.diag(got_reg) > 0)
    # fewer draws than dimensions: singular without the shrinkage, a factor with it
    few = rng.normal(size=(2, 2, 5))
    with pytest.raises(ValueError):
        estimate_chol(few, regularize=False)
    f = estimate_chol(few)
    assert np.all(np.isfinite(f)) and np.all(np.diag(f) > 0)
    assert np.allclose(f @ f.T, 4 / 9.0 * np.cov(few.reshape(-1, 5).T, bias=True) + 1e-3 * 5.0 / 9.0 * np.eye(5), rtol=1e-10, atol=1e-14)
    with pytest.raises(ValueError):
        estimate_chol(flat)


def test_chunked_torch_reduction_is_the_unchunked_one(monkeypatch):
    import torch

    from mini_mcmc_amd import warmup

    a = torch.from_numpy(np.random.default_rng(6).normal(size=(7, 11, 5)).astype(np.float32))
    whole = warmup.estimate_chol(a)
    monkeypatch.setattr(warmup, "_CHUNK", 10)  # 77 rows: seven full chunks and a tail
    assert np.allclose(warmup.estimate_chol(a), whole, rtol=1e-12, atol=1e-14)


def test_dense_metric_entry_points_reject_a_null_handle_and_are_declared_in_every_binding():
    from mini_mcmc_amd import _lib as L

    lib = L.lib()
    s = (C.c_double * 9)(1.0, 0.0, 0.0, 0.5, 1.0, 0.0, 0.25, 0.5, 1.0)
    names = ("mmcmc_hmc_set_metric_dense", "mmcmc_hmc_metric_dense", "mmcmc_nuts_set_metric_dense", "mmcmc_nuts_metric_dense")
    for name in names:
        assert getattr(lib, name)(None, s) == L.ERR_INVALID_ARG, name
        assert getattr(lib, name)(None, None) == L.ERR_INVALID_ARG, name
        assert name in L.SIGNATURES
    assert lib.mmcmc_version() == 102
    read = lambda *p: open(os.path.join(DM.ROOT, *p)).read()  # noqa: E731
    hpp, sys_rs, safe_rs = read("include", "mmcmc.hpp"), read("rust", "mini-mcmc-hip-sys", "src", "lib.rs"), read("rust", "mini-mcmc-hip", "src", "lib.rs")
    for name in names:
        assert name in read("include", "mmcmc.h") and name in hpp and f"pub fn {name}(" in sys_rs and f"sys::{name}(" in safe_rs, name
