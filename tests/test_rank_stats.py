"""Rank-normalised split R-hat, bulk / tail ESS and quantiles (include/mmcmc.h "rank-normalised diagnostics",
csrc/mm_rank.hip) against the float64 yardstick of tests/rank_f64.py.

What is exact is compared exactly: rank2 = 2 x the tie-averaged rank is an integer, element for element.  What is not:
  * scores: z is one f32 rounding (2^-24) of an f64 inverse normal CDF, with a factor two for the f64 routine's own error:
    |z - ndtri(u)| <= 2^-23 |ndtri(u)|;
  * quantiles: between the bracketing order statistics a <= q <= b, and |q - np.quantile| <= 2^-22 (b - a) + 4 x 2^-52 max(|a|, |b|)
    (the first term: the worst absolute error of h = (S - 1) p at S < 2^31);
  * R-hat 1e-4 and ESS oracle.stats_f64.ess_rtol with the lag-sum bound of the kernel path in use: the project's own tolerances
    (tests/test_stats_f64.py), on the yardstick's transformed arrays rounded to f32.  Geyer's truncation is a discontinuity, so
    every compared parameter must have all the pair sums the loop looks at further from zero than the f32 finish can move them
    (rank_f64.geyer_margin > 1): asserted, never skipped.
"""
import ctypes as C

import numpy as np
import pytest

import rank_f64 as R
from oracle import stats_f64 as F
from test_stats_f64 import _close, _lag_tol

EPS = F.EPS32


def _ar1(rng, c, n, d, phi=0.6):
    from scipy.signal import lfilter

    return lfilter([1.0], [1.0, -phi], rng.standard_normal((c, n, d)), axis=1).astype(np.float32)


def _scale_shifted(c, n):
    """the issue's input: c chains x n standard-normal draws, the last half of the chains multiplied by 2 (same location)"""
    x = np.random.default_rng(1).standard_normal((c, n, 1)).astype(np.float32)
    x[c // 2:] *= 2.0
    return x


# ---------------------------------------------------------------- CPU: the yardstick itself, statuses


def test_yardstick_ranks_by_hand():
    x = np.array([3.0, 1.0, 1.0, 2.0], dtype=np.float32).reshape(1, 4, 1)
    assert R.rank2(x).ravel().tolist() == [8, 3, 3, 6]
    # -0.0 and +0.0 tie; +-inf sort like numbers
    y = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45], dtype=np.float32).reshape(2, 3, 1)
    assert R.rank2(y).ravel().tolist() == [7, 7, 12, 2, 10, 4]
    # a NaN anywhere: the whole parameter is rank 0 / NaN, the other parameter untouched
    z = np.stack([np.array([1.0, np.nan, 3.0, 2.0]), np.array([4.0, 3.0, 2.0, 1.0])], axis=1).astype(np.float32).reshape(2, 2, 2)
    r2 = R.rank2(z)
    assert r2[:, :, 0].ravel().tolist() == [0, 0, 0, 0] and r2[:, :, 1].ravel().tolist() == [8, 6, 4, 2]
    s = R.scores_from_rank2(r2)
    assert np.isnan(s[:, :, 0]).all() and not np.isnan(s[:, :, 1]).any()
    # Blom scores of four distinct values: Phi^-1((k - 3/8) / 4.25), antisymmetric
    s4 = R.normal_scores(np.array([10.0, 20.0, 30.0, 40.0], dtype=np.float32).reshape(2, 2, 1)).ravel()
    from scipy.special import ndtri

    np.testing.assert_allclose(s4, ndtri((np.arange(1, 5) - 0.375) / 4.25), rtol=1e-15)
    np.testing.assert_allclose(s4, -s4[::-1], rtol=1e-14)
    # folded: |x - median| of 1..5 around 3 -> 2 1 0 1 2
    f = R.fold(np.arange(1.0, 6.0, dtype=np.float32).reshape(1, 5, 1)).ravel()
    assert f.tolist() == [2.0, 1.0, 0.0, 1.0, 2.0]
    assert R.rank2(np.arange(1.0, 6.0, dtype=np.float32).reshape(1, 5, 1), folded=True).ravel().tolist() == [9, 5, 2, 5, 9]
    # type-7 quantiles and their brackets
    q = R.quantiles(np.array([1.0, 2.0, 3.0, 10.0], dtype=np.float32).reshape(2, 2, 1), (0.0, 0.5, 0.9, 1.0))
    np.testing.assert_allclose(q.ravel(), [1.0, 2.5, 7.9, 10.0], rtol=1e-15)
    a, b = R.brackets(np.array([1.0, 2.0, 3.0, 10.0], dtype=np.float32).reshape(2, 2, 1), (0.0, 0.5, 0.9, 1.0))
    assert a.ravel().tolist() == [1.0, 2.0, 3.0, 10.0] and b.ravel().tolist() == [2.0, 3.0, 10.0, 10.0]


def test_yardstick_sees_a_scale_difference_the_mean_rhat_cannot():
    """8 chains x 1000 N(0, 1) draws, the last four times 2: same location, other scale.  Mean-based split R-hat 1.0006, bulk
    1.0006, folded 1.078 (float64): the conventional 1.01 threshold separates them with a wide margin."""
    x = _scale_shifted(8, 1000)
    y = R.diagnostics(x)
    mean_rhat = 1.0 / F.diagnostics(x).rhat[0]
    assert mean_rhat < 1.005 and y.rhat_bulk[0] < 1.005
    assert y.rhat_folded[0] > 1.05 and y.rhat[0] == y.rhat_folded[0]
    assert 0 < y.ess_tail[0] and 0 < y.ess_bulk[0]


def _call_normalize(lib, x, c, n, d, z=True):
    zbuf = np.empty(64, dtype=np.float32)  # only ever written by the one valid call below, [2, 4, 1]
    return lib.mmcmc_rank_normalize(x.ctypes.data if x is not None else None, 0, 0, c, n, d, 0,
                                    zbuf.ctypes.data if z else None, 0, None, 0, None)


def test_new_entry_points_statuses_without_a_device():
    import torch

    import mini_mcmc_amd
    from mini_mcmc_amd import MmcmcError
    from mini_mcmc_amd import stats as S

    lib = mini_mcmc_amd.lib()
    x = np.zeros((2, 4, 1), dtype=np.float32)
    dp = C.POINTER(C.c_double)
    probs = np.array([0.5], dtype=np.float64)
    out = np.empty(1, dtype=np.float64)
    # arguments and shapes are judged before the device is looked for, and before anything is allocated
    assert _call_normalize(lib, None, 2, 4, 1) == -1
    assert _call_normalize(lib, x, 2, 4, 1, z=False) == -1
    assert _call_normalize(lib, x, 0, 4, 1) == -1
    assert lib.mmcmc_rank_normalize(x.ctypes.data, 0, 7, 2, 4, 1, 0, x.ctypes.data, 0, None, 0, None) == -1  # dtype
    assert _call_normalize(lib, x, 1 << 16, 1 << 15, 1) == -3  # S = 2^31
    assert _call_normalize(lib, x, 1, 1 << 31, 1) == -3
    assert _call_normalize(lib, x, 1 << 40, 1 << 40, 1) == -3  # a product that wraps in 64 bits
    assert _call_normalize(lib, x, 2, 4, 1 << 16) == -3
    q = lib.mmcmc_quantiles
    assert q(None, 0, 0, 2, 4, 1, probs.ctypes.data_as(dp), 1, out.ctypes.data_as(dp), 0, None) == -1
    assert q(x.ctypes.data, 0, 0, 2, 4, 1, None, 1, out.ctypes.data_as(dp), 0, None) == -1
    for bad in (-0.01, 1.01, float("nan")):
        p = np.array([0.5, bad], dtype=np.float64)
        assert q(x.ctypes.data, 0, 0, 2, 4, 1, p.ctypes.data_as(dp), 2, out.ctypes.data_as(dp), 0, None) == -1
    assert q(x.ctypes.data, 0, 0, 1 << 16, 1 << 15, 1, probs.ctypes.data_as(dp), 1, out.ctypes.data_as(dp), 0, None) == -3
    rd = lib.mmcmc_rank_diagnostics
    nul = [None] * 5
    assert rd(None, 0, 0, 2, 4, 1, *nul, None, 0, None, 0, None) == -1
    assert rd(x.ctypes.data, 0, 0, 2, 4, 1, *nul, None, 1, out.ctypes.data_as(dp), 0, None) == -1
    p = np.array([2.0], dtype=np.float64)
    assert rd(x.ctypes.data, 0, 0, 2, 4, 1, *nul, p.ctypes.data_as(dp), 1, out.ctypes.data_as(dp), 0, None) == -1
    assert rd(x.ctypes.data, 0, 0, 8, 1, 1, *nul, None, 0, None, 0, None) == -3  # n < 2
    assert rd(x.ctypes.data, 0, 0, 1 << 16, 1 << 15, 1, *nul, None, 0, None, 0, None) == -3
    # a shape limit of mmcmc_split_rhat_mean_ess: the residue transform's bins (dim x 2048 x ceil(n/2 / 1024) < 2^32)
    assert rd(x.ctypes.data, 0, 0, 1, 1 << 17, 40000, *nul, None, 0, None, 0, None) == -3
    if torch.cuda.is_available():
        return
    assert _call_normalize(lib, x, 2, 4, 1) == -4
    assert q(x.ctypes.data, 0, 0, 2, 4, 1, probs.ctypes.data_as(dp), 1, out.ctypes.data_as(dp), 0, None) == -4
    assert rd(x.ctypes.data, 0, 0, 2, 4, 1, *nul, None, 0, None, 0, None) == -4
    for call in (lambda: S.rank_normalize(x), lambda: S.quantiles(x, [0.5]), lambda: S.rank_diagnostics(x), lambda: S.summary(x)):
        with pytest.raises(MmcmcError) as e:
            call()
        assert e.value.status == -4


def test_facade_compiles_with_the_rank_wrappers(tmp_path):
    """include/mmcmc.hpp's rank_normalize / quantiles / rank_diagnostics instantiate against the header (syntax only)"""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "rank.cpp"
    src.write_text('#include "mmcmc.hpp"\n'
                   "int main() {\n"
                   "    std::vector<float> s(8);\n"
                   "    std::vector<uint32_t> r2;\n"
                   "    auto z = mmcmc::rank_normalize(s, 2, 4, 1, true, &r2);\n"
                   "    auto q = mmcmc::quantiles(s, 2, 4, 1, {0.5});\n"
                   "    auto d = mmcmc::rank_diagnostics(s, 2, 4, 1);\n"
                   "    return (int)(z.size() + q.size() + d.rhat.size());\n"
                   "}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(root, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---------------------------------------------------------------- GPU


def _specials(rng, c, n, d):
    """-0.0 / +0.0, +-inf, denormals, a few ordinary values: many ties, every corner of the key map"""
    pool = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754944e-38, -1.1754944e-38, 1.0, -1.0,
                     3.4028235e38, -3.4028235e38, 0.5, 2.0], dtype=np.float32)
    return pool[rng.integers(0, pool.size, size=(c, n, d))]


def _mh_sample(c, n):
    from mini_mcmc_amd.core import init_with_seed
    from mini_mcmc_amd.distributions import Gaussian2D, IsotropicGaussian
    from mini_mcmc_amd.metropolis_hastings import MetropolisHastings

    init = init_with_seed(c, 2, 42, np.float32)
    mh = MetropolisHastings(Gaussian2D([0.0, 1.0], [[4.0, 2.0], [2.0, 3.0]]), IsotropicGaussian(1.0), init).seed(42)
    return mh.run(n, 10)


def _rank_input(kind, c, n, d):
    rng = np.random.default_rng(c * 1000003 + n * 101 + d)
    if kind == "normal":
        return rng.standard_normal((c, n, d)).astype(np.float32)
    if kind == "mh":
        assert d == 2
        return _mh_sample(c, n)
    if kind == "stuck":  # every chain at its own constant, two chains at the same one
        v = (0.25 * (np.arange(c) % max(c - 1, 1))).astype(np.float32)
        return np.broadcast_to(v[:, None, None], (c, n, d)).copy()
    if kind == "specials":
        return _specials(rng, c, n, d)
    if kind == "two":
        return np.where(rng.random((c, n, d)) < 0.3, np.float32(-1.5), np.float32(2.5)).astype(np.float32)
    if kind == "f64":  # ranked by its f32 casts: neighbours in f64 that collapse in f32 must tie
        base = rng.standard_normal((c, n, d))
        return base + 1e-12 * rng.standard_normal((c, n, d))
    raise ValueError(kind)


def _rel(err, ref):
    """max err / |ref| over the elements with ref != 0 (a middle rank scores exactly 0)"""
    ok = ref != 0
    return float(np.max(err[ok] / np.abs(ref[ok]), initial=0.0))


# S is a multiple of no block size in most of them (4096-key sort tiles, 2048-key tie tiles, 256 threads, 64 lanes)
RANK_CASES = [("normal", 2, 4, 1), ("specials", 2, 4, 1), ("normal", 1, 1, 3), ("two", 3, 5, 7), ("normal", 3, 21, 3),
              ("specials", 5, 67, 7), ("stuck", 7, 33, 1), ("normal", 4, 1024, 1), ("normal", 5, 4099, 3),
              ("specials", 3, 1367, 7), ("two", 9, 2731, 1), ("stuck", 6, 701, 3), ("mh", 64, 257, 2), ("mh", 1000, 101, 2),
              ("f64", 11, 1001, 3), ("normal", 33, 6007, 7), ("two", 2, 300001, 1), ("stuck", 3, 100003, 1),
              ("normal", 1, 1048577, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,c,n,d", RANK_CASES)
def test_ranks_exact_and_scores(kind, c, n, d):
    """rank2 == 2 x scipy's average rank, element for element, plain and folded; the scores within 2^-23 relative of
    float64 ndtri; host arrays and device tensors give the same bits."""
    import torch

    from mini_mcmc_amd import stats as S

    x = _rank_input(kind, c, n, d)
    for folded in (False, True):
        ref = R.rank2(x, folded)
        z, r2 = S.rank_normalize(x, folded=folded, return_ranks=True)
        assert r2.dtype == np.uint32 and z.dtype == np.float32 and z.shape == x.shape
        bad = np.flatnonzero(r2.astype(np.int64).ravel() != ref.ravel())
        assert bad.size == 0, (kind, folded, bad[:8], r2.ravel()[bad[:8]], ref.ravel()[bad[:8]])
        z64 = R.scores_from_rank2(ref)
        err = np.abs(z.astype(np.float64) - z64)
        print(f"{kind} [{c}, {n}, {d}] folded={folded}: max |z - ndtri| / |ndtri| = {_rel(err, z64) * 2**24:.3f} x 2^-24")
        assert np.all(err <= 2.0**-23 * np.abs(z64))
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    zd, rd = S.rank_normalize(t, return_ranks=True)
    assert zd.is_cuda and np.array_equal(zd.cpu().numpy().view(np.uint32), S.rank_normalize(x).view(np.uint32))
    assert np.array_equal(rd.cpu().numpy(), R.rank2(x))


@pytest.mark.gpu
def test_nan_parameter_is_nan_by_position():
    from mini_mcmc_amd import stats as S

    rng = np.random.default_rng(3)
    x = rng.standard_normal((5, 333, 4)).astype(np.float32)
    x[3, 17, 2] = np.nan
    x[0, 0, 0] = np.inf
    for folded in (False, True):
        z, r2 = S.rank_normalize(x, folded=folded, return_ranks=True)
        assert np.isnan(z[:, :, 2]).all() and (r2[:, :, 2] == 0).all()
        assert not np.isnan(z[:, :, [0, 1, 3]]).any()
        assert np.array_equal(r2.astype(np.int64), R.rank2(x, folded))
    q = S.quantiles(x, [0.0, 0.3, 1.0])
    assert np.isnan(q[:, 2]).all() and not np.isnan(q[:, [1, 3]]).any() and q[2, 0] == np.inf
    d = S.rank_diagnostics(x)
    for v in (d.rhat, d.rhat_bulk, d.rhat_folded, d.ess_bulk, d.ess_tail, d.ess_tail_lower, d.ess_tail_upper):
        assert np.isnan(v[2]) and not np.isnan(v[[1, 3]]).any()
    assert np.isnan(d.quantiles[:, 2]).all()


@pytest.mark.gpu
def test_config3_shape_ranks_exact_and_reproducible():
    """[65 536, 400, 3]: S = 26 214 400 > 2^24 keys per parameter, where an index stops being exact in f32.  The same input
    sorted twice, and on two streams: z bit-identical."""
    import torch

    from mini_mcmc_amd import stats as S
    from mini_mcmc_amd.core import init_with_seed
    from mini_mcmc_amd.distributions import RosenbrockND
    from mini_mcmc_amd.hmc import HMC

    c, n = 65536, 400
    hmc = HMC(RosenbrockND(3), init_with_seed(c, 3, 42, np.float32), 0.032, 10).set_seed(42)
    t = hmc.run(n, 50, to="torch")
    z1, r2 = S.rank_normalize(t, return_ranks=True)
    z2 = S.rank_normalize(t)
    assert torch.equal(z1.view(torch.int32), z2.view(torch.int32))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        za = S.rank_normalize(t)
    with torch.cuda.stream(s2):
        zb = S.rank_normalize(t, folded=True)
        zc = S.rank_normalize(t)
    torch.cuda.synchronize()
    assert torch.equal(za.view(torch.int32), z1.view(torch.int32)) and torch.equal(zc.view(torch.int32), z1.view(torch.int32))
    x = t.cpu().numpy()
    ref = R.rank2(x)
    assert np.array_equal(r2.cpu().numpy(), ref)
    z64 = R.scores_from_rank2(ref)
    err = np.abs(z1.cpu().numpy().astype(np.float64) - z64)
    print(f"config 3: max |z - ndtri| / |ndtri| = {_rel(err, z64) * 2**24:.3f} x 2^-24")
    assert np.all(err <= 2.0**-23 * np.abs(z64))
    assert np.array_equal(S.rank_normalize(t, folded=True, return_ranks=True)[1].cpu().numpy(), R.rank2(x, folded=True))
    assert torch.equal(zb.view(torch.int32), S.rank_normalize(t, folded=True).view(torch.int32))
    # fixed-(eps, L) HMC on the Rosenbrock density mixes worst in the tail
    d = S.rank_diagnostics(t)
    print("config 3 run(400, 50): rhat", d.rhat, "ess_bulk", d.ess_bulk, "ess_tail", d.ess_tail)
    assert np.all(d.ess_tail < d.ess_bulk)


QUANTILE_PROBS = (0.0, 1.0, 0.5, 0.05, 0.95, 0.25, 1.0 / 3.0, 0.999999, 1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,c,n,d", [("normal", 2, 4, 1), ("normal", 1, 1, 3), ("two", 3, 5, 7), ("mh", 64, 257, 2),
                                        ("stuck", 6, 701, 3), ("normal", 5, 4099, 3), ("f64", 11, 1001, 3),
                                        ("two", 2, 300001, 1), ("normal", 33, 6007, 7)])
def test_quantiles(kind, c, n, d):
    from mini_mcmc_amd import stats as S

    x = _rank_input(kind, c, n, d)
    q = S.quantiles(x, QUANTILE_PROBS)
    ref = R.quantiles(x, QUANTILE_PROBS)
    a, b = R.brackets(x, QUANTILE_PROBS)
    assert q.shape == ref.shape and q.dtype == np.float64
    assert np.all((a <= q) & (q <= b)), (q, a, b)
    bound = 2.0**-22 * (b - a) + 4 * 2.0**-52 * np.maximum(np.abs(a), np.abs(b))
    print(f"{kind} [{c}, {n}, {d}]: max |q - np.quantile| / bound = {np.max(np.abs(q - ref) / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(np.abs(q - ref) <= bound), (q - ref, bound)
    assert np.array_equal(q[0], a[0]) and np.array_equal(q[1], b[1])  # p = 0, 1: the extremes themselves
    assert np.array_equal(S.rank_diagnostics(x, QUANTILE_PROBS).quantiles, q) if n >= 2 else True


def _diag_input(kind, c, n):
    rng = np.random.default_rng(n * 31 + c)
    if kind == "ar1":
        x = np.concatenate([_ar1(rng, c, n, 2, 0.6), _ar1(rng, c, n, 1, 0.9)], axis=2)
        x[:, :, 1] += (0.2 * np.arange(c))[:, None]
        return x
    if kind == "trend":
        t = np.arange(n, dtype=np.float64)
        return (3.0 * t[None, :, None] / n * (1.0 + 0.1 * np.arange(c))[:, None, None]
                + rng.standard_normal((c, n, 2))).astype(np.float32)
    if kind == "mh":
        return _mh_sample(c, n)
    raise ValueError(kind)


def _check_against_yardstick(x, d, label):
    """item 4 of the issue: every part against oracle.stats_f64 on the yardstick's transformed arrays; returns the yardstick"""
    y = R.diagnostics(x)
    m = x.shape[1] // 2
    lag_tol = _lag_tol("auto", m, 2 * x.shape[0])
    for name, r in (("bulk", y.bulk), ("folded", y.folded), ("lower", y.lower), ("upper", y.upper)):
        margin = R.geyer_margin(r, lag_tol)
        assert np.all(margin > 1.0), (label, name, margin)  # zero parameters skipped: none is near the truncation's jump
    _close(d.rhat_bulk, y.rhat_bulk, 1e-4, f"{label} rhat_bulk")
    _close(d.rhat_folded, y.rhat_folded, 1e-4, f"{label} rhat_folded")
    _close(d.rhat, y.rhat, 1e-4, f"{label} rhat")
    eb = _close(d.ess_bulk, y.ess_bulk, F.ess_rtol(y.bulk, lag_tol), f"{label} ess_bulk")
    el = _close(d.ess_tail_lower, y.ess_tail_lower, F.ess_rtol(y.lower, lag_tol), f"{label} ess_tail_lower")
    eu = _close(d.ess_tail_upper, y.ess_tail_upper, F.ess_rtol(y.upper, lag_tol), f"{label} ess_tail_upper")
    assert np.array_equal(d.ess_tail, np.minimum(d.ess_tail_lower, d.ess_tail_upper))
    assert np.array_equal(d.rhat, np.maximum(d.rhat_bulk, d.rhat_folded))
    print(f"{label}: ESS error / bound bulk {eb:.3f} lower {el:.3f} upper {eu:.3f}")
    return y


# half-chains on both sides of the reference's n <= 100 switch from direct sums to the power spectrum
@pytest.mark.gpu
@pytest.mark.parametrize("kind,c,n", [("ar1", 4, 60), ("ar1", 16, 200), ("ar1", 7, 201), ("ar1", 5, 2600), ("trend", 6, 120),
                                      ("trend", 3, 1001), ("mh", 64, 150), ("mh", 32, 1200)])
def test_rank_diagnostics_against_f64(kind, c, n):
    import torch

    from mini_mcmc_amd import stats as S

    x = _diag_input(kind, c, n)
    d = S.rank_diagnostics(x)
    _check_against_yardstick(x, d, f"{kind} [{c}, {n}]")
    dd = S.rank_diagnostics(torch.from_numpy(x).cuda())
    for a, b in ((d.rhat, dd.rhat), (d.ess_bulk, dd.ess_bulk), (d.ess_tail, dd.ess_tail), (d.quantiles, dd.quantiles)):
        assert np.array_equal(a, b)
    s = S.summary(x, names=[f"p{j}" for j in range(x.shape[2])])
    h = F.splitcat(x)
    np.testing.assert_allclose(s.mean, h.mean(axis=(0, 1)), rtol=0, atol=1e-5 * np.abs(h).max())
    np.testing.assert_allclose(s.sd, h.reshape(-1, x.shape[2]).std(axis=0, ddof=1), rtol=1e-4)
    _, ess_mean = S.split_rhat_mean_ess(x)
    np.testing.assert_allclose(s.mcse_mean, s.sd / np.sqrt(ess_mean.astype(np.float64)), rtol=1e-12)
    assert np.array_equal(s.q50, d.quantiles[1]) and np.array_equal(s.rhat, d.rhat) and np.array_equal(s.ess_tail, d.ess_tail)
    assert str(s).splitlines()[0].split() == ["mean", "sd", "mcse_mean", "q5", "q50", "q95", "rhat", "ess_bulk", "ess_tail"]
    assert len(str(s).splitlines()) == 1 + x.shape[2] and str(s).splitlines()[1].startswith("p0")


@pytest.mark.gpu
def test_sees_what_the_mean_rhat_cannot():
    """same location, different scale: the conventional 1.01 threshold passes the mean-based split R-hat and fails the
    rank-normalised one, through its folded part -- at 8 chains against the yardstick, and at 65 536 chains"""
    import torch

    from mini_mcmc_amd import stats as S

    x = _scale_shifted(8, 1000)
    d = S.rank_diagnostics(x)
    assert S.standard_split_rhat(x)[0] < 1.01
    assert d.rhat[0] > 1.01 and d.rhat[0] == d.rhat_folded[0] and d.rhat_bulk[0] < 1.01
    _check_against_yardstick(x, d, "scale-shifted [8, 1000]")
    g = torch.Generator(device="cuda").manual_seed(1)
    t = torch.randn((65536, 400, 1), generator=g, device="cuda", dtype=torch.float32)
    t[32768:] *= 2.0
    big = S.rank_diagnostics(t)
    print("65 536 chains: mean-based", S.standard_split_rhat(t), "bulk", big.rhat_bulk, "folded", big.rhat_folded)
    assert S.standard_split_rhat(t)[0] < 1.01
    assert big.rhat[0] > 1.01 and big.rhat[0] == big.rhat_folded[0] and big.rhat_bulk[0] < 1.01


@pytest.mark.gpu
def test_existing_diagnostics_unchanged_by_a_rank_call():
    import torch

    from mini_mcmc_amd import stats as S

    x = torch.from_numpy(_diag_input("ar1", 16, 200)).cuda()
    r0, e0 = S.split_rhat_mean_ess(x)
    S.rank_diagnostics(x)
    r1, e1 = S.split_rhat_mean_ess(x)
    S.rank_normalize(x, folded=True)
    r2, e2 = S.split_rhat_mean_ess(x)
    for a, b in ((r0, r1), (e0, e1), (r0, r2), (e0, e2)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
