"""Split R-hat / ESS against a float64 restatement of stats.rs:396-546 (oracle/stats_f64.py).

oracle/stats.c does the reference's f32 arithmetic, so it only pins a kernel to f32 tolerance, and R-hat / ESS read the lag sums
only until Geyer's paired sum turns non-positive (lag 10-22 for AR(1) with phi = 0.6).  Here every output of `stats_partials`
-- means, centred sums of squares and the lag sum at EVERY lag -- is compared with float64 values, on every kernel path, with
inputs whose ESS reads their late lags (a random walk, a trend, phi = 0.999), and the degenerate inputs whose answers are
exact (stuck chains) are asserted, NaN by position.

Error model (f32, unit roundoff eps = 2^-24; every bound relative to the float64 lag-0 sum a64[0] of the same parameter):
  * transform paths (a zero-padded N-point f32 FFT of each half-chain, power spectra summed, one inverse): each of the
    log2(N) radix passes of the forward transform, the squaring and the inverse adds ~eps of the spectrum's largest bins,
    whose inverse is a64[0]: |a[k] - a64[k]| <= 4 eps log2(N) a64[0] -- 2.6e-6 at N = 2048, 4.3e-6 at N = 2^18;
  * direct-sum paths (tile1, tile, mfma, direct, any-length): f32 running sums of at most m products per half-chain plus the
    sum over c2 half-chains; each product and partial sum is bounded by a64[0] (Cauchy-Schwarz), and with rounding errors of
    either sign the total is 4 eps sqrt(m + c2) a64[0] at four standard deviations;
  * means: an f32 sum of m draws, 4 eps sqrt(m) max|x| (+ 2 eps |mean| for the division); centred sums of squares:
    (4 sqrt(m) + 3) eps ssq64 plus m times the mean's error squared;
  * R-hat 1e-4; ESS 1e-3 plus what the lag-sum error and the finish's f32 Geyer sum can move tau by (oracle.stats_f64.ess_rtol:
    about (pairs summed) x (lag-sum error + 4 eps) of rho each).
"""
import numpy as np
import pytest

from oracle import stats_f64 as F

EPS = F.EPS32
SIGNALS = ("ar06", "walk", "trend", "ar0999", "alt", "tone", "offset")


def _deep(kind, m):
    """inputs whose ESS reads lags beyond m / 2 (asserted wherever they are used as such): the trend up to m = 32 768, the
    slow tone and phi = 0.999 up to 8192.  Beyond, Geyer's sum ends before m / 2 (phi = 0.999) or the f32 finish's own error
    over 10^5 pairs (pairs x eps) outweighs what the late lags move; the lag sums themselves are compared at every lag there."""
    return (kind == "trend" and m <= 32768) or (kind in ("tone", "ar0999") and m <= 8192)


def _signal(kind, rng, c, n):
    """[c, n] float64 test signal with unit-scale innovations."""
    from scipy.signal import lfilter

    t = np.arange(n, dtype=np.float64)
    e = rng.standard_normal((c, n))
    if kind == "ar06":
        return lfilter([1.0], [1.0, -0.6], e, axis=1)
    if kind == "ar0999":
        return lfilter([1.0], [1.0, -0.999], e, axis=1) * 0.05
    if kind == "walk":
        return np.cumsum(e, axis=1)
    if kind == "trend":
        return 10.0 * t / max(n, 1) * (1.0 + 0.1 * np.arange(c))[:, None] + e
    if kind == "alt":
        return np.broadcast_to(np.where(t % 2 == 0, 1.0, -1.0), (c, n)).copy()
    if kind == "tone":
        # bin 1 of the shortest power-of-two transform longer than 2 m: rho ~ cos(2 pi k / L), positive beyond lag m / 2
        L = 1
        while L <= 2 * max(n // 2, 1):
            L <<= 1
        return np.cos(2.0 * np.pi * t / L + rng.uniform(0, 2 * np.pi, (c, 1))) + 0.01 * e
    if kind == "offset":
        return lfilter([1.0], [1.0, -0.6], e, axis=1) + 100.0
    raise ValueError(kind)


def _sample(rng, c, n, kinds, dtype=np.float32):
    return np.stack([_signal(k, rng, c, n) for k in kinds], axis=2).astype(dtype)


def _stuck(c, n):
    """chain i stuck at the dyadic constant 0.25 (i + 1): R-hat 0, ESS = c2 m / (4 floor(m / 2) - 1)"""
    return np.broadcast_to((0.25 * np.arange(1, c + 1))[:, None], (c, n)).astype(np.float32)


def _common(c, n):
    """one dyadic constant in every chain: 0 / 0 in the reference -> NaN (exact means need m a power of two)"""
    return np.full((c, n), 0.75, dtype=np.float32)


def _stuck_ess(c, m):
    return 2 * c * m / (4 * (m // 2) - 1)


def _close(got, ref, rtol, what):
    """elementwise |got - ref| <= rtol |ref| with NaN only where ref is NaN"""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    rtol = np.broadcast_to(np.asarray(rtol, dtype=np.float64), ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, got, ref)
    ok = ~np.isnan(ref)
    err = np.abs(got[ok] - ref[ok])
    assert np.all(err <= rtol[ok] * np.abs(ref[ok])), (what, got, ref, err / np.abs(ref[ok]), rtol)
    return float(np.max(err / np.maximum(rtol[ok] * np.abs(ref[ok]), 1e-300), initial=0.0))


# ---------------------------------------------------------------- the restatement itself (CPU)


def test_autocov_known_answers_and_ess_1(O, kats):
    # stats.rs:777-808: the reference's autocov of one 4-point series (lag sums / n)
    for ka in kats["autocov"]:
        d = np.array(ka["data"], dtype=np.float64)
        got = F.lag_sums(d[None]) / d.shape[0]
        np.testing.assert_allclose(got, np.array(ka["expected"]), atol=ka["atol"])
    # stats.rs:810-834 ess_1
    k = kats["ess_1"]
    r = O.SmallRng(k["seed"])
    data = np.array([[r.f32() for _ in range(k["n"])] for _ in range(k["chains"])], dtype=np.float32)[:, :, None]
    rhat, ess = F.split_rhat_mean_ess(data)
    assert ess.min() > k["ess_min_gt"] and rhat.max() < k["rhat_max_lt"]


@pytest.mark.parametrize("m", [2, 3, 63, 64, 65, 100, 101, 1000])
def test_fft_lag_sums_equal_direct_sums(m):
    rng = np.random.default_rng(m)
    h = rng.standard_normal((3, m, 2)) + 5.0
    y = h - h.mean(axis=1, keepdims=True)
    direct = np.stack([(y[:, :m - k] * y[:, k:]).sum(axis=(0, 1)) for k in range(m)])
    np.testing.assert_allclose(F.lag_sums(h), direct, rtol=0, atol=1e-12 * direct[0].max())


@pytest.mark.parametrize("c,n,kinds", [(4, 60, ("ar06", "offset")), (3, 201, ("walk", "ar06", "tone")),
                                       (5, 2600, ("walk", "trend", "ar0999")), (2, 6001, ("ar06", "walk")),
                                       (8, 1001, ("alt", "ar06", "trend"))])
def test_agrees_with_the_f32_oracle(O, c, n, kinds):
    """oracle/stats.c (the reference's f32 arithmetic, f32 FFT above 100 draws) against float64: R-hat to 1e-4, ESS within
    the f32 model of an L-point transform (lag sums to 4 eps log2(L) of lag 0), with Geyer's sum running deep."""
    x = _sample(np.random.default_rng(c * n), c, n, kinds)
    r = F.diagnostics(x)
    r0, e0 = O.split_rhat_mean_ess(x)
    L = 1
    while L < 2 * r.m:
        L <<= 1
    _close(r0, r.rhat, 1e-4, "rhat")
    _close(e0, r.ess, F.ess_rtol(r, 4 * EPS * np.log2(L)), "ess")
    if any(_deep(k, r.m) for k in kinds):
        assert r.pairs.max() >= 20  # deep: more than the first few lags decide the ESS


@pytest.mark.parametrize("c,n", [(2, 2), (3, 3), (2, 8), (5, 201), (3, 4097), (2, 20000)])
def test_closed_forms(O, c, n):
    m = n // 2
    x = np.stack([_stuck(c, n), _signal("ar06", np.random.default_rng(n), c, n).astype(np.float32)], axis=2)
    rhat, ess = F.split_rhat_mean_ess(x)
    assert rhat[0] == 0.0
    if m >= 2:
        assert ess[0] == pytest.approx(_stuck_ess(c, m), rel=1e-14)
    else:  # m = 1: no pair to add, tau = -1
        assert ess[0] == -2 * c
    # one constant in every chain: 0 / 0
    y = _common(c, 2 * m if m & (m - 1) == 0 else n)[:, :, None]
    rh, es = F.split_rhat_mean_ess(y)
    assert np.isnan(rh[0]) and (np.isnan(es[0]) if m >= 2 else es[0] == -2 * c)  # m = 1 reads no rho
    r0, e0 = O.split_rhat_mean_ess(x)
    assert r0[0] == 0.0 and e0[0] == pytest.approx(ess[0], rel=1e-6)


def _deep_case(kind, c, n, seed=0):
    x = _sample(np.random.default_rng(seed), c, n, (kind,))
    return x, F.diagnostics(x)


@pytest.mark.parametrize("kind,c,n", [("walk", 4, 200), ("walk", 2, 6000), ("walk", 1, 300000), ("trend", 3, 4096),
                                      ("trend", 2, 60000), ("tone", 2, 16001), ("tone", 5, 1025), ("ar0999", 2, 4000)])
def test_deep_inputs_read_their_late_lags(kind, c, n):
    """the inputs the GPU tests call deep: scaling the float64 lag sums from m / 2 up by 1.5 moves the ESS by far more than
    its tolerance -- so an error at late lags cannot pass unseen"""
    _, r = _deep_case(kind, c, n)
    s = F.late_lag_sensitivity(r)
    tol = F.ess_rtol(r, 4 * EPS * 18)
    assert np.all(s > 10 * tol), (s, tol, r.pairs)


@pytest.mark.parametrize("c,n,kinds", [(4, 60, ("ar06", "walk")), (3, 2049, ("walk", "trend", "ar06")), (2, 8000, SIGNALS),
                                       (2, 262146, ("walk", "ar06", "trend"))])
def test_host_finish_against_f64(c, n, kinds):
    """mmcmc_stats_finish and mmcmc_stats_finish_sums (no device) on float64-made partials cast to f32, against the float64
    finish: R-hat to 1e-5, ESS to 16 eps plus the f32 Geyer accumulation (pairs x eps, oracle.stats_f64.ess_rtol)."""
    import mini_mcmc_amd
    from mini_mcmc_amd import stats as S

    mini_mcmc_amd.lib()
    x = _sample(np.random.default_rng(n), c, n, kinds)
    stuck = np.stack([_stuck(c, n), _common(c, n)], axis=2)
    x = np.concatenate([x[:, :, :1], stuck, x[:, :, 1:]], axis=2)
    r = F.diagnostics(x)
    rtol = F.ess_rtol(r, EPS, base=16 * EPS)
    rhat, ess = S.stats_finish(r.means.astype(np.float32), r.ssq.astype(np.float32), r.acov.astype(np.float32))
    _close(rhat, r.rhat, 1e-5, "rhat")
    _close(ess, r.ess, rtol, "ess")
    overall = r.means.mean(axis=0)
    dsum = ((r.means - overall) ** 2).sum(axis=0)
    wsum = (r.ssq / r.m).sum(axis=0)
    rhat2, ess2 = S.stats_finish_sums(dsum, wsum, r.acov.astype(np.float32), r.c2)
    _close(rhat2, r.rhat, 1e-5, "rhat (sums)")
    _close(ess2, r.ess, rtol, "ess (sums)")
    # the closed forms through the host finish (m = n // 2 is not a power of two everywhere here, but the partials are exact)
    assert rhat[1] == 0.0 and ess[1] == pytest.approx(_stuck_ess(c, r.m), rel=1e-6)
    assert np.isnan(rhat[2]) and np.isnan(ess[2])


# ---------------------------------------------------------------- the kernels against it (GPU)

SELECTIONS = ("auto", "fft", "tile1", "tile", "mfma", "direct")


def _selections(m):
    if m <= 1024:
        return SELECTIONS
    if m <= 16384:
        return ("auto", "mfma", "direct")
    return ("auto", "direct")


def _transform_n(sel, m):
    """the transform length the library uses for (selection, m), or 0 for a direct-sum path"""
    if sel not in ("auto", "fft"):
        return 0
    if m <= 1024:
        if m < 2 or (sel == "auto" and m <= 100):
            return 0
        return 512 if m <= 256 else 1024 if m <= 512 else 2048
    if m <= 131072:
        return 2048 * max(2, -(-m // 1024))
    return 0


def _lag_tol(sel, m, c2):
    N = _transform_n(sel, m)
    return 4 * EPS * np.log2(N) if N else 4 * EPS * np.sqrt(m + c2)


# (m, odd n, D, chains): the first and last length of each path, N1 = 2 .. 128 with m = 1024 N1 and 1024 N1 + 1, D > 16 (the
# any-length moments kernel), chain counts that are not multiples of the residue path's 8-wide chain groups
LAG_CASES = [(1, 0, 3, 2), (1, 1, 17, 1), (2, 0, 1, 5), (3, 1, 16, 3), (100, 0, 33, 2), (100, 1, 1, 9), (101, 1, 3, 13),
             (512, 0, 17, 2), (513, 1, 1, 5), (1024, 0, 3, 9), (1024, 1, 16, 1), (1025, 1, 1, 2), (2048, 0, 33, 1),
             (2048, 1, 3, 5), (2049, 0, 17, 2), (3072, 1, 1, 13), (3073, 0, 3, 3), (4096, 1, 16, 2), (4097, 0, 1, 9),
             (5120, 0, 3, 5), (5121, 1, 17, 1), (10240, 1, 1, 13), (10241, 0, 33, 1), (17408, 0, 16, 2), (17409, 1, 3, 3),
             (50176, 1, 1, 2), (50177, 0, 3, 1), (125952, 0, 17, 1), (125953, 1, 1, 3), (131071, 1, 3, 1),
             (131072, 0, 1, 2), (131073, 1, 16, 1), (150000, 0, 3, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("m,odd,d,c", LAG_CASES)
def test_stats_partials_every_lag_every_path(m, odd, d, c):
    """`stats_partials` under every kernel selection that applies: means, centred sums of squares and the lag sum at every
    lag against float64 (bounds in the module docstring).  Parameter j carries SIGNALS[(j + m) % 7], f32 and f64 samples."""
    import torch

    from mini_mcmc_amd import stats as S

    n = 2 * m + odd
    kinds = [SIGNALS[(j + m) % len(SIGNALS)] for j in range(d)]
    x = _sample(np.random.default_rng(m * 7 + d), c, n, kinds, np.float64 if (m + d) % 2 else np.float32)
    r = F.diagnostics(x)
    h = F.splitcat(x)
    mean_tol = 4 * EPS * np.sqrt(m) * np.abs(h).max(axis=1) + 2 * EPS * np.abs(r.means)
    ssq_tol = (4 * np.sqrt(m) + 3) * EPS * r.ssq + m * mean_tol ** 2
    t = torch.from_numpy(x).cuda()
    try:
        for sel in _selections(m):
            S.set_kernel(sel)
            means, ssq, acov = (v.cpu().numpy().astype(np.float64) for v in S.stats_partials(t))
            assert np.all(np.abs(means.reshape(-1, d) - r.means) <= mean_tol), (sel, means, r.means)
            assert np.all(np.abs(ssq.reshape(-1, d) - r.ssq) <= ssq_tol), (sel, ssq, r.ssq)
            tol = _lag_tol(sel, m, r.c2)
            err = np.abs(acov - r.acov).max(axis=0)
            print(f"m={m} n={n} D={d} C={c} {sel}: lag sums {np.max(err / np.maximum(tol * r.acov[0], 1e-300)):.3f} of the bound")
            assert np.all(err <= tol * r.acov[0]), (sel, kinds, err / r.acov[0], tol, np.abs(acov - r.acov).argmax(axis=0))
    finally:
        S.set_kernel("auto")


# (m, odd n, chains, dtype, device sample): short (wave-level transform), N1 = 2, residues, any length -- each with the
# seven signals and both closed-form degenerate parameters between them
E2E_CASES = [(64, 0, 3, np.float32, False), (512, 1, 5, np.float64, True), (2048, 0, 4, np.float32, True),
             (8192, 1, 9, np.float64, False), (32768, 0, 2, np.float32, True), (262144, 1, 2, np.float32, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("m,odd,c,dtype,on_device", E2E_CASES)
def test_split_rhat_mean_ess_against_f64(m, odd, c, dtype, on_device):
    """split_rhat_mean_ess and run_stats against the float64 restatement: R-hat to 1e-4, ESS to 1e-3 plus the propagated
    lag-sum and Geyer-sum error; stuck chains give R-hat 0 and ESS c2 m / (4 floor(m / 2) - 1), one constant everywhere NaN
    -- compared by position, never masked -- in the same sample as live parameters.  The deep parameters prove on the host
    that their ESS reads lags beyond m / 2."""
    import torch

    from mini_mcmc_amd import stats as S

    n = 2 * m + odd
    rng = np.random.default_rng(m + c)
    live = _sample(rng, c, n, SIGNALS)
    x = np.concatenate([live[:, :, :3], _stuck(c, n)[:, :, None], live[:, :, 3:6], _common(c, n)[:, :, None],
                        live[:, :, 6:]], axis=2).astype(dtype)
    kinds = list(SIGNALS[:3]) + ["stuck"] + list(SIGNALS[3:6]) + ["common"] + list(SIGNALS[6:])
    r = F.diagnostics(x)
    assert r.rhat[3] == 0.0 and r.ess[3] == pytest.approx(_stuck_ess(c, m), rel=1e-12)
    assert np.isnan(r.rhat[7]) and np.isnan(r.ess[7])
    N = _transform_n("auto", m)
    lag_tol = 4 * EPS * np.log2(N) if N else 4 * EPS * np.sqrt(m + r.c2)
    ess_tol = F.ess_rtol(r, lag_tol)
    sens = F.late_lag_sensitivity(r)
    for j, k in enumerate(kinds):
        if _deep(k, m):
            assert sens[j] > 10 * ess_tol[j], (k, sens[j], ess_tol[j])
    sample = torch.from_numpy(x).cuda() if on_device else x
    rhat, ess = S.split_rhat_mean_ess(sample)
    rhat_ok = _close(rhat, r.rhat, 1e-4, "rhat")
    ess_ok = _close(ess, r.ess, ess_tol, "ess")
    assert rhat[3] == 0.0
    print(f"m={m}: max error / bound rhat {rhat_ok:.3f} ess {ess_ok:.3f}")
    st = S.run_stats(x[:, :, [0, 1, 2, 4, 5]])
    e5, r5 = r.ess[[0, 1, 2, 4, 5]], r.rhat[[0, 1, 2, 4, 5]]
    t5 = ess_tol[[0, 1, 2, 4, 5]]
    assert abs(st.ess.min - e5.min()) <= t5.max() * abs(e5.min())
    assert abs(st.ess.max - e5.max()) <= t5.max() * abs(e5.max())
    assert abs(st.rhat.min - r5.min()) <= 1e-4 * r5.min() and abs(st.rhat.max - r5.max()) <= 1e-4 * r5.max()
