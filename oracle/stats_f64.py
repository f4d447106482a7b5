"""Split R-hat / ESS (stats.rs:396-546) restated in float64 with NumPy -- TEST INFRASTRUCTURE ONLY.

oracle/stats.c follows the reference in f32 (its FFT is an f32 transform like rustfft's), so it cannot tell a kernel's
f32 error from its own.  This module takes the sample exactly as the reference does (cast to f32 first, RunStats::from,
stats.rs:365) and then does every step in float64:

  splitcat     (stats.rs:396-402)  the first m = n // 2 draws, then the last m; odd n drops the middle draw
  withinvar    (stats.rs:429-478)  c = number of half-chains c2, n = m, W the mean of the biased variances
  rhat         (stats.rs:425-427)  sqrt(W / var+), the reference's definition
  lag sums                         acov_sum[k, d] = sum over half-chains of sum_t y_t y_(t+k), y centred on its half-chain's
                                   mean: what the library's `stats_partials` returns (the reference's autocov divided by
                                   n and averaged over chains is acov_sum / m / c2)
  ess          (stats.rs:496-546)  Geyer's pairing as windows_with_stride(2, 2) walks it: the starting minimum
                                   rho0 + rho1 (0 when m < 2), a break on p <= 0, the cap, ESS = c2 m / tau

The lag sums come from a zero-padded float64 FFT of length >= 2 m (direct sums up to m = 64); their error is ~1e-15 of
lag 0, nothing beside an f32 kernel's.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

EPS32 = float(np.finfo(np.float32).eps) / 2  # unit roundoff of f32, 2^-24


def splitcat(sample) -> np.ndarray:
    """[chains, n, params] -> float64 [2 chains, m, params] of the f32-cast draws (stats.rs:396-402)."""
    x = np.asarray(sample)
    if x.ndim != 3:
        raise ValueError("sample must be [chains, n, params]")
    x = x.astype(np.float32).astype(np.float64)
    n = x.shape[1]
    m = n // 2
    return np.concatenate([x[:, :m], x[:, n - m:]], axis=0)


def lag_sums(halves: np.ndarray, chunk: int = 64) -> np.ndarray:
    """halves [c2, m, D] float64 -> acov_sum [m, D]: sum over half-chains of sum_t y_t y_(t+k), y = x - mean(x)."""
    c2, m, d = halves.shape
    out = np.zeros((m, d), dtype=np.float64)
    if m <= 64:
        y = halves - halves.mean(axis=1, keepdims=True)
        for k in range(m):
            out[k] = (y[:, :m - k] * y[:, k:]).sum(axis=(0, 1))
        return out
    L = 1
    while L < 2 * m:
        L <<= 1
    for j in range(d):
        spec = np.zeros(L // 2 + 1, dtype=np.float64)
        for c0 in range(0, c2, chunk):
            y = halves[c0:c0 + chunk, :, j]
            y = y - y.mean(axis=1, keepdims=True)
            f = np.fft.rfft(y, n=L, axis=1)
            spec += (f.real * f.real + f.imag * f.imag).sum(axis=0)
        out[:, j] = np.fft.irfft(spec, n=L)[:m]
    return out


@dataclass
class Diagnostics:
    """Everything a split-R-hat / ESS call computes, in float64.  means, ssq: [c2, D] in splitcat order (first halves of
    all chains, then second halves); acov: [m, D]; pairs: Geyer pairs added into tau per parameter."""
    means: np.ndarray
    ssq: np.ndarray
    acov: np.ndarray
    within: np.ndarray
    var: np.ndarray
    rhat: np.ndarray
    ess: np.ndarray
    tau: np.ndarray
    pairs: np.ndarray
    c2: int
    m: int


def finish(means, ssq, acov, c2: int, m: int):
    """withinvar + rhat + ess (stats.rs:425-546) in float64 from the sufficient statistics -> (W, var+, rhat, ess, tau, pairs)."""
    means = np.asarray(means, dtype=np.float64).reshape(c2, -1)
    ssq = np.asarray(ssq, dtype=np.float64).reshape(c2, -1)
    acov = np.asarray(acov, dtype=np.float64).reshape(m, -1)
    overall = means.mean(axis=0)
    b = ((means - overall) ** 2).sum(axis=0) * (m / (c2 - 1))
    w = (ssq / m).mean(axis=0)
    v = ((m - 1.0) / m) * w + b / m
    with np.errstate(divide="ignore", invalid="ignore"):
        rhat = np.sqrt(w / v)
        rho = 1.0 - (w - acov / m / c2) / v
    d = means.shape[1]
    tau = np.empty(d)
    pairs = np.zeros(d, dtype=np.int64)
    for j in range(d):
        r = rho[:, j]
        mn = r[0] + r[1] if m >= 2 else 0.0
        out = 0.0
        for t in range(0, m - 1, 2):
            p = r[t] + r[t + 1]
            if p <= 0.0:
                break
            if p > mn:
                p = mn
            mn = p
            out += p
            pairs[j] += 1
        tau[j] = -1.0 + 2.0 * out
    with np.errstate(divide="ignore", invalid="ignore"):
        ess = (1.0 / tau) * c2 * m
    return w, v, rhat, ess, tau, pairs


def diagnostics(sample) -> Diagnostics:
    """split_rhat_mean_ess (stats.rs:416-423) of [chains, n, params] in float64, with its sufficient statistics."""
    h = splitcat(sample)
    c2, m, _ = h.shape
    if m < 1:
        raise ValueError("split diagnostics need n >= 2")
    means = h.mean(axis=1)
    ssq = ((h - means[:, None, :]) ** 2).sum(axis=1)
    acov = lag_sums(h)
    w, v, rhat, ess, tau, pairs = finish(means, ssq, acov, c2, m)
    return Diagnostics(means, ssq, acov, w, v, rhat, ess, tau, pairs, c2, m)


def split_rhat_mean_ess(sample):
    """(rhat[params], ess[params]) in float64."""
    r = diagnostics(sample)
    return r.rhat, r.ess


def ess_rtol(r: Diagnostics, lag_tol: float, base: float = 1e-3) -> np.ndarray:
    """Relative ESS tolerance per parameter: `base` plus what an f32 finish on lag sums off by at most lag_tol * acov[0]
    can move tau by.  Each rho_t carries the lag-sum error divided by m c2 var+ and ~4 f32 roundings of quantities no larger
    than max(1, |rho|); every pair adds two of those, and the f32 running sum of `pairs` terms adds up to pairs x eps of
    itself.  tau = 2 out - 1, so tau moves by twice what `out` does."""
    m, c2 = r.m, r.c2
    with np.errstate(divide="ignore", invalid="ignore"):
        rho_err = lag_tol * r.acov[0] / (m * c2 * r.var)
        rho = 1.0 - (r.within - r.acov / m / c2) / r.var
        rmax = np.where(np.isnan(rho), 0.0, np.abs(rho)).max(axis=0)
        k = np.maximum(r.pairs, 1)
        out = (r.tau + 1.0) / 2.0
        dtau = 2.0 * (k * 2.0 * (rho_err + 4.0 * EPS32 * np.maximum(1.0, rmax)) + k * EPS32 * np.abs(out))
        return base + dtau / np.abs(r.tau)


def late_lag_sensitivity(r: Diagnostics, factor: float = 1.5) -> np.ndarray:
    """Relative change of the float64 ESS when every lag sum from m // 2 up is multiplied by `factor`: an input whose ESS
    does not move this way never reads its late lags, and cannot show an error there."""
    a = r.acov.copy()
    a[r.m // 2:] *= factor
    ess2 = finish(r.means, r.ssq, a, r.c2, r.m)[3]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.abs(ess2 - r.ess) / np.abs(r.ess)
