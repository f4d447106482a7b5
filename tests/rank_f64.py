"""Float64 yardstick of the rank-normalised diagnostics (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021) as
include/mmcmc.h defines them -- TEST INFRASTRUCTURE ONLY, independent of the library:

  ranks       scipy.stats.rankdata(..., "average") of the pooled f32 draws of a parameter (-0.0 == +0.0 there too)
  scores      scipy.special.ndtri((rank - 3/8) / (S + 1/4)) in float64
  folded      the same for |x - med| formed in f32, med = the type-7 median rounded to f32
  quantiles   np.quantile (default method) of the f32 draws as float64
  R-hat, ESS  oracle.stats_f64.diagnostics (the reference's split R-hat / ESS restated in float64) of the transformed arrays
              rounded to f32 -- what the library's own split ESS is given; the conventional R-hat is 1 / its rhat

A parameter with a NaN draw is NaN throughout and has rank2 = 0.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
from scipy.special import ndtri
from scipy.stats import rankdata

from oracle import stats_f64 as F


def _cols(sample):
    x = np.asarray(sample)
    if x.ndim != 3:
        raise ValueError("sample must be [chains, n, params]")
    x32 = x.astype(np.float32)
    return x32, x32.reshape(-1, x32.shape[2])


def fold(sample) -> np.ndarray:
    """|x - med| in f32, [chains, n, params]"""
    x32, flat = _cols(sample)
    med = np.empty(flat.shape[1], dtype=np.float32)
    for j in range(flat.shape[1]):
        col = flat[:, j]
        med[j] = np.float32(np.quantile(col.astype(np.float64), 0.5)) if not np.isnan(col).any() else np.float32("nan")
    with np.errstate(invalid="ignore"):
        return np.abs(x32 - med)


def rank2(sample, folded: bool = False) -> np.ndarray:
    """2 x the tie-averaged 1-based rank among the pooled draws of each parameter: int64 [chains, n, params]"""
    x32 = fold(sample) if folded else _cols(sample)[0]
    flat = x32.reshape(-1, x32.shape[2])
    out = np.zeros(flat.shape, dtype=np.int64)
    for j in range(flat.shape[1]):
        col = flat[:, j]
        if not np.isnan(col).any():
            out[:, j] = np.rint(2.0 * rankdata(col, method="average")).astype(np.int64)
    return out.reshape(x32.shape)


def scores_from_rank2(r2: np.ndarray) -> np.ndarray:
    """float64 normal scores; NaN where rank2 == 0 (the NaN-flagged parameters)"""
    s = r2.shape[0] * r2.shape[1]
    u = (r2.astype(np.float64) * 0.5 - 0.375) / (s + 0.25)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(r2 == 0, np.nan, ndtri(np.where(r2 == 0, 0.5, u)))


def normal_scores(sample, folded: bool = False) -> np.ndarray:
    return scores_from_rank2(rank2(sample, folded))


def quantiles(sample, probs) -> np.ndarray:
    """float64 [len(probs), params]"""
    _, flat = _cols(sample)
    out = np.full((len(probs), flat.shape[1]), np.nan)
    for j in range(flat.shape[1]):
        col = flat[:, j]
        if not np.isnan(col).any():
            out[:, j] = np.quantile(col.astype(np.float64), np.asarray(probs, dtype=np.float64))
    return out


def brackets(sample, probs):
    """the order statistics (a, b) = sorted[j], sorted[min(j + 1, S - 1)], j = floor((S - 1) p): float64 [len(probs), params] each"""
    _, flat = _cols(sample)
    s = flat.shape[0]
    srt = np.sort(flat.astype(np.float64), axis=0)
    j = np.floor((s - 1) * np.asarray(probs, dtype=np.float64)).astype(np.int64)
    return srt[j], srt[np.minimum(j + 1, s - 1)]


@dataclass
class RankYardstick:
    """F.Diagnostics of the four transformed arrays, and what the library reports from them"""
    bulk: F.Diagnostics
    folded: F.Diagnostics
    lower: F.Diagnostics
    upper: F.Diagnostics
    rhat_bulk: np.ndarray
    rhat_folded: np.ndarray
    rhat: np.ndarray
    ess_bulk: np.ndarray
    ess_tail_lower: np.ndarray
    ess_tail_upper: np.ndarray
    ess_tail: np.ndarray
    quantiles: np.ndarray


def diagnostics(sample, probs=(0.05, 0.5, 0.95)) -> RankYardstick:
    x32, _ = _cols(sample)
    z = normal_scores(sample).astype(np.float32)
    zf = normal_scores(sample, folded=True).astype(np.float32)
    q = quantiles(sample, (0.05, 0.95))
    with np.errstate(invalid="ignore"):
        lo = (x32.astype(np.float64) <= q[0]).astype(np.float32)
        hi = (x32.astype(np.float64) <= q[1]).astype(np.float32)
    nan = np.isnan(x32).any(axis=(0, 1))
    lo[:, :, nan] = np.nan
    hi[:, :, nan] = np.nan
    with np.errstate(invalid="ignore", divide="ignore"):
        b, f, l, u = F.diagnostics(z), F.diagnostics(zf), F.diagnostics(lo), F.diagnostics(hi)
        rb, rf = 1.0 / b.rhat, 1.0 / f.rhat
    either = np.isnan(rb) | np.isnan(rf)
    rhat = np.where(either, np.nan, np.maximum(rb, rf))
    tail = np.where(np.isnan(l.ess) | np.isnan(u.ess), np.nan, np.minimum(l.ess, u.ess))
    return RankYardstick(b, f, l, u, rb, rf, rhat, b.ess, l.ess, u.ess, tail, quantiles(sample, probs))


def geyer_margin(r: F.Diagnostics, lag_tol: float) -> np.ndarray:
    """Per parameter: (the smallest |pair sum| Geyer's loop looks at, the stopping pair included) / (what an f32 finish on lag
    sums within lag_tol of lag 0 can move a pair sum by -- the per-pair term of oracle.stats_f64.ess_rtol).  Above 1 the
    truncation point cannot differ between float64 and the library; the tests assert it for every parameter they compare."""
    m, c2 = r.m, r.c2
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = 1.0 - (r.within - r.acov / m / c2) / r.var
        rho_err = lag_tol * r.acov[0] / (m * c2 * r.var)
    out = np.full(rho.shape[1], np.inf)
    for j in range(rho.shape[1]):
        col = rho[:, j]
        if np.isnan(col).any():
            continue
        rmax = np.abs(col).max()
        err = 2.0 * (rho_err[j] + 4.0 * F.EPS32 * max(1.0, rmax))
        smallest = np.inf
        for t in range(0, m - 1, 2):
            p = col[t] + col[t + 1]
            smallest = min(smallest, abs(p))
            if p <= 0.0:
                break
        out[j] = smallest / err
    return out
