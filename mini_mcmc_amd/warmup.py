"""Cross-chain warm-up of the metric -- diagonal (`HMC.metric`, `NUTS.metric`) or, with `dense=True`, dense
(`HMC.metric_chol`, `NUTS.metric_chol`) --: host policy over the handles' own entry points.

A many-chain engine estimates a scale per coordinate from a few dozen transitions: the standard deviation pooled over
thousands of chains has thousands of nearly independent draws behind it after one short window, where a single chain needs
its whole warm-up.  The windows grow (Stan's 25 / 50 / 100 ...) because each is sampled under the previous window's metric
and is therefore better mixed than the one before.

    s = NUTS(target, x0, 0.8)
    scale, windows = warmup_nuts(s, seed=7)      # s.metric is set, iteration 0, epsilon = sentinel
    sample = s.set_seed(8).run(1000, 200)        # the caller's own run: searches epsilon under the metric, then adapts it

A per-coordinate scale helps only when the posterior's long and short directions lie along the axes.  For a rotated
posterior -- correlated regression coefficients, a Gaussian with a dense precision matrix -- `dense=True` estimates the
pooled covariance instead and sets its Cholesky factor: with thousands of chains one short window gives a well-conditioned
estimate of a full 32 x 32 covariance.
"""
from __future__ import annotations

import numpy as np

#: Stan's regulariser of the variance estimate: var' = N / (N + 5) var + 1e-3 * 5 / (N + 5)
_SHRINK_N, _SHRINK_TO = 5.0, 1e-3


def estimate_scale(sample, regularize: bool = True) -> np.ndarray:
    """The pooled standard deviation of a sample [C, n, D] -- a torch tensor (reduced on its device, only D numbers come
    back) or anything numpy takes -- over all C * n draws, per coordinate, computed in float64 with the population
    normalisation (divisor N).  regularize: Stan's shrinkage of the variance towards 1e-3, var' = N / (N + 5) var +
    1e-3 * 5 / (N + 5) with N = C * n, before the square root.  Returns [D] float64."""
    if type(sample).__module__.startswith("torch"):
        import torch

        if sample.ndim != 3:
            raise ValueError(f"sample: {tuple(sample.shape)}, expected [chains, draws, dim]")
        x = sample.reshape(-1, sample.shape[-1]).to(torch.float64)
        n = x.shape[0]
        var = ((x - x.mean(dim=0)) ** 2).mean(dim=0).cpu().numpy().astype(np.float64)
    else:
        a = np.asarray(sample, dtype=np.float64)
        if a.ndim != 3:
            raise ValueError(f"sample: {a.shape}, expected [chains, draws, dim]")
        x = a.reshape(-1, a.shape[-1])
        n = x.shape[0]
        var = ((x - x.mean(axis=0)) ** 2).mean(axis=0)
    if n < 1:
        raise ValueError("sample: no draws")
    if regularize:
        var = n / (n + _SHRINK_N) * var + _SHRINK_TO * _SHRINK_N / (n + _SHRINK_N)
    return np.sqrt(var)


#: rows of a torch sample reduced at a time by estimate_chol: bounds the float64 scratch to _CHUNK * D numbers
_CHUNK = 1 << 16


def estimate_chol(sample, regularize: bool = True) -> np.ndarray:
    """The lower Cholesky factor of the pooled covariance of a sample [C, n, D] over all N = C * n draws, computed in float64
    with the population normalisation (divisor N).  regularize: Stan's dense shrinkage, cov' = N / (N + 5) cov +
    1e-3 * 5 / (N + 5) * I.  A torch tensor is reduced on its device in chunks of rows (two passes: the mean, then the
    centred cross-products), so no float64 copy of the whole sample is made and only D^2 numbers come back.  Without the
    shrinkage N <= D draws have a singular covariance and no factor: ValueError.  Returns [D, D] float64."""
    if type(sample).__module__.startswith("torch"):
        import torch

        if sample.ndim != 3:
            raise ValueError(f"sample: {tuple(sample.shape)}, expected [chains, draws, dim]")
        x = sample.reshape(-1, sample.shape[-1])
        n, d = int(x.shape[0]), int(x.shape[1])
        if n < 1:
            raise ValueError("sample: no draws")
        total = torch.zeros(d, dtype=torch.float64, device=x.device)
        for lo in range(0, n, _CHUNK):
            total += x[lo:lo + _CHUNK].to(torch.float64).sum(dim=0)
        mean = total / n
        acc = torch.zeros((d, d), dtype=torch.float64, device=x.device)
        for lo in range(0, n, _CHUNK):
            xc = x[lo:lo + _CHUNK].to(torch.float64) - mean
            acc += xc.T @ xc
        cov = (acc / n).cpu().numpy().astype(np.float64)
    else:
        a = np.asarray(sample, dtype=np.float64)
        if a.ndim != 3:
            raise ValueError(f"sample: {a.shape}, expected [chains, draws, dim]")
        x = a.reshape(-1, a.shape[-1])
        n, d = x.shape
        if n < 1:
            raise ValueError("sample: no draws")
        xc = x - x.mean(axis=0)
        cov = xc.T @ xc / n
    cov = 0.5 * (cov + cov.T)
    if regularize:
        cov = n / (n + _SHRINK_N) * cov + _SHRINK_TO * _SHRINK_N / (n + _SHRINK_N) * np.eye(d)
    elif n <= d:
        raise ValueError(f"sample: the covariance of {n} draws in {d} dimensions is singular (regularize=True shrinks it)")
    try:
        return np.linalg.cholesky(cov)
    except np.linalg.LinAlgError as e:
        raise ValueError(f"sample: its covariance has no Cholesky factor ({e})") from None


def _sentinel_epsilon(sampler) -> None:
    """every chain's step size back to 'not searched yet' (-1): the next run's init_chain searches it, under the metric set"""
    from . import checkpoint as K

    ad = K.adapt_array(sampler)
    ad[:, 0] = -1.0
    K.set_adapt_array(sampler, ad)


def warmup_nuts(sampler, windows=(25, 50, 100), eps_transitions: int = 50, seed: int = 0, dense: bool = False):
    """Estimate a NUTS handle's diagonal metric over `windows`.  Window k: seed `seed + k + 1` (no window replays another's
    noise), iteration 0, every chain's epsilon at the sentinel -1 (init_chain searches it again, under the metric of the
    window before), `run(n_collect=windows[k], n_discard=eps_transitions, to="torch")`, then
    `sampler.metric = estimate_scale(sample)`.

    Returns (scale [dim] float64, records): one record per window with its "scale" and "mean_leapfrogs" (gradient
    evaluations per chain and transition of that window, from leapfrog_counts).  The handle is left with the final metric,
    iteration 0 and the epsilon sentinel, ready for the caller's own run(n_collect, n_discard); the seed is window
    len(windows)'s and the caller's to set.  Deterministic: the same arguments on the same handle state give the same
    bits.

    dense=True: each window sets `sampler.metric_chol = estimate_chol(sample)` instead; the first value returned is the
    factor [dim, dim] and the records carry "chol" in place of "scale"."""
    records = []
    scale = None
    for k, n in enumerate(windows):
        sampler.set_seed(int(seed) + k + 1)
        sampler.set_iteration(0)
        _sentinel_epsilon(sampler)
        before = sampler.leapfrog_counts().astype(np.float64)
        sample = sampler.run(int(n), int(eps_transitions), to="torch")
        # run(n, d) takes n + d - 1 transitions when d > 0 (the reference's N - 1 steps), n - 1 when d == 0
        steps = max(int(n) + int(eps_transitions) - 1, 1)
        mean_lf = float((sampler.leapfrog_counts().astype(np.float64) - before).mean()) / steps
        scale = estimate_chol(sample) if dense else estimate_scale(sample)
        del sample
        if dense:
            sampler.metric_chol = scale
        else:
            sampler.metric = scale
        records.append({"chol" if dense else "scale": scale.copy(), "mean_leapfrogs": mean_lf})
    sampler.set_iteration(0)
    _sentinel_epsilon(sampler)
    return scale, records


def warmup_hmc(sampler, windows=(25, 50, 100), discard: int = 50, seed: int = 0, dense: bool = False):
    """The same loop for an HMC handle, without the step-size part: window k runs
    `run(n_collect=windows[k], n_discard=discard, to="torch")` under seed `seed + k + 1` from iteration 0 and sets
    `sampler.metric = estimate_scale(sample)`.  The caller owns `step_size` and `n_leapfrog` (nothing here adapts them):
    without a metric the step must suit the smallest scale; with a metric of the posterior's standard deviations a step
    size of order 1 is the natural scale, so a caller usually raises step_size after the first window.  Returns
    (scale, records) with each window's "scale" and "accept_rate"; the handle is left at iteration 0.  dense=True: as
    warmup_nuts -- `sampler.metric_chol = estimate_chol(sample)`, "chol" in place of "scale"."""
    records = []
    scale = None
    for k, n in enumerate(windows):
        sampler.set_seed(int(seed) + k + 1)
        sampler.set_iteration(0)
        sample = sampler.run(int(n), int(discard), to="torch")
        rate = float(sampler.accept_counts.mean()) / max(int(n) + int(discard), 1)
        scale = estimate_chol(sample) if dense else estimate_scale(sample)
        del sample
        if dense:
            sampler.metric_chol = scale
        else:
            sampler.metric = scale
        records.append({"chol" if dense else "scale": scale.copy(), "accept_rate": rate})
    sampler.set_iteration(0)
    return scale, records
