"""A rotated Gaussian by NUTS, with and without a dense metric (not in the reference).

The target is a 9-D Gaussian whose principal axes have standard deviations from 0.1 to 10 and are rotated away from the
coordinate axes: every marginal is wide, so a per-coordinate metric sees nothing to rescale and NUTS runs to its tree-depth
cap.  `warmup_nuts(..., dense=True)` estimates the pooled covariance over all chains in three short windows and sets its
Cholesky factor as the metric; the same loop with a diagonal metric is run next to it.  Printed: the leapfrogs per
transition of `run(200, 50)` under either metric, and how well the estimated factor whitens the true covariance."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mini_mcmc_amd.core import init_with_seed
from mini_mcmc_amd.distributions import GaussianND
from mini_mcmc_amd.nuts import NUTS
from mini_mcmc_amd.warmup import warmup_nuts


def main(n_chains=1024, dim=9):
    sigma = np.logspace(-1.0, 1.0, dim)
    q, _ = np.linalg.qr(np.random.default_rng(1).normal(size=(dim, dim)))
    cov = (q * sigma ** 2) @ q.T
    target = GaussianND((q / sigma ** 2) @ q.T)
    x0 = init_with_seed(n_chains, dim, 42)
    result = {}
    for name, dense in (("dense", True), ("diagonal", False)):
        sampler = NUTS(target, x0, 0.8, mode=2)
        metric, windows = warmup_nuts(sampler, windows=(25, 50, 100), seed=7, dense=dense)
        sampler.set_seed(8)
        before = sampler.leapfrog_counts().astype(np.float64).sum()
        sample = sampler.run(200, 50)
        leapfrogs = (sampler.leapfrog_counts().astype(np.float64).sum() - before) / (n_chains * 249)
        print(f"{name:8s} metric: warm-up leapfrogs per transition {[round(w['mean_leapfrogs'], 1) for w in windows]}, "
              f"run(200, 50): {leapfrogs:.1f}")
        result[name] = (sample, leapfrogs, metric)
        sampler.close()
    chol = result["dense"][2]
    whitened = np.linalg.solve(chol, np.linalg.solve(chol, cov).T)
    print(f"condition number of the covariance: {np.linalg.cond(cov):.0f}; whitened by the estimated factor: {np.linalg.cond(whitened):.3f}")
    assert result["dense"][0].shape == (n_chains, 200, dim)
    return result


if __name__ == "__main__":
    main()
