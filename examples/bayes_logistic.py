"""Bayesian logistic regression on a dataset: 9 coefficients (an intercept and 8 regressors), 500 synthetic observations
generated here, a N(0, 1) prior, NUTS from the log-likelihood alone.  Not one of the reference's examples: there a struct
`LogisticRegression { x, y }` would implement `GradientTarget` and own its observations; here the observations are bound to
a run-time compiled kind (`AutodiffTarget(..., data=)`), the density body reads them row by row (`mm_data_row`) and its
gradient is forward-mode automatic differentiation on the device.  Prints `stats.summary` and returns it with the
coefficients the data was generated from."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mini_mcmc_amd.core import init_with_seed
from mini_mcmc_amd.distributions import AutodiffTarget
from mini_mcmc_amd.nuts import NUTS
from mini_mcmc_amd.stats import summary

DIM = 9

LOGP = r"""
template <class T> struct mmcmc_user_logp {
    static constexpr int dim = 9;
    template <class S> MM_HD static S logp(const mm_tparams<T> &P, const S *x) {
        const int rows = (int)P.p[0];                 // the number of observations travels in params
        S acc = 0;
        for (int r = 0; r < rows; ++r) {              // the loop over the observations stays rolled
            T row[dim + 1];                           // x_r0 .. x_r8, y_r
            mm_data_row<dim + 1>(P.mat, r, row);
            S eta = 0;
            MM_UNROLL
            for (int i = 0; i < dim; ++i) eta = mm_fma(row[i], x[i], eta);
            acc = acc + (row[dim] * eta - mm_softplusT(eta));   // y eta - log(1 + e^eta)
        }
        S pr = 0;
        MM_UNROLL
        for (int i = 0; i < dim; ++i) pr = mm_fma(x[i], x[i], pr);
        return mm_fma(T(-0.5), pr, acc);              // N(0, 1) prior
    }
};
"""


def synthetic(n_rows: int, seed: int = 1):
    """(rows [n, 10] = [1, x1 .. x8, y], the coefficients y was drawn with)"""
    rng = np.random.default_rng(seed)
    beta = np.array([-0.5, 1.0, -1.0, 0.5, 0.0, 0.75, -0.25, 0.0, 1.5])
    x = np.concatenate([np.ones((n_rows, 1)), rng.standard_normal((n_rows, DIM - 1))], axis=1)
    y = (rng.random(n_rows) < 1.0 / (1.0 + np.exp(-x @ beta))).astype(np.float64)
    return np.concatenate([x, y[:, None]], axis=1), beta


def main(n_chains: int = 1024, n_rows: int = 500, n_collect: int = 200, n_discard: int = 200):
    rows, beta = synthetic(n_rows)
    target = AutodiffTarget("bayes_logistic", DIM, LOGP, params=[n_rows], data=rows)
    sampler = NUTS(target, init_with_seed(n_chains, DIM, 42) * 0.1, 0.8).set_seed(42)
    sample = sampler.run(n_collect, n_discard, to="torch")
    s = summary(sample, names=["intercept"] + [f"b{j}" for j in range(1, DIM)])
    print(f"--- logistic regression, {n_rows} observations, NUTS, {n_chains} chains, {n_collect} draws kept of {n_collect + n_discard}")
    print(s)
    print("generated with:", beta)
    return s, beta


if __name__ == "__main__":
    main()
