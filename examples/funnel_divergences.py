"""Neal's funnel by NUTS with per-draw statistics: where the sampler diverges (not in the reference).

v ~ N(0, 3^2), x_i | v ~ N(0, e^v), i = 1 .. 4: the neck of the funnel (v << 0) has a curvature no single step size fits, so
a sampler whose step was adapted in the mouth diverges there and under-samples it -- while R-hat, computed from what was
sampled, can look clean.  The target is written as its log-density alone (`AutodiffTarget`: the gradient is forward-mode
automatic differentiation on the device); `NUTS.set_draw_stats()` records every transition.  Printed: the share of divergent
transitions, the mean of v over the draws that follow a divergent transition against its mean over all draws (the exact
mean is 0; divergences sit in the neck, and the sample as a whole is biased away from it), and the smallest E-BFMI."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mini_mcmc_amd import stats
from mini_mcmc_amd.core import init_with_seed
from mini_mcmc_amd.distributions import AutodiffTarget
from mini_mcmc_amd.nuts import NUTS, unpack_tree

FUNNEL = """
template <class T> struct mmcmc_user_logp {
    static constexpr int dim = 5;
    template <class S> MM_HD static S logp(const mm_tparams<T> &, const S *x) {
        S q = x[1] * x[1];
        MM_UNROLL
        for (int i = 2; i < dim; ++i)
            q = q + x[i] * x[i];
        return T(-1.0 / 18.0) * (x[0] * x[0]) - T(0.5 * (dim - 1)) * x[0] - T(0.5) * (mm_expT(-x[0]) * q);
    }
};
"""


def main(n_chains=1024, n_collect=200, n_discard=200):
    target = AutodiffTarget("example_funnel5", 5, FUNNEL)
    sampler = NUTS(target, 0.5 * init_with_seed(n_chains, 5, 42), 0.8, mode=0).set_seed(7).set_draw_stats()
    sample = sampler.run(n_collect, n_discard)
    records = sampler.draw_stats()
    _, depth, divergent, _, transition = unpack_tree(records["tree"])
    summary = stats.nuts_summary(records)
    v = sample[:, :, 0].astype(np.float64)
    print(summary)
    print(f"mean tree depth {depth[transition].mean():.2f}, mean accept stat {np.nanmean(summary.mean_accept):.3f}")
    if divergent.any():
        print(f"mean of v over the {int(divergent.sum())} draws after a divergent transition: {v[divergent].mean():+.3f}; over all draws: "
              f"{v.mean():+.3f} (exact: 0)")
    else:
        print(f"no divergent transition; mean of v over all draws: {v.mean():+.3f} (exact: 0)")
    assert records.shape == (n_chains, n_collect) and summary.total_transitions == int(transition.sum())
    assert summary.total_divergent == int(divergent.sum())
    sampler.close()
    return summary, sample, records


if __name__ == "__main__":
    main()
