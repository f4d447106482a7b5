"""Rank-normalised diagnostics (Vehtari et al. 2021) of two runs on the 3-D Rosenbrock density, side by side:
the headline's fixed-(eps, L) HMC run, run(400, 50) of 65 536 chains, whose chains get stuck in the stiff tail, and the converged
`run_jittered` run (eps and L drawn per block of 100 transitions).  Not one of the reference's examples: its diagnostics end at
the mean-based split R-hat and the mean ESS, which `run_stats` prints here for comparison."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mini_mcmc_amd.core import init_with_seed
from mini_mcmc_amd.distributions import RosenbrockND
from mini_mcmc_amd.hmc import HMC, run_jittered
from mini_mcmc_amd.stats import run_stats, summary


def main(n_chains: int = 65536, keep_blocks: int = 40):
    init = init_with_seed(n_chains, 3, 42, np.float32)
    fixed = HMC(RosenbrockND(3), init, 0.032, 10).set_seed(42).run(400, 50, to="torch")
    jittered, _ = run_jittered(RosenbrockND(3), init, (0.004, 0.016), (100, 400), 100, 20, keep_blocks, seed=42)
    out = []
    for label, sample in (("fixed (eps, L) = (0.032, 10), run(400, 50)", fixed),
                          (f"jittered eps ~ U(0.004, 0.016), L ~ U{{100..400}}, {keep_blocks * 100} draws kept", jittered)):
        s = summary(sample, names=["x0", "x1", "x2"])
        print(f"--- {label}: {list(sample.shape)}")
        print(run_stats(sample))
        print(s)
        out.append(s)
    return out


if __name__ == "__main__":
    main()
