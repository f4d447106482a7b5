"""The pilot split of the NUTS persistent scheduler (csrc/mm_nuts_plan.h: mm_nuts_pilot_split; mm_nuts_api.hip: run_lg_queue).

A fresh lane-group handle on variant 3 has no depth histogram to choose its first compaction level from, so a run of at least
64 transitions goes out as two launches: a 16-transition pilot, then the rest at the level the pilot's histogram gives.  The
split must not change a result: the second launch continues the stream at step m0 + 16 and writes behind the pilot's rows.
GaussianND of dim 16 at condition number 10 (shallow trees), mode 2, 2056 chains: at least 2048, so the scheduler runs, and not a
multiple of 16, so the last group of 16 is ragged.  Against variant 1 (one launch, no compaction), with the pilot inside the
unrecorded transitions, inside the recorded ones behind an initial row, and across the two."""
import numpy as np
import pytest

from mini_mcmc_amd.core import init_with_seed
from mini_mcmc_amd.distributions import GaussianND
from mini_mcmc_amd.nuts import NUTS

CHAINS, DIM = 2056, 16


@pytest.fixture(scope="module")
def problem():
    return GaussianND.ill_conditioned(DIM, 10.0, 5), init_with_seed(CHAINS, DIM, 31) * 0.3


@pytest.mark.gpu
@pytest.mark.parametrize("n_collect,n_discard", [(40, 30), (70, 0), (60, 10)],
                         ids=["pilot_in_unrecorded", "initial_row_pilot_in_recorded", "pilot_straddles"])
def test_pilot_split_changes_no_result(problem, n_collect, n_discard):
    target, init = problem
    assert n_collect + n_discard - 1 >= 64  # run() takes N - 1 transitions: enough for a split
    got = {}
    for variant in (3, 1):
        s = NUTS(target, init, 0.8, mode=2).set_seed(17)  # fresh: no histogram, no set_compaction
        assert s.kernel_variant == 3
        s.set_kernel_variant(variant)
        out = s.run(n_collect, n_discard)
        launches = s.timing()["n_launches"]
        print(f"variant {variant} run({n_collect}, {n_discard}): {launches} launches")
        assert launches == (2 if variant == 3 else 1)
        got[variant] = (out, s.positions(), s.leapfrog_counts(), s.adapt_state(), s.depth_histogram())
        assert got[variant][4].sum() == CHAINS * (n_collect + n_discard - 1)
        s.run(5, 0)
        assert s.timing()["n_launches"] == 1  # the level is known now: no pilot
        s.close()
    a, b = got[3], got[1]
    assert a[0].shape == (CHAINS, n_collect, DIM)
    bits = lambda x: np.ascontiguousarray(x).view(np.uint64)  # noqa: E731 -- mode 2: every value is a float64
    assert a[0].dtype == np.float64 and np.array_equal(bits(a[0]), bits(b[0]))
    assert np.array_equal(bits(a[1]), bits(b[1]))
    assert np.array_equal(a[2], b[2])
    for k in ("epsilon", "epsilon_bar", "h_bar", "mu"):
        assert np.array_equal(bits(a[3][k]), bits(b[3][k])), k
    assert np.array_equal(a[4], b[4])
