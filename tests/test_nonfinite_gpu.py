"""MH and HMC where energies and log-ratios are inf or NaN, on every kernel path a handle can take.

mm_samplers.h promises "MH strict `>`, HMC `>=`, NaN rejects".  The device decides through code the host build does not run
(the band filters of mm_rng.h, LDS tiles, ballots, packed pairs, lane-group reductions), and the parity tests elsewhere start
from init_with_seed * 0.3 .. 0.8, where every energy is finite.  Here (inputs and classifier: tests/nonfinite_common.py) every
case is checked three ways:

  1. bit equality with the host twin -- samples, states, accept counts, compared as integers so that NaN payloads and signed
     zeros count; a run(24, 4) continued by a run(12, 0);
  2. invariants computed from the device's output alone (nonfinite_common.device_invariants): rows that changed = accept
     count; no NaN / inf in a chain that started finite; the NaN / +inf / -inf chains keep their start bits and count 0; no
     accepted row whose sum of squares (2 |logp|, the quantity that overflows) exceeds 1.01 x the type's largest finite value;
  3. neighbour independence: the finite-start chains equal, bit for bit, a run of those chains alone at their chain offsets.

The CPU half of every case (also run on its own, without a device: test_inputs_show_every_class) asserts from the host twin
and the classifier that the inputs show at least 10 transitions of each class -- ratio +inf (must accept), NaN (must reject),
-inf (must reject), ordinary accepts, ordinary rejects -- per (dtype, dim), and that no twin row lies within 1 % of the edge.

Variants come from the handle: every number set_kernel_variant accepts (mm_path.h: mm_variant_status) is run, so a path added
later is covered without an edit here; the sets in NEED_VARIANTS must be among them.  Not run: 1 (an alias, launches what 2
launches) and HMC's 8 (other summation order, margin-safe inputs and its own overflow case: tests/test_wide_hmc_edges.py).
"""
import functools

import numpy as np
import pytest

import nonfinite_common as N

DTYPES = [np.float32, np.float64]
MH_DIMS = [1, 2, 3, 8, 9]  # f32 1, 2: the paired stream and its mhp filter; 3, 8: the plain filter; 9: generic kernel and unit
HMC_DIMS = [1, 2, 3, 8, 9]
HMC_CASES = ((1.0, 1), (1.0, 2), (1.0, 10), (2.5, 1))  # (eps, L); 2.5: past the leapfrog's stability limit, |x| grows: the falls
MH_SEED = {(np.float32, 1): 33, (np.float32, 2): 37, (np.float32, 3): 30, (np.float32, 8): 30, (np.float32, 9): 30}
HMC_SEED = 29
MIN_PER_CLASS = 10
SKIP_VARIANTS = {"mh": (1,), "hmc": (1, 8)}
NEED_VARIANTS = {"mh": lambda dim: {0, 2, 5, 6, 7} if dim <= 8 else {6, 7}, "hmc": lambda dim: {0, 2, 5, 6, 7} if dim <= 8 else {6, 7}}


@pytest.fixture(scope="module")
def M():
    import mini_mcmc_amd
    from mini_mcmc_amd import core, distributions, hmc, metropolis_hastings

    mini_mcmc_amd.lib()

    class NS:
        pass

    ns = NS()
    ns.core, ns.dist, ns.hmc, ns.mh = core, distributions, hmc, metropolis_hastings
    return ns


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(N.bits(a), N.bits(b))


class Twin:
    """what the host build says about one case: the run in two parts, every row, the class of every transition"""


def _twin(run, init):
    """run(init, nc, nd, iter0) -> (out, state, acc)"""
    t = Twin()
    t.init = init
    t.out1, t.st1, t.acc1 = run(init, N.FIRST[0], N.FIRST[1], 0)
    t.out2, t.st2, t.acc2 = run(t.st1, N.SECOND, 0, N.FIRST[0] + N.FIRST[1])
    full, st, acc = run(init, N.N_TRANS, 0, 0)
    assert same(full[:, N.FIRST[1]:], np.concatenate([t.out1, t.out2], axis=1)) and same(st, t.st2)
    assert np.array_equal(acc, t.acc1 + t.acc2)
    t.rows, t.acc = np.concatenate([init[:, None], full], axis=1), acc
    return t


@functools.lru_cache(maxsize=None)
def mh_twin(O, dtype, dim):
    init, isbad = N.starts(O, dtype, dim)
    std, seed = N.mh_std(dtype, dim), MH_SEED.get((dtype, dim), 29)
    t = _twin(lambda x, nc, nd, it0: O.engine_host_run("mh", O.STANDARD_NORMAL, dim, [], x, std, nc, nd, seed=seed, iter0=it0,
                                                       dtype=dtype), init)
    t.isbad, t.std, t.seed = isbad, std, seed
    t.counts = N.count(N.mh_classes(O, dtype, t.rows, isbad, std, seed=seed))
    return t


@functools.lru_cache(maxsize=None)
def hmc_twin(O, dtype, dim, eps, L):
    init, isbad = N.starts(O, dtype, dim)
    t = _twin(lambda x, nc, nd, it0: O.engine_host_run("hmc", O.STANDARD_NORMAL, dim, [], x, eps, nc, nd, seed=HMC_SEED, iter0=it0,
                                                       n_leapfrog=L, dtype=dtype), init)
    t.isbad, t.seed = isbad, HMC_SEED
    t.counts = N.count(N.hmc_classes(O, dtype, t.rows, isbad, eps, L, seed=HMC_SEED))
    return t


def _check_counts(counts, what):
    for name in N.CLASSES:
        assert counts[name] >= MIN_PER_CLASS, (what, counts)


def _pooled(twins):
    return {name: sum(t.counts[name] for t in twins) for name in N.CLASSES}


def _cpu_half_mh(O, dtype, dim):
    t = mh_twin(O, dtype, dim)
    _check_counts(t.counts, ("mh", dtype.__name__, dim))
    N.device_invariants(dtype, t.init, t.isbad, t.rows, t.acc, ("twin mh", dtype.__name__, dim))
    return t


def _cpu_half_hmc(O, dtype, dim):
    twins = [hmc_twin(O, dtype, dim, eps, L) for eps, L in HMC_CASES]
    _check_counts(_pooled(twins), ("hmc", dtype.__name__, dim))
    for t, (eps, L) in zip(twins, HMC_CASES):
        N.device_invariants(dtype, t.init, t.isbad, t.rows, t.acc, ("twin hmc", dtype.__name__, dim, eps, L))
    return twins


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_inputs_show_every_class(O, dtype):
    """The CPU half alone: per dim, MH and HMC (the four (eps, L) pooled) show >= 10 transitions of each of the five classes
    on the host build, the twin itself keeps the three rules and the invariants, and none of its rows lies at the edge."""
    for dim in MH_DIMS:
        _cpu_half_mh(O, dtype, dim)
    for dim in HMC_DIMS:
        _cpu_half_hmc(O, dtype, dim)


# ------------------------------------------------------------------ GPU


def _variants(make, sampler, dim):
    from mini_mcmc_amd import _lib as L

    got = set()
    for v in range(-1, 12):
        s = make()
        try:
            s.set_kernel_variant(v)
            got.add(v)
        except L.MmcmcError as e:  # a refusal is one of these two; anything else is a failure of the test
            assert e.status in (L.ERR_INVALID_ARG, L.ERR_UNSUPPORTED), (sampler, dim, v, e)
        finally:
            s.close()
    assert NEED_VARIANTS[sampler](dim) <= got, (sampler, dim, got)
    print(sampler, "dim", dim, "variants accepted", sorted(got))
    return sorted(got - set(SKIP_VARIANTS[sampler]))


def _device_case(make, t, dtype, what, prepare=lambda s: s, ranges=None):
    """make(init, offset) -> a fresh handle on those chains; prepare(handle): variant, metric, ...  The three checks.
    ranges: the chains run alone (default: every stretch of finite-start chains between the bad ones)."""
    s = prepare(make(t.init, 0))
    out1 = s.run(*N.FIRST)
    acc1 = s.accept_counts.copy()
    assert same(out1, t.out1), (what, "samples of run 1")
    assert np.array_equal(acc1, t.acc1), (what, "accept counts of run 1")
    assert same(s.state(), t.st1), (what, "state after run 1")
    out2 = s.run(N.SECOND, 0)
    assert same(out2, t.out2) and np.array_equal(s.accept_counts, t.acc2) and same(s.state(), t.st2), (what, "continued run")
    s.close()
    s = prepare(make(t.init, 0))
    rows = np.concatenate([t.init[:, None], s.run(N.N_TRANS, 0)], axis=1)
    acc = s.accept_counts.copy()
    s.close()
    assert same(rows, t.rows) and np.array_equal(acc, t.acc), (what, "every row")
    N.device_invariants(dtype, t.init, t.isbad, rows, acc, what)
    for lo, hi in ranges or N.stretches(t.isbad):
        a = prepare(make(t.init[lo:hi], lo))
        alone = a.run(N.N_TRANS, 0)
        assert same(alone, rows[lo:hi, 1:]) and np.array_equal(a.accept_counts, acc[lo:hi]), (what, "alone", lo, hi)
        a.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dim", MH_DIMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_mh_nonfinite_ratios_on_every_variant(M, O, dtype, dim):
    t = _cpu_half_mh(O, dtype, dim)

    def make(init, off):
        s = M.mh.MetropolisHastings(M.dist.StandardNormal(dim), M.dist.IsotropicGaussian(t.std), init).seed(t.seed)
        return s.set_chain_offset(off) if off else s

    for v in _variants(lambda: make(t.init, 0), "mh", dim):
        _device_case(make, t, dtype, ("mh", dtype.__name__, dim, "variant", v), lambda s: s.set_kernel_variant(v))


@pytest.mark.gpu
@pytest.mark.parametrize("dim", HMC_DIMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_hmc_nonfinite_energies_on_every_variant(M, O, dtype, dim):
    """L = 10 takes the compile-time-L launchers of variants 2 and 5 (run_hmc_pp10, run_hmc_split10), L = 1 and 2 the others."""
    twins = _cpu_half_hmc(O, dtype, dim)
    variants = _variants(lambda: M.hmc.HMC(M.dist.StandardNormal(dim), twins[0].init, 1.0, 1), "hmc", dim)
    for t, (eps, L) in zip(twins, HMC_CASES):

        def make(init, off):
            s = M.hmc.HMC(M.dist.StandardNormal(dim), init, eps, L).set_seed(t.seed)
            return s.set_chain_offset(off) if off else s

        for v in variants:
            _device_case(make, t, dtype, ("hmc", dtype.__name__, dim, eps, L, "variant", v), lambda s: s.set_kernel_variant(v))


ROS_EPS = (0.2, 5.0, 1e6)


@functools.lru_cache(maxsize=None)
def ros_twin(O, dtype, eps):
    init = O.init_with_seed(35, 3, 42, dtype)
    t = _twin(lambda x, nc, nd, it0: O.engine_host_run("hmc", O.ROSENBROCK_ND, 3, [], x, eps, nc, nd, seed=HMC_SEED, iter0=it0,
                                                       n_leapfrog=10, dtype=dtype), init)
    t.isbad, t.seed = np.zeros(35, dtype=bool), HMC_SEED
    return t


def _cpu_half_ros(O, dtype):
    twins = [ros_twin(O, dtype, eps) for eps in ROS_EPS]
    for t in twins:  # every trajectory's energy is huge, inf or NaN: nothing is accepted, no row changes
        assert t.acc.sum() == 0 and (N.bits(t.rows) == N.bits(t.init)[:, None]).all()
    return twins


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_rosenbrock_inputs_reject_everything(O, dtype):
    _cpu_half_ros(O, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_hmc_rosenbrock3_huge_steps_reject_everything(M, O, dtype):
    """RosenbrockND(3) from init_with_seed, L = 10 (the headline kernel's shape), eps 0.2, 5 and 1e6: 35 chains x 40
    transitions, none accepted on the host build in either type; the device must say the same on every variant, and a
    sub-range of the chains alone gives the same rows."""
    twins = _cpu_half_ros(O, dtype)
    variants = _variants(lambda: M.hmc.HMC(M.dist.RosenbrockND(3), twins[0].init, 0.2, 10), "hmc", 3)
    for t, eps in zip(twins, ROS_EPS):

        def make(init, off):
            s = M.hmc.HMC(M.dist.RosenbrockND(3), init, eps, 10).set_seed(t.seed)
            return s.set_chain_offset(off) if off else s

        for v in variants:
            _device_case(make, t, dtype, ("hmc rosenbrock3", dtype.__name__, eps, "variant", v), lambda s: s.set_kernel_variant(v),
                         ranges=[(7, 29)])


# ------------------------------------------------------------------ lane groups (HMC variant 3)

LG_CASES = ((0.1, 10), (0.4, 1))  # (eps, L); 0.4: eps^2 lambda_max = 8 > 4, the stiff direction grows threefold a step: the falls
LG_GOOD = 82  # with the three bad chains 85 = five 16-chain groups and five


def _lg_matrix(dim):
    from mini_mcmc_amd.distributions import GaussianND

    return GaussianND.ill_conditioned(dim, 50.0, 7).precision


def _lg_inputs(O, dtype, dim):
    """init_with_seed * 0.3, and on top of it, by chain c % 6, a multiple r of the edge radius along an eigenvector of A
    (x^T A x = r^2 x the largest finite value): 1, 5: r about 1.05 along the softest direction (logp -inf; a trajectory
    brings x^T A x and p.p back under the edge: escapes); 2: r about 0.9 along the stiffest (finite; at eps = 0.4 it grows
    past the edge: falls); 3: r = 3 (never comes back: stuck); 0, 4: nothing added.  Plus a NaN, a +inf and a -inf chain."""
    lam, vec = np.linalg.eigh(_lg_matrix(dim).astype(dtype).astype(np.float64))
    good = O.init_with_seed(LG_GOOD, dim, 3, np.float64) * 0.3
    R = float(np.sqrt(N.tmax(dtype)))
    for c in range(LG_GOOD):
        wob = 1.0 + 0.02 * np.cos(2.3 * c)
        r, k = {1: (1.045 * wob, 0), 5: (1.05 * wob, 0), 2: (0.9 * wob, dim - 1), 3: (3.0, 0)}.get(c % 6, (0.0, 0))
        good[c] += r * R / np.sqrt(lam[k]) * vec[:, k] * (1.0 if c % 4 < 2 else -1.0)
    return N.insert_bad(good.astype(dtype), (9, 48, LG_GOOD + 2))


@functools.lru_cache(maxsize=None)
def lg_twin(O, dtype, dim, eps, L):
    A = _lg_matrix(dim)
    init, isbad = _lg_inputs(O, dtype, dim)
    fn = O.engine_host_hmc_grouped_run_f32 if dtype == np.float32 else O.engine_host_hmc_grouped_run
    t = _twin(lambda x, nc, nd, it0: fn(A, x, eps, L, nc, nd, seed=HMC_SEED, iter0=it0), init)
    t.isbad, t.seed, t.A = isbad, HMC_SEED, A
    t.counts = N.count(N.hmc_classes(O, dtype, t.rows, isbad, eps, L, seed=HMC_SEED, matrix=A))
    return t


def _cpu_half_lg(O, dtype, dim):
    """the five classes, counted apart by the long-double classifier on x^T A x and p.p, pooled over the two (eps, L)"""
    twins = [lg_twin(O, dtype, dim, eps, L) for eps, L in LG_CASES]
    _check_counts(_pooled(twins), ("hmc lane groups", dtype.__name__, dim))
    for t, (eps, L) in zip(twins, LG_CASES):
        N.device_invariants(dtype, t.init, t.isbad, t.rows, t.acc, ("twin lg", dtype.__name__, dim, eps, L), matrix=t.A)
    return twins


@pytest.mark.parametrize("dim", [16, 32])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_lane_group_inputs(O, dtype, dim):
    _cpu_half_lg(O, dtype, dim)


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [16, 32])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_hmc_lane_groups_nonfinite(M, O, dtype, dim):
    """HMC variant 3 (16 chains per wave, reductions across the lanes of a chain, MFMA gradient) in f32 and f64 against its
    grouped twin, with energies that cross the edge in both directions: a +inf, -inf or NaN ratio must come out of the
    reductions as the rule says, and a NaN in one chain's coordinates must not reach the 15 chains that share its wave."""
    for t, (eps, L) in zip(_cpu_half_lg(O, dtype, dim), LG_CASES):
        g = M.dist.GaussianND(t.A)

        def make(init, off):
            s = M.hmc.HMC(g, init, eps, L).set_seed(t.seed)
            assert s.kernel_variant == 3
            return s.set_chain_offset(off) if off else s

        what = ("hmc lane groups", dtype.__name__, dim, eps, L)
        s = make(t.init, 0)
        out1 = s.run(*N.FIRST)
        assert same(out1, t.out1) and np.array_equal(s.accept_counts, t.acc1) and same(s.state(), t.st1), what
        out2 = s.run(N.SECOND, 0)
        assert same(out2, t.out2) and np.array_equal(s.accept_counts, t.acc2) and same(s.state(), t.st2), what
        s.close()
        s = make(t.init, 0)
        rows = np.concatenate([t.init[:, None], s.run(N.N_TRANS, 0)], axis=1)
        acc = s.accept_counts.copy()
        s.close()
        assert same(rows, t.rows) and np.array_equal(acc, t.acc), what
        N.device_invariants(dtype, t.init, t.isbad, rows, acc, what, matrix=t.A)
        for lo, hi in N.stretches(t.isbad):
            a = make(t.init[lo:hi], lo)
            assert same(a.run(N.N_TRANS, 0), rows[lo:hi, 1:]) and np.array_equal(a.accept_counts, acc[lo:hi]), (what, "alone", lo, hi)
            a.close()


# ------------------------------------------------------------------ the metric unit and scheduled runs


METRIC_EPS, METRIC_L = 0.8, 2
# steps 1.6, 0.8, 0.4 (all stable: escapes, ordinary accepts) and 0.4, 3.2, 0.8 (the second coordinate grows: the falls)
METRIC_SCALES = ((2.0, 1.0, 0.5), (0.5, 4.0, 1.0))


@functools.lru_cache(maxsize=None)
def metric_twin(O, dtype, METRIC_SCALE):
    """HMC on StandardNormal(3) under the diagonal metric s is, in y_i = x_i / s_i, HMC without a metric on the Gaussian with
    precision diag(s_i^2): the same energies, drifts y_i += eps p_i and kicks p_i -= eps s_i^2 y_i.  With powers of two for s
    every product on either side is the other's, scaled exactly (eps s_i, s_i^2 y_i = s_i x_i, y_i (s_i^2 y_i) = x_i^2), so
    the host build of the unscaled sampler, run from x / s and multiplied by s, is the metric kernel's twin bit for bit."""
    init, isbad = N.starts(O, dtype, 3)
    s = np.asarray(METRIC_SCALE, dtype=dtype)
    A = np.diag(np.asarray(METRIC_SCALE, dtype=np.float64) ** 2)
    t = _twin(lambda y, nc, nd, it0: O.engine_host_run("hmc", O.GAUSSIAN_ND, 3, [], y, METRIC_EPS, nc, nd, seed=HMC_SEED, iter0=it0,
                                                       n_leapfrog=METRIC_L, matrix=A, dtype=dtype), init / s)
    for k in ("init", "out1", "st1", "out2", "st2", "rows"):
        setattr(t, k, getattr(t, k) * s)
    assert same(t.init, init)
    t.isbad, t.seed = isbad, HMC_SEED
    t.counts = N.count(N.hmc_classes(O, dtype, t.rows, isbad, METRIC_EPS, METRIC_L, seed=HMC_SEED, scale=METRIC_SCALE))
    return t


def _cpu_half_metric(O, dtype):
    twins = [metric_twin(O, dtype, sc) for sc in METRIC_SCALES]
    _check_counts(_pooled(twins), ("hmc metric", dtype.__name__))
    for t in twins:
        N.device_invariants(dtype, t.init, t.isbad, t.rows, t.acc, ("twin metric", dtype.__name__))
    return twins


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_metric_inputs(O, dtype):
    _cpu_half_metric(O, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_hmc_metric_unit_nonfinite(M, O, dtype):
    """The metric unit (variant 7 while a metric is set), StandardNormal(3), L = 2, two sets of unequal scales: all three
    checks against the twin that metric_twin derives, all five classes counted on the CPU over the two together."""
    for t, scale in zip(_cpu_half_metric(O, dtype), METRIC_SCALES):

        def make(init, off):
            s = M.hmc.HMC(M.dist.StandardNormal(3), init, METRIC_EPS, METRIC_L).set_seed(t.seed)
            s.metric = list(scale)
            assert s.kernel_variant == 7
            return s.set_chain_offset(off) if off else s

        _device_case(make, t, dtype, ("hmc metric", dtype.__name__, scale))


SCHED = [(2.5, 1), (1.0, 1), (1.0, 10), (1.0, 2), (0.7, 3)]  # transition k takes SCHED[k % 5]; 2.5 first: while chains sit near the edge


@functools.lru_cache(maxsize=None)
def sched_twin(O, dtype, dim):
    """a scheduled run is, bit for bit, the loop `step_size = eps_k; n_leapfrog = L_k; step()`: the twin, one transition a call"""
    init, isbad = N.starts(O, dtype, dim)
    x, rows, acc = init, [init], np.zeros(len(init), dtype=np.uint64)
    for k in range(N.N_TRANS):
        eps, L = SCHED[k % len(SCHED)]
        out, x, a = O.engine_host_run("hmc", O.STANDARD_NORMAL, dim, [], x, eps, 1, 0, seed=HMC_SEED, iter0=k, n_leapfrog=L, dtype=dtype)
        rows.append(out[:, 0])
        acc += a
    t = Twin()
    t.init, t.isbad, t.rows, t.acc, t.seed = init, isbad, np.stack(rows, axis=1), acc, HMC_SEED
    eps = [SCHED[k % len(SCHED)][0] for k in range(N.N_TRANS)]
    nl = [SCHED[k % len(SCHED)][1] for k in range(N.N_TRANS)]
    t.eps, t.nl = eps, nl
    t.counts = N.count(N.hmc_classes(O, dtype, t.rows, isbad, eps, nl, seed=HMC_SEED))
    return t


def _cpu_half_sched(O, dtype, dim):
    t = sched_twin(O, dtype, dim)
    _check_counts(t.counts, ("hmc scheduled", dtype.__name__, dim))
    N.device_invariants(dtype, t.init, t.isbad, t.rows, t.acc, ("twin scheduled", dtype.__name__, dim))
    return t


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_scheduled_inputs_show_every_class(O, dtype):
    _cpu_half_sched(O, dtype, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [5, 2])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_hmc_scheduled_runs_nonfinite(M, O, dtype, variant):
    """One scheduled run each on a handle set to the split kernel (variant 5) and to the paired kernel (variant 2), (eps, L)
    changing every transition: 4 discarded, 36 collected.  Variant 2 reads the schedule on the device in both types
    (run_hmc_pp_sched); variant 5 does so in f32 only (run_hmc_split_sched has no f64 instance): the f64 case takes the
    segmented path, one unscheduled split launch per stretch of equal (eps, L) -- here one per transition."""
    dim = 3
    t = _cpu_half_sched(O, dtype, dim)
    what = ("hmc scheduled", dtype.__name__, "variant", variant)

    def make(init, off):
        s = M.hmc.HMC(M.dist.StandardNormal(dim), init, 1.0, 1).set_seed(t.seed).set_kernel_variant(variant)
        return s.set_chain_offset(off) if off else s

    s = make(t.init, 0)
    out = s.run_scheduled(t.eps, t.nl, N.N_TRANS - N.FIRST[1])
    assert same(out, t.rows[:, 1 + N.FIRST[1]:]) and np.array_equal(s.accept_counts, t.acc) and same(s.state(), t.rows[:, -1]), what
    s = make(t.init, 0)
    rows = np.concatenate([t.init[:, None], s.run_scheduled(t.eps, t.nl, N.N_TRANS)], axis=1)
    acc = s.accept_counts.copy()
    assert same(rows, t.rows) and np.array_equal(acc, t.acc), what
    N.device_invariants(dtype, t.init, t.isbad, rows, acc, what)
    for lo, hi in N.stretches(t.isbad):
        a = make(t.init[lo:hi], lo)
        assert same(a.run_scheduled(t.eps, t.nl, N.N_TRANS), rows[lo:hi, 1:]) and np.array_equal(a.accept_counts, acc[lo:hi]), (what, lo, hi)
