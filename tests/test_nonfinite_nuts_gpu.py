"""NUTS on the device from far starts and from starts whose log-density is not real.

tests/test_nonfinite_host.py shows on the host build that the step-size search ends and that a chain without a real
log-density stays where it started.  Here the device is held to the same, on every kernel path of the handles below --
every variant a one-chain-per-lane handle accepts (0 lanes in step, 4 asynchronous lanes, 5 leaves in pairs, 6 run-time
dimension, 7 the run-time compiled unit) and the lane-group variants 1 and 2 -- in the type modes each has, three ways:

  1. bit equality with the host twin: samples, positions, leapfrog counts and the four adaptation values, as integers, over a
     run(6, 4) continued by a run(5, 0);
  2. from the device's output alone: the depth histogram counts every transition once and is the same on every variant; a
     chain that started finite holds no NaN / inf and has a real, positive step size; a chain that started at NaN, +-inf or
     at a finite point where the density overflows keeps its start bits in every row and makes one leapfrog per transition
     (one doubling of one leaf);
  3. neighbour independence: the healthy chains equal, bit for bit, the run of those chains alone at their chain offsets,
     and the histograms add up.

Case (a): far-but-finite starts (the search's halving loop is entered and ends on its own) and a stiff f32 target, max_depth
10.  Case (b): the non-real starts, max_depth 3, at most 70 chains, mixed with healthy ones.

Lane-group variant 3, the persistent scheduler, launches what variant 1 launches below 2048 chains.  It therefore has a
case (a) of its own, 2069 chains; case (b) is held to at most 70 chains, where it would repeat variant 1, so the scheduler
is NOT covered from starts without a real log-density.

The twin runs in a child process under a time limit (the helper of tests/test_nonfinite_host.py): if the search stopped
ending, these tests would fail, not hang.
"""
import functools
import pathlib
import tempfile

import numpy as np
import pytest

import nonfinite_common as N
import test_nonfinite_host as H

SEED = 41
RUN1, RUN2 = (6, 4), 5
KNOWN_VARIANTS = set(range(8))


@pytest.fixture(scope="module")
def M():
    import mini_mcmc_amd
    from mini_mcmc_amd import core, distributions

    mini_mcmc_amd.lib()

    class NS:
        pass

    ns = NS()
    ns.core, ns.dist = core, distributions
    return ns


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(N.bits(a), N.bits(b))


def _spd(dim):
    from mini_mcmc_amd.distributions import GaussianND

    return GaussianND.ill_conditioned(dim, 50.0, 7).precision


class Case:
    """target: (distributions class name, constructor arguments); okind: (oracle kind name, params); twin_mode(mode): the
    host twin's mode for the handle's type mode (3: the lane-group twin; dimensions without a fixed instance fall through to
    the run-time-dimension twin by themselves)."""

    def __init__(self, name, target, okind, dim, modes, variants, twin_mode=lambda m: m, matrix=None, every=True, n_a=66, which="ab"):
        self.name, self.target, self.okind, self.dim, self.modes, self.variants = name, target, okind, dim, modes, variants
        self.twin_mode, self.matrix = twin_mode, matrix
        # every: also run whatever else the handle accepts (one chain per lane: all variants share the twin); n_a: chains of
        # case (a); which: the cases the handle takes part in
        self.every, self.n_a, self.which = every, n_a, which

    def make_target(self, M):
        cls, args = self.target
        return getattr(M.dist, cls)(*args)


CASES = [
    Case("rosenbrock3", ("RosenbrockND", (3,)), ("ROSENBROCK_ND", []), 3, (0, 1, 2), (0, 4, 5, 6)),
    Case("stiff4", ("IsotropicGaussian", (1e-3, 4)), ("ISOTROPIC_GAUSSIAN", [1e-3]), 4, (0, 1), (0, 4, 5)),
    Case("rosenbrock11", ("RosenbrockND", (11,)), ("ROSENBROCK_ND", []), 11, (0, 1, 2), (6, 7)),
    # lane groups: the one-chain-per-lane variants these handles also accept sum in another order (another twin): not run here.
    # Below 2048 chains variant 3 launches what variant 1 launches (mm_nuts_api.hip), so the small cases leave it out ...
    Case("gauss16", ("GaussianND", (_spd(16),)), ("GAUSSIAN_ND", []), 16, (2,), (1, 2), lambda m: 3, _spd(16), every=False),
    Case("gauss32", ("GaussianND", (_spd(32),)), ("GAUSSIAN_ND", []), 32, (2,), (1, 2), lambda m: 3, _spd(32), every=False),
    # ... and the persistent scheduler gets a case (a) of its own size: 2069 chains = 129 groups of 16 and five
    Case("gauss16-scheduler", ("GaussianND", (_spd(16),)), ("GAUSSIAN_ND", []), 16, (2,), (3,), lambda m: 3, _spd(16), every=False,
         n_a=2069, which="a"),
]
CASE_MODES = [(c, m) for c in CASES for m in c.modes]
_ids = lambda cm: f"{cm[0].name}-mode{cm[1]}"


def _far(case, mode, n):
    """case (a): n chains (a ragged wave / lane group), some of them far away"""
    x = _init_rows(n, case.dim) * (1.0 if case.name == "stiff4" else 0.5)  # stiff4: every start is 1000 sigma out
    f32 = mode < 2
    if case.name.startswith("rosenbrock"):
        alt = np.where(np.arange(case.dim) % 2 == 0, 1.0, -1.0)
        x[1], x[n // 2], x[n - 1] = 30.0 * alt, -30.0 * alt, (1e6 if f32 else 1e40) * alt
    if case.name.startswith("gauss"):
        x[1] *= 1e6
        x[n - 1] *= 1e12
    return x, np.zeros(n, dtype=bool)


def _init_rows(n, dim):
    import oracle as O

    return O.init_with_seed(n, dim, 31).astype(np.float64)


def _bad(case, mode, n_good):
    """case (b): healthy chains with a NaN, a +inf, a -inf and an overflowing start among them"""
    good = _init_rows(n_good, case.dim) * (1.0 if case.name == "stiff4" else 0.5)
    at = (2, 17, n_good // 2 + 1, n_good + 3)
    rows = np.empty((n_good + 4, case.dim))
    isbad = np.zeros(n_good + 4, dtype=bool)
    isbad[list(at)] = True
    rows[~isbad] = good
    for k, (c, v) in enumerate(zip(at, (np.nan, np.inf, -np.inf, 1e20 if mode < 2 else 1e200))):
        rows[c] = np.linspace(-0.9, 1.1, case.dim)
        rows[c, (k * 5 + 1) % case.dim] = v
    return rows, isbad


class Twin:
    pass


@functools.lru_cache(maxsize=None)
def twin(O, case, mode, which):
    t = Twin()
    t.init, t.isbad = _far(case, mode, case.n_a) if which == "a" else _bad(case, mode, 63)
    t.max_depth = 10 if which == "a" else 3

    def run(x, nc, nd, m0, adapt):
        # in a child process under a time limit, like tests/test_nonfinite_host.py: a search that does not end fails the test
        spec = H._run(case.twin_mode(mode), case.okind[0], case.dim, x, seed=SEED, max_depth=t.max_depth, matrix=case.matrix,
                      n_collect=nc, n_discard=nd, params=case.okind[1], m0=m0, adapt=adapt, n_threads=8 if len(x) > 256 else 1)
        with tempfile.TemporaryDirectory() as d:
            r = H._run_child(pathlib.Path(d), [spec], f"nuts_{case.name}_{mode}_{which}_{m0}")[0]
        return r["sample"], r["pos"], r["adapt"], r["nlf"]

    t.out1, t.pos1, t.ad1, t.nlf1 = run(t.init, RUN1[0], RUN1[1], 0, None)
    t.out2, t.pos2, t.ad2, t.nlf2 = run(t.pos1, RUN2, 0, RUN1[0] + RUN1[1] - 1, t.ad1)
    t.n_trans = (RUN1[0] + RUN1[1] - 1, RUN2 - 1)  # run() makes N - 1 transitions (nuts.rs:163-170)
    # the twin itself keeps the invariants (check 2 on the host build)
    _invariants(t, t.out1, t.out2, t.pos2, t.ad2, t.nlf1 + t.nlf2, None, (case.name, mode, which, "twin"))
    return t


def _invariants(t, out1, out2, pos, ad, nlf, hist, what):
    tdt = out1.dtype.type
    start = t.init.astype(tdt)
    good, n_trans = ~t.isbad, sum(t.n_trans)
    rows = np.concatenate([out1, out2], axis=1)
    assert np.isfinite(rows[good]).all() and np.isfinite(pos[good]).all(), (what, "NaN or inf in a chain that started finite")
    assert np.isfinite(ad[good]).all() and (ad[good, 0] > 0).all(), (what, "adaptation state of a healthy chain")
    b = N.bits(start)[t.isbad]
    assert (N.bits(rows)[t.isbad] == b[:, None, :]).all() and (N.bits(pos)[t.isbad] == b).all(), (what, "a bad chain moved")
    assert (nlf[t.isbad] == n_trans).all(), (what, "a bad chain's tree went past its first leaf", nlf[t.isbad])
    assert (nlf[good] >= n_trans).all(), what
    if hist is not None:
        assert int(hist.sum()) == len(t.init) * n_trans, (what, "depth histogram", hist)
        assert hist[0] == 0 and hist[1] >= int(t.isbad.sum()) * n_trans, (what, "depth histogram", hist)  # index: doublings made


def _device(M, case, mode, t, variant, init, offset=0):
    from mini_mcmc_amd.nuts import NUTS

    s = NUTS(case.make_target(M), init, 0.8, mode=mode).set_seed(SEED).set_max_depth(t.max_depth)
    if offset:
        s.set_chain_offset(offset)
    s.set_kernel_variant(variant)
    out1 = s.run(*RUN1)
    a1 = s.adapt_state()
    pos1, nlf1 = s.positions(), s.leapfrog_counts().copy()
    out2 = s.run(RUN2, 0)
    a2 = s.adapt_state()
    ad = lambda a: np.stack([a["epsilon"], a["epsilon_bar"], a["h_bar"], a["mu"]], axis=1)
    res = dict(out1=out1, pos1=pos1, ad1=ad(a1), nlf1=nlf1, out2=out2, pos2=s.positions(), ad2=ad(a2),
               nlf=s.leapfrog_counts().copy(), hist=s.depth_histogram().copy())
    s.close()
    return res


def _accepted_variants(M, case, mode, init):
    from mini_mcmc_amd.nuts import NUTS

    from mini_mcmc_amd import _lib as L

    got = set()
    for v in range(-1, 12):
        s = NUTS(case.make_target(M), init[:4], 0.8, mode=mode)
        try:
            s.set_kernel_variant(v)
            got.add(v)
        except L.MmcmcError as e:  # a refusal is one of these two; anything else is a failure of the test
            assert e.status in (L.ERR_INVALID_ARG, L.ERR_UNSUPPORTED), (case.name, mode, v, e)
        finally:
            s.close()
    assert set(case.variants) <= got and got <= KNOWN_VARIANTS, (case.name, mode, got)
    return tuple(sorted(got)) if case.every else tuple(case.variants)


def _three_checks(M, O, case, mode, which):
    t = twin(O, case, mode, which)
    variants = _accepted_variants(M, case, mode, t.init)
    hists = {}
    for v in variants:
        what = (case.name, "mode", mode, which, "variant", v)
        d = _device(M, case, mode, t, v, t.init)
        # 1. the host twin
        assert same(d["out1"], t.out1) and same(d["pos1"], t.pos1), (what, "run 1")
        assert np.array_equal(d["nlf1"], t.nlf1), (what, "leapfrog counts of run 1")
        assert same(d["ad1"], t.ad1), (what, "adaptation state after run 1")
        assert same(d["out2"], t.out2) and same(d["pos2"], t.pos2) and same(d["ad2"], t.ad2), (what, "continued run")
        assert np.array_equal(d["nlf"], t.nlf1 + t.nlf2), (what, "leapfrog counts")
        # 2. the device alone
        _invariants(t, d["out1"], d["out2"], d["pos2"], d["ad2"], d["nlf"], d["hist"], what)
        hists[v] = d["hist"]
        # 3. the healthy chains alone
        total = np.zeros_like(d["hist"])
        ranges = N.stretches(t.isbad) if t.isbad.any() else [(0, 20), (20, len(t.init))]  # 20: a ragged lane group
        for lo, hi in ranges:
            a = _device(M, case, mode, t, v, t.init[lo:hi], lo)
            for k in ("out1", "out2", "pos2", "ad2", "nlf"):
                assert same(a[k], d[k][lo:hi]), (what, "alone", lo, hi, k)
            total += a["hist"]
        total[1] += int(t.isbad.sum()) * sum(t.n_trans)  # a bad chain's transitions: one doubling of one leaf
        assert np.array_equal(total, d["hist"]), (what, "histograms of the parts", total, d["hist"])
    for v in variants[1:]:
        assert np.array_equal(hists[v], hists[variants[0]]), (case.name, mode, which, "histogram of variant", v)


@pytest.mark.parametrize("cm", CASE_MODES, ids=_ids)
def test_twin_keeps_the_invariants(O, cm):
    """The CPU half: on both sets of starts the host build returns and keeps what check 2 asks of the device."""
    for which in cm[0].which:
        twin(O, cm[0], cm[1], which)


@pytest.mark.gpu
@pytest.mark.parametrize("cm", [cm for cm in CASE_MODES if "a" in cm[0].which], ids=_ids)
def test_nuts_far_starts_and_stiff_target(M, O, cm):
    """Case (a)."""
    _three_checks(M, O, cm[0], cm[1], "a")


@pytest.mark.gpu
@pytest.mark.parametrize("cm", [cm for cm in CASE_MODES if "b" in cm[0].which], ids=_ids)
def test_nuts_nonreal_starts(M, O, cm):
    """Case (b): 67 chains, four of them without a real log-density."""
    _three_checks(M, O, cm[0], cm[1], "b")
