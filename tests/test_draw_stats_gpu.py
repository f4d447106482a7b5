"""NUTS's per-draw statistics on the device (include/mmcmc.h: "Per-draw sampler statistics").

96 chains throughout: one full wave and one partial wave.  Every comparison of a sampler's output is exact -- recording
changes which kernels run, never an operation of a chain -- and the reference of the records is the host twin
(tests/cpp/draw_stats_twin.cpp).  Only the summary's floats have a tolerance (test_summary_*).

Units compiled here, once per process: the stats units of RosenbrockND(3) without a metric, with a diagonal and with a dense
one, of Gaussian2D (the forced divergence) and of one autodiff kind at dim 3.  That a unit's pair kernel and its lanes-in-step
kernel write the same records is checked by the library itself before mmcmc_nuts_set_draw_stats returns MMCMC_OK
(mm_nuts_api.hip: unit_verified, where the referee is trusted); the tests here see it as that return value."""
import numpy as np
import pytest

import autodiff_common as A
import draw_stats_common as DS

pytestmark = pytest.mark.gpu
N, SEED = 96, 13
HOWS = {"run_10_20": (10, 20, False), "run_10_0": (10, 0, False), "run_progress_10_20": (10, 20, True)}
WHAT = ("samples", "positions", "adaptation records", "leapfrog counts", "depth histogram")
_cache = {}


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _rosen(mode, metric="none"):
    from mini_mcmc_amd.distributions import RosenbrockND
    from mini_mcmc_amd.nuts import NUTS

    h = NUTS(RosenbrockND(3), DS.start(N, 3), 0.8, mode=mode).set_seed(SEED)
    _set_metric(h, metric)
    return h


def _set_metric(h, metric):
    if metric == "diag":
        h.metric = DS.DIAG
    elif metric == "dense":
        h.metric_chol = DS.CHOL


def _all(h, how):
    """everything a NUTS run leaves behind"""
    n_collect, n_discard, progress = HOWS[how]
    sample = h.run_progress(n_collect, n_discard)[0] if progress else h.run(n_collect, n_discard)
    ad = h.adapt_state()
    return sample, h.positions(), np.stack([ad[k] for k in ("epsilon", "epsilon_bar", "h_bar", "mu")], axis=1), h.leapfrog_counts(), h.depth_histogram()


def _pair(mode, how, metric="none"):
    """(what a fresh handle with recording off leaves, what one with recording on leaves, its records, the variant before,
    what each leaves after one more run with recording switched off again): computed once"""
    key = (mode, how, metric)
    if key not in _cache:
        off, on = _rosen(mode, metric), _rosen(mode, metric)
        before = on.kernel_variant
        assert not on.draw_stats_enabled
        on.set_draw_stats()
        assert on.draw_stats_enabled and on.kernel_variant == 7
        r_off, r_on = _all(off, how), _all(on, how)
        rec = on.draw_stats()
        on.set_draw_stats(False)
        after = on.kernel_variant
        _cache[key] = (r_off, r_on, rec, before, after, _all(off, how), _all(on, how))
        off.close()
        on.close()
    return _cache[key]


# ------------------------------------------------------------------------------------------------ 7: on equals off

@pytest.mark.parametrize("how", list(HOWS))
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_recording_on_equals_off_and_off_again_is_the_former_variant(mode, how):
    r_off, r_on, rec, before, after, again_off, again_on = _pair(mode, how)
    for u, v, what in zip(r_off, r_on, WHAT):
        assert _bits_equal(u, v), (mode, how, what)
    assert rec.shape == (N, HOWS[how][0]) and rec.dtype == DS.DRAW
    assert before == 5 and after == before  # RosenbrockND(3): the pair kernel of the compiled instance
    for u, v, what in zip(again_off, again_on, WHAT):
        assert _bits_equal(u, v), (mode, how, what, "after switching off")
    assert r_off[3].sum() > 0 and not _bits_equal(r_off[0][:, 0], r_off[0][:, -1])


# ------------------------------------------------------------------------------------------------ 8: the host twin

@pytest.mark.parametrize("how", list(HOWS))
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_device_records_are_the_twins_byte_for_byte(tmp_path_factory, mode, how):
    n_collect, n_discard, progress = HOWS[how]
    ref = DS.twin_nuts(tmp_path_factory, mode, N, n_collect, n_discard, progress, SEED)
    _, r_on, rec, *_ = _pair(mode, how)
    assert _bits_equal(r_on[0], ref[0]) and _bits_equal(r_on[1], ref[1]), (mode, how)
    assert _bits_equal(rec, ref[5]), (mode, how, np.argwhere(rec != ref[5])[:5])
    if how == "run_10_0":  # row 0 is the initial position: the no-transition record, the current epsilon in it
        assert np.all(rec["tree"][:, 0] == DS.NONE) and np.all(np.isnan(rec["energy"][:, 0])) and np.all(np.isnan(rec["accept_stat"][:, 0]))
        assert np.all(rec["step_size"][:, 0] > 0)
    else:
        assert np.all(rec["tree"] >> np.uint32(31) == 0)


# ------------------------------------------------------------------------------------------------ 9: self-consistency

@pytest.mark.parametrize("mode", [0, 1, 2])
def test_records_add_up_to_the_handles_counters(mode):
    from mini_mcmc_amd.nuts import unpack_tree

    h = _rosen(mode).set_draw_stats()
    h.run(4, 3)  # counters that do not start at zero
    lf0, hist0 = h.leapfrog_counts(), h.depth_histogram()
    m0 = h.stream_position()[2]
    h.run(10, 0)
    n_lf, depth, _, _, transition = unpack_tree(h.draw_stats()["tree"])
    assert transition[:, 1:].all() and not transition[:, 0].any() and h.stream_position()[2] == m0 + 9
    assert np.array_equal(n_lf.sum(axis=1).astype(np.uint64), h.leapfrog_counts() - lf0)
    assert np.array_equal(np.bincount(depth[transition], minlength=13).astype(np.uint32), h.depth_histogram() - hist0)
    h.close()


# ------------------------------------------------------------------------------------------------ 10: divergence

@pytest.mark.parametrize("eps", [64.0, 0.1], ids=["forced", "absent"])
def test_divergence_forced_and_absent_is_the_twins(tmp_path_factory, eps):
    from mini_mcmc_amd.distributions import Gaussian2D
    from mini_mcmc_amd.nuts import NUTS, unpack_tree

    rows = 20
    ref = DS.twin_gauss(tmp_path_factory, 0, N, rows, eps, 7)
    x0 = DS.start(N, 2)
    h = NUTS(Gaussian2D([0.0, 0.0], [[1.0, 0.0], [0.0, 1.0]]), x0, 0.8, mode=0).set_seed(7).set_draw_stats()
    h.set_adapt_state(np.tile([eps, eps, 0.0, np.log(10.0)], (N, 1)))
    sample = h.run(rows, 0)
    rec = h.draw_stats()
    assert _bits_equal(sample, ref[0]) and _bits_equal(rec, ref[5])
    n_lf, depth, divergent, _, transition = unpack_tree(rec["tree"])
    if eps == 64.0:  # every transition leaves the slice at its first leaf, and no chain moves
        assert divergent[:, 1:].all() and np.all(depth[:, 1:] == 1) and np.all(n_lf[:, 1:] == 1)
        assert np.all(sample == x0.astype(np.float32)[:, None, :]) and np.all(rec["step_size"] == 64.0)
    else:
        assert not divergent.any() and transition[:, 1:].all() and not np.all(sample == sample[:, :1])
    h.close()


# ------------------------------------------------------------------------------------------------ 11: metrics, a user kind

@pytest.mark.parametrize("metric", ["diag", "dense"])
@pytest.mark.parametrize("mode", [0, 2])
def test_with_a_metric_on_equals_off_records_are_the_twins_and_the_setters_commute(tmp_path_factory, mode, metric):
    how = "run_10_20"
    r_off, r_on, rec, before, after, again_off, again_on = _pair(mode, how, metric)
    for u, v, what in zip(r_off, r_on, WHAT):
        assert _bits_equal(u, v), (mode, metric, what)
    for u, v, what in zip(again_off, again_on, WHAT):
        assert _bits_equal(u, v), (mode, metric, what, "after switching off")
    assert before == 7 and after == 7  # the metric's unit before, and again after
    ref = DS.twin_nuts(tmp_path_factory, mode, N, 10, 20, False, SEED, metric)
    assert _bits_equal(r_on[0], ref[0]) and _bits_equal(rec, ref[5])
    assert not _bits_equal(rec, _pair(mode, how)[2])  # the metric changes the trajectories
    # recording first, the metric after: the same bits; clearing the metric keeps recording, clearing both gives variant 5 back
    h = _rosen(mode).set_draw_stats()
    _set_metric(h, metric)
    assert h.kernel_variant == 7 and h.draw_stats_enabled
    got = _all(h, how)
    for u, v, what in zip(r_on, got, WHAT):
        assert _bits_equal(u, v), (mode, metric, what, "metric set after recording")
    assert _bits_equal(h.draw_stats(), rec)
    if metric == "diag":
        h.metric = None
    else:
        h.metric_chol = None
    assert h.kernel_variant == 7 and h.draw_stats_enabled and h.metric is None
    h.set_draw_stats(False)
    assert h.kernel_variant == 5
    h.close()
    h = _rosen(mode, metric).set_draw_stats()  # the other order of leaving: recording off first, then the metric
    h.set_draw_stats(False)
    assert h.kernel_variant == 7
    h.metric = None
    assert h.kernel_variant == 5
    h.close()


def test_autodiff_kind_on_equals_off_and_its_records_add_up():
    from mini_mcmc_amd.distributions import AutodiffTarget
    from mini_mcmc_amd.nuts import NUTS, unpack_tree

    tgt = AutodiffTarget("draw_stats_rosen3_ad", 3, A.case_source("rosenbrock3")[0])
    make = lambda: NUTS(tgt, DS.start(N, 3), 0.8, mode=0).set_seed(SEED)  # noqa: E731
    off, on = make(), make()
    before = on.kernel_variant
    on.set_draw_stats()
    assert on.kernel_variant == 7
    lf0 = on.leapfrog_counts()
    r_off, r_on = _all(off, "run_10_0"), _all(on, "run_10_0")
    for u, v, what in zip(r_off, r_on, WHAT):
        assert _bits_equal(u, v), what
    rec = on.draw_stats()
    n_lf, _, _, _, transition = unpack_tree(rec["tree"])
    assert np.array_equal(n_lf.sum(axis=1).astype(np.uint64), on.leapfrog_counts() - lf0) and transition[:, 1:].all()
    assert np.all(np.isfinite(rec["energy"][:, 1:])) and np.all((rec["accept_stat"][:, 1:] >= 0) & (rec["accept_stat"][:, 1:] <= 1))
    on.set_draw_stats(False)
    assert on.kernel_variant == before
    off.close()
    on.close()


# ------------------------------------------------------------------------------------------------ 12: refusals

def test_refusals_change_nothing():
    from mini_mcmc_amd import _lib as L
    from mini_mcmc_amd.core import init_with_seed
    from mini_mcmc_amd.distributions import IsotropicGaussian, RosenbrockND
    from mini_mcmc_amd.group import NUTSGroup
    from mini_mcmc_amd.nuts import NUTS

    lib = L.lib()
    x33 = init_with_seed(N, 33, 42)
    a, b = NUTS(IsotropicGaussian(1.0, 33), x33, 0.8).set_seed(3), NUTS(IsotropicGaussian(1.0, 33), x33, 0.8).set_seed(3)
    v = b.kernel_variant
    assert lib.mmcmc_nuts_set_draw_stats(b._h, 1) == L.ERR_UNSUPPORTED
    assert not b.draw_stats_enabled and b.kernel_variant == v
    assert lib.mmcmc_nuts_draw_stats(b._h, None, 0, None) == L.ERR_SHAPE
    assert _bits_equal(a.run(6, 3), b.run(6, 3))
    a.close()
    b.close()
    x0 = DS.start(N, 3)
    g, one = NUTSGroup(RosenbrockND(3), x0, 0.8, devices=[0]).set_seed(SEED), _rosen(0)
    assert lib.mmcmc_nuts_group_set_draw_stats(g._h, 1) == L.ERR_UNSUPPORTED
    with pytest.raises(L.MmcmcError):
        g.set_draw_stats()
    assert _bits_equal(g.run(6, 3), one.run(6, 3))
    g.close()
    h = _rosen(0).set_draw_stats()
    assert lib.mmcmc_nuts_set_kernel_variant(h._h, 2) == L.ERR_UNSUPPORTED and lib.mmcmc_nuts_set_kernel_variant(h._h, 0) == L.ERR_UNSUPPORTED
    assert lib.mmcmc_nuts_set_kernel_variant(h._h, 7) == L.OK and lib.mmcmc_nuts_set_kernel_variant(h._h, 99) == L.ERR_INVALID_ARG
    assert h.kernel_variant == 7 and h.draw_stats_enabled
    assert lib.mmcmc_nuts_draw_stats(h._h, None, 0, None) == L.ERR_SHAPE  # no run yet
    h.close()
    one.close()


def test_a_refused_variant_leaves_the_next_run_untouched():
    from mini_mcmc_amd import _lib as L

    h, ref = _rosen(0).set_draw_stats(), _rosen(0)
    assert L.lib().mmcmc_nuts_set_kernel_variant(h._h, 2) == L.ERR_UNSUPPORTED
    assert _bits_equal(h.run(6, 3), ref.run(6, 3)) and h.draw_stats().shape == (N, 6)
    h.close()
    ref.close()


# ------------------------------------------------------------------------------------------------ 13: the reduction

def _synthetic(n_chains, n_rows, seed):
    """energies f32 normal(50, 3), random flag bits, depth and leapfrogs, a no-transition record in row 0 of some chains"""
    rng = np.random.default_rng(seed)
    rec = np.zeros((n_chains, n_rows), dtype=DS.DRAW)
    rec["energy"] = rng.normal(50.0, 3.0, size=(n_chains, n_rows)).astype(np.float32)
    rec["accept_stat"] = rng.random((n_chains, n_rows)).astype(np.float32)
    rec["step_size"] = (0.01 + rng.random((n_chains, n_rows))).astype(np.float32)
    depth = rng.integers(1, 13, size=(n_chains, n_rows)).astype(np.uint32)
    n_lf = rng.integers(1, 4096, size=(n_chains, n_rows)).astype(np.uint32)
    flags = rng.integers(0, 4, size=(n_chains, n_rows)).astype(np.uint32)
    rec["tree"] = n_lf | (depth << np.uint32(16)) | (flags << np.uint32(24))
    none = np.arange(n_chains) % 3 == 0
    rec["tree"][none, 0] = DS.NONE
    rec["energy"][none, 0] = np.nan
    rec["accept_stat"][none, 0] = np.nan
    return rec


def _check_summary(got, rec):
    want = DS.summary_f64(rec)
    for k in ("n_transitions", "n_divergent", "n_depth_cap", "max_depth_seen", "n_leapfrog"):
        assert np.array_equal(getattr(got, k).astype(np.uint64), want[k].astype(np.uint64)), k
    for k in ("mean_accept", "mean_step", "ebfmi"):
        g, w = getattr(got, k), want[k]
        with np.errstate(invalid="ignore", divide="ignore"):
            print(k, "largest relative difference", np.nanmax(np.abs(g - w) / np.abs(w)) if np.isfinite(w).any() else "-", "of", g.size)
        assert np.array_equal(np.isnan(g), np.isnan(w)), (k, g, w)  # NaN exactly where defined
        assert np.allclose(g[~np.isnan(w)], w[~np.isnan(w)], rtol=1e-9, atol=0), k


@pytest.mark.parametrize("n_chains", [1, 65])
@pytest.mark.parametrize("n_rows", [1, 2, 3, 63, 64, 65, 4097])
def test_summary_of_synthetic_records_from_host_and_from_device_memory(n_rows, n_chains):
    """the shapes at which a one-wave-per-chain strided loop with a carried neighbour can go wrong: an empty or single-trip
    chain, the trip boundary, a partial last trip, a partial grid.  rtol 1e-9: sums of at most 4097 non-negative float64 terms
    with at most three roundings each bound the error near 2e-12; the rest of the margin is for the reduction order."""
    import torch

    from mini_mcmc_amd import stats as S

    rec = _synthetic(n_chains, n_rows, 100 * n_rows + n_chains)
    from_host = S.nuts_summary(rec)
    _check_summary(from_host, rec)
    dev = torch.from_numpy(rec.view(np.uint8).reshape(n_chains, n_rows, 16).copy()).cuda()
    from_device = S.nuts_summary(dev)
    for k in ("n_transitions", "n_divergent", "n_depth_cap", "max_depth_seen", "n_leapfrog", "mean_accept", "mean_step", "ebfmi"):
        assert _bits_equal(getattr(from_host, k), getattr(from_device, k)), k
    want = DS.summary_f64(rec)
    assert from_host.total_transitions == int(want["n_transitions"].sum()) and from_host.total_divergent == int(want["n_divergent"].sum())
    if n_rows == 1:  # fewer than two transitions: no E-BFMI; a chain whose one row is no transition has no means either
        assert np.all(np.isnan(from_host.ebfmi)) and np.isnan(from_host.mean_accept[0]) and from_host.n_transitions[0] == 0
    if np.all(np.isnan(want["ebfmi"])):  # also 2 rows of which row 0 is no transition, in a lone chain
        assert from_host.min_ebfmi_chain == -1 and np.isnan(from_host.min_ebfmi)
    else:
        assert from_host.min_ebfmi_chain == int(np.nanargmin(want["ebfmi"])) and from_host.min_ebfmi == from_host.ebfmi[from_host.min_ebfmi_chain]


@pytest.mark.parametrize("how", list(HOWS))
def test_summary_of_real_records(how):
    from mini_mcmc_amd import stats as S

    rec = _pair(0, how)[2]
    got = S.nuts_summary(rec)
    _check_summary(got, rec)
    assert got.total_transitions == N * (9 if how == "run_10_0" else 10) and 0.0 <= got.divergent_share <= 1.0
