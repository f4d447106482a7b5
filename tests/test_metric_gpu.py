"""The diagonal metric of HMC and NUTS on the device (include/mmcmc.h: "A diagonal mass matrix").

Chain counts throughout: 1, 63, 64, 65, 130 -- a lone lane, a partial wave, a full wave, waves with a tail.  Every comparison
but the last test's statistics is exact: a metric changes which numbers are multiplied, never the order of the operations.

  * a metric of ones gives the bits of no metric, through the C ABI, on built-in, autodiff and data-bound targets;
  * the power-of-two identity of tests/cpp/metric_twin.cpp on the device, the constants baked into the functor's source;
  * the device against the host twin at scales that are not powers of two (level C of DESIGN.md 4);
  * the contract's edges: refusals, the variant while a metric is set and after, scheduled runs, run_progress, checkpoints;
  * warmup_nuts on an axis-aligned Gaussian with scales from 1e-2 to 1e2."""
import ctypes as C

import numpy as np
import pytest

import autodiff_common as A
import data_common as D
import metric_common as M

pytestmark = pytest.mark.gpu
CHAINS = [1, 63, 64, 65, 130]
_made = {}


def _once(key, make):
    if key not in _made:
        _made[key] = make()
    return _made[key]


def _rosen9_autodiff():
    from mini_mcmc_amd.distributions import AutodiffTarget

    return _once("rosen9", lambda: AutodiffTarget("metric_rosen9_ad", 9, A.case_source("rosenbrock9")[0]))


def _logit9():
    from mini_mcmc_amd.distributions import AutodiffTarget

    dim, data, params = D.MODELS["logit9"]
    return _once("logit9", lambda: AutodiffTarget("metric_logit9_logp", dim, D.source("logit9", "logp"), params=params, data=data))


def _quad_source(c):
    """logp = -1/2 sum (x_i c_i)^2, g_i = -(x_i c_i) c_i with the constants in the source text"""
    consts = ", ".join(f"T({float(v)!r})" for v in c)
    body = f"const T c[dim] = {{{consts}}};\n        T s = 0;\n        MM_UNROLL\n        for (int i = 0; i < dim; ++i) {{ const T t = x[i] * c[i]; s = mm_fma(t, t, s); %s}}\n        return T(-0.5) * s;"
    return ("template <class T> struct mmcmc_user_target {\n"
            f"    static constexpr int dim = {len(c)};\n"
            "    MM_HD static T logp(const mm_tparams<T> &, const T *x) {\n        " + body % "" + "\n    }\n"
            "    MM_HD static T logp_grad(const mm_tparams<T> &, const T *x, T *g) {\n        " + body % "g[i] = -t * c[i]; " + "\n    }\n"
            "};\n")


def _quad(name, c):
    from mini_mcmc_amd.distributions import UserTarget

    return _once(name, lambda: UserTarget(name, len(c), _quad_source(c)))


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _nuts_all(s, n_collect, n_discard):
    """everything a NUTS run leaves behind"""
    sample = s.run(n_collect, n_discard)
    ad = s.adapt_state()
    return sample, s.positions(), np.stack([ad[k] for k in ("epsilon", "epsilon_bar", "h_bar", "mu")], axis=1), s.leapfrog_counts(), s.depth_histogram()


# ------------------------------------------------------------------------------------------------ 5: ones = none

@pytest.mark.parametrize("n", CHAINS)
def test_ones_metric_is_no_metric_hmc(n):
    from mini_mcmc_amd.core import init_with_seed
    from mini_mcmc_amd.distributions import Gaussian2D, RosenbrockND
    from mini_mcmc_amd.hmc import HMC

    cases = [("RosenbrockND(3) f32", RosenbrockND(3), np.float32, 3, 0.032),
             ("Gaussian2D f64", Gaussian2D([0.0, 1.0], [[4.0, 2.0], [2.0, 3.0]]), np.float64, 2, 0.3),
             ("autodiff RosenbrockND(9) f32", _rosen9_autodiff(), np.float32, 9, 0.02),
             ("autodiff RosenbrockND(9) f64", _rosen9_autodiff(), np.float64, 9, 0.02)]
    for what, tgt, dt, dim, eps in cases:
        x0 = (0.5 * init_with_seed(n, dim, 42)).astype(dt)
        a = HMC(tgt, x0, eps, 7).set_seed(9)
        b = HMC(tgt, x0, eps, 7).set_seed(9)
        plain = b.kernel_variant
        assert b.metric is None
        b.metric = np.ones(dim)
        assert b.kernel_variant == 7 and np.array_equal(b.metric, np.ones(dim))
        sa, sb = a.run(24, 7), b.run(24, 7)
        assert _bits_equal(sa, sb), what
        assert _bits_equal(a.state(), b.state()) and np.array_equal(a.accept_counts, b.accept_counts), what
        assert a.accept_counts.sum() > 0 and not np.array_equal(sa[:, 0], sa[:, -1]), what
        b.metric = None
        assert b.metric is None and b.kernel_variant == plain, what
        assert _bits_equal(a.run(6, 1), b.run(6, 1)), what  # ... and the bits of no metric again after NULL
        a.close()
        b.close()


@pytest.mark.parametrize("n", CHAINS)
def test_ones_metric_is_no_metric_nuts(n):
    from mini_mcmc_amd.core import init_with_seed
    from mini_mcmc_amd.distributions import RosenbrockND
    from mini_mcmc_amd.nuts import NUTS

    cases = [(RosenbrockND(3), 3, m) for m in (0, 1, 2)] + [(_logit9(), 9, 2)]
    for tgt, dim, mode in cases:
        x0 = 0.5 * init_with_seed(n, dim, 42)
        a = NUTS(tgt, x0, 0.8, mode=mode).set_seed(9)
        b = NUTS(tgt, x0, 0.8, mode=mode).set_seed(9)
        b.metric = np.ones(dim)
        assert b.kernel_variant == 7
        ra, rb = _nuts_all(a, 12, 12), _nuts_all(b, 12, 12)
        for u, v, what in zip(ra, rb, ("samples", "positions", "adaptation records", "leapfrog counts", "depth histogram")):
            assert _bits_equal(u, v), (type(tgt).__name__, mode, what)
        assert ra[3].sum() >= 23 * n and ra[4].sum() == 23 * n
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------ 6: powers of two

def _pow2(dim):
    k = (np.arange(dim) * 5 + 3) % 13 - 6  # -6 .. 6, as the twin
    return np.ldexp(1.0, k), np.ldexp(1.0, -k)


@pytest.mark.parametrize("dim", [1, 3, 8, 9, 32])
def test_power_of_two_identity_on_the_device(dim):
    """metric s_i = 2^k_i on the functor with c_i = 2^-k_i from s * y0 == s * (no metric, c_i = 1, from y0), bit for bit"""
    from mini_mcmc_amd.core import init_with_seed
    from mini_mcmc_amd.hmc import HMC
    from mini_mcmc_amd.nuts import NUTS

    s, c = _pow2(dim)
    scaled, unit = _quad(f"metric_quad_scaled{dim}", c), _quad(f"metric_quad_unit{dim}", np.ones(dim))
    for n in CHAINS:
        y0 = init_with_seed(n, dim, 42).astype(np.float32).astype(np.float64)  # exact in both element types
        for dt in (np.float32, np.float64):
            for L in (0, 1, 7):
                a = HMC(scaled, (y0 * s).astype(dt), 0.3, L).set_seed(5)
                a.metric = s
                b = HMC(unit, y0.astype(dt), 0.3, L).set_seed(5)
                sa, sb = a.run(14, 6), b.run(14, 6)
                assert _bits_equal(sa, sb * s.astype(dt)), (n, dt.__name__, L)
                assert _bits_equal(a.state(), b.state() * s.astype(dt)) and np.array_equal(a.accept_counts, b.accept_counts), (n, dt.__name__, L)
                assert L == 0 or a.accept_counts.sum() > 0
                a.close()
                b.close()
        for mode in (0, 2):
            dt = np.float64 if mode == 2 else np.float32
            a = NUTS(scaled, y0 * s, 0.8, mode=mode).set_seed(5)
            a.metric = s
            b = NUTS(unit, y0, 0.8, mode=mode).set_seed(5)
            ra, rb = _nuts_all(a, 10, 6), _nuts_all(b, 10, 6)
            assert _bits_equal(ra[0], rb[0] * s.astype(dt)) and _bits_equal(ra[1], rb[1] * s.astype(dt)), (n, mode)
            for u, v, what in zip(ra[2:], rb[2:], ("adaptation records", "leapfrog counts", "depth histogram")):
                assert _bits_equal(u, v), (n, mode, what)
            assert ra[3].sum() >= 15 * n
            a.close()
            b.close()


# ------------------------------------------------------------------------------------------------ 7: the host twin

GENERAL = np.array([0.37, 2.9, 11.0])


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_hmc_with_a_general_metric_is_the_host_twin_bit_for_bit(tmp_path_factory, tmp_path, dtype):
    from mini_mcmc_amd.distributions import RosenbrockND
    from mini_mcmc_amd.hmc import HMC

    exe = M.build_twin(tmp_path_factory)
    n, eps, L = 65, 0.004, 7
    ref_s, ref_x, ref_acc, _ = M.twin_hmc(exe, tmp_path, dtype, "rosen3", n, 24, 7, eps, L, 13, scale=GENERAL)
    h = HMC(RosenbrockND(3), M.start(n, 3).astype(dtype), eps, L).set_seed(13)
    h.metric = GENERAL
    got = h.run(24, 7)
    assert _bits_equal(got, ref_s) and _bits_equal(h.state(), ref_x) and np.array_equal(h.accept_counts, ref_acc)
    assert 0 < ref_acc.sum() and not _bits_equal(M.twin_hmc(exe, tmp_path, dtype, "rosen3", n, 24, 7, eps, L, 13)[0], ref_s)


def test_nuts_with_a_general_metric_is_the_host_twin_bit_for_bit(tmp_path_factory, tmp_path):
    from mini_mcmc_amd.distributions import RosenbrockND
    from mini_mcmc_amd.nuts import NUTS

    exe = M.build_twin(tmp_path_factory)
    n = 65
    ref = M.twin_nuts(exe, tmp_path, 0, n, 12, 12, 13, scale=GENERAL)
    h = NUTS(RosenbrockND(3), M.start(n, 3), 0.8, mode=0).set_seed(13)
    h.metric = GENERAL
    got = _nuts_all(h, 12, 12)
    for u, v, what in zip(got, ref, ("samples", "positions", "adaptation records", "leapfrog counts", "depth histogram")):
        assert _bits_equal(u, np.asarray(v)), what
    assert not _bits_equal(M.twin_nuts(exe, tmp_path, 0, n, 12, 12, 13)[0], ref[0])


# ------------------------------------------------------------------------------------------------ 8: contract edges

def test_bad_values_and_unsupported_handles_change_nothing():
    from mini_mcmc_amd import _lib as L
    from mini_mcmc_amd.core import init_with_seed
    from mini_mcmc_amd.distributions import IsotropicGaussian, RosenbrockND
    from mini_mcmc_amd.hmc import HMC
    from mini_mcmc_amd.nuts import NUTS

    lib = L.lib()
    x0 = init_with_seed(65, 3, 42)
    good = np.array([0.5, 2.0, 3.0])
    for h, pre in ((HMC(RosenbrockND(3), x0.astype(np.float32), 0.03, 5), "hmc"), (NUTS(RosenbrockND(3), x0, 0.8), "nuts")):
        setm, getm = getattr(lib, f"mmcmc_{pre}_set_metric"), getattr(lib, f"mmcmc_{pre}_metric")
        out = (C.c_double * 3)()
        assert getm(h._h, out) == 0 and list(out) == [1.0, 1.0, 1.0]
        h.metric = good
        for bad in (np.nan, np.inf, 0.0, -1.0, 1e-60, 1e60):  # the last two: not finite and > 0 as f32
            v = good.copy()
            v[1] = bad
            assert setm(h._h, v.ctypes.data_as(C.POINTER(C.c_double))) == L.ERR_INVALID_ARG, bad
            assert getm(h._h, out) == 1 and list(out) == list(good), bad
        with pytest.raises(ValueError):
            h.metric = np.ones(4)
        assert np.array_equal(h.metric, good) and h.kernel_variant == 7
        set_variant = getattr(lib, f"mmcmc_{pre}_set_kernel_variant")
        assert set_variant(h._h, 2 if pre == "hmc" else 0) == L.ERR_UNSUPPORTED and set_variant(h._h, 7) == L.OK
        assert set_variant(h._h, 99) == L.ERR_INVALID_ARG
        h.close()
    x33 = init_with_seed(65, 33, 42)
    for h, pre in ((HMC(IsotropicGaussian(1.0, 33), x33.astype(np.float32), 0.1, 3), "hmc"), (NUTS(IsotropicGaussian(1.0, 33), x33, 0.8), "nuts")):
        v = h.kernel_variant
        ones = np.ones(33)
        assert getattr(lib, f"mmcmc_{pre}_set_metric")(h._h, ones.ctypes.data_as(C.POINTER(C.c_double))) == L.ERR_UNSUPPORTED
        assert h.metric is None and h.kernel_variant == v
        h.close()


def test_a_scale_without_an_f32_reciprocal_is_hmcs_to_take_and_nuts_to_refuse():
    """The one respect in which the two diagonal checks differ (csrc/mm_metric_host.h: mm_diag_prepare): 1e-39 is finite and
    > 0 as f32, 1 / 1e-39 is not.  HMC never forms r_i = 1 / s_i; NUTS's stop criterion multiplies by it.  Neither handle is
    run with that metric."""
    from mini_mcmc_amd import _lib as L
    from mini_mcmc_amd.core import init_with_seed
    from mini_mcmc_amd.distributions import RosenbrockND
    from mini_mcmc_amd.hmc import HMC
    from mini_mcmc_amd.nuts import NUTS

    lib = L.lib()
    x0 = init_with_seed(65, 3, 42)
    tiny, good = np.array([1.0, 1e-39, 1.0]), np.array([0.5, 2.0, 3.0])
    p_tiny = tiny.ctypes.data_as(C.POINTER(C.c_double))
    out = (C.c_double * 3)()
    h = HMC(RosenbrockND(3), x0.astype(np.float32), 0.03, 5)
    assert lib.mmcmc_hmc_set_metric(h._h, p_tiny) == L.OK
    assert lib.mmcmc_hmc_metric(h._h, out) == 1 and list(out) == list(tiny)
    h.close()
    n = NUTS(RosenbrockND(3), x0, 0.8, mode=0)  # tensor type f32
    n.metric = good
    assert lib.mmcmc_nuts_set_metric(n._h, p_tiny) == L.ERR_INVALID_ARG
    assert lib.mmcmc_nuts_metric(n._h, out) == 1 and list(out) == list(good) and n.kernel_variant == 7
    n.close()


def test_lane_group_handle_moves_to_the_unit_and_back():
    from mini_mcmc_amd.core import init_with_seed
    from mini_mcmc_amd.distributions import GaussianND
    from mini_mcmc_amd.hmc import HMC

    tgt = GaussianND.ill_conditioned(16, 50.0)
    x0 = init_with_seed(130, 16, 42)
    a, b = HMC(tgt, x0, 0.05, 4).set_seed(3), HMC(tgt, x0, 0.05, 4).set_seed(3)
    assert a.kernel_variant == 3
    b.metric = np.linspace(0.5, 2.0, 16)
    assert b.kernel_variant == 7
    with_metric = b.run(8, 2)
    b.metric = None
    assert b.kernel_variant == 3
    b.set_iteration(0).positions = x0
    ref = a.run(8, 2)
    assert _bits_equal(b.run(8, 2), ref) and not _bits_equal(with_metric, ref)
    a.close()
    b.close()


@pytest.mark.parametrize("n", CHAINS)
def test_scheduled_run_with_a_metric_is_the_loop_of_steps(n):
    from mini_mcmc_amd.distributions import RosenbrockND
    from mini_mcmc_amd.hmc import HMC

    eps = np.array([0.004, 0.004, 0.006, 0.003, 0.003, 0.003, 0.005])
    nl = np.array([3, 3, 5, 0, 2, 2, 7], dtype=np.int32)
    x0 = M.start(n, 3).astype(np.float32)
    a, b = HMC(RosenbrockND(3), x0, 0.01, 1).set_seed(21), HMC(RosenbrockND(3), x0, 0.01, 1).set_seed(21)
    a.metric = b.metric = GENERAL
    got = a.run_scheduled(eps, nl, 4)
    rows = []
    for e, k in zip(eps, nl):
        b.step_size, b.n_leapfrog = float(e), int(k)
        b.step()
        rows.append(b.state())
    assert _bits_equal(got, np.stack(rows[-4:], axis=1)) and _bits_equal(a.state(), b.state())
    assert a.stream_position() == b.stream_position() and a.step_size == 0.01 and a.n_leapfrog == 1
    a.close()
    b.close()


def test_run_progress_uses_the_metric():
    from mini_mcmc_amd.distributions import RosenbrockND
    from mini_mcmc_amd.hmc import HMC
    from mini_mcmc_amd.nuts import NUTS

    for make in (lambda: HMC(RosenbrockND(3), M.start(65, 3).astype(np.float32), 0.004, 7).set_seed(4),
                 lambda: NUTS(RosenbrockND(3), M.start(65, 3), 0.8).set_seed(4)):
        a, b, c = make(), make(), make()
        b.metric = GENERAL
        c.metric = np.ones(3)
        sa, sb, sc = a.run_progress(16, 8)[0], b.run_progress(16, 8)[0], c.run_progress(16, 8)[0]
        assert np.all(np.isfinite(sb)) and not _bits_equal(sa, sb) and _bits_equal(sa, sc)
        for h in (a, b, c):
            h.close()


def test_checkpoint_and_restore_with_a_metric(tmp_path):
    from mini_mcmc_amd import checkpoint as K
    from mini_mcmc_amd.distributions import RosenbrockND
    from mini_mcmc_amd.hmc import HMC
    from mini_mcmc_amd.nuts import NUTS

    for kind, make in (("hmc", lambda: HMC(RosenbrockND(3), M.start(65, 3).astype(np.float32), 0.004, 7).set_seed(4)),
                       ("nuts", lambda: NUTS(RosenbrockND(3), M.start(65, 3), 0.8, mode=0).set_seed(4))):
        a, b, c = make(), make(), make()
        plain = K.take(c)  # what a checkpoint written before metrics existed holds
        assert "metric" not in plain
        a.metric = GENERAL
        a.run(10, 5)
        K.save(tmp_path / f"{kind}.npz", a.checkpoint())
        ck = K.load(tmp_path / f"{kind}.npz")
        assert np.array_equal(ck["metric"], GENERAL)
        ref = a.run(10, 3)
        b.restore(ck)
        assert np.array_equal(b.metric, GENERAL) and b.kernel_variant == 7
        assert _bits_equal(b.run(10, 3), ref), kind
        if kind == "nuts":
            assert _bits_equal(a.positions(), b.positions()) and all(_bits_equal(a.adapt_state()[k], b.adapt_state()[k]) for k in a.adapt_state())
        # a metric of the wrong length is refused before anything is set
        bad = dict(ck, metric=np.ones(4), seed=77)
        before = b.stream_position()
        with pytest.raises(ValueError):
            b.restore(bad)
        assert b.stream_position() == before and np.array_equal(b.metric, GENERAL)
        b.restore(plain)  # no "metric": no metric
        assert b.metric is None and _bits_equal(b.run(6, 2), c.run(6, 2)), kind
        for h in (a, b, c):
            h.close()


# ------------------------------------------------------------------------------------------------ 9: the adaptation

def test_warmup_nuts_recovers_the_scales_and_cuts_the_leapfrogs():
    """Axis-aligned Gaussian, sigma_i = 10^((i - 4) / 2) (1e-2 .. 1e2), NUTS mode 0, 256 chains started from the exact
    posterior, so every window is stationary and the estimate's error is statistical: the first window already has >= 256
    independent draws, the relative error of a standard deviation is <= 1 / sqrt(512) = 4.4 %, the band [0.75, 1.25] more
    than five of those (the regulariser moves s^2 by less than 1 %).  Under the identity metric epsilon adapts to the 1e-2
    scale, the 1e2 coordinate would need ~1e4 steps, so every tree stops at the cap (1023 gradients); a unit-scale 9-D
    Gaussian takes 7 to 15: a ratio of 8 leaves roughly a tenfold margin.  R-hat <= 1.05: DESIGN.md level G's bar.
    Measured: s / sigma within 0.966 .. 1.027 after the first window and 0.991 .. 1.008 after the third;
    6.3 against 864.4 leapfrogs per transition, a ratio of 137; worst R-hat 1.0081."""
    import torch

    from mini_mcmc_amd import stats as S
    from mini_mcmc_amd.core import init_with_seed
    from mini_mcmc_amd.nuts import NUTS
    from mini_mcmc_amd.warmup import warmup_nuts

    sigma = 10.0 ** ((np.arange(9) - 4) / 2.0)
    tgt = _quad("metric_gauss9_scales", 1.0 / sigma)
    x0 = sigma * init_with_seed(256, 9, 42)
    adapted, identity = NUTS(tgt, x0, 0.8, mode=0), NUTS(tgt, x0, 0.8, mode=0)
    scale, records = warmup_nuts(adapted, windows=(25, 50, 100), seed=100)
    for k, r in enumerate(records):
        print(f"window {k}: mean leapfrogs {r['mean_leapfrogs']:.1f} scale / sigma {np.array2string(r['scale'] / sigma, precision=3)}")
    assert np.array_equal(adapted.metric, scale) and adapted.stream_position()[2] == 0
    assert np.all(adapted.adapt_state()["epsilon"] == -1.0)
    ratio_s = scale / sigma
    assert np.all((ratio_s >= 0.75) & (ratio_s <= 1.25)), ratio_s
    # deterministic: the same arguments give the same bits
    again = NUTS(tgt, x0, 0.8, mode=0)
    scale2, _ = warmup_nuts(again, windows=(25, 50, 100), seed=100)
    assert _bits_equal(scale, scale2)
    again.close()
    lf = []
    for h in (adapted, identity):
        h.set_seed(99)
        before = h.leapfrog_counts().astype(np.float64).sum()
        sample = h.run(200, 50, to="torch")
        torch.cuda.synchronize()
        lf.append(h.leapfrog_counts().astype(np.float64).sum() - before)
        if h is adapted:
            rhat = S.rank_diagnostics(sample).rhat
    print(f"adapted leapfrogs per transition {lf[0] / (256 * 249):.1f}, identity {lf[1] / (256 * 249):.1f}, ratio {lf[1] / lf[0]:.1f}; "
          f"rank-normalised split R-hat max {rhat.max():.4f}")
    assert np.all(rhat <= 1.05), rhat
    assert lf[0] * 8 <= lf[1], (lf[0], lf[1])
    adapted.close()
    identity.close()
