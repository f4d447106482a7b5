"""Targets registered from a log-density alone (mmcmc_target_register_logp_source, csrc/mm_autodiff.h) on the device.

 * device = host: mmcmc_logp_grad_batch on the bodies of tests/cpp/autodiff_cases/ returns, value and gradient, f32 and f64,
   the bits the host program tests/cpp/autodiff_host.cpp computes with the host twin's compiler (257 points: the last wave
   is partly empty);
 * the plumbing is exact: for logp = -1/2 sum x_i^2 written as a loop of mm_fma, forward mode yields -x_i with every
   operation exact (fma(1, x, fma(x, 1, 0)) = 2 x, times -1/2), so the autodiff kind equals a hand-written target with
   g[i] = -x[i] bit for bit under HMC (split kernel, variant 2, chunked passes), NUTS (pair kernel and generic one), MH, a
   device group and a user proposal;
 * a real density: RosenbrockND(3) from its log-density equals the built-in target under MH and unnorm_logp_batch; the banana
   under HMC passes the bands of test_user_target.py::test_new_density_samples_what_it_describes;
 * an operation without a dual overload is a compile error whose text arrives in the log."""
import numpy as np
import pytest

import autodiff_common as A

HALF_SQUARES_LOGP = r"""
template <class T> struct mmcmc_user_logp {
    static constexpr int dim = MM_USER_DIM;
    template <class S> MM_HD static S logp(const mm_tparams<T> &, const S *x) {
        S acc = 0;
        MM_UNROLL
        for (int i = 0; i < dim; ++i) acc = mm_fma(x[i], x[i], acc);
        return T(-0.5) * acc;
    }
};
"""

HALF_SQUARES_HAND = r"""
template <class T> struct mmcmc_user_target {
    static constexpr int dim = MM_USER_DIM;
    MM_HD static T logp(const mm_tparams<T> &, const T *x) {
        T acc = 0;
        MM_UNROLL
        for (int i = 0; i < dim; ++i) acc = mm_fma(x[i], x[i], acc);
        return T(-0.5) * acc;
    }
    MM_HD static T logp_grad(const mm_tparams<T> &P, const T *x, T *g) {
        MM_UNROLL
        for (int i = 0; i < dim; ++i) g[i] = -x[i];
        return logp(P, x);
    }
};
"""

ISOTROPIC = r"""
template <class T> struct mmcmc_user_proposal {
    MM_HD static void sample(T sigma, const T *x, const T *z, T *out) {
        for (int i = 0; i < MM_USER_DIM; ++i)
            out[i] = mm_fma(sigma, z[i], x[i]);
    }
    MM_HD static T logp(T sigma, const T *from, const T *to) {
        const T var = sigma * sigma;
        T acc = 0;
        for (int i = 0; i < MM_USER_DIM; ++i) {
            const T d = to[i] - from[i];
            acc += -(d * d) / (T(2) * var);
        }
        return acc;
    }
};
"""

_made = {}


def _pair(dim):
    """(autodiff kind, hand-written kind) of -1/2 sum x^2 at `dim`, registered once per session"""
    from mini_mcmc_amd.distributions import AutodiffTarget, UserTarget

    if dim not in _made:
        _made[dim] = (AutodiffTarget(f"half_squares_ad{dim}", dim, HALF_SQUARES_LOGP), UserTarget(f"half_squares_hand{dim}", dim, HALF_SQUARES_HAND))
    return _made[dim]


def _case_target(case):
    from mini_mcmc_amd.distributions import AutodiffTarget

    if ("case", case) not in _made:
        src, dim = A.case_source(case)
        _made[("case", case)] = AutodiffTarget("ad_" + case, dim, src, params=A.BANANA_PARAMS if case == "banana" else ())
    return _made[("case", case)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["rosenbrock2", "rosenbrock3", "rosenbrock8", "rosenbrock9", "rosenbrock17", "rosenbrock32", "banana",
                                  "div", "log", "exp", "sqrt", "abs", "branch"])
def test_device_gradient_is_the_host_programs_bit_for_bit(case):
    tgt = _case_target(case)
    assert tgt.kind >= 1000
    for ty, dt in (("f32", np.float32), ("f64", np.float64)):
        host = A.host_results()[(case, ty)]
        assert host["x"].shape[0] == 257
        lp, g = tgt.unnorm_logp_batch(host["x"], dt, with_grad=True)
        assert np.array_equal(A.bits(lp), A.bits(host["value"])), (case, ty)
        assert np.array_equal(A.bits(g), A.bits(host["grad"])), (case, ty)
        assert np.array_equal(A.bits(tgt.unnorm_logp_batch(host["x"], dt)), A.bits(host["value"])), (case, ty)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("dim", [3, 9, 32])
def test_hmc_with_the_derived_gradient_equals_the_hand_written_one(dim, dtype):
    from mini_mcmc_amd.core import init_with_seed
    from mini_mcmc_amd.hmc import HMC

    ad, hand = _pair(dim)
    init = init_with_seed(333, dim, 42, dtype)
    for nc, nd, L in ((40, 9, 10), (33, 0, 7), (1, 3, 10)):
        a = HMC(ad, init, 0.2, L).set_seed(42)
        b = HMC(hand, init, 0.2, L).set_seed(42)
        assert a.kernel_variant == b.kernel_variant
        out_a, out_b = a.run(nc, nd), b.run(nc, nd)
        assert np.array_equal(A.bits(out_a), A.bits(out_b)), (dim, dtype.__name__, nc, nd, L)
        assert np.array_equal(a.accept_counts, b.accept_counts) and np.array_equal(A.bits(a.state()), A.bits(b.state()))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("dim", [3, 9])
def test_nuts_with_the_derived_gradient_equals_the_hand_written_one(dim, mode):
    from mini_mcmc_amd.core import init_with_seed
    from mini_mcmc_amd.nuts import NUTS

    ad, hand = _pair(dim)
    init = init_with_seed(64, dim, 42) * 0.5
    a = NUTS(ad, init, 0.8, mode=mode).set_seed(9)
    b = NUTS(hand, init, 0.8, mode=mode).set_seed(9)
    assert a.kernel_variant == b.kernel_variant == 7
    out_a, out_b = a._run(20, 20, False, "numpy"), b._run(20, 20, False, "numpy")
    assert np.array_equal(A.bits(out_a), A.bits(out_b)) and np.array_equal(A.bits(a.positions()), A.bits(b.positions()))
    assert np.array_equal(a.leapfrog_counts(), b.leapfrog_counts()) and np.array_equal(a.depth_histogram(), b.depth_histogram())
    sa, sb = a.adapt_state(), b.adapt_state()
    assert np.array_equal(sa["epsilon"], sb["epsilon"]) and np.array_equal(sa["h_bar"], sb["h_bar"])


@pytest.mark.gpu
def test_mh_group_and_user_proposal_over_the_autodiff_kind():
    from mini_mcmc_amd.core import init_with_seed
    from mini_mcmc_amd.distributions import IsotropicGaussian, UserProposal
    from mini_mcmc_amd.group import HMCGroup
    from mini_mcmc_amd.hmc import HMC
    from mini_mcmc_amd.metropolis_hastings import MetropolisHastings

    ad, hand = _pair(3)
    for dtype in (np.float32, np.float64):
        init = init_with_seed(333, 3, 42, dtype)
        m_a = MetropolisHastings(ad, IsotropicGaussian(0.5), init).seed(7)
        m_b = MetropolisHastings(hand, IsotropicGaussian(0.5), init).seed(7)
        assert np.array_equal(A.bits(m_a.run(65, 6)), A.bits(m_b.run(65, 6))) and np.array_equal(m_a.accept_counts, m_b.accept_counts)
        assert np.array_equal(A.bits(m_a.positions), A.bits(m_b.positions))
    init = init_with_seed(300, 3, 3, np.float32)
    group = HMCGroup(ad, init, 0.2, 10, devices=[0, 0]).set_seed(5)
    one = HMC(hand, init, 0.2, 10).set_seed(5)
    out_g, out_1 = group.run(20, 5), one.run(20, 5)
    assert np.array_equal(A.bits(out_g), A.bits(out_1)) and np.array_equal(group.accept_counts, one.accept_counts)
    assert np.array_equal(A.bits(group.state()), A.bits(one.state()))
    # a proposal compiled over the autodiff kind: the stored functor source carries the adapter
    p_a = UserProposal("iso_over_ad", ad, ISOTROPIC, 0.5)
    p_b = UserProposal("iso_over_hand", hand, ISOTROPIC, 0.5)
    init = init_with_seed(333, 3, 11, np.float64)
    u_a = MetropolisHastings(ad, p_a, init).seed(5)
    u_b = MetropolisHastings(hand, p_b, init).seed(5)
    assert np.array_equal(A.bits(u_a.run(40, 5)), A.bits(u_b.run(40, 5))) and np.array_equal(u_a.accept_counts, u_b.accept_counts)
    assert np.array_equal(A.bits(u_a.positions), A.bits(u_b.positions))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rosenbrock_from_its_log_density_equals_the_builtin_target(dtype):
    from mini_mcmc_amd.core import init_with_seed
    from mini_mcmc_amd.distributions import IsotropicGaussian, RosenbrockND
    from mini_mcmc_amd.metropolis_hastings import MetropolisHastings

    user = _case_target("rosenbrock3")
    init = init_with_seed(333, 3, 42, dtype)
    m_a = MetropolisHastings(user, IsotropicGaussian(0.1), init).seed(7)
    m_b = MetropolisHastings(RosenbrockND(3), IsotropicGaussian(0.1), init).seed(7)
    assert np.array_equal(A.bits(m_a.run(65, 6)), A.bits(m_b.run(65, 6))) and np.array_equal(m_a.accept_counts, m_b.accept_counts)
    x = (np.random.default_rng(0).standard_normal((100, 3)) * 0.8).astype(dtype)
    assert np.array_equal(A.bits(user.unnorm_logp_batch(x, dtype)), A.bits(RosenbrockND(3).unnorm_logp_batch(x, dtype)))
    lp, _ = user.unnorm_logp_batch(x, dtype, with_grad=True)
    assert np.array_equal(A.bits(lp), A.bits(RosenbrockND(3).unnorm_logp_batch(x, dtype)))


@pytest.mark.gpu
def test_banana_from_its_log_density_samples_what_it_describes():
    """the run and the bands of test_user_target.py::test_new_density_samples_what_it_describes"""
    from mini_mcmc_amd import stats as S
    from mini_mcmc_amd.core import init_with_seed
    from mini_mcmc_amd.hmc import HMC

    s, b = A.BANANA_PARAMS
    tgt = _case_target("banana")
    h = HMC(tgt, init_with_seed(4096, 2, 3, np.float32), 0.15, 12).set_seed(5)
    smp = h.run(150, 150)
    flat = smp.reshape(-1, 2).astype(np.float64)
    assert abs(flat[:, 0].mean()) < 0.03 and abs(flat[:, 0].var() / s**2 - 1) < 0.03
    assert abs(flat[:, 1].mean() - b * s**2) < 0.04 and abs(flat[:, 1].var() / (1 + 2 * b**2 * s**4) - 1) < 0.05
    assert 0.6 < h.accept_counts.mean() / 300 <= 1.0
    rhat, ess = S.split_rhat_mean_ess(smp)
    assert np.all(rhat > 0.9) and np.all(ess > 4096)


@pytest.mark.gpu
def test_operation_without_a_dual_overload_is_reported_with_the_compilers_log():
    from mini_mcmc_amd import _lib as L
    from mini_mcmc_amd.distributions import AutodiffTarget

    src = r"""
template <class T> struct mmcmc_user_logp {
    static constexpr int dim = 2;
    template <class S> MM_HD static S logp(const mm_tparams<T> &, const S *x) { return -x[1] * x[1] - cosh(x[0]); }
};
"""
    with pytest.raises(L.MmcmcError) as e:
        AutodiffTarget("no_overload", 2, src)
    assert e.value.status == L.ERR_INVALID_ARG and "error" in str(e.value) and "cosh" in str(e.value)
