"""Targets that carry data (mmcmc_target_register_data_source, csrc/mm_data.h) on the device: the two models of
tests/data_common.py, each from its log-density alone and with a hand-written gradient.

 * device = host program: unnorm_logp_batch at the 257 points of tests/cpp/data_host.cpp (the last wave is partly empty)
   returns its bits, value and gradient, f32 and f64, for all four kinds;
 * the plumbing under every sampler: the autodiff kind equals the hand-written one bit for bit (the host program shows the
   two gradients equal, for logit9 as well) under HMC (with chunked launches too), NUTS, MH, a device group and a user proposal;
 * the data is what is sampled: another last element, other samples; the same array, the same bits; the host array may be
   overwritten after create; with_data compiles nothing;
 * refusals: matrix == NULL from every create and the batch call, data_len == 0 at registration;
 * linreg3's posterior is Gaussian in closed form: NUTS reproduces its mean and variance within derived bands
   (tests/test_data_target_host.py shows that the model without its last row lies outside them);
 * checkpoint / restore over the same array continues bit for bit."""
import ctypes as C

import numpy as np
import pytest

import autodiff_common as A
import data_common as D

pytestmark = pytest.mark.gpu
_made = {}


def _target(model, flavour):
    """the kind of `model` as `flavour` ("logp" | "hand") over the model's own array, registered once per session"""
    from mini_mcmc_amd.distributions import AutodiffTarget, UserTarget

    if (model, flavour) not in _made:
        dim, data, params = D.MODELS[model]
        cls = AutodiffTarget if flavour == "logp" else UserTarget
        _made[(model, flavour)] = cls(f"{model}_{flavour}", dim, D.source(model, flavour), params=params, data=data)
    return _made[(model, flavour)]


def _without_matrix(tgt):
    """a description of tgt's kind whose `matrix` is NULL"""
    from mini_mcmc_amd.distributions import Target

    bare = Target(tgt.dim, tgt.params)
    bare.kind = tgt.kind
    return bare


@pytest.mark.parametrize("flavour", ["logp", "hand"])
@pytest.mark.parametrize("model", ["linreg3", "logit9"])
def test_device_value_and_gradient_are_the_host_programs_bit_for_bit(model, flavour):
    tgt = _target(model, flavour)
    assert tgt.kind >= 1000 and tgt.data_len == D.MODELS[model][1].size
    n = C.c_size_t(0)
    from mini_mcmc_amd import _lib as L

    assert L.lib().mmcmc_target_data_len(tgt.kind, C.byref(n)) == L.OK and n.value == tgt.data_len
    v, g = ("value", "grad") if flavour == "logp" else ("value_hand", "grad_hand")
    for ty, dt in (("f32", np.float32), ("f64", np.float64)):
        host = D.host_results()[(model, ty)]
        assert host["x"].shape[0] == 257
        lp, grad = tgt.unnorm_logp_batch(host["x"], dt, with_grad=True)
        assert np.array_equal(A.bits(lp), A.bits(host[v])), (model, flavour, ty)
        assert np.array_equal(A.bits(grad), A.bits(host[g])), (model, flavour, ty)
        assert np.array_equal(A.bits(tgt.unnorm_logp_batch(host["x"], dt)), A.bits(host[v])), (model, flavour, ty)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("model", ["linreg3", "logit9"])
def test_hmc_with_the_derived_gradient_equals_the_hand_written_one(model, dtype):
    from mini_mcmc_amd.core import init_with_seed
    from mini_mcmc_amd.hmc import HMC

    ad, hand = _target(model, "logp"), _target(model, "hand")
    init = init_with_seed(333, ad.dim, 42, dtype)
    for nc, nd, L in ((40, 9, 10), (33, 0, 7), (1, 3, 10)):
        a = HMC(ad, init, 0.1, L).set_seed(42)
        b = HMC(hand, init, 0.1, L).set_seed(42)
        c = HMC(ad, init, 0.1, L).set_seed(42).set_iters_per_launch(7)  # chunked launches
        assert a.kernel_variant == b.kernel_variant
        out_a, out_b, out_c = a.run(nc, nd), b.run(nc, nd), c.run(nc, nd)
        assert np.array_equal(A.bits(out_a), A.bits(out_b)), (model, dtype.__name__, nc, nd, L)
        assert np.array_equal(a.accept_counts, b.accept_counts) and np.array_equal(A.bits(a.state()), A.bits(b.state()))
        assert np.array_equal(A.bits(out_c), A.bits(out_b)) and np.array_equal(c.accept_counts, b.accept_counts)
        assert np.array_equal(A.bits(c.state()), A.bits(b.state()))
        assert 0 < a.accept_counts.mean() <= nc + nd  # a density, not -inf or NaN everywhere


@pytest.mark.parametrize("model,mode", [("linreg3", 0), ("linreg3", 1), ("linreg3", 2), ("logit9", 2)])
def test_nuts_with_the_derived_gradient_equals_the_hand_written_one(model, mode):
    from mini_mcmc_amd.core import init_with_seed
    from mini_mcmc_amd.nuts import NUTS

    ad, hand = _target(model, "logp"), _target(model, "hand")
    init = init_with_seed(96, ad.dim, 42) * 0.5
    a = NUTS(ad, init, 0.8, mode=mode).set_seed(9)
    b = NUTS(hand, init, 0.8, mode=mode).set_seed(9)
    assert a.kernel_variant == b.kernel_variant == 7
    out_a, out_b = a.run(5, 5), b.run(5, 5)
    assert np.all(np.isfinite(out_a))
    assert np.array_equal(A.bits(out_a), A.bits(out_b)) and np.array_equal(A.bits(a.positions()), A.bits(b.positions()))
    assert np.array_equal(a.leapfrog_counts(), b.leapfrog_counts()) and np.array_equal(a.depth_histogram(), b.depth_histogram())
    sa, sb = a.adapt_state(), b.adapt_state()
    assert np.array_equal(sa["epsilon"], sb["epsilon"]) and np.array_equal(sa["h_bar"], sb["h_bar"])


def test_mh_group_and_user_proposal_over_the_data_kind():
    from mini_mcmc_amd.core import init_with_seed
    from mini_mcmc_amd.distributions import IsotropicGaussian, UserProposal
    from mini_mcmc_amd.group import HMCGroup
    from mini_mcmc_amd.hmc import HMC
    from mini_mcmc_amd.metropolis_hastings import MetropolisHastings

    ad, hand = _target("linreg3", "logp"), _target("linreg3", "hand")
    for dtype in (np.float32, np.float64):
        init = init_with_seed(333, 3, 42, dtype)
        m_a = MetropolisHastings(ad, IsotropicGaussian(0.5), init).seed(7)
        m_b = MetropolisHastings(hand, IsotropicGaussian(0.5), init).seed(7)
        assert np.array_equal(A.bits(m_a.run(50, 0)), A.bits(m_b.run(50, 0))) and np.array_equal(m_a.accept_counts, m_b.accept_counts)
        assert np.array_equal(A.bits(m_a.positions), A.bits(m_b.positions))
        assert 0 < m_a.accept_counts.mean() < 50
    init = init_with_seed(300, 3, 3, np.float32)
    group = HMCGroup(ad, init, 0.1, 10, devices=[0, 0]).set_seed(5)  # one copy of the array per shard
    one = HMC(hand, init, 0.1, 10).set_seed(5)
    out_g, out_1 = group.run(20, 5), one.run(20, 5)
    assert np.array_equal(A.bits(out_g), A.bits(out_1)) and np.array_equal(group.accept_counts, one.accept_counts)
    assert np.array_equal(A.bits(group.state()), A.bits(one.state()))
    # a proposal compiled over the data kind: its model reads the same array, uploaded with the kind's length
    if "proposals" not in _made:
        _made["proposals"] = (UserProposal("iso_over_data_ad", ad, D.ISOTROPIC, 0.5), UserProposal("iso_over_data_hand", hand, D.ISOTROPIC, 0.5))
    p_a, p_b = _made["proposals"]
    init = init_with_seed(333, 3, 11, np.float64)
    u_a = MetropolisHastings(ad, p_a, init).seed(5)
    u_b = MetropolisHastings(hand, p_b, init).seed(5)
    out_u = u_a.run(40, 5)
    assert np.array_equal(A.bits(out_u), A.bits(u_b.run(40, 5))) and np.array_equal(u_a.accept_counts, u_b.accept_counts)
    assert np.array_equal(A.bits(u_a.positions), A.bits(u_b.positions))
    assert 0 < u_a.accept_counts.mean() < 45
    from mini_mcmc_amd import _lib as L

    with pytest.raises(L.MmcmcError) as e:
        MetropolisHastings(_without_matrix(ad), p_a, init)
    assert e.value.status == L.ERR_INVALID_ARG


def test_the_data_is_what_is_sampled_and_with_data_compiles_nothing():
    from mini_mcmc_amd.core import init_with_seed
    from mini_mcmc_amd.hmc import HMC

    base = _target("linreg3", "logp")
    log_before = base.compile_log
    same = np.array(D.LINREG3, dtype=np.float64).reshape(-1)  # a copy of the model's array
    other = same.copy()
    other[-1] += 0.5  # only the LAST element differs: an upload one element short could not tell them apart
    t_same, t_other = base.with_data(same), base.with_data(other)
    assert t_same.kind == t_other.kind == base.kind and t_same.compile_log is log_before and base.compile_log is log_before
    assert t_same.data_len == 28 and np.array_equal(base.data, D.LINREG3.reshape(-1))
    with pytest.raises(ValueError):
        base.with_data(same[:-1])
    init = init_with_seed(333, 3, 42, np.float32)
    ref = HMC(base, init, 0.1, 10).set_seed(3).run(20, 5)
    h_same = HMC(t_same, init, 0.1, 10).set_seed(3)
    h_other = HMC(t_other, init, 0.1, 10).set_seed(3)
    same[:] = -7.0  # the handle owns its device copy: the host array may be overwritten (t_same aliases `same`) ...
    assert np.all(t_same.data == -7.0)
    assert np.array_equal(A.bits(h_same.run(20, 5)), A.bits(ref))  # ... as soon as create has returned
    assert not np.array_equal(h_other.run(20, 5), ref)
    x = D.host_results()[("linreg3", "f64")]["x"]
    assert not np.array_equal(t_other.unnorm_logp_batch(x, np.float64), base.unnorm_logp_batch(x, np.float64))


def test_a_description_without_the_array_is_refused_everywhere_and_so_is_an_empty_dataset():
    from mini_mcmc_amd import _lib as L
    from mini_mcmc_amd.core import init_with_seed
    from mini_mcmc_amd.distributions import IsotropicGaussian, UserTarget
    from mini_mcmc_amd.group import HMCGroup, MetropolisHastingsGroup, NUTSGroup
    from mini_mcmc_amd.hmc import HMC
    from mini_mcmc_amd.metropolis_hastings import MetropolisHastings
    from mini_mcmc_amd.nuts import NUTS

    bare = _without_matrix(_target("linreg3", "hand"))
    init32, init64 = init_with_seed(64, 3, 1, np.float32), init_with_seed(64, 3, 1)
    creates = [lambda: MetropolisHastings(bare, IsotropicGaussian(0.5), init32), lambda: MetropolisHastings(bare, IsotropicGaussian(0.5), init64),
               lambda: HMC(bare, init32, 0.1, 5), lambda: HMC(bare, init64, 0.1, 5),
               lambda: NUTS(bare, init64, 0.8, mode=0), lambda: NUTS(bare, init64, 0.8, mode=1), lambda: NUTS(bare, init64, 0.8, mode=2),
               lambda: MetropolisHastingsGroup(bare, IsotropicGaussian(0.5), init32, devices=[0, 0]),
               lambda: HMCGroup(bare, init32, 0.1, 5, devices=[0, 0]), lambda: NUTSGroup(bare, init64, 0.8, mode=2, devices=[0, 0]),
               lambda: bare.unnorm_logp_batch(init32, np.float32), lambda: bare.unnorm_logp_batch(init64, np.float64, with_grad=True)]
    for i, create in enumerate(creates):
        with pytest.raises(L.MmcmcError) as e:
            create()
        assert e.value.status == L.ERR_INVALID_ARG, i
    kind = C.c_int(-5)
    src = D.source("linreg3", "hand").encode()
    assert L.lib().mmcmc_target_register_data_source(b"empty", 3, 0, 0, src, C.byref(kind), None, 0) == L.ERR_INVALID_ARG and kind.value == -5
    with pytest.raises(L.MmcmcError) as e:
        UserTarget("empty", 3, D.source("linreg3", "hand"), data=np.zeros(0))
    assert e.value.status == L.ERR_INVALID_ARG


def test_nuts_reproduces_the_closed_form_posterior_of_linreg3():
    """4096 independent chains from init_with_seed, NUTS mode 2, 100 warm-up + 100 kept draws.  The mean over all kept draws has
    variance <= sd^2 / 4096 per coordinate (the chains are independent; draws within a chain only help), so
    |mean - mu| <= 5 sd / sqrt(4096); the pooled variance of at least 4096 independent Gaussian draws has relative standard
    deviation <= sqrt(2 / 4096), so |var / sd^2 - 1| <= 5 sqrt(2 / 4096).  Both bands are derived, not measured."""
    from mini_mcmc_amd import stats as S
    from mini_mcmc_amd.core import init_with_seed
    from mini_mcmc_amd.nuts import NUTS

    mu, cov = D.linreg3_posterior()
    sd = np.sqrt(np.diag(cov))
    smp = NUTS(_target("linreg3", "logp"), init_with_seed(4096, 3, 42), 0.8, mode=2).set_seed(7).run(100, 100)
    assert smp.shape == (4096, 100, 3)
    flat = smp.reshape(-1, 3).astype(np.float64)
    mean, var = flat.mean(axis=0), flat.var(axis=0)
    print("mean error in units of the band:", np.abs(mean - mu) / (5 * sd / 64), " variance:", np.abs(var / sd ** 2 - 1) / (5 * np.sqrt(2 / 4096)))
    assert np.all(np.abs(mean - mu) <= 5 * sd / np.sqrt(4096))
    assert np.all(np.abs(var / sd ** 2 - 1) <= 5 * np.sqrt(2 / 4096))
    assert np.all(S.rank_diagnostics(smp).rhat <= 1.05)


def test_checkpoint_and_restore_over_the_same_array_continue_bit_for_bit():
    from mini_mcmc_amd.core import init_with_seed
    from mini_mcmc_amd.hmc import HMC

    tgt = _target("logit9", "logp")

    def make(k):
        init = (init_with_seed(200, 9, (42, 7)[k]) * 0.5).astype(np.float32)
        return HMC(tgt.with_data(D.LOGIT9), init, (0.05, 0.1)[k], (6, 3)[k]).set_seed((11, 99)[k])  # fresh handle, the same array

    a = make(0)
    a.run(5, 4)
    ck = a.checkpoint()
    assert "data" not in ck and "matrix" not in ck  # the kind is stored, not the array
    out_a = a.run(12, 3)
    b = make(1)
    b.restore(ck)
    out_b = b.run(12, 3)
    assert np.array_equal(A.bits(out_a), A.bits(out_b)) and np.array_equal(a.accept_counts, b.accept_counts)
    assert np.array_equal(A.bits(a.state()), A.bits(b.state()))


def test_unit_built_by_hiprtc_reads_the_array_like_the_one_built_by_hipcc():
    """the fallback compiler has no host headers and its own copy of the compiler proper: csrc/mm_data.h must build there and
    the batch kernel must return the host program's bits"""
    from mini_mcmc_amd.distributions import AutodiffTarget, rtc_compiler_info, set_rtc_compiler

    assert rtc_compiler_info()["hiprtc_path"], "a machine with a GPU has the HIP runtime's libhiprtc.so"
    dim, data, params = D.MODELS["logit9"]
    set_rtc_compiler("hiprtc")
    try:
        tgt = AutodiffTarget("logit9_logp_hiprtc", dim, D.source("logit9", "logp"), params=params, data=data)
    finally:
        set_rtc_compiler("auto")
    assert tgt.compiler == "hiprtc" and _target("logit9", "logp").compiler == "hipcc"
    for ty, dt in (("f32", np.float32), ("f64", np.float64)):
        host = D.host_results()[("logit9", ty)]
        lp, grad = tgt.unnorm_logp_batch(host["x"], dt, with_grad=True)
        assert np.array_equal(A.bits(lp), A.bits(host["value"])) and np.array_equal(A.bits(grad), A.bits(host["grad"]))
