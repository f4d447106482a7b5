"""The reference's public HMC fields (hmc.rs:41-49: step_size, n_leapfrog, positions) as setters, and scheduled runs
(mmcmc_hmc_run_scheduled): transition k of a run uses (eps_k, L_k), defined as -- and bit for bit equal to -- the loop
`set (eps_k, L_k); one transition` on the same handle.  The noise is keyed by (seed, chain, iteration) alone, so the loop and
the single launch draw the same noise; every comparison below is exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_new_entry_points_reject_a_null_handle():
    from mini_mcmc_amd import _lib as L

    lib = L.lib()
    eps = (C.c_double * 2)(0.1, 0.1)
    nl = (C.c_int32 * 2)(3, 3)
    d, n = C.c_double(), C.c_int()
    x = (C.c_float * 3)()
    assert lib.mmcmc_hmc_set_step_size(None, 0.1) == L.ERR_INVALID_ARG
    assert lib.mmcmc_hmc_set_n_leapfrog(None, 3) == L.ERR_INVALID_ARG
    assert lib.mmcmc_hmc_params(None, C.byref(d), C.byref(n)) == L.ERR_INVALID_ARG
    assert lib.mmcmc_hmc_set_state(None, C.cast(x, C.c_void_p), 0, None) == L.ERR_INVALID_ARG
    assert lib.mmcmc_hmc_run_scheduled(None, 1, 1, eps, nl, None, 0, None, None) == L.ERR_INVALID_ARG


def test_jitter_schedule_reproduces_run_chain_of_handles_draws():
    """run_chain_of_handles draws, per launch k, eps_k = rng.uniform(*eps_range) then L_k = rng.integers(lo, hi + 1) from
    numpy's PCG64(schedule_seed); jitter_schedule must give the same pairs, each repeated `block` times."""
    from mini_mcmc_amd.hmc import jitter_schedule

    eps, nl = jitter_schedule(60, 100, (0.004, 0.016), (100, 400), 7)
    assert eps.shape == nl.shape == (6000,) and eps.dtype == np.float64 and nl.dtype == np.int32
    rng = np.random.default_rng(7)
    for k in range(60):
        e = float(rng.uniform(0.004, 0.016))
        n = int(rng.integers(100, 401))
        assert np.all(eps[k * 100:(k + 1) * 100] == e) and np.all(nl[k * 100:(k + 1) * 100] == n)
    assert 0.004 <= eps.min() and eps.max() < 0.016 and 100 <= nl.min() and nl.max() <= 400


def _build_cpp(tmp_path):
    exe = tmp_path / "hmc_fields_test"
    libdir = os.path.join(ROOT, "mini_mcmc_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "hmc_fields_test.cpp"), "-o", str(exe), "-L", libdir, "-lmmcmc",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return str(exe)


def test_cpp_facade_fields_compile_and_fail_loudly_without_gpu(tmp_path):
    """mmcmc.hpp's HMC setters / run_scheduled compile against the facade; without a GPU the first call fails with
    MMCMC_ERR_NO_DEVICE, with one the program checks run_scheduled against the loop of setters and steps."""
    import torch

    mode = "1" if torch.cuda.is_available() else "0"
    out = subprocess.run([_build_cpp(tmp_path), mode], capture_output=True, text=True)
    want = "hmc fields ok (gpu)" if mode == "1" else "hmc fields ok (no gpu"
    assert out.returncode == 0 and want in out.stdout, out.stdout + out.stderr


# ---------------------------------------------------------------------------------------------------------------- GPU

def _init(dim, dtype, n=N, seed=42, scale=1.0):
    from mini_mcmc_amd.core import init_with_seed

    return (init_with_seed(n, dim, seed) * scale).astype(dtype)


def _hmc(target, init, eps, nl, variant=None, seed=11):
    from mini_mcmc_amd.hmc import HMC

    h = HMC(target, init, eps, nl).set_seed(seed)
    if variant is not None:
        h.set_kernel_variant(variant)
    return h


def _schedule(n, seed, eps_lo=0.005, eps_hi=0.03, l_choices=(0, 1, 3, 7, 10, 12)):
    rng = np.random.default_rng(seed)
    return rng.uniform(eps_lo, eps_hi, n), rng.choice(np.array(l_choices, dtype=np.int32), n).astype(np.int32)


def _loop(h, eps, nl, n_discard):
    """the definition: per transition set (eps_k, L_k) and do one transition; keep rows k >= n_discard"""
    rows, acc = [], np.zeros(h.n_chains, dtype=np.uint64)
    for k in range(len(eps)):
        h.step_size = float(eps[k])
        h.n_leapfrog = int(nl[k])
        r = h.run(1 if k >= n_discard else 0, 0 if k >= n_discard else 1)
        acc += h.accept_counts
        if k >= n_discard:
            rows.append(r)
    return np.concatenate(rows, axis=1), acc


@pytest.mark.gpu
def test_setters_before_the_first_run_equal_a_fresh_handle():
    from mini_mcmc_amd.distributions import RosenbrockND

    init = _init(3, np.float32)
    h = _hmc(RosenbrockND(3), init, 0.05, 4)
    h.step_size = 0.021
    h.n_leapfrog = 9
    assert h.step_size == 0.021 and h.n_leapfrog == 9
    a = h.run(30, 10)
    f = _hmc(RosenbrockND(3), init, 0.021, 9)
    b = f.run(30, 10)
    assert np.array_equal(a, b) and np.array_equal(h.accept_counts, f.accept_counts)
    assert np.array_equal(h.state(), f.state())


@pytest.mark.gpu
@pytest.mark.parametrize("source", ["host", "device"])
def test_set_state_equals_a_fresh_handle_on_those_positions(source):
    import torch

    from mini_mcmc_amd.distributions import RosenbrockND

    x0, x1 = _init(3, np.float32), _init(3, np.float32, seed=5, scale=0.5)
    h = _hmc(RosenbrockND(3), x0, 0.02, 10)
    h.run(5, 3)  # the iteration counter moves on: 8
    h.positions = torch.from_numpy(x1).to("cuda:0") if source == "device" else x1
    assert np.array_equal(h.positions, x1)
    a = h.run(20, 4)
    f = _hmc(RosenbrockND(3), x1, 0.02, 10)
    f.run(0, 8)  # the same iteration counter, then the same positions
    f.positions = x1
    b = f.run(20, 4)
    assert np.array_equal(a, b) and np.array_equal(h.accept_counts, f.accept_counts)
    assert np.array_equal(h.state(), f.state())
    # before the first run: equal to a handle constructed on x1
    g = _hmc(RosenbrockND(3), x1, 0.02, 10)
    h2 = _hmc(RosenbrockND(3), x0, 0.02, 10)
    h2.positions = torch.from_numpy(x1).to("cuda:0") if source == "device" else x1
    assert np.array_equal(h2.run(20, 4), g.run(20, 4)) and np.array_equal(h2.state(), g.state())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,variant", [(np.float32, None), (np.float64, None), (np.float32, 0)])
def test_per_transition_schedule_equals_the_loop(dtype, variant):
    from mini_mcmc_amd.distributions import RosenbrockND

    init = _init(3, dtype)
    eps, nl = _schedule(40, 3)
    h = _hmc(RosenbrockND(3), init, 0.02, 10, variant)
    a = h.run_scheduled(eps, nl, 30)
    assert h.step_size == 0.02 and h.n_leapfrog == 10
    ref = _hmc(RosenbrockND(3), init, 0.02, 10, variant)
    b, acc = _loop(ref, eps, nl, 10)
    assert a.shape == (N, 30, 3)
    assert np.array_equal(a, b) and np.array_equal(h.accept_counts, acc)
    assert np.array_equal(h.state(), ref.state())
    # the iteration counters agree: one more plain transition on both
    ref.step_size, ref.n_leapfrog = 0.02, 10
    assert np.array_equal(h.run(3, 0), ref.run(3, 0))


def _gaussian_nd(dim):
    from mini_mcmc_amd.distributions import GaussianND

    rng = np.random.default_rng(dim)
    a = rng.standard_normal((dim, dim)) / np.sqrt(dim)
    return GaussianND(a @ a.T + np.eye(dim))


def _case(name):
    """(target, dim, dtype, variant to force or None, the variant expected in use, n_chains)"""
    from mini_mcmc_amd import distributions as D

    if name == "f32-rosenbrock3-v5":
        return D.RosenbrockND(3), 3, np.float32, None, 5, N
    if name == "f32-rosenbrock3-v2":
        return D.RosenbrockND(3), 3, np.float32, 2, 2, N
    if name == "f32-rosenbrock3-v0":
        return D.RosenbrockND(3), 3, np.float32, 0, 0, N
    if name == "f64-rosenbrock3-v2":
        return D.RosenbrockND(3), 3, np.float64, None, 2, N
    if name == "f32-standardnormal40-v6":
        return D.StandardNormal(40), 40, np.float32, None, 6, N
    if name == "f64-gaussiannd16-v3":
        return _gaussian_nd(16), 16, np.float64, None, 3, N
    if name == "f32-standardnormal256-v8":
        return D.StandardNormal(256), 256, np.float32, 8, 8, N
    if name == "f32-user-rosenbrock3-v7":
        from test_user_target import ROSENBROCK3

        return D.UserTarget("rosenbrock3_sched", 3, ROSENBROCK3), 3, np.float32, None, 7, N
    raise KeyError(name)


CASES = ["f32-rosenbrock3-v5", "f32-rosenbrock3-v2", "f32-rosenbrock3-v0", "f64-rosenbrock3-v2", "f32-standardnormal40-v6",
         "f64-gaussiannd16-v3", "f32-standardnormal256-v8", "f32-user-rosenbrock3-v7"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_block_constant_schedule_equals_runs_per_block(name):
    """One scheduled call against `set (eps, L); run(n_k, 0)` per block on one handle, concatenated -- on every variant:
    the scheduled kernels (5, 2) and the segmented fallback (0, 6, 3, 8, 7)."""
    target, dim, dtype, force, expect, n = _case(name)
    scale = 0.1 if dim > 8 else 1.0
    init = _init(dim, dtype, n=n, scale=scale)
    blocks = [(0.011, 10, 7), (0.023, 3, 12), (0.017, 0, 5), (0.011, 10, 9), (0.008, 6, 1)]
    if dim > 8:
        blocks = [(e * 0.5, l, k) for e, l, k in blocks]
    eps = np.concatenate([np.full(k, e) for e, _, k in blocks])
    nl = np.concatenate([np.full(k, l, dtype=np.int32) for _, l, k in blocks])
    h = _hmc(target, init, 0.01, 5, force)
    assert h.kernel_variant == expect
    a = h.run_scheduled(eps, nl, len(eps))
    ref = _hmc(target, init, 0.01, 5, force)
    parts, acc = [], np.zeros(n, dtype=np.uint64)
    for e, l, k in blocks:
        ref.step_size, ref.n_leapfrog = e, l
        parts.append(ref.run(k, 0))
        acc += ref.accept_counts
    assert np.array_equal(a, np.concatenate(parts, axis=1))
    assert np.array_equal(h.accept_counts, acc)
    assert np.array_equal(h.state(), ref.state())
    assert h.step_size == 0.01 and h.n_leapfrog == 5


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n_leap", [10, 7])
def test_constant_schedule_equals_plain_run(dtype, n_leap):
    """L = 10 runs the unrolled instances in a plain run (split10 / pp10) and the run-time L scheduled ones here"""
    from mini_mcmc_amd.distributions import RosenbrockND

    init = _init(3, dtype)
    h = _hmc(RosenbrockND(3), init, 0.019, n_leap)
    a = h.run_scheduled(np.full(50, 0.019), np.full(50, n_leap, dtype=np.int32), 37)
    f = _hmc(RosenbrockND(3), init, 0.019, n_leap)
    b = f.run(37, 13)
    assert np.array_equal(a, b) and np.array_equal(h.accept_counts, f.accept_counts)
    assert np.array_equal(h.state(), f.state())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,variant", [(np.float32, None), (np.float64, None), (np.float32, 0)])
def test_schedule_with_iters_per_launch_equals_unchunked(dtype, variant):
    """chunks index the schedule from the RUN's first iteration"""
    from mini_mcmc_amd.distributions import RosenbrockND

    init = _init(3, dtype)
    eps, nl = _schedule(45, 9)
    h = _hmc(RosenbrockND(3), init, 0.02, 10, variant)
    h.run(3, 2)  # the run does not start at iteration 0
    h.set_iters_per_launch(7)
    a = h.run_scheduled(eps, nl, 31)
    assert h.timing()["n_launches"] >= 7
    f = _hmc(RosenbrockND(3), init, 0.02, 10, variant)
    f.run(3, 2)
    b = f.run_scheduled(eps, nl, 31)
    assert np.array_equal(a, b) and np.array_equal(h.accept_counts, f.accept_counts)
    assert np.array_equal(h.state(), f.state())


@pytest.mark.gpu
def test_bad_arguments_are_refused_and_fields_survive():
    from mini_mcmc_amd import _lib as L
    from mini_mcmc_amd.distributions import RosenbrockND

    lib = L.lib()
    init = _init(3, np.float32, n=256)
    h = _hmc(RosenbrockND(3), init, 0.02, 10)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)

    def sched(eps, nl, n_collect=2, n_discard=1):
        e = np.ascontiguousarray(eps, dtype=np.float64)
        n = np.ascontiguousarray(nl, dtype=np.int32)
        return lib.mmcmc_hmc_run_scheduled(h._h, n_collect, n_discard, e.ctypes.data_as(dp), n.ctypes.data_as(ip), None, 0,
                                           None, None)

    for bad in (np.nan, np.inf, -np.inf, 0.0, -0.1):
        assert lib.mmcmc_hmc_set_step_size(h._h, bad) == L.ERR_INVALID_ARG
        assert sched([0.02, bad, 0.02], [1, 1, 1]) == L.ERR_INVALID_ARG
    assert lib.mmcmc_hmc_set_n_leapfrog(h._h, -1) == L.ERR_INVALID_ARG
    assert sched([0.02, 0.02, 0.02], [1, -1, 1]) == L.ERR_INVALID_ARG
    assert lib.mmcmc_hmc_run_scheduled(h._h, 2, 1, None, None, None, 0, None, None) == L.ERR_INVALID_ARG
    e = np.full(3, 0.02)
    assert lib.mmcmc_hmc_run_scheduled(h._h, 2, 1, e.ctypes.data_as(dp), None, None, 0, None, None) == L.ERR_INVALID_ARG
    assert lib.mmcmc_hmc_run_scheduled(h._h, 0, 0, None, None, None, 0, None, None) == L.OK  # nothing to do
    assert lib.mmcmc_hmc_set_state(h._h, None, 0, None) == L.ERR_INVALID_ARG
    host = np.zeros((256, 3), dtype=np.float32)
    assert lib.mmcmc_hmc_set_state(h._h, host.ctypes.data, 1, None) == L.ERR_INVALID_ARG  # host memory flagged as device
    assert h.step_size == 0.02 and h.n_leapfrog == 10
    assert np.array_equal(h.state(), init)  # nothing ran
    h.run_scheduled([0.03, 0.01, 0.002], [0, 4, 20], 2)
    assert h.step_size == 0.02 and h.n_leapfrog == 10
    with pytest.raises(ValueError):
        h.run_scheduled([0.03, 0.01], [1], 1)
    with pytest.raises(ValueError):
        h.positions = np.zeros((255, 3), dtype=np.float32)


@pytest.mark.gpu
def test_rosenbrock3_run_jittered_converges():
    """run_chain_of_handles' converged workload (test_rosenbrock3_hmc_converges_as_a_chain_of_handles) on one handle and one
    scheduled launch, with that test's assertions"""
    import mini_mcmc_amd as M
    from mini_mcmc_amd import stats as S
    from mini_mcmc_amd.hmc import jitter_schedule, run_jittered

    x0 = np.linspace(-5.0, 6.0, 220001)
    w = np.exp(-(1 - x0) ** 2 - (100.0 / 101.0) * (1 - x0 ** 2) ** 2)
    w /= w.sum()
    mu1, s1 = (100.0 * x0 ** 2 + 1.0) / 101.0, 1.0 / 202.0
    m0, m1 = (w * x0).sum(), (w * mu1).sum()
    e1sq = (w * (mu1 ** 2 + s1)).sum()
    e14 = (w * (mu1 ** 4 + 6 * mu1 ** 2 * s1 + 3 * s1 ** 2)).sum()
    mean = np.array([m0, m1, e1sq])
    var = np.array([(w * (x0 - m0) ** 2).sum(), e1sq - m1 ** 2, e14 + 1.0 / 200.0 - e1sq ** 2])
    t, info = run_jittered(M.distributions.RosenbrockND(3), M.core.init_with_seed(65536, 3, 42, np.float32), (0.004, 0.016),
                           (100, 400), 100, 20, 40, seed=42)
    eps, nl = jitter_schedule(60, 100, (0.004, 0.016), (100, 400), 7)
    assert info["schedule_head"] == [(float(eps[k * 100]), int(nl[k * 100])) for k in range(4)]
    assert t.shape == (65536, 4000, 3) and info["launches"] == 1 and 0.85 < info["accept_rate"] < 0.999
    assert info["wall_ms"] >= info["kernel_ms"] > 0
    rhat, ess = S.split_rhat_mean_ess(t)
    assert float((1.0 / rhat).max()) <= 1.05, rhat
    assert float(ess.min()) > 5e6, ess
    x = t.double().reshape(-1, 3)
    np.testing.assert_allclose(x.mean(dim=0).cpu().numpy(), mean, rtol=0.01)
    np.testing.assert_allclose(x.var(dim=0).cpu().numpy(), var, rtol=0.01)
