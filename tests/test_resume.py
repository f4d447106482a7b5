"""Settable chain state on every sampler, and checkpoint / resume (include/mmcmc.h: "chain state and stream position").

The engine's noise is keyed by (seed, global chain id, iteration) alone, so a handle given another's positions, fields,
stream position and (NUTS) adaptation records continues exactly as that one does.  The core property, checked bit for bit:
run A; ckpt = A.checkpoint(); run A again.  B, built with other positions and another seed, restore(ckpt) and the same run:
samples, final state, accept counts, NUTS's adaptation and the leapfrog counts the run added are equal."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 2048

NEW_ENTRY_POINTS = [
    "mmcmc_mh_set_proposal_std", "mmcmc_mh_params", "mmcmc_mh_set_state", "mmcmc_nuts_set_state",
    "mmcmc_nuts_set_adapt_state", "mmcmc_nuts_params", "mmcmc_nuts_set_target_accept_p", "mmcmc_mh_discrete_set_state",
    "mmcmc_gibbs_mixture_set_state", "mmcmc_hmc_group_set_state", "mmcmc_mh_group_set_state", "mmcmc_nuts_group_set_state",
    "mmcmc_hmc_group_set_step_size", "mmcmc_hmc_group_set_n_leapfrog", "mmcmc_hmc_group_params",
    "mmcmc_mh_group_set_proposal_std", "mmcmc_mh_group_params", "mmcmc_nuts_group_adapt_state",
    "mmcmc_nuts_group_set_adapt_state", "mmcmc_nuts_group_params", "mmcmc_nuts_group_set_target_accept_p",
] + [f"mmcmc_{p}_{f}" for p in ("mh", "hmc", "nuts", "mh_discrete", "gibbs_mixture", "hmc_group", "mh_group", "nuts_group")
     for f in ("stream_position", "set_iteration")]


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_new_entry_points_reject_a_null_handle():
    from mini_mcmc_amd import _lib as L

    lib = L.lib()
    buf = (C.c_double * 64)()
    for name in NEW_ENTRY_POINTS:
        fn = getattr(lib, name)
        args = [None]
        for t in fn.argtypes[1:]:
            if t in (C.c_double,):
                args.append(0.5)
            elif t in (C.c_int, C.c_uint64):
                args.append(1)
            else:
                args.append(C.cast(buf, t) if t is not C.c_void_p else C.cast(buf, C.c_void_p))
        assert fn(*args) == L.ERR_INVALID_ARG, name


def test_new_entry_points_are_declared_and_listed_in_the_version_note():
    src = open(os.path.join(ROOT, "include", "mmcmc.h")).read()
    for name in NEW_ENTRY_POINTS:
        assert f"int {name}(" in src, name
    assert "#define MMCMC_VERSION 102" in src


def _build_cpp(tmp_path):
    exe = tmp_path / "resume_test"
    libdir = os.path.join(ROOT, "mini_mcmc_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "resume_test.cpp"), "-o", str(exe), "-L", libdir, "-lmmcmc",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return str(exe)


def test_cpp_facade_compiles_and_fails_loudly_without_gpu(tmp_path):
    """mmcmc.hpp's setters and stream positions compile (every member of the class templates is instantiated); without
    a GPU the first constructor fails with MMCMC_ERR_NO_DEVICE, with one the program checks a resumed continuation."""
    import torch

    mode = "1" if torch.cuda.is_available() else "0"
    out = subprocess.run([_build_cpp(tmp_path), mode], capture_output=True, text=True)
    want = "resume ok (gpu)" if mode == "1" else "resume ok (no gpu"
    assert out.returncode == 0 and want in out.stdout, out.stdout + out.stderr


def _sample_ckpt():
    rng = np.random.default_rng(1)
    return {"format": 1, "sampler": "nuts", "n_chains": 3, "dim": 2, "dtype": "float32", "mode": 1, "target_kind": 4,
            "seed": 2 ** 64 - 1, "first_global_chain": 12, "iteration": 2 ** 32 - 1, "target_accept_p": 0.8, "max_depth": 10,
            "positions": rng.standard_normal((3, 2)).astype(np.float32),
            "adapt": np.array([[-1.0, 1.0, 0.0, np.log(10.0)]] * 3)}


def test_checkpoint_file_round_trip_without_pickle(tmp_path):
    from mini_mcmc_amd import checkpoint as K

    ck = _sample_ckpt()
    ck["mode"] = -1
    p = tmp_path / "c.npz"
    K.save(p, ck)
    back = K.load(p)
    assert set(back) == set(ck)
    for k, v in ck.items():
        if isinstance(v, np.ndarray):
            assert back[k].dtype == v.dtype and np.array_equal(back[k], v), k
        else:
            assert type(back[k]) is type(v) and back[k] == v, k
    with np.load(p, allow_pickle=False) as z:  # readable without pickle: no object arrays inside
        assert all(z[k].dtype != object for k in z.files)
    for bad in ({"x": np.array([None], dtype=object)}, {"x": True}, {"x": [1, 2]}):
        with pytest.raises(TypeError):
            K.save(tmp_path / "bad.npz", bad)


def test_adaptation_rows_are_checked_on_the_host():
    from mini_mcmc_amd import checkpoint as K

    good = np.array([[0.1, 0.2, 0.0, 1.0], [-1.0, 1.0, 0.0, 2.3]])
    assert np.array_equal(K.check_adapt(good, 2, 0), good)
    for bad in ([[np.nan, 1, 0, 1], [0.1, 1, 0, 1]], [[0.0, 1, 0, 1], [0.1, 1, 0, 1]], [[-0.5, 1, 0, 1], [0.1, 1, 0, 1]],
                [[0.1, np.inf, 0, 1], [0.1, 1, 0, 1]], [[0.1, 1, 0, 1]]):
        with pytest.raises(ValueError):
            K.check_adapt(bad, 2, 0)
    with pytest.raises(ValueError):  # finite in f64, not in mode 1's f32 scalars
        K.check_adapt([[0.1, 1e300, 0, 1], [0.1, 1, 0, 1]], 2, 1)


# ---------------------------------------------------------------------------------------------------------------- GPU

def _init(n, dim, seed, dtype=np.float32, scale=1.0):
    from mini_mcmc_amd.core import init_with_seed

    return (init_with_seed(n, dim, seed) * scale).astype(dtype)


def _gaussian_nd(dim):
    from mini_mcmc_amd.distributions import GaussianND

    return GaussianND.ill_conditioned(dim, 10.0, 3)


def _user_rosenbrock3():
    from mini_mcmc_amd.distributions import UserTarget

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_user_target import ROSENBROCK3

    return UserTarget("rosenbrock3", 3, ROSENBROCK3)


def _resume_equal(make, run1, run2, extra=None):
    """A: make(init 1, seed 11); run1; checkpoint; run2.  B: make(init 2, seed 99); restore; run2.  Everything equal."""
    a = make(0)
    run1(a)
    ck = a.checkpoint()
    before_a = extra(a) if extra else None
    ra = run2(a)
    b = make(1)
    b.restore(ck)
    assert b.checkpoint()["iteration"] == ck["iteration"]
    before_b = extra(b) if extra else None
    rb = run2(b)
    for x, y in zip(ra, rb):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    if extra:
        assert np.array_equal(extra(a) - before_a, extra(b) - before_b)
    return a, b


def _run_sampler(n_collect, n_discard):
    def f(h):
        s = h.run(n_collect, n_discard)
        return s, h.accept_counts, h.state()
    return f


MH_CASES = [(v, dt) for v in (0, 2, 5, 6) for dt in (np.float32, np.float64)]


@pytest.mark.gpu
@pytest.mark.parametrize("variant,dtype", MH_CASES)
def test_mh_resume(variant, dtype):
    from mini_mcmc_amd.distributions import IsotropicGaussian, RosenbrockND
    from mini_mcmc_amd.metropolis_hastings import MetropolisHastings

    def make(k):
        h = MetropolisHastings(RosenbrockND(3), IsotropicGaussian((0.3, 0.9)[k]), _init(N, 3, (42, 7)[k], dtype))
        return h.seed((11, 99)[k]).set_kernel_variant(variant)

    _resume_equal(make, lambda h: h.run(7, 13), _run_sampler(25, 6))


HMC_CASES = ["rosenbrock3-v0", "rosenbrock3-v2", "rosenbrock3-v5", "rosenbrock3-v6", "gaussiannd16-v3", "gaussiannd32-v3",
             "rosenbrock64-v8", "user-rosenbrock3"]


def _hmc_case(name):
    from mini_mcmc_amd import distributions as D

    if name.startswith("rosenbrock3"):
        return D.RosenbrockND(3), 3, int(name[-1])
    if name.startswith("gaussiannd"):
        return _gaussian_nd(int(name[10:12])), int(name[10:12]), 3
    if name == "rosenbrock64-v8":
        return D.RosenbrockND(64), 64, 8
    return _user_rosenbrock3(), 3, None


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("case", HMC_CASES)
def test_hmc_resume(case, dtype):
    from mini_mcmc_amd.hmc import HMC

    target, dim, variant = _hmc_case(case)
    n = 256 if variant == 8 else N

    def make(k):
        h = HMC(target, _init(n, dim, (42, 7)[k], dtype, 0.5), (0.02, 0.05)[k], (6, 3)[k]).set_seed((11, 99)[k])
        if variant is not None:
            h.set_kernel_variant(variant)
        assert variant is None or h.kernel_variant == variant
        return h

    _resume_equal(make, lambda h: h.run(5, 4), _run_sampler(12, 3))


NUTS_CASES = [(v, m) for v in (0, 4, 5, 6) for m in (0, 1, 2)] + [(v, 2) for v in (1, 2, 3)] + [("user", 0), ("user", 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("variant,mode", NUTS_CASES)
def test_nuts_resume(variant, mode):
    """The first run ends inside warm-up (m = 24 < n_discard of the second run = 40): restoring m and h_bar matters."""
    from mini_mcmc_amd.distributions import RosenbrockND
    from mini_mcmc_amd.nuts import NUTS

    dims = [16, 32] if variant in (1, 2, 3) else [3]
    for dim in dims:
        target = _user_rosenbrock3() if variant == "user" else _gaussian_nd(dim) if variant in (1, 2, 3) else RosenbrockND(3)
        n = 4096 if variant in (1, 2, 3) else N

        def make(k):
            h = NUTS(target, _init(n, dim, (42, 7)[k], np.float64, 0.5), (0.8, 0.6)[k], mode=mode).set_seed((11, 99)[k])
            if variant != "user":
                h.set_kernel_variant(variant)
            if k:
                h.set_max_depth(6)
            return h

        def run2(h):
            s = h.run(10, 40)
            a = h.adapt_state()
            return s, h.positions(), np.stack([a[k] for k in ("epsilon", "epsilon_bar", "h_bar", "mu")], 1)

        a, b = _resume_equal(make, lambda h: h.run(5, 20), run2, extra=lambda h: h.leapfrog_counts())
        assert a.stream_position()[2] == b.stream_position()[2] == 24 + 49
        if variant == "user":
            assert a.kernel_variant == 7


@pytest.mark.gpu
def test_discrete_and_gibbs_resume():
    from mini_mcmc_amd.discrete import BinomialClamp, DiscreteMetropolisHastings
    from mini_mcmc_amd.gibbs import GibbsSampler, MixtureConditional

    def make_d(k):
        return DiscreteMetropolisHastings(BinomialClamp(20, 0.3), np.arange(8192) % (7, 13)[k]).seed((11, 99)[k])

    def run_d(h):
        acc0 = h.accept_counts()
        s = h.run(30, 5)
        return s, h.state(), h.accept_counts() - acc0

    _resume_equal(make_d, lambda h: h.run(4, 9), run_d)
    mix = MixtureConditional(-2.0, 1.0, 3.0, 0.5, 0.3)

    def make_g(k):
        x = np.stack([_init(8192, 1, (42, 7)[k], np.float64)[:, 0], np.zeros(8192)], 1)
        return GibbsSampler(mix, x).set_seed((11, 99)[k])

    _resume_equal(make_g, lambda h: h.run(4, 9), lambda h: (h.run(30, 5), h.state()))


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, {root!r})
from mini_mcmc_amd import checkpoint as K
from mini_mcmc_amd.core import init_with_seed
from mini_mcmc_amd.distributions import RosenbrockND
from mini_mcmc_amd.hmc import HMC
path, out, step = sys.argv[1], sys.argv[2], sys.argv[3]
if step == "first":
    h = HMC(RosenbrockND(3), init_with_seed(2048, 3, 42).astype(np.float32), 0.02, 6).set_seed(11)
    h.run(5, 4)
    K.save(path, h.checkpoint())
else:
    h = HMC(RosenbrockND(3), init_with_seed(2048, 3, 7).astype(np.float32), 0.05, 3).set_seed(99)
    h.restore(K.load(path))
    s = h.run(12, 3)
    np.savez(out, s=s, acc=h.accept_counts, x=h.state())
"""


@pytest.mark.gpu
def test_resume_in_another_process(tmp_path):
    from mini_mcmc_amd.distributions import RosenbrockND
    from mini_mcmc_amd.hmc import HMC

    script = tmp_path / "child.py"
    script.write_text(_CHILD.format(root=ROOT))
    ck, out = str(tmp_path / "ck.npz"), str(tmp_path / "out.npz")
    flags = ["-s"] if sys.flags.no_user_site else []
    for step in ("first", "second"):
        r = subprocess.run([sys.executable, *flags, str(script), ck, out, step], capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
    a = HMC(RosenbrockND(3), _init(2048, 3, 42), 0.02, 6).set_seed(11)
    a.run(5, 4)
    s = a.run(12, 3)
    with np.load(out) as z:
        assert np.array_equal(z["s"], s) and np.array_equal(z["acc"], a.accept_counts) and np.array_equal(z["x"], a.state())


def _group_and_single(kind, devices, k):
    from mini_mcmc_amd import group as G
    from mini_mcmc_amd.distributions import IsotropicGaussian, RosenbrockND
    from mini_mcmc_amd.hmc import HMC
    from mini_mcmc_amd.metropolis_hastings import MetropolisHastings
    from mini_mcmc_amd.nuts import NUTS

    n, t = 1000, RosenbrockND(3)
    x = _init(n, 3, (42, 7)[k], np.float64 if kind == "nuts" else np.float32, 0.5)
    seed = (11, 99)[k]
    if kind == "hmc":
        return (G.HMCGroup(t, x, 0.02, 6, devices=devices).set_seed(seed) if devices else HMC(t, x, 0.02, 6).set_seed(seed))
    if kind == "mh":
        p = IsotropicGaussian((0.3, 0.8)[k])
        return G.MetropolisHastingsGroup(t, p, x, devices=devices).seed(seed) if devices else MetropolisHastings(t, p, x).seed(seed)
    return G.NUTSGroup(t, x, 0.8, mode=0, devices=devices).set_seed(seed) if devices else NUTS(t, x, 0.8, mode=0).set_seed(seed)


def _advance(h, kind, first):
    if kind == "nuts":
        return h.run(5, 20) if first else h.run(10, 40)
    return h.run(6, 5) if first else h.run(14, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["hmc", "mh", "nuts"])
def test_resume_across_shard_counts(kind):
    """A group on [0, 0, 0] (shards of 333, 333 and 334 chains) restored into a single handle and into [0]; a single handle
    restored into the group on [0, 0, 0].  Group and handle checkpoints have one layout."""
    for src, dsts in (([0, 0, 0], [None, [0]]), (None, [[0, 0, 0]])):
        a = _group_and_single(kind, src, 0)
        _advance(a, kind, True)
        ck = a.checkpoint()
        ref = _advance(a, kind, False)
        ref_x = a.checkpoint()["positions"]
        ref_ad = a.checkpoint().get("adapt")
        for dst in dsts:
            b = _group_and_single(kind, dst, 1)
            b.restore(ck)
            assert np.array_equal(_advance(b, kind, False), ref) and np.array_equal(b.checkpoint()["positions"], ref_x)
            if kind == "nuts":
                assert np.array_equal(b.checkpoint()["adapt"], ref_ad)
            else:
                assert np.array_equal(b.accept_counts, a.accept_counts)


@pytest.mark.gpu
def test_mh_fields_before_the_first_run_equal_a_fresh_handle():
    import torch

    from mini_mcmc_amd.distributions import IsotropicGaussian, RosenbrockND
    from mini_mcmc_amd.metropolis_hastings import MetropolisHastings

    x0, x1 = _init(N, 3, 42), _init(N, 3, 5, scale=0.5)
    fresh = MetropolisHastings(RosenbrockND(3), IsotropicGaussian(0.37), x1).seed(3)
    want = fresh.run(20, 5)
    for path in ("host", "torch"):
        h = MetropolisHastings(RosenbrockND(3), IsotropicGaussian(1.0), x0).seed(3)
        h.proposal_std = 0.37
        h.positions = torch.from_numpy(x1).to("cuda:0") if path == "torch" else x1
        assert h.proposal_std == 0.37 and np.array_equal(h.positions, x1)
        assert h.stream_position() == (3, 0, 0)
        assert np.array_equal(h.run(20, 5), want) and np.array_equal(h.accept_counts, fresh.accept_counts)
        assert np.array_equal(h.state(), fresh.state())


@pytest.mark.gpu
def test_bad_arguments_are_refused_and_change_nothing():
    from mini_mcmc_amd import _lib as L
    from mini_mcmc_amd import group as G
    from mini_mcmc_amd.distributions import IsotropicGaussian, RosenbrockND, StandardNormal
    from mini_mcmc_amd.hmc import HMC
    from mini_mcmc_amd.metropolis_hastings import MetropolisHastings
    from mini_mcmc_amd.nuts import NUTS

    mh = MetropolisHastings(RosenbrockND(3), IsotropicGaussian(0.5), _init(256, 3, 42)).seed(4)
    mh.run(3, 2)
    ck = mh.checkpoint()
    for std in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(L.MmcmcError):
            mh.proposal_std = std
    for it in (2 ** 32, 2 ** 40):
        with pytest.raises(ValueError):
            mh.set_iteration(it)
        assert L.lib().mmcmc_mh_set_iteration(mh._h, it) == L.ERR_INVALID_ARG
    with pytest.raises(ValueError):
        mh.positions = np.zeros((256, 4), np.float32)
    for bad in ({**ck, "sampler": "hmc"}, {**ck, "n_chains": 255}, {**ck, "dim": 2}, {**ck, "dtype": "float64"},
                {**ck, "target_kind": StandardNormal.kind}, {**ck, "iteration": 2 ** 32}, {**ck, "proposal_std": 0.0},
                {**ck, "positions": ck["positions"].astype(np.float64)}, {**ck, "positions": ck["positions"][:, :2].copy()},
                {**ck, "seed": 1, "positions": ck["positions"][:10]}):
        with pytest.raises(ValueError):
            mh.restore(bad)
    after = mh.checkpoint()
    for k in ck:
        assert np.array_equal(after[k], ck[k]) if isinstance(ck[k], np.ndarray) else after[k] == ck[k], k

    nuts = NUTS(RosenbrockND(3), _init(256, 3, 42, np.float64), 0.8, mode=1).set_seed(2)
    nuts.run(3, 10)
    ad = nuts.adapt_state()
    rows = np.stack([ad[k] for k in ("epsilon", "epsilon_bar", "h_bar", "mu")], 1)
    for bad_rows in (np.where(np.arange(4) == 2, np.nan, rows), np.where(np.arange(4) == 0, 0.0, rows),
                     np.where(np.arange(4) == 0, -0.5, rows)):
        assert L.lib().mmcmc_nuts_set_adapt_state(nuts._h, np.ascontiguousarray(bad_rows).ctypes.data_as(
            C.POINTER(C.c_double))) == L.ERR_INVALID_ARG
        with pytest.raises(ValueError):
            nuts.set_adapt_state(bad_rows)
    with pytest.raises(ValueError):
        nuts.set_adapt_state(rows[:, :3])
    with pytest.raises(ValueError):
        nuts.restore({**nuts.checkpoint(), "mode": 0})
    back = nuts.adapt_state()
    assert all(np.array_equal(back[k], ad[k]) for k in ad)
    nuts.set_adapt_state(rows)  # a round trip is exact in mode 1 (f32 through f64)
    back = nuts.adapt_state()
    assert all(np.array_equal(back[k], ad[k]) for k in ad)

    hg = G.HMCGroup(RosenbrockND(3), _init(300, 3, 1), 0.02, 5, devices=[0, 0])
    for eps in (0.0, float("nan")):
        with pytest.raises(L.MmcmcError):
            hg.step_size = eps
    with pytest.raises(L.MmcmcError):
        hg.n_leapfrog = -1
    assert hg.step_size == 0.02 and hg.n_leapfrog == 5
    with pytest.raises(ValueError):
        hg.restore({**HMC(RosenbrockND(3), _init(300, 3, 1), 0.02, 5).checkpoint(), "dtype": "float64"})
    # a group's setters go through the same checks
    assert L.lib().mmcmc_hmc_group_set_iteration(hg._h, 2 ** 32) == L.ERR_INVALID_ARG
    assert hg.stream_position() == (0, 0, 0)
