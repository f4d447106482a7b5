"""The in-library collective branch of group_split_rhat_ess (csrc/mm_group.hip) with N > 1 ranks, against float64.

RCCL refuses one device twice and the GPU box has one device, so tests/test_device_group.py reaches that branch -- the
all-gather of [means | ssq] slots padded to the largest shard, the all-reduce of the lag sums, mm_group_cross_sums_kernel
with gridDim.y = N and per-rank counts, the f64 finish over N x 4 partial sums -- with one rank only.  Here the four
collective entry points are bound (mmcmc_group_bind_collectives) from tests/c/fake_collectives.c, a stand-in that carries them
out with host threads and HIP copies and accepts several ranks on one device, so the branch runs with 2, 3, 4, 8 and 64 ranks.
The binding holds for the life of a process: it happens in a fresh child (tests/group_collectives_child.py), one for all
cases and one for the failing-initialisation fallback, never in the pytest process; the child writes samples and results,
this file does the float64 work (oracle/stats_f64.py) and the assertions.

Cases (ranks, chains (shards), sampler, run -- what it reaches):
  n2-mh-2chains       2, 2 (1, 1), MH Gaussian2D f32, run(8)                   smallest group: c2 = 2, per = 1, quarters 2, 3 empty
  n3-hmc-7chains-odd  3, 7 (3, 2, 2), HMC RosenbrockND(3) f32, run(123)        padding behind ranks 1 and 2; m = 61, m D odd: the
                                                                               f64 area behind the lag sums is rounded up
  n3-hmc-1000         3, 1000 (334, 333, 333), HMC, run(120, 30)               the shape of test_group_reproduces_single_handle_run
  n3-mh-f64-offset    3, 257, MH Gaussian2D f64, chain offset 1 << 33, run(64, 8)   the f64 sample path
  n8-hmc-4803         8, 4803 (3 x 601, 5 x 600), HMC, run(100)                config 4's rank count; 2 n_i > 1024: a quarter has more
                                                                               than 256 entries, the strided loop runs more than once
  n64-mh-101          64, 101 (37 x 2, 27 x 1), MH f32, run(16)                the last slot of GroupCounts, gridDim.y = 64
  n3-nuts-d32         3, 100, NUTS GaussianND.ill_conditioned(32, 100, 5) mode 2, run(20, 12)   D = 32: gridDim.x = 128
  n3-mh-far-target    3, 8192, MH Gaussian2D centred at (3000, -2000), run(400, 100)   the shift is rank 0's first entry and is
                                                                               applied to ranks 1 and 2; |rhat - 1| < 0.05
  n4-mh-ramp          4, 403, MH unit Gaussian2D at (5, -3) started on a ramp, run(30)   tells the ranks apart (see its test)
  reuse-0..3          one group of 3 ranks, 1000 chains: run(120, 30), run(50) (a smaller total in a grown buffer, m D = 75 odd),
                      run(301) (regrowth), run(303) (regrowth, m D = 453 odd)

Every case: exchange status 1 with N ranks, one all-gather of 4 cmax D floats and one all-reduce of m D floats per rank per
diagnostics call (the stand-in counts them); the sample equal to the single handle's bit for bit; R-hat / ESS equal to the
single-GPU entry point's on that sample to 2e-6 / 1e-4 (NUTS 2e-4 / 2e-3: the tolerances of tests/test_device_group.py), and
to float64 to 1e-4 / oracle.stats_f64.ess_rtol with the lag-sum bound of tests/test_stats_f64.py for the path the half-chain
length selects (4 eps log2(L) through the transform, 4 eps sqrt(m + c2) through direct sums), NaN by position.
"""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from oracle import stats_f64 as F
from test_stats_f64 import _close, _lag_tol

import group_collectives_child as child

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "fake_collectives.c")
CHILD = os.path.join(ROOT, "tests", "group_collectives_child.py")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
# The children do a few seconds of device work (the largest case is 8192 chains x 500 MH transitions; 64 ranks mean 64 small
# handles) after the start-up of the interpreter, torch and the HIP runtime; the stand-in's own barrier deadline is 30 s and
# must be able to expire inside the limit, so that a rank that never arrives is reported by status, not by the limit.
CHILD_TIMEOUT_S = 90
TOL_SINGLE = {"nuts": (2e-4, 2e-3)}  # (R-hat, ESS) against the single-GPU entry point; MH / HMC: 2e-6 / 1e-4


def build_stand_in(d):
    """tests/c/fake_collectives.c -> a shared library in d (plain C: gcc, the HIP runtime API's header and library)"""
    lib = os.path.join(str(d), "libfake_collectives.so")
    cmd = [shutil.which("gcc") or "gcc", "-std=gnu11", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-I" + os.path.join(ROCM, "include"),
           SRC, "-o", lib, "-L" + os.path.join(ROCM, "lib"), "-lamdhip64", "-lpthread", "-Wl,-rpath," + os.path.join(ROCM, "lib")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    return lib


def test_stand_in_and_binding_entry_point_without_a_device(tmp_path):
    """The stand-in compiles, exports its five symbols and refuses another element type / reduction before it touches
    HIP; libmmcmc.so exports mmcmc_group_bind_collectives, which refuses NULL and a library that cannot be loaded (and so
    leaves the collectives of THIS process unbound)."""
    import mini_mcmc_amd
    from mini_mcmc_amd import _lib as L

    lib = mini_mcmc_amd.lib()  # torch's HIP runtime first, as every user of the package has it
    fake = C.CDLL(build_stand_in(tmp_path))
    for sym in ("ncclCommInitAll", "ncclCommDestroy", "ncclAllGather", "ncclAllReduce", "fake_collectives_counts"):
        assert hasattr(fake, sym), sym
    fake.ncclAllGather.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    fake.ncclAllReduce.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    buf = (C.c_float * 4)()
    comm = (C.c_void_p * 2)()  # never dereferenced: the element type and the reduction are looked at first
    assert fake.ncclAllGather(buf, buf, 4, 0, comm, None) != 0  # dtype 0 is ncclInt8; 7 is ncclFloat32
    assert fake.ncclAllReduce(buf, buf, 4, 7, 1, comm, None) != 0  # op 1 is ncclProd; 0 is ncclSum
    assert fake.ncclAllReduce(buf, buf, 4, 0, 0, comm, None) != 0
    counts = (C.c_size_t * 4)()
    fake.fake_collectives_counts(counts)
    assert list(counts) == [0, 0, 0, 0]
    assert hasattr(lib, "mmcmc_group_bind_collectives") and "mmcmc_group_bind_collectives" in L.SIGNATURES
    assert lib.mmcmc_group_bind_collectives(None, 0) == L.ERR_INVALID_ARG
    assert lib.mmcmc_group_bind_collectives(os.fsencode(str(tmp_path / "no_such_library.so")), 0) == L.ERR_INVALID_ARG
    # a library without the four entry points: libm
    import ctypes.util

    libm = ctypes.util.find_library("m")
    if libm:
        assert lib.mmcmc_group_bind_collectives(libm.encode(), 1) == L.ERR_INVALID_ARG


# ---------------------------------------------------------------- the children (GPU)


def _run_child(d, mode, extra_env):
    """one fresh process under its own time limit: it binds the stand-in, runs, writes, and ends non-zero at the first
    error; a failure raises here, and pytest fails every test that depends on the (module-scoped) fixture without a rerun"""
    lib = build_stand_in(d)
    env = dict(os.environ)
    env.pop("FAKE_COLLECTIVES_FAIL_INIT", None)
    env.update(extra_env)
    r = subprocess.run([sys.executable, CHILD, lib, str(d), mode], capture_output=True, text=True, timeout=CHILD_TIMEOUT_S, env=env)
    assert r.returncode == 0, f"group_collectives_child {mode} ended with {r.returncode}: {r.stdout[-1000:]} {r.stderr[-3000:]}"
    with open(os.path.join(str(d), "results.json")) as f:
        return str(d), json.load(f)


@pytest.fixture(scope="module")
def cases_child(tmp_path_factory):
    return _run_child(tmp_path_factory.mktemp("group_collectives"), "cases", {})


@pytest.fixture(scope="module")
def fallback_child(tmp_path_factory, cases_child):
    """depends on `cases_child`, so it does not start after that one failed"""
    return _run_child(tmp_path_factory.mktemp("group_collectives_fallback"), "fallback", {"FAKE_COLLECTIVES_FAIL_INIT": "1"})


def _shard_sizes(ranks, chains):
    return [chains // ranks + (1 if i < chains % ranks else 0) for i in range(ranks)]


def _check_diagnostics(d, name, sampler):
    """R-hat / ESS of <name>.npz against the single-GPU entry point and against float64 -> (Diagnostics, sample, ratios)"""
    z = np.load(os.path.join(d, name + ".npz"))
    sample, rhat, ess = z["sample"], z["rhat"], z["ess"]
    rt, et = TOL_SINGLE.get(sampler, (2e-6, 1e-4))
    np.testing.assert_allclose(rhat, z["rhat_single"], rtol=rt, err_msg=name)
    np.testing.assert_allclose(ess, z["ess_single"], rtol=et, err_msg=name)
    r = F.diagnostics(sample)
    rhat_ok = _close(rhat, r.rhat, 1e-4, name + " rhat")
    ess_ok = _close(ess, r.ess, F.ess_rtol(r, _lag_tol("auto", r.m, r.c2)), name + " ess")
    print(f"{name}: max error / bound against float64: rhat {rhat_ok:.2e} ess {ess_ok:.2e}")
    return r, z, (rhat_ok, ess_ok)


def _check_exchange(res, ranks, chains, dim, n_collect):
    """status 1 over `ranks` ranks; per diagnostics call every rank asks once for 2 part = 4 cmax D and for m D floats"""
    assert res["exchange"] == [1, ranks] and res["exchange_status"] == 1 and res["used_rccl"]
    assert res["shards"] == _shard_sizes(ranks, chains)
    cmax, m = max(res["shards"]), n_collect // 2
    b, a = res["counts_before"], res["counts_after"]
    assert (a[0] - b[0], a[1] - b[1]) == (ranks, ranks), (b, a)
    assert (a[2], a[3]) == (4 * cmax * dim, m * dim), (a, cmax, m, dim)
    assert res["sample_equal"] and res["accept_equal"]  # against the single handle, bit for bit


@pytest.mark.gpu
@pytest.mark.parametrize("name", [k for k in child.CASES if k != "n4-mh-ramp"])
def test_collective_branch_against_f64(cases_child, name):
    d, results = cases_child
    assert results["bind_again"] == -1  # MMCMC_ERR_INVALID_ARG: already bound
    ranks, chains, sampler, n_collect, _ = child.CASES[name]
    dim = {"hmc": 3, "nuts": 32}.get(sampler, 2)
    _check_exchange(results[name], ranks, chains, dim, n_collect)
    r, z, _ = _check_diagnostics(d, name, sampler)
    assert r.c2 == 2 * chains and r.m == n_collect // 2
    if sampler == "mhfar":  # a converged unit Gaussian far from the origin: with the digits lost this is far off or NaN
        assert np.all(np.abs(z["rhat"] - 1.0) < 0.05)


@pytest.mark.gpu
def test_collective_branch_tells_the_ranks_apart(cases_child):
    """Shards of a converged run are statistically alike: a kernel that read rank 0 in place of rank 1 would hardly move
    R-hat.  Here every chain starts on a ramp across the target, chains are contiguous per shard, and the run is short, so
    the four ranks' half-chain means stand apart.  Before the case is trusted, on the float64 side: the potential scale
    reduction sqrt(var+ / W) is above 1.1 at both parameters -- the library's `rhat` is the reference's sqrt(W / var+)
    (quirk Q7), which never exceeds sqrt(m / (m - 1)), so the condition is put on its reciprocal -- and replacing any
    rank's half-chain means and sums of squares by its neighbour's (truncated or repeated to length) moves R-hat by at
    least 100 times the 1e-4 the comparison allows.  With run(60) the second condition failed (ranks 0, 1, 2 moved R-hat
    by 0.0091, 0.0011, 0.0095 of itself); with run(30) every rank moves it by at least 0.0136 and sqrt(var+ / W) is 1.40
    (measured on the host build of the sampler, whose sample equals the device's bit for bit)."""
    d, results = cases_child
    name = "n4-mh-ramp"
    ranks, chains, sampler, n_collect, _ = child.CASES[name]
    _check_exchange(results[name], ranks, chains, 2, n_collect)
    r, _, _ = _check_diagnostics(d, name, sampler)
    assert np.all(1.0 / r.rhat > 1.1), r.rhat
    sizes = _shard_sizes(ranks, chains)
    first = np.concatenate([[0], np.cumsum(sizes)])
    rows = [np.concatenate([np.arange(first[k], first[k + 1]), chains + np.arange(first[k], first[k + 1])]) for k in range(ranks)]
    for k in range(ranks):
        means, ssq = r.means.copy(), r.ssq.copy()
        other = rows[(k + 1) % ranks]
        for half in range(2):  # splitcat order: the first halves of all chains, then the second halves
            mine = rows[k][half * sizes[k]:(half + 1) * sizes[k]]
            theirs = other[half * sizes[(k + 1) % ranks]:(half + 1) * sizes[(k + 1) % ranks]]
            take = np.resize(theirs, mine.shape)
            means[mine], ssq[mine] = r.means[take], r.ssq[take]
        swapped = F.finish(means, ssq, r.acov, r.c2, r.m)[2]
        moved = np.abs(swapped - r.rhat) / r.rhat
        print(f"{name}: rank {k} replaced by rank {(k + 1) % ranks}: R-hat moves by {moved}")
        assert moved.max() >= 100 * 1e-4, (k, swapped, r.rhat)


@pytest.mark.gpu
def test_collective_branch_reuses_and_regrows_its_buffer(cases_child):
    """one group, diagnostics after runs of different lengths: a smaller total in a buffer grown for a larger one (stale
    statistics behind the live ones), then regrowth twice; the all-gather slot does not change, the lag sums' length does"""
    d, results = cases_child
    for k, (n_collect, _) in enumerate(child.REUSE_RUNS):
        res = results[f"reuse-{k}"]
        # a continued run: the single handle continues too, so the samples stay equal
        _check_exchange(res, 3, 1000, 3, n_collect)
        r, _, _ = _check_diagnostics(d, f"reuse-{k}", "hmc")
        assert r.m == n_collect // 2
    assert [(n // 2) * 3 % 2 for n, _ in child.REUSE_RUNS] == [0, 1, 0, 1]  # m D odd after run(50) and run(303)


@pytest.mark.gpu
def test_failing_initialisation_falls_back_to_the_host_with_status_minus_2(fallback_child):
    """ncclCommInitAll fails (the stand-in under FAKE_COLLECTIVES_FAIL_INIT): the group reports -2 with no ranks from
    creation on, calls no collective, and the host exchange gives the single-GPU entry point's R-hat / ESS"""
    d, results = fallback_child
    res = results["fallback"]
    assert res["exchange"] == [-2, 0] and res["exchange_status"] == -2 and not res["used_rccl"]
    assert res["counts_before"] == [0, 0, 0, 0] and res["counts_after"] == [0, 0, 0, 0]
    assert res["sample_equal"] and res["accept_equal"] and res["shards"] == [334, 333, 333]
    _check_diagnostics(d, "fallback", "hmc")
