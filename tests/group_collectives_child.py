"""The child process of tests/test_group_collectives.py -- TEST INFRASTRUCTURE ONLY, not collected by pytest.

    python group_collectives_child.py <stand-in library> <output directory> cases|fallback

The collectives of libmmcmc.so are bound once per process, so the stand-in (tests/c/fake_collectives.c) is bound HERE, in a
fresh process, and never in the pytest process.  `cases` binds it as accepting several ranks on one device and runs every
case of CASES plus the buffer-reuse sequence; `fallback` is started with FAKE_COLLECTIVES_FAIL_INIT set, so ncclCommInitAll
fails and the group must take the host exchange with status -2.  Each case leaves <name>.npz (the group's sample, its R-hat
/ ESS, the single-GPU entry point's on the single-handle sample) and an entry in results.json; the parent does the float64
work and every assertion.  Any exception -- a HIP error status among them -- ends the process with a non-zero exit code at
once: nothing further runs on the device."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# name -> (ranks, chains, sampler, n_collect, n_discard): the table of the module docstring of test_group_collectives.py
CASES = {
    "n2-mh-2chains": (2, 2, "mh", 8, 0),
    "n3-hmc-7chains-odd": (3, 7, "hmc", 123, 0),
    "n3-hmc-1000": (3, 1000, "hmc", 120, 30),
    "n3-mh-f64-offset": (3, 257, "mh64", 64, 8),
    "n8-hmc-4803": (8, 8 * 600 + 3, "hmc", 100, 0),
    "n64-mh-101": (64, 64 + 37, "mh", 16, 0),
    "n3-nuts-d32": (3, 100, "nuts", 20, 12),
    "n3-mh-far-target": (3, 8192, "mhfar", 400, 100),
    "n4-mh-ramp": (4, 403, "mhramp", 30, 0),
}
REUSE_RUNS = ((120, 30), (50, 0), (301, 0), (303, 0))  # buffer reuse: one group of 3 ranks and 1000 chains


def make(sampler, chains, devices):
    """(single handle, group) of one case: the same target, initial positions and seed"""
    from mini_mcmc_amd.core import init_with_seed
    from mini_mcmc_amd.distributions import Gaussian2D, GaussianND, IsotropicGaussian, RosenbrockND
    from mini_mcmc_amd.group import HMCGroup, MetropolisHastingsGroup, NUTSGroup
    from mini_mcmc_amd.hmc import HMC
    from mini_mcmc_amd.metropolis_hastings import MetropolisHastings
    from mini_mcmc_amd.nuts import NUTS

    if sampler == "hmc":
        init = init_with_seed(chains, 3, 42, np.float32)
        return (HMC(RosenbrockND(3), init, 0.032, 10).set_seed(42),
                HMCGroup(RosenbrockND(3), init, 0.032, 10, devices=devices).set_seed(42))
    if sampler == "nuts":
        tgt = GaussianND.ill_conditioned(32, 100.0, 5)
        init = init_with_seed(chains, 32, 42) * 0.1
        return NUTS(tgt, init, 0.8, mode=2).set_seed(42), NUTSGroup(tgt, init, 0.8, mode=2, devices=devices).set_seed(42)
    prop = IsotropicGaussian(1.0)
    if sampler == "mh":
        tgt, init, seed, off = Gaussian2D([0.0, 1.0], [[4.0, 2.0], [2.0, 3.0]]), init_with_seed(chains, 2, 42, np.float32), 42, 0
    elif sampler == "mh64":
        tgt, init, seed, off = Gaussian2D([0.0, 1.0], [[4.0, 2.0], [2.0, 3.0]]), init_with_seed(chains, 2, 7, np.float64), 5, 1 << 33
    elif sampler == "mhfar":
        mean = np.array([3000.0, -2000.0])
        tgt = Gaussian2D(mean.tolist(), [[1.0, 0.0], [0.0, 1.0]])
        init, seed, off = (init_with_seed(chains, 2, 42, np.float32).astype(np.float64) + mean).astype(np.float32), 42, 0
    elif sampler == "mhramp":
        # contiguous shards of a ramp of starting points: the ranks' half-chain means stand apart, the sample is unconverged
        centre = np.array([5.0, -3.0])
        tgt = Gaussian2D(centre.tolist(), [[1.0, 0.0], [0.0, 1.0]])
        ramp = 6.0 * (np.arange(chains, dtype=np.float64) / chains - 0.5)
        init, seed, off = (centre[None, :] + ramp[:, None]).astype(np.float32), 42, 0
    else:
        raise ValueError(sampler)
    one = MetropolisHastings(tgt, prop, init).seed(seed)
    grp = MetropolisHastingsGroup(tgt, prop, init, devices=devices).seed(seed)
    if off:
        one.set_chain_offset(off)
        grp.set_chain_offset(off)
    return one, grp


def run_pair(sampler, one, grp, n_collect, n_discard):
    if sampler == "nuts":
        return one._run(n_collect, n_discard, False, "numpy"), grp.run(n_collect, n_discard), True
    ref, out = one.run(n_collect, n_discard), grp.run(n_collect, n_discard)
    return ref, out, bool(np.array_equal(grp.accept_counts, one.accept_counts))


def counts(fake):
    out = (C.c_size_t * 4)()
    fake.fake_collectives_counts(out)
    return [int(v) for v in out]


def one_case(fake, outdir, name, sampler, one, grp, n_collect, n_discard):
    from mini_mcmc_amd import stats as S

    t0 = time.perf_counter()
    exchange = grp.exchange()
    ref, out, accept_equal = run_pair(sampler, one, grp, n_collect, n_discard)
    before = counts(fake)
    rhat, ess = grp.split_rhat_mean_ess()
    after = counts(fake)
    rhat1, ess1 = S.split_rhat_mean_ess(ref)
    print(f"{name}: {time.perf_counter() - t0:.2f} s", flush=True)  # the parent shows this when the child fails: how far it came
    np.savez(os.path.join(outdir, name + ".npz"), sample=out, rhat=rhat, ess=ess, rhat_single=rhat1, ess_single=ess1)
    return dict(exchange=list(exchange), exchange_status=int(grp.exchange_status), used_rccl=bool(grp.used_rccl),
                sample_equal=bool(np.array_equal(out, ref)), accept_equal=accept_equal, shards=[int(s[2]) for s in shards(grp)],
                counts_before=before, counts_after=after)


def shards(grp):
    """(device, first chain, chains) per rank: only the HMC group has the C entry point; the split rule is group_create's"""
    if hasattr(grp, "shards"):
        return grp.shards()
    n, c = len(grp.devices), grp.n_chains
    sizes = [c // n + (1 if i < c % n else 0) for i in range(n)]
    return [(0, sum(sizes[:i]), sizes[i]) for i in range(n)]


def main(lib_path, outdir, mode):
    import mini_mcmc_amd
    from mini_mcmc_amd import _lib as L
    from mini_mcmc_amd.group import bind_collectives

    mini_mcmc_amd.lib()
    fake = C.CDLL(lib_path)  # the same mapping the engine binds: its counters are the engine's calls
    fake.fake_collectives_counts.argtypes = [C.POINTER(C.c_size_t)]
    fake.fake_collectives_counts.restype = None
    bind_collectives(lib_path, ranks_may_share_a_device=True)
    # the binding holds for the life of the process: a second one is refused
    again = L.lib().mmcmc_group_bind_collectives(os.fsencode(lib_path), 1)
    results = {"bind_again": int(again)}
    if mode == "fallback":
        one, grp = make("hmc", 1000, [0, 0, 0])
        results["fallback"] = one_case(fake, outdir, "fallback", "hmc", one, grp, 120, 30)
        grp.close()
    else:
        for name, (ranks, chains, sampler, n_collect, n_discard) in CASES.items():
            one, grp = make(sampler, chains, [0] * ranks)
            results[name] = one_case(fake, outdir, name, sampler, one, grp, n_collect, n_discard)
            grp.close()
        one, grp = make("hmc", 1000, [0, 0, 0])
        for k, (n_collect, n_discard) in enumerate(REUSE_RUNS):
            results[f"reuse-{k}"] = one_case(fake, outdir, f"reuse-{k}", "hmc", one, grp, n_collect, n_discard)
        grp.close()
    with open(os.path.join(outdir, "results.json"), "w") as f:
        json.dump(results, f)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], sys.argv[3])
