#!/usr/bin/env python3
"""Records which kernel variants MH / HMC handles take: tests/golden/kernel_paths.json, through the public API only.

    python3 tools/record_kernel_paths.py [--commit HASH] [--out PATH]

Run on a checkout of the commit whose behaviour is to be kept (its hash goes into the file); tests/test_kernel_paths.py then
asserts that the library under test reproduces the file.  Per case: the default variant (HMC: mmcmc_hmc_kernel_variant; MH
has no getter), the status of set_kernel_variant(v) for v = -1 .. 9 on a fresh handle each time and, for HMC, the getter's
value after each successful set.

The cases are the smallest shapes at which the rule can go wrong, 96 chains unless stated, f32 and f64, MH and HMC:
Rosenbrock2D; RosenbrockND at 3 and 8 (split kernels exist), 9 (no fixed kernel: the built-in's run-time compiled unit), 16 and
32 (fixed; plain default above 16), 33 (run-time dimension only), 128 with 96 chains (wide default under HMC) and with 1024
(not wide by default); GaussianND at 8, 16 and 32 (lane groups under HMC at 16 / 32); a source-registered user target of dim 2
(the banana of tests/test_user_target.py); for MH, a target + proposal model (the isotropic proposal of
tests/test_user_proposal.py over Gaussian2D).  Handle creation only, except one run-time compile per dim-9 unit and per source."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_paths.json")
VARIANTS = list(range(-1, 10))
DTYPES = {"f32": np.float32, "f64": np.float64}
EPS, N_LEAPFROG, STD = 0.01, 10, 0.1

# name -> (dim, n_chains)
TARGETS = {
    "rosenbrock2d": (2, 96),
    "rosenbrock_nd_3": (3, 96), "rosenbrock_nd_8": (8, 96), "rosenbrock_nd_9": (9, 96), "rosenbrock_nd_16": (16, 96),
    "rosenbrock_nd_32": (32, 96), "rosenbrock_nd_33": (33, 96), "rosenbrock_nd_128": (128, 96),
    "rosenbrock_nd_128_c1024": (128, 1024),
    "gaussian_nd_8": (8, 96), "gaussian_nd_16": (16, 96), "gaussian_nd_32": (32, 96),
    "user_banana": (2, 96),
    "model_iso_gaussian2d": (2, 96),  # MH only: a target + proposal model
}
CASES = [(sampler, ty, name) for name in TARGETS for sampler in ("mh", "hmc") for ty in DTYPES
         if not (name.startswith("model_") and sampler == "hmc")]
_made = {}


def case_id(case):
    return "-".join(case)


def _sources():
    tests = os.path.join(ROOT, "tests")
    if tests not in sys.path:
        sys.path.insert(0, tests)
    import test_user_proposal
    import test_user_target

    return test_user_target.BANANA, test_user_proposal.ISOTROPIC


def target(name):
    """(target, proposal or None); sources are registered once per process"""
    from mini_mcmc_amd import distributions as D

    if name not in _made:
        dim = TARGETS[name][0]
        prop = None
        if name == "rosenbrock2d":
            tgt = D.Rosenbrock2D()
        elif name.startswith("rosenbrock_nd"):
            tgt = D.RosenbrockND(dim)
        elif name.startswith("gaussian_nd"):  # a well-conditioned tridiagonal precision
            tgt = D.GaussianND(2.0 * np.eye(dim) - 0.5 * np.eye(dim, k=1) - 0.5 * np.eye(dim, k=-1))
        elif name == "user_banana":
            tgt = D.UserTarget("banana_kernel_paths", 2, _sources()[0], params=[1.5, 0.5])
        else:
            tgt = D.Gaussian2D([0.0, 1.0], [[4.0, 2.0], [2.0, 3.0]])
            prop = D.UserProposal("iso_rw_kernel_paths", tgt, _sources()[1], STD)
        _made[name] = (tgt, prop)
    return _made[name]


def make(case):
    """a fresh handle of the case, seeded; its start is the same every time"""
    from mini_mcmc_amd import distributions as D
    from mini_mcmc_amd.core import init_with_seed
    from mini_mcmc_amd.hmc import HMC
    from mini_mcmc_amd.metropolis_hastings import MetropolisHastings

    sampler, ty, name = case
    dim, n_chains = TARGETS[name]
    tgt, prop = target(name)
    init = (0.1 * init_with_seed(n_chains, dim, 42)).astype(DTYPES[ty])
    if sampler == "hmc":
        return HMC(tgt, init, EPS, N_LEAPFROG).set_seed(7)
    return MetropolisHastings(tgt, prop or D.IsotropicGaussian(STD), init).seed(7)


def observe(case):
    """what the library says about the case's handles: {"default", "status": {v: status}, "reported": {v: getter after set}}"""
    from mini_mcmc_amd import _lib as L

    lib = L.lib()
    hmc = case[0] == "hmc"
    setter = lib.mmcmc_hmc_set_kernel_variant if hmc else lib.mmcmc_mh_set_kernel_variant
    h = make(case)
    res = {"default": int(lib.mmcmc_hmc_kernel_variant(h._h)) if hmc else None, "status": {}, "reported": {}}
    h.close()
    for v in VARIANTS:
        h = make(case)
        st = int(setter(h._h, C.c_int(v)))
        res["status"][str(v)] = st
        if hmc and st == L.OK:
            res["reported"][str(v)] = int(lib.mmcmc_hmc_kernel_variant(h._h))
        h.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--commit", help="hash of the commit the library was built from (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True,
                                           check=True).stdout.strip()
    doc = {"commit": commit, "variants": VARIANTS, "cases": {case_id(c): observe(c) for c in CASES}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(doc['cases'])} cases of commit {commit} -> {args.out}")


if __name__ == "__main__":
    main()
