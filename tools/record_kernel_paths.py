#!/usr/bin/env python3
"""Records which kernel variants MH / HMC handles take: tests/golden/kernel_paths.json, through the public API only.

    python3 tools/record_kernel_paths.py [--commit HASH] [--out PATH]
    python3 tools/record_kernel_paths.py --nuts [--commit HASH] [--out PATH]     (NUTS handles: tests/golden/nuts_kernel_paths.json,
                                                                                 tests/test_nuts_kernel_paths.py; the cases at NUTS_CASES below)

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


# ---- NUTS handles: a record of their own (--nuts), tests/golden/nuts_kernel_paths.json.  64 chains each.  (target, mode):
# compiled instances with a pair kernel (StandardNormal(2), RosenbrockND(3): modes 0 / 1 / 2); RosenbrockND(10), a compiled
# instance whose f64 form is at the pair kernel's size limit, and RosenbrockND(9), which has none (the built-in's run-time
# compiled unit, or the run-time-dimension kernel): modes 0 and 2; GaussianND at 16 and 32 in mode 2 (lane groups) and in
# mode 0 (none); RosenbrockND(40), above the unit limit of 32.
NUTS_GOLDEN = os.path.join(ROOT, "tests", "golden", "nuts_kernel_paths.json")
NUTS_CHAINS = 64
NUTS_TARGETS = {"standard_normal_2": 2, "rosenbrock_nd_3": 3, "rosenbrock_nd_9": 9, "rosenbrock_nd_10": 10, "gaussian_nd_16": 16,
                "gaussian_nd_32": 32, "rosenbrock_nd_40": 40}
NUTS_CASES = ([(name, mode) for name in ("standard_normal_2", "rosenbrock_nd_3") for mode in (0, 1, 2)] +
              [(name, mode) for name in ("rosenbrock_nd_9", "rosenbrock_nd_10", "gaussian_nd_16", "gaussian_nd_32") for mode in (0, 2)] +
              [("rosenbrock_nd_40", 0)])
# the same walk on a handle with a diagonal metric, a dense metric or per-draw statistics switched on: each compiles one unit
# at run time (about two seconds at dim 3; a lane-group handle's GaussianND(16) unit takes seven, so it is left to the host
# walk of the rule), so on one small compiled instance.  Without a run-time compiler the toggle is refused and the record
# says so.
NUTS_TOGGLED = [("rosenbrock_nd_3", 0, "diag"), ("rosenbrock_nd_3", 0, "dense"), ("rosenbrock_nd_3", 0, "stats")]


def nuts_case_id(case):
    return "-".join(str(x) for x in case)


def make_nuts(case):
    from mini_mcmc_amd import distributions as D
    from mini_mcmc_amd.core import init_with_seed
    from mini_mcmc_amd.nuts import NUTS

    name, mode = case[0], case[1]
    dim = NUTS_TARGETS[name]
    if name.startswith("standard_normal"):
        tgt = D.StandardNormal(dim)
    elif name.startswith("rosenbrock_nd"):
        tgt = D.RosenbrockND(dim)
    else:
        tgt = D.GaussianND(2.0 * np.eye(dim) - 0.5 * np.eye(dim, k=1) - 0.5 * np.eye(dim, k=-1))
    return NUTS(tgt, 0.1 * init_with_seed(NUTS_CHAINS, dim, 42), 0.8, mode=mode).set_seed(7)


def _nuts_toggle(lib, h, toggle, on):
    dim = h.dim
    if toggle == "stats":
        return int(lib.mmcmc_nuts_set_draw_stats(h._h, 1 if on else 0))
    if not on:
        return int(lib.mmcmc_nuts_set_metric(h._h, None))
    if toggle == "diag":
        a = np.linspace(0.5, 2.0, dim)
        return int(lib.mmcmc_nuts_set_metric(h._h, a.ctypes.data_as(C.POINTER(C.c_double))))
    a = np.ascontiguousarray(np.eye(dim) + 0.25 * np.tril(np.ones((dim, dim)), -1))
    return int(lib.mmcmc_nuts_set_metric_dense(h._h, a.ctypes.data_as(C.POINTER(C.c_double))))


def observe_nuts(case):
    """(target, mode): {"default", "status": {v: status on a fresh handle}, "reported": {v: the getter after a successful set}}.
    (target, mode, toggle): one handle, fresh and set to variant 0 where it takes it; {"toggle_status", "default": the getter
    once the toggle is on, "status" / "reported" over every v on that handle, "after": the getter once it is off again}."""
    from mini_mcmc_amd import _lib as L

    lib = L.lib()
    getter, setter = lib.mmcmc_nuts_kernel_variant, lib.mmcmc_nuts_set_kernel_variant
    res = {"status": {}, "reported": {}}
    if len(case) == 2:
        h = make_nuts(case)
        res["default"] = int(getter(h._h))
        h.close()
    else:
        held = make_nuts(case)
        res["before"] = int(getter(held._h))
        res["toggle_status"] = _nuts_toggle(lib, held, case[2], True)
        res["default"] = int(getter(held._h))
    for v in VARIANTS:
        h = make_nuts(case) if len(case) == 2 else held
        st = int(setter(h._h, C.c_int(v)))
        res["status"][str(v)] = st
        if st == L.OK:
            res["reported"][str(v)] = int(getter(h._h))
        if len(case) == 2:
            h.close()
    if len(case) == 3:
        res["off_status"] = _nuts_toggle(lib, held, case[2], False)
        res["after"] = int(getter(held._h))
        held.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--commit", help="hash of the commit the library was built from (default: git rev-parse HEAD)")
    ap.add_argument("--nuts", action="store_true", help="record the NUTS handles (tests/golden/nuts_kernel_paths.json) instead")
    ap.add_argument("--out")
    args = ap.parse_args()
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True,
                                           check=True).stdout.strip()
    if args.nuts:
        doc = {"commit": commit, "variants": VARIANTS, "cases": {nuts_case_id(c): observe_nuts(c) for c in NUTS_CASES},
               "toggled": {nuts_case_id(c): observe_nuts(c) for c in NUTS_TOGGLED}}
    else:
        doc = {"commit": commit, "variants": VARIANTS, "cases": {case_id(c): observe(c) for c in CASES}}
    out = args.out or (NUTS_GOLDEN if args.nuts else GOLDEN)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(doc['cases'])} cases of commit {commit} -> {out}")


if __name__ == "__main__":
    main()
