"""Device time of HMC with a forward-mode gradient (csrc/mm_autodiff.h) beside the hand-written and the built-in one.

    python tools/time_autodiff.py [--out profiles/autodiff_timing.jsonl] [--repeats 7] [--timeout 600]

Workload: HMC on RosenbrockND(dim), f32, 65 536 chains, run(400, 50), L = 10, at dim 3 (the split kernel) and dim 32
(variant 2), for three targets of the same density:
    builtin    RosenbrockND(dim)                                     the library's analytic gradient
    hand       UserTarget, a hand-written logp_grad                  (the source of tests/test_user_target.py)
    autodiff   AutodiffTarget, tests/cpp/autodiff_cases/rosenbrock.inc
One child process measures one (dim, target) under its own time limit: a warm-up run, then `repeats` runs each between two
HIP events on the stream the run is enqueued on (the sample stays in HBM); the median is reported with the minimum and
maximum.  A child that fails or runs out of time ends the run -- nothing more is started on the device."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DIMS = (3, 32)
TARGETS = ("builtin", "hand", "autodiff")
N_CHAINS, N_COLLECT, N_DISCARD, N_LEAPFROG = 65536, 400, 50, 10

HAND = r"""
template <class T> struct mmcmc_user_target {
    static constexpr int dim = MM_USER_DIM;
    MM_HD static T logp(const mm_tparams<T> &, const T *x) {
        T acc = 0;
        MM_UNROLL
        for (int i = 0; i + 1 < dim; ++i) {
            T t = mm_fma(-x[i], x[i], x[i + 1]);
            T u = T(1) - x[i];
            acc = mm_fma(T(100) * t, t, acc);
            acc = mm_fma(u, u, acc);
        }
        return -acc;
    }
    MM_HD static T logp_grad(const mm_tparams<T> &, const T *x, T *g) {
        T acc = 0, tprev = 0;
        MM_UNROLL
        for (int i = 0; i + 1 < dim; ++i) {
            T t = mm_fma(-x[i], x[i], x[i + 1]);
            T u = T(1) - x[i];
            acc = mm_fma(T(100) * t, t, acc);
            acc = mm_fma(u, u, acc);
            T a = mm_fma(T(400) * x[i], t, T(2) * u);
            g[i] = (i > 0) ? mm_fma(T(-200), tprev, a) : a;
            tprev = t;
        }
        g[dim - 1] = T(-200) * tprev;
        return -acc;
    }
};
"""


def measure(dim, which, repeats):
    import numpy as np
    import torch

    from mini_mcmc_amd.core import init_with_seed
    from mini_mcmc_amd.distributions import AutodiffTarget, RosenbrockND, UserTarget
    from mini_mcmc_amd.hmc import HMC

    if which == "builtin":
        tgt = RosenbrockND(dim)
    elif which == "hand":
        tgt = UserTarget(f"rosenbrock{dim}_hand", dim, HAND)
    else:
        tgt = AutodiffTarget(f"rosenbrock{dim}_ad", dim, open(os.path.join(ROOT, "tests", "cpp", "autodiff_cases", "rosenbrock.inc")).read())
    eps = 0.032 if dim == 3 else 0.01
    h = HMC(tgt, init_with_seed(N_CHAINS, dim, 42, np.float32), eps, N_LEAPFROG).set_seed(42)
    h.run(N_COLLECT, N_DISCARD, to="torch", accept_counts=False)
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = h.run(N_COLLECT, N_DISCARD, to="torch", accept_counts=False)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
        del out
    return {"dim": dim, "target": which, "kernel_variant": h.kernel_variant, "n_chains": N_CHAINS, "n_collect": N_COLLECT,
            "n_discard": N_DISCARD, "n_leapfrog": N_LEAPFROG, "repeats": repeats, "ms_median": float(np.median(ms)), "ms_min": min(ms),
            "ms_max": max(ms), "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--child", nargs=2, metavar=("DIM", "TARGET"), default=None)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(int(a.child[0]), a.child[1], a.repeats)), flush=True)
        return 0
    rows = []
    for dim in DIMS:
        for which in TARGETS:
            cmd = [sys.executable, os.path.abspath(__file__), "--repeats", str(a.repeats), "--child", str(dim), which]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            except subprocess.TimeoutExpired:
                print(f"dim {dim} {which}: no result within {a.timeout} s; stopping", file=sys.stderr)
                return 1
            if r.returncode != 0:
                print(f"dim {dim} {which}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
                return 1
            row = json.loads(r.stdout.strip().splitlines()[-1])
            rows.append(row)
            print(json.dumps(row), flush=True)
        by = {r["target"]: r["ms_median"] for r in rows if r["dim"] == dim}
        rows.append({"dim": dim, "autodiff_over_hand": by["autodiff"] / by["hand"], "autodiff_over_builtin": by["autodiff"] / by["builtin"]})
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
