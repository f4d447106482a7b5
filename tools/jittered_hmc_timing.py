"""bench.py's converged HMC workload (side.config3_hmc_converged: RosenbrockND(3), f32, 65 536 chains, eps_k ~ U(0.004, 0.016),
L_k ~ U{100..400} per block of 100 transitions, 20 blocks burned, 40 kept) timed both ways, one JSON line per case:

  handles   hmc.run_chain_of_handles: 60 handles, the state copied to the host and back between them
  jittered  hmc.run_jittered: one handle, one mmcmc_hmc_run_scheduled call (one launch on the split kernel)
  eps_only  a per-transition jitter of eps alone (L fixed at 250, the mean of U{100..400}): R-hat, ESS, moments
  same_work one handle, eps = 0.01, L = 250, 6000 transitions: plain run() (the run-time L split kernel) against a constant
            schedule (its scheduled form) -- the kernels alone, without the launch pattern

    python tools/jittered_hmc_timing.py [--out FILE] [--timeout S]

Every case runs in a child process of its own under `timeout -k 10 S`; the first that fails ends the tool.  kernel_ms: the
handles' HIP-event time (summed over the handles); wall_ms: the call, synchronised, on the host clock, warm (the case runs once
before it is timed)."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("handles", "jittered", "eps_only", "same_work")
N_CHAINS, DIM, SEED = 65536, 3, 42


def exact_moments():
    import numpy as np

    x0 = np.linspace(-5.0, 6.0, 220001)
    w = np.exp(-(1 - x0) ** 2 - (100.0 / 101.0) * (1 - x0 ** 2) ** 2)
    w /= w.sum()
    mu1, s1 = (100.0 * x0 ** 2 + 1.0) / 101.0, 1.0 / 202.0
    m0, m1 = (w * x0).sum(), (w * mu1).sum()
    e1sq = (w * (mu1 ** 2 + s1)).sum()
    e14 = (w * (mu1 ** 4 + 6 * mu1 ** 2 * s1 + 3 * s1 ** 2)).sum()
    return [m0, m1, e1sq], [(w * (x0 - m0) ** 2).sum(), e1sq - m1 ** 2, e14 + 1.0 / 200.0 - e1sq ** 2]


def quality(t):
    from mini_mcmc_amd import stats as S

    rh, es = S.split_rhat_mean_ess(t)
    xd = t.double().reshape(-1, DIM)
    mean = [float(v) for v in xd.mean(dim=0).cpu()]
    var = [float(v) for v in xd.var(dim=0).cpu()]
    em, ev = exact_moments()
    err = max(max(abs(mean[i] - em[i]) / abs(em[i]) for i in range(DIM)), max(abs(var[i] - ev[i]) / ev[i] for i in range(DIM)))
    rmax = float((1.0 / rh).max())
    return {"split_rhat_max_conventional": rmax, "ess_min": float(es.min()), "posterior_mean": mean, "posterior_var": var,
            "max_rel_moment_error": err, "converged": bool(rmax <= 1.05 and err <= 0.01)}


def one_case(case):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from mini_mcmc_amd.core import init_with_seed
    from mini_mcmc_amd.distributions import RosenbrockND
    from mini_mcmc_amd.hmc import HMC, run_chain_of_handles, run_jittered

    init = init_with_seed(N_CHAINS, DIM, SEED, np.float32)
    res = {"case": case, "n_chains": N_CHAINS, "blocks": "20 burned + 40 kept x 100 transitions"}
    if case in ("handles", "jittered"):
        fn = run_chain_of_handles if case == "handles" else run_jittered
        for rep in range(2):  # the first run warms up (module loads, allocations); the second is reported
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t, info = fn(RosenbrockND(DIM), init, (0.004, 0.016), (100, 400), 100, 20, 40, seed=SEED)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            if rep == 0:
                del t
        res.update({"kernel_ms": info["kernel_ms"], "wall_ms": wall, "launches": info["launches"], "accept_rate": info["accept_rate"],
                    "leapfrog_steps_per_s": info["leapfrogs"] / (info["kernel_ms"] * 1e-3)})
        if case == "jittered":
            res["wall_ms_of_the_call"] = info["wall_ms"]
        res.update(quality(t))
    elif case == "eps_only":
        rng = np.random.default_rng(7)
        eps = rng.uniform(0.004, 0.016, 6000)
        nl = np.full(6000, 250, dtype=np.int32)
        for rep in range(2):
            h = HMC(RosenbrockND(DIM), init, float(eps[0]), 250).set_seed(SEED)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t = h.run_scheduled(eps, nl, 4000, to="torch")
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
        res.update({"schedule": "eps ~ U(0.004, 0.016) per transition, L = 250", "kernel_ms": float(h.timing()["kernel_ms"]),
                    "wall_ms": wall, "launches": int(h.timing()["n_launches"]),
                    "accept_rate": float(h.accept_counts.mean()) / 6000})
        res.update(quality(t))
    else:
        eps, nl = np.full(6000, 0.01), np.full(6000, 250, dtype=np.int32)
        ms = {"plain_run": [], "constant_schedule": []}
        for rep in range(3):
            for how in ms:
                h = HMC(RosenbrockND(DIM), init, 0.01, 250).set_seed(SEED)
                t = h.run(4000, 2000, to="torch") if how == "plain_run" else h.run_scheduled(eps, nl, 4000, to="torch")
                torch.cuda.synchronize()
                ms[how].append(float(h.timing()["kernel_ms"]))
                h.close()
                del t
        res.update({"schedule": "eps = 0.01, L = 250, 2000 + 4000 transitions", "kernel_ms_plain_run": ms["plain_run"],
                    "kernel_ms_constant_schedule": ms["constant_schedule"]})
    print(json.dumps(res), flush=True)


def main():
    if "--case" in sys.argv:
        one_case(sys.argv[sys.argv.index("--case") + 1])
        return 0
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    limit = sys.argv[sys.argv.index("--timeout") + 1] if "--timeout" in sys.argv else "300"
    for case in CASES:
        p = subprocess.run(["timeout", "-k", "10", limit, sys.executable, os.path.abspath(__file__), "--case", case],
                           capture_output=True, text=True, cwd=ROOT)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not lines:
            sys.stderr.write(p.stdout[-4000:] + p.stderr[-4000:])
            print(json.dumps({"case": case, "exit_status": p.returncode}), flush=True)
            return 1
        print(lines[-1], flush=True)
        if out:
            with open(out, "a") as f:
                f.write(lines[-1] + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
