"""Device time of HMC on a likelihood over a bound array (csrc/mm_data.h), hand-written gradient beside forward mode.

    python tools/time_data_target.py [--out profiles/data_target_timing.jsonl] [--repeats 7] [--timeout 900]

Workload: logistic regression, D = 8 coefficients, N = 256 and 4096 rows [x0 .. x7 y] bound to the kind
(`UserTarget(..., data=)` / `AutodiffTarget(..., data=)`), N(0, 1) prior, HMC, f32, 65 536 chains, run(100, 20), L = 10 (the
split kernel).  One chain per lane walks all N rows in every gradient evaluation; a transition makes L of them.
    hand       logp_grad written by hand: eta, one sigmoid, D fused multiply-adds for the gradient, one softplus for the value
    autodiff   the log-likelihood alone, differentiated in forward mode (W = 8 tangents, one pass)
One child process measures one (N, flavour) under its own time limit: a warm-up run, then `repeats` runs each between two HIP
events on the stream the run is enqueued on (the sample stays in HBM); the median is reported with the minimum and maximum.
Autodiff at N = 4096 falls back to 8 192 chains if its warm-up run takes more than a minute; the row then says so
(`n_chains`).  A child that fails or runs out of time ends the run -- nothing more is started on the device.

Derived figures.  row_evals_per_s = n_chains x 120 transitions x L x N / time.  frac_f32_vector_peak = row_evals_per_s x
VALU_PER_ROW / (157.3e12 / 2): every vector instruction of a row counted as one multiply-add slot of the 157.3 TFLOP/s f32
vector peak (which is reached by packed multiply-adds only: scalar-operand code like this tops out at one half).  VALU_PER_ROW
is counted in the disassembly of the split HMC kernel of each unit at N = 256: every vector instruction in
the extent of the row loop inside logp_grad, the special-case blocks of the exponential and the logarithm included (an upper
count: a lane that skips them executes fewer).  include/mmcmc.h predicts autodiff / hand = about (1 + W) / 2 = 4.5 for a body
whose work is all differentiated arithmetic; here the exponential and the logarithm are shared by value and tangents (measured: 1.3 - 1.4)."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ROWS = (256, 4096)
FLAVOURS = ("hand", "autodiff")
DIM, N_CHAINS, N_COLLECT, N_DISCARD, N_LEAPFROG, STEP = 8, 65536, 100, 20, 10, 0.01
VALU_PER_ROW = {"hand": 107, "autodiff": 124}  # vector instructions in the extent of the row loop of logp_grad (see above)
F32_VECTOR_PEAK_FMA_PER_S = 157.3e12 / 2

HAND = r"""
template <class T> struct mmcmc_user_target {
    static constexpr int dim = 8;
    static constexpr int rows = %(rows)d;
    MM_HD static T logp(const mm_tparams<T> &P, const T *x) {
        T acc = 0;
        for (int r = 0; r < rows; ++r) {
            T row[dim + 1];
            mm_data_row<dim + 1>(P.mat, r, row);
            T eta = 0;
            MM_UNROLL
            for (int i = 0; i < dim; ++i) eta = mm_fma(row[i], x[i], eta);
            acc += row[dim] * eta - mm_softplusT(eta);
        }
        T pr = 0;
        MM_UNROLL
        for (int i = 0; i < dim; ++i) pr = mm_fma(x[i], x[i], pr);
        return mm_fma(T(-0.5), pr, acc);
    }
    MM_HD static T logp_grad(const mm_tparams<T> &P, const T *x, T *g) {
        T acc = 0;
        MM_UNROLL
        for (int k = 0; k < dim; ++k) g[k] = -x[k];
        for (int r = 0; r < rows; ++r) {
            T row[dim + 1];
            mm_data_row<dim + 1>(P.mat, r, row);
            T eta = 0;
            MM_UNROLL
            for (int i = 0; i < dim; ++i) eta = mm_fma(row[i], x[i], eta);
            const T w = row[dim] - mm_sigmoidT(eta);
            MM_UNROLL
            for (int k = 0; k < dim; ++k) g[k] = mm_fma(row[k], w, g[k]);
            acc += row[dim] * eta - mm_softplusT(eta);
        }
        T pr = 0;
        MM_UNROLL
        for (int i = 0; i < dim; ++i) pr = mm_fma(x[i], x[i], pr);
        return mm_fma(T(-0.5), pr, acc);
    }
};
"""

AUTODIFF = r"""
template <class T> struct mmcmc_user_logp {
    static constexpr int dim = 8;
    static constexpr int rows = %(rows)d;
    template <class S> MM_HD static S logp(const mm_tparams<T> &P, const S *x) {
        S acc = 0;
        for (int r = 0; r < rows; ++r) {
            T row[dim + 1];
            mm_data_row<dim + 1>(P.mat, r, row);
            S eta = 0;
            MM_UNROLL
            for (int i = 0; i < dim; ++i) eta = mm_fma(row[i], x[i], eta);
            acc = acc + (row[dim] * eta - mm_softplusT(eta));
        }
        S pr = 0;
        MM_UNROLL
        for (int i = 0; i < dim; ++i) pr = mm_fma(x[i], x[i], pr);
        return mm_fma(T(-0.5), pr, acc);
    }
};
"""


def design(n_rows: int):
    """rows [n, 9] = [1, x1 .. x7, y]: a synthetic design, y drawn from the model with fixed coefficients"""
    import numpy as np

    rng = np.random.default_rng(n_rows)
    beta = np.array([-0.5, 1.0, -1.0, 0.5, 0.25, 0.75, -0.25, 1.5])
    x = np.concatenate([np.ones((n_rows, 1)), rng.standard_normal((n_rows, DIM - 1))], axis=1)
    y = (rng.random(n_rows) < 1.0 / (1.0 + np.exp(-x @ beta))).astype(np.float64)
    return np.concatenate([x, y[:, None]], axis=1)


def measure(n_rows, which, repeats):
    import numpy as np
    import torch

    from mini_mcmc_amd.core import init_with_seed
    from mini_mcmc_amd.distributions import AutodiffTarget, UserTarget
    from mini_mcmc_amd.hmc import HMC

    data = design(n_rows)
    if which == "hand":
        tgt = UserTarget(f"logit8_{n_rows}_hand", DIM, HAND % {"rows": n_rows}, data=data)
    else:
        tgt = AutodiffTarget(f"logit8_{n_rows}_ad", DIM, AUTODIFF % {"rows": n_rows}, data=data)

    def warm(n_chains):
        h = HMC(tgt, init_with_seed(n_chains, DIM, 42, np.float32) * 0.1, STEP, N_LEAPFROG).set_seed(42)
        t0 = time.perf_counter()
        h.run(N_COLLECT, N_DISCARD, to="torch", accept_counts=False)
        torch.cuda.synchronize()
        return h, time.perf_counter() - t0

    n_chains = N_CHAINS
    h, first = warm(n_chains)
    if first > 60.0 and which == "autodiff":
        n_chains = 8192
        h, first = warm(n_chains)
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = h.run(N_COLLECT, N_DISCARD, to="torch", accept_counts=False)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
        del out
    med = float(np.median(ms))
    row_evals = n_chains * (N_COLLECT + N_DISCARD) * N_LEAPFROG * n_rows / (med * 1e-3)
    return {"rows": n_rows, "dim": DIM, "flavour": which, "kernel_variant": h.kernel_variant, "n_chains": n_chains, "n_collect": N_COLLECT,
            "n_discard": N_DISCARD, "n_leapfrog": N_LEAPFROG, "repeats": repeats, "ms_median": med, "ms_min": min(ms), "ms_max": max(ms),
            "row_evals_per_s": row_evals, "valu_per_row": VALU_PER_ROW[which],
            "frac_f32_vector_peak": row_evals * VALU_PER_ROW[which] / F32_VECTOR_PEAK_FMA_PER_S, "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--child", nargs=2, metavar=("ROWS", "FLAVOUR"), default=None)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(int(a.child[0]), a.child[1], a.repeats)), flush=True)
        return 0
    rows = []
    for n_rows in ROWS:
        for which in FLAVOURS:
            cmd = [sys.executable, os.path.abspath(__file__), "--repeats", str(a.repeats), "--child", str(n_rows), which]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            except subprocess.TimeoutExpired:
                print(f"rows {n_rows} {which}: no result within {a.timeout} s; stopping", file=sys.stderr)
                return 1
            if r.returncode != 0:
                print(f"rows {n_rows} {which}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
                return 1
            row = json.loads(r.stdout.strip().splitlines()[-1])
            rows.append(row)
            print(json.dumps(row), flush=True)
        by = {r["flavour"]: r for r in rows if r.get("rows") == n_rows and "flavour" in r}
        per_chain = {k: v["ms_median"] / v["n_chains"] for k, v in by.items()}  # autodiff may have run fewer chains
        rows.append({"rows": n_rows, "autodiff_over_hand": per_chain["autodiff"] / per_chain["hand"], "predicted": (1 + DIM) / 2})
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
