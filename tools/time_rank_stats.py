"""Device time of the rank-normalised diagnostics (csrc/mm_rank.hip) beside an independent sort of the same keys.

    python tools/time_rank_stats.py [--out profiles/rank_stats_timing.jsonl] [--repeats 7] [--timeout 300]

For each shape [chains, n, params] and each of
    rank_normalize     stats.rank_normalize(sample)            one sort per parameter + tie scans, scores, scatter
    rank_diagnostics   stats.rank_diagnostics(sample)          two sorts per parameter + four split R-hat / ESS reductions
    torch_sort         torch.sort(keys, stable=True) per parameter, values and indices, keys = the parameter's column as
                       order-preserving int32 (the library's uint32 keys with the sign bit flipped back, so the order and the
                       32 key bits a radix sort walks are the same); extraction of the column is outside the timed region
one child process measures one (shape, step) under its own time limit: a warm-up call, then `repeats` calls each between two
HIP events on the stream the work runs on; the median is reported with the minimum and maximum.  A child that fails or
runs out of time ends the run -- nothing more is started on the device.

The byte model the fractions refer to: a 4-pass LSD sort of (key, index) pairs reads and writes 16 B per key and pass, plus one
4 B counting read: 68 B per key and parameter; `hbm_frac` = those bytes / median time / 8 TB/s.  It is the SORT's model for
every row (rank_diagnostics sorts twice and reduces four arrays on top: its fraction is a lower bound by construction).
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = [(65536, 400, 3), (65536, 4000, 3), (16384, 20000, 3)]
STEPS = ("torch_sort", "rank_normalize", "rank_diagnostics")
HBM_BYTES_PER_S = 8e12
SORT_BYTES_PER_KEY = 4 * 16 + 4


def measure(shape, step, repeats):
    import numpy as np
    import torch

    from mini_mcmc_amd import stats as S

    c, n, d = shape
    g = torch.Generator(device="cuda").manual_seed(c + n)
    t = torch.randn((c, n, d), generator=g, device="cuda", dtype=torch.float32)
    t = torch.cumsum(t.view(c, n // 50, 50, d), dim=2).view(c, n, d).contiguous()  # correlated within blocks, like a chain

    if step == "torch_sort":
        cols = []
        for j in range(d):
            bits = t[:, :, j].reshape(-1).contiguous().view(torch.int32)
            cols.append(bits ^ ((bits >> 31) & 0x7FFFFFFF))

        def call():
            for k in cols:
                torch.sort(k, stable=True)
    elif step == "rank_normalize":
        def call():
            S.rank_normalize(t)
    else:
        def call():
            S.rank_diagnostics(t)

    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = float(np.median(ms))
    nbytes = SORT_BYTES_PER_KEY * c * n * d
    return {"shape": list(shape), "step": step, "repeats": repeats, "ms_median": med, "ms_min": min(ms), "ms_max": max(ms),
            "sort_model_bytes": nbytes, "hbm_frac": nbytes / (med * 1e-3) / HBM_BYTES_PER_S,
            "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--child", nargs=4, metavar=("C", "N", "D", "STEP"), default=None)
    a = ap.parse_args()
    if a.child:
        c, n, d, step = int(a.child[0]), int(a.child[1]), int(a.child[2]), a.child[3]
        print(json.dumps(measure((c, n, d), step, a.repeats)), flush=True)
        return 0
    rows = []
    for shape in SHAPES:
        for step in STEPS:
            cmd = [sys.executable, os.path.abspath(__file__), "--repeats", str(a.repeats), "--child", *map(str, shape), step]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            except subprocess.TimeoutExpired:
                print(f"{shape} {step}: no result within {a.timeout} s; stopping", file=sys.stderr)
                return 1
            if r.returncode != 0:
                print(f"{shape} {step}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
                return 1
            row = json.loads(r.stdout.strip().splitlines()[-1])
            rows.append(row)
            print(json.dumps(row), flush=True)
        by = {r["step"]: r for r in rows if r["shape"] == list(shape)}
        print(json.dumps({"shape": list(shape), "rank_normalize_over_torch_sort": by["rank_normalize"]["ms_median"] / by["torch_sort"]["ms_median"]}),
              flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
