#!/usr/bin/env python3
"""Retake tests/golden/rtc_unit_texts.json: the texts of the run-time compiled units as a given commit builds them.

    git worktree add /tmp/rtc_parent <commit>            # a scratch copy of the commit the record is taken from
    git -C /tmp/rtc_parent apply tools/experiments/rtc_dump_units.patch
    python3 tools/experiments/rtc_record_units.py /tmp/rtc_parent <commit hash> [out.json]

The patch (nothing of it is applied to the repository) makes compile_and_register write each unit's text to
$MMCMC_RTC_DUMP_DIR before the device check and register the unit without compiling or loading it, so a machine without a GPU
can produce user kinds and the metric and stats units over them; it also exposes the four internal makers.  This script
builds the patched mm_rtc.hip alone into a shared library (it has no kernel and needs no other unit of the engine), drives
it through the cases of the issue, and writes per case the byte length, the sha256 and the ordered kernel names.  The functor
texts are the ones the tests use (tests/rtc_units_common.py)."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rtc_units_common as U  # noqa: E402

ROSENBROCK_ND, GAUSSIAN_ND, GAUSSIAN2D = 4, 6, 0
RTC_HDRS = ("mm_math.h mm_icdf_table.h mm_rng.h mm_targets.h mm_samplers.h mm_kernels.h mm_split_kernels.h mm_nuts.h "
            "mm_nuts_kernels.h mm_autodiff.h mm_data.h mm_discrete.h mm_discrete_kernels.h").split()


def main():
    tree, commit = sys.argv[1], sys.argv[2]
    out_json = sys.argv[3] if len(sys.argv) > 3 else U.GOLDEN
    csrc = os.path.join(tree, "mini_mcmc_amd", "csrc")
    work = tempfile.mkdtemp(prefix="rtc_record_")
    dump = os.path.join(work, "units")
    os.mkdir(dump)
    subprocess.run([sys.executable, os.path.join(tree, "tools", "gen_rtc_headers.py"), os.path.join(work, "mm_rtc_headers.inc")] + RTC_HDRS,
                   check=True, cwd=csrc)
    so = os.path.join(work, "librtc_dump.so")
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "-shared", "-I" + work, os.path.join(csrc, "mm_rtc.hip"),
                    "-o", so, "-ldl", "-lpthread"], check=True)
    os.environ["MMCMC_RTC_DUMP_DIR"] = dump
    lib = C.CDLL(so)
    F = {k: v.encode() for k, v in U.functors().items()}
    kind = C.c_int()

    def ok(status):
        assert status == 0, status
        return kind.value

    banana = ok(lib.mmcmc_target_register_source(b"target_banana", 2, F["banana"], C.byref(kind), None, 0))
    ok(lib.mmcmc_target_register_logp_source(b"target_banana_logp", 2, F["banana_logp"], C.byref(kind), None, 0))
    linreg3 = ok(lib.mmcmc_target_register_data_source(b"target_linreg3_hand", 3, C.c_size_t(U.LINREG3_DATA_LEN), 0, F["linreg3_hand"],
                                                       C.byref(kind), None, 0))
    ok(lib.mmcmc_target_register_data_source(b"target_linreg3_logp", 3, C.c_size_t(U.LINREG3_DATA_LEN), 1, F["linreg3_logp"], C.byref(kind),
                                             None, 0))
    ok(lib.mmcmc_proposal_register_source(b"model_gaussian2d", GAUSSIAN2D, 2, F["isotropic"], C.byref(kind), None, 0))
    ok(lib.mmcmc_proposal_register_source(b"model_banana", banana, 2, F["isotropic"], C.byref(kind), None, 0))
    ok(lib.mmcmc_proposal_register_source(b"model_linreg3", linreg3, 3, F["isotropic"], C.byref(kind), None, 0))
    ok(lib.mmcmc_discrete_register_source(b"discrete_poisson_reflect", F["poisson_reflect"], C.byref(kind), None, 0))

    def internal(name, which, k, dim, x=0):
        assert lib.mmcmc_rtc_dump_internal(name.encode(), which, k, dim, x) == 1, name

    for dim in (9, 16, 17):
        internal(f"builtin_rosenbrock_{dim}", 0, ROSENBROCK_ND, dim)
    internal("builtin_nuts_rosenbrock_9", 1, ROSENBROCK_ND, 9)
    internal("builtin_nuts_gaussian_17", 1, GAUSSIAN_ND, 17)
    for dense, word in ((0, "metric"), (1, "dense")):
        internal(f"{word}_rosenbrock_3", 2, ROSENBROCK_ND, 3, dense)
        internal(f"{word}_rosenbrock_17", 2, ROSENBROCK_ND, 17, dense)
        internal(f"{word}_banana", 2, banana, 2, dense)
    internal("metric_linreg3", 2, linreg3, 3, 0)
    for mk in range(3):
        internal(f"stats{mk}_rosenbrock_3", 3, ROSENBROCK_ND, 3, mk)
        internal(f"stats{mk}_banana", 3, banana, 2, mk)

    record = {"parent_commit": commit, "cases": U.summarise(dump)}
    with open(out_json, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print(len(record["cases"]), "cases ->", out_json, "(texts kept in", dump + ")")


if __name__ == "__main__":
    main()
