"""The host rules of a NUTS handle (csrc/mm_nuts_plan.h) on the host: tests/cpp/nuts_plan.cpp, a stand-alone program with its
own main, built with the host compiler of oracle/Makefile and -fsanitize=address,undefined, walks the step plan, the kernel-path
rule over every consistent handle, the lane-group schedule (mode, scheduler grid, level from a histogram), the pilot split and
the chain groups of variant 2 -- the checks are listed at the top of the program.  It prints how many cases it walked and the
counts are asserted exactly here, so the walk cannot be vacuous.  The statuses of real handles are compared with the recorded
ones in tests/test_nuts_kernel_paths.py (GPU)."""
import os
import re
import subprocess

import autodiff_common as A

ROOT = A.ROOT
SRC = os.path.join(ROOT, "tests", "cpp", "nuts_plan.cpp")


def test_header_is_host_only():
    text = open(os.path.join(ROOT, "mini_mcmc_amd", "csrc", "mm_nuts_plan.h")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', text) == ["../../include/mmcmc.h"]
    assert "getenv" not in text  # the measurement knobs are read in mm_nuts_api.hip and handed in


def test_nuts_plan_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """plain host code with its own main: linked with the sanitizers' runtimes, no preload involved"""
    cxx, flags = A.host_flags()
    exe = str(tmp_path / "nuts_plan")
    r = subprocess.run([cxx] + flags + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", SRC, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-4000:])
    m = re.search(r"step plans (\d+) caps (\d+) handles (\d+) accepted (\d+) schedules (\d+) pilot cases (\d+) splits (\d+) "
                  r"group cases (\d+) groups (\d+) transitions (\d+) failed (\d+)", r.stdout)
    assert m, r.stdout[-1000:]
    steps, caps, handles, accepted, schedules, pilots, splits, group_cases, groups, transitions, failed = map(int, m.groups())
    assert failed == 0
    assert steps == 7 * 7 * 5 + 3 + 10  # (n_collect, n_discard, progress), the row limit per progress, ten edge cases
    # six booleans; consistent: an instance (x async x pair x lane groups x generic), a unit (x lane groups x generic), or
    # neither and the run-time-dimension kernel (x lane groups)
    assert caps == 64 and handles == 16 + 4 + 2
    # per handle: the variants it takes without a metric, plus 7 alone under each of the five (metric, recording) states
    assert accepted == 191 and accepted > handles * 6
    assert schedules == 3 * 3 * 6 + 4200 * 2 * 2 * 6 + 13 * 4  # modes, grids, levels
    assert pilots == 41 * 81 * 2 * 2 * 2
    assert splits == sum(1 for p in range(41) for r in range(81) if p + r >= 64) * 4  # level unknown only
    assert group_cases == (700 + 3) * 17 and groups > group_cases
    assert transitions == sum(p + r for p in range(6) for r in range(6)) * 4
