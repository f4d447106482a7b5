"""The kernel-path rule of an MH / HMC handle (csrc/mm_path.h) on the host: tests/cpp/path_rule.cpp, a stand-alone program
with its own main, built with the host compiler of oracle/Makefile and -fsanitize=address,undefined, walks every combination of
the handle facts, every variant from -1 to 9, n_leapfrog in {0, 9, 10} and scheduled or not.  It asserts that the default
variant is always accepted, that an accepted variant never names a launcher the handle lacks (no null function pointer can
be reached), that every other variant is INVALID_ARG or UNSUPPORTED, and each quirk of the public variant numbers.  The
statuses of real handles are compared with the recorded ones in tests/test_kernel_paths.py (GPU)."""
import os
import re
import subprocess

import autodiff_common as A

ROOT = A.ROOT
SRC = os.path.join(ROOT, "tests", "cpp", "path_rule.cpp")
DIMS, BOOLS, UNITS = 8, 9, 3


def test_header_is_host_only():
    text = open(os.path.join(ROOT, "mini_mcmc_amd", "csrc", "mm_path.h")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', text) == ["../../include/mmcmc.h"]


def test_path_rule_over_every_handle_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """plain host code with its own main: linked with the sanitizers' runtimes, no preload involved"""
    cxx, flags = A.host_flags()
    exe = str(tmp_path / "path_rule")
    r = subprocess.run([cxx] + flags + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", SRC, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-4000:])
    m = re.search(r"combinations (\d+) handles (\d+) tuples (\d+) failed (\d+)", r.stdout)
    assert m, r.stdout[-1000:]
    combos, handles, tuples, failed = map(int, m.groups())
    assert failed == 0
    assert combos == 2 * 2 * DIMS * (1 << BOOLS) * UNITS  # sampler x dtype x dim x every boolean x unit state
    # not vacuous: at the least every fixed-entry handle without a unit at each dim (2 x 2 x 8 x 2^4 launcher / generic facts),
    # and every one of them has its default plus at least one more accepted variant, walked at 3 L x 2 schedules
    assert handles >= 2 * 2 * DIMS * 16
    assert tuples >= handles * 6
