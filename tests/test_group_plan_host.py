"""The host rules of a device group (csrc/mm_group_plan.h): tests/cpp/group_plan.cpp, a stand-alone program with its own main,
built with the host compiler of oracle/Makefile and -fsanitize=address,undefined, walks the partition of the chains over
every n_devices in 1..64 and n_chains in n_devices..n_devices + 130, the exchange status over all eight combinations of its
three facts, and both rules for a failed run over every (n_advanced, N) with N <= 8.  These rules sit between HIP calls in
csrc/mm_group.hip and no GPU test provokes a failed run; here they are checked without a device."""
import os
import re
import subprocess

import autodiff_common as A

ROOT = A.ROOT
SRC = os.path.join(ROOT, "tests", "cpp", "group_plan.cpp")


def test_header_is_host_only():
    text = open(os.path.join(ROOT, "mini_mcmc_amd", "csrc", "mm_group_plan.h")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', text) == ["../../include/mmcmc.h"]


def test_group_rules_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """plain host code with its own main: linked with the sanitizers' runtimes, no preload involved"""
    cxx, flags = A.host_flags()
    exe = str(tmp_path / "group_plan")
    r = subprocess.run([cxx] + flags + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", SRC, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-4000:])
    m = re.search(r"partitions (\d+) device lists (\d+) exchanges (\d+) break cases (\d+) failed (\d+)", r.stdout)
    assert m, r.stdout[-1000:]
    partitions, lists, exchanges, breaks, failed = map(int, m.groups())
    assert failed == 0
    assert partitions == 64 * 131  # n_devices x n_chains
    assert lists == 3 + 9 + 27 + 81  # every list of one to four devices out of three
    assert exchanges == 8
    assert breaks == 3 * sum(n + 1 for n in range(1, 9))  # three statuses x n_advanced in 0..N x N in 1..8
