"""The staged device-to-host copy without a GPU (csrc/mm_hostcopy_plan.h): tests/cpp/hostcopy_ring.cpp, a stand-alone program
with its own main, built with the host compiler and flags of oracle/Makefile, walks the chunk and slice arithmetic, the
direct / staged decision, the copy-thread count of copies that enter together, and runs the ring's ordering protocol over a
memcpy transport -- the checks are listed at the top of the program.  It is built twice, with -fsanitize=thread and with
-fsanitize=address,undefined, and run directly (no preload involved).  The program prints how many cases of each kind it
walked and the counts are asserted exactly, so the walk cannot be vacuous."""
import os
import re
import subprocess

import pytest

import autodiff_common as A

ROOT = A.ROOT
SRC = os.path.join(ROOT, "tests", "cpp", "hostcopy_ring.cpp")


def test_header_is_host_only():
    text = open(os.path.join(ROOT, "mini_mcmc_amd", "csrc", "mm_hostcopy_plan.h")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', text) == ["sched.h", "atomic", "cstddef", "cstring", "thread", "vector"]
    assert not re.search(r"\bhip[A-Z_]\w*", text)  # no call, type or constant of the runtime
    unit = open(os.path.join(ROOT, "mini_mcmc_amd", "csrc", "mm_hostcopy.hip")).read()
    assert '#include "mm_hostcopy_plan.h"' in unit and "mm_hostcopy_ring(" in unit
    assert "std::thread" not in unit and "memory_order_acquire" not in unit  # one copy of the protocol: the header's


@pytest.mark.parametrize("sanitizer", ["thread", "address,undefined"], ids=["tsan", "asan_ubsan"])
def test_plan_budget_ring_protocol_and_failures_under_sanitizers(tmp_path, sanitizer):
    """plain host code with its own main: linked with the sanitizers' runtimes, no preload involved"""
    cxx, flags = A.host_flags()
    exe = str(tmp_path / "hostcopy_ring")
    r = subprocess.run([cxx] + flags + ["-fsanitize=" + sanitizer, "-fno-sanitize-recover=all", "-g", "-pthread", SRC, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66", ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-6000:])
    assert "WARNING: ThreadSanitizer" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr, r.stderr[-6000:]
    m = re.search(r"slices (\d+) chunk tilings (\d+) decisions (\d+) budgets (\d+) protocol (\d+) real chunk (\d+) failures (\d+) "
                  r"failed (\d+)", r.stdout)
    assert m, r.stdout[-1000:]
    slices, tilings, decisions, budgets, protocol, real, failures, failed = map(int, m.groups())
    assert failed == 0
    assert slices == (3 * 4096 + 1 + 4098) * 8  # len in {1 .. 3 * 4096 + 1} and {8 MiB - 4097 .. 8 MiB}, T in 1 .. 8
    assert tilings == 7 and decisions == 2 * 2 * 2
    assert budgets == 256 * 16  # cpus x copies entering together
    assert protocol == 13 * 5 * 3 == 195  # byte counts x T x destination offsets
    assert real == 2 * 2  # 8 MiB + 4 and 32 MiB + 4, T = 3 and 8, with the library's own chunk
    assert failures == 4 + 4 + 2  # issue, query at chunks 0, 3, 4, last; thread 0, T - 1 cannot start
