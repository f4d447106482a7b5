"""The diagnostics dispatch without a GPU (csrc/mm_stats_plan.h, stats_partials_impl in csrc/mm_stats.hip).

  * tests/cpp/stats_launch_trace.cpp includes mm_stats.hip itself behind recording stubs of the HIP calls its host code makes
    and walks 262 164 calls: every launch (kernel instance, grid, block, LDS bytes, arguments, workspace offsets) and every
    status must be what tests/golden/stats_launch_trace.json holds -- one SHA-256 per half-chain length, recorded from the
    commit the file names, before the dispatch moved onto one plan, and the full lines of forty named cases;
  * tests/cpp/stats_plan.cpp -- the header on its own, a plain host program -- checks every plan of the same grid (its head
    comment), as built and once more under the address and undefined-behaviour sanitizers (no preload involved);
  * the header includes nothing of HIP.

To record the golden file anew after a change that is meant to move a launch: build the trace program as the test does and
run `python3 tests/test_stats_plan_host.py <program> <commit>`."""
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "stats_launch_trace.json")
# 6 selectors x 2 dtypes x 2 alignments x 2 wb x 27 m x 2 n x 11 dims x 9 chain counts; 3 m beyond the direct-work limit x
# 2 limits x 2 dtypes; 2 entry points x 2 x 2 x 3 dtypes x 3 chain counts x 7 dims x 11 n
CALLS = 6 * 2 * 2 * 2 * 27 * 2 * 11 * 9 + 3 * 2 * 2 + 2 * (2 * 2 * 3 * 3 * 7 * 11)


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def _trace(exe):
    """({"<m>" | "entry": sha256}, calls, {name: [lines]}) of a built trace program"""
    out = _run(exe)
    digests = dict(re.findall(r"^(?:m )?(\w+) calls \d+ sha256 ([0-9a-f]{64})$", out, flags=re.M))
    named = {}
    for block in _run(exe, "--named").split("# ")[1:]:
        name, *lines = block.rstrip("\n").split("\n")
        named[name] = lines
    return digests, int(re.search(r"^calls (\d+)$", out, flags=re.M).group(1)), named


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "ubsan"])
def trace_exe(tmp_path_factory, request):
    """the trace program as built, and once more with the host code under the undefined-behaviour sanitizer (a stand-alone
    program: no preload involved)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("stats_trace") / "stats_launch_trace")
    extra = ["-Xarch_host", "-fsanitize=undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if request.param else []
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wno-unused-function", "-Wno-pass-failed"] + extra +
                       [os.path.join(ROOT, "tests", "cpp", "stats_launch_trace.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_launch_trace_of_the_dispatch_is_the_recorded_one(trace_exe):
    golden = json.load(open(GOLDEN))
    digests, calls, named = _trace(trace_exe)
    assert calls == CALLS == golden["calls"]  # the walk cannot shrink unnoticed
    assert len(golden["digests"]) == 27 + 1 and 38 <= len(golden["named"]) <= 42
    # the program's own SHA-256 against hashlib's on one length
    assert hashlib.sha256(_run(trace_exe, "--lines", "1").encode()).hexdigest() == digests["1"]
    for name, lines in golden["named"].items():
        assert named.get(name) == lines, "\n".join([name, "recorded:"] + lines + ["now:"] + named.get(name, ["(no such case)"]))
    assert set(digests) == set(golden["digests"])
    for m, sha in golden["digests"].items():
        if digests[m] != sha:
            print(_run(trace_exe, "--lines", m)[-20000:])
        assert digests[m] == sha, f"the launches of half-chain length {m} differ from those of {golden['parent']}"


def test_stats_plan_header_is_host_only():
    text = open(os.path.join(ROOT, "mini_mcmc_amd", "csrc", "mm_stats_plan.h")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', text) == ["../../include/mmcmc.h", "algorithm", "cstddef", "cstdint"]
    assert not re.search(r"getenv|mm_tuning_env\(", text)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_every_plan_fits_the_workspace_and_the_launch_limits(tmp_path, sanitize):
    """tests/cpp/stats_plan.cpp (its head comment), plain host code with its own main: as built and once more linked with
    the address and undefined-behaviour sanitizers' runtimes, no preload involved"""
    import autodiff_common as A

    cxx, flags = A.host_flags()
    exe = str(tmp_path / "stats_plan")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    r = subprocess.run([cxx] + flags + extra + [os.path.join(ROOT, "tests", "cpp", "stats_plan.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-4000:])
    plans, beyond = map(int, re.search(r"plans (\d+) beyond_limit (\d+)", r.stdout).groups())
    checks, failed = map(int, re.search(r"checks (\d+) failed (\d+)", r.stdout).groups())
    assert failed == 0
    # not vacuous: the trace's grid under 4 settings of the knobs, each plan the direct-work limit refuses once more without
    # the limit, 3 bad calls per selector; 12 checks per plan
    assert beyond == 54384 and plans == 4 * 6 * 2 * 2 * 2 * 27 * 2 * 11 * 9 + beyond + 6 * 3
    assert checks == 12 * plans


if __name__ == "__main__":
    digests, calls, named = _trace(sys.argv[1])
    json.dump({"parent": sys.argv[2], "calls": calls, "digests": digests, "named": named}, open(GOLDEN, "w"), indent=1)
    print(f"{GOLDEN}: {calls} calls, {len(digests)} digests, {len(named)} named cases")
