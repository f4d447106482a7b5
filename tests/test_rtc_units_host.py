"""The rules of the run-time compiled units (csrc/mm_rtc_units.h) on the host: tests/cpp/rtc_units.cpp, a stand-alone program
with its own main, built with the host compiler of oracle/Makefile and -fsanitize=address,undefined, produces the text of every
unit kind from the header's builders and walks the kernel table, the compiler child's result rule and environment filter and
the unit-kind predicates -- the checks are listed at the top of the program.  The texts are compared here with
tests/golden/rtc_unit_texts.json, taken from the commit before the header existed (tools/experiments/rtc_record_units.py): byte
length, sha256 and the ordered kernel names of each.  The program prints how many cases it walked and the counts are asserted
exactly, so the walk cannot be vacuous."""
import json
import os
import re
import subprocess

import autodiff_common as A
import rtc_units_common as U

ROOT = A.ROOT
SRC = os.path.join(ROOT, "tests", "cpp", "rtc_units.cpp")


def test_header_is_host_only():
    text = open(os.path.join(ROOT, "mini_mcmc_amd", "csrc", "mm_rtc_units.h")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', text) == ["string", "vector", "../../include/mmcmc.h"]
    assert "getenv" not in text  # the environment is read in mm_rtc.hip and handed in


def test_unit_texts_tables_and_child_rules_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """plain host code with its own main: linked with the sanitizers' runtimes, no preload involved"""
    cxx, flags = A.host_flags()
    exe = str(tmp_path / "rtc_units")
    r = subprocess.run([cxx] + flags + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", SRC, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    functors, units = tmp_path / "functors", tmp_path / "units"
    functors.mkdir()
    units.mkdir()
    U.write_functors(str(functors))
    r = subprocess.run([exe, str(functors), str(units)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-4000:])
    m = re.search(r"texts (\d+) tables (\d+) crossed (\d+) child results (\d+) env entries (\d+) predicates (\d+) flag lists (\d+) "
                  r"failed (\d+)", r.stdout)
    assert m, r.stdout[-1000:]
    texts, tables, crossed, results, env, predicates, flag_lists, failed = map(int, m.groups())
    assert failed == 0
    assert texts == 26 and crossed == texts  # the cases of the record, each also held against the kernel table
    assert tables == 7 * 4  # unit kinds x dims 1, 8, 9, 32
    assert results == 2 * 2 * 7 * 3  # spawned, reaped elsewhere, statuses, code object present / empty / absent
    assert env == 20 and predicates == 7 * 4 and flag_lists == 1

    record = json.load(open(U.GOLDEN))
    assert re.fullmatch(r"[0-9a-f]{40}", record["parent_commit"])
    got = U.summarise(str(units))
    assert len(record["cases"]) == 26 and sorted(got) == sorted(record["cases"])
    for name, want in record["cases"].items():
        assert got[name]["kernels"] == want["kernels"], name
        assert got[name]["bytes"] == want["bytes"], name
        assert got[name]["sha256"] == want["sha256"], name
