"""Shared by tests/test_autodiff_host.py and tests/test_autodiff_gpu.py: builds and runs the host program
tests/cpp/autodiff_host.cpp (forward-mode gradients of csrc/mm_autodiff.h with the host twin's compiler and flags) once per
session and hands out its arrays; the log-density bodies it evaluates are the files the GPU tests register."""
import functools
import os
import re
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "cpp", "autodiff_cases")
SRC = os.path.join(ROOT, "tests", "cpp", "autodiff_host.cpp")
BANANA_PARAMS = [1.5, 0.5]  # s, b of tests/test_user_target.py::test_new_density_samples_what_it_describes


def host_flags():
    """CXX and CXXFLAGS of oracle/Makefile: what engine_host.cpp, the host twin of the kernels, is built with"""
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    cxx = re.search(r"^CXX\s*\?=\s*(\S+)", mk, flags=re.M).group(1)
    flags = re.search(r"^CXXFLAGS\s*\?=\s*(.+)$", mk, flags=re.M).group(1).split()
    return cxx, flags


def build_host(out_dir, sanitize=False):
    cxx, flags = host_flags()
    exe = os.path.join(out_dir, "autodiff_host" + ("_san" if sanitize else ""))
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    r = subprocess.run([cxx] + flags + extra + [SRC, "-o", exe, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run_host(exe, out_dir):
    """{(case, "f32" | "f64"): {"x", "value", "value_plain", "grad", ["value_hand", "grad_hand"]}}"""
    path = os.path.join(out_dir, os.path.basename(exe) + ".bin")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    raw = open(path, "rb").read()
    res = {}
    for ln in r.stdout.splitlines():
        name, ty, dim, n, off, hand = ln.split()
        dim, n, off = int(dim), int(n), int(off)
        dt = np.float32 if ty == "f32" else np.float64
        fields = [("x", (n, dim)), ("value", (n,)), ("value_plain", (n,)), ("grad", (n, dim))]
        if hand == "1":
            fields += [("value_hand", (n,)), ("grad_hand", (n, dim))]
        rec = {}
        for key, shape in fields:
            cnt = int(np.prod(shape))
            rec[key] = np.frombuffer(raw, dtype=dt, count=cnt, offset=off).reshape(shape).copy()
            off += cnt * np.dtype(dt).itemsize
        res[(name, ty)] = rec
    return res


@functools.lru_cache(maxsize=None)
def host_results():
    """the host program's output, built with the host twin's flags; computed once and shared (treat as read-only)"""
    d = tempfile.mkdtemp(prefix="autodiff_host_")
    return run_host(build_host(d), d)


def case_source(name):
    """the HIP source of case `name` of the host program and its dimension: ("rosenbrock9" -> rosenbrock.inc, 9)"""
    m = re.fullmatch(r"rosenbrock(\d+)", name)
    text = open(os.path.join(CASES, "rosenbrock.inc" if m else name + ".inc")).read()
    return text, int(m.group(1)) if m else 2


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)
