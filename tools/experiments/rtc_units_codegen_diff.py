#!/usr/bin/env python3
"""Do the run-time compiled units give the same gfx950 machine code against two sets of kernel headers?  (no GPU needed)

    python3 tools/experiments/rtc_units_codegen_diff.py <unit texts dir> <old csrc> <new csrc> [name filter]

The unit texts are the ones tests/cpp/rtc_units.cpp writes (its second argument: `rtc_units <functors dir> <units dir>`, the
functors from tests/rtc_units_common.write_functors), named <case>.hip; the dimension (-DMM_USER_DIM) is read off the name.
Each text is compiled twice with the flag list of csrc/mm_rtc_units.h, device side only, to assembly, and the kernels are
compared instruction by instruction (directives and comments stripped, as tools/codeobj_diff.py strips addresses and
encodings), with the register / LDS / scratch figures of the kernel descriptors.  Exit status 1 if anything differs."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

DIMS = {"banana": 2, "linreg3": 3, "gaussian2d": 2}
FIGURES = (".amdhsa_next_free_vgpr", ".amdhsa_next_free_sgpr", ".amdhsa_accum_offset", ".amdhsa_group_segment_fixed_size",
           ".amdhsa_private_segment_fixed_size")


def dim_of(case):
    m = re.search(r"_(\d+)$", case)
    if m:
        return int(m.group(1))
    return next((d for k, d in DIMS.items() if k in case), 1)  # an integer-state unit has no dimension


def kernels(asm):
    out, name = {}, None
    for ln in asm.splitlines():
        m = re.match(r"^(\w+):", ln)
        if m and not m.group(1).startswith((".L", "__hip_cuid_")):  # the per-unit hash symbol differs by construction
            name = m.group(1)
            out[name] = []
        elif ln.startswith(".Lfunc_end"):
            name = None
        elif name and ln.startswith("\t") and not ln.startswith(("\t.", "\t;")):
            out[name].append(ln.split(";")[0].strip())
        m = re.match(r"^\t(\.amdhsa_\w+) (\S+)", ln)
        if m and m.group(1) in FIGURES:
            out.setdefault("figures", []).append(ln.strip())
    return out


def build(text, csrc, dim, out):
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", f"-DMM_USER_DIM={dim}", "-Wno-pass-failed",
                    "--cuda-device-only", "-S", "-I" + csrc, text, "-o", out], check=True, capture_output=True)
    return kernels(open(out).read())


def main():
    units, old, new = sys.argv[1:4]
    only = sys.argv[4] if len(sys.argv) > 4 else ""
    cases = sorted(f[:-4] for f in os.listdir(units) if f.endswith(".hip") and only in f)
    work = tempfile.mkdtemp(prefix="rtc_codegen_")

    def one(case):
        text = os.path.join(units, case + ".hip")
        a = build(text, old, dim_of(case), os.path.join(work, case + ".old.s"))
        b = build(text, new, dim_of(case), os.path.join(work, case + ".new.s"))
        return case, a, b

    bad = n_k = n_i = 0
    with ThreadPoolExecutor(8) as pool:
        for case, a, b in pool.map(one, cases):
            diff = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
            n_k += len(a) - 1
            n_i += sum(len(v) for k, v in b.items() if k != "figures")
            print(case, len(a) - 1, "kernels", "identical" if not diff else "DIFFER: " + " ".join(diff))
            bad += len(diff)
    print(f"{len(cases)} units, {n_k} kernels, {n_i} instructions, {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
