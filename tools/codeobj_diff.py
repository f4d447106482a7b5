"""Are the gfx950 kernels of two builds of libmmcmc.so the same machine code?  (no GPU needed)
    python3 tools/codeobj_diff.py old/libmmcmc.so new/libmmcmc.so [--rename names.txt]
Unwraps every gfx950 code object of both libraries (isa_mix.code_objects), disassembles them (llvm-objdump -d) and compares
kernel by kernel: the instruction streams (addresses and encodings stripped; branch offsets are relative and stay) and the
register / LDS / scratch figures of the code-object metadata (llvm-readelf --notes).  names.txt: lines `old-symbol new-symbol`
for kernels whose mangled name changed.  Lists what differs; exit status 1 if anything does."""
import os
import re
import subprocess
import sys
import tempfile

from isa_mix import OBJDUMP, code_objects

READELF = os.path.join(os.path.dirname(OBJDUMP), "llvm-readelf")
FIGURES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def kernels(so):
    """{symbol: (instruction lines, {figure: value})} over all gfx950 code objects of `so`"""
    out = {}
    for co in code_objects(so):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            dis = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", f.name], capture_output=True, text=True, check=True).stdout
            notes = subprocess.run([READELF, "--notes", f.name], capture_output=True, text=True, check=True).stdout
        figures = {}
        for entry in re.split(r"\n  - (?=\.)", notes):  # one per kernel: the list items at the outer indent
            name = re.search(r"^    \.name:\s+(\S+)", entry, re.M)
            if name:
                figures[name.group(1)] = {k: int(re.search(re.escape(k) + r":\s+(\d+)", entry).group(1)) for k in FIGURES}
        name = None
        for ln in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\w+)>:", ln)
            if m:
                name = m.group(1)
                out[name] = ([], figures.get(name, {}))
            elif name and ln.startswith("\t") and ln.strip() != "...":  # "...": zero fill up to the next symbol, no instruction
                out[name][0].append(ln.split("//")[0].strip())
    return out


def main(argv):
    args = [a for a in argv if not a.startswith("--")]
    rename = {}
    if "--rename" in argv:
        path = argv[argv.index("--rename") + 1]
        args.remove(path)
        rename = dict(ln.split() for ln in open(path) if ln.strip())
    old = {rename.get(k, k): v for k, v in kernels(args[0]).items()}
    new = kernels(args[1])
    cuid = re.compile(r"^__hip_cuid_")
    bad = 0
    for k in sorted(set(old) ^ set(new)):
        if not cuid.match(k):
            print(("only in old: " if k in old else "only in new: ") + k)
            bad += 1
    for k in sorted(set(old) & set(new)):
        (ia, fa), (ib, fb) = old[k], new[k]
        if ia != ib:
            at = next((i for i, (x, y) in enumerate(zip(ia, ib)) if x != y), min(len(ia), len(ib)))
            print(f"code differs: {k}: {len(ia)} / {len(ib)} instructions, first at {at}: {ia[at:at + 1]} / {ib[at:at + 1]}")
            bad += 1
        if fa != fb:
            print(f"figures differ: {k}: {fa} / {fb}")
            bad += 1
    print(f"{len(set(old) & set(new))} symbols in both, {sum(len(v[0]) for v in new.values())} instructions in new, {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
