#!/usr/bin/env python3
"""Is the device code of two builds of the library the same?  Two libraries in, a verdict out (exit status 1 if not).

    tools/isa_diff.py OLD.so NEW.so [--map REGEX=REPLACEMENT ...] [--may-differ REGEX] [-v]

Every gfx950 code object of either library is disassembled and cut by symbol; kernels (the symbols with a descriptor) and device
functions are compared by demangled name.  --map rewrites OLD's names first (a refactor that drops a template argument:
--map '(k_step5<[^>]*), false>=\\1>').  Required: the same names, none in more code objects than before, the same instruction
text.  One difference is tolerated and named: literals of s_add_u32 / s_addc_u32, the pc-relative distance to a constant or a
callee, which moves with whatever else the code object holds.  --may-differ names the kernels a change is MEANT to alter or to
remove; they are listed, not refused.  The lb_* exports of the two libraries must be the same set.
"""
import collections
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_agpr_window import LLVM, code_objects


def functions(lib):
    """({demangled name: [instruction text, one list per code object that holds it]}, {kernel names})"""
    funcs, kernels = collections.defaultdict(list), set()
    for co in code_objects(lib):
        with tempfile.NamedTemporaryFile(prefix="isa_", suffix=".co") as f:
            f.write(co)
            f.flush()
            run = lambda *cmd: subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
            for line in run(LLVM + "/llvm-objdump", "-t", "-C", f.name).splitlines():
                m = re.search(r"\s[0-9a-f]{16}\s+(?:\.\w+ )?(.*?) ?\(?\.kd\)?$", line)
                if m:
                    kernels.add(m.group(1))
            body = None
            for line in run(LLVM + "/llvm-objdump", "-d", "-C", "--no-show-raw-insn", "--no-leading-addr", f.name).splitlines():
                m = re.match(r"^(?:[0-9a-f]+ )?<(.*)>:$", line)
                if m:
                    body = []
                    funcs[m.group(1)].append(body)
                elif body is not None and line.strip():
                    body.append(line.split("//")[0].strip())
    return funcs, kernels


def pc_relative_only(a, b):
    mask = lambda s: re.sub(r"^(s_addc?_u32 \S+ \S+) \S+$", r"\1 #", s)
    return len(a) == len(b) and all(mask(x) == mask(y) for x, y in zip(a, b))


def exports(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout      # (an object file: none)
    return {l.split()[-1] for l in out.splitlines() if l.split() and l.split()[-1].startswith("lb_")}


def main():
    argv, maps, may, verbose = sys.argv[1:], [], None, False
    libs = []
    while argv:
        a = argv.pop(0)
        if a == "--map":
            maps.append(argv.pop(0).split("=", 1))
        elif a == "--may-differ":
            may = re.compile(argv.pop(0))
        elif a == "-v":
            verbose = True
        else:
            libs.append(a)
    (fo, ko), (fn, kn) = functions(libs[0]), functions(libs[1])

    def mapped(name):
        for rx, rep in maps:
            name = re.sub(rx, rep, name)
        return name
    fo = {mapped(k): v for k, v in fo.items()}
    ko = {mapped(k) for k in ko}
    bad = 0
    print("kernels: %d | %d; functions in all: %d | %d" % (len(ko), len(kn), len(fo), len(fn)))
    for k in sorted(set(fo) ^ set(fn)):
        if k in fo and may and may.search(k):
            print("   removed, as meant: %s" % k)
            continue
        print("   ONLY IN %s: %s" % ("OLD" if k in fo else "NEW", k))
        bad += 1
    same = moved = 0
    for k in sorted(set(fo) & set(fn)):
        if len(fn[k]) > len(fo[k]):
            print("   IN MORE CODE OBJECTS (%d -> %d): %s" % (len(fo[k]), len(fn[k]), k))
            bad += 1
        for a, b in zip(sorted(fo[k]), sorted(fn[k])):
            if a == b:
                same += 1
            elif pc_relative_only(a, b):
                moved += 1
                print("   pc-relative offsets only: %s" % k)
            elif may and may.search(k):
                print("   differs, as meant (%d -> %d instructions): %s" % (len(a), len(b), k))
            else:
                print("   DIFFERS (%d -> %d instructions): %s" % (len(a), len(b), k))
                bad += 1
                if verbose:
                    import difflib
                    print("\n".join(list(difflib.unified_diff(a, b, lineterm="", n=1))[:40]))
    eo, en = exports(libs[0]), exports(libs[1])
    print("instruction text equal: %d; equal but for pc-relative offsets: %d; lb_* exports: %d | %d" % (same, moved, len(eo), len(en)))
    if eo != en:
        print("   EXPORTS DIFFER:", sorted(eo ^ en))
        bad += 1
    print("IDENTICAL" if not bad else "NOT IDENTICAL: %d findings" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
