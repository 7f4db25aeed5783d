#!/usr/bin/env python3
"""Is every kernel's device code the same in two builds?  (the check behind
"every existing kernel's figures are unchanged")

  hipcc <the Makefile's FLAGS> --cuda-device-only -S csrc/f.hip -o old/f.s   (per .hip file, both trees)
  python3 tools/isa_diff.py old/ new/ [--rename upd_hist_kernel=grp_hist_kernel ...]

Each side is a directory of .s files or a single file.  Functions are matched
by symbol over the whole set, so one that moved to another file still matches.
Compared: a function's instructions, labels and its .amdhsa_ kernel
descriptor (registers, LDS, scratch).  Ignored: comments, .file / .ident /
.loc / .cfi / .section directives, __hip_cuid_ lines and the numbering of
local labels, which follows the function's position in its file.  Prints
`same` or `differs` per function; exit status 1 on a difference or on a
function that one side lacks.
"""
import argparse
import glob
import os
import re
import subprocess

SKIP = re.compile(r"\s*\.(file|ident|loc|cfi_\w+|section)\b|.*__hip_cuid_")


def functions(path, renames):
    """symbol -> list of bodies (one per file that defines it)"""
    files = sorted(glob.glob(os.path.join(path, "*.s"))) if os.path.isdir(path) else [path]
    out = {}
    for f in files:
        text = open(f).read()
        for old, new in renames:
            text = text.replace("%d%s" % (len(old), old), "%d%s" % (len(new), new))
        funcs, cur = set(re.findall(r"^\s*\.type\s+(\S+),@function", text, re.M)), None
        for ln in text.splitlines():
            ln = ln.split(";")[0].rstrip()
            m = re.match(r"(\S+):$", ln)
            if m and m.group(1) in funcs:
                cur = out.setdefault(m.group(1), [])
                cur.append([])
            elif re.match(r"\.Lfunc_end\d+:$", ln):
                cur = None
            elif cur is not None and ln.strip() and not SKIP.match(ln):
                cur[-1].append(re.sub(r"\.L([A-Za-z_]+?)\d+_", r".L\1_", " ".join(ln.split())))
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
        return [re.sub(r"espgpu::\(anonymous namespace\)::", "", d) for d in r.stdout.splitlines()]
    except OSError:
        return names


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[], metavar="old=new",
                    help="a function renamed on purpose (applied to the old side's symbols)")
    a = ap.parse_args()
    old = functions(a.old, [r.split("=", 1) for r in a.rename])
    new = functions(a.new, [])
    names = sorted(set(old) | set(new))
    bad = 0
    for n, d in zip(names, demangle(names)):
        if n in old and n in new:
            verdict = "same" if sorted(old[n]) == sorted(new[n]) else "differs"
        else:
            verdict = "missing in " + (a.old if n not in old else a.new)
        bad += verdict != "same"
        print("%-8s %s" % (verdict, d[:110]))
    print("%d functions, %d not the same" % (len(names), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    raise SystemExit(main())
