#!/usr/bin/env python3
"""Did a change of the source files change a kernel?  Compiles .hip files of two source trees to gfx950 assembly
(the Makefile's HIPCC / ARCH / CXXFLAGS with --cuda-device-only -S; once plain, once with -DPPRHIP_TEST_HOOKS) and
compares, kernel by kernel, the function text (label .. .Lfunc_end) and the .amdhsa_kernel descriptor (registers,
LDS and private segment sizes), comments stripped and local labels renumbered.  A kernel may move between files;
it has to be defined in exactly one file of each tree.  Text is compared as text: no instruction is looked for.

  python tools/kernel_isa_diff.py --old ../parent --old-files csrc/kernels_push.hip \\
      --new-files csrc/kernels_push.hip csrc/kernels_dense.hip ... [-o profiles/push_split_isa.txt]

Paths of files are relative to the package directory (where the Makefile is); --new defaults to this checkout.
Exit status 0 iff both builds have the same kernel symbols and every kernel's two texts are identical."""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

PKG = "personalized-pagerank-algorithms-on-neo4j_amd"
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_var(makefile, name, default=None):
    m = re.search(r"^%s\s*[?:]?=\s*(.*)$" % name, open(makefile).read(), re.M)
    return m.group(1).strip() if m else default


def assembly(tree, rel, defines):
    pkg = os.path.join(os.path.abspath(tree), PKG)
    mk = os.path.join(pkg, "Makefile")
    cmd = [make_var(mk, "HIPCC"), "--offload-arch=" + make_var(mk, "ARCH")] + make_var(mk, "CXXFLAGS").split() + defines
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.check_call(cmd + ["--cuda-device-only", "-S", os.path.join(pkg, rel), "-o", out], cwd=pkg)
        return open(out).read().split("\n")


def normal(lines):
    """comments out, local labels (.LBB<function>_<n>, .Lfunc_end<function>, ...) without the function's number"""
    out = []
    for ln in lines:
        ln = ln.split(";", 1)[0].rstrip()
        ln = re.sub(r"\.L([A-Za-z_]+?)\d+_(\d+)", r".L\1_\2", ln)
        ln = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", ln)
        if ln.strip():
            out.append(ln)
    return "\n".join(out)


def kernels(lines):
    """{symbol: (function text, descriptor text)} of one assembly file"""
    found = {}
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if not m:
            continue
        sym = m.group(1)
        j = next(k for k in range(i, len(lines)) if lines[k].strip() == ".end_amdhsa_kernel")
        a = next(k for k in range(len(lines)) if lines[k].startswith(sym + ":"))
        b = next(k for k in range(a, len(lines)) if re.match(r"\.Lfunc_end\d+:", lines[k]))
        found[sym] = (normal(lines[a:b + 1]), normal(lines[i:j + 1]))
    return found


def collect(tree, files, defines):
    """{symbol: (file, function text, descriptor text)}; a symbol defined by two files is an error"""
    table = {}
    for rel in files:
        for sym, (fn, desc) in kernels(assembly(tree, rel, defines)).items():
            if sym in table:
                raise SystemExit("%s is defined in %s and in %s" % (sym, table[sym][0], rel))
            table[sym] = (os.path.basename(rel), fn, desc)
    return table


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--old", required=True, help="checkout of the commit to compare against")
    ap.add_argument("--new", default=HERE)
    ap.add_argument("--old-files", nargs="+", required=True)
    ap.add_argument("--new-files", nargs="+", required=True)
    ap.add_argument("-o", "--output")
    args = ap.parse_args()
    rows, ok = [], True
    for build, defines in (("plain", []), ("hooks", ["-DPPRHIP_TEST_HOOKS"])):
        old, new = collect(args.old, args.old_files, defines), collect(args.new, args.new_files, defines)
        for sym in sorted(set(old) | set(new)):
            if sym not in old or sym not in new:
                rows.append("%s %s only in the %s tree" % (build, sym, "old" if sym in old else "new"))
                ok = False
                continue
            (fo, to, do), (fn, tn, dn) = old[sym], new[sym]
            same_t, same_d = to == tn, do == dn
            ok = ok and same_t and same_d
            rows.append("%s %s %s -> %s: text %d lines %s %s, descriptor %s %s" % (
                build, sym, fo, fn, tn.count("\n") + 1, hashlib.sha1(tn.encode()).hexdigest()[:12],
                "identical" if same_t else "DIFFERS", hashlib.sha1(dn.encode()).hexdigest()[:12],
                "identical" if same_d else "DIFFERS"))
        rows.append("%s: %d kernels in the old files, %d in the new files" % (build, len(old), len(new)))
    rows.append("verdict: " + ("no kernel changed" if ok else "KERNELS CHANGED"))
    text = "\n".join(rows) + "\n"
    sys.stdout.write(text)
    if args.output:
        open(args.output, "w").write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
