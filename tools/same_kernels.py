#!/usr/bin/env python
"""Do two versions of some kernel sources compile to the same device code?  The check behind every refactor of a kernel file
that claims "the instruction streams are the previous commit's" (DESIGN.md 4.8), as a script.

    python tools/same_kernels.py REV FILE [FILE...] [--against FILE...] [-D MACRO...]

The FILEs of git revision REV (with that revision's csrc/*.h and include/) against the --against files of the working tree
(default: the same names), each compiled with build.FLAGS plus --cuda-device-only -S.  A kernel is the text from its label
to its .Lfunc_end, its .amdhsa_kernel descriptor block (kernarg size, register counts, LDS, scratch) and the .set lines of its
resource symbols, with comments, .file / .ident and the __hip_cuid_* symbol stripped, the .LBB<n>_ labels renumbered and its
own mangled name replaced; it is keyed by its demangled name without the anonymous-namespace component, so a kernel may move
between files and namespaces.  Reports the kernels on one side only, the pairs that differ (first differing line) and the
number of identical ones; a kernel that several files carry (the static kernels of common.h) must equal the other side's in
every copy and is listed.  Exit status 0 only if both sets are equal and every pair is identical.  Text only, CPU only."""
import argparse
import bisect
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from equihgnn_amd import build  # noqa: E402

CXXFILT = next((c for c in ("/opt/rocm/llvm/bin/llvm-cxxfilt", shutil.which("llvm-cxxfilt"), shutil.which("c++filt"))
                if c and os.path.exists(c)), None)       # the toolchain's demangler, or binutils'
HEADER_DIRS = (os.path.relpath(build.CSRC, build.ROOT), os.path.relpath(build.INCLUDE, build.ROOT))


def git(*args):
    return subprocess.check_output(["git", "-C", build.ROOT, *args])


def checkout(rev, files, dst):
    """`files` and every header of revision `rev` under dst/, at their paths in the repository"""
    headers = [p for d in HEADER_DIRS for p in git("ls-tree", "--name-only", rev, d + "/").decode().split() if p.endswith(".h")]
    for path in [*headers, *files]:
        out = os.path.join(dst, path)
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "wb") as f:
            f.write(git("show", f"{rev}:{path}"))


def assembly(root, path, defines, out):
    """device assembly of root/path, compiled against root's headers"""
    flags = list(build.FLAGS)
    for i, f in enumerate(flags):                 # -I INCLUDE -I CSRC -> the same directories under `root`
        if f in (build.INCLUDE, build.CSRC):
            flags[i] = os.path.join(root, os.path.relpath(f, build.ROOT))
    subprocess.check_call([build._hipcc(), *flags, *(f"-D{d}" for d in defines), "--cuda-device-only", "-S",
                           os.path.join(root, path), "-o", out])
    with open(out) as f:
        return f.read()


def kernels(asm):
    """{mangled name: normalised text} of the kernels of one assembly file"""
    lines = [re.sub(r"\s*;.*$", "", ln).rstrip() for ln in asm.split("\n")]
    lines = [ln for ln in lines if ln.strip() and not re.match(r"\s*\.(file|ident)\b", ln) and "__hip_cuid_" not in ln]
    # one pass: where every label, .Lfunc_end and descriptor block stands, and the .set lines by the symbol they define
    label, ends, desc, sets = {}, [], {}, {}
    for i, ln in enumerate(lines):
        word = ln.split()
        if ln[0] not in " \t." and ln.endswith(":"):
            label[ln[:-1]] = i
        elif re.match(r"\.Lfunc_end\d+:", ln):
            ends.append(i)
        elif word[0] == ".amdhsa_kernel":
            desc[word[1]] = i
        elif word[0] == ".set" and "." in word[1]:
            sets.setdefault(word[1].rsplit(".", 1)[0], []).append(ln)
    res = {}
    for name, d0 in desc.items():
        end = ends[bisect.bisect_left(ends, label[name])]
        d1 = next(i for i in range(d0, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
        text = "\n".join([*lines[label[name]:end + 1], *lines[d0:d1 + 1], *sets.get(name, [])]).replace(name, "<kernel>")
        res[name] = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", re.sub(r"\.(LBB|LJTI|Ltmp)\d+_", r".\1_", text))
    return res


def keyed(per_file):
    """{demangled key: [(file, text), ...]} over the files of one side"""
    names = sorted({n for ks in per_file.values() for n in ks})
    plain = subprocess.run([CXXFILT], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    key = {n: d.replace("(anonymous namespace)::", "") for n, d in zip(names, plain)}
    res = {}
    for path, ks in per_file.items():
        for n, text in ks.items():
            res.setdefault(key[n], []).append((path, text))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("rev")
    ap.add_argument("files", nargs="+", metavar="FILE")
    ap.add_argument("--against", nargs="+", metavar="FILE", help="working-tree files (default: the same names)")
    ap.add_argument("-D", dest="defines", action="append", default=[], metavar="MACRO")
    a = ap.parse_args()
    rel = lambda p: os.path.relpath(os.path.abspath(p), build.ROOT)
    old_files, new_files = [rel(p) for p in a.files], [rel(p) for p in (a.against or a.files)]
    with tempfile.TemporaryDirectory() as tmp:
        checkout(a.rev, old_files, os.path.join(tmp, "rev"))
        jobs = [(os.path.join(tmp, "rev"), p, a.defines, os.path.join(tmp, f"old{i}.s")) for i, p in enumerate(old_files)]
        jobs += [(build.ROOT, p, a.defines, os.path.join(tmp, f"new{i}.s")) for i, p in enumerate(new_files)]
        with ThreadPoolExecutor(min(build.MAX_COMPILES, os.cpu_count() or 1)) as pool:
            texts = list(pool.map(lambda j: assembly(*j), jobs))
    per = [(j[1], kernels(t)) for j, t in zip(jobs, texts)]
    old, new = keyed(dict(per[:len(old_files)])), keyed(dict(per[len(old_files):]))
    bad = 0
    for side, only in ((a.rev, sorted(set(old) - set(new))), ("the working tree", sorted(set(new) - set(old)))):
        for k in only:
            bad += 1
            print(f"only in {side}: {k}")
    same = 0
    for k in sorted(set(old) & set(new)):
        ref = old[k][0][1]
        copies = old[k][1:] + new[k]
        if len(old[k]) + len(new[k]) > 2:
            print(f"copies: {k}: {len(old[k])} in {a.rev} ({', '.join(p for p, _ in old[k])}), "
                  f"{len(new[k])} in the working tree ({', '.join(p for p, _ in new[k])})")
        differs = [(p, t) for p, t in copies if t != ref]
        for p, t in differs:
            x, y = ref.split("\n"), t.split("\n")
            i = next((i for i, (u, v) in enumerate(zip(x, y)) if u != v), min(len(x), len(y)))
            print(f"differs: {k} ({old[k][0][0]} | {p}) at line {i + 1} of {len(x)} | {len(y)}:\n"
                  f"    - {x[i] if i < len(x) else '<end>'}\n    + {y[i] if i < len(y) else '<end>'}")
        bad += len(differs)
        same += not differs
    print(f"{len(old)} kernels in {a.rev}, {len(new)} in the working tree ({sum(len(v) for v in new.values())} with copies): "
          f"{same} identical, {bad} missing, new or different")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
