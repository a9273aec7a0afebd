#!/usr/bin/env python3
"""Compare the device code of two source trees, kernel by kernel.  CPU only.

    tools/kernel_asm_diff.py A B [-D MACRO ...] [-o report.txt] [--show N] [--allow-removed NAME ...]

A and B are each a source tree (a directory holding the package with build.py and csrc/) or
a git revision of this repository, which is exported to a temporary directory.  Every
csrc/*.hip of both is compiled to gfx950 assembly with the tree's own build.py CFLAGS
(hipcc --cuda-device-only -S), the assembly is split per kernel symbol, and each kernel is
reported as identical (same instruction stream and same .amdhsa_* block), differing, only in
A or only in B.  Exit status 0 only if every kernel of every source is identical; a kernel
deleted on purpose is named with --allow-removed (its demangled name without template and
function arguments, e.g. rc::some_kernel: every instantiation), and then may be only in A.

The comparison is a plain text diff after dropping comments and renumbering the
compiler's local labels (.LBB<function>_<block> and the long-branch .Lpost_getpc<n>: the
function number and n depend on the order in which kernels are emitted, not on their code).  Refactors that must not change device
code (moving kernels between headers, merging duplicated device helpers) are checked with
    tools/kernel_asm_diff.py <parent revision> .
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import difflib
import glob
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def export_revision(rev: str, dst: str) -> None:
    ar = subprocess.run(["git", "-C", REPO, "archive", "--format=tar", rev], capture_output=True)
    if ar.returncode != 0:
        sys.exit(f"{rev}: neither a directory nor a revision: {ar.stderr.decode().strip()}")
    subprocess.run(["tar", "-x", "-C", dst], input=ar.stdout, check=True)


def load_build(tree: str):
    """The tree's build.py as a module (its CFLAGS carry the tree's own include paths)."""
    found = [p for p in glob.glob(os.path.join(tree, "*", "build.py")) if os.path.isdir(os.path.join(os.path.dirname(p), "csrc"))]
    if len(found) != 1:
        sys.exit(f"{tree}: expected one package with build.py and csrc/, found {len(found)}")
    spec = importlib.util.spec_from_file_location(f"_build_{abs(hash(tree))}", found[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_asm(build, src: str, extra: list[str], out: str) -> str:
    cmd = [build.HIPCC, *build.CFLAGS, *extra, "--cuda-device-only", "-S", src, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
    return open(out).read()


LOCAL_LABEL = re.compile(r"\.L(BB|func_begin|func_end|tmp|post_getpc)(\d+)")


def normalise(lines: list[str]) -> list[str]:
    out = []
    for ln in lines:
        ln = ln.split(";", 1)[0].rstrip()
        if not ln.strip():
            continue
        out.append(LOCAL_LABEL.sub(lambda m: ".L" + m.group(1), ln))
    return out


def split_kernels(asm: str) -> dict[str, tuple[list[str], list[str]]]:
    """kernel symbol -> (instruction stream, .amdhsa_* block), both normalised."""
    lines = asm.splitlines()
    desc: dict[str, list[str]] = {}
    i = 0
    while i < len(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[i])
        if m:
            j = i + 1
            while not lines[j].strip().startswith(".end_amdhsa_kernel"):
                j += 1
            desc[m.group(1)] = normalise(lines[i + 1:j])
            i = j
        i += 1
    body: dict[str, list[str]] = {}
    for i, ln in enumerate(lines):
        m = re.match(r"(\S+):", ln)
        if not m or m.group(1) not in desc or m.group(1) in body:
            continue
        j = i + 1
        while j < len(lines) and not re.match(r"\.Lfunc_end\d+:", lines[j]):
            j += 1
        body[m.group(1)] = normalise(lines[i + 1:j])
    missing = sorted(set(desc) - set(body))
    if missing:
        raise RuntimeError(f"kernel descriptors without a body: {missing}")
    return {k: (body[k], desc[k]) for k in desc}


def demangle(names: list[str]) -> dict[str, str]:
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    if not names or not os.path.exists(filt):
        return {n: n for n in names}
    r = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True)
    out = r.stdout.splitlines()
    return dict(zip(names, out)) if r.returncode == 0 and len(out) == len(names) else {n: n for n in names}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("a", help="tree or git revision A")
    ap.add_argument("b", help="tree or git revision B")
    ap.add_argument("-D", dest="defines", action="append", default=[], help="extra macro for both builds")
    ap.add_argument("-o", dest="report", help="also write the report to this file")
    ap.add_argument("--show", type=int, default=40, help="diff lines shown per differing kernel")
    ap.add_argument("--only", action="append", default=[], metavar="NAME", help="only csrc/NAME.hip (default: every source)")
    ap.add_argument("--keep", metavar="DIR", help="keep the assembly files (A_<source>.s, B_<source>.s) in DIR")
    ap.add_argument("--allow-removed", action="append", default=[], metavar="NAME",
                    help="a kernel that may be only in A (demangled name without template / function arguments)")
    ap.add_argument("-j", dest="jobs", type=int, default=min(8, os.cpu_count() or 4))
    args = ap.parse_args()
    extra = ["-D" + d for d in args.defines]

    report: list[str] = []

    def say(s: str = "") -> None:
        print(s, flush=True)
        report.append(s)

    with tempfile.TemporaryDirectory(prefix="kernel_asm_diff_") as tmp:
        trees = {}
        for side, arg in (("A", args.a), ("B", args.b)):
            if os.path.isdir(arg):
                trees[side] = os.path.abspath(arg)
            else:
                trees[side] = os.path.join(tmp, "tree_" + side)
                os.makedirs(trees[side])
                export_revision(arg, trees[side])
        builds = {side: load_build(t) for side, t in trees.items()}
        srcs = {side: {os.path.basename(s): s for s in b._sources()} for side, b in builds.items()}
        if args.only:
            srcs = {side: {n: s for n, s in d.items() if n[:-len(".hip")] in args.only} for side, d in srcs.items()}
        jobs = {}
        with cf.ThreadPoolExecutor(max(1, args.jobs)) as ex:
            for side in ("A", "B"):
                for name, src in srcs[side].items():
                    out = os.path.join(tmp, f"{side}_{name}.s")
                    jobs[side, name] = ex.submit(compile_asm, builds[side], src, extra, out)
        asm = {k: split_kernels(f.result()) for k, f in jobs.items()}
        if args.keep:
            os.makedirs(args.keep, exist_ok=True)
            for f in glob.glob(os.path.join(tmp, "*.s")):
                shutil.copy(f, args.keep)

    say(f"kernel_asm_diff  A = {args.a}  B = {args.b}  flags: {' '.join(extra) or '(product build)'}")
    total = {"identical": 0, "differing": 0, "only in A": 0, "only in B": 0}
    removed = 0  # kernels only in A that --allow-removed names
    for name in sorted(set(srcs["A"]) | set(srcs["B"])):
        ka, kb = asm.get(("A", name), {}), asm.get(("B", name), {})
        status = {}
        for k in sorted(set(ka) | set(kb)):
            status[k] = "only in B" if k not in ka else "only in A" if k not in kb else "identical" if ka[k] == kb[k] else "differing"
        count = {s: sum(1 for v in status.values() if v == s) for s in total}
        for s in total:
            total[s] += count[s]
        say()
        say(f"{name}: {len(status)} kernels: " + ", ".join(f"{count[s]} {s}" for s in total))
        pretty = demangle(list(status))
        for k, s in status.items():
            allowed = s == "only in A" and re.split(r"[<(]", pretty[k])[0].split()[-1] in args.allow_removed
            removed += allowed
            say(f"  {s:10s} {pretty[k]}" + ("  (allowed: --allow-removed)" if allowed else ""))
            if s == "differing":
                for part, x, y in (("instructions", ka[k][0], kb[k][0]), (".amdhsa", ka[k][1], kb[k][1])):
                    d = list(difflib.unified_diff(x, y, "A", "B", lineterm="", n=1))
                    for ln in d[:args.show]:
                        say(f"      {part}: {ln}")
                    if len(d) > args.show:
                        say(f"      {part}: ... {len(d) - args.show} more diff lines")
    say()
    say("total: " + ", ".join(f"{total[s]} {s}" for s in total))
    ok = total["differing"] == 0 and total["only in A"] == removed and total["only in B"] == 0
    say("RESULT: " + ("DEVICE CODE DIFFERS" if not ok else
                      f"device code identical, {removed} kernel(s) removed as allowed" if removed else "device code identical"))
    if args.report:
        os.makedirs(os.path.dirname(os.path.abspath(args.report)), exist_ok=True)
        with open(args.report, "w") as f:
            f.write("\n".join(report) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
