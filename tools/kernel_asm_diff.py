#!/usr/bin/env python3
r"""Compare the device code of two source trees, kernel by kernel.  CPU only.

    tools/kernel_asm_diff.py A B [-D MACRO ...] [-o report.txt] [--show N] [--allow-removed NAME ...]
                             [--rename REGEX=REPLACEMENT ...]

A and B are each a source tree (a directory holding the package with build.py and csrc/) or
a git revision of this repository, which is exported to a temporary directory.  Every
csrc/*.hip of both is compiled to gfx950 assembly with the tree's own build.py CFLAGS and the
unit's UNIT_FLAGS (hipcc --cuda-device-only -S), the assembly is split per kernel symbol, and each kernel is
reported as identical (same instruction stream and same .amdhsa_* block), differing, only in
A or only in B.  Exit status 0 only if every kernel of every source is identical; a kernel
deleted on purpose is named with --allow-removed (its demangled name without template and
function arguments, e.g. rc::some_kernel: every instantiation), and then may be only in A.

The comparison is a plain text diff after dropping comments and renumbering the
compiler's local labels (.LBB<function>_<block> and the long-branch .Lpost_getpc<n>: the
function number and n depend on the order in which kernels are emitted, not on their code), with
the kernel's own symbol replaced by a placeholder on both sides.

Kernels pair by demangled name.  A refactor that renames a kernel or changes its signature says so
with --rename REGEX=REPLACEMENT (repeatable; re.sub on side A's demangled names before pairing), e.g.
    --rename 'some_metric_kernel<(\S+), (\d+)>\(.*\)=some_kernel<\1, \2, true>(rc::SomeArgs)'
For a pair matched through a rule, .amdhsa_kernarg_size is reported and not counted as a difference
(the signature changed on purpose); every other .amdhsa_* line still counts.  Refactors that must
not change device code (moving kernels between headers, merging duplicated device helpers) are checked with
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
    unit = getattr(build, "UNIT_FLAGS", {}).get(os.path.basename(src), [])  # the shipped code's flags
    cmd = [build.HIPCC, *build.CFLAGS, *extra, *unit, "--cuda-device-only", "-S", src, "-o", out]
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


def parse_renames(specs: list[str]) -> list[tuple[re.Pattern, str]]:
    rules = []
    for spec in specs:
        regex, sep, repl = spec.partition("=")
        if not sep:
            sys.exit(f"--rename {spec}: expected REGEX=REPLACEMENT")
        rules.append((re.compile(regex), repl))
    return rules


KERNARG = re.compile(r"\s*\.amdhsa_kernarg_size\s+(\d+)")


def compare_kernels(ka: dict, kb: dict, pretty_a: dict[str, str], pretty_b: dict[str, str],
                    rules: list[tuple[re.Pattern, str]]) -> list[dict]:
    """Pair the kernels of one source (split_kernels' dictionaries) by demangled name, side A's
    after the rename rules, and compare each pair.  One record per name, sorted: name, status
    (identical / differing / only in A / only in B), renamed, a, b (the two sides' (instructions,
    .amdhsa) with the kernel's own symbol replaced; None where missing) and kernarg (sizes A, B)."""
    def own(sym: str, k: tuple[list[str], list[str]]):
        return tuple([ln.replace(sym, "<kernel>") for ln in part] for part in k)

    side_a = {}
    for sym in ka:
        name, n = pretty_a[sym], 0
        for regex, repl in rules:
            name, m = regex.subn(repl, name)
            n += m
        side_a[name] = (sym, n > 0)
    side_b = {pretty_b[sym]: sym for sym in kb}
    out = []
    for name in sorted(set(side_a) | set(side_b)):
        rec = {"name": name, "renamed": False, "a": None, "b": None, "kernarg": None}
        if name in side_a:
            rec["a"] = own(side_a[name][0], ka[side_a[name][0]])
            rec["renamed"] = side_a[name][1]
            if rec["renamed"]:
                rec["name"] = f"{name}  (A: {pretty_a[side_a[name][0]]})"
        if name in side_b:
            rec["b"] = own(side_b[name], kb[side_b[name]])
        if rec["a"] is None or rec["b"] is None:
            rec["status"] = "only in B" if rec["a"] is None else "only in A"
        else:
            rec["kernarg"] = tuple(next((m.group(1) for m in map(KERNARG.match, k[1]) if m), "?") for k in (rec["a"], rec["b"]))
            if rec["renamed"]:  # (the directive can sit in either part: the stream runs to the function's end label)
                rec["a"], rec["b"] = (tuple([ln for ln in part if not KERNARG.match(ln)] for part in k) for k in (rec["a"], rec["b"]))
            rec["status"] = "identical" if rec["a"] == rec["b"] else "differing"
        out.append(rec)
    return out


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
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPLACEMENT",
                    help="re.sub applied to side A's demangled kernel names before pairing (a renamed kernel, a changed signature)")
    ap.add_argument("-j", dest="jobs", type=int, default=min(8, os.cpu_count() or 4))
    args = ap.parse_args()
    rules = parse_renames(args.rename)
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
    for spec in args.rename:
        say(f"  --rename {spec}")
    total = {"identical": 0, "differing": 0, "only in A": 0, "only in B": 0}
    removed = 0  # kernels only in A that --allow-removed names
    for name in sorted(set(srcs["A"]) | set(srcs["B"])):
        ka, kb = asm.get(("A", name), {}), asm.get(("B", name), {})
        recs = compare_kernels(ka, kb, demangle(list(ka)), demangle(list(kb)), rules)
        count = {s: sum(1 for r in recs if r["status"] == s) for s in total}
        for s in total:
            total[s] += count[s]
        say()
        say(f"{name}: {len(recs)} kernels: " + ", ".join(f"{count[s]} {s}" for s in total))
        for r in recs:
            s = r["status"]
            allowed = s == "only in A" and re.split(r"[<(]", r["name"])[0].split()[-1] in args.allow_removed
            removed += allowed
            note = "  (allowed: --allow-removed)" if allowed else ""
            if r["renamed"] and r["kernarg"] and r["kernarg"][0] != r["kernarg"][1]:
                note += f"  [kernarg_size {r['kernarg'][0]} -> {r['kernarg'][1]}, not counted]"
            say(f"  {s:10s} {r['name']}{note}")
            if s == "differing":
                for part, x, y in (("instructions", r["a"][0], r["b"][0]), (".amdhsa", r["a"][1], r["b"][1])):
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
