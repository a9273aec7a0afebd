#!/usr/bin/env python3
"""Registers, LDS and scratch of this tree's kernels, from their gfx950 resource blocks.  CPU only.

    tools/kernel_resources.py --only search_mfma --list 'filter_qs|filter_gemm|prepare_queries_metric' \\
        --only rescore_metric_f16 ... --no-scratch 'metric' [-o report.txt]

Every csrc/NAME.hip named with --only (default: every source) is compiled to device assembly with
build.py's CFLAGS (hipcc --cuda-device-only -S), as tools/kernel_asm_diff.py does.  Per source the
report gives the number of kernels and the maxima of .amdhsa_next_free_vgpr and
.amdhsa_private_segment_fixed_size; kernels whose demangled name matches --list are listed one per
line (vgpr, accum_offset, LDS bytes, scratch bytes).  Exit status 1 if a kernel whose demangled
name matches --no-scratch has a non-zero private segment: the guard for kernels that sit at their
register budget (the metric filter's ld-512 form holds nothing across its K loop that the cosine
form does not, and only the compiler's allocation shows whether that still suffices).
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_asm_diff as kad  # noqa: E402  (load_build, compile_asm, demangle)

FIELDS = ("next_free_vgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size")


def resources(asm: str) -> dict[str, tuple[int, ...]]:
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, re.S):
        out[m.group(1)] = tuple(int(re.search(r"\.amdhsa_" + f + r"\s+(\d+)", m.group(2)).group(1)) for f in FIELDS)
    return out


def short(name: str) -> str:
    """Demangled name without the return type, the namespace and the function arguments."""
    name = re.sub(r"^void ", "", name).replace("rc::", "")
    depth = 0
    for i, c in enumerate(name):
        depth += c == "<"
        depth -= c == ">"
        if c == "(" and depth == 0:
            return name[:i]
    return name


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--only", action="append", default=[], metavar="NAME", help="only csrc/NAME.hip (default: every source)")
    ap.add_argument("--list", default=None, metavar="REGEX", help="list the kernels whose demangled name matches")
    ap.add_argument("--no-scratch", default=None, metavar="REGEX", help="fail if a matching kernel uses scratch")
    ap.add_argument("-o", dest="report", help="also write the report to this file")
    ap.add_argument("-j", dest="jobs", type=int, default=min(8, os.cpu_count() or 4))
    args = ap.parse_args()
    tree = kad.REPO
    build = kad.load_build(tree)
    srcs = {os.path.basename(s)[:-len(".hip")]: s for s in build._sources()}
    if args.only:
        srcs = {n: s for n, s in srcs.items() if n in args.only}
    lines = [f"kernel_resources  {' '.join(sys.argv[1:])}", "(gfx950, the build's flags; vgpr = .amdhsa_next_free_vgpr, accoff = .amdhsa_accum_offset,",
             " lds = .amdhsa_group_segment_fixed_size, scratch = .amdhsa_private_segment_fixed_size, bytes)", ""]
    bad = []
    with tempfile.TemporaryDirectory(prefix="kernel_resources_") as tmp:
        with cf.ThreadPoolExecutor(max(1, args.jobs)) as ex:
            jobs = {n: ex.submit(kad.compile_asm, build, s, [], os.path.join(tmp, n + ".s")) for n, s in srcs.items()}
        for n in sorted(jobs):
            res = resources(jobs[n].result())
            pretty = kad.demangle(list(res))
            lines.append(f"{n}.hip: {len(res)} kernels, max vgpr {max(r[0] for r in res.values())}, "
                         f"max scratch {max(r[3] for r in res.values())}")
            rows = sorted((short(pretty[k]), r) for k, r in res.items())
            for name, r in rows:
                if args.list and re.search(args.list, name):
                    lines.append("  %-52s vgpr %3d  accoff %3d  lds %6d  scratch %d" % ((name,) + r))
                if args.no_scratch and re.search(args.no_scratch, name) and r[3] != 0:
                    bad.append(f"{name}: scratch {r[3]}")
    lines.append("")
    lines.append("RESULT: " + ("SCRATCH IN " + "; ".join(bad) if bad else
                               f"no kernel matching '{args.no_scratch}' uses scratch" if args.no_scratch else "listed"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.report:
        os.makedirs(os.path.dirname(os.path.abspath(args.report)), exist_ok=True)
        with open(args.report, "w") as f:
            f.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
