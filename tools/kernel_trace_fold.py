#!/usr/bin/env python
"""The launches of chosen kernels in `rocprofv3 --kernel-trace --output-format csv` traces, in launch order with their grids, folded:
a launch whose name contains --group-at starts a group (a call: its weight layout, then its convolutions), and consecutive groups with
the same kernels and grids become one group whose `times` is the number of groups.  profiles/hw3_grouping_kernel_trace.txt:
  rocprofv3 --kernel-trace --output-format csv -d DIR1 -- python -m pytest tests/test_conv_gru_gpu.py::test_bits_do_not_depend_on_the_batch_grouping
  rocprofv3 --kernel-trace --output-format csv -d DIR2 -- python -m pytest tests/test_decoder_gpu.py::test_bits_do_not_depend_on_the_batch_grouping
  python tools/kernel_trace_fold.py --out profiles/hw3_grouping_kernel_trace.txt "<first test id>" DIR1 "<second test id>" DIR2
Usage: python tools/kernel_trace_fold.py [--out FILE] [--keep NAME ...] [--group-at NAME] [--counts] TITLE DIR [TITLE DIR ...]
--counts: no launch order; one row per (kernel, workgroups, threads) with the number of its launches, sorted by name -- what two
traces of the same work must agree in (profiles/conv_nodes_kernel_trace.txt; --keep "" keeps every kernel)."""
import argparse
import csv
import glob
import os
import re


def launches(trace_dir):
    """(kernel name without arguments, workgroups, threads per workgroup) of every launch under trace_dir, in start order"""
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as fh:
            for r in csv.DictReader(fh):
                grid, wg = r.get("Grid_Size_X") or r.get("Grid_Size"), r.get("Workgroup_Size_X") or r.get("Workgroup_Size")
                name = re.sub(r"\(.*", "", re.sub(r"^void ", "", r["Kernel_Name"].replace("(anonymous namespace)::", "")))
                rows.append((int(r["Start_Timestamp"]), name, int(grid) // int(wg), int(wg)))
    return [r[1:] for r in sorted(rows)]


def folded(rows, group_at):
    groups = []
    for row in rows:
        if group_at in row[0] or not groups:
            groups.append([row])
        else:
            groups[-1].append(row)
    out = []
    for g in groups:
        if out and out[-1][0] == g:
            out[-1][1] += 1
        else:
            out.append([g, 1])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--keep", nargs="+", default=["gru_conv_kernel", "decoder_conv_kernel", "hw3::"])
    ap.add_argument("--group-at", default="weight_layout_kernel")
    ap.add_argument("--counts", action="store_true")
    ap.add_argument("pairs", nargs="+", help="TITLE DIR [TITLE DIR ...]")
    args = ap.parse_args()
    lines = ["Kernel launches from `rocprofv3 --kernel-trace --output-format csv`, each trace collected in a run of its own, folded by",
             "tools/kernel_trace_fold.py: rows are in launch order; a launch of %s starts a group (one call), and consecutive" % args.group_at,
             "groups with the same kernels and grids are one group whose `times` is their number.  Kept: kernels named %s." % ", ".join(args.keep), ""]
    if args.counts:
        lines[1:3] = ["tools/kernel_trace_fold.py --counts: one row per (kernel, workgroups, threads); `times` is the number of its launches.  Kept: "
                      "%s." % ("kernels named " + ", ".join(args.keep) if all(args.keep) else "every kernel")]
    for title, d in zip(args.pairs[0::2], args.pairs[1::2]):
        rows = launches(d)
        kept = [r for r in rows if any(k in r[0] for k in args.keep)]
        lines.append("%s: %d kernel launches in the trace, %d kept" % (title, len(rows), len(kept)))
        lines.append("  %5s  %-72s %12s %10s" % ("times", "kernel", "workgroups", "threads"))
        groups = [([r], kept.count(r)) for r in sorted(set(kept))] if args.counts else folded(kept, args.group_at)
        for g, n in groups:
            for name, wgs, wg in g:
                lines.append("  %5d  %-72s %12d %10d" % (n, name, wgs, wg))
        lines.append("")
    text = "\n".join(lines).rstrip("\n") + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
