#!/usr/bin/env python3
"""The edges of one bench step from a rocprofv3 --kernel-trace --memory-copy-trace run (CSV output): every kernel,
memset (a fill kernel) and copy from the end of the step's k_probe_table_batch to the step's last kernel, with its
start and end relative to that point, its duration and the idle gap in front of it -- the time since the latest end of
anything started before it, so work on another stream counts as busy.

usage: call_edges.py DIR [STEP]     (STEP: which k_probe_table_batch of the run opens the table; default the last)
"""
import csv
import glob
import os
import sys


def short(name):
    name = name.replace("(anonymous namespace)::", "").replace("void ", "")
    cut = name.find("(")
    return (name if cut < 0 else name[:cut])[:44]


def main():
    root = sys.argv[1]
    ev = []  # (start, end, what, stream)
    for f in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"]), r.get("Stream_Id", r.get("Queue_Id", "?"))))
    for f in glob.glob(os.path.join(root, "**", "*memory_copy_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "copy " + r.get("Direction", "?").replace("MEMORY_COPY_", ""), r.get("Stream_Id", "?")))
    ev.sort()
    opens = [i for i, e in enumerate(ev) if e[2].startswith("k_probe_table_batch")]
    if not opens:
        sys.exit("no k_probe_table_batch in the trace")
    which = int(sys.argv[2]) if len(sys.argv) > 2 else len(opens) - 1
    i0 = opens[which]
    i1 = opens[which + 1] if which + 1 < len(opens) else len(ev)
    # the step ends at its k_route_count (what follows belongs to the next step's staging or to the run's end)
    last = max((i for i in range(i0, i1) if ev[i][2].startswith("k_route_count")), default=i1 - 1)
    t0 = ev[i0][1]
    busy_until = t0
    # a builder that runs beside k_probe_table_batch may end after it
    for e in ev[:i0]:
        busy_until = max(busy_until, min(e[1], t0))
    print("%-44s %7s %9s %9s %8s %8s" % ("what", "stream", "start_us", "end_us", "dur_us", "gap_us"))
    gaps = []
    for s, e, what, st in ev[i0 + 1:last + 1]:
        gap = (s - busy_until) / 1e3
        gaps.append((gap, what))
        print("%-44s %7s %9.1f %9.1f %8.1f %8.1f" % (what, st, (s - t0) / 1e3, (e - t0) / 1e3, (e - s) / 1e3, gap))
        busy_until = max(busy_until, e)
    idle = sum(g for g, _ in gaps if g > 0)
    print("# from the table builder's end to the last kernel's end: %.1f us, device idle for %.1f us of them" % ((busy_until - t0) / 1e3, idle))
    # the yardstick: gaps between two launches behind one another on one stream -- the layout kernels, which no host wait
    # separates, and k_scan_reduce (behind pass B's last launch; since round 14 behind the host's second look where the
    # wavefront layout's rounds are not launched: that gap then is the look's)
    chain = [g for g, w in gaps if w.startswith(("k_pair_route", "k_sub_order", "k_pair_block", "k_pair_offsets", "k_items", "k_scan_reduce"))]
    if chain:
        chain.sort()
        print("# back-to-back launches on one stream (layout kernels, k_scan_reduce): gap median %.1f us, min %.1f, max %.1f (n = %d)"
              % (chain[len(chain) // 2], chain[0], chain[-1], len(chain)))


if __name__ == "__main__":
    main()
