#!/usr/bin/env python3
"""The early kernels of overlapped flushes against k_combined, from a rocprofv3 kernel trace of
bench.py (plain run): each early kernel's duration and whether it started inside a k_combined run,
the early stream's busy time per tick and the main stream's idle time per tick.

    python tools/early_trace.py run_kernel_trace.csv [label]

The main queue is k_combined's; an overlapped flush is one whose apply ran on another queue.  A tick
runs from one overlapped apply's start to the next one's (early busy) and from one k_combined's start
to the next one's (main idle).  The first two overlapped ticks and the last one are left out.
"""
import bisect
import csv
import re
import statistics
import sys

EARLY = ("k_moves_apply_n", "k_keygen", "k_scan64", "k_arrive_special", "k_arrive", "k_merge_gather")


def short(n):
    m = re.search(r"(k_[a-z_0-9]+(?:<[^>]*>)?|__amd_[a-zA-Z_]+)", n)
    return m.group(1) if m else n[:30]


def med(v):
    return statistics.median(v) if v else float("nan")


def main():
    rows = [(short(r["Kernel_Name"]), r["Queue_Id"], int(r["Start_Timestamp"]), int(r["End_Timestamp"]))
            for r in csv.DictReader(open(sys.argv[1]))]
    rows.sort(key=lambda r: r[2])
    label = sys.argv[2] if len(sys.argv) > 2 else ""
    comb = [r for r in rows if r[0] == "k_combined"]
    if not comb:
        sys.exit("no k_combined in the trace")
    main_q = statistics.mode(r[1] for r in comb)
    applies = [r for r in rows if r[0].startswith("k_moves_apply_n") and r[1] != main_q]
    if len(applies) < 5:
        sys.exit("fewer than 5 overlapped flushes in the trace")
    early_q = statistics.mode(r[1] for r in applies)
    marks = [r[2] for r in applies][2:]  # tick boundaries: overlapped apply starts
    t_lo, t_hi = marks[0], marks[-1]
    cs, ce = [r[2] for r in comb], [r[3] for r in comb]

    def in_combined(t):  # index of the k_combined run holding time t, or -1
        i = bisect.bisect_right(cs, t) - 1
        return i if i >= 0 and t < ce[i] else -1

    def share(s, e):  # part of [s, e) that lies inside k_combined runs
        tot = 0
        for a, b in zip(cs, ce):
            tot += max(0, min(e, b) - max(s, a))
        return tot / max(1, e - s)

    us = lambda ns: ns / 1e3
    print(f"# {label}: early kernels of overlapped flushes against k_combined; {len(marks) - 1} ticks; "
          f"main queue {main_q}, early queue {early_q}; times in us")
    print("# per kernel instance: tick, kernel, start (from the tick's apply), dur, started inside a k_combined run, "
          "share of its run inside k_combined, offset of its start into that k_combined run")
    per = {}
    for r in rows:
        k, q, s, e = r
        if q != early_q or not (t_lo <= s < t_hi) or not k.startswith(EARLY):
            continue
        tick = bisect.bisect_right(marks, s) - 1
        ci = in_combined(s)
        sh = share(s, e)
        off = f"{us(s - cs[ci]):6.1f}/{us(ce[ci] - cs[ci]):5.1f}" if ci >= 0 else "     -"
        print(f"{tick:3d} {k[:30]:30s} start {us(s - marks[tick]):7.1f} dur {us(e - s):6.1f}  "
              f"{'inside ' if ci >= 0 else 'outside'} share {sh:4.2f}  at {off}")
        per.setdefault(k, {"in": [], "out": [], "full": [], "none": []})
        per[k]["in" if ci >= 0 else "out"].append(us(e - s))
        if sh >= 0.9:
            per[k]["full"].append(us(e - s))
        if sh <= 0.1:
            per[k]["none"].append(us(e - s))
    print("# medians (count): started inside / outside a k_combined run; >= 90 % / <= 10 % of its run inside k_combined")
    for k, d in per.items():
        print(f"   {k[:30]:30s} inside {med(d['in']):6.1f} ({len(d['in']):2d})  outside {med(d['out']):6.1f} ({len(d['out']):2d})"
              f"   >=90% {med(d['full']):6.1f} ({len(d['full']):2d})  <=10% {med(d['none']):6.1f} ({len(d['none']):2d})"
              f"   inside/outside {med(d['in']) / med(d['out']) if d['in'] and d['out'] else float('nan'):4.2f}")
    busy, span = [], []
    for a, b in zip(marks, marks[1:]):
        busy.append(us(sum(r[3] - r[2] for r in rows if r[1] == early_q and a <= r[2] < b)))
        span.append(us(b - a))
    idle, cdur = [], []
    for a, b in zip(cs, cs[1:]):
        if not (t_lo <= a < t_hi):
            continue
        work = sum(min(r[3], b) - r[2] for r in rows if r[1] == main_q and a <= r[2] < b)
        idle.append(us((b - a) - work))
        cdur.append(us(ce[cs.index(a)] - a))
    print("# per tick: tick span, early stream busy, main stream idle (k_combined start to the next one's, less "
          "the main queue's kernels), k_combined dur")
    for i, (sp, bu) in enumerate(zip(span, busy)):
        print(f"{i:3d} span {sp:6.1f} early busy {bu:6.1f}  main idle {idle[i] if i < len(idle) else float('nan'):6.1f}"
              f"  k_combined {cdur[i] if i < len(cdur) else float('nan'):6.1f}")
    print(f"# medians: tick span {med(span):.1f}, early stream busy {med(busy):.1f} (min {min(busy):.1f}, max {max(busy):.1f}), "
          f"main stream idle {med(idle):.1f} (min {min(idle):.1f}, max {max(idle):.1f}), k_combined {med(cdur):.1f}")


if __name__ == "__main__":
    main()
