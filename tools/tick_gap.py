#!/usr/bin/env python3
"""Where a tick's time goes between two QP launches, from a kernel trace (rocprofv3 --kernel-trace, CSV).

For every pair of consecutive `usv_qp_rti` launches (tick t, tick t + 1) it prints
  gap      start of the QP launch of tick t + 1 - end of the QP launch of tick t: the time the device is not running the QP
  overrun  how long the speculative lineariser (usv_linearize<..., 1> or <..., 3>, started beside the QP launch of tick t) runs past that launch's end
  fixup    the fix-up lineariser (usv_linearize<..., 2> or <..., 4>) inside the gap
  full     a whole-batch lineariser (usv_linearize<..., 0>) inside the gap (ticks that were not pipelined)
  sort     usv_sort_hist + usv_sort_scan + usv_sort_scatter inside the gap
  advance  usv_advance inside the gap
and the medians over the ticks after the first `--skip` (default 2: the pipeline is not running yet), `overrun` over every speculative
launch in the trace.

    python tools/tick_gap.py profiles/r06_g_kernel_trace.csv
"""
import argparse
import csv
import json
import re
import statistics
import sys


def read_trace(path):
    """[(name, start_ns, end_ns)] sorted by start; accepts the column names of rocprofv3's kernel trace in either of its layouts."""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name") or r.get("Name")
            if name is None:
                continue
            rows.append((name, int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows.sort(key=lambda r: r[1])
    return rows


_LIN = re.compile(r"usv_linearize<.*,\s*(\d)>\(")


def lin_mode(name):
    """0 whole batch, 1 speculative (kernel MODE 1 or 3), 2 fix-up (MODE 2 or 4); None: not the lineariser"""
    m = _LIN.search(name)
    return {0: 0, 1: 1, 2: 2, 3: 1, 4: 2}.get(int(m.group(1))) if m else None


def ticks(rows):
    """One record per pair of consecutive QP launches; times in ms."""
    qp = [r for r in rows if "usv_qp_rti<" in r[0]]
    out = []
    big = max((r[2] for r in rows), default=0) + 1
    for i, (_, s0, e0) in enumerate(qp):
        last = i + 1 == len(qp)  # (no gap behind the last launch; the speculative lineariser beside it is still in the trace)
        s1 = big if last else qp[i + 1][1]
        rec = {"qp_ms": (e0 - s0) * 1e-6, "gap": None if last else (s1 - e0) * 1e-6, "overrun": None, "fixup": 0.0, "full": 0.0, "sort": 0.0, "advance": 0.0}
        spec = None
        for name, s, e in rows:
            if e <= s0 or s >= s1:
                continue
            mode = lin_mode(name)
            if mode == 1:
                # The one enqueued beside the launch of tick t: the QP launch of tick t + 1 waits for it, so it ends before s1 (the first such
                # in start order: the one made for tick t + 2 may come onto the device inside the gap, and ends after s1).
                if e <= s1 and spec is None:
                    spec = (s, e)
                continue
            if s < e0 or last:
                continue
            d = (e - s) * 1e-6
            if mode == 2:
                rec["fixup"] += d
            elif mode == 0:
                rec["full"] += d
            elif "usv_sort_" in name:
                rec["sort"] += d
            elif "usv_advance" in name:
                rec["advance"] += d
        if spec is not None:
            rec["overrun"] = max((spec[1] - e0) * 1e-6, 0.0)
        out.append(rec)
    return out


KEYS = ("qp_ms", "gap", "overrun", "fixup", "full", "sort", "advance")


def summary(recs, skip=2):
    """Medians over the ticks after the first `skip` that have a following QP launch; `overrun` over every speculative launch of the trace
    (the ticks left out of the other medians are those before the pipeline runs: they have none, or the first one)."""
    tail = [r for r in recs[skip:] if r["gap"] is not None]
    if not tail:
        return {}
    s = {"ticks": len(tail)}
    for k in KEYS:
        v = [r[k] for r in (recs if k == "overrun" else tail) if r[k] is not None]
        if v:
            s[k] = {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}
    return s


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("trace", help="kernel trace CSV")
    ap.add_argument("--skip", type=int, default=2, help="ticks left out of the medians (default 2)")
    ap.add_argument("--json", action="store_true", help="print the summary as one JSON line instead of the table")
    a = ap.parse_args(argv)
    recs = ticks(read_trace(a.trace))
    s = summary(recs, a.skip)
    if a.json:
        print(json.dumps(s))
        return 0
    print("tick " + " ".join("%8s" % k for k in KEYS) + "   (ms)")
    for i, r in enumerate(recs):
        print("%4d " % i + " ".join("%8s" % "-" if r[k] is None else "%8.3f" % r[k] for k in KEYS) +
              ("   (not in the medians but overrun's)" if i < a.skip or r["gap"] is None else ""))
    if s:
        print("median over %d ticks (min - max):" % s["ticks"])
        for k in KEYS:
            if k in s:
                print("  %-8s %8.3f  (%.3f - %.3f)  n = %d" % (k, s[k]["median"], s[k]["min"], s[k]["max"], s[k]["n"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
