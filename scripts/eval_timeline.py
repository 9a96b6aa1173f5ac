#!/usr/bin/env python
"""Where an evaluation's wall time goes when consecutive evaluations overlap: from the kernel trace of

    rocprofv3 --kernel-trace --output-format csv -d <dir> -o run -- python bench.py --steps 100 --warmup 5

(the default two evaluation streams; no counters, no other tracing), per evaluation: the time
during which an 8-bit sweep runs (whatever runs beside it is hidden), the time during which only
other kernels run, by kernel, and the time during which nothing runs.

usage: scripts/eval_timeline.py <run_kernel_trace.csv> [--steps 100]

The timed steps are found in the trace itself: an evaluation starts with one k_eval_prep launch, and
the timed steps are the longest run of k_eval_prep launches that follow each other at a steady
period (gaps under three times the median gap). The window is the last --steps periods of that
run, from one k_eval_prep launch to the run's last one, so it holds whole periods whichever way
the streams interleave. Instants at which several other
kernels run (and no 8-bit sweep) are split evenly among them, so the columns sum to the period."""
import argparse
import csv
import re
import statistics
from collections import defaultdict


def short(name):
    """mmre::k_sweep_valu<6, false, false, 0, 1, 8>(args) -> k_sweep_valu<6, false, false, 0, 1, 8>"""
    n = re.sub(r"^void\s+", "", name.strip())
    depth, cut = 0, len(n)
    for i, ch in enumerate(n):  # the argument list: the first '(' outside the template arguments
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            cut = i
            break
    n = n[:cut]
    return n.split("::")[-1] if "<" not in n else re.sub(r"^(\w+::)+", "", n)


def is_sweep8(name):
    return re.search(r"k_sweep_valu<6,|k_sweep_valuILi6E", name) is not None


def load(path):
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    ks = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in rows]
    ks.sort()
    return ks


def timed_window(ks, steps):
    preps = [s for s, _, n in ks if "k_eval_prep" in n]
    if len(preps) < 3:
        raise SystemExit("eval_timeline: fewer than three k_eval_prep launches in the trace")
    gaps = [b - a for a, b in zip(preps, preps[1:])]
    med = statistics.median(gaps)
    best, cur = (0, 0), 0  # (length, first index) of the longest steady run of launches
    for i, g in enumerate(gaps):
        if g >= 3 * med:
            cur = i + 1
        elif i + 2 - cur > best[0]:
            best = (i + 2 - cur, cur)
    n, first = best
    last = first + n - 1  # index of the run's last launch: the window's end (its evaluation runs out alone)
    use = min(steps, n - 1)
    return preps[last - use], preps[last], use, n


def timeline(ks, t0, t1):
    ev = []
    for s, e, n in ks:
        s, e = max(s, t0), min(e, t1)
        if s < e:
            ev.append((s, 1, n))
            ev.append((e, -1, n))
    ev.sort(key=lambda x: (x[0], x[1]))
    active = defaultdict(int)
    sweep = idle = 0.0
    other = defaultdict(float)
    t = t0
    for at, d, n in ev + [(t1, 0, "")]:
        dt = at - t
        if dt > 0:
            names = [k for k, c in active.items() if c > 0]
            if any(is_sweep8(k) for k in names):
                sweep += dt
            elif names:
                for k in names:
                    other[short(k)] += dt / len(names)
            else:
                idle += dt
        t = at
        if d:
            active[n] += d
    return sweep, other, idle


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("csv")
    ap.add_argument("--steps", type=int, default=100)
    a = ap.parse_args()
    ks = load(a.csv)
    t0, t1, n, run = timed_window(ks, a.steps)
    sweep, other, idle = timeline(ks, t0, t1)
    us = lambda x: x / n / 1e3
    print(f"{n} evaluations of a steady run of {run} ({a.csv}); us per evaluation")
    print(f"{'period':58s} {us(t1 - t0):9.1f}")
    print(f"{'an 8-bit sweep running':58s} {us(sweep):9.1f}")
    print(f"{'only other kernels running':58s} {us(sum(other.values())):9.1f}")
    for k, v in sorted(other.items(), key=lambda kv: -kv[1]):
        print(f"    {k[:54]:54s} {us(v):9.1f}")
    print(f"{'idle':58s} {us(idle):9.1f}")
    dur = defaultdict(list)
    for s, e, k in ks:
        if t0 <= s < t1:
            dur[short(k)].append(e - s)
    print("kernels launched in the window: launches per evaluation, average us each")
    for k, v in sorted(dur.items(), key=lambda kv: -sum(kv[1])):
        print(f"    {k[:54]:54s} {len(v) / n:6.2f} {sum(v) / len(v) / 1e3:9.1f}")


if __name__ == "__main__":
    main()
