"""Row-tile changes of the grouped sweep's claim rules, counted on the CPU from the rules alone
(csrc/link_valu.hip: sweep_valu_body's claim_affine and the sequential counter). One XCD group of C2:
128 workgroups, 103 row tiles of 13 or 14 units (13 main entity tiles + the group's share of the
7 leftover tiles' units). A unit costs 1 (the lightest row tile) to `heavy` (the first), +-10 %;
a row-tile change is a unit whose row tile differs from the workgroup's previous one (the flush /
reload branch of the epilogue). usage: python scripts/sim_affine_claims.py [heavy]"""
import heapq
import sys

import numpy as np

P, NQT, M, R, G = 128, 103, 13, 7, 8


def units(g):
    lo0, lo1 = NQT * R * g // G, NQT * R * (g + 1) // G
    return [M + max(0, min(lo1, (t + 1) * R) - max(lo0, t * R)) for t in range(NQT)]


def run(share, heavy, seed=0, g=3):
    """share = 0: the sequential counter; else claim_affine with `share` workgroups per first tile."""
    rng = np.random.default_rng(seed)
    n = units(g)
    order = [t for t in range(NQT) for _ in range(n[t])]  # the sequential counter's unit order
    taken, hint, seq = [0] * NQT, 0, P
    cost = lambda t: (1.0 + (heavy - 1.0) * (1.0 - t / (NQT - 1))) * rng.uniform(0.9, 1.1)

    def claim(t):
        nonlocal hint, seq
        if share == 0:
            seq += 1
            return order[seq - 1] if seq - 1 < len(order) else None
        hinted = False
        while True:
            if taken[t] < n[t]:
                taken[t] += 1
                return t
            if hinted:
                hint = max(hint, t + 1)
            hinted = True
            if hint >= NQT:
                return None
            t = hint

    heap, changes, done = [], 0, 0.0
    for w in range(P):
        t = order[w] if share == 0 else claim((w // share) % NQT)
        if t is not None:
            changes += 1
            heapq.heappush(heap, (cost(t), w, t))
    while heap:
        now, w, t = heapq.heappop(heap)
        done = now
        nt = claim(t)
        if nt is not None:
            changes += nt != t
            heapq.heappush(heap, (now + cost(nt), w, nt))
    return changes, done


if __name__ == "__main__":
    heavy = float(sys.argv[1]) if len(sys.argv) > 1 else 2.0
    total = sum(units(3))
    print(f"one XCD group: {total} units, {P} workgroups, unit cost 1 .. {heavy}")
    for share in (0, 1, 2, 3, 4, 6, 8, 13):
        c, d = run(share, heavy)
        name = "sequential" if share == 0 else f"affine, {share} per first tile"
        print(f"{name:28s} row-tile changes {c:5d} ({8 * c:6d} per evaluation)  makespan {d:6.2f}")
