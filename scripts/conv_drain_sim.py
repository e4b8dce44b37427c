#!/usr/bin/env python3
"""How a launch of k_conv3x3_sg drains: a list-scheduling MODEL of the workgroup order (no GPU; plain Python).

THIS IS A MODEL, NOT A MEASUREMENT.  The measurement is profiles/conv_drain_timeline.txt (scripts/stamp_conv.py --drain on the
-DTG_CONV_STAMP build); DESIGN.md 8.12 sets the two side by side.

The machine of the model: 8 XCDs x 32 CUs x `--slots` workgroup slots.  Workgroup b of the grid belongs to XCD b % 8, and every XCD
dispatches its list in order: whenever a slot is free, the next workgroup goes to the CU with the fewest resident workgroups.  The
CUs are processor-sharing servers; a workgroup is a job of F/16 x taps stage-times (72 / 48 / 32 at F = 128) plus `--fixed`.
  pipe model A: a resident workgroup always advances at 1 / slots of a CU, however many neighbours it has;
  pipe model B: a CU with n resident workgroups advances at min(1, 0.4 n) in all, shared equally (one workgroup alone cannot
                saturate the matrix pipe, three can).
The figure printed is balanced makespan / makespan: total work / (256 CUs at full rate) over the end of the last XCD, 1.0 = no drain.

Orders:
  today   range-major over the whole grid, XCD x takes the contiguous run [x * tpx, (x + 1) * tpx), inside a range conv_pos_of order
          (interior, edge, corner positions);
  drain   conv_rows.h conv_launch_wg: per XCD its whole ranges range-major but for the last K, which are spent class-major together
          with the XCD's share of the nrange % 8 leftover ranges (all interior positions, then all edges, then all corners).

    python3 scripts/conv_drain_sim.py [--S 9] [--F 128] [--rows 15700 ...] [--slots 4] [--pipe A|B] [--order today|drain|both] [--K 1 2 4]
"""
import argparse


def classes(S):
    I = S - 2
    return [(I * I, 9), (4 * I, 6), (4, 4)]                  # (positions, taps) of the interior, edge and corner class


def order_today(nrange, S):
    """Per-XCD lists of (range, class)."""
    P = S * S
    cl = classes(S)
    per_range = [c for c, (n, _) in enumerate(cl) for _ in range(n)]
    total = nrange * P
    tpx = ((total + 7) // 8 * 8) // 8
    lists = []
    for x in range(8):
        lists.append([(b // P, per_range[b % P]) for b in range(x * tpx, min((x + 1) * tpx, total))])
    return lists


def order_drain(nrange, S, K):
    """conv_launch_wg of conv_rows.h, written from its description (tests/test_conv_launch_order.py checks the header itself)."""
    cl = classes(S)
    q, m = divmod(nrange, 8)
    kd = min(K, q)
    lists = [[] for _ in range(8)]
    for x in range(8):
        for r in range(x * q, x * q + q - kd):
            lists[x] += [(r, c) for c, (n, _) in enumerate(cl) for _ in range(n)]
    g = 0                                                      # class-major number of the leftover workgroups
    for c, (n, _) in enumerate(cl):
        for x in range(8):
            for r in range(x * q + q - kd, x * q + q):
                lists[x] += [(r, c)] * n
        for r in range(8 * q, nrange):
            for _ in range(n):
                lists[g % 8].append((r, c))
                g += 1
    return lists


def xcd_end(jobs, cus, slots, pipe):
    """End time of one XCD that dispatches `jobs` (work per job) in order."""
    res = [[] for _ in range(cus)]                             # remaining work of the resident workgroups, per CU
    nxt, t = 0, 0.0

    def rate(n):                                               # per workgroup
        return 1.0 / slots if pipe == "A" else min(1.0, 0.4 * n) / n

    while True:
        while nxt < len(jobs):                                 # in-order dispatch to the least-loaded CU with a free slot
            cu = min(range(cus), key=lambda i: len(res[i]))
            if len(res[cu]) >= slots:
                break
            res[cu].append(jobs[nxt])
            nxt += 1
        dt = min((min(r) / rate(len(r)) for r in res if r), default=None)
        if dt is None:
            return t
        t += dt
        for r in res:
            if r:
                adv = dt * rate(len(r))
                r[:] = [w - adv for w in r if w - adv > 1e-9]


def makespan_ratio(lists, S, F, slots, pipe, fixed, cus=32):
    work = [F // 16 * taps + fixed for _, taps in classes(S)]
    total = sum(work[c] for l in lists for _, c in l)
    balanced = total / (8 * cus)                               # a full CU advances one stage-time per unit of time in both models
    end = max(xcd_end([work[c] for _, c in l], cus, slots, pipe) for l in lists)
    return balanced / end


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--S", type=int, default=9)
    ap.add_argument("--F", type=int, default=128)
    ap.add_argument("--rows", type=int, nargs="+", default=[14000, 15000, 15700, 16000, 16384], help="boards of the launch")
    ap.add_argument("--slots", type=int, default=None, help="workgroups per CU (default 4 at F = 128, 2 at F = 256)")
    ap.add_argument("--pipe", choices=["A", "B", "both"], default="both")
    ap.add_argument("--order", choices=["today", "drain", "both"], default="both")
    ap.add_argument("--K", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--fixed", type=float, default=0.0, help="fixed part of a workgroup, in stage-times")
    a = ap.parse_args()
    slots = a.slots or (4 if a.F == 128 else 2)
    print(f"MODEL (not a measurement): S {a.S}, F {a.F}, {slots} workgroups per CU, fixed part {a.fixed} stage-times; "
          f"balanced makespan / makespan")
    for pipe in (["A", "B"] if a.pipe == "both" else [a.pipe]):
        for rows in a.rows:
            nrange = (rows + 127) // 128
            cols = []
            if a.order in ("today", "both"):
                cols.append(("today", makespan_ratio(order_today(nrange, a.S), a.S, a.F, slots, pipe, a.fixed)))
            if a.order in ("drain", "both"):
                for K in a.K:
                    cols.append((f"drain K={K}", makespan_ratio(order_drain(nrange, a.S, K), a.S, a.F, slots, pipe, a.fixed)))
            print(f"pipe {pipe}  rows {rows:6d}  ranges {nrange:4d}  " + "  ".join(f"{n} {v:.4f}" for n, v in cols))


if __name__ == "__main__":
    main()
