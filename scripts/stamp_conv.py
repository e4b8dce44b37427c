"""Where a workgroup of k_conv3x3_sg<9,128> spends its time outside the walk, from in-kernel cycle-counter stamps (diagnostic build:
net.hip with -DTG_CONV_STAMP, `scripts/build_variant.sh cstamp net.hip -DTG_CONV_STAMP`, copied over transgo_amd/libtransgo_hip.so on
the GPU box; the shipped library has no stamp).  `python scripts/stamp_conv.py [rows blocks]`: forwards of a 9x9 / F = 128 tower as
scripts/time_net.py runs them; the stamps are those of lane 0 of wave 0 of six workgroups of XCD 0 in the last conv1 launch and the
last stream-to-stream conv2 launch: the first interior, edge and corner position of board range 0 (first round) and of range 7 (the
middle of the XCD's run).  Read the SHARES: the stamps fence the scheduler, the build is slower than the product.
`python scripts/stamp_conv.py --drain [rows blocks]`: how the same two launches DRAIN, from the record that lane 0 of
wave 0 of EVERY workgroup leaves in that build: entry and end (its last store issued) on the cycle counter and on the device-wide
100 MHz clock, its (range, p), the XCD and the CU it ran on."""
import ctypes, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transgo_amd import _lib
from transgo_amd.model import HipNetwork, random_weights

DRAIN = "--drain" in sys.argv
if DRAIN:
    sys.argv.remove("--drain")
B = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
NB = int(sys.argv[2]) if len(sys.argv) > 2 else 6


def drain_records(epi):
    cap = 16384
    fn = _lib.load().tg_debug_conv_drain
    fn.restype = ctypes.c_int; fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    raw = (ctypes.c_ulonglong * (cap * 6))()
    assert fn(raw, epi, cap) == 0
    return np.frombuffer(raw, dtype=np.uint64).reshape(cap, 6).copy()


def drain_table(r, kern):
    """One launch, seen from its workgroups.  Times on the 100 MHz clock (10 ns a tick; one clock for the whole device, so the XCDs can
    be set against each other); the cycle counter is printed beside it for the lifetimes."""
    grid = ((B + 127) // 128 * 81 + 7) // 8 * 8
    r = r[:grid]
    assert (r[:, 2] != 0).all(), "a workgroup of the grid left no record"
    live = r[:, 4] != np.uint64(0xffffffffffffffff)
    b = np.arange(grid)[live]
    t0 = r[live, 2].astype(np.int64); t1 = r[live, 3].astype(np.int64)
    c0 = r[live, 0].astype(np.int64); c1 = r[live, 1].astype(np.int64)
    rng = (r[live, 4] >> np.uint64(32)).astype(np.int64); p = (r[live, 4] & np.uint64(0xffffffff)).astype(np.int64)
    xcc = (r[live, 5] >> np.uint64(32)).astype(np.int64) & 15; cu = (r[live, 5] >> np.uint64(8)).astype(np.int64) & 255
    y, x = p // 9, p % 9
    nt = np.where((y % 8 == 0) & (x % 8 == 0), 4, np.where((y % 8 == 0) | (x % 8 == 0), 6, 9))
    start = t0.min(); t0 -= start; t1 -= start
    dur = t1.max()
    us = lambda v: v / 100.0
    print(f"== {kern}: {live.sum()} workgroups of a grid of {grid}, {len(np.unique(rng))} ranges; launch (first entry -> last end) {us(dur):.1f} us")
    print("   hardware XCC_ID of the workgroups b with b % 8 = 0..7 (one value each: the lists are the XCDs' own): "
          + " ".join("/".join(str(v) for v in np.unique(xcc[b % 8 == k])) for k in range(8))
          + f"; CUs seen per XCD: {[len(np.unique(cu[xcc == k])) for k in range(8)]}.  The tables below go by XCC_ID.")
    life = t1 - t0
    print("   lifetime, us (mean) by walk: " + ", ".join(f"{n} taps {us(life[nt == n].mean()):.1f} (cycle counter {np.mean((c1 - c0)[nt == n]):.0f} ticks, n {np.sum(nt == n)})" for n in (9, 6, 4)))
    slots = 8 * 32 * 4
    print(f"   drain = 1 - sum(lifetimes) / ({slots} x launch) = {1 - life.sum() / (slots * dur):.4f}")
    inv = []
    for k in range(8):
        m = b % 8 == k
        e = t0[m][np.argsort(b[m])]
        inv.append(float(np.mean(np.diff(e) < 0)))
    print("   dispatch in blockIdx order per XCD: share of neighbours (b, b + 8) that entered in the opposite order: " + " ".join(f"{v:.3f}" for v in inv))
    print("   XCD   first entry  last entry  end (us)   <4/CU   <3/CU   <2/CU (us below that many resident workgroups per CU on average, after the XCD's first fill)   last 3 workgroups (range, p, taps, end us)")
    ends = []
    for k in range(8):
        m = xcc == k
        ev = np.concatenate([np.stack([t0[m], np.ones(m.sum(), np.int64)], 1), np.stack([t1[m], -np.ones(m.sum(), np.int64)], 1)])
        ev = ev[np.lexsort((ev[:, 1], ev[:, 0]))]
        res = np.cumsum(ev[:, 1]); seg = np.diff(ev[:, 0], append=ev[-1, 0])
        filled = np.argmax(res >= 128) if (res >= 128).any() else 0
        below = [us(seg[filled:][res[filled:] < 32 * n].sum()) for n in (4, 3, 2)]
        last = np.argsort(t1[m])[-3:]
        ends.append(t1[m].max())
        print(f"   {k}     {us(t0[m].min()):8.1f}   {us(t0[m].max()):8.1f}   {us(t1[m].max()):8.1f}  " + "  ".join(f"{v:6.1f}" for v in below) + "   "
              + "; ".join(f"({rng[m][i]}, {p[m][i]}, {nt[m][i]}, {us(t1[m][i]):.1f})" for i in last))
    print(f"   XCD ends: min {us(min(ends)):.1f}, max {us(max(ends)):.1f} us; spread {us(max(ends) - min(ends)):.1f} us = {100 * (max(ends) - min(ends)) / dur:.2f} % of the launch")
    ev = np.concatenate([np.stack([t0, np.ones_like(t0)], 1), np.stack([t1, -np.ones_like(t1)], 1)])
    ev = ev[np.lexsort((ev[:, 1], ev[:, 0]))]
    res = np.cumsum(ev[:, 1]); seg = np.diff(ev[:, 0], append=ev[-1, 0])
    print("   device: us with fewer than 4 / 3 / 2 workgroups per CU resident on average (of 256 CUs): "
          + " / ".join(f"{us(seg[res < 256 * n].sum()):.1f}" for n in (4, 3, 2)))
    print("   resident workgroups per XCD (of 128) at the given share of the launch:")
    marks = [0.02, 0.25, 0.5, 0.75, 0.9, 0.92, 0.94, 0.96, 0.97, 0.98, 0.99, 0.995]
    print("   share  " + " ".join(f"{100 * s:6.1f}" for s in marks))
    for k in range(8):
        m = xcc == k
        print(f"   XCD {k}  " + " ".join(f"{int(np.sum((t0[m] <= s * dur) & (t1[m] > s * dur))):6d}" for s in marks))


if DRAIN:
    h = HipNetwork(9, 10, 128, NB, rows_cap=B, precision="f32")
    h.set_weights(random_weights(9, 10, 128, NB))
    x = (np.random.RandomState(0).rand(B, 10, 9, 9) < 0.2).astype(np.float32)
    h.main_prediction(x[:256])
    for _ in range(2):
        h.main_prediction(x)
    print(f"# drain timeline of k_conv3x3_sg<9,128>: rows {B}, {NB} blocks, the stamped build (slower than the product: read the shapes)")
    drain_table(drain_records(0), "conv1 <9,128,0,SIN>")
    drain_table(drain_records(1), "conv2 <9,128,1,SIN,SOUT>")
    sys.exit(0)

h = HipNetwork(9, 10, 128, NB, rows_cap=B, precision="f32")
h.set_weights(random_weights(9, 10, 128, NB))
x = (np.random.RandomState(0).rand(B, 10, 9, 9) < 0.2).astype(np.float32)
h.main_prediction(x[:256])
h.ctx.call("tg_prof_enable", 1, 4096)
for _ in range(3):
    h.main_prediction(x)
ms, n, fl = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
h.ctx.call("tg_prof_read", ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl))
fn = _lib.load().tg_debug_conv_stamps
fn.restype = ctypes.c_int; fn.argtypes = [ctypes.c_void_p, ctypes.c_int]
out = (ctypes.c_ulonglong * 96)()
assert fn(out, 96) == 0
s = np.array([int(v) for v in out], dtype=np.int64).reshape(2, 2, 3, 8)           # [EPI][round][class][phase]
# The unit is the tick of __builtin_readcyclecounter.  It is NOT the 10 ns of s_memrealtime: an interior workgroup's walk of 72 stages
# reads ~480 k ticks while a launch of 9936 workgroups on 1024 slots takes ~2.4 ms (~250 us per workgroup), about 0.5 ns per tick.
print(f"rows {B}, blocks {NB}; stamped build: "
      f"{n.value} conv launches, {ms.value / n.value:.3f} ms on average (not the product's time)")
names = ["entry -> bias (|s2|t2) issued", "-> weight DMAs of the prologue issued", "-> first counted wait + barrier passed",
         "-> first MFMAs issued (B fragments, residual landed)", "-> last MFMA issued (all stores but the last tile's are out)",
         "-> the last cout tile's stores issued", "-> stores written"]
for e, kern in enumerate(("conv1 <9,128,0,SIN>", "conv2 <9,128,1,SIN,SOUT>")):
    for r, rnd in enumerate(("first round (range 0)", "middle round (range 7)")):
        print(f"{kern}, {rnd}: ticks per phase (share of the workgroup) for interior | edge | corner")
        d = np.diff(s[e, r], axis=1).astype(float)                                       # [class][7 phases]
        for i, nm in enumerate(names):
            print(f"  {nm:62s} " + " | ".join(f"{d[c, i]:8.0f} ({100 * d[c, i] / d[c].sum():4.1f} %)" for c in range(3)))
        fixed = d[:, :4].sum(1) + d[:, 5:].sum(1)
        print(f"  {'fixed part = everything but the walk':62s} " + " | ".join(f"{fixed[c]:8.0f} ({100 * fixed[c] / d[c].sum():4.1f} %)" for c in range(3)))
