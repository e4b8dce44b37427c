"""What symmetry-aware evaluation costs: device time of the engine's evaluation (tg_sp_eval: no PCIe traffic) on a full batch under
modes none / position / mean8, in one process, and the two symmetry kernels' own times from HIP events.

    python scripts/time_symmetry.py [rows=16384] [filters=128] [blocks=6] [precision=f32] [out=profiles/symmetry_cost.txt]

The batch is the root batch of `rows` fresh games (every row the empty board: the kernels' work does not depend on the planes'
contents).  Expectations are relative to mode none of the same run: position = the forward plus the two kernels, mean8 = eight of
each."""
import ctypes, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transgo_amd import model
from transgo_amd.engine import SelfPlayEngine

B = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
F = int(sys.argv[2]) if len(sys.argv) > 2 else 128
NB = int(sys.argv[3]) if len(sys.argv) > 3 else 6
PREC = sys.argv[4] if len(sys.argv) > 4 else "f32"
OUT = sys.argv[5] if len(sys.argv) > 5 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "symmetry_cost.txt")
S, C, REPS = 9, 10, 9

eng = SelfPlayEngine(B, board_size=S, num_simulation=1, parallel_readouts=1, net_blocks=NB, net_filters=F, net_precision=PREC,
                     record_games=False, pool_slots=2048)
model.load_into(eng.ctx, model.random_weights(S, C, F, NB), S, C, F, NB)
seeds = np.arange(B, dtype=np.uint32)
lines = [f"symmetry-aware evaluation, {NB}x{F} {PREC} tower at {S}x{S}, {B} rows per evaluation, median of {REPS} (tg_sp_eval + tg_sync, wall clock)"]
base = None
for mode in ("none", "position", "mean8"):
    eng.set_symmetry(mode, 1)
    eng.ctx.call("tg_sp_reset", seeds.ctypes.data_as(ctypes.c_void_p), None)          # leaves the root batch pending: B rows
    for _ in range(2):
        eng.ctx.call("tg_sp_eval")
    eng.ctx.call("tg_sync")
    eng.ctx.call("tg_prof_enable_symmetry", 1, 4 * 8 * REPS)
    ts = []
    for _ in range(REPS):
        t = time.perf_counter()
        eng.ctx.call("tg_sp_eval"); eng.ctx.call("tg_sync")
        ts.append((time.perf_counter() - t) * 1e3)
    tm, bm, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
    eng.ctx.call("tg_prof_read_symmetry", ctypes.byref(tm), ctypes.byref(bm), ctypes.byref(n))
    eng.ctx.call("tg_prof_enable_symmetry", 0, 0)
    eng.ctx.call("tg_sp_expand_roots")
    ms = float(np.median(ts))
    base = base or ms
    per = max(n.value // 2, 1)                            # launches of each kernel
    lines.append(f"{mode:<9} {ms:8.3f} ms / evaluation   x{ms / base:5.3f} of none   bit-plane transform {tm.value / per * 1e3:7.1f} us, "
                 f"output back-map {bm.value / per * 1e3:7.1f} us per launch ({n.value // 2 // REPS} of each per evaluation)")
staging = ctypes.c_uint64()
eng.ctx.call("tg_net_symmetry_staging", ctypes.byref(staging))
lines.append(f"staging buffers: {staging.value / 2**20:.1f} MiB")
eng.close()
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write(text)
