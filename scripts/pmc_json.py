#!/usr/bin/env python3
"""rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of scripts/collect_profiles.sh -> profiles/rN_pmc_traffic.json.
usage: pmc_json.py [gpurun_out/prof_r2] [out.json]"""
import collections, csv, glob, json, statistics, sys

ROOT = sys.argv[1] if len(sys.argv) > 1 else "gpurun_out/prof_r2"
OUT = sys.argv[2] if len(sys.argv) > 2 else "profiles/r2_pmc_traffic.json"
F = 128


def load(d, counter):
    per = collections.defaultdict(list)
    for f in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if r["Counter_Name"] != counter:
                continue
            k = r["Kernel_Name"].replace("void (anonymous namespace)::", "").split("(")[0]
            per[k].append((int(r["Dispatch_Id"]), float(r["Counter_Value"]), float(r["End_Timestamp"]) - float(r["Start_Timestamp"]), int(r["Grid_Size"])))
    return {k: sorted(v) for k, v in per.items()}


fe, wr = load(ROOT + "/fetch", "FETCH_SIZE"), load(ROOT + "/write", "WRITE_SIZE")
out = {"source": "rocprofv3 --kernel-trace --pmc FETCH_SIZE / --pmc WRITE_SIZE (separate passes, scripts/collect_profiles.sh) on `python3 bench.py "
                 "--steps 1 --warmup 1 --no-cpu-baseline`; medians over the launches of the last (timed) step -- for the conv kernel over its "
                 "full-batch launches (grid within 5 % of the largest)",
       "correction": "FETCH_SIZE doubled (gfx950 tallies 128-B requests as 64 B: MI355X_MICROARCH.md, HBM section); WRITE_SIZE exact; counter unit KB",
       "kernels": {}}
for k in sorted(set(fe) | set(wr)):
    if not k.startswith("k_"):
        continue
    conv = "k_conv3x3_sg" in k
    f, w = fe.get(k, []), wr.get(k, [])
    if not f or not w:
        continue
    if conv:
        f = [x for x in f if x[3] >= 0.95 * max(y[3] for y in f)][-600:]
        w = [x for x in w if x[3] >= 0.95 * max(y[3] for y in w)][-600:]
    else:
        f, w = f[-101:], w[-101:]
    fk, wk, grid = statistics.median(x[1] for x in f), statistics.median(x[1] for x in w), statistics.median(x[3] for x in f)
    e = {"launches_summarised": len(f), "grid_size_median": grid, "FETCH_SIZE_KB_raw_median": round(fk, 1), "WRITE_SIZE_KB_median": round(wk, 1),
         "hbm_bytes_per_launch": round((2 * fk + wk) * 1024.0, 1), "duration_us_median": round(statistics.median(x[2] for x in f) / 1e3, 2)}
    if conv:
        targs = [t.strip(" >") for t in k.split(",")]                                         # k_conv3x3_sg<S, F, EPI, SIN, SOUT>
        epi = int(targs[2])
        rows = grid / 256 * 128                        # one workgroup per (128 boards, position): workgroups * 128 = boards * P = rows
        # EPI 0 reads its input and writes h: 8F bytes per row; EPI 1 reads h and the residual and writes the stream: 12F
        alg = (8 * F if epi == 0 else 12 * F) * rows
        e.update(boards_per_workgroup=128, rows_per_launch_approx=int(rows), algorithmic_bytes_per_launch=int(alg),
                 traffic_over_algorithmic=round(e["hbm_bytes_per_launch"] / alg, 3))
    out["kernels"][k] = e
convs = [v for k, v in out["kernels"].items() if "k_conv3x3_sg" in k and v["launches_summarised"] > 50]
out["dominant_kernel"] = ("k_conv3x3_sg<9,128,EPI,SIN,SOUT> (EPI 0: relu, SIN: input activated on load; EPI 1: residual stream in the conv's "
                          "row order in (SIN) and out (SOUT); one workgroup per board position x 128 boards, off-board taps skipped)")
out["hbm_bytes_per_launch_mean"] = sum(v["hbm_bytes_per_launch"] for v in convs) / len(convs)
out["algorithmic_bytes_per_launch_mean"] = sum(v["algorithmic_bytes_per_launch"] for v in convs) / len(convs)
tc, ta = out["kernels"]["k_collect<9>"], out["kernels"]["k_absorb<9>"]
out["tree_stage"] = {"hbm_bytes_per_wave": tc["hbm_bytes_per_launch"] + ta["hbm_bytes_per_launch"],
                     "note": "k_collect + k_absorb per search wave (4096 games x up to 4 read-outs, ~16 k simulations); bench.py prices the same wave at "
                             "bytes_per_sim x sims (roofline_tree); the 32-B-record reads are outside the FETCH_SIZE calibration, so treat the ratio as indicative"}
import os, sys as _sys
_sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import net_source_hash
out["net_hip_sha16"] = net_source_hash()      # bench.py reports `traffic` only while the network kernels' code is this (comments apart)
json.dump(out, open(OUT, "w"), indent=1)
for k, v in out["kernels"].items():
    if "conv3x3_sg" in k:
        print(k, v["launches_summarised"], v["duration_us_median"], v["hbm_bytes_per_launch"], v.get("traffic_over_algorithmic"))
print(out["hbm_bytes_per_launch_mean"], out["tree_stage"]["hbm_bytes_per_wave"])
