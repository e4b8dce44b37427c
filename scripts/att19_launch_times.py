#!/usr/bin/env python3
"""rocprofv3 per-dispatch kernel trace of a 19x19 MainNetwork run -> per-launch time of the tiled attention core (k_attention_t), of
its q|k|v projection (k_conv3x3 with 1.5 F output channels) and of the F->F conv of a residual block (k_conv3x3_sg), each over its
FULL-BATCH launches (grid within 5 % of the kernel's largest: the same row count for all three; the root evaluations of a few dozen
rows are left out).  usage: att19_launch_times.py <trace_kernel_trace.csv> <out.json> [filters]"""
import collections, csv, json, sys

F = int(sys.argv[3]) if len(sys.argv) > 3 else 128
per = collections.defaultdict(list)
for r in csv.DictReader(open(sys.argv[1])):
    k = r["Kernel_Name"].replace("void (anonymous namespace)::", "").split("(")[0]
    proj = k.startswith("k_conv3x3<") and f", {F}, {F * 3 // 2}," in k
    if k.startswith("k_attention_t") or k.startswith("k_conv3x3_sg") or proj:
        grid = int(r["Grid_Size"]) if "Grid_Size" in r else int(r["Grid_Size_X"])
        per[k].append((grid, float(r["End_Timestamp"]) - float(r["Start_Timestamp"])))
out = {"source": "rocprofv3 --kernel-trace on `python3 bench.py --no-launcher --no-cpu-baseline --gpus 1 --board 19 --network transgo "
                 f"--filters {F} ...` (the line beside this file), per-dispatch trace, full-batch launches only", "kernels": {}}
for k, v in sorted(per.items()):
    g = max(x[0] for x in v)
    full = [d for gs, d in v if gs >= 0.95 * g]
    out["kernels"][k] = {"launches": len(v), "full_batch_launches": len(full), "full_batch_grid": g,
                         "avg_us_all": round(sum(d for _, d in v) / len(v) / 1e3, 1), "avg_us_full_batch": round(sum(full) / len(full) / 1e3, 1),
                         "min_us_full_batch": round(min(full) / 1e3, 1)}
json.dump(out, open(sys.argv[2], "w"), indent=1)
print(json.dumps(out["kernels"], indent=1))
