"""The instruction side of the tree kernel from rocprofv3 counter passes (`--pmc ...` alone, no tracing in the same run,
`--kernel-include-regex k_sim_step --output-format csv`; the SQ block has eight slots, so the counters take two passes):

    python scripts/sim_step_icache.py OUT.json PASS_DIR [PASS_DIR ...] [--last N] [--stats KERNEL_STATS.csv] [--command CMD]

Per k_sim_step* kernel: every counter's mean per launch over the last N launches (the timed window), the instruction cache's hit
rate and misses per launch, and the instruction-wait cycles as a share of wave cycles.  --stats: the per-launch times of a separate
`--kernel-trace --stats` run as scripts/kernel_stats.py tabulates them.  OUT.json's other keys ("code_size") are kept."""
import argparse
import csv
import glob
import json
import os
import re
from collections import defaultdict

ap = argparse.ArgumentParser()
ap.add_argument("out_json")
ap.add_argument("dirs", nargs="+")
ap.add_argument("--last", type=int, default=0)
ap.add_argument("--stats", default=None)
ap.add_argument("--command", default=None)
args = ap.parse_args()


def short(name):
    return re.sub(r"\(.*$", "", name).replace("void ", "").strip()


acc = defaultdict(lambda: defaultdict(list))
for d in args.dirs:
    for path in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        with open(path, newline="") as f:
            rows = sorted(csv.DictReader(f), key=lambda r: int(r["Dispatch_Id"]))
        for r in rows:
            acc[short(r["Kernel_Name"])][r["Counter_Name"]].append(float(r["Counter_Value"]))
kernels = {}
for name, cs in acc.items():
    if "k_sim_step" not in name:
        continue
    k = {"launches": max(len(v) for v in cs.values()), "per_launch": {}}
    for c, vals in sorted(cs.items()):
        sel = vals[-args.last:] if args.last > 0 else vals
        k["per_launch"][c] = sum(sel) / len(sel)
        k["launches_averaged"] = len(sel)
    p = k["per_launch"]
    if p.get("SQC_ICACHE_REQ"):
        k["icache_hit_rate"] = p.get("SQC_ICACHE_HITS", 0.0) / p["SQC_ICACHE_REQ"]
        k["icache_misses_per_launch"] = p.get("SQC_ICACHE_MISSES", 0.0)
        k["icache_miss_rate_incl_duplicates"] = (p.get("SQC_ICACHE_MISSES", 0.0) + p.get("SQC_ICACHE_MISSES_DUPLICATE", 0.0)) / p["SQC_ICACHE_REQ"]
    if p.get("SQ_WAVE_CYCLES"):
        for c in ("SQ_WAIT_INST_ANY", "SQ_WAIT_ANY", "SQ_ACTIVE_INST_ANY"):
            if c in p:
                k[c.lower() + "_share_of_wave_cycles"] = p[c] / p["SQ_WAVE_CYCLES"]
    kernels[name] = k
doc = {}
if os.path.exists(args.out_json):
    with open(args.out_json) as f:
        doc = json.load(f)
doc["command"] = args.command or "rocprofv3 --pmc <counters> --kernel-include-regex k_sim_step --output-format csv -- python bench.py --gpus 1 --steps 20 --warmup 5"
doc["units"] = ("per_launch: rocprofv3's Counter_Value per dispatch, summed over the chip; SQ_WAVE_CYCLES / SQ_WAIT_* / SQ_ACTIVE_INST_* "
                "count quad-cycles; SQC_* count requests of the instruction cache a pair of CUs shares")
doc["counters"] = kernels
if args.stats:
    times = {}
    with open(args.stats, newline="") as f:
        for r in csv.DictReader(f):
            if "k_sim_step" in r["Name"]:
                times[short(r["Name"])] = dict(calls=int(r["Calls"]), averaged=int(r["CallsAveraged"]), avg_us=float(r["AverageNs"]) / 1e3,
                                               min_us=float(r["MinNs"]) / 1e3, max_us=float(r["MaxNs"]) / 1e3)
    doc["kernel_trace_us_per_launch"] = times
with open(args.out_json, "w") as f:
    json.dump(doc, f, indent=1)
print(json.dumps({k: {x: v[x] for x in v if x != "per_launch"} for k, v in kernels.items()}, indent=1))
