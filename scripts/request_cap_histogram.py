"""The value net's step at its resident set, measured: per-launch durations of k_vn_conv, k_vn_fc1 and k_sim_step from a
`rocprofv3 --kernel-trace --output-format csv` run of the benchmark command, joined launch by launch with the requests every
launch serves (scripts/request_counts.py: the same games, the same launches).

    python scripts/request_cap_histogram.py <trace dir> <counts.json> <out.json> [--warmup 5] [--cap 2048]

Reports, over the timed window (the moves after --warmup): the share q of launches with n > cap, the excess e = n - cap by move,
the cost of an overflow round (conv + fc1 of launches just above the cap against launches just below), the cost of a full step,
q x overflow cost x sims per move (the go / no-go figure of the request cap) and T = 1 + overflow cost / full step cost."""
import csv
import glob
import json
import os
import sys

import numpy as np

argv = [x for x in sys.argv[1:]]


def opt(name, default):
    if name in argv:
        i = argv.index(name)
        v = int(argv[i + 1])
        del argv[i:i + 2]
        return v
    return default


warmup, cap, band = opt("--warmup", 5), opt("--cap", 2048), opt("--band", 256)
src, counts_path, out = argv[0], argv[1], argv[2]
with open(counts_path) as f:
    doc = json.load(f)
counts = np.asarray(doc["counts"], np.int64)
moves, sims = counts.shape
by_kernel = {"conv": [], "fc1": [], "tree": []}
for path in glob.glob(os.path.join(src, "**", "*kernel_trace.csv"), recursive=True):
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            key = "conv" if "k_vn_conv" in name else "fc1" if "k_vn_fc1" in name else "tree" if "k_sim_step" in name else None
            if key:
                by_kernel[key].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
dur = {}
for key, ls in by_kernel.items():
    ls.sort()
    dur[key] = np.asarray([x[1] for x in ls], np.float64) / 1e3      # us, in start order
launches = {k: int(len(v)) for k, v in dur.items()}
# the join needs the benchmark's launches to be the counted ones: sims evaluator launches a move, sims + 1 tree launches, no catch-up
if launches["conv"] != moves * sims or launches["fc1"] != moves * sims or launches["tree"] != moves * (sims + 1):
    sys.exit("the trace has %s launches, the counts describe %d moves x %d: not the same run shape" % (launches, moves, sims))
conv = dur["conv"].reshape(moves, sims)
fc1 = dur["fc1"].reshape(moves, sims)
tree = dur["tree"].reshape(moves, sims + 1)[:, 1:]      # the launch that follows evaluator launch i (backup of i, front of i + 1)
w = slice(warmup, moves)
n, c, f, t = counts[w].ravel(), conv[w].ravel(), fc1[w].ravel(), tree[w].ravel()
nn = c + f


def stats(x):
    if len(x) == 0:
        return None
    return {"launches": int(len(x)), "mean": round(float(x.mean()), 2), "p10": round(float(np.percentile(x, 10)), 2),
            "p50": round(float(np.percentile(x, 50)), 2), "p90": round(float(np.percentile(x, 90)), 2), "max": round(float(x.max()), 2)}


over, below, above = n > cap, (n <= cap) & (n > cap - band), (n > cap) & (n <= cap + band)
q = float(over.mean())
bins = []
for lo in range(int(n.min()) // 128 * 128, int(n.max()) + 1, 128):
    sel = (n >= lo) & (n < lo + 128)
    if sel.any():
        bins.append({"requests": [lo, lo + 127], "launches": int(sel.sum()), "conv_us_mean": round(float(c[sel].mean()), 2),
                     "conv_us_max": round(float(c[sel].max()), 2), "fc1_us_mean": round(float(f[sel].mean()), 2),
                     "fc1_us_p90": round(float(np.percentile(f[sel], 90)), 2), "tree_us_mean": round(float(t[sel].mean()), 2)})
by_move = []
for m in range(warmup, moves):
    e = counts[m] - cap
    o = e > 0
    by_move.append({"move": m + 1, "requests_mean": round(float(counts[m].mean()), 1), "requests_max": int(counts[m].max()),
                    "launches_over": int(o.sum()), "excess_mean": round(float(e[o].mean()), 1) if o.any() else None,
                    "excess_max": int(e[o].max()) if o.any() else None,
                    "first_and_last_launch_over": [int(np.flatnonzero(o)[0]), int(np.flatnonzero(o)[-1])] if o.any() else None,
                    "value_net_us_mean": round(float((conv[m] + fc1[m]).mean()), 2)})
res = {"what": __doc__.split("\n\n")[0],
       "trace": "rocprofv3 --kernel-trace --output-format csv -- python bench.py --gpus 1 --steps %d --warmup %d" % (moves - warmup, warmup),
       "counts": "scripts/request_counts.py --games %d --sims %d --moves %d" % (doc["games"], sims, moves),
       "cap": cap, "band": band, "timed_window_moves": [warmup + 1, moves], "launches_in_the_window": int(len(n)),
       "requests_per_launch": stats(n.astype(np.float64)),
       "share_of_launches_over_the_cap_q": q,
       "excess_over_the_cap": stats((n[over] - cap).astype(np.float64)),
       "conv_us": {"all": stats(c), "just_below": stats(c[below]), "just_above": stats(c[above]), "over": stats(c[over]), "not_over": stats(c[~over])},
       "fc1_us": {"all": stats(f), "just_below": stats(f[below]), "just_above": stats(f[above]), "over": stats(f[over]), "not_over": stats(f[~over])},
       "tree_us": {"all": stats(t)},
       "by_requests": bins, "by_move": by_move}
if above.any() and below.any():
    overflow = float(nn[above].mean() - nn[below].mean())
    full = float((nn[below] + t[below]).mean())
    res["overflow_round_cost_us"] = round(overflow, 2)
    res["full_step_cost_us"] = round(full, 2)
    res["T"] = round(1.0 + overflow / full, 3)
    res["q_x_overflow_cost_x_sims_ms_per_move"] = round(q * overflow * sims / 1e3, 3)
    # what the launches over the cap really paid over a launch just below it (their excess grows past the band)
    res["paid_by_launches_over_the_cap_ms_per_move"] = round(float((nn[over] - nn[below].mean()).sum()) / (moves - warmup) / 1e3, 3)
else:
    res["overflow_round_cost_us"] = None
    res["q_x_overflow_cost_x_sims_ms_per_move"] = 0.0 if not over.any() else None
res["go"] = bool(res["q_x_overflow_cost_x_sims_ms_per_move"] is not None and res["q_x_overflow_cost_x_sims_ms_per_move"] >= 1.5)
with open(out, "w") as fo:
    json.dump(res, fo, indent=1)
print(json.dumps({k: res[k] for k in ("share_of_launches_over_the_cap_q", "overflow_round_cost_us", "full_step_cost_us", "T",
                                      "q_x_overflow_cost_x_sims_ms_per_move", "go") if k in res}))
