"""scripts/sim_step_icache.py: rocprofv3's counter_collection.csv of two counter passes -> per-kernel means per launch, the
instruction cache's hit rate and the instruction-wait share, merged into a JSON that already holds other keys."""
import csv
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS = ["Correlation_Id", "Dispatch_Id", "Kernel_Name", "Counter_Name", "Counter_Value"]


def _pass(path, rows):
    os.makedirs(os.path.dirname(path))
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(COLS)
        w.writerows(rows)


def test_icache_summary_of_two_passes(tmp_path):
    k, other = "void tmcts::k_sim_step<false>(tm_store, int)", "void tmcts::k_vn_conv_fc1(Args)"
    a, b = [], []
    for d, (req, hit, miss, cyc, wait) in enumerate([(1000, 900, 100, 4000, 400), (1000, 990, 10, 4000, 1200), (3000, 2970, 30, 8000, 800)]):
        a += [[d, d + 1, k, "SQC_ICACHE_REQ", req], [d, d + 1, k, "SQC_ICACHE_HITS", hit], [d, d + 1, k, "SQC_ICACHE_MISSES", miss]]
        b += [[d, d + 1, k, "SQ_WAVE_CYCLES", cyc], [d, d + 1, k, "SQ_WAIT_INST_ANY", wait]]
    a.append([9, 10, other, "SQC_ICACHE_REQ", 5])
    _pass(str(tmp_path / "A" / "x" / "a_counter_collection.csv"), a)
    _pass(str(tmp_path / "B" / "x" / "b_counter_collection.csv"), b)
    stats = tmp_path / "stats.csv"
    stats.write_text("Name,Calls,CallsAveraged,TotalDurationNs,AverageNs,MinNs,MaxNs\n\"%s\",3,2,118000,59000.0,50000,70000\n" % k)
    out = tmp_path / "out.json"
    out.write_text(json.dumps({"code_size": {"kept": 1}}))
    subprocess.check_call([sys.executable, os.path.join(ROOT, "scripts", "sim_step_icache.py"), str(out), str(tmp_path / "A"), str(tmp_path / "B"),
                           "--last", "2", "--stats", str(stats)], stdout=subprocess.DEVNULL)
    doc = json.loads(out.read_text())
    assert doc["code_size"] == {"kept": 1}
    assert list(doc["counters"]) == ["tmcts::k_sim_step<false>"]                 # other kernels are left out
    c = doc["counters"]["tmcts::k_sim_step<false>"]
    assert c["launches"] == 3 and c["launches_averaged"] == 2                     # the last two launches, in dispatch order
    assert c["per_launch"]["SQC_ICACHE_REQ"] == 2000 and c["icache_misses_per_launch"] == 20
    assert abs(c["icache_hit_rate"] - 1980 / 2000) < 1e-12
    assert abs(c["sq_wait_inst_any_share_of_wave_cycles"] - 1000 / 6000) < 1e-12
    assert doc["kernel_trace_us_per_launch"]["tmcts::k_sim_step<false>"]["avg_us"] == 59.0
