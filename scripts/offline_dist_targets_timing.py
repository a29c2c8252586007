#!/usr/bin/env python
"""Time of the categorical episode targets on a synthetic recording (profiles/offline_dist_targets_timing.json).

    python scripts/offline_dist_targets_timing.py [--json FILE] [--slots 4096] [--moves 200] [--atoms 50]

The table is scripts/offline_targets_timing.py's: `--slots` slots x `--moves` moves in file order, 819 200 rows by default, episode
lengths long-tailed (geometric, mean 25 moves) with eight slots that play ONE episode through all the moves.  The distributions by
table row are softmax draws in float32 [n, 64]; atoms over [0, 5000).

Timed on the device, each the median of 20 single calls of tm_episode_dist_targets between two events after 3 warm-ups, the
outputs allocated once before (the call itself allocates nothing): mode 0, and mode 1 at lambda = 0.9 with horizon 0, 16 and 64,
visit weights over variance.  A single call between two events carries the events' own cost (some 10 us): at these sizes it is
below a percent.  Then offline.predict_rows_dist over the table under a seeded Model_Dist: host clock around the call up to a
synchronise, the median of 5.  On the host, for comparison, offline.dist_targets_numpy on the first segments of the table (some
16 000 rows; the median of 3), scaled by the rows to the whole table; the kernel's output on those rows is compared with it in ulp.
One process, nothing else on the device; clocks and power state as the machine had them.  Needs a GPU: there is no fall-back."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--moves", type=int, default=200)
    ap.add_argument("--atoms", type=int, default=50)
    ap.add_argument("--host_rows", type=int, default=16384, help="the numpy statement runs on the segments before this position")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("offline_dist_targets_timing.py measures the device route: it needs a GPU")
    from offline_targets_timing import device_ms, host_ms, make_table
    from tetris_mcts_amd import _lib
    from tetris_mcts_amd import offline as O
    from tetris_mcts_amd.model_distributional import Model_Dist
    K, vmin, vmax, lam, wmode = a.atoms, 0.0, 5000.0, 0.9, 3
    rows, ep = make_table(a.slots, a.moves)
    n = len(rows)
    rows_d = O.rows_tensor(rows, "cuda")
    index = O.episode_index(rows_d, None, ep, None)
    kind = index.ended.to(torch.uint8)
    rng = np.random.default_rng(1)
    logits = rng.normal(0, 2.5, (n, K)).astype(np.float32)
    p = np.zeros((n, 64), np.float32)
    p[:, :K] = np.exp(logits - logits.max(1, keepdims=True))
    p[:, :K] /= p[:, :K].sum(1, keepdims=True)
    p_d = torch.from_numpy(p).cuda()
    target = torch.zeros(n, 64, dtype=torch.float32, device="cuda")
    weight = torch.zeros(n, dtype=torch.float32, device="cuda")
    fault = torch.zeros(1, dtype=torch.int32, device="cuda")
    L = _lib.lib()

    def call(mode, horizon, n_seg=None):
        _lib.check(L.tm_episode_dist_targets(
            rows_d.data_ptr(), n, index.order.data_ptr(), index.seg.data_ptr(), kind.shape[0] if n_seg is None else n_seg,
            kind.data_ptr(), index.final_score.data_ptr(), p_d.data_ptr(), 64, K, vmin, vmax, mode, lam, horizon, wmode, O.EPS,
            target.data_ptr(), 64, weight.data_ptr(), fault.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
            "tm_episode_dist_targets")
    length = (index.seg[1:] - index.seg[:-1]).cpu().numpy()
    res = dict(slots=a.slots, moves=a.moves, rows=n, atoms=K, vmin=vmin, vmax=vmax, lam=lam, weight_mode=wmode,
               device=torch.cuda.get_device_name(0),
               segments=dict(count=len(length), longest=int(length.max()), mean=float(length.mean())))
    res["mode_0"] = device_ms(lambda: call(0, 0))
    for h in (0, 16, 64):
        res["mode_1_horizon_%d" % h] = device_ms(lambda: call(1, h))
    res["fault_word"] = int(fault.item())
    model = Model_Dist(atoms=K, backend="hip", seed=0)

    def predict():
        O.predict_rows_dist(model, rows_d)
        torch.cuda.synchronize()
    predict()
    res["predict_rows_dist"] = dict(host_ms(predict, calls=5), chunk=65536)
    # the numpy statement on the first segments
    seg_h, order_h = index.seg.cpu().numpy(), index.order.cpu().numpy()
    m = int(np.searchsorted(seg_h, a.host_rows, side="right")) - 1
    sub, end = seg_h[:m + 1], int(seg_h[m])
    kind_h, score_h = kind.cpu().numpy()[:m], index.final_score.cpu().numpy()[:m]
    host = {}
    for h in (16, 64):
        def run(h=h):
            return O.dist_targets_numpy(rows, order_h, sub, kind_h, score_h, K, vmin, vmax, 1, lam, h, wmode, O.EPS, p)
        t = host_ms(run)
        want = run()
        target.zero_()
        call(1, h, n_seg=m)
        got = target[:end, :K].cpu().numpy()
        ulp = int(np.abs(got.view(np.int32).astype(np.int64) - want[0][:end].view(np.int32).astype(np.int64)).max())
        host["horizon_%d" % h] = dict(t, rows=end, segments=m, scaled_to_the_table_ms=t["median_ms"] * n / end, kernel_max_ulp=ulp,
                                      weight_bits=weight[:end].cpu().numpy().tobytes() == want[1][:end].tobytes())
    res["host_dist_targets_numpy"] = host
    res["host_over_device_horizon_64"] = host["horizon_64"]["scaled_to_the_table_ms"] / res["mode_1_horizon_64"]["median_ms"]
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
