#!/usr/bin/env python
"""Time of the offline targets on a synthetic recording (profiles/offline_targets_timing.json).

    python scripts/offline_targets_timing.py [--json FILE] [--slots 4096] [--moves 200]

The table: `--slots` slots x `--moves` moves in file order (move-major, slot-minor), 819 200 rows of 368 bytes by default, episode
lengths long-tailed (geometric, mean 25 moves) with eight slots that play ONE episode through all the moves.  Timed on the
device, each the median of 20 calls between two events after 3 warm-ups: offline.episode_index (the two stable sorts and the
episode table's lookup), tm_episode_targets in mode 1 (lambda = 0.9, visit weights over variance) and tm_episode_gather_states
over every row; the kernel again on the segments longer than 64 rows alone and on the others alone (long episodes run their
chunks one after the other: how much of the launch is theirs).  On the host, the median of 3: EpisodeLoader's sort and copy
(np.lexsort and the fancy index of the 368-byte table) and offline.targets_numpy.  Peak device memory is torch's.
Needs a GPU: there is no fall-back.

    python scripts/offline_targets_timing.py --discounted [--json FILE]      (profiles/offline_targets_discounted_timing.json)

The same table, mode 1, lambda = 0.9, visit weights over variance: tm_episode_targets against tm_episode_targets_discounted at
gamma = 0.999 without and with v_rows, in one process, ALTERNATING - `--repeats` passes, each timing every side once as the median
of 20 single calls between two events (the way the figure above was taken) and once as 200 calls back to back between two events
(a window long enough that the events' own cost does not count).  The spread is that of a side's passes.  Then predict_rows over
the table under a seeded Model_VV: host clock around the call up to a synchronise, the median of 5, and the same loop with the
gathers alone.  The values of the discounted call are compared with offline.targets_numpy in ulp."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_table(G, M, seed=0):
    from tetris_mcts_amd.episodes import EPISODE_DTYPE, STATE_DTYPE
    rng = np.random.default_rng(seed)
    ends = rng.random((M, G)) < 1.0 / 25            # the slot's episode ends with this move
    ends[:, :8] = False                             # eight slots play one episode all the way
    ends[M - 1] = False                             # what is under way at the end is censored
    started = np.zeros((M, G), bool)
    started[0] = True
    started[1:] = ends[:-1]
    # ids: the first G episodes are the slots, later ones by move, then by slot (the recorder's rule)
    new_id = np.zeros((M, G), np.int64)
    new_id[0] = np.arange(G)
    later = started.copy()
    later[0] = False
    new_id[later] = G + np.arange(int(later.sum()))
    start_move = np.where(started, np.arange(M)[:, None], 0)
    start_move = np.maximum.accumulate(start_move, axis=0)
    episode = np.take_along_axis(new_id, start_move, axis=0)
    step = rng.integers(0, 4001, (M, G))
    total = np.cumsum(step, axis=0) - step          # the score before the move
    score = total - np.take_along_axis(total, start_move, axis=0)
    rows = np.zeros(M * G, STATE_DTYPE)
    rows["episode"], rows["cycle"], rows["slot"] = episode.reshape(-1), 1, np.tile(np.arange(G), M)
    rows["move"], rows["score"] = (np.arange(M)[:, None] - start_move).reshape(-1), score.reshape(-1)
    rows["value"] = rng.uniform(0, 200, M * G).astype(np.float32)
    rows["variance"] = rng.uniform(1e-3, 500, M * G).astype(np.float32)
    rows["child_stats"][:, 0, :] = rng.integers(0, 400, (M * G, 7)).astype(np.float32)
    rows["board"] = rng.integers(0, 2, (M * G, 20, 10), dtype=np.int8)
    ep = np.zeros(int(ends.sum()), EPISODE_DTYPE)
    m, g = np.nonzero(ends)
    ep["episode"], ep["cycle"], ep["slot"] = episode[m, g], 1, g
    ep["moves"], ep["score"] = rows["move"].reshape(M, G)[m, g] + 1, score[m, g] + step[m, g]
    return rows, ep


def device_ms(fn, calls=20, warm=3):
    import torch
    for _ in range(warm):
        fn()
    out = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return dict(median_ms=statistics.median(out), min_ms=min(out), max_ms=max(out), calls=calls)


def host_ms(fn, calls=3):
    out = []
    for _ in range(calls):
        t = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t))
    return dict(median_ms=statistics.median(out), min_ms=min(out), max_ms=max(out), calls=calls)


def batch_ms(fn, calls=200, warm=3):
    """one call's share of `calls` calls back to back between two events"""
    import torch
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def discounted(a):
    import torch
    from tetris_mcts_amd import offline as O
    from tetris_mcts_amd.model import Model_VV
    rows, ep = make_table(a.slots, a.moves)
    n = len(rows)
    rows_d = O.rows_tensor(rows, "cuda")
    index = O.episode_index(rows_d, None, ep, None)
    kind = index.ended.to(torch.uint8)
    tval = torch.zeros(kind.shape[0], dtype=torch.float32, device="cuda")
    v_rows = torch.from_numpy(np.random.default_rng(1).uniform(0, 200, n).astype(np.float32)).cuda()
    head = (rows_d, index.order, index.seg, kind, index.final_score, tval, 1, 0.9, 3)
    sides = {"tm_episode_targets": lambda: O.targets_device(*head),
             "discounted_gamma_0.999": lambda: O.targets_device(*head, gamma=0.999),
             "discounted_gamma_0.999_v_rows": lambda: O.targets_device(*head, gamma=0.999, v_rows=v_rows)}
    single, batched = {k: [] for k in sides}, {k: [] for k in sides}
    for _ in range(a.repeats):
        for k, fn in sides.items():
            single[k].append(device_ms(fn)["median_ms"])
        for k, fn in sides.items():
            batched[k].append(batch_ms(fn))

    def spread(x):
        return dict(median_ms=statistics.median(x), min_ms=min(x), max_ms=max(x), passes=len(x))
    res = dict(slots=a.slots, moves=a.moves, rows=n, segments=int(kind.shape[0]), device=torch.cuda.get_device_name(0),
               mode=1, lam=0.9, gamma=0.999, weight_mode=3,
               single_call_median_of_20={k: spread(v) for k, v in single.items()},
               per_call_of_200_back_to_back={k: spread(v) for k, v in batched.items()})
    base = res["per_call_of_200_back_to_back"]["tm_episode_targets"]
    for k in ("discounted_gamma_0.999", "discounted_gamma_0.999_v_rows"):
        r = res["per_call_of_200_back_to_back"][k]
        res[k + "_over_tm_episode_targets"] = r["median_ms"] / base["median_ms"]
    # (each call above also allocates and clears its three outputs: both sides alike)
    order_h, seg_h = index.order.cpu().numpy(), index.seg.cpu().numpy()
    tail_h = (kind.cpu().numpy(), index.final_score.cpu().numpy(), tval.cpu().numpy())
    same = {}
    for name, v in (("discounted_gamma_0.999", None), ("discounted_gamma_0.999_v_rows", v_rows)):
        got = [x.cpu().numpy() for x in O.targets_device(*head, gamma=0.999, v_rows=v)[:3]]
        want = O.targets_numpy(rows, order_h, seg_h, *tail_h, 1, 0.9, 3, gamma=0.999, v_rows=None if v is None else v.cpu().numpy())
        same[name] = dict(value_max_ulp=int(np.abs(got[0].view(np.int32).astype(np.int64) - want[0].view(np.int32).astype(np.int64)).max()),
                          variance_bits=got[1].tobytes() == want[1].tobytes(), weight_bits=got[2].tobytes() == want[2].tobytes())
    res["same_results"] = same
    model = Model_VV(backend="hip", seed=0)

    def gathers(chunk=65536):
        for lo in range(0, n, chunk):
            O.gather_states(rows_d, torch.arange(lo, min(n, lo + chunk), dtype=torch.int32, device="cuda"))

    def synced(fn):
        def run():
            fn()
            torch.cuda.synchronize()
        return run
    O.predict_rows(model, rows_d)
    total = host_ms(synced(lambda: O.predict_rows(model, rows_d)), calls=5)
    gather = host_ms(synced(gathers), calls=5)
    res["predict_rows"] = dict(chunk=65536, total=total, gathers_alone=gather, gather_share=gather["median_ms"] / total["median_ms"])
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--moves", type=int, default=200)
    ap.add_argument("--discounted", action="store_true", help="time tm_episode_targets_discounted against tm_episode_targets")
    ap.add_argument("--repeats", type=int, default=7, help="--discounted: alternating passes over the sides")
    a = ap.parse_args()
    import torch
    from tetris_mcts_amd import offline as O
    from tetris_mcts_amd.episodes import ROW_BYTES, STATE_DTYPE
    if not torch.cuda.is_available():
        sys.exit("offline_targets_timing.py measures the device route: it needs a GPU")
    if a.discounted:
        return discounted(a)
    rows, ep = make_table(a.slots, a.moves)
    n = len(rows)
    t = time.perf_counter()
    rows_d = O.rows_tensor(rows, "cuda")
    torch.cuda.synchronize()
    upload_ms = 1e3 * (time.perf_counter() - t)
    torch.cuda.reset_peak_memory_stats()
    res = dict(slots=a.slots, moves=a.moves, rows=n, table_bytes=n * ROW_BYTES, episodes_ended=len(ep), upload_ms_once=upload_ms,
               device=torch.cuda.get_device_name(0))
    index = O.episode_index(rows_d, None, ep, None)
    length = (index.seg[1:] - index.seg[:-1]).cpu().numpy()
    res["segments"] = dict(count=len(length), longest=int(length.max()), mean=float(length.mean()),
                           longer_than_64=int((length > 64).sum()), rows_in_longer_than_64=int(length[length > 64].sum()))
    res["episode_index"] = device_ms(lambda: O.episode_index(rows_d, None, ep, None))
    kind = index.ended.to(torch.uint8)
    tval = torch.zeros(len(length), dtype=torch.float32, device="cuda")

    def targets(seg=index.seg, kind=kind, score=index.final_score, tval=tval):
        return O.targets_device(rows_d, index.order, seg, kind, score, tval, 1, 0.9, 3)
    res["tm_episode_targets"] = device_ms(targets)
    # long episodes alone, short ones alone: each segment handed over as a table of its own two bounds would need a call per
    # segment, so the rows are re-indexed instead - the same rows, the same order, only the segments of one kind
    seg = index.seg.cpu().numpy().astype(np.int64)
    order = index.order.cpu().numpy()
    for name, pick in (("long_only", length > 64), ("short_only", length <= 64)):
        take = np.nonzero(pick)[0]
        pieces = [order[seg[e]:seg[e + 1]] for e in take]
        sub_order = torch.from_numpy(np.concatenate(pieces).astype(np.int32)).cuda()
        sub_seg = torch.from_numpy(np.concatenate([[0], np.cumsum(length[take])]).astype(np.int32)).cuda()
        idx = torch.from_numpy(take).cuda()
        k, s, v = kind[idx].contiguous(), index.final_score[idx].contiguous(), tval[idx].contiguous()
        res["tm_episode_targets_" + name] = dict(
            device_ms(lambda: O.targets_device(rows_d, sub_order, sub_seg, k, s, v, 1, 0.9, 3)), segments=len(take),
            rows=int(length[take].sum()))
    res["tm_episode_gather_states"] = device_ms(lambda: O.gather_states(rows_d, index.order))
    res["peak_device_bytes"] = int(torch.cuda.max_memory_allocated())
    got = [x.cpu().numpy() for x in targets()[:3]]

    def loader_sort_and_copy():
        o = np.lexsort((rows["move"], rows["episode"], rows["cycle"]))
        return rows.view(np.uint8).reshape(n, ROW_BYTES)[o].view(STATE_DTYPE).reshape(-1)
    res["host_sort_and_copy"] = host_ms(loader_sort_and_copy)
    order_h, seg_h = order, seg
    kind_h, score_h, tval_h = kind.cpu().numpy(), index.final_score.cpu().numpy(), tval.cpu().numpy()
    res["host_targets_numpy"] = host_ms(lambda: O.targets_numpy(rows, order_h, seg_h, kind_h, score_h, tval_h, 1, 0.9, 3))
    want = O.targets_numpy(rows, order_h, seg_h, kind_h, score_h, tval_h, 1, 0.9, 3)
    ulp = int(np.abs(got[0].view(np.int32).astype(np.int64) - want[0].view(np.int32).astype(np.int64)).max())
    res["same_results"] = dict(value_max_ulp=ulp, variance_bits=got[1].tobytes() == want[1].tobytes(),
                               weight_bits=got[2].tobytes() == want[2].tobytes())
    dev = res["episode_index"]["median_ms"] + res["tm_episode_targets"]["median_ms"]
    host = res["host_sort_and_copy"]["median_ms"] + res["host_targets_numpy"]["median_ms"]
    res["routes"] = dict(device_index_plus_targets_ms=dev, host_sort_copy_plus_targets_ms=host, host_over_device=host / dev)
    line = json.dumps(res)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
