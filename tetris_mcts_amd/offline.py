"""Offline training from recorded episodes: the middle of the reference's play-then-train cycle (train.py:64-176, cycle.sh).

`play.py --save` leaves State rows in FILE order - move-major, slot-minor, an episode's rows n_games rows apart - and a table of
the episodes that ended (episodes.py).  This module turns them into what `Model_VV.train_data` takes, [states, values, variances,
weights], with the targets that only episodes can give: the realised return and the lambda-return along the moves played.

The rows go to the device once, as they are.  `episode_index` finds the episodes from the int columns alone (two stable sorts of
int64 keys; the 368-byte rows never move), `episode_targets` computes value / variance / weight per sorted position
(csrc/episode_targets.hip: tm_episode_targets), and `training_set` gathers the 200 board bytes of the rows that will train
(tm_episode_gather_states).  With CPU tensors `episode_index` runs the same torch statements on the host, and
`episode_targets(..., device="cpu")` is a numpy statement of the same definitions in fp64 - one backward pass, all episodes at
once.  That statement is the specification: tests/test_offline.py holds it to exact rationals, tests/test_gpu_offline.py holds
the kernel to it.

The three target rules are the reference's (train.py:81-131):
    mode 0  not --td              value_i = s_end - s_i                       (Monte Carlo; integer arithmetic)
    mode 1  --td with a trace     value_i = sum_k lam^k (s_{i+k} + v_{i+k} - s_i) / sum_k lam^k       (the lambda-return)
    mode 2  --td                  value_i = v_i                               (the search's own estimate)
Where the reference's `_v` is sum(n q) / sum(n) over a child_stats row that does not exist, v is the recorded root value.
`terminal="final"` appends to an episode that ended one virtual element (its FINAL score from the episode table, value 0): the
State rows carry the score before the last action, so without it the last action's points are lost.  `terminal="rows"` is the
reference's rule - no such element anywhere, the last row is the end.  An episode without a row in the episode table was cut off
by the end of the run: it is CENSORED.  In mode 1 it has no tail and its last row's value bootstraps the rest; in mode 0
`censored="drop"` leaves its rows out and `censored="keep"` takes its last row as the end (the reference's rule).
Weights: the reference applies --weighted only to mode 2; here the four rules apply in every mode.  weight_mode of the C call =
0 without --weighted, else --weighted_mode + 1.  The reference divides the visits by their mean; `train_data` divides whatever
weights it is given by their mean, so nothing here normalises.

Two options go beyond the reference's rules (tm_episode_targets_discounted); their defaults reproduce the rules above bit for bit:
    gamma     the discount per move.  With r_k = s_{k+1} - s_k:
              mode 0  value_i = sum_k gamma^k r_{i+k}                         (D_i = r_i + gamma D_{i+1})
              mode 1  value_i = sum_k lam^k T_{i,k} / sum_k lam^k,  T_{i,k} = sum_{j<k} gamma^j r_{i+j} + gamma^k v_{i+k}
                      (N_i = v_i + lam (gamma N_{i+1} + B_{i+1} r_i), B_i = 1 + lam B_{i+1}, value_i = N_i / B_i)
              The search backs up score difference + gamma * value' with gamma = 0.999 (ValueSim(gamma=0.999), tm_store.gamma), so
              0.999 is the choice under which the fitted net answers the question the search asks it; 1.0 is the reference's.
    v_rows    float32 by TABLE row: the v_k of the rows, instead of their value column (mode 1 and 2).  `predict_rows` fills it
              from the net being fitted, and fit_episodes(bootstrap="net") refreshes it before every round of the fit.

The distributional head has the same route with categorical targets (the second half of this file): dist_targets_numpy is the
specification, dist_targets_device the call (csrc/episode_dist_targets.hip: tm_episode_dist_targets), episode_dist_targets,
predict_rows_dist and fit_episodes_dist what episode_targets, predict_rows and fit_episodes are to the value net.

The harvested tree nodes (`play.py --save_nodes`, nodes.py) are a third training set, the one the online fit learns from: the
next part of this file - node_targets (csrc/node_records.hip: tm_node_targets), node_training_set and fit_nodes.  The
distributional head's harvest (`play.py --save_dist_nodes`) is the fourth, with rows that carry the node's distribution: the last
part - node_dist_targets (tm_node_dist_targets), dist_node_training_set and fit_dist_nodes.
"""
import ctypes as C
import glob
import os
from collections import namedtuple

import numpy as np
import torch

from .episodes import EPISODE_DTYPE, ROW_BYTES, STATE_DTYPE, _PART, _concat, _parts

EPS = 0.001                    # train.py:10
ROW_DW = ROW_BYTES // 4
COL = dict(episode=0, cycle=1, move=3, board=41)      # dword offsets of a row (include/tetris_mcts_hip.h)

EpisodeIndex = namedtuple("EpisodeIndex", "order seg ended final_score stem cycle episode")
EpisodeIndex.__doc__ = """order int32 [n]: rows[order[j]] is sorted by (stem, cycle, episode, move); seg int32 [n_seg + 1]: episode e is
the sorted positions seg[e] .. seg[e+1]-1; ended bool [n_seg]: the episode table has a row for it; final_score int32 [n_seg]: that
row's score (0 where censored); stem, cycle, episode int32 [n_seg]: the episode's key.  Tensors on the rows' device."""


def _row_bytes(rows, dtype, name):
    """Rows as a contiguous uint8 tensor [n, dtype.itemsize] - such a tensor already, or a numpy table of `dtype` (`name` in the
    message), which is then returned beside it (else None).  ValueError for anything else."""
    if torch.is_tensor(rows):
        if rows.dtype != torch.uint8 or rows.dim() != 2 or rows.shape[1] != dtype.itemsize or not rows.is_contiguous():
            raise ValueError("rows: a contiguous uint8 tensor [n, %d]" % dtype.itemsize)
        return rows, None
    table = np.ascontiguousarray(rows)
    if table.dtype != dtype:
        raise ValueError("rows: a table of %s, not %s" % (name, table.dtype))
    return torch.from_numpy(table.view(np.uint8).reshape(len(table), dtype.itemsize)), table


def rows_tensor(rows, device=None):
    """State rows as a uint8 tensor [n, 368]: a numpy STATE_DTYPE table (one copy, to `device`) or such a tensor already."""
    t = _row_bytes(rows, STATE_DTYPE, "STATE_DTYPE")[0]
    return t if device is None else t.to(device)


def _unsigned(x):
    """an int32 column as an int64 in [0, 2^32) that sorts as the int32 does"""
    return x.to(torch.int64) + (1 << 31)


def episode_index(rows, stem_rows=None, episodes=None, episode_stems=None):
    """Find the episodes.  rows: uint8 tensor [n, 368] on any device, in any order (rows_tensor).  stem_rows: how many rows each
    stem contributed, in the order they were concatenated (None: one stem) - ids under `.r<rank>` stems are rank-local, so the
    stem's number is part of the key (stem, cycle, episode, move).  episodes: the EPISODE_DTYPE table of the episodes that ended
    (numpy, host), episode_stems: the stem number of each of its rows (None: stem 0)."""
    dev, n = rows.device, rows.shape[0]
    if n > (1 << 31) - 64:
        raise ValueError("at most 2^31 - 64 rows")
    cols = rows.view(torch.int32).view(n, ROW_DW)
    stem_rows = [n] if stem_rows is None else [int(c) for c in stem_rows]
    if sum(stem_rows) != n or min(stem_rows, default=0) < 0:
        raise ValueError("stem_rows must add up to the %d rows" % n)
    stem = torch.repeat_interleave(torch.arange(len(stem_rows), dtype=torch.int64, device=dev),
                                   torch.tensor(stem_rows, dtype=torch.int64, device=dev), output_size=n)
    lo = (_unsigned(cols[:, COL["episode"]]) << 32) | _unsigned(cols[:, COL["move"]])
    hi = (stem << 32) | _unsigned(cols[:, COL["cycle"]])
    o1 = torch.sort(lo, stable=True).indices
    order = o1[torch.sort(hi[o1], stable=True).indices]
    key = torch.stack([stem[order], cols[:, COL["cycle"]][order].to(torch.int64), cols[:, COL["episode"]][order].to(torch.int64)], 1)
    first = torch.ones(n, dtype=torch.bool, device=dev)
    if n > 1:
        first[1:] = (key[1:] != key[:-1]).any(1)
    starts = torch.nonzero(first).flatten()
    seg = torch.cat([starts, torch.tensor([n], dtype=torch.int64, device=dev)]).to(torch.int32)
    seg_key = key[starts]
    n_seg = seg_key.shape[0]
    ended = torch.zeros(n_seg, dtype=torch.bool, device=dev)
    final = torch.zeros(n_seg, dtype=torch.int32, device=dev)
    if episodes is not None and len(episodes) and n_seg:
        if episodes.dtype != EPISODE_DTYPE:
            raise ValueError("episodes: a table of EPISODE_DTYPE, not %s" % (episodes.dtype,))
        es = np.zeros(len(episodes), np.int64) if episode_stems is None else np.asarray(episode_stems, np.int64)
        tab = torch.from_numpy(np.stack([es, episodes["cycle"].astype(np.int64), episodes["episode"].astype(np.int64)], 1)).to(dev)
        score = torch.from_numpy(np.ascontiguousarray(episodes["score"]).astype(np.int32)).to(dev)
        # one id per distinct (stem, cycle, episode) over both lists; the table's score filed under its id
        ids = torch.unique(torch.cat([seg_key, tab]), dim=0, return_inverse=True)[1]
        n_ids = int(ids.max().item()) + 1
        have = torch.zeros(n_ids, dtype=torch.bool, device=dev)
        by_id = torch.zeros(n_ids, dtype=torch.int32, device=dev)
        have[ids[n_seg:]] = True
        by_id[ids[n_seg:]] = score
        ended, final = have[ids[:n_seg]], by_id[ids[:n_seg]]
    return EpisodeIndex(order.to(torch.int32), seg, ended, final, seg_key[:, 0].to(torch.int32), seg_key[:, 1].to(torch.int32),
                        seg_key[:, 2].to(torch.int32))


def target_mode(td, lam):
    """(mode, lambda) of tm_episode_targets for the command line's --td / --td_lambda"""
    if not td:
        return 0, 0.0
    if lam is None:
        return 2, 0.0
    lam = float(lam)
    if not 0.0 <= lam <= 1.0:
        raise ValueError("lam (--td_lambda) is in [0, 1], not %r" % (lam,))
    return 1, lam


def weight_mode(weighted, weighted_mode):
    if not weighted:
        return 0
    if weighted_mode not in (0, 1, 2):
        raise ValueError("weighted_mode: 0 inverse of variance, 1 number of visits, 2 both; not %r" % (weighted_mode,))
    return int(weighted_mode) + 1


def _check_discount(mode, gamma, v_rows):
    gamma = float(gamma)
    if not 0.0 < gamma <= 1.0:
        raise ValueError("gamma is in (0, 1], not %r" % (gamma,))
    if v_rows is not None and mode == 0:
        raise ValueError("v_rows replaces the rows' values, and mode 0 (not --td) reads none")
    return gamma


def targets_numpy(rows, order, seg, tail_kind, tail_score, tail_value, mode, lam, wmode, eps=EPS, gamma=1.0, v_rows=None):
    """The specification of tm_episode_targets and tm_episode_targets_discounted in numpy (include/tetris_mcts_hip.h): fp64, ONE
    backward pass in which step t handles the t-th row from the end of every episode that has one.  rows: STATE_DTYPE table.
    gamma, v_rows (float32 [n_rows] by table row): the module docstring; at their defaults every statement computes what it
    computed without them (gamma * N is exact at 1.0).  Returns value, variance, weight (float32, by sorted position) and fault
    (0 / 1)."""
    gamma = _check_discount(mode, gamma, v_rows)
    n_rows, n = len(rows), len(order)
    if v_rows is not None:
        v_rows = np.asarray(v_rows)
        if v_rows.dtype != np.float32 or v_rows.shape != (n_rows,):
            raise ValueError("v_rows: float32 [%d], one value per table row" % n_rows)
    order, seg = np.asarray(order, np.int64), np.clip(np.asarray(seg, np.int64), 0, n_rows)
    fault = int((np.asarray(seg) != seg).any())
    ok = (order >= 0) & (order < n_rows)
    covered = np.zeros(n, bool)
    for a, b in zip(seg[:-1], seg[1:]):
        covered[a:b] = True
    fault |= int((~ok & covered).any())
    safe = np.where(ok, order, 0)
    zero = np.float32(0)
    s = np.where(ok, rows["score"][safe].astype(np.int64), 0) if n_rows else np.zeros(n, np.int64)
    v32 = np.where(ok, (rows["value"] if v_rows is None else v_rows)[safe], zero) if n_rows else np.zeros(n, np.float32)
    variance = np.where(ok, rows["variance"][safe], zero).astype(np.float32) if n_rows else np.zeros(n, np.float32)
    value = np.zeros(n, np.float32)
    first, last = seg[:-1], seg[1:]
    tail = np.asarray(tail_kind) == 1
    if mode == 2:
        value = v32.astype(np.float32)
    else:
        lam = float(lam)
        N = np.where(tail, np.asarray(tail_value, np.float64), 0.0)
        B = np.where(tail, 1.0, 0.0)
        D = np.zeros(len(tail))                                               # mode 0 with a discount: D_i = r_i + gamma D_{i+1}
        s_next = np.where(tail, np.asarray(tail_score, np.int64), 0)          # the score of the next element that exists ...
        has = tail.copy()                                                     # ... if there is one (mode 0: the end is known)
        for t in range(int((last - first).max(initial=0))):
            live = np.nonzero(last - first > t)[0]
            j = last[live] - 1 - t
            good = ok[j]
            e, j = live[good], j[good]
            if mode == 0 and gamma == 1.0:
                s_next[e] = np.where(has[e], s_next[e], s[j])                 # without a tail the last row that exists is the end
                has[e] = True
                value[j] = (s_next[e] - s[j]).astype(np.float32)
            elif mode == 0:
                d = np.where(has[e], s_next[e] - s[j], 0).astype(np.float64)
                D[e] = d + gamma * D[e]
                value[j] = D[e].astype(np.float32)
                s_next[e], has[e] = s[j], True
            else:
                d = np.where(has[e], s_next[e] - s[j], 0).astype(np.float64)
                Ne = v32[j].astype(np.float64) + lam * (gamma * N[e] + B[e] * d)
                Be = 1.0 + lam * B[e]
                value[j] = (Ne / Be).astype(np.float32)
                N[e], B[e], s_next[e], has[e] = Ne, Be, s[j], True
    one = np.float32(1)
    if wmode >= 2:
        st = rows["child_stats"][safe][:, 0, :] if n_rows else np.zeros((n, 7), np.float32)
        weight = st[:, 0].astype(np.float32)
        for a in range(1, 7):
            weight = weight + st[:, a]
    else:
        weight = np.full(n, one, np.float32)
    if wmode in (1, 3):
        with np.errstate(all="ignore"):
            weight = weight / (variance + np.float32(eps))
    value, weight = np.where(ok, value, zero), np.where(ok, weight, zero)
    value[~covered], variance[~covered], weight[~covered] = 0, 0, 0          # (the call leaves them alone: callers cover every row)
    return value.astype(np.float32), variance, weight.astype(np.float32), fault


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def targets_device(rows, order, seg, tail_kind, tail_score, tail_value, mode, lam, wmode, eps=EPS, gamma=1.0, v_rows=None):
    """tm_episode_targets on the rows' device, on the current stream; returns value, variance, weight and the fault word
    (device tensors: nothing is read back here).  tm_episode_targets_discounted is called only when gamma or v_rows (a
    contiguous float32 tensor [n_rows] on that device) is off its default: with the defaults this is the call it always was."""
    from . import _lib
    gamma = _check_discount(mode, gamma, v_rows)
    dev, n = rows.device, order.shape[0]
    if v_rows is not None and (v_rows.dtype != torch.float32 or v_rows.shape != (rows.shape[0],) or v_rows.device != dev
                               or not v_rows.is_contiguous()):
        raise ValueError("v_rows: a contiguous float32 tensor [%d] on %s, one value per table row" % (rows.shape[0], dev))
    value, variance, weight = (torch.zeros(n, dtype=torch.float32, device=dev) for _ in range(3))
    fault = torch.zeros(1, dtype=torch.int32, device=dev)
    head = (_ptr(rows), rows.shape[0], _ptr(order), _ptr(seg), seg.shape[0] - 1, _ptr(tail_kind), _ptr(tail_score), _ptr(tail_value))
    out = (_ptr(value), _ptr(variance), _ptr(weight), _ptr(fault))
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if gamma == 1.0 and v_rows is None:
            _lib.check(_lib.lib().tm_episode_targets(*head, int(mode), float(lam), int(wmode), float(eps), *out, stream),
                       "tm_episode_targets")
        else:
            _lib.check(_lib.lib().tm_episode_targets_discounted(
                *head, C.c_void_p(0) if v_rows is None else _ptr(v_rows), int(mode), float(lam), gamma, int(wmode), float(eps), *out,
                stream), "tm_episode_targets_discounted")
    return value, variance, weight, fault


def gather_states(rows, idx):
    """float32 [n, 1, 20, 10]: the boards of rows[idx] (tm_episode_gather_states on a GPU, numpy indexing on the host)"""
    n = idx.shape[0]
    if not rows.is_cuda:
        board = rows[:, 4 * COL["board"]:4 * COL["board"] + 200].view(torch.int8)
        return board[idx.to(torch.int64)].to(torch.float32).reshape(n, 1, 20, 10)
    from . import _lib
    idx = idx.to(torch.int32).contiguous()
    out = torch.empty(n, 1, 20, 10, dtype=torch.float32, device=rows.device)
    fault = torch.zeros(1, dtype=torch.int32, device=rows.device)
    with torch.cuda.device(rows.device):
        _lib.check(_lib.lib().tm_episode_gather_states(_ptr(rows), rows.shape[0], _ptr(idx), n, _ptr(out), _ptr(fault),
                                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                   "tm_episode_gather_states")
    if int(fault.item()):
        raise RuntimeError("tm_episode_gather_states: an index outside the %d rows" % rows.shape[0])
    return out


def predict_rows(model, rows, chunk=65536):
    """float32 [n_rows] value and variance of every table row's board under `model` (a Model_VV), in table order: `chunk` rows at a
    time through tm_episode_gather_states and Model_VV.inference_device - the kernels the search asks, which is what a bootstrap
    should come from.  rows: the uint8 tensor [n, 368] on the model's device.  No host synchronisation beyond those calls' own
    (gather_states reads its fault word)."""
    if chunk < 1:
        raise ValueError("chunk: at least one row, not %r" % (chunk,))
    n = rows.shape[0]
    value, variance = (torch.empty(n, dtype=torch.float32, device=rows.device) for _ in range(2))
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        boards = gather_states(rows, torch.arange(a, b, dtype=torch.int32, device=rows.device))
        model.inference_device(boards.reshape(b - a, 200).to(torch.int8), value[a:b], variance[a:b])
    return value, variance


def episode_targets(rows, index, td=False, lam=None, weighted=False, weighted_mode=0, terminal="final", censored="drop",
                    device=None, eps=EPS, gamma=1.0, v_rows=None):
    """value, variance, weight (float32 tensors by SORTED position j, i.e. of rows[index.order[j]]) and `keep` (bool: False for
    the rows `censored="drop"` leaves out).  td / lam / weighted / weighted_mode: the command line's (module docstring).
    gamma, v_rows (a float32 tensor by table row on the rows' device): the module docstring.
    device: None - where the rows are; "cpu" - the numpy statement, whatever the rows' device."""
    if terminal not in ("final", "rows"):
        raise ValueError("terminal is 'final' or 'rows', not %r" % (terminal,))
    if censored not in ("drop", "keep"):
        raise ValueError("censored is 'drop' or 'keep', not %r" % (censored,))
    mode, lam = target_mode(td, lam)
    wmode = weight_mode(weighted, weighted_mode)
    rows = rows_tensor(rows)
    on = rows.device if device is None else torch.device(device)
    tail_kind = (index.ended if terminal == "final" else torch.zeros_like(index.ended)).to(torch.uint8)
    tail_value = torch.zeros(index.ended.shape[0], dtype=torch.float32, device=tail_kind.device)
    if on.type == "cpu":
        table = rows.cpu().numpy().reshape(-1).view(STATE_DTYPE)
        value, variance, weight, fault = targets_numpy(table, index.order.cpu().numpy(), index.seg.cpu().numpy(), tail_kind.cpu().numpy(),
                                                       index.final_score.cpu().numpy(), tail_value.cpu().numpy(), mode, lam, wmode, eps,
                                                       gamma, None if v_rows is None else v_rows.cpu().numpy())
        value, variance, weight = (torch.from_numpy(x) for x in (value, variance, weight))
    else:
        rows, order, seg, tail_kind, final, tail_value = (t.to(on).contiguous() for t in (rows, index.order, index.seg, tail_kind,
                                                                                         index.final_score, tail_value))
        value, variance, weight, fault = targets_device(rows, order, seg, tail_kind, final, tail_value, mode, lam, wmode, eps, gamma,
                                                        None if v_rows is None else v_rows.to(on).contiguous())
        fault = int(fault.item())
    if fault:
        raise RuntimeError("episode_targets: the index names rows outside the %d given" % rows.shape[0])
    return value, variance, weight, _kept(index, mode, censored, value.device)


def choose_stems(paths, last_nfiles=1):
    """train.py:68-77 over stems: every path is a glob pattern (or a stem, or a directory of shards); what it matches is mapped to
    stems - one "file" is one stem, whatever the number of its parts - which are ordered by the time their newest State shard was
    written; the last `last_nfiles` are kept (<= 0: all)."""
    if isinstance(paths, (str, os.PathLike)):
        paths = [paths]
    shard = ".part[0-9][0-9][0-9][0-9][0-9].npy"
    stems = []
    for p in map(str, paths):
        found = []
        for f in glob.glob(p) or glob.glob(glob.escape(p) + shard):
            found += glob.glob(os.path.join(glob.escape(f), "*" + shard)) if os.path.isdir(f) else [f]
        stems += [_PART.sub("", f).removesuffix(".episodes") for f in found if _PART.search(f)]
    stems = [s for s in dict.fromkeys(stems) if _parts(s)]
    stems.sort(key=lambda s: (max(os.path.getmtime(f) for f in _parts(s)), s))
    if last_nfiles > 0:
        stems = stems[-last_nfiles:]
    if not stems:
        raise RuntimeError("list_of_data is empty.")
    return stems


def load_stems(stems):
    """the State rows of the stems one after the other in file order, how many each has, their episode tables as one and the stem
    number of each of its rows"""
    tables = [[np.load(f) for f in _parts(s)] for s in stems]
    ep = [_concat([np.load(f) for f in _parts(s, episodes=True)], EPISODE_DTYPE) for s in stems]
    rows = _concat([t for ts in tables for t in ts], STATE_DTYPE)
    return (rows, [sum(len(t) for t in ts) for ts in tables], _concat(ep, EPISODE_DTYPE),
            np.concatenate([np.full(len(e), i, np.int64) for i, e in enumerate(ep)] + [np.zeros(0, np.int64)]))


def validation_fraction(n, n_val):
    """a fraction for which train_data's own split, int(n * fraction), is n_val exactly"""
    if n_val == 0 or n == 0:
        return 0.0
    f = (n_val + 0.5) / n
    assert int(n * f) == n_val, (n, n_val)
    return f


def _split(index, keep, validation, val_mode, val_episodes, val_set_size, val_set_size_max, generator, dev):
    """training_set's split (train.py:148-174): the sorted positions that train followed by the ones held out, and how many the
    latter are.  keep: bool by sorted position, the rows that take part at all."""
    n_all = keep.shape[0]
    held = torch.zeros(n_all, dtype=torch.bool, device=dev)
    if validation and val_mode == 1 and val_episodes > 0:
        length = (index.seg[1:] - index.seg[:-1]).to(torch.int64)
        held = torch.repeat_interleave(index.episode < val_episodes + 1, length, output_size=n_all) & keep
    pos = torch.nonzero(keep & ~held).flatten()
    val = torch.nonzero(held).flatten()

    def draw(k):
        g = generator.device if generator is not None else dev
        return torch.randperm(k, generator=generator, device=g).to(dev)
    if validation and val_mode == 0:
        n = pos.shape[0]
        n_val = 0 if val_set_size <= 0 else n if val_set_size >= 1 else int(n * val_set_size)
        if val_set_size_max > 0 and 0 < val_set_size < 1:
            n_val = min(n_val, val_set_size_max)
        chosen = torch.zeros(n, dtype=torch.bool, device=dev)
        chosen[draw(n)[:n_val]] = True
        pos, val = pos[~chosen], pos[chosen]
    elif validation and val_mode == 1:
        if val_set_size_max > 0 and val.shape[0] > val_set_size_max:
            val = val[torch.sort(draw(val.shape[0])[:val_set_size_max]).values]
    elif validation:
        raise ValueError("val_mode: 0 random, 1 episodic; not %r" % (val_mode,))
    return torch.cat([pos, val]), int(val.shape[0])


def training_set(paths, td=False, lam=None, weighted=False, weighted_mode=0, terminal="final", censored="drop", last_nfiles=1,
                 validation=False, val_mode=0, val_episodes=0, val_set_size=0.05, val_set_size_max=-1, generator=None,
                 device="cuda", eps=EPS, gamma=1.0, v_rows=None):
    """data = [states [n,1,20,10], values [n,1], variances [n,1], weights [n,1]] (float32 on `device`), training rows first and
    the held-out rows last - the layout train_data splits - and a dict with n_val, validation_fraction (train_data's
    int(n * fraction) is n_val exactly), n_train, the stems and the row counts, and what a refresh of the values needs without
    reading the files again: `rows` (the table on `device`), `index` (episode_index of it) and `sel` (the sorted positions of the
    n rows of `data`, in its order).  gamma, v_rows: episode_targets'.  Files as train.py --data_paths / --last_nfiles
    chooses them (choose_stems).  validation: train.py:148-174 - val_mode 0 holds out a random int(n * val_set_size) rows (at most
    val_set_size_max if that is positive; `generator`: a torch.Generator for the draw), val_mode 1 whole episodes with
    episode < val_episodes + 1 (a random val_set_size_max of their rows if that is positive)."""
    stems = choose_stems(paths, last_nfiles)
    table, stem_rows, episodes, episode_stems = load_stems(stems)
    dev = torch.device(device)
    rows = rows_tensor(table, dev)
    index = episode_index(rows, stem_rows, episodes, episode_stems)
    value, variance, weight, keep = episode_targets(rows, index, td=td, lam=lam, weighted=weighted, weighted_mode=weighted_mode,
                                                    terminal=terminal, censored=censored, eps=eps, gamma=gamma, v_rows=v_rows)
    n_all = keep.shape[0]
    sel, n_val = _split(index, keep, validation, val_mode, val_episodes, val_set_size, val_set_size_max, generator, dev)
    n = int(sel.shape[0])
    if n == 0:
        raise RuntimeError("no rows to train on: every episode of %s is censored (censored='keep' takes them as they are)" % (stems,))
    states = gather_states(rows, index.order[sel])
    data = [states] + [x[sel].reshape(n, 1) for x in (value, variance, weight)]
    return data, dict(n=n, n_val=n_val, n_train=n - n_val, validation_fraction=validation_fraction(n, n_val), stems=stems,
                      n_rows=n_all, episodes=int(index.ended.shape[0]), censored_episodes=int((~index.ended).sum().item()),
                      rows=rows, index=index, sel=sel)


def _iterations(max_iters, iters_per_val, n_train):
    """(iters, the iters_per_val keyword of train_data if one was given): either may be a function - max_iters of the number of
    training rows, iters_per_val of the iterations"""
    iters = int(max_iters(n_train)) if callable(max_iters) else int(max_iters)
    extra = {}
    if iters_per_val is not None:
        extra["iters_per_val"] = int(iters_per_val(iters)) if callable(iters_per_val) else int(iters_per_val)
    return iters, extra


def _round_iters(iters, r, rounds):
    """the iterations of round r of `rounds`: iters // rounds each, the remainder to the last"""
    return iters // rounds + (iters % rounds if r == rounds - 1 else 0)


def _save_on_rank0(model):
    from . import dist as tdist
    if tdist.rank() == 0:                  # replicas are identical: one checkpoint file, written by rank 0
        model.save(verbose=False)


def _consolidate(model, data, n_train, res, penalised, **fisher):
    """The end of a fit with ewc_lambda: the model's compute_fisher (Model_VV's or Model_Dist's; fisher: its state_format) over
    the training rows of `data`, whose last array holds the weights, with the weights as the fit used them - train_data fits with
    weighted=True on the weights divided by their mean over ALL rows: the same per-sample losses here -, the checkpoint, and
    `res` with the ewc dict."""
    w = data[-1] / data[-1].mean()
    model.compute_fisher([d[:n_train] for d in data[:-1]] + [w[:n_train]], weighted=True, **fisher)
    _save_on_rank0(model)
    return dict(res, ewc=dict(penalised=bool(penalised), fisher_rows=int(n_train)))


def fit_episodes(model, paths, batch_size=32, max_iters=100000, iters_per_val=None, early_stopping=False,
                 early_stopping_patience=10, fit_backend="torch", validation_backend="torch", gamma=1.0, bootstrap="recorded",
                 bootstrap_rounds=1, on_round=None, ewc_lambda=None, **options):
    """training_set(paths, gamma=gamma, **options) on the model's device, then model.train_data on it; returns what train_data
    returns plus `rounds`: one dict per round with iters, best_validation and graph_replay.
    max_iters and iters_per_val may be functions of the number of training rows (train.py computes its iterations from it).

    bootstrap="recorded" (one round): the v_k of the lambda-return are the recorded root values - one training_set, one
    train_data.  bootstrap="net" (needs td=True and a lam: mode 2 would fit the net to its own output, and mode 0 bootstraps
    nothing) takes them from `model` itself and refreshes them: the iterations are split into `bootstrap_rounds` parts
    (iters // R each, the remainder to the last), and before each part the values of ALL selected rows, held-out rows included,
    are recomputed - predict_rows under the model as it stands, episode_targets with those v_rows - and written into the same
    data[1] tensor.  The split, the variances and the weights are computed once.  Early stopping and the best-weights reload act
    within a round; the optimiser's state persists across rounds, as it does across online fits.  A prediction that is not
    finite raises RuntimeError before a target is computed from it (one .item() a round).
    on_round(r, data, v_rows), r = 0 .. R-1, is called before each round's train_data with the tensors in use (v_rows: None
    with bootstrap="recorded").

    ewc_lambda (None: off; needs fit_backend="hip"): elastic weight consolidation.  Every round's train_data gets it and
    penalises against the Fisher and anchor the model holds (a loaded checkpoint's), if any.  After the last round
    Model_VV.compute_fisher runs over the TRAINING rows (the held-out tail excluded) with that round's targets and the weights
    as the fit used them, the new Fisher and anchor replace the model's, and rank 0 writes the checkpoint.  The result gains
    ewc = dict(penalised: whether the fits were penalised, fisher_rows: the rows the new Fisher averages over)."""
    from .model import Model_VV
    if not isinstance(model, Model_VV):
        raise TypeError("fit_episodes fits a Model_VV: the reference has no episode target for a distribution (%s)"
                        % type(model).__name__)
    rounds = int(bootstrap_rounds)
    if bootstrap not in ("recorded", "net"):
        raise ValueError("bootstrap is 'recorded' or 'net', not %r" % (bootstrap,))
    if rounds < 1:
        raise ValueError("bootstrap_rounds: at least 1, not %r" % (bootstrap_rounds,))
    if bootstrap == "net" and (not options.get("td") or options.get("lam") is None):
        raise ValueError("bootstrap='net' refreshes the v of the lambda-return: it needs td=True and a lam")
    if bootstrap == "recorded" and rounds > 1:
        raise ValueError("bootstrap='recorded' with %d rounds: nothing would change between them" % rounds)
    _check_discount(target_mode(options.get("td", False), options.get("lam"))[0], gamma, None)
    if ewc_lambda is not None and fit_backend != "hip":
        raise ValueError("ewc_lambda needs fit_backend='hip', not %r" % (fit_backend,))
    data, info = training_set(paths, device=model.device, gamma=gamma, **options)
    iters, extra = _iterations(max_iters, iters_per_val, info["n_train"])
    if rounds > 1 and iters < rounds:
        raise ValueError("%d iterations do not make %d rounds" % (iters, rounds))
    targets = {k: options[k] for k in ("td", "lam", "weighted", "weighted_mode", "terminal", "censored", "eps") if k in options}
    done = []
    if ewc_lambda is not None:
        extra["ewc_lambda"] = ewc_lambda
    penalised = ewc_lambda is not None and model.fisher is not None
    for r in range(rounds):
        v_rows = None
        if bootstrap == "net":
            model.training(False)
            v_rows = predict_rows(model, info["rows"])[0]
            if not bool(torch.isfinite(v_rows).all().item()):
                raise RuntimeError("fit_episodes: round %d: the net's values of the recorded boards are not all finite" % r)
            value = episode_targets(info["rows"], info["index"], gamma=gamma, v_rows=v_rows, **targets)[0]
            data[1].copy_(value[info["sel"]].reshape(-1, 1))
        if on_round is not None:
            on_round(r, data, v_rows)
        res = model.train_data(data, batch_size=batch_size, max_iters=_round_iters(iters, r, rounds),
                               validation_fraction=info["validation_fraction"], shuffle=False, early_stopping=early_stopping,
                               early_stopping_patience=early_stopping_patience, fit_backend=fit_backend,
                               validation_backend=validation_backend, **extra)
        done.append(dict(iters=res["iters"], best_validation=res["best_validation"], graph_replay=res["graph_replay"]))
    if ewc_lambda is not None:
        res = _consolidate(model, data, info["n_train"], res, penalised)
    return dict(res, rounds=done)


# ---- the distributional head: categorical targets (csrc/episode_dist_targets.hip: tm_episode_dist_targets) ----------------------
#
# What the search's distributional backup does along a trace - shift a distribution by the score gained, mix it into the node
# above - done along the moves played.  atoms K over [vmin, vmax), delta = (vmax - vmin) / K in double.  The shift S_c(p) by an
# integer score difference c >= 0 (tm_distpy_shift's rule): bs = c / delta, n = floor(bs), f = bs - n; source atom a gives
# p[a] (1 - f) to lb = min(a + n, K-1) and p[a] f to min(lb + 1, K-1).  An episode's series is its rows in move order and, where it
# ended (terminal="final"), one tail element: its final score with all mass in atom 0, the search's v_dummy.
#     mode 0  not --td                 target_i = S_{s_end - s_i}(e_0)                                       (Monte Carlo)
#     mode 1  --td --td_lambda L       target_i = sum_{k<=m} L^k S_{s_{i+k} - s_i}(P_{i+k}) / sum_{k<=m} L^k,  m = min(horizon, what follows i)
# P comes from `p_rows`, float32 [n_rows, >= K] by TABLE row: the head's own output (predict_rows_dist), or the root distributions
# recorded beside the rows (recorded_root_dists: play.py --save_root_dists, reanalyse.py --root_dists).  There is no mode 2: at
# lambda = 0 mode 1 copies p_rows, which for recorded distributions is the value net's mode 2.  There is no discount (the distributional backup has none).  Two interpolating shifts composed are not the
# shift by the sum, so nothing is carried from one target to the next: every term is one exact shift over a bounded horizon.

def dist_target_mode(td, lam):
    """(mode, lambda) of tm_episode_dist_targets for the command line's --td / --td_lambda"""
    if not td:
        return 0, 0.0
    if lam is None:
        raise ValueError("td without a lam: the rows record no distribution to fit (the value net's mode 2 has no counterpart)")
    lam = float(lam)
    if not 0.0 <= lam <= 1.0:
        raise ValueError("lam (--td_lambda) is in [0, 1], not %r" % (lam,))
    return 1, lam


def _check_dist(atoms, vmin, vmax, mode, horizon, p_rows, n_rows):
    atoms, vmin, vmax = int(atoms), float(vmin), float(vmax)
    if not 1 <= atoms <= 64:
        raise ValueError("atoms: 1 .. 64, not %r" % (atoms,))
    if not (np.isfinite(vmin) and np.isfinite(vmax) and vmax > vmin and np.isfinite(vmax - vmin)):
        raise ValueError("[vmin, vmax): two finite bounds with vmin < vmax, not %r, %r" % (vmin, vmax))
    if mode not in (0, 1):
        raise ValueError("mode: 0 Monte Carlo, 1 the truncated lambda-return; not %r" % (mode,))
    if int(horizon) < 0:
        raise ValueError("horizon: at least 0, not %r" % (horizon,))
    if mode == 1 and (p_rows is None or p_rows.dtype not in (np.float32, torch.float32) or len(p_rows.shape) != 2
                      or p_rows.shape[0] != n_rows or p_rows.shape[1] < atoms):
        raise ValueError("p_rows: float32 [%d, >= %d], one distribution per table row" % (n_rows, atoms))
    return atoms, (vmax - vmin) / atoms


def _shift_terms(P, suf, el, n, f, K):
    """S(P[el]) in gather form, fp64 [len(el), K]: atom b < K-1 = P[b-n] (1-f) + P[b-n-1] f, the top atom = suf[max(K-1-n, 0)] +
    P[K-2-n] f.  P: [., K+1] with a last column of zeros (what a source below atom 0 reads), suf: [., K] its sums from the top."""
    b = np.arange(K - 1)
    src = b[None, :] - n[:, None]
    row = el[:, None]
    t = np.empty((len(el), K))
    t[:, :K - 1] = P[row, np.where(src >= 0, src, K)] * (1.0 - f)[:, None] + P[row, np.where(src >= 1, src - 1, K)] * f[:, None]
    top = K - 1 - n
    t[:, K - 1] = suf[el, np.maximum(top, 0)] + P[el, np.where(top >= 1, top - 1, K)] * f
    return t


def _shift_of(c, delta, K):
    """(n, f, a score fell) of int64 score differences; a negative one is taken as 0"""
    fell = bool((c < 0).any())
    bs = np.maximum(c, 0).astype(np.float64) / delta
    fl = np.floor(bs)
    return np.minimum(fl, K).astype(np.int64), bs - fl, fell


def dist_targets_numpy(rows, order, seg, tail_kind, tail_score, atoms, vmin, vmax, mode, lam, horizon, wmode, eps=EPS, p_rows=None):
    """The specification of tm_episode_dist_targets in numpy (include/tetris_mcts_hip.h): fp64, all targets at once, one pass per
    k.  rows: STATE_DTYPE table; seg does not fall.  Returns target float32 [n, atoms] and weight float32 [n] by sorted position,
    and the fault word (bit 0: an order entry that is not a row, or a seg entry outside the table; bit 1: a score that fell)."""
    n_rows, n = len(rows), len(order)
    K, delta = _check_dist(atoms, vmin, vmax, mode, horizon, p_rows, n_rows)
    order, seg0 = np.asarray(order, np.int64), np.asarray(seg, np.int64)
    seg = np.clip(seg0, 0, n_rows)
    fault = int((seg0 != seg).any())
    ok = (order >= 0) & (order < n_rows)
    n_seg = len(seg) - 1
    ep = np.full(n, -1, np.int64)
    for e in range(n_seg):
        ep[seg[e]:seg[e + 1]] = e
    covered = ep >= 0
    fault |= int((~ok & covered).any())
    safe = np.where(ok, order, 0)
    zero, one = np.float32(0), np.float32(1)
    if wmode >= 2:
        st = rows["child_stats"][safe][:, 0, :] if n_rows else np.zeros((n, 7), np.float32)
        weight = st[:, 0].astype(np.float32)
        for a in range(1, 7):
            weight = weight + st[:, a]
    else:
        weight = np.full(n, one, np.float32)
    if wmode in (1, 3):
        variance = rows["variance"][safe].astype(np.float32) if n_rows else np.zeros(n, np.float32)
        with np.errstate(all="ignore"):
            weight = weight / (variance + np.float32(eps))
    weight = np.where(ok & covered, weight, zero).astype(np.float32)
    target = np.zeros((n, K), np.float32)
    pos = np.nonzero(ok & covered)[0]                                     # ascending: episode by episode, in move order
    if not len(pos):
        return target, weight, fault
    # the series of all episodes one after the other: the rows that exist, then the tail
    tail = np.asarray(tail_kind)[:n_seg] == 1
    cnt = np.bincount(ep[pos], minlength=n_seg)
    off = np.concatenate([[0], np.cumsum(cnt + tail)])
    first = np.concatenate([[0], np.cumsum(cnt)])[:-1]
    x = off[ep[pos]] + (np.arange(len(pos)) - first[ep[pos]])             # the element that position is
    end = off[ep[pos] + 1]                                                # one past its series' last element
    S = np.zeros(off[-1], np.int64)
    S[x] = rows["score"][order[pos]].astype(np.int64)
    S[off[1:][tail] - 1] = np.asarray(tail_score, np.int64)[:n_seg][tail]
    if mode == 0:
        has = (cnt + tail) > 0
        s_end = np.zeros(n_seg, np.int64)
        s_end[has] = S[off[1:][has] - 1]                                  # the tail's score; without a tail the last row's
        nn, f, fell = _shift_of(s_end[ep[pos]] - S[x], delta, K)
        e0 = np.zeros((1, K + 1))
        e0[0, 0] = 1.0
        target[pos] = _shift_terms(e0, e0[:, :K], np.zeros(len(pos), np.int64), nn, f, K).astype(np.float32)
        return target, weight, fault | (2 if fell else 0)
    P = np.zeros((off[-1], K + 1))
    P[x, :K] = np.asarray(p_rows)[order[pos], :K].astype(np.float64)      # (the padding atoms are never read)
    P[off[1:][tail] - 1, 0] = 1.0
    suf = np.cumsum(P[:, K - 1::-1], axis=1)[:, ::-1]                     # p[K-1] + p[K-2] + .., added in that order
    lam = float(lam)
    H = 0 if lam == 0.0 else int(horizon)
    acc, wsum, w = np.zeros((len(pos), K)), np.zeros(len(pos)), np.ones(len(pos))
    fell = False
    for k in range(H + 1):
        act = np.nonzero(x + k < end)[0]
        if not len(act):
            break
        nn, f, fell_k = _shift_of(S[x[act] + k] - S[x[act]], delta, K)
        fell |= fell_k
        acc[act] = acc[act] + w[act][:, None] * _shift_terms(P, suf, x[act] + k, nn, f, K)
        wsum[act] = wsum[act] + w[act]
        w[act] = w[act] * lam
    target[pos] = (acc / wsum[:, None]).astype(np.float32)
    return target, weight, fault | (2 if fell else 0)


def dist_targets_device(rows, order, seg, tail_kind, tail_score, atoms, vmin, vmax, mode, lam, horizon, wmode, eps=EPS, p_rows=None):
    """tm_episode_dist_targets on the rows' device, on the current stream; returns target (float32 [n, 64]: the atoms first, the
    padding zero), weight and the fault word (device tensors: nothing is read back here).  p_rows: a float32 tensor [n_rows, >=
    atoms] on that device with contiguous rows (mode 1)."""
    from . import _lib
    dev, n = rows.device, order.shape[0]
    K, _ = _check_dist(atoms, vmin, vmax, mode, horizon, p_rows, rows.shape[0])
    if p_rows is not None and mode == 1 and (p_rows.device != dev or p_rows.stride(1) != 1):
        raise ValueError("p_rows: on %s, its rows contiguous" % (dev,))
    target = torch.zeros(n, 64, dtype=torch.float32, device=dev)
    weight = torch.zeros(n, dtype=torch.float32, device=dev)
    fault = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().tm_episode_dist_targets(
            _ptr(rows), rows.shape[0], _ptr(order), _ptr(seg), seg.shape[0] - 1, _ptr(tail_kind), _ptr(tail_score),
            C.c_void_p(0) if mode == 0 else _ptr(p_rows), 0 if mode == 0 else p_rows.stride(0), K, float(vmin), float(vmax), int(mode),
            float(lam), int(horizon), int(wmode), float(eps), _ptr(target), target.stride(0), _ptr(weight), _ptr(fault),
            C.c_void_p(torch.cuda.current_stream().cuda_stream)), "tm_episode_dist_targets")
    return target, weight, fault


def _kept(index, mode, censored, dev):
    """bool by sorted position: False for the rows of the censored episodes that mode 0 with censored="drop" leaves out"""
    n, n_seg = index.order.shape[0], index.ended.shape[0]
    if mode == 0 and censored == "drop" and n_seg:
        length = (index.seg[1:] - index.seg[:-1]).to(torch.int64)
        return torch.repeat_interleave(index.ended, length, output_size=n).to(dev)
    return torch.ones(n, dtype=torch.bool, device=dev)


def episode_dist_targets(rows, index, td=False, lam=None, horizon=64, atoms=50, vmin=0.0, vmax=5000.0, weighted=False,
                         weighted_mode=0, terminal="final", censored="drop", p_rows=None, device=None, eps=EPS):
    """target (float32 [n, atoms]), weight (float32 [n]) by SORTED position j, i.e. of rows[index.order[j]], and `keep` (bool:
    False for the rows `censored="drop"` leaves out).  td / lam: dist_target_mode; horizon: the terms after the row's own that a
    mode-1 target takes at most; p_rows: the distributions by table row (mode 1), a float32 tensor [n_rows, >= atoms].
    device: None - where the rows are; "cpu" - the numpy statement, whatever the rows' device.  Raises RuntimeError on a set
    fault word (one .item())."""
    if terminal not in ("final", "rows"):
        raise ValueError("terminal is 'final' or 'rows', not %r" % (terminal,))
    if censored not in ("drop", "keep"):
        raise ValueError("censored is 'drop' or 'keep', not %r" % (censored,))
    mode, lam = dist_target_mode(td, lam)
    wmode = weight_mode(weighted, weighted_mode)
    rows = rows_tensor(rows)
    on = rows.device if device is None else torch.device(device)
    tail_kind = (index.ended if terminal == "final" else torch.zeros_like(index.ended)).to(torch.uint8)
    if on.type == "cpu":
        table = rows.cpu().numpy().reshape(-1).view(STATE_DTYPE)
        target, weight, fault = dist_targets_numpy(table, index.order.cpu().numpy(), index.seg.cpu().numpy(), tail_kind.cpu().numpy(),
                                                   index.final_score.cpu().numpy(), atoms, vmin, vmax, mode, lam, horizon, wmode, eps,
                                                   None if p_rows is None else p_rows.cpu().numpy())
        target, weight = torch.from_numpy(target), torch.from_numpy(weight)
    else:
        rows, order, seg, tail_kind, final = (t.to(on).contiguous() for t in (rows, index.order, index.seg, tail_kind, index.final_score))
        target, weight, fault = dist_targets_device(rows, order, seg, tail_kind, final, atoms, vmin, vmax, mode, lam, horizon, wmode,
                                                    eps, None if p_rows is None else p_rows.to(on))
        target, fault = target[:, :int(atoms)], int(fault.item())
    if fault & 1:
        raise RuntimeError("episode_dist_targets: the index names rows outside the %d given" % rows.shape[0])
    if fault & 2:
        raise RuntimeError("episode_dist_targets: a score falls inside an episode: these are not recorded rows in move order")
    return target, weight, _kept(index, mode, censored, target.device)


def predict_rows_dist(model, rows, chunk=65536):
    """float32 [n_rows, 64]: the distribution of every table row's board under `model` (a Model_Dist) in table order, the atoms
    first - `chunk` rows at a time through tm_episode_gather_states and Model_Dist.inference_device, the kernels the search asks.
    rows: the uint8 tensor [n, 368] on the model's device."""
    if chunk < 1:
        raise ValueError("chunk: at least one row, not %r" % (chunk,))
    n = rows.shape[0]
    out = torch.zeros(n, 64, dtype=torch.float32, device=rows.device)
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        boards = gather_states(rows, torch.arange(a, b, dtype=torch.int32, device=rows.device))
        model.inference_device(boards.reshape(b - a, 200).to(torch.int8), out[a:b])
    return out


def recorded_root_dists(stems, atoms, vmin, vmax, n_rows=None):
    """float32 [n_rows, 64] by TABLE row (load_stems' order): the root distributions recorded beside the State shards of `stems`
    (episodes.RootDistLoader pairs them row by row).  ValueError, before anything is computed from them, for a stem without
    root-distribution shards or sidecar, a sidecar that is not (atoms, vmin, vmax) and a recorded atom that is not finite or is
    negative."""
    from .episodes import RootDistLoader, rootdist_stem
    from .nodes import head_file
    for s in stems:
        if not _parts(rootdist_stem(s)):
            raise ValueError("%s has no root-distribution shards (%s.partNNNNN.npy): bootstrap='search' fits what play.py --agent_type "
                             "DistValueSim --save --save_root_dists or reanalyse.py --root_dists recorded" % (s, rootdist_stem(s)))
    from .nodes import load_head
    loaders = [RootDistLoader([s], positions=False) for s in stems]        # (stem by stem: the table's order is load_stems')
    head, want = load_head([rootdist_stem(s) for s in stems]), (int(atoms), float(vmin), float(vmax))
    if head != want:
        raise ValueError("the root distributions of %s were recorded by a head of (atoms, vmin, vmax) = %s (%s), the model and the "
                         "range given are %s" % (list(stems), head, head_file(rootdist_stem(stems[0])), want))
    files = [f for L in loaders for f in L.dist_files]
    counts = [c for L in loaders for c in L.counts]
    d = np.concatenate([np.ascontiguousarray(L.dists["dist"], dtype=np.float32).reshape(L.length, 64) for L in loaders])
    if n_rows is not None and len(d) != n_rows:
        raise ValueError("%d root distributions for %d State rows" % (len(d), n_rows))
    bad = ~(np.isfinite(d[:, :want[0]]) & (d[:, :want[0]] >= 0)).all(axis=1)
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        j = int(np.searchsorted(np.cumsum(counts), i, side="right"))
        raise ValueError("%s: row %d holds an atom that is not finite or is negative: not a recorded distribution"
                         % (files[j], i - int(sum(counts[:j]))))
    return d


def fit_episodes_dist(model, paths, batch_size=32, max_iters=100000, iters_per_val=None, early_stopping=False,
                      early_stopping_patience=10, fit_backend=None, validation_backend="torch", td=False, lam=None, horizon=64,
                      vmin=0.0, vmax=5000.0, rounds=1, on_round=None, weighted=False, weighted_mode=0, terminal="final",
                      censored="drop", last_nfiles=1, validation=False, val_mode=0, val_episodes=0, val_set_size=0.05,
                      val_set_size_max=-1, generator=None, eps=EPS, bootstrap="net", ewc_lambda=None):
    """fit_episodes for the distributional head: the recorded episodes of `paths` (choose_stems) -> categorical targets over the
    model's atoms on [vmin, vmax) (episode_dist_targets on the model's device) -> Model_Dist.train_data -> the checkpoint
    (Model_Dist.save, after every round).  Returns what train_data returns plus `rounds`, as fit_episodes does.
    Not td: mode 0, the realised return as a distribution; computed once (rounds must be 1).  td with a lam: mode 1; the
    distributions inside it are the MODEL's own, over every recorded board (predict_rows_dist), refreshed before each of `rounds`
    parts of the iterations (iters // rounds each, the remainder to the last) - the targets of all selected rows, held-out rows
    included, are recomputed and written into the same data[1] tensor, as fit_episodes(bootstrap="net") does.  The split
    (training_set's), the boards and the weights are computed once.  A prediction that is not finite raises RuntimeError before a
    target is computed from it, and so does a set fault word.
    bootstrap="search" (with td): the distributions inside the target are the ones the SEARCH backed up into the roots, recorded
    beside the rows (recorded_root_dists; the `rootdist` shards beside the chosen stems), loaded once; nothing is predicted and
    rounds must be 1.  lam=None then means lambda = 0: the target is the recorded distribution itself, bit for bit - the
    counterpart of the value net's mode 2.  A stem without such shards, a sidecar that is not the model's atoms and [vmin, vmax),
    and a recorded atom that is not finite or is negative are a ValueError before any target is computed.
    fit_backend: None - "hip_dist" on a GPU, "torch" on the host.  max_iters / iters_per_val may be functions, as in fit_episodes.
    on_round(r, data, p_rows), r = 0 .. rounds-1, is called before each round's train_data with the tensors in use (p_rows: None
    in mode 0).
    ewc_lambda (None: off; needs fit_backend="hip_dist"): elastic weight consolidation, as in fit_episodes.  Every round is
    penalised against the Fisher and anchor the model holds (a loaded checkpoint's), if any.  After the last round
    Model_Dist.compute_fisher runs over the TRAINING rows (the held-out tail excluded) with that round's targets and the weights
    as the fit used them, the new Fisher and anchor replace the model's, and rank 0 writes the checkpoint once more.  The result
    gains ewc = dict(penalised, fisher_rows)."""
    from .model_distributional import Model_Dist
    if not isinstance(model, Model_Dist):
        raise TypeError("fit_episodes_dist fits a Model_Dist: the value net's episode targets are fit_episodes' (%s)"
                        % type(model).__name__)
    if bootstrap not in ("net", "search"):
        raise ValueError("bootstrap is 'net' (the head's own distributions) or 'search' (the recorded root distributions), not %r"
                         % (bootstrap,))
    if bootstrap == "search":
        if not td:
            raise ValueError("bootstrap='search' puts the recorded root distributions inside the td target: it needs td=True")
        if lam is None:
            lam = 0.0                          # the recorded distribution itself
    mode, lam_ = dist_target_mode(td, lam)
    rounds = int(rounds)
    if rounds < 1:
        raise ValueError("rounds: at least 1, not %r" % (rounds,))
    if bootstrap == "search" and rounds > 1:
        raise ValueError("%d rounds with bootstrap='search': recorded distributions do not change between them" % rounds)
    if mode == 0 and rounds > 1:
        raise ValueError("%d rounds without td: the Monte Carlo targets do not change between them" % rounds)
    dev = torch.device(model.device)
    _check_dist(model.atoms, vmin, vmax, 0, horizon, None, 0)
    if fit_backend is None:
        fit_backend = "hip_dist" if dev.type == "cuda" else "torch"
    if ewc_lambda is not None and fit_backend != "hip_dist":
        raise ValueError("ewc_lambda needs fit_backend='hip_dist', not %r" % (fit_backend,))
    stems = choose_stems(paths, last_nfiles)
    table, stem_rows, episodes, episode_stems = load_stems(stems)
    recorded = None
    if bootstrap == "search":
        recorded = torch.from_numpy(recorded_root_dists(stems, model.atoms, vmin, vmax, len(table))).to(dev)
    rows = rows_tensor(table, dev)
    index = episode_index(rows, stem_rows, episodes, episode_stems)
    sel, n_val = _split(index, _kept(index, mode, censored, dev), validation, val_mode, val_episodes, val_set_size, val_set_size_max,
                        generator, dev)
    n = int(sel.shape[0])
    if n == 0:
        raise RuntimeError("no rows to train on: every episode of %s is censored (censored='keep' takes them as they are)" % (stems,))
    states = torch.zeros(n, 1, 22, 10, dtype=torch.float32, device=dev)
    states[:, :, 2:, :] = gather_states(rows, index.order[sel])              # the head's 22 rows: two empty ones on top
    iters, extra = _iterations(max_iters, iters_per_val, n - n_val)
    if rounds > 1 and iters < rounds:
        raise ValueError("%d iterations do not make %d rounds" % (iters, rounds))
    options = dict(td=td, lam=lam, horizon=horizon, atoms=model.atoms, vmin=vmin, vmax=vmax, weighted=weighted,
                   weighted_mode=weighted_mode, terminal=terminal, censored=censored, eps=eps)
    data, done = None, []
    if ewc_lambda is not None:
        extra["ewc_lambda"] = ewc_lambda
    penalised = ewc_lambda is not None and model.fisher is not None
    for r in range(rounds):
        p_rows = None
        if recorded is not None:
            p_rows = recorded
        elif mode == 1:
            model.training(False)
            p_rows = predict_rows_dist(model, rows)
            if not bool(torch.isfinite(p_rows[:, :model.atoms]).all().item()):
                raise RuntimeError("fit_episodes_dist: round %d: the head's distributions of the recorded boards are not all finite" % r)
        if data is None or mode == 1:
            target, weight, _ = episode_dist_targets(rows, index, p_rows=p_rows, **options)
            if data is None:
                data = [states, target[sel].contiguous(), weight[sel].reshape(n, 1)]
            else:
                data[1].copy_(target[sel])
        if on_round is not None:
            on_round(r, data, p_rows)
        res = model.train_data(data, fit_backend=fit_backend, batch_size=batch_size, max_iters=_round_iters(iters, r, rounds),
                               validation_fraction=validation_fraction(n, n_val), shuffle=False, early_stopping=early_stopping,
                               early_stopping_patience=early_stopping_patience, validation_backend=validation_backend, **extra)
        _save_on_rank0(model)
        done.append(dict(iters=res["iters"], best_validation=res["best_validation"], graph_replay=res["graph_replay"]))
    if ewc_lambda is not None:
        res = _consolidate(model, data, n - n_val, res, penalised)
    return dict(res, rounds=done)


# ---- node records: the harvested tree nodes as a training set (csrc/node_records.hip: tm_node_targets) ---------------------------
#
# `play.py --save_nodes` leaves NODE_DTYPE rows (nodes.py): the tuples the online fit trains on - packed observation, the search's
# value and variance, the visits.  A node has no return and no episode: the target is the search's own value (the value net's mode
# 2), the held-out rows are a random draw, and the fit reads the packed observations as they are (state_format="packed").

def _node_rows(rows, dtype, name, device):
    """What the two target functions of node rows take in: the rows as a uint8 tensor [n, ROW] (_row_bytes) on the device `on`
    the targets are computed on - `device`; None: the tensor's own, "cuda" for a table - and, where that is the host, the table
    of `dtype` the numpy statement reads (else None).  Returns rows, table, on."""
    on = torch.device(device) if device is not None else (rows.device if torch.is_tensor(rows) else torch.device("cuda"))
    rows, table = _row_bytes(rows, dtype, name)
    if on.type != "cpu":
        return rows.to(on), None, on
    return rows, rows.cpu().numpy().reshape(-1).view(dtype) if table is None else table, on


def node_targets(rows, weighted=False, weighted_mode=0, eps=EPS, device=None):
    """obs (int32 [n,12]), value, variance, weight (float32 [n]) of node rows: tm_node_targets on the rows' device, on the current
    stream (`rows`: a NODE_DTYPE table or a contiguous uint8 tensor [n,64]; device: where a table goes), or with device="cpu"
    the numpy statement of the same definitions.  Raises RuntimeError on a set fault word (one .item())."""
    from . import nodes as N
    wmode = weight_mode(weighted, weighted_mode)
    rows, table, on = _node_rows(rows, N.NODE_DTYPE, "NODE_DTYPE", device)
    n = rows.shape[0]
    if on.type == "cpu":
        obs, value, variance, weight, fault = N.node_targets_numpy(table, wmode, eps)
        obs, value, variance, weight = (torch.from_numpy(np.ascontiguousarray(x)) for x in (obs.view(np.int32), value, variance, weight))
    else:
        from . import _lib
        obs = torch.zeros(n, 12, dtype=torch.int32, device=on)
        value, variance, weight = (torch.zeros(n, dtype=torch.float32, device=on) for _ in range(3))
        fault = torch.zeros(1, dtype=torch.int32, device=on)
        if n:
            with torch.cuda.device(on):
                _lib.check(_lib.lib().tm_node_targets(_ptr(rows), n, wmode, float(eps), _ptr(obs), _ptr(value), _ptr(variance),
                                                      _ptr(weight), _ptr(fault),
                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)), "tm_node_targets")
        fault = int(fault.item())
    if fault:
        raise RuntimeError("node_targets: a row's value or variance is not finite, or its visit count is below 1: these are not "
                           "rows a collection harvested")
    return obs, value, variance, weight


def _node_files(paths, last_nfiles):
    """the stems choose_stems picks and their shards"""
    stems = choose_stems(paths, last_nfiles)
    return stems, [f for s in stems for f in _parts(s)]


def _node_hold_out(n_all, what, stems, files, validation, val_set_size, val_set_size_max, generator, dev):
    """The random hold-out of a node table of n_all rows (a node table has no episodes: _split's val_mode 0): the rows that train
    followed by the ones held out, how many they are together, and the training set's dict.  RuntimeError for no row at all."""
    if n_all == 0:
        raise RuntimeError("no rows to train on: the %s shards of %s are empty" % (what, stems))
    sel, n_val = _split(None, torch.ones(n_all, dtype=torch.bool, device=dev), validation, 0, 0, val_set_size, val_set_size_max,
                        generator, dev)
    n = int(sel.shape[0])
    return sel, n, dict(n=n, n_val=n_val, n_train=n - n_val, validation_fraction=validation_fraction(n, n_val), stems=stems,
                        files=files, n_rows=n_all)


def node_training_set(paths, weighted=False, weighted_mode=0, last_nfiles=1, validation=False, val_set_size=0.05,
                      val_set_size_max=-1, generator=None, device="cuda", eps=EPS):
    """data = [observations int32 [n,12], values [n,1], variances [n,1], weights [n,1]] on `device`, the training rows first and
    the held-out rows last - what Model_VV.train_data(state_format="packed") splits - and a dict with n, n_val, n_train,
    validation_fraction (train_data's int(n * fraction) is n_val exactly), the stems and the files.  paths / last_nfiles:
    choose_stems' rule over node shards.  The rows go to the device once; values and variances are the search's own.
    validation: a random int(n * val_set_size) rows are held out (at most val_set_size_max if that is positive; `generator`: a
    torch.Generator for the draw) - a node table has no episodes, so there is no episodic split."""
    from . import nodes as N
    stems, files = _node_files(paths, last_nfiles)
    table = N.load_rows(files)
    dev = torch.device(device)
    obs, value, variance, weight = node_targets(table, weighted=weighted, weighted_mode=weighted_mode, eps=eps, device=dev)
    sel, n, info = _node_hold_out(obs.shape[0], "node", stems, files, validation, val_set_size, val_set_size_max, generator, dev)
    data = [obs[sel].contiguous()] + [x[sel].reshape(n, 1) for x in (value, variance, weight)]
    return data, info


def fit_nodes(model, paths, batch_size=32, max_iters=100000, iters_per_val=None, early_stopping=False,
              early_stopping_patience=10, fit_backend="hip", validation_backend="hip", ewc_lambda=None, **options):
    """node_training_set(paths, **options) on the model's device, then model.train_data(..., state_format="packed") on it;
    returns what train_data returns plus n_train and n_val.  max_iters and iters_per_val may be functions, as in fit_episodes.
    The packed observations are read by the HIP kernels alone: fit_backend must be "hip", and validation_backend "hip" unless
    nothing is held out (ValueError otherwise).  ewc_lambda: as in fit_episodes - the fit is penalised against the Fisher and
    anchor the model holds, then Model_VV.compute_fisher(state_format="packed") runs over the training rows with the weights as
    the fit used them and rank 0 writes the checkpoint."""
    from .model import Model_VV
    if not isinstance(model, Model_VV):
        raise TypeError("fit_nodes fits a Model_VV: a node row holds a value and a variance, not a distribution (%s); the "
                        "distributional head's harvest has rows and a fit of its own, fit_dist_nodes" % type(model).__name__)
    if fit_backend != "hip":
        raise ValueError("fit_nodes hands the fit packed observations, which only the HIP gradient step reads: it needs "
                         "fit_backend='hip', not %r" % (fit_backend,))
    data, info = node_training_set(paths, device=model.device, **options)
    if info["n_val"] and validation_backend != "hip":
        raise ValueError("fit_nodes holds %d rows out, and the torch validation does not read packed observations: it needs "
                         "validation_backend='hip' (or no validation), not %r" % (info["n_val"], validation_backend))
    iters, extra = _iterations(max_iters, iters_per_val, info["n_train"])
    if ewc_lambda is not None:
        extra["ewc_lambda"] = ewc_lambda
    penalised = ewc_lambda is not None and model.fisher is not None
    res = model.train_data(data, batch_size=batch_size, max_iters=iters, validation_fraction=info["validation_fraction"],
                           shuffle=False, early_stopping=early_stopping, early_stopping_patience=early_stopping_patience,
                           fit_backend=fit_backend, validation_backend=validation_backend, state_format="packed", **extra)
    if ewc_lambda is not None:
        res = _consolidate(model, data, info["n_train"], res, penalised, state_format="packed")
    return dict(res, n_train=info["n_train"], n_val=info["n_val"])


# ---- dist node records: the harvested nodes of the distributional head (csrc/node_records.hip: tm_node_dist_targets) -------------
#
# `play.py --agent_type DistValueSim --save_dist_nodes` leaves NODE_DIST_DTYPE rows (nodes.py): the tuples the head's online fit
# trains on - packed observation, the node's backed-up distribution, the visits.  The target is that distribution as recorded -
# nothing is rebuilt from the head's own predictions -, the held-out rows are a random draw, and the fit reads the packed
# observations as they are (Model_Dist.train_data(fit_backend="hip_dist", state_format="packed")).

def dist_weight_mode(weighted, weighted_mode):
    """weight_mode of tm_node_dist_targets: 0 without `weighted`, 2 (the visits) with weighted_mode 1; a dist row carries no
    variance, so the value net's modes 0 (inverse of variance) and 2 (both) are a ValueError"""
    if not weighted:
        return 0
    if weighted_mode != 1:
        raise ValueError("weighted_mode must be 1 (number of visits) for dist node rows, not %r: they record no variance to "
                         "divide by" % (weighted_mode,))
    return 2


def node_dist_targets(rows, atoms, weighted=False, weighted_mode=1, device=None):
    """obs (int32 [n,12]), target (float32 [n,atoms]), weight (float32 [n]) of dist node rows: tm_node_dist_targets on the rows'
    device, on the current stream (`rows`: a NODE_DIST_DTYPE table or a contiguous uint8 tensor [n,320]; device: where a table
    goes), or with device="cpu" the numpy statement of the same definitions.  Raises RuntimeError on a set fault word (one .item())."""
    from . import nodes as N
    wmode = dist_weight_mode(weighted, weighted_mode)
    atoms = int(atoms)
    if not 1 <= atoms <= 64:
        raise ValueError("atoms: 1 .. 64, not %r" % (atoms,))
    rows, table, on = _node_rows(rows, N.NODE_DIST_DTYPE, "NODE_DIST_DTYPE", device)
    n = rows.shape[0]
    if on.type == "cpu":
        obs, target, weight, fault = N.node_dist_targets_numpy(table, atoms, wmode)
        obs, target, weight = (torch.from_numpy(np.ascontiguousarray(x)) for x in (obs.view(np.int32), target, weight))
    else:
        from . import _lib
        obs = torch.zeros(n, 12, dtype=torch.int32, device=on)
        target = torch.zeros(n, atoms, dtype=torch.float32, device=on)
        weight = torch.zeros(n, dtype=torch.float32, device=on)
        fault = torch.zeros(1, dtype=torch.int32, device=on)
        if n:
            with torch.cuda.device(on):
                _lib.check(_lib.lib().tm_node_dist_targets(_ptr(rows), n, atoms, wmode, _ptr(obs), _ptr(target), atoms, _ptr(weight),
                                                           _ptr(fault), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                           "tm_node_dist_targets")
        fault = int(fault.item())
    if fault:
        raise RuntimeError("node_dist_targets: a row's visit count is not finite or below 1, one of its %d atoms is not finite or "
                           "negative, none of them is above 0, or a float beyond them is not 0 (a file recorded with more atoms): "
                           "these are not rows a collection of this head harvested" % atoms)
    return obs, target, weight


def dist_node_training_set(paths, weighted=False, weighted_mode=1, last_nfiles=1, validation=False, val_set_size=0.05,
                           val_set_size_max=-1, generator=None, device="cuda"):
    """data = [observations int32 [n,12], targets [n,atoms], weights [n,1]] on `device`, the training rows first and the held-out
    rows last - what Model_Dist.train_data(state_format="packed") splits - and a dict with n, n_val, n_train, validation_fraction
    (train_data's int(n * fraction) is n_val exactly), the stems, the files and atoms, vmin, vmax from the stems' sidecars (which
    must agree: ValueError).  paths / last_nfiles: choose_stems' rule over dist node shards.  The rows go to the device once; the
    targets are the recorded distributions.  validation: node_training_set's random hold-out."""
    from . import nodes as N
    stems, files = _node_files(paths, last_nfiles)
    atoms, vmin, vmax = N.load_head(stems)
    table = N.load_rows(files, N.NODE_DIST_DTYPE)
    dev = torch.device(device)
    obs, target, weight = node_dist_targets(table, atoms, weighted=weighted, weighted_mode=weighted_mode, device=dev)
    sel, n, info = _node_hold_out(obs.shape[0], "dist node", stems, files, validation, val_set_size, val_set_size_max, generator, dev)
    data = [obs[sel].contiguous(), target[sel].contiguous(), weight[sel].reshape(n, 1)]
    return data, dict(info, atoms=atoms, vmin=vmin, vmax=vmax)


def fit_dist_nodes(model, paths, batch_size=32, max_iters=100000, iters_per_val=None, early_stopping=False,
                   early_stopping_patience=10, fit_backend="hip_dist", validation_backend="hip", ewc_lambda=None, **options):
    """dist_node_training_set(paths, **options) on the model's device, then model.train_data(..., fit_backend="hip_dist",
    state_format="packed") on it and, on rank 0, model.save(); returns what train_data returns plus n_train, n_val and the
    sidecar's atoms, vmin, vmax.  model: a Model_Dist (TypeError otherwise) with the file's atoms (ValueError otherwise).
    max_iters and iters_per_val may be functions, as in fit_episodes.  The packed observations are read by the HIP kernels
    alone: fit_backend must be "hip_dist", and validation_backend "hip" unless nothing is held out (ValueError otherwise).
    ewc_lambda: as in fit_episodes_dist - the fit is penalised against the Fisher and anchor the model holds, then
    Model_Dist.compute_fisher(state_format="packed") runs over the training rows with the weights as the fit used them and rank 0
    writes the checkpoint; the result gains ewc = dict(penalised, fisher_rows)."""
    from .model_distributional import Model_Dist
    if not isinstance(model, Model_Dist):
        raise TypeError("fit_dist_nodes fits a Model_Dist: a dist node row holds a distribution, not a value and a variance (%s); "
                        "the value net's harvest is fit_nodes'" % type(model).__name__)
    if fit_backend != "hip_dist":
        raise ValueError("fit_dist_nodes hands the fit packed observations, which only the head's HIP gradient step reads: it "
                         "needs fit_backend='hip_dist', not %r" % (fit_backend,))
    from . import nodes as N
    stems = choose_stems(paths, options.get("last_nfiles", 1))
    atoms = N.load_head(stems)[0]          # (before a row is read: the targets below are cut at the file's atoms)
    if atoms != int(model.atoms):
        raise ValueError("the shards of %s were recorded by a head of %d atoms, the model has %d" % (stems, atoms, int(model.atoms)))
    data, info = dist_node_training_set(paths, device=model.device, **options)
    if info["n_val"] and validation_backend != "hip":
        raise ValueError("fit_dist_nodes holds %d rows out, and the torch validation does not read packed observations: it needs "
                         "validation_backend='hip' (or no validation), not %r" % (info["n_val"], validation_backend))
    iters, extra = _iterations(max_iters, iters_per_val, info["n_train"])
    if ewc_lambda is not None:
        extra["ewc_lambda"] = ewc_lambda
    penalised = ewc_lambda is not None and model.fisher is not None
    res = model.train_data(data, fit_backend="hip_dist", state_format="packed", shuffle=False, batch_size=batch_size, max_iters=iters,
                           validation_fraction=info["validation_fraction"], early_stopping=early_stopping,
                           early_stopping_patience=early_stopping_patience, validation_backend=validation_backend, **extra)
    if ewc_lambda is not None:
        res = _consolidate(model, data, info["n_train"], res, penalised, state_format="packed")
    else:
        _save_on_rank0(model)
    return dict(res, n_train=info["n_train"], n_val=info["n_val"], atoms=info["atoms"], vmin=info["vmin"], vmax=info["vmax"])
