"""Shared cases of the node records' tests (tests/test_nodes.py on the host, tests/test_gpu_nodes.py on the GPU): numpy
statements of tm_nodes_drain and tm_nodes_sweep (include/tetris_mcts_hip.h), synthetic harvests, the refusals of the three
calls and synthetic node rows."""
import ctypes as C

import numpy as np

INVALID = 1      # hipErrorInvalidValue
KIND_DIST = 6
ROW = 64
GS_DW, GS_LOW_OBS = 64, 27


def node_dtype():
    from tetris_mcts_amd.nodes import NODE_DTYPE
    return NODE_DTYPE


def harvest(G, cap, seed, empty=False):
    """random bytes for replay_obs [G,cap,12] u4 and replay_stat [G,cap,4] u4 and counts drawn from 0, 1, 5 and 9 (9: more than a
    buffer of 5 holds - the drain clamps it); about a third of the games empty, or all of them"""
    rng = np.random.default_rng(seed)
    obs = rng.integers(0, 2 ** 32, (G, cap, 12), dtype=np.uint64).astype(np.uint32)
    stat = rng.integers(0, 2 ** 32, (G, cap, 4), dtype=np.uint64).astype(np.uint32)
    count = rng.choice(np.array([0, 0, 1, 5, 9], np.int32), G).astype(np.int32)
    if G >= 3 and not empty:
        count[0], count[G // 2], count[-1] = 9, 0, 5         # the first game over-full, one in the middle empty, the last full
    elif not empty:
        count[0] = 9 if seed % 2 == 0 else 1
    if empty:
        count[:] = 0
    return obs, stat, count


def drain_statement(obs, stat, count, cap):
    """the rows tm_nodes_drain appends for one harvest, as bytes [n, 64]: game-major, tuples 0 .. min(count, cap)-1 of a game in
    order; the observation's 48 bytes, the first three words of the statistics, the game index"""
    out = []
    for g in range(len(count)):
        c = int(min(max(int(count[g]), 0), cap))
        r = np.zeros((c, 16), np.uint32)
        r[:, :12] = obs[g, :c]
        r[:, 12:15] = stat[g, :c, :3]
        r[:, 15] = g
        out.append(r)
    return np.concatenate(out + [np.zeros((0, 16), np.uint32)]).view(np.uint8).reshape(-1, ROW)


def sweep_statement(obs_stat, obs_key, gs, min_visits):
    """the rows tm_nodes_sweep appends, as bytes [n, 64], and the slots taken per game.  obs_stat [G,N,4] u4, obs_key [G,N,12] u4,
    gs [G,64] i4: per game, ascending o >= gs[LOW_OBS], every slot with (int)stat.x >= max(min_visits, 1) and bit 31 clear"""
    G, N = obs_stat.shape[:2]
    out, per = [], []
    for g in range(G):
        low = int(min(max(int(gs[g, GS_LOW_OBS]), 0), N))
        x = obs_stat[g, low:, 0]
        keep = (x.view(np.int32) >= max(int(min_visits), 1)) & ((x >> 31) == 0)
        o = low + np.nonzero(keep)[0]
        r = np.zeros((len(o), 16), np.uint32)
        r[:, :12] = obs_key[g, o]
        r[:, 12:14] = obs_stat[g, o, 1:3]
        r[:, 14] = obs_stat[g, o, 0].view(np.int32).astype(np.float32).view(np.uint32)
        r[:, 15] = g
        out.append(r)
        per.append(o)
    return np.concatenate(out + [np.zeros((0, 16), np.uint32)]).view(np.uint8).reshape(-1, ROW), per


def synthetic_rows(n, seed, faults=()):
    """n node rows as a collection could have harvested them (finite values, variances > 0, visits >= 1, random observations);
    faults: (row, column, value) written over them"""
    rng = np.random.default_rng(seed)
    rows = np.zeros(n, node_dtype())
    rows["obs"] = rng.integers(0, 2 ** 32, (n, 12), dtype=np.uint64).astype(np.uint32)
    rows["value"] = rng.uniform(0, 60, n).astype(np.float32)
    rows["variance"] = rng.uniform(0.05, 300, n).astype(np.float32)
    rows["visit"] = rng.integers(1, 500, n).astype(np.float32)
    rows["slot"] = rng.integers(0, 64, n)
    if n > 3:
        rows["variance"][1] = 0.0                # 1 / (0 + eps) is finite
        rows["visit"][2] = 1.0
    for r, col, v in faults:
        rows[col][r] = v
    return rows


def _store(L, kind=0, n_games=8, replay_cap=5):
    """a description of a store whose pointers are never followed (every call below is refused before a launch)"""
    s = L.TmStore()
    s.n_games, s.max_nodes, s.kind, s.replay_cap, s.online, s.min_visits_to_store = n_games, 64, kind, replay_cap, 1, 3
    for name in ("replay_obs", "replay_stat", "replay_count", "obs_stat", "obs_key", "gs"):
        setattr(s, name, 4096)
    return s


def refused_node_arguments(L, ptr):
    """every refusal of tm_nodes_drain, tm_nodes_sweep and tm_node_targets returns hipErrorInvalidValue; `ptr`: a non-null,
    16-byte aligned address that is never dereferenced (the checks come before the first HIP call)"""
    lib = L.lib()
    p, null, odd = C.c_void_p(ptr), C.c_void_p(0), C.c_void_p(ptr + 8)
    for fn in (lib.tm_nodes_drain, lib.tm_nodes_sweep):
        s = _store(L)

        def call(store=s, ring=p, cap=16, counters=p, offsets=p):
            return fn(C.byref(store) if store is not None else None, ring, cap, counters, offsets, null)
        for kw in (dict(store=None), dict(ring=null), dict(counters=null), dict(offsets=null), dict(cap=0), dict(cap=-3),
                   dict(ring=odd), dict(ring=C.c_void_p(ptr + 4)), dict(store=_store(L, kind=KIND_DIST)), dict(store=_store(L, n_games=0))):
            assert call(**kw) == INVALID, (fn.__name__, kw)
    for cap in (0, -1):
        assert lib.tm_nodes_drain(C.byref(_store(L, replay_cap=cap)), p, 16, p, p, null) == INVALID, cap
    for name in ("replay_obs", "replay_stat", "replay_count"):
        s = _store(L)
        setattr(s, name, None)
        assert lib.tm_nodes_drain(C.byref(s), p, 16, p, p, null) == INVALID, name
    for name in ("obs_stat", "obs_key", "gs"):
        s = _store(L)
        setattr(s, name, None)
        assert lib.tm_nodes_sweep(C.byref(s), p, 16, p, p, null) == INVALID, name

    # the store's arrays are read as 16-byte pieces
    for fn, names in ((lib.tm_nodes_drain, ("replay_obs", "replay_stat")), (lib.tm_nodes_sweep, ("obs_stat", "obs_key"))):
        for name in names:
            s = _store(L)
            setattr(s, name, 4096 + 8)
            assert fn(C.byref(s), p, 16, p, p, null) == INVALID, name

    def targets(rows=p, n=10, wmode=0, obs=p, value=p, variance=p, weight=p, fault=p):
        return lib.tm_node_targets(rows, n, wmode, 0.001, obs, value, variance, weight, fault, null)
    for kw in (dict(rows=null), dict(obs=null), dict(value=null), dict(variance=null), dict(weight=null), dict(fault=null),
               dict(n=-1), dict(n=2 ** 29), dict(wmode=-1), dict(wmode=4), dict(rows=odd), dict(rows=C.c_void_p(ptr + 4)),
               dict(obs=C.c_void_p(ptr + 2))):
        assert targets(**kw) == INVALID, kw
    # nothing to do is not an error - unless an argument is refused whatever the size
    assert targets(n=0) == 0
    assert targets(n=0, wmode=4) == INVALID and targets(n=0, rows=odd) == INVALID and targets(n=0, fault=null) == INVALID
