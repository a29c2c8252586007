"""Shared cases of the dist node records' tests (tests/test_dist_nodes.py on the host, tests/test_gpu_dist_nodes.py on the GPU):
the byte statement of tm_nodes_drain_dist (include/tetris_mcts_hip.h), synthetic harvests of a TM_KIND_DIST store, synthetic
dist node rows with a fault injector, and the refusals of the two calls."""
import ctypes as C

import numpy as np

INVALID = 1      # hipErrorInvalidValue
KIND_DIST = 6
ROW = 320
DIST_ROW = 64


def dist_dtype():
    from tetris_mcts_amd.nodes import NODE_DIST_DTYPE
    return NODE_DIST_DTYPE


def harvest(G, cap, seed, empty=False):
    """random bytes for replay_obs [G,cap,12] u4, replay_stat [G,cap,4] u4 and replay_dist [G,cap,64] u4, and counts drawn from 0,
    1, 5 and 9 (9: more than a buffer of 5 holds - the drain clamps it); about a third of the games empty, or all of them"""
    rng = np.random.default_rng(seed)
    obs = rng.integers(0, 2 ** 32, (G, cap, 12), dtype=np.uint64).astype(np.uint32)
    stat = rng.integers(0, 2 ** 32, (G, cap, 4), dtype=np.uint64).astype(np.uint32)
    dist = rng.integers(0, 2 ** 32, (G, cap, DIST_ROW), dtype=np.uint64).astype(np.uint32)
    count = rng.choice(np.array([0, 0, 1, 5, 9], np.int32), G).astype(np.int32)
    if G >= 3 and not empty:
        count[0], count[G // 2], count[-1] = 9, 0, 5         # the first game over-full, one in the middle empty, the last full
    elif not empty:
        count[0] = 9 if seed % 2 == 0 else 1
    if empty:
        count[:] = 0
    return obs, stat, dist, count


def drain_statement(obs, stat, dist, count, cap):
    """the rows tm_nodes_drain_dist appends for one harvest, as bytes [n, 320]: game-major, tuples 0 .. min(count, cap)-1 of a game
    in order; the observation's 48 bytes, the first three words of the statistics, the game index, the distribution's 256 bytes"""
    out = []
    for g in range(len(count)):
        c = int(min(max(int(count[g]), 0), cap))
        r = np.zeros((c, ROW // 4), np.uint32)
        r[:, :12] = obs[g, :c]
        r[:, 12:15] = stat[g, :c, :3]
        r[:, 15] = g
        r[:, 16:] = dist[g, :c]
        out.append(r)
    return np.concatenate(out + [np.zeros((0, ROW // 4), np.uint32)]).view(np.uint8).reshape(-1, ROW)


# the kinds of fault of tm_node_dist_targets: name -> (column, index inside the column or None, value); "beyond" needs atoms < 64
FAULT_KINDS = ("visit_zero", "visit_nan", "visit_inf", "atom_nan", "atom_inf", "atom_negative", "all_zero", "beyond")


def inject(rows, r, kind, atoms):
    """make row r of `rows` faulty in one way (in place); False when the kind does not exist at this number of atoms"""
    if kind == "visit_zero":
        rows["visit"][r] = 0.0
    elif kind == "visit_nan":
        rows["visit"][r] = np.float32("nan")
    elif kind == "visit_inf":
        rows["visit"][r] = np.float32("inf")
    elif kind == "atom_nan":
        rows["dist"][r, atoms - 1] = np.float32("nan")
    elif kind == "atom_inf":
        rows["dist"][r, 0] = np.float32("inf")
    elif kind == "atom_negative":
        rows["dist"][r, atoms // 2] = np.float32(-1e-6)
    elif kind == "all_zero":
        rows["dist"][r, :atoms] = 0.0
    elif kind == "beyond":
        if atoms >= DIST_ROW:
            return False
        rows["dist"][r, DIST_ROW - 1] = np.float32(1e-30)
    else:
        raise ValueError(kind)
    return True


def synthetic_rows(n, seed, atoms, faults=()):
    """n dist node rows as a collection could have harvested them: random observations, value and variance 0, visits >= 1, a
    distribution over the first `atoms` floats (some atoms exactly 0, a -0.0 among them) and zero padding behind them;
    faults: (row, kind) made by `inject`"""
    rng = np.random.default_rng(seed)
    rows = np.zeros(n, dist_dtype())
    rows["obs"] = rng.integers(0, 2 ** 32, (n, 12), dtype=np.uint64).astype(np.uint32)
    rows["visit"] = rng.integers(1, 500, n).astype(np.float32)
    rows["slot"] = rng.integers(0, 64, n)
    p = rng.uniform(0, 1, (n, atoms)) * (rng.uniform(0, 1, (n, atoms)) < 0.7)
    p[:, rng.integers(0, atoms)] += 0.25                     # no row without mass
    rows["dist"][:, :atoms] = (p / p.sum(1, keepdims=True)).astype(np.float32)
    if n > 3:
        rows["visit"][2] = 1.0
        rows["dist"][1, :atoms] = 0.0
        rows["dist"][1, atoms - 1] = 1.0                     # all mass in the last atom
        if atoms > 1:
            rows["dist"][3, 0] = np.float32(-0.0)            # compares equal to 0: no fault
            rows["dist"][3, 1] = 0.5
        if atoms < DIST_ROW:
            rows["dist"][3, DIST_ROW - 1] = np.float32(-0.0)
    for r, kind in faults:
        assert inject(rows, r, kind, atoms), (kind, atoms)
    return rows


def _store(L, kind=KIND_DIST, n_games=8, replay_cap=5):
    """a description of a store whose pointers are never followed (every call below is refused before a launch)"""
    s = L.TmStore()
    s.n_games, s.max_nodes, s.kind, s.replay_cap, s.online, s.min_visits_to_store = n_games, 64, kind, replay_cap, 1, 3
    s.dist_bins = 50
    for name in ("replay_obs", "replay_stat", "replay_count", "replay_dist", "obs_stat", "obs_key", "gs"):
        setattr(s, name, 4096)
    return s


def refused_dist_node_arguments(L, ptr):
    """every refusal of tm_nodes_drain_dist and tm_node_dist_targets returns hipErrorInvalidValue; `ptr`: a non-null, 16-byte
    aligned address that is never dereferenced (the checks come before the first HIP call)"""
    lib = L.lib()
    p, null, odd = C.c_void_p(ptr), C.c_void_p(0), C.c_void_p(ptr + 8)
    s = _store(L)

    def drain(store=s, ring=p, cap=16, counters=p, offsets=p):
        return lib.tm_nodes_drain_dist(C.byref(store) if store is not None else None, ring, cap, counters, offsets, null)
    for kw in (dict(store=None), dict(ring=null), dict(counters=null), dict(offsets=null), dict(cap=0), dict(cap=-3),
               dict(ring=odd), dict(ring=C.c_void_p(ptr + 4)), dict(store=_store(L, n_games=0)), dict(store=_store(L, n_games=-2)),
               dict(store=_store(L, replay_cap=0)), dict(store=_store(L, replay_cap=-1))):
        assert drain(**kw) == INVALID, kw
    for kind in (0, 1, 2, 3, 4, 5, 7):                       # every store that is not TM_KIND_DIST
        assert drain(store=_store(L, kind=kind)) == INVALID, kind
    for name in ("replay_obs", "replay_stat", "replay_count", "replay_dist"):
        st = _store(L)
        setattr(st, name, None)
        assert drain(store=st) == INVALID, name
    for name in ("replay_obs", "replay_stat", "replay_dist"):          # read as 16-byte pieces
        for off in (4, 8):
            st = _store(L)
            setattr(st, name, 4096 + off)
            assert drain(store=st) == INVALID, (name, off)
    # the value net's drain keeps refusing this kind
    assert lib.tm_nodes_drain(C.byref(_store(L)), p, 16, p, p, null) == INVALID

    def targets(rows=p, n=10, atoms=50, wmode=0, obs=p, target=p, stride=64, weight=p, fault=p):
        return lib.tm_node_dist_targets(rows, n, atoms, wmode, obs, target, stride, weight, fault, null)
    for kw in (dict(rows=null), dict(obs=null), dict(target=null), dict(weight=null), dict(fault=null), dict(n=-1), dict(n=2 ** 29),
               dict(atoms=0), dict(atoms=-1), dict(atoms=65), dict(atoms=50, stride=49), dict(atoms=64, stride=50), dict(stride=0),
               dict(wmode=-1), dict(wmode=1), dict(wmode=3), dict(wmode=4), dict(rows=odd), dict(rows=C.c_void_p(ptr + 4)),
               dict(obs=C.c_void_p(ptr + 2)), dict(target=C.c_void_p(ptr + 2)), dict(weight=C.c_void_p(ptr + 1))):
        assert targets(**kw) == INVALID, kw
    # nothing to do is not an error - unless an argument is refused whatever the size
    assert targets(n=0) == 0
    for kw in (dict(wmode=1), dict(rows=odd), dict(fault=null), dict(atoms=65), dict(stride=3), dict(target=C.c_void_p(ptr + 2))):
        assert targets(n=0, **kw) == INVALID, kw
