"""Synthetic self-play shards for the offline targets (tetris_mcts_amd/offline.py, csrc/episode_targets.hip), built with numpy
alone - no engine - and an EXACT oracle of the lambda-return.

The table: G = 5 slots, each playing its episodes one after another for 400 moves, the rows emitted move-major, slot-minor as the
recorder writes them and numbered by its rule (the first G episodes are the slots, later ids by move, then by slot).  The
episode lengths cover 1, 2, 63, 64, 65, 127, 128, 129 and 300 - the 64-lane chunk of the kernel, its neighbours and several
carries - and the last episode of every slot is cut off by the end of the run: it has no row in the episode table (censored).
Scores do not fall: a start of up to 2 000 000, steps of up to 4 000; the episode table holds the FINAL score (one more step).
Values: `draw="pos"` in [0, 200), `draw="mixed"` in [-200, 200).  Variances are positive, visits integer-valued floats, board
cells int8 of both signs.

The oracle is the reference's forward loop (train.py:91-101: for every row, walk to the end of its episode with
weight *= lambda) restated in exact arithmetic.  Every input is a dyadic rational - an int score, a float32 value, a double
lambda = a / 2^b - so the loop runs over Python ints scaled by a power of two instead of normalising a fractions.Fraction at
every step (the same numbers, some thousand times faster at 300 moves); `Exact.fraction(i)` gives a row's return as a Fraction.
"""
import os
from fractions import Fraction

import numpy as np

G, MOVES = 5, 400
LENGTHS = [[1, 2, 300], [63, 128], [64, 129], [65, 127], [300, 5]]         # per slot; the rest of the 400 moves is the censored one
CYCLE = 4
LAMBDAS = (0.0, 0.5, 0.9, 1.0)


def make_table(draw="pos", seed=0, cycle=CYCLE, first_id=0):
    """(rows STATE_DTYPE in file order, episodes EPISODE_DTYPE in the order they ended)"""
    from tetris_mcts_amd.episodes import EPISODE_DTYPE, STATE_DTYPE
    rng = np.random.default_rng([seed, {"pos": 0, "mixed": 1}[draw]])
    plan = [ls + [MOVES - sum(ls)] for ls in LENGTHS]
    assert all(p[-1] > 0 for p in plan)
    ids, which, move, next_id = [first_id + g for g in range(G)], [0] * G, [0] * G, first_id + G
    score = [int(rng.integers(0, 2_000_001)) for _ in range(G)]
    rows, done = np.zeros(G * MOVES, STATE_DTYPE), []
    for m in range(MOVES):
        for g in range(G):
            r = rows[m * G + g]
            r["episode"], r["cycle"], r["slot"], r["move"] = ids[g], cycle, g, move[g]
            r["score"], r["lines"], r["combo"] = score[g], score[g] // 100, int(rng.integers(-1, 5))
            r["line_stats"] = rng.integers(0, 1000, 4)
            lo = 0.0 if draw == "pos" else -200.0
            r["value"] = np.float32(rng.uniform(lo, 200.0))
            r["variance"] = np.float32(rng.uniform(1e-3, 500.0))
            st = np.zeros((3, 7), np.float32)
            st[0] = rng.integers(0, 400, 7).astype(np.float32)
            st[1:] = rng.uniform(-50, 50, (2, 7)).astype(np.float32)
            r["child_stats"] = st
            r["policy"] = st[0] / max(st[0].sum(), 1)
            r["board"] = rng.integers(-2, 3, (20, 10)).astype(np.int8)
            r["action"] = int(rng.integers(0, 7))
        for g in range(G):                              # the recorder's advance: by move, then by slot
            score[g] += int(rng.integers(0, 4001))
            move[g] += 1
            if move[g] == plan[g][which[g]] and which[g] + 1 < len(plan[g]):
                done.append((ids[g], cycle, g, move[g], score[g], score[g] // 100, [0, 0, 0, 0]))
                ids[g], next_id, which[g], move[g] = next_id, next_id + 1, which[g] + 1, 0
                score[g] = int(rng.integers(0, 2_000_001))
    ep = np.zeros(len(done), EPISODE_DTYPE)
    for i, d in enumerate(done):
        ep[i] = d
    return rows, ep


def write_shards(stem, rows, episodes, split=150 * G):
    """two parts of both tables under `stem` (the episodes that ended inside a part go with it)"""
    os.makedirs(os.path.dirname(stem) or ".", exist_ok=True)
    a, b = rows[:split], rows[split:]
    in_a = np.zeros(len(episodes), bool)
    for i, e in enumerate(episodes):                    # an episode that ended shows its last row: which part holds it
        last = np.nonzero((rows["episode"] == e["episode"]) & (rows["move"] == e["moves"] - 1))[0][0]
        in_a[i] = last < split
    for k, (r, e) in enumerate(((a, episodes[in_a]), (b, episodes[~in_a]))):
        np.save("%s.part%05d.npy" % (stem, k), r)
        np.save("%s.episodes.part%05d.npy" % (stem, k), e)


def by_episode(rows):
    """(order, seg): the sort EpisodeLoader(by_episode=True) does, and where its episodes begin and end"""
    order = np.lexsort((rows["move"], rows["episode"], rows["cycle"]))
    key = np.stack([rows["cycle"][order], rows["episode"][order]], 1)
    first = np.append(True, (key[1:] != key[:-1]).any(1))
    return order.astype(np.int32), np.append(np.nonzero(first)[0], len(rows)).astype(np.int32)


def tails(rows, episodes, order, seg, final=True):
    """per segment (tail_kind u8, tail_score i32, tail_value f32): the FINAL score of the episodes the table names"""
    table = {(int(e["cycle"]), int(e["episode"])): int(e["score"]) for e in episodes}
    kind, score = np.zeros(len(seg) - 1, np.uint8), np.zeros(len(seg) - 1, np.int32)
    for e, a in enumerate(seg[:-1]):
        r = rows[order[a]]
        k = (int(r["cycle"]), int(r["episode"]))
        if final and k in table:
            kind[e], score[e] = 1, table[k]
    return kind, score, np.zeros(len(seg) - 1, np.float32)


def _dyadic(x, E):
    """x * 2^E as an int (x a float whose denominator divides 2^E)"""
    p, q = float(x).as_integer_ratio()
    return p * ((1 << E) // q)


class Exact:
    """The lambda-return of every sorted position, exactly.  For position i of an episode with the series (s_k, v_k), k up to
    the end (the tail included): SN = sum w_k T_k, SA = sum w_k |T_k|, SW = sum w_k with T_k = (s_{i+k} + v_{i+k} - s_i) 2^E and
    w_k = lambda^k 2^(b (K-1)) - all ints; the return is SN / (SW 2^E), the bound's M is SA / (SW 2^E)."""

    def __init__(self, rows, order, seg, tail, lam):
        kind, tscore, tvalue = tail
        a, q = float(lam).as_integer_ratio()
        b = q.bit_length() - 1
        v = rows["value"][order]
        self.E = E = max([float(x).as_integer_ratio()[1].bit_length() - 1 for x in v] + [0])
        n = len(order)
        self.SN, self.SA, self.SW = [0] * n, [0] * n, [0] * n
        for e in range(len(seg) - 1):
            pos = list(range(seg[e], seg[e + 1]))
            S = [int(rows["score"][order[j]]) << E for j in pos] + ([int(tscore[e]) << E] if kind[e] == 1 else [])
            V = [_dyadic(v[j], E) for j in pos] + ([_dyadic(tvalue[e], E)] if kind[e] == 1 else [])
            K = len(S)
            for i, j in enumerate(pos):
                w = 1 << (b * (K - 1 - i))               # weight = 1, scaled so that every later weight is an int
                sn = sa = sw = 0
                for r in range(i, K):                    # the reference's while loop: to the end of the episode
                    t = S[r] + V[r] - S[i]
                    sn += w * t
                    sa += w * abs(t)
                    sw += w
                    w = (w * a) >> b                     # weight *= lambda (exact: w holds at least b factors of two, or is 0)
                self.SN[j], self.SA[j], self.SW[j] = sn, sa, sw

    def fraction(self, j):
        return Fraction(self.SN[j], self.SW[j] << self.E)

    def bound_fraction(self, value):
        """max over the positions of |value_j - exact_j| / (2^-23 M_j) (0 where both sides are 0; inf where only M is)"""
        worst = 0.0
        for j, x in enumerate(np.asarray(value, np.float32).tolist()):
            p, q = float(x).as_integer_ratio()
            lhs = abs(p * (self.SW[j] << self.E) - self.SN[j] * q) << 23
            rhs = self.SA[j] * q
            if lhs:
                worst = max(worst, float("inf") if rhs == 0 or lhs >> 900 > rhs else lhs / rhs)
        return worst


_cache = {}


def case(draw, final, lam):
    """the table of `draw` sorted by episode, its tails, and the exact returns - computed once and shared"""
    key = (draw, bool(final), float(lam))
    if key not in _cache:
        if ("table", draw) not in _cache:
            rows, ep = make_table(draw)
            _cache[("table", draw)] = (rows, ep) + by_episode(rows)
        rows, ep, order, seg = _cache[("table", draw)]
        tail = tails(rows, ep, order, seg, final)
        _cache[key] = dict(rows=rows, episodes=ep, order=order, seg=seg, tail=tail, exact=Exact(rows, order, seg, tail, lam))
    return _cache[key]
