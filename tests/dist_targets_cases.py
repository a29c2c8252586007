"""Small synthetic recordings for the categorical episode targets (tetris_mcts_amd/offline.py dist_targets_numpy,
csrc/episode_dist_targets.hip) and an EXACT oracle of them.

The table: three stems, the episodes of a stem played side by side from move 0 and emitted move-major, slot-minor as the recorder
writes them; the stems one after the other.  Episode lengths 1, 63, 130 | 2, 64, (20) | 65, (7): a wave, the kernel's run of 64
targets and its chunk of 64 rows, their neighbours, and an episode over three chunks; the two in brackets have no row in the
episode table (censored: no tail).  Sorted by (stem, episode, move) the episodes begin at 0, 1, 64, 194, 196, 260, 280, 345, so
runs begin inside episodes, at their first row and one row before their end.
Scores do not fall.  The steps, in units of the atoms' width delta: 0, exactly 2 delta (rounded to an int: a whole number of
atoms where delta is an integer), a draw below 3 delta, and now and then more than the whole range; the mean step is about one
delta, so the sum crosses the range inside a window of 64 moves.  The distributions by table row are softmax draws in float32
with atoms set to exactly 0 and a few subnormal entries; the padding atoms hold NaN.

The oracle states the shift in SCATTER form, as the definition does (source atom a gives p[a] (1 - f) to lb = min(a + n, K-1) and
p[a] f to min(lb + 1, K-1)), over Python ints: a float32 is an int times 2^-149, f = bs - floor(bs) of the double bs = c / delta is
an int times 2^-EF, lambda = a / 2^q; the weighted sum runs as Horner's rule in ints, R_k = T_k 2^(q (m - k)) + a R_{k+1}, so a
target atom is the rational R_0[b] / (W_0 2^(149 + EF)) with nothing rounded anywhere.  n, f and lambda are the DOUBLES the
statement uses (include/tetris_mcts_hip.h), taken exactly."""
import math
from fractions import Fraction

import numpy as np

LENGTHS = [[(1, True), (63, True), (130, True)], [(2, True), (64, True), (20, False)], [(65, True), (7, False)]]
EF = 200                                       # f = bs - floor(bs) is a multiple of 2^-EF for every bs the cases meet
GEOMETRY = {1: (0.0, 700.0), 2: (-10.0, 7.0), 50: (0.0, 5000.0), 64: (0.0, 1000.0)}       # atoms -> [vmin, vmax)


def make_table(atoms, seed=0):
    """rows STATE_DTYPE in file order, episodes EPISODE_DTYPE, stem_rows, episode_stems, p_rows float32 [n_rows, 64]"""
    from tetris_mcts_amd.episodes import EPISODE_DTYPE, STATE_DTYPE, _concat
    vmin, vmax = GEOMETRY[atoms]
    delta = (vmax - vmin) / atoms
    rng = np.random.default_rng([seed, atoms])
    tables, done, stem_rows, done_stem = [], [], [], []
    for k, plan in enumerate(LENGTHS):
        moves = max(length for length, _ in plan)
        score = [int(rng.integers(0, 1_000_001)) for _ in plan]
        out, filled = np.zeros(sum(length for length, _ in plan), STATE_DTYPE), 0
        for m in range(moves):
            for g, (length, ended) in enumerate(plan):
                if m >= length:
                    continue
                r = out[filled]
                filled += 1
                r["episode"], r["cycle"], r["slot"], r["move"], r["score"] = g, 4, g, m, score[g]
                r["value"] = np.float32(rng.uniform(0, 200.0))
                r["variance"] = np.float32(rng.uniform(1e-3, 500.0))
                st = np.zeros((3, 7), np.float32)
                st[0] = rng.integers(0, 400, 7).astype(np.float32)
                r["child_stats"] = st
                r["board"] = rng.integers(0, 2, (20, 10)).astype(np.int8)
                kind = int(rng.integers(0, 8))
                step = (0 if kind == 0 else int(round(2 * delta)) if kind == 1 else int(vmax - vmin) + 5 if kind == 2 and m % 9 == 4
                        else int(rng.integers(0, int(3 * delta) + 1)))
                score[g] += step
                if m == length - 1 and ended:
                    done.append((g, 4, g, length, score[g], 0, [0, 0, 0, 0]))
                    done_stem.append(k)
        tables.append(out)
        stem_rows.append(len(out))
    rows = _concat(tables, STATE_DTYPE)                                 # (np.concatenate would pack the fields)
    ep = np.zeros(len(done), EPISODE_DTYPE)
    for i, d in enumerate(done):
        ep[i] = d
    logits = rng.normal(0, 2.5, (len(rows), atoms))
    p = np.exp(logits - logits.max(1, keepdims=True))
    p = (p / p.sum(1, keepdims=True)).astype(np.float32)
    p[rng.random(p.shape) < 0.15] = 0.0
    p[rng.random(p.shape) < 0.01] = np.float32(3e-45)                 # subnormal: two units of 2^-149
    p_rows = np.full((len(rows), 64), np.nan, np.float32)
    p_rows[:, :atoms] = p
    return rows, ep, stem_rows, np.asarray(done_stem, np.int64), p_rows


def by_episode(rows, stem_rows):
    """(order, seg): sorted by (stem, episode, move), and where the episodes begin and end"""
    stem = np.repeat(np.arange(len(stem_rows)), stem_rows)
    order = np.lexsort((rows["move"], rows["episode"], stem))
    key = np.stack([stem[order], rows["episode"][order]], 1)
    first = np.append(True, (key[1:] != key[:-1]).any(1))
    return order.astype(np.int32), np.append(np.nonzero(first)[0], len(rows)).astype(np.int32)


def tails(rows, ep, episode_stems, stem_rows, order, seg, final=True):
    stem = np.repeat(np.arange(len(stem_rows)), stem_rows)
    table = {(int(s), int(e["episode"])): int(e["score"]) for s, e in zip(episode_stems, ep)}
    kind, score = np.zeros(len(seg) - 1, np.uint8), np.zeros(len(seg) - 1, np.int32)
    for e, a in enumerate(seg[:-1]):
        k = (int(stem[order[a]]), int(rows["episode"][order[a]]))
        if final and k in table:
            kind[e], score[e] = 1, table[k]
    return kind, score


_cache = {}


def case(atoms, final=True):
    """the table of `atoms` sorted by episode, its tails and its distributions - made once and shared, never changed"""
    key = (atoms, bool(final))
    if key not in _cache:
        if ("table", atoms) not in _cache:
            rows, ep, stem_rows, ep_stems, p_rows = make_table(atoms)
            _cache[("table", atoms)] = (rows, ep, stem_rows, ep_stems, p_rows) + by_episode(rows, stem_rows)
        rows, ep, stem_rows, ep_stems, p_rows, order, seg = _cache[("table", atoms)]
        vmin, vmax = GEOMETRY[atoms]
        _cache[key] = dict(rows=rows, episodes=ep, stem_rows=stem_rows, episode_stems=ep_stems, p_rows=p_rows, order=order, seg=seg,
                           tail=tails(rows, ep, ep_stems, stem_rows, order, seg, final), atoms=atoms, vmin=vmin, vmax=vmax)
    return _cache[key]


def shift_doubles(c, delta, K):
    """(n, numerator of f over 2^EF) from the doubles the statement computes: bs = (double)c / delta, n = floor(bs), f = bs - n"""
    bs = float(max(int(c), 0)) / delta
    fl = math.floor(bs)
    f = bs - fl
    num, den = f.as_integer_ratio()
    assert (1 << EF) % den == 0, "f needs more than EF bits"
    return min(fl, K), num * ((1 << EF) // den)


def shift_scatter(p, n, fn, K):
    """S(p) of ints p (units of 2^-149) -> ints in units of 2^-(149 + EF): the definition, source atom by source atom"""
    out = [0] * K
    one = 1 << EF
    for a, x in enumerate(p):
        if x:
            lb = min(a + n, K - 1)
            out[lb] += x * (one - fn)
            out[min(lb + 1, K - 1)] += x * fn
    return out


def _units(x):
    """a float32 as an int times 2^-149"""
    num, den = float(x).as_integer_ratio()
    return num * ((1 << 149) // den)


class Exact:
    """The target of every sorted position of a case, exactly: atom b of position j is num[j][b] / den[j] (both ints).
    order / seg as given (an order entry that is not a row is left out of its episode's series and gets no target)."""

    def __init__(self, c, mode, lam=0.0, horizon=0, order=None):
        rows, seg, K = c["rows"], c["seg"], c["atoms"]
        order = c["order"] if order is None else order
        kind, tscore = c["tail"]
        delta = (c["vmax"] - c["vmin"]) / K
        a, den = float(lam).as_integer_ratio()
        q = den.bit_length() - 1
        H = 0 if lam == 0.0 else int(horizon)
        e0 = [1 << 149] + [0] * (K - 1)
        self.num, self.den, n_rows = {}, {}, len(rows)
        shifts = {}

        def shift(cdiff):
            if cdiff not in shifts:
                shifts[cdiff] = shift_doubles(cdiff, delta, K)
            return shifts[cdiff]
        for e in range(len(seg) - 1):
            pos = [j for j in range(seg[e], seg[e + 1]) if 0 <= order[j] < n_rows]
            S = [int(rows["score"][order[j]]) for j in pos] + ([int(tscore[e])] if kind[e] == 1 else [])
            if mode == 1:
                P = [[_units(x) for x in c["p_rows"][order[j], :K]] for j in pos] + ([e0] if kind[e] == 1 else [])
            for i, j in enumerate(pos):
                if mode == 0:
                    self.num[j], self.den[j] = shift_scatter(e0, *shift(S[-1] - S[i]), K), 1 << (149 + EF)
                    continue
                m = min(H, len(S) - 1 - i)
                R, W = [0] * K, 0
                for k in range(m, -1, -1):
                    T = shift_scatter(P[i + k], *shift(S[i + k] - S[i]), K)
                    up = q * (m - k)
                    R = [(t << up) + a * r for t, r in zip(T, R)]
                    W = (1 << up) + a * W
                self.num[j], self.den[j] = R, W << (149 + EF)

    def fraction(self, j, b):
        return Fraction(self.num[j][b], self.den[j])

    def bound_fraction(self, target):
        """max over the positions and atoms of |x - exact| / (2^-23 exact + 2^-149); where exact is 0, x must be +0 (inf if
        not).  target: float32 [n, K] by sorted position."""
        worst = 0.0
        for j, num in self.num.items():
            den = self.den[j]
            for b, x in enumerate(np.asarray(target[j], np.float32).tolist()):
                if num[b] == 0:
                    if x != 0.0 or math.copysign(1.0, x) < 0:
                        return float("inf")
                    continue
                px, qx = float(x).as_integer_ratio()
                # |px / qx - num / den| <= 2^-23 num / den + 2^-149, times qx den 2^149
                lhs = abs(px * den - num[b] * qx) << 149
                rhs = ((num[b] * qx) << 126) + qx * den
                if lhs:
                    worst = max(worst, lhs / rhs if lhs >> 900 <= rhs else float("inf"))
        return worst
