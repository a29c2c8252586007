"""Tables and an EXACT oracle for the discounted offline targets (tetris_mcts_amd/offline.py: gamma, v_rows;
csrc/episode_targets.hip: tm_episode_targets_discounted), shared by tests/test_offline_discount.py and
tests/test_gpu_offline_discount.py.

The table: 37 episodes whose lengths go round 1, 2, 63, 64, 65, 130 - the kernel's 64-lane chunk, its neighbours and two
carries - laid out in a random permutation of the table's rows (`order` is what sorts them; `presorted` gives the same rows
sorted).  Scores are non-decreasing integers up to 10^6, values float32 in [0, 100], and a second set of values by table row
stands for a net's predictions (v_rows).  Every episode has a tail entry (its final score, value 0) that a case may use or not.

The oracle evaluates the recurrences of the definitions over dyadic rationals (num / 2^exp with Python ints: every input - an
int score, a float32 value, the doubles lambda and gamma - is one, and so is every sum and product of them), which is exact;
`forward_sums` evaluates the definitions themselves, the double sums, in fractions.Fraction, and the tests hold the one to the
other on the short episodes.  For position i the oracle keeps N_i, B_i (value_i = N_i / B_i; mode 0: B_i = 1) and the same with
absolute values, MN_i, so that the bound |value_i - exact_i| <= 2^-23 M_i, M_i = MN_i / B_i, is a comparison of integers."""
from fractions import Fraction

import numpy as np

LENGTHS = (1, 2, 63, 64, 65, 130)
N_SEG = 37
GAMMAS = (1.0, 0.999, 0.9, 0.5)
LAMBDAS = (0.0, 0.5, 0.9, 1.0)


class Dy:
    """num / 2^exp, exactly"""
    __slots__ = ("num", "exp")

    def __init__(self, num, exp=0):
        self.num, self.exp = num, exp

    @staticmethod
    def of(x):
        p, q = float(x).as_integer_ratio()
        return Dy(p, q.bit_length() - 1)

    def __mul__(self, o):
        return Dy(self.num * o.num, self.exp + o.exp)

    def __add__(self, o):
        e = max(self.exp, o.exp)
        return Dy((self.num << (e - self.exp)) + (o.num << (e - o.exp)), e)

    def __abs__(self):
        return Dy(abs(self.num), self.exp)

    def fraction(self):
        return Fraction(self.num, 1 << self.exp)


_tables = {}


def table(seed=0):
    """dict(rows STATE_DTYPE in table order, order int32, seg int32 [38], tail = (kind all 1, score, value 0), v_rows float32 by
    TABLE row, sorted = the rows sorted by episode and move)"""
    if seed in _tables:
        return _tables[seed]
    from tetris_mcts_amd.episodes import STATE_DTYPE
    rng = np.random.default_rng([77, seed])
    lengths = np.array([LENGTHS[e % len(LENGTHS)] for e in range(N_SEG)])
    n = int(lengths.sum())
    seg = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    srt = np.zeros(n, STATE_DTYPE)
    tscore = np.zeros(N_SEG, np.int32)
    for e in range(N_SEG):
        L = int(lengths[e])
        steps = rng.integers(0, 1_000_000 // (L + 1) + 1, L + 1)
        steps[rng.random(L + 1) < 0.3] = 0                                # moves that score nothing
        s = np.cumsum(steps)                                              # non-decreasing, at most 10^6
        a, b = seg[e], seg[e + 1]
        srt["episode"][a:b], srt["cycle"][a:b], srt["slot"][a:b], srt["move"][a:b] = e, 2, e % 5, np.arange(L)
        srt["score"][a:b], tscore[e] = s[:L], s[L]
    srt["value"] = rng.uniform(0, 100, n).astype(np.float32)
    srt["variance"] = rng.uniform(1e-3, 500, n).astype(np.float32)
    srt["child_stats"][:, 0, :] = rng.integers(0, 400, (n, 7)).astype(np.float32)
    srt["board"] = rng.integers(-2, 3, (n, 20, 10)).astype(np.int8)
    order = rng.permutation(n).astype(np.int32)                           # sorted position j lies at table row order[j]
    rows = np.zeros(n, STATE_DTYPE)
    rows[order] = srt
    v_rows = rng.uniform(0, 100, n).astype(np.float32)
    assert srt["score"].max() <= 10 ** 6 and tscore.max() <= 10 ** 6 and (np.diff(order) != 1).any()
    _tables[seed] = dict(rows=rows, order=order, seg=seg, v_rows=v_rows, sorted=srt,
                         tail=(np.ones(N_SEG, np.uint8), tscore, np.zeros(N_SEG, np.float32)))
    return _tables[seed]


def tails(t, final):
    kind, score, value = t["tail"]
    return (kind if final else np.zeros_like(kind)), score, value


def series(t, e, final, use_v_rows, order=None, seg=None):
    """(scores, values) of episode e as Python ints / floats, the tail included if `final`"""
    order, seg = t["order"] if order is None else order, t["seg"] if seg is None else seg
    pos = order[seg[e]:seg[e + 1]]
    v = (t["v_rows"] if use_v_rows else t["rows"]["value"])[pos]
    s = [int(x) for x in t["rows"]["score"][pos]] + ([int(t["tail"][1][e])] if final else [])
    return s, [float(x) for x in v] + ([float(t["tail"][2][e])] if final else [])


class Exact:
    """The exact targets of the first n_seg episodes: mode 1 (N_i, B_i, MN_i per sorted position) or mode 0 (D_i, 1, MD_i)."""

    def __init__(self, t, mode, lam, gamma, final, use_v_rows, n_seg=N_SEG, order=None, seg=None):
        seg = t["seg"] if seg is None else seg
        lam_d, gam, one = Dy.of(lam), Dy.of(gamma), Dy(1)
        self.N, self.B, self.M = {}, {}, {}
        for e in range(n_seg):
            s, v = series(t, e, final, use_v_rows, order, seg)
            K, rows = len(s), int(seg[e + 1] - seg[e])
            N = B = M = None
            for k in range(K - 1, -1, -1):
                vk = Dy.of(v[k])
                if mode == 0:                                             # D_k = r_k + gamma D_{k+1}; the last element is the end
                    if N is None:
                        N, M, B = Dy(0), Dy(0), one
                    else:
                        r = Dy(s[k + 1] - s[k])
                        N, M = r + gam * N, abs(r) + gam * M
                elif N is None:
                    N, M, B = vk, abs(vk), one
                else:                                                     # N_k = v_k + lam (gamma N_{k+1} + B_{k+1} r_k)
                    r = Dy(s[k + 1] - s[k])
                    N, M = vk + lam_d * (gam * N + B * r), abs(vk) + lam_d * (gam * M + B * abs(r))
                    B = one + lam_d * B
                if k < rows:
                    self.N[int(seg[e]) + k], self.B[int(seg[e]) + k], self.M[int(seg[e]) + k] = N, B, M

    def fraction(self, j):
        return self.N[j].fraction() / self.B[j].fraction()

    def bound(self, j):
        return self.M[j].fraction() / self.B[j].fraction()

    def bound_fraction(self, value, positions=None):
        """max over the positions of |value_j - exact_j| / (2^-23 M_j) (0 where both sides are 0; inf where only M is):
        |x B - N| 2^23 against MN, all brought to one power of two"""
        worst = 0.0
        for j in (sorted(self.N) if positions is None else positions):
            x, N, B, M = Dy.of(float(value[j])), self.N[j], self.B[j], self.M[j]
            lhs = abs(x * B + Dy(-N.num, N.exp))
            e = max(lhs.exp, M.exp)
            a, b = (lhs.num << (e - lhs.exp)) << 23, M.num << (e - M.exp)
            if a:
                worst = max(worst, float("inf") if b == 0 else a / b)           # (int / int: correctly rounded, whatever the sizes)
        return worst


def forward_sums(s, v, i, mode, lam, gamma):
    """the definitions as written, over Fractions: (value_i, M_i) of position i of the series (s, v)"""
    lam, gamma = Fraction(lam), Fraction(gamma)
    r = [Fraction(s[k + 1] - s[k]) for k in range(len(s) - 1)]
    if mode == 0:
        return (sum(gamma ** (k - i) * r[k] for k in range(i, len(r))), sum(gamma ** (k - i) * abs(r[k]) for k in range(i, len(r))))
    num = den = m = head = head_abs = Fraction(0)                         # head: sum_{j<k} gamma^j r_{i+j}
    w = g = Fraction(1)                                                   # lam^k (0^0 = 1), gamma^k
    for k in range(len(s) - i):
        T, A = head + g * Fraction(v[i + k]), head_abs + g * abs(Fraction(v[i + k]))
        num, m, den = num + w * T, m + w * A, den + w
        if i + k < len(r):
            head, head_abs = head + g * r[i + k], head_abs + g * abs(r[i + k])
        w, g = w * lam, g * gamma
    return num / den, m / den


_exact = {}


def exact(mode, lam, gamma, final, use_v_rows, n_seg=N_SEG):
    """the oracle of the table's first n_seg episodes, computed once (an oracle of more episodes serves fewer: pass
    `positions` to its bound_fraction)"""
    key = (mode, float(lam), float(gamma), bool(final), bool(use_v_rows))
    if key not in _exact or _exact[key][0] < n_seg:
        _exact[key] = (n_seg, Exact(table(), *key, n_seg=n_seg))
    return _exact[key][1]
