"""The request cap's arithmetic: a launch of the value net serves the first min(n, cap) dense positions of the request list,
counted through the segments cyclically from segment `rot`, and tells the tree kernel how many entries of every segment that is.
tm_request_served and tm_request_at are host loops over the three one-line formulas the kernels share with them (valuenet.hip
req_segment, req_served, req_entry); the kernels' own prefix and lookup (shuffles and ballots over the same formulas, in k_vn_conv,
k_vn_fc1 and their split-precision twins) are held by the bit-identity tests of tests/test_gpu_request_cap.py, not here.  Held to
the definition, without a GPU: the served counts add up to the positions served, never exceed a segment's entries, the positions
served are exactly the entries below the served counts, and `rot` only changes the order the segments are counted in."""
import ctypes as C

import numpy as np
import pytest

SEGS = (1, 2, 64)


def _lib():
    from tetris_mcts_amd import _lib as L
    return L.lib()


def _served(lib, counts, rot, cap):
    c = np.ascontiguousarray(counts, np.int32)
    out = np.full(len(c), -7, np.int32)
    n = lib.tm_request_served(c.ctypes.data_as(C.c_void_p), len(c), rot, cap, out.ctypes.data_as(C.c_void_p))
    return n, out


def _at(lib, counts, rot, slots, p):
    c = np.ascontiguousarray(counts, np.int32)
    out = np.zeros(3, np.int32)
    rc = lib.tm_request_at(c.ctypes.data_as(C.c_void_p), len(c), rot, slots, p, out.ctypes.data_as(C.c_void_p))
    return rc, tuple(int(x) for x in out)


def _count_vectors(segs):
    rng = np.random.default_rng(1000 + segs)
    vs = [rng.integers(0, 5, segs), rng.integers(0, 70, segs), np.where(rng.random(segs) < 0.5, 0, rng.integers(1, 9, segs))]
    one = np.zeros(segs, np.int64)
    one[segs - 1] = 3
    return [v.astype(np.int32) for v in vs + [one]]


@pytest.mark.parametrize("segs", SEGS)
def test_served_counts_and_positions_follow_the_definition(segs):
    lib = _lib()
    for counts in _count_vectors(segs):
        n = int(counts.sum())
        for rot in range(segs):
            order = [(i + rot) % segs for i in range(segs)]
            for cap in sorted({0, 1, max(n - 1, 0), n, n + 1}):
                n_eff, served = _served(lib, counts, rot, cap)
                want = n if cap == 0 else min(n, cap)
                assert n_eff == want and int(served.sum()) == want, (segs, rot, cap)
                assert (served >= 0).all() and (served <= counts).all(), (segs, rot, cap)
                # the definition: clamp(cap - entries before s in the rotated order, 0, count[s]); cap == 0: the counts
                before = 0
                for s in order:
                    assert served[s] == (counts[s] if cap == 0 else min(max(cap - before, 0), counts[s])), (segs, rot, cap, s)
                    before += counts[s]
                # positions [0, n_eff) <-> {(s, d): d < served[s]}, one to one, in the rotated order, entries ascending
                seen = []
                for p in range(n_eff):
                    rc, (s, d, at) = _at(lib, counts, rot, 1, p)
                    assert rc == 0 and 0 <= d < served[s], (segs, rot, cap, p, s, d)
                    assert at == s + segs * d
                    seen.append((s, d))
                assert len(set(seen)) == n_eff
                assert seen == [(s, d) for s in order for d in range(served[s])], (segs, rot, cap)
                # past the end of the list there is no position
                assert _at(lib, counts, rot, 1, n)[0] == -1


@pytest.mark.parametrize("segs", SEGS)
def test_rot_only_permutes_the_segments(segs):
    """counting from segment rot = counting from segment 0 of the list whose segments are rolled by rot"""
    lib = _lib()
    for counts in _count_vectors(segs):
        n = int(counts.sum())
        for rot in range(segs):
            rolled = np.roll(counts, -rot)
            for cap in sorted({0, 1, max(n - 1, 0), n, n + 1}):
                n_a, a = _served(lib, counts, rot, cap)
                n_b, b = _served(lib, rolled, 0, cap)
                assert n_a == n_b and (np.roll(a, -rot) == b).all(), (segs, rot, cap)
                for p in range(n_a):
                    (_, (s, d, _)), (_, (s0, d0, _)) = _at(lib, counts, rot, 1, p), _at(lib, rolled, 0, 1, p)
                    assert (s, d) == ((s0 + rot) % segs, d0)


def test_list_index_with_seven_slots_a_game_and_refused_arguments():
    lib = _lib()
    counts = np.array([9, 0, 15], np.int32)
    for p, (s, d) in enumerate([(2, d) for d in range(15)] + [(0, d) for d in range(9)]):
        rc, got = _at(lib, counts, 2, 7, p)
        assert rc == 0 and got == (s, d, (s + 3 * (d // 7)) * 7 + d % 7)
    assert _served(lib, counts, 3, 0)[0] == -1 and _served(lib, counts, -1, 0)[0] == -1 and _served(lib, counts, 0, -1)[0] == -1
    assert _served(lib, np.array([1, -1], np.int32), 0, 0)[0] == -1
    assert _at(lib, counts, 0, 0, 0)[0] == -1 and _at(lib, counts, 0, 1, -1)[0] == -1


def test_store_mirror_carries_the_cap_fields_last():
    from tetris_mcts_amd import _lib as L
    from tetris_mcts_amd import store as st
    names = [f[0] for f in L.TmStore._fields_]
    assert names[-3:] == ["eval_cap", "eval_rot", "eval_served"]
    assert st.GS["EVAL_ENTRY"] == 30 and st.GS["N_EVAL_DEFERRED"] == 31
    assert [k for k, v in st.GS.items() if v in (30, 31)] == ["EVAL_ENTRY", "N_EVAL_DEFERRED"]
