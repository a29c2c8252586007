"""Self-play records (csrc/episodes.hip, tetris_mcts_amd/episodes.py, scripts/episode_stats.py), what holds without a GPU: the
row layouts against the reference's State columns and the header, the argument checks of the three calls, the shard writer and
the loader on synthetic rows, the statistics script."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1     # hipErrorInvalidValue
# util/Data.py:14-26, class State: column -> (dtype, shape)
REFERENCE_STATE = {"episode": ("<i4", ()), "board": ("i1", (20, 10)), "policy": ("<f4", (7,)), "action": ("i1", ()),
                   "combo": ("<i4", ()), "lines": ("<i4", ()), "line_stats": ("<i4", (4,)), "score": ("<i4", ()),
                   "child_stats": ("<f4", (3, 7)), "cycle": ("<i4", ()), "value": ("<f4", ()), "variance": ("<f4", ())}


def _lib():
    import __graft_entry__ as ge
    if not os.path.exists(ge.LIB):
        ge.build()
    from tetris_mcts_amd import _lib
    return _lib


def _header():
    return open(os.path.join(ROOT, "include", "tetris_mcts_hip.h")).read()


def test_state_rows_have_the_references_columns_and_the_headers_size():
    from tetris_mcts_amd import episodes as E
    hdr = _header()
    cols = dict(REFERENCE_STATE, slot=("<i4", ()), move=("<i4", ()))
    assert set(E.STATE_DTYPE.names) == set(cols)
    for name, (fmt, shape) in cols.items():
        f = E.STATE_DTYPE.fields[name][0]
        assert f.base == np.dtype(fmt) and f.shape == shape, name
    assert E.STATE_DTYPE.itemsize == int(re.search(r"#define\s+TM_EPISODE_ROW_BYTES\s+(\d+)", hdr).group(1)) == 368
    assert E.EPISODE_DTYPE.itemsize == int(re.search(r"#define\s+TM_EPISODE_DONE_BYTES\s+(\d+)", hdr).group(1)) == 40
    assert E.SLOT_DW == int(re.search(r"#define\s+TM_EPISODE_SLOT_DW\s+(\d+)", hdr).group(1))
    # the offsets of the header's table; no two fields overlap and only the three pad bytes are left over
    want = dict(episode=0, cycle=4, slot=8, move=12, combo=16, lines=20, score=24, line_stats=28, value=44, variance=48,
                child_stats=52, policy=136, board=164, action=364)
    assert {n: E.STATE_DTYPE.fields[n][1] for n in E.STATE_DTYPE.names} == want
    used = np.zeros(368, int)
    for n in E.STATE_DTYPE.names:
        f, off = E.STATE_DTYPE.fields[n][:2]
        used[off:off + f.itemsize] += 1
    assert used[:365].tolist() == [1] * 365 and used[365:].tolist() == [0] * 3
    assert E.EPISODE_DTYPE.names == ("episode", "cycle", "slot", "moves", "score", "lines", "line_stats")
    assert all(E.EPISODE_DTYPE.fields[n][0].base == np.dtype("<i4") for n in E.EPISODE_DTYPE.names)
    assert [E.EPISODE_DTYPE.fields[n][1] for n in E.EPISODE_DTYPE.names] == [0, 4, 8, 12, 16, 20, 24]


def test_the_three_calls_are_declared_exported_and_bound():
    L = _lib()
    lib = L.lib()
    declared = set(re.findall(r"\bint\s+(tm_[a-z_0-9]+)\s*\(", _header()))
    for name in ("tm_episode_init", "tm_episode_record", "tm_episode_advance"):
        assert name in declared and hasattr(lib, name) and name in L.SYMBOLS, name
    import __graft_entry__ as ge
    assert "episodes.hip" in ge.SOURCES


def _env(L, n_games=8):
    """a description of the games whose pointers are never followed (every call below is refused before a launch)"""
    s = L.TmStore()
    s.n_games, s.max_nodes = n_games, 64
    for name in ("env_game", "env_line_stats", "gs", "node_rec", "obs_stat"):
        setattr(s, name, 4096)
    return s


def test_the_calls_refuse_bad_arguments_before_any_hip_call():
    L = _lib()
    lib = L.lib()
    p, null = C.c_void_p(4096), C.c_void_p(0)
    env, tree = _env(L), _env(L)
    init, rec, adv = lib.tm_episode_init, lib.tm_episode_record, lib.tm_episode_advance
    assert init(8, 0, null, p, null) == INVALID and init(8, 0, p, null, null) == INVALID
    for n in (0, -1):
        assert init(n, 0, p, p, null) == INVALID
    assert init(8, -1, p, p, null) == INVALID
    # record: env, stats, action, slot_state, rows (tree may be NULL, but not a tree of another batch)
    assert rec(None, C.byref(tree), p, p, 0, p, p, null) == INVALID
    for hole in range(4):
        a = [p, p, p, p]
        a[hole] = null
        assert rec(C.byref(env), C.byref(tree), a[0], a[1], 0, a[2], a[3], null) == INVALID, hole
        assert rec(C.byref(env), None, a[0], a[1], 0, a[2], a[3], null) == INVALID, hole
    for n in (0, -5):
        assert rec(C.byref(_env(L, n)), None, p, p, 0, p, p, null) == INVALID
    assert rec(C.byref(env), C.byref(_env(L, 9)), p, p, 0, p, p, null) == INVALID
    assert rec(C.byref(env), None, p, p, 0, p, C.c_void_p(4098), null) == INVALID       # rows are stored as dwords
    for field in ("env_game", "env_line_stats"):
        e = _env(L)
        setattr(e, field, None)
        assert rec(C.byref(e), None, p, p, 0, p, p, null) == INVALID, field
        assert adv(C.byref(e), 0, p, p, p, 8, null) == INVALID, field
    # advance: env, slot_state, counters, done, cap
    assert adv(None, 0, p, p, p, 8, null) == INVALID
    for hole in range(3):
        a = [p, p, p]
        a[hole] = null
        assert adv(C.byref(env), 0, *a, 8, null) == INVALID, hole
    for cap in (0, -2):
        assert adv(C.byref(env), 0, p, p, p, cap, null) == INVALID
    for n in (0, -5):
        assert adv(C.byref(_env(L, n)), 0, p, p, p, 8, null) == INVALID


# ---- synthetic rows ----
def _flush(moves, G, first_move, ids, ended_slots=(), cycle=3):
    """`moves` moves of G slots, move-major: slot g plays episode ids[g]; an ended slot's rows carry episode -1 and zeros"""
    from tetris_mcts_amd.episodes import STATE_DTYPE
    rows = np.zeros(moves * G, STATE_DTYPE)
    for m in range(moves):
        for g in range(G):
            r = rows[m * G + g]
            if g in ended_slots:
                r["episode"] = -1
                continue
            r["episode"], r["cycle"], r["slot"], r["move"] = ids[g], cycle, g, first_move + m
            r["lines"], r["score"], r["action"] = 10 * g + first_move + m, 100 * g + first_move + m, (m + g) % 7
            r["board"][g % 20, m % 10] = 1
            r["policy"] = np.arange(7) / 21.0
    return rows


def _cat(*tables):
    """one after the other in the tables' own layout (np.concatenate packs the fields)"""
    out = np.zeros(sum(len(t) for t in tables), tables[0].dtype)
    at = 0
    for t in tables:
        for name in t.dtype.names:
            out[name][at:at + len(t)] = t[name]
        at += len(t)
    return out


def _done(cap, entries, cycle=3):
    from tetris_mcts_amd.episodes import EPISODE_DTYPE
    d = np.zeros(cap, EPISODE_DTYPE)
    for i, (ep, slot, moves, score, lines) in enumerate(entries):
        d[i] = (ep, cycle, slot, moves, score, lines, [lines, 0, 0, 0])
    return d


def test_writer_and_loader_round_trip(tmp_path):
    from tetris_mcts_amd import episodes as E
    d = str(tmp_path) + "/sub/"                       # (created by the writer)
    w = E.ShardWriter(d, "data", 3)
    assert (w.part, w.next_id) == (0, 0)
    a = _flush(4, 3, 0, [0, 1, 2], ended_slots=(1,))
    names = w.write(a, _done(12, [(1, 1, 5, 777, 9)]), 1, 12)
    assert [os.path.basename(n) for n in names] == ["data3.part00000.npy", "data3.episodes.part00000.npy"]
    b = _flush(2, 3, 4, [0, 3, 2])
    w.write(b, _done(12, []), 0, 12)
    assert sorted(os.listdir(d)) == ["data3.episodes.part00000.npy", "data3.episodes.part00001.npy", "data3.part00000.npy",
                                     "data3.part00001.npy"]
    # episode == -1 rows are dropped, everything else is kept byte for byte in the order written
    kept = _cat(a[a["episode"] != -1], b)
    ld = E.EpisodeLoader([d + "data3"], by_episode=False)
    assert ld.length == len(kept) == 8 + 6 and ld.rows.tobytes() == kept.tobytes() and ld.rows.dtype == E.STATE_DTYPE
    for c in E.STATE_DTYPE.names:
        assert np.array_equal(getattr(ld, c), kept[c]), c
    assert ld.getScore(10 ** 6) == kept["score"][-1] and ld.getLines(-4) == kept["lines"][0]
    assert ld.getBoard(2).shape == (20, 10) and ld.getPolicy(2).shape == (7,) and ld.getCycle(0) == 3 and ld.getCombo(0) == 0
    assert ld.episodes.dtype == E.EPISODE_DTYPE and ld.episodes.tobytes() == _done(1, [(1, 1, 5, 777, 9)]).tobytes()
    # the shards named one by one give the same table
    assert E.EpisodeLoader(sorted(n for n in (d + f for f in os.listdir(d)) if ".episodes." not in n), by_episode=False).rows.tobytes() == kept.tobytes()
    # by_episode: every episode contiguous, in the order of its moves, episodes ascending
    le = E.EpisodeLoader(d + "data3")
    assert le.length == ld.length
    runs = [(int(e), le.move[le.episode == e].tolist()) for e in dict.fromkeys(le.episode.tolist())]
    assert [e for e, _ in runs] == [0, 2, 3]
    for e, mv in runs:
        idx = np.nonzero(le.episode == e)[0]
        assert (np.diff(idx) == 1).all(), e
        assert mv == sorted(mv) and len(set(mv)) == len(mv), e
    assert runs[0][1] == list(range(6)) and runs[2][1] == [4, 5]
    # opening over existing parts continues the numbering and the episode ids (3 is under way in the last rows written)
    w2 = E.ShardWriter(d, "data", 3)
    assert (w2.part, w2.next_id) == (2, 4)
    w2.write(_flush(1, 3, 6, [0, 3, 2]), _done(12, []), 0, 12)
    assert os.path.exists(d + "data3.part00002.npy") and E.EpisodeLoader(d + "data3").length == ld.length + 3
    # another cycle and another rank are other stems
    assert E.ShardWriter(d, "data", 4).part == 0 and E.ShardWriter(d, "data", 3, rank=1).stem.endswith("data3.r1")


def test_an_overflow_of_the_episode_log_raises(tmp_path):
    from tetris_mcts_amd import episodes as E
    w = E.ShardWriter(str(tmp_path) + "/", "data", 0)
    with pytest.raises(RuntimeError, match="overflow"):
        w.write(_flush(1, 3, 0, [0, 1, 2]), _done(2, [(0, 0, 1, 1, 1), (1, 1, 1, 1, 1)]), 3, 2)
    assert os.listdir(str(tmp_path)) == []


def test_the_recorder_needs_an_agent():
    import inspect
    from tetris_mcts_amd.episodes import EpisodeRecorder
    sig = inspect.signature(EpisodeRecorder.__init__).parameters
    assert list(sig)[1:] == ["save_dir", "save_file", "cycle", "n_games", "ring_moves", "device"]
    assert sig["ring_moves"].default == 64 and sig["device"].default == "cuda"
    rec = EpisodeRecorder.__new__(EpisodeRecorder)        # (no device: add refuses before it touches one)
    with pytest.raises(TypeError, match="TreeAgent"):
        rec.add(agent=None, game=object())


def test_episode_stats_reports_finished_and_censored_episodes(tmp_path):
    from tetris_mcts_amd import episodes as E
    d = str(tmp_path) + "/"
    w = E.ShardWriter(d, "data", 3)
    # slots 0 and 1 finish episodes 0 and 1 after 3 and 4 moves; episode 2 (slot 0 again) is under way at the end
    rows = _cat(_flush(3, 1, 0, [0]), _flush(4, 1, 0, [1]), _flush(2, 1, 0, [2]))
    rows["lines"][-1] = 6
    w.write(rows, _done(4, [(0, 0, 3, 1200, 4), (1, 1, 4, 300, 11)]), 2, 4)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "episode_stats.py"), d + "data3"], capture_output=True,
                         text=True, timeout=120, check=True).stdout.strip().splitlines()
    assert len(out) == 1
    r = json.loads(out[0])
    assert r["state_rows"] == 9 and r["files"] == 1
    assert r["finished"]["count"] == 2
    assert r["finished"]["lines"] == dict(mean=7.5, median=7.5, max=11)
    assert r["finished"]["score"] == dict(mean=750.0, median=750.0, max=1200)
    assert r["under_way_at_the_end"]["count"] == 1
    assert r["under_way_at_the_end"]["lines_so_far"] == dict(mean=6.0, median=6.0, max=6)
    assert "censored" in r["censoring"] and "biased low" in r["censoring"]


def test_play_save_needs_an_agent_and_the_other_storage_flags_stay_refused():
    import play
    with pytest.raises(SystemExit) as e:
        play.main(["--save"])
    assert "--save" in str(e.value.code) and "--agent_type" in str(e.value.code)
    for flag in ("--save_tree", "--gui", "--interactive"):
        with pytest.raises(SystemExit) as e:
            play.main(["--agent_type", "Vanilla", flag])
        assert flag in str(e.value.code) and "--save " not in str(e.value.code) + " "
