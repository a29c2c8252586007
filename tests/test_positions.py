"""Position records and the host half of re-analysis (tetris_mcts_amd/episodes.py: POSITION_DTYPE, ShardWriter, PositionLoader;
tetris_mcts_amd/reanalyse.py: rerecord_numpy; the refusals of play.py --save_positions and reanalyse.py).  No device."""
import builtins
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cli(name):
    spec_ = importlib.util.spec_from_file_location("tm_cli_positions_" + name, os.path.join(ROOT, name + ".py"))
    mod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(mod)
    return mod


def _refused(monkeypatch, cli, argv, package=False):
    """the SystemExit text of cli.main(argv), with every import of the package, the environment or torch forbidden; package: the
    package's modules may be imported, torch (through which alone the HIP library and a device are reached) and the environment not"""
    real = builtins.__import__

    def no_package(name, *a, **k):
        assert (package or not name.startswith("tetris_mcts_amd")) and name not in ("pyTetris", "torch"), "imported before the refusal"
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_package)
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    monkeypatch.setattr(builtins, "__import__", real)
    assert isinstance(e.value.code, str), "a refusal is a message"
    return e.value.code


def test_position_dtype_is_the_table():
    from tetris_mcts_amd.episodes import IDENTITY, POSITION_BYTES, POSITION_DTYPE, STATE_DTYPE
    assert POSITION_DTYPE.itemsize == POSITION_BYTES == 96
    want = dict(episode=(0, "<i4", ()), cycle=(4, "<i4", ()), slot=(8, "<i4", ()), move=(12, "<i4", ()), game=(16, "<u4", (16,)),
                line_stats=(80, "<i4", (4,)))
    assert set(POSITION_DTYPE.names) == set(want)
    for name, (off, fmt, shape) in want.items():
        dt, at = POSITION_DTYPE.fields[name][:2]
        assert at == off and dt.base == np.dtype(fmt) and dt.shape == shape, name
    for c in IDENTITY:        # the same four values, at the same offsets, as the State row
        assert POSITION_DTYPE.fields[c][1] == STATE_DTYPE.fields[c][1] and POSITION_DTYPE.fields[c][0] == STATE_DTYPE.fields[c][0]
    hdr = open(os.path.join(ROOT, "include", "tetris_mcts_hip.h")).read()
    assert "#define TM_POSITION_ROW_BYTES 96" in hdr


def _flush(n, ended=(), cycle=3, first_episode=0):
    """a flush as the device leaves it: n State rows and their position rows, `ended` with episode -1 and zeros"""
    from tetris_mcts_amd.episodes import POSITION_DTYPE, STATE_DTYPE
    rng = np.random.default_rng(n)
    rows, pos = np.zeros(n, STATE_DTYPE), np.zeros(n, POSITION_DTYPE)
    for t in (rows, pos):
        t["episode"], t["cycle"], t["slot"], t["move"] = first_episode + np.arange(n), cycle, np.arange(n) % 4, np.arange(n) // 4
    rows["score"] = rng.integers(0, 1000, n)
    pos["game"] = rng.integers(0, 2 ** 32, (n, 16), dtype=np.uint64).astype(np.uint32)
    pos["line_stats"] = rng.integers(0, 9, (n, 4))
    for i in ended:
        rows[i], pos[i] = np.zeros((), STATE_DTYPE), np.zeros((), POSITION_DTYPE)
        rows["episode"][i] = pos["episode"][i] = -1
    return rows, pos


def _raw(table, keep=None):
    """the bytes of the rows `keep` of a table, pad bytes included (fancy indexing of a padded dtype does not carry them)"""
    raw = np.ascontiguousarray(table).view(np.uint8).reshape(len(table), table.dtype.itemsize)
    return (raw if keep is None else raw[list(keep)]).tobytes()


def test_the_writer_drops_ended_rows_of_both_tables_with_one_mask(tmp_path):
    from tetris_mcts_amd.episodes import EPISODE_DTYPE, POSITION_DTYPE, ShardWriter, positions_file, positions_stem
    w = ShardWriter(str(tmp_path) + "/", "data", 3)
    rows, pos = _flush(10, ended=(2, 7))
    # (the mask is the State rows': a position that says -1 where its State row does not is kept, and found by the loader)
    names = w.write(rows, np.zeros(4, EPISODE_DTYPE), 0, 4, pos)
    assert len(names) == 3 and names[2] == positions_file(names[0]) == str(tmp_path / "positions3.part00000.npy")
    got_rows, got_pos = np.load(names[0]), np.load(names[2])
    keep = [i for i in range(10) if i not in (2, 7)]
    assert got_pos.dtype == POSITION_DTYPE and _raw(got_pos) == _raw(pos, keep) and _raw(got_rows) == _raw(rows, keep)
    # the next flush is the next part of both; without positions nothing but the two files of before is written
    rows2, pos2 = _flush(4, first_episode=10)
    names2 = w.write(rows2, np.zeros(4, EPISODE_DTYPE), 0, 4, pos2)
    assert names2[2].endswith("positions3.part00001.npy") and names2[0].endswith("data3.part00001.npy")
    assert len(w.write(rows2, np.zeros(4, EPISODE_DTYPE), 0, 4)) == 2
    assert sorted(os.listdir(tmp_path)) == sorted(["data3.part%05d.npy" % k for k in range(3)] + ["data3.episodes.part%05d.npy" % k for k in range(3)]
                                                   + ["positions3.part00000.npy", "positions3.part00001.npy"])
    with pytest.raises(ValueError):
        w.write(rows2, np.zeros(4, EPISODE_DTYPE), 0, 4, pos2[:3])
    # the names: never one that D/data* matches; ranked stems keep their rank
    assert positions_stem("D/data3.r1") == "D/positions3.r1" and positions_stem("D/run7") == "D/positions.run7"
    import glob
    assert not [f for f in glob.glob(str(tmp_path / "data*")) if "positions" in f]


def test_the_loader_pairs_parts_and_refuses_what_does_not_belong(tmp_path):
    from tetris_mcts_amd.episodes import EPISODE_DTYPE, PositionLoader, ShardWriter
    D = str(tmp_path) + "/"
    w = ShardWriter(D, "data", 3)
    a, pa = _flush(10, ended=(1,))
    b, pb = _flush(6, first_episode=10)
    fa, fb = w.write(a, np.zeros(4, EPISODE_DTYPE), 0, 4, pa), w.write(b, np.zeros(4, EPISODE_DTYPE), 0, 4, pb)
    for given in ([D + "data3"], [fb[0], fa[0]], [D + "data3", fa[0]]):
        L = PositionLoader(given)
        assert L.files == [fa[0], fb[0]] and L.position_files == [fa[2], fb[2]] and L.counts == [9, 6] and L.length == 15
        keep = [0] + list(range(2, 10))
        assert _raw(L.positions) == _raw(pa, keep) + _raw(pb) and _raw(L.rows) == _raw(a, keep) + _raw(b)
    # a row whose identity differs: each of the four values
    good = np.load(fb[2])
    for col in ("episode", "cycle", "slot", "move"):
        bad = good.copy()
        bad[col][4] += 1
        np.save(fb[2], bad)
        with pytest.raises(ValueError) as e:
            PositionLoader([D + "data3"])
        assert fb[2] in str(e.value) and "row 4" in str(e.value), (col, str(e.value))
    # a shorter part
    np.save(fb[2], good[:5])
    with pytest.raises(ValueError) as e:
        PositionLoader([D + "data3"])
    assert fb[2] in str(e.value) and "5 rows" in str(e.value) and "row 5" in str(e.value)
    # a missing part
    os.remove(fb[2])
    with pytest.raises(ValueError) as e:
        PositionLoader([D + "data3"])
    assert fb[2] in str(e.value) and "no position shard" in str(e.value)
    assert PositionLoader([fa[0]]).length == 9


def test_play_refuses_save_positions_without_save_before_anything_is_imported(monkeypatch):
    msg = _refused(monkeypatch, _cli("play"), ["--agent_type", "ValueSim", "--n_games", "8", "--save_positions"])
    assert "--save_positions" in msg and "needs --save" in msg


def test_reanalyse_refusals_come_before_anything_is_imported(monkeypatch, tmp_path):
    from tetris_mcts_amd import episodes, reanalyse as RA
    from tetris_mcts_amd.episodes import EPISODE_DTYPE, ShardWriter
    cli = _cli("reanalyse")
    D, R = str(tmp_path / "D") + "/", str(tmp_path / "R")
    rows, pos = _flush(8)
    names = ShardWriter(D, "data", 3).write(rows, np.zeros(4, EPISODE_DTYPE), 0, 4, pos)
    for given in ([D + "data3"], [D + "data*"], [D + "*"], [names[0]]):
        assert RA.choose_inputs(given) == [names[0]], given
    assert episodes.positions_file(D + "run7.r1.part00002.npy") == D + "positions.run7.r1.part00002.npy"
    base = ["--data_paths", D + "data3", "--out_dir", R]
    for agent, words in (("Vanilla", ("Vanilla", "rollouts", "no net")), ("VanillaC", ("VanillaC", "rollouts")),
                         ("DistValueSim", ("DistValueSim", "no distribution"))):
        msg = _refused(monkeypatch, cli, base + ["--agent_type", agent])
        assert all(w in msg for w in words), msg
    assert "--agent_type is required" in _refused(monkeypatch, cli, base)
    msg = _refused(monkeypatch, cli, ["--data_paths", D + "data3", "--out_dir", D, "--agent_type", "ValueSim"], package=True)
    assert "--out_dir" in msg and "directory of" in msg and names[0] in msg
    # an older stem without positions refuses a run that reads it, not one that --last_nfiles keeps away from it
    old = ShardWriter(D, "data", 2).write(rows, np.zeros(4, EPISODE_DTYPE), 0, 4)
    os.utime(old[0], (1, 1))
    both = ["--data_paths", D + "data*", "--out_dir", R, "--agent_type", "ValueSimLP"]
    msg = _refused(monkeypatch, cli, both, package=True)
    assert "no positions beside the data" in msg and old[0] in msg
    assert cli.check(cli.build_parser().parse_args(both + ["--last_nfiles", "1"])) is None
    os.remove(names[2])
    msg = _refused(monkeypatch, cli, base + ["--agent_type", "ValueSimLP"], package=True)
    assert "no positions beside the data" in msg and names[0] in msg and names[2] in msg
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert "one process" in _refused(monkeypatch, cli, base + ["--agent_type", "ValueSim"])
    assert not os.path.exists(R)


# ---- rerecord_numpy on hand-made rows ----
def _game(rows16=None, piece=2, rot=0, x=3, y=0, combo=-1, score=0, lines=0, ended=False):
    g = np.zeros(16, np.uint32)
    r = np.zeros(20, np.uint16) if rows16 is None else np.asarray(rows16, np.uint16)
    g[:10] = r.view(np.uint32)
    g[10] = piece | (rot << 8) | ((x & 0xFF) << 16) | ((y & 0xFF) << 24)
    g[11] = (1 << 8 if ended else 0) | ((combo & 0xFFFF) << 16)
    g[12], g[13], g[14], g[15] = 1, 77, score, lines
    return g


def _hand_made():
    """three positions and State rows that belong to them"""
    from tetris_mcts_amd.episodes import POSITION_DTYPE, STATE_DTYPE
    from tetris_mcts_amd.reanalyse import render_boards_numpy
    floor = np.zeros(20, np.uint16)
    floor[19], floor[18] = 0x3FE, 0x0F0
    games = np.stack([_game(), _game(floor, piece=0, rot=1, x=4, y=5, combo=2, score=340, lines=3),
                      _game(floor, piece=6, rot=3, x=-1 & 0xFF, y=10, combo=0, score=2 ** 20 + 5, lines=41)])
    pos, old = np.zeros(3, POSITION_DTYPE), np.zeros(3, STATE_DTYPE)
    pos["game"], pos["line_stats"] = games, [[0, 0, 0, 0], [1, 1, 0, 0], [30, 4, 1, 0]]
    for t in (pos, old):
        t["episode"], t["cycle"], t["slot"], t["move"] = [5, 9, 9], 4, [0, 3, 1], [0, 17, 18]
    old["combo"], old["lines"], old["score"] = [-1, 2, 0], [0, 3, 41], [0, 340, 2 ** 20 + 5]
    old["line_stats"], old["board"], old["action"] = pos["line_stats"], render_boards_numpy(games), [3, 0, 6]
    old["value"], old["variance"], old["child_stats"], old["policy"] = 1.5, 2.5, 7.0, 1 / 7
    old.view(np.uint8).reshape(3, 368)[:, 365:] = [[1, 2, 3]] * 3          # pad bytes: copied as they are
    return old, pos


def test_the_rendering_of_a_packed_game():
    from tetris_mcts_amd.reanalyse import render_boards_numpy
    old, pos = _hand_made()
    b = render_boards_numpy(pos["game"])
    assert b.dtype == np.int8 and b.shape == (3, 20, 10)
    # game 0: an empty well and the T piece in its spawn box at (3, 0): (1,0), (0,1), (1,1), (2,1)
    want = np.zeros((20, 10), np.int8)
    for c, r in ((4, 0), (3, 1), (4, 1), (5, 1)):
        want[r, c] = -1
    assert (b[0] == want).all()
    # game 1: rows 18 and 19 locked, a vertical I in column 6 from row 5
    assert b[1, 19].tolist() == [0] + [1] * 9 and b[1, 18].tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 0, 0]
    assert [tuple(v) for v in np.argwhere(b[1] == -1)] == [(5, 6), (6, 6), (7, 6), (8, 6)]
    ended = render_boards_numpy(np.stack([_game(ended=True)]))
    assert not ended.any(), "an ended game shows no falling piece"


def test_rerecord_numpy_copies_recomputes_and_takes_the_search():
    from tetris_mcts_amd.reanalyse import rerecord_numpy
    old, pos = _hand_made()
    stats = np.zeros((3, 3, 7), np.float32)
    stats[0, 0] = [3, 1, 4, 1, 5, 9, 2]
    stats[1, 0] = [2 ** 24, 1, 1, 1, 1, 1, 1]          # the float32 sum in index order: the ones are lost one by one
    stats[2, 0] = 0                                    # no visit: NaN
    stats[:, 1:] = np.arange(42, dtype=np.float32).reshape(3, 2, 7) / 3
    value, variance = np.array([10, 20, 30], np.float32), np.array([.5, .25, .125], np.float32)
    new, fault = rerecord_numpy(old, pos, stats, value, variance)
    assert fault is None
    for c in ("episode", "cycle", "slot", "move", "action", "combo", "lines", "score", "line_stats", "board"):
        assert new[c].tobytes() == old[c].tobytes(), c
    assert new.view(np.uint8).reshape(3, 368)[:, 365:].tolist() == [[1, 2, 3]] * 3
    assert new["value"].tolist() == [10, 20, 30] and new["variance"].tolist() == [.5, .25, .125]
    assert new["child_stats"].tobytes() == stats.tobytes()
    assert new["policy"][0].tobytes() == (stats[0, 0] / np.float32(25)).tobytes()
    assert new["policy"][1].tobytes() == (stats[1, 0] / np.float32(2 ** 24)).tobytes(), "the sum is float32, added in index order"
    assert np.isnan(new["policy"][2]).all()
    # the recomputed columns come from the GAME: an old row that says otherwise is the fault, whatever it says
    for group, edit in ((0, lambda r: r["score"].__setitem__(1, r["score"][1] ^ 1)), (0, lambda r: r["combo"].__setitem__(1, 3)),
                        (0, lambda r: r["lines"].__setitem__(1, 4)), (1, lambda r: r["line_stats"].__setitem__((1, 3), 1)),
                        (2, lambda r: r["board"].__setitem__((1, 0, 9), 1))):
        bad = old.copy()
        edit(bad)
        new2, fault = rerecord_numpy(bad, pos, stats, value, variance)
        assert fault == (1, group, 1), (group, fault)
        for c in ("combo", "lines", "score", "line_stats", "board"):
            assert new2[c].tobytes() == new[c].tobytes(), c
    # two bad rows: the first one and the count; a row with two bad groups names the lower; an ended game has no row
    bad = old.copy()
    bad["board"][2, 3, 3] = 1
    bad["line_stats"][2, 0] += 1
    bad["board"][0, 19, 0] = 1
    assert rerecord_numpy(bad, pos, stats, value, variance)[1] == (0, 2, 2)
    assert rerecord_numpy(bad[1:], pos[1:], stats[1:], value[1:], variance[1:])[1] == (1, 1, 1)
    over = pos.copy()
    over["game"][2, 11] |= 1 << 8
    old_over = old.copy()
    old_over["board"][2][old_over["board"][2] == -1] = 0          # (its board is the well alone: only the flag differs)
    assert rerecord_numpy(old_over, over, stats, value, variance)[1] == (2, 3, 1)
