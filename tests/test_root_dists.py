"""Root-distribution records on the host (tetris_mcts_amd/episodes.py: ROOT_DIST_DTYPE, ShardWriter, RootDistLoader,
record_root_dists_numpy; tetris_mcts_amd/offline.py: fit_episodes_dist(bootstrap="search"); the refusals of tm_episode_record_root_dists,
play.py --save_root_dists, train.py --bootstrap search and reanalyse.py --root_dists).  No device."""
import builtins
import ctypes as C
import glob
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cli(name):
    spec_ = importlib.util.spec_from_file_location("tm_cli_root_dists_" + name, os.path.join(ROOT, name + ".py"))
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


def _raw(table, keep=None):
    raw = np.ascontiguousarray(table).view(np.uint8).reshape(len(table), table.dtype.itemsize)
    return (raw if keep is None else raw[list(keep)]).tobytes()


def _flush(n, ended=(), cycle=3, first_episode=0, atoms=50):
    """a flush as the device leaves it: n State rows, their position rows and their root-distribution rows, `ended` with episode -1
    and zeros"""
    from tetris_mcts_amd.episodes import POSITION_DTYPE, ROOT_DIST_DTYPE, STATE_DTYPE
    rng = np.random.default_rng(n)
    rows, pos, dist = np.zeros(n, STATE_DTYPE), np.zeros(n, POSITION_DTYPE), np.zeros(n, ROOT_DIST_DTYPE)
    for t in (rows, pos, dist):
        t["episode"], t["cycle"], t["slot"], t["move"] = first_episode + np.arange(n), cycle, np.arange(n) % 4, np.arange(n) // 4
    rows["score"] = np.arange(n) * 10
    rows.view(np.uint8).reshape(n, 368)[:, 365:] = 7              # pad bytes: kept as they are
    pos["game"] = rng.integers(0, 2 ** 32, (n, 16), dtype=np.uint64).astype(np.uint32)
    p = rng.random((n, atoms)).astype(np.float32)
    dist["dist"][:, :atoms] = p / p.sum(axis=1, keepdims=True)
    for i in ended:
        rows[i], pos[i], dist[i] = np.zeros((), STATE_DTYPE), np.zeros((), POSITION_DTYPE), np.zeros((), ROOT_DIST_DTYPE)
        rows["episode"][i] = pos["episode"][i] = dist["episode"][i] = -1
    return rows, pos, dist


def test_root_dist_dtype_is_the_table():
    from tetris_mcts_amd.episodes import IDENTITY, ROOT_DIST_BYTES, ROOT_DIST_DTYPE, STATE_DTYPE
    assert ROOT_DIST_DTYPE.itemsize == ROOT_DIST_BYTES == 272
    want = dict(episode=(0, "<i4", ()), cycle=(4, "<i4", ()), slot=(8, "<i4", ()), move=(12, "<i4", ()), dist=(16, "<f4", (64,)))
    assert set(ROOT_DIST_DTYPE.names) == set(want)
    for name, (off, fmt, shape) in want.items():
        dt, at = ROOT_DIST_DTYPE.fields[name][:2]
        assert at == off and dt.base == np.dtype(fmt) and dt.shape == shape, name
    for c in IDENTITY:
        assert ROOT_DIST_DTYPE.fields[c][1] == STATE_DTYPE.fields[c][1] and ROOT_DIST_DTYPE.fields[c][0] == STATE_DTYPE.fields[c][0]
    hdr = open(os.path.join(ROOT, "include", "tetris_mcts_hip.h")).read()
    assert "#define TM_ROOT_DIST_ROW_BYTES 272" in hdr and "tm_episode_record_root_dists(const tm_store *tree" in hdr


def test_the_writer_drops_ended_rows_of_all_three_tables_with_one_mask(tmp_path):
    from tetris_mcts_amd.episodes import (EPISODE_DTYPE, ROOT_DIST_DTYPE, ShardWriter, positions_file, rootdist_file, rootdist_stem)
    D = str(tmp_path) + "/"
    w = ShardWriter(D, "data", 3)
    rows, pos, dist = _flush(10, ended=(2, 7))
    ep = np.zeros(4, EPISODE_DTYPE)
    names = w.write(rows, ep, 0, 4, pos, dist)
    assert len(names) == 4 and names[2] == positions_file(names[0]) and names[3] == rootdist_file(names[0]) == D + "rootdist3.part00000.npy"
    keep = [i for i in range(10) if i not in (2, 7)]
    got = np.load(names[3])
    assert got.dtype == ROOT_DIST_DTYPE and _raw(got) == _raw(dist, keep)
    assert _raw(np.load(names[0])) == _raw(rows, keep) and _raw(np.load(names[2])) == _raw(pos, keep)
    # (the mask is the State rows': a distribution row that says -1 where its State row does not is kept, and found by the loader)
    rows2, pos2, dist2 = _flush(4, first_episode=10)
    dist2["episode"][1] = -1
    n2 = w.write(rows2, ep, 0, 4, root_dists=dist2)
    assert len(n2) == 3 and n2[2] == D + "rootdist3.part00001.npy" and n2[0] == D + "data3.part00001.npy"
    assert _raw(np.load(n2[2])) == _raw(dist2) and not os.path.exists(D + "positions3.part00001.npy")
    # without the new argument nothing new is written, and the old tables are the same bytes
    n3 = w.write(rows, ep, 0, 4, pos)
    assert len(n3) == 3 and _raw(np.load(n3[0])) == _raw(rows, keep) and not os.path.exists(D + "rootdist3.part00002.npy")
    with pytest.raises(ValueError, match="3 root-distribution rows for 4 State rows"):
        w.write(rows2, ep, 0, 4, root_dists=dist2[:3])
    # the names: nothing that D/data*, D/dist* or D/positions* matches; ranked stems keep their rank
    assert rootdist_stem("D/data3.r1") == "D/rootdist3.r1" and rootdist_stem("D/run7") == "D/rootdist.run7"
    assert rootdist_file("D/run7.r1.part00002.npy") == "D/rootdist.run7.r1.part00002.npy"
    for pattern in ("data*", "dist*", "positions*"):
        assert not [f for f in glob.glob(D + pattern) if "rootdist" in f], pattern
    assert len(glob.glob(D + "rootdist*")) == 2


def test_one_flush_with_both_companions_keeps_the_same_rows_in_all_three_tables(tmp_path):
    """2 slots x 3 moves, the smallest flush in which a dropped row sits between kept ones: ended rows first, in the middle, last"""
    from tetris_mcts_amd.episodes import (EPISODE_DTYPE, IDENTITY, POSITION_DTYPE, ROOT_DIST_DTYPE, STATE_DTYPE, RootDistLoader,
                                          ShardWriter, write_root_dist_head)
    D = str(tmp_path) + "/"
    tables = _flush(6)
    for t in tables:
        t["slot"], t["move"] = np.arange(6) % 2, np.arange(6) // 2            # move-major, slot-minor
    ended, keep = (0, 3, 5), [1, 2, 4]
    for t in tables:
        t[list(ended)] = np.zeros((), t.dtype)
        t["episode"][list(ended)] = -1
    rows, pos, dist = tables
    w = ShardWriter(D, "data", 3)
    names = w.write(rows, np.zeros(6, EPISODE_DTYPE), 0, 6, positions=pos, root_dists=dist)
    assert names == (D + "data3.part00000.npy", D + "data3.episodes.part00000.npy", D + "positions3.part00000.npy",
                     D + "rootdist3.part00000.npy"), "State, episodes, positions, rootdist"
    got = [np.load(names[i]) for i in (0, 2, 3)]
    assert [g.dtype for g in got] == [STATE_DTYPE, POSITION_DTYPE, ROOT_DIST_DTYPE]
    assert [len(g) for g in got] == [3, 3, 3], "the three tables have the same length"
    for g, t in zip(got, tables):
        assert _raw(g) == _raw(t, keep), "the kept rows' bytes"
        for c in IDENTITY:
            assert g[c].tolist() == got[0][c].tolist() == rows[c][keep].tolist(), c
    write_root_dist_head(D + "data3", 50, 0, 5000)
    L = RootDistLoader(D + "data3", positions=None)
    assert (L.files, L.position_files, L.dist_files) == ([names[0]], [names[2]], [names[3]])
    assert L.counts == [3] and L.length == 3
    assert (_raw(L.rows), _raw(L.positions), _raw(L.dists)) == (_raw(rows, keep), _raw(pos, keep), _raw(dist, keep))


def test_the_sidecar_is_written_once_and_must_agree(tmp_path):
    from tetris_mcts_amd.episodes import write_root_dist_head
    from tetris_mcts_amd.nodes import load_head
    stem = str(tmp_path / "D" / "data3")
    name = write_root_dist_head(stem, 50, 0, 5000)
    assert name == str(tmp_path / "D" / "rootdist3.head.npy")
    h = np.load(name)
    assert h.dtype == np.float64 and h.tolist() == [50.0, 0.0, 5000.0]
    before = open(name, "rb").read()
    assert write_root_dist_head(stem, 50, 0.0, 5000.0) == name and open(name, "rb").read() == before
    for other in ((7, 0, 5000), (50, -1, 5000), (50, 0, 4000)):
        with pytest.raises(ValueError, match="records a head"):
            write_root_dist_head(stem, *other)
    with pytest.raises(ValueError):
        write_root_dist_head(str(tmp_path / "E" / "data3"), 65, 0, 1)
    assert load_head([str(tmp_path / "D" / "rootdist3")]) == (50, 0.0, 5000.0)
    assert not glob.glob(str(tmp_path / "D" / "data*")) and not glob.glob(str(tmp_path / "D" / "dist*"))


def test_the_loader_pairs_parts_and_refuses_what_does_not_belong(tmp_path):
    from tetris_mcts_amd.episodes import EPISODE_DTYPE, RootDistLoader, ShardWriter, write_root_dist_head
    D = str(tmp_path) + "/"
    w = ShardWriter(D, "data", 3)
    ep = np.zeros(4, EPISODE_DTYPE)
    a, pa, da = _flush(10, ended=(1,))
    b, pb, db = _flush(6, first_episode=10)
    fa, fb = w.write(a, ep, 0, 4, pa, da), w.write(b, ep, 0, 4, pb, db)
    with pytest.raises(ValueError, match="head.npy is missing"):
        RootDistLoader([D + "data3"])
    write_root_dist_head(D + "data3", 50, 0, 5000)
    keep = [0] + list(range(2, 10))
    for given in ([D + "data3"], [fb[0], fa[0]], [D + "data3", fa[0]]):
        L = RootDistLoader(given)
        assert L.files == [fa[0], fb[0]] and L.dist_files == [fa[3], fb[3]] and L.position_files == [fa[2], fb[2]]
        assert L.counts == [9, 6] and L.length == 15 and (L.atoms, L.vmin, L.vmax) == (50, 0.0, 5000.0)
        assert _raw(L.dists) == _raw(da, keep) + _raw(db) and _raw(L.rows) == _raw(a, keep) + _raw(b)
        assert _raw(L.positions) == _raw(pa, keep) + _raw(pb)
    L = RootDistLoader([D + "data3"], positions=False)
    assert L.position_files is None and not hasattr(L, "positions") and L.length == 15
    good = np.load(fb[3])
    for col in ("episode", "cycle", "slot", "move"):
        bad = good.copy()
        bad[col][4] += 1
        np.save(fb[3], bad)
        with pytest.raises(ValueError) as e:
            RootDistLoader([D + "data3"])
        assert fb[3] in str(e.value) and "row 4" in str(e.value), (col, str(e.value))
    np.save(fb[3], good[:5])                                # a shorter part
    with pytest.raises(ValueError) as e:
        RootDistLoader([D + "data3"])
    assert fb[3] in str(e.value) and "5 rows" in str(e.value) and "row 5" in str(e.value)
    np.save(fb[3], good.astype(np.dtype([(n, good.dtype[n]) for n in good.dtype.names])))          # a packed copy is the same layout
    assert RootDistLoader([D + "data3"]).length == 15
    np.save(fb[3], np.zeros(6, np.float32))
    with pytest.raises(ValueError, match="another layout"):
        RootDistLoader([D + "data3"])
    os.remove(fb[3])                                        # a missing part
    with pytest.raises(ValueError) as e:
        RootDistLoader([D + "data3"])
    assert fb[3] in str(e.value) and "no root-distribution shard" in str(e.value)
    assert RootDistLoader([fa[0]]).length == 9
    # positions asked for and not there; not asked for where one is missing
    os.remove(fa[2])
    with pytest.raises(ValueError, match="no position shard"):
        RootDistLoader([fa[0]], positions=True)
    assert RootDistLoader([fa[0]]).position_files is None


def test_the_numpy_statement_on_hand_made_rows():
    from tetris_mcts_amd.episodes import ROOT_DIST_DTYPE, STATE_DTYPE, record_root_dists_numpy
    G, N = 5, 6
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 2 ** 32, (G, N, 64), dtype=np.uint64).astype(np.uint32)
    bits[0, 2, 3], bits[0, 2, 4], bits[3, 5, 0] = 0x7FC00001, 0xFFC12345, 0x7F800001            # NaNs with payloads
    node_dist = bits.view(np.float32)
    rows = np.zeros(G, STATE_DTYPE)
    rows["episode"], rows["cycle"], rows["slot"], rows["move"] = [4, -1, 6, 7, 8], 9, np.arange(G), [0, 0, 3, 2 ** 20, 1]
    roots = np.array([2, 1, N, 5, -1])                       # game 2: one past the pool; game 4: negative
    for atoms in (7, 50, 64):
        out = record_root_dists_numpy(rows, roots, node_dist, atoms)
        assert out.dtype == ROOT_DIST_DTYPE and len(out) == G
        got = out["dist"].view(np.uint32)
        assert (got[0, :atoms] == bits[0, 2, :atoms]).all() and (got[3, :atoms] == bits[3, 5, :atoms]).all(), "bits, NaN payloads kept"
        assert not got[:, atoms:].any(), "atoms beyond dist_bins are written as 0"
        assert not got[2].any() and not got[4].any(), "a root outside the pool is never an address"
        for c in ("episode", "cycle", "slot", "move"):
            assert out[c][[0, 2, 3, 4]].tolist() == rows[c][[0, 2, 3, 4]].tolist(), c
        assert out["episode"][1] == -1 and not np.frombuffer(_raw(out, [1]), np.uint8)[4:].any(), "an ended row: -1, then zeros"
    assert len(record_root_dists_numpy(rows[:2], roots, node_dist, 50)) == 2, "n rows of a larger store"
    with pytest.raises(ValueError):
        record_root_dists_numpy(rows, roots, node_dist, 65)
    with pytest.raises(ValueError):
        record_root_dists_numpy(rows, roots, node_dist[:3], 50)


def refused_root_dist_arguments(lib, ptr):
    """every refusal of tm_episode_record_root_dists returns hipErrorInvalidValue; `ptr`: a non-null, 4-byte aligned address that is
    never dereferenced (the checks come before the first HIP call)"""
    from tetris_mcts_amd import _lib
    from tetris_mcts_amd.store import KIND_DIST, KIND_VALUESIM
    INVALID, p = 1, C.c_void_p(ptr)

    def store(**kw):
        s = _lib.TmStore()
        s.n_games, s.max_nodes, s.kind, s.dist_bins, s.node_dist, s.gs = 8, 64, KIND_DIST, 50, ptr, ptr
        for k, v in kw.items():
            setattr(s, k, v)
        return C.byref(s)

    call = lib.tm_episode_record_root_dists
    assert call(None, p, 1, p, None) == INVALID and call(store(), None, 1, p, None) == INVALID and call(store(), p, 1, None, None) == INVALID
    for n in (-1, 9, 2 ** 31 - 1):
        assert call(store(), p, n, p, None) == INVALID, n
    for kw in (dict(kind=KIND_VALUESIM), dict(kind=5), dict(node_dist=None), dict(gs=None), dict(max_nodes=0), dict(max_nodes=-4),
               dict(dist_bins=0), dict(dist_bins=65), dict(dist_bins=-1), dict(n_games=0)):
        assert call(store(**kw), p, 1, p, None) == INVALID, kw
    for off in (1, 2, 3):
        assert call(store(), C.c_void_p(ptr + off), 1, p, None) == INVALID and call(store(), p, 1, C.c_void_p(ptr + off), None) == INVALID
    # nothing to do is not an error and launches nothing - unless an argument is refused whatever n
    assert call(store(), p, 0, p, None) == 0
    assert call(store(kind=KIND_VALUESIM), p, 0, p, None) == INVALID and call(store(), p, 0, C.c_void_p(ptr + 2), None) == INVALID


def test_refused_arguments_without_a_gpu():
    from tetris_mcts_amd import _lib
    buf = (C.c_char * 64)()
    refused_root_dist_arguments(_lib.lib(), (C.addressof(buf) + 15) // 16 * 16)


def test_play_refusals_come_before_anything_is_imported(monkeypatch):
    cli = _cli("play")
    base = ["--n_games", "8", "--save_root_dists"]
    msg = _refused(monkeypatch, cli, base + ["--agent_type", "DistValueSim"])
    assert "--save_root_dists" in msg and "needs --save" in msg
    for agent in ("ValueSim", "ValueSimLP", "ValueSimC", "Vanilla", "VanillaC"):
        msg = _refused(monkeypatch, cli, base + ["--save", "--agent_type", agent])
        assert "--save_root_dists" in msg and "DistValueSim" in msg and agent in msg, msg
    msg = _refused(monkeypatch, cli, base + ["--save", "--agent_type", "DistValueSim", "--valuenet_backend", "torch", "--dense_requests"])
    assert "--save_root_dists" in msg and "--dense_requests" in msg and "not been shown to work" in msg
    # it combines with the other records: these pass every refusal (and are stopped here at the first import)
    args = cli.build_parser().parse_args(base + ["--save", "--agent_type", "DistValueSim", "--save_positions", "--save_dist_nodes"])
    assert cli.check_save_root_dists(args) is None and cli.check_save_dist_nodes(args) is None
    assert cli.build_parser().parse_args([]).save_root_dists is False


def test_train_refusals_come_before_anything_is_imported(monkeypatch):
    cli = _cli("train")
    base = ["--data_paths", "x", "--bootstrap", "search"]
    msg = _refused(monkeypatch, cli, base + ["--td"])
    assert "--bootstrap search" in msg and "--head dist" in msg
    msg = _refused(monkeypatch, cli, base + ["--head", "value", "--td", "--td_lambda", "0.5"])
    assert "--bootstrap search" in msg and "--head dist" in msg
    for flag in ("--nodes", "--dist_nodes"):
        msg = _refused(monkeypatch, cli, base + ["--head", "dist", "--td", flag])
        assert "--bootstrap search" in msg and flag in msg, msg
    msg = _refused(monkeypatch, cli, base + ["--head", "dist"])
    assert "--bootstrap search" in msg and "needs --td" in msg
    msg = _refused(monkeypatch, cli, base + ["--head", "dist", "--td", "--bootstrap_rounds", "2"])
    assert "--bootstrap search" in msg and "--bootstrap_rounds" in msg
    # what is pinned stays: --td alone names --td_lambda, recorded values name --bootstrap net (and now --bootstrap search too)
    msg = _refused(monkeypatch, cli, ["--data_paths", "x", "--head", "dist", "--td"])
    assert "--td_lambda" in msg
    msg = _refused(monkeypatch, cli, ["--data_paths", "x", "--head", "dist", "--td", "--td_lambda", "0.5"])
    assert "--bootstrap net" in msg and "--bootstrap search" in msg
    # accepted: with and without a lambda; the head flags given are remembered for the comparison with the sidecar
    for flags in (["--td"], ["--td", "--td_lambda", "0.9"], ["--td", "--new"]):
        argv = base + ["--head", "dist", "--atoms", "7"] + flags
        args = cli.build_parser().parse_args(argv)
        assert cli.check_args(args, argv) is None and args.head_given == {"atoms": 7}


def test_train_takes_the_head_from_the_sidecar_and_refuses_another(monkeypatch, tmp_path):
    from tetris_mcts_amd.episodes import EPISODE_DTYPE, ShardWriter, write_root_dist_head
    cli = _cli("train")
    D = str(tmp_path) + "/"
    rows, pos, dist = _flush(8, atoms=7)
    ShardWriter(D, "data", 3).write(rows, np.zeros(4, EPISODE_DTYPE), 0, 4, root_dists=dist)
    base = ["--data_paths", D + "data*", "--head", "dist", "--td", "--bootstrap", "search"]
    with pytest.raises(SystemExit) as e:
        cli.main(base)
    assert "head.npy is missing" in str(e.value.code) and "--save_root_dists" in str(e.value.code)
    write_root_dist_head(D + "data3", 7, 0, 700)
    for flags, word in ((["--atoms", "50"], "--atoms 50"), (["--vmax", "5000"], "--vmax 5000"), (["--vmin", "-1"], "--vmin -1")):
        with pytest.raises(SystemExit) as e:
            cli.main(base + flags)
        assert word in str(e.value.code) and "sidecar" in str(e.value.code), e.value.code


def test_reanalyse_refusals_come_before_anything_is_imported(monkeypatch, tmp_path):
    from tetris_mcts_amd import reanalyse as RA
    from tetris_mcts_amd.episodes import EPISODE_DTYPE, ShardWriter, write_root_dist_head
    cli = _cli("reanalyse")
    D, R = str(tmp_path / "D") + "/", str(tmp_path / "R")
    rows, pos, dist = _flush(8)
    names = ShardWriter(D, "data", 3).write(rows, np.zeros(4, EPISODE_DTYPE), 0, 4, pos, dist)
    write_root_dist_head(D + "data3", 50, 0, 5000)
    for given in ([D + "data3"], [D + "data*"], [D + "*"], [names[0]]):
        assert RA.choose_inputs(given) == [names[0]], given
    base = ["--data_paths", D + "data3", "--out_dir", R]
    msg = _refused(monkeypatch, cli, base + ["--agent_type", "DistValueSim"])
    assert all(w in msg for w in ("DistValueSim", "no distribution", "--save_root_dists", "--root_dists")), msg
    for agent in ("ValueSim", "ValueSimLP", "ValueSimC"):
        msg = _refused(monkeypatch, cli, base + ["--agent_type", agent, "--root_dists"])
        assert "--root_dists" in msg and "DistValueSim" in msg and agent in msg, msg
    assert "rollouts" in _refused(monkeypatch, cli, base + ["--agent_type", "Vanilla", "--root_dists"])
    ok = base + ["--agent_type", "DistValueSim", "--root_dists", "--valuenet_backend", "hip_bf16x3"]
    args = cli.build_parser().parse_args(ok)
    assert cli.check(args) is None and args.head == (50, 0.0, 5000.0)
    args = cli.build_parser().parse_args(base + ["--agent_type", "ValueSim"])
    assert cli.check(args) is None and args.head is None
    # the sidecar and the shards are looked for with numpy alone: no torch, no HIP library, no environment
    head = D + "rootdist3.head.npy"
    os.rename(head, head + ".away")
    msg = _refused(monkeypatch, cli, ok, package=True)
    assert "--root_dists" in msg and head in msg and "missing" in msg
    os.rename(head + ".away", head)
    os.remove(names[3])
    msg = _refused(monkeypatch, cli, ok, package=True)
    assert "no root distributions beside the data" in msg and names[0] in msg and names[3] in msg
    os.remove(names[2])
    assert "no positions beside the data" in _refused(monkeypatch, cli, ok, package=True)
    assert not os.path.exists(R)


def _recording(tmp_path, atoms=20, corrupt=None):
    """a stem of synthetic episodes (two parts) with root-distribution shards beside it: (stem, the distributions by table row)"""
    import episode_targets_cases as K
    from tetris_mcts_amd.episodes import ROOT_DIST_DTYPE, rootdist_stem, write_root_dist_head
    rows, ep = K.make_table("pos")
    rows = rows[:K.G * 40]
    stem = str(tmp_path / "data4")
    K.write_shards(stem, rows, ep[ep["moves"] <= 2], split=K.G * 20)
    rng = np.random.default_rng(3)
    p = rng.random((len(rows), atoms)).astype(np.float32)
    p = (p / p.sum(axis=1, keepdims=True)).astype(np.float32)
    p[5] = 0
    p[5, atoms - 1] = 1                                      # all mass in the top atom
    dist = np.zeros(len(rows), ROOT_DIST_DTYPE)
    for c in ("episode", "cycle", "slot", "move"):
        dist[c] = rows[c]
    dist["dist"][:, :atoms] = p
    if corrupt:
        corrupt(dist)
    for k, part in enumerate((dist[:K.G * 20], dist[K.G * 20:])):
        np.save("%s.part%05d.npy" % (rootdist_stem(stem), k), part)
    write_root_dist_head(stem, atoms, 0, 40000)
    return stem, rows, dist["dist"].copy()


def test_lambda_zero_targets_are_the_recorded_distributions_bit_for_bit(tmp_path):
    import episode_targets_cases as K
    from tetris_mcts_amd import offline as O
    stem, rows, p = _recording(tmp_path)
    got = O.recorded_root_dists([stem], 20, 0, 40000, len(rows))
    assert got.dtype == np.float32 and got.shape == (len(rows), 64) and got.tobytes() == p.tobytes()
    order, seg = K.by_episode(rows)
    kind, score, _ = K.tails(rows, np.zeros(0, O.EPISODE_DTYPE), order, seg, final=False)
    target, weight, fault = O.dist_targets_numpy(rows, order, seg, kind, score, 20, 0.0, 40000.0, 1, 0.0, 64, 0, p_rows=got)
    assert fault == 0 and target.dtype == np.float32 and target.tobytes() == p[order, :20].tobytes() and (weight == 1).all()


def test_fit_episodes_dist_search_refusals(tmp_path):
    from tetris_mcts_amd import offline as O
    from tetris_mcts_amd.model_distributional import Model_Dist
    m = Model_Dist(atoms=20, device="cpu", seed=0, backend="torch")
    with pytest.raises(ValueError, match="bootstrap is 'net'"):
        O.fit_episodes_dist(m, ["nothing"], td=True, lam=0.5, bootstrap="recorded")
    with pytest.raises(ValueError, match="needs td=True"):
        O.fit_episodes_dist(m, ["nothing"], bootstrap="search")
    with pytest.raises(ValueError, match="rounds"):
        O.fit_episodes_dist(m, ["nothing"], td=True, bootstrap="search", rounds=2)
    with pytest.raises(ValueError, match="lam"):
        O.fit_episodes_dist(m, ["nothing"], td=True, lam=1.5, bootstrap="search")
    with pytest.raises(ValueError, match="no distribution"):
        O.fit_episodes_dist(m, ["nothing"], td=True)        # bootstrap="net" keeps its refusal
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        import episode_targets_cases as K
        from tetris_mcts_amd.episodes import rootdist_stem
        called = []
        kw = dict(td=True, bootstrap="search", vmin=0, vmax=40000, max_iters=2, batch_size=8, on_round=lambda *a: called.append(a))
        rows, ep = K.make_table("pos")
        bare = str(tmp_path / "bare" / "data4")
        K.write_shards(bare, rows[:K.G * 40], ep[ep["moves"] <= 2], split=K.G * 20)
        with pytest.raises(ValueError) as e:
            O.fit_episodes_dist(m, [bare], **kw)
        assert "no root-distribution shards" in str(e.value) and bare in str(e.value)
        stem, _, _ = _recording(tmp_path / "a")
        with pytest.raises(ValueError, match="recorded by a head"):
            O.fit_episodes_dist(m, [stem], **dict(kw, vmax=5000))
        with pytest.raises(ValueError, match="recorded by a head"):
            O.fit_episodes_dist(Model_Dist(atoms=50, device="cpu", seed=0, backend="torch"), [stem], **kw)
        for name, value in (("nan", np.nan), ("inf", np.inf), ("negative", -0.25)):
            stem, _, _ = _recording(tmp_path / name, corrupt=lambda d: d["dist"].__setitem__((K.G * 20 + 3, 4), value))
            with pytest.raises(ValueError) as e:
                O.fit_episodes_dist(m, [stem], **kw)
            assert rootdist_stem(stem) + ".part00001.npy" in str(e.value) and "row 3 " in str(e.value), str(e.value)
        # an atom of the padding is not the head's: it is not looked at
        stem, _, _ = _recording(tmp_path / "pad", corrupt=lambda d: d["dist"].__setitem__((2, 20), np.nan))
        assert O.recorded_root_dists([stem], 20, 0, 40000).shape == (K.G * 40, 64)
        assert not called and not os.path.exists("pytorch_model"), "refused before a target was computed"
    finally:
        os.chdir(cwd)


def test_the_search_route_on_the_host(tmp_path):
    """fit_episodes_dist(bootstrap="search") with a torch head on CPU tensors: nothing is predicted, on_round's p_rows are the
    file's, at lambda = 0 the targets handed to train_data are the recorded distributions bit for bit, with a lambda the numpy
    statement over them; the checkpoint is written"""
    import torch
    from tetris_mcts_amd import offline as O
    from tetris_mcts_amd.model_distributional import Model_Dist
    stem, rows, p = _recording(tmp_path)
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        table, stem_rows, eps, ep_stems = O.load_stems([stem])
        idx = O.episode_index(O.rows_tensor(table), stem_rows, eps, ep_stems)
        order = idx.order.numpy()
        for lam in (None, 0.9):
            m = Model_Dist(atoms=20, device="cpu", seed=0, backend="torch")
            m.inference_device = None                        # (a prediction would fail)
            seen = []
            res = O.fit_episodes_dist(m, [stem], td=True, lam=lam, horizon=8, vmin=0, vmax=40000, bootstrap="search", max_iters=2,
                                      batch_size=8, on_round=lambda r, data, q: seen.append((r, [d.clone() for d in data], q.clone())))
            assert len(seen) == 1 and [r["iters"] for r in res["rounds"]] == [2] and os.path.isfile("pytorch_model/model_checkpoint_dist")
            r, data, q = seen[0]
            assert q.numpy().tobytes() == p.tobytes(), "p_rows are the file's, by table row"
            if lam is None:
                assert data[1].numpy().tobytes() == p[order, :20].tobytes()
            else:
                want, _, _ = O.episode_dist_targets(table, idx, td=True, lam=lam, horizon=8, atoms=20, vmin=0, vmax=40000,
                                                    p_rows=torch.from_numpy(p), device="cpu")
                assert data[1].numpy().tobytes() == want.numpy().tobytes() and data[1].numpy().tobytes() != p[order, :20].tobytes()
    finally:
        os.chdir(cwd)
