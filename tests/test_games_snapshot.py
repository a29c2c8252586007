"""Game snapshots (csrc/games_snapshot.hip, tetris_mcts_amd/games.py, play.py --games_in / --games_out / --games_every): what
holds without a GPU - the refusals of the four calls, the command line, the file, the loader's refusals that need no device, the
numpy statement of the fault rule against ENGINE_SPEC.md's cell lists and the oracle engine, and the new kernels' resources."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

import games_snapshot_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("tm_env_check", "tm_env_save", "tm_env_load", "tm_episode_resume")


def _lib():
    import __graft_entry__ as ge
    if not os.path.exists(ge.LIB):
        ge.build()
    from tetris_mcts_amd import _lib
    return _lib


def _cli():
    spec_ = importlib.util.spec_from_file_location("tm_play_cli_games", os.path.join(ROOT, "play.py"))
    mod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(mod)
    return mod


def test_the_four_calls_are_declared_exported_and_bound():
    L = _lib()
    hdr = open(os.path.join(ROOT, "include", "tetris_mcts_hip.h")).read()
    declared = set(re.findall(r"\bint\s+(tm_[a-z_0-9]+)\s*\(", hdr))
    for name in CALLS:
        assert name in declared and hasattr(L.lib(), name) and name in L.SYMBOLS, name
    import __graft_entry__ as ge
    assert "games_snapshot.hip" in ge.SOURCES
    from tetris_mcts_amd import games as G
    for name, bit in (("PIECE", G.BAD_PIECE), ("ROT", G.BAD_ROT), ("ROWS", G.BAD_ROWS), ("PLACE", G.BAD_PLACE),
                      ("FIELDS", G.BAD_FIELDS), ("LINE_STATS", G.BAD_LINE_STATS)):
        assert int(re.search(r"#define\s+TM_GAME_BAD_%s\s+(\d+)" % name, hdr).group(1)) == bit == getattr(K, name)


def test_the_calls_refuse_bad_arguments_before_any_hip_call():
    """hipErrorInvalidValue (1) before anything touches a device: the pointers are never dereferenced"""
    L = _lib()
    lib = L.lib()
    buf = (C.c_char * 320)()
    b = (C.addressof(buf) + 15) // 16 * 16
    s = L.TmStore()
    s.n_games, s.app, s.env_game, s.env_line_stats = 4, 1, b, b

    def store(**kw):
        t = L.TmStore()
        C.memmove(C.byref(t), C.byref(s), C.sizeof(s))
        for k, v in kw.items():
            setattr(t, k, v)
        return C.byref(t)

    # tm_env_check(games, line_stats | NULL, n, app, fault, n_bad, stream)
    good = [b, b, 4, 1, b, b, None]
    for k in (0, 4, 5):
        bad = list(good)
        bad[k] = None
        assert lib.tm_env_check(*bad) == 1, k
    for k in (0, 1, 4, 5):
        for off in (1, 2, 3):
            bad = list(good)
            bad[k] = b + off
            assert lib.tm_env_check(*bad) == 1, (k, off)
    for n in (0, -1, -2 ** 31):
        assert lib.tm_env_check(b, b, n, 1, b, b, None) == 1 and lib.tm_env_check(b, None, n, 1, b, b, None) == 1
    for app in (0, -1):
        assert lib.tm_env_check(b, b, 4, app, b, b, None) == 1
    # tm_env_save(s, games, line_stats, stream)
    assert lib.tm_env_save(None, b, b, None) == 1 and lib.tm_env_save(store(), None, b, None) == 1
    assert lib.tm_env_save(store(), b, None, None) == 1
    assert lib.tm_env_save(store(), b + 2, b, None) == 1 and lib.tm_env_save(store(), b, b + 1, None) == 1
    for kw in (dict(n_games=0), dict(n_games=-3), dict(env_game=None), dict(env_line_stats=None)):
        assert lib.tm_env_save(store(**kw), b, b, None) == 1, kw
    # tm_env_load(s, games, line_stats, fault, n_bad, stream)
    good = [store(), b, b, b, b, None]
    for k in range(5):
        bad = list(good)
        bad[k] = None
        assert lib.tm_env_load(*bad) == 1, k
    for k in range(1, 5):
        bad = list(good)
        bad[k] = b + 2
        assert lib.tm_env_load(*bad) == 1, k
    for kw in (dict(n_games=0), dict(app=0), dict(app=-1), dict(env_game=None), dict(env_line_stats=None)):
        assert lib.tm_env_load(store(**kw), b, b, b, b, None) == 1, kw
    # tm_episode_resume(n_games, first_id, move_idx, slot_state, counters, stream)
    good = [4, 0, b, b, b, None]
    for k in (2, 3, 4):
        bad = list(good)
        bad[k] = None
        assert lib.tm_episode_resume(*bad) == 1, k
        bad[k] = b + 2
        assert lib.tm_episode_resume(*bad) == 1, k
    assert lib.tm_episode_resume(0, 0, b, b, b, None) == 1 and lib.tm_episode_resume(-1, 0, b, b, b, None) == 1
    assert lib.tm_episode_resume(4, -1, b, b, b, None) == 1
    del buf


def test_play_cli_defaults_and_help():
    cli = _cli()
    p = cli.build_parser()
    a = p.parse_args([])
    assert a.games_out is None and a.games_in is None and a.games_every == 0
    a = p.parse_args(["--games_out", "x/games", "--games_in", "y/games", "--games_every", "5"])
    assert (a.games_out, a.games_in, a.games_every) == ("x/games", "y/games", 5)
    text = " ".join(p.format_help().split())
    assert "--seed does not touch loaded games" in text and "does not touch games loaded with --games_in" in text


@pytest.mark.parametrize("flags,words", [
    (["--games_every", "5"], ("--games_every", "needs --games_out")),
    (["--games_every", "0", "--games_out", "x"], ("--games_every", "at least 1")),
    (["--games_every", "-3", "--games_out", "x"], ("--games_every", "at least 1")),
    (["--games_in", "NOWHERE/games"], ("--games_in", "NOWHERE/games", "no such file"))])
def test_play_cli_exits_before_anything_is_imported(flags, words, monkeypatch, tmp_path):
    cli = _cli()
    import builtins
    real = builtins.__import__

    def no_package(name, *a, **k):
        assert not name.startswith("tetris_mcts_amd") and name not in ("pyTetris", "torch"), "imported before the refusal"
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_package)
    flags = [f.replace("NOWHERE", str(tmp_path)) for f in flags]
    with pytest.raises(SystemExit) as e:
        cli.main(["--agent_type", "ValueSim", "--n_games", "8"] + flags)
    for w in words:
        assert w.replace("NOWHERE", str(tmp_path)) in str(e.value.code), (w, e.value.code)


def _arrays(n=6, seed=3):
    rng = np.random.default_rng(seed)
    games = rng.integers(0, 2 ** 32, size=(n, 16), dtype=np.uint64).astype(np.uint32)
    return games, rng.integers(0, 1000, size=(n, 4)).astype(np.int32), rng.integers(0, 5000, size=n).astype(np.int32)


def test_file_round_trip_of_hand_made_arrays(tmp_path):
    from tetris_mcts_amd import games as G
    games, ls, move = _arrays()
    path = str(tmp_path / "sub" / "games")                    # no extension is added, the directory is made
    env = K.fake_env(6, app=2, scoring=1, randomizer=1)
    assert G.write_snapshot(path, G._meta(env), games, ls, move) == path
    assert sorted(os.listdir(tmp_path / "sub")) == ["games"], "the temporary file is gone"
    with np.load(path) as z:
        assert sorted(z.files) == ["games", "line_stats", "meta", "move"]
        assert z["meta"].dtype == np.int32 and z["meta"].tolist() == [G.VERSION, 6, 2, 1, 1]
    import zipfile
    assert all(i.compress_type == zipfile.ZIP_STORED for i in zipfile.ZipFile(path).infolist()), "uncompressed"
    g2, l2, m2 = G.read_snapshot(path, env)
    assert g2.dtype == np.uint32 and l2.dtype == np.int32 and m2.dtype == np.int32
    assert g2.tobytes() == games.tobytes() and l2.tobytes() == ls.tobytes() and m2.tobytes() == move.tobytes()
    # written over an existing file in one step
    G.write_snapshot(path, G._meta(env), games[::-1], ls, move)
    assert G.read_snapshot(path, env)[0].tobytes() == games[::-1].tobytes()


def test_load_games_refusals_that_need_no_device(tmp_path):
    from tetris_mcts_amd import games as G
    games, ls, move = _arrays()
    env = K.fake_env(6, app=2, scoring=1, randomizer=1)
    meta = G._meta(env)
    path = str(tmp_path / "games")

    def refused(words, meta=meta, games=games, ls=ls, move=move, env=env, raw=None):
        if raw is None:
            with open(path, "wb") as fh:
                np.savez(fh, meta=meta, games=games, line_stats=ls, move=move)
        else:
            open(path, "wb").write(raw)
        with pytest.raises(ValueError) as e:
            G.load_games(path, env)                      # (raises before it looks for a device)
        for w in (path,) + tuple(words):
            assert w in str(e.value), (w, str(e.value))

    bump = lambda i: np.concatenate([meta[:i], [meta[i] + 1], meta[i + 1:]]).astype(np.int32)  # noqa: E731
    refused(("version",), meta=bump(0))
    refused(("n_games", "6", "7"), meta=bump(1))
    refused(("n_games",), env=K.fake_env(5, 2, 1, 1))
    refused(("app",), env=K.fake_env(6, 1, 1, 1))
    refused(("scoring",), env=K.fake_env(6, 2, 0, 1))
    refused(("randomizer",), env=K.fake_env(6, 2, 1, 0))
    refused(("games", "shape"), games=games[:5])
    refused(("games", "shape"), games=games.reshape(6, 4, 4))
    refused(("line_stats", "shape"), ls=ls[:, :3])
    refused(("move", "shape"), move=move[:-1])
    refused(("games", "dtype"), games=games.astype(np.int64))
    refused(("games", "dtype"), games=games.view(np.int32))
    refused(("line_stats", "dtype"), ls=ls.astype(np.float32))
    refused(("move", "dtype"), move=move.astype(np.int64))
    refused(("meta",), meta=meta.astype(np.int64))
    refused(("meta",), meta=meta[:4])
    with open(path, "wb") as fh:
        np.savez(fh, meta=meta, games=games, line_stats=ls, move=move)
    whole = open(path, "rb").read()
    for cut in (len(whole) - 1, len(whole) // 2, 40, 0):
        refused(("not a game snapshot",), raw=whole[:cut])
    with open(path, "wb") as fh:
        np.savez(fh, meta=meta, games=games, move=move)
    with pytest.raises(ValueError, match="line_stats"):
        G.load_games(path, env)


# ENGINE_SPEC.md section 3, written out: cells as (column,row) inside the 4x4 box
SPEC_CELLS = """
I: r0 (0,1)(1,1)(2,1)(3,1)  r1 (2,0)(2,1)(2,2)(2,3)  r2 (0,2)(1,2)(2,2)(3,2)  r3 (1,0)(1,1)(1,2)(1,3)
O: r0 (1,0)(2,0)(1,1)(2,1)  r1 (1,0)(2,0)(1,1)(2,1)  r2 (1,0)(2,0)(1,1)(2,1)  r3 (1,0)(2,0)(1,1)(2,1)
T: r0 (1,0)(0,1)(1,1)(2,1)  r1 (1,0)(1,1)(2,1)(1,2)  r2 (0,1)(1,1)(2,1)(1,2)  r3 (1,0)(0,1)(1,1)(1,2)
S: r0 (1,0)(2,0)(0,1)(1,1)  r1 (1,0)(1,1)(2,1)(2,2)  r2 (1,1)(2,1)(0,2)(1,2)  r3 (0,0)(0,1)(1,1)(1,2)
Z: r0 (0,0)(1,0)(1,1)(2,1)  r1 (2,0)(1,1)(2,1)(1,2)  r2 (0,1)(1,1)(1,2)(2,2)  r3 (1,0)(0,1)(1,1)(0,2)
J: r0 (0,0)(0,1)(1,1)(2,1)  r1 (1,0)(2,0)(1,1)(1,2)  r2 (0,1)(1,1)(2,1)(2,2)  r3 (1,0)(1,1)(0,2)(1,2)
L: r0 (2,0)(0,1)(1,1)(2,1)  r1 (1,0)(1,1)(1,2)(2,2)  r2 (0,1)(1,1)(2,1)(0,2)  r3 (0,0)(1,0)(1,1)(1,2)
"""


def _spec_cells():
    out = []
    for line in SPEC_CELLS.strip().splitlines():
        rots = re.split(r"r\d", line.split(":", 1)[1])[1:]
        out.append([[tuple(map(int, c)) for c in re.findall(r"\((\d),(\d)\)", r)] for r in rots])
    assert len(out) == 7 and all(len(p) == 4 and all(len(r) == 4 for r in p) for p in out)
    return out


def test_collides_numpy_against_the_specs_cell_lists():
    from tetris_mcts_amd import games as G
    cells = _spec_cells()
    assert [[sorted(r) for r in p] for p in cells] == [[sorted(r) for r in p] for p in G.PIECE_CELLS]
    rng = np.random.default_rng(11)
    for trial in range(3):
        rows = (rng.integers(0, 1024, size=20) & rng.integers(0, 1024, size=20)).astype(np.uint16)
        rows[:6] = 0
        for piece in range(7):
            for rot in range(4):
                for x in range(-5, 12):
                    for y in range(-5, 22):
                        want = any(not (0 <= x + c <= 9 and 0 <= y + r <= 19) or (int(rows[min(max(y + r, 0), 19)]) >> (x + c)) & 1
                                   for c, r in cells[piece][rot])
                        assert G.collides_numpy(rows, piece, rot, x, y) == want, (piece, rot, x, y)
    # the engine's header builds its masks from the same lists: TM_CL(c0,r0, c1,r1, ...) in csrc/engine.h
    src = open(os.path.join(ROOT, "tetris_mcts_amd", "csrc", "engine.h")).read()
    table = src[src.index("PIECE_MASK_C[7][4]"):src.index("#undef TM_CL")]
    lists = [list(map(int, m.split(","))) for m in re.findall(r"TM_CL\(([^)]*)\)", table)]
    assert len(lists) == 28
    for i, l in enumerate(lists):
        assert sorted(zip(l[0::2], l[1::2])) == sorted(cells[i // 4][i % 4]), i


def test_check_games_numpy_one_game_per_fault_bit():
    from tetris_mcts_amd import games as G
    floor = np.zeros(20, np.uint16)
    floor[19], floor[18] = 0x3FE, 0x0F0
    live = K.make_game(rows=floor, piece=2, rot=0, x=4, y=7, combo=0, piece_count=9, score=140, lines=1)
    # a well-formed ended game: the spawned piece (rot 0 at (3, 0)) met the stack
    stack = np.zeros(20, np.uint16)
    stack[0:20] = 0x078
    ended = K.make_game(rows=stack, piece=0, rot=0, x=3, y=0, flags=1, piece_count=40)
    # a well-formed live game with a negative box origin: the vertical I (rot 1, column 2 of its box) at the left wall
    wall = K.make_game(rows=floor, piece=0, rot=1, x=-2, y=3)
    good = np.stack([live, ended, wall])
    ls = np.zeros((3, 4), np.int32)
    for app in (1, 2):
        assert G.check_games_numpy(good, ls, app).tolist() == [0, 0, 0]
        assert G.check_games_numpy(good, None, app).tolist() == [0, 0, 0]
    # the I one column further left is in the wall, a flag bit 1 (the back-to-back flag) is legal, so is drop_ctr 1 under app 2
    moved = wall.copy()
    K.set_piece(moved, x=-3)
    assert G.check_games_numpy(moved[None], None, 1).tolist() == [K.PLACE]
    b2b = live.copy()
    K.set_fields(b2b, flags=2, drop_ctr=1)
    assert G.check_games_numpy(b2b[None], None, 2).tolist() == [0] and G.check_games_numpy(b2b[None], None, 1).tolist() == [K.FIELDS]
    # one injection per class (and the combinations) into the live game: the named bits are among the faults
    games = np.stack([live] * len(K.INJECTIONS))
    lss = np.zeros((len(K.INJECTIONS), 4), np.int32)
    bad, bad_ls, where = K.inject(games, lss, list(range(len(K.INJECTIONS))))
    f = G.check_games_numpy(bad, bad_ls, 1)
    for g, (name, bits) in where.items():
        assert int(f[g]) & bits == bits, (name, int(f[g]), bits)
    singles = {name: int(f[g]) for g, (name, bits) in where.items()}
    assert singles["piece 7"] == K.PIECE and singles["rot 4"] == K.ROT and singles["a full row"] == K.ROWS
    assert singles["far below"] == K.PLACE and singles["combo -2"] == K.FIELDS
    assert singles["negative line statistic"] == K.LINE_STATS and singles["piece 255 and y 127"] == K.PIECE | K.PLACE
    assert singles["piece 200 inside the box range"] == K.PIECE, "no placement is evaluated without a piece"
    assert set(np.bitwise_or.reduce(f[None], axis=1).tolist()) == {63}, "every bit of the rule occurs"
    neg = [g for g, v in where.items() if v[0] == "negative line statistic"][0]
    assert G.check_games_numpy(bad, None, 1)[neg] == 0, "without line statistics there is nothing to find in them"
    for bits in f.tolist():
        assert G.describe_fault(bits)


def test_the_rule_admits_what_the_oracle_engine_produces_and_agrees_on_collisions():
    """random play of the oracle engine (ENGINE_SPEC.md in C): no state it produces has a fault, ended ones included; and a move
    to the side happens exactly where collides_numpy says the place is free"""
    from oracle import binding as B
    from tetris_mcts_amd import games as G
    rng = np.random.default_rng(5)
    checked = ended_seen = side_moves = 0
    for app in (1, 2):
        for randomizer in (0, 1):
            for seed in range(3):
                og = B.Game(app=app, scoring=0, randomizer=randomizer, seed=seed)
                for move in range(400):
                    packed = og.g.view(np.uint32).reshape(1, 16)
                    assert G.check_games_numpy(packed, og.line_stats[None], app).tolist() == [0], (app, randomizer, seed, move)
                    checked += 1
                    if og.end:
                        ended_seen += 1
                        og.reset()
                        continue
                    a = int(rng.integers(0, 7)) if move % 3 else 3
                    if a in (1, 2):
                        f = G.unpack_fields(packed)
                        x, y, piece, rot = (int(f[k][0]) for k in ("x", "y", "piece", "rot"))
                        nx = x + (-1 if a == 1 else 1)
                        free = not G.collides_numpy(f["rows"][0], piece, rot, nx, y)
                        count = int(f["piece_count"][0])
                        og.play(a)
                        if int(og.g["piece_count"][0]) == count:          # (gravity did not lock it)
                            assert int(og.g["x"][0]) == (nx if free else x), (app, seed, move)
                            side_moves += 1
                    else:
                        og.play(a)
    assert checked > 4000 and ended_seen >= 4 and side_moves > 200


def test_episode_stats_counts_continued_episodes(tmp_path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import episode_stats
    finally:
        sys.path.pop(0)
    from tetris_mcts_amd.episodes import EPISODE_DTYPE, STATE_DTYPE

    def table(first_moves):
        rows = np.zeros(3 * len(first_moves), STATE_DTYPE)
        for e, m0 in enumerate(first_moves):
            for k in range(3):
                r = rows[3 * e + k]
                r["episode"], r["cycle"], r["slot"], r["move"] = e, 2, e, m0 + k
        return rows

    stem = str(tmp_path / "data2")
    np.save(stem + ".part00000.npy", table([0, 0, 0]))
    np.save(stem + ".episodes.part00000.npy", np.zeros(0, EPISODE_DTYPE))
    assert "continued" not in episode_stats.stats([stem])
    np.save(stem + ".part00000.npy", table([40, 0, 12]))
    ep = np.zeros(1, EPISODE_DTYPE)
    ep["episode"], ep["cycle"], ep["slot"], ep["moves"] = 2, 2, 2, 15
    np.save(stem + ".episodes.part00000.npy", ep)
    out = episode_stats.stats([stem])
    assert out["continued"]["count"] == 2 and out["continued"]["finished"] == 1 and "complete" in out["continued"]["note"]


def test_new_kernels_use_no_scratch_memory(tmp_path):
    """no private segment and no spilled registers in any kernel of games_snapshot.hip, read from the code object in the built
    HIP object"""
    import shutil
    import subprocess
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("no llvm binutils")
    obj = os.path.join(ROOT, "tetris_mcts_amd", "csrc", "_obj", "games_snapshot.o")
    if not os.path.exists(obj):
        pytest.skip("HIP objects not built")
    local = str(tmp_path / "games_snapshot.o")
    shutil.copy(obj, local)
    subprocess.check_call([objdump, "--offloading", local], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    cos = [f for f in os.listdir(tmp_path) if f.startswith("games_snapshot.o.") and "amdgcn" in f]
    assert cos, "no device code object in " + obj
    notes = subprocess.check_output([readelf, "--notes", str(tmp_path / cos[0])]).decode()
    want = {"k_env_check", "k_env_count", "k_env_copy", "k_episode_resume"}
    seen = set()
    for name, scratch, spills in re.findall(r"\.name:\s+(\S+)\s.*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", notes, re.S):
        for w in want:
            if w in name:
                seen.add(w)
                assert int(scratch) == 0 and int(spills) == 0, (name, scratch, spills)
    assert seen == want, want - seen
    assert "gfx950" in notes


def test_the_recorder_resumes_through_a_method_before_the_first_row():
    """the constructor keeps its parameters; resume(move_idx) refuses, before it touches a device, a recorder that has rows, a
    closed one and an array of another length"""
    import inspect
    from tetris_mcts_amd.episodes import EpisodeRecorder
    assert list(inspect.signature(EpisodeRecorder.resume).parameters) == ["self", "move_idx"]
    assert "move_idx" not in inspect.signature(EpisodeRecorder.__init__).parameters
    for pos, flushes, closed in ((1, 0, False), (0, 1, False), (0, 0, True)):
        rec = EpisodeRecorder.__new__(EpisodeRecorder)
        rec._pos, rec._flushes, rec.closed, rec.G = pos, flushes, closed, 4
        with pytest.raises(RuntimeError, match="before the first add"):
            rec.resume(np.zeros(4, np.int32))
    rec = EpisodeRecorder.__new__(EpisodeRecorder)
    rec._pos, rec._flushes, rec.closed, rec.G = 0, 0, False, 4
    with pytest.raises(ValueError, match="3 entries for 4 games"):
        rec.resume(np.zeros(3, np.int32))
