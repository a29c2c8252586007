"""Self-play records written on the device (csrc/episodes.hip, tetris_mcts_amd/episodes.py) against a recorder in Python that
does what the reference's DataSaver.add does - the public getters, every move - and numbers the episodes by the rule of the
header: the first G episodes are the slots, later ids go by move, then by slot.

Episodes are made to end by forcing the odd slots (the only slot of a one-game batch) to action 3, the hard drop, through
add(..., action=...): a game fed only hard drops ends after 10 or 11 moves, so 24 moves finish two episodes in every such slot.
get_value_and_variance() works for every kind today (TM_KIND_DIST keeps node_rec[.., 29] = the node itself), so ValueSimLP and
DistValueSim are compared like the others."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from gpu_helpers import hash_eval_torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIMS, MAX_NODES, MOVES, RING = 12, 8000, 24, 5
CYCLE = 3


def _uniform_dist(boards):
    return np.full((len(boards), 50), 1.0 / 50, np.float32)


def _make(name, G, seed):
    from test_gpu_tree import _make as make
    kw = {"DistValueSim": dict(evaluator=_uniform_dist), "Vanilla": dict(random_seed=11)}.get(name, dict(evaluator=hash_eval_torch))
    return make(name, G, SIMS, MAX_NODES, seed, **kw)


class Checker:
    """DataSaver.add through the getters, for a batch, with the numbering rule"""

    def __init__(self, G, cycle):
        from tetris_mcts_amd.episodes import STATE_DTYPE
        self.G, self.cycle, self.dtype = G, cycle, STATE_DTYPE
        self.ids, self.move, self.live, self.next_id = list(range(G)), [0] * G, [False] * G, G
        self.rows, self.done = [], []

    def add(self, agent, game, action):
        G = self.G
        end = np.atleast_1d(game.end)
        board = game.getState().reshape(G, 20, 10)
        with np.errstate(all="ignore"):
            prob = agent.get_prob().reshape(G, 7)
        stats = agent.get_stats().reshape(G, 3, 7)
        v, var = (np.atleast_1d(x) for x in agent.get_value_and_variance())
        combo, lines, score = (np.atleast_1d(x) for x in (game.combo, game.line_clears, game.score))
        ls = np.asarray(game.line_stats).reshape(G, 4)
        for g in range(G):
            if end[g]:
                continue
            r = np.zeros((), self.dtype)
            r["episode"], r["cycle"], r["slot"], r["move"] = self.ids[g], self.cycle, g, self.move[g]
            r["combo"], r["lines"], r["score"], r["line_stats"] = combo[g], lines[g], score[g], ls[g]
            r["value"], r["variance"], r["child_stats"], r["policy"] = v[g], var[g], stats[g], prob[g]
            r["board"], r["action"] = board[g], action[g]
            self.rows.append(r)
            self.live[g] = True

    def advance(self, game):
        end, score, lines = (np.atleast_1d(x) for x in (game.end, game.score, game.line_clears))
        ls = np.asarray(game.line_stats).reshape(self.G, 4)
        for g in range(self.G):
            if self.live[g] and end[g]:
                self.done.append((self.ids[g], self.cycle, g, self.move[g] + 1, int(score[g]), int(lines[g]), ls[g].tolist()))
                self.ids[g], self.move[g] = self.next_id, 0
                self.next_id += 1
            elif self.live[g]:
                self.move[g] += 1
            self.live[g] = False


def _forced(G):
    return [0] if G == 1 else list(range(1, G, 2))


_runs = {}


def _run(name, G, record, tmp_root):
    """24 moves of `name` with the forced hard drops; with `record` a recorder (ring of 5 moves) beside the checker"""
    key = (name, G, record)
    if key in _runs:
        return _runs[key]
    from tetris_mcts_amd.episodes import EpisodeRecorder
    game, agent = _make(name, G, 0)                  # (seeds 0 .. G-1: hard drops alone end those games after 10 or 11 moves)
    out = dict(dir=os.path.join(str(tmp_root), "%s_%d/" % (name, G)), trace=[], chk=Checker(G, CYCLE), printed=[])
    rec = EpisodeRecorder(out["dir"], "data", CYCLE, G, ring_moves=RING) if record else None
    for m in range(MOVES):
        act = np.atleast_1d(agent.play()).astype(np.int32).copy()
        out["trace"].append((act.copy(), agent.get_stats().tobytes()))
        act[_forced(G)] = 3
        played = act if G > 1 else int(act[0])
        if rec is not None:
            rec.add(agent, game, action=played)
            out["chk"].add(agent, game, act)
        game.play(played)
        if rec is not None:
            rec.advance(game)
            out["chk"].advance(game)
        agent.update_root(game)
        ended = np.atleast_1d(game.end)
        if ended.any():
            out["printed"] += [(m, int(g)) for g in np.nonzero(ended)[0]]        # play.py's Episode: lines, in their order
            game.reset("ended")
            agent.update_root(game)
    if rec is not None:
        rec.close()
        out["files"] = rec.files
    torch.cuda.synchronize()
    assert not bool(agent.store.errors().any().item())
    _runs[key] = out
    return out


@pytest.fixture(scope="module")
def tmp_root(tmp_path_factory):
    return tmp_path_factory.mktemp("episodes")


def _same_bits(a, b):
    """equal bit for bit; a NaN compares as a NaN (only its sign may differ)"""
    if a.dtype.kind == "f":
        ua, ub = a.view("<u4"), b.view("<u4")
        return bool(((ua == ub) | (np.isnan(a) & np.isnan(b))).all())
    return bool(np.array_equal(a, b))


def _want_rows(chk):
    w = np.zeros(len(chk.rows), chk.dtype)
    for i, r in enumerate(chk.rows):
        w[i] = r
    return w


CASES = [("ValueSim", 12), ("Vanilla", 12), ("ValueSim", 1), ("ValueSimLP", 12), ("DistValueSim", 12)]


@pytest.mark.parametrize("name,G", CASES)
def test_rows_equal_the_getters_bit_for_bit(name, G, tmp_root):
    """every column of the loaded State rows (file order: move-major, slot-minor) against the checker's, the pad bytes zero,
    five parts from a ring of five moves over 24, ids 0, 1, 2 with one game"""
    from tetris_mcts_amd.episodes import EpisodeLoader, STATE_DTYPE
    run = _run(name, G, True, tmp_root)
    assert len(run["files"]) == 5 == -(-MOVES // RING)
    assert [os.path.basename(f[0]) for f in run["files"]] == ["data%d.part%05d.npy" % (CYCLE, i) for i in range(5)]
    got = EpisodeLoader(run["dir"] + "data%d" % CYCLE, by_episode=False)
    want = _want_rows(run["chk"])
    assert got.length == len(want) > 0
    for c in STATE_DTYPE.names:
        a, b = getattr(got, c), want[c]
        print(name, G, c, "rows that differ:", int((a.reshape(len(a), -1) != b.reshape(len(b), -1)).any(axis=1).sum()))
        assert _same_bits(a, b), c
    for f, _ in run["files"]:
        raw = np.load(f)
        assert raw.dtype == STATE_DTYPE
        assert not np.ascontiguousarray(raw).view(np.uint8).reshape(len(raw), 368)[:, 365:].any(), "pad bytes"
        assert (raw["episode"] >= 0).all()
    assert len(want) == G * MOVES, "no slot was left ended: every slot has a row every move"
    assert len(run["chk"].done) >= 2 * len(_forced(G)), "every forced slot finished two episodes"
    if G == 1:
        assert sorted(set(got.episode.tolist())) == [0, 1, 2]
        assert (np.diff(got.episode) >= 0).all()


@pytest.mark.parametrize("name,G", CASES[:3])
def test_episode_table(name, G, tmp_root):
    """the table equals the checker's (episode, slot, moves, score, lines, line_stats) in the order play.py prints; moves = the
    State rows of the episode; the final score = the last row's score + that action's points (the game's own score after it)"""
    from tetris_mcts_amd.episodes import EpisodeLoader, EPISODE_DTYPE
    run = _run(name, G, True, tmp_root)
    d = EpisodeLoader(run["dir"] + "data%d" % CYCLE)
    ep, want = d.episodes, run["chk"].done
    assert ep.dtype == EPISODE_DTYPE and len(ep) == len(want) == len(run["printed"])
    for r, w in zip(ep, want):
        assert (int(r["episode"]), int(r["cycle"]), int(r["slot"]), int(r["moves"]), int(r["score"]), int(r["lines"]),
                r["line_stats"].tolist()) == w
    assert [int(s) for s in ep["slot"]] == [g for _, g in run["printed"]]
    if G == 1:
        assert ep["episode"].tolist() == list(range(len(ep))) and len(ep) >= 2        # the reference's ngames counter
    for r in ep:
        mine = d.episode == r["episode"]
        assert int(mine.sum()) == int(r["moves"]) and d.move[mine].tolist() == list(range(int(r["moves"])))
        assert (d.slot[mine] == r["slot"]).all()
        last = np.nonzero(mine)[0][-1]
        # the ending action's points (the table's score is the game's own after it, compared above): under the guideline scoring
        # a drop earns 1 or 2 points a row and a clear a multiple of 50 - never a loss
        assert int(r["score"]) >= int(d.score[last]) and int(r["lines"]) >= int(d.lines[last])
        if int(r["slot"]) in _forced(G):
            assert int(d.action[last]) == 3 and (int(r["score"]) - int(d.score[last])) % 2 == 0


def test_recording_perturbs_nothing(tmp_root):
    """the actions and the 84 statistics bytes of every move with a recorder equal those of the same run without one"""
    a, b = _run("ValueSim", 12, True, tmp_root), _run("ValueSim", 12, False, tmp_root)
    assert len(a["trace"]) == len(b["trace"]) == MOVES
    for m, ((act_a, st_a), (act_b, st_b)) in enumerate(zip(a["trace"], b["trace"])):
        assert np.array_equal(act_a, act_b) and st_a == st_b, m
    assert a["printed"] == b["printed"]


def _drops(G, slots):
    a = np.zeros(G, np.int32)
    a[list(slots)] = 3
    return a


def test_a_slot_left_ended(tmp_root):
    """slot 1 is not reset for three moves after its first end: no State rows for those moves, exactly one episode row, and its
    rows resume under the id it was given.  (No search runs on the ended root: the agent played once, the statistics stay.)"""
    from tetris_mcts_amd.episodes import EpisodeLoader, EpisodeRecorder
    G = 4
    game, agent = _make("Vanilla", G, 0)
    agent.play()
    chk, d = Checker(G, CYCLE), os.path.join(str(tmp_root), "left_ended/")
    rec = EpisodeRecorder(d, "data", CYCLE, G, ring_moves=RING)
    acts, first_end, given = _drops(G, (1, 3)), None, None
    for m in range(20):
        rec.add(agent, game, action=acts)
        chk.add(agent, game, acts)
        game.play(acts)
        rec.advance(game)
        chk.advance(game)
        end = np.atleast_1d(game.end).copy()
        if end[1] and first_end is None:
            first_end, given = m, chk.ids[1]
        if first_end is not None and m < first_end + 3:
            end[1] = False                            # slot 1 stays ended for the moves first_end + 1 .. first_end + 3
        if end.any():
            game.reset(end)
    rec.close()
    assert first_end is not None and first_end + 4 < 20
    ld = EpisodeLoader(d + "data%d" % CYCLE, by_episode=False)
    want = _want_rows(chk)
    assert ld.length == len(want) == G * 20 - 3
    for c in ld.rows.dtype.names:
        assert _same_bits(getattr(ld, c), want[c]), c
    s1 = ld.rows[ld.slot == 1]
    assert s1["episode"][:first_end + 1].tolist() == [1] * (first_end + 1) and s1["move"][:first_end + 1].tolist() == list(range(first_end + 1))
    resumed = s1[first_end + 1:]
    assert resumed["episode"][0] == given and resumed["move"][0] == 0
    assert [tuple(int(x) for x in (r["episode"], r["slot"], r["moves"])) for r in ld.episodes] == [w[:1] + w[2:4] for w in chk.done]
    assert int((ld.episodes["episode"] == 1).sum()) == 1
    upto = [w for w in chk.done if w[2] == 1]
    assert upto[0][0] == 1 and (len(upto) == 1 or upto[1][0] == given)


GUARD, FILL = 4096, 0x5A


class Arena:
    """the four arrays the calls write, carved out of one device tensor with guard bands before, between and after them"""

    def __init__(self, sizes):
        off, self.seg = GUARD, []
        for n in sizes:
            self.seg.append((off, n))
            off = (off + n + 15) // 16 * 16 + GUARD
        self.t = torch.full((off,), FILL, dtype=torch.uint8, device="cuda")

    def ptr(self, i):
        return C.c_void_p(self.t.data_ptr() + self.seg[i][0])

    def bytes(self, i):
        o, n = self.seg[i]
        return self.t[o:o + n].cpu().numpy()

    def check(self):
        torch.cuda.synchronize()
        outside = torch.ones(self.t.numel(), dtype=torch.bool, device="cuda")
        for o, n in self.seg:
            outside[o:o + n] = False
        assert int(outside.sum()) >= GUARD * (len(self.seg) + 1)
        bad = torch.nonzero(outside & (self.t != FILL)).flatten()
        assert bad.numel() == 0, ("stores outside the arrays at byte offsets", bad[:8].tolist(), self.seg)


def _raw_drive(G, seeds, dropped, cap, moves=13):
    """the three calls themselves into guarded arrays: `moves` moves, the slots `dropped` hard-dropping, nothing reset"""
    from tetris_mcts_amd.episodes import EPISODE_DTYPE, STATE_DTYPE
    game, agent = _make("Vanilla", G, 5)
    game.seed(np.asarray(seeds))
    agent.update_root(game)
    agent.play()
    L, s = agent.store.L, agent.store
    arena = Arena([G * 368, cap * 40, G * 16, 8])
    rows, done, slots, cnt = (arena.ptr(i) for i in range(4))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    acts_host = _drops(G, dropped)
    acts = torch.from_numpy(acts_host).cuda()
    assert L.tm_episode_init(G, 0, slots, cnt, stream) == 0
    arena.check()
    assert arena.bytes(2).view(np.int32).reshape(G, 4).tolist() == [[g, 0, 0, 0] for g in range(G)]
    assert arena.bytes(3).view(np.int32).tolist() == [G, 0]
    finished, seen = [], []                    # (move, slot, score, lines) in the order of the numbering
    for m in range(moves):
        was_ended = np.atleast_1d(game.end).copy()
        assert L.tm_episode_record(C.byref(game.s), C.byref(s.s), C.c_void_p(s.stats_buf.data_ptr()), C.c_void_p(acts.data_ptr()),
                                   CYCLE, slots, rows, stream) == 0
        arena.check()
        r = arena.bytes(0).view(STATE_DTYPE)
        # (nothing is reset: a slot records its first episode, g, until it ends, and -1 and zeros from then on)
        assert r["episode"].tolist() == [-1 if was_ended[g] else g for g in range(G)]
        for g in range(G):
            if was_ended[g]:
                assert not r[g:g + 1].view(np.uint8)[4:].any(), "an ended slot's row is -1 and zeros"
            else:
                assert (int(r["slot"][g]), int(r["move"][g]), int(r["cycle"][g]), int(r["action"][g])) == (g, m, CYCLE, int(acts_host[g]))
        game.play(acts)
        assert L.tm_episode_advance(C.byref(game.s), CYCLE, slots, cnt, done, cap, stream) == 0
        arena.check()
        end, score, lines = (np.atleast_1d(x) for x in (game.end, game.score, game.line_clears))
        now = [int(g) for g in range(G) if end[g] and not was_ended[g]]
        finished += [(m, g, int(score[g]), int(lines[g])) for g in now]
        seen.append(len(now))
        assert arena.bytes(3).view(np.int32).tolist() == [G + len(finished), len(finished)]
        assert not arena.bytes(2).view(np.int32).reshape(G, 4)[:, 2].any(), "live is cleared"
    d = arena.bytes(1).view(EPISODE_DTYPE)
    n = min(cap, len(finished))
    assert [(int(x["slot"]), int(x["moves"]), int(x["score"]), int(x["lines"])) for x in d[:n]] == \
        [(g, m + 1, sc, li) for m, g, sc, li in finished[:n]]
    assert d["episode"][:n].tolist() == [g for _, g, _, _ in finished[:n]] and (d["cycle"][:n] == CYCLE).all()
    ids = arena.bytes(2).view(np.int32).reshape(G, 4)[:, 0].tolist()
    assert ids == [G + [f[1] for f in finished].index(g) if g in [f[1] for f in finished] else g for g in range(G)]
    return finished, seen, arena.bytes(1)


@pytest.mark.parametrize("G", [1, 5, 12])
def test_nothing_else_is_written(G):
    """guard bytes around the rows, the done buffer, the slot state and the counters stay intact through init, record and advance"""
    dropped = [0] if G == 1 else list(range(1, G, 2))
    finished, _, _ = _raw_drive(G, np.arange(G), dropped, cap=G)
    assert sorted(g for _, g, _, _ in finished) == dropped, "every hard-dropping slot ended once"


def test_a_full_done_buffer_is_counted_not_written():
    """cap = 2 while three slots (the same seed, the same hard drops) finish in one move: two rows are written, n_done is 3 (checked
    inside the drive), the bytes behind the two rows are the guard's"""
    finished, seen, done_bytes = _raw_drive(5, [5, 100, 5, 101, 5], (0, 2, 4), cap=2)
    assert 3 in seen and len(finished) == 3 and [g for _, g, _, _ in finished] == [0, 2, 4]
    assert len(done_bytes) == 80


def test_recording_enqueues_only(tmp_root):
    """add, advance and a flush under torch's sync debug mode: a call that makes the host wait for the device raises.  (The calls
    of the library are launches by construction; the recorder's own wait is Event.synchronize() in _drain, on a flush two rings
    old - it is counted here and must not happen before the third flush.)"""
    from tetris_mcts_amd.episodes import EpisodeRecorder
    G = 4
    game, agent = _make("Vanilla", G, 0)
    agent.play()
    rec = EpisodeRecorder(os.path.join(str(tmp_root), "nosync/"), "data", CYCLE, G, ring_moves=2)
    acts = torch.from_numpy(_drops(G, (1,))).cuda()
    waits, sync = [], torch.cuda.Event.synchronize

    def counted(ev):
        waits.append(rec._flushes)
        return sync(ev)
    torch.cuda.synchronize()
    torch.cuda.Event.synchronize = counted
    torch.cuda.set_sync_debug_mode("error")
    try:
        for m in range(6):                     # three flushes
            rec.add(agent, game, action=acts)
            game.play(acts)
            rec.advance(game)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        torch.cuda.Event.synchronize = sync
    assert rec._flushes == 3 and waits == [2], waits
    rec.close()
    assert len(rec.files) == 3


def test_command_line(tmp_path):
    """play.py --save in a fresh process: parts exist, every row carries the cycle, the episode table has as many rows as the
    process counted finished games"""
    from tetris_mcts_amd.episodes import EpisodeLoader
    d = str(tmp_path) + "/"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "play.py"), "--agent_type", "Vanilla", "--mcts_sims", "8", "--n_games", "4",
                        "--ngames", "3", "--save", "--save_dir", d, "--cycle", "7"], capture_output=True, text=True, timeout=600,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    played = int(re.findall(r"Games played:\s*(\d+)", r.stdout)[-1])
    assert played >= 3
    assert os.path.exists(d + "data7.part00000.npy") and os.path.exists(d + "data7.episodes.part00000.npy")
    ld = EpisodeLoader(d + "data7")
    assert ld.length > 0 and (ld.cycle == 7).all()
    assert len(ld.episodes) == played and (ld.episodes["cycle"] == 7).all()
    for e in ld.episodes:
        assert int((ld.episode == e["episode"]).sum()) == int(e["moves"])
