"""Reanalysis: the recorded moves of `play.py --save --save_positions` searched again under the current weights, written as State
shards of the recorded format (reanalyse.py).

A State row holds the rendered board, which cannot be searched; its position row (episodes.POSITION_DTYPE) holds the packed game.
A batch of positions is loaded into a `Tetris` environment through the all-or-nothing device check of game snapshots
(tm_env_load), every tree is put into the state of a newly built store (TreeStore.pool_fresh), the agent searches its ordinary
`sims` simulations from the new roots, and tm_episode_rerecord (csrc/episodes.hip) writes the rows again: identity and the action
PLAYED from the old row, the game's columns recomputed and compared with the old row's bit for bit (the guard against a mis-paired
or edited position file), value, variance, child_stats and policy from the new search.

THE CONTRACT: a re-analysed row is a function of its position, the agent kind, the simulations, max_nodes, the backend and the
weights - not of the slot, the batch, the batch size or the order of the input: every game's tree, counters and rand() stream
start as a new store's, and the hip value nets are a function of the state alone.

DistValueSim (an agent whose store is KIND_DIST; reanalyse.py --agent_type DistValueSim --root_dists): the root-distribution rows
recorded beside the State rows (episodes.ROOT_DIST_DTYPE, play.py --save_root_dists) are made again too - tm_episode_record_root_dists
on the rows tm_episode_rerecord has just written - and the contract is claimed for all 368 + 272 bytes: the HIP head is a function
of the state alone, and a dist tree that starts empty grows by the same seven nodes a simulation.

`rerecord_numpy` is the numpy statement of tm_episode_rerecord's definitions: what the kernel is held to.
"""
import ctypes as C
import glob
import os
import shutil

import numpy as np

from .episodes import (_PART, IDENTITY, POSITION_DTYPE, ROOT_DIST_BYTES, ROOT_DIST_DTYPE, ROW_BYTES, STATE_DTYPE, PositionLoader,
                       RootDistLoader, _expand, _parts, rootdist_file, write_root_dist_head)
from .games import PIECE_CELLS, describe_fault, unpack_fields

AGENTS = ("ValueSim", "ValueSimLP", "ValueSimC", "DistValueSim")
GROUPS = ("combo, lines or score", "line_stats", "board", "the game of the position has ended")     # TM_REREC_*
NO_FAULT = 0x7FFFFFFF


def default_max_nodes(sims):
    """The pool of a re-analysis: a tree that starts empty holds the null node, the root and its seven children, and grows by at
    most seven nodes (the successors of the one leaf it expands) a simulation: 7 (sims + 1) + 2 nodes and no more observations.
    1024 on top keep the free count above the store's speculative-marking threshold (at most 256), so no collection ever starts."""
    return 8 * int(sims) + 1024


def choose_inputs(paths, last_nfiles=0):
    """the State shards of `paths` (glob patterns, stems or shards; position and episode shards a pattern matches are left out) in
    the order (stem, part); last_nfiles > 0: of the stems written last only, as train.py --last_nfiles counts them"""
    if isinstance(paths, (str, os.PathLike)):
        paths = [paths]
    found = []
    for p in map(str, paths):
        found += sorted(glob.glob(p)) or [p]
    found = [f for f in found if not os.path.basename(f).startswith(("positions", "rootdist"))]
    files = _expand(found)
    stems = list(dict.fromkeys(_PART.sub("", f) for f in files))
    if last_nfiles and last_nfiles > 0:
        stems.sort(key=lambda s: (max(os.path.getmtime(f) for f in _parts(s)), s))
        keep = set(stems[-last_nfiles:])
        files = [f for f in files if _PART.sub("", f) in keep]
    return files


def render_boards_numpy(games):
    """int8 [n,20,10] of packed games [n,16], the engine's rendering: 0 empty, 1 locked, -1 the falling piece (none once ended)"""
    f = unpack_fields(games)
    n = len(f["piece"])
    board = ((f["rows"][:, :, None] >> np.arange(10)[None, None, :]) & 1).astype(np.int8)
    for g in range(n):
        if f["flags"][g] & 1:
            continue
        for c, r in PIECE_CELLS[int(f["piece"][g])][int(f["rot"][g])]:
            board[g, int(f["y"][g]) + r, int(f["x"][g]) + c] = -1
    return board


def rerecord_numpy(old_rows, positions, stats, value, variance):
    """tm_episode_rerecord as a numpy statement: (rows, fault).  old_rows: STATE_DTYPE [n]; positions: POSITION_DTYPE [n], the
    games loaded (row i with row i); stats: float32 [n,3,7], the root statistics of the new search; value, variance: float32 [n],
    the new roots' observation statistics.  rows: episode, cycle, slot, move, action and the pad bytes from old_rows; combo, lines,
    score, line_stats, board recomputed from the games; value, variance, child_stats from the arguments and policy = visits over
    their float32 sum added in index order.  fault: None, or (first bad row, its first differing column group as an index into
    GROUPS, number of bad rows) where a recomputed column is not the old row's or the game has ended."""
    n = len(old_rows)
    old = np.ascontiguousarray(old_rows)
    # the copied columns and the pad bytes (whole rows as bytes: a copy of a padded dtype does not carry the padding)
    new = old.view(np.uint8).reshape(n, ROW_BYTES).copy().view(STATE_DTYPE).reshape(-1)
    games = np.ascontiguousarray(positions["game"], dtype=np.uint32).reshape(n, 16)
    f = unpack_fields(games)
    new["combo"], new["lines"], new["score"] = f["combo"], f["lines"], f["score"]
    new["line_stats"] = positions["line_stats"]
    new["board"] = render_boards_numpy(games)
    st = np.ascontiguousarray(stats, dtype=np.float32).reshape(n, 3, 7)
    new["child_stats"] = st
    total = st[:, 0, 0].copy()
    for a in range(1, 7):
        total = (total + st[:, 0, a]).astype(np.float32)
    with np.errstate(all="ignore"):
        new["policy"] = (st[:, 0, :] / total[:, None]).astype(np.float32)
    new["value"], new["variance"] = np.asarray(value, np.float32), np.asarray(variance, np.float32)
    group = np.full(n, 4, np.int64)
    checks = ((3, (f["flags"] & 1) != 0),
              (2, (new["board"] != old["board"]).reshape(n, -1).any(axis=1)),
              (1, (new["line_stats"] != old["line_stats"]).any(axis=1)),
              (0, (new["combo"] != old["combo"]) | (new["lines"] != old["lines"]) | (new["score"] != old["score"])))
    for k, bad in checks:                                      # (descending: the lowest group that differs stays)
        group[bad] = k
    bad = np.nonzero(group < 4)[0]
    fault = (int(bad[0]), int(group[bad[0]]), int(len(bad))) if len(bad) else None
    return new, fault


def _p(t, offset=0):
    return C.c_void_p(t.data_ptr() + offset)


class Reanalyser:
    """The device half for one agent and one environment of the same n_games: submit(rows, positions) loads, searches and
    re-records a batch of at most n_games rows and enqueues the copy of the new rows and of the guard's words to a pinned buffer;
    collect() waits for that copy and returns the rows (ValueError if the guard fired).  An agent whose store is KIND_DIST
    (`.dist`): the root-distribution rows are written after the State rows and copied before the same event, and collect()
    returns (rows, dists).  One batch at a time: the load report and
    the search itself (tm_search_run reads its catch-up counts back) synchronise with the host anyway, so there is nothing a
    second buffer could overlap but the 368 bytes a row of the copy."""

    def __init__(self, agent, game):
        import torch
        from . import _lib
        if agent.store is None:
            agent._build(game.n_games)
        if agent.store.n_games != game.n_games:
            raise ValueError("the agent holds %d games, the environment %d" % (agent.store.n_games, game.n_games))
        if agent.search_model() is False:
            raise ValueError("re-analysis runs the native launch loop of the hip back ends (hip, hip_bf16x3): a row is then a "
                             "function of its position; the torch back end and callables are not offered")
        self.torch, self.L, self._check = torch, _lib.lib(), _lib.check
        self.agent, self.game, self.G = agent, game, game.n_games
        G, dev = self.G, game.device
        self.d_games = torch.zeros(G, 16, dtype=torch.int32, device=dev)
        self.d_ls = torch.zeros(G, 4, dtype=torch.int32, device=dev)
        self.d_old = torch.zeros(G * ROW_BYTES, dtype=torch.uint8, device=dev)
        self.d_new = torch.zeros(G * ROW_BYTES, dtype=torch.uint8, device=dev)
        self.report = torch.zeros(G + 1, dtype=torch.int32, device=dev)        # tm_env_load: fault [G], then n_bad
        self.fault = torch.zeros(2, dtype=torch.int32, device=dev)
        self._fault0 = torch.tensor([NO_FAULT, 0], dtype=torch.int32, device=dev)
        self._host = torch.zeros(G * ROW_BYTES + 8, dtype=torch.uint8).pin_memory()
        from .store import KIND_DIST
        self.dist = agent.store.s.kind == KIND_DIST
        if self.dist:
            self.d_new_dists = torch.zeros(G * ROOT_DIST_BYTES, dtype=torch.uint8, device=dev)
            self._host_dists = torch.zeros(G * ROOT_DIST_BYTES, dtype=torch.uint8).pin_memory()
        self._pending = None               # (event, n, what) of the batch submitted and not yet collected
        # the games of the slots a short batch does not use: new ones, kept from the environment's first reset
        game.reset()
        self._fresh = game.games.clone()
        self.timing = None                 # a dict of lists of torch events when a caller asks for the stages' times

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def _mark(self, name):
        if self.timing is not None:
            e = self.torch.cuda.Event(enable_timing=True)
            e.record()
            self.timing.setdefault(name, []).append(e)

    def submit(self, rows, positions, what="batch"):
        torch, G, n = self.torch, self.G, len(rows)
        if not 0 < n <= G or len(positions) != n:
            raise ValueError("a batch is 1 .. %d rows with as many positions, not %d and %d" % (G, n, len(positions)))
        if self._pending is not None:
            raise RuntimeError("a batch is held: collect() it first")
        for c in IDENTITY:
            bad = np.nonzero(rows[c] != positions[c])[0]
            if len(bad):
                raise ValueError("%s: row %d and its position differ in %s (%d and %d)" % (what, int(bad[0]), c, int(rows[c][bad[0]]),
                                                                                         int(positions[c][bad[0]])))
        self._mark("start")
        # 1. the batch's 80 bytes a position, the unused slots new empty games
        games = np.ascontiguousarray(positions["game"], dtype=np.uint32).reshape(n, 16)
        self.d_games[:n].copy_(torch.from_numpy(games.view(np.int32)), non_blocking=False)
        self.d_ls[:n].copy_(torch.from_numpy(np.ascontiguousarray(positions["line_stats"], dtype=np.int32).reshape(n, 4)))
        if n < G:
            self.d_games[n:].copy_(self._fresh[n:])
            self.d_ls[n:].zero_()
        old = np.ascontiguousarray(rows).view(np.uint8).reshape(-1)
        self.d_old[:n * ROW_BYTES].copy_(torch.from_numpy(old))
        # 2. into the environment, all or nothing
        game, agent = self.game, self.agent
        self._check(self.L.tm_env_load(C.byref(game.s), _p(self.d_games), _p(self.d_ls), _p(self.report),
                                       _p(self.report, 4 * G), self._stream()), "tm_env_load")
        host = self.report.cpu().numpy()
        if int(host[-1]):
            first = int(np.nonzero(host[:-1])[0][0])
            raise ValueError("%s: %d of %d positions are not well-formed games, nothing was loaded and nothing is written; the first "
                             "is row %d with fault bits %d (%s)" % (what, int(host[-1]), n, first, int(host[first]),
                                                                    describe_fault(host[first])))
        game._host = None
        self._mark("loaded")
        # 3. every tree as a new store's, new roots, the agent's ordinary search
        agent._pending_pool_reset = None
        agent.store.pool_fresh()
        self._mark("fresh")
        agent.update_root(game)
        agent.mcts(agent.sims)
        stats, _ = agent.compute_stats()
        self._mark("searched")
        err = agent.store.errors()
        if bool((err != 0).any().item()):
            raise RuntimeError("%s: tree engine error flags %s (a pool too small for %d simulations from an empty tree: raise "
                               "--max_nodes)" % (what, sorted(set(err.cpu().numpy().tolist())), agent.sims))
        # 4. the rows again, and on their way to the host
        self.fault.copy_(self._fault0)
        self._check(self.L.tm_episode_rerecord(C.byref(game.s), C.byref(agent.store.s), _p(stats), _p(self.d_old), n,
                                               _p(self.d_new), _p(self.fault), self._stream()), "tm_episode_rerecord")
        if self.dist:
            self._check(self.L.tm_episode_record_root_dists(C.byref(agent.store.s), _p(self.d_new), n, _p(self.d_new_dists),
                                                            self._stream()), "tm_episode_record_root_dists")
            self._host_dists[:n * ROOT_DIST_BYTES].copy_(self.d_new_dists[:n * ROOT_DIST_BYTES], non_blocking=True)
        buf = self._host
        buf[:n * ROW_BYTES].copy_(self.d_new[:n * ROW_BYTES], non_blocking=True)
        buf[G * ROW_BYTES:].copy_(self.fault.view(torch.uint8), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._mark("rerecorded")
        self._pending = (ev, n, what)

    def collect(self):
        (ev, n, what), self._pending = self._pending, None
        ev.synchronize()
        buf = self._host.numpy()
        first, count = (int(v) for v in buf[self.G * ROW_BYTES:].view(np.int32))
        if count:
            raise ValueError("%s: %d of %d rows do not belong to their positions, nothing is written for it; the first is row %d, "
                             "which differs in %s (a position file of another recording, or an edited one)"
                             % (what, count, n, first >> 2, GROUPS[first & 3]))
        rows = buf[:n * ROW_BYTES].copy().view(STATE_DTYPE)          # (copied as bytes: the pad bytes stay)
        if self.dist:
            return rows, self._host_dists.numpy()[:n * ROOT_DIST_BYTES].copy().view(ROOT_DIST_DTYPE)
        return rows


def reanalyse_rows(agent, game, rows, positions):
    """The State rows `rows` (STATE_DTYPE [n]) searched again from `positions` (POSITION_DTYPE [n], row i with row i) by `agent`
    (a ValueSim, ValueSimLP, ValueSimC or DistValueSim on a hip back end, agent.sims simulations a position) in batches of
    game.n_games: STATE_DTYPE [n] in the order given; for an agent whose store is KIND_DIST (DistValueSim) the pair (rows, dists),
    dists ROOT_DIST_DTYPE [n], row i with row i.  ValueError for a malformed game and for a row that is not its position's."""
    R = Reanalyser(agent, game)
    G, out, dists = game.n_games, [], []
    for a in range(0, len(rows), G):
        R.submit(rows[a:a + G], positions[a:a + G], what="rows %d..%d" % (a, min(a + G, len(rows)) - 1))
        got = R.collect()
        if R.dist:
            got, d = got
            dists.append(d)
        out.append(got)
    raw = [r.view(np.uint8).reshape(len(r), ROW_BYTES) for r in out] + [np.zeros((0, ROW_BYTES), np.uint8)]
    new = np.concatenate(raw).view(STATE_DTYPE).reshape(-1)
    if not R.dist:
        return new
    raw = [d.view(np.uint8).reshape(len(d), ROOT_DIST_BYTES) for d in dists] + [np.zeros((0, ROOT_DIST_BYTES), np.uint8)]
    return new, np.concatenate(raw).view(ROOT_DIST_DTYPE).reshape(-1)


def reanalyse_files(paths, out_dir, agent, game, last_nfiles=0, log=None):
    """reanalyse.py's loop: the State shards of `paths` (choose_inputs) with the position shards beside them -> shards of the same
    names, row counts and row order in out_dir, and copies of their .episodes tables.  Batches of game.n_games positions in file
    order, whatever the files' boundaries; a shard is written as soon as its last row has come back.  Returns the files written.
    An agent whose store is KIND_DIST (DistValueSim): the input must have root-distribution shards and their sidecar beside it,
    recorded by a head of the agent's atoms and range (RootDistLoader), and the re-analysed ones - rootdist<rest>.partNNNNN.npy
    and the sidecar - are written beside the State shards, each right after its State shard.
    ValueError, with nothing written of either table for the batch at fault or after it, for what PositionLoader, the load check
    and the guard refuse."""
    files = choose_inputs(paths, last_nfiles)
    if not files:
        raise ValueError("no State shards match %s" % (list(paths),))
    out_dir = str(out_dir)
    if any(os.path.abspath(os.path.dirname(f) or ".") == os.path.abspath(out_dir) for f in files):
        raise ValueError("--out_dir %s is the directory of the input: the re-analysed shards take the names of the recorded ones" % out_dir)
    names = [os.path.basename(f) for f in files]
    if len(set(names)) != len(names):
        raise ValueError("two inputs of the same file name would be written to the same output: %s" % sorted(names))
    R = Reanalyser(agent, game)
    if R.dist:
        data = RootDistLoader(files, positions=True)
        head, mine = (data.atoms, data.vmin, data.vmax), (int(agent.atoms), float(agent.vrange[0]), float(agent.vrange[1]))
        if head != mine:
            raise ValueError("the root distributions of %s were recorded by a head of (atoms, vmin, vmax) = %s, the agent's is %s"
                             % (files[0], head, mine))
        out_dists = np.zeros(data.length, ROOT_DIST_DTYPE)
        raw_dists = out_dists.view(np.uint8).reshape(data.length, ROOT_DIST_BYTES)
    else:
        data = PositionLoader(files)
    os.makedirs(out_dir, exist_ok=True)
    G, total = game.n_games, data.length
    ends = np.cumsum(data.counts)
    out = np.zeros(total, STATE_DTYPE)
    raw = out.view(np.uint8).reshape(total, ROW_BYTES)
    written = []

    def name_rows(a, b):
        j = int(np.searchsorted(ends, a, side="right"))
        return "%s rows %d..%d (batch rows %d..%d)" % (files[j], a - (ends[j] - data.counts[j]), b - 1 - (ends[j] - data.counts[j]), a, b - 1)

    def write_complete(done):
        """the shards whose last row is among the first `done` rows"""
        while len(written) < len(files) and ends[len(written)] <= done:
            j = len(written)
            lo = ends[j] - data.counts[j]
            target = os.path.join(out_dir, names[j])
            np.save(target, out[lo:ends[j]])
            if R.dist:
                write_root_dist_head(_PART.sub("", target), *mine)
                np.save(rootdist_file(target), out_dists[lo:ends[j]])
            ep = _PART.sub(lambda m: ".episodes" + m.group(0), files[j])
            if os.path.exists(ep):
                shutil.copyfile(ep, os.path.join(out_dir, os.path.basename(ep)))
            written.append(target)
            if log:
                log("%s: %d rows" % (target, data.counts[j]))

    for a in range(0, total, G):
        b = min(a + G, total)
        R.submit(data.rows[a:b], data.positions[a:b], what=name_rows(a, b))
        got = R.collect()
        if R.dist:
            got, d = got
            raw_dists[a:b] = d.view(np.uint8).reshape(b - a, ROOT_DIST_BYTES)
        raw[a:b] = got.view(np.uint8).reshape(b - a, ROW_BYTES)
        write_complete(b)
    write_complete(total)                            # (shards without a row at the end, or no row at all)
    return written
