"""Self-play records: the reference's `DataSaver` / `DataLoader` (util/Data.py:42-183) for a batch of games.

The reference writes one `State` row per move through the agent's and the game's getters into a PyTables file.  Here the rows
are written ON THE DEVICE (csrc/episodes.hip: tm_episode_record, tm_episode_advance) into a ring that is copied to pinned host
memory when it is full, and the host turns a copy into files later, when it needs that buffer again.  The container is numpy's
`.npy` (a table of fixed-size records), NOT HDF5: neither PyTables nor h5py is a dependency.  Where PyTables exists,
`table.append(rows[list(State.columns)])` converts a shard.

Files of `EpisodeRecorder(save_dir, save_file, cycle, ...)`, with stem = save_dir + save_file + str(cycle) (the reference's file
name; `.r<rank>` is appended under torch.distributed with more than one rank, and episode ids are then rank-local):
    <stem>.part00000.npy, .part00001.npy, ...             STATE_DTYPE rows, move-major, slot-minor
    <stem>.episodes.part00000.npy, ...                    EPISODE_DTYPE rows: the episodes that ended, with their FINAL score
Opening over existing parts continues their numbering and the episode ids (the reference's mode='a').

After record_positions() (play.py --save_positions) the device writes, beside every State row, a POSITION row of 96 bytes
(tm_episode_record_positions): the row's identity, the packed game the row was made from and its line statistics - what a later
re-analysis (reanalyse.py) loads into an environment and searches again.  They go into
    <dir>positions<rest>.part00000.npy, ...               POSITION_DTYPE rows; <rest>: the stem's file name after "data"
(positions_stem), with the part number, the row count and the row order of the State shard the same flush wrote.

After record_root_dists() (play.py --agent_type DistValueSim --save_root_dists) the device also writes a ROOT-DISTRIBUTION row of
272 bytes (tm_episode_record_root_dists): the row's identity and the 64 floats of the distribution the search backed up into the
root - what the distributional head is fitted to (train.py --head dist --td --bootstrap search).  They go into
    <dir>rootdist<rest>.part00000.npy, ...                ROOT_DIST_DTYPE rows, paired with the State shard as the positions are
    <dir>rootdist<rest>.head.npy                          float64 [3] = atoms, vmin, vmax of the head (nodes.py's sidecar)
"""
import ctypes as C
import glob
import os
import re
from typing import NamedTuple

import numpy as np

ROW_BYTES, DONE_BYTES, SLOT_DW = 368, 40, 4       # TM_EPISODE_ROW_BYTES, TM_EPISODE_DONE_BYTES, TM_EPISODE_SLOT_DW
POSITION_BYTES = 96                               # TM_POSITION_ROW_BYTES
ROOT_DIST_BYTES, DIST_ROW = 272, 64               # TM_ROOT_DIST_ROW_BYTES, TM_DIST_ROW
N_ACTIONS = 7

# the reference's State columns (util/Data.py:14-26) plus slot and move; the order is the device row's, readers go by name
STATE_DTYPE = np.dtype({
    "names": ["episode", "cycle", "slot", "move", "combo", "lines", "score", "line_stats", "value", "variance", "child_stats",
              "policy", "board", "action"],
    "formats": ["<i4", "<i4", "<i4", "<i4", "<i4", "<i4", "<i4", ("<i4", (4,)), "<f4", "<f4", ("<f4", (3, N_ACTIONS)),
                ("<f4", (N_ACTIONS,)), ("i1", (20, 10)), "i1"],
    "offsets": [0, 4, 8, 12, 16, 20, 24, 28, 44, 48, 52, 136, 164, 364],
    "itemsize": ROW_BYTES})
EPISODE_DTYPE = np.dtype({
    "names": ["episode", "cycle", "slot", "moves", "score", "lines", "line_stats"],
    "formats": ["<i4", "<i4", "<i4", "<i4", "<i4", "<i4", ("<i4", (4,))],
    "offsets": [0, 4, 8, 12, 16, 20, 24],
    "itemsize": DONE_BYTES})
# the game a State row was recorded from (include/tetris_mcts_hip.h, the table at tm_episode_record_positions)
POSITION_DTYPE = np.dtype({
    "names": ["episode", "cycle", "slot", "move", "game", "line_stats"],
    "formats": ["<i4", "<i4", "<i4", "<i4", ("<u4", (16,)), ("<i4", (4,))],
    "offsets": [0, 4, 8, 12, 16, 80],
    "itemsize": POSITION_BYTES})
# the distribution the search backed up into the root a State row was recorded at (the table at tm_episode_record_root_dists)
ROOT_DIST_DTYPE = np.dtype({
    "names": ["episode", "cycle", "slot", "move", "dist"],
    "formats": ["<i4", "<i4", "<i4", "<i4", ("<f4", (DIST_ROW,))],
    "offsets": [0, 4, 8, 12, 16],
    "itemsize": ROOT_DIST_BYTES})
IDENTITY = ("episode", "cycle", "slot", "move")

_PART = re.compile(r"\.part(\d{5})\.npy$")


def _parts(stem, episodes=False):
    """the existing part files of a stem in the order of their numbers"""
    found = glob.glob(glob.escape(stem) + (".episodes" if episodes else "") + ".part[0-9][0-9][0-9][0-9][0-9].npy")
    return sorted(found, key=lambda f: int(_PART.search(f).group(1)))


class Companion(NamedTuple):
    """A table recorded beside the State rows, row for row: what the writer, the recorder and the loaders know of it."""
    key: str             # the keyword of ShardWriter.write and of the loaders
    prefix: str          # the file name's, in place of "data"
    dtype: np.dtype
    phrase: str          # in messages
    hint: str            # how such shards come about

    @property
    def adj(self):
        return self.phrase.replace(" ", "-")


POSITIONS = Companion("positions", "positions", POSITION_DTYPE, "position", "record with play.py --save --save_positions")
ROOT_DISTS = Companion("root_dists", "rootdist", ROOT_DIST_DTYPE, "root distribution",
                       "record with play.py --agent_type DistValueSim --save --save_root_dists")
COMPANIONS = (POSITIONS, ROOT_DISTS)     # the order of the writer's names, of the flush's copies and of the attributes


def companion_stem(table, stem):
    """The stem of a companion's shards that go with the State shards of `stem`: the prefix in place of a file name's leading "data"
    (D/data3.r1 -> D/positions3.r1, D/rootdist3.r1), the prefix and "." before any other file name - never a name that `D/data*`,
    `D/dist*` or another companion's prefix matches."""
    d, base = os.path.split(str(stem))
    return os.path.join(d, table.prefix + base[4:] if base.startswith("data") else table.prefix + "." + base)


def companion_file(table, state_file):
    """a companion's shard of a State shard: the same part of companion_stem"""
    m = _PART.search(str(state_file))
    if not m:
        raise ValueError("%s is not a part of a stem" % state_file)
    return companion_stem(table, str(state_file)[:m.start()]) + m.group(0)


def positions_stem(stem):
    """the stem of the position shards that go with the State shards of `stem` (companion_stem)"""
    return companion_stem(POSITIONS, stem)


def positions_file(state_file):
    """the position shard of a State shard: the same part of positions_stem"""
    return companion_file(POSITIONS, state_file)


def rootdist_stem(stem):
    """the stem of the root-distribution shards that go with the State shards of `stem` (companion_stem)"""
    return companion_stem(ROOT_DISTS, stem)


def rootdist_file(state_file):
    """the root-distribution shard of a State shard: the same part of rootdist_stem"""
    return companion_file(ROOT_DISTS, state_file)


def write_root_dist_head(stem, atoms, vmin, vmax):
    """The sidecar of the root-distribution shards of the State stem `stem`, <rootdist_stem>.head.npy (float64 [3]: atoms, vmin,
    vmax; nodes.write_head): written if it is not there, a ValueError if one is there that says otherwise.  Returns its name."""
    from .nodes import write_head
    return write_head(rootdist_stem(stem), atoms, vmin, vmax, "distributions go")[0]


def _stem(save_dir, save_file, cycle, rank=None):
    """save_dir + save_file + str(cycle), `.r<rank>` after it for a rank; the stem's directory is made"""
    stem = "%s%s%s" % (save_dir, save_file, cycle)
    if rank is not None:
        stem += ".r%d" % rank
    d = os.path.dirname(stem)
    if d:
        os.makedirs(d, exist_ok=True)
    return stem


def _rank():
    """this process's rank under torch.distributed with more than one rank, else None"""
    import torch
    if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
        return torch.distributed.get_rank()
    return None


def _keep_raw(table, keep, dtype):
    """the rows `keep` of a table as whole rows of bytes: the pad bytes stay what the device wrote"""
    return np.ascontiguousarray(table).view(np.uint8).reshape(len(table), dtype.itemsize)[keep].view(dtype).reshape(-1)


class ShardWriter:
    """The host half of the recorder: numbered shards of a stem.  `write(rows, episodes, n_done, cap)` takes a flush as the
    device left it - STATE_DTYPE rows with episode == -1 where a game had ended, the `done` buffer of `cap` EPISODE_DTYPE rows
    of which the first n_done are valid - drops the -1 rows and writes the next part of both tables."""

    def __init__(self, save_dir, save_file, cycle, rank=None):
        self.stem = _stem(save_dir, save_file, cycle, rank)
        have, have_ep = _parts(self.stem), _parts(self.stem, episodes=True)
        self.part = 1 + max([int(_PART.search(f).group(1)) for f in have + have_ep], default=-1)
        # the ids already given: the episodes that ended, and the ones under way in the last rows written
        ids = [int(t["episode"].max()) for t in (np.load(f, mmap_mode="r") for f in have_ep) if len(t)]
        if have:
            last = np.load(have[-1], mmap_mode="r")
            if len(last):
                ids.append(int(last["episode"].max()))
        self.next_id = 1 + max(ids, default=-1)

    def write(self, rows, episodes, n_done, cap, positions=None, root_dists=None):
        """positions: None, or the flush's POSITION_DTYPE rows, one per row of `rows` in the same order: the rows the State rows'
        mask keeps are written as the same part of positions_stem(stem) (returned as a third name).  root_dists: None, or the
        flush's ROOT_DIST_DTYPE rows in the same way: the same part of rootdist_stem(stem) (returned as the last name)."""
        n_done = int(n_done)
        if n_done > int(cap) or n_done > len(episodes):
            raise RuntimeError("episode log overflow: %d episodes ended since the last flush, the buffer holds %d - their rows "
                               "are lost; flush more often (ring_moves)" % (n_done, min(int(cap), len(episodes))))
        beside = [(t, table) for t, table in zip(COMPANIONS, (positions, root_dists)) if table is not None]
        for t, table in beside:
            if len(table) != len(rows):
                raise ValueError("%d %s rows for %d State rows" % (len(table), t.adj, len(rows)))
        keep = rows["episode"] != -1             # the one mask: what it drops is dropped from every table
        beside = [(t, _keep_raw(table, keep, t.dtype)) for t, table in beside]
        rows = _keep_raw(rows, keep, STATE_DTYPE)
        names = ("%s.part%05d.npy" % (self.stem, self.part), "%s.episodes.part%05d.npy" % (self.stem, self.part))
        np.save(names[0], rows)
        np.save(names[1], np.ascontiguousarray(episodes[:n_done]))
        for t, table in beside:
            names += ("%s.part%05d.npy" % (companion_stem(t, self.stem), self.part),)
            np.save(names[-1], table)
        self.part += 1
        return names


class EpisodeRecorder:
    """DataSaver for a batch: add(agent, game) right after agent.play(), advance(game) right after game.play(action) and
    before game.reset('ended'), close() at the end.

    Device: a ring of ring_moves x G State rows, a `done` buffer of ring_moves x G episode rows (a slot ends at most once a move,
    so it cannot overflow between two flushes), the per-slot state and the counters.  add() and advance() are one kernel launch
    each.  When the ring is full (and at close()) a FLUSH copies ring, done buffer and counters into one of two pinned host
    buffers with stream-ordered asynchronous copies followed by an event, and clears n_done on the device; nothing waits.  The
    host makes files of a pinned buffer only when it needs that buffer again, two flushes later, or at close(); the event's
    synchronize() is then the only wait there is, on work enqueued 2 x ring_moves moves before."""

    def __init__(self, save_dir, save_file, cycle, n_games, ring_moves=64, device="cuda"):
        import torch
        from . import _lib
        if int(n_games) < 1 or int(ring_moves) < 1:
            raise ValueError("n_games and ring_moves must be at least 1")
        self.L = _lib.lib()
        self.torch, self._check = torch, _lib.check
        self.cycle, self.G, self.ring_moves = int(cycle), int(n_games), int(ring_moves)
        self.device = torch.device(device)
        self.writer = ShardWriter(save_dir, save_file, cycle, _rank())
        self.cap = self.ring_moves * self.G
        dev = self.device
        self.ring = torch.zeros(self.cap * ROW_BYTES, dtype=torch.uint8, device=dev)
        self.done = torch.zeros(self.cap * DONE_BYTES, dtype=torch.uint8, device=dev)
        self.slot_state = torch.zeros(self.G, SLOT_DW, dtype=torch.int32, device=dev)
        self.counters = torch.zeros(2, dtype=torch.int32, device=dev)
        self._act = torch.zeros(self.G, dtype=torch.int32, device=dev)
        # a pinned buffer: the ring, the done buffer, then the counters
        self._off_done = self.cap * ROW_BYTES
        self._off_cnt = self._off_done + self.cap * DONE_BYTES
        self._host = [torch.zeros(self._off_cnt + 8, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.positions = False               # record_positions()
        self.root_dists = False              # record_root_dists()
        self._beside = {}                    # per companion recorded, by its keyword: (ring, the two pinned buffers)
        self._pending = [None, None]         # per pinned buffer: (event, moves held)
        self._flushes, self._pos, self.closed = 0, 0, False
        self.files = []
        self._check(self.L.tm_episode_init(self.G, self.writer.next_id, self._p(self.slot_state), self._p(self.counters),
                                           self._stream()), "tm_episode_init")

    def _before_add(self, caller):
        if self._pos or self._flushes or self.closed:
            raise RuntimeError("EpisodeRecorder.%s comes before the first add()" % caller)

    def _record_beside(self, table, caller, head=None):
        """A companion's ring of ring_moves x G rows beside the State ring and a pair of pinned buffers of its own, copied by the
        same flush and waited for by the same event; returns the ring.  A second call allocates nothing.  head: the (atoms, vmin,
        vmax) of the stem's sidecar, written first, so that a stem of another head leaves no ring behind."""
        self._before_add(caller)
        if table.key not in self._beside:
            if head is not None:
                write_root_dist_head(self.writer.stem, *head)
            torch, n = self.torch, self.cap * table.dtype.itemsize
            self._beside[table.key] = (torch.zeros(n, dtype=torch.uint8, device=self.device),
                                       [torch.zeros(n, dtype=torch.uint8).pin_memory() for _ in range(2)])
        return self._beside[table.key][0]

    def record_positions(self):
        """Also write a position row of 96 bytes beside every State row (play.py --save_positions): call once, before the first
        add()."""
        self.pos_ring = self._record_beside(POSITIONS, "record_positions")
        self.positions = True

    def record_root_dists(self, atoms, vmin, vmax):
        """Also write a root-distribution row of 272 bytes beside every State row (play.py --save_root_dists; an agent whose store
        is KIND_DIST): call once, before the first add(), with the head's atoms and range, which go into the stem's sidecar."""
        self.dist_ring = self._record_beside(ROOT_DISTS, "record_root_dists", (atoms, vmin, vmax))
        self.root_dists = True

    def resume(self, move_idx):
        """Games that go on from an earlier run (games.py): call once, before the first add(), with the moves played so far in
        each slot's episode.  The rows then continue that run's move numbers slot by slot (tm_episode_resume); episode ids are
        numbered as without it."""
        self._before_add("resume")
        m = np.ascontiguousarray(np.asarray(move_idx).reshape(-1), dtype=np.int32)
        if m.shape != (self.G,):
            raise ValueError("move_idx: %d entries for %d games" % (m.size, self.G))
        self._move_idx = self.torch.from_numpy(m).to(self.device)
        self._check(self.L.tm_episode_resume(self.G, self.writer.next_id, self._p(self._move_idx), self._p(self.slot_state),
                                             self._p(self.counters), self._stream()), "tm_episode_resume")

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    @staticmethod
    def _p(t, offset=0):
        return C.c_void_p(t.data_ptr() + offset)

    def add(self, agent=None, game=None, action=None):
        """Record this move of every game: call after agent.play() (the statistics are the store's root_stats buffers as the
        last get_action() left them) and before game.play().  `action`: what is actually played where that is not the agent's
        choice (an int, an array or a tensor of n_games)."""
        store = getattr(agent, "store", None)
        if store is None or game is None:
            raise TypeError("EpisodeRecorder.add needs a TreeAgent (with its store built) and the game")
        torch = self.torch
        if store.n_games != self.G or game.n_games != self.G:
            raise ValueError("the recorder was made for %d games" % self.G)
        if self.root_dists:
            from .store import KIND_DIST
            if store.s.kind != KIND_DIST or store.t.get("node_dist") is None:
                raise TypeError("record_root_dists records the root's distribution of a distributional tree (DistValueSim): this "
                                "agent's store is of kind %d and keeps none" % store.s.kind)
        if self._pos == self.ring_moves:
            self._flush()
        act = store.action_buf
        if action is not None:
            if torch.is_tensor(action):
                self._act.copy_(action.to(torch.int32).reshape(-1), non_blocking=True)
            else:
                self._act.copy_(torch.from_numpy(np.array(np.broadcast_to(np.asarray(action, np.int32).reshape(-1), (self.G,)))))
            act = self._act
        self._check(self.L.tm_episode_record(C.byref(game.s), C.byref(store.s), self._p(store.stats_buf), self._p(act), self.cycle,
                                             self._p(self.slot_state), self._p(self.ring, self._pos * self.G * ROW_BYTES),
                                             self._stream()), "tm_episode_record")
        if self.positions:
            self._check(self.L.tm_episode_record_positions(C.byref(game.s), self._p(self.slot_state), self.cycle,
                                                           self._p(self.pos_ring, self._pos * self.G * POSITION_BYTES),
                                                           self._stream()), "tm_episode_record_positions")
        if self.root_dists:
            self._check(self.L.tm_episode_record_root_dists(C.byref(store.s), self._p(self.ring, self._pos * self.G * ROW_BYTES), self.G,
                                                            self._p(self.dist_ring, self._pos * self.G * ROOT_DIST_BYTES),
                                                            self._stream()), "tm_episode_record_root_dists")
        self._pos += 1

    def advance(self, game):
        """Number the episodes: call after game.play(action) and before ended games are reset."""
        self._check(self.L.tm_episode_advance(C.byref(game.s), self.cycle, self._p(self.slot_state), self._p(self.counters),
                                              self._p(self.done), self.cap, self._stream()), "tm_episode_advance")
        if self._pos == self.ring_moves:
            self._flush()

    def _recorded_beside(self):
        """(companion, (ring, pinned buffers)) of the companions recorded, in COMPANIONS' order whatever the order of the calls"""
        return [(t, self._beside[t.key]) for t in COMPANIONS if t.key in self._beside]

    def _flush(self):
        k = self._flushes % 2
        self._drain(k)                       # the buffer's earlier contents become files first
        host, n = self._host[k], self._pos * self.G * ROW_BYTES
        host[:n].copy_(self.ring[:n], non_blocking=True)
        host[self._off_done:self._off_cnt].copy_(self.done, non_blocking=True)
        host[self._off_cnt:].copy_(self.counters.view(self.torch.uint8), non_blocking=True)
        for t, (ring, hosts) in self._recorded_beside():
            m = self._pos * self.G * t.dtype.itemsize
            hosts[k][:m].copy_(ring[:m], non_blocking=True)
        self.counters[1:].zero_()            # the done buffer starts over (stream-ordered, after the copy)
        ev = self.torch.cuda.Event()
        ev.record()
        self._pending[k] = (ev, self._pos)
        self._flushes += 1
        self._pos = 0

    def _drain(self, k):
        if self._pending[k] is None:
            return
        ev, moves = self._pending[k]
        self._pending[k] = None
        ev.synchronize()
        buf = self._host[k].numpy()
        rows = buf[:moves * self.G * ROW_BYTES].view(STATE_DTYPE)
        episodes = buf[self._off_done:self._off_cnt].view(EPISODE_DTYPE)
        n_done = int(buf[self._off_cnt:].view(np.int32)[1])
        beside = {t.key: hosts[k].numpy()[:moves * self.G * t.dtype.itemsize].view(t.dtype) for t, (_, hosts) in self._recorded_beside()}
        self.files.append(self.writer.write(rows, episodes, n_done, self.cap, **beside))

    def close(self):
        """flush the partial ring and write every copy that is still held"""
        if self.closed:
            return
        self.closed = True
        if self._pos:
            self._flush()
        for k in (self._flushes % 2, (self._flushes + 1) % 2):      # the older copy first: parts are in the order of the moves
            self._drain(k)


def _concat(tables, dtype):
    """the tables one after the other IN `dtype` (np.concatenate would pack the fields and lose the row's layout)"""
    for t in tables:
        if t.dtype != dtype:
            raise ValueError("a shard of another layout: %s" % (t.dtype,))
    raw = [np.ascontiguousarray(t).view(np.uint8).reshape(len(t), dtype.itemsize) for t in tables]
    return np.concatenate(raw + [np.zeros((0, dtype.itemsize), np.uint8)]).view(dtype).reshape(-1)


def _expand(list_of_files):
    """state shards named directly, or through a stem; in the order (stem, part)"""
    if isinstance(list_of_files, (str, os.PathLike)):
        list_of_files = [list_of_files]
    out = []
    for f in map(str, list_of_files):
        if ".episodes.part" in f:
            continue
        out.extend([f] if _PART.search(f) else _parts(f))
    key = lambda f: (_PART.sub("", f), int(_PART.search(f).group(1)))  # noqa: E731
    return sorted(dict.fromkeys(out), key=key)


class EpisodeLoader:
    """The reference's DataLoader (util/Data.py:135-183) over shards: every column a concatenated attribute, `length`, the get*
    accessors; `.episodes` the table of ended episodes that goes with the shards.  list_of_files: state shards or stems.
    by_episode: rows stable-sorted by (cycle, episode, move), so that an episode's rows are contiguous and in order, as the
    reference's consumers assume; False: the order of the files (move-major, slot-minor)."""

    def __init__(self, list_of_files, by_episode=True):
        self.files = _expand(list_of_files)
        rows = _concat([np.load(f) for f in self.files], STATE_DTYPE)
        if by_episode:
            order = np.lexsort((rows["move"], rows["episode"], rows["cycle"]))           # (lexsort is stable)
            rows = rows.view(np.uint8).reshape(len(rows), ROW_BYTES)[order].view(STATE_DTYPE).reshape(-1)
        self.rows = rows
        for c in STATE_DTYPE.names:
            setattr(self, c, np.ascontiguousarray(rows[c]))
        self.length = len(rows)
        ep_files = [f for f in (_PART.sub(lambda m: ".episodes" + m.group(0), s) for s in self.files) if os.path.exists(f)]
        self.episodes = _concat([np.load(f) for f in ep_files], EPISODE_DTYPE)

    def bound_index(self, index):
        return min(max(index, 0), self.length - 1)

    def getBoard(self, index):
        return self.board[self.bound_index(index)]

    def getPolicy(self, index):
        return self.policy[self.bound_index(index)]

    def getCycle(self, index):
        return self.cycle[self.bound_index(index)]

    def getScore(self, index):
        return self.score[self.bound_index(index)]

    def getLines(self, index):
        return self.lines[self.bound_index(index)]

    def getCombo(self, index):
        return self.combo[self.bound_index(index)]


def _check_paired(f, r, of, o, what):
    """ValueError, naming the file and the row, unless table `o` (of file `of`) has the rows of the State table `r` (of `f`)"""
    if len(o) != len(r):
        raise ValueError("%s holds %d rows, %s holds %d: row %d has no %s" % (
            of, len(o), f, len(r), min(len(o), len(r)), what if len(o) < len(r) else "State row"))
    bad = np.zeros(len(r), bool)
    for c in IDENTITY:
        bad |= r[c] != o[c]
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise ValueError("%s: row %d is (episode, cycle, slot, move) = %s, row %d of %s is %s: the two files do not belong "
                         "together" % (of, i, tuple(int(o[c][i]) for c in IDENTITY), i, f, tuple(int(r[c][i]) for c in IDENTITY)))


def _load_paired(files, tables):
    """The State shards `files` and, beside each, the shard of every companion of `tables` (at least one), paired part by part.
    Checked file by file and, within a file, companion by companion in the order of `tables`: the companion's shard is there, the
    State shard's layout, the companion's layout, its length and identity columns (_check_paired).  Returns the State table, the
    rows per file and {keyword: (the companion's files, its table)}."""
    names = {t.key: [companion_file(t, f) for f in files] for t in tables}
    rows, beside = [], {t.key: [] for t in tables}
    for i, f in enumerate(files):
        r = None
        for t in tables:
            of = names[t.key][i]
            if not os.path.isfile(of):
                raise ValueError("%s: there is no %s shard %s beside it (%s)" % (f, t.adj, of, t.hint))
            first = r is None
            if first:
                r = np.load(f)
            o = np.load(of)                  # (both are read before either layout is judged)
            if first and r.dtype != STATE_DTYPE:
                raise ValueError("a shard of another layout: %s: %s" % (f, r.dtype))
            if o.dtype != t.dtype:
                raise ValueError("a %s shard of another layout: %s: %s" % (t.adj, of, o.dtype))
            _check_paired(f, r, of, o, t.phrase)
            beside[t.key].append(o)
        rows.append(r)
    return _concat(rows, STATE_DTYPE), [len(r) for r in rows], {t.key: (names[t.key], _concat(beside[t.key], t.dtype)) for t in tables}


class PositionLoader:
    """State shards and the position shards recorded beside them, paired part by part in the order of the files.
    stems_or_files: State shards or stems, as EpisodeLoader takes them.  `.files` / `.position_files` the pairs, `.rows`
    (STATE_DTYPE) and `.positions` (POSITION_DTYPE) the tables, row i of one with row i of the other, `.counts` the rows per file.
    ValueError, naming the file and the row, for a position shard that is missing or of another length and for a row whose
    identity (episode, cycle, slot, move) differs."""

    def __init__(self, stems_or_files):
        self.files = _expand(stems_or_files)
        self.rows, self.counts, beside = _load_paired(self.files, [POSITIONS])
        self.position_files, self.positions = beside["positions"]
        self.length = len(self.rows)


class RootDistLoader:
    """State shards and the root-distribution shards recorded beside them (play.py --save_root_dists, reanalyse.py --root_dists),
    paired part by part in the order of the files.  stems_or_files: State shards or stems, as EpisodeLoader takes them.  `.files` /
    `.dist_files` the pairs, `.rows` (STATE_DTYPE) and `.dists` (ROOT_DIST_DTYPE) the tables, row i of one with row i of the other,
    `.counts` the rows per file, `.atoms`, `.vmin`, `.vmax` the head of the stems' sidecars (which must agree).  positions: True -
    the position shards are paired too (`.position_files`, `.positions`), as PositionLoader pairs them; None - where every State
    shard has one; False - not.  ValueError, naming the file and the row, for a shard that is missing or of another length and for a
    row whose identity (episode, cycle, slot, move) differs; for a stem without a sidecar and for sidecars that disagree."""

    def __init__(self, stems_or_files, positions=None):
        from .nodes import load_head
        self.files = _expand(stems_or_files)
        if positions is None:
            positions = bool(self.files) and all(os.path.isfile(positions_file(f)) for f in self.files)
        self.rows, self.counts, beside = _load_paired(self.files, [ROOT_DISTS, POSITIONS] if positions else [ROOT_DISTS])
        self.dist_files, self.dists = beside["root_dists"]
        self.position_files = None
        if positions:
            self.position_files, self.positions = beside["positions"]
        self.length = len(self.rows)
        self.atoms, self.vmin, self.vmax = load_head(dict.fromkeys(rootdist_stem(_PART.sub("", f)) for f in self.files))


def record_root_dists_numpy(state_rows, roots, node_dist, atoms):
    """tm_episode_record_root_dists as a numpy statement: ROOT_DIST_DTYPE [n].  state_rows: STATE_DTYPE [n], the rows just written
    for the slots 0 .. n-1; roots: int [>= n], gs[g][ROOT]; node_dist: float32 [G, max_nodes, 64]; atoms: the store's dist_bins.
    The identity is the State row's; dist the BITS of node_dist[g, roots[g], :atoms], zeros from `atoms` on; a State row with
    episode -1 gives -1 and zeros; a root outside [0, max_nodes) gives a dist of zeros."""
    n, atoms = len(state_rows), int(atoms)
    if not 1 <= atoms <= DIST_ROW:
        raise ValueError("atoms: 1 .. 64, not %r" % (atoms,))
    nd = np.ascontiguousarray(node_dist, dtype=np.float32).view(np.uint32)
    if nd.ndim != 3 or nd.shape[2] != DIST_ROW or nd.shape[0] < n:
        raise ValueError("node_dist: float32 [>= %d, max_nodes, 64], not %s" % (n, nd.shape))
    out = np.zeros(n, ROOT_DIST_DTYPE)
    bits = out["dist"].view(np.uint32)                         # (bits, not values: a NaN's payload stays)
    roots = np.asarray(roots).reshape(-1)[:n].astype(np.int64)
    for g in range(n):
        if state_rows["episode"][g] == -1:
            out["episode"][g] = -1
            continue
        for c in IDENTITY:
            out[c][g] = state_rows[c][g]
        if 0 <= roots[g] < nd.shape[1]:
            bits[g, :atoms] = nd[g, roots[g], :atoms]
    return out
