"""Node records: the tuples the collections harvest, written to files (the reference's `--save_tree` idea, Agent.save_nodes at
every collection, agents/agent.py:246-289, ValueSim.py:117-118 - with another row: what a fit needs, not the HDF5 State row).

A collection harvests on the device the packed observation, value, variance and visits of every freed observation with at least
`min_visits_to_store` visits (tree.hip; tm_store.replay_obs / replay_stat / replay_count).  The online fit consumes those tuples
and throws them away; `NodeRecorder` moves them after every move into ONE dense ring of 64-byte rows (csrc/node_records.hip:
tm_nodes_drain), copies the rows in use to pinned host memory every few moves and turns a copy into a file later, when it needs
that buffer again - the scheme of episodes.EpisodeRecorder.  The device row is the file's row.

Files of `NodeRecorder(save_dir, save_file, cycle, ...)`, with stem = save_dir + save_file + str(cycle) (`.r<rank>` is appended
under torch.distributed with more than one rank):
    <stem>.part00000.npy, .part00001.npy, ...             NODE_DTYPE rows: per flush game-major, harvest order within a game
Opening over existing parts continues their numbering.  A flush that holds no row writes no file.

The volume is bounded by the search: an observation reaches `min_visit` visits only through visits, and a move of one game
makes sims x (mean trace length) of them, so a game and move adds at most sims x mean trace length / min_visit rows.
"""
import ctypes as C
import os
import sys

import numpy as np

from .episodes import _PART, _concat, _expand, _parts

ROW_BYTES = 64                 # TM_NODE_ROW_BYTES
NODE_DTYPE = np.dtype({
    "names": ["obs", "value", "variance", "visit", "slot"],
    "formats": [("<u4", (12,)), "<f4", "<f4", "<f4", "<i4"],
    "offsets": [0, 48, 52, 56, 60],
    "itemsize": ROW_BYTES})
# The default ring (2^22 rows: 256 MiB on the device and twice that pinned) is 6.0 times the largest flush measured at 4 096 games x
# 100 simulations with min_visit 40 (696 859 rows; 8 980 rows a move on average: profiles/node_records_timing.json);
# a flush at least every 8 moves keeps a file at tens of megabytes there.
RING_ROWS, FLUSH_MOVES = 1 << 22, 8


class NodeShardWriter:
    """The host half of the recorder: the numbered shards of a stem.  `write(rows)` writes the next part (nothing for no rows)."""

    def __init__(self, save_dir, save_file, cycle, rank=None):
        self.stem = "%s%s%s" % (save_dir, save_file, cycle)
        if rank is not None:
            self.stem += ".r%d" % rank
        d = os.path.dirname(self.stem)
        if d:
            os.makedirs(d, exist_ok=True)
        self.part = 1 + max([int(_PART.search(f).group(1)) for f in _parts(self.stem)], default=-1)

    def write(self, rows):
        if rows.dtype != NODE_DTYPE:
            raise ValueError("rows: a table of NODE_DTYPE, not %s" % (rows.dtype,))
        if not len(rows):
            return None
        name = "%s.part%05d.npy" % (self.stem, self.part)
        np.save(name, np.ascontiguousarray(rows))
        self.part += 1
        return name


def report_loss(lost, dropped, ring_rows, replay_cap, out=None):
    """Loss is never silent: rows that did not fit the ring, tuples that did not fit a game's harvest buffer (out: sys.stderr as
    it is when the call is made)"""
    out = sys.stderr if out is None else out
    if lost > 0:
        print("WARNING: {} node rows did not fit the recorder's ring (ring_rows={}) and are lost; raise ring_rows or flush more "
              "often (flush_moves)".format(lost, ring_rows), file=out, flush=True)
    if dropped > 0:
        print("WARNING: {} harvested tuples did not fit the device replay buffer (replay_cap={}) and are lost; raise replay_cap"
              .format(dropped, replay_cap), file=out, flush=True)


class NodeRecorder:
    """drain(agent) right after every move (after agent.update_root(game): never beside a search), close(agent) at the end.

    Device: a ring of `ring_rows` node rows, the four counters (head, lost, drains, spare) and the scan's scratch.  drain() is one
    tm_nodes_drain followed by a 16-byte asynchronous copy of the counters to pinned memory and an event.  The next drain, a move
    later, synchronises on that event - recorded a whole move earlier, so the call returns at once in practice, though it is a
    wait in form - and reads the ring's head, exact because nothing has drained since.  When the head has reached half the ring,
    or `flush_moves` drains after the last flush if the ring holds anything, a FLUSH copies the rows in use and the counters into
    one of two pinned host buffers with stream-ordered asynchronous copies followed by an event, and clears head and lost on the
    device; the flush itself waits for nothing.  The host makes a file of a pinned buffer only when it needs that buffer again,
    two flushes later, or at close(); that event's synchronize() is the only other wait.  A single drain that brings more rows
    than the ring has free loses the rest (never silently): the ring should hold twice the largest burst of one move.
    `agent`: a ValueSim, ValueSimLP or ValueSimC built with harvest=True."""

    def __init__(self, save_dir, save_file, cycle, n_games, ring_rows=RING_ROWS, flush_moves=FLUSH_MOVES, device="cuda"):
        import torch
        from . import _lib
        if int(n_games) < 1 or int(ring_rows) < 1 or int(flush_moves) < 1:
            raise ValueError("n_games, ring_rows and flush_moves must be at least 1")
        self.L = _lib.lib()
        self.torch, self._check = torch, _lib.check
        self.cycle, self.G, self.ring_rows, self.flush_moves = int(cycle), int(n_games), int(ring_rows), int(flush_moves)
        self.device = torch.device(device)
        rank = None
        if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            rank = torch.distributed.get_rank()
        self.writer = NodeShardWriter(save_dir, save_file, cycle, rank)
        dev = self.device
        self._ring_bytes = self.ring_rows * ROW_BYTES
        self.ring = torch.zeros(self._ring_bytes, dtype=torch.uint8, device=dev)
        self.counters = torch.zeros(4, dtype=torch.int32, device=dev)
        self.offsets = torch.zeros(self.G + 1, dtype=torch.int32, device=dev)
        self._host = [torch.zeros(self._ring_bytes + 16, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self._pending = [None, None]         # per pinned buffer: the event of its copy
        self._seen = torch.zeros(4, dtype=torch.int32).pin_memory()      # the counters as the last drain left them
        self._seen_ev = None
        self._flushes, self._since, self.closed = 0, 0, False
        self.files, self.rows_written, self.lost = [], 0, 0
        self._dropped_seen = 0
        self._replay_cap = 0

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    @staticmethod
    def _p(t):
        return C.c_void_p(t.data_ptr())

    def _store(self, agent):
        store = getattr(agent, "store", None)
        if store is None:
            raise TypeError("NodeRecorder needs a TreeAgent (with its store built)")
        if store.n_games != self.G:
            raise ValueError("the recorder was made for %d games" % self.G)
        if not store.s.online or store.s.replay_cap < 1:
            raise ValueError("the agent's store does not harvest: build the agent with harvest=True")
        self._replay_cap = int(store.s.replay_cap)
        return store

    def _head(self):
        """the ring's head as the last drain left it (nothing has drained since); the copy it reads was enqueued a move ago"""
        if self._seen_ev is None:
            return 0
        self._seen_ev.synchronize()
        return int(self._seen.numpy()[0])

    def _drain(self, store):
        self._check(self.L.tm_nodes_drain(C.byref(store.s), self._p(self.ring), self.ring_rows, self._p(self.counters),
                                          self._p(self.offsets), self._stream()), "tm_nodes_drain")
        self._seen.copy_(self.counters, non_blocking=True)
        self._seen_ev = self.torch.cuda.Event()
        self._seen_ev.record()
        self._since += 1

    def drain(self, agent):
        """Move what the collections of the last move harvested into the ring: one tm_nodes_drain."""
        store = self._store(agent)
        head = self._head()
        if head and (2 * head >= self.ring_rows or self._since >= self.flush_moves):
            self._flush(head)
        self._drain(store)

    def _flush(self, head):
        k = self._flushes % 2
        self._write(k)                       # the buffer's earlier contents become a file first
        host, n = self._host[k], head * ROW_BYTES
        host[:n].copy_(self.ring[:n], non_blocking=True)
        host[self._ring_bytes:].copy_(self.counters.view(self.torch.uint8), non_blocking=True)
        self.counters[:2].zero_()            # the ring starts over (stream-ordered, after the copy)
        ev = self.torch.cuda.Event()
        ev.record()
        self._pending[k] = ev
        self._flushes += 1
        self._since, self._seen_ev = 0, None

    def _write(self, k):
        if self._pending[k] is None:
            return
        ev, self._pending[k] = self._pending[k], None
        ev.synchronize()
        buf = self._host[k].numpy()
        head, lost = (int(x) for x in buf[self._ring_bytes:].view(np.int32)[:2])
        name = self.writer.write(buf[:head * ROW_BYTES].view(NODE_DTYPE))
        if name:
            self.files.append(name)
        self.rows_written += head
        self.lost += lost
        report_loss(lost, 0, self.ring_rows, self._replay_cap)

    def close(self, agent, occupied=False):
        """drain, optionally append the observations still in the pools (tm_nodes_sweep, the reference's save_occupied), flush
        and write every copy that is still held; reports the tuples that did not fit a game's harvest buffer (N_DROPPED)"""
        if self.closed:
            return
        self.closed = True
        store = self._store(agent)
        self._drain(store)
        if occupied:
            self._flush(self._head())        # the sweep gets the whole ring
            self._check(self.L.tm_nodes_sweep(C.byref(store.s), self._p(self.ring), self.ring_rows, self._p(self.counters),
                                              self._p(self.offsets), self._stream()), "tm_nodes_sweep")
        self._flush(int(self.counters[0].item()))
        for k in (self._flushes % 2, (self._flushes + 1) % 2):      # the older copy first: parts are in the order of the moves
            self._write(k)
        dropped = store.counter("N_DROPPED")
        report_loss(0, dropped - self._dropped_seen, self.ring_rows, self._replay_cap)
        self._dropped_seen = dropped


def load_rows(files):
    """the NODE_DTYPE rows of the shards one after the other; a shard of another layout (an episode shard) is a ValueError"""
    return _concat([np.load(f) for f in files], NODE_DTYPE)


class NodeLoader:
    """Node shards as one table: `rows`, `length`, and every column (obs, value, variance, visit, slot) a concatenated attribute.
    paths: node shards or stems."""

    def __init__(self, paths):
        self.files = _expand(paths)
        self.rows = load_rows(self.files)
        for c in NODE_DTYPE.names:
            setattr(self, c, np.ascontiguousarray(self.rows[c]))
        self.length = len(self.rows)


def node_targets_numpy(rows, wmode, eps):
    """The specification of tm_node_targets in numpy (include/tetris_mcts_hip.h): obs uint32 [n,12], value, variance, weight
    float32 [n] and the fault word (0 / 1).  rows: a NODE_DTYPE table."""
    if wmode not in (0, 1, 2, 3):
        raise ValueError("weight_mode: 0 .. 3, not %r" % (wmode,))
    value, variance, visit = (np.ascontiguousarray(rows[c]).astype(np.float32) for c in ("value", "variance", "visit"))
    weight = visit.copy() if wmode >= 2 else np.ones(len(rows), np.float32)
    if wmode in (1, 3):
        with np.errstate(all="ignore"):
            weight = (weight / (variance + np.float32(eps))).astype(np.float32)
    with np.errstate(invalid="ignore"):
        bad = ~np.isfinite(value) | ~np.isfinite(variance) | ~(visit >= np.float32(1))
    weight[bad] = 0
    return np.ascontiguousarray(rows["obs"]), value, variance, weight, int(bad.any())
