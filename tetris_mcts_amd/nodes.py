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

The distributional head has the same scheme with a row of its own (`DistNodeRecorder`, `DistNodeLoader`; tm_nodes_drain_dist):
what the collections of a DistValueSim harvest - the packed observation, the node's backed-up distribution and its visits, of
every freed node with at least `min_visits_to_store` visits whose seven children have all been visited - as NODE_DIST_DTYPE rows
of 320 bytes: the node row (value and variance are the zeros the harvest leaves) followed by the 64 floats of the distribution.
Beside the parts a stem has one sidecar, <stem>.head.npy: float64 [3] = atoms, vmin, vmax of the head that recorded them.
"""
import ctypes as C
import os
import sys

import numpy as np

from .episodes import _PART, _concat, _expand, _parts, _rank, _stem

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

DIST_ROW_BYTES = 320           # TM_NODE_DIST_ROW_BYTES
NODE_DIST_DTYPE = np.dtype({
    "names": ["obs", "value", "variance", "visit", "slot", "dist"],
    "formats": [("<u4", (12,)), "<f4", "<f4", "<f4", "<i4", ("<f4", (64,))],
    "offsets": [0, 48, 52, 56, 60, 64],
    "itemsize": DIST_ROW_BYTES})
# The default ring of the dist rows (2^22 rows: 1.25 GiB on the device and twice that pinned) is 1.74 times the largest flush
# measured at DistValueSim's benchmark batch, 4 096 games x 1 000 simulations with min_visit 50 over 200 moves (2 409 959 rows;
# 87 327 rows a move on average, most of them late, once the pools have filled; nothing lost: profiles/dist_node_records_timing.json,
# DESIGN 3.17).  The ring this started from, 2^20 rows, overflowed there (3.5 % of the rows lost, every large flush the whole ring).
# The margin is thinner than RING_ROWS' 6.0: a larger batch wants a larger ring (--nodes_ring_rows), and loss is reported.
DIST_RING_ROWS = 1 << 22


class NodeShardWriter:
    """The host half of the recorder: the numbered shards of a stem.  `write(rows)` writes the next part (nothing for no rows)."""
    DTYPE, DTYPE_NAME = NODE_DTYPE, "NODE_DTYPE"

    def __init__(self, save_dir, save_file, cycle, rank=None):
        self.stem = _stem(save_dir, save_file, cycle, rank)
        self.part = 1 + max([int(_PART.search(f).group(1)) for f in _parts(self.stem)], default=-1)

    def write(self, rows):
        if rows.dtype != self.DTYPE:
            raise ValueError("rows: a table of %s, not %s" % (self.DTYPE_NAME, rows.dtype))
        if not len(rows):
            return None
        name = "%s.part%05d.npy" % (self.stem, self.part)
        np.save(name, np.ascontiguousarray(rows))
        self.part += 1
        return name


def head_file(stem):
    """the sidecar of a stem of dist node shards"""
    return stem + ".head.npy"


def _head_array(atoms, vmin, vmax):
    head = np.array([float(int(atoms)), float(vmin), float(vmax)], np.float64)
    if not (1 <= int(atoms) <= 64 and np.isfinite(head).all() and head[1] < head[2]):
        raise ValueError("a head of 1 .. 64 atoms over [vmin, vmax) with two finite bounds, not %r, %r, %r" % (atoms, vmin, vmax))
    return head


def write_head(stem, atoms, vmin, vmax, goes="harvest goes"):
    """The sidecar of `stem`, <stem>.head.npy (float64 [3]: atoms, vmin, vmax): written if it is not there, a ValueError if one is
    there that says otherwise (goes: what another head's then does, in the message's words).  Returns its name and the array."""
    head, name = _head_array(atoms, vmin, vmax), head_file(stem)
    if os.path.exists(name):
        have = np.load(name)
        if have.dtype != np.float64 or have.shape != (3,) or have.tobytes() != head.tobytes():
            raise ValueError("%s records a head of (atoms, vmin, vmax) = %s, this run's is %s: another head's %s to another stem "
                             "(--save_dir or --cycle)" % (name, have.tolist(), head.tolist(), goes))
    else:
        d = os.path.dirname(name)
        if d:
            os.makedirs(d, exist_ok=True)
        np.save(name, head)
    return name, head


class DistNodeShardWriter(NodeShardWriter):
    """NodeShardWriter for NODE_DIST_DTYPE rows.  Creating it writes the stem's sidecar, <stem>.head.npy (float64 [3]: atoms, vmin,
    vmax); over a stem that has one already, a sidecar that differs is a ValueError: one stem holds the harvest of one head."""
    DTYPE, DTYPE_NAME = NODE_DIST_DTYPE, "NODE_DIST_DTYPE"

    def __init__(self, save_dir, save_file, cycle, atoms, vmin, vmax, rank=None):
        super().__init__(save_dir, save_file, cycle, rank)
        self.head = write_head(self.stem, atoms, vmin, vmax)[1]


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
    `agent`: a ValueSim, ValueSimLP or ValueSimC built with harvest=True.
    A subclass records another row through the same scheme: ROW and DTYPE, the drain (`_call_drain`), the writer (`_writer`)
    and what it asks of the store (`_check_store`)."""
    ROW, DTYPE = ROW_BYTES, NODE_DTYPE

    def _writer(self, save_dir, save_file, cycle, rank):
        return NodeShardWriter(save_dir, save_file, cycle, rank)

    def _call_drain(self, store):
        self._check(self.L.tm_nodes_drain(C.byref(store.s), self._p(self.ring), self.ring_rows, self._p(self.counters),
                                          self._p(self.offsets), self._stream()), "tm_nodes_drain")

    def _check_store(self, store):
        pass

    def __init__(self, save_dir, save_file, cycle, n_games, ring_rows=RING_ROWS, flush_moves=FLUSH_MOVES, device="cuda"):
        import torch
        from . import _lib
        if int(n_games) < 1 or int(ring_rows) < 1 or int(flush_moves) < 1:
            raise ValueError("n_games, ring_rows and flush_moves must be at least 1")
        self.L = _lib.lib()
        self.torch, self._check = torch, _lib.check
        self.cycle, self.G, self.ring_rows, self.flush_moves = int(cycle), int(n_games), int(ring_rows), int(flush_moves)
        self.device = torch.device(device)
        self.writer = self._writer(save_dir, save_file, cycle, _rank())
        dev = self.device
        self._ring_bytes = self.ring_rows * self.ROW
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
        self._check_store(store)
        self._replay_cap = int(store.s.replay_cap)
        return store

    def _head(self):
        """the ring's head as the last drain left it (nothing has drained since); the copy it reads was enqueued a move ago"""
        if self._seen_ev is None:
            return 0
        self._seen_ev.synchronize()
        return int(self._seen.numpy()[0])

    def _drain(self, store):
        self._call_drain(store)
        self._seen.copy_(self.counters, non_blocking=True)
        self._seen_ev = self.torch.cuda.Event()
        self._seen_ev.record()
        self._since += 1

    def drain(self, agent):
        """Move what the collections of the last move harvested into the ring: one tm_nodes_drain (or the subclass's drain)."""
        store = self._store(agent)
        head = self._head()
        if head and (2 * head >= self.ring_rows or self._since >= self.flush_moves):
            self._flush(head)
        self._drain(store)

    def _flush(self, head):
        k = self._flushes % 2
        self._write(k)                       # the buffer's earlier contents become a file first
        host, n = self._host[k], head * self.ROW
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
        name = self.writer.write(buf[:head * self.ROW].view(self.DTYPE))
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


class DistNodeRecorder(NodeRecorder):
    """NodeRecorder for the harvest of the distributional head: the same drain after every move, the same two-buffer pinned flush
    without waits, the same reports of loss, with rows of NODE_DIST_DTYPE moved by tm_nodes_drain_dist.  `agent`: a DistValueSim
    built with harvest=True whose atoms and range are the ones given here; they go into the stem's sidecar when the recorder is
    made (DistNodeShardWriter).  There is no sweep of the pools for this harvest (it is per node and needs the seven-children
    test over live nodes only): close(agent, occupied=True) raises."""
    ROW, DTYPE = DIST_ROW_BYTES, NODE_DIST_DTYPE

    def __init__(self, save_dir, save_file, cycle, n_games, atoms, vmin, vmax, ring_rows=DIST_RING_ROWS, flush_moves=FLUSH_MOVES,
                 device="cuda"):
        self.head = _head_array(atoms, vmin, vmax)
        super().__init__(save_dir, save_file, cycle, n_games, ring_rows=ring_rows, flush_moves=flush_moves, device=device)

    def _writer(self, save_dir, save_file, cycle, rank):
        return DistNodeShardWriter(save_dir, save_file, cycle, *self.head, rank=rank)

    def _call_drain(self, store):
        self._check(self.L.tm_nodes_drain_dist(C.byref(store.s), self._p(self.ring), self.ring_rows, self._p(self.counters),
                                               self._p(self.offsets), self._stream()), "tm_nodes_drain_dist")

    def _check_store(self, store):
        from .store import KIND_DIST
        if store.s.kind != KIND_DIST or store.t.get("replay_dist") is None:
            raise TypeError("DistNodeRecorder needs a DistValueSim built with harvest=True (a value net's harvest is NodeRecorder's)")
        have = (float(store.s.dist_bins), float(store.s.dist_vmin), float(store.s.dist_vmax))
        if have != tuple(self.head.tolist()):
            raise ValueError("the recorder was made for a head of (atoms, vmin, vmax) = %s, the agent's is %s"
                             % (self.head.tolist(), list(have)))

    def close(self, agent, occupied=False):
        if occupied:
            raise ValueError("occupied=True: there is no sweep of the pools for the distributional harvest (it is per node and "
                             "needs the seven-children test over live nodes only)")
        super().close(agent)


def load_rows(files, dtype=NODE_DTYPE):
    """the rows of the shards one after the other, NODE_DTYPE or the `dtype` given; a shard of another layout (an episode shard)
    is a ValueError"""
    return _concat([np.load(f) for f in files], dtype)


class NodeLoader:
    """Node shards as one table: `rows`, `length`, and every column (obs, value, variance, visit, slot) a concatenated attribute.
    paths: node shards or stems."""
    DTYPE = NODE_DTYPE

    def __init__(self, paths):
        self.files = _expand(paths)
        self.rows = load_rows(self.files, self.DTYPE)
        for c in self.DTYPE.names:
            setattr(self, c, np.ascontiguousarray(self.rows[c]))
        self.length = len(self.rows)


class DistNodeLoader(NodeLoader):
    """Dist node shards as one table: `rows`, `length`, every column (obs, value, variance, visit, slot, dist) a concatenated
    attribute, and `atoms`, `vmin`, `vmax` from the stems' sidecars.  paths: dist node shards or stems.  A shard of another layout
    and stems whose sidecars disagree (or a stem without one) are a ValueError."""
    DTYPE = NODE_DIST_DTYPE

    def __init__(self, paths):
        super().__init__(paths)
        self.atoms, self.vmin, self.vmax = load_head(dict.fromkeys(_PART.sub("", f) for f in self.files))


def load_head(stems):
    """(atoms, vmin, vmax) of the sidecars of `stems`, which must all say the same"""
    heads = {}
    for s in stems:
        name = head_file(s)
        if not os.path.exists(name):
            raise ValueError("%s is missing: the shards of %s do not say which head recorded them" % (name, s))
        h = np.load(name)
        if h.dtype != np.float64 or h.shape != (3,):
            raise ValueError("%s is not a sidecar of dist node shards (float64 [3]: atoms, vmin, vmax)" % name)
        heads[s] = h
    if not heads:
        raise ValueError("no dist node shards: nothing says which head recorded them")
    first = next(iter(heads.values()))
    for s, h in heads.items():
        if h.tobytes() != first.tobytes():
            raise ValueError("the sidecars disagree: %s has (atoms, vmin, vmax) = %s, %s has %s"
                             % (next(iter(heads)), first.tolist(), s, h.tolist()))
    _head_array(*first)
    return int(first[0]), float(first[1]), float(first[2])


def node_dist_targets_numpy(rows, atoms, wmode):
    """The specification of tm_node_dist_targets in numpy (include/tetris_mcts_hip.h): obs uint32 [n,12], target float32 [n,atoms]
    (the bits of the row's first `atoms` floats), weight float32 [n] and the fault word (0 / 1).  rows: a NODE_DIST_DTYPE table."""
    atoms = int(atoms)
    if not 1 <= atoms <= 64:
        raise ValueError("atoms: 1 .. 64, not %r" % (atoms,))
    if wmode not in (0, 2):
        raise ValueError("weight_mode: 0 (1) or 2 (visits), not %r: the row carries no variance to divide by" % (wmode,))
    dist, visit = np.ascontiguousarray(rows["dist"]), np.ascontiguousarray(rows["visit"]).astype(np.float32)
    p, rest = dist[:, :atoms], dist[:, atoms:]
    with np.errstate(invalid="ignore"):
        bad = ~np.isfinite(visit) | ~(visit >= np.float32(1))
        bad |= (~np.isfinite(p) | (p < 0)).any(1) | ~(p > 0).any(1) | (rest != 0).any(1)
    weight = visit.copy() if wmode == 2 else np.ones(len(rows), np.float32)
    weight[bad] = 0
    return np.ascontiguousarray(rows["obs"]), np.ascontiguousarray(p), weight, int(bad.any())


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
