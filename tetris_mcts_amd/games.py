"""Game snapshots: the games of a `Tetris` batch written to a file and loaded into another batch, so that the games alive when a
self-play run stops go on in the next run (under other weights) instead of starting from empty boards.

A game is its 64-byte packed record (ENGINE_SPEC.md section 2) and its four line statistics; the randomizer is a function of the
record's seed and piece count.  Trees are NOT carried: `agent.update_root(game)` builds a root from any game, a tree pool (100 000 x 128 bytes a
game) is five orders of magnitude larger than the game and its values are stale once the weights change.

The file is one uncompressed `.npz`, written through a temporary file and `os.replace` (a reader never sees half a file):
    meta        int32 [5]     format version, n_games, app, scoring, randomizer
    games       uint32 [G,16] the packed games
    line_stats  int32 [G,4]
    move        int32 [G]     the moves played so far in each slot's current episode (what the episode recorder numbers rows by)

The engine trusts a packed game (its piece and rotation index tables, a lock writes the rows under the piece), so loading checks
every game ON THE DEVICE (csrc/games_snapshot.hip: tm_env_load, the TM_GAME_BAD_* bits of include/tetris_mcts_hip.h) and copies
all of them into the environment or none.  `check_games_numpy` is the same rule as a numpy statement: what the kernel is held to.
"""
import ctypes as C
import os

import numpy as np

VERSION = 1
META_NAMES = ("version", "n_games", "app", "scoring", "randomizer")
BAD_PIECE, BAD_ROT, BAD_ROWS, BAD_PLACE, BAD_FIELDS, BAD_LINE_STATS = 1, 2, 4, 8, 16, 32        # TM_GAME_BAD_*
FAULT_NAMES = {BAD_PIECE: "piece > 6", BAD_ROT: "rot > 3", BAD_ROWS: "a row with bits beyond column 9 or a full row",
               BAD_PLACE: "the falling piece is not inside the well", BAD_FIELDS: "drop counter, flags, combo or piece count",
               BAD_LINE_STATS: "a negative line statistic"}

# ENGINE_SPEC.md section 3: the cells (col, row) of every orientation inside its 4x4 box
PIECE_CELLS = (
    (((0, 1), (1, 1), (2, 1), (3, 1)), ((2, 0), (2, 1), (2, 2), (2, 3)), ((0, 2), (1, 2), (2, 2), (3, 2)), ((1, 0), (1, 1), (1, 2), (1, 3))),
    (((1, 0), (2, 0), (1, 1), (2, 1)),) * 4,
    (((1, 0), (0, 1), (1, 1), (2, 1)), ((1, 0), (1, 1), (2, 1), (1, 2)), ((0, 1), (1, 1), (2, 1), (1, 2)), ((1, 0), (0, 1), (1, 1), (1, 2))),
    (((1, 0), (2, 0), (0, 1), (1, 1)), ((1, 0), (1, 1), (2, 1), (2, 2)), ((1, 1), (2, 1), (0, 2), (1, 2)), ((0, 0), (0, 1), (1, 1), (1, 2))),
    (((0, 0), (1, 0), (1, 1), (2, 1)), ((2, 0), (1, 1), (2, 1), (1, 2)), ((0, 1), (1, 1), (1, 2), (2, 2)), ((1, 0), (0, 1), (1, 1), (0, 2))),
    (((0, 0), (0, 1), (1, 1), (2, 1)), ((1, 0), (2, 0), (1, 1), (1, 2)), ((0, 1), (1, 1), (2, 1), (2, 2)), ((1, 0), (1, 1), (0, 2), (1, 2))),
    (((2, 0), (0, 1), (1, 1), (2, 1)), ((1, 0), (1, 1), (1, 2), (2, 2)), ((0, 1), (1, 1), (2, 1), (0, 2)), ((0, 0), (1, 0), (1, 1), (1, 2))),
)


def collides_numpy(rows, piece, rot, x, y):
    """The engine's collides() for one game: rows uint16 [20], a cell of PIECE_CELLS[piece][rot] at box origin (x, y) outside
    columns 0..9 or rows 0..19, or on a set bit of rows."""
    for c, r in PIECE_CELLS[piece][rot]:
        col, row = x + c, y + r
        if col < 0 or col > 9 or row < 0 or row > 19 or (int(rows[row]) >> col) & 1:
            return True
    return False


def unpack_fields(games):
    """the scalar fields of packed games [G,16] as a dict of int64 arrays (ENGINE_SPEC.md section 2)"""
    g = np.ascontiguousarray(games, dtype=np.uint32).reshape(-1, 16)
    a, b = g[:, 10].astype(np.int64), g[:, 11].astype(np.int64)
    s8 = lambda v: ((v & 0xFF) ^ 0x80) - 0x80  # noqa: E731
    return dict(rows=g[:, :10].copy().view(np.uint16).reshape(-1, 20).astype(np.int64),
                piece=a & 0xFF, rot=(a >> 8) & 0xFF, x=s8(a >> 16), y=s8(a >> 24),
                drop_ctr=b & 0xFF, flags=(b >> 8) & 0xFF, combo=(((b >> 16) & 0xFFFF) ^ 0x8000) - 0x8000,
                piece_count=g[:, 12].astype(np.int64), seed=g[:, 13].astype(np.int64),
                score=g[:, 14].view(np.int32).astype(np.int64), lines=g[:, 15].view(np.int32).astype(np.int64))


def check_games_numpy(games, line_stats, app):
    """The fault rule of tm_env_check as a numpy statement: int32 [G] of TM_GAME_BAD_* bits, 0 for a well-formed game.
    games: uint32 [G,16]; line_stats: int32 [G,4] or None; app: actions per drop."""
    f = unpack_fields(games)
    n = len(f["piece"])
    out = np.zeros(n, np.int32)
    out[f["piece"] > 6] |= BAD_PIECE
    out[f["rot"] > 3] |= BAD_ROT
    rows = f["rows"]
    out[((rows & ~0x3FF) != 0).any(axis=1) | (rows == 0x3FF).any(axis=1)] |= BAD_ROWS
    for g in range(n):
        piece, rot, x, y = (int(f[k][g]) for k in ("piece", "rot", "x", "y"))
        if f["flags"][g] & 1:
            place = (rot, x, y) != (0, 3, 0)
        else:
            place = x < -3 or x > 9 or y < -3 or y > 19
            if not place and piece <= 6 and rot <= 3:
                place = collides_numpy(rows[g], piece, rot, x, y)
        if place:
            out[g] |= BAD_PLACE
    out[(f["drop_ctr"] >= int(app)) | ((f["flags"] & ~3) != 0) | (f["combo"] < -1) | (f["piece_count"] == 0)] |= BAD_FIELDS
    if line_stats is not None:
        out[(np.asarray(line_stats).reshape(n, 4) < 0).any(axis=1)] |= BAD_LINE_STATS
    return out


def describe_fault(bits):
    return "; ".join(name for bit, name in FAULT_NAMES.items() if int(bits) & bit)


def _ranked(path):
    """`.r<rank>` on the path under torch.distributed with more than one rank, as ShardWriter names its stems"""
    from .episodes import _rank
    rank = _rank()
    return str(path) if rank is None else "%s.r%d" % (path, rank)


def _meta(game):
    return np.array([VERSION, game.n_games, game.env_args[1], game.env_args[2], game.env_args[3]], np.int32)


def write_snapshot(path, meta, games, line_stats, move):
    """the file from host arrays: a temporary file beside `path`, then os.replace"""
    path = str(path)
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    tmp = "%s.tmp%d" % (path, os.getpid())
    try:
        with open(tmp, "wb") as fh:
            np.savez(fh, meta=np.asarray(meta, np.int32), games=np.asarray(games, np.uint32),
                     line_stats=np.asarray(line_stats, np.int32), move=np.asarray(move, np.int32))
            fh.flush()
            os.fsync(fh.fileno())
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return path


def read_snapshot(path, game):
    """(games, line_stats, move) of a file made for an environment like `game` (its n_games and env_args are all that is read):
    ValueError, naming the file and what differs, for anything else.  Touches no device."""
    path = str(path)
    try:
        with np.load(path, allow_pickle=False) as z:
            missing = [k for k in ("meta", "games", "line_stats", "move") if k not in z.files]
            if missing:
                raise ValueError("no array %s" % ", ".join(missing))
            meta, games, line_stats, move = z["meta"], z["games"], z["line_stats"], z["move"]
    except FileNotFoundError:
        raise
    except ValueError as e:
        raise ValueError("%s is not a game snapshot: %s" % (path, e)) from None
    except Exception as e:          # a truncated or foreign file: zipfile.BadZipFile, EOFError, OSError, ...
        raise ValueError("%s is not a game snapshot (truncated or not an .npz): %s: %s" % (path, type(e).__name__, e)) from None
    if meta.dtype != np.int32 or meta.shape != (len(META_NAMES),):
        raise ValueError("%s: meta is %s %s, not int32 (%d,)" % (path, meta.dtype, meta.shape, len(META_NAMES)))
    want = _meta(game)
    if int(meta[0]) != VERSION:
        raise ValueError("%s: format version %d, this package reads version %d" % (path, int(meta[0]), VERSION))
    for name, have, need in zip(META_NAMES[1:], meta[1:].tolist(), want[1:].tolist()):
        if have != need:
            raise ValueError("%s: %s is %d in the file, %d in this environment" % (path, name, have, need))
    G = int(want[1])
    for name, arr, dtype, shape in (("games", games, np.uint32, (G, 16)), ("line_stats", line_stats, np.int32, (G, 4)),
                                    ("move", move, np.int32, (G,))):
        if arr.dtype != dtype:
            raise ValueError("%s: %s has dtype %s, not %s" % (path, name, arr.dtype, np.dtype(dtype)))
        if arr.shape != shape:
            raise ValueError("%s: %s has shape %s, not %s" % (path, name, arr.shape, shape))
    return games, line_stats, move


def save_games(path, game, moves):
    """Write the games of `game` (a pyTetris.Tetris) and `moves`, int [G]: the moves played so far in each slot's episode."""
    import torch
    from . import _lib
    from .store import _p, _stream
    moves = np.asarray(moves).reshape(-1)
    if moves.shape != (game.n_games,):
        raise ValueError("moves: %d entries for %d games" % (moves.size, game.n_games))
    games = torch.empty(game.n_games, 16, dtype=torch.int32, device=game.device)
    ls = torch.empty(game.n_games, 4, dtype=torch.int32, device=game.device)
    _lib.check(game.L.tm_env_save(C.byref(game.s), _p(games), _p(ls), _stream()), "tm_env_save")
    return write_snapshot(_ranked(path), _meta(game), games.cpu().numpy().view(np.uint32), ls.cpu().numpy(), moves.astype(np.int32))


def load_games(path, game):
    """Load a snapshot into `game`; returns its `move` array (int32 [G]).  Every game is checked on the device before any enters
    the environment: on a fault nothing is loaded and a ValueError names the first bad slot and its fault bits.  Games stored as
    ended are reset (game.reset('ended')) and get move 0."""
    import torch
    from . import _lib
    from .store import _p, _stream
    path = _ranked(path)
    games, line_stats, move = read_snapshot(path, game)
    dev = game.device
    d_games = torch.from_numpy(np.ascontiguousarray(games).view(np.int32)).to(dev)
    d_ls = torch.from_numpy(np.ascontiguousarray(line_stats)).to(dev)
    report = torch.zeros(game.n_games + 1, dtype=torch.int32, device=dev)           # fault [G], then n_bad
    _lib.check(game.L.tm_env_load(C.byref(game.s), _p(d_games), _p(d_ls), _p(report),
                                  C.c_void_p(report.data_ptr() + 4 * game.n_games), _stream()), "tm_env_load")
    host = report.cpu().numpy()                                                    # the one read-back
    fault, n_bad = host[:-1], int(host[-1])
    if n_bad:
        first = int(np.nonzero(fault)[0][0])
        raise ValueError("%s: %d of %d games are not well-formed, nothing was loaded; the first is slot %d with fault bits %d (%s)"
                         % (path, n_bad, game.n_games, first, int(fault[first]), describe_fault(fault[first])))
    game._host = None
    move = np.maximum(move, 0).astype(np.int32)
    ended = ((games[:, 11] >> 8) & 1) != 0
    if ended.any():
        game.reset("ended")
        move[ended] = 0
    return move
