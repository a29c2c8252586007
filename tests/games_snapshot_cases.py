"""Hand-made packed games and fault injections shared by tests/test_games_snapshot.py (no GPU) and
tests/test_gpu_games_snapshot.py: every class of the TM_GAME_BAD_* rule (include/tetris_mcts_hip.h) and combinations."""
import types

import numpy as np

PIECE, ROT, ROWS, PLACE, FIELDS, LINE_STATS = 1, 2, 4, 8, 16, 32


def fake_env(n_games, app=1, scoring=0, randomizer=0):
    """what games.read_snapshot reads of an environment"""
    return types.SimpleNamespace(n_games=n_games, env_args=((20, 10), app, scoring, randomizer))


def make_game(rows=None, piece=0, rot=0, x=3, y=0, drop_ctr=0, flags=0, combo=-1, piece_count=1, seed=7, score=0, lines=0):
    """one packed game (ENGINE_SPEC.md section 2) as uint32 [16]"""
    g = np.zeros(16, np.uint32)
    r = np.zeros(20, np.uint16) if rows is None else np.asarray(rows, np.uint16)
    g[:10] = r.view(np.uint32)
    g[10] = (piece & 0xFF) | ((rot & 0xFF) << 8) | ((x & 0xFF) << 16) | ((y & 0xFF) << 24)
    g[11] = (drop_ctr & 0xFF) | ((flags & 0xFF) << 8) | ((combo & 0xFFFF) << 16)
    g[12], g[13], g[14], g[15] = piece_count, seed, score & 0xFFFFFFFF, lines & 0xFFFFFFFF
    return g


def set_piece(g, piece=None, rot=None, x=None, y=None):
    a = int(g[10])
    f = [a & 0xFF, (a >> 8) & 0xFF, (a >> 16) & 0xFF, (a >> 24) & 0xFF]
    for i, v in enumerate((piece, rot, x, y)):
        if v is not None:
            f[i] = v & 0xFF
    g[10] = f[0] | (f[1] << 8) | (f[2] << 16) | (f[3] << 24)


def set_fields(g, drop_ctr=None, flags=None, combo=None):
    b = int(g[11])
    f = [b & 0xFF, (b >> 8) & 0xFF, (b >> 16) & 0xFFFF]
    for i, (v, m) in enumerate(((drop_ctr, 0xFF), (flags, 0xFF), (combo, 0xFFFF))):
        if v is not None:
            f[i] = v & m
    g[11] = f[0] | (f[1] << 8) | (f[2] << 16)


def _row(g, r, value):
    g[:10].view(np.uint16)[r] = value


# (name, edit(game, line_stats), the bits that MUST be among the game's faults).  The edits are applied to LIVE well-formed games.
INJECTIONS = [
    ("piece 7", lambda g, ls: set_piece(g, piece=7), PIECE),
    ("rot 4", lambda g, ls: set_piece(g, rot=4), ROT),
    ("a bit at column 10", lambda g, ls: _row(g, 19, int(g[:10].view(np.uint16)[19]) | 0x400), ROWS),
    ("a bit at column 15", lambda g, ls: _row(g, 0, 0x8000), ROWS),
    ("a full row", lambda g, ls: _row(g, 19, 0x3FF), ROWS),
    ("below the floor", lambda g, ls: set_piece(g, y=19), PLACE),
    ("far below", lambda g, ls: set_piece(g, y=127), PLACE),
    ("far above", lambda g, ls: set_piece(g, y=-128), PLACE),
    ("left of the wall", lambda g, ls: set_piece(g, x=-4), PLACE),
    ("x = -128", lambda g, ls: set_piece(g, x=-128), PLACE),
    ("right of the wall", lambda g, ls: set_piece(g, x=9), PLACE),
    ("x = 127", lambda g, ls: set_piece(g, x=127), PLACE),
    ("drop counter at app", lambda g, ls: set_fields(g, drop_ctr=200), FIELDS),
    ("flag bit 2", lambda g, ls: set_fields(g, flags=4), FIELDS),
    ("flag bit 7", lambda g, ls: set_fields(g, flags=0x80), FIELDS),
    ("combo -2", lambda g, ls: set_fields(g, combo=-2), FIELDS),
    ("piece count 0", lambda g, ls: g.__setitem__(12, 0), FIELDS),
    ("negative line statistic", lambda g, ls: ls.__setitem__(2, -1), LINE_STATS),
    ("ended, but not at the spawn place", lambda g, ls: (set_fields(g, flags=1), set_piece(g, rot=0, x=3, y=5)), PLACE),
    ("ended with rot 1", lambda g, ls: (set_fields(g, flags=1), set_piece(g, rot=1, x=3, y=0)), PLACE),
    # combinations: the placement must not be looked up through the mask table
    ("piece 255 and y 127", lambda g, ls: set_piece(g, piece=255, y=127), PIECE | PLACE),
    ("piece 255, rot 255, x -128, y -128", lambda g, ls: set_piece(g, piece=255, rot=255, x=-128, y=-128), PIECE | ROT | PLACE),
    ("piece 200 inside the box range", lambda g, ls: set_piece(g, piece=200, x=3, y=0), PIECE),
    ("rot 77 and a full row", lambda g, ls: (set_piece(g, rot=77), _row(g, 10, 0x3FF)), ROT | ROWS),
    ("everything", lambda g, ls: (set_piece(g, piece=9, rot=9, x=100, y=100), _row(g, 3, 0xFFFF), set_fields(g, drop_ctr=255, flags=0xFE, combo=-300),
                                  ls.__setitem__(0, -5)), PIECE | ROT | ROWS | PLACE | FIELDS | LINE_STATS),
]


def inject(games, line_stats, slots):
    """copies of (games, line_stats) with INJECTIONS[k] applied to game slots[k] (live games); returns (games, line_stats,
    {slot: (name, bits)})"""
    games, line_stats = np.array(games, np.uint32), np.array(line_stats, np.int32)
    assert len(slots) >= len(INJECTIONS) and len(set(slots)) == len(slots), "a live game of its own for every injection"
    where = {}
    for (name, edit, bits), g in zip(INJECTIONS, slots):
        assert not (int(games[g, 11]) >> 8) & 1, "the injections are written for live games"
        edit(games[g], line_stats[g])
        where[int(g)] = (name, bits)
    return games, line_stats, where
