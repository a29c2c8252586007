"""k_vn_fc1's grid of work items (valuenet.hip: fc1_item_count / fc1_item_index / fc1_item): `requests` states make
ceil(requests / rows) tiles of `parts` parts; the items are numbered tiles fastest, so that a tile's parts start far apart and
on one XCD (item()); workgroup b of a grid of `grid` takes items b, b + grid, ...  Restated here in Python and held to what a dealing has to be:
every (tile, part) of the tiles that exist exactly once, nothing past the end, shares that differ by at most one item.  The
library's own arithmetic (tm_fc1_deal, the same inline functions the kernel and its launch call) is held to the restatement."""
import ctypes as C

import numpy as np

GRIDS = (1, 7, 255, 256, 512)
SINGLE_LEAF = (32, 4)        # rows, parts of k_vn_fc1<2, 4, 256, 6, 2>
LEAF_PARALLEL = (64, 4)      # k_vn_fc1<4, 4, 128, 3, 2>
LP_COUNTS = sorted(set([0, 1, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 7168, 7169, 7231, 7232, 7233, 8191, 8192, 8193, 9001,
                        16383, 16384, 16385, 28607, 28608, 28609, 28671, 28672] + list(range(0, 28673, 997))))


def item_count(requests, rows, parts):
    return (requests + rows - 1) // rows * parts if requests > 0 else 0


def deal(requests, rows, parts, grid, b):
    """the (tile, part) items of workgroup b"""
    n_items, out, k = item_count(requests, rows, parts), [], 0
    while b + k * grid < n_items:
        out.append(item(b + k * grid, requests, rows, parts))
        k += 1
    return out


def item(i, requests, rows, parts):
    """item i as (tile, part): tiles fastest over the whole multiples of eight tiles (a tile's parts a multiple of eight
    workgroups apart: one XCD), then the tiles left over, tiles fastest again"""
    tiles = (requests + rows - 1) // rows
    t8 = tiles // 8 * 8
    if i < t8 * parts:
        return i % t8, i // t8
    rest, j = tiles - t8, i - t8 * parts
    return t8 + j % rest, j // rest


def _check(requests, rows, parts, grid):
    tiles = (requests + rows - 1) // rows
    # all workgroups at once: item i belongs to workgroup i % grid, as its (i // grid)-th
    idx = np.arange(item_count(requests, rows, parts))
    t8 = tiles // 8 * 8
    rest, j = max(tiles - t8, 1), idx - t8 * parts
    bulk = idx < t8 * parts
    tile = np.where(bulk, idx % max(t8, 1), t8 + j % rest)
    part = np.where(bulk, idx // max(t8, 1), j // rest)
    assert ((tile >= 0) & (tile < tiles) & (part >= 0) & (part < parts)).all()          # no item past the end
    assert (tile * rows < requests).all()                                               # every tile taken has a state
    taken = np.zeros((tiles, parts), np.int64)
    np.add.at(taken, (tile, part), 1)
    assert (taken == 1).all(), (requests, grid)                                          # every (tile, part) exactly once
    share = np.bincount(idx % grid, minlength=grid)
    assert share.max() - share.min() <= 1, (requests, grid)
    return tile, part, share


def test_every_item_is_dealt_exactly_once_single_leaf_shape():
    rows, parts = SINGLE_LEAF
    for requests in range(0, 4097):
        for grid in GRIDS:
            _check(requests, rows, parts, grid)


def test_every_item_is_dealt_exactly_once_leaf_parallel_shape():
    rows, parts = LEAF_PARALLEL
    for requests in LP_COUNTS:
        for grid in GRIDS:
            _check(requests, rows, parts, grid)


def test_the_vectorised_check_is_the_per_workgroup_loop():
    """_check deals all workgroups at once; deal() is the kernel's loop, one workgroup at a time"""
    for (rows, parts), counts in ((SINGLE_LEAF, (0, 1, 32, 33, 1867, 4096)), (LEAF_PARALLEL, (64, 65, 7169, 28672))):
        for requests in counts:
            for grid in GRIDS:
                tile, part, share = _check(requests, rows, parts, grid)
                seen = set()
                for b in range(grid):
                    mine = deal(requests, rows, parts, grid, b)
                    assert len(mine) == share[b]
                    for k, tp in enumerate(mine):
                        assert tp == (int(tile[b + k * grid]), int(part[b + k * grid])) and tp not in seen
                        seen.add(tp)
                assert len(seen) == item_count(requests, rows, parts)


def test_a_tiles_parts_share_an_xcd_and_start_far_apart():
    """workgroups go to the eight XCDs round robin, and a tile's four parts read the same rows of activations: at the headline's
    1 867 requests (59 tiles) on 256 workgroups the parts of tiles 0..55 are 56 workgroups apart - the same XCD, not neighbours -
    and only the three tiles left over are dealt across XCDs; the leaf-parallel 7 169 requests (113 tiles) leave one tile over"""
    at = {}
    for b in range(256):
        for tp in deal(1867, 32, 4, 256, b):
            at[tp] = b
    assert len(at) == 236
    for t in range(56):
        assert [at[(t, p)] for p in range(4)] == [t, t + 56, t + 112, t + 168]
        assert len({at[(t, p)] % 8 for p in range(4)}) == 1
    for t in range(56, 59):
        assert [at[(t, p)] for p in range(4)] == [224 + (t - 56) + 3 * p for p in range(4)]
    at = {}
    for b in range(512):
        for tp in deal(7169, 64, 4, 512, b):
            at[tp] = b
    assert len(at) == 452
    assert sum(len({at[(t, p)] % 8 for p in range(4)}) == 1 for t in range(113)) == 112


def test_the_library_deals_as_restated():
    import __graft_entry__ as ge
    import os
    if not os.path.exists(ge.LIB):
        ge.build()
    from tetris_mcts_amd import _lib
    f = _lib.lib().tm_fc1_deal
    f.argtypes, f.restype = [C.c_int] * 5 + [C.c_void_p, C.c_int], C.c_int
    cap = 2048
    buf = np.zeros(2 * cap, np.int32)
    cases = [(SINGLE_LEAF, r) for r in (0, 1, 31, 32, 33, 1867, 2048, 4095, 4096)] + \
            [(LEAF_PARALLEL, r) for r in (8191, 8192, 8193, 9001, 28672)]
    for (rows, parts), requests in cases:
        for grid in GRIDS:
            for b in sorted(set((0, 1, grid // 2, grid - 1)) & set(range(grid))):
                want = deal(requests, rows, parts, grid, b)
                k = f(requests, rows, parts, grid, b, buf.ctypes.data, cap)
                assert k == len(want) <= cap, (requests, grid, b, k)
                assert [tuple(x) for x in buf[:2 * k].reshape(-1, 2).tolist()] == want, (requests, grid, b)
    assert f(10, 32, 4, 0, 0, None, 0) == -1 and f(10, 32, 4, 4, 4, None, 0) == -1 and f(-1, 32, 4, 4, 0, None, 0) == -1
    assert f(4096, 32, 4, 256, 5, None, 0) == 2          # counting only
