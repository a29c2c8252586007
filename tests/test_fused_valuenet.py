"""k_vn_conv_fc1's hand-off arithmetic (valuenet_fused.inc), host side only: the count a tile's poller waits for
(tm_fused_tile_rows), who waits for which tile (tm_fc1_deal over the fused kernel's grid), and the order of a workgroup's own
work - all its convolution positions before its first item - under which no workgroup can wait for itself or for a workgroup
that waits."""
import ctypes as C

import pytest

from tetris_mcts_amd import _lib

ROWS, PARTS, WAVES = 32, 4, 8
COUNTS = (0, 1, 31, 32, 33, 2047, 2048, 2049, 4096)
GRIDS = (1, 8, 256)


def rows_of(requests, tile):
    return _lib.lib().tm_fused_tile_rows(requests, tile)


def deal(requests, grid, b):
    f = _lib.lib().tm_fc1_deal
    buf = (C.c_int32 * (2 * 64))()
    k = f(requests, ROWS, PARTS, grid, b, buf, 64)
    if k > 64:
        buf = (C.c_int32 * (2 * k))()
        assert f(requests, ROWS, PARTS, grid, b, buf, k) == k
    return [(buf[2 * i], buf[2 * i + 1]) for i in range(k)]


@pytest.mark.parametrize("requests", COUNTS)
def test_tile_rows_sum_to_the_requests(requests):
    tiles = (requests + ROWS - 1) // ROWS
    rows = [rows_of(requests, t) for t in range(tiles)]
    assert sum(rows) == requests
    assert all(r == ROWS for r in rows[:-1])
    assert not rows or 1 <= rows[-1] <= ROWS
    assert rows_of(requests, tiles) == 0 and rows_of(requests, tiles + 5) == 0
    assert rows_of(-1, 0) == -1 and rows_of(requests, -1) == -1


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("requests", COUNTS)
def test_every_tile_part_is_waited_for_once(requests, grid):
    tiles = (requests + ROWS - 1) // ROWS
    seen = {}
    for b in range(grid):
        for item in deal(requests, grid, b):
            assert item not in seen, (item, b, seen[item])
            seen[item] = b
    assert set(seen) == {(t, p) for t in range(tiles) for p in range(PARTS)}


def programme(requests, grid, b):
    """workgroup b's operations in program order: every wave's convolution positions (phase 1), then one wait per item (phase 2)"""
    conv = [p for w in range(WAVES) for p in range(b * WAVES + w, requests, grid * WAVES)]
    return [("conv", p) for p in conv] + [("wait", t) for t, _ in deal(requests, grid, b)]


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("requests", COUNTS)
def test_no_workgroup_waits_for_itself(requests, grid):
    progs = [programme(requests, grid, b) for b in range(grid)]
    # every position is convolved exactly once
    assert sorted(p for pr in progs for op, p in pr if op == "conv") == list(range(requests))
    for b, pr in enumerate(progs):
        first_wait = next((i for i, (op, _) in enumerate(pr) if op == "wait"), len(pr))
        assert all(op == "conv" for op, _ in pr[:first_wait]) and all(op == "wait" for op, _ in pr[first_wait:]), b
    # the worst schedule: one workgroup at a time, each run as far as it gets before the next one starts, the last one first.
    # Every wait finds its tile complete after one pass over the convolutions, which never wait.
    ready, at = {}, [0] * grid
    for sweep in range(2):
        for b in reversed(range(grid)):
            pr = progs[b]
            while at[b] < len(pr):
                op, x = pr[at[b]]
                if op == "conv":
                    ready[x // ROWS] = ready.get(x // ROWS, 0) + 1
                elif ready.get(x, 0) != rows_of(requests, x):
                    break
                at[b] += 1
        if sweep == 0:      # after the first sweep no convolution is left anywhere
            assert all(op == "wait" for b in range(grid) for op, _ in progs[b][at[b]:])
    assert all(at[b] == len(progs[b]) for b in range(grid))
    assert all(ready.get(t, 0) == rows_of(requests, t) for t in range((requests + ROWS - 1) // ROWS))
