#!/usr/bin/env python
"""Complete-episode statistics of recorded self-play (tetris_mcts_amd/episodes.py): one JSON line.

    python scripts/episode_stats.py data/data0            (a stem: every part of it; or the state shards themselves)

`finished`: the episodes that ended inside the recording, from the episode table - their FINAL lines and score.
`under_way_at_the_end`: the episodes that had not ended when the recording stopped, from the last State row of each - their
lines SO FAR.  They are censored, not short: in a run of fixed length the episodes that end are the ones that die early, so a
mean over the finished episodes alone is biased low, the more the shorter the run.  The line says so in `censoring`.
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _summary(x):
    x = np.asarray(x, np.float64)
    if not len(x):
        return dict(mean=None, median=None, max=None)
    return dict(mean=float(x.mean()), median=float(np.median(x)), max=int(x.max()))


def stats(files):
    from tetris_mcts_amd.episodes import EpisodeLoader
    d = EpisodeLoader(files, by_episode=True)
    ep = d.episodes
    ended = set(zip(ep["cycle"].tolist(), ep["episode"].tolist()))
    # rows are sorted by (cycle, episode, move): the last row of a run of equal (cycle, episode) is the episode's last move
    key = np.stack([d.cycle, d.episode], axis=1) if d.length else np.zeros((0, 2), np.int32)
    last = np.nonzero(np.append((key[1:] != key[:-1]).any(axis=1), True))[0] if d.length else np.zeros(0, np.int64)
    open_rows = [i for i in last.tolist() if (int(d.cycle[i]), int(d.episode[i])) not in ended]
    lines_so_far = [int(d.lines[i]) for i in open_rows]
    # an episode whose first recorded move is above 0 went on from an earlier run's games (play.py --games_in): its rows here are
    # its later part, its row in the episode table counts ALL its moves and carries its final score and lines
    first = np.nonzero(np.append(True, (key[1:] != key[:-1]).any(axis=1)))[0] if d.length else np.zeros(0, np.int64)
    continued = [i for i in first.tolist() if int(d.move[i]) > 0]
    out = {
        "files": len(d.files), "state_rows": int(d.length),
        "finished": dict(count=int(len(ep)), lines=_summary(ep["lines"]), score=_summary(ep["score"]),
                         moves=_summary(ep["moves"])),
        "under_way_at_the_end": dict(count=len(open_rows), lines_so_far=_summary(lines_so_far),
                                     moves_so_far=_summary([int(d.move[i]) + 1 for i in open_rows])),
        "censoring": "finished covers only the episodes that ended inside the recording; the %d under way at the end are censored "
                     "(lines so far, before their last recorded action), and a mean over finished episodes only is biased low in a "
                     "fixed-length run" % len(open_rows),
    }
    if continued:
        n_fin = sum((int(d.cycle[i]), int(d.episode[i])) in ended for i in continued)
        out["continued"] = dict(count=len(continued), finished=n_fin, moves_before=_summary([int(d.move[i]) for i in continued]),
                                note="%d episodes were continued from an earlier run (their first recorded move is above 0); the %d "
                                     "of them that finished are in `finished` with totals that are complete: all their moves, final "
                                     "score and lines" % (len(continued), n_fin))
    return out


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if not argv:
        sys.exit(__doc__)
    print(json.dumps(stats(argv)))


if __name__ == "__main__":
    main()
