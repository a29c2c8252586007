#!/usr/bin/env python
"""play.py — self-play driver with the command line of the reference's play.py (flags: play.py:46-70), running
on the MI355X engine.  `python play.py --agent_type ValueSimLP --mcts_sims 500 --ngames 10` behaves like the
reference (same per-game log lines, play.py:25-37,164); `--n_games N` plays N games concurrently on the GPU
(new, optional).  `--save` writes the reference's self-play rows (util/Data.py State), recorded on the device, as numbered
.npy shards (tetris_mcts_amd/episodes.py; the container is numpy's, not HDF5); `--save_positions` adds the packed game of every
row, which reanalyse.py searches again under other weights; `--save_root_dists` adds, for DistValueSim, the distribution the search
backed up into the root (what `train.py --head dist --td --bootstrap search` fits).  `--save_nodes` writes the tree nodes the
collections harvest (tetris_mcts_amd/nodes.py), the training set of `train.py --nodes`; `--save_dist_nodes` does so for
DistValueSim, whose harvest carries a distribution per node (`train.py --dist_nodes`).  `--games_out` / `--games_in` carry the
games of the batch from one run to the next (tetris_mcts_amd/games.py).  --save_tree, --gui and --interactive belong to
the reference's storage / UI layers and are refused with a clear message.
"""
import argparse
import sys

import numpy as np


def games_every_moves(text):
    """the value of --games_every: a number of moves, at least 1 (the default, 0, is not a value one can give)"""
    k = int(text)
    if k < 1:
        sys.exit('--games_every %s: it is a number of moves, at least 1 (leave the flag out to write only at the end)' % text)
    return k


def build_parser():
    p = argparse.ArgumentParser()
    add = p.add_argument
    add('--agent_type', default=None, type=str, help='Which agent to use')
    add('--app', default=1, type=int, help='Actions-per-drop')
    add('--benchmark', default=False, help='Benchmark mode for agent', action='store_true')
    add('--cycle', default=0, type=int, help='Number of cycle')
    add('--endless', default=False, help='Endless plays', action='store_true')
    add('--gamma', default=0.9, type=float, help='Discount factor')
    add('--gui', default=False, help='A simple GUI', action='store_true')
    add('--interactive', default=False, help='Text interactive interface', action='store_true')
    add('--mcts_const', default=5.0, type=float, help='PUCT constant')
    add('--mcts_sims', default=50, type=int, help='Number of MCTS sims')
    add('--mcts_tau', default=1.0, type=float, help='Temperature constant')
    add('--min_visit', default=40, type=int, help='Minimum visits for node storage')
    add('--ngames', default=50, type=int, help='Number of episodes to play')
    add('--online', default=False, help='Online agent training', action='store_true')
    add('--printboard', default=False, help='Print board', action='store_true')
    add('--print_board_to_file', default=False, help='Print board to file', action='store_true')
    add('--realtime_status', default=False, help='Save realtime game status through numpy memmap', action='store_true')
    add('--save', default=False, help='Save self-play episodes', action='store_true')
    add('--save_dir', default='./data/', type=str, help='Directory for save')
    add('--save_file', default='data', type=str, help='Filename to save')
    add('--save_tree', default=False, help='Save expanded tree nodes', action='store_true')
    add('--tetris_randomizer', default=0, type=int, help='Queue randomizer used by Tetris (0: bag, 1: uniform)')
    add('--tetris_scoring', default=0, type=int, help='Scoring system used by Tetris (0: official guideline, 1: line clears)')
    # extensions (not in the reference)
    add('--n_games', default=1, type=int, help='[new] concurrent games on the GPU')
    add('--seed', default=0, type=int, help='[new] environment seed (game g uses seed+g); it does not touch games loaded with '
        '--games_in: each of them carries its own seed')
    add('--max_moves', default=0, type=int, help='[new] stop after this many moves (0 = no limit)')
    add('--train_every', default=0, type=int, help='[new] online mode: look for harvested tuples every k moves (0: every move '
        'with one game - the reference trains at every collection, ValueSim.py:101-120 - every 10 moves with more)')
    add('--train_min_tuples', default=0, type=int, help='[new] online mode: fit only once this many fresh tuples are held over '
        'all ranks (0: 1 with one game, 1024 = one training batch with more)')
    add('--valuenet_backend', default='hip', choices=('hip', 'hip_bf16x3', 'torch'), help='[new] value net of ValueSim, '
        'ValueSimLP and ValueSimC, distributional head of DistValueSim: hip (fp32 matrix cores), hip_bf16x3 (split-precision '
        'bf16 matrix cores) or torch')
    add('--valuenet_fc1', default='fp32', choices=('fp32', 'bf16x3'), help='[new] fc1 of the value net of ValueSim, ValueSimLP and '
        'ValueSimC under --valuenet_backend hip_bf16x3: fp32 (the fp32 matrix pipe) or bf16x3 (split-precision as the '
        'convolutions; for the leaf-parallel kinds)')
    add('--fit_backend', default='torch', choices=('torch', 'hip', 'hip_dist'), help='[new] online mode: gradients of the fits '
        'through PyTorch autograd (torch) or the hand-written gfx950 forward / loss / backward kernels: hip for the value net '
        'of ValueSim, ValueSimLP and ValueSimC, hip_dist for the distributional head of DistValueSim')
    add('--validation_backend', default='torch', choices=('torch', 'hip'), help='[new] online mode: validation of the fits through '
        'PyTorch (torch) or the forward of the same gfx950 kernels (hip: needs --fit_backend hip or hip_dist)')
    add('--fit_states', default='dense', choices=('dense', 'packed'), help='[new] online mode: what the fits are fed - the harvested '
        'observations rendered to float boards (dense) or the 48-byte packed observations themselves, read by the gfx950 kernels '
        '(packed: needs --fit_backend hip or hip_dist and --validation_backend hip)')
    add('--dense_requests', default=False, action='store_true', help='[new] with --valuenet_backend torch: hand the evaluator the '
        'posted leaf requests as a dense batch instead of every slot of every game')
    add('--evaluator_pure', default=False, action='store_true', help='[new] with --valuenet_backend torch: the evaluator is a '
        'function of the state and the weights alone, so the search posts only the requests its backup will use (ValueSim and '
        'ValueSimC without leaf parallelism: together with --dense_requests)')
    add('--save_nodes', default=False, action='store_true', help='[new] write the tree nodes the collections harvest - packed '
        'observation, value, variance, visits of every freed observation with at least --min_visit visits - as <save_dir>nodes<cycle> '
        '(ValueSim, ValueSimLP, ValueSimC; tetris_mcts_amd/nodes.py), what train.py --nodes fits')
    add('--save_nodes_occupied', default=False, action='store_true', help='[new] with --save_nodes: at the end of the run also '
        'write the observations still in the trees that pass the same test (the reference\'s save_occupied)')
    add('--save_dist_nodes', default=False, action='store_true', help='[new] DistValueSim: write the tree nodes its collections '
        'harvest - packed observation, the node\'s backed-up distribution, visits of every freed node with at least --min_visit '
        'visits whose seven children have all been visited - as <save_dir>distnodes<cycle> with a sidecar of the head\'s atoms and '
        'range (tetris_mcts_amd/nodes.py), what train.py --dist_nodes fits')
    add('--nodes_ring_rows', default=0, type=int, help='[new] with --save_nodes / --save_dist_nodes: rows of the recorder\'s ring on '
        'the device, 64 / 320 bytes each and twice that in pinned host memory (0: the default, tetris_mcts_amd/nodes.py RING_ROWS / '
        'DIST_RING_ROWS); it should hold twice the rows one move can harvest')
    add('--nodes_flush_moves', default=0, type=int, help='[new] with --save_nodes / --save_dist_nodes: copy the ring to the host at '
        'least every this many moves when it holds rows (0: the default, FLUSH_MOVES)')
    add('--games_out', default=None, type=str, help='[new] at the end of the run write the games as they stand - the packed games, '
        'their line statistics and each slot\'s move count (tetris_mcts_amd/games.py) - to this file, for a later --games_in; a game '
        'that has just ended is stored ended')
    add('--games_in', default=None, type=str, help='[new] go on with the games of this file (written by --games_out with the same '
        '--n_games, --app, --tetris_scoring and --tetris_randomizer) instead of new ones; every game is checked on the device before '
        'any is loaded; --seed does not touch loaded games, each carries its seed; trees are not carried, the agent builds new roots')
    add('--save_positions', default=False, action='store_true', help='[new] with --save: beside every row also write the packed game '
        'it was recorded from, as <save_dir>positions<cycle> (tetris_mcts_amd/episodes.py POSITION_DTYPE): what reanalyse.py '
        'searches again under other weights')
    add('--save_root_dists', default=False, action='store_true', help='[new] DistValueSim with --save: beside every row also write '
        'the distribution the search backed up into the root, as <save_dir>rootdist<cycle> with a sidecar of the head\'s atoms and '
        'range (tetris_mcts_amd/episodes.py ROOT_DIST_DTYPE): what train.py --head dist --td --bootstrap search fits and '
        'reanalyse.py --agent_type DistValueSim --root_dists makes again under other weights')
    add('--games_every', default=0, type=games_every_moves, help='[new] with --games_out: also write the file every this many moves (0: only at '
        'the end)')
    return p


def check_games(args):
    """the refusals of --games_in / --games_out / --games_every, before anything is imported"""
    import os
    if args.games_every and not args.games_out:
        sys.exit('--games_every says how often --games_out is written: it needs --games_out')
    if args.games_in is not None and not os.path.isfile(args.games_in):
        sys.exit('--games_in %s: there is no such file (a first run of a cycle starts without --games_in)' % args.games_in)


def check_save_nodes(args):
    """the refusals of --save_nodes, before anything is imported"""
    if args.save_nodes_occupied and not args.save_nodes:
        sys.exit('--save_nodes_occupied adds the trees\' remaining observations to what --save_nodes writes: it needs --save_nodes')
    if not args.save_nodes:
        return
    if not args.agent_type:
        sys.exit('--save_nodes records what an agent\'s collections harvest: it needs --agent_type (ValueSim, ValueSimLP, ValueSimC)')
    if args.agent_type in ('Vanilla', 'VanillaC'):
        sys.exit('--save_nodes is not offered for %s: the harvest of the rollout kinds is untested (no test checks their '
                 'tuples); use ValueSim, ValueSimLP or ValueSimC' % args.agent_type)
    if args.agent_type == 'DistValueSim':
        sys.exit('--save_nodes is not offered for DistValueSim: its harvest is of another row shape (a distribution per node, '
                 'tm_store.replay_dist), which the 64-byte node row does not hold; use ValueSim, ValueSimLP or ValueSimC, or record '
                 'DistValueSim\'s harvest in rows of its own with --save_dist_nodes')
    if args.agent_type not in ('ValueSim', 'ValueSimLP', 'ValueSimC'):
        sys.exit('--save_nodes applies to ValueSim, ValueSimLP and ValueSimC only')
    if args.online:
        sys.exit('--save_nodes together with --online: the online fit drains the same harvest buffers the recorder drains; '
                 'record with --save_nodes and fit with train.py --nodes, or fit with --online')
    if args.valuenet_backend == 'torch' and args.dense_requests:
        sys.exit('--save_nodes with --valuenet_backend torch --dense_requests has not been shown to work: record with the hip '
                 'back ends or without --dense_requests')
    if args.nodes_ring_rows < 0 or args.nodes_flush_moves < 0:
        sys.exit('--nodes_ring_rows and --nodes_flush_moves are positive (0: the defaults)')
    if args.min_visit < 1:
        sys.exit('--min_visit is at least 1 with --save_nodes (an observation without a visit has no statistics)')


def check_save_dist_nodes(args):
    """the refusals of --save_dist_nodes, before anything is imported"""
    if not args.save_dist_nodes:
        return
    if args.agent_type != 'DistValueSim':
        sys.exit('--save_dist_nodes records the harvest of the distributional head: it needs --agent_type DistValueSim, not %s '
                 '(--save_nodes records the harvest of ValueSim, ValueSimLP and ValueSimC)' % args.agent_type)
    if args.save_nodes:
        sys.exit('--save_dist_nodes together with --save_nodes: --save_nodes is not offered for DistValueSim, give --save_dist_nodes alone')
    if args.online:
        sys.exit('--save_dist_nodes together with --online: the online fit drains the same harvest buffers the recorder drains; '
                 'record with --save_dist_nodes and fit with train.py --dist_nodes, or fit with --online')
    if args.save_nodes_occupied:
        sys.exit('--save_dist_nodes takes no --save_nodes_occupied: there is no sweep of the pools for the distributional harvest '
                 '(it is per node and needs the seven-children test over live nodes only)')
    if args.valuenet_backend == 'torch' and args.dense_requests:
        sys.exit('--save_dist_nodes with --valuenet_backend torch --dense_requests has not been shown to work: record with the hip '
                 'back ends or without --dense_requests')
    if args.nodes_ring_rows < 0 or args.nodes_flush_moves < 0:
        sys.exit('--nodes_ring_rows and --nodes_flush_moves are positive (0: the defaults)')
    if args.min_visit < 1:
        sys.exit('--min_visit is at least 1 with --save_dist_nodes (a node without a visit has no distribution)')


def check_save_root_dists(args):
    """the refusals of --save_root_dists, before anything is imported"""
    if not args.save_root_dists:
        return
    if not args.save:
        sys.exit('--save_root_dists writes the root\'s distribution beside every row that --save writes: it needs --save')
    if args.agent_type != 'DistValueSim':
        sys.exit('--save_root_dists records the distribution a distributional search backs up into its root: it needs --agent_type '
                 'DistValueSim, not %s (the trees of the other agents keep a value and a variance, which --save records already)'
                 % args.agent_type)
    if args.valuenet_backend == 'torch' and args.dense_requests:
        sys.exit('--save_root_dists with --valuenet_backend torch --dense_requests has not been shown to work: record with the hip '
                 'back ends or without --dense_requests')


class Scoreboard:
    """Running min/max/mean/std of finished episodes, printed like the reference's ScoreTracker (play.py:25-37)."""

    def __init__(self):
        self.scores, self.lines = [], []

    def add(self, score, line):
        self.scores.append(score)
        self.lines.append(line)

    def show(self):
        s, l = np.asarray(self.scores, float), np.asarray(self.lines, float)
        print('\rGames played:{:>3}    min/max/mean/std:{:5.2f}({:5.2f})/{:5.2f}({:5.2f})/{:5.2f}({:5.2f})/{:5.2f}({:5.2f})'
              .format(len(s), s.min(), l.min(), s.max(), l.max(), s.mean(), l.mean(), s.std(), l.std()), end='', flush=True)


def main(argv=None):
    args = build_parser().parse_args(argv)
    for flag in ('save_tree', 'gui', 'interactive'):
        if getattr(args, flag):
            sys.exit('--%s is part of the reference\'s storage / UI layer (util/Data.py: PyTables / HDF5 files of expanded tree '
                     'nodes; util/gui.py), which this engine does not reimplement' % flag)
    if args.save and not args.agent_type:
        sys.exit('--save records what an agent plays (its root statistics, value and policy beside the board): it needs '
                 '--agent_type (ValueSim, ValueSimLP, ValueSimC, Vanilla, VanillaC, DistValueSim)')
    if args.save_positions and not args.save:
        sys.exit('--save_positions writes the game beside every row that --save writes: it needs --save')
    check_save_root_dists(args)
    check_save_dist_nodes(args)
    check_save_nodes(args)
    check_games(args)
    if not args.agent_type:
        sys.exit('--agent_type is required (ValueSim, ValueSimLP, ValueSimC, Vanilla, VanillaC, DistValueSim)')
    if args.fit_backend == 'hip_dist' and args.agent_type != 'DistValueSim':
        sys.exit('--fit_backend hip_dist applies to DistValueSim only')
    if args.validation_backend == 'hip' and args.fit_backend == 'torch':
        sys.exit('--validation_backend hip reads the parameters of a HIP fit: it needs --fit_backend hip or hip_dist')
    if args.fit_states == 'packed' and not (args.fit_backend != 'torch' and args.validation_backend == 'hip'):
        sys.exit('--fit_states packed is read by the HIP fit and the HIP validation: it needs --fit_backend hip or hip_dist and '
                 '--validation_backend hip')
    if args.valuenet_fc1 != 'fp32':
        if args.agent_type not in ('ValueSim', 'ValueSimLP', 'ValueSimC'):
            sys.exit('--valuenet_fc1 applies to ValueSim, ValueSimLP and ValueSimC only (the distributional head has no such option)')
        if args.valuenet_backend != 'hip_bf16x3':
            sys.exit('--valuenet_fc1 bf16x3 needs --valuenet_backend hip_bf16x3')
    for flag in ('dense_requests', 'evaluator_pure'):
        if getattr(args, flag) and not (args.agent_type in ('ValueSim', 'ValueSimLP', 'ValueSimC', 'DistValueSim')
                                        and args.valuenet_backend == 'torch'):
            sys.exit('--%s applies to the search loop that runs in Python: ValueSim, ValueSimLP, ValueSimC and DistValueSim under '
                     '--valuenet_backend torch (the native loop of the hip back ends asks only for what it needs already)' % flag)
    if args.evaluator_pure and not args.dense_requests and args.agent_type == 'ValueSim':
        sys.exit('--evaluator_pure needs --dense_requests with ValueSim (a leaf answered from the per-observation cache keeps its slot)')
    from importlib import import_module
    from pyTetris import Tetris                       # the reference's own two import lines (play.py:1,81-82)
    _agent_module = import_module('agents.' + args.agent_type)

    env_args = ((20, 10), args.app, args.tetris_scoring, args.tetris_randomizer)
    G = args.n_games
    game = Tetris(*env_args, seed=args.seed, n_games=G)
    extra = {}
    if args.agent_type in ('ValueSim', 'ValueSimLP', 'ValueSimC', 'DistValueSim'):
        extra['valuenet_backend'] = args.valuenet_backend
    elif args.valuenet_backend != 'hip':
        sys.exit('--valuenet_backend applies to ValueSim, ValueSimLP, ValueSimC and DistValueSim only')
    if args.valuenet_fc1 != 'fp32':
        extra['valuenet_fc1'] = args.valuenet_fc1
    if args.agent_type in ('ValueSim', 'ValueSimLP', 'ValueSimC', 'DistValueSim'):
        extra['fit_backend'] = args.fit_backend      # (DistValueSim refuses 'hip' itself)
        extra['validation_backend'] = args.validation_backend
        if args.fit_states != 'dense':
            extra['fit_states'] = args.fit_states
    elif args.fit_backend != 'torch':
        sys.exit('--fit_backend applies to ValueSim, ValueSimLP, ValueSimC and DistValueSim only')
    if args.dense_requests:
        extra['dense_requests'] = True
    if args.evaluator_pure:
        extra['evaluator_pure'] = True
    if args.save_nodes:
        # the store harvests without a fit; --min_visit is the harvest's threshold (ValueSimC takes it as min_visit already)
        extra['harvest'] = True
        if args.agent_type != 'ValueSimC':
            extra['min_visits_to_store'] = args.min_visit
    if args.save_dist_nodes:
        extra['harvest'] = True
        extra['min_visits_to_store'] = args.min_visit
    agent = getattr(_agent_module, args.agent_type)(sims=args.mcts_sims, env=Tetris, env_args=env_args, benchmark=args.benchmark,
                                             online=args.online, min_visit=args.min_visit, n_games=G, **extra)
    slot_moves = np.zeros(G, np.int32)        # the moves played so far in each slot's episode
    if args.games_in is not None:
        try:
            slot_moves = game.load_games(args.games_in)
        except ValueError as e:
            sys.exit('--games_in: %s' % e)
    agent.update_root(game)
    rec = None
    if args.save:
        from tetris_mcts_amd.episodes import EpisodeRecorder
        rec = EpisodeRecorder(args.save_dir, args.save_file, args.cycle, G)
        if args.save_positions:
            rec.record_positions()
        if args.save_root_dists:
            try:
                rec.record_root_dists(agent.atoms, *agent.vrange)
            except ValueError as e:
                sys.exit('--save_root_dists: %s' % e)
        if args.games_in is not None:
            rec.resume(slot_moves)
    node_rec = None
    if args.save_nodes:
        from tetris_mcts_amd.nodes import NodeRecorder
        from tetris_mcts_amd.nodes import FLUSH_MOVES, RING_ROWS
        node_rec = NodeRecorder(args.save_dir, 'nodes', args.cycle, G, ring_rows=args.nodes_ring_rows or RING_ROWS,
                                flush_moves=args.nodes_flush_moves or FLUSH_MOVES)
    if args.save_dist_nodes:
        from tetris_mcts_amd.nodes import DIST_RING_ROWS, FLUSH_MOVES, DistNodeRecorder
        node_rec = DistNodeRecorder(args.save_dir, 'distnodes', args.cycle, G, agent.atoms, *agent.vrange,
                                    ring_rows=args.nodes_ring_rows or DIST_RING_ROWS, flush_moves=args.nodes_flush_moves or FLUSH_MOVES)

    board_file = open('board_output', 'wb') if args.print_board_to_file else None
    if args.realtime_status:
        mm = {k: np.memmap('./tmp/' + k, dtype=d, mode='w+', shape=s) for k, d, s in (
            ('board', np.int8, (20, 10)), ('combo', np.int32, (1,)), ('score', np.int32, (1,)), ('lines', np.int32, (1,)),
            ('line_stats', np.int32, (4,)))}
    board = Scoreboard()
    finished, moves = 0, 0
    while True:
        if args.printboard:
            game.printState()
        action = agent.play()
        if rec is not None:
            rec.add(agent, game)
        if board_file is not None or args.realtime_status:
            st = game.getState().reshape(-1, 20, 10)[0]
            if board_file is not None:
                board_file.truncate(0)
                board_file.seek(0)
                board_file.write(st.tobytes())
                board_file.flush()
            if args.realtime_status:
                mm['board'][:] = st
                mm['combo'][:] = np.atleast_1d(game.combo)[0]
                mm['lines'][:] = np.atleast_1d(game.line_clears)[0]
                mm['score'][:] = np.atleast_1d(game.score)[0]
                mm['line_stats'][:] = np.asarray(game.line_stats).reshape(-1, 4)[0]
        game.play(action)
        if rec is not None:
            rec.advance(game)
        agent.update_root(game)
        moves += 1
        if args.online and not args.benchmark and hasattr(agent, 'train_if_collected'):
            # the reference trains inside remove_nodes(), i.e. at every collection (ValueSim.py:101-120); the batched engine
            # harvests on the device during the move and fits here, right after a move in which a collection harvested
            # (a batch of games collects somewhere on nearly every move: it looks every few moves and waits for a batch's worth)
            agent.train_if_collected(every=args.train_every or (1 if G == 1 else 10),
                                     min_tuples=args.train_min_tuples or (1 if G == 1 else 1024))
        ended = np.atleast_1d(game.end)
        slot_moves += 1
        slot_moves[ended] = 0
        if ended.any():
            scores, lines = np.atleast_1d(game.score), np.atleast_1d(game.line_clears)
            for g in np.nonzero(ended)[0]:
                finished += 1
                if args.endless:
                    print('Episode: {:>5} Score: {:>10} Lines Cleared: {:>10}'.format(finished, int(scores[g]), int(lines[g])),
                          flush=True)
                else:
                    board.add(int(scores[g]), int(lines[g]))
            if not args.endless:
                board.show()
                if finished >= args.ngames:
                    break
            game.reset('ended')
            agent.update_root(game)
        if node_rec is not None:
            node_rec.drain(agent)       # between two moves: what this move's collections harvested goes into the ring
        if args.games_every and moves % args.games_every == 0:
            game.save_games(args.games_out, slot_moves)
        if args.max_moves and moves >= args.max_moves:
            break
    print(flush=True)
    if rec is not None:
        rec.close()
    if args.games_out:
        print('games written to %s' % game.save_games(args.games_out, slot_moves), flush=True)
    if node_rec is not None:
        node_rec.close(agent, occupied=args.save_nodes_occupied)
        print('node rows written: %d in %d file(s), %d lost' % (node_rec.rows_written, len(node_rec.files), node_rec.lost),
              flush=True)
    agent.close()


if __name__ == '__main__':
    main()
