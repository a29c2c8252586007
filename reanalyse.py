#!/usr/bin/env python
"""reanalyse.py — search the recorded moves of `play.py --save --save_positions` again under the current weights.

    python reanalyse.py --data_paths D/data3 D/data4 --out_dir R/ --agent_type ValueSimLP --mcts_sims 200 --n_games 4096

reads the State shards of the stems (or shards, or glob patterns) and the position shards beside them, loads the positions into an
environment in batches of --n_games, gives every game an empty tree, searches --mcts_sims simulations with the agent's ordinary
search under the model the agent builds and loads (pytorch_model/model_checkpoint, as play.py does), and writes R/data3.partNNNNN.npy
... with the rows, row counts and row order of the input: identity and the action played as recorded, value, variance, child_stats
and policy from the new search.  The .episodes tables are copied, so `train.py --td --data_paths R/data*` reads the result as it
reads a recording.  A re-analysed row is a function of its position, the agent kind, --mcts_sims, --max_nodes, the back end and the
weights, not of the slot, the batch, --n_games or the order of the input (tetris_mcts_amd/reanalyse.py).

    python reanalyse.py --data_paths D/data3 --out_dir R/ --agent_type DistValueSim --root_dists --mcts_sims 200

does the same for the moves of `play.py --agent_type DistValueSim --save --save_positions --save_root_dists`: the root-distribution
shards beside the data (D/rootdist3.partNNNNN.npy and their sidecar, which gives the agent its atoms and range) are paired with the
rows, and R/rootdist3.partNNNNN.npy and the sidecar are written beside R/data3..., so that `train.py --head dist --td --bootstrap
search --data_paths R/data*` reads the result as a recording.  The contract is claimed for the 368 + 272 bytes of such a row.

ValueSim, ValueSimLP and ValueSimC, and DistValueSim with --root_dists, on the hip back ends, one process.  Vanilla and VanillaC (no
net) are refused, and so is DistValueSim without --root_dists: a State row alone records no distribution.
"""
import argparse
import os
import sys


def build_parser():
    p = argparse.ArgumentParser()
    add = p.add_argument
    add('--data_paths', default=[], nargs='*', help='State shards, their stems or glob patterns (play.py --save --save_positions)')
    add('--out_dir', default=None, type=str, help='Directory of the re-analysed shards (not the input\'s)')
    add('--agent_type', default=None, type=str, help='ValueSim, ValueSimLP or ValueSimC; DistValueSim with --root_dists')
    add('--root_dists', default=False, action='store_true', help='DistValueSim: also read the root-distribution shards recorded '
        'beside the data (play.py --save_root_dists) and write the re-analysed ones and their sidecar beside the output')
    add('--mcts_sims', default=50, type=int, help='Simulations per position')
    add('--n_games', default=4096, type=int, help='Positions searched at a time')
    add('--max_nodes', default=0, type=int, help='Nodes per tree (0: 8 x mcts_sims + 1024, more than a tree that starts empty '
        'can grow to)')
    add('--valuenet_backend', default='hip', choices=('hip', 'hip_bf16x3'), help='Value net (DistValueSim: the distributional head): fp32 '
        'matrix cores or split-precision bf16')
    add('--last_nfiles', default=0, type=int, help='Only the stems written last, as train.py counts them (0: all)')
    add('--app', default=1, type=int, help='Actions-per-drop of the recording')
    add('--tetris_randomizer', default=0, type=int, help='Queue randomizer of the recording')
    add('--tetris_scoring', default=0, type=int, help='Scoring system of the recording')
    return p


AGENTS = ('ValueSim', 'ValueSimLP', 'ValueSimC')


def check(args):
    """the refusals, before torch, the HIP library or the environment is imported"""
    if args.agent_type in ('Vanilla', 'VanillaC'):
        sys.exit('re-analysis is not offered for %s: its leaves are rollouts, there is no net whose weights could have changed; '
                 'use ValueSim, ValueSimLP or ValueSimC' % args.agent_type)
    if args.agent_type == 'DistValueSim' and not args.root_dists:
        sys.exit('re-analysis of DistValueSim needs --root_dists: a State row alone records no distribution, so a re-searched row '
                 'would have nothing the distributional fit reads; record with play.py --save --save_positions --save_root_dists and '
                 'give --root_dists, or use ValueSim, ValueSimLP or ValueSimC')
    if args.root_dists and args.agent_type != 'DistValueSim':
        sys.exit('--root_dists re-analyses the root distributions of a distributional search: it needs --agent_type DistValueSim, '
                 'not %s (the trees of the other agents keep no distribution)' % args.agent_type)
    if args.agent_type not in AGENTS + ('DistValueSim',):
        sys.exit('--agent_type is required: ValueSim, ValueSimLP or ValueSimC')
    if not args.data_paths:
        sys.exit('--data_paths is required: the State shards of play.py --save --save_positions, their stems or glob patterns')
    if not args.out_dir:
        sys.exit('--out_dir is required: where the re-analysed shards go')
    if args.mcts_sims < 1 or args.n_games < 1 or args.max_nodes < 0:
        sys.exit('--mcts_sims and --n_games are at least 1, --max_nodes is positive (0: the default)')
    ws = os.environ.get('WORLD_SIZE', '1')
    if ws.isdigit() and int(ws) > 1:
        sys.exit('re-analysis runs in one process: WORLD_SIZE is %s (shards of ranked stems are read as any other stem)' % ws)
    # the files the run would read, by the package's own rules (numpy alone is imported: no torch, no HIP library, no device)
    from tetris_mcts_amd.episodes import positions_file, rootdist_file, rootdist_stem
    from tetris_mcts_amd.reanalyse import choose_inputs
    files = choose_inputs(args.data_paths, args.last_nfiles)
    if not files:
        sys.exit('--data_paths %s: no State shards there' % ' '.join(args.data_paths))
    for f in files:
        if os.path.abspath(os.path.dirname(f) or '.') == os.path.abspath(args.out_dir):
            sys.exit('--out_dir %s is the directory of %s: the re-analysed shards take the names of the recorded ones and would '
                     'replace them; give another directory' % (args.out_dir, f))
    for f in files:
        if not os.path.isfile(positions_file(f)):
            sys.exit('%s: there are no positions beside the data (no %s): record with play.py --save --save_positions'
                     % (f, positions_file(f)))
    args.head = None
    if args.root_dists:
        from tetris_mcts_amd.episodes import _PART
        from tetris_mcts_amd.nodes import load_head
        for f in files:
            if not os.path.isfile(rootdist_file(f)):
                sys.exit('%s: there are no root distributions beside the data (no %s): record with play.py --agent_type DistValueSim '
                         '--save --save_positions --save_root_dists' % (f, rootdist_file(f)))
        try:
            args.head = load_head(dict.fromkeys(rootdist_stem(_PART.sub('', f)) for f in files))
        except ValueError as e:
            sys.exit('--root_dists: %s' % e)


def main(argv=None):
    args = build_parser().parse_args(argv)
    check(args)
    from importlib import import_module
    import torch
    if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
        sys.exit('re-analysis runs in one process, not under torch.distributed with more than one rank')
    from pyTetris import Tetris
    from tetris_mcts_amd.reanalyse import default_max_nodes, reanalyse_files
    env_args = ((20, 10), args.app, args.tetris_scoring, args.tetris_randomizer)
    G = args.n_games
    game = Tetris(*env_args, seed=0, n_games=G)
    module = import_module('agents.' + args.agent_type)
    extra = {}
    if args.head is not None:              # the head that recorded the distributions: its atoms and range
        extra = dict(atoms=args.head[0], vmin=args.head[1], vmax=args.head[2])
    agent = getattr(module, args.agent_type)(sims=args.mcts_sims, env=Tetris, env_args=env_args, online=False, n_games=G,
                                             max_nodes=args.max_nodes or default_max_nodes(args.mcts_sims),
                                             valuenet_backend=args.valuenet_backend, **extra)
    try:
        written = reanalyse_files(args.data_paths, args.out_dir, agent, game, last_nfiles=args.last_nfiles, log=lambda m: print(m, flush=True))
    except ValueError as e:
        sys.exit('reanalyse: %s' % e)
    print('re-analysed %d shard(s) into %s' % (len(written), args.out_dir), flush=True)
    agent.close()


if __name__ == '__main__':
    main()
