#!/usr/bin/env python
"""train.py — the offline fit with the command line of the reference's train.py (flags: train.py:15-39), on the MI355X engine:
the middle of cycle.sh's loop.  `play.py --save` writes a cycle's episodes, this fits the value net to them
(tetris_mcts_amd/offline.py: targets on the device from the rows as recorded, csrc/episode_targets.hip) and writes
pytorch_model/model_checkpoint, which the next play.py loads.

The reference's script does not run as committed (`backend`, `eligibility_trace` and `eligibility_trace_lambda` are undefined and
it reads row 3 of a 3-row child_stats), so what is kept is its intent: its flags, its file choice, its three target rules, its
validation split and its iteration count.  `--td_lambda` stands for its eligibility trace: without it `--td` fits the recorded
root values, with it the lambda-return.  --save_loss is refused with a message.

--ewc --ewc_lambda L is elastic weight consolidation (the reference sketches it: model_vv.py:170-208, train.py:321-322): the fit is
penalised by 0.5 L sum F (p - p*)^2 against the Fisher diagonal F and the weights p* that the loaded checkpoint carries (none on the
first cycle, or with --new: nothing is penalised), and after the fit the Fisher of the fitted net over the training rows is computed
by the HIP Fisher pass (csrc/valuenet_fit.hip: tm_valuenet_fit_fisher) and written into pytorch_model/model_checkpoint with the
weights as the next cycle's anchor.  --ewc_lambda has no default: the Fisher's magnitude follows the loss's scale, and the
reference's default of 1 never met a Fisher that was not zero.  The value net only, with --fit_backend hip.

--ewc_dist --ewc_lambda L is the same for the distributional head: with --head dist (--bootstrap search included) and with
--dist_nodes the fit is penalised against the Fisher and anchor that pytorch_model/model_checkpoint_dist carries, and after the fit
the head's Fisher over the training rows (csrc/distnet_fit.hip: tm_distnet_fit_fisher) is written into it with the weights.  It
needs --fit_backend hip; --ewc stays the value net's flag and is refused with --head dist and --dist_nodes.

Beyond the reference: --target_gamma discounts the targets per move (0.999 is the search's discount; the default 1.0 is the
reference's undiscounted rule), and --bootstrap net takes the values inside the lambda-return from the net being fitted, refreshed
before each of --bootstrap_rounds parts of the fit, instead of the values the playing net recorded.

--head dist fits the distributional head of DistValueSim instead (offline.fit_episodes_dist: categorical targets over --atoms
atoms on [--vmin, --vmax), csrc/episode_dist_targets.hip) and writes pytorch_model/model_checkpoint_dist, which a DistValueSim
that builds its own model loads.  Without --td the target is the realised return as a distribution; --td --td_lambda L
--bootstrap net is the lambda-return of the head's own distributions over at most --td_horizon moves, refreshed before each of
--bootstrap_rounds parts.  --fit_backend hip then means the head's gradient step (hip_dist).  A State row records no distribution
and the head's backup has no discount, so --td alone, --bootstrap recorded with --td and a --target_gamma other than 1 are refused.

--head dist --td [--td_lambda L] --bootstrap search takes the distributions inside the target from the `rootdist` shards beside the
data (`play.py --agent_type DistValueSim --save --save_root_dists`, or `reanalyse.py --agent_type DistValueSim --root_dists`): what
the SEARCH backed up into each move's root, not the bare head's opinion.  Without --td_lambda the target is the recorded
distribution itself (lambda = 0, the counterpart of the value net's --td alone).  Atoms and range come from the shards' sidecar; an
--atoms, --vmin or --vmax that says otherwise is refused.  Nothing is predicted, so it takes no --bootstrap_rounds above 1; it is
refused with --head value, --nodes and --dist_nodes and without --td.

--nodes --td --data_paths D/nodes* fits the node shards of `play.py --save_nodes` instead of episodes (offline.fit_nodes,
csrc/node_records.hip): the harvested tree nodes, the training set of the online fit.  A node has the search's value and
variance and no return, so --nodes needs --td and takes no --td_lambda, --bootstrap net, --target_gamma, --val_mode 1, --head
dist or --fit_backend torch; --weighted, --validation, --early_stopping, --last_nfiles and --ewc keep their meaning.

--dist_nodes --data_paths D/distnodes* fits the distributional head to the dist node shards of `play.py --agent_type DistValueSim
--save_dist_nodes` (offline.fit_dist_nodes): the target of a node is the distribution the search backed up into it, as recorded, so
nothing is bootstrapped from the head's own predictions.  Atoms and range come from the shards' sidecar; an --atoms, --vmin or
--vmax that says otherwise is refused.  It writes pytorch_model/model_checkpoint_dist.  It takes no --nodes, --td_lambda,
--bootstrap net, --target_gamma, --val_mode 1, --ewc (its consolidation is --ewc_dist) or --fit_backend torch, and --weighted only
with --weighted_mode 1 (visits).
"""
import argparse
import sys


def build_parser():
    p = argparse.ArgumentParser()
    add = p.add_argument
    add('--batch_size', default=32, type=int, help='Batch size (default:32)')
    add('--cycle', default=-1, type=int, help='Cycle (default:-1)')
    add('--data_paths', default=[], nargs='*', help='Training data paths (default: empty list)')
    add('--early_stopping', default=False, help='Use early stopping', action='store_true')
    add('--early_stopping_patience', default=10, type=int, help='Early stopping patience (default:10)')
    add('--epochs', default=10, type=int, help='Training epochs (default:10)')
    add('--ewc', default=False, help='Elastic weight consolidation (default:False)', action='store_true')
    add('--ewc_lambda', default=None, type=float, help='Elastic weight consolidation lambda (no default: give it with --ewc)')
    add('--ewc_dist', default=False, action='store_true', help='[new] --head dist / --dist_nodes: elastic weight consolidation of the '
        'distributional head, with --ewc_lambda (the head\'s Fisher and anchor travel in pytorch_model/model_checkpoint_dist)')
    add('--last_nfiles', default=1, type=int, help='Use last n files in training only (default:1, -1 for all)')
    add('--min_iters', default=-1, type=int, help='Min training iterations (default:-1, negative for unlimited)')
    add('--max_iters', default=-1, type=int, help='Max training iterations (default:-1, negative for unlimited)')
    add('--new', default=False, help='Create a new model instead of training the old one', action='store_true')
    add('--validation', default=False, help='Validation set (default:False)', action='store_true')
    add('--val_episodes', default=0, type=float, help='Number of validation episodes (default:0)')
    add('--val_mode', default=0, type=int, help='Validation mode (0: random, 1:episodic, default:0)')
    add('--val_set_size', default=0.05, type=float, help='Validation set size (fraction of total) (default:0.05)')
    add('--val_set_size_max', default=-1, type=int, help='Maximum validation set size (default:-1, negative for unlimited)')
    add('--val_total', default=25, type=int, help='Total number of validations (default:25)')
    add('--save_loss', default=False, help='Save loss history', action='store_true')
    add('--td', default=False, help='Temporal difference update', action='store_true')
    add('--weighted', default=False, help='Weighted loss', action='store_true')
    add('--weighted_mode', default=0, type=int, help='0: inverse of variance, 1: number of visits, 2: both')
    # extensions (not in the reference)
    add('--td_lambda', default=None, type=float, help='[new] with --td: fit the lambda-return along the moves played (the '
        'reference\'s eligibility trace), lambda in [0, 1]; without it --td fits the recorded root values')
    add('--terminal', default='final', choices=('final', 'rows'), help='[new] final: an episode that ended ends with its FINAL '
        'score from the episode table (value 0); rows: the reference\'s rule, the last recorded row is the end')
    add('--censored', default='drop', choices=('drop', 'keep'), help='[new] without --td: the episodes the run cut off are left '
        'out (drop) or end at their last row (keep, the reference\'s rule)')
    add('--target_gamma', default=1.0, type=float, help='[new] the discount per move of the targets, in (0, 1]: 0.999 is the '
        'search\'s discount (the value it adds to discounted score differences); default 1.0, the reference\'s undiscounted rule')
    add('--bootstrap', default='recorded', choices=('recorded', 'net', 'search'), help='[new] with --td --td_lambda: the values inside '
        'the lambda-return are the recorded root values (recorded) or the fitted net\'s own, refreshed every round (net); --head dist '
        'with --td: search takes the root distributions recorded beside the rows (play.py --save_root_dists, reanalyse.py '
        '--root_dists), and without --td_lambda fits them as they are')
    add('--bootstrap_rounds', default=1, type=int, help='[new] with --bootstrap net: the iterations are split into this many '
        'parts and the targets recomputed from the net before each (default:1)')
    add('--fit_backend', default='hip', choices=('torch', 'hip'), help='[new] gradients through PyTorch autograd (torch) or the '
        'hand-written gfx950 forward / loss / backward kernels (hip)')
    add('--validation_backend', default=None, choices=('torch', 'hip'), help='[new] validation through PyTorch (torch) or the '
        'forward of the same gfx950 kernels (hip: needs --fit_backend hip); default: as --fit_backend')
    add('--head', default='value', choices=('value', 'dist'), help='[new] the net that is fitted: the value net (value) or the '
        'distributional head of DistValueSim (dist: categorical targets, pytorch_model/model_checkpoint_dist)')
    add('--atoms', default=50, type=int, help='[new] --head dist: the atoms of the head, 1 .. 64 (default:50)')
    add('--vmin', default=0.0, type=float, help='[new] --head dist: the lower end of the atoms\' range (default:0)')
    add('--vmax', default=5000.0, type=float, help='[new] --head dist: the upper end of the atoms\' range (default:5000)')
    add('--td_horizon', default=64, type=int, help='[new] --head dist with --td: the moves after a row that its target takes in '
        'at most (default:64)')
    add('--nodes', default=False, action='store_true', help='[new] --data_paths are the node shards of play.py --save_nodes (the '
        'harvested tree nodes, e.g. data/self1/nodes*): fit the search\'s value and variance of every node from its packed '
        'observation; needs --td')
    add('--dist_nodes', default=False, action='store_true', help='[new] --data_paths are the dist node shards of play.py '
        '--agent_type DistValueSim --save_dist_nodes (e.g. data/self1/distnodes*): fit the distributional head to the recorded '
        'distribution of every node from its packed observation; atoms and range come from the shards\' sidecar')
    return p


def _given(argv, flag):
    """whether the command line names `flag` itself (`--flag value` or `--flag=value`)"""
    return any(a == flag or a.startswith(flag + '=') for a in argv)


def check_dist_nodes(args, argv):
    """the refusals of --dist_nodes that need no file"""
    if args.nodes:
        sys.exit('--dist_nodes together with --nodes: --nodes fits the value net to 64-byte node rows, --dist_nodes the '
                 'distributional head to rows with a distribution; give one of the two')
    if args.td_lambda is not None:
        sys.exit('--dist_nodes takes no --td_lambda: a node table has no moves to trace along')
    if args.bootstrap != 'recorded':
        sys.exit('--dist_nodes takes no --bootstrap net: the target is the recorded distribution, nothing is bootstrapped')
    if args.target_gamma != 1.0:
        sys.exit('--dist_nodes takes no --target_gamma other than 1: the distributional backup does not discount')
    if args.val_mode == 1:
        sys.exit('--dist_nodes takes no --val_mode 1: a node table has no episodes (--val_mode 0 holds out random rows)')
    if args.ewc:
        sys.exit('--dist_nodes takes no --ewc: the Fisher pass exists for the value net only behind that flag (the distributional '
                 'head\'s consolidation is --ewc_dist)')
    if args.fit_backend != 'hip':
        sys.exit('--dist_nodes takes no --fit_backend torch: the packed observations are read by the HIP gradient step alone')
    if args.validation and args.validation_backend not in (None, 'hip'):
        sys.exit('--dist_nodes with --validation needs --validation_backend hip: the torch validation does not read packed '
                 'observations')
    if args.weighted and args.weighted_mode != 1:
        sys.exit('--dist_nodes with --weighted needs --weighted_mode 1 (number of visits), not %d: a dist node row records no '
                 'variance' % args.weighted_mode)
    args.head_given = {k: getattr(args, k) for k in ('atoms', 'vmin', 'vmax') if _given(argv, '--' + k)}


def check_search(args, argv):
    """the refusals of --bootstrap search that need no file"""
    if args.head != 'dist':
        sys.exit('--bootstrap search takes the root distributions recorded beside the rows: it needs --head dist (the value net\'s '
                 'recorded values are --bootstrap recorded)')
    if args.nodes or args.dist_nodes:
        sys.exit('--bootstrap search takes no --nodes or --dist_nodes: it reads the episodes\' rows and the root distributions beside '
                 'them, a node table has neither')
    if not args.td:
        sys.exit('--bootstrap search puts the recorded root distributions inside the target of --td: it needs --td (with '
                 '--td_lambda L the lambda-return over them, without it the recorded distribution itself)')
    if args.bootstrap_rounds > 1:
        sys.exit('--bootstrap search takes no --bootstrap_rounds above 1: recorded distributions do not change between rounds')
    args.head_given = {k: getattr(args, k) for k in ('atoms', 'vmin', 'vmax') if _given(argv, '--' + k)}


def check_nodes(args):
    """the refusals of --nodes"""
    if not args.td:
        sys.exit('--nodes needs --td: a node has no return, only the search\'s value')
    if args.td_lambda is not None:
        sys.exit('--nodes takes no --td_lambda: a node table has no moves to trace along')
    if args.bootstrap != 'recorded':
        sys.exit('--nodes takes no --bootstrap net: there is no lambda-return whose values the net could refresh')
    if args.target_gamma != 1.0:
        sys.exit('--nodes takes no --target_gamma other than 1: the search discounted the node\'s value already')
    if args.val_mode == 1:
        sys.exit('--nodes takes no --val_mode 1: a node table has no episodes (--val_mode 0 holds out random rows)')
    if args.head == 'dist':
        sys.exit('--nodes takes no --head dist: a node row holds a value and a variance, not a distribution (the distributional '
                 'head\'s harvest, play.py --save_dist_nodes, is fitted with --dist_nodes)')
    if args.fit_backend != 'hip':
        sys.exit('--nodes takes no --fit_backend torch: the packed observations are read by the HIP gradient step alone')
    if args.validation and args.validation_backend not in (None, 'hip'):
        sys.exit('--nodes with --validation needs --validation_backend hip: the torch validation does not read packed observations')


def check_args(args, argv=()):
    """the refusals, before anything is imported or read"""
    if args.bootstrap == 'search':
        check_search(args, argv)
    if args.dist_nodes:
        check_dist_nodes(args, argv)
    if args.nodes:
        check_nodes(args)
    if args.ewc and args.head == 'dist':
        sys.exit('--ewc: the Fisher pass exists for the value net only (--head value) behind this flag, not for --head dist: the '
                 'distributional head\'s consolidation is --ewc_dist')
    if args.ewc_dist and not (args.head == 'dist' or args.dist_nodes):
        sys.exit('--ewc_dist consolidates the distributional head: it needs --head dist or --dist_nodes (the value net\'s flag is '
                 '--ewc)')
    if args.ewc_dist and args.ewc_lambda is None:
        sys.exit('--ewc_dist needs --ewc_lambda: there is no default, because the magnitude of the Fisher follows the scale of the '
                 'loss, as for --ewc')
    if args.ewc and args.ewc_lambda is None:
        sys.exit('--ewc needs --ewc_lambda: there is no default, because the magnitude of the Fisher follows the scale of the loss, '
                 'and the reference\'s default of 1 never met a Fisher that was not zero')
    if args.ewc_lambda is not None and not (args.ewc or args.ewc_dist):
        sys.exit('--ewc_lambda is the weight of --ewc: it needs --ewc')
    if args.ewc_lambda is not None and not (args.ewc_lambda >= 0.0 and args.ewc_lambda != float('inf')):
        sys.exit('--ewc_lambda is finite and at least 0')
    if args.ewc and args.fit_backend != 'hip':
        sys.exit('--ewc adds its penalty to the gradient of the HIP fit and computes its Fisher with the HIP kernels: it needs '
                 '--fit_backend hip')
    if args.ewc_dist and args.fit_backend != 'hip':
        sys.exit('--ewc_dist adds its penalty to the gradient of the head\'s HIP fit and computes its Fisher with the HIP kernels: it '
                 'needs --fit_backend hip')
    if args.save_loss:
        sys.exit('--save_loss writes the reference\'s HDF5 loss table (util/Data.py LossSaver: PyTables), which this engine does '
                 'not reimplement; the fit logs its losses to stderr')
    if args.td_lambda is not None and not args.td:
        sys.exit('--td_lambda is the trace of --td: it needs --td')
    if args.head == 'dist':
        if args.td and args.td_lambda is None and not args.dist_nodes and args.bootstrap != 'search':
            sys.exit('--head dist with --td needs --td_lambda: the rows record no distribution to fit (the root distributions of '
                     'play.py --save_root_dists are fitted with --bootstrap search)')
        if args.td and args.bootstrap not in ('net', 'search') and not args.dist_nodes:
            sys.exit('--head dist with --td needs --bootstrap net (the distributions inside the target are the head\'s own) or '
                     '--bootstrap search (they are the recorded root distributions of play.py --save_root_dists)')
        if args.target_gamma != 1.0:
            sys.exit('--head dist takes no --target_gamma other than 1: the distributional backup does not discount')
        if args.td_horizon < 0:
            sys.exit('--td_horizon is at least 0')
        if not 1 <= args.atoms <= 64:
            sys.exit('--atoms is in 1 .. 64')
        if not args.vmin < args.vmax:
            sys.exit('--vmin is below --vmax')
    if args.td_lambda is not None and not 0.0 <= args.td_lambda <= 1.0:
        sys.exit('--td_lambda is in [0, 1]')
    if not 0.0 < args.target_gamma <= 1.0:
        sys.exit('--target_gamma is in (0, 1]')
    if args.bootstrap == 'net' and not (args.td and args.td_lambda is not None):
        sys.exit('--bootstrap net refreshes the values inside the lambda-return: it needs --td --td_lambda')
    if args.bootstrap == 'net' and args.new:
        sys.exit('--bootstrap net with --new: the values of a random net are noise')
    if args.bootstrap_rounds < 1:
        sys.exit('--bootstrap_rounds is at least 1')
    if args.bootstrap_rounds > 1 and args.bootstrap == 'recorded':
        sys.exit('--bootstrap_rounds above 1 needs --bootstrap net: recorded values do not change between rounds')
    if args.weighted_mode not in (0, 1, 2):
        sys.exit('--weighted_mode: 0 inverse of variance, 1 number of visits, 2 both')
    args.validation_backend = args.validation_backend or args.fit_backend
    if args.validation_backend == 'hip' and args.fit_backend != 'hip':
        sys.exit('--validation_backend hip reads the parameters of a HIP fit: it needs --fit_backend hip')
    if args.early_stopping and not args.validation:
        sys.exit('Early stopping without validation?')
    if not args.data_paths:
        sys.exit('list_of_data is empty: give --data_paths (what play.py --save wrote, e.g. data/self1/data*)')


def iterations(args, n_data):
    """train.py:193-203: (iterations, iterations between two validations)"""
    iters_per_epoch = n_data // args.batch_size
    iters = int(args.epochs * iters_per_epoch)
    if args.max_iters >= 0:
        iters = int(min(iters, args.max_iters))
    if args.min_iters >= 0:
        iters = int(max(iters, args.min_iters))
    if args.early_stopping:
        # the reference's early-stopping loop validates once an epoch until its patience runs out (train.py:246-277);
        # --max_iters still bounds it here
        return (args.max_iters if args.max_iters >= 0 else 100000), max(1, iters_per_epoch)
    return iters, iters // args.val_total + 1


def main_dist(args):
    """--head dist: the same files, split and iteration count; categorical targets (offline.fit_episodes_dist)"""
    from tetris_mcts_amd.model_distributional import Model_Dist
    from tetris_mcts_amd.offline import fit_episodes_dist
    if args.bootstrap == 'search':
        from tetris_mcts_amd.episodes import rootdist_stem
        from tetris_mcts_amd.nodes import load_head
        from tetris_mcts_amd.offline import choose_stems
        try:
            head = dict(zip(('atoms', 'vmin', 'vmax'), load_head([rootdist_stem(s) for s in choose_stems(args.data_paths, args.last_nfiles)])))
        except ValueError as e:
            sys.exit('--bootstrap search: %s (record with play.py --agent_type DistValueSim --save --save_root_dists)' % e)
        for k, v in args.head_given.items():
            if v != head[k]:
                sys.exit('--%s %s, but the root distributions were recorded by a head with %s %s (their sidecar, .head.npy): leave '
                         '--%s out, or give the files of that head' % (k, v, k, head[k], k))
        args.atoms, args.vmin, args.vmax = head['atoms'], head['vmin'], head['vmax']
    model = Model_Dist(atoms=args.atoms, backend='hip')
    if not args.new:
        model.load()
    plan = {}

    def max_iters(n_train):
        plan['iters'], plan['val'] = iterations(args, n_train)
        return plan['iters']
    res = fit_episodes_dist(model, args.data_paths, batch_size=args.batch_size, max_iters=max_iters, iters_per_val=lambda _: plan['val'],
                            early_stopping=args.early_stopping, early_stopping_patience=args.early_stopping_patience,
                            fit_backend='hip_dist' if args.fit_backend == 'hip' else 'torch', validation_backend=args.validation_backend,
                            td=args.td, lam=args.td_lambda, horizon=args.td_horizon, vmin=args.vmin, vmax=args.vmax,
                            rounds=args.bootstrap_rounds, weighted=args.weighted, weighted_mode=args.weighted_mode,
                            terminal=args.terminal, censored=args.censored, last_nfiles=args.last_nfiles, validation=args.validation,
                            val_mode=args.val_mode, val_episodes=args.val_episodes, val_set_size=args.val_set_size,
                            val_set_size_max=args.val_set_size_max, bootstrap='search' if args.bootstrap == 'search' else 'net',
                            ewc_lambda=args.ewc_lambda if args.ewc_dist else None)
    print('iters:%d/%d' % (sum(r['iters'] for r in res['rounds']), plan['iters'])
          + (' best validation loss: %.5f' % res['best_validation'] if args.early_stopping else ''), flush=True)
    model.save()


def main_dist_nodes(args):
    """--dist_nodes: the head of the shards' sidecar fitted to the recorded distributions (offline.fit_dist_nodes)"""
    from tetris_mcts_amd.model_distributional import Model_Dist
    from tetris_mcts_amd.nodes import load_head
    from tetris_mcts_amd.offline import choose_stems, fit_dist_nodes
    head = dict(zip(('atoms', 'vmin', 'vmax'), load_head(choose_stems(args.data_paths, args.last_nfiles))))
    for k, v in args.head_given.items():
        if v != head[k]:
            sys.exit('--%s %s, but the shards were recorded by a head with %s %s (their sidecar, .head.npy): leave --%s out, '
                     'or give the files of that head' % (k, v, k, head[k], k))
    model = Model_Dist(atoms=head['atoms'], backend='hip')
    if not args.new:
        model.load()
    plan = {}

    def max_iters(n_train):
        plan['iters'], plan['val'] = iterations(args, n_train)
        return plan['iters']
    res = fit_dist_nodes(model, args.data_paths, batch_size=args.batch_size, max_iters=max_iters, iters_per_val=lambda _: plan['val'],
                         early_stopping=args.early_stopping, early_stopping_patience=args.early_stopping_patience,
                         fit_backend='hip_dist', validation_backend=args.validation_backend, weighted=args.weighted,
                         weighted_mode=args.weighted_mode, last_nfiles=args.last_nfiles, validation=args.validation,
                         val_set_size=args.val_set_size, val_set_size_max=args.val_set_size_max,
                         ewc_lambda=args.ewc_lambda if args.ewc_dist else None)
    print('iters:%d/%d' % (res['iters'], plan['iters'])
          + (' best validation loss: %.5f' % res['best_validation'] if args.early_stopping else ''), flush=True)
    model.save()


def main(argv=None):
    args = build_parser().parse_args(argv)
    check_args(args, sys.argv[1:] if argv is None else argv)
    if args.dist_nodes:
        return main_dist_nodes(args)
    if args.head == 'dist':
        return main_dist(args)
    from tetris_mcts_amd.model import Model_VV
    from tetris_mcts_amd.offline import fit_episodes
    model = Model_VV(backend='hip')
    if not args.new:
        model.load()
    plan = {}

    def max_iters(n_train):
        plan['iters'], plan['val'] = iterations(args, n_train)
        return plan['iters']
    if args.nodes:
        from tetris_mcts_amd.offline import fit_nodes
        res = fit_nodes(model, args.data_paths, batch_size=args.batch_size, max_iters=max_iters, iters_per_val=lambda _: plan['val'],
                        early_stopping=args.early_stopping, early_stopping_patience=args.early_stopping_patience,
                        fit_backend=args.fit_backend, validation_backend=args.validation_backend,
                        weighted=args.weighted, weighted_mode=args.weighted_mode, last_nfiles=args.last_nfiles,
                        validation=args.validation, val_set_size=args.val_set_size, val_set_size_max=args.val_set_size_max,
                        ewc_lambda=args.ewc_lambda if args.ewc else None)
        print('iters:%d/%d' % (res['iters'], plan['iters'])
              + (' best validation loss: %.5f' % res['best_validation'] if args.early_stopping else ''), flush=True)
        model.save()
        return
    res = fit_episodes(model, args.data_paths, batch_size=args.batch_size, max_iters=max_iters, iters_per_val=lambda _: plan['val'],
                       early_stopping=args.early_stopping, early_stopping_patience=args.early_stopping_patience,
                       fit_backend=args.fit_backend, validation_backend=args.validation_backend,
                       td=args.td, lam=args.td_lambda, weighted=args.weighted, weighted_mode=args.weighted_mode,
                       terminal=args.terminal, censored=args.censored, last_nfiles=args.last_nfiles, validation=args.validation,
                       val_mode=args.val_mode, val_episodes=args.val_episodes, val_set_size=args.val_set_size,
                       val_set_size_max=args.val_set_size_max, gamma=args.target_gamma, bootstrap=args.bootstrap,
                       bootstrap_rounds=args.bootstrap_rounds, ewc_lambda=args.ewc_lambda if args.ewc else None)
    print('iters:%d/%d' % (sum(r['iters'] for r in res['rounds']), plan['iters'])
          + (' best validation loss: %.5f' % res['best_validation'] if args.early_stopping else ''), flush=True)
    model.save()


if __name__ == '__main__':
    main()
