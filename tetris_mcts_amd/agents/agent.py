"""Batched mirror of the reference's `Agent` / `TreeAgent` (agents/agent.py:10-307).

Same surface — play(), get_action(), get_prob(), get_stats(), get_value_and_variance(), update_root(game),
close() — over `n_games` concurrent games whose trees live on the GPU (store.TreeStore).  With n_games == 1
return values have the reference's scalar shapes, so play.py drives it unchanged.
"""
import numpy as np
import torch

from .. import store as st


class Agent:
    def __init__(self, n_actions=7, benchmark=False, **kwargs):
        self.episode = 0
        self.n_actions = n_actions
        self.benchmark = benchmark

    def play(self):
        raise NotImplementedError('update_root not implemented')

    def get_action(self):
        raise NotImplementedError('get_action not implemented')

    def get_prob(self):
        raise NotImplementedError('get_action not implemented')

    def update_root(self, game):
        raise NotImplementedError('update_root not implemented')

    def close(self):
        raise NotImplementedError('close not implemented')


class TreeAgent(Agent):
    kind = st.KIND_VALUESIM
    low = 1

    def __init__(self, sims=100, max_nodes=500000, env=None, env_args=None, node_saver=None, projection=True,
                 min_visits=30, n_games=None, gamma=0.999, online=False, min_visits_to_store=10, replay_cap=0,
                 max_trace=1024, nq_size=1 << 20, reset_on_pool_exhaustion=True, n_sub=1, ev_every=0,
                 gc_slice_cycles=150000, gc_spec_nodes=None, gc_cost_units=0, gc_collectors=0, dense_requests=False,
                 dense_pad=256, evaluator_pure=False, **kwargs):
        """The last three are for the evaluators the engine does not own - a callable, the torch back ends - which the Python loop
        below drives (where the native loop runs they are accepted and change nothing: it asks only for what it needs already).
        `dense_requests`: the evaluator is handed the posted requests only, as a dense batch padded to a multiple of `dense_pad`
        rows with zero boards (store.gather_eval / scatter_eval), instead of every slot of every game.  `evaluator_pure`: the
        caller's promise that the outputs are a function of the state and of the weights alone; the loop then posts only the
        requests the backup will use (TM_SIM_EVAL_NEEDED) - tell evaluator_changed() when a callable's weights change."""
        super().__init__(**kwargs)
        if not projection:
            raise NotImplementedError("projection=False is broken in the reference itself (ValueSim.py:73-74)")
        single_leaf = self.kind in (st.KIND_VALUESIM, st.KIND_CPPAGENT)
        if evaluator_pure and self.kind in (st.KIND_VANILLA, st.KIND_VANILLA_C):
            raise ValueError("evaluator_pure: the Vanilla agents have no evaluator (their leaves are rollouts inside the tree kernel)")
        if int(dense_pad) < 1:
            raise ValueError("dense_pad must be at least 1")
        self.dense_requests, self.dense_pad, self.evaluator_pure = bool(dense_requests), int(dense_pad), bool(evaluator_pure)
        self._epoch_cache = single_leaf        # the kinds whose store keeps obs_eval
        self._evaluator_epoch = None
        self.sims = sims
        self.max_nodes = max_nodes
        self.env, self.env_args = env, env_args or ((20, 10), 1, 0, 0)
        self.min_visits = min_visits
        self.node_saver = node_saver
        self.projection = True
        self.gamma = gamma
        self.n_games = n_games
        self._store_kwargs = dict(kind=self.kind, env_args=self.env_args, gamma=gamma, low=self.low, online=online,
                                  min_visits_to_store=min_visits_to_store, replay_cap=replay_cap, max_trace=max_trace,
                                  nq_size=nq_size, gc_slice_cycles=gc_slice_cycles, gc_spec_nodes=gc_spec_nodes,
                                  gc_cost_units=gc_cost_units, gc_collectors=gc_collectors)
        self.n_sub, self.ev_every = int(n_sub), int(ev_every)
        self._pending_events, self.loop_events, self.catchup_launches = [], dict(timed=0, nn_ms_sum=0.0, tree_ms_sum=0.0), 0
        self.store = None
        self.reset_on_pool_exhaustion = reset_on_pool_exhaustion
        self._pending_pool_reset = None
        self.stats = None
        if n_games is not None:
            self._build(n_games)

    def _build(self, n_games):
        self.n_games = int(n_games)
        self.n_sub = max(1, min(self.n_sub, self.n_games // 4))     # a sub-batch is at least one workgroup of the tree kernel
        self.store = st.TreeStore(self.n_games, self.max_nodes, **self._store_kwargs)

    # ---- evaluation hook (the `evaluator` callable of MCTSAgent, agent.cpp:396-405) ----
    def evaluate(self, states, v_out, var_out):
        raise NotImplementedError('evaluate not implemented for this agent.')

    def evaluate_requests(self):
        """Evaluate the store's pending leaf requests into eval_v / eval_var.  Default: render the observations
        to int8 [B,200] and call evaluate(); agents with the HIP value net override this with the fused path."""
        s = self.store
        if self.dense_requests:
            states, _, n = s.gather_eval(self.dense_pad)
            if n == 0:
                return
            v, var = s.dense_outputs(states.shape[0])
            self.evaluate(states, v, var)
            s.scatter_eval(v, var)
            return
        states = s.render_eval()
        self.evaluate(states, s.t["eval_v"], s.t["eval_var"])

    def evaluator_changed(self):
        """evaluator_pure with a callable: its outputs are no longer the ones it gave before (new weights): what the tree engine
        filed per observation is not used again"""
        from ..model import next_weights_epoch
        self._evaluator_epoch = next_weights_epoch()

    def _eval_epoch(self):
        """the version of the evaluator's weights: the built-in model's, or this agent's own count for a callable"""
        if getattr(self, "evaluator", None) is None and hasattr(getattr(self, "model", None), "weights_epoch"):
            return int(self.model.weights_epoch)
        if self._evaluator_epoch is None:
            self.evaluator_changed()
        return self._evaluator_epoch

    def search_model(self):
        """The model whose HIP value net the native launch loop (search.hip) evaluates leaves with; False = this agent's
        evaluator is a Python callable, so the loop runs here instead."""
        return False

    def mcts(self, sims):
        """`sims` simulations for every game (TreeAgent.play -> self.mcts(self.root, self.sims), agents/agent.py:147-150).
        A launch starts a simulation only for games with quota left; a game that collects garbage loses launches and
        catches up at the end (store.sims_remaining)."""
        s = self.store
        model = self.search_model()
        if model is not False:
            s.search(sims, model, n_sub=self.n_sub, ev_every=self.ev_every)
            return
        both = st.SIM_BACKUP | st.SIM_FRONT
        if self.evaluator_pure:
            both |= st.SIM_EVAL_NEEDED
            if self._epoch_cache:
                if not self.dense_requests:
                    # a leaf answered from the per-observation cache has its outputs put into its slot by the tree kernel; the
                    # padded path writes every slot, that one too
                    raise ValueError("evaluator_pure on a single-leaf agent needs dense_requests=True where the Python loop runs "
                                     "(the padded path overwrites the slot of a leaf answered from the per-observation cache)")
                s.s.eval_epoch = self._eval_epoch()
        s.move_begin(sims)
        s.sim_step(both)
        todo, first = sims, True
        ev = self.ev_every if first else 0
        while todo > 0:
            for i in range(todo):
                if first and ev and i % ev == 0:
                    # events around the evaluator and the tree kernel of every ev-th simulation (the Python-driven loop's
                    # counterpart of tm_search_stats; summed in self.loop_events and read by the benchmark)
                    import torch
                    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                    e[0].record()
                    self.evaluate_requests()
                    e[1].record()
                    s.sim_step(both)
                    e[2].record()
                    self._pending_events.append(e)
                    if len(self._pending_events) >= 256:
                        self._fold_events()                 # bounded whether or not anybody reads loop_stats()
                else:
                    self.evaluate_requests()
                    s.sim_step(both)
            if not first:
                self.catchup_launches += todo
            first = False
            todo, collecting = s.sims_remaining()
            while collecting:                      # catch-up: collections under way are finished by collector-only launches
                for _ in range(6):
                    s.gc_step()
                todo, collecting = s.sims_remaining()

    def _fold_events(self, wait=False):
        """completed event triples into the running sums (all of them after a synchronize)"""
        import torch
        if wait:
            torch.cuda.synchronize()
        keep = []
        for e in self._pending_events:
            if wait or e[2].query():
                self.loop_events["nn_ms_sum"] += e[0].elapsed_time(e[1])
                self.loop_events["tree_ms_sum"] += e[1].elapsed_time(e[2])
                self.loop_events["timed"] += 1
            else:
                keep.append(e)
        self._pending_events = keep

    def loop_stats(self, reset=True):
        """Python-driven loop only: dict(timed, nn_ms_sum, tree_ms_sum, catchup_launches) from the sampled event triples"""
        self._fold_events(wait=True)
        out = dict(self.loop_events, catchup_launches=self.catchup_launches)
        if reset:
            self.loop_events = dict(timed=0, nn_ms_sum=0.0, tree_ms_sum=0.0)
            self.catchup_launches = 0
        return out

    def play(self):
        self.mcts(self.sims)
        return self.get_action()

    def compute_stats(self):
        stats, action = self.store.root_stats()
        return stats, action

    def get_action(self):
        stats, action = self.compute_stats()
        self._stats_dev, self._action_dev = stats, action
        self.stats = None
        err = self.store.errors()
        a = action.cpu().numpy()
        if bool((err != 0).any().item()):
            pool = (err & 1) != 0
            if self.reset_on_pool_exhaustion and bool(((err & ~1) == 0).all().item()):
                # The reachable tree outgrew the pool (the reference prints "MAX_NODES EXCEEDED" and runs into undefined
                # behaviour, agent.cpp:227-231).  Those games keep the action of the search done so far and restart
                # with an empty tree at their next update_root.
                from sys import stderr
                print("MAX_NODES EXCEEDED in %d game(s): their trees are re-initialised" % int(pool.sum().item()),
                      file=stderr, flush=True)
                self._pending_pool_reset = pool.clone()
            else:
                raise RuntimeError("tree engine error flags: %s" % sorted(set(err.cpu().numpy().tolist())))
        return int(a[0]) if self.n_games == 1 else a

    def get_stats(self):
        if self.stats is None:
            self.stats = self._stats_dev.cpu().numpy()
        return np.copy(self.stats[0]) if self.n_games == 1 else np.copy(self.stats)

    def get_prob(self):
        s = self.get_stats().reshape(-1, 3, 7)
        p = s[:, 0] / s[:, 0].sum(axis=1, keepdims=True)
        return p[0] if self.n_games == 1 else p

    def new_node(self, game):
        """Node index of `game`'s state in every tree, inserted if new (agents/agent.py:90-130, agent.cpp:265-270);
        an int with one game, else an int32 array [n_games]."""
        if self.store is None:
            self._build(getattr(game, "n_games", 1))
        idx = self.store.new_node(game.games).cpu().numpy()
        return int(idx[0]) if self.n_games == 1 else idx

    def expand(self, game):
        """idx = new_node(game); child[idx][a] = new_node(game after action a) (agents/agent.py:136-145, agent.cpp:201-218)."""
        if self.store is None:
            self._build(getattr(game, "n_games", 1))
        self.store.new_node(game.games, expand=True)

    def remove_nodes(self):
        """Collect everything unreachable from the root now (agents/agent.py:246-257); harvests replay tuples when online."""
        self.store.remove_nodes()

    def get_value_and_variance(self, node=None):
        """(value, variance) of a node's observation (agents/agent.py:195-204); node=None is the root, else a node index
        (one game) or an array of n_games indices."""
        s = self.store
        g = torch.arange(self.n_games, device=s.device)
        if node is None:
            root = s.t["gs"][:, st.GS["ROOT"]].long()
        else:
            root = torch.as_tensor(np.atleast_1d(node), device=s.device).long().reshape(self.n_games)
        o = s.t["node_rec"][g, root, 29].long()
        vv = s.t["obs_stat"][g, o, 1:3].view(torch.float32).cpu().numpy()
        return (vv[0, 0], vv[0, 1]) if self.n_games == 1 else (vv[:, 0], vv[:, 1])

    def update_root(self, game):
        if self.store is None:
            self._build(getattr(game, "n_games", 1))
        self.store.set_root_games(game.games)
        if self._pending_pool_reset is not None:
            self.store.pool_reset(self._pending_pool_reset)
            self._pending_pool_reset = None
        self.store.update_root()
        ended = np.atleast_1d(game.end)
        self.episode += int(ended.sum())

    def close(self):
        pass


class OnlineFit:
    """The bookkeeping of the online fits, a mixin beside TreeAgent for ValueSim and DistValueSim: the reference trains inside
    remove_nodes() (ValueSim.py:101-120,161-185; DistValueSimOnline.py:143-170); the batched engine harvests tuples at the
    collections on the device and trains between moves, on the union over all games and all ranks (tetris_mcts_amd/dist.py).
    The agent supplies what differs:
      _drain()             this rank's tuples harvested since the last drain as a tuple of tensors with one row a tuple (the
                           packed observations first); the device buffers are emptied
      _gather(rows)        the rows of all ranks
      _dense_set(rows)     the job's rows -> the list model.train_data takes, the states rendered (dist.render_observations)
      _packed_set(rows)    the same list with the packed observations as they are in place of the states
      _dump(path, data)    the dense list in the agent's np.savez layout (rank 0 writes)
    and DUMP_PATH, online, evaluator, model, fit_backend, validation_backend, memory_size, memory_growth_rate, n_trains = 0 and
    _memory = None (the rows carried over between two looks).

    fit_states (check_fit_states, called by the agent's constructor): "dense", the default, renders the job's rows before the
    fit; "packed" hands train_data the gathered observations themselves (state_format="packed": the HIP kernels read the cell
    out of the 48 bytes), and only a dump renders."""
    # Whether the rows an earlier look moved into _memory ("not enough training data") count towards train_if_collected's
    # min_tuples.  ValueSim counts them, DistValueSim does not: a difference of behaviour between the two agents that is kept
    # as it is.
    COUNT_HELD = False
    fit_states = "dense"

    def check_fit_states(self, fit_states, hip_fit):
        """keep `fit_states`; ValueError unless it is "dense", or "packed" with the HIP fit (`hip_fit`: its fit_backend's name)
        and the HIP validation - what train_data(state_format="packed") needs (fit_backend and validation_backend are set)"""
        if fit_states not in ("dense", "packed"):
            raise ValueError("fit_states must be 'dense' or 'packed', not %r" % (fit_states,))
        if fit_states == "packed" and not (self.fit_backend == hip_fit and self.validation_backend == "hip"):
            raise ValueError("fit_states='packed' needs fit_backend=%r and validation_backend='hip' (the torch fit and the torch "
                             "validation read rendered states)" % (hip_fit,))
        self.fit_states = fit_states

    def _training_set(self, rows):
        return self._packed_set(rows) if self.fit_states == "packed" else self._dense_set(rows)

    def train_if_collected(self, every=1, min_tuples=1, **kwargs):
        """train_nodes() if garbage collections have harvested tuples since the last fit (the reference's remove_nodes ->
        store_nodes -> train_nodes chain, ValueSim.py:101-120, runs at every collection of its one game); None otherwise.
        One game: call it after every move with the defaults and the cadence is the reference's.  A batch of games collects
        somewhere on nearly every move, and looking costs a device sync and a collective: `every` = look only on every k-th
        call, `min_tuples` = fit only once the job (all ranks) holds that many fresh tuples (play.py: --train_every,
        --train_min_tuples).  Every rank must call this on the same moves: the count is a collective."""
        from .. import dist as tdist
        if not self.online or self.store is None or self.store.s.replay_cap == 0:
            return None
        self._train_calls = getattr(self, "_train_calls", 0) + 1
        if self._train_calls % max(1, int(every)):
            return None
        held = int(self._memory[0].shape[0]) if (self.COUNT_HELD and self._memory is not None) else 0
        if tdist.all_sum(int(self.store.t["replay_count"].sum().item()) + held, self.store.device) < max(1, int(min_tuples)):
            return None
        return self.train_nodes(**kwargs)

    def train_nodes(self, dump_data=False, dump_path=None, **train_kwargs):
        from sys import stderr
        from .. import dist as tdist
        if not self.online or self.evaluator is not None:
            return None
        rows = self._drain()
        dropped = self.store.counter("N_DROPPED")
        if dropped > getattr(self, "_dropped_seen", 0):
            # the reference keeps every qualifying observation up to memory_size (ValueSim.py:122-159): say so when the
            # device-side harvest buffer was too small between two drains
            print("WARNING: {} harvested tuples did not fit the device replay buffer (replay_cap={}); drain more often or "
                  "raise replay_cap".format(dropped - getattr(self, "_dropped_seen", 0), self.store.s.replay_cap),
                  file=stderr, flush=True)
            self._dropped_seen = dropped
        if self._memory is not None:
            rows = tuple(torch.cat([a, b]) for a, b in zip(self._memory, rows))
        rows = tuple(a[:self.memory_size] for a in rows)
        rows_all = tdist.job_memory(self.memory_size, *self._gather(rows))      # (memory_size is the job's, not a rank's)
        d_size = int(rows_all[0].shape[0])
        m_size = min(self.n_trains * self.memory_growth_rate, self.memory_size)
        if d_size < max(m_size, 1):
            print("Not enough training data ({} < {}), collecting more data.".format(d_size, m_size), file=stderr, flush=True)
            self._memory = rows
            return None
        print("Enough training data ({} >= {}), proceed to training.".format(d_size, m_size), file=stderr, flush=True)
        data = self._training_set(rows_all)
        if dump_data:      # (the dump keeps its layout: with packed rows the states are rendered for it alone)
            self._dump(dump_path or self.DUMP_PATH, data if self.fit_states == "dense" else self._dense_set(rows_all))
        self.n_trains += 1
        opts = dict(iters_per_val=100, batch_size=1024, max_iters=50000, fit_backend=self.fit_backend,     # DistValueSimOnline.py:165
                    validation_backend=self.validation_backend)
        if self.fit_states != "dense":
            opts["state_format"] = self.fit_states
        opts.update(train_kwargs)
        res = self.model.train_data(data, **opts)
        self.model.training(False)
        self._memory = None
        print("Training complete.", file=stderr, flush=True)
        return res
