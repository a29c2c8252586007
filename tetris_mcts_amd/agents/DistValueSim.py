"""DistValueSim: the reference's distributional agent (agents/DistValueSimOnline.py:12-94, BASELINE configs[4]) rebuilt from
its working parts - the file itself does not import (it names `model.ValueSim`, `select_trace_obs_dist`,
`backup_trace_obs_dist`, none of which exist), so there is no behaviour to be a drop-in for beyond the pieces:

  * the tree of TreeAgent WITHOUT the observation projection: per-node statistics (visit, mean, score, variance, M2) and
    a distribution of `atoms` bins over [vmin, vmax) per node, as agents/core_distributional.py's kernels hold them;
  * selection = select_trace_distributional (core_distributional.py:81-104) with the check_low it means to call
    (under-visited children first, low = 5; libc rand()) and policy_dist (:66-79);
  * leaf evaluation = model_distributional.Net (model/model_distributional.py:18-57: softmax over the atoms; input the
    reference's 22 x 10 board = the 20 visible rows under two empty ones) as hand-written HIP kernels (csrc/distnet.hip)
    launched by the native loop of csrc/search.hip; v_dummy for a finished game;
  * backup = backup_trace_distributional (:108-124) with r = the leaf's score;
  * compute_stats / the action = DistValueSimOnline.py:76-98.
The tree loop is tree.hip (TM_KIND_DIST: wave_dist_front / wave_dist_back, one lane per atom in the backup); numerics =
oracle/dist_oracle.c, held to a pure-Python run of the reference functions (tests/golden/ref_distpy.npz)."""
import numpy as np
import torch

from .. import store as st
from .agent import OnlineFit, TreeAgent


class DistValueSim(OnlineFit, TreeAgent):
    kind = st.KIND_DIST
    low = 5
    DUMP_PATH = "./data/memory_dump"

    def __init__(self, atoms=50, vmin=0, vmax=5000, max_nodes=100000, model=None, evaluator=None, online=False,
                 min_visits_to_store=50, memory_size=500000, memory_growth_rate=5000, valuenet_backend=None, fit_backend="torch",
                 validation_backend="torch", fit_states="dense", harvest=False, **kwargs):
        """fit_backend: how train_nodes takes the gradients of the head's fits - "torch" (autograd, torch.optim.Adam) or
        "hip_dist" (csrc/distnet_fit.hip and the fused Adam).  "hip" names the value net's step (csrc/valuenet_fit.hip: the
        Gaussian loss, not this head's) and is refused here.
        validation_backend: how those fits validate - "torch" or "hip" (the same kernels' forward over the held-out rows; it
        needs fit_backend="hip_dist").
        fit_states: what those fits are fed - "dense" (the harvested observations rendered to [n,1,22,10] floats) or "packed" (the
        48-byte observations themselves, read by the kernels; it needs fit_backend="hip_dist" and validation_backend="hip").
        valuenet_backend: the Model_Dist backend of the model the agent builds when `model` is None (None: Model_Dist's
        default; "hip", "hip_bf16x3" - the split-precision kernels - or "torch").  That model loads
        pytorch_model/model_checkpoint_dist (train.py --head dist) when the file exists; a checkpoint of another atom count is
        refused.
        online: the reference's online leg (DistValueSimOnline.py:116-170) - a collection stores the freed nodes with at
        least `min_visits_to_store` visits whose seven children have all been visited (its commented store_nodes, default 50)
        as (board, distribution, visits) tuples, train_nodes fits the head on them (memory_size / memory_growth_rate as
        ValueSim's).
        harvest: ValueSim's - the store harvests at its collections (tm_store.online = 1, the default `replay_cap`,
        `min_visits_to_store` as given) WITHOUT any fit: nothing else about the agent changes, and whoever asked for it drains the
        tuples (nodes.DistNodeRecorder).  Not together with an online fit, which drains the same buffers."""
        if harvest and online and not kwargs.get("benchmark", False):
            raise ValueError("harvest=True records the harvested tuples and online=True fits them: both drain the same buffers, "
                             "give one of the two")
        if fit_backend not in ("torch", "hip_dist"):
            raise ValueError("DistValueSim: fit_backend must be 'torch' or 'hip_dist', not %r ('hip' is the value net's gradient "
                             "step)" % (fit_backend,))
        if validation_backend not in ("torch", "hip"):
            raise ValueError("DistValueSim: validation_backend must be 'torch' or 'hip', not %r" % (validation_backend,))
        if validation_backend == "hip" and fit_backend != "hip_dist":
            raise ValueError("DistValueSim: validation_backend='hip' needs fit_backend='hip_dist'")
        self.fit_backend, self.validation_backend = fit_backend, validation_backend
        self.check_fit_states(fit_states, "hip_dist")
        kwargs.pop("min_visit", None)
        kwargs.pop("gamma", None)                      # the distributional backup does not discount
        self.atoms, self.vrange = int(atoms), (float(vmin), float(vmax))
        self.evaluator = evaluator
        benchmark = kwargs.get("benchmark", False)
        self.online = bool(online) and not benchmark
        self.harvest = bool(harvest)
        harvesting = self.harvest or self.online
        kwargs.setdefault("replay_cap", min(int(max_nodes), 16384) if harvesting else 0)
        self.memory_size, self.memory_growth_rate, self.n_trains, self._memory = int(memory_size), int(memory_growth_rate), 0, None
        super().__init__(max_nodes=max_nodes, online=harvesting, min_visits_to_store=min_visits_to_store, **kwargs)
        if evaluator is None:
            from ..model_distributional import Model_Dist
            if model is None:
                model = Model_Dist(atoms=self.atoms, backend=valuenet_backend)
                import os
                from ..model_distributional import CHECKPOINT
                if os.path.isfile(CHECKPOINT):         # what train.py --head dist wrote; without the file nothing is touched
                    model.load(verbose=False)
            self.model = model
            if int(getattr(self.model, "atoms", self.atoms)) != self.atoms:
                # the head's parameter blob is indexed with the store's atom count (tm_distnet_forward_requests): another
                # count reads fc_v out of bounds
                raise ValueError("DistValueSim(atoms=%d) was given a model with %d atoms" % (self.atoms, int(self.model.atoms)))
        else:
            self.model = None

    def _build(self, n_games):
        self.n_games = int(n_games)
        self.n_sub = 1
        kw = dict(self._store_kwargs)
        kw.update(dist_bins=self.atoms, dist_range=self.vrange)
        self.store = st.TreeStore(self.n_games, self.max_nodes, **kw)

    def search_model(self):
        """the HIP head (either HIP backend) is driven by the native launch loop (search.hip); a Python callable or the
        torch back end by TreeAgent.mcts"""
        from ..model_distributional import HIP_BACKENDS
        return self.model if (self.evaluator is None and self.model.backend in HIP_BACKENDS) else False

    @torch.no_grad()
    def evaluate_requests(self):
        """The pending leaves' observations -> distributions over the atoms, into the store's eval_dist."""
        from ..model_distributional import HIP_BACKENDS
        s = self.store
        if self.evaluator is None and self.model.backend in HIP_BACKENDS:
            self.model.inference_requests(s)                              # nodes rendered inside the convolution kernel
            return
        if self.dense_requests:
            states, _, n = s.gather_eval(self.dense_pad)                  # int8 [m, 200]: the pending leaves, then zero boards
            if n == 0:
                return
        else:
            states = s.render_eval()                                      # int8 [G, 200]; all zero where nothing is asked
        rows = states.shape[0]
        if self.evaluator is not None:
            d = torch.as_tensor(np.asarray(self.evaluator(states.cpu().numpy().reshape(-1, 20, 10)), np.float32), device=s.device)
        else:
            x = torch.zeros(rows, 1, 22, 10, dtype=torch.float32, device=s.device)
            x[:, 0, 2:, :] = states.view(rows, 20, 10).float()           # the reference's net sees 22 rows (model_distributional.py:27)
            d = self.model.model(x)
        d = d.reshape(rows, self.atoms)
        if self.dense_requests:
            s.scatter_eval_dist(d)
        else:
            s.t["eval_dist"][:, :self.atoms].copy_(d)

    def get_value(self, node=None):
        """(mean, variance) of the root's distribution (DistValueSimOnline.py:100-109: mean_variance of node_dist)."""
        s = self.store
        g = torch.arange(self.n_games, device=s.device)
        root = s.t["gs"][:, st.GS["ROOT"]].long() if node is None else torch.as_tensor(np.atleast_1d(node), device=s.device).long()
        d = s.t["node_dist"][g, root, :self.atoms].double()
        delta = (self.vrange[1] - self.vrange[0]) / self.atoms
        centre = (torch.arange(self.atoms, device=s.device, dtype=torch.float64) + 0.5) * delta
        mean = (d * centre).sum(1)
        var = (d * centre * centre).sum(1) - mean * mean
        mean, var = mean.cpu().numpy(), var.cpu().numpy()
        return (mean[0], var[0]) if self.n_games == 1 else (mean, var)

    # ---- online training (DistValueSimOnline.py:143-170): agent.OnlineFit, with tuples harvested on the device at the collections
    # (tree.hip dist_keep / dist_harvest_store), all-gathered over the ranks, the head fitted on their union with Model_Dist's loss ----
    def harvested(self):
        """(packed observations int32 [n,12], distributions float32 [n,64], visits float32 [n]) of this rank since the last
        drain; the device buffers are emptied."""
        s = self.store
        keys, dists, visits = s.replay_dist()
        keys, dists, visits = keys.clone(), dists.clone(), visits.clone()
        s.t["replay_count"].zero_()
        return keys, dists, visits

    def _drain(self):
        return self.harvested()

    def _gather(self, rows):
        from .. import dist as tdist
        return tdist.all_gather_rows(rows[0].view(torch.int32), *rows[1:])

    def _packed_set(self, rows):
        keys, dists, visits = rows
        return [keys, dists[:, :self.atoms].contiguous(), visits.reshape(-1, 1)]

    def _dense_set(self, rows):
        from .. import dist as tdist
        keys, dists, visits = rows
        states = torch.zeros(keys.shape[0], 1, 22, 10, dtype=torch.float32, device=keys.device)
        states[:, :, 2:, :] = tdist.render_observations(keys)          # the net's 22 rows: two empty ones on top
        return [states, dists[:, :self.atoms].contiguous(), visits.reshape(-1, 1)]

    def _dump(self, path, data):
        import os
        from .. import dist as tdist
        if tdist.rank() == 0:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            np.savez(path, states=data[0].cpu().numpy(), values=data[1].cpu().numpy(), weights=data[2].cpu().numpy())
