"""Batched mirror of the reference's `ValueSim` agent (agents/ValueSim.py:12-185): per simulation
select -> evaluate the leaf with the value net -> expand -> backup (gamma 0.999, check_low threshold 1,
pool of 100000 nodes per game).  The tree loop runs in tree.hip; leaf states of all games are evaluated
as one batch."""
from .. import store as st
from ..model import HIP_BACKENDS, Model_VV as Model
from .agent import OnlineFit, TreeAgent


class ValueSim(OnlineFit, TreeAgent):
    kind = st.KIND_VALUESIM
    low = 1
    COUNT_HELD, DUMP_PATH = True, "./data/dump"

    def __init__(self, online=True, memory_size=500000, min_visits_to_store=10, gamma=0.999, memory_growth_rate=5000,
                 max_nodes=100000, model=None, evaluator=None, valuenet_backend="hip", fit_backend="torch",
                 validation_backend="torch", valuenet_fc1="fp32", fit_states="dense", harvest=False, **kwargs):
        """`valuenet_backend`: the Model_VV backend of the model the agent builds when `model` is None ("hip", the default;
        "hip_bf16x3", the split-precision kernels; "torch"), `valuenet_fc1` its fc1 ("fp32", the default; "bf16x3": fc1 split
        as well, with "hip_bf16x3" only - Model_VV refuses any other pairing).  `fit_backend`: how the online fits take their gradients
        (train.train_data: "torch", the default, or "hip", csrc/valuenet_fit.hip).  `validation_backend`: how they validate
        ("torch", the default, or "hip": the same kernels' forward over the held-out rows; it needs fit_backend="hip").
        `fit_states`: what the fits are fed ("dense", the default: the harvested observations rendered to [n,1,20,10] floats;
        "packed": the 48-byte observations themselves, read by the kernels - it needs fit_backend="hip" and validation_backend="hip").
        `evaluator`: a callable, int8 device tensor [B, 200] -> (v[B], var[B]); B is every slot of every game, or, under TreeAgent's
        `dense_requests`, the posted requests padded to a multiple of `dense_pad`.
        `harvest`: the store harvests at its collections (tm_store.online = 1, a `replay_cap`, `min_visits_to_store` as given)
        WITHOUT any fit: nothing else about the agent changes, and whoever asked for it drains the tuples (nodes.NodeRecorder).
        Not together with an online fit, which drains the same buffers."""
        benchmark = kwargs.get("benchmark", False)
        if harvest and online and not benchmark:
            raise ValueError("harvest=True records the harvested tuples and online=True fits them: both drain the same buffers, "
                             "give one of the two")
        if fit_backend not in ("torch", "hip"):
            raise ValueError("fit_backend must be 'torch' or 'hip', not %r ('hip_dist' is DistValueSim's)" % (fit_backend,))
        if validation_backend not in ("torch", "hip"):
            raise ValueError("validation_backend must be 'torch' or 'hip', not %r" % (validation_backend,))
        if validation_backend == "hip" and fit_backend != "hip":
            raise ValueError("validation_backend='hip' needs fit_backend='hip'")
        self.fit_backend, self.validation_backend = fit_backend, validation_backend
        self.check_fit_states(fit_states, "hip")
        kwargs.pop("min_visit", None)  # play.py:89 forwards it; the reference ValueSim ignores it too
        harvesting = bool(harvest) or (online and not benchmark)
        # device-side harvest buffer per game (64 B per tuple); a GC at a 100 000-entry pool frees a few thousand
        # observations with enough visits, and whatever exceeds the buffer between two drains is dropped
        kwargs.setdefault("replay_cap", min(int(max_nodes), 16384) if harvesting else 0)
        super().__init__(max_nodes=max_nodes, gamma=gamma, online=harvesting,
                         min_visits_to_store=min_visits_to_store, **kwargs)
        self.online = online
        self.harvest = bool(harvest)
        self.n_trains = 0
        self._memory = None       # (packed observations, stats) carried over between trainings
        self.memory_size = memory_size
        self.memory_growth_rate = memory_growth_rate
        self.min_visits_to_store = min_visits_to_store
        self.evaluator = evaluator
        if evaluator is None:
            if model is not None:
                self.model = model
            elif valuenet_fc1 == "fp32":
                self.model = Model(backend=valuenet_backend)
            else:
                self.model = Model(backend=valuenet_backend, fc1=valuenet_fc1)
            if model is None:
                self.model.load()
            self.model.training(False)

    def evaluate(self, states, v_out, var_out):
        if self.evaluator is not None:
            v, var = self.evaluator(states)
            v_out.copy_(v)
            var_out.copy_(var)
        else:
            self.model.inference_device(states, v_out, var_out)

    def search_model(self):
        return self.model if (self.evaluator is None and self.model.backend in HIP_BACKENDS) else False

    def evaluate_requests(self):
        if self.evaluator is None and self.model.backend in HIP_BACKENDS:
            self.model.inference_requests(self.store)   # observations rendered inside the conv kernel
        else:
            super().evaluate_requests()

    # ---- online training (ValueSim.py:161-185): agent.OnlineFit, with the value net's tuples (packed observations, stats) ----
    @staticmethod
    def dump_training_set(path, state, value, variance, visit):
        """np.savez layout of the reference's replay dump (ValueSim.py:176-177, ValueSimC.py:8): keys states [n,1,20,10],
        values / variance / weights [n,1]; written by rank 0 only."""
        import os
        import numpy as np
        from .. import dist as tdist
        if tdist.rank() != 0:
            return
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        np.savez(path, states=state.cpu().numpy(), values=value.cpu().numpy(), variance=variance.cpu().numpy(),
                 weights=visit.cpu().numpy())

    def _drain(self):
        keys, stats = self.store.replay()
        self.store.t["replay_count"].zero_()
        return keys, stats

    def _gather(self, rows):
        import torch
        from .. import dist as tdist
        return tdist.all_gather_tuples(rows[0].view(torch.int32), rows[1])

    def _dense_set(self, rows):
        from .. import dist as tdist
        return list(tdist.training_arrays(*rows))

    def _packed_set(self, rows):
        from .. import dist as tdist
        return [rows[0]] + list(tdist.training_targets(rows[1]))

    def _dump(self, path, data):
        self.dump_training_set(path, *data)
