"""Distributional value head of the reference (model/model_distributional.py:18-57 `Net`, 60-107 `Model_Dist`;
BASELINE configs[4]): conv4x4(1->32) -> LeakyReLU -> conv4x4(32->32) -> LeakyReLU -> flatten -> FC 128 -> LeakyReLU ->
FC `atoms` -> softmax, on the reference's 22 x 10 input (the two rows that are hidden today included: the reference's
network was never moved to the 20-row engine, `convOutShape((22, 10), ...)` is hard-coded at
model_distributional.py:27).  Same module names, so `state_dict`s are interchangeable.  Back ends, as model.Model_VV:
  * "hip"        - csrc/distnet.hip: hand-written gfx950 kernels on the fp32 matrix cores (wave-per-state convolutions, a
                   batched FC + softmax kernel), bit-identical to oracle/distnet_oracle.c's fma chains, driven by the native
                   launch loop (csrc/search.hip) when it is the leaf evaluator of DistValueSim;
  * "hip_bf16x3" - csrc/distnet_x3.inc: conv2 on the bf16 matrix cores with every operand split into three bf16 planes (six
                   plane products, fp32 accumulation), the rest as "hip": within 1e-6 relative of the
                   reference at the fixture's weights (logit spread 0.3), in general log p within 8x the reference's own
                   fp32 error against an fp64 forward, not bit-equal to "hip" (opt-in);
  * "torch"      - PyTorch-ROCm ops (MIOpen / rocBLAS): training (`loss`) and a cross-check.
The distribution arithmetic around it is in csrc/tree.hip (wave_dist_front / wave_dist_back)."""
import ctypes as C
import os
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .model import EXP_PATH, VALUENET_BACKEND, _HipHead
from .store import _p, _stream

PARAM_ORDER = ["seq.conv1.weight", "seq.conv1.bias", "seq.conv2.weight", "seq.conv2.bias", "seq.fc1.weight", "seq.fc1.bias",
               "seq.fc_v.weight", "seq.fc_v.bias"]
PREPARED = 278528       # TM_DISTNET_PREPARED: tm_distnet_prepare's fp32 operand streams
PREPARED_X3 = 24576     # TM_DISTNET_PREPARED_X3: conv2's bf16 planes behind them under "hip_bf16x3"
HIP_BACKENDS = ("hip", "hip_bf16x3")    # the backends the native search loop (search.hip) runs
SCRATCH = 2048          # TM_DISTNET_SCRATCH
ROW = 64                # TM_DIST_ROW
CHECKPOINT = EXP_PATH + "model_checkpoint_dist"     # beside Model_VV's model_checkpoint


def _conv_out(shape, k, stride):
    return ((shape[0] - k) // stride + 1, (shape[1] - k) // stride + 1)


class Net(nn.Module):
    def __init__(self, input_shape=(22, 10), atoms=50):
        super().__init__()
        k, stride, filters, n_fc1 = 4, 1, 32, 128
        shape = _conv_out(_conv_out((22, 10), k, stride), k, stride)
        act = nn.LeakyReLU(inplace=True)
        self.seq = nn.Sequential(OrderedDict([
            ("conv1", nn.Conv2d(1, filters, k, stride)), ("act1", act),
            ("conv2", nn.Conv2d(filters, filters, k, stride)), ("act2", act),
            ("flatten", nn.Flatten()),
            ("fc1", nn.Linear(shape[0] * shape[1] * filters, n_fc1)), ("act3", act),
            ("fc_v", nn.Linear(n_fc1, atoms)),
        ]))

    def forward(self, x):
        return F.softmax(self.seq(x), 1)

    def log_prob(self, x):
        return F.log_softmax(self.seq(x), 1)


class Model_Dist(_HipHead):
    """inference(batch [B,1,22,10]) -> [dist [B, atoms]] (model_distributional.py:100-107); loss = the cross entropy
    against a target distribution, -value * (log p - log value) summed over atoms (model_distributional.py:86-98)."""
    PARAM_ORDER, SCRATCH_ROW, PREPARE = PARAM_ORDER, SCRATCH, "tm_distnet_prepare"
    fisher = ewc_anchor = None      # compute_fisher's, or a checkpoint's: what train_data(ewc_lambda=) penalises against

    def __init__(self, atoms=50, device=None, seed=None, backend=None):
        if seed is not None:
            torch.manual_seed(seed)
        self.device = torch.device(device or ("cuda" if torch.cuda.is_available() else "cpu"))
        self.atoms = int(atoms)
        self.model = Net(atoms=atoms).to(self.device).eval()
        self.backend = backend or ("hip" if self.device.type == "cuda" else "torch")
        if self.backend in HIP_BACKENDS and not (0 < self.atoms <= ROW):
            raise ValueError("the HIP head holds 1..64 atoms")
        self._flat = self._prepared = self._scratch = None

    def training(self, mode=True):
        self.model.train(mode)

    def _mode(self):
        return (VALUENET_BACKEND.get(self.backend, 0),)      # ("torch": the fp32 kernels, as before)

    def _prepared_floats(self):
        return PREPARED + (PREPARED_X3 if self.backend == "hip_bf16x3" else 0)

    @torch.no_grad()
    def inference_device(self, states, out=None):
        """states: int8 [B,200] (or [B,20,10]) on the device, the 20 visible rows -> float32 [B, 64] (atoms first, zero padded
        rows are NOT guaranteed: only [:, :atoms] is written)."""
        B = states.shape[0]
        if out is None:
            out = torch.zeros(B, ROW, dtype=torch.float32, device=self.device)
        if self.backend in HIP_BACKENDS:
            P, prep, scr = self.hip_buffers(B)
            st = states.reshape(B, 200).to(torch.int8).contiguous()
            _lib.check(_lib.lib().tm_distnet_forward(P, prep, *self._mode(), _p(st), B, self.atoms, _p(out), out.stride(0), scr,
                                                     _stream()), "tm_distnet_forward")
        else:
            x = torch.zeros(B, 1, 22, 10, dtype=torch.float32, device=self.device)
            x[:, 0, 2:, :] = states.reshape(B, 20, 10).float()   # the reference's net sees 22 rows (model_distributional.py:27)
            out[:, :self.atoms].copy_(self.model(x))
        return out

    @torch.no_grad()
    def inference_requests(self, store):
        """Evaluate a TreeStore's pending leaf requests into its eval_dist (fused render + forward, HIP back ends only)."""
        P, prep, scr = self.hip_buffers(store.n_games)
        _lib.check(_lib.lib().tm_distnet_forward_requests(P, prep, *self._mode(), C.byref(store.s), scr, _stream()),
                   "tm_distnet_forward_requests")

    @torch.no_grad()
    def inference(self, batch):
        """Reference signature (model_distributional.py:100-107): float array [B,1,22,10] -> [dist [B, atoms]] numpy."""
        b = torch.as_tensor(batch, dtype=torch.float32, device=self.device)
        if self.backend in HIP_BACKENDS and bool((b[:, 0, :2] == 0).all().item()):
            out = self.inference_device(b[:, 0, 2:, :].reshape(b.shape[0], 200).to(torch.int8))
            return [out[:, :self.atoms].cpu().numpy()]
        return [self.model(b).cpu().numpy()]     # something in the two hidden rows: only the torch ops take 22 rows

    def loss(self, state, value, weight=None):
        """model_distributional.py:84-98: -value * (log p - log value) summed over the atoms = KL(value || p), optionally
        weighted.  The reference's expression is NaN wherever a target atom is exactly 0 (0 * -inf; its targets would be the
        search's shifted distributions, whose lowest bins are empty): value * log value is taken as 0 there (torch.xlogy), the
        same number everywhere else."""
        lp = self.model.log_prob(state)
        per = torch.xlogy(value, value) - value * lp
        if weight is not None:
            per = weight.reshape(-1, 1) * per     # model_distributional.py:93-94 (weight.squeeze() broadcasts over the LAST axis
                                                  # there, which only lines up for batch == atoms; per-sample weights are what is meant)
        std, mean = torch.std_mean(per.sum(dim=1))
        return mean, std

    def _optimizer(self):
        if getattr(self, "optimizer", None) is None:
            # Model_Dist.__init__ (model_distributional.py:66): what the class ends up with (its _init_model's Yogi is overwritten)
            self.optimizer = torch.optim.Adam(self.model.parameters(), lr=1e-4, eps=1e-5, amsgrad=True)
        return self.optimizer

    def load(self, filename=CHECKPOINT, verbose=True):
        """Model_VV.load for this head: the same dictionary keys in a file of its own.  A checkpoint with another number of atoms
        is refused (fc_v would not fit, and the search indexes the parameter blob with the store's atom count); an optimiser state
        that does not fit the optimiser restarts it with a warning.  Without the file nothing changes."""
        if os.path.isfile(filename):
            if verbose:
                print("Loading model...", flush=True)
            ck = torch.load(filename, map_location=self.device)
            state = ck["model_state_dict"]
            atoms = int(state["seq.fc_v.weight"].shape[0])
            if atoms != self.atoms:
                raise ValueError("%s holds a head of %d atoms, this Model_Dist has %d" % (filename, atoms, self.atoms))
            fisher = anchor = None      # the Fisher and its anchor, when the checkpoint carries them (both or neither)
            if "fisher" in ck and "ewc_anchor" in ck:
                fisher, anchor = self._ewc_flat(ck["fisher"], "fisher"), self._ewc_flat(ck["ewc_anchor"], "ewc_anchor")
            self.model.load_state_dict(state)
            self.fisher, self.ewc_anchor = fisher, anchor
            if ck.get("optimizer_state_dict"):
                try:
                    (getattr(self, "optimizer", None) or self._optimizer()).load_state_dict(ck["optimizer_state_dict"])
                except (ValueError, KeyError) as e:
                    from sys import stderr
                    print("WARNING: optimizer state of %s not loaded (%s): the optimiser restarts with fresh moments"
                          % (filename, e), file=stderr, flush=True)
        elif verbose:
            print("Checkpoint not found, using default model", flush=True)
        self.weights_changed()

    def save(self, filename=CHECKPOINT, verbose=True):
        """model_state_dict and optimizer_state_dict, as Model_VV.save writes them; a fused Adam's state dict is torch.optim.Adam's
        (train._FlatBuffers.state_dict), so either optimiser loads what the other wrote."""
        if verbose:
            print("Saving model...", flush=True)
        os.makedirs(os.path.dirname(filename) or ".", exist_ok=True)
        opt = getattr(self, "optimizer", None) or self._optimizer()
        ck = {"model_state_dict": self.model.state_dict(), "optimizer_state_dict": opt.state_dict()}
        if self.fisher is not None:      # (a model without a Fisher writes exactly those two keys)
            ck["fisher"], ck["ewc_anchor"] = self._ewc_dict(self.fisher), self._ewc_dict(self.ewc_anchor)
        torch.save(ck, filename)

    def _ewc_dict(self, flat):
        """a flat [TM_DISTNET_PARAMS(atoms)] tensor as {parameter name: CPU tensor shaped like the parameter}, in PARAM_ORDER"""
        sd, out, off = self.model.state_dict(), OrderedDict(), 0
        for k in PARAM_ORDER:
            n = sd[k].numel()
            out[k] = flat[off:off + n].detach().reshape(sd[k].shape).cpu().clone()
            off += n
        return out

    def _ewc_flat(self, d, key):
        sd = self.model.state_dict()
        for k in PARAM_ORDER:
            if k not in d or tuple(d[k].shape) != tuple(sd[k].shape):
                raise ValueError("checkpoint key %r: %s has shape %s, the net's is %s"
                                 % (key, k, tuple(d[k].shape) if k in d else None, tuple(sd[k].shape)))
        return torch.cat([d[k].reshape(-1).float() for k in PARAM_ORDER]).to(self.device).contiguous()

    @torch.no_grad()
    def compute_fisher(self, data, weighted=False, state_format="dense", slab=1024):
        """The empirical Fisher diagonal of the fit's loss over the rows of `data`, F[i] = (1/n) sum_b (d loss_b / d p_i)^2, by
        ONE call of tm_distnet_fit_fisher (csrc/distnet_fit.hip).  data: [states, targets, weights] laid
        out as for train_data(fit_backend="hip_dist") and checked by its rules (train.HipDistFit._check_rows): states [n,1,22,10]
        with the two top rows empty, or with state_format="packed" the packed observations, int32 [n,12] on the GPU; targets
        [n,atoms] finite and >= 0; one weight a row.  weighted: the row's weight multiplies its loss, the weights taken AS GIVEN
        (train_data divides its weights by their mean before it fits: hand over those to get the Fisher of the loss it fitted).
        slab: rows per launch sequence; the result does not depend on a slab >= n.  Sets self.fisher (flat float32
        [279232 + 129 atoms] on the device, PARAM_ORDER) and self.ewc_anchor (a copy of the flat weights as they stand) and
        returns self.fisher.  The optimiser and the weights are not touched."""
        from . import train as T
        dev = self.device
        if dev.type != "cuda":
            raise ValueError("Model_Dist.compute_fisher runs the HIP Fisher pass: the model must be on the GPU, not %s" % (dev,))
        if state_format not in ("dense", "packed"):
            raise ValueError("state_format must be 'dense' or 'packed', not %r" % (state_format,))
        if len(data) != 3:
            raise ValueError("Model_Dist.compute_fisher needs data = [states, targets, weights]")
        packed = state_format == "packed"
        data = [d if packed and i == 0 else torch.as_tensor(d, dtype=torch.float32, device=dev) for i, d in enumerate(data)]
        rows = T.HipDistFit.__new__(T.HipDistFit)      # the rules and the kept copies of a hip_dist fit's rows, without a fit
        rows.packed, rows.atoms = packed, self.atoms
        n = rows._check_rows(data, "Model_Dist.compute_fisher", "data")
        rows._keep(data, n, "")
        slab = int(slab)
        n_ws = _lib.lib().tm_distnet_fit_fisher_workspace(slab, self.atoms)
        if n_ws < 0:
            raise ValueError("Model_Dist.compute_fisher: a slab of %d rows is refused" % slab)
        sd = self.model.state_dict()
        P = torch.cat([sd[k].detach().reshape(-1).float() for k in PARAM_ORDER]).contiguous()      # (a fresh copy: the anchor)
        ws = torch.empty(n_ws, dtype=torch.float32, device=dev)
        fisher = torch.empty(P.numel(), dtype=torch.float32, device=dev)
        name = "tm_distnet_fit_fisher" + ("_packed" if packed else "")
        with torch.cuda.device(dev):
            _lib.check(getattr(_lib.lib(), name)(_p(P), _p(rows.states), _p(rows.target), rows.target.stride(0), _p(rows.weight), None,
                                                 n, slab, self.atoms, int(bool(weighted)), _p(fisher), _p(ws), _stream()), name)
        self.fisher, self.ewc_anchor = fisher, P
        return self.fisher

    def _fused_optimizer(self, commit=True):
        """the model's optimiser as a train.FusedAdam (one HIP kernel a step, a flat gradient buffer), the state of the Adam it
        replaces carried over through a copy of its state dict; with `commit` it becomes the model's optimiser for later fits
        (train_data commits only once a hip_dist fit has passed its checks: a refused fit leaves the model as it was)"""
        import copy
        from .train import FusedAdam
        old = getattr(self, "optimizer", None)
        if isinstance(old, FusedAdam):
            return old
        new = FusedAdam(self.model.parameters(), lr=1e-4, eps=1e-5, amsgrad=True)
        if old is not None:
            new.load_state_dict(copy.deepcopy(old.state_dict()))
        if commit:
            self.optimizer = new
        return new

    def train_data(self, data, fit_backend="torch", ewc_lambda=None, **kwargs):
        """data: [states [n,1,22,10], distributions [n,atoms], weights [n,1]]; Model.train_data (model/model.py:176-249) with
        this class's loss; data-parallel over the ranks as train.train_data describes.  fit_backend: "torch" (the default:
        autograd and the model's optimiser as it stands) or "hip_dist" (csrc/distnet_fit.hip's gradient step and the fused Adam;
        train.HipDistFit lists what it needs); "hip" names the value net's step and is refused.  validation_backend (in kwargs): "torch"
        or "hip" (csrc/distnet_fit.hip's validation pass; it needs fit_backend="hip_dist").  state_format (in kwargs): "dense" or
        "packed" (data[0] holds the packed observations, int32 [n,12] on the GPU, and is passed on as it is; train.train_data).
        ewc_lambda: None, or the lambda of elastic weight consolidation against this model's Fisher and anchor (compute_fisher's or
        a checkpoint's; train.train_data's `ewc_dist`, fit_backend="hip_dist"); a model that holds no Fisher logs one line and
        fits unpenalised, as on the first cycle."""
        from . import train as T
        if ewc_lambda is not None:
            import math
            from sys import stderr
            if isinstance(ewc_lambda, bool) or not isinstance(ewc_lambda, (int, float)) or not (math.isfinite(ewc_lambda) and ewc_lambda >= 0):
                raise ValueError("Model_Dist.train_data: ewc_lambda must be finite and >= 0, not %r" % (ewc_lambda,))
            if fit_backend != "hip_dist":
                raise ValueError("Model_Dist.train_data: ewc_lambda needs fit_backend='hip_dist'")
            if "ewc_dist" in kwargs:
                raise ValueError("Model_Dist.train_data: give ewc_lambda or ewc_dist, not both")
            if self.fisher is None:
                print("Model_Dist.train_data: no Fisher to consolidate against (first cycle?): fitting without the penalty",
                      file=stderr, flush=True)
            else:
                kwargs["ewc_dist"] = dict(fisher=self.fisher, anchor=self.ewc_anchor, lam=float(ewc_lambda))
        if fit_backend not in ("torch", "hip_dist"):
            raise ValueError("Model_Dist.train_data: fit_backend must be 'torch' or 'hip_dist', not %r" % (fit_backend,))
        if kwargs.get("validation_backend", "torch") not in ("torch", "hip"):
            raise ValueError("Model_Dist.train_data: validation_backend must be 'torch' or 'hip', not %r" % (kwargs["validation_backend"],))
        if kwargs.get("validation_backend", "torch") == "hip" and fit_backend != "hip_dist":
            raise ValueError("Model_Dist.train_data: validation_backend='hip' needs fit_backend='hip_dist'")
        packed = kwargs.get("state_format", "dense") == "packed"
        T.check_state_format(kwargs.get("state_format", "dense"), fit_backend, kwargs.get("validation_backend", "torch"),
                             kwargs.get("validation_fraction", 0.1), data)
        data = [d if packed and i == 0 else torch.as_tensor(d, dtype=torch.float32, device=self.device) for i, d in enumerate(data)]
        best = {}

        def save():
            best["model"] = {k: v.detach().clone() for k, v in self.model.state_dict().items()}

        def load():
            self.model.load_state_dict(best["model"])

        def loss_fn(net, batch, weighted):
            return self.loss(batch[0], batch[1], batch[2] if weighted else None)
        if fit_backend == "hip_dist":
            loss_fn.is_model_dist_loss = True      # (what tm_distnet_fit_grad computes: train_data refuses any other loss_fn)
            kwargs["fit_backend"] = fit_backend
        opt = self._fused_optimizer(commit=False) if fit_backend == "hip_dist" else self._optimizer()
        try:
            res = T.train_data(self.model, opt, data, save=save, load=load, loss_fn=loss_fn, **kwargs)
        finally:
            if getattr(opt, "_flat", None) is not None:      # flattened = past HipDistFit's checks: the parameters are its views now
                self.optimizer = opt
        self.model.eval()
        self.weights_changed()
        return res
