"""Value network of the reference (model/model_vv.py:13-52, `Net`; `Model_VV.inference` 210-217) on the GPU.

Same architecture, same state_dict keys (`head.conv1.weight` ... `head.fc_out.bias`, `out_ubound`,
`out_lbound`) and the same checkpoint dict format (`model_state_dict`, model/model.py:152-160), so the
reference's checkpoints load unchanged.  fp32 end to end: outputs within 1e-4 of the reference's CPU
result at the fixtures' weights (tests/golden/ref_valuenet.npz); at any weight scale, within 8x the
reference's own fp32 error against an fp64 forward plus 4 ulp of the largest output (DESIGN.md section 6,
tests/test_gpu_heads_accuracy.py).  Back ends:
  * "hip"        — tm_valuenet_forward: hand-written gfx950 kernels (fp32 MFMA), bit-identical to
                   oracle/valuenet_oracle.c's fma chains;
  * "hip_bf16x3" — tm_valuenet_forward under TM_VALUENET_BF16X3: conv2 / conv3 on the bf16 matrix cores with every
                   operand split into three bf16 planes (six plane products, fp32 accumulation; DESIGN.md section
                   3.3), the rest as "hip": the same accuracy contract (for operands of magnitude 2^-110 and above:
                   planes below bf16's normal range are lost), not bit-equal to "hip" (opt-in);
                   with fc1="bf16x3" fc1 is split the same way (TM_VALUENET_FC1_BF16X3, k_vn_fc1_x3: opt-in, for
                   the leaf-parallel kinds; fc1="fp32", the default, keeps k_vn_fc1);
  * "torch"      — PyTorch-ROCm ops (MIOpen / rocBLAS), used for training and as a cross-check.
"""
import ctypes as C
import os
from collections import OrderedDict

import torch
import torch.nn as nn

from . import _lib
from .store import _p, _stream

SCRATCH_MFMA = 2064     # TM_VALUENET_SCRATCH_MFMA (include/tetris_mcts_hip.h): floats of scratch per state (no initial contents required)
# tm_valuenet_prepare's buffer, in its order (TM_VALUENET_PREPARED_TOTAL): the fp32 operand streams, then under "hip_bf16x3"
# the convolutions' bf16 planes, then under fc1="bf16x3" fc1's
PREPARED = 477184       # TM_VALUENET_PREPARED
PREPARED_X3 = 27648     # TM_VALUENET_PREPARED_X3
PREPARED_FC1_X3 = 688128    # TM_VALUENET_PREPARED_FC1_X3
HIP_BACKENDS = ("hip", "hip_bf16x3")    # the backends the native search loop (search.hip) runs
VALUENET_BACKEND = {"hip": 0, "hip_bf16x3": 1}      # TM_VALUENET_FP32 / TM_VALUENET_BF16X3 (the C ABI's `backend`)
VALUENET_FC1 = {"fp32": 0, "bf16x3": 1}             # TM_VALUENET_FC1_FP32 / TM_VALUENET_FC1_BF16X3 (the C ABI's `fc1`)
PARAM_ORDER = ["head.conv1.weight", "head.conv1.bias", "head.conv2.weight", "head.conv2.bias", "head.conv3.weight",
               "head.conv3.bias", "head.fc1.weight", "head.fc1.bias", "head.fc_out.weight", "head.fc_out.bias",
               "out_ubound", "out_lbound"]
EXP_PATH = "./pytorch_model/"
variance_bound = 1e-1
_epoch = [0]


def next_weights_epoch():
    """A number no other set of evaluator weights in this process has had (>= 1): the tree engine files the evaluator's output
    per observation under it (tm_store::obs_eval) and uses only what was filed under the current one."""
    _epoch[0] += 1
    return _epoch[0]


class Net(nn.Module):
    def __init__(self, eps=variance_bound):
        super().__init__()
        act = nn.ReLU(inplace=True)
        self.head = nn.Sequential(OrderedDict([
            ("conv1", nn.Conv2d(1, 32, 3, 1, bias=True)), ("act1", act),
            ("conv2", nn.Conv2d(32, 32, 3, 1, bias=True)), ("act2", act),
            ("conv3", nn.Conv2d(32, 32, 3, 1, bias=True)), ("act3", act),
            ("flatten", nn.Flatten()),
            ("fc1", nn.Linear(32 * 14 * 4, 256)), ("fc_act1", act),
            ("fc_out", nn.Linear(256, 2)), ("act_out", nn.Sigmoid()),
        ]))
        self.out_ubound = nn.Parameter(torch.tensor([1e2, 1e3]), requires_grad=False)
        self.out_lbound = nn.Parameter(torch.tensor([0, eps]), requires_grad=False)

    def forward(self, x):
        return self.head(x) * self.out_ubound + self.out_lbound


class _HipHead:
    """What Model_VV and Model_Dist share towards the C ABI: the flat parameter blob, the prepared buffer of the mode and the
    scratch rows.  A subclass names PARAM_ORDER, SCRATCH_ROW (floats of scratch per state) and PREPARE (its prepare entry
    point), and gives _mode(), the (backend[, fc1]) arguments of its entry points, and _prepared_floats(), the size of that
    mode's prepared buffer."""

    def weights_changed(self):
        """call after the parameters were written (an optimiser step, load_state_dict): the blob and the prepared buffer -
        operand streams and planes live in the one buffer - are rebuilt"""
        self._flat = self._prepared = None

    def flat_params(self):
        if self._flat is None:
            sd = self.model.state_dict()
            self._flat = torch.cat([sd[k].detach().reshape(-1).float() for k in self.PARAM_ORDER]).contiguous()
        return self._flat

    def set_flat_params(self, flat):
        """flat: the parameters in PARAM_ORDER (478342 floats for the value net, TM_DISTNET_PARAMS(atoms) for the head)"""
        sd = self.model.state_dict()
        off = 0
        flat = torch.as_tensor(flat, dtype=torch.float32)
        for k in self.PARAM_ORDER:
            n = sd[k].numel()
            sd[k].copy_(flat[off:off + n].reshape(sd[k].shape))
            off += n
        assert off == flat.numel()
        self.weights_changed()

    def _ensure_scratch(self, n):
        if self._scratch is None or self._scratch.shape[0] < n or self._scratch.shape[1] < self.SCRATCH_ROW:
            self._scratch = torch.zeros(n, self.SCRATCH_ROW, dtype=torch.float32, device=self.device)
        return self._scratch

    def _ensure_prepared(self):
        """the mode's one buffer, one prepare call; a buffer prepared for a larger mode serves (the parts are prefixes)"""
        total = self._prepared_floats()
        if self._prepared is None or self._prepared.numel() < total:
            prep = torch.empty(total, dtype=torch.float32, device=self.device)
            _lib.check(getattr(_lib.lib(), self.PREPARE)(_p(self.flat_params()), _p(prep), *self._mode(), _stream()), self.PREPARE)
            self._prepared = prep
        return self._prepared

    @torch.no_grad()
    def hip_buffers(self, n_states):
        """(params, the mode's prepared buffer, scratch for n_states) as ctypes pointers for the C ABI (search.hip)"""
        scratch = self._ensure_scratch(n_states)      # (allocated first, then the blob, then the prepared buffer)
        return _p(self.flat_params()), _p(self._ensure_prepared()), _p(scratch)


class Model_VV(_HipHead):
    """Inference-side mirror of the reference's Model_VV (load / inference / training(False))."""
    PARAM_ORDER, SCRATCH_ROW, PREPARE = PARAM_ORDER, SCRATCH_MFMA, "tm_valuenet_prepare"
    fisher = ewc_anchor = None      # compute_fisher's, or a checkpoint's: what train_data(ewc_lambda=) penalises against

    def __init__(self, backend="hip", device="cuda", seed=None, fc1="fp32", **kwargs):
        if fc1 not in VALUENET_FC1:
            raise ValueError("Model_VV: fc1 is 'fp32' or 'bf16x3', not %r" % (fc1,))
        if fc1 == "bf16x3" and backend != "hip_bf16x3":
            raise ValueError("Model_VV: fc1='bf16x3' belongs to backend='hip_bf16x3', not %r" % (backend,))
        if seed is not None:
            torch.manual_seed(seed)
        self.fc1 = fc1
        self.device = torch.device(device)
        self.model = Net().to(self.device).eval()
        self.backend = backend
        self.weights_changed()
        self._scratch = None         # "hip": rows of SCRATCH_MFMA floats (k_vn_fc1's per-tile counters live in their padding; every evaluation clears them)
        self._scratch_plain = None   # "hip_plain": its own buffer - never handed to the matrix-core kernels

    def training(self, mode=True):
        self.model.train(mode)

    def _mode(self):
        # ("torch", "hip_plain": the fp32 kernels, as inference_requests and hip_buffers always ran there)
        return VALUENET_BACKEND.get(self.backend, 0), VALUENET_FC1[self.fc1]

    def _prepared_floats(self):
        return PREPARED + (PREPARED_X3 if self.backend == "hip_bf16x3" else 0) + (PREPARED_FC1_X3 if self.fc1 == "bf16x3" else 0)

    def weights_changed(self):
        """... and the tree engine's per-observation outputs filed under the old weights are not used"""
        super().weights_changed()
        self.weights_epoch = next_weights_epoch()

    # ---- training side (model/model.py:97-249, model_vv.py:125-134,227-231) ----
    def _optimizer(self):
        if getattr(self, "optimizer", None) is None:
            from .train import Yogi
            # all 12 parameters in one group, out_ubound / out_lbound included, as model_vv.py:132 does
            # (Yogi(self.model.parameters(), ...)): a checkpoint's optimizer_state_dict then loads on either side
            self.optimizer = Yogi(self.model.parameters(), lr=1e-3, eps=1e-3, weight_decay=1e-3)
        return self.optimizer

    def train_data(self, data, ewc_lambda=None, **kwargs):
        """data: [states [n,1,20,10], values [n,1], variances [n,1], weights [n,1]] (numpy or tensors); fit_backend,
        validation_backend and state_format as train.train_data describes them (state_format="packed": data[0] holds the packed
        observations, int32 [n,12] on the GPU, and is passed on as it is).  ewc_lambda: None, or the lambda of elastic weight
        consolidation against this model's Fisher and anchor (compute_fisher's or a checkpoint's; train.train_data's `ewc`,
        fit_backend="hip"); a model that holds no Fisher logs one line and fits unpenalised, as on the first cycle."""
        from . import train as T
        dev = self.device
        if ewc_lambda is not None:
            import math
            from sys import stderr
            if isinstance(ewc_lambda, bool) or not isinstance(ewc_lambda, (int, float)) or not (math.isfinite(ewc_lambda) and ewc_lambda >= 0):
                raise ValueError("Model_VV.train_data: ewc_lambda must be finite and >= 0, not %r" % (ewc_lambda,))
            if kwargs.get("fit_backend", "torch") != "hip":
                raise ValueError("Model_VV.train_data: ewc_lambda needs fit_backend='hip'")
            if "ewc" in kwargs:
                raise ValueError("Model_VV.train_data: give ewc_lambda or ewc, not both")
            if self.fisher is None:
                print("Model_VV.train_data: no Fisher to consolidate against (first cycle?): fitting without the penalty",
                      file=stderr, flush=True)
            else:
                kwargs["ewc"] = dict(fisher=self.fisher, anchor=self.ewc_anchor, lam=float(ewc_lambda))
        packed = kwargs.get("state_format", "dense") == "packed"
        T.check_state_format(kwargs.get("state_format", "dense"), kwargs.get("fit_backend", "torch"),
                             kwargs.get("validation_backend", "torch"), kwargs.get("validation_fraction", 0.1), data)
        if kwargs.get("fit_backend") == "hip_dist":
            raise ValueError("Model_VV.train_data: fit_backend='hip_dist' is the distributional head's gradient step "
                             "('hip' is the value net's)")
        if kwargs.get("validation_backend", "torch") == "hip" and kwargs.get("fit_backend", "torch") != "hip":
            raise ValueError("Model_VV.train_data: validation_backend='hip' needs fit_backend='hip'")
        data = [d if packed and i == 0 else torch.as_tensor(d, dtype=torch.float32, device=dev) for i, d in enumerate(data)]
        with torch.no_grad():
            self.model.out_ubound.copy_(torch.stack([data[1].max(), data[2].max()]))   # model_vv.py:228-229
        best = {}

        def save():
            best["model"] = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
            from . import dist as tdist
            if tdist.rank() == 0:      # replicas are identical: one checkpoint file, written by rank 0
                self.save(verbose=False)

        def load():
            self.model.load_state_dict(best["model"])
        res = T.train_data(self.model, self._optimizer(), data, save=save, load=load, **kwargs)
        self.model.eval()
        self.weights_changed()
        return res

    def _flat_learnable(self):
        """a fresh flat float32 copy of the ten learnable tensors in PARAM_ORDER: what tm_valuenet_fit_grad calls params"""
        sd = self.model.state_dict()
        return torch.cat([sd[k].detach().reshape(-1).float() for k in PARAM_ORDER[:10]]).contiguous()

    @torch.no_grad()
    def compute_fisher(self, data, weighted=False, state_format="dense", slab=1024):
        """The empirical Fisher diagonal of the fit's loss over the rows of `data`, F[i] = (1/n) sum_b (d loss_b / d p_i)^2, by
        ONE call of tm_valuenet_fit_fisher (csrc/valuenet_fit.hip; the reference's Model_VV.compute_fisher, model_vv.py:188-208,
        one backward per row there).  data: [states, values, variances, weights] laid out as for train_data, device tensors (or
        anything torch.as_tensor takes); with state_format="packed" data[0] holds the packed observations, int32 [n,12] on the
        GPU.  weighted: the row's weight multiplies its loss, the weights taken AS GIVEN (train_data divides its weights by their
        mean before it fits: hand over those to get the Fisher of the loss it fitted).  slab: rows per launch sequence; the
        result does not depend on a slab >= n.  Sets self.fisher (flat float32 [478338] on the device, PARAM_ORDER[:10]) and
        self.ewc_anchor (a copy of the flat learnable weights as they stand) and returns self.fisher.  The optimiser and the
        weights are not touched."""
        from . import train as T
        dev = self.device
        if dev.type != "cuda":
            raise ValueError("Model_VV.compute_fisher runs the HIP Fisher pass: the model must be on the GPU, not %s" % (dev,))
        if state_format not in ("dense", "packed"):
            raise ValueError("state_format must be 'dense' or 'packed', not %r" % (state_format,))
        if len(data) != 4:
            raise ValueError("Model_VV.compute_fisher needs data = [states, values, variances, weights]")
        if state_format == "packed":
            fault = T._packed_states_fault(data[0])
            if fault:
                raise ValueError("state_format='packed' needs " + fault)
            states, n, name = data[0].contiguous(), data[0].shape[0], "tm_valuenet_fit_fisher_packed"
        else:
            s = torch.as_tensor(data[0], device=dev)
            n = s.shape[0]
            if n < 1 or s.numel() != n * 200:
                raise ValueError("Model_VV.compute_fisher needs states of 20 x 10 cells a row, got shape %s" % (tuple(s.shape),))
            if not bool(((s == s.round()) & (s.abs() <= 127)).all()):
                raise ValueError("Model_VV.compute_fisher reads the states as int8: they must be integers in [-127, 127]")
            states, name = s.reshape(n, 200).to(torch.int8).contiguous(), "tm_valuenet_fit_fisher"
        if n < 1:
            raise ValueError("Model_VV.compute_fisher needs at least one row")
        value, variance, weight = (torch.as_tensor(d, dtype=torch.float32, device=dev).reshape(-1).contiguous() for d in data[1:])
        if any(t.numel() != n for t in (value, variance, weight)):
            raise ValueError("Model_VV.compute_fisher needs one value, variance and weight a row")
        slab = int(slab)
        n_ws = _lib.lib().tm_valuenet_fit_fisher_workspace(slab)
        if n_ws < 0:
            raise ValueError("Model_VV.compute_fisher: a slab of %d rows is refused" % slab)
        P = self._flat_learnable()
        bounds = torch.cat([self.model.out_ubound.detach().reshape(2), self.model.out_lbound.detach().reshape(2)]).float().contiguous()
        ws = torch.empty(n_ws, dtype=torch.float32, device=dev)
        fisher = torch.empty(P.numel(), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(getattr(_lib.lib(), name)(_p(P), _p(bounds), _p(states), _p(value), _p(variance), _p(weight), None, n, slab,
                                                 int(bool(weighted)), float(variance_bound), _p(fisher), _p(ws), _stream()), name)
        self.fisher, self.ewc_anchor = fisher, P
        return self.fisher

    def _ewc_dict(self, flat):
        """a flat [478338] tensor as {parameter name: CPU tensor shaped like the parameter}"""
        sd, out, off = self.model.state_dict(), OrderedDict(), 0
        for k in PARAM_ORDER[:10]:
            n = sd[k].numel()
            out[k] = flat[off:off + n].detach().reshape(sd[k].shape).cpu().clone()
            off += n
        return out

    def _ewc_flat(self, d, key):
        sd = self.model.state_dict()
        for k in PARAM_ORDER[:10]:
            if k not in d or tuple(d[k].shape) != tuple(sd[k].shape):
                raise ValueError("checkpoint key %r: %s has shape %s, the net's is %s"
                                 % (key, k, tuple(d[k].shape) if k in d else None, tuple(sd[k].shape)))
        return torch.cat([d[k].reshape(-1).float() for k in PARAM_ORDER[:10]]).to(self.device).contiguous()

    def load(self, filename=EXP_PATH + "model_checkpoint", verbose=True):
        if os.path.isfile(filename):
            if verbose:
                print("Loading model...", flush=True)
            ck = torch.load(filename, map_location=self.device)
            self.model.load_state_dict(ck["model_state_dict"])
            if ck.get("optimizer_state_dict"):
                try:
                    self._optimizer().load_state_dict(ck["optimizer_state_dict"])
                except (ValueError, KeyError) as e:
                    from sys import stderr
                    print("WARNING: optimizer state of %s not loaded (%s): the optimiser restarts with fresh moments"
                          % (filename, e), file=stderr, flush=True)
            # the Fisher and its anchor, when the checkpoint carries them (both or neither)
            self.fisher = self.ewc_anchor = None
            if "fisher" in ck and "ewc_anchor" in ck:
                self.fisher, self.ewc_anchor = self._ewc_flat(ck["fisher"], "fisher"), self._ewc_flat(ck["ewc_anchor"], "ewc_anchor")
        elif verbose:
            print("Checkpoint not found, using default model", flush=True)
        self.weights_changed()

    def save(self, filename=EXP_PATH + "model_checkpoint", verbose=True):
        if verbose:
            print("Saving model...", flush=True)
        os.makedirs(os.path.dirname(filename) or ".", exist_ok=True)
        # the reference's Model.load indexes optimizer_state_dict['param_groups'] (model.py:166-170): always write a real one
        ck = {"model_state_dict": self.model.state_dict(), "optimizer_state_dict": self._optimizer().state_dict()}
        if self.fisher is not None:      # (a model without a Fisher writes exactly those two keys)
            ck["fisher"], ck["ewc_anchor"] = self._ewc_dict(self.fisher), self._ewc_dict(self.ewc_anchor)
        torch.save(ck, filename)

    @torch.no_grad()
    def inference_device(self, states, v_out=None, var_out=None):
        """states: int8 [B,200] (or [B,20,10]) on the device -> (v[B], var[B]) float32 device tensors."""
        B = states.shape[0]
        if v_out is None:
            v_out = torch.empty(B, dtype=torch.float32, device=self.device)
            var_out = torch.empty(B, dtype=torch.float32, device=self.device)
        if self.backend in HIP_BACKENDS:
            P, prep, scr = self.hip_buffers(B)
            _lib.check(_lib.lib().tm_valuenet_forward(P, prep, *self._mode(), _p(states), B, _p(v_out), _p(var_out), scr,
                                                      _stream()), "tm_valuenet_forward")
        elif self.backend == "hip_plain":
            if self._scratch_plain is None or self._scratch_plain.shape[0] < B:
                self._scratch_plain = torch.empty(B, 9728, dtype=torch.float32, device=self.device)
            _lib.check(_lib.lib().tm_valuenet_forward_plain(_p(self.flat_params()), _p(states), B, _p(v_out), _p(var_out),
                                                            _p(self._scratch_plain), _stream()), "tm_valuenet_forward_plain")
        else:
            out = self.model(states.reshape(B, 1, 20, 10).float())
            v_out.copy_(out[:, 0])
            var_out.copy_(out[:, 1])
        return v_out, var_out

    @torch.no_grad()
    def inference_requests(self, store):
        """Evaluate a TreeStore's pending leaf requests in place (fused render + forward, HIP back ends only).  Enqueues only; the
        fp32 mode's one-launch kernel reports a wait that ran out in a sticky word (fused_wait_failed, after a synchronisation)."""
        P, prep, scr = self.hip_buffers(store.n_games * store.eval_slots)
        _lib.check(_lib.lib().tm_valuenet_forward_requests(P, prep, *self._mode(), C.byref(store.s), scr, _stream()),
                   "tm_valuenet_forward_requests")

    @staticmethod
    def fused_wait_failed(reset=True):
        """True once a launch of the one-launch kernel gave up its bounded wait (tm_valuenet_fused_error): what it left in eval_v /
        eval_var is not an evaluation.  Call when the stream is idle."""
        return _lib.lib().tm_valuenet_fused_error(int(bool(reset))) != 0

    def inference(self, batch):
        """Reference signature (model_vv.py:210-217): float array [B,1,20,10] -> [v[B,1], var[B,1]] numpy."""
        b = torch.as_tensor(batch).to(self.device)
        B = b.shape[0]
        v, var = self.inference_device(b.reshape(B, 200).to(torch.int8).contiguous())
        return [v.cpu().numpy().reshape(B, 1), var.cpu().numpy().reshape(B, 1)]
