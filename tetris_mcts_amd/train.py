"""Online TD training of the value net — the reference's learning half, as plain PyTorch on
the GPU (plumbing, not a hot kernel):

  * Yogi optimiser                      model/yogi.py:39-90   (lr 1e-3, eps 1e-3, weight decay 1e-3: model_vv.py:132)
  * Gaussian KL / likelihood loss       model/model_vv.py:94-101,136-150 (variance clipped at 0.1, optional weights)
  * Model.train_data                    model/model.py:176-249 (weights / mean, last 10 % validation, random minibatches
                                        with replacement, validation every `iters_per_val`, early stopping with patience,
                                        best-checkpoint reload)
  * Model_VV.train_data                 model/model_vv.py:227-231 (output upper bounds = data maxima)
  * checkpoint format                   model/model.py:143-174 ({'model_state_dict', 'optimizer_state_dict'})
"""
import math
from sys import stderr

import torch
from torch.optim.optimizer import Optimizer

variance_bound = 1e-1


class _FlatBuffers:
    """The fused surface Yogi and FusedAdam share: the parameters that take gradients, their gradients and the moments named by
    `_MOMENTS` as views of flat buffers (`_flat`: params, n, p, g, m, v[, vmax], state, t), stepped by ONE HIP kernel with the
    step count on the device.  A subclass names itself (`_NAME`, for the messages) and its moments, says how its state dict keeps
    a step count (`_step_value`), and makes the C call (`_launch`)."""
    _NAME, _MOMENTS = None, ()

    def _fusable(self):
        ps = [p for g in self.param_groups for p in g["params"] if p.requires_grad]
        return (len(self.param_groups) == 1 and len(ps) > 0 and all(p.is_cuda and p.dtype == torch.float32 for p in ps)
                and len({p.device for p in ps}) == 1)

    def fused(self):
        """whether step() is the one-kernel form: every parameter on one GPU, float32, a single group (or asked for / refused
        at construction)"""
        if self._fused_wanted is False:
            return False
        ok = self._fusable()
        if self._fused_wanted and not ok:
            raise ValueError(self._NAME + "(fused=True) needs float32 parameters on one GPU in a single group")
        return ok

    def _takes_flat_route(self):
        """whether zero_grad and state_dict go through the flat buffers"""
        return self._flat is not None

    def flatten(self):
        """(idempotent) the parameters that take gradients, their gradients and moments as views of flat buffers, in the order
        the parameters were given"""
        if self._flat is not None:
            return self._flat
        ps = [p for p in self.param_groups[0]["params"] if p.requires_grad]
        dev, n = ps[0].device, sum(p.numel() for p in ps)
        moments = list(zip(("m", "v", "vmax"), self._MOMENTS))
        F = dict(params=ps, n=n, p=torch.empty(n, device=dev), g=torch.zeros(n, device=dev))
        F.update((key, torch.zeros(n, device=dev)) for key, _ in moments)
        F["state"] = torch.zeros(8, dtype=torch.float64, device=dev)
        off, steps = 0, set()
        with torch.no_grad():
            for p in ps:
                k = p.numel()
                sl = slice(off, off + k)
                F["p"][sl].copy_(p.reshape(-1))
                p.data = F["p"][sl].view_as(p)
                if p.grad is not None:
                    F["g"][sl].copy_(p.grad.reshape(-1))
                p.grad = F["g"][sl].view_as(p)
                st = self.state[p]
                if st:       # moments loaded from a state dict (or steps taken by the per-tensor form)
                    for key, name in moments:
                        if key != "vmax" or name in st:      # (torch's Adam keeps no maximum unless amsgrad is set)
                            F[key][sl].copy_(st[name].reshape(-1))
                    steps.add(int(st["step"]))
                for key, name in moments:
                    st[name] = F[key][sl].view_as(p)
                st["step"] = self._step_value(st.get("step", 0))
                off += k
        if len(steps) > 1:
            raise ValueError("%s: the parameters' step counts differ (%s)" % (self._NAME, sorted(steps)))
        t = steps.pop() if steps else 0
        b1, b2 = self.param_groups[0]["betas"]
        lr = self.param_groups[0]["lr"]
        if t > 0:
            F["state"].copy_(torch.tensor([t, b1 ** t, b2 ** t, lr / (1 - b1 ** t), math.sqrt(1 - b2 ** t), 0, 0, 0], dtype=torch.float64))
        F["t"] = t
        self._flat = F
        return F

    def flat_grad(self):
        return self.flatten()["g"] if self.fused() else None

    def zero_grad(self, set_to_none=True):
        if self._takes_flat_route():
            self._flat["g"].zero_()      # (the gradients stay the views they are: autograd accumulates into them in place)
            return
        super().zero_grad(set_to_none=set_to_none)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        if self._flat is not None:       # the loaded moments are tensors of their own: back into the flat buffers
            ps = self._flat["params"]
            with torch.no_grad():
                for p in ps:
                    p.data = p.data.clone()
                    p.grad = None
            self._flat = None
            self.flatten()

    def state_dict(self):
        if self._takes_flat_route():
            for p in self._flat["params"]:
                self.state[p]["step"] = self._step_value(self._flat["t"])
        return super().state_dict()

    def _fused_step(self):
        from . import _lib
        F = self.flatten()
        self._launch(_lib, F, self.param_groups[0], torch.cuda.current_stream(F["p"].device).cuda_stream)
        F["t"] += 1


class Yogi(_FlatBuffers, Optimizer):
    """Yogi (Zaheer et al. 2018) with the reference's conventions: v0 = g0^2 (before weight decay), coupled weight
    decay added to the gradient, bias-corrected step  p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps).

    Parameters on the GPU: the step is ONE HIP kernel over flat buffers (csrc/yogi.hip `tm_yogi_step`: the same operations per
    element in the same order) - the parameters, their gradients and the two moments become views of four flat tensors at the
    first step (`flatten`), the step count lives on the device, and an iteration of the fit is a fixed sequence of launches
    that train_data replays from a HIP graph.  The state dict keeps the reference's layout (per parameter: step, exp_avg,
    exp_avg_sq), so checkpoints load on either side.  Parameters on the CPU: the reference's own sequence of tensor operations."""
    _NAME, _MOMENTS = "Yogi", ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr=1e-2, betas=(0.9, 0.999), eps=1e-3, weight_decay=0.0, fused=None):
        if lr <= 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1):
            raise ValueError("invalid Yogi hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._fused_wanted = fused
        self._flat = None

    @staticmethod
    def _step_value(t):
        return t      # the reference's layout: an int

    def _launch(self, _lib, F, g, stream):
        _lib.check(_lib.lib().tm_yogi_step(F["p"].data_ptr(), F["g"].data_ptr(), F["m"].data_ptr(), F["v"].data_ptr(),
                                           F["state"].data_ptr(), F["n"], float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]),
                                           float(g["eps"]), float(g["weight_decay"]), stream), "tm_yogi_step")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.fused():
            self._fused_step()
            return loss
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = p.grad
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p)
                    st["exp_avg_sq"] = g * g
                st["step"] += 1
                t = st["step"]
                # the reference's own sequence of tensor primitives (model/yogi.py:69-88), so parameter trajectories are
                # bit-identical to it (tests/golden/ref_training.npz)
                if group["weight_decay"] != 0:
                    g = g.add(p, alpha=group["weight_decay"])
                m, v = st["exp_avg"], st["exp_avg_sq"]
                m.mul_(b1).add_(g, alpha=1 - b1)
                g2 = g.mul(g)
                v.addcmul_(torch.sign(v - g2), g2, value=-(1 - b2))
                denom = (v.sqrt() / math.sqrt(1 - b2 ** t)).add_(group["eps"])
                p.addcdiv_(m, denom, value=-(group["lr"] / (1 - b1 ** t)))
        return loss


class FusedAdam(_FlatBuffers, torch.optim.Adam):
    """torch.optim.Adam (AMSGrad and coupled weight decay included) with Yogi's fused surface, for the distributional head's fit.

    Parameters on the GPU: the step is ONE HIP kernel over flat buffers (csrc/yogi.hip `tm_adam_step`: torch's single-tensor step
    per element, fp32, in its order of operations) - the parameters, their gradients and the three moments become views of five
    flat tensors at the first step (`flatten`, in the order the parameters were given: model_distributional.PARAM_ORDER for
    Net.parameters()), the step count lives on the device, and train_data replays an iteration from a HIP graph.  The state dict
    is torch.optim.Adam's (per parameter: step, exp_avg, exp_avg_sq, max_exp_avg_sq), so a state saved by either loads into the
    other.  Parameters on the CPU: torch's own step (this class IS torch.optim.Adam there: the same bits)."""
    _NAME, _MOMENTS = "FusedAdam", ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, fused=None):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad)
        self._fused_wanted = fused
        self._flat = None

    def _fusable(self):
        """as Yogi's, and torch's plain options"""
        g0 = self.param_groups[0]
        return (super()._fusable() and not g0.get("maximize") and not g0.get("decoupled_weight_decay")
                and not isinstance(g0["lr"], torch.Tensor) and g0["betas"][0] > 0.5)

    def _takes_flat_route(self):
        """In the fused form the gradients are zeroed, never cleared: they stay the views of the flat buffer that autograd
        accumulates into and the kernel reads, so EVERY parameter is stepped in every iteration (one that received no gradient
        moves by its momentum, where torch.optim.Adam would skip it; Net's eight tensors always receive one).  Anywhere else
        (CPU parameters, flattened or not) zero_grad and state_dict are torch.optim.Adam's."""
        return self._flat is not None and self.fused()

    @staticmethod
    def _step_value(t):
        return torch.tensor(float(t))      # torch.optim.Adam's layout: a 0-d float tensor

    def _launch(self, _lib, F, g, stream):
        _lib.check(_lib.lib().tm_adam_step(F["p"].data_ptr(), F["g"].data_ptr(), F["m"].data_ptr(), F["v"].data_ptr(),
                                           F["vmax"].data_ptr(), F["state"].data_ptr(), F["n"], float(g["lr"]), float(g["betas"][0]),
                                           float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]), int(bool(g["amsgrad"])),
                                           stream), "tm_adam_step")

    def step(self, closure=None):
        if not self.fused():
            return super().step(closure)      # torch.optim.Adam itself (on flattened CPU parameters too: the views are its state)
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        with torch.no_grad():
            self._fused_step()
        return loss


def gaussian_kl(var_pred, mean_pred, var, mean):
    """KL( N(mean,var) || N(mean_pred,var_pred) ) up to the factor 1/2 the reference also drops."""
    return var_pred.log() + ((mean - mean_pred) ** 2 + var) / var_pred - var.log() - 1.0


def batch_loss(net, batch, weighted, variance_clip=variance_bound):
    state, value, variance, weight = batch
    variance = variance.clamp(min=variance_clip)
    out = net(state)
    v, var = out[:, 0:1], out[:, 1:2]
    per = gaussian_kl(var, v, variance, value)
    if weighted:
        per = weight * per
    std, mean = torch.std_mean(per, unbiased=False)      # model_vv.py:146-149 (one fused reduction: same bits as the reference)
    return mean, std


@torch.no_grad()
def validation_loss(net, data, weighted, chunk=1024, loss_fn=None):
    """Weighted combination over chunks (model.py:49-84): chunk weight = sum of sample weights (or the count).  The chunks'
    (weight, mean, std) stay on the device until the last one is in: ONE host synchronisation per validation (r05: three per
    chunk, ~150 per validation of a 50 000-tuple set)."""
    loss_fn = loss_fn or batch_loss
    rows = []
    for c in range(0, data[0].shape[0], chunk):
        b = [d[c:c + chunk] for d in data]
        mean, std = loss_fn(net, b, weighted)
        w = b[-1].sum() if weighted else torch.full((), float(b[0].shape[0]), device=mean.device)
        rows.append(torch.stack([w.to(torch.float64), mean.to(torch.float64), std.to(torch.float64)]))
    return combine_chunk_rows(torch.stack(rows).cpu().tolist())


def combine_chunk_rows(rows):
    """(mean, std) of a validation set from its chunks' [w, mean, std] (Python floats): the reference's arithmetic, in Python
    doubles as there.  Both validation backends end here - "torch" with the rows validation_loss collected, "hip" with the rows
    tm_valuenet_fit_validate / tm_distnet_fit_validate wrote."""
    tot_w, acc, acc2 = 0.0, 0.0, 0.0
    for w, mean, std in rows:
        if math.isnan(std):
            std = 0.0
        tot_w += w
        acc += w * mean
        acc2 += w * (std * std + mean * mean)
    mean = acc / tot_w
    return mean, math.sqrt(max(acc2 / tot_w - mean * mean, 0.0))


def check_data_parallel_batch(batch_size, world):
    """Equal shards only: the average of the ranks' shard means is then the batch mean (with unequal shards it is not, and
    a rank with an empty shard would feed NaN into the all-reduce)."""
    if world > 1 and batch_size % world:
        raise ValueError("data-parallel training needs batch_size (%d) to be a multiple of the number of ranks (%d)"
                         % (batch_size, world))


def flat_order_is_param_order(net, optimizer):
    """Whether Yogi's flat buffers hold exactly the ten learnable tensors of model.Net in model.PARAM_ORDER - the layout
    tm_valuenet_fit_grad reads its parameters in and writes its gradient in."""
    from .model import PARAM_ORDER
    named = dict(net.named_parameters())
    want = [named.get(k) for k in PARAM_ORDER[:10]]
    got = optimizer.flatten()["params"]
    return (all(w is not None for w in want) and len(got) == len(want) and all(a is b for a, b in zip(got, want))
            and not any(named[k].requires_grad for k in PARAM_ORDER[10:] if k in named))


# validation_backend="hip": the chunk is validation_loss's (the chunks' rows feed the same host combination), the slab the
# number of rows forwarded per launch sequence (DESIGN 3.3 has the measurement behind it; the result does not depend on it)
VALIDATION_CHUNK = 1024
VALIDATION_SLAB = 4096


def _validation_slab(rows, chunk, slab):
    """the slab of a validation pass over `rows` rows: a multiple of `chunk`, no larger than the rows need"""
    if chunk < 1 or slab < chunk or slab % chunk:
        raise ValueError("validation_backend='hip' needs slab >= chunk >= 1 and a slab that is a multiple of the chunk, got "
                         "chunk %d, slab %d" % (chunk, slab))
    return min(slab, (rows + chunk - 1) // chunk * chunk)


def _packed_states_fault(states):
    """why `states` is not what state_format='packed' reads (None when it is): the observations as the engine harvests them,
    int32 [n,12] on the GPU (ENGINE_SPEC section 7)"""
    if not isinstance(states, torch.Tensor) or states.dtype != torch.int32:
        return "int32 observations, got %s" % (getattr(states, "dtype", type(states).__name__),)
    if states.dim() != 2 or states.shape[1] != 12:
        return "observations of 12 words a row, got shape %s" % (tuple(states.shape),)
    if not states.is_cuda:
        return "the observations on the GPU (they are on %s)" % (states.device,)
    return None


def check_state_format(state_format, fit_backend, validation_backend, validation_fraction, data):
    """The refusals of train_data's `state_format`, a ValueError that names the option, raised before the model, the optimiser
    or a sampling stream is touched (train_data and the models' train_data call it first)."""
    if state_format not in ("dense", "packed"):
        raise ValueError("state_format must be 'dense' or 'packed', not %r" % (state_format,))
    if state_format == "dense":
        return
    if fit_backend not in ("hip", "hip_dist"):
        raise ValueError("state_format='packed': only the HIP gradient steps read packed observations, it needs fit_backend='hip' "
                         "or 'hip_dist', not %r" % (fit_backend,))
    rows = len(data[0]) if hasattr(data[0], "__len__") else 0
    if validation_backend != "hip" and int(rows * validation_fraction) > 0:
        raise ValueError("state_format='packed': the torch validation does not read packed observations, it needs "
                         "validation_backend='hip' or a validation_fraction that holds no rows out")
    fault = _packed_states_fault(data[0])
    if fault:
        raise ValueError("state_format='packed' needs " + fault)


EWC_PARAMS = 478338      # the learnable floats of model.Net in model.PARAM_ORDER[:10]: the length of a Fisher and of its anchor


def check_ewc(ewc, fit_backend):
    """The refusals of train_data's `ewc`, a ValueError raised with the other early checks (before the optimiser is flattened).
    ewc: None or dict(fisher=, anchor=, lam=); returns (fisher, anchor, lam) with contiguous tensors, or None."""
    if ewc is None:
        return None
    if fit_backend != "hip":
        raise ValueError("ewc adds its penalty to the flat gradient of the value net's HIP fit: it needs fit_backend='hip', not %r"
                         % (fit_backend,))
    if not isinstance(ewc, dict) or set(ewc) != {"fisher", "anchor", "lam"}:
        raise ValueError("ewc is None or dict(fisher=, anchor=, lam=)")
    for key in ("fisher", "anchor"):
        t = ewc[key]
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.numel() == EWC_PARAMS):
            raise ValueError("ewc: %s must be a float32 CUDA tensor of %d elements" % (key, EWC_PARAMS))
    try:
        lam = float(ewc["lam"])
    except (TypeError, ValueError):
        raise ValueError("ewc: lam must be a number, not %r" % (ewc["lam"],)) from None
    if not (math.isfinite(lam) and lam >= 0.0):
        raise ValueError("ewc: lam must be finite and >= 0, not %r" % (ewc["lam"],))
    return ewc["fisher"].reshape(-1).contiguous(), ewc["anchor"].reshape(-1).contiguous(), lam


def check_ewc_dist(ewc_dist, fit_backend, net):
    """check_ewc for the distributional head: the refusals of train_data's `ewc_dist`, raised with the other early checks.
    ewc_dist: None or dict(fisher=, anchor=, lam=) with float32 CUDA tensors of the 279232 + 129 atoms flat parameters of `net`
    (model_distributional.PARAM_ORDER); returns (fisher, anchor, lam) with contiguous tensors, or None."""
    if ewc_dist is None:
        return None
    if fit_backend != "hip_dist":
        raise ValueError("ewc_dist adds its penalty to the flat gradient of the distributional head's HIP fit: it needs "
                         "fit_backend='hip_dist', not %r" % (fit_backend,))
    atoms = getattr(getattr(getattr(net, "seq", None), "fc_v", None), "out_features", None)
    if not isinstance(atoms, int):
        raise ValueError("ewc_dist: fit_backend='hip_dist' computes model_distributional.Net, not %s" % type(net).__name__)
    if not isinstance(ewc_dist, dict) or set(ewc_dist) != {"fisher", "anchor", "lam"}:
        raise ValueError("ewc_dist is None or dict(fisher=, anchor=, lam=)")
    n = HipDistFit.N_PARAMS_0 + 129 * atoms
    for key in ("fisher", "anchor"):
        t = ewc_dist[key]
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.numel() == n):
            raise ValueError("ewc_dist: %s must be a float32 CUDA tensor of %d elements (%d atoms)" % (key, n, atoms))
    try:
        lam = float(ewc_dist["lam"])
    except (TypeError, ValueError):
        raise ValueError("ewc_dist: lam must be a number, not %r" % (ewc_dist["lam"],)) from None
    if not (math.isfinite(lam) and lam >= 0.0):
        raise ValueError("ewc_dist: lam must be finite and >= 0, not %r" % (ewc_dist["lam"],))
    return ewc_dist["fisher"].reshape(-1).contiguous(), ewc_dist["anchor"].reshape(-1).contiguous(), lam


class _HipFitBase:
    """What the per-fit states of fit_backend="hip" and "hip_dist" share: the order of the checks (once per fit, everything that
    can refuse before the optimiser is flattened), the workspaces of the gradient step and of the validation pass, the index
    check and the two calls.  A subclass names its backend (`BACKEND`, for the messages), checks the net, the optimiser and one
    list of rows (`_check`, `_check_rows`, `_check_flat`), keeps its copies of the rows (`_keep`) and makes the C calls
    (`_workspace`, `_grad`, `_validate`).

    state_format="packed": the first array of `train` and of `val` holds the packed observations (int32 [rows,12]) in place
    of rendered states.  The kernels give every bit pattern a meaning, so the rows' check is of dtype, shape and device alone,
    the rows are kept as they are (a contiguous view: no copy of contiguous rows), and the calls are the `_packed` entry points,
    whose outputs are the bits of the int8 ones on the rendered rows."""
    BACKEND = None

    def __init__(self, net, optimizer, train, batch, val=None, val_chunk=VALIDATION_CHUNK, val_slab=VALIDATION_SLAB,
                 state_format="dense", ewc=None):
        from . import _lib
        self._lib = _lib
        self.ewc = self._check_ewc(net, ewc)
        if state_format not in ("dense", "packed"):
            raise ValueError("state_format must be 'dense' or 'packed', not %r" % (state_format,))
        self.packed = state_format == "packed"
        L, V = "fit_backend='%s'" % self.BACKEND, "validation_backend='hip'"
        rows = self._check(net, optimizer, train, L)
        if val is not None:      # validation_backend="hip": the same checks on the held-out rows, before the optimiser is touched
            vrows = self._check_rows(val, V, "validation data")
            val_slab = _validation_slab(vrows, val_chunk, val_slab)
            if self._workspace(val_slab, validation=True) < 0:
                raise ValueError(V + ": a slab of %d rows is refused" % val_slab)
        if self.ewc is not None and any(t.device != train[0].device for t in self.ewc[:2]):
            raise ValueError(L + ": ewc's fisher and anchor must be on %s, where the data is" % (train[0].device,))
        F = optimizer.flatten()
        self._check_flat(net, optimizer, F, train[0].device, L)
        if batch < 1:
            raise ValueError(L + " needs a batch of at least one row per rank")
        self.F, self.batch, self.rows, self.dev = F, batch, rows, train[0].device
        self._keep(train, rows, "")
        n_ws = self._workspace(batch)
        if n_ws < 0:
            raise ValueError(L + ": a batch of %d rows is refused" % batch)
        self.ws = torch.empty(n_ws, dtype=torch.float32, device=self.dev)
        self.loss = torch.zeros(2, dtype=torch.float32, device=self.dev)
        if self.ewc is not None:      # the penalty's workspace and its loss (one double), once per fit
            self.ewc_ws = torch.empty(_lib.lib().tm_ewc_penalty_workspace(F["n"]), dtype=torch.float32, device=self.dev)
            self.ewc_loss = torch.zeros(1, dtype=torch.float64, device=self.dev)
        self._idx_checked = False
        self.val_rows = 0
        if val is not None:      # the int8 copy of the held-out states (once per fit), the slab's workspace and the chunks' rows
            self.val_rows, self.val_chunk, self.val_slab = vrows, val_chunk, val_slab
            self._keep(val, vrows, "val_")
            self.val_ws = torch.empty(self._workspace(val_slab, validation=True), dtype=torch.float32, device=self.dev)
            self.val_out = torch.zeros((vrows + val_chunk - 1) // val_chunk, 3, dtype=torch.float64, device=self.dev)

    def _check_ewc(self, net, ewc):
        return check_ewc(ewc, self.BACKEND)

    def validate(self, weighted):
        """the held-out rows' [w, mean, std] per chunk (a list of lists of Python floats, what combine_chunk_rows takes), at the
        optimiser's flat parameters as they stand: ONE call of tm_valuenet_fit_validate / tm_distnet_fit_validate on the current
        stream and ONE .cpu() (the head's std of a one-row chunk is NaN, as torch.std_mean's: combine_chunk_rows maps it to 0)"""
        if not self.val_rows:
            raise ValueError("validation_backend='hip': this fit holds no validation rows")
        self._validate(int(bool(weighted)), torch.cuda.current_stream(self.dev).cuda_stream)
        return self.val_out.cpu().tolist()

    def _check_packed(self, data, L, what):
        """the first array of `data` as packed observations: dtype, shape and device (no sweep over the contents)"""
        fault = _packed_states_fault(data[0]) if len(data) else "a list of arrays"
        if fault:
            raise ValueError(L + " with state_format='packed' needs " + fault + " as the " + what + "'s states")
        if data[0].shape[0] < 1:
            raise ValueError(L + " with state_format='packed' needs at least one row of " + what)

    def _fn(self, name):
        """the entry point `name` for this fit's kind of rows"""
        return getattr(self._lib.lib(), name + ("_packed" if self.packed else ""))

    def check_idx(self, idx):
        """ValueError unless every index names a training row (a host synchronisation: not inside a graph capture)"""
        lo, hi = int(idx.min()), int(idx.max())
        if lo < 0 or hi >= self.rows:
            raise ValueError("fit_backend='%s': indices in [%d, %d] do not all name one of the %d training rows"
                             % (self.BACKEND, lo, hi, self.rows))

    def grad(self, idx, weighted):
        """loss (a 0-d device tensor) of the rows idx (int64, every value in [0, rows)); the gradient of its mean lands in the
        optimiser's flat buffer.  The kernels read the rows idx names without a bounds check of their own: the first call of a
        fit that is not being captured checks the range here (one host synchronisation), and train_data's draws are indices
        into [0, rows) by construction; a caller who changes where idx comes from between calls calls check_idx itself."""
        if idx.dtype != torch.int64 or idx.numel() != self.batch:
            raise ValueError("fit_backend='%s': expected %d int64 indices, got %d %s" % (self.BACKEND, self.batch, idx.numel(), idx.dtype))
        if not self._idx_checked and not torch.cuda.is_current_stream_capturing():
            self.check_idx(idx)
            self._idx_checked = True
        self._grad(idx.contiguous(), int(bool(weighted)), torch.cuda.current_stream(self.dev).cuda_stream)
        return self.loss[0]

    def penalty(self):
        """ONE call of tm_ewc_penalty on the current stream: lam F (p - anchor) is added to the optimiser's flat gradient as it
        stands; returns the penalty 0.5 lam sum F (p - anchor)^2 (a 0-d float64 device tensor).  Needs a fit built with `ewc`."""
        fisher, anchor, lam = self.ewc
        F = self.F
        self._lib.check(self._lib.lib().tm_ewc_penalty(
            F["p"].data_ptr(), anchor.data_ptr(), fisher.data_ptr(), F["n"], lam, F["g"].data_ptr(), self.ewc_loss.data_ptr(),
            self.ewc_ws.data_ptr(), torch.cuda.current_stream(self.dev).cuda_stream), "tm_ewc_penalty")
        return self.ewc_loss[0]


class HipFit(_HipFitBase):
    """The per-fit state of fit_backend="hip": the checks (once per fit), the int8 copy of the training states, the flattened
    targets, the output bounds and the workspace; grad(idx) is one call of tm_valuenet_fit_grad on the current stream."""
    BACKEND = "hip"
    N_PARAMS = 478338

    def _check_rows(self, data, L, what):
        """the checks of one list of rows (`what`: "data", the training rows, or "validation data"); the number of rows"""
        if self.packed:
            self._check_packed(data, L, what)
            rows = data[0].shape[0]
            if len(data) != 4 or not all(d.is_cuda and d.dtype == torch.float32 for d in data[1:]):
                raise ValueError(L + " needs %s = [observations, values, variances, weights], the last three float32 CUDA tensors" % what)
            if any(t.shape[0] != rows or t.numel() != rows for t in data[1:]):
                raise ValueError(L + " needs one value, variance and weight a row")
            return rows
        rows = data[0].shape[0]
        if len(data) != 4 or rows < 1 or data[0].numel() != rows * 200:
            if what != "data":
                raise ValueError(L + " needs validation data = [states of 20 x 10 cells a row, values, variances, weights]")
            if len(data) != 4:
                raise ValueError(L + " needs data = [states, values, variances, weights]")
            raise ValueError(L + " needs states of 20 x 10 cells a row, got shape %s" % (tuple(data[0].shape),))
        if not bool(((data[0] == data[0].round()) & (data[0].abs() <= 127)).all()):
            raise ValueError(L + " reads the states as int8: they must be integers in [-127, 127]")
        if not all(d.is_cuda and d.dtype == torch.float32 for d in data):
            raise ValueError(L + " needs float32 CUDA tensors (the %s is on %s)" % (what, data[0].device))
        if any(t.shape[0] != rows or t.numel() != rows for t in data[1:]):
            raise ValueError(L + " needs one value, variance and weight a row")
        return rows

    def _check(self, net, optimizer, train, L):
        from .model import Net
        rows = self._check_rows(train, L, "data")
        if not isinstance(net, Net):
            raise ValueError(L + " computes model.Net, not %s" % type(net).__name__)
        if not (hasattr(optimizer, "fused") and optimizer.fused()):
            raise ValueError(L + " writes the fused Yogi's flat gradient buffer: the optimizer must be a Yogi "
                             "whose fused() holds (float32 parameters on one GPU in a single group)")
        self.bounds = torch.cat([net.out_ubound.detach().reshape(2), net.out_lbound.detach().reshape(2)]).float().contiguous()
        return rows

    def _check_flat(self, net, optimizer, F, dev, L):
        if F["n"] != self.N_PARAMS or not flat_order_is_param_order(net, optimizer):
            raise ValueError(L + ": the optimizer's flat buffers are not the net's learnable tensors in model.PARAM_ORDER")

    def _keep(self, data, rows, pre):
        setattr(self, pre + "states", data[0].contiguous() if self.packed else data[0].reshape(rows, 200).to(torch.int8).contiguous())
        for name, t in zip(("value", "variance", "weight"), data[1:]):
            setattr(self, pre + name, t.reshape(rows).contiguous())

    def _workspace(self, n, validation=False):
        return self._lib.lib().tm_valuenet_fit_validate_workspace(n) if validation else self._lib.lib().tm_valuenet_fit_workspace(n)

    def _validate(self, weighted, stream):
        self._lib.check(self._fn("tm_valuenet_fit_validate")(
            self.F["p"].data_ptr(), self.bounds.data_ptr(), self.val_states.data_ptr(), self.val_value.data_ptr(),
            self.val_variance.data_ptr(), self.val_weight.data_ptr(), self.val_rows, self.val_chunk, self.val_slab, weighted,
            float(variance_bound), self.val_out.data_ptr(), self.val_ws.data_ptr(), stream), "tm_valuenet_fit_validate")

    def _grad(self, idx, weighted, stream):
        F = self.F
        self._lib.check(self._fn("tm_valuenet_fit_grad")(
            F["p"].data_ptr(), self.bounds.data_ptr(), self.states.data_ptr(), self.value.data_ptr(), self.variance.data_ptr(),
            self.weight.data_ptr(), idx.data_ptr(), self.batch, weighted, float(variance_bound), F["g"].data_ptr(),
            self.loss.data_ptr(), self.ws.data_ptr(), stream), "tm_valuenet_fit_grad")


def dist_batch_loss(net, batch, weighted):
    """Model_Dist.loss as a train_data loss_fn: batch = [states [b,1,22,10], targets [b,atoms], weights [b,1]]"""
    state, value, weight = batch
    per = torch.xlogy(value, value) - value * net.log_prob(state)
    if weighted:
        per = weight.reshape(-1, 1) * per
    std, mean = torch.std_mean(per.sum(dim=1))
    return mean, std


# The mark by which train_data(fit_backend="hip_dist") recognises "the model's own loss".  It is a convention, not a check: setting it
# on a function ASSERTS that the function computes what tm_distnet_fit_grad computes (Model_Dist.loss: per sample
# w sum_a (xlogy(t, t) - t log p), mean and n-1 standard deviation over the batch).  The kernels take the training gradient either
# way; a marked function that computes something else would only make validation measure another quantity than the one fitted.
# Model_Dist.train_data's closure around Model_Dist.loss carries the mark, and so does this function; nothing else should.
dist_batch_loss.is_model_dist_loss = True


def flat_order_is_dist_param_order(net, optimizer):
    """Whether FusedAdam's flat buffers hold (or, before flatten(), will hold) exactly the eight tensors of model_distributional.Net in its PARAM_ORDER - the layout
    tm_distnet_fit_grad reads its parameters in and writes its gradient in."""
    from .model_distributional import PARAM_ORDER
    named = dict(net.named_parameters())
    want = [named.get(k) for k in PARAM_ORDER]
    # (the order flatten() WILL use, read without flattening: a refused fit leaves the optimiser and the parameters as they were)
    flat = getattr(optimizer, "_flat", None)
    got = flat["params"] if flat is not None else [p for g in optimizer.param_groups[:1] for p in g["params"] if p.requires_grad]
    return (len(optimizer.param_groups) == 1 and all(w is not None for w in want) and len(got) == len(want) == len(named)
            and all(a is b for a, b in zip(got, want)))


class HipDistFit(_HipFitBase):
    """The per-fit state of fit_backend="hip_dist" (HipFit's sibling for the distributional head): the checks (once per fit), the
    int8 copy of the 20 visible rows of the training states, the targets, the weights and the workspace; grad(idx) is one call
    of tm_distnet_fit_grad on the current stream."""
    BACKEND = "hip_dist"
    N_PARAMS_0 = 279232      # the flat parameters without fc_v's 129 an atom

    def _check_ewc(self, net, ewc):
        """`ewc` is train_data's ewc_dist here: the head's Fisher and anchor (check_ewc_dist)"""
        return check_ewc_dist(ewc, self.BACKEND, net)

    def _check_rows(self, data, L, what):
        """the checks of one list of rows (`what`: "data", the training rows, or "validation data"); the number of rows"""
        if self.packed:      # (20 board rows a row: the kernels supply the two empty rows on top, which holds the dense rule by construction)
            self._check_packed(data, L, what)
            if len(data) != 3:
                raise ValueError(L + " needs %s = [observations, targets, weights]" % what)
        rows, atoms = data[0].shape[0], self.atoms
        if not self.packed and (len(data) != 3 or rows < 1 or data[0].numel() != rows * 220):
            if what != "data":
                raise ValueError(L + " needs validation data = [states of 22 x 10 cells a row, targets, weights]")
            if len(data) != 3:
                raise ValueError(L + " needs data = [states, targets, weights]")
            raise ValueError(L + " needs states of 22 x 10 cells a row, got shape %s" % (tuple(data[0].shape),))
        states, target, weight = data
        if target.dim() != 2 or target.shape[0] != rows or target.shape[1] != atoms:
            raise ValueError(L + " needs targets [rows, atoms] = [%d, %d]%s, got %s"
                             % (rows, atoms, " as the net's atoms" if what == "data" else "", tuple(target.shape)))
        if weight.shape[0] != rows or weight.numel() != rows:
            raise ValueError(L + " needs one weight a row")
        if not self.packed:
            s3 = states.reshape(rows, 22, 10)
            if not bool(((s3 == s3.round()) & (s3.abs() <= 127)).all()):
                raise ValueError(L + " reads the states as int8: they must be integers in [-127, 127]")
            if not bool((s3[:, :2] == 0).all()):
                raise ValueError(L + " supplies the two top rows of the 22 itself: they must be all zero in the data")
        if not bool((torch.isfinite(target) & (target >= 0)).all()):
            raise ValueError(L + " needs finite targets >= 0")
        if not all(d.is_cuda and d.dtype == torch.float32 for d in data[1 if self.packed else 0:]):
            raise ValueError(L + " needs float32 CUDA tensors (the %s is %s on %s)" % (what, states.dtype, states.device))
        return rows

    def _check(self, net, optimizer, train, L):
        from .model_distributional import Net, ROW
        if not isinstance(net, Net):
            raise ValueError(L + " computes model_distributional.Net, not %s" % type(net).__name__)
        self.atoms = net.seq.fc_v.out_features
        if not (1 <= self.atoms <= ROW):
            raise ValueError(L + " holds 1..64 atoms, the net has %d" % self.atoms)
        if not isinstance(optimizer, FusedAdam):
            raise ValueError(L + " writes FusedAdam's flat gradient buffer: the optimizer must be a train.FusedAdam, not %s"
                             % type(optimizer).__name__)
        if not flat_order_is_dist_param_order(net, optimizer):
            raise ValueError(L + ": the optimizer's flat buffers are not the net's tensors in model_distributional.PARAM_ORDER")
        rows = self._check_rows(train, L, "data")
        if not optimizer.fused():
            raise ValueError(L + ": the FusedAdam's fused() must hold (float32 parameters on one GPU in a single group)")
        return rows

    def _check_flat(self, net, optimizer, F, dev, L):
        want = self.N_PARAMS_0 + 129 * self.atoms
        if F["n"] != want or F["p"].device != dev:
            raise ValueError(L + ": %d flat parameters on %s, expected %d on %s" % (F["n"], F["p"].device, want, dev))

    def _keep(self, data, rows, pre):
        setattr(self, pre + "states", data[0].contiguous() if self.packed else
                data[0].reshape(rows, 22, 10)[:, 2:].reshape(rows, 200).to(torch.int8).contiguous())
        setattr(self, pre + "target", data[1].contiguous())
        setattr(self, pre + "weight", data[2].reshape(rows).contiguous())

    def _workspace(self, n, validation=False):
        lib = self._lib.lib()
        return lib.tm_distnet_fit_validate_workspace(n, self.atoms) if validation else lib.tm_distnet_fit_workspace(n, self.atoms)

    def _validate(self, weighted, stream):
        self._lib.check(self._fn("tm_distnet_fit_validate")(
            self.F["p"].data_ptr(), self.val_states.data_ptr(), self.val_target.data_ptr(), self.val_target.stride(0),
            self.val_weight.data_ptr(), self.val_rows, self.val_chunk, self.val_slab, self.atoms, weighted,
            self.val_out.data_ptr(), self.val_ws.data_ptr(), stream), "tm_distnet_fit_validate")

    def _grad(self, idx, weighted, stream):
        F = self.F
        self._lib.check(self._fn("tm_distnet_fit_grad")(
            F["p"].data_ptr(), self.states.data_ptr(), self.target.data_ptr(), self.target.stride(0), self.weight.data_ptr(),
            idx.data_ptr(), self.batch, self.atoms, weighted, F["g"].data_ptr(), self.loss.data_ptr(), self.ws.data_ptr(), stream),
            "tm_distnet_fit_grad")


def train_data(net, optimizer, data, batch_size=128, iters_per_val=500, validation_fraction=0.1,
               sample_replacement=True, oversampling=False, weighted=True, early_stopping=True, early_stopping_patience=10,
               early_stopping_threshold=1.0, shuffle=False, max_iters=100000, grad_clip=0.0, save=None, load=None,
               generator=None, log=True, data_parallel=True, group=None, loss_fn=None, fit_backend="torch",
               validation_backend="torch", state_format="dense", ewc=None, ewc_dist=None):
    """data = [states f32 [n,1,20,10], values [n,1], variances [n,1], weights [n,1]] (device tensors); with `loss_fn`
    (net, batch, weighted) -> (mean, std) any list of arrays whose LAST one holds the sample weights (Model.train_data is
    generic in the reference too, model/model.py:176-249: the model class supplies `_loss`).
    save() / load() persist and restore the best weights (the reference goes through its checkpoint file).

    With torch.distributed initialised and more than one rank (every rank holding the same data and the same weights, as
    after dist.all_gather_tuples), `data_parallel` splits each batch: every rank draws the SAME batch_size indices (one
    sampling stream shared by the ranks: `generator`, or one seeded by a number rank 0 broadcasts) and takes every
    world-th of them, the flattened gradients (1.9 MB) are averaged with one all-reduce per iteration, and every rank takes
    the same optimizer step - the replicas stay bit-identical and one iteration sees batch_size distinct draws, as in a
    single process.  Validation runs on every rank (same numbers, same stopping).

    `fit_backend`: "torch" (the default) takes the gradient of an iteration through autograd (MIOpen / rocBLAS); "hip" takes
    it with ONE call of tm_valuenet_fit_grad (csrc/valuenet_fit.hip: forward, loss and backward as hand-written gfx950 kernels,
    writing the loss and Yogi's flat gradient buffer; the minibatch is gathered inside the kernels from an int8 copy of the
    states).  The index draws, the all-reduce, the gradient norm, clipping, the optimiser step, validation, early stopping and
    the best-weights reload are the same code for both.  "hip" is for Net + batch_loss on the GPU with the fused Yogi and
    refuses anything else with a ValueError (HipFit).  "hip_dist" is the same for the distributional head: ONE call of
    tm_distnet_fit_grad (csrc/distnet_fit.hip) for model_distributional.Net + Model_Dist.loss on data = [states [n,1,22,10],
    targets [n,atoms], weights [n,1]] with a FusedAdam (HipDistFit); validation goes through `loss_fn` (Model_Dist's own, or
    dist_batch_loss when none is given) on torch.

    `validation_backend`: "torch" (the default) validates with validation_loss (eager forwards, 1 024 rows at a time); "hip"
    replaces that call with ONE call of tm_valuenet_fit_validate / tm_distnet_fit_validate on the current stream (the gradient
    step's own forward and per-sample losses over the held-out rows, reduced per chunk of 1 024 on the device) and one .cpu()
    of the chunks' rows, which feed the same host combination (combine_chunk_rows).  It reads the optimiser's flat parameter
    buffer as it stands, so it needs fit_backend "hip" or "hip_dist" and refuses anything else with a ValueError before the
    model, the optimiser or a sampling stream is touched; with validation_fraction 0 it is accepted and does nothing.

    `state_format`: "dense" (the default) takes data[0] as rendered states; "packed" takes it as the observations the engine
    harvests, int32 [n,12] on the GPU (dist.render_observations' input), and hands them to the HIP kernels as they are: no
    rendered copy exists at any point, and the fit computes the bits of the dense one on the rendered rows.  The shuffle, the
    split, the index draws and the graph capture treat the keys as they treat dense rows.  It needs fit_backend "hip" or
    "hip_dist", and validation_backend "hip" unless no rows are held out; anything else is a ValueError raised before the model,
    the optimiser or a sampling stream is touched (check_state_format).

    `ewc`: None, or dict(fisher=, anchor=, lam=) - elastic weight consolidation: the objective gains 0.5 lam sum F (p - anchor)^2
    over the 478 338 learnable floats (fisher, anchor: float32 CUDA tensors of that length, Model_VV.compute_fisher's; lam finite
    and >= 0).  ONE call of tm_ewc_penalty (csrc/yogi.hip) adds lam F (p - anchor) to the flat gradient after the gradient step
    and after the data-parallel all-reduce (every rank adds the same penalty once) and before the gradient norm, which is then
    the penalised objective's; the iteration stays a fixed sequence of launches and is replayed from the graph as before.  At
    each validation one more line reports the mean penalty since the last.  It needs fit_backend="hip"; anything else, and a
    fisher, anchor or lam that is not as described, is a ValueError raised before the optimiser is flattened.

    `ewc_dist`: the same for the distributional head - None, or dict(fisher=, anchor=, lam=) with float32 CUDA tensors of the
    279 232 + 129 atoms flat parameters of the net (Model_Dist.compute_fisher's).  The same ONE call of tm_ewc_penalty
    at the same place of the iteration, the same log line.  It needs fit_backend="hip_dist"; `ewc` and `ewc_dist` together are
    refused, and `ewc` itself stays the value net's (with "hip_dist" it is refused as before)."""
    import torch.distributed as tdist
    check_state_format(state_format, fit_backend, validation_backend, validation_fraction, data)
    if fit_backend not in ("torch", "hip", "hip_dist"):
        raise ValueError("fit_backend must be 'torch', 'hip' or 'hip_dist', not %r" % (fit_backend,))
    if validation_backend not in ("torch", "hip"):
        raise ValueError("validation_backend must be 'torch' or 'hip', not %r" % (validation_backend,))
    if validation_backend == "hip" and fit_backend == "torch":
        raise ValueError("validation_backend='hip' reads the flat parameter buffer of a HIP fit: it needs fit_backend='hip' or "
                         "'hip_dist' (a custom loss_fn, CPU tensors and the torch fit validate with validation_backend='torch')")
    if ewc is not None and ewc_dist is not None:
        raise ValueError("ewc is the value net's penalty and ewc_dist the distributional head's: give one of the two, not both")
    check_ewc(ewc, fit_backend)
    check_ewc_dist(ewc_dist, fit_backend, net)
    if fit_backend == "hip_dist":
        if loss_fn is not None and not getattr(loss_fn, "is_model_dist_loss", False):
            raise ValueError("fit_backend='hip_dist' computes Model_Dist.loss: a custom loss_fn needs fit_backend='torch'")
        if oversampling:
            raise ValueError("fit_backend='hip_dist' does not sample by the visit weights: oversampling needs fit_backend='torch'")
        loss_fn = loss_fn or dist_batch_loss
    if fit_backend == "hip":
        if loss_fn is not None:
            raise ValueError("fit_backend='hip' computes train.batch_loss: a custom loss_fn needs fit_backend='torch'")
        if oversampling:
            raise ValueError("fit_backend='hip' does not sample by the visit weights: oversampling needs fit_backend='torch'")
    world = tdist.get_world_size(group) if (data_parallel and tdist.is_available() and tdist.is_initialized()) else 1
    my_rank = tdist.get_rank(group) if world > 1 else 0
    check_data_parallel_batch(batch_size, world)
    if world > 1 and generator is None:
        seed = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).to(data[0].device)
        tdist.broadcast(seed, src=tdist.get_global_rank(group, 0) if group is not None else 0, group=group)
        generator = torch.Generator(device=data[0].device).manual_seed(int(seed.item()))
    n = data[0].shape[0]
    n_val = int(n * validation_fraction)
    data = list(data)
    data[-1] = data[-1] / data[-1].mean()
    loss_fn = loss_fn or batch_loss
    if shuffle:
        perm = torch.randperm(n, device=data[0].device, generator=generator)
        data = [d[perm] for d in data]
    train = [d[:n - n_val] for d in data] if n_val else data
    val = [d[n - n_val:] for d in data] if n_val else None
    if log:
        print("Training data size: {}    Validation data size: {}".format(n - n_val, n_val), file=stderr, flush=True)
    fails, best = 0, float("inf")
    loss_avg = torch.zeros((), device=data[0].device)      # running sums stay on the device: no sync per iteration
    g_norm_avg = torch.zeros((), device=data[0].device)
    iters_done = 0
    net.train()
    # the one-kernel optimiser step (Yogi on the GPU): parameters and gradients are views of flat buffers from here on
    hip_val = val if validation_backend == "hip" else None
    hip = (HipFit(net, optimizer, train, batch_size // world, val=hip_val, state_format=state_format, ewc=ewc) if fit_backend == "hip" else
           HipDistFit(net, optimizer, train, batch_size // world, val=hip_val, state_format=state_format, ewc=ewc_dist)
           if fit_backend == "hip_dist" else None)
    if hip is not None and hip.rows != n - n_val:      # every draw below is an index into [0, n - n_val): the rows the kernels hold
        raise ValueError("fit_backend=%r: %d training rows, but the index draws cover %d" % (fit_backend, hip.rows, n - n_val))
    flat_g = optimizer.flat_grad() if hasattr(optimizer, "flat_grad") else None
    ewc = ewc if ewc is not None else ewc_dist      # (one of the two at the most: the penalty of the fit's own head)
    ewc_avg = torch.zeros((), dtype=torch.float64, device=data[0].device) if ewc is not None else None

    def one_iteration():
        if oversampling:    # model.py:194-195: draw proportionally to the visit weights
            idx = torch.multinomial(train[-1].reshape(-1), batch_size, replacement=sample_replacement, generator=generator)
        elif sample_replacement:
            idx = torch.randint(0, n - n_val, (batch_size,), device=data[0].device, generator=generator)
        else:
            idx = torch.randperm(n - n_val, device=data[0].device, generator=generator)[:batch_size]
        if world > 1:
            idx = idx[my_rank::world]
        if hip is not None:
            loss = hip.grad(idx, weighted)           # (overwrites the flat gradient: no zero_grad)
        else:
            optimizer.zero_grad(set_to_none=True)
            loss, _ = loss_fn(net, [d[idx] for d in train], weighted)
            loss.backward()
        if world > 1:
            if flat_g is not None:
                tdist.all_reduce(flat_g, group=group)
                flat_g.div_(world)
            else:
                grads = [p.grad for p in net.parameters() if p.grad is not None]
                flat = torch.cat([g.reshape(-1) for g in grads])
                tdist.all_reduce(flat, group=group)
                flat /= world
                off = 0
                for g in grads:
                    g.copy_(flat[off:off + g.numel()].view_as(g))
                    off += g.numel()
        if ewc is not None:      # after the all-reduce: every rank adds the same penalty once
            ewc_avg.add_(hip.penalty())
        # 2-norm over all parameter gradients (model.py:87-95), reported in the log line the dashboards parse
        if flat_g is not None:
            g_norm_avg.add_(torch.linalg.vector_norm(flat_g))
        else:
            g_norm_avg.add_(torch.sqrt(sum((p.grad.detach() ** 2).sum() for p in net.parameters() if p.grad is not None)))
        if grad_clip > 0:
            torch.nn.utils.clip_grad_norm_(net.parameters(), grad_clip)
        optimizer.step()
        loss_avg.add_(loss.detach())

    # One iteration is a fixed sequence of launches (index draw, gather, forward, backward, the one-kernel step): after three
    # of them it is captured in a HIP graph and replayed - the fit of a 478 342-parameter net on batches of 1 024 was bound by
    # its launches, not by its arithmetic (r05: 2.3 ms an iteration for 0.1 ms of matrix work).  Not with more than one rank
    # (the all-reduce stays outside), a sampling stream of the caller's, or gradient clipping.
    import os
    graph, n_warm = None, 3
    want_graph = (flat_g is not None and world == 1 and flat_g.is_cuda and generator is None and grad_clip <= 0 and not oversampling
                  and sample_replacement and os.environ.get("TM_TRAIN_GRAPH", "1") != "0" and max_iters > n_warm)
    it = 0
    while it < max_iters:
        if want_graph and graph is None and it == n_warm:
            t_before = optimizer._flat["t"]
            try:
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    one_iteration()
                optimizer._flat["t"] = t_before          # (captured, not run)
            except Exception as e:                        # noqa: BLE001 - whatever the runtime refuses: the eager loop is the same fit
                graph, want_graph = None, False
                optimizer._flat["t"] = t_before          # (a capture that failed after the step was recorded ran no step either)
                torch.cuda.synchronize()
                if log:
                    print("train_data: no graph replay (%s: %s)" % (type(e).__name__, str(e).splitlines()[0][:120]), file=stderr, flush=True)
        if graph is not None:
            graph.replay()
            optimizer._flat["t"] += 1
        else:
            one_iteration()
        iters_done = it + 1
        if (it + 1) % iters_per_val == 0 and val is not None:
            if hip_val is not None:
                vmean, vstd = combine_chunk_rows(hip.validate(weighted))
            else:
                net.eval()
                vmean, vstd = validation_loss(net, val, weighted, loss_fn=loss_fn)
                net.train()
            vstd /= max(n_val, 1) ** 0.5
            mark = ""
            if early_stopping:
                if vmean - best < vstd * early_stopping_threshold:
                    fails = 0
                    if vmean < best:
                        mark = "*"
                        best = vmean
                        if save:
                            save()
                else:
                    fails += 1
            if world > 1:      # the logged training loss is the mean over ranks (the gradient norm already is global)
                tdist.all_reduce(loss_avg, group=group)
                loss_avg /= world
            if log:
                print("Iteration:{:7d}  training loss:{:6.4f}  validation loss:{:6.4f}±{:6.4f}  gradient norm:{:6.3f}    {}"
                      .format(it + 1, float(loss_avg) / iters_per_val, vmean, vstd, float(g_norm_avg) / iters_per_val, mark),
                      file=stderr, flush=True)
            if ewc is not None:
                if log:
                    print("EWC penalty (mean over the last %d iterations):%.6g" % (iters_per_val, float(ewc_avg) / iters_per_val),
                          file=stderr, flush=True)
                ewc_avg.zero_()
            loss_avg.zero_()
            g_norm_avg.zero_()
            if early_stopping and fails >= early_stopping_patience:
                break
        it += 1
    replayed = graph is not None
    del graph
    if early_stopping and load and best < float("inf"):
        load()
    elif save:
        save()
    net.eval()
    return dict(iters=iters_done, best_validation=best, graph_replay=replayed)
