"""Cases and references for the HIP gradient step of the fit (csrc/valuenet_fit.hip), shared by tests/test_fit_hip.py (CPU: the
references alone - that the yardstick's denominators are non-zero) and tests/test_gpu_fit_hip.py (GPU: the kernels against them).

The reference's arithmetic is torch autograd of model.Net + train.batch_loss on the CPU, in fp64 (g64) and in fp32 (g32).  The
yardstick is measure B of DESIGN.md section 6 applied to gradients, per parameter tensor and for the two loss outputs:
    max|g_hip - g64| <= M max|g32 - g64| + 4 u max|g64|,   M = 8, u = 2^-24.
A tensor whose fp64 gradient is identically zero is compared for exact zeros instead.

Run as a program (`python tests/fit_hip_cases.py digest`) it prints the SHA-256 of one case's gradient and loss bytes: the
second process of the determinism test."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
M_CAP, U = 8.0, 2.0 ** -24
N_LEARN = 478338
BATCHES = (1, 31, 32, 33, 256, 512, 1000, 1024)
# the batch decides the shape of the two-stage reductions of csrc/valuenet_fit.hip through s1 = ceil(B / FC_KC) splits of fc1's
# weight gradient (added by k_fit_reduce<RED_G_FC> in 4 interleaved groups), hchunks = ceil(B / HEAD_CHUNK) partials of the FC bias
# sums and chunks = ceil(B / SPW) partials of the convolutions' weight gradients (both added in RED_G = 16 groups).  BATCHES ends
# at s1 = 4: LARGE_BATCHES are the smallest batches with a split of one sample (257) and with a group of more than one split
# (1 025: s1 = 5, hchunks = 33, chunks = 257).  Their cases come after all others and draw from a generator of their own.
FC_KC, HEAD_CHUNK, SPW, RED_G_FC, RED_G = 256, 32, 4, 4, 16
LARGE_BATCHES = (FC_KC + 1, RED_G_FC * FC_KC + 1)


def boards(n, seed):
    """n boards [n,200] int8: a stack of random height filled at 70 %, and a falling piece (-1) above it"""
    rng = np.random.default_rng(seed)
    s = np.zeros((n, 20, 10), np.int8)
    h = rng.integers(0, 14, n)
    for i in range(n):
        s[i, 20 - h[i]:, :] = rng.random((h[i], 10)) < 0.7
        y, x = rng.integers(0, max(1, 18 - h[i])), rng.integers(0, 7)
        s[i, y, x:x + 4] = -1
    return s.reshape(n, 200), h


def dataset(n, seed, scale=1.0):
    """(states int8 [n,200], value, variance, weight fp32 [n]); a tenth of the variances lie below the clip of 0.1"""
    rng = np.random.default_rng(seed + 1000)
    s, h = boards(n, seed)
    value = ((2.0 + 3.0 * h + rng.normal(0, 1.0, n)) * scale).astype(np.float32)
    variance = (rng.uniform(0.2, 8.0, n) * scale * scale).astype(np.float32)
    variance[rng.random(n) < 0.1] = np.float32(0.01)
    weight = rng.integers(3, 50, n).astype(np.float32)
    weight /= weight.mean()
    return s, value, variance, weight


def fresh_net(seed=0):
    from tetris_mcts_amd.model import Net
    torch.manual_seed(seed)
    return Net()


def net_from_flat(flat):
    from tetris_mcts_amd.model import Net, PARAM_ORDER
    net = Net()
    sd, off = net.state_dict(), 0
    flat = torch.as_tensor(np.asarray(flat), dtype=torch.float32)
    for k in PARAM_ORDER:
        n = sd[k].numel()
        sd[k].copy_(flat[off:off + n].reshape(sd[k].shape))
        off += n
    return net


def net_from_checkpoint(name, value, variance):
    from tetris_mcts_amd.model import Net
    net = Net()
    ck = torch.load(os.path.join(ROOT, "tetris_mcts_amd", "checkpoints", name), map_location="cpu")
    net.load_state_dict(ck["model_state_dict"])
    with torch.no_grad():
        net.out_ubound.copy_(torch.tensor([float(value.max()), float(variance.max())]))      # model_vv.py:228-229
    return net


def learnable(net):
    from tetris_mcts_amd.model import PARAM_ORDER
    named = dict(net.named_parameters())
    return [named[k] for k in PARAM_ORDER[:10]]


def reference(case, dtype):
    """autograd of Net + batch_loss on the CPU in `dtype`: ([10 gradients as float64 arrays], (mean, std))"""
    import copy
    from tetris_mcts_amd import train as T
    (states, value, variance, weight), weighted = case["data"], case["weighted"]
    net = copy.deepcopy(case["net"]).to(dtype).train()
    idx = np.arange(case["batch"]) if case["idx"] is None else np.asarray(case["idx"])
    batch = [torch.from_numpy(states[idx].reshape(-1, 1, 20, 10).astype(np.float64)).to(dtype)] + \
            [torch.from_numpy(a[idx].reshape(-1, 1).astype(np.float64)).to(dtype) for a in (value, variance, weight)]
    for p in net.parameters():
        p.grad = None
    mean, std = T.batch_loss(net, batch, weighted)
    mean.backward()
    grads = [p.grad.detach().double().numpy().copy() for p in learnable(net)]
    return grads, (float(mean.detach().double()), float(std.detach().double()))


def off_the_kink(net, states):
    """Rows whose every ReLU pre-activation z keeps clear of zero: |z| >= 64 u (|bias| + sum_k |w_k a_k|), from an fp64 forward.

    The gradient is discontinuous where a pre-activation is zero: a unit whose z lies inside the rounding error of an fp32
    forward is switched on in one summation order and off in another (and in fp64), and the gradients then differ by that
    unit's whole contribution - no multiple of anybody's rounding error.  Measure B compares rounding errors, so its inputs
    must keep away from the kink by more than an fp32 forward can move z: sqrt(K) u sum|w a| for a sum of K terms in any
    order (K <= 1 792: sqrt(K) <= 43 < 64).  Random rows are filtered by this rule, computed from the reference alone (a
    tenth to a fifth of them go: a row has 9 728 pre-activations); the fixed golden batch is not filtered."""
    import copy
    import torch.nn.functional as F
    net = copy.deepcopy(net).double()
    h = net.head
    x = torch.from_numpy(np.asarray(states).reshape(-1, 1, 20, 10).astype(np.float64))
    keep = torch.ones(x.shape[0], dtype=torch.bool)
    with torch.no_grad():
        for conv in (h.conv1, h.conv2, h.conv3):
            z = conv(x)
            S = F.conv2d(x.abs(), conv.weight.abs(), conv.bias.abs())
            keep &= (z.abs() >= 64 * U * S).flatten(1).all(1)
            x = torch.relu(z)
        x = x.flatten(1)
        z = h.fc1(x)
        S = F.linear(x.abs(), h.fc1.weight.abs(), h.fc1.bias.abs())
        keep &= (z.abs() >= 64 * U * S).all(1)
    return keep.numpy()


def _restrict(data, net):
    keep = off_the_kink(net, data[0])
    assert keep.sum() >= 0.5 * len(keep), keep.mean()
    return tuple(a[keep] for a in data)


def _fresh_rows():
    return _restrict(dataset(1800, 7), fresh_net(0))


def large_cases(data=None):
    """the regimes past BATCHES: a split of fc1's weight gradient that holds one sample, and more splits than the second stage has
    groups.  `data` is the fresh net's filtered candidate set (built here when not given)."""
    data = _fresh_rows() if data is None else data
    n = len(data[0])
    b1, b5 = LARGE_BATCHES
    assert n >= b5
    rng = np.random.default_rng(12)
    out = {}
    out["fresh net, batch %d" % b1] = dict(net=fresh_net(0), data=data, idx=rng.integers(0, n, b1), batch=b1, weighted=True)
    out["fresh net, batch %d" % b5] = dict(net=fresh_net(0), data=data, idx=rng.integers(0, n, b5), batch=b5, weighted=True)
    out["fresh net, batch %d, unweighted, idx NULL" % b5] = dict(net=fresh_net(0), data=data, idx=None, batch=b5, weighted=False)
    ck = "value_net_online_r06.pt"
    big = dataset(800, 21, scale=40.0)
    big = _restrict(big, net_from_checkpoint(ck, big[1], big[2]))
    out["%s, weighted, batch %d" % (ck, b5)] = dict(net=net_from_checkpoint(ck, big[1], big[2]), data=big,
                                                   idx=rng.integers(0, len(big[0]), b5), batch=b5, weighted=True)
    return out


def cases(full=True):
    """name -> dict(net, data = (states, value, variance, weight), idx (array or None), batch, weighted)"""
    out = {}
    g = np.load(os.path.join(ROOT, "tests", "golden", "ref_training.npz"))
    gold = (g["tr_states"].reshape(-1, 200).astype(np.int8), g["tr_values"].reshape(-1).copy(), g["tr_variances"].reshape(-1).copy(),
            g["tr_weights"].reshape(-1) / g["tr_weights"].mean())
    out["golden batch, tr_params0"] = dict(net=net_from_flat(g["tr_params0"]), data=gold, idx=None, batch=48, weighted=True)
    data = _fresh_rows()
    n = len(data[0])
    assert n >= 1024
    rng = np.random.default_rng(11)
    for b in (BATCHES if full else (1, 33)):
        out["fresh net, batch %d" % b] = dict(net=fresh_net(0), data=data, idx=rng.integers(0, n, b), batch=b, weighted=True)
    out["fresh net, unweighted, idx NULL"] = dict(net=fresh_net(0), data=data, idx=None, batch=256, weighted=False)
    out["fresh net, weighted, idx NULL"] = dict(net=fresh_net(0), data=data, idx=None, batch=100, weighted=True)
    out["fresh net, unweighted, repeats"] = dict(net=fresh_net(0), data=data, idx=rng.integers(0, 40, 256), batch=256, weighted=False)
    for ck in ("value_net_online_r05.pt", "value_net_online_r06.pt"):
        big = dataset(800, 21, scale=40.0)
        big = _restrict(big, net_from_checkpoint(ck, big[1], big[2]))
        for weighted in (True, False):
            out["%s, %s" % (ck, "weighted" if weighted else "unweighted")] = dict(
                net=net_from_checkpoint(ck, big[1], big[2]), data=big, idx=rng.integers(0, len(big[0]), 512), batch=512,
                weighted=weighted)
    # every target variance below the clip
    low = tuple(a.copy() for a in data)
    low[2][:] = np.float32(0.003)
    out["targets below the variance clip"] = dict(net=fresh_net(0), data=low, idx=rng.integers(0, n, 64), batch=64, weighted=True)
    # saturated sigmoids: the output layer's pre-activations near +-12
    sat = fresh_net(0)
    with torch.no_grad():
        sat.head.fc_out.bias.copy_(torch.tensor([12.0, -12.0]))
    out["saturated sigmoid"] = dict(net=sat, data=data, idx=rng.integers(0, n, 64), batch=64, weighted=True)
    if full:
        out.update(large_cases(data))          # last, with a generator of their own: every case above keeps its index draw
    return out


def dead_relu_case():
    """conv3's bias large and negative: a3 = 0 everywhere, and the gradients of conv1, conv2, conv3 and fc1.weight are exactly 0"""
    net = fresh_net(0)
    with torch.no_grad():
        net.head.conv3.bias.fill_(-1e3)
    rng = np.random.default_rng(5)
    data = _restrict(dataset(300, 9), net)
    return dict(net=net, data=data, idx=rng.integers(0, len(data[0]), 96), batch=96, weighted=True)


TENSORS = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv3.weight", "conv3.bias", "fc1.weight", "fc1.bias",
           "fc_out.weight", "fc_out.bias")


def split(flat):
    sizes = (288, 32, 9216, 32, 9216, 32, 458752, 256, 512, 2)
    out, off = [], 0
    for n in sizes:
        out.append(np.asarray(flat[off:off + n], dtype=np.float64))
        off += n
    assert off == N_LEARN
    return out


def measure(got, g32, g64):
    """(error of `got`, the rule's bound, the multiple of torch's own fp32 error that `got` needs beyond the 4 u term)"""
    got, g32, g64 = (np.asarray(a, np.float64).reshape(-1) for a in (got, g32, g64))
    err, own, top = np.abs(got - g64).max(), np.abs(g32 - g64).max(), np.abs(g64).max()
    need = max(err - 4 * U * top, 0.0) / own if own > 0 else (0.0 if err <= 4 * U * top else float("inf"))
    return err, M_CAP * own + 4 * U * top, need


# ---- the device side (imported lazily: the CPU tests use the references alone) ----
def hip_grad(case, device="cuda", grad_fill=None, place=None):
    """one tm_valuenet_fit_grad call for a case: (flat gradient [478338] float32 array, loss [2] float32 array).

    `place(n_workspace, n_grad, inputs)` may supply the three buffers the call writes, as float32 views (workspace, grad, loss)
    of storage of its own (tests: an arena with guard bands, `Arena` below); `inputs` is the dict of the device tensors the call
    reads, handed over before the launch so that the caller can copy them.  The buffers are filled as without `place`.  A read
    past an input cannot be seen this way (a stray read changes nothing); stray stores within 64 KiB of a buffer and stores into
    an input can."""
    from tetris_mcts_amd import _lib
    lib = _lib.lib()
    net, (states, value, variance, weight), idx, B = case["net"], case["data"], case["idx"], case["batch"]
    dev = torch.device(device)
    P = torch.cat([p.detach().reshape(-1).float() for p in learnable(net)]).to(dev).contiguous()
    assert P.numel() == N_LEARN
    bounds = torch.cat([net.out_ubound.detach(), net.out_lbound.detach()]).float().to(dev).contiguous()
    s8 = torch.from_numpy(np.ascontiguousarray(states, dtype=np.int8)).to(dev)
    val, var, w = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in (value, variance, weight))
    if idx is not None:
        assert len(idx) == B and 0 <= int(np.min(idx)) and int(np.max(idx)) < len(states)
        idx_t = torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(dev)
    else:
        assert B <= len(states)
        idx_t = None
    n_ws = lib.tm_valuenet_fit_workspace(B)
    assert n_ws > 0
    if place is None:
        ws, grad, loss = (torch.empty(n, dtype=torch.float32, device=dev) for n in (n_ws, N_LEARN, 2))
    else:
        ws, grad, loss = place(n_ws, N_LEARN, dict(params=P, bounds=bounds, states=s8, value=val, variance=var, weight=w, idx=idx_t))
        assert (ws.numel(), grad.numel(), loss.numel()) == (n_ws, N_LEARN, 2) and all(t.dtype == torch.float32 for t in (ws, grad, loss))
    ws.fill_(float("nan"))                                                         # no initial contents required
    grad.fill_(float("nan") if grad_fill is None else grad_fill)
    loss.fill_(float("nan"))
    _lib.check(lib.tm_valuenet_fit_grad(P.data_ptr(), bounds.data_ptr(), s8.data_ptr(), val.data_ptr(), var.data_ptr(), w.data_ptr(),
                                        idx_t.data_ptr() if idx_t is not None else None, B, int(case["weighted"]), 0.1,
                                        grad.data_ptr(), loss.data_ptr(), ws.data_ptr(),
                                        torch.cuda.current_stream(dev).cuda_stream), "tm_valuenet_fit_grad")
    torch.cuda.synchronize()
    return grad.cpu().numpy(), loss.cpu().numpy()


class Arena:
    """The three buffers a fit call writes, carved out of one device tensor with a guard band of GUARD bytes before, between
    and after them, for hip_grad's `place`.  Every segment starts on a 16-byte boundary and has exactly the size the ABI states;
    the whole arena starts as PATTERN (a finite float, so that the guards compare as integers).  After the call `check()` asserts
    that every byte outside the three segments is unchanged and that every input is bit-identical to the copy taken before the
    launch.  What this cannot see: a read past an input or past a segment, and a store that lands inside another of the three
    segments or beyond the guard bands."""
    GUARD, PATTERN = 64 * 1024, 0x5A5A5A5A

    def __init__(self, device="cuda"):
        self.device, self.arena, self.segments, self.inputs, self.before = torch.device(device), None, [], None, None

    def __call__(self, n_ws, n_grad, inputs):
        g = self.GUARD // 4
        off, self.segments = g, []
        for n in (n_ws, n_grad, 2):
            assert off % 4 == 0
            self.segments.append((off, n))
            off = (off + n + 3) // 4 * 4 + g          # the padding up to the 16-byte boundary belongs to the guard
        self.arena = torch.full((off,), self.PATTERN, dtype=torch.int32, device=self.device)
        assert self.arena.data_ptr() % 16 == 0
        self.inputs = {k: v for k, v in inputs.items() if v is not None}
        self.before = {k: v.clone() for k, v in self.inputs.items()}
        views = [self.arena[o:o + n].view(torch.float32) for o, n in self.segments]
        assert all(v.data_ptr() % 16 == 0 and v.data_ptr() == self.arena.data_ptr() + 4 * o for v, (o, n) in zip(views, self.segments))
        return views

    def check(self):
        torch.cuda.synchronize()
        outside = torch.ones(self.arena.numel(), dtype=torch.bool, device=self.device)
        for o, n in self.segments:
            outside[o:o + n] = False
        assert int(outside.sum()) >= 4 * (self.GUARD // 4)
        touched = torch.nonzero(outside & (self.arena != self.PATTERN)).flatten()
        assert touched.numel() == 0, ("stores outside the buffers at float offsets", touched[:8].tolist(), self.segments)
        for k, v in self.inputs.items():
            a, b = v.cpu().numpy(), self.before[k].cpu().numpy()
            assert a.tobytes() == b.tobytes(), ("input changed", k)


def digest_case():
    c = cases(full=False)["fresh net, batch 33"]
    return c


if __name__ == "__main__":
    if sys.argv[1:] == ["digest"]:
        import hashlib
        g, l = hip_grad(digest_case())
        print("DIGEST " + hashlib.sha256(g.tobytes() + l.tobytes()).hexdigest(), flush=True)
