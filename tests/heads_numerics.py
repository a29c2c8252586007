"""Shared numerics for the accuracy tests of the two evaluators (tests/test_heads_accuracy.py, tests/test_gpu_heads_accuracy.py):
weight regimes, board families, CPU torch forwards that return every layer's activations (fp64, and fp32 "as the reference runs
it": the same torch ops as its `Net` classes), and two error measures.  A plain module, imported by the tests.

Measure A - a derived bound, one or two layers deep
---------------------------------------------------
u = 2^-24, gamma_k = k u / (1 - k u).  One layer y = W x + b evaluated in fp32 by K fused multiply-adds onto the bias, in ANY
order or grouping (a sequential chain, an MFMA's k-blocks, torch's blocked sums), satisfies, element by element,

    |y_hat - y| <= gamma_(K+1) * (|b| + sum_k |x_k| |w_k|)                                     (Higham, ASNA 2nd ed., sec. 3.1)

with y evaluated exactly (here: fp64) from the layer's ACTUAL fp32 input.  ReLU is 1-Lipschitz and exact in fp32, so the bound
carries over to the activation; LeakyReLU's negative branch is one more fp32 product by (float)0.01, which differs from the fp64
forward's 0.01 by less than u relative: + 2 u |a|.  Where only every second layer can be observed, with x1 the exact output of
the first layer and E1 its bound, the computed input of the second layer lies within E1 of x1, so

    E2 = gamma * (|b2| + |W2| (|x1| + E1)) + |W2| E1

and so on (`chain_bound`).  End to end the recursion is vacuous; it is used up to three layers deep only.

Split-precision (bf16x3) layers, from csrc/bf16x3.h and DESIGN 3.3 / 3.8: x = hi + mid + lo + r with |hi| <= (1 + 2^-8)|x|,
|mid| <= 2^-8 |x|, |lo| <= 2^-16 |x|, |r| <= 2^-24 |x|, and the same for w.  Of the nine plane products the kernels keep the six
with i + j <= 2.  Truncation of one product x w:
    dropped (mid, lo), (lo, mid), (lo, lo)      <= (2 * 2^-24 + 2^-32) |x| |w|
    the split remainders r_x w + (x - r_x) r_w  <= (2 * 2^-24 + 2^-48) |x| |w|
together <= 4.01 u |x| |w|.  Each kept plane product is exact in fp32 (8 x 8 significant bits); the 6 K of them are added onto the
bias in fp32 (grouping them before a rounding, as a matrix core does, only removes roundings):
    <= gamma_(6K+1) * (|b| + sum over the kept |x_i| |w_j|),   sum over the kept <= 1.016 |x| |w|
((1 + 2^-8)^2 (1 + 2 * 2^-8 + 3 * 2^-16)).  So a split layer obeys the fp32 form with the constant
    c_x3(K) = 1.016 * gamma_(6K+1) + 4.01 u                                                   (`c_x3`)
in place of gamma_(K+1).  It is about six times the fp32 constant: it cannot tell a dropped `lo` plane (2^-15 |x||w| per product,
random signs) from rounding; the "within 2x the fp32 path's error" assertions of test_split_precision.py do that.

Value-net output: out = fl(fl(sigmoid(z)) * ub) + lb.  The sigmoid's slope is at most 1/4, the three roundings and the sigmoid's
own evaluation are "a few u" (8 u taken) of the magnitudes involved:
    |out_hat - out| <= ub * E_z / 4 + 8 u (ub * sigmoid(z) + |lb|).
Softmax: log p_i = z_i - logsumexp(z), so |d log p_i| <= |dz_i| + max |dz| <= 2 max E_z; the subtraction z_i - max z is itself
rounded in fp32 by torch (u |z_i - max z|; the HIP kernel subtracts in double), and exp, the division and the rounding of p add
a few u (8 u taken):
    |log p_hat_i - log p_i| <= 2 max_j E_z[j] + u |z_i - max z| + 8 u,
over the atoms whose fp64 p is in fp32's normal range.

The bounds ignore underflow: `assert_normal_range` holds every regime's nonzero activations above 2^-100.

Measure B - end to end, against the reference's own fp32 arithmetic
-------------------------------------------------------------------
err(impl) = max |impl - fp64|, err(ref32) = max |reference fp32 forward - fp64|, per (regime, family, output):
    err(impl) <= M * err(ref32) + 4 u max |fp64 output|.
`needed_M` is the smallest M that satisfies it (0 when the floor alone covers the error).
"""
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CHECKPOINTS = os.path.join(ROOT, "tetris_mcts_amd", "checkpoints")
U = 2.0 ** -24
F32_MIN_NORMAL = 2.0 ** -126
P_MIN_B = 2.0 ** -100         # measure B's log p runs over the atoms with fp64 p >= this

VN_SHAPES = [("conv1.w", (32, 1, 3, 3)), ("conv1.b", (32,)), ("conv2.w", (32, 32, 3, 3)), ("conv2.b", (32,)),
             ("conv3.w", (32, 32, 3, 3)), ("conv3.b", (32,)), ("fc1.w", (256, 1792)), ("fc1.b", (256,)),
             ("fc_out.w", (2, 256)), ("fc_out.b", (2,)), ("ub", (2,)), ("lb", (2,))]
VN_PARAMS = 478342
VN_LEARNABLE = 478338           # everything before out_ubound
VN_CKPT_KEYS = ["head.conv1.weight", "head.conv1.bias", "head.conv2.weight", "head.conv2.bias", "head.conv3.weight",
                "head.conv3.bias", "head.fc1.weight", "head.fc1.bias", "head.fc_out.weight", "head.fc_out.bias", "out_ubound",
                "out_lbound"]
DN_KEYS = ["seq__conv1__weight", "seq__conv1__bias", "seq__conv2__weight", "seq__conv2__bias", "seq__fc1__weight",
           "seq__fc1__bias", "seq__fc_v__weight", "seq__fc_v__bias"]
# scratch rows of the kernels (include/tetris_mcts_hip.h): where each layer's activations are left
VN_PLAIN_ROW, VN_PLAIN_OFF = 9728, (0, 4608, 4608 + 3072, 4608 + 3072 + 1792)      # a1, a2, a3, hidden
VN_MFMA_ROW, VN_MFMA_OFF = 2064, (0, 1792)                                           # a3, hidden
DN_ROW = 2048                                                                         # a2


def gamma(k):
    return k * U / (1.0 - k * U)


def c_x3(K):
    """the constant of a split-precision layer of K products (module docstring)"""
    return 1.016 * gamma(6 * K + 1) + 4.01 * U


# ---------------------------------------------------------------------------------------------------------------- layers
class Layer:
    def __init__(self, name, kind, w, b, act):
        self.name, self.kind, self.act = name, kind, act
        self.w, self.b = np.ascontiguousarray(w, np.float32), np.ascontiguousarray(b, np.float32)
        self.K = int(self.w[0].size)

    def tensors(self, dtype):
        return torch.from_numpy(self.w).to(dtype), torch.from_numpy(self.b).to(dtype)

    def replace(self, w=None, b=None, act="same"):
        return Layer(self.name, self.kind, self.w if w is None else w, self.b if b is None else b,
                     self.act if act == "same" else act)


def lin(layer, x, w, b):
    if layer.kind == "conv":
        return F.conv2d(x, w, b)
    return F.linear(x.flatten(1), w, b)


def act(layer, y):
    if layer.act == "relu":
        return torch.relu(y)
    if layer.act == "leaky":
        return F.leaky_relu(y, 0.01)
    return y


def vn_split(P):
    P = np.asarray(P, np.float32)
    assert P.size == VN_PARAMS
    out, off = OrderedDict(), 0
    for k, shape in VN_SHAPES:
        n = int(np.prod(shape))
        out[k] = P[off:off + n].reshape(shape)
        off += n
    return out


def vn_layers(P):
    d = vn_split(P)
    return [Layer("conv1", "conv", d["conv1.w"], d["conv1.b"], "relu"), Layer("conv2", "conv", d["conv2.w"], d["conv2.b"], "relu"),
            Layer("conv3", "conv", d["conv3.w"], d["conv3.b"], "relu"), Layer("fc1", "fc", d["fc1.w"], d["fc1.b"], "relu"),
            Layer("fc_out", "fc", d["fc_out.w"], d["fc_out.b"], None)]


def dn_layers(W):
    return [Layer("conv1", "conv", W[0], W[1], "leaky"), Layer("conv2", "conv", W[2], W[3], "leaky"),
            Layer("fc1", "fc", W[4], W[5], "leaky"), Layer("fc_v", "fc", W[6], W[7], None)]


def dn_flat(W):
    return np.concatenate([np.asarray(w, np.float32).ravel() for w in W])


# -------------------------------------------------------------------------------------------------------------- forwards
@torch.no_grad()
def run_layers(layers, x, dtype):
    """every layer's activation (the last layer's pre-head output), computed in `dtype` by the torch ops the reference's Nets use"""
    acts, x = [], x.to(dtype)
    for L in layers:
        w, b = L.tensors(dtype)
        x = act(L, lin(L, x, w, b))
        acts.append(x)
    return acts


def vn_input(boards):
    return torch.from_numpy(np.asarray(boards, np.int8).reshape(-1, 1, 20, 10).astype(np.float32))


def dn_input(boards):
    """the 20 visible rows under two empty ones (model_distributional.Model_Dist.inference_device)"""
    b = np.asarray(boards, np.int8).reshape(-1, 20, 10)
    x = np.zeros((b.shape[0], 1, 22, 10), np.float32)
    x[:, 0, 2:, :] = b
    return torch.from_numpy(x)


@torch.no_grad()
def vn_forward(P, boards, dtype):
    """-> (acts [a1, a2, a3, hidden, z], out [n, 2]) of Net.forward = head(x) * out_ubound + out_lbound in `dtype`"""
    d = vn_split(P)
    acts = run_layers(vn_layers(P), vn_input(boards), dtype)
    out = torch.sigmoid(acts[-1]) * torch.from_numpy(d["ub"]).to(dtype) + torch.from_numpy(d["lb"]).to(dtype)
    return acts, out


@torch.no_grad()
def dn_forward(W, boards, dtype):
    """-> (acts [a1, a2, hidden, logits], p [n, atoms]) of Net.forward = softmax(seq(x), 1) in `dtype`"""
    acts = run_layers(dn_layers(W), dn_input(boards), dtype)
    return acts, F.softmax(acts[-1], 1)


# -------------------------------------------------------------------------------------------------------------- measure A
@torch.no_grad()
def chain_bound(layers, x_in, cs=None, tiny=False):
    """Exact (fp64) activations of `layers` from the actual input x_in of the first one, and the elementwise bound on what an
    fp32 evaluation of them can give.  cs: one constant per layer (default gamma_(K+1)).  tiny: absolute allowances for
    arithmetic that loses what lies below the normal range (2^-126, of fp32 and bf16 alike; the subnormal regime of
    tests/test_gpu_heads_accuracy.py): K * 2^-126 per layer for lost products, and for a split layer (one with a constant in
    cs) the `mid` and `lo` planes of every operand - each below 2^-126 when lost, and never more than 2^-8 + 2^-16 of the
    operand: sum min(2^-125, (2^-8 + 2^-16) |x|) |w| + sum |x| min(2^-125, (2^-8 + 2^-16) |w|).
    -> [(a64, E), ...] per layer."""
    x, E, out = x_in.double(), None, []
    for i, L in enumerate(layers):
        w, b = L.tensors(torch.float64)
        c = gamma(L.K + 1) if cs is None or cs[i] is None else cs[i]
        Enew = c * lin(L, x.abs() if E is None else x.abs() + E, w.abs(), b.abs())
        if E is not None:
            Enew = Enew + lin(L, E, w.abs(), None)
        if tiny:
            Enew = Enew + L.K * F32_MIN_NORMAL
            if cs is not None and cs[i] is not None:
                ax = x.abs() if E is None else x.abs() + E
                lost = lambda t: torch.clamp((2.0 ** -8 + 2.0 ** -16) * t, max=2 * F32_MIN_NORMAL)      # noqa: E731
                Enew = Enew + lin(L, lost(ax), w.abs(), None) + lin(L, ax, lost(w.abs()), None)
        a = act(L, lin(L, x, w, b))
        if L.act == "leaky":
            Enew = Enew + 2 * U * a.abs()
        x, E = a, Enew
        out.append((a, E))
    return out


def ratio_A(impl, a64, E):
    """max over the elements of |impl - a64| / E (0 / 0 = 0; anything above 0 bound 0, or a NaN, = inf)"""
    d = (impl.double().reshape(a64.shape) - a64).abs()
    r = torch.where(d == 0, torch.zeros_like(d), d / E)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max())


def vn_out_bound(P, hidden_in):
    """fc_out + sigmoid + affine from the actual hidden layer: (out64 [n, 2], E [n, 2])"""
    d = vn_split(P)
    (z, Ez), = chain_bound(vn_layers(P)[4:], hidden_in)
    ub, lb = torch.from_numpy(d["ub"]).double(), torch.from_numpy(d["lb"]).double()
    sg = torch.sigmoid(z)
    return sg * ub + lb, ub.abs() * Ez / 4 + 8 * U * (ub.abs() * sg + lb.abs())


def dn_logp_bound(W, hidden_in):
    """fc_v + softmax from the actual hidden layer: (logp64 [n, atoms], E [n, atoms], p64)"""
    (z, Ez), = chain_bound(dn_layers(W)[3:], hidden_in)
    lp = F.log_softmax(z, 1)
    E = 2 * Ez.max(1, keepdim=True).values + U * (z - z.max(1, keepdim=True).values).abs() + 8 * U
    return lp, E.expand_as(lp), lp.exp()


def ratio_logp(p_impl, lp64, E):
    """measure A on log p over the atoms whose fp64 p is in fp32's normal range"""
    ok = lp64 >= np.log(F32_MIN_NORMAL)
    lp = torch.log(p_impl.double().reshape(lp64.shape))
    d = torch.where(ok, (lp - lp64).abs(), torch.zeros_like(lp64))
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    return float((d / E).max())


def vn_check_A(P, boards, observed, cs=None, tiny=False):
    """Measure A over what an implementation exposes.  observed: {index into [a1, a2, a3, hidden, out]: tensor}; each observed
    layer is bounded from the nearest observed layer before it (or the boards).  cs: per-layer constants for indices 0..3.
    -> {index: largest |error| / bound}"""
    layers, res = vn_layers(P), {}
    src, start = vn_input(boards), 0
    for i in sorted(observed):
        if i == 4:
            assert start == 4, "the outputs are bounded from the hidden layer"
            o64, E = vn_out_bound(P, src)
            res[4] = ratio_A(observed[4], o64, E)
            continue
        ch = chain_bound(layers[start:i + 1], src, None if cs is None else cs[start:i + 1], tiny)
        res[i] = ratio_A(observed[i], *ch[-1])
        src, start = observed[i].double().reshape(ch[-1][0].shape), i + 1
    return res


def dn_check_A(W, boards, observed, cs=None):
    """as vn_check_A over [a1, a2, hidden, p]; index 3 takes the probabilities (bounded in log p from the hidden layer; when
    the hidden layer was not observed, from the last observed layer through fc1, exact + E carried into the logits)"""
    layers, res = dn_layers(W), {}
    src, start = dn_input(boards), 0
    for i in sorted(observed):
        if i == 3:
            ch = chain_bound(layers[start:], src, None if cs is None else cs[start:])
            z, Ez = ch[-1]
            lp = F.log_softmax(z, 1)
            E = 2 * Ez.max(1, keepdim=True).values + U * (z - z.max(1, keepdim=True).values).abs() + 8 * U
            res[3] = ratio_logp(observed[3], lp, E.expand_as(lp))
            continue
        ch = chain_bound(layers[start:i + 1], src, None if cs is None else cs[start:i + 1])
        res[i] = ratio_A(observed[i], *ch[-1])
        src, start = observed[i].double().reshape(ch[-1][0].shape), i + 1
    return res


def assert_normal_range(acts):
    """the bounds ignore underflow: every nonzero activation of a regime is far above fp32's subnormals"""
    for a in acts:
        nz = a[a != 0].abs()
        assert nz.numel() == 0 or float(nz.min()) >= 2.0 ** -100, float(nz.min())
        assert bool(torch.isfinite(a).all())


# -------------------------------------------------------------------------------------------------------------- measure B
def errs_B(impl, ref32, ref64, per_column=False):
    """(err(impl), err(ref32), floor) = max |impl - fp64|, max |ref32 - fp64|, 4 u max |fp64|; per_column: one figure per column
    (the value net's v and var)"""
    impl, ref32, ref64 = (np.asarray(t, np.float64) for t in (impl, ref32, ref64))
    ax = 0 if per_column else None
    return np.abs(impl - ref64).max(axis=ax), np.abs(ref32 - ref64).max(axis=ax), 4 * U * np.abs(ref64).max(axis=ax)


def needed_M(e_impl, e_ref, floor):
    """the smallest M with e_impl <= M e_ref + floor (inf when e_ref = 0 and the floor does not cover the error)"""
    over = np.maximum(np.asarray(e_impl, np.float64) - floor, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = np.where(over == 0, 0.0, over / np.asarray(e_ref, np.float64))
    return float(np.max(m))


def vn_B(out_impl, out32, out64):
    """needed M over (v, var)"""
    return needed_M(*errs_B(out_impl, out32, out64, per_column=True))


def dn_B(p_impl, p32, p64):
    """distributional head: needed M on log p over the atoms with fp64 p >= 2^-100 and on |sum p - 1|; asserts that p is zero
    only where the fp64 p is below fp32's normal range"""
    p_impl, p32, p64 = (np.asarray(t, np.float64) for t in (p_impl, p32, p64))
    assert not np.any((p_impl == 0) & (p64 >= F32_MIN_NORMAL)), "a zero probability where fp64's is a normal fp32 number"
    assert np.all(np.isfinite(p_impl)) and np.all(p_impl >= 0)
    ok = p64 >= P_MIN_B
    with np.errstate(divide="ignore"):
        lp, lp32, lp64 = np.log(p_impl), np.log(p32), np.log(p64)
    z = lambda a: np.where(ok, a, 0.0)      # noqa: E731
    m_lp = needed_M(np.abs(z(lp) - z(lp64)).max(), np.abs(z(lp32) - z(lp64)).max(), 4 * U * np.abs(z(lp64)).max())
    m_sum = needed_M(np.abs(p_impl.sum(1) - 1).max(), np.abs(p32.sum(1) - 1).max(), 4 * U)
    return m_lp, m_sum


# Measure B's multiples.  The rule: the largest needed M over every regime x family, rounded up to the next power of two, measured
# with tests/test_heads_accuracy.py (its docstring and DESIGN.md section 6 have the figures) - the oracle for the fp32 kernels
# (4.21 / 4.78 -> 8), the numpy emulations for themselves (2.10 / 0.61 -> 4 / 1).  The split-precision KERNELS are held to the
# larger of their emulation's M and the fp32 path's: conv1, fc1 and the output layer run as the fp32 path's sequential fma chains
# and the matrix core adds its 6 x 18 (6 x 32) plane sums one after the other, while the emulations sum whole planes with numpy's
# blocked matmul - they model the split, not the order of summation.  Measured on the MI355X the kernels need 5.29 / 4.96, whose
# next power of two is the same 8.
M_VN_FP32, M_DN_FP32 = 8, 8
M_VN_X3_EMU, M_DN_X3_EMU = 4, 1
M_VN_X3, M_DN_X3 = max(M_VN_X3_EMU, M_VN_FP32), max(M_DN_X3_EMU, M_DN_FP32)
VALUE_REGIMES = ["params", "params2", "r05", "r06", "x4", "x0.25", "dead", "saturated", "train_ubound"]
DIST_REGIMES = (["fixture"] + ["seed%d" % a for a in (1, 7, 16, 17, 49, 50, 63, 64)]
                + ["peaked%d_%d" % (a, s) for a in (7, 50, 64) for s in (5, 50, 150)] + ["fitted"])


# ------------------------------------------------------------------------------------------------------------ the oracle
def orc_vn(oracle, P, boards):
    """oracle/valuenet_oracle.c on boards -> [n, 2] (v, var)"""
    s = np.ascontiguousarray(np.asarray(boards, np.int8).reshape(-1, 200))
    v, var = np.zeros(len(s), np.float32), np.zeros(len(s), np.float32)
    oracle.lib().orc_valuenet_forward(oracle.ptr(np.ascontiguousarray(P, np.float32)), oracle.ptr(s), len(s), oracle.ptr(v),
                                      oracle.ptr(var))
    return np.stack([v, var], 1)


def orc_dn(oracle, W, boards, atoms):
    """oracle/distnet_oracle.c on boards -> [n, atoms]"""
    s = np.ascontiguousarray(np.asarray(boards, np.int8).reshape(-1, 200))
    out = np.zeros((len(s), atoms), np.float32)
    oracle.lib().orc_distnet_forward(oracle.ptr(np.ascontiguousarray(dn_flat(W))), oracle.ptr(s), len(s), atoms, oracle.ptr(out))
    return out


# ---------------------------------------------------------------------------------------------------------------- boards
def fixture_boards():
    return np.load(os.path.join(GOLDEN, "ref_valuenet.npz"))["states"].astype(np.int8)


def ternary_boards(n=192, seed=20261016):
    rng = np.random.default_rng(seed)
    b = rng.integers(-1, 2, size=(n, 20, 10)).astype(np.int8)
    b[: n // 2, :10, :] = 0                   # half of them with an empty upper half, like real boards
    return b


def onehot_boards():
    """all 400 signed one-hot boards: a per-cell sensitivity map (a wrong tap at a border shows here and nowhere else)"""
    b = np.zeros((400, 20, 10), np.int8)
    for i in range(200):
        b[2 * i].reshape(200)[i] = 1
        b[2 * i + 1].reshape(200)[i] = -1
    return b


def uniform_boards():
    """empty, full, all -1, column stripes and row stripes (both phases)"""
    b = np.zeros((7, 20, 10), np.int8)
    b[1], b[2] = 1, -1
    b[3, :, 0::2], b[4, :, 1::2], b[5, 0::2, :], b[6, 1::2, :] = 1, 1, 1, 1
    return b


def played_boards(games=4, steps=140, every=7):
    """boards from play: the oracle engine under the action mix of tests/test_gpu_engine.py, getState() every few moves, all
    three `app` modes"""
    from oracle import binding as B
    out = []
    for app in (1, 2, 3):
        rng = np.random.default_rng(100 * app)
        gs = [B.Game(app, 0, 0, 777 + g) for g in range(games)]
        for t in range(steps):
            a = rng.choice(7, size=games, p=[0.1, 0.15, 0.15, 0.25, 0.1, 0.125, 0.125])
            for g, game in enumerate(gs):
                game.play(int(a[g]))
                if t % every == every - 1:
                    out.append(game.getState().copy())
                if game.end:
                    game.reset()
    return np.stack(out).astype(np.int8)


def board_families():
    return OrderedDict([("fixture", fixture_boards()), ("ternary", ternary_boards()), ("onehot", onehot_boards()),
                        ("uniform", uniform_boards()), ("played", played_boards())])


def golden_boards():
    """the ~300 boards of tests/golden/ref_heads_trained.npz: a cut through every family"""
    f = board_families()
    return np.concatenate([f["fixture"], f["ternary"][::3], f["onehot"][::4], f["uniform"], f["played"][::4]])


# --------------------------------------------------------------------------------------------------------------- regimes
def load_checkpoint(name):
    """flat parameters of a committed checkpoint (tetris_mcts_amd/checkpoints/value_net_online_<name>.pt)"""
    ck = torch.load(os.path.join(CHECKPOINTS, "value_net_online_%s.pt" % name), map_location="cpu")
    sd = ck["model_state_dict"]
    return np.concatenate([sd[k].detach().numpy().ravel() for k in VN_CKPT_KEYS]).astype(np.float32)


def _vn_set(P, key, value):
    P = P.copy()
    off = 0
    for k, shape in VN_SHAPES:
        n = int(np.prod(shape))
        if k == key:
            P[off:off + n] = np.asarray(value, np.float32).ravel()
        off += n
    return P


def value_regimes():
    """name -> 478342 floats.  Fresh and rescaled weights (the fixtures), both trained checkpoints, every learnable layer x4 and
    x0.25, a dead conv3 (a3 all zero), a saturated sigmoid (0 and 1), and out_ubound as train_data sets it from data."""
    z = np.load(os.path.join(GOLDEN, "ref_valuenet.npz"))
    p, p2 = z["params"].astype(np.float32), z["params2"].astype(np.float32)
    r = OrderedDict([("params", p), ("params2", p2), ("r05", load_checkpoint("r05")), ("r06", load_checkpoint("r06"))])
    for name, s in (("x4", 4.0), ("x0.25", 0.25)):
        q = p.copy()
        q[:VN_LEARNABLE] *= np.float32(s)
        r[name] = q
    r["dead"] = _vn_set(p2, "conv3.b", np.full(32, -1e3))
    r["saturated"] = _vn_set(p, "fc_out.b", [40.0, -40.0])
    # Model_VV.train_data: out_ubound = (values.max(), variances.max()) of the replay data - not round numbers
    rng = np.random.default_rng(11)
    values, variances = (rng.random(512) * 9000).astype(np.float32), (rng.random(512) * 3e5).astype(np.float32)
    r["train_ubound"] = _vn_set(r["r05"], "ub", [values.max(), variances.max()])
    return r


def subnormal_value_regime():
    """`params` rescaled by exact powers of two so that every single product of conv2 is below fp32's normal range (a1 ~ 2^-60,
    conv2's weights ~ 2^-72: products ~ 2^-134) while every sum is normal (conv2's bias, at least 2^-121 in magnitude, dominates
    them), and conv2's output (~ 2^-120) has bf16 `mid` and `lo` planes that are bf16 subnormals; conv3 and fc1 scale back up
    (2^96, 2^24)."""
    d = vn_split(np.load(os.path.join(GOLDEN, "ref_valuenet.npz"))["params"].astype(np.float32))
    d["conv2.b"] = np.copysign(np.maximum(np.abs(d["conv2.b"]), np.float32(2.0 ** -5)), d["conv2.b"])
    scale = {"conv1.w": -60, "conv1.b": -60, "conv2.w": -68, "conv2.b": -116, "conv3.w": 96, "conv3.b": -24, "fc1.w": 24}
    return np.concatenate([np.ldexp(d[k], scale.get(k, 0)).astype(np.float32).ravel() for k, _ in VN_SHAPES])


def seeded_dist_net(atoms, seed=None):
    """a fresh head at `atoms` outputs: torch's default initialisation (uniform in +-1/sqrt(fan_in)) drawn from numpy, so that
    the weights do not depend on the torch build"""
    rng = np.random.default_rng(1000 + atoms if seed is None else seed)
    shapes = [(32, 1, 4, 4), (32,), (32, 32, 4, 4), (32,), (128, 2048), (128,), (atoms, 128), (atoms,)]
    fan = [16, 16, 512, 512, 2048, 2048, 128, 128]
    return [rng.uniform(-1, 1, s).astype(np.float32) / np.float32(np.sqrt(f)) for s, f in zip(shapes, fan)]


def logit_spread(W, boards=None):
    """mean over the boards of the fp64 logits' max - min"""
    z = dn_forward(W, ternary_boards(64, 5) if boards is None else boards, torch.float64)[0][-1]
    return float((z.max(1).values - z.min(1).values).mean())


def peaked(W, spread):
    """the last layer scaled so that the fp64 logit spread is about `spread`"""
    s = np.float32(spread / logit_spread(W))
    return list(W[:6]) + [W[6] * s, W[7] * s]


def fixture_dist_net():
    z = np.load(os.path.join(GOLDEN, "ref_distnet.npz"))
    return [z[k] for k in DN_KEYS]


def fitted_dist_net():
    """the reference's Net after a short fit towards peaked targets (tests/golden/ref_heads_trained.npz)"""
    z = np.load(os.path.join(GOLDEN, "ref_heads_trained.npz"))
    return [z["dn_" + k] for k in DN_KEYS]


def dist_regimes(fitted=True):
    """name -> (atoms, [8 arrays]): the fixture net, seeded nets around the 16-atom tiles of k_dn_fc and at both ends, peaked
    variants (spread 5, 50, 150: at 150 some fp64 probabilities are below fp32's range) and the fitted net"""
    r = OrderedDict([("fixture", (50, fixture_dist_net()))])
    for a in (1, 7, 16, 17, 49, 50, 63, 64):
        r["seed%d" % a] = (a, seeded_dist_net(a))
    for a in (7, 50, 64):
        for s in (5, 50, 150):
            r["peaked%d_%d" % (a, s)] = (a, peaked(seeded_dist_net(a), s))
    if fitted:
        r["fitted"] = (50, fitted_dist_net())
    return r
