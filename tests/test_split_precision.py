"""The split-precision value-net backend ("hip_bf16x3", valuenet_x3.inc) on the build machine: the C ABI declares and exports it,
play.py passes it on, and a numpy emulation of its numerics contract holds the 1e-4 output contract."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TOL = 1e-4
OFF = dict(c1w=0, c1b=288, c2w=320, c2b=9536, c3w=9568, c3b=18784, f1w=18816, f1b=477568, fow=477824, fob=478336, ub=478338,
           lb=478340)


# ---- numpy emulation of the numerics contract ----
def bf16_rn(x):
    """fp32 -> the nearest bf16 (ties to even), as fp32.  Finite inputs only (the kernels use the hardware conversion, which also
    keeps NaNs and infinities; the bit trick here does not)."""
    x = np.ascontiguousarray(x, np.float32)
    assert np.isfinite(x).all()
    u = x.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def split3(x):
    """x = hi + mid + lo (+ a remainder below 2^-24 |x|), each a bf16 value; the differences are exact in fp32."""
    x = np.asarray(x, np.float32)
    hi = bf16_rn(x)
    r1 = (x - hi).astype(np.float32)
    mid = bf16_rn(r1)
    lo = bf16_rn((r1 - mid).astype(np.float32))
    return hi, mid, lo


# the plane products of each fp32 product, as (weight plane, activation plane) indices 0 hi / 1 mid / 2 lo
PRODUCTS = {"x3": ((1, 1), (2, 0), (0, 2), (1, 0), (0, 1), (0, 0)),      # i + j <= 2: the kernel's six
            "x3_nolo": ((1, 1), (1, 0), (0, 1), (0, 0)),                  # a dropped plane: what the bounds must catch
            "x3_nomidmid": ((2, 0), (0, 2), (1, 0), (0, 1), (0, 0))}


def _im2col(a, H, W):
    """a [n, 32, H, W] -> [n, (H-2)(W-2), 288] with k = tap * 32 + ci (the kernel's order of k)"""
    n = a.shape[0]
    cols = [a[:, :, ky:ky + H - 2, kx:kx + W - 2] for ky in range(3) for kx in range(3)]      # tap = ky * 3 + kx
    x = np.stack(cols, axis=1)                                                                # [n, 9, 32, OH, OW]
    return x.reshape(n, 288, (H - 2) * (W - 2)).transpose(0, 2, 1)


def _conv(a, w, b, H, W, mode):
    """3x3 valid conv 32 -> 32, ReLU.  w [32, 32, 3, 3]"""
    n, dt = a.shape[0], np.float64 if mode == "f64" else np.float32
    wk = w.reshape(32, 32, 9).transpose(0, 2, 1).reshape(32, 288).astype(dt)                # [co, tap * 32 + ci]
    x = _im2col(a.astype(dt), H, W)
    if mode in ("f64", "f32"):
        y = x @ wk.T
    else:
        # every plane product is exact in fp32 (8 x 8 significant bits); each is summed over k in fp32 (the matrix core's
        # accumulator), and the products in fp32
        wp, xp = split3(wk), split3(x)
        y = np.zeros(x.shape[:2] + (32,), np.float32)
        for i, j in PRODUCTS[mode]:
            y = (y + xp[j] @ wp[i].T).astype(np.float32)
    y = (y + b.astype(dt)).astype(dt)
    y = np.maximum(y, 0)
    return y.transpose(0, 2, 1).reshape(n, 32, H - 2, W - 2)


def forward(P, states, mode, a3_only=False):
    """The value net on int8 states [n, 20, 10]: mode "f64" (reference in double), "f32" (the fp32 path's arithmetic, any
    summation order) or one of PRODUCTS (conv2 and conv3 as plane products; conv1, fc1, the output layer in fp32).
    a3_only: conv3's output [n, 1792] (channel-major, the kernels' a3 rows) instead of (v, var) [n, 2]."""
    dt = np.float64 if mode == "f64" else np.float32
    P = np.asarray(P, np.float32)
    g = lambda k, n: P[OFF[k]:OFF[k] + n].astype(dt)
    x = np.asarray(states, dt).reshape(-1, 1, 20, 10)
    n = x.shape[0]
    w1 = g("c1w", 288).reshape(32, 9)
    cols = np.stack([x[:, 0, ky:ky + 18, kx:kx + 8] for ky in range(3) for kx in range(3)], axis=1).reshape(n, 9, 144)
    a1 = np.maximum((np.einsum("ck,nkp->ncp", w1, cols) + g("c1b", 32)[None, :, None]).astype(dt), 0).reshape(n, 32, 18, 8)
    a2 = _conv(a1, g("c2w", 9216).reshape(32, 32, 3, 3), g("c2b", 32), 18, 8, mode)
    a3 = _conv(a2, g("c3w", 9216).reshape(32, 32, 3, 3), g("c3b", 32), 16, 6, mode)
    if a3_only:
        return a3.reshape(n, 1792).astype(np.float64)
    h =np.maximum((a3.reshape(n, 1792) @ g("f1w", 458752).reshape(256, 1792).T + g("f1b", 256)).astype(dt), 0)
    o = (h @ g("fow", 512).reshape(2, 256).T + g("fob", 2)).astype(np.float64)
    sg = 1.0 / (1.0 + np.exp(-o))
    return (sg.astype(dt) * g("ub", 2) + g("lb", 2)).astype(np.float64)


def _tol(P):
    """1e-4, scaled as tests/test_gpu_valuenet.py scales it: (v, var)"""
    return np.array([TOL * max(1.0, float(P[478338]) / 100.0), TOL * max(1.0, float(P[478339]) / 1000.0)])


def test_split_is_exact_to_fp32():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(100000) * np.exp(rng.uniform(-20, 20, 100000))).astype(np.float32)
    hi, mid, lo = split3(x)
    for p in (hi, mid, lo):
        assert np.array_equal(bf16_rn(p), p)            # every plane is a bf16 value
    r = x.astype(np.float64) - hi - mid - lo
    assert np.all(np.abs(r) <= np.abs(x.astype(np.float64)) * 2.0 ** -24)
    assert np.array_equal(bf16_rn(np.float32([1.0, -2.5, 0.0])), np.float32([1.0, -2.5, 0.0]))
    # ties to even: 1 + 2^-8 lies halfway between 1 and 1 + 2^-7
    assert bf16_rn(np.float32([1.0 + 2.0 ** -8]))[0] == 1.0


def test_emulated_split_holds_the_output_contract():
    z = np.load(os.path.join(GOLDEN, "ref_valuenet.npz"))
    for pk, ok in (("params", "out"), ("params2", "out2")):
        P, S = z[pk], z["states"]
        r64 = forward(P, S, "f64")
        e32 = np.abs(forward(P, S, "f32") - r64).max(axis=0)
        x3 = forward(P, S, "x3")
        e3 = np.abs(x3 - r64).max(axis=0)
        tol = _tol(P)
        # the reference's own outputs and the fp64 forward, within the output contract
        assert np.all(np.abs(x3 - z[ok]).max(axis=0) <= tol), pk
        assert np.all(e3 <= tol), pk
        # as accurate as fp32 arithmetic: within a few times the fp32 forward's error (+ a floor of a few fp32 ulps of the
        # outputs, for an output the fp32 forward happens to round right)
        floor = 4 * np.abs(r64).max(axis=0) * 2.0 ** -24
        assert np.all(e3 <= 2 * e32 + floor), (pk, e3, e32)
        # ... and so are the split convolutions themselves (conv3's output, where fc1's fp32 rounding does not hide them),
        # a bound that a dropped plane breaks twice over
        a64 = forward(P, S, "f64", a3_only=True)
        a32 = np.abs(forward(P, S, "f32", a3_only=True) - a64).max()
        ax3 = np.abs(forward(P, S, "x3", a3_only=True) - a64).max()
        assert ax3 <= 2 * a32, (pk, ax3, a32)
        for drop in ("x3_nolo", "x3_nomidmid"):
            ad = np.abs(forward(P, S, drop, a3_only=True) - a64).max()
            assert ad > 4 * a32, (pk, drop, ad, a32)


def test_library_exports_the_split_precision_abi():
    import abi_shape
    abi_shape.check(abi_shape.VALUENET)
    abi_shape.check_defines((("TM_VALUENET_PREPARED_X3", 27648), ("TM_VALUENET_FP32", 0), ("TM_VALUENET_BF16X3", 1)))
    from tetris_mcts_amd import model
    assert model.PREPARED_X3 == 27648 and model.VALUENET_BACKEND == {"hip": 0, "hip_bf16x3": 1}
    assert "hip_bf16x3" in model.HIP_BACKENDS


def test_build_rebuilds_valuenet_when_the_x3_kernels_change():
    src = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "valuenet_x3.inc" in src
    assert re.search(r'#include\s+"valuenet_x3.inc"', open(os.path.join(ROOT, "tetris_mcts_amd", "csrc", "valuenet.hip")).read())


def test_play_cli_takes_the_backend_and_keeps_the_reference_flags():
    import play
    p = play.build_parser()
    assert p.parse_args([]).valuenet_backend == "hip"
    assert p.parse_args(["--valuenet_backend", "hip_bf16x3"]).valuenet_backend == "hip_bf16x3"
    assert p.parse_args(["--valuenet_backend", "torch"]).valuenet_backend == "torch"
    ref = dict(agent_type=None, app=1, benchmark=False, cycle=0, endless=False, gamma=0.9, gui=False, interactive=False,
               mcts_const=5.0, mcts_sims=50, mcts_tau=1.0, min_visit=40, ngames=50, online=False, printboard=False,
               print_board_to_file=False, realtime_status=False, save=False, save_dir='./data/', save_file='data',
               save_tree=False, tetris_randomizer=0, tetris_scoring=0)
    d = vars(p.parse_args(["--valuenet_backend", "hip_bf16x3"]))
    for k, v in ref.items():
        assert d[k] == v and type(d[k]) is type(v), k
    try:
        p.parse_args(["--valuenet_backend", "bf16"])
    except SystemExit:
        pass
    else:
        raise AssertionError("an unknown backend must be refused")


def test_agents_take_the_backend_keyword():
    """The keyword reaches the model the agent builds, and ValueSim / ValueSimLP / ValueSimC hand a "hip_bf16x3" model to the
    native search loop (search_model) like a "hip" one - without it they would fall back to the Python-driven loop."""
    import inspect
    from tetris_mcts_amd.agents import ValueSim
    assert inspect.signature(ValueSim.__init__).parameters["valuenet_backend"].default == "hip"
    src = inspect.getsource(ValueSim)
    assert "Model(backend=valuenet_backend)" in src
    for name in ("ValueSim", "ValueSimLP", "ValueSimC"):
        import tetris_mcts_amd.agents as A
        cls = getattr(A, name)
        fake = cls.__new__(cls)
        fake.evaluator = None
        fake.model = type("M", (), {"backend": "hip_bf16x3"})()
        assert fake.search_model() is fake.model, name
        fake.model = type("M", (), {"backend": "torch"})()
        assert fake.search_model() is False, name
