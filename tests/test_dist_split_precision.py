"""The split-precision backend of the distributional head ("hip_bf16x3", distnet_x3.inc) on the build machine: the C ABI declares
and exports it, DistValueSim and play.py pass it on, and a numpy emulation of its numerics contract
holds the head's 1e-6 relative contract against the reference's own Net."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KEYS = ["seq__conv1__weight", "seq__conv1__bias", "seq__conv2__weight", "seq__conv2__bias", "seq__fc1__weight",
        "seq__fc1__bias", "seq__fc_v__weight", "seq__fc_v__bias"]


# ---- numpy emulation of the numerics contract ----
def bf16_rn(x):
    """fp32 -> the nearest bf16 (ties to even), as fp32 (finite inputs)"""
    x = np.ascontiguousarray(x, np.float32)
    assert np.isfinite(x).all()
    u = x.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def split3(x):
    """x = hi + mid + lo (+ a remainder below 2^-24 |x|), each a bf16 value; the differences are exact in fp32"""
    x = np.asarray(x, np.float32)
    hi = bf16_rn(x)
    r1 = (x - hi).astype(np.float32)
    mid = bf16_rn(r1)
    return hi, mid, bf16_rn((r1 - mid).astype(np.float32))


# the plane products of each fp32 product in the order they are accumulated, as (weight plane, activation plane) indices
# 0 hi / 1 mid / 2 lo
PRODUCTS = {"x3": ((1, 1), (2, 0), (0, 2), (1, 0), (0, 1), (0, 0)),      # i + j <= 2: the kernel's six
            "x3_nolo": ((1, 1), (1, 0), (0, 1), (0, 0)),                  # a dropped plane: what the bounds must catch
            "x3_nomidmid": ((2, 0), (0, 2), (1, 0), (0, 1), (0, 0))}


def _leaky(x):
    return np.where(x > 0, x, x * x.dtype.type(0.01))


def _cols(a, k=4):
    """a [n, C, H, W] -> [n, (H-k+1)(W-k+1), k*k*C] with column tap * C + c, tap = ky * k + kx (the kernel's order of k)"""
    n, c, h, w = a.shape
    oh, ow = h - k + 1, w - k + 1
    x = np.stack([a[:, :, ky:ky + oh, kx:kx + ow] for ky in range(k) for kx in range(k)], axis=1)    # [n, taps, C, OH, OW]
    return x.reshape(n, k * k * c, oh * ow).transpose(0, 2, 1)


def _conv2(a1, w, b, mode):
    """conv2 (4x4 valid, 32 -> 32 channels, 19 x 7 -> 16 x 4) before the activation: [n, 32 channels, 64 positions]"""
    dt = np.float64 if mode == "f64" else np.float32
    wk = w.reshape(32, 32, 16).transpose(0, 2, 1).reshape(32, 512).astype(dt)                # [co, tap * 32 + ci]
    x = _cols(a1.astype(dt))                                                                   # [n, 64, 512]
    if mode in ("f64", "f32"):
        y = (x @ wk.T + b.astype(dt)).astype(dt)
    else:
        # the matrix core per step of 16 k: each plane product is exact, its 16 terms are summed (here in fp64) and rounded
        # once to fp32, then added to the fp32 accumulator, which starts at the bias; the products in the contract's order
        wp, xp = split3(wk), split3(x)
        y = np.broadcast_to(b.astype(np.float32), x.shape[:2] + (32,)).copy()
        for s in range(32):
            ks = slice(16 * s, 16 * s + 16)
            for i, j in PRODUCTS[mode]:
                part = (xp[j][:, :, ks].astype(np.float64) @ wp[i][:, ks].T.astype(np.float64)).astype(np.float32)
                y = (y + part).astype(np.float32)
    return y.transpose(0, 2, 1)


def forward(P, x, mode, a2_only=False):
    """The head on float boards [n, 1, 22, 10]: mode "f64" (reference in double), "f32" (fp32 matmuls, any summation order) or
    one of PRODUCTS (conv2 as plane products; conv1, fc1, fc_v in fp32).  a2_only: conv2's LeakyReLU'd output [n, 2048] in
    the flatten order co*64 + y*4 + x (the kernels' scratch rows) instead of the softmax [n, atoms]."""
    dt = np.float64 if mode == "f64" else np.float32
    c1w, c1b, c2w, c2b, f1w, f1b, fvw, fvb = (np.asarray(p).astype(dt) for p in P)
    x = np.asarray(x, dt)
    n = x.shape[0]
    a1 = _leaky((_cols(x) @ c1w.reshape(32, 16).T + c1b).astype(dt))                          # [n, 133, 32]
    a1 = a1.transpose(0, 2, 1).reshape(n, 32, 19, 7)
    a2 = _leaky(_conv2(a1, c2w, c2b, mode).astype(dt)).reshape(n, 2048)
    if a2_only:
        return a2.astype(np.float64)
    h = _leaky((a2 @ f1w.T + f1b).astype(dt))
    lg = (h @ fvw.T + fvb).astype(dt).astype(np.float64)
    e = np.exp(lg - lg.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def _fixture():
    z = np.load(os.path.join(GOLDEN, "ref_distnet.npz"))
    return z, [z[k] for k in KEYS]


def _random_boards(n=256, seed=20261016):
    rng = np.random.default_rng(seed)
    x = np.zeros((n, 1, 22, 10), np.float32)
    x[:, 0, 2:, :] = rng.integers(-1, 2, size=(n, 20, 10))
    x[: n // 2, 0, 2:12, :] = 0                   # half of them with an empty upper half, like real boards
    return x


def test_emulated_split_holds_the_output_contract():
    """the head's 1e-6 relative contract against the reference's own outputs, elementwise"""
    z, P = _fixture()
    y = forward(P, z["x"], "x3")
    ref = z["y"].astype(np.float64)
    assert np.abs(y - ref).max() <= 1e-6 * np.abs(ref).max()
    assert np.all(np.abs(y - ref) <= 1e-6 * ref + 1e-9)


@pytest.mark.parametrize("boards", ["fixture", "random"])
def test_emulated_split_conv2_is_as_accurate_as_fp32(boards):
    """conv2's output (a2, where fc1's fp32 rounding does not hide it) within 2x the fp32 arithmetic's error against fp64 plus a
    floor of a few fp32 ulps; a dropped plane breaks that bound"""
    z, P = _fixture()
    x = z["x"] if boards == "fixture" else _random_boards()
    a64 = forward(P, x, "f64", a2_only=True)
    e32 = np.abs(forward(P, x, "f32", a2_only=True) - a64).max()
    floor = 4 * np.abs(a64).max() * 2.0 ** -24
    ex3 = np.abs(forward(P, x, "x3", a2_only=True) - a64).max()
    assert ex3 <= 2 * e32 + floor, (ex3, e32, floor)
    for drop in ("x3_nolo", "x3_nomidmid"):
        ed = np.abs(forward(P, x, drop, a2_only=True) - a64).max()
        assert ed > 2 * e32 + floor, (drop, ed, e32, floor)
    # and the distribution, on the same boards: as close to the fp64 forward as the fp32 arithmetic's, within a floor
    p64 = forward(P, x, "f64")
    p32 = np.abs(forward(P, x, "f32") - p64).max()
    px3 = np.abs(forward(P, x, "x3") - p64).max()
    assert px3 <= 2 * p32 + 4 * np.abs(p64).max() * 2.0 ** -24, (px3, p32)


# ---- every layer accepts the backend ----
def test_library_exports_the_split_precision_abi():
    import abi_shape
    abi_shape.check(abi_shape.DISTNET)
    abi_shape.check_defines((("TM_DISTNET_PREPARED_X3", 24576),))
    from tetris_mcts_amd import model_distributional as md
    assert md.PREPARED_X3 == 24576
    assert md.HIP_BACKENDS == ("hip", "hip_bf16x3")


def test_build_rebuilds_distnet_when_the_x3_kernel_changes():
    src = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "distnet_x3.inc" in src
    assert re.search(r'#include\s+"distnet_x3.inc"', open(os.path.join(ROOT, "tetris_mcts_amd", "csrc", "distnet.hip")).read())


def test_dist_agent_takes_the_backend_keyword():
    """the keyword reaches the model the agent builds, and DistValueSim hands a "hip_bf16x3" model to the native search loop
    (search_model) like a "hip" one - without it, the Python-driven loop would run it"""
    import inspect
    from tetris_mcts_amd.agents import DistValueSim
    assert inspect.signature(DistValueSim.__init__).parameters["valuenet_backend"].default is None
    assert "backend=valuenet_backend" in inspect.getsource(DistValueSim.__init__)
    fake = DistValueSim.__new__(DistValueSim)
    fake.evaluator = None
    for backend, native in (("hip", True), ("hip_bf16x3", True), ("torch", False)):
        fake.model = type("M", (), {"backend": backend})()
        assert fake.search_model() is (fake.model if native else False), backend


def test_play_passes_the_backend_to_the_dist_agent(monkeypatch):
    import agents.DistValueSim as agent_module
    import play
    import pyTetris

    class Reached(Exception):
        pass

    seen = {}

    def recorder(**kwargs):
        seen.update(kwargs)
        raise Reached()

    monkeypatch.setattr(pyTetris, "Tetris", lambda *a, **k: None)      # (the real one needs a GPU)
    monkeypatch.setattr(agent_module, "DistValueSim", recorder)
    with pytest.raises(Reached):
        play.main(["--agent_type", "DistValueSim", "--valuenet_backend", "hip_bf16x3", "--mcts_sims", "8"])
    assert seen["valuenet_backend"] == "hip_bf16x3" and seen["sims"] == 8
