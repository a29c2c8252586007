"""Accuracy of the two evaluators at trained-scale weights, on the CPU: the oracle's fma chains (which the GPU tests hold
bit-equal to the fp32 kernels) and the numpy emulations of the split-precision backends, against an fp64 forward, with the
reference's own fp32 arithmetic (torch CPU fp32) as the yardstick.  tests/heads_numerics.py has the regimes, the board
families, the forwards and the derivations of the two measures.

Measure B, err(impl) <= M * err(ref32) + 4 * 2^-24 * max |fp64 output|.  M by the rule "largest needed M over every regime x
family, rounded up to the next power of two", measured with this file (needed M = (err(impl) - floor) / err(ref32)):

    head            implementation                 largest needed M   where                      M
    value net       oracle fma chains (= "hip")    4.21               x4 / ternary               8
    value net       numpy bf16x3 emulation         2.10               x4 / uniform               4
    distributional  oracle fma chains (= "hip")    4.78 (log p)       peaked7_150 / onehot       8
    distributional  numpy bf16x3 emulation         0.61 (log p)       peaked50_150 / fixture     1

(|sum p - 1| never needed more than the floor.)  The emulations sum every plane product and the fc layers with numpy's blocked
fp32 matmul; the kernels add the matrix core's plane sums one after the other and run fc1 / the output layer as one sequential
fma chain (K = 1792 / 2048), which is where the oracle's 4-5 comes from.  With the fc layers summed sequentially the emulations
still need only 1.8 / 3.8: they model the split, not the order of summation.  The GPU test therefore holds the split-precision
kernels to the larger of the emulation's M and the fp32 path's, 8 (heads_numerics.M_*); measured there: 5.29 / 4.96.

Measure A on the torch fp32 forward, the largest |error| / bound over every regime and family (smallest per-regime maximum
in brackets):

    value net       conv1 0.29 (0.08)  conv2 0.012  conv3 0.011  fc1 0.0037  outputs from the hidden layer 0.22
                    a3 from the boards, three layers deep 0.0008
    distributional  conv1 0.24  conv2 0.013  fc1 0.0021  log p from the hidden layer 0.078
                    two deep: a2 from the boards 0.012
    emulations      value a3 three deep (c_x3) 0.0001, distributional a2 two deep (c_x3) 0.0023

The mutation list (test_wrong_*_layers_exceed_the_bound, test_softmax_without_max_subtraction_exceeds_the_bound): every variant
exceeds the bound in every regime in which it changes the layer's output at all; none had to be removed.
"""
import functools
import os

import numpy as np
import pytest
import torch

import heads_numerics as H

from heads_numerics import (DIST_REGIMES, M_DN_FP32, M_DN_X3_EMU, M_VN_FP32, M_VN_X3_EMU, VALUE_REGIMES, orc_dn, orc_vn)


@functools.lru_cache(None)
def families():
    return H.board_families()


@functools.lru_cache(None)
def vregimes():
    r = H.value_regimes()
    assert list(r) == VALUE_REGIMES
    return r


@functools.lru_cache(None)
def dregimes():
    r = H.dist_regimes()
    assert list(r) == DIST_REGIMES
    return r


# ------------------------------------------------------------------------------------------ the helper against the reference
def test_helper_forwards_equal_the_reference_nets():
    """tests/golden/ref_heads_trained.npz (the reference's own Net classes, make_golden.gen_heads_trained) against the helper's
    torch forwards: fp64 to 1e-12 relative; fp32 bit for bit where this CPU and torch build sum as the generating one did,
    and always within measure B with M = 1 plus the floor."""
    z = np.load(os.path.join(H.GOLDEN, "ref_heads_trained.npz"))
    boards = z["boards"]
    assert np.array_equal(boards, H.golden_boards())
    P = vregimes()["r06"]
    o64 = H.vn_forward(P, boards, torch.float64)[1].numpy()
    o32 = H.vn_forward(P, boards, torch.float32)[1].numpy()
    assert np.all(np.abs(o64 - z["vn_out64"]) <= 1e-12 * np.abs(z["vn_out64"]).max(0))
    if not np.array_equal(o32, z["vn_out32"]):
        assert H.vn_B(o32, z["vn_out32"], z["vn_out64"]) <= 1
    W = H.fitted_dist_net()
    lp64 = torch.log_softmax(H.dn_forward(W, boards, torch.float64)[0][-1], 1).numpy()
    lp32 = torch.log_softmax(H.dn_forward(W, boards, torch.float32)[0][-1], 1).numpy()
    assert np.abs(lp64 - z["dn_lp64"]).max() <= 1e-12 * np.abs(z["dn_lp64"]).max()
    if not np.array_equal(lp32, z["dn_lp32"]):
        e, e_ref = np.abs(lp32 - z["dn_lp64"]).max(), np.abs(z["dn_lp32"] - z["dn_lp64"]).max()
        assert e <= e_ref + 4 * H.U * np.abs(z["dn_lp64"]).max(), (e, e_ref)
    # the fit made a peaked head out of every layer: the spread of log p is far beyond the random-init fixture's 0.3
    assert float((z["dn_lp64"].max(1) - z["dn_lp64"].min(1)).mean()) > 5


# ----------------------------------------------------------------------------------------------------------- measure B
@pytest.mark.parametrize("regime", VALUE_REGIMES)
def test_value_oracle_measure_B(oracle, regime):
    P = vregimes()[regime]
    for fam, boards in families().items():
        acts64, o64 = H.vn_forward(P, boards, torch.float64)
        H.assert_normal_range(acts64)
        o32 = H.vn_forward(P, boards, torch.float32)[1]
        got = orc_vn(oracle, P, boards)
        e, e_ref, floor = H.errs_B(got, o32.numpy(), o64.numpy(), per_column=True)
        m = H.needed_M(e, e_ref, floor)
        print("B value oracle %-12s %-8s err %s ref32 %s floor %s needed M %.2f" % (regime, fam, e, e_ref, floor, m))
        assert m <= M_VN_FP32, (regime, fam, e, e_ref, floor)


@pytest.mark.parametrize("regime", DIST_REGIMES)
def test_dist_oracle_measure_B(oracle, regime):
    atoms, W = dregimes()[regime]
    for fam, boards in families().items():
        acts64, p64 = H.dn_forward(W, boards, torch.float64)
        H.assert_normal_range(acts64[:-1])
        p32 = H.dn_forward(W, boards, torch.float32)[1]
        got = orc_dn(oracle, W, boards, atoms)
        m_lp, m_sum = H.dn_B(got, p32.numpy(), p64.numpy())
        print("B dist oracle %-12s %-8s needed M log p %.2f sum %.2f" % (regime, fam, m_lp, m_sum))
        assert m_lp <= M_DN_FP32 and m_sum <= M_DN_FP32, (regime, fam, m_lp, m_sum)


@pytest.mark.parametrize("regime", VALUE_REGIMES)
def test_value_x3_emulation_measures_A_and_B(regime):
    """the numpy emulation of valuenet_x3.inc's contract (tests/test_split_precision.py): measure B end to end, measure A on
    conv3's output three layers deep (conv1 fp32, conv2 and conv3 split: heads_numerics.c_x3); every second board of the
    large families"""
    import test_split_precision as X
    P = vregimes()[regime]
    cs = [None, H.c_x3(288), H.c_x3(288)]
    for fam, boards in families().items():
        boards = boards[::2] if len(boards) > 100 else boards
        o64 = H.vn_forward(P, boards, torch.float64)[1].numpy()
        o32 = H.vn_forward(P, boards, torch.float32)[1].numpy()
        got = X.forward(P, boards, "x3")
        e, e_ref, floor = H.errs_B(got, o32, o64, per_column=True)
        m = H.needed_M(e, e_ref, floor)
        a3 = torch.from_numpy(X.forward(P, boards, "x3", a3_only=True))
        rA = H.vn_check_A(P, boards, {2: a3}, cs + [None])[2]
        print("B value x3emu %-12s %-8s err %s ref32 %s needed M %.2f | A a3 %.4f" % (regime, fam, e, e_ref, m, rA))
        assert m <= M_VN_X3_EMU, (regime, fam, e, e_ref, floor)
        assert rA <= 1, (regime, fam, rA)


@pytest.mark.parametrize("regime", DIST_REGIMES)
def test_dist_x3_emulation_measures_A_and_B(regime):
    """the numpy emulation of distnet_x3.inc's contract (tests/test_dist_split_precision.py): measure B on log p, measure A on
    conv2's output two layers deep (conv1 fp32, conv2 split); a quarter / a half of the boards of the larger families"""
    import test_dist_split_precision as X
    atoms, W = dregimes()[regime]
    for fam, boards in families().items():
        boards = boards[::4] if len(boards) > 100 else boards[::2] if len(boards) > 20 else boards
        x = H.dn_input(boards).numpy()
        p64 = H.dn_forward(W, boards, torch.float64)[1].numpy()
        p32 = H.dn_forward(W, boards, torch.float32)[1].numpy()
        m_lp, m_sum = H.dn_B(X.forward(W, x, "x3"), p32, p64)
        a2 = torch.from_numpy(X.forward(W, x, "x3", a2_only=True))
        rA = H.dn_check_A(W, boards, {1: a2}, [None, H.c_x3(512), None, None])[1]
        print("B dist x3emu %-12s %-8s needed M log p %.2f sum %.2f | A a2 %.4f" % (regime, fam, m_lp, m_sum, rA))
        assert m_lp <= M_DN_X3_EMU and m_sum <= M_DN_X3_EMU, (regime, fam, m_lp, m_sum)
        assert rA <= 1, (regime, fam, rA)


# ----------------------------------------------------------------------------------------------------------- measure A
@pytest.mark.parametrize("regime", VALUE_REGIMES)
def test_value_measure_A_holds_for_the_reference_arithmetic(regime):
    """every layer of the torch fp32 forward within its bound, from its own actual input (one layer deep), the outputs from the
    hidden layer, and a3 from the boards (three layers deep, the form the GPU test uses where a1 and a2 are not kept)"""
    P = vregimes()[regime]
    for fam, boards in families().items():
        acts, out = H.vn_forward(P, boards, torch.float32)
        r = H.vn_check_A(P, boards, {0: acts[0], 1: acts[1], 2: acts[2], 3: acts[3], 4: out})
        deep = H.vn_check_A(P, boards, {2: acts[2]})[2]
        print("A value torch32 %-12s %-8s conv1 %.4f conv2 %.4f conv3 %.4f fc1 %.4f out %.4f | a3 from the boards %.5f" % (
            regime, fam, r[0], r[1], r[2], r[3], r[4], deep))
        assert max(r.values()) <= 1 and deep <= 1, (regime, fam, r, deep)


@pytest.mark.parametrize("regime", DIST_REGIMES)
def test_dist_measure_A_holds_for_the_reference_arithmetic(regime):
    atoms, W = dregimes()[regime]
    for fam, boards in families().items():
        acts, p = H.dn_forward(W, boards, torch.float32)
        r = H.dn_check_A(W, boards, {0: acts[0], 1: acts[1], 2: acts[2], 3: p})
        deep = H.dn_check_A(W, boards, {1: acts[1], 3: p})
        print("A dist torch32 %-12s %-8s conv1 %.4f conv2 %.4f fc1 %.4f log p %.4f | two deep: a2 %.4f log p %.4f" % (
            regime, fam, r[0], r[1], r[2], r[3], deep[1], deep[3]))
        assert max(r.values()) <= 1 and max(deep.values()) <= 1, (regime, fam, r, deep)


# ------------------------------------------------------------------------------------------------------- the bound bites
def _variants(L, first_fc):
    """deliberately wrong fp64 versions of one layer: name -> (layer, transform of its input)"""
    ident = lambda x: x       # noqa: E731
    v = {}
    if L.kind == "conv":
        v["taps transposed"] = (L.replace(w=L.w.transpose(0, 1, 3, 2)), ident)
        v["window shifted one column"] = (L, lambda x: torch.roll(x, 1, -1))
    w = L.w.copy()
    w.reshape(w.shape[0], -1)[:, -1] = 0
    v["last k term dropped"] = (L.replace(w=w), ident)
    v["bias added twice"] = (L.replace(b=2 * L.b), ident)
    if L.act == "leaky":
        v["ReLU for LeakyReLU"] = (L.replace(act="relu"), ident)
    if first_fc:
        v["flatten position-major"] = (L, lambda x: x.permute(0, 2, 3, 1).contiguous())
    if L.name == "fc_v" and L.w.shape[0] > 1:
        sw = np.arange(L.w.shape[0])
        sw[[0, 1]] = [1, 0]
        v["two atoms swapped"] = (L.replace(w=L.w[sw], b=L.b[sw]), ident)
    return v


def _mutations(layers, x0):
    """(layer, variant, differs, exceeds) for every wrong variant of every layer, each layer fed its actual fp32 input"""
    boards_x = x0
    acts = H.run_layers(layers, boards_x, torch.float32)
    for i, L in enumerate(layers):
        x_in = (boards_x if i == 0 else acts[i - 1]).double()
        (a64, E), = H.chain_bound([L], x_in)
        for name, (Lm, tf) in _variants(L, L.kind == "fc" and i > 0 and layers[i - 1].kind == "conv").items():
            wm, bm = Lm.tensors(torch.float64)
            am = H.act(Lm, H.lin(Lm, tf(x_in), wm, bm))
            d = (am - a64).abs()
            yield L.name, name, bool((d > 0).any()), bool((d > E).any())


ALL_BOARDS = lambda: np.concatenate(list(families().values()))[::2]      # noqa: E731


@pytest.mark.parametrize("regime", VALUE_REGIMES)
def test_wrong_value_layers_exceed_the_bound(regime):
    """Measure A bites: taps transposed, the window shifted by a column, the last k term dropped, the bias added twice, the
    flatten order position-major - each, in each layer it applies to, exceeds the layer's bound on at least one board of the
    committed families, in every regime where the variant changes the layer's output at all (in the "dead" regime conv3's
    output and fc1's input are zero whatever the taps are; under the checkpoints the last hidden unit is dead, so dropping
    fc_out's last term changes nothing)."""
    seen = 0
    for layer, name, differs, exceeds in _mutations(H.vn_layers(vregimes()[regime]), H.vn_input(ALL_BOARDS())):
        print("mutation value %-12s %-7s %-28s differs %d exceeds %d" % (regime, layer, name, differs, exceeds))
        assert exceeds or not differs, (regime, layer, name)
        seen += exceeds
    assert seen >= 10, seen


@pytest.mark.parametrize("regime", DIST_REGIMES)
def test_wrong_dist_layers_exceed_the_bound(regime):
    """as above for the distributional head, plus ReLU where LeakyReLU belongs and two atoms swapped (on the logits)"""
    atoms, W = dregimes()[regime]
    seen = 0
    for layer, name, differs, exceeds in _mutations(H.dn_layers(W), H.dn_input(ALL_BOARDS())):
        print("mutation dist %-12s %-7s %-28s differs %d exceeds %d" % (regime, layer, name, differs, exceeds))
        assert exceeds or not differs, (regime, layer, name)
        seen += exceeds
    assert seen >= 12, seen


@pytest.mark.parametrize("regime", ["peaked7_150", "peaked50_150", "peaked64_150"])
def test_softmax_without_max_subtraction_exceeds_the_bound(regime):
    """an fp32 softmax that does not subtract the maximum, at a logit spread of 150: exp overflows or the small terms vanish
    against the sum - log p leaves its bound (or is NaN) on at least one board"""
    atoms, W = dregimes()[regime]
    boards = ALL_BOARDS()
    acts, p = H.dn_forward(W, boards, torch.float32)
    lp64, E, _ = H.dn_logp_bound(W, acts[2])
    assert H.ratio_logp(p, lp64, E) <= 1
    e = torch.exp(acts[3])
    bad = e / e.sum(1, keepdim=True)
    assert H.ratio_logp(bad, lp64, E) > 1


# -------------------------------------------------------------------------------------------------- orc_exp, saturation
def test_orc_exp_beyond_40_and_its_clamp(oracle):
    import math
    L = oracle.lib()
    for x in np.concatenate([np.linspace(-700, 700, 2801), np.random.default_rng(1).uniform(-700, 700, 2000)]):
        assert abs(L.orc_exp(float(x)) / math.exp(x) - 1) < 4e-16, x
    for x in (700.0001, 710.0, 1e3, 1e300, float("inf")):
        assert L.orc_exp(x) == L.orc_exp(700.0)
        assert L.orc_exp(-x) == L.orc_exp(-700.0)
    assert L.orc_exp(700.0) == pytest.approx(math.exp(700.0), rel=4e-16)
    assert L.orc_exp(-700.0) == pytest.approx(math.exp(-700.0), rel=4e-16)


def test_saturated_outputs_are_the_bounds_to_an_ulp(oracle):
    """fc_out's bias at +-40: v = ub + lb and var = lb, to an ulp"""
    P = vregimes()["saturated"]
    d = H.vn_split(P)
    ub, lb = d["ub"].astype(np.float64), d["lb"].astype(np.float64)
    for fam, boards in families().items():
        got = orc_vn(oracle, P, boards).astype(np.float64)
        z = H.vn_forward(P, boards, torch.float64)[0][-1].numpy()
        assert z[:, 0].min() > 30 and z[:, 1].max() < -30, (fam, z[:, 0].min(), z[:, 1].max())
        assert np.all(np.abs(got[:, 0] - (ub[0] + lb[0])) <= np.spacing(np.float32(ub[0] + lb[0]))), fam
        assert np.all(np.abs(got[:, 1] - lb[1]) <= np.spacing(np.float32(lb[1]))), fam
