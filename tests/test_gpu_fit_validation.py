"""The HIP validation pass of the fits on the GPU (tm_valuenet_fit_validate, tm_distnet_fit_validate,
train_data(validation_backend="hip")): accuracy against train.validation_loss on the CPU (measure B), the same bits as the
gradient step's loss, independence of the slab, prefixes, determinism, stores only where the ABI says, the pass inside replayed
fits of both heads, and the refusals.  tests/fit_validation_cases.py has the cases, the references and the rule."""
import copy
import math

import numpy as np
import pytest
import torch

import dist_fit_cases as DC
import fit_hip_cases as FC
import fit_validation_cases as VC

pytestmark = pytest.mark.gpu
CHUNK, SLAB = VC.CHUNK, VC.SLAB
assert (VC.ROWS, CHUNK, SLAB) == ((33, 97, 161), 32, 64)


# ------------------------------------------------------------------------------------------------------------------ 1. accuracy
@pytest.mark.parametrize("head,name", VC.ALL)
def test_chunks_and_combined_loss_within_measure_b(head, name):
    torch.set_num_threads(16)
    case = VC.regime(head, name)
    bad, worst = [], 0.0
    for n in VC.ROWS + (1,):
        rows = VC.hip_validate(case, n)
        b, w = VC.compare(head, name, n, rows)
        bad += [(n,) + tuple(x) for x in b]
        worst = max(worst, w)
    print("%-6s %-34s the largest multiple of torch's own fp32 error needed: M = %.2f" % (head, name, worst))
    assert not bad, (head, name, bad)


# ------------------------------------------------------------------------------- 2. the same bits as the gradient step's loss
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("batch", [1, 33, 257])
@pytest.mark.parametrize("head", ["value", "dist"])
def test_one_chunk_is_the_gradient_steps_loss_bit_for_bit(head, batch, weighted):
    """n == chunk == slab == batch: (float) of row 0's mean and std are loss[0], loss[1] of the gradient step with idx NULL"""
    if head == "value":
        data = FC.dataset(batch, 31)
        grad_case = dict(net=FC.fresh_net(0), data=data, idx=None, batch=batch, weighted=weighted)
        case = dict(head="value", net=grad_case["net"], data=data, weighted=weighted)
        _, loss = FC.hip_grad(grad_case)
    else:
        atoms, W = DC.nets()["fixture"]
        data = DC.dataset(batch, atoms, 31, normalised=False)
        grad_case = dict(W=W, atoms=atoms, data=data, idx=None, batch=batch, weighted=weighted, tstride=64)
        case = dict(head="dist", W=W, atoms=atoms, data=data, weighted=weighted, tstride=64)
        _, loss = DC.hip_grad(grad_case)
    rows = VC.hip_validate(case, batch, chunk=batch, slab=batch)
    assert rows.shape == (1, 3)
    got = rows[0, 1:].astype(np.float32)
    print(head, batch, weighted, "validate", rows[0].tolist(), "gradient step", loss.tolist())
    assert got.tobytes() == loss.tobytes(), (got, loss)
    w64 = float(np.asarray(data[-1], np.float64).sum()) if weighted else float(batch)
    assert abs(rows[0, 0] - w64) <= 1e-12 * w64


# -------------------------------------------------------------------------------------------- 3., 4., 5. slabs, prefixes, repeats
@pytest.mark.parametrize("head,name", [("value", "r06 checkpoint, scale 40"), ("value", "fresh net, unweighted"), ("dist", "fitted"),
                                       ("dist", "seed7, targets off 1, stride 64")])
def test_slab_independence_prefixes_and_determinism(head, name):
    case = VC.regime(head, name)
    for n in VC.ROWS:
        base = VC.hip_validate(case, n)                                   # slab 64
        for slab in (32, 256):                                            # one chunk a slab; a slab of at least n rows
            assert VC.hip_validate(case, n, slab=slab).tobytes() == base.tobytes(), (n, slab)
        assert VC.hip_validate(case, n).tobytes() == base.tobytes(), n    # again, on a workspace of NaN again
        for k in range(1, n // CHUNK + 1):                                # the first k whole chunks are a call on k * chunk rows
            assert VC.hip_validate(case, k * CHUNK)[:k].tobytes() == base[:k].tobytes(), (n, k)
    # the other weighting of the same rows is another result (the flag is read)
    other = VC.hip_validate(case, 97, weighted=not case["weighted"])
    assert other.tobytes() != VC.hip_validate(case, 97).tobytes()


# --------------------------------------------------------------------------------------------------- 6. writes only where it says
@pytest.mark.parametrize("head,name,n", [("value", "fresh net, weighted", 161), ("value", "fresh net, weighted", 1),
                                         ("dist", "fixture", 161), ("dist", "seed7, targets off 1, stride 64", 97)])
def test_the_call_writes_only_where_it_says(head, name, n):
    """the workspace (exactly the ABI's floats) and rows_out (3 doubles a chunk) carved out of one device tensor with 64 KiB guard
    bands: the guards and every input are unchanged, the outputs are those of a plain call"""
    case = VC.regime(head, name)
    arena = FC.Arena()
    rows = VC.hip_validate(case, n, place=arena)
    arena.check()
    o, k = arena.segments[2]                                              # the two spare floats behind rows_out: not the call's
    assert (arena.arena[o:o + k] == FC.Arena.PATTERN).all()
    assert rows.tobytes() == VC.hip_validate(case, n).tobytes()
    assert set(arena.inputs) == ({"params", "bounds", "states", "value", "variance", "weight"} if head == "value"
                                 else {"params", "states", "targets", "weight"})


# ----------------------------------------------------------------------------------------------------------------- 7. inside a fit
def _value_set(n=600):
    rng = np.random.default_rng(0)
    states = rng.integers(-1, 2, size=(n, 1, 20, 10)).astype(np.float32)
    values = (states.sum(axis=(1, 2, 3)) * 0.5 + 20).astype(np.float32)[:, None]
    variances = rng.uniform(0.05, 6.0, (n, 1)).astype(np.float32)                 # a few below the clip
    weights = rng.integers(1, 20, size=(n, 1)).astype(np.float32)
    return [states, values, variances, weights]


def _dist_set(n=600, atoms=50):
    rng = np.random.default_rng(0)
    x = np.zeros((n, 1, 22, 10), np.float32)
    x[:, :, 2:, :] = rng.integers(-1, 2, size=(n, 1, 20, 10))
    centre = np.clip(x.sum(axis=(1, 2, 3)) * 0.5 + atoms / 2, 3, atoms - 3).reshape(-1, 1)
    t = np.exp(-0.5 * ((np.arange(atoms).reshape(1, -1) - centre) / 2.0) ** 2)
    t[:, :2] = 0.0
    t = (t / t.sum(1, keepdims=True) * rng.uniform(0.9, 1.1, (n, 1))).astype(np.float32)
    return [x, t, rng.integers(1, 20, size=(n, 1)).astype(np.float32)]


def _new_model(head, tmp_path, monkeypatch):
    from tetris_mcts_amd import model as M
    from tetris_mcts_amd.model_distributional import Model_Dist
    monkeypatch.setattr(M, "EXP_PATH", str(tmp_path) + "/")
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(5)
    return Model_Dist(atoms=50, seed=0, backend="torch") if head == "dist" else M.Model_VV(backend="torch", seed=0)


def _flat(mdl):
    return torch.cat([p.detach().reshape(-1) for p in mdl.model.parameters()]).cpu().numpy().tobytes()


@pytest.mark.parametrize("head", ["value", "dist"])
def test_the_validation_pass_inside_a_replayed_fit(head, tmp_path, monkeypatch):
    """600 rows, batch 64, iters_per_val=4, max_iters=12: three validations of 60 held-out rows, the second and third between
    graph replays.  At each, the net goes to the CPU and train.validation_loss is computed there in fp32 and fp64: the HIP
    numbers are held to measure B at the weights the fit has reached.  Without early stopping the final parameters are the bits
    of the same fit validated by torch; with it, the best weights are reloaded and best_validation is finite."""
    from tetris_mcts_amd import train as T
    monkeypatch.setenv("TM_TRAIN_GRAPH", "1")
    torch.set_num_threads(16)
    data = _dist_set() if head == "dist" else _value_set()
    fit_backend, Fit, loss_fn = ("hip_dist", T.HipDistFit, T.dist_batch_loss) if head == "dist" else ("hip", T.HipFit, T.batch_loss)
    kw = dict(iters_per_val=4, batch_size=64, max_iters=12, log=False, fit_backend=fit_backend)
    seen, real = [], Fit.validate

    def checked(self, weighted):
        rows = real(self, weighted)
        got = T.combine_chunk_rows(rows)
        net = copy.deepcopy(mdl.model).cpu()
        s = self.val_states.cpu().float()
        if head == "dist":
            x = torch.zeros(s.shape[0], 1, 22, 10)
            x[:, 0, 2:, :] = s.reshape(-1, 20, 10)
            val = [x, self.val_target.cpu(), self.val_weight.cpu().reshape(-1, 1)]
        else:
            val = [s.reshape(-1, 1, 20, 10)] + [t.cpu().reshape(-1, 1) for t in (self.val_value, self.val_variance, self.val_weight)]
        r32 = T.validation_loss(net, val, weighted, loss_fn=loss_fn)
        r64 = T.validation_loss(net.double(), [v.double() for v in val], weighted, loss_fn=loss_fn)
        seen.append((len(rows), got, r32, r64, _flat(mdl)))
        return rows
    monkeypatch.setattr(Fit, "validate", checked)
    mdl = _new_model(head, tmp_path, monkeypatch)
    start = _flat(mdl)
    res = mdl.train_data(list(data), early_stopping=False, validation_backend="hip", **kw)
    assert res["iters"] == 12 and res["graph_replay"] is True and len(seen) == 3
    hip_bits = _flat(mdl)
    bad = []
    for i, (chunks, got, r32, r64, _) in enumerate(seen):
        assert chunks == 1 and all(math.isfinite(v) for v in got + r32 + r64)
        for k, what in enumerate(("mean", "std")):
            err, bound, need = FC.measure([got[k]], [r32[k]], [r64[k]])
            print("%-5s validation %d  %-4s hip %.9g  f64 %.9g  err %.3e  bound %.3e  needs M = %.2f" % (head, i, what, got[k], r64[k], err, bound, need))
            if not err <= bound:
                bad.append((i, what, err, bound, need))
    assert not bad, bad
    assert len({s[4] for s in seen}) == 3 and seen[0][4] != start          # the weights moved between the validations
    # the same fit validated by torch: the same parameters, bit for bit
    monkeypatch.setattr(Fit, "validate", real)
    mdl = _new_model(head, tmp_path, monkeypatch)
    assert _flat(mdl) == start
    res_t = mdl.train_data(list(data), early_stopping=False, validation_backend="torch", **kw)
    assert res_t["iters"] == 12 and res_t["graph_replay"] is True
    assert _flat(mdl) == hip_bits and hip_bits != start
    # early stopping on: the best weights are reloaded
    mdl = _new_model(head, tmp_path, monkeypatch)
    res_e = mdl.train_data(list(data), early_stopping=True, validation_backend="hip", **kw)
    assert res_e["iters"] == 12 and math.isfinite(res_e["best_validation"])
    assert min(s[1][0] for s in seen) == res_e["best_validation"]         # the same three validations: the best of them
    assert all(torch.isfinite(p).all() for p in mdl.model.parameters())


def test_validation_fraction_zero_accepts_the_option_and_does_nothing(tmp_path, monkeypatch):
    from tetris_mcts_amd import train as T
    called = []
    monkeypatch.setattr(T.HipFit, "validate", lambda self, weighted: called.append(1))
    mdl = _new_model("value", tmp_path, monkeypatch)
    res = mdl.train_data(_value_set(200), iters_per_val=2, batch_size=32, max_iters=4, log=False, fit_backend="hip",
                         validation_backend="hip", validation_fraction=0.0)
    assert res["iters"] == 4 and not called and res["best_validation"] == float("inf")


def test_refusals_inside_train_data_that_need_a_device(tmp_path, monkeypatch):
    """held-out rows the kernels cannot read are refused before the optimiser is flattened"""
    from tetris_mcts_amd import train as T
    mdl = _new_model("value", tmp_path, monkeypatch)
    data = [torch.from_numpy(a).cuda() for a in _value_set(200)]
    half = [data[0].clone()] + data[1:]
    half[0][-3, 0, 4, 4] = 0.5                                           # a validation row that is no int8
    opt = mdl._optimizer()
    before = _flat(mdl)
    with pytest.raises(ValueError, match="int8"):
        T.train_data(mdl.model, opt, half, iters_per_val=2, batch_size=32, max_iters=4, log=False, fit_backend="hip", validation_backend="hip")
    assert getattr(opt, "_flat", None) is None and _flat(mdl) == before
    half[0][-3, 0, 4, 4] = 1.0
    res = T.train_data(mdl.model, opt, half, iters_per_val=2, batch_size=32, max_iters=4, log=False, fit_backend="hip", validation_backend="hip")
    assert res["iters"] == 4 and math.isfinite(res["best_validation"])


# ------------------------------------------------------------------------------------------------------------------ 8. refusals
@pytest.mark.parametrize("head,name", [("value", "fresh net, weighted"), ("dist", "fixture")])
def test_refused_arguments_launch_nothing(head, name):
    case = VC.regime(head, name)
    n = 97
    inp = VC.device_inputs(case, n)
    ws = torch.zeros(VC.workspace_floats(case, SLAB) + 4, device="cuda")
    rows = torch.full((4, 3), 7.0, dtype=torch.float64, device="cuda")
    ws_before = ws.clone()
    for k in inp:                                                         # each pointer NULL in turn
        assert VC.call(case, dict(inp, **{k: None}), n, CHUNK, SLAB, rows, ws) == 1, k          # hipErrorInvalidValue
    assert VC.call(case, inp, n, CHUNK, SLAB, None, ws) == 1 and VC.call(case, inp, n, CHUNK, SLAB, rows, None) == 1
    for bad_n, chunk, slab in ((0, CHUNK, SLAB), (-5, CHUNK, SLAB), (n, 0, SLAB), (n, -1, SLAB), (n, CHUNK, CHUNK - 1), (n, CHUNK, 0),
                               (n, CHUNK, SLAB + 1), (n, 3, 64), (n, CHUNK, (1 << 20) + CHUNK)):
        assert VC.call(case, inp, bad_n, chunk, slab, rows, ws) == 1, (bad_n, chunk, slab)
    assert VC.call(case, inp, n, CHUNK, SLAB, rows, ws[1:]) == 1          # a workspace off its 16 bytes
    if head == "dist":
        for atoms, stride in ((0, 50), (65, 70), (50, 49)):
            assert VC.call(dict(case, atoms=atoms, tstride=stride), inp, n, CHUNK, SLAB, rows, ws) == 1, (atoms, stride)
    torch.cuda.synchronize()
    assert (rows == 7.0).all() and torch.equal(ws, ws_before)            # nothing ran
    assert VC.call(case, inp, n, CHUNK, SLAB, rows, ws) == 0              # ... and the same arguments complete are accepted
    torch.cuda.synchronize()
    assert rows.cpu().numpy().tobytes() == VC.hip_validate(case, n).tobytes()
