"""The training-mode forward / backward formulas, pinned without a GPU.

tests/golden/train/*.npz hold three epochs of the reference's own weight-training loop (tools/make_train_golden.py:
gnn/marglik_training.py:159-186 on the reference's GCN / GraphSAGE / STEGCN in train() mode, with the dropout masks it drew).
``forward_backward`` below is an fp64 sparse restatement of BaseGNN.forward (gnn/models/base_gnn.py:136-161,
gnn/models/layers.py:18-46) and of its backward written as FORMULAS (no autograd) -- the ones csrc/train.hip implements:
propagated GCN bias, repeated node ids added in the gather's backward, LayerNorm backward, mask * 1 / (1 - p).  It must
reproduce the reference's gradients to 1e-6 (the reference computes in fp32: its own rounding is ~1e-7).  tests/test_gpu_train.py
imports it as the CPU side of the device tests.  Also here: the host-side behaviour that needs no device."""
import glob
import os

import numpy as np
import pytest
import scipy.sparse as sp

import gnn_laplace_oracle as O
from conftest import GOLDEN

TRAIN = os.path.join(GOLDEN, "train")
CASES = sorted(glob.glob(os.path.join(TRAIN, "*.npz")))
IDS = [os.path.basename(p)[:-4] for p in CASES]
TOL = 1e-6


def rel(a, b):
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-30))


def propagation64(edge_index, n, kind, symmetric):
    """fp64 CSR of the matrix the convs multiply with (gnn/models/utils.py:106-112 resp. gnn/models/layers.py:18-24)."""
    rp, col = O.edge_index_to_adj_csr(edge_index, n, kind, symmetric)
    A = sp.csr_matrix((np.ones(len(col)), col, rp), shape=(n, n))
    deg = np.diff(rp).astype(np.float64)
    if kind == "gcn":
        d = np.where(deg > 0, deg ** -0.5, 0.0)
        return (sp.diags(d) @ A.T @ sp.diags(d)).tocsr()
    return (sp.diags(1.0 / np.where(deg > 0, deg, 1.0)) @ A).tocsr()


def forward_backward(kind, P, X, params, idx, y, masks, p, act="relu", eps=1e-5):
    """(logits [M, C], mean cross entropy, {name: gradient}) in fp64.  ``params``: name -> array under the module's names
    (convs.{l}.lin.weight|bias, res.{l}.weight|bias, norms.{l}.weight|bias); ``masks``: keep-masks per hidden layer or None."""
    prm = {k: np.asarray(v, np.float64) for k, v in params.items()}
    L = sum(1 for k in prm if k.startswith("convs.") and k.endswith("lin.weight"))
    res, ln = "res.0.weight" in prm, "norms.0.weight" in prm
    scale = 1.0 / (1.0 - p)
    x = np.asarray(X, np.float64)
    tape = []
    for l in range(L):
        W, b = prm[f"convs.{l}.lin.weight"], prm[f"convs.{l}.lin.bias"]
        lin_in = x if kind == "gcn" else np.concatenate([x, P @ x], axis=1)
        s = P @ (lin_in @ W.T + b) if kind == "gcn" else lin_in @ W.T + b
        if l == L - 1:
            tape.append((x, lin_in))
            out = s
            break
        if res:
            s = s + x @ prm[f"res.{l}.weight"].T + prm[f"res.{l}.bias"]
        xhat = rstd = None
        if ln:
            mu = s.mean(1, keepdims=True)
            rstd = 1.0 / np.sqrt(((s - mu) ** 2).mean(1, keepdims=True) + eps)
            xhat = (s - mu) * rstd
            s = xhat * prm[f"norms.{l}.weight"] + prm[f"norms.{l}.bias"]
        a = np.maximum(s, 0.0) if act == "relu" else np.tanh(s)
        keep = np.ones_like(a) if masks is None or masks[l] is None else (np.asarray(masks[l]) != 0).astype(np.float64)
        tape.append((x, lin_in, xhat, rstd, a, keep))
        x = a * keep * (scale if masks is not None and masks[l] is not None else 1.0)
    idx, y = np.asarray(idx), np.asarray(y)
    M = len(idx)
    f = out[idx]
    z = f - f.max(1, keepdims=True)
    logp = z - np.log(np.exp(z).sum(1, keepdims=True))
    loss = float(-logp[np.arange(M), y].mean())
    df = np.exp(logp)
    df[np.arange(M), y] -= 1.0
    d = np.zeros_like(out)
    np.add.at(d, idx, df / M)  # a repeated node id receives the sum of its rows
    grads = {}
    for l in range(L - 1, -1, -1):
        W = prm[f"convs.{l}.lin.weight"]
        x, lin_in = tape[l][0], tape[l][1]
        hid_res = res and l < L - 1
        if kind == "gcn":
            T = P.T @ d
            grads[f"convs.{l}.lin.weight"] = T.T @ x
            grads[f"convs.{l}.lin.bias"] = T.sum(0)  # = sum_n rowsum(P)[n] d[n]: the bias is propagated
            dx = T @ W
        else:
            grads[f"convs.{l}.lin.weight"] = d.T @ lin_in
            grads[f"convs.{l}.lin.bias"] = d.sum(0)
            dcat = d @ W
            F_ = x.shape[1]
            dx = dcat[:, :F_] + P.T @ dcat[:, F_:]
        if hid_res:
            grads[f"res.{l}.weight"] = d.T @ x
            grads[f"res.{l}.bias"] = d.sum(0)
            dx = dx + d @ prm[f"res.{l}.weight"]
        if l == 0:
            break
        _, _, xhat, rstd, a, keep = tape[l - 1]
        dact = (a > 0).astype(np.float64) if act == "relu" else 1.0 - a * a
        has_mask = masks is not None and masks[l - 1] is not None
        d = dx * keep * (scale if has_mask else 1.0) * dact
        if ln:
            grads[f"norms.{l - 1}.weight"] = (d * xhat).sum(0)
            grads[f"norms.{l - 1}.bias"] = d.sum(0)
            dxh = d * prm[f"norms.{l - 1}.weight"]
            d = rstd * (dxh - dxh.mean(1, keepdims=True) - xhat * (dxh * xhat).mean(1, keepdims=True))
    return f, loss, grads


def batches(g):
    bs, n = int(g["batch_size"]), len(g["train_idx"])
    return [(g["train_idx"][i:i + bs], g["train_y"][i:i + bs]) for i in range(0, n, bs)]


def step_inputs(g, s):
    """What step s of the stored loop saw: the parameters before the step, the batch, the masks."""
    names = [str(k) for k in g["names"]]
    params = {k: g["P/" + k][s] for k in names}
    idx, y = batches(g)[int(g["batch_of_step"][s])]
    masks = [g[f"masks_{l}"][s] for l in range(int(g["num_layers"]) - 1)]
    return names, params, idx, y, masks


def test_fixtures_cover_the_cases():
    assert len(CASES) >= 12
    seen = set()
    for path in CASES:
        g = np.load(path)
        seen.add((str(g["kind"]), bool(g["res"]), str(g["norm"]), float(g["p"]) > 0))
        assert os.path.getsize(path) < 200 * 1024
        assert len(set(g["train_idx"].tolist())) < len(g["train_idx"])  # a repeated node id
        for k in g["names"]:
            assert "adj" not in str(k)
            assert all(np.linalg.norm(x) > 0 for x in g["G/" + str(k)])
        if float(g["p"]) > 0:
            kept = np.mean([g[f"masks_{l}"].mean() for l in range(int(g["num_layers"]) - 1)])
            assert 0.3 < kept < 0.9  # (entries whose input was zero are stored as kept)
    for kind in ("gcn", "sage"):
        for res, norm in ((False, ""), (True, "layer")):
            for drop in (False, True):
                assert (kind, res, norm, drop) in seen
    assert {int(np.load(p)["num_layers"]) for p in CASES} >= {2, 3}
    assert {str(np.load(p)["act"]) for p in CASES} >= {"relu", "tanh"}
    assert {bool(np.load(p)["symmetric"]) for p in CASES} == {True, False}


@pytest.mark.parametrize("path", CASES, ids=IDS)
def test_fp64_formulas_reproduce_the_reference(path):
    g = np.load(path)
    kind = str(g["kind"])
    P = propagation64(g["edge_index"], int(g["num_nodes"]), kind, bool(g["symmetric"]))
    for s in range(len(g["loss"])):
        names, params, idx, y, masks = step_inputs(g, s)
        f, loss, grads = forward_backward(kind, P, g["X"], params, idx, y, masks, float(g["p"]), str(g["act"]))
        assert rel(f, g[f"logits_{s}"]) < TOL, ("logits", s)
        assert abs(loss - float(g["loss"][s])) < TOL * abs(float(g["loss"][s])), ("loss", s)
        assert sorted(grads) == sorted(names)
        for k in names:
            assert rel(grads[k], g["G/" + k][s]) < TOL, (k, s, rel(grads[k], g["G/" + k][s]))


def test_propagated_bias_is_not_a_column_sum():
    """GCN: db = sum_n rowsum(P)[n] d[n, :]; the plain column sum of d (what a Linear outside the propagation would get) is
    off by tens of percent on the fixture graph -- the golden tells the two apart."""
    g = np.load(os.path.join(TRAIN, "gcn_plain_p05.npz"))
    P = propagation64(g["edge_index"], int(g["num_nodes"]), "gcn", bool(g["symmetric"]))
    assert np.abs(np.asarray(P.sum(1)).ravel() - 1.0).max() > 0.1
    names, params, idx, y, masks = step_inputs(g, 0)
    _, _, grads = forward_backward("gcn", P, g["X"], params, idx, y, masks, float(g["p"]))
    assert rel(grads["convs.1.lin.bias"], g["G/convs.1.lin.bias"][0]) < TOL
    M = len(idx)
    f = g["logits_0"].astype(np.float64)
    sm = np.exp(f - f.max(1, keepdims=True))
    sm /= sm.sum(1, keepdims=True)
    sm[np.arange(M), y] -= 1.0
    assert rel(sm.sum(0) / M, g["G/convs.1.lin.bias"][0]) > 1e-2


# ---- host-side behaviour (no device) ------------------------------------------------------------------------------------
def _small_model(**kw):
    import torch

    import laplace_gnn_amd as lg

    gen = torch.Generator().manual_seed(0)
    X = torch.randn(20, 5, generator=gen)
    ei = torch.randint(0, 20, (2, 60), generator=gen)
    return lg.GCN(5, 8, 3, kw.pop("layers", 2), X, ei, **kw)


def test_mask_injection_checks_shapes():
    import torch

    m = _small_model(layers=3)
    with pytest.raises(ValueError, match="one dropout mask per hidden layer"):
        m.set_dropout_masks([torch.ones(20, 8)])
    with pytest.raises(ValueError, match="shape"):
        m.set_dropout_masks([torch.ones(20, 8), torch.ones(20, 7)])
    with pytest.raises(ValueError, match="shape"):
        m.set_dropout_masks([torch.ones(20, 8), np.ones((20, 8))])
    m.set_dropout_masks([torch.ones(20, 8), (torch.rand(20, 8) > 0.5).float()])
    assert [t.dtype for t in m._next_masks] == [torch.uint8, torch.uint8]
    assert set(m._next_masks[1].unique().tolist()) <= {0, 1}
    m.set_dropout_masks(None)
    assert m._next_masks is None


def test_training_forward_needs_a_gpu_and_batchnorm_is_refused():
    import torch

    m = _small_model(norm="batch").train()
    with pytest.raises(NotImplementedError, match="batch"):
        m(torch.arange(4))
    m = _small_model().train()  # the constructor default dropout_p = 0.5
    with pytest.raises(RuntimeError, match="GPU"):  # no CPU fallback: the engine refuses a model that is not on a device
        m(torch.arange(4))
    with torch.no_grad(), pytest.raises(NotImplementedError):
        m(torch.arange(4))


def test_train_parameter_order_is_named_parameters_order():
    m = _small_model(layers=3, res=True, norm="layer")
    named = [p for k, p in m.named_parameters() if "adj" not in k]
    assert len(named) == len(m._train_params()) and all(a is b for a, b in zip(named, m._train_params()))
