"""Pins the activation-generic fp64 helper (tests/act_reference.py), entirely on the CPU.

At ``act="relu"`` it must reproduce the oracle (itself golden-checked against the reference's code) and two goldens to
<= 1e-5 relative -- that fixes every scaling convention (n_train, sqrt(0.5) of regression, the loss).  The anchor inputs keep
every hidden pre-activation away from zero, so fp32 and fp64 agree on every ReLU sign.  At ``act="tanh"``: a central finite
difference proves the helper differentiates tanh, and the inputs of tests/test_gpu_tanh.py are shown to sit where tanh is
neither linear nor saturated -- otherwise a 1e-4 bar could not tell tanh from ReLU or from the identity."""
import os

import numpy as np
import pytest
import torch

import gnn_laplace_oracle as O
from act_reference import ActReference
from conftest import GOLDEN
from golden_utils import model_extras
from gpu_utils import oracle_from_arrays, rel
from test_gpu_resnorm import _extras
from test_gpu_scale import _make
from test_gpu_tanh import (DIAG_CASES, DIAG_SHAPE, FRONT_SHAPE, HUB_CASES, JAC_CASES, JAC_SHAPE, KFAC_CASES, PLANE_CASES,
                           RESNORM_CASES, hub_inputs, resnorm_extras, tanh_inputs)

TOL = 1e-5
N, F, H, C, E, M = 60, 7, 10, 4, 200, 24

ANCHORS = [("gcn", 2, None, False), ("sage", 2, None, False), ("gcn", 3, None, False), ("sage", 3, None, False),
           ("gcn", 2, "layer", True), ("sage", 3, "batch", True), ("sage", 2, "layer", True)]


def _anchor(kind, L, norm, res, act="relu", likelihood="classification", seed=0):
    ei, X, Ws, bs = _make(kind, N, F, H, C, E, L=L, seed=seed)
    kw = _extras(H, L, norm, res, [F] + [H] * (L - 2), seed + 50) if (norm or res) else {}
    host = {k: ([t.numpy() for t in v] if isinstance(v, list) else v) for k, v in kw.items()}
    om = oracle_from_arrays(kind, N, ei.numpy(), X.numpy(), [w.numpy() for w in Ws], [b.numpy() for b in bs], True, **host)
    ref = ActReference(kind, om.P, X, Ws, bs, act=act, likelihood=likelihood, **kw)
    g = torch.Generator().manual_seed(seed + 1)
    idx = torch.randperm(N, generator=g)[:M]
    idx[5] = idx[2]  # a node listed twice
    y = torch.randint(0, C, (M,), generator=g)
    return om, ref, idx.numpy(), y.numpy()


def _assert_kfacs(got, want, what):
    assert len(got) == len(want)
    for i, (Fg, Fw) in enumerate(zip(got, want)):
        for j, (a, b) in enumerate(zip(Fg, Fw)):
            assert rel(a.numpy(), b) <= TOL, (what, i, j, rel(a.numpy(), b))


@pytest.mark.parametrize("kind,L,norm,res", ANCHORS)
def test_relu_helper_reproduces_the_oracle(kind, L, norm, res):
    om, ref, idx, y = _anchor(kind, L, norm, res)
    fw = ref.forward()
    assert min(float(p.detach().abs().min()) for p in fw["pre"]) > 1e-6  # no ReLU sign can differ between fp32 and fp64
    assert rel(fw["out"].detach().numpy(), O.forward_all(om)[0]) <= TOL
    for fork in (True, False):
        ol, oH = O.fit_kron(om, idx, y, 10, fork_exact=fork)  # 10 / 10 / 4
        loss, kf = ref.kfac_fit(idx, y, 10, fork_exact=fork)
        _assert_kfacs(kf, oH, ("fit_kron", fork))
        assert abs(loss - float(ol)) <= TOL * abs(float(ol))
    ol, ok = O.kfac_batch(om, idx, y, 77, True, (1, 3))  # a class-range share, another n_train
    loss, kf = ref.kfac_batch(idx, y, 77, True, (1, 3))
    for i in range(0, len(kf), 2):
        assert rel(kf[i][0].numpy(), ok[i][0]) <= TOL and float(kf[i][1].abs().max()) == 0.0 and loss == 0.0
    _, shares = ref.kfac_fit(idx, y, 10, shares=[(0, 1), (1, C)])
    _assert_kfacs(shares, O.fit_kron(om, idx, y, 10)[1], "shares")
    J = ref.jacobians(idx)
    oJ, of = O.jacobians_batch(om, idx)
    assert rel(J[0].numpy(), oJ) <= TOL and rel(J[1].numpy(), of) <= TOL
    ol, od = O.fit_diag(om, idx, y, M)
    loss, Hd = ref.ggn(idx, y, J=J)
    assert rel(Hd.numpy(), od) <= TOL and abs(loss - float(ol)) <= TOL * abs(float(ol))
    assert rel(ref.ggn(idx, y, True, J)[1].numpy(), O.full_batch(om, idx, y)[1]) <= TOL
    for full in (False, True):
        ol, oe = O.ef_batch(om, idx, y, full=full)
        loss, He, _ = ref.ef(idx, y, full, J)
        assert rel(He.numpy(), oe) <= TOL and abs(loss - float(ol)) <= TOL * abs(float(ol))
    if norm is None and not res:  # what the oracle has for plain models only
        assert rel(ref.lastlayer_full(idx, y, J)[1].numpy(), O.lastlayer_full_batch(om, idx, y)[1]) <= TOL
        g = torch.Generator().manual_seed(4)
        draws = [torch.randint(0, C, (M,), generator=g).numpy() for _ in range(3)]
        for labels in (None, draws):
            ol, oH = O.kfac_fisher_batch(om, idx, y, M, mc_labels=labels)
            loss, kf = ref.kfac_fisher_batch(idx, y, M, mc_labels=labels)
            _assert_kfacs(kf, oH, ("fisher", labels is None))
            assert abs(loss - float(ol)) <= TOL * abs(float(ol))


@pytest.mark.parametrize("kind,L", [("gcn", 2), ("sage", 2), ("sage", 3)])
def test_relu_helper_reproduces_the_oracle_regression(kind, L):
    om, ref, idx, _ = _anchor(kind, L, None, False, likelihood="regression")
    y = torch.randn(M, C, generator=torch.Generator().manual_seed(8)).numpy()
    ol, oH = O.fit_kron(om, idx, y, 10, likelihood="regression")
    loss, kf = ref.kfac_fit(idx, y, 10)
    _assert_kfacs(kf, oH, "regression fit_kron")
    assert abs(loss - float(ol)) <= TOL * abs(float(ol))
    J = ref.jacobians(idx)
    ol, od = O.diag_batch(om, idx, y, "regression")
    loss, Hd = ref.ggn(idx, y, J=J)
    assert rel(Hd.numpy(), od) <= TOL and abs(loss - float(ol)) <= TOL * abs(float(ol))
    assert rel(ref.ggn(idx, y, True, J)[1].numpy(), O.full_batch(om, idx, y, "regression")[1]) <= TOL
    ol, oe = O.ef_batch(om, idx, y, "regression", full=True)
    loss, He, _ = ref.ef(idx, y, True, J)
    assert rel(He.numpy(), oe) <= TOL and abs(loss - float(ol)) <= TOL * abs(float(ol))
    ol, oH = O.kfac_fisher_batch(om, idx, y, M, "regression")
    loss, kf = ref.kfac_fisher_batch(idx, y, M)
    _assert_kfacs(kf, oH, "regression fisher")
    assert abs(loss - float(ol)) <= TOL * abs(float(ol))


@pytest.mark.parametrize("name", ["gcn_resln_small_3batch_s1", "sage_small_3batch_s1"])
def test_relu_helper_reproduces_the_reference_goldens(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    L, n = int(g["num_layers"]), int(g["num_nodes"])
    ref = ActReference(str(g["kind"]), (g["prop_row"], g["prop_col"], g["prop_val"]), g["X"], [g[f"W{l}"] for l in range(L)],
                       [g[f"b{l}"] for l in range(L)], **model_extras(g))
    assert min(float(p.detach().abs().min()) for p in ref.forward()["pre"]) > 1e-6
    assert rel(ref.forward()["out"].detach().numpy(), g["logits"]) <= TOL
    loss, kf = ref.kfac_fit(g["train_idx"], g["train_y"], int(g["batch_size"]))
    assert len(kf) == int(g["kron_n_blocks"])
    for i, Fs in enumerate(kf):
        for j, Hm in enumerate(Fs):
            assert rel(Hm.numpy(), g[f"kron_{i}_{j}"]) <= TOL, (i, j)
    assert abs(loss - float(g["kron_loss"])) <= TOL * abs(float(g["kron_loss"]))
    loss, Hd = ref.ggn(g["train_idx"], g["train_y"])
    assert rel(Hd.numpy(), g["diag_H"]) <= TOL and abs(loss - float(g["diag_loss"])) <= TOL * abs(float(g["diag_loss"]))


@pytest.mark.parametrize("kind,L,norm,res", ANCHORS)
def test_tanh_jacobian_entries_against_a_central_finite_difference(kind, L, norm, res):
    """(a): ~20 random entries of the helper's tanh Jacobian against (f(theta + e) - f(theta - e)) / 2e in fp64."""
    om, ref, idx, y = _anchor(kind, L, norm, res, act="tanh")
    J, _ = ref.jacobians(idx[:6])
    r = np.random.default_rng(3)
    big = (J.abs() > 1e-3 * J.abs().max()).nonzero()
    picks = big[r.choice(len(big), 20, replace=False)]
    flat = torch.cat([p.detach().reshape(-1) for p in ref.params])
    eps = 1e-5

    def out_at(theta):
        ps, o = [], 0
        for p in ref.params:
            ps.append(theta[o:o + p.numel()].reshape(p.shape)); o += p.numel()
        kw = dict(res_weights=ps[2 * L::2], res_biases=ps[2 * L + 1::2]) if res else {}
        m = ActReference(kind, ref.P, ref.X, ps[0:2 * L:2], ps[1:2 * L:2], act="tanh", norm=ref.norm, norm_weight=ref.nw,
                         norm_bias=ref.nb, norm_mean=ref.nm, norm_var=ref.nv, norm_eps=ref.eps, **kw)
        return m.forward()["out"].detach()[idx[:6]]

    for m, c, p in picks.tolist():
        d = torch.zeros_like(flat)
        d[p] = eps
        fd = float((out_at(flat + d)[m, c] - out_at(flat - d)[m, c]) / (2 * eps))
        assert abs(fd - float(J[m, c, p])) <= 1e-6 * max(abs(float(J[m, c, p])), float(J.abs().max()) * 1e-3), (m, c, p)


def _mid_fraction(ref):
    return [float(((h.abs() >= 0.1) & (h.abs() <= 0.9)).double().mean()) for h in ref.forward()["hid"]]


def _host_ref(kind, n, ei, X, Ws, bs, symmetric=True, **kw):
    rp, col = O.edge_index_to_adj_csr(ei.numpy(), n, kind, symmetric)
    return ActReference(kind, O.propagation_matrix(rp, col, kind), X, Ws, bs, act="tanh", **kw)


def _gpu_test_inputs():
    for kind, H_, C_, L in KFAC_CASES:
        yield ("kfac", kind, H_, C_, L), (kind, 1200) + tanh_inputs(kind, 1200, 40, H_, C_, 5000, L=L, seed=21), {}
    for kind, H_, L in HUB_CASES:
        yield ("hub", kind, H_, L), (kind, 5000) + hub_inputs(kind, H_, L)[:4], {}
    for kind in PLANE_CASES:
        yield ("plane", kind), (kind, 3000) + tanh_inputs(kind, 3000, 20, 256, 5, 9000, L=3, seed=77), {}
    for kind, L, norm in RESNORM_CASES:
        yield ("resnorm", kind, L, norm), (kind, 1200) + tanh_inputs(kind, 1200, 40, 64, 6, 5000, L=L, seed=31), \
            resnorm_extras(64, L, norm, 40)
    j = JAC_SHAPE
    for kind, L, resnorm in JAC_CASES:
        yield ("jac", kind, L, resnorm), (kind, j["N"]) + tanh_inputs(kind, j["N"], j["F"], j["H"], j["C"], j["E"], L=L, seed=23), \
            (resnorm_extras(j["H"], L, "layer", j["F"]) if resnorm else {})
    d = DIAG_SHAPE
    for kind, f, h, L, _ in DIAG_CASES:
        yield ("diag", kind, f, h, L), (kind, d["N"]) + tanh_inputs(kind, d["N"], f, h, d["C"], d["E"], L=L, seed=23), {}
    n, f, h, c, e = FRONT_SHAPE
    for kind in ("gcn", "sage"):
        yield ("front", kind), (kind, n) + tanh_inputs(kind, n, f, h, c, e, L=2, seed=61), {}
    yield ("front", "regression"), ("gcn", n) + tanh_inputs("gcn", n, f, 64, 3, e, L=2, seed=61), {}


@pytest.mark.parametrize("case", list(_gpu_test_inputs()), ids=lambda c: "-".join(map(str, c[0])))
def test_gpu_test_inputs_sit_in_the_curved_part_of_tanh(case):
    """(b): on the shapes tests/test_gpu_tanh.py uses, at least half of the hidden units of every layer have |h| in
    [0.1, 0.9]: not in the linear part (where tanh' ~ 1, indistinguishable from the identity) and not saturated."""
    _, (kind, n, ei, X, Ws, bs), kw = case
    fr = _mid_fraction(_host_ref(kind, n, ei, X, Ws, bs, **kw))
    print(case[0], ["%.2f" % v for v in fr])
    assert min(fr) >= 0.5, fr


@pytest.mark.parametrize("kind,L", [("gcn", 2), ("sage", 2), ("gcn", 3)])
def test_tanh_factors_differ_from_relu_factors(kind, L):
    """(c): B_0 under tanh and under ReLU of the same weights differ by more than 1e-2 relative, on a GPU-test shape."""
    ei, X, Ws, bs = tanh_inputs(kind, 1200, 40, 30, 4, 5000, L=L, seed=21)
    rp, col = O.edge_index_to_adj_csr(ei.numpy(), 1200, kind, True)
    P = O.propagation_matrix(rp, col, kind)
    idx, y = np.arange(0, 260, 2), np.zeros(130, np.int64)
    B = [ActReference(kind, P, X, Ws, bs, act=a).kfac_batch(idx, y, 130)[1][0][0] for a in ("tanh", "relu")]
    assert rel(B[0].numpy(), B[1].numpy()) > 1e-2
