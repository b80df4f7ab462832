"""``lgnn_sampled_forward`` (csrc/sampled.hip) through the C ABI, and the fronts that sit on it: the logits of S parameter
samples in one pass against the per-sample loop (laplace/baselaplace.py:1160-1199) and an fp64 dense restatement."""
import os

import numpy as np
import pytest
import torch
from torch.nn.utils import parameters_to_vector, vector_to_parameters

from conftest import GOLDEN
from gpu_utils import rel
from test_gpu_frontend import CASES, IDS, model_from_golden

pytestmark = pytest.mark.gpu


def _small_graph(N=70, seed=0):
    """Directed; node 0 has 66 neighbours in both directions (a row of P longer than a wave), node N - 1 is isolated."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(1, N - 1, (150,), generator=g)
    dst = torch.randint(1, N - 1, (150,), generator=g)
    keep = src != dst
    hub = torch.arange(1, 67)
    zero = torch.zeros_like(hub)
    return torch.stack([torch.cat([src[keep], hub, zero]), torch.cat([dst[keep], zero, hub])])


def _sym_graph(N=300, E=1200, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, N, (2, E), generator=g)


def _model(kind, N, F, H, C, L, ei, symmetric, act="relu", seed=0, **kw):
    import laplace_gnn_amd as lg

    g = torch.Generator().manual_seed(seed + 17)
    X = torch.randn(N, F, generator=g)
    torch.manual_seed(seed)
    cls = lg.GCN if kind == "gcn" else lg.GraphSAGE
    model = cls(F, H, C, L, X, ei, symmetric=symmetric, act=act, **kw).cuda().eval()
    with torch.no_grad():  # biases away from zero, weights large enough that activations switch between samples
        for p in model.parameters():
            p.copy_(torch.randn(p.shape, generator=g).to(p.device) * (0.3 if p.dim() > 1 else 0.5))
    return model


def _params(model):
    return [p for c in model.convs for p in (c.lin.weight, c.lin.bias)]


def _theta(model, S, seed=3, scale=0.2):
    mean = parameters_to_vector(_params(model)).detach()
    g = torch.Generator().manual_seed(seed)
    return mean.reshape(1, -1) + scale * torch.randn(S, mean.numel(), generator=g).cuda()


@torch.no_grad()
def _loop_route(model, idx, theta, params=None):
    params = _params(model) if params is None else params
    mean = parameters_to_vector(params).detach().clone()
    outs = []
    try:
        for t in theta:
            vector_to_parameters(t, params)
            outs.append(model(idx).clone())
    finally:
        vector_to_parameters(mean.clone(), params)
    return torch.stack(outs)


def _fp64_dense(model, idx, theta):
    """The model's definition in fp64 with a dense propagation matrix (gnn/models/layers.py:18-46)."""
    eng = model.engine
    N = model.num_nodes
    r, c, v = eng.export_propagation()
    Pm = torch.zeros(N, N, dtype=torch.float64, device=r.device)
    Pm[r, c] = v.double()
    X = model.X.double().to(r.device)
    act = torch.relu if model.act_name == "relu" else torch.tanh
    shapes = [tuple(p.shape) for p in _params(model)]
    outs = []
    for t in theta.double():
        ps, off = [], 0
        for sh in shapes:
            n = int(np.prod(sh))
            ps.append(t[off:off + n].reshape(sh))
            off += n
        h = X
        for l in range(len(ps) // 2):
            W, b = ps[2 * l], ps[2 * l + 1]
            if model.kind == "gcn":
                h = Pm @ (h @ W.T + b)
            else:
                h = torch.cat([h, Pm @ h], dim=1) @ W.T + b
            if l < len(ps) // 2 - 1:
                h = act(h)
        outs.append(h[idx])
    return torch.stack(outs)


def _err(f, f64):
    return float((f.double() - f64).abs().max() / max(1.0, float(f64.abs().max())))


SMALL = dict(N=70, F=13, H=20, C=3, L=2, graph="small")
BIG = dict(N=300, F=64, C=47, L=2, graph="sym")
PARITY = {
    "gcn_small_m1": dict(SMALL, kind="gcn", S=7, M=1),
    "gcn_small_m33": dict(SMALL, kind="gcn", S=7, M=33),
    "sage_small_m1": dict(SMALL, kind="sage", S=7, M=1),
    "sage_small_m33": dict(SMALL, kind="sage", S=7, M=33),
    "gcn_h132_all": dict(BIG, kind="gcn", H=132, S=5, M=None),
    "gcn_h260_all": dict(BIG, kind="gcn", H=260, S=5, M=None),
    "sage_h132_all": dict(BIG, kind="sage", H=132, S=5, M=None),
    "sage_h260_all": dict(BIG, kind="sage", H=260, S=5, M=None),
    "gcn_1layer": dict(SMALL, kind="gcn", F=9, C=4, L=1, S=7, M=33),
    "sage_1layer": dict(SMALL, kind="sage", F=9, C=4, L=1, S=7, M=33),
    "gcn_tanh": dict(SMALL, kind="gcn", S=7, M=33, act="tanh"),
    "sage_tanh": dict(SMALL, kind="sage", S=7, M=33, act="tanh"),
    "gcn_one_sample": dict(SMALL, kind="gcn", S=1, M=33),
    "sage_two_windows_of_z": dict(SMALL, kind="sage", C=70, S=2, M=33),  # 2 C = 140 columns of z: two windows of 128
    # the same ragged second window (12 of 128 columns) over two row tiles of the needed rows, the second one ragged too
    "sage_two_windows_two_row_tiles": dict(SMALL, kind="sage", N=96, H=10, C=70, S=2, M=33),
}


def _case(c):
    ei = _small_graph(c["N"]) if c["graph"] == "small" else _sym_graph(c["N"])
    model = _model(c["kind"], c["N"], c["F"], c["H"], c["C"], c["L"], ei, c["graph"] == "sym", act=c.get("act", "relu"))
    N, M = c["N"], c["M"]
    if M is None:
        idx = torch.arange(N)
    elif M == 1:
        idx = torch.tensor([0])  # the long row
    else:
        idx = torch.randperm(N, generator=torch.Generator().manual_seed(5))[:M]
        idx[0], idx[1], idx[2], idx[7] = 0, N - 1, 5, 5  # the long row, the isolated node, a repeated id
    return model, idx.cuda(), _theta(model, c["S"])


@pytest.mark.parametrize("name", list(PARITY))
def test_parity_with_the_loop_route_and_fp64(name):
    """err(route) = max |f_route - f_64| / max(1, max |f_64|); the loop is the yardstick (the same products in another order:
    factor two), 1e-6 the floor tests/test_gpu_lastlayer_kron.py documents for logits of this size."""
    c = PARITY[name]
    model, idx, theta = _case(c)
    eng = model.engine
    if c["graph"] == "small":
        rows = eng.export_propagation()[0]
        assert int(torch.bincount(rows, minlength=c["N"]).max()) >= 66
    got = eng.sampled_forward(idx, theta)
    assert got.shape == (c["S"], idx.shape[0], c["C"])
    loop = _loop_route(model, idx, theta)
    f64 = _fp64_dense(model, idx, theta)
    e_new, e_loop = _err(got, f64), _err(loop, f64)
    print(f"sampled_forward parity {name}: err(new) = {e_new:.3e}  err(loop) = {e_loop:.3e}")
    assert e_new <= 2 * e_loop + 1e-6, (e_new, e_loop)
    eng.check_async_errors()


@pytest.mark.parametrize("kind,L", [("gcn", 2), ("sage", 2), ("gcn", 1)])
def test_softmax_flag(kind, L):
    c = dict(SMALL, kind=kind, L=L, S=4, M=33)
    model, idx, theta = _case(c)
    logits = model.engine.sampled_forward(idx, theta)
    probs = model.engine.sampled_forward(idx, theta, softmax=True)
    assert (probs - torch.softmax(logits, dim=-1)).abs().max() < 1e-6


def test_bit_identical_twice_and_across_chunk_seams():
    c = dict(BIG, kind="gcn", H=132, S=40, M=None)
    model_a, idx, theta = _case(c)
    model_b, _, _ = _case(c)
    a1 = model_a.engine.sampled_forward(idx, theta)
    a2 = model_a.engine.sampled_forward(idx, theta)
    assert torch.equal(a1, a2)
    eng_b = model_b.engine
    eng_b.set_workspace_limit(1 << 20)
    b = eng_b.sampled_forward(idx, theta)
    assert torch.equal(a1, b)
    # more than one chunk ran under the small limit: the products z [chunk, N, C] of the two engines differ in size
    per_sample = c["N"] * c["C"] * 4
    chunk = (1 << 20) // per_sample
    assert 1 <= chunk < c["S"]
    assert model_a.engine.device_bytes() - eng_b.device_bytes() >= (c["S"] - chunk) * per_sample
    # a sample's numbers do not depend on its neighbours in the chunk
    assert torch.equal(model_a.engine.sampled_forward(idx, theta[7:9]), a1[7:9])


def _fitted(model, structure="diag", likelihood="classification", **kw):
    import laplace_gnn_amd as lg

    N, C = model.num_nodes, model.out_channels
    g = torch.Generator().manual_seed(11)
    idx = torch.randperm(N, generator=g)[:40].cuda()
    y = torch.randn(40, C, generator=g).cuda() if likelihood == "regression" else torch.randint(0, C, (40,), generator=g).cuda()
    la = lg.Laplace(model, likelihood, kw.pop("subset", "all"), structure, **kw)
    la.fit(lg.TensorBatchLoader(idx, y, batch_size=20))
    return la


@pytest.mark.parametrize("kind", ["gcn", "sage"])
def test_the_predictive_writes_nothing(kind):
    model, idx, _ = _case(dict(SMALL, kind=kind, S=1, M=33))
    la = _fitted(model)
    assert la._nn_device_route()
    eng = model.engine
    logits = model(idx).clone()
    state = [(p.data_ptr(), p._version) for p in model.parameters()]
    rebinds, versions = getattr(eng, "_rebinds", 0), list(eng._versions)
    la(idx, pred_type="nn", link_approx="mc", n_samples=6, generator=torch.Generator(device="cuda").manual_seed(0))
    ps = la.predictive_samples(idx, "nn", n_samples=6, generator=torch.Generator(device="cuda").manual_seed(0))
    assert ps.shape == (6, 33, 3) and torch.allclose(ps.sum(-1), torch.ones(6, 33, device="cuda"), atol=1e-5)
    assert [(p.data_ptr(), p._version) for p in model.parameters()] == state
    assert getattr(eng, "_rebinds", 0) == rebinds and eng._versions == versions
    assert torch.equal(model(idx), logits)
    eng.check_async_errors()


@pytest.mark.parametrize("path", CASES, ids=IDS)
def test_fronts_meet_the_reference_goldens(path):
    """``predictive_samples(x, "nn").mean(0)`` against the reference's Monte-Carlo predictive on the same draws, at the
    tolerance of test_gpu_frontend.py; plain 1- / 2-layer cases take the device route, the others the loop."""
    import laplace_gnn_amd as lg

    g = np.load(path)
    model = model_from_golden(g)
    loader = lg.TensorBatchLoader(torch.from_numpy(g["train_idx"]).cuda(), torch.from_numpy(g["train_y"]).cuda(),
                                  batch_size=int(g["batch_size"]))
    eps, idx = torch.from_numpy(g["pred_eps"]).cuda(), torch.from_numpy(g["pred_idx"]).cuda()
    plain = int(g["num_layers"]) <= 2 and not len(model.res) and model.norm_kind is None
    for structure in ("kron", "diag"):
        la = lg.Laplace(model, "classification", "all", structure)
        la.fit(loader)
        assert la._nn_device_route() == plain
        ps = la.predictive_samples(idx, "nn", n_samples=len(eps), eps=eps)
        assert ps.shape == (len(eps), len(idx), la.n_outputs)
        assert np.abs(ps.mean(0).cpu().numpy() - g[structure + "_nn_py"]).max() < 5e-5
    model.engine.check_async_errors()


def test_subnetwork_and_regression_fronts_equal_the_loop_route(monkeypatch):
    import laplace_gnn_amd as lg

    model, idx, _ = _case(dict(SMALL, kind="gcn", S=1, M=33))
    P = sum(p.numel() for p in model.parameters())
    sub = torch.randperm(P, generator=torch.Generator().manual_seed(2))[:25].cuda()
    la = _fitted(model, "diag", subset="subnetwork", subnetwork_indices=sub)
    assert isinstance(la, lg.DiagSubnetLaplace) and la._nn_device_route()
    eps = torch.randn(12, 25, generator=torch.Generator().manual_seed(4)).cuda()  # draws over the subnetwork
    fast = la(idx, pred_type="nn", link_approx="mc", eps=eps)
    with monkeypatch.context() as mp:
        mp.setattr(la, "_nn_device_route", lambda: False)
        slow = la(idx, pred_type="nn", link_approx="mc", eps=eps)
    assert (fast - slow).abs().max() < 1e-5
    # regression: mean and variance over the samples
    lr = _fitted(model, "diag", likelihood="regression", sigma_noise=0.7)
    assert lr._nn_device_route()
    eps = torch.randn(12, P, generator=torch.Generator().manual_seed(6)).cuda()
    m_fast, v_fast = lr(idx, pred_type="nn", link_approx="mc", eps=eps)
    with monkeypatch.context() as mp:
        mp.setattr(lr, "_nn_device_route", lambda: False)
        m_slow, v_slow = lr(idx, pred_type="nn", link_approx="mc", eps=eps)
    assert (m_fast - m_slow).abs().max() < 1e-5 and (v_fast - v_slow).abs().max() < 1e-5
    fs = lr.predictive_samples(idx, "nn", eps=eps)
    assert fs.shape == (12, 33, 3) and (fs.mean(0) - m_fast).abs().max() < 1e-6
    model.engine.check_async_errors()


@pytest.mark.parametrize("structure", ["kron", "diag"])
def test_last_layer_fronts_return_the_per_sample_softmax(structure):
    model, idx, _ = _case(dict(SMALL, kind="sage", S=1, M=33))
    la = _fitted(model, structure, subset="last_layer")
    state = [(p.data_ptr(), p._version) for p in model.parameters()]
    eps = torch.randn(9, la.n_params, generator=torch.Generator().manual_seed(9)).cuda()
    ps = la.predictive_samples(idx, "nn", eps=eps)
    assert ps.shape == (9, 33, 3) and torch.allclose(ps.sum(-1), torch.ones(9, 33, device="cuda"), atol=1e-5)
    assert (ps.mean(0) - la(idx, pred_type="nn", link_approx="mc", eps=eps)).abs().max() < 1e-6
    geps = torch.randn(3, 5, generator=torch.Generator().manual_seed(10)).cuda()
    gs = la.predictive_samples(idx, "glm", n_samples=5, eps=geps)
    assert gs.shape == (5, 33, 3)
    assert (gs.mean(0) - la(idx, pred_type="glm", link_approx="mc", n_samples=5, eps=geps)).abs().max() < 1e-6
    assert [(p.data_ptr(), p._version) for p in model.parameters()] == state
    model.engine.check_async_errors()


def test_out_of_scope_models_are_refused_and_the_fronts_keep_the_loop():
    import laplace_gnn_amd as lg

    ei = _small_graph(70)
    for what, kw, L in (("res / norm", dict(res=True, norm="layer"), 2), ("more than two layers", {}, 3)):
        model = _model("gcn", 70, 13, 20, 3, L, ei, False, **kw)
        eng = model.engine
        idx = torch.arange(0, 70, 3).cuda()
        theta = torch.zeros(2, eng.n_params, device="cuda")
        with pytest.raises(lg._lib.HipLibraryError, match=what):
            eng.sampled_forward(idx, theta)
        la = _fitted(model)
        assert not la._nn_device_route()
        eps = torch.randn(5, la.n_params, generator=torch.Generator().manual_seed(8)).cuda()
        got = la(idx, pred_type="nn", link_approx="mc", eps=eps)
        want = torch.softmax(_loop_route(model, idx, la.sample(eps=eps), params=la.params), dim=-1).mean(0)
        assert (got - want).abs().max() < 1e-6
        eng.check_async_errors()


def test_an_out_of_range_id_is_reported():
    import laplace_gnn_amd as lg

    model, idx, theta = _case(dict(SMALL, kind="gcn", S=2, M=33))
    bad = idx.clone()
    bad[4] = 70
    out = model.engine.sampled_forward(bad, theta)
    with pytest.raises(lg._lib.HipLibraryError, match="node index"):
        model.engine.check_async_errors()
    assert torch.equal(out[:, 4], torch.zeros(2, 3, device="cuda"))
    good = model.engine.sampled_forward(idx, theta)
    keep = torch.arange(33) != 4
    assert torch.equal(out[:, keep], good[:, keep])
    model.engine.check_async_errors()


def test_a_captured_fit_survives_the_sampling_predictive():
    """The entry's buffers are its own: a captured ``DiagLaplace.fit_graph`` holds raw pointers into the workspace and the
    forward cache, and replays correctly after a sampling predictive ran in between."""
    import laplace_gnn_amd as lg

    g = np.load(os.path.join(GOLDEN, "gcn_mid_3batch_sym_s1.npz"))
    model = model_from_golden(g)
    idx, y = torch.from_numpy(g["train_idx"]).cuda(), torch.from_numpy(g["train_y"]).cuda()
    loader = lg.TensorBatchLoader(idx, y, batch_size=int(g["batch_size"]))
    ref = lg.DiagLaplace(model, "classification")
    ref.fit(loader)
    H0, l0 = ref.H.clone(), float(ref.loss)
    la = lg.DiagLaplace(model, "classification")
    la.fit_graph = True
    la.fit(loader)
    la.fit(loader)  # captured and replayed
    assert la._fit_graph_state["graph"] is not None and not la._fit_graph_state["off"]
    assert la._nn_device_route()
    py = la(torch.from_numpy(g["pred_idx"]).cuda(), pred_type="nn", link_approx="mc", n_samples=16,
            generator=torch.Generator(device="cuda").manual_seed(0))
    assert torch.allclose(py.sum(-1), torch.ones(py.shape[0], device="cuda"), atol=1e-5)
    la.fit(loader)
    assert la._fit_graph_state["graph"] is not None and not la._fit_graph_state["off"]
    assert rel(la.H.cpu().numpy(), H0.cpu().numpy()) < 1e-6 and abs(float(la.loss) - l0) <= 1e-6 * abs(l0)
    model.engine.check_async_errors()
