"""GPU parity of the last-layer Kronecker / diagonal GGN kernels (csrc/lastlayer_kron.hip), their backend and fronts
(``KronLLLaplace`` / ``DiagLLLaplace``) and the Jacobian-free predictive, against the reference's numbers on the head
(tests/golden/lastlayer) and the fp64 restatement of the definitions (tests/lastlayer_reference.py).  fp32 <= 1e-4 relative
Frobenius per block.  Shapes are the smallest at which the kernels can go wrong: widths that do not fill a
tile (D = 33, 14), the widest head (D = 512, C = 47: four Gram tiles, C^2 entries over nine passes of a workgroup), C = 2, one
sample, a ragged chunk (M = 37), several workgroups with repeated ids (M = 1 000), a deeper model, an isolated batch node."""
import os

import numpy as np
import pytest
import torch

import gnn_laplace_oracle as O
import lastlayer_reference as R
from act_reference import ActReference
from conftest import GOLDEN
from gpu_utils import engine_from_golden, oracle_from_arrays, rel
from test_gpu_scale import _make

pytestmark = pytest.mark.gpu
RTOL = 1e-4
LL_GOLDENS = ["ll_gcn_dir_3batch", "ll_gcn_sym_1batch", "ll_sage_dir_1batch", "ll_sage_sym_3batch"]


def _accumulate(eng, idx, y, batch_size, fork_exact):
    """Sums over the batches through the engine: dict(A, B, Bb, diag, loss, diag_loss) as numpy."""
    idx, y = torch.as_tensor(idx).cuda(), torch.as_tensor(y).cuda()
    _, A, B, Bb, loss = eng.new_lastlayer_kron_buffers()
    C, D = eng.dims[-1], eng.in_dims[-1]
    dg, dloss = torch.zeros(C * D + C, device="cuda"), torch.zeros(1, device="cuda")
    n = idx.shape[0]
    for s0 in range(0, n, batch_size):
        eng.lastlayer_kron_accumulate(idx[s0:s0 + batch_size], y[s0:s0 + batch_size], n, A, B, Bb, loss, fork_exact=fork_exact)
        eng.lastlayer_diag_accumulate(idx[s0:s0 + batch_size], y[s0:s0 + batch_size], dg, dloss)
    eng.check_async_errors()
    return dict(A=A.cpu().numpy(), B=B.cpu().numpy(), Bb=Bb.cpu().numpy(), diag=dg.cpu().numpy(), loss=float(loss),
                diag_loss=float(dloss))


# ---- 1. the goldens through the C ABI --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LL_GOLDENS)
def test_goldens_through_the_c_abi(name):
    g = np.load(os.path.join(GOLDEN, "lastlayer", name + ".npz"))
    eng = engine_from_golden(g)
    phi, s, f = eng.lastlayer_features(torch.from_numpy(g["train_idx"]).cuda())
    assert rel(phi.cpu().numpy(), g["Phi"]) < RTOL and rel(s.cpu().numpy(), g["s"]) < RTOL
    for batch_size in (int(g["batch_size"]), 10000, 9):  # the golden's own batches, one batch, three ragged ones
        got = _accumulate(eng, g["train_idx"], g["train_y"], batch_size, fork_exact=True)
        up = _accumulate(eng, g["train_idx"], g["train_y"], batch_size, fork_exact=False)
        errs = dict(A=rel(got["A"], g["A"]), B=rel(got["B"], g["B"]), diag=rel(got["diag"], g["diag"]),
                    Bb_lambda=rel(up["Bb"], g["Bb_lambda"]), A_up=rel(up["A"], g["A"]))
        if str(g["kind"]) == "sage":
            errs.update(Bb=rel(got["Bb"], g["Bb"]), B_up=rel(up["B"], g["Bb_lambda"]))
        print(name, batch_size, {k: f"{v:.1e}" for k, v in errs.items()})
        assert max(errs.values()) < RTOL, errs
        for l in (got["loss"], got["diag_loss"], up["loss"]):
            assert abs(l - float(g["loss"])) < RTOL * abs(float(g["loss"]))
        assert np.array_equal(got["A"], got["A"].T) and rel(got["B"], got["B"].T) < 1e-6
    eng.close()


# ---- 2. against the fp64 restatement on random graphs ------------------------------------------------------------------------
CASES = {
    # name: kind, F, H, C, L, M, act
    "gcn_D33": ("gcn", 20, 33, 5, 2, 37, "relu"),
    "sage_D14_M1": ("sage", 10, 7, 4, 2, 1, "relu"),
    "sage_D512_C47_M1000": ("sage", 16, 256, 47, 2, 1000, "relu"),
    "gcn_C2": ("gcn", 12, 16, 2, 2, 37, "relu"),
    "gcn_3layer": ("gcn", 12, 24, 6, 3, 100, "relu"),
    "sage_3layer_tanh": ("sage", 9, 12, 5, 3, 37, "tanh"),
    "gcn_tanh_M1000": ("gcn", 14, 40, 7, 2, 1000, "tanh"),
}


def _random_case(kind, F, H, C, L, M, act, seed=5):
    N, E = 300, 1200
    ei, X, Ws, bs = _make(kind, N - 1, F, H, C, E, L=L, seed=seed)  # node N - 1 gets no edge at all
    X = torch.cat([X, torch.randn(1, F, generator=torch.Generator().manual_seed(seed + 1))])
    g = torch.Generator().manual_seed(seed + 2)
    idx = torch.randint(0, N, (M,), generator=g)  # with replacement: repeated ids are samples of their own
    idx[0] = N - 1                                # the isolated node is a batch sample
    y = torch.randint(0, C, (M,), generator=g)
    return N, ei, X, Ws, bs, idx, y


def _reference_features(kind, N, ei, X, Ws, bs, act, idx):
    """(phi, s, f) of the batch rows in fp64 (autograd-free part of tests/act_reference.py's forward)."""
    om = oracle_from_arrays(kind, N, ei.numpy(), X.numpy(), [w.numpy() for w in Ws], [b.numpy() for b in bs], True)
    ref = ActReference(kind, om.P, X, Ws, bs, act=act)
    with torch.no_grad():
        fw = ref.forward()
        a = fw["a"][-1]
        phi, s = (ref.P @ a, ref.P.sum(dim=1)) if kind == "gcn" else (a, torch.ones(N, dtype=torch.float64))
    ix = idx.numpy()
    return phi.numpy()[ix], s.numpy()[ix], fw["out"].numpy()[ix]


@pytest.mark.parametrize("case", list(CASES))
def test_kernels_against_the_fp64_restatement(case):
    import laplace_gnn_amd as lg

    kind, F, H, C, L, M, act = CASES[case]
    N, ei, X, Ws, bs, idx, y = _random_case(*CASES[case])
    eng = lg.GraphEngine(ei.cuda(), N, kind=kind, symmetric=True)
    eng.bind(X.cuda(), [w.cuda() for w in Ws], [b.cuda() for b in bs], act=act)
    phi, s, f = _reference_features(kind, N, ei, X, Ws, bs, act, idx)
    assert phi.shape[1] == eng.in_dims[-1]
    _, dg = R.diag_from_features(phi, s, f, y.numpy())
    for fork_exact in (True, False):
        loss, A, B, Bb = R.kron_from_features(phi, s, f, y.numpy(), 3 * M, fork_exact)
        _, Ag, Bg, Bbg, lg_ = eng.new_lastlayer_kron_buffers()
        eng.lastlayer_kron_accumulate(idx.cuda(), y.cuda(), 3 * M, Ag, Bg, Bbg, lg_, fork_exact=fork_exact)
        dgg, dl = torch.zeros(len(dg), device="cuda"), torch.zeros(1, device="cuda")
        eng.lastlayer_diag_accumulate(idx.cuda(), y.cuda(), dgg, dl)
        eng.check_async_errors()
        errs = dict(A=rel(Ag.cpu().numpy(), A), B=rel(Bg.cpu().numpy(), B), Bb=rel(Bbg.cpu().numpy(), Bb),
                    diag=rel(dgg.cpu().numpy(), dg), loss=abs(float(lg_) - loss) / loss, diag_loss=abs(float(dl) - loss) / loss)
        print(case, "fork" if fork_exact else "upstream", {k: f"{v:.1e}" for k, v in errs.items()})
        assert max(errs.values()) < RTOL, errs
    eng.close()


# ---- 3. consistency with what exists -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gcn", "sage"])
def test_consistent_with_the_full_last_layer_ggn_and_the_backend(kind):
    import laplace_gnn_amd as lg

    F, H, C, M = 11, 10, 4, 90
    N, ei, X, Ws, bs, idx, y = _random_case(kind, F, H, C, 2, M, "relu", seed=9)
    cls = lg.GCN if kind == "gcn" else lg.GraphSAGE
    model = cls(F, H, C, 2, X, ei, symmetric=True).cuda()
    with torch.no_grad():
        for conv, w, b in zip(model.convs, Ws, bs):
            conv.lin.weight.copy_(w)
            conv.lin.bias.copy_(b)
    eng = model.engine
    idx, y = idx.cuda(), y.cuda()
    D = eng.in_dims[-1]
    p_ll = C * D + C
    Hf, lf = torch.zeros(p_ll, p_ll, device="cuda"), torch.zeros(1, device="cuda")
    eng.lastlayer_full_accumulate(idx, y, Hf, lf)
    up = lg.HipGGN(model, "classification", last_layer=True, fork_exact_seed=False)
    loss_k, kron = up.kron(idx, y, N=M)
    loss_d, dg = up.diag(idx, y)
    assert dg.shape == (p_ll,) and len(kron.kfacs) == 2 and [t.shape[0] for F_ in kron.kfacs for t in F_] == [C, D, C]
    assert rel(dg.cpu().numpy(), torch.diagonal(Hf).cpu().numpy()) < RTOL
    (B, A), (Bb,) = kron.kfacs
    bias_block = Hf[C * D:, C * D:].cpu().numpy()
    assert rel((B if kind == "sage" else Bb).cpu().numpy(), bias_block) < RTOL
    assert abs(float(loss_k) - float(lf)) < RTOL * float(lf) and abs(float(loss_d) - float(lf)) < RTOL * float(lf)
    # ... and not the all-weights curvature, which last_layer=False still returns untouched
    allw = lg.HipGGN(model, "classification")
    _, kron_all = allw.kron(idx, y, N=M)
    _, dg_all = allw.diag(idx, y)
    assert len(kron_all.kfacs) == 4 and dg_all.shape == (eng.n_params,)
    # fresh tensors per call
    _, kron2 = up.kron(idx, y, N=M)
    assert kron2.kfacs[0][0].data_ptr() != B.data_ptr() and kron2.kfacs[0][1].data_ptr() != A.data_ptr()
    assert rel(kron2.kfacs[0][1].cpu().numpy(), A.cpu().numpy()) < 1e-6  # (float atomics: equal up to the order of the sums)


# ---- 4. the fronts ---------------------------------------------------------------------------------------------------------
def _gpu_model(kind, F=9, H=16, C=5, L=2, M=70, seed=3, **kw):
    import laplace_gnn_amd as lg

    N, ei, X, Ws, bs, idx, y = _random_case(kind, F, H, C, L, M, "relu", seed=seed)
    cls = lg.GCN if kind == "gcn" else lg.GraphSAGE
    model = cls(F, H, C, L, X, ei, symmetric=True, **kw).cuda()
    with torch.no_grad():
        for conv, w, b in zip(model.convs, Ws, bs):
            conv.lin.weight.copy_(w)
            conv.lin.bias.copy_(b)
    return model.eval(), idx.cuda(), y.cuda()


def _hand_marglik(loss, A, B, Bb, mean, delta):
    A, B, Bb, mean = (np.asarray(t, np.float64) for t in (A, B, Bb, mean))
    ld = np.log(np.outer(np.linalg.eigvalsh(B).clip(0), np.linalg.eigvalsh(A).clip(0)) + delta).sum()
    ld += np.log(np.linalg.eigvalsh(Bb).clip(0) + delta).sum()
    return -loss - 0.5 * (ld - len(mean) * np.log(delta) + delta * (mean * mean).sum())


@pytest.mark.parametrize("kind", ["gcn", "sage"])
def test_fronts_sum_the_batches_and_give_the_hand_marglik(kind):
    import laplace_gnn_amd as lg

    model, idx, y = _gpu_model(kind)
    M = idx.shape[0]
    loader = lg.TensorBatchLoader(idx, y, batch_size=48)  # 48 + 22
    want = _accumulate(model.engine, idx, y, 48, fork_exact=True)
    la = lg.Laplace(model, "classification", prior_precision=0.7)
    assert type(la) is lg.KronLLLaplace
    la.fit(loader)
    (B, A), (Bb,) = la.H_facs.kfacs
    assert rel(A.cpu().numpy(), want["A"]) < 1e-5 and rel(B.cpu().numpy(), want["B"]) < 1e-5
    assert rel(Bb.cpu().numpy(), want["Bb"]) < 1e-5
    assert float(la.loss) == pytest.approx(want["loss"], rel=1e-5) and la.n_data == M
    mean = torch.cat([model.convs[-1].lin.weight.reshape(-1), model.convs[-1].lin.bias]).detach().cpu().numpy()
    assert torch.equal(la.mean.cpu(), torch.from_numpy(mean))
    hand = _hand_marglik(float(la.loss), A.cpu(), B.cpu(), Bb.cpu(), mean, 0.7)
    got = float(la.log_marginal_likelihood())
    print(kind, "kron marglik", got, hand)
    assert abs(got - hand) < RTOL * abs(hand)
    ld = lg.Laplace(model, "classification", "last_layer", "diag", prior_precision=0.7)
    assert type(ld) is lg.DiagLLLaplace
    ld.fit(loader)
    assert rel(ld.H.cpu().numpy(), want["diag"]) < 1e-5 and float(ld.loss) == pytest.approx(want["loss"], rel=1e-5)
    Hd = ld.H.double().cpu().numpy()
    hand_d = -float(ld.loss) - 0.5 * (np.log(Hd + 0.7).sum() - len(mean) * np.log(0.7) + 0.7 * (mean.astype(np.float64) ** 2).sum())
    assert abs(float(ld.log_marginal_likelihood()) - hand_d) < RTOL * abs(hand_d)
    # a second fit with override=False: KronLaplace's discounting, the diagonal summed
    la.fit(loader, override=False)
    ld.fit(loader, override=False)
    (B2, A2), (Bb2,) = la.H_facs.kfacs
    assert rel(A2.cpu().numpy(), want["A"]) < 1e-5 and rel(B2.cpu().numpy(), 2 * want["B"]) < 1e-5
    assert rel(ld.H.cpu().numpy(), 2 * want["diag"]) < 1e-5 and la.n_data == 2 * M
    la.optimize_prior_precision(n_steps=5)
    assert float(la.prior_precision) > 0


# ---- 5. the predictive -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,res", [("gcn", False), ("sage", False), ("gcn", True)])
def test_predictive_without_jacobians(kind, res):
    import laplace_gnn_amd as lg
    from math import pi

    model, idx, y = _gpu_model(kind, res=res, norm="layer" if res else None)
    loader = lg.TensorBatchLoader(idx, y, batch_size=48)
    x = torch.arange(50, device="cuda")
    C, D = model.convs[-1].lin.weight.shape
    for sub in ("kron", "diag"):
        la = lg.Laplace(model, "classification", "last_layer", sub, prior_precision=1.0)
        la.fit(loader)
        Js, f = la.backend.last_layer_jacobians(x)
        Js64 = Js.double().cpu()
        if sub == "kron":
            (B, A), (Bb,) = [[t.double().cpu() for t in F_] for F_ in la.H_facs.kfacs]
            P = torch.block_diag(torch.kron(B, A), Bb) + torch.eye(C * D + C, dtype=torch.float64)
        else:
            P = torch.diag(la.H.double().cpu() + 1.0)
        want = torch.einsum("ncp,pq,nkq->nck", Js64, torch.linalg.inv(P), Js64)
        f_mu, f_var = la._glm_predictive_distribution(x)
        errs = dict(f_var=rel(f_var.cpu().numpy(), want.numpy()),
                    functional=rel(la.functional_variance(Js).cpu().numpy(), want.numpy()),
                    f_mu=rel(f_mu.cpu().numpy(), f.cpu().numpy()))
        kappa = 1 / torch.sqrt(1 + pi / 8 * torch.diagonal(want, dim1=1, dim2=2))
        probit = torch.softmax(kappa * f.double().cpu(), dim=-1)
        errs["probit"] = rel(la(x, pred_type="glm", link_approx="probit").cpu().numpy(), probit.numpy())
        print(kind, res, sub, {k: f"{v:.1e}" for k, v in errs.items()})
        assert max(errs.values()) < RTOL, errs
        for link in ("bridge", "bridge_norm", "mc"):
            p = la(x, link_approx=link, n_samples=10, generator=torch.Generator(device="cuda").manual_seed(0))
            assert p.shape == (50, C) and bool(torch.isfinite(p).all())
        # pred_type="nn": head samples on the features == writing every sample into the model and calling it
        eps = torch.randn(6, la.n_params, generator=torch.Generator().manual_seed(1)).cuda()
        before = [q.detach().clone() for q in model.parameters()]
        got = la(x, pred_type="nn", link_approx="mc", eps=eps)
        assert all(torch.equal(a, b) for a, b in zip(before, model.parameters()))
        head = model.convs[-1].lin
        outs = []
        with torch.no_grad():
            for th in la.sample(6, eps=eps):
                head.weight.copy_(th[:C * D].view(C, D))
                head.bias.copy_(th[C * D:])
                outs.append(torch.softmax(model(x), dim=-1))
            head.weight.copy_(before[[id(q) for q in model.parameters()].index(id(head.weight))])
            head.bias.copy_(before[[id(q) for q in model.parameters()].index(id(head.bias))])
        # fp32 rounding: the two routes sum the same D products per logit in different orders -- |f| <= ~10 gives ~1e-6 in f and
        # in the probabilities; a sample written to the wrong place would show at 1e-2
        assert torch.allclose(got, torch.stack(outs).mean(0), atol=1e-5, rtol=1e-5)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_and_flagged_batches():
    import laplace_gnn_amd as lg
    from laplace_gnn_amd._lib import HipLibraryError

    model, idx, y = _gpu_model("gcn")
    C = model.convs[-1].lin.weight.shape[0]
    loader = lg.TensorBatchLoader(idx, y, batch_size=48)
    for sub in ("kron", "diag"):
        with pytest.raises(NotImplementedError, match="classification"):
            lg.Laplace(model, "regression", "last_layer", sub)
        with pytest.raises(NotImplementedError, match="stochastic"):
            lg.Laplace(model, "classification", "last_layer", sub, backend_kwargs=dict(stochastic=True)).fit(loader)
        with pytest.raises(NotImplementedError):
            lg.Laplace(model, "classification", "last_layer", sub, backend=lg.HipEF).fit(loader)
    with pytest.raises(NotImplementedError, match="classification"):
        lg.HipGGN(model, "regression", last_layer=True)
    eng = model.engine
    _, A, B, Bb, loss = eng.new_lastlayer_kron_buffers()
    eng.set_likelihood("regression")  # the C ABI itself refuses a regression binding: a message, not a wrong number
    with pytest.raises(HipLibraryError, match="classification"):
        eng.lastlayer_kron_accumulate(idx, y, 70, A, B, Bb, loss)
    with pytest.raises(HipLibraryError, match="classification"):
        eng.lastlayer_diag_accumulate(idx, y, torch.zeros(eng.in_dims[-1] * C + C, device="cuda"), loss)
    eng.set_likelihood("classification")
    assert float(A.abs().sum()) == 0 and float(loss) == 0
    y_bad = y.clone()
    y_bad[60] = C
    idx_bad = idx.clone()
    idx_bad[3] = eng.num_nodes
    for sub in ("kron", "diag"):
        with pytest.raises(HipLibraryError, match="label"):
            lg.Laplace(model, "classification", "last_layer", sub).fit(lg.TensorBatchLoader(idx, y_bad, batch_size=48))
        with pytest.raises(HipLibraryError, match="node index"):
            lg.Laplace(model, "classification", "last_layer", sub).fit(lg.TensorBatchLoader(idx_bad, y, batch_size=48))
    la = lg.Laplace(model, "classification")
    la.fit(loader)  # the flags are cleared by the raising read: the next fit is clean
    with pytest.raises(NotImplementedError, match="adjacency"):
        la.neg_marglik_adj_grad(loader)
