"""Subnetwork Laplace on the GPU (csrc/subnet.hip behind ``lgnn_jacobians_subset`` / ``lgnn_subnet_full_accumulate``):

1. the fitted ``H`` is the sub-block of the reference's full-posterior ``H`` on the six small cases that carry it (closed-form
   and gather route), and marginal likelihood, samples and GLM predictive match the reference's own subnetwork Laplace;
2. ``lgnn_jacobians_subset`` equals the same columns of ``lgnn_jacobians`` (pinned to fp64 by tests/test_gpu_tanh.py) on
   graphs with a hub row, isolated nodes, duplicate edges, a repeated batch id and M = 1;
3. workspace chunks and ragged batches add up;
4. the regression GGN is ``J_S^T J_S`` of the existing Jacobians;
5. ``LargestVarianceDiagLaplaceSubnetMask`` -> ``FullSubnetLaplace`` end to end.
Every case prints what it measured."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from subnet_utils import SETS, SUBNET_CASES, model_from_golden, param_ranges, rel, subnet_golden

pytestmark = pytest.mark.gpu
RTOL = 1e-4
# Largest relative difference max|a - b| / max|b| between lgnn_jacobians_subset and the same columns of lgnn_jacobians over
# every case of test_jacobians_subset_equals_columns, measured on the first GPU run: 0 -- both routes
# evaluate the same fp32 products in the same order.  The bound is 4x the measured value.
JAC_SUBSET_MEASURED = 0.0
JAC_SUBSET_BOUND = 4 * JAC_SUBSET_MEASURED
assert JAC_SUBSET_BOUND <= 1e-6

FULL_CASES = ("gcn_small_1batch_s0", "sage_small_1batch_s0", "gcn3_small_1batch_s0", "sage3_small_1batch_s0",
              "gcn_resln_small_1batch_s0", "sage_resln_small_1batch_s0")
BLOCK_SETS = [(c, s) for c in FULL_CASES for s in (SETS if c in SUBNET_CASES else ()) + ("all_reversed", "single")]


def _indices(case, which, P):
    if which == "all_reversed":
        return torch.arange(P - 1, -1, -1)
    if which == "single":
        return torch.tensor([P // 2])
    return torch.from_numpy(subnet_golden(case)[which + "_indices"])


@pytest.mark.parametrize("case,which", BLOCK_SETS, ids=[f"{c}-{s}" for c, s in BLOCK_SETS])
def test_subnet_fit_is_the_reference_sub_block(case, which):
    import laplace_gnn_amd as lg

    g = np.load(os.path.join(GOLDEN, case + ".npz"))
    model = model_from_golden(g, "cuda")
    P = int(g["n_params"])
    idx = _indices(case, which, P)
    sel = idx.numpy()
    loader = lg.TensorBatchLoader(torch.from_numpy(g["train_idx"]).cuda(), torch.from_numpy(g["train_y"]).cuda(),
                                  batch_size=int(g["batch_size"]))
    la = lg.Laplace(model, "classification", "subnetwork", "full", subnetwork_indices=idx, prior_precision=0.7)
    assert isinstance(la, lg.FullSubnetLaplace) and la._backend_cls is lg.HipGGN
    la.fit(loader)
    block = g["fullla_H"][sel][:, sel]
    assert np.linalg.norm(block) > 0
    e_h, e_l = rel(la.H.cpu().numpy(), block), abs(float(la.loss) - float(g["full_loss"])) / abs(float(g["full_loss"]))
    ld = lg.Laplace(model, "classification", "subnetwork", "diag", subnetwork_indices=idx, prior_precision=0.7)
    ld.fit(loader)
    assert np.linalg.norm(g["diag_H"][sel]) > 0
    e_d = rel(ld.H.cpu().numpy(), g["diag_H"][sel])
    print(f"{case} {which} S={len(sel)}: H {e_h:.2e} loss {e_l:.2e} diag {e_d:.2e}")
    assert tuple(la.H.shape) == (len(sel), len(sel)) and e_h < RTOL and e_l < RTOL
    assert torch.equal(la.H, la.H.T)
    assert tuple(ld.H.shape) == (len(sel),) and e_d < RTOL
    assert abs(float(ld.loss) - float(g["diag_loss"])) < RTOL * abs(float(g["diag_loss"]))
    if which in SETS:
        sg, k = subnet_golden(case), which + "_"
        assert rel(la.H.cpu().numpy(), sg[k + "H"]) < RTOL and rel(ld.H.cpu().numpy(), sg[k + "diag_H"]) < RTOL
        for obj, pre in ((la, ""), (ld, "diag_")):
            for pp, key in ((None, "marglik_pp07"), (torch.tensor(1.0), "marglik_pp1")):
                got, want = float(obj.log_marginal_likelihood(prior_precision=pp)), float(sg[k + pre + key])
                print(f"  {pre}{key}: {abs(got - want) / abs(want):.2e}")
                assert abs(got - want) < 3e-4 * abs(want)
            obj.prior_precision = 0.7
        eps, pidx = torch.from_numpy(sg[k + "eps"]).cuda(), torch.from_numpy(g["pred_idx"]).cuda()
        samples = la.sample(eps=eps)
        _, f_var = la._glm_predictive_distribution(pidx)
        e_s, e_v = rel(samples.cpu().numpy(), sg[k + "samples"]), rel(f_var.cpu().numpy(), sg[k + "glm_fvar"])
        e_p = np.abs(la(pidx).cpu().numpy() - sg[k + "glm_probit"]).max()
        print(f"  samples {e_s:.2e} f_var {e_v:.2e} probit {e_p:.2e}")
        assert e_s < 1e-4 and e_v < 1e-4 and e_p < 1e-4
        rest = np.setdiff1d(np.arange(P), sel)
        assert torch.equal(samples[:, rest], la.mean[rest].expand(eps.shape[0], -1))
        assert rel(ld.sample(eps=eps).cpu().numpy(), sg[k + "diag_samples"]) < 1e-4
        assert np.abs(ld(pidx).cpu().numpy() - sg[k + "diag_glm_probit"]).max() < 1e-4
        probs = la(pidx, pred_type="nn", link_approx="mc", eps=eps)
        assert torch.allclose(probs.sum(-1), torch.ones(len(pidx), device="cuda"), atol=1e-5)
    model.engine.check_async_errors()


# ---- kernel edges -------------------------------------------------------------------------------------------------
def edge_graph(N, seed):
    """Random edges with duplicates, node 3 with more than 64 stored entries, nodes N-1 and N-2 isolated."""
    g = torch.Generator().manual_seed(seed)
    hi = N - 2
    ei = torch.randint(0, hi, (2, 3 * N), generator=g)
    hub = torch.randperm(hi, generator=g)[:70]
    ei = torch.cat([ei, ei[:, :N // 3], torch.stack([torch.full((70,), 3), hub]), torch.stack([hub, torch.full((70,), 3)])], 1)
    return ei


def edge_model(kind, L, act, shape, seed=0):
    import laplace_gnn_amd as lg

    N, F, H, C = shape
    g = torch.Generator().manual_seed(seed + 1)
    X = torch.randn(N, F, generator=g)
    torch.manual_seed(seed)
    cls = lg.GCN if kind == "gcn" else lg.GraphSAGE
    return cls(F, H, C, L, X, edge_graph(N, seed), act=act).eval().cuda()


def edge_batch(N, M=37, seed=0):
    idx = torch.randperm(N - 2, generator=torch.Generator().manual_seed(seed + 2))[:M].clone()
    idx[0], idx[1], idx[2] = 3, N - 1, N - 2  # the hub, the isolated nodes
    idx[7] = idx[9]                           # a repeated id
    return idx.cuda()


def edge_index_sets(model, seed=0):
    r = param_ranges(model)
    L = len(model.convs)
    P = sum(n for _, n in r.values())
    w0, nw0 = r["convs.0.lin.weight"]
    b0, nb0 = r["convs.0.lin.bias"]
    in0 = nw0 // nb0
    wl, nwl = r[f"convs.{L - 1}.lin.weight"]
    bl, nbl = r[f"convs.{L - 1}.lin.bias"]
    g = torch.Generator().manual_seed(seed + 3)
    S = min(257, P - 1)
    S -= S % 4 == 0  # S % 4 != 0: the padded row stride differs from S (257 wherever P allows it)
    return {
        "first_bias": torch.arange(b0, b0 + nb0).flip(0),
        "last_layer": torch.cat([torch.arange(bl, bl + nbl), torch.arange(wl, wl + nwl)]),
        "first_row": torch.arange(w0 + in0 * (nb0 // 2), w0 + in0 * (nb0 // 2 + 1)),
        "random": torch.randperm(P, generator=g)[:S],
        "all_unsorted": torch.randperm(P, generator=g),
    }, P


EDGE_SHAPES = [(96, 13, 10, 5), (300, 37, 64, 7)]
EDGE_CASES = [(k, L, a, s) for k in ("gcn", "sage") for L in (1, 2) for a in ("relu", "tanh") for s in EDGE_SHAPES]


@pytest.mark.parametrize("kind,L,act,shape", EDGE_CASES, ids=[f"{k}{L}-{a}-N{s[0]}" for k, L, a, s in EDGE_CASES])
def test_jacobians_subset_equals_columns(kind, L, act, shape):
    model = edge_model(kind, L, act, shape)
    eng = model.engine
    sets, P = edge_index_sets(model)
    assert P == eng.n_params
    if shape == EDGE_SHAPES[1]:
        assert sets["random"].numel() == 257
    worst = 0.0
    for idx in (edge_batch(shape[0]), edge_batch(shape[0])[:1]):  # M = 37 and M = 1 (the hub row)
        J, f = eng.jacobians(idx)
        scale = float(J.abs().max())
        assert scale > 0
        for name, sub in sets.items():
            Js, fs = eng.jacobians_subset(idx, sub.cuda())
            want = J[:, :, sub.cuda()]
            assert tuple(Js.shape) == (idx.numel(), shape[3], sub.numel()) and torch.equal(fs, f)
            assert float(want.abs().max()) > 0, name
            d = float((Js - want).abs().max()) / scale
            worst = max(worst, d)
            assert d <= JAC_SUBSET_BOUND, (name, d)
    print(f"{kind} L={L} {act} N={shape[0]} P={P}: largest relative difference {worst:.3e}")
    eng.check_async_errors()


@pytest.mark.parametrize("kind,L", [("gcn", 2), ("sage", 1), ("gcn", 3)])
def test_out_of_range_ids_give_zeros_and_the_sticky_flag(kind, L):
    import laplace_gnn_amd as lg

    shape = EDGE_SHAPES[0]
    model = edge_model(kind, L, "relu", shape)
    eng = model.engine
    sets, P = edge_index_sets(model)
    sub = sets["random"].cuda()
    idx = edge_batch(shape[0])
    good, _ = eng.jacobians_subset(idx, sub)
    eng.check_async_errors()
    bad_idx = idx.clone()
    bad_idx[4], bad_idx[11] = shape[0], -1
    Js, _ = eng.jacobians_subset(bad_idx, sub)
    keep = torch.ones(idx.numel(), dtype=torch.bool, device="cuda")
    keep[[4, 11]] = False
    assert torch.equal(Js[keep], good[keep]) and float(Js[~keep].abs().max()) == 0.0
    with pytest.raises(lg._lib.HipLibraryError, match="node index"):
        eng.check_async_errors()
    eng.check_async_errors()  # cleared
    # an out-of-range subnetwork index (the front validates on the host; the device is the backstop): a zero column
    bad_sub = sub.clone()
    bad_sub[5] = P
    Js, _ = eng.jacobians_subset(idx, bad_sub)
    cols = torch.ones(sub.numel(), dtype=torch.bool, device="cuda")
    cols[5] = False
    assert torch.equal(Js[:, :, cols], good[:, :, cols]) and float(Js[:, :, 5].abs().max()) == 0.0
    with pytest.raises(lg._lib.HipLibraryError, match="subnetwork index"):
        eng.check_async_errors()
    eng.check_async_errors()


# ---- chunking, additivity, regression ---------------------------------------------------------------------------------
ROUTES = [("gcn", 2, 200), ("sage", 2, 200), ("gcn", 3, 60)]  # closed form, closed form, gather: kind, layers, batch size


@pytest.mark.parametrize("kind,L,M", ROUTES, ids=["gcn2-closed", "sage2-closed", "gcn3-gather"])
def test_chunks_and_ragged_batches_add_up(kind, L, M):
    import laplace_gnn_amd as lg

    shape = EDGE_SHAPES[1]
    N, F, H, C = shape
    model = edge_model(kind, L, "relu", shape, seed=4)
    eng = model.engine
    sets, P = edge_index_sets(model, seed=4)
    sub = sets["random"]
    S, ld = sub.numel(), -(-sub.numel() // 4) * 4
    g = torch.Generator().manual_seed(9)
    idx = torch.randint(0, N, (M,), generator=g).cuda()
    y = torch.randint(0, C, (M,), generator=g).cuda()

    def fit(batch_size):
        la = lg.Laplace(model, "classification", "subnetwork", "full", subnetwork_indices=sub)
        la.fit(lg.TensorBatchLoader(idx, y, batch_size=batch_size))
        return la.H.clone(), float(la.loss)

    H_one, loss_one = fit(M)
    H_ragged, loss_ragged = fit(-(-M * 3 // 8))  # three ragged batches
    assert -(-M // -(-M * 3 // 8)) == 3 and M % -(-M * 3 // 8) != 0
    limit = 1 << 20
    per_sample = C * (ld if L <= 2 else P + ld) * 4  # csrc/subnet.hip: bytes of a sample's rows in the chunk buffers
    assert limit // per_sample >= 1 and M > limit // per_sample, "the batch must go through at least two chunks"
    eng.set_workspace_limit(limit)
    H_chunk, loss_chunk = fit(M)
    e_r, e_c = rel(H_ragged.cpu().numpy(), H_one.cpu().numpy()), rel(H_chunk.cpu().numpy(), H_one.cpu().numpy())
    print(f"{kind} L={L} S={S} M={M}: ragged {e_r:.2e} chunked ({-(-M // (limit // per_sample))} chunks) {e_c:.2e}")
    assert float(H_one.norm()) > 0 and e_r < 1e-5 and e_c < 1e-5
    assert abs(loss_ragged - loss_one) < 1e-5 * abs(loss_one) and abs(loss_chunk - loss_one) < 1e-5 * abs(loss_one)
    # and the sub-block of the existing full fit
    if P * P * 4 < 1 << 28:
        lf = lg.Laplace(model, "classification", "all", "full")
        eng.set_workspace_limit(32 << 30)
        lf.fit(lg.TensorBatchLoader(idx, y, batch_size=M))
        e_f = rel(H_one.cpu().numpy(), lf.H[sub.cuda()][:, sub.cuda()].cpu().numpy())
        print(f"  against FullLaplace.H[S][:, S]: {e_f:.2e}")
        assert e_f < 1e-5
    eng.check_async_errors()


@pytest.mark.parametrize("kind,L,M", ROUTES, ids=["gcn2-closed", "sage2-closed", "gcn3-gather"])
def test_regression_ggn_is_the_gram_of_the_subset_jacobians(kind, L, M):
    import laplace_gnn_amd as lg

    shape = EDGE_SHAPES[1]
    N, F, H, C = shape
    model = edge_model(kind, L, "relu", shape, seed=5)
    sets, P = edge_index_sets(model, seed=5)
    sub = sets["random"].cuda()
    g = torch.Generator().manual_seed(10)
    idx = torch.randint(0, N, (M,), generator=g).cuda()
    y = torch.randn(M, C, generator=g).cuda()
    be = lg.HipGGN(model, "regression", subnetwork_indices=sub)
    loss, Hs = be.full(idx, y)
    be.subnetwork_indices = None
    J, f = be.jacobians(idx)
    Jd = J[:, :, sub].double().reshape(M * C, -1)
    want = Jd.T @ Jd
    # 1e-5: the bound re-batched fp32 sums get (test_full_laplace_all_weights); a Gram over M C rows in fp32 against fp64
    e = rel(Hs.cpu().numpy(), want.cpu().numpy())
    e_l = abs(float(loss) - 0.5 * float(((f - y) ** 2).sum())) / float(loss)
    print(f"{kind} L={L} regression: H {e:.2e} loss {e_l:.2e}")
    assert float(want.norm()) > 0 and e < 1e-5 and e_l < 1e-5
    model.engine.check_async_errors()


def test_largest_variance_mask_end_to_end():
    import laplace_gnn_amd as lg

    shape = EDGE_SHAPES[1]
    N, F, H, C = shape
    model = edge_model("gcn", 2, "relu", shape, seed=6)
    g = torch.Generator().manual_seed(11)
    idx = torch.randint(0, N, (150,), generator=g).cuda()
    y = torch.randint(0, C, (150,), generator=g).cuda()
    loader = lg.TensorBatchLoader(idx, y, batch_size=64)
    diag = lg.Laplace(model, "classification", "all", "diag")
    mask = lg.LargestVarianceDiagLaplaceSubnetMask(model, 300, diag)
    sub = mask.select(loader)
    var = 1.0 / diag.posterior_precision
    assert sub.numel() == 300 and sub.unique().numel() == 300 and sub.is_cuda
    assert float(var[sub].min()) >= float(torch.sort(var, descending=True).values[299])
    la = lg.Laplace(model, "classification", "subnetwork", "full", subnetwork_indices=sub)
    la.fit(loader)
    probs = la(torch.arange(N).cuda())
    assert tuple(probs.shape) == (N, C) and torch.allclose(probs.sum(-1), torch.ones(N, device="cuda"), atol=1e-5)
    assert bool(torch.isfinite(la.log_marginal_likelihood()))
    model.engine.check_async_errors()
