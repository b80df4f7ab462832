"""Training-mode forward with HIP weight gradients (csrc/train.hip) on the device: the five lines of the reference's loop
(gnn/marglik_training.py:165-186) on the ``lg.*`` models, against the reference's own goldens (tests/golden/train/*.npz,
tools/make_train_golden.py) and against an fp64 torch restatement at a mid-size shape.  Bar: relative Frobenius error
<= 1e-4 per tensor (BASELINE.json north_star; RTOL of the GPU suites)."""
import glob
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F_

from conftest import GOLDEN
from test_gpu_scale import _make
from test_train_golden import batches, rel

pytestmark = pytest.mark.gpu

RTOL = 1e-4
TRAIN = os.path.join(GOLDEN, "train")
CASES = sorted(glob.glob(os.path.join(TRAIN, "*.npz")))
IDS = [os.path.basename(p)[:-4] for p in CASES]


def model_from_train_golden(g, step=0):
    import laplace_gnn_amd as lg

    X, ei = torch.from_numpy(g["X"]), torch.from_numpy(g["edge_index"])
    L, H = int(g["num_layers"]), int(g["hidden"])
    C = g[f"P/convs.{L - 1}.lin.bias"].shape[1]
    cls = {"gcn": lg.GCN, "sage": lg.GraphSAGE, "stegcn": lg.STEGCN}[str(g["model"])]
    model = cls(X.shape[1], H, C, L, X, ei, dropout_p=float(g["p"]), act=str(g["act"]), symmetric=bool(g["symmetric"]),
                res=bool(g["res"]), norm=str(g["norm"]) or None)
    names = [str(k) for k in g["names"]]
    assert [k for k, _ in model.named_parameters() if "adj" not in k] == names  # the reference's own parameter order
    model = model.cuda()
    load_step(model, g, step)
    return model, names


def load_step(model, g, step):
    params = dict(model.named_parameters())
    with torch.no_grad():
        for k in g["names"]:
            params[str(k)].copy_(torch.from_numpy(g["P/" + str(k)][step]))


def masks_of(g, s):
    return [torch.from_numpy(g[f"masks_{l}"][s]).cuda() for l in range(int(g["num_layers"]) - 1)]


@pytest.mark.parametrize("path", CASES, ids=IDS)
def test_every_step_of_the_reference_loop(path):
    """Per step: the parameters the reference had BEFORE that step, its masks, its batch -> logits, loss, every p.grad."""
    g = np.load(path)
    model, names = model_from_train_golden(g)
    params = dict(model.named_parameters())
    bt = batches(g)
    for s in range(len(g["loss"])):
        load_step(model, g, s)
        idx, y = (torch.from_numpy(a).cuda() for a in bt[int(g["batch_of_step"][s])])
        model.train()
        model.zero_grad(set_to_none=True)
        model.set_dropout_masks(masks_of(g, s))
        f = model(idx)
        loss = F_.cross_entropy(f, y)
        loss.backward()
        assert rel(f.detach().cpu().numpy(), g[f"logits_{s}"]) <= RTOL, ("logits", s)
        assert abs(float(loss) - float(g["loss"][s])) <= RTOL * abs(float(g["loss"][s])), ("loss", s)
        for k in names:
            e = rel(params[k].grad.cpu().numpy(), g["G/" + k][s])
            print(f"{os.path.basename(path)} step {s} {k}: {e:.2e}")
            assert e <= RTOL, (k, s, e)
        for k, p in model.named_parameters():
            if "adj" in k:
                assert p.grad is None, k
    model.engine.check_async_errors()


@pytest.mark.parametrize("path", CASES, ids=IDS)
def test_the_loop_unchanged_with_adam(path):
    """gnn/marglik_training.py:91-93, 159-186 as written, three epochs from the initial parameters with the stored masks."""
    g = np.load(path)
    model, names = model_from_train_golden(g)
    optimizer = torch.optim.Adam([v for k, v in model.named_parameters() if "adj" not in k], lr=float(g["lr"]),
                                 weight_decay=float(g["weight_decay"]))
    criterion = torch.nn.CrossEntropyLoss()
    bt = batches(g)
    s = 0
    for _ in range(int(g["epochs"])):
        model.train()
        for idx, y in bt:
            train_indices, train_labels = torch.from_numpy(idx).cuda(), torch.from_numpy(y).cuda()
            model.set_dropout_masks(masks_of(g, s))
            f = model(train_indices)
            optimizer.zero_grad()
            loss = criterion(f, train_labels)
            loss.backward()
            optimizer.step()
            assert abs(loss.item() - float(g["loss"][s])) <= RTOL * abs(float(g["loss"][s])), ("loss", s)
            s += 1
    params = dict(model.named_parameters())
    for k in names:
        e = rel(params[k].detach().cpu().numpy(), g["P/" + k][-1])
        print(f"{os.path.basename(path)} {k} after {s} steps: {e:.2e}")
        assert e <= RTOL, (k, e)


# ---- mid size against fp64 ----------------------------------------------------------------------------------------------
def _midsize_model(kind, L, res, norm, N=3000, F=72, H=64, C=9, E=12000, p=0.5, act="relu", seed=11):
    import laplace_gnn_amd as lg

    ei, X, Ws, bs = _make(kind, N, F, H, C, E, L=L, seed=seed, skew=True)
    cls = lg.GCN if kind == "gcn" else lg.GraphSAGE
    torch.manual_seed(seed)
    model = cls(F, H, C, L, X, ei, dropout_p=p, act=act, symmetric=True, res=res, norm=norm)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for l, conv in enumerate(model.convs):
            conv.lin.weight.copy_(Ws[l])
            conv.lin.bias.copy_(bs[l])
        if norm == "layer":
            for m in model.norms:
                m.weight.add_(0.2 * torch.randn(H, generator=gen))
                m.bias.add_(0.2 * torch.randn(H, generator=gen))
    return model.cuda()


def _fp64_grads(model, idx, y, masks, p):
    """torch autograd in fp64 on the CPU over a sparse P from export_propagation."""
    r, c, v = model.engine.export_propagation()
    N = model.num_nodes
    P = torch.sparse_coo_tensor(torch.stack([r, c]).cpu(), v.cpu().double(), (N, N)).coalesce()
    prm = {k: t.detach().cpu().double().requires_grad_(True) for k, t in model.named_parameters() if "adj" not in k}
    x = model.X.detach().cpu().double()
    L = model.num_layers
    for l in range(L):
        W, b = prm[f"convs.{l}.lin.weight"], prm[f"convs.{l}.lin.bias"]
        if model.kind == "gcn":
            s = torch.sparse.mm(P, x @ W.T + b)
        else:
            s = torch.cat([x, torch.sparse.mm(P, x)], 1) @ W.T + b
        if l == L - 1:
            break
        if len(model.res):
            s = s + x @ prm[f"res.{l}.weight"].T + prm[f"res.{l}.bias"]
        if model.norm_kind == "layer":
            s = F_.layer_norm(s, (s.shape[1],), prm[f"norms.{l}.weight"], prm[f"norms.{l}.bias"], model.norms[l].eps)
        a = torch.relu(s) if model.act_name == "relu" else torch.tanh(s)
        x = a if masks is None else a * masks[l].cpu().double() / (1.0 - p)
    f = s[idx.cpu()]
    loss = F_.cross_entropy(f, y.cpu())
    loss.backward()
    return f.detach(), float(loss), {k: t.grad for k, t in prm.items()}


def _check_against_fp64(model, M=2000, batch=700, p=0.5, seed=5):
    N, H = model.num_nodes, model.hidden_channels
    gen = torch.Generator().manual_seed(seed)
    idx_all = torch.randperm(N, generator=gen)[:M]
    idx_all[7] = idx_all[3]  # a repeated node id
    y_all = torch.randint(0, model.out_channels, (M,), generator=gen)
    params = {k: t for k, t in model.named_parameters() if "adj" not in k}
    model.train()
    for b0 in range(0, M, batch):
        idx, y = idx_all[b0:b0 + batch].cuda(), y_all[b0:b0 + batch].cuda()
        masks = [(torch.rand(N, H, generator=gen) >= p).to(torch.uint8).cuda() for _ in range(model.num_layers - 1)]
        model.zero_grad(set_to_none=True)
        model.set_dropout_masks(masks)
        f = model(idx)
        loss = F_.cross_entropy(f, y)
        loss.backward()
        rf, rloss, rg = _fp64_grads(model, idx, y, masks, p)
        assert rel(f.detach().cpu().numpy(), rf.numpy()) <= RTOL
        assert abs(float(loss) - rloss) <= RTOL * abs(rloss)
        for k, t in params.items():
            e = rel(t.grad.cpu().numpy(), rg[k].numpy())
            print(f"{model.kind} L={model.num_layers} batch@{b0} {k}: {e:.2e}")
            assert e <= RTOL, (k, b0, e)
    model.engine.check_async_errors()


@pytest.mark.parametrize("kind", ["gcn", "sage"])
@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("res,norm", [(False, None), (True, "layer")])
def test_midsize_gradients_vs_fp64(kind, L, res, norm):
    _check_against_fp64(_midsize_model(kind, L, res, norm))


@pytest.mark.parametrize("kind,kw", [("gcn", dict(F=1433)), ("sage", dict(F=1433)), ("gcn", dict(H=256)), ("sage", dict(H=256)),
                                     ("gcn", dict(act="tanh"))])
def test_midsize_wide_shapes_vs_fp64(kind, kw):
    """Cora's feature width (1 433: not a multiple of 4) and a 256-wide hidden layer."""
    _check_against_fp64(_midsize_model(kind, 2, True, "layer", **kw))


# ---- properties ---------------------------------------------------------------------------------------------------------
def _grads_once(model, idx, y, masks):
    model.train()
    model.zero_grad(set_to_none=True)
    model.set_dropout_masks(masks)
    F_.cross_entropy(model(idx), y).backward()
    return {k: t.grad.clone() for k, t in model.named_parameters() if t.grad is not None}


@pytest.mark.parametrize("kind,L,kw", [
    ("gcn", 3, {}), ("sage", 3, {}),
    # shapes at which a GEMM with few output tiles and a long K would split K over workgroups: Cora's feature width on a
    # Cora-sized graph (K = 1 433 resp. 2 866, 22 row tiles) and a 256-wide res model on a small graph (dx GEMM: K = 512)
    ("gcn", 2, dict(N=2708, F=1433, E=10556)), ("sage", 2, dict(N=2708, F=1433, E=10556)),
    ("gcn", 3, dict(N=1500, H=256, E=6000)), ("sage", 3, dict(N=1500, H=256, E=6000)),
])
def test_two_identical_calls_agree_bit_for_bit(kind, L, kw):
    model = _midsize_model(kind, L, True, "layer", **kw)
    N, H = model.num_nodes, model.hidden_channels
    gen = torch.Generator().manual_seed(1)
    idx = torch.randint(0, N, (1200,), generator=gen).cuda()  # many repeated ids
    y = torch.randint(0, model.out_channels, (1200,), generator=gen).cuda()
    masks = [(torch.rand(N, H, generator=gen) >= 0.5).to(torch.uint8).cuda() for _ in range(L - 1)]
    runs = [_grads_once(model, idx, y, masks) for _ in range(3)]
    assert len(runs[0]) == len(list(model.parameters()))
    for other in runs[1:]:
        for k in runs[0]:
            assert torch.equal(runs[0][k], other[k]), k
    model.train()
    model.set_dropout_masks(masks)
    f1 = model(idx).detach().clone()
    model.set_dropout_masks(masks)
    assert torch.equal(model(idx).detach(), f1)


@pytest.mark.parametrize("kind", ["gcn", "sage"])
def test_eval_forward_is_untouched_and_follows_the_optimizer(kind):
    import laplace_gnn_amd as lg

    model = _midsize_model(kind, 2, True, "layer")
    N = model.num_nodes
    gen = torch.Generator().manual_seed(2)
    idx = torch.randperm(N, generator=gen)[:900].cuda()
    y = torch.randint(0, model.out_channels, (900,), generator=gen).cuda()
    before = model.eval()(idx).clone()
    # p = 0: the training forward computes what the eval forward computes
    model.dropout.p = 0.0
    f0 = model.train()(idx)
    assert f0.grad_fn is not None
    assert rel(f0.detach().cpu().numpy(), before.cpu().numpy()) <= 1e-6
    # p = 0.5: dropped activations never reach the cache the eval-mode calls read
    model.dropout.p = 0.5
    opt = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=5e-4)
    f = model.train()(idx)
    assert torch.equal(model.eval()(idx), before)
    opt.zero_grad()
    F_.cross_entropy(f, y).backward()
    assert torch.equal(model.eval()(idx), before)
    opt.step()
    after = model.eval()(idx)
    assert not torch.equal(after, before)
    # la.fit on the stepped model == a fresh model built from the stepped state_dict
    loader = lg.TensorBatchLoader(idx, y, batch_size=300)
    la = lg.Laplace(model, "classification", "all", "kron")
    la.fit(loader)
    fresh = _midsize_model(kind, 2, True, "layer")
    fresh.load_state_dict(model.state_dict())
    assert torch.equal(fresh.eval()(idx), after)
    lb = lg.Laplace(fresh, "classification", "all", "kron")
    lb.fit(loader)
    va, vb = float(la.log_marginal_likelihood()), float(lb.log_marginal_likelihood())
    assert abs(va - vb) <= 1e-5 * abs(vb)


def test_backward_without_a_matching_forward_raises():
    import laplace_gnn_amd as lg

    model = _midsize_model("gcn", 2, False, None).train()
    idx = torch.arange(50).cuda()
    y = torch.zeros(50, dtype=torch.int64).cuda()
    loss = F_.cross_entropy(model(idx), y)
    loss.backward(retain_graph=True)
    with pytest.raises(lg._lib.HipLibraryError, match="without a matching"):
        loss.backward()
    loss = F_.cross_entropy(model(idx), y)
    with torch.no_grad():
        model.convs[0].lin.bias.add_(1.0)  # a parameter write between forward and backward: the tape is stale
    with pytest.raises(lg._lib.HipLibraryError, match="without a matching"):
        loss.backward()
    f1 = model(idx)
    f2 = model(idx)  # one tape per engine: the older forward's backward is refused
    with pytest.raises(lg._lib.HipLibraryError, match="another training forward"):
        f1.sum().backward()
    f2.sum().backward()


def test_gradients_accumulate_into_an_existing_grad():
    model = _midsize_model("sage", 2, True, "layer")
    N, H = model.num_nodes, model.hidden_channels
    gen = torch.Generator().manual_seed(3)
    idx = torch.randperm(N, generator=gen)[:400].cuda()
    y = torch.randint(0, model.out_channels, (400,), generator=gen).cuda()
    masks = [(torch.rand(N, H, generator=gen) >= 0.5).to(torch.uint8).cuda()]
    one = _grads_once(model, idx, y, masks)
    model.set_dropout_masks(masks)
    F_.cross_entropy(model(idx), y).backward()  # no zero_grad in between
    for k, t in model.named_parameters():
        assert torch.equal(t.grad, 2 * one[k]), k


def test_drawn_masks():
    model = _midsize_model("gcn", 2, False, None).train()
    N, H, p = model.num_nodes, model.hidden_channels, 0.5
    idx = torch.arange(10).cuda()

    def draw():
        model(idx)
        (m,) = model.engine._train_keep[1]
        assert m.dtype == torch.uint8 and tuple(m.shape) == (N, H) and m.is_cuda
        return m.clone()

    torch.manual_seed(123)
    a, b = draw(), draw()
    for m in (a, b):
        assert abs(float(m.float().mean()) - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / (N * H))
    assert not torch.equal(a, b)
    torch.manual_seed(123)
    assert torch.equal(draw(), a)
    # an injected mask is used once, then drawing resumes
    model.set_dropout_masks([torch.ones(N, H)])
    assert bool(draw().all()) and not bool(draw().all())


def test_memory_grows_with_the_tape_not_with_per_sample_gradients():
    model = _midsize_model("gcn", 2, False, None)
    N, M = model.num_nodes, 2000
    gen = torch.Generator().manual_seed(4)
    idx = torch.randperm(N, generator=gen)[:M].cuda()
    y = torch.randint(0, model.out_channels, (M,), generator=gen).cuda()
    model.eval()(idx)
    warm = model.engine.device_bytes()
    F_.cross_entropy(model.train()(idx), y).backward()
    grown = model.engine.device_bytes() - warm
    n_params = sum(p.numel() for p in model.parameters())
    print(f"device bytes: +{grown} for the training step; M * P * 4 = {M * n_params * 4}")
    assert 0 < grown < M * n_params * 4


def test_ste_loop_with_training_steps():
    """One epoch of the driver's loop on lg.STEGCN (gnn/marglik_training.py:159-224): training steps, then fit,
    neg_marglik.backward(), adj step, re-binarise, refit."""
    import laplace_gnn_amd as lg

    g = np.load(os.path.join(GOLDEN, "steloop_kron_sym.npz"))
    X, ei = torch.from_numpy(g["X"]), torch.from_numpy(g["edge_index"])
    init = torch.from_numpy(g["adj_init"]) > 0.5
    train_idx, train_y = torch.from_numpy(g["train_idx"]).cuda(), torch.from_numpy(g["train_y"]).cuda()
    torch.manual_seed(0)
    model = lg.STEGCN(X.shape[1], int(g["W0"].shape[0]), int(g["W1"].shape[0]), 2, X, ei, threshold=float(g["threshold"]),
                      symmetric=bool(g["symmetric"]), candidates=(~init).nonzero().t().contiguous()).cuda()
    assert model.dropout.p == 0.5  # the constructor default
    optimizer = torch.optim.Adam([v for k, v in model.named_parameters() if "adj" not in k], lr=0.01, weight_decay=5e-4)
    adj_optimizer = torch.optim.SGD([model.adj], lr=float(g["lr_adj"]))
    loader = lg.TensorBatchLoader(train_idx, train_y, batch_size=int(g["batch_size"]))
    before = [p.detach().clone() for k, p in model.named_parameters() if "adj" not in k]
    model.train()
    for idx, y in loader:
        f = model(idx)
        optimizer.zero_grad()
        loss = torch.nn.CrossEntropyLoss()(f, y)
        loss.backward()
        optimizer.step()
        assert model.adj.grad is None and math.isfinite(loss.item())
    assert all(not torch.equal(a, p) for a, (k, p) in zip(before, [kp for kp in model.named_parameters() if "adj" not in kp[0]]))
    la = lg.KronLaplace(model, "classification", prior_precision=float(g["prior"]))
    la.fit(loader)
    adj_optimizer.zero_grad()
    value = model.adj_backward(la, loader)
    assert math.isfinite(float(value)) and model.adj.grad is not None and bool(torch.isfinite(model.adj.grad).all())
    adj_optimizer.step()
    model.apply_adj()
    la.fit(loader)
    assert math.isfinite(float(la.log_marginal_likelihood()))
    model.train()
    f = model(train_idx)  # and the next epoch's training step runs on the edited graph
    F_.cross_entropy(f, train_y).backward()
    model.engine.check_async_errors()


def test_lora_stegcn_training_step_and_structure_step():
    """The five training lines on lg.LoRASTEGCN (constructor defaults), then the LoRA structure step and the next training
    step on the re-thresholded graph; adj / adj_lora_* never receive a gradient from the training step."""
    import laplace_gnn_amd as lg

    gen = torch.Generator().manual_seed(9)
    N, F, H, C = 96, 10, 8, 3
    X = torch.randn(N, F, generator=gen)
    ei = torch.randint(0, N, (2, 260), generator=gen)
    idx = torch.randperm(N, generator=gen)[:40].cuda()
    y = torch.randint(0, C, (40,), generator=gen).cuda()
    torch.manual_seed(9)
    model = lg.LoRASTEGCN(F, H, C, 2, X, ei, r=4, lora_alpha=16.0, symmetric=True).cuda()
    assert model.dropout.p == 0.5
    optimizer = torch.optim.Adam([v for k, v in model.named_parameters() if "adj" not in k], lr=0.01, weight_decay=5e-4)
    adj_opt = torch.optim.SGD([model.adj_lora_A, model.adj_lora_B], lr=0.05, weight_decay=1e-3)
    loader = lg.TensorBatchLoader(idx, y, batch_size=16)

    def train_epoch():
        model.train()
        for bi, by in loader:
            before = model.convs[0].lin.weight.detach().clone()
            f = model(bi)
            optimizer.zero_grad()
            loss = torch.nn.CrossEntropyLoss()(f, by)
            loss.backward()
            optimizer.step()
            assert math.isfinite(loss.item()) and not torch.equal(before, model.convs[0].lin.weight)
            assert all(p.grad is not None for k, p in model.named_parameters() if "adj" not in k)

    train_epoch()
    assert model.adj.grad is None and model.adj_lora_A.grad is None and model.adj_lora_B.grad is None
    la = lg.KronLaplace(model, "classification", prior_precision=1.0)
    la.fit(loader)
    adj_opt.zero_grad()
    value = model.adj_backward(la, loader)
    assert math.isfinite(float(value)) and model.adj_lora_A.grad is not None
    adj_opt.step()
    model.apply_adj()
    train_epoch()  # on the re-thresholded graph
    la.fit(loader)
    assert math.isfinite(float(la.log_marginal_likelihood()))
    model.engine.check_async_errors()


def test_sampled_graphsage_trains_on_its_seeded_subgraph():
    """GraphSAGE with the seeded neighbour sample: the training step's gradients equal those of a model built on the sampled
    edge list (same masks), bit for bit -- the sample only changes the graph."""
    import laplace_gnn_amd as lg

    ei, X, Ws, bs = _make("sage", 800, 24, 16, 5, 6000, L=2, seed=4, skew=True)
    gen = torch.Generator().manual_seed(4)
    idx = torch.randperm(800, generator=gen)[:300].cuda()
    y = torch.randint(0, 5, (300,), generator=gen).cuda()
    masks = [(torch.rand(800, 16, generator=gen) >= 0.5).to(torch.uint8).cuda()]
    torch.manual_seed(4)
    sampled = lg.GraphSAGE(24, 16, 5, 2, X, ei, symmetric=True, num_sampled_nodes_per_hop=3, sample_seed=7).cuda()
    direct = lg.GraphSAGE(24, 16, 5, 2, X, sampled.sampled_edge_index(torch.device("cuda")).cpu(), symmetric=False).cuda()
    direct.load_state_dict(sampled.state_dict())
    assert sampled.engine.nnz == direct.engine.nnz < 800 * 3 + 1
    a, b = _grads_once(sampled, idx, y, masks), _grads_once(direct, idx, y, masks)
    assert len(a) == 4
    for k in a:
        assert torch.equal(a[k], b[k]), k
