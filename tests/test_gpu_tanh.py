"""GPU parity of every curvature route under ``act="tanh"`` against the activation-generic fp64 helper
(tests/act_reference.py; pinned to the oracle and the goldens at ReLU by tests/test_act_reference.py, which also shows that
the inputs used here sit in the curved part of tanh).  ReLU's derivative is 0 / 1: a kernel that reads it as a bit mask or as
row sparsity, applies it to the wrong operand, twice, or not at all on one branch is wrong under tanh only -- and a tanh
model is steered onto branches ReLU models of the same shape never take (no path route, the float ``hact`` epilogues, the
no-mask backward GEMM, MODE 0 of the 256-wide fused kernel on GraphSAGE's compact planes).

Bar: relative Frobenius error <= 1e-4 per block and for the loss (BASELINE.json north_star; RTOL of the GPU suites), always
against the fp64 helper, never against another HIP route.  Every case prints what it measured."""
import numpy as np
import pytest
import torch

from act_reference import ActReference
from gpu_utils import kfac_fit_engine, rel

pytestmark = pytest.mark.gpu
RTOL = 1e-4

# The weights of test_gpu_scale._make (variance 1 / fan-in) leave a GCN's second hidden layer in the linear part of tanh (the
# propagation averages ~9 rows); these gains put at least half of every hidden layer at |h| in [0.1, 0.9]
# (tests/test_act_reference.py::test_gpu_test_inputs_sit_in_the_curved_part_of_tanh).
GAIN = {"gcn": 2.5, "sage": 1.0}

KFAC_CASES = [
    ("gcn", 256, 47, 2),   # backward GEMM without mask bits (hact), odd K
    ("gcn", 256, 12, 3),   # store path, hidden -> hidden GEMM epilogue, K = 256
    ("gcn", 128, 9, 2),
    ("gcn", 96, 5, 2),
    ("gcn", 30, 4, 2),     # unfused SpMM + Gram
    ("gcn", 200, 70, 2),   # K > 64: generic GEMM epilogue
    ("gcn", 320, 8, 2),    # width > 256: unfused
    ("sage", 256, 10, 2),  # fused256 MODE 0 + self plane + hact on the compact planes
    ("sage", 256, 40, 2),
    ("sage", 192, 9, 3),
    ("sage", 64, 33, 3),
    ("sage", 30, 4, 2),    # width % 4 != 0: unfused, SpMM with hact (GraphSAGE's hact_ld = 2 H = 60 is still a multiple of 4)
    ("sage", 33, 4, 2),    # the same with hact_ld = 66, % 4 != 0: act' rows start unaligned
]
HUB_CASES = [("gcn", 256, 2), ("sage", 256, 2), ("sage", 132, 3)]
PLANE_CASES = ["sage", "gcn"]
RESNORM_CASES = [("gcn", 2, "layer"), ("sage", 2, "layer"), ("gcn", 3, "layer"), ("sage", 3, "layer"), ("gcn", 2, "batch")]
FRONT_SHAPE = (600, 24, 32, 5, 2400)  # N, F, H, C, E
JAC_CASES = [("gcn", 2, False), ("sage", 2, False), ("gcn", 3, False), ("sage", 3, False), ("gcn", 2, True)]  # kind, L, res + LayerNorm
JAC_SHAPE = dict(F=20, H=32, C=5, N=600, E=2400)
# kind, F, H, L and the first-layer kernel lgnn_diag_accumulate picks (csrc/diag.hip): GraphSAGE takes the register-staged
# kernel; a GCN the owned-tile kernel when ncb = cdiv(F + 1, 192) >= 4 (kTileCols = 192, so F >= 576) and H % 4 == 0, else the
# MFMA kernel with gx = cdiv(F + 1, 256) column blocks; three layers go through the Jacobians.  The engine has no query
# for this choice: first_layer_kernel() below restates the arithmetic and each case asserts the kernel it is here for.
DIAG_CASES = [
    ("gcn", 40, 64, 2, "mfma"),     # ncb = 1, gx = 1
    ("gcn", 600, 64, 2, "tile"),    # ncb = cdiv(601, 192) = 4: act' staged by LDS-DMA, fixed-order tile reduction
    ("gcn", 600, 30, 2, "mfma"),    # ncb = 4 but H % 4 != 0: falls back to the MFMA kernel, gx = 3
    ("sage", 40, 64, 2, "staged"),
    ("sage", 70, 33, 2, "staged"),
    ("gcn", 40, 64, 3, "jacobians"),
]
DIAG_SHAPE = dict(C=4, N=800, E=3000)


def first_layer_kernel(kind, F, H, L):
    if L != 2:
        return "jacobians"
    if kind == "sage":
        return "staged"
    return "tile" if -(-(F + 1) // 192) >= 4 and H % 4 == 0 else "mfma"


def tanh_inputs(kind, N, F, H, C, E, L=2, seed=0, skew=False):
    from test_gpu_scale import _make

    ei, X, Ws, bs = _make(kind, N, F, H, C, E, L=L, seed=seed, skew=skew)
    return ei, X, [GAIN[kind] * w for w in Ws], bs


def hub_inputs(kind, H, L):
    """The graph of test_gpu_scale.test_long_rows_take_the_side_kernel_vs_oracle: hubs of 2 600 / 1 100 / 300 / 90 / 65."""
    N, F, C, E = 5000, 32, 6, 20000
    ei, X, Ws, bs = tanh_inputs(kind, N, F, H, C, E, L=L, seed=41)
    g = torch.Generator().manual_seed(2)
    hubs = []
    for hub, deg in ((7, 2600), (1234, 1100), (4999, 300), (42, 90), (3000, 65)):
        nb = torch.randperm(N, generator=g)[:deg]
        hubs.append(torch.stack([torch.full((deg,), hub), nb]))
    ei = torch.cat([ei] + hubs, dim=1)
    idx = torch.randperm(N, generator=g)[:600]
    y = torch.randint(0, C, (600,), generator=g)
    return ei, X, Ws, bs, idx, y


def resnorm_extras(H, L, norm, F):
    from test_gpu_resnorm import _extras

    return _extras(H, L, norm, True, [F] + [H] * (L - 2), 81)


def _engine(kind, N, ei, X, Ws, bs, act="tanh", symmetric=True, likelihood="classification", **kw):
    import laplace_gnn_amd as lg

    eng = lg.GraphEngine(ei.cuda(), N, kind=kind, symmetric=symmetric)
    dev = {k: ([t.cuda() for t in v] if isinstance(v, list) else v) for k, v in kw.items()}
    eng.bind(X.cuda(), [w.cuda() for w in Ws], [b.cuda() for b in bs], act=act, likelihood=likelihood, **dev)
    return eng


def _ref(eng, kind, X, Ws, bs, act="tanh", likelihood="classification", **kw):
    """The fp64 helper on the device, over the engine's exported propagation matrix (bit exact, tests/test_gpu_parity.py)."""
    return ActReference(kind, eng.export_propagation(), X, Ws, bs, act=act, likelihood=likelihood, device="cuda", **kw)


def _batch(N, M, C, seed, dup=0, regression=False):
    """M node ids and labels; ``dup``: ids 0 .. dup-1 are listed again at dup .. 2 dup - 1, i.e. twice inside the FIRST batch
    of any batch size >= 2 dup (a repeated id must accumulate within one accumulate call, not across two)."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randperm(N, generator=g)[:M]
    if dup:
        idx[dup:2 * dup] = idx[:dup]
    y = torch.randn(M, C, generator=g) if regression else torch.randint(0, C, (M,), generator=g)
    return idx, y


def _np(t):
    return t.detach().cpu().numpy()


class _Errors:
    """Collects (name, measured error), prints them all, then asserts the bar -- so a failing run still shows every figure."""

    def __init__(self, what):
        self.what, self.items = what, []

    def add(self, name, got, want):
        self.items.append((name, rel(_np(got), _np(want))))

    def scalar(self, name, got, want):
        self.items.append((name, abs(float(got) - float(want)) / max(abs(float(want)), 1e-30)))

    def check(self, tol=RTOL):
        print(f"{self.what}: " + "  ".join(f"{k} {e:.2e}" for k, e in self.items))
        bad = [(k, e) for k, e in self.items if not e <= tol]
        assert not bad, (self.what, bad)


def _compare_kfac(err, views, loss, ref_loss, kf):
    assert len(views) == len(kf) // 2
    for k, (A, B) in enumerate(views):
        err.add(f"B_{k}", B, kf[2 * k][0])
        err.add(f"A_{k}", A, kf[2 * k][1])
    err.scalar("loss", loss, ref_loss)


# ---- KFAC ---------------------------------------------------------------------------------------------------------------
def _expected_route(plan, kind, H, C, L, act):
    """What the plan must say for the case to reach the branch it is in the table for."""
    assert not plan["paths"] or act == "relu", plan  # tanh never takes the two-hop path route
    fused = H % 4 == 0 and H <= 256  # otherwise SpMM + Gram through HBM on every level
    assert plan["fused"][1:] == [fused] * (L - 1), plan
    assert plan["backgemm"][L - 1] == (fused and C <= 64), plan  # K > 64 takes the generic GEMM and its epilogue
    assert plan["sage_compact"] == (kind == "sage" and fused), plan


@pytest.mark.parametrize("kind,H,C,L,act", [c + ("tanh",) for c in KFAC_CASES] + [("gcn", 320, 8, 2, "relu")])
def test_kfac_kernel_variants_vs_fp64(kind, H, C, L, act):
    N, F, E = 1200, 40, 5000
    ei, X, Ws, bs = tanh_inputs(kind, N, F, H, C, E, L=L, seed=21)
    idx, y = _batch(N, 260, C, 3, dup=4)
    eng = _engine(kind, N, ei, X, Ws, bs, act=act)
    eng.set_workspace_limit(64 << 20)  # as test_kfac_kernel_variants_vs_oracle: the larger heads go in several class chunks
    _expected_route(eng.kfac_plan(), kind, H, C, L, act)
    views, loss = kfac_fit_engine(eng, idx.cuda(), y.cuda(), 130)
    assert not eng.last_kfac_used_paths
    rl, kf = _ref(eng, kind, X, Ws, bs, act=act).kfac_fit(idx, y, 130)
    err = _Errors(f"kfac {kind} H={H} C={C} L={L} {act}")
    _compare_kfac(err, views, loss, rl, kf)
    err.check()
    eng.check_async_errors()
    eng.close()


@pytest.mark.parametrize("kind", ["gcn", "sage"])
def test_the_bar_tells_a_relu_kernel_from_the_tanh_reference(kind):
    """The other direction: the same weights bound with ReLU miss the tanh helper by far more than the bar, on the first
    layer's B (through act') and on the last layer's A (through the activations) -- so these inputs cannot pass by accident."""
    N, F, H, C, E = 1200, 40, 96, 5, 5000
    ei, X, Ws, bs = tanh_inputs(kind, N, F, H, C, E, seed=21)
    idx, y = _batch(N, 260, C, 3)
    eng = _engine(kind, N, ei, X, Ws, bs, act="relu")
    views, _ = kfac_fit_engine(eng, idx.cuda(), y.cuda(), 130)
    _, kf = _ref(eng, kind, X, Ws, bs, act="tanh").kfac_fit(idx, y, 130)
    eB, eA = rel(_np(views[0][1]), _np(kf[0][0])), rel(_np(views[1][0]), _np(kf[2][1]))
    print(f"relu kernel vs tanh reference, {kind}: B_0 {eB:.2e}  A_1 {eA:.2e}")
    assert eB > 1e-2 and eA > 1e-2
    eng.check_async_errors()
    eng.close()


@pytest.mark.parametrize("kind,H,C,L", [("gcn", 256, 47, 2), ("sage", 256, 10, 2)])
def test_kfac_unfused_vs_fp64(kind, H, C, L):
    N, F, E = 1200, 40, 5000
    ei, X, Ws, bs = tanh_inputs(kind, N, F, H, C, E, L=L, seed=21)
    idx, y = _batch(N, 260, C, 3, dup=4)
    eng = _engine(kind, N, ei, X, Ws, bs)
    eng.set_workspace_limit(64 << 20)
    assert not any(eng.kfac_plan(fuse=False)["fused"]), eng.kfac_plan(fuse=False)
    for fork in (True, False):
        views, loss = kfac_fit_engine(eng, idx.cuda(), y.cuda(), 130, fork_exact=fork, fuse=False)
        assert not eng.last_kfac_used_paths
        rl, kf = _ref(eng, kind, X, Ws, bs).kfac_fit(idx, y, 130, fork_exact=fork)
        err = _Errors(f"kfac unfused {kind} H={H} fork_exact={fork}")
        _compare_kfac(err, views, loss, rl, kf)
        err.check()
    eng.check_async_errors()
    eng.close()


def test_kfac_class_range_shares_repeated_ids_directed_graph_vs_fp64():
    kind, H, C, L, N, F, E = "gcn", 256, 47, 2, 1200, 40, 5000
    ei, X, Ws, bs = tanh_inputs(kind, N, F, H, C, E, L=L, seed=21)
    idx, y = _batch(N, 260, C, 3, dup=30)
    assert len(set(idx[:130].tolist())) == 100  # 30 ids twice inside the first batch of 130
    eng = _engine(kind, N, ei, X, Ws, bs, symmetric=False)
    eng.set_workspace_limit(64 << 20)
    assert not eng.is_symmetric and not eng.kfac_plan()["paths"]
    _, views, loss = eng.new_kfac_buffers()
    cut = 13
    for s in range(0, 260, 130):
        for cr in ((0, cut), (cut, C)):
            eng.kfac_accumulate(idx[s:s + 130].cuda(), y[s:s + 130].cuda(), 260, views, loss, classes=cr)
            assert not eng.last_kfac_used_paths
    torch.cuda.synchronize()
    rl, kf = _ref(eng, kind, X, Ws, bs).kfac_fit(idx, y, 130, shares=[(0, cut), (cut, C)])
    err = _Errors("kfac class-range shares, directed")
    _compare_kfac(err, views, float(loss), rl, kf)
    err.check()
    eng.check_async_errors()
    eng.close()


@pytest.mark.parametrize("kind,H,L", HUB_CASES)
def test_kfac_hub_rows_take_the_side_kernel_vs_fp64(kind, H, L):
    N, C = 5000, 6
    ei, X, Ws, bs, idx, y = hub_inputs(kind, H, L)
    eng = _engine(kind, N, ei, X, Ws, bs)
    eng.set_workspace_limit(96 << 20)
    plan = eng.kfac_plan()
    assert not plan["paths"] and plan["fused"][L - 1], plan
    views, loss = kfac_fit_engine(eng, idx.cuda(), y.cuda(), 250)  # 250 / 250 / 100
    assert not eng.last_kfac_used_paths
    assert eng.num_long_rows >= 5, eng.num_long_rows
    rl, kf = _ref(eng, kind, X, Ws, bs).kfac_fit(idx, y, 250)
    err = _Errors(f"kfac hubs {kind} H={H} L={L}")
    _compare_kfac(err, views, loss, rl, kf)
    err.check()
    eng.check_async_errors()
    eng.close()


@pytest.mark.parametrize("kind", PLANE_CASES)
def test_kfac_large_plane_path_vs_fp64(kind, monkeypatch):
    monkeypatch.setenv("LGNN_PLANE_LIMIT", "1000000")
    N, F, H, C, E, L = 3000, 20, 256, 5, 9000, 3
    ei, X, Ws, bs = tanh_inputs(kind, N, F, H, C, E, L=L, seed=77)
    idx, y = _batch(N, 300, C, 9, dup=20)
    eng = _engine(kind, N, ei, X, Ws, bs)
    plan = eng.kfac_plan()
    assert not plan["paths"] and not any(plan["fused"][1:]), plan  # the backward steps left the fused path
    views, loss = kfac_fit_engine(eng, idx.cuda(), y.cuda(), 128)  # 128 / 128 / 44
    assert not eng.last_kfac_used_paths
    rl, kf = _ref(eng, kind, X, Ws, bs).kfac_fit(idx, y, 128)
    err = _Errors(f"kfac large planes {kind}")
    _compare_kfac(err, views, loss, rl, kf)
    err.check()
    eng.check_async_errors()
    eng.close()


@pytest.mark.parametrize("kind,L,norm", RESNORM_CASES)
def test_kfac_with_res_and_norm_vs_fp64(kind, L, norm):
    """The tanh branch of csrc/resnorm.hip, forward and backward, the B factors of the res.* blocks included."""
    N, F, H, C, E = 1200, 40, 64, 6, 5000
    ei, X, Ws, bs = tanh_inputs(kind, N, F, H, C, E, L=L, seed=31)
    kw = resnorm_extras(H, L, norm, F)
    idx, y = _batch(N, 260, C, 5, dup=3)
    eng = _engine(kind, N, ei, X, Ws, bs, **kw)
    plan = eng.kfac_plan()
    assert not plan["paths"] and not any(plan["fused"]), plan  # res / norm models take the unfused route
    views, loss = kfac_fit_engine(eng, idx.cuda(), y.cuda(), 130)
    assert not eng.last_kfac_used_paths and len(views) == 2 * L - 1
    ref = _ref(eng, kind, X, Ws, bs, **kw)
    err = _Errors(f"kfac res+{norm} {kind} L={L}")
    err.add("logits", eng.forward_all(), ref.forward()["out"])
    rl, kf = ref.kfac_fit(idx, y, 130)
    _compare_kfac(err, views, loss, rl, kf)
    err.check()
    eng.check_async_errors()
    eng.close()


# ---- the Jacobian family at small shapes: one reference per case, shared ------------------------------------------------------
def _small(kind, L, resnorm=False, F=20, H=32, C=5, N=600, E=2400, M=40, likelihood="classification"):  # (JAC_SHAPE)
    """Inputs, batch, the fp64 helper and its Jacobians of one small case."""
    ei, X, Ws, bs = tanh_inputs(kind, N, F, H, C, E, L=L, seed=23)
    kw = resnorm_extras(H, L, "layer", F) if resnorm else {}
    idx, y = _batch(N, M, C, 9, dup=2, regression=likelihood == "regression")
    eng = _engine(kind, N, ei, X, Ws, bs, likelihood=likelihood, **kw)
    ref = _ref(eng, kind, X, Ws, bs, likelihood=likelihood, **kw)
    eng.close()
    return (kind, N, ei, X, Ws, bs), kw, idx, y, ref, ref.jacobians(idx)


@pytest.fixture(scope="module")
def small():
    """``_small`` computed once per case and shared by the tests of this module (never modified); the device tensors go
    when the module is done."""
    cache = {}

    def get(*args, **kw):
        key = (args, tuple(sorted(kw.items())))
        if key not in cache:
            cache[key] = _small(*args, **kw)
        return cache[key]

    yield get
    cache.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("kind,L,resnorm", JAC_CASES)
def test_jacobians_vs_fp64(kind, L, resnorm, small, monkeypatch):
    """The closed form (what ``lgnn_jacobians`` serves models of <= 2 layers with) and the plane route (what deeper models
    always take; ``LGNN_JAC_PLANES=1`` sends the 2-layer models there as well)."""
    args, kw, idx, y, ref, (J, f) = small(kind, L, resnorm)
    eng = _engine(*args, **kw)
    err = _Errors(f"jacobians {kind} L={L} resnorm={resnorm}")
    Js, fs = eng.jacobians(idx.cuda())
    err.add("J", Js, J)
    err.add("f", fs, f)
    if L == 2:
        monkeypatch.setenv("LGNN_JAC_PLANES", "1")
        err.add("J(planes)", eng.jacobians(idx.cuda())[0], J)
        monkeypatch.delenv("LGNN_JAC_PLANES")
    err.check()
    eng.check_async_errors()
    eng.close()


def _diag(eng, idx, y):
    Hd = torch.zeros(eng.n_params, device="cuda")
    loss = torch.zeros(1, device="cuda")
    eng.diag_accumulate(idx.cuda(), y.cuda(), Hd, loss)
    torch.cuda.synchronize()
    return Hd, float(loss)


@pytest.mark.parametrize("kind,F,H,L,kernel", DIAG_CASES)
def test_diag_ggn_vs_fp64(kind, F, H, L, kernel, small, monkeypatch):
    """``dact0`` through every first-layer kernel of csrc/diag.hip (and, for the GCN, the register-staged one by switch)."""
    assert first_layer_kernel(kind, F, H, L) == kernel
    args, kw, idx, y, ref, J = small(kind, L, False, F=F, H=H, M=40, **DIAG_SHAPE)
    eng = _engine(*args)
    rl, rH = ref.ggn(idx, y, J=J)
    err = _Errors(f"diag {kind} F={F} H={H} L={L}")
    Hd, loss = _diag(eng, idx, y)
    err.add("H", Hd, rH)
    err.scalar("loss", loss, rl)
    if kind == "gcn" and L == 2:
        monkeypatch.setenv("LGNN_DIAG_STAGED", "1")
        err.add("H(staged)", _diag(eng, idx, y)[0], rH)
        monkeypatch.delenv("LGNN_DIAG_STAGED")
    err.check()
    eng.check_async_errors()
    eng.close()


@pytest.mark.parametrize("kind", ["gcn", "sage"])
def test_full_lastlayer_ef_and_fisher_accumulators_vs_fp64(kind, small):
    args, kw, idx, y, ref, J = small(kind, 2, False)
    eng = _engine(*args)
    P = eng.n_params
    M = len(idx)
    di, dy = idx.cuda(), y.cuda()
    err = _Errors(f"accumulators {kind}")
    Hf, loss = torch.zeros(P, P, device="cuda"), torch.zeros(1, device="cuda")
    eng.full_accumulate(di, dy, Hf, loss)
    rl, rH = ref.ggn(idx, y, True, J)
    err.add("full", Hf, rH)
    err.scalar("full loss", loss, rl)
    sl = ref.lastlayer_slice()
    p_ll = sl.stop - sl.start
    Hl, loss = torch.zeros(p_ll, p_ll, device="cuda"), torch.zeros(1, device="cuda")
    eng.lastlayer_full_accumulate(di, dy, Hl, loss)
    err.add("last layer", Hl, ref.lastlayer_full(idx, y, J)[1])
    err.scalar("last-layer loss", loss, rl)
    d1, F1, loss = torch.zeros(P, device="cuda"), torch.zeros(P, P, device="cuda"), torch.zeros(1, device="cuda")
    eng.ef_accumulate(di, dy, resid_scale=0.7, scale=0.25, diag=d1)
    G = eng.ef_accumulate(di, dy, dy, resid_scale=0.7, scale=0.25, full=F1, grads=True, loss=loss)
    _, rd, rG = ref.ef(idx, y, False, J, resid_scale=0.7, scale=0.25)
    err.add("EF diag", d1, rd)
    err.add("EF full", F1, ref.ef(idx, y, True, J, resid_scale=0.7, scale=0.25)[1])
    err.add("EF grads", G, rG)
    err.scalar("EF loss", loss, rl)
    draws = [torch.randint(0, eng.dims[-1], (M,), generator=torch.Generator().manual_seed(40 + s)) for s in range(3)]
    for labels in (None, draws):
        _, views, loss = eng.new_kfac_buffers()
        seeds = [y] if labels is None else labels
        for s_, ys in enumerate(seeds):
            eng.kfac_accumulate_fisher(di, ys.cuda(), dy if s_ == 0 else None, M, views, loss, b_scale=1.0 / len(seeds))
        torch.cuda.synchronize()
        fl, kf = ref.kfac_fisher_batch(idx, y, M, mc_labels=labels)
        tag = "EF-KFAC" if labels is None else "MC-KFAC"
        for k, (A, B) in enumerate(views):
            err.add(f"{tag} B_{k}", B, kf[2 * k][0])
            err.add(f"{tag} A_{k}", A, kf[2 * k][1])
        err.scalar(f"{tag} loss", loss, fl)
    err.check()
    eng.check_async_errors()
    eng.close()


# ---- front end ----------------------------------------------------------------------------------------------------------------
def _model(kind, L=2, likelihood="classification", cls=None, C=None, H=None, **ctor):
    import laplace_gnn_amd as lg

    N, F, H0, C0, E = FRONT_SHAPE
    H, C = H or H0, C or C0
    ei, X, Ws, bs = tanh_inputs(kind, N, F, H, C, E, L=L, seed=61)
    cls = cls or (lg.GCN if kind == "gcn" else lg.GraphSAGE)
    torch.manual_seed(5)
    model = cls(F, H, C, L, X, ei, act="tanh", symmetric=True, **ctor)
    with torch.no_grad():
        for l, conv in enumerate(model.convs):
            conv.lin.weight.copy_(Ws[l])
            conv.lin.bias.copy_(bs[l])
    model = model.eval().cuda()
    idx, y = _batch(N, 60, C, 7, dup=2, regression=likelihood == "regression")
    ref = _ref(model.engine, kind, X, Ws, bs, likelihood=likelihood)
    return model, ref, idx, y


def _release(model):
    model.engine.check_async_errors()
    model.engine.close()


def _loader(idx, y, bs=25):
    import laplace_gnn_amd as lg

    return lg.TensorBatchLoader(idx.cuda(), y.cuda(), batch_size=bs)


def _probit(f_mu, f_var_diag):
    return torch.softmax(f_mu / torch.sqrt(1.0 + (np.pi / 8.0) * f_var_diag), dim=-1)


def _kron_covariance(kf, prior):
    """Dense posterior covariance [P, P] of Kronecker factors [[B, A], [B]] ... : weight blocks kron(B, A) (row-major
    weights), bias blocks B, plus the prior precision, inverted per block in fp64."""
    blocks = []
    for Fs in kf:
        Hb = torch.kron(Fs[0], Fs[1]) if len(Fs) == 2 else Fs[0]
        blocks.append(torch.linalg.inv(Hb + prior * torch.eye(len(Hb), dtype=Hb.dtype, device=Hb.device)))
    return torch.block_diag(*blocks)


@pytest.mark.parametrize("kind", ["gcn", "sage"])
def test_laplace_front_end_vs_fp64(kind):
    """kron / diag / full fits of a tanh model and the probit predictive against the helper's factors and its J Sigma J^T."""
    import laplace_gnn_amd as lg

    model, ref, idx, y = _model(kind)
    assert model.engine._bind_opts[0] == "tanh"
    loader = _loader(idx, y)
    x = torch.arange(0, 600, 61)  # 10 evaluation nodes
    J, f = ref.jacobians(x)
    Jt = ref.jacobians(idx)
    err = _Errors(f"front end {kind}")
    for s in ("kron", "diag", "full"):
        la = lg.Laplace(model, "classification", "all", s)
        la.fit(loader)
        if s == "kron":
            rl, kf = ref.kfac_fit(idx, y, 25)
            for i, Fs in enumerate(la.H_facs.kfacs):
                for j, Hm in enumerate(Fs):
                    err.add(f"kron_{i}_{j}", Hm, kf[i][j])
            Sigma = _kron_covariance(kf, 1.0)
            assert not model.engine.last_kfac_used_paths
            assert la._glm_variance_matrix_free(x.cuda()) is None  # 2-layer tanh: the Jacobian route
        else:
            rl, rH = ref.ggn(idx, y, s == "full", Jt)
            err.add(s, la.H, rH)
            Sigma = 1.0 / (rH + 1.0) if s == "diag" else torch.linalg.inv(rH + torch.eye(len(rH), dtype=rH.dtype, device="cuda"))
        err.scalar(f"{s} loss", la.loss, rl)
        fvar = torch.diagonal(ref.functional_variance(J, Sigma), dim1=1, dim2=2)
        err.add(f"{s} probit", la(x.cuda(), link_approx="probit"), _probit(f, fvar))
    err.check()
    _release(model)


def test_one_layer_tanh_model_keeps_the_matrix_free_predictive():
    import laplace_gnn_amd as lg

    model, ref, idx, y = _model("gcn", L=1)
    la = lg.KronLaplace(model, "classification")
    la.fit(_loader(idx, y))
    assert la._glm_variance_matrix_free(torch.arange(10).cuda()) is not None  # no hidden layer: the activation never runs
    _release(model)


def test_regression_with_tanh_on_a_graph_with_edges_vs_fp64():
    import laplace_gnn_amd as lg

    model, ref, idx, y = _model("gcn", likelihood="regression", C=3, H=64)
    assert model.engine.nnz > model.engine.num_nodes
    loader = _loader(idx, y)
    err = _Errors("regression gcn H=64 C=3")
    la = lg.Laplace(model, "regression", "all", "kron")
    la.fit(loader)
    assert not model.engine.last_kfac_used_paths
    rl, kf = ref.kfac_fit(idx, y, 25)
    for i, Fs in enumerate(la.H_facs.kfacs):
        for j, Hm in enumerate(Fs):
            err.add(f"kron_{i}_{j}", Hm, kf[i][j])
    err.scalar("kron loss", la.loss, rl)
    ld = lg.Laplace(model, "regression", "all", "diag")
    ld.fit(loader)
    rl, rH = ref.ggn(idx, y)
    err.add("diag", ld.H, rH)
    err.scalar("diag loss", ld.loss, rl)
    err.check()
    _release(model)


def test_diag_fit_graph_equals_the_ordinary_fit_under_tanh():
    import laplace_gnn_amd as lg

    model, ref, idx, y = _model("gcn")
    loader = _loader(idx, y)
    plain = lg.DiagLaplace(model, "classification")
    plain.fit(loader)
    la = lg.DiagLaplace(model, "classification")
    la.fit_graph = True
    for k in range(3):  # ordinary, capture + replay, replay
        la.fit(loader)
        e = rel(_np(la.H), _np(plain.H))
        print(f"fit_graph pass {k}: {e:.2e}")
        assert e <= 1e-6 and abs(float(la.loss) - float(plain.loss)) <= 1e-6 * abs(float(plain.loss)), k
    assert la._fit_graph_state["graph"] is not None and not la._fit_graph_state["off"]
    err = _Errors("fit_graph diag vs fp64")
    err.add("H", la.H, ref.ggn(idx, y)[1])
    err.check()
    _release(model)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("structure,dense", [("kron", False), ("diag", False), ("full", False), ("kron", True)])
def test_adjacency_gradient_refuses_tanh(structure, dense):
    import laplace_gnn_amd as lg
    from laplace_gnn_amd._lib import HipLibraryError

    model, _, idx, y = _model("gcn", cls=lg.STEGCN, H=8, C=3)
    loader = _loader(idx, y)
    la = lg.Laplace(model, "classification", "all", structure)
    la.fit(loader)
    with pytest.raises(HipLibraryError, match="ReLU"):
        la.neg_marglik_adj_grad(loader, dense=True) if dense else la.neg_marglik_adj_grad(loader)
    _release(model)


def test_matrix_free_variance_entries_under_tanh():
    """``lgnn_glm_variance_ext`` refuses a tanh model; the plain ``lgnn_glm_variance`` entry, called directly with the operands
    of a fitted Kronecker posterior, is compared with the Jacobian route (the Python front keeps tanh models off it)."""
    import laplace_gnn_amd as lg
    from laplace_gnn_amd._lib import HipLibraryError

    model, _, idx, y = _model("gcn", res=True, norm="layer")
    la = lg.KronLaplace(model, "classification")
    la.fit(_loader(idx, y))
    x = torch.arange(0, 600, 31).cuda()
    ops = la._matrix_free_operands()
    assert ops is not None and "Sr" in ops
    with pytest.raises(HipLibraryError, match="ReLU"):
        model.engine.glm_variance_ext(x, **ops)
    _release(model)

    model, _, idx, y = _model("gcn")
    la = lg.KronLaplace(model, "classification")
    la.fit(_loader(idx, y))
    ops = la._matrix_free_operands()
    assert ops is not None
    Js, f = model.engine.jacobians(x)
    want = torch.diagonal(la.functional_variance(Js), dim1=1, dim2=2)
    f_mu, f_var = model.engine.glm_variance(x, **ops)
    err = _Errors("lgnn_glm_variance under tanh vs the Jacobian route")
    err.add("f_var", f_var, want)
    err.add("f_mu", f_mu, f)
    E = torch.randn(7, la.n_outputs, generator=torch.Generator().manual_seed(1)).cuda()  # lgnn_glm_variance_mapped
    _, v_map = model.engine.glm_variance(x, out_map=E, **la._matrix_free_operands(E))
    err.add("var(E f)", v_map, torch.einsum("rc,mck,rk->mr", E, la.functional_variance(Js), E))
    err.check()
    _release(model)
