"""dev: wall time of the last-layer posteriors at a products-shaped head (3-layer GraphSAGE, H = 256 -> D = 512, C = 47) on a
graph small enough to build quickly (N = 200 000, 4 batches of 10 000).  Medians over repeated, alternated runs; every timed
window ends in a device synchronise.

  fits         KronLLLaplace.fit, DiagLLLaplace.fit and FullLLLaplace.fit on the same model and loader, alternating
  accumulate   lgnn_lastlayer_kron_accumulate / lgnn_lastlayer_diag_accumulate over the loader's batches against the same
               quantities composed from lgnn_lastlayer_features + torch (Phi^T Phi, softmax, the seed blocks and their einsum),
               alternating, with their agreement
  predictive   la(x) on all N nodes (probit), Kronecker last-layer against FullLLLaplace, at a head where the latter is
               affordable (--small-hidden / --small-classes)

  --json PATH  write all records as one JSON document"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import laplace_gnn_amd as lg

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=200_000)
ap.add_argument("--degree", type=int, default=10)
ap.add_argument("--features", type=int, default=100)
ap.add_argument("--hidden", type=int, default=256)
ap.add_argument("--classes", type=int, default=47)
ap.add_argument("--batches", type=int, default=4)
ap.add_argument("--batch", type=int, default=10_000)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--small-hidden", type=int, default=32)
ap.add_argument("--small-classes", type=int, default=10)
ap.add_argument("--skip", default="", help="comma list of fits,accumulate,predictive")
ap.add_argument("--json", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "a timing needs the GPU"
RECORDS = []


def emit(**rec):
    print(json.dumps(rec), flush=True)
    RECORDS.append(rec)


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def make(hidden, classes):
    g = torch.Generator().manual_seed(0)
    N = args.nodes
    ei = torch.randint(0, N, (2, N * args.degree), generator=g)
    X = torch.randn(N, args.features, generator=g)
    torch.manual_seed(0)
    model = lg.GraphSAGE(args.features, hidden, classes, 3, X, ei, symmetric=True).to("cuda").eval()
    M = args.batches * args.batch
    idx = torch.randperm(N, generator=g)[:M].cuda()
    y = torch.randint(0, classes, (M,), generator=g).cuda()
    return model, idx, y, lg.TensorBatchLoader(idx, y, batch_size=args.batch)


def torch_kron(eng, idx, y, n_train, A, B, Bb, loss):
    """The fork-exact factors from the feature rows with library kernels (oracle/gnn_laplace_oracle.py:424-448)."""
    phi, s, f = eng.lastlayer_features(idx)
    A.addmm_(phi.T, phi, alpha=1.0 / n_train)
    p = torch.softmax(f, dim=-1)
    sp = p.sqrt()
    eye = torch.eye(f.shape[1], device=f.device)
    fm = f - (p * f).sum(dim=1, keepdim=True)
    V = sp.unsqueeze(1) * (eye - (p * (1 + fm)).unsqueeze(2) + 0.5 * (eye - p.unsqueeze(2)) * fm.unsqueeze(1))  # [M, k, c]
    B += torch.einsum("nkc,njc->kj", V, V)
    Bb += torch.einsum("n,nkc,njc->kj", s * s, V, V)
    loss += torch.nn.functional.cross_entropy(f, y, reduction="sum")


def torch_diag(eng, idx, y, H, loss):
    phi, s, f = eng.lastlayer_features(idx)
    C, D = f.shape[1], phi.shape[1]
    p = torch.softmax(f, dim=-1)
    lam = p * (1 - p)
    H[:C * D] += (lam.T @ (phi * phi)).reshape(-1)
    H[C * D:] += lam.T @ (s * s)
    loss += torch.nn.functional.cross_entropy(f, y, reduction="sum")


skip = set(args.skip.split(","))
shape = dict(nodes=args.nodes, edges=args.nodes * args.degree, layers=3, kind="sage", batches=args.batches, batch=args.batch)

if "fits" not in skip or "accumulate" not in skip:
    model, idx, y, loader = make(args.hidden, args.classes)
    eng = model.engine
    C, D = args.classes, 2 * args.hidden
    eng.forward_all()
    torch.cuda.synchronize()

if "fits" not in skip:
    las = {"kron": lg.Laplace(model, "classification", "last_layer", "kron"),
           "diag": lg.Laplace(model, "classification", "last_layer", "diag"),
           "full": lg.Laplace(model, "classification", "last_layer", "full")}
    times = {k: [] for k in las}
    for rep in range(args.reps + 1):  # (the first round warms every shape up and is dropped)
        for k, la in las.items():
            _, ms = timed(lambda: la.fit(loader))
            if rep:
                times[k].append(ms)
    for k, ts in times.items():
        emit(what="fit", posterior=k, D=D, C=C, ms_median=statistics.median(ts), ms_min=min(ts), ms_max=max(ts), reps=len(ts),
             **shape)
    # the three posteriors see the same curvature: the Kronecker factors' diagonal blocks against the full matrix
    Hf = las["full"].H
    emit(what="fit_agreement", diag_vs_full=rel(las["diag"].H, torch.diagonal(Hf)),
         kron_loss_vs_full=abs(float(las["kron"].loss) - float(las["full"].loss)) / abs(float(las["full"].loss)))
    del las, Hf
    torch.cuda.empty_cache()

if "accumulate" not in skip:
    n_train = idx.shape[0]
    cuts = [(s0, min(n_train, s0 + args.batch)) for s0 in range(0, n_train, args.batch)]

    def hip_kron():
        _, A, B, Bb, loss = eng.new_lastlayer_kron_buffers()
        for a, b in cuts:
            eng.lastlayer_kron_accumulate(idx[a:b], y[a:b], n_train, A, B, Bb, loss)
        return A, B, Bb, loss

    def lib_kron():
        _, A, B, Bb, loss = eng.new_lastlayer_kron_buffers()
        for a, b in cuts:
            torch_kron(eng, idx[a:b], y[a:b], n_train, A, B, Bb, loss)
        return A, B, Bb, loss

    def hip_diag():
        H, loss = torch.zeros(C * D + C, device="cuda"), torch.zeros(1, device="cuda")
        for a, b in cuts:
            eng.lastlayer_diag_accumulate(idx[a:b], y[a:b], H, loss)
        return H, loss

    def lib_diag():
        H, loss = torch.zeros(C * D + C, device="cuda"), torch.zeros(1, device="cuda")
        for a, b in cuts:
            torch_diag(eng, idx[a:b], y[a:b], H, loss)
        return H, loss

    for name, hip, lib in (("kron", hip_kron, lib_kron), ("diag", hip_diag, lib_diag)):
        t_hip, t_lib = [], []
        for rep in range(args.reps + 1):
            out_h, ms_h = timed(hip)
            out_l, ms_l = timed(lib)
            if rep:
                t_hip.append(ms_h); t_lib.append(ms_l)
        emit(what="accumulate", structure=name, D=D, C=C, hip_ms_median=statistics.median(t_hip), hip_ms_min=min(t_hip),
             hip_ms_max=max(t_hip), torch_ms_median=statistics.median(t_lib), torch_ms_min=min(t_lib), torch_ms_max=max(t_lib),
             reps=len(t_hip), agreement=[rel(a, b) for a, b in zip(out_h, out_l)], **shape)
    eng.check_async_errors()

if "fits" not in skip or "accumulate" not in skip:
    eng.close()
    del model, eng
    torch.cuda.empty_cache()

if "predictive" not in skip:
    model, idx, y, loader = make(args.small_hidden, args.small_classes)
    every = torch.arange(args.nodes, device="cuda")
    las = {"kron": lg.Laplace(model, "classification", "last_layer", "kron"),
           "full": lg.Laplace(model, "classification", "last_layer", "full")}
    outs, times = {}, {k: [] for k in las}
    for la in las.values():
        la.fit(loader)
    for rep in range(4):
        for k, la in las.items():
            outs[k], ms = timed(lambda: la(every, link_approx="probit"))
            if rep:
                times[k].append(ms)
    for k, ts in times.items():
        emit(what="predictive", posterior=k, link="probit", D=2 * args.small_hidden, C=args.small_classes,
             ms_median=statistics.median(ts), ms_min=min(ts), ms_max=max(ts), reps=len(ts), **shape)
    emit(what="predictive_agreement", note="different posteriors: the mean absolute difference of the class probabilities",
         mean_abs_diff=float((outs["kron"] - outs["full"]).abs().mean()))
    # the products-shaped head, Kronecker only (the full posterior would invert a 24 111 x 24 111 matrix per call)
    model.engine.close()
    model, idx, y, loader = make(args.hidden, args.classes)
    la = lg.Laplace(model, "classification", "last_layer", "kron")
    la.fit(loader)
    ts = []
    for rep in range(4):
        _, ms = timed(lambda: la(every, link_approx="probit"))
        if rep:
            ts.append(ms)
    emit(what="predictive", posterior="kron", link="probit", D=2 * args.hidden, C=args.classes, ms_median=statistics.median(ts),
         ms_min=min(ts), ms_max=max(ts), reps=len(ts), **shape)

if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(dict(tool="tools/time_lastlayer_fit.py", device=torch.cuda.get_device_name(0), records=RECORDS), f, indent=1)
