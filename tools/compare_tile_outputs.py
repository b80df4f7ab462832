"""dev: what the kernels on the shared fp32 MFMA tile steps (csrc/mfma_tile.h) return, from two builds of the
library, compared.

  python tools/compare_tile_outputs.py --parent lib_parent [--branch lib] [--procs 2] [--runs 3] [--json PATH]

Each build (a directory beside the package's lib/, see LGNN_LIB_DIR in _lib.py) is driven in ``--procs`` fresh child processes
of ``--runs`` runs each, parent and branch alternating, every child under its own time limit; the script stops at the first
child that does not exit with 0.  (More than one process a side: an accumulation behind float atomics can repeat its bits
inside one process and still differ from the next one, so a spread taken in one process can be 0 where the parent's is not.)
Both sides build the same seeded inputs -- the small builders of the tests -- and the posterior weightings of the dense
adjacency gradient are computed once (by the first child) and reused.  Cases:

  sampled/*      sampled_forward on gcn-2, sage-2, gcn-1 at SMALL and the two-window, two-row-tile GraphSAGE case
  ggn/*          jvp_block and ggn_matmat_ on the structured route and over Jacobian rows, k = 5 and 33, at SHAPES[0] and WIDE
  gp/*           gp_kernel on the structured route at SHAPES[0]
  knn/*          lg.knn at the small shapes and the first fast-path shape of tests/test_gpu_knn.py
  dense/*        adjgrad_batch_dense / diag_adjgrad_batch_dense on the smallest plain-GCN fixture
  full/*         full_directions on the small GCN fixture
  plain/*        forward and the Kronecker factors of a fit without the path route (gemm_kernel)

Arrays with no float atomic behind them must be bit-equal over all runs of both sides.  `full/Kn`, `plain/*` (float atomics:
K_n, split-K, the factors) must differ from the parent by no more than twice the parent's own run-to-run spread
(max |a - b| / max |b| over all pairs of the parent's runs, of all its processes).  Every figure is recorded."""
import argparse, itertools, json, os, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOMIC = ("full/Kn", "plain/")  # prefixes of the arrays under the spread rule


def worker(args):
    os.environ["LGNN_LIB_DIR"] = args.worker
    os.environ["LGNN_NO_PATHS"] = "1"  # plain/*: the class-plane route, whose GEMMs are gemm_kernel
    for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    import laplace_gnn_amd as lg
    import test_gpu_sampled_forward as tsf
    import test_gpu_ggn_matmat as tgm
    import test_gpu_gp as tgp
    import test_gpu_knn as tkn
    import test_gpu_lora as tlo
    import test_gpu_full_adjgrad as tfa
    from lowrank_utils import case_id, directions, edge_model, train_batches, train_set
    from test_gpu_frontend import model_from_golden

    have = os.path.exists(args.operands)
    stored = torch.load(args.operands) if have else {}
    out = {}

    def keep(name, r, t):
        out[f"{name}/{r}"] = t.detach().cpu().numpy()

    for name in ("gcn_small_m33", "sage_small_m33", "gcn_1layer", "sage_two_windows_two_row_tiles"):
        model, idx, theta = tsf._case(tsf.PARITY[name])
        for r in range(args.runs):
            keep(f"sampled/{name}", r, model.engine.sampled_forward(idx, theta))
        model.engine.check_async_errors()

    s0 = tgm.SHAPES[0]
    ggn_cases = [("gcn", 2, "relu", s0, False), ("sage", 2, "tanh", s0, False), ("gcn", 1, "relu", s0, False),
                 ("gcn", 3, "relu", s0, False)] + tgm.WIDE  # (the 3-layer model: jvp_block's route over Jacobian rows)
    for case in ggn_cases:
        eng = edge_model(*case).engine
        N, C = case[3][0], case[3][3]
        idx = train_set(N, C)[0][:37].contiguous()
        for k in (5, 33):
            V = directions(k, eng.n_params)
            for r in range(args.runs):
                keep(f"ggn/{case_id(case)}/jvp_block/k{k}", r, eng.jvp_block(idx, V))
                for route in ("structured", "from_jacobians"):
                    G, loss = torch.zeros_like(V), torch.zeros(1, device="cuda")
                    for bi, by in train_batches(N, C):
                        eng.ggn_matmat_(G, loss, bi, by, V, from_jacobians=route == "from_jacobians")
                    keep(f"ggn/{case_id(case)}/ggn_matmat/{route}/k{k}", r, G)
        eng.check_async_errors()

    gp_case = ("gcn", 2, "relu", tgp.SHAPES[0], False)
    for r in range(args.runs):
        for layout, K in tgp.device_kernels(gp_case).items():
            keep(f"gp/{layout}", r, K)

    for N, F, k in [(5, 3, 4), (65, 1, 32), tkn.SHAPES[0]]:
        X = torch.tensor(tkn.normal(N, F, 50 + N)).cuda()
        for r in range(args.runs):
            nbr, dist = lg.knn(X, k)
            keep(f"knn/N{N}F{F}k{k}/nbr", r, nbr)
            keep(f"knn/N{N}F{F}k{k}/dist", r, dist)

    path = min(tlo.PLAIN_GCN, key=lambda p: int(np.load(p)["X"].shape[0]))
    g = np.load(path)
    model = model_from_golden(g)
    eng = model.engine
    idx, y = torch.from_numpy(g["train_idx"]).cuda(), torch.from_numpy(g["train_y"]).cuda()
    loader = lg.TensorBatchLoader(idx, y, batch_size=int(g["batch_size"]))
    if not have:  # the weightings d(1/2 logdet) / d(factor): from one fit, the same bits for every child
        la = lg.KronLaplace(model, "classification", prior_precision=float(g["adjgrad_prior"]))
        la.fit(loader)
        stored["gB"] = [(0.5 * b).float().cpu() for b in la._logdet_factor_gradients()[0]]
        ld = lg.DiagLaplace(model, "classification", prior_precision=float(g["adjgrad_prior"]))
        ld.fit(loader)
        stored["gamma"] = (0.5 * ld._H_factor / ld.posterior_precision).float().cpu()
    gB, gamma = [b.cuda() for b in stored["gB"]], stored["gamma"].cuda()
    N, dims = eng.num_nodes, eng.dims
    eng.set_likelihood("classification")
    for r in range(args.runs):
        out_bar, G = torch.zeros(N, dims[-1], device="cuda"), torch.zeros(N, N, device="cuda")
        for X_b, y_b in loader:
            eng.adjgrad_batch_dense(X_b.cuda(), y_b.cuda(), gB, out_bar, G)
        keep("dense/kron/grad_dense", r, G)
        out_bar, G = torch.zeros(N, dims[-1], device="cuda"), torch.zeros(N, N, device="cuda")
        h1_bar, e_bar = torch.zeros(N, dims[1], device="cuda"), torch.zeros(N, dims[0] + 1, device="cuda")
        for X_b, y_b in loader:
            eng.diag_adjgrad_batch_dense(X_b.cuda(), y_b.cuda(), gamma, out_bar, h1_bar, e_bar, G)
        keep("dense/diag/grad_dense", r, G)
    eng.check_async_errors()

    model, idx, _, _ = tfa._product_case("gcn_golden")
    P = model.engine.n_params
    gen = torch.Generator().manual_seed(7)
    B = torch.randn(P, P, generator=gen, dtype=torch.float64)
    Gamma = B @ B.T / P + torch.diag(0.5 + torch.rand(P, generator=gen, dtype=torch.float64))
    Gamma = (0.5 * (Gamma + Gamma.T)).float().cuda().contiguous()
    for r in range(args.runs):
        Kn, R = model.engine.full_directions(idx, Gamma)
        keep("full/Kn", r, Kn)
        keep("full/R", r, R)
    model.engine.check_async_errors()

    g = np.load(os.path.join(ROOT, "tests", "golden", "gcn_mid_1batch_s0.npz"))
    model = model_from_golden(g)
    idx, y = torch.from_numpy(g["train_idx"]).cuda(), torch.from_numpy(g["train_y"]).cuda()
    loader = lg.TensorBatchLoader(idx, y, batch_size=int(g["batch_size"]))
    for r in range(args.runs):
        keep("plain/forward", r, model.engine.forward(idx))
        la = lg.KronLaplace(model, "classification")
        la.fit(loader)
        for l, facs in enumerate(la.H_facs.kfacs):
            for j, f in enumerate(facs):
                keep(f"plain/kron_factor_{l}_{j}", r, f)
    out["plain/used_paths"] = np.array(bool(getattr(model.engine, "last_kfac_used_paths", False)))
    model.engine.check_async_errors()
    if not have:
        torch.save(stored, args.operands)
    np.savez(args.out, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="lib_parent")
    ap.add_argument("--branch", default="lib")
    ap.add_argument("--runs", type=int, default=3, help="runs per child process")
    ap.add_argument("--procs", type=int, default=2, help="child processes per side")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child")
    ap.add_argument("--json", default=None)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--operands", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    import numpy as np

    with tempfile.TemporaryDirectory() as tmp:
        side = {args.parent: [], args.branch: []}
        for proc in range(args.procs):
            for lib in (args.parent, args.branch):  # fresh child processes, the parent's build first; the first failure ends the run
                out = os.path.join(tmp, f"{lib}_{proc}.npz")
                subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", lib, "--runs", str(args.runs), "--operands",
                                os.path.join(tmp, "operands.pt"), "--out", out], check=True, timeout=args.timeout)
                side[lib].append(dict(np.load(out)))
    used_paths = [bool(s.pop("plain/used_paths")) for lib in side for s in side[lib]]
    par, new = side[args.parent], side[args.branch]
    names = sorted({k.rsplit("/", 1)[0] for k in par[0]})
    assert all(names == sorted({k.rsplit("/", 1)[0] for k in s}) for s in par + new)

    def dist(a, b):
        return float(np.abs(a.astype(np.float64) - b).max() / max(np.abs(b.astype(np.float64)).max(), 1e-30))

    report, failed = [], []
    for name in names:
        p = [s[f"{name}/{r}"] for s in par for r in range(args.runs)]
        n = [s[f"{name}/{r}"] for s in new for r in range(args.runs)]
        rec = {"array": name, "bit_equal": all(np.array_equal(a, p[0]) for a in p + n),
               "parent_spread": max(dist(a, b) for a, b in itertools.combinations(p, 2)),
               "branch_spread": max(dist(a, b) for a, b in itertools.combinations(n, 2)),
               "branch_vs_parent": max(dist(a, b) for a in n for b in p)}
        rec["rule"] = "spread" if name.startswith(ATOMIC) else "bit_equal"
        rec["ok"] = bool(rec["branch_vs_parent"] <= 2 * rec["parent_spread"] if rec["rule"] == "spread" else rec["bit_equal"])
        report.append(rec)
        if not rec["ok"]:
            failed.append(rec)
        print(json.dumps(rec), flush=True)
    print(f"{len(report)} arrays, {len(failed)} outside: " + ", ".join(r["array"] for r in failed))
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"processes_per_side": args.procs, "runs_per_process": args.runs, "plain_fit_used_the_path_route": used_paths, "arrays": report}, f, indent=1)
    return 1 if failed or any(used_paths) else 0


if __name__ == "__main__":
    sys.exit(main())
