"""dev: f_mu / f_var of the matrix-free GLM predictive (csrc/predictive.hip) from two builds of the library, compared.

  python tools/compare_predictive.py --parent lib_parent [--branch lib] [--runs 8] [--json PATH]

Each build (a directory beside the package's lib/, see LGNN_LIB_DIR in _lib.py) is driven in a fresh child process.  Cases:
{gcn, sage} x {kron, diag} x {plain entry, mapped entry, ext entry on a plain model, ext entry on a res + LayerNorm model}
on 2-layer models, and the plain and mapped entries on 1-layer models of the same graphs.  The posterior operands are computed
once (by the first child) and reused, so that both sides see the same bits.  f_mu and the one-layer f_var have no float atomics
behind them and must be bit-equal over all runs of both sides; a 2-layer f_var (LDS float atomics) must differ from the parent
by no more than twice the parent's own run-to-run spread (max |a - b| / max |b| over all pairs of runs)."""
import argparse, itertools, json, os, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN = {"gcn": "gcn_mid_1batch_s0", "sage": "sage_mid_2batch_s2"}
RESNORM = {"gcn": "gcn_resln_mid_2batch_s0", "sage": "sage_ln_mid_2batch_s1"}


def worker(args):
    os.environ["LGNN_LIB_DIR"] = args.worker
    for p in (ROOT, os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    import laplace_gnn_amd as lg
    from test_gpu_frontend import model_from_golden

    have = os.path.exists(args.operands)
    stored = torch.load(args.operands) if have else {}
    out = {}

    def cases(kind, post, tag, model, g, entries):
        loader = lg.TensorBatchLoader(torch.from_numpy(g["train_idx"]).cuda(), torch.from_numpy(g["train_y"]).cuda(),
                                      batch_size=int(g["batch_size"]))
        la = (lg.KronLaplace if post == "kron" else lg.DiagLaplace)(model, "classification", prior_precision=2.0)
        la.fit(loader)  # (also leaves the forward's buffers in the engine)
        x = torch.from_numpy(g["pred_idx"]).cuda()
        C = la.n_outputs
        E = torch.from_numpy(np.random.default_rng(5).standard_normal((C + 3, C)).astype(np.float32)).cuda()
        for entry in entries:
            name = f"{kind}/{post}/{tag}/{entry}"
            out_map = E if entry == "mapped" else None
            if not have:
                stored[name] = {k: None if v is None else v.cpu() for k, v in la._matrix_free_operands(out_map).items()}
            ops = {k: None if v is None else v.cuda() for k, v in stored[name].items()}
            call = model.engine.glm_variance_ext if entry.startswith("ext") else model.engine.glm_variance
            for r in range(args.runs):
                f_mu, f_var = call(x, out_map=out_map, **ops)
                out[f"{name}/f_mu/{r}"], out[f"{name}/f_var/{r}"] = f_mu.cpu().numpy(), f_var.cpu().numpy()
        model.engine.check_async_errors()

    for kind, post in itertools.product(("gcn", "sage"), ("kron", "diag")):
        g = np.load(os.path.join(ROOT, "tests", "golden", PLAIN[kind] + ".npz"))
        cases(kind, post, "2layer", model_from_golden(g), g, ("plain", "mapped", "ext_plain"))
        gr = np.load(os.path.join(ROOT, "tests", "golden", RESNORM[kind] + ".npz"))
        cases(kind, post, "2layer", model_from_golden(gr), gr, ("ext_resnorm",))
        torch.manual_seed(0)
        X, ei = torch.from_numpy(g["X"]), torch.from_numpy(g["edge_index"])
        one = (lg.GCN if kind == "gcn" else lg.GraphSAGE)(X.shape[1], 16, int(g["n_outputs"]), 1, X, ei,
                                                          symmetric=bool(g["symmetric"])).eval().cuda()
        cases(kind, post, "1layer", one, g, ("plain", "mapped"))
    if not have:
        torch.save(stored, args.operands)
    np.savez(args.out, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="lib_parent")
    ap.add_argument("--branch", default="lib")
    ap.add_argument("--runs", type=int, default=8)
    ap.add_argument("--json", default=None)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--operands", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    import numpy as np

    with tempfile.TemporaryDirectory() as tmp:
        side = {}
        for lib in (args.parent, args.branch):  # fresh child processes, the parent's build first
            out = os.path.join(tmp, f"{len(side)}.npz")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", lib, "--runs", str(args.runs), "--operands",
                            os.path.join(tmp, "operands.pt"), "--out", out], check=True, timeout=600)
            side[lib] = dict(np.load(out))
    par, new = side[args.parent], side[args.branch]
    names = sorted({k.rsplit("/", 1)[0] for k in par})
    dist = lambda a, b: float(np.abs(a.astype(np.float64) - b).max() / max(np.abs(b).max(), 1e-30))
    report, failed = [], []
    for name in names:
        p = [par[f"{name}/{r}"] for r in range(args.runs)]
        n = [new[f"{name}/{r}"] for r in range(args.runs)]
        rec = {"array": name}
        if name.endswith("f_mu") or "/1layer/" in name:
            rec["bit_equal"] = all(np.array_equal(a, p[0]) for a in p + n)
            ok = rec["bit_equal"]
        else:
            rec["parent_spread"] = max(dist(a, b) for a, b in itertools.combinations(p, 2))
            rec["branch_spread"] = max(dist(a, b) for a, b in itertools.combinations(n, 2))
            rec["branch_vs_parent"] = max(dist(a, b) for a in n for b in p)
            ok = rec["branch_vs_parent"] <= 2 * rec["parent_spread"]
        rec["ok"] = bool(ok)
        report.append(rec)
        if not ok:
            failed.append(rec)
        print(json.dumps(rec), flush=True)
    print(f"{len(report)} arrays, {len(failed)} outside: " + ", ".join(r["array"] for r in failed))
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"runs_per_side": args.runs, "arrays": report}, f, indent=1)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
