"""dev: ``HipGGN.ggn_matmat`` against ``HipHessian.hessian_matmat`` (the GGN product plus the residual product of
csrc/hessmat.hip) with k = 32 directions on the same engine, at two shapes:

  cora    2-layer GCN at bench.py's Cora-shaped workload (BASELINE.json configs[1]: N = 2 708, F = 1 433, H = 64, C = 7), one
          batch of its 1 299 training nodes
  test    2-layer GCN at the (300, 37, 64, 7) shape of tests/test_gpu_hessian.py, 60 random training nodes

Warm-up 3, then the median, minimum and maximum of 20 device-synchronised runs, the two products alternating so that both
see the same machine state.  The residual product does one tile GEMM and two outer products where the GGN product does the same
plus a gather, a curvature pass and a transpose: the ratio is expected below 2 and is reported, not tuned.

  --ggn-only    time the GGN product alone: runs on a commit that has no HipHessian yet (the comparison with the parent commit)
  --json PATH   write all records as one JSON document (default: $LGNN_OUT_DIR or out/ + hessian_matmat.json)"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bench
import laplace_gnn_amd as lg

ap = argparse.ArgumentParser()
ap.add_argument("--k", type=int, default=32)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--ggn-only", action="store_true")
ap.add_argument("--json", default=os.path.join(os.environ.get("LGNN_OUT_DIR", os.path.join(ROOT, "out")), "hessian_matmat.json"))
args = ap.parse_args()
assert torch.cuda.is_available(), "a timing needs the GPU"
RECORDS = []


def emit(**rec):
    print(json.dumps(rec), flush=True)
    RECORDS.append(rec)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(dict(tool="tools/time_hessian_matmat.py", device=torch.cuda.get_device_name(0), records=RECORDS), f, indent=1)


def summary(ts):
    return dict(ms_median=statistics.median(ts), ms_min=min(ts), ms_max=max(ts), reps=len(ts), warmup=args.warmup)


def cora():
    w, ei, X, tri, try_ = bench.make_workload("cora", "cuda")
    torch.manual_seed(0)
    m = lg.GCN(w["F"], w["H"], w["C"], 2, X, ei, symmetric=True).to("cuda").eval()
    return m, tri.cuda().contiguous(), try_.cuda().contiguous(), dict(N=w["N"], F=w["F"], H=w["H"], C=w["C"])


def test_shape():
    N, F, H, C = 300, 37, 64, 7
    g = torch.Generator().manual_seed(0)
    X, ei = torch.randn(N, F, generator=g), torch.randint(0, N, (2, 3 * N), generator=g)
    torch.manual_seed(0)
    m = lg.GCN(F, H, C, 2, X, ei).to("cuda").eval()
    return m, torch.randperm(N, generator=g)[:60].cuda(), torch.randint(0, C, (60,), generator=g).cuda(), dict(N=N, F=F, H=H, C=C)


for name, make in (("cora", cora), ("test", test_shape)):
    m, idx, y, shape = make()
    P = m.engine.n_params
    V = torch.randn(args.k, P, generator=torch.Generator().manual_seed(4)).cuda()
    products = {"ggn_matmat": lg.HipGGN(m, "classification").ggn_matmat}
    if not args.ggn_only:
        products["hessian_matmat"] = lg.HipHessian(m, "classification").hessian_matmat
    times, outs = {n: [] for n in products}, {}
    for rep in range(args.warmup + args.reps):
        for pname, fn in products.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            outs[pname] = fn([(idx, y)], V)[0]
            torch.cuda.synchronize()
            if rep >= args.warmup:
                times[pname].append((time.perf_counter() - t0) * 1e3)
    m.engine.check_async_errors()
    for pname in products:
        emit(what=pname, shape=name, M=int(idx.shape[0]), k=args.k, P=P, **summary(times[pname]), **shape)
    if args.ggn_only:
        continue
    g_ms, h_ms = statistics.median(times["ggn_matmat"]), statistics.median(times["hessian_matmat"])
    resid = outs["hessian_matmat"] - outs["ggn_matmat"]
    emit(what="ratio", shape=name, hessian_over_ggn=h_ms / g_ms, below_two=h_ms < 2 * g_ms,
         max_abs_resid_over_max_abs_ggn=float(resid.abs().max()) / float(outs["ggn_matmat"].abs().max()))
