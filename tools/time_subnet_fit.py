"""dev: wall time of subnetwork Laplace at the arxiv shape (2-layer GCN, F = 128, H = 256, C = 40, P = 43 304, bench.py's
arxiv-shaped synthetic graph), 4 096 training nodes in one batch, subnetworks of the S largest-magnitude weights.

  subnet_fit    FullSubnetLaplace.fit (lgnn_subnet_full_accumulate: only the selected Jacobian columns are built)
  predictive    la(x) with the probit link on 10 000 nodes under that posterior (lgnn_jacobians_subset)
  full_fit      the route to the same matrix without the subnetwork entry points: FullLaplace.fit on the same batch, then the
                sub-block -- timed once per run of the tool, compared with every S

Warm-up 2, then the median, minimum and maximum of 10 device-synchronised runs.  Each record also carries the Jacobian bytes
written and the Gram flops executed per fit, computed from the shapes.  The one condition checked: at S = 2 048 the subset fit
executes ~450x fewer Gram flops and ~21x fewer Jacobian bytes than the full fit, so it must be faster.

  --json PATH   write all records as one JSON document (default: $LGNN_OUT_DIR or out/ + subnet_fit.json)"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bench
import laplace_gnn_amd as lg

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="256,2048,8192")
ap.add_argument("--train", type=int, default=4096)
ap.add_argument("--eval", type=int, default=10_000)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--full-reps", type=int, default=10)
ap.add_argument("--skip", default="", help="comma list of full_fit,predictive")
ap.add_argument("--json", default=os.path.join(os.environ.get("LGNN_OUT_DIR", os.path.join(ROOT, "out")), "subnet_fit.json"))
args = ap.parse_args()
assert torch.cuda.is_available(), "a timing needs the GPU"
RECORDS = []
skip = set(args.skip.split(","))


def dump():
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(dict(tool="tools/time_subnet_fit.py", device=torch.cuda.get_device_name(0), records=RECORDS), f, indent=1)


def emit(**rec):
    print(json.dumps(rec), flush=True)
    RECORDS.append(rec)
    dump()


def timed(fn, warmup, reps):
    ts, out = [], None
    for rep in range(warmup + reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if rep >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return out, dict(ms_median=statistics.median(ts), ms_min=min(ts), ms_max=max(ts), reps=len(ts), warmup=warmup)


w, ei, X, tri, try_ = bench.make_workload("arxiv", "cuda")
torch.manual_seed(0)
model = lg.GCN(w["F"], w["H"], w["C"], 2, X, ei, symmetric=True).to("cuda").eval()
eng = model.engine
M, C, P = args.train, w["C"], eng.n_params
idx, y = tri[:M].cuda().contiguous(), try_[:M].cuda().contiguous()
loader = lg.TensorBatchLoader(idx, y, batch_size=M)
every = torch.randperm(w["N"], generator=torch.Generator().manual_seed(1))[:args.eval].cuda()
shape = dict(N=w["N"], F=w["F"], H=w["H"], C=C, P=P, M=M)
eng.forward_all()

full_ms, H_full = None, None
if "full_fit" not in skip:
    lf = lg.Laplace(model, "classification", "all", "full")
    _, t = timed(lambda: lf.fit(loader), args.warmup, args.full_reps)
    full_ms, H_full = t["ms_median"], lf.H
    emit(what="full_fit", jacobian_bytes=M * C * P * 4, gram_flops=2 * M * C * P * P, **t, **shape)

for S in [int(s) for s in args.sizes.split(",")]:
    sub = lg.LargestMagnitudeSubnetMask(model, S).select()
    ld = -(-S // 4) * 4
    la = lg.Laplace(model, "classification", "subnetwork", "full", subnetwork_indices=sub)
    _, t = timed(lambda: la.fit(loader), args.warmup, args.reps)
    rec = dict(what="subnet_fit", S=S, jacobian_bytes=M * C * ld * 4, gram_flops=2 * M * C * S * S, **t, **shape)
    if H_full is not None:
        block = H_full[sub][:, sub]
        rec.update(full_fit_ms_median=full_ms, speedup_vs_full_fit=full_ms / t["ms_median"],
                   flops_ratio=(P / S) ** 2, bytes_ratio=P / ld,
                   rel_err_vs_full_block=float((la.H.double() - block.double()).norm() / block.double().norm()))
        if S == 2048:
            assert t["ms_median"] < full_ms, "the subset fit at S = 2048 must be faster than the full fit: the route is broken"
        del block
    emit(**rec)
    if "predictive" not in skip:
        out, t = timed(lambda: la(every, link_approx="probit"), args.warmup, args.reps)
        assert torch.allclose(out.sum(-1), torch.ones(len(every), device="cuda"), atol=1e-4)
        emit(what="predictive", link="probit", S=S, nodes=len(every), jacobian_bytes=len(every) * C * S * 4, **t, **shape)
    del la
    torch.cuda.empty_cache()
eng.check_async_errors()
dump()
