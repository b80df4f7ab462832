"""dev: the GGN-times-block product and LowRankLaplace.fit at the arxiv shape (2-layer GCN, F = 128, H = 256, C = 40,
P = 43 304, bench.py's arxiv-shaped synthetic graph).

  ggn_matmat    one batch of 10 000 training nodes, k = 18 directions (K = 10 plus oversampling): the structured route and
                the route over lgnn_jacobians rows (from_jacobians=True) on the same commit, alternating; device bytes of
                each (lgnn_device_bytes before / after, a fresh engine per route); the per-phase kernel times of the
                structured route from the library's timing events, and the achieved flop rate of its two outer products
                against 4 |R| (F + 1) H k flops
  fit           LowRankLaplace.fit on the workload's full training loader (batches of 10 000): wall time and sweep count

Warm-up 2, then the median, minimum and maximum of device-synchronised runs.  Two conditions are checked and reported, not
tuned: the structured route allocates no M C P buffer, and it is not slower than the general route.

  --json PATH   write all records as one JSON document (default: $LGNN_OUT_DIR or out/ + lowrank_fit.json)"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bench
import laplace_gnn_amd as lg

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=10_000)
ap.add_argument("--k", type=int, default=18)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--fit-reps", type=int, default=3)
ap.add_argument("--skip", default="", help="comma list of general,fit")
ap.add_argument("--json", default=os.path.join(os.environ.get("LGNN_OUT_DIR", os.path.join(ROOT, "out")), "lowrank_fit.json"))
args = ap.parse_args()
assert torch.cuda.is_available(), "a timing needs the GPU"
RECORDS = []
skip = set(args.skip.split(","))


def emit(**rec):
    print(json.dumps(rec), flush=True)
    RECORDS.append(rec)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(dict(tool="tools/time_lowrank_fit.py", device=torch.cuda.get_device_name(0), records=RECORDS), f, indent=1)


def summary(ts, warmup):
    return dict(ms_median=statistics.median(ts), ms_min=min(ts), ms_max=max(ts), reps=len(ts), warmup=warmup)


def fresh_model():
    torch.manual_seed(0)
    return lg.GCN(w["F"], w["H"], w["C"], 2, X, ei, symmetric=True).to("cuda").eval()


w, ei, X, tri, try_ = bench.make_workload("arxiv", "cuda")
M, k, C = args.batch, args.k, w["C"]
idx, y = tri[:M].cuda().contiguous(), try_[:M].cuda().contiguous()
models = {"structured": fresh_model()}
if "general" not in skip:
    models["general"] = fresh_model()
P = models["structured"].engine.n_params
V = torch.randn(k, P, generator=torch.Generator().manual_seed(4)).cuda()
shape = dict(N=w["N"], F=w["F"], H=w["H"], C=C, P=P, M=M, k=k)
# |R|: the rows the batch reads (the batch, its in- and out-neighbours: symmetric propagation with self loops)
eic = ei.cuda()
in_batch = torch.zeros(w["N"], dtype=torch.bool, device="cuda")
in_batch[idx] = True
need = in_batch.clone()
need[eic[1][in_batch[eic[0]]]] = True
need[eic[0][in_batch[eic[1]]]] = True
R = int(need.sum())

times, bytes_, outs = {n: [] for n in models}, {}, {}
for name, m in models.items():
    m.engine.forward_all()
    bytes_[name] = [m.engine.device_bytes()]


def run(name):
    eng = models[name].engine
    G = torch.zeros_like(V)
    loss = torch.zeros(1, device="cuda")
    torch.cuda.synchronize(); t0 = time.perf_counter()
    eng.ggn_matmat_(G, loss, idx, y, V, from_jacobians=name == "general")
    torch.cuda.synchronize()
    outs[name] = G
    return (time.perf_counter() - t0) * 1e3


for rep in range(args.warmup + args.reps):  # alternating: both routes see the same machine state
    for name in models:
        t = run(name)
        if rep >= args.warmup:
            times[name].append(t)
for name, m in models.items():
    bytes_[name].append(m.engine.device_bytes())
    m.engine.check_async_errors()
    emit(what="ggn_matmat_" + name, device_bytes_before=bytes_[name][0], device_bytes_after=bytes_[name][1],
         device_bytes_added=bytes_[name][1] - bytes_[name][0], jacobian_bytes_M_C_P=M * C * P * 4, needed_rows=R,
         **summary(times[name], args.warmup), **shape)
st = statistics.median(times["structured"])
cond = dict(what="conditions", structured_allocates_no_M_C_P_buffer=bytes_["structured"][1] - bytes_["structured"][0] < M * C * P * 4)
if "general" in models:
    gt = statistics.median(times["general"])
    diff = float((outs["structured"] - outs["general"]).abs().max()) / float(outs["general"].abs().max())
    cond.update(structured_not_slower_than_general=st <= gt, speedup=gt / st, max_abs_diff_over_max=diff)
emit(**cond)

# per-phase kernel times of the structured route (the library's event pairs; one chunk of directions at this shape)
eng = models["structured"].engine
eng.enable_kernel_timing(True)
phases = []
for _ in range(5):
    run("structured")
    phases.append(eng.kernel_timing_launches()[-4:])
eng.enable_kernel_timing(False)
med = [statistics.median(p[j] for p in phases) for j in range(4)]
flops = 4.0 * R * (w["F"] + 1) * w["H"] * k
emit(what="structured_phases", ms_forward_gather=med[0], ms_curvature=med[1], ms_qbar_bias=med[2], ms_outer_finish=med[3],
     outer_gemm_flops=flops, outer_gemm_tflops=flops / ((med[0] + med[3]) * 1e-3) / 1e12,
     note="flop rate: 4 |R| (F + 1) H k over the forward + gather and outer-products + finish phases (an upper bound of the two "
          "outer products' own time)", **shape)

if "fit" not in skip:
    loader = lg.TensorBatchLoader(tri.cuda(), try_.cuda(), batch_size=args.batch)
    la = lg.Laplace(models["structured"], "classification", "all", "lowrank", backend_kwargs=dict(low_rank=10))
    ts = []
    for rep in range(1 + args.fit_reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        la.fit(loader)
        torch.cuda.synchronize()
        if rep >= 1:
            ts.append((time.perf_counter() - t0) * 1e3)
    lam = [float(v) for v in la.H[1]]
    emit(what="lowrank_fit", n_train=len(loader.dataset), batches=len(loader), low_rank=10, block=18, n_sweeps=la.n_sweeps,
         converged=bool(la.converged), tol=lg.lowrank.DEFAULT_TOL, eigenvalues=lam,
         max_residual_over_l1=float(la.residuals.max()) / lam[0], **summary(ts, 1), **shape)
