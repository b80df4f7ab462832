"""dev: wall time of the functional (GP) Laplace at the arxiv shape (2-layer GCN, F = 128, H = 256, C = 40, P = 43 304,
bench.py's arxiv-shaped synthetic graph).

  gp_kernel       lgnn_gp_kernel(a, a): M = 1 024 with the full [M C, M C] layout and M = 8 192 with independent outputs, on the
                  structured route and under from_jacobians (the route the reference takes: Jacobian rows, then J J^T).  If one
                  from_jacobians call takes more than a minute, its M is halved and the time scaled by (M / M')^2 -- the record
                  says so.
  stages          the structured route's split over (a) tables, (b) NT GEMM, (c) class contraction, (d) placement from the
                  library's event pairs, with the bytes of G written by (b) and read by (c)
  fit             FunctionalLaplace.fit at the two sizes, split into kernel matrix / mu / Cholesky
  predictive      la(x) with the probit link on 10 000 nodes

Warm-up 2, then the median, minimum and maximum of 10 device-synchronised runs (fewer where a record says so).  The one
condition checked: the structured route executes ~120x fewer flops than the route over Jacobians and writes none, so it must
be faster at both sizes.

  --json PATH   write all records as one JSON document (default: $LGNN_OUT_DIR or out/ + gp_fit.json)"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bench
import laplace_gnn_amd as lg

ap = argparse.ArgumentParser()
ap.add_argument("--full", type=int, default=1024, help="M of the full-layout case")
ap.add_argument("--indep", type=int, default=8192, help="M of the independent-outputs case")
ap.add_argument("--eval", type=int, default=10_000)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--slow-reps", type=int, default=3, help="repetitions of anything whose first run takes more than 2 s")
ap.add_argument("--skip", default="", help="comma list of from_jacobians,fit,predictive")
ap.add_argument("--json", default=os.path.join(os.environ.get("LGNN_OUT_DIR", os.path.join(ROOT, "out")), "gp_fit.json"))
args = ap.parse_args()
assert torch.cuda.is_available(), "a timing needs the GPU"
RECORDS = []
skip = set(args.skip.split(","))


def dump():
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(dict(tool="tools/time_gp_fit.py", device=torch.cuda.get_device_name(0), records=RECORDS), f, indent=1)


def emit(**rec):
    print(json.dumps(rec), flush=True)
    RECORDS.append(rec)
    dump()


def once(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def timed(fn):
    """Warm-up and repetitions by the convention; a call whose first run takes more than 2 s gets warm-up 1 and --slow-reps."""
    out, first = once(fn)
    warmup, reps = (args.warmup, args.reps) if first < 2000 else (1, args.slow_reps)
    ts = []
    for rep in range(warmup - 1 + reps):
        out = None
        out, ms = once(fn)
        if rep >= warmup - 1:
            ts.append(ms)
    return out, dict(ms_median=statistics.median(ts), ms_min=min(ts), ms_max=max(ts), reps=len(ts), warmup=warmup)


w, ei, X, tri, try_ = bench.make_workload("arxiv", "cuda")
torch.manual_seed(0)
model = lg.GCN(w["F"], w["H"], w["C"], 2, X, ei, symmetric=True).to("cuda").eval()
eng = model.engine
C, P, F, H = w["C"], eng.n_params, w["F"], w["H"]
shape = dict(N=w["N"], F=F, H=H, C=C, P=P)
every = torch.randperm(w["N"], generator=torch.Generator().manual_seed(1))[:args.eval].cuda()
train = torch.randperm(w["N"], generator=torch.Generator().manual_seed(2)).cuda()  # distinct ids
eng.forward_all()

for M, indep in ((args.full, False), (args.indep, True)):
    a = train[:M].contiguous()
    Q = C if indep else C * C
    layout = "independent" if indep else "full"
    flops_struct = 2 * M * M * H * (F + 1) + 2 * M * M * H * Q
    flops_jac = 2 * M * M * Q * P
    K, t = timed(lambda: eng.gp_kernel(a, a, independent=indep))
    rec = dict(what="gp_kernel", route="structured", layout=layout, M=M, flops=flops_struct, jacobian_bytes=0, **t, **shape)
    struct_ms = t["ms_median"]
    # per-stage split from the library's event pairs: four per chunk pair, in the order (a) (b) (c) (d)
    eng.enable_kernel_timing(True)
    _ = eng.gp_kernel(a, a, independent=indep)
    torch.cuda.synchronize()
    ms = eng.kernel_timing_launches()
    eng.enable_kernel_timing(False)
    assert len(ms) % 4 == 0 and len(ms) > 0
    pairs_done = len(ms) // 4
    stages = {n: sum(ms[i::4]) for i, n in enumerate(("tables_ms", "nt_gemm_ms", "class_contraction_ms", "placement_ms"))}
    emit(**rec)
    # G [H][pairs] of every computed chunk pair is written once by (b) and read once by (c); with the same ids on both sides only
    # the upper chunk pairs are computed.  chunk: the library's rule (half the workspace limit for G and Kt, at most 2 048)
    per_pair = (H + Q + 1) * 4
    mc = max(1, min(int(((32 << 30) // 2 / per_pair) ** 0.5), 2048, M))
    nchunk = -(-M // mc)
    sizes = [min(mc, M - i * mc) for i in range(nchunk)]
    g_pairs = sum(sizes[i] * sizes[j] for i in range(nchunk) for j in range(i, nchunk))
    assert pairs_done == nchunk * (nchunk + 1) // 2, (pairs_done, nchunk)
    emit(what="stages", layout=layout, M=M, chunk=mc, chunk_pairs=pairs_done, g_bytes_written=g_pairs * H * 4,
         g_bytes_read=g_pairs * H * 4, k_bytes=M * M * Q * 4, **stages, **shape)
    if "from_jacobians" not in skip:
        Mj, scale, note = M, 1.0, None
        Kj, first = once(lambda: eng.gp_kernel(a, a, independent=indep, from_jacobians=True))
        while first > 60_000 and Mj > 64:
            del Kj
            Mj //= 2
            scale = (M / Mj) ** 2
            note = f"measured at M = {Mj}, scaled by (M / M')^2 = {scale:.0f}"
            aj = a[:Mj].contiguous()
            Kj, first = once(lambda: eng.gp_kernel(aj, aj, independent=indep, from_jacobians=True))
        aj = a[:Mj].contiguous()
        if Mj == M:
            err = float((K - Kj).abs().max()) / float(Kj.abs().max())
        else:
            sub = K[:, :Mj, :Mj] if indep else K[:Mj * C, :Mj * C]
            err = float((sub - Kj).abs().max()) / float(Kj.abs().max())
        del Kj
        _, t = timed(lambda: eng.gp_kernel(aj, aj, independent=indep, from_jacobians=True))
        jac_ms = t["ms_median"] * scale
        emit(what="gp_kernel", route="from_jacobians", layout=layout, M=M, measured_M=Mj, note=note, flops=flops_jac,
             jacobian_bytes=M * C * P * 4, scaled_ms_median=jac_ms, max_abs_diff_vs_structured_over_max=err,
             speedup_structured=jac_ms / struct_ms, flops_ratio=flops_jac / flops_struct, **t, **shape)
        assert struct_ms < jac_ms, "the structured route must be faster than the route over Jacobians: the route is broken"
    del K
    torch.cuda.empty_cache()

    if "fit" not in skip:
        loader = lg.TensorBatchLoader(a, torch.randint(0, C, (M,), generator=torch.Generator().manual_seed(3)).cuda(), batch_size=M)
        la = lg.FunctionalLaplace(model, "classification", n_subset=M, independent_outputs=indep)
        _, t = timed(lambda: la.fit(loader))
        sub = la.train_loader.indices
        _, tk = timed(lambda: la._kernel_batch(sub, sub))
        _, tm = timed(lambda: la._jvp(sub, la.mean))
        _, tc = timed(la._build_Sigma_inv)
        emit(what="fit", layout=layout, M=M, kernel_matrix_ms=tk["ms_median"], mu_ms=tm["ms_median"], cholesky_ms=tc["ms_median"],
             **t, **shape)
        if "predictive" not in skip:
            out, t = timed(lambda: la(every, link_approx="probit"))
            assert torch.allclose(out.sum(-1), torch.ones(len(every), device="cuda"), atol=1e-4)
            emit(what="predictive", link="probit", layout=layout, M=M, nodes=len(every), nodes_per_chunk=la._star_chunk(), **t,
                 **shape)
        del la
        torch.cuda.empty_cache()
eng.check_async_errors()
dump()
