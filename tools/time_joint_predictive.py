"""dev: wall time of the joint GLM predictive ``la.glm_covariance(x)`` at the arxiv shape (2-layer GCN, F = 128, H = 256,
C = 40, P = 43 304, bench.py's arxiv-shaped synthetic graph) under a fitted ``KronLaplace`` and ``DiagLaplace``, against the
reference's formula on ANOTHER build of the library (the parent commit, which has no joint call):

  new        ``la.glm_covariance(x)`` for M = 64 and M = 512 evaluation nodes (K: 26 MB and 1.7 GB), and the structured route's
             split over its five stages (tables, V, NT GEMM, class contraction, placement) from the library's event pairs, with
             the NT stage's share of the fp32 MFMA peak (157.3 TFLOP/s) from the flop count of the shapes;
  baseline   ``Js = la.backend.jacobians(x)[0]`` and ``la.posterior_precision.inv_square_form(Js.reshape(1, M C, P))``
             (KronLaplace, laplace/baselaplace.py:1638-1644) resp. ``einsum("np,p,mp->nm", Js, 1 / precision, Js)`` (DiagLaplace,
             :1905-1910), with the package imported from ``--baseline-tree``.  M = 512 needs 3.5 GB of Jacobians and as much
             again for their product with P^-1: it is run if it fits, otherwise the record says it did not.

Each measurement: device events around a synchronised call, 3 warm-ups, 10 timed.  The two builds run as fresh processes,
alternated ``--rounds`` times.  The one condition checked: at M = 64 the new call is faster than the baseline on both
posteriors, outside the spread of the two (the slowest new run against the fastest baseline run over all rounds).

  python tools/time_joint_predictive.py --baseline-tree /path/to/a/built/parent/checkout
  --json PATH   one JSON document (default: profiles/joint_predictive.json)"""
import argparse, json, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_FP32_MFMA = 157.3e12

ap = argparse.ArgumentParser()
ap.add_argument("--baseline-tree", default=None, help="a built checkout of the commit to compare against")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--sizes", default="64,512")
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--child", choices=("new", "baseline"), default=None, help="(internal) one measuring process")
ap.add_argument("--tree", default=ROOT, help="(internal) where the child imports the package from")
ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "joint_predictive.json"))
args = ap.parse_args()
SIZES = [int(s) for s in args.sizes.split(",")]


def child():
    sys.path.insert(0, args.tree)
    import torch
    import bench
    import laplace_gnn_amd as lg

    assert torch.cuda.is_available(), "a timing needs the GPU"
    assert os.path.abspath(os.path.dirname(lg.__file__)).startswith(os.path.abspath(args.tree)), lg.__file__

    def emit(**rec):
        print("RECORD " + json.dumps(rec), flush=True)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ts, e0, e1 = [], torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.reps):
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return dict(ms_median=statistics.median(ts), ms_min=min(ts), ms_max=max(ts), reps=len(ts), warmup=args.warmup)

    w, ei, X, tri, try_ = bench.make_workload("arxiv", "cuda")
    torch.manual_seed(0)
    model = lg.GCN(w["F"], w["H"], w["C"], 2, X, ei, symmetric=True).to("cuda").eval()
    eng = model.engine
    C, P, F, H = w["C"], eng.n_params, w["F"], w["H"]
    shape = dict(N=w["N"], F=F, H=H, C=C, P=P)
    loader = lg.TensorBatchLoader(tri.to("cuda"), try_.to("cuda"), batch_size=w["batch"])
    nodes = torch.randperm(w["N"], generator=torch.Generator().manual_seed(1)).cuda()
    for structure in ("kron", "diag"):
        la = lg.Laplace(model, "classification", "all", structure)
        la.fit(loader)
        torch.cuda.synchronize()
        for M in SIZES:
            x = nodes[:M].contiguous()
            rec = dict(what=args.child, posterior=structure, M=M, k_bytes=(M * C) ** 2 * 4, **shape)
            if args.child == "new":
                rec.update(timed(lambda: la.glm_covariance(x)))
                eng.enable_kernel_timing(True)
                la.glm_covariance(x)
                torch.cuda.synchronize()
                ms = eng.kernel_timing_launches()
                eng.enable_kernel_timing(False)
                pairs = eng.glm_covariance_chunk_pairs()
                assert len(ms) == 5 * pairs, (len(ms), pairs)
                names = ("tables_ms", "v_ms", "nt_gemm_ms", "class_contraction_ms", "placement_ms")
                stages = {n: sum(ms[i::5]) for i, n in enumerate(names)}
                # NT stage: the last layer's C weighted Grams and, Kronecker: <V, S0 . V> over rows (n, c); diagonal: the H Grams of
                # the tables.  (One chunk pair at these sizes; of <V, S0 . V> only the 128 x 128 tiles on and above the diagonal are
                # computed, the mirror copies the upper triangle: the count is of the computed tiles.)
                nt_tiles = -(-M * C // 128)
                cov0_flops = nt_tiles * (nt_tiles + 1) // 2 * 2 * 128 * 128 * H * (F + 1)
                nt_flops = 2 * M * M * C * (H + 1) + (cov0_flops if structure == "kron" else 2 * M * M * H * (F + 1))
                rec.update(chunk_pairs=pairs, nt_flops=nt_flops, **stages,
                           nt_stage_share_of_fp32_mfma_peak=nt_flops / (stages["nt_gemm_ms"] * 1e-3) / PEAK_FP32_MFMA)
            else:
                inv = (1.0 / la.posterior_precision) if structure == "diag" else None

                def reference_formula():
                    Js = la.backend.jacobians(x)[0]
                    if structure == "kron":
                        return la.posterior_precision.inv_square_form(Js.reshape(1, M * C, P)).squeeze(0)
                    Js = Js.reshape(M * C, P)
                    return torch.einsum("np,p,mp->nm", Js, inv, Js)
                try:
                    rec.update(timed(reference_formula), jacobian_bytes=M * C * P * 4)
                except torch.OutOfMemoryError:
                    rec.update(did_not_fit=True, jacobian_bytes=M * C * P * 4)
                    torch.cuda.empty_cache()
            emit(**rec)
        del la
        torch.cuda.empty_cache()
    eng.check_async_errors()


def main():
    assert args.baseline_tree, "--baseline-tree: a built checkout of the commit to compare against"
    records = []
    for rnd in range(args.rounds):
        for mode, tree in (("baseline", os.path.abspath(args.baseline_tree)), ("new", ROOT)):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--tree", tree, "--sizes", args.sizes,
                   "--warmup", str(args.warmup), "--reps", str(args.reps)]
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=tree)
            if out.returncode != 0:
                sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
                raise SystemExit(f"{mode} process of round {rnd} failed ({out.returncode})")
            for line in out.stdout.splitlines():
                if line.startswith("RECORD "):
                    rec = dict(json.loads(line[7:]), round=rnd)
                    records.append(rec)
                    print(json.dumps(rec), flush=True)
    summary = []
    for structure in ("kron", "diag"):
        for M in SIZES:
            sel = lambda what: [r for r in records if r["what"] == what and r["posterior"] == structure and r["M"] == M and "ms_median" in r]
            new, base = sel("new"), sel("baseline")
            s = dict(what="summary", posterior=structure, M=M, new_ms_median=[r["ms_median"] for r in new],
                     baseline_ms_median=[r["ms_median"] for r in base] or "did not fit")
            if new and base:
                s.update(new_ms_max=max(r["ms_max"] for r in new), baseline_ms_min=min(r["ms_min"] for r in base),
                         speedup_of_medians=statistics.median(s["baseline_ms_median"]) / statistics.median(s["new_ms_median"]))
                s["faster_outside_the_spread"] = s["new_ms_max"] < s["baseline_ms_min"]
            summary.append(s)
            print(json.dumps(s), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(dict(tool="tools/time_joint_predictive.py", rounds=args.rounds, records=records, summary=summary), f, indent=1)
    for s in summary:
        if s["M"] == 64:
            assert s.get("faster_outside_the_spread"), f"the new call is not faster than the baseline at M = 64 ({s})"


if __name__ == "__main__":
    child() if args.child else main()
