#!/usr/bin/env python3
"""la.fit() throughput of the curvature path on MI355X (BASELINE.json metric).

Default workload (BASELINE.json configs[2], SURVEY.md 8(d) "C3"): 2-layer GCN on a synthetic ogbn-arxiv-shaped
graph -- N = 169 343 nodes, 1 166 243 undirected random edges (symmetrised, self loops added), F = 128, H = 256,
C = 40, N_train = 90 941 in 10 mini-batches of 10 000 (reference loader: batch_size=10000, shuffle=False),
hessian_structure="kron".  Other workloads: ``--workload cora`` (configs[1], diag), ``--workload products``
(configs[4], last-layer full GGN), ``arxiv_sage`` / ``arxiv_powerlaw`` (not BASELINE configs).

A *step* is one complete ``la.fit(loader)``: forward + A-factor Grams (recomputed every step: the engine's cache is
invalidated first), the per-batch accumulations, the factor all-reduce (N > 1) and, for kron, the eigendecomposition
``fit`` ends with.  value = steps * N_train / wall.  Besides the wall of the K steps the line carries per-step medians
from device events: ``ms_per_step_median`` (fit total) and ``accumulate_ms`` (the batch loop only: no all-reduce, no
decomposition), SURVEY.md 8(d).

    python bench.py --gpus N --steps K --warmup W        # N > 1: launches its own ranks (torch.distributed.run)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \\
        --master-port P bench.py --gpus N --steps K --warmup W

A plain run only sets up, warms up, times the K steps and prints the line (``roofline`` and ``cpu_baseline`` are null).
``--full`` adds everything else: the dominant kernel's launch timing during the timed steps (plus, for a captured diag fit,
three launch-by-launch fits behind them), the roofline block built from it and the CPU baselines (``--no-cpu-baseline``
leaves those out again).  ``--dump-outputs DIR`` writes what ``la.fit()`` handed back after the last timed step as
``DIR/<name>.npy`` (``_fit_outputs``): the inputs are seeded, so two builds can be compared output for output.

N > 1: one process per GPU, the graph / features / weights replicated.  A batch's SAMPLES are never split for KFAC
(B factors have cross-sample terms inside a batch), but B = sum over batches and class columns, so the 10 x 40
(batch, class) units are dealt in balanced runs of 400/N (laplace_gnn_amd.units_of_rank) and one RCCL all-reduce sums
the flat factor buffer; every rank then runs the one batched eigendecomposition on its bit-identical factors (no
second collective).  diag / last-layer: every rank takes its slice of every batch's samples.  Total work is fixed =>
"strong" scaling; the forward pass and the per-batch seeds are replicated (Amdahl).
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WORKLOADS = {
    # name: N, undirected edges, F, H, C, N_train, batch
    "arxiv": dict(N=169_343, E=1_166_243, F=128, H=256, C=40, n_train=90_941, batch=10_000),
    "cora": dict(N=2_708, E=5_278, F=1_433, H=64, C=7, n_train=1_299, batch=10_000),
    # same graph and widths as "arxiv" with the other model family of the path (GraphSAGE, mean aggregation)
    "arxiv_sage": dict(N=169_343, E=1_166_243, F=128, H=256, C=40, n_train=90_941, batch=10_000, kind="sage"),
    # the same sizes with power-law degrees (hubs of ~1e4 neighbours like the real ogbn-arxiv citation graph)
    "arxiv_powerlaw": dict(N=169_343, E=1_166_243, F=128, H=256, C=40, n_train=90_941, batch=10_000, powerlaw=0.5),
    # BASELINE configs[4]: 3-layer GraphSAGE, last-layer full GGN (P_LL = 47 * 513 = 24 111), power-law degrees
    "products": dict(N=2_449_029, E=61_859_140, F=100, H=256, C=47, n_train=196_615, batch=10_000, layers=3,
                     kind="sage", powerlaw=0.5),
}
BASELINE_CONFIG = dict(arxiv=2, cora=1, products=4)
DEFAULT_STRUCTURE = {"arxiv": "kron", "arxiv_sage": "kron", "arxiv_powerlaw": "kron", "cora": "diag",
                     "products": "lastlayer"}
PEAK_MFMA_F32_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
PEAK_HBM_GBS = 8000.0


def make_workload(name: str, device, seed: int = 0):
    """Seeded synthetic inputs of the named shape; generated on the CPU generator so
    every rank (and the CPU baseline) sees identical data."""
    import torch

    w = WORKLOADS[name]
    g = torch.Generator().manual_seed(seed)
    if "powerlaw" in w:
        # endpoints from P(i) ~ i^-alpha by inverse CDF, node ids shuffled; alpha = 0.5 gives hubs of ~1e4..1e5
        # neighbours next to a median degree of a few tens (ogbn-products: max 17 481, median ~ 26)
        a = w["powerlaw"]
        perm = torch.randperm(w["N"], generator=g)
        ends = []
        for _ in range(2):
            u = torch.rand(w["E"], generator=g, dtype=torch.float64)
            ends.append(perm[(u.pow(1.0 / (1.0 - a)) * w["N"]).long().clamp_(max=w["N"] - 1)])
        ei = torch.stack(ends)
    else:
        ei = torch.randint(0, w["N"], (2, w["E"]), generator=g, dtype=torch.int64)
    X = torch.randn(w["N"], w["F"], generator=g)
    y_all = torch.randint(0, w["C"], (w["N"],), generator=g, dtype=torch.int64)
    train_idx = torch.randperm(w["N"], generator=g)[: w["n_train"]]
    train_y = y_all[train_idx]
    return w, ei, X, train_idx, train_y


def _threads():
    try:
        from threadpoolctl import threadpool_info
        return max([p.get("num_threads", 1) for p in threadpool_info()] + [1])
    except Exception:
        return os.cpu_count() or 1


def cpu_baseline(name: str, ei, X, Ws, bs, train_idx, train_y, w, structure, model=None):
    """Oracle (CPU restatement, numpy + scipy; oracle/gnn_laplace_oracle.py, kind "port") timed on the host cores on
    a BOUNDED sample of the same workload.  Dense GEMMs run on all BLAS threads; scipy's CSR products are single
    threaded (said in ``sample``).  The reference itself cannot execute the arxiv / products shapes (dense N x N
    adjacency: 115 GB / 24 TB); for the Cora shape ``cpu_baseline_dense`` times the reference-faithful dense mode."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import gnn_laplace_oracle as O
    import numpy as np

    cores = int(_threads())
    kind = w.get("kind", "gcn")
    M = min(w["batch"], w["n_train"])
    if structure == "lastlayer":
        # the forward pass (3 sparse layers over 2.4 M nodes) is NOT part of the sample: features and logits of the
        # sampled batch nodes come from the GPU forward; timed = the reference-style Jacobian einsum of 48 samples
        ms = 48
        eng = model.engine
        idx = train_idx[:ms].to(eng.device)
        f = eng.forward(idx).cpu().numpy()
        d = eng.in_dims[-1]
        rng = np.random.default_rng(0)
        phi = rng.standard_normal((ms, d)).astype(np.float32)  # same shape / arithmetic; values do not change the cost
        t0 = time.perf_counter()
        O.lastlayer_full_from_features(phi, np.ones(ms, np.float32), f)
        dt = time.perf_counter() - t0
        return {"value": ms / dt, "unit": "samples/s", "cores": cores, "kind": "port",
                "sample": f"{ms} samples of the first mini-batch, last-layer Jacobian einsum only (P = {d * w['C'] + w['C']}; "
                          f"the 3-layer forward over {w['N']} nodes excluded, which favours the CPU), "
                          f"oracle.lastlayer_full_from_features, {dt:.1f} s"}
    rp, col = O.edge_index_to_adj_csr(ei.numpy(), w["N"], kind, True)
    om = O.GnnModel(kind, rp, col, X.numpy(), Ws, bs)
    # scipy's CSR products run on one core; BASELINE.md section 3 plans the baseline on all host cores: the same row-sequential
    # fp32 sums from an OpenMP loop (oracle/spmm_omp.c), checked here against scipy on this very model before the clock starts
    threaded = False
    if structure == "kron":
        plain = om.P @ om.X[:, :8].copy()
        threaded = O.use_threaded_products(om)
        if threaded:
            assert np.array_equal(om.P @ np.ascontiguousarray(om.X[:, :8]), plain), "threaded CSR product differs from scipy's"
        t0 = time.perf_counter()
        O.kfac_batch(om, train_idx[:M].numpy(), train_y[:M].numpy(), w["n_train"])
        dt = time.perf_counter() - t0
        what, ms = "kfac_batch", M
    else:
        ms = min(M, 256)  # 30 ms of python per sample: bounded to ~10 s
        t0 = time.perf_counter()
        O.diag_batch(om, train_idx[:ms].numpy(), train_y[:ms].numpy())
        dt = time.perf_counter() - t0
        what = "diag_batch"
    sparse_note = (f"CSR products on {cores} OpenMP threads (oracle/spmm_omp.c)" if threaded
                   else "scipy CSR products on one core" + ("" if structure != "kron" else " (oracle/_build/libspmm_omp.so not built)"))
    return {
        "value": ms / dt, "unit": "samples/s", "cores": cores, "kind": "port",
        "sample": f"{ms} of the {w['n_train']} samples (first mini-batch) of the same {name}-shaped {structure} fit, forward "
                  f"and A factors included (the reference recomputes them per batch), oracle/gnn_laplace_oracle.{what} "
                  f"(sparse restatement: dense GEMMs on {cores} BLAS threads, {sparse_note}), {dt:.1f} s",
    }


def cpu_baseline_dense(ei, X, Ws, bs, train_idx, train_y, w, structure):
    """Reference-faithful dense mode for the Cora shape: dense N x N adjacency, normalize_adj as two
    dense N^3 products on every forward, three forwards per batch, dense backward passes -- comparable with the
    reference's own 8-vCPU measurement in BASELINE.md (~0.5 k samples/s kron, ~30 samples/s diag)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import gnn_laplace_oracle as O

    rp, col = O.edge_index_to_adj_csr(ei.numpy(), w["N"], "gcn", True)
    om = O.GnnModel("gcn", rp, col, X.numpy(), Ws, bs)
    M = min(w["batch"], w["n_train"])
    if structure == "kron":
        ms = M
        t0 = time.perf_counter()
        O.dense_mode_kron_batch(om, train_idx[:ms].numpy(), train_y[:ms].numpy(), w["n_train"])
    else:
        ms = min(M, 128)
        t0 = time.perf_counter()
        O.dense_mode_diag_batch(om, train_idx[:ms].numpy(), train_y[:ms].numpy())
    dt = time.perf_counter() - t0
    return {"value": ms / dt, "unit": "samples/s", "cores": int(_threads()), "kind": "port",
            "sample": f"{ms} of {w['n_train']} samples, reference-faithful DENSE mode (dense adjacency, per-forward "
                      f"normalize_adj, 3 forwards, dense backward passes), oracle.dense_mode_{structure}_batch, {dt:.1f} s"}


def _parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="arxiv", choices=sorted(WORKLOADS))
    ap.add_argument("--structure", default=None, choices=["kron", "diag", "lastlayer"],
                    help="hessian_structure; default kron for arxiv (BASELINE configs[2]), diag for cora (configs[1]), "
                         "last-layer full GGN for products (configs[4])")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: kernel launch timing, roofline, CPU baselines")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the arrays the last timed la.fit() produced as DIR/<name>.npy (at most 64 MB in all)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave out the CPU baselines")
    ap.add_argument("--no-fit-graph", action="store_true",
                    help="diag workloads: time the launch-by-launch fit instead of the captured graph")
    ap.add_argument("--emulate-world", type=int, default=0,
                    help="dev aid, 1 GPU: time only the share rank 0 of an N-rank job would execute (no all-reduce); "
                         "prints the per-rank time, not a valid bench line")
    return ap.parse_args()


def _launch_ranks(args) -> int:
    """``python bench.py --gpus N`` without a launcher: start N ranks of this same file under torch.distributed.run
    as a CHILD process (this parent never touches the GPU), relay rank 0's JSON line, return the child's code."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC for RCCL on this pool
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // max(args.gpus, 1))))
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, env=env, text=True)
    lines = []
    for line in proc.stdout:
        if line.lstrip().startswith("{"):
            lines.append(line.rstrip("\n"))
        else:
            sys.stderr.write(line)
    rc = proc.wait()
    if rc != 0:
        sys.stderr.write(f"bench.py: the {args.gpus}-rank child exited with code {rc}\n")
        return rc
    if not lines:
        sys.stderr.write("bench.py: the ranks produced no JSON line\n")
        return 1
    print(lines[-1], flush=True)
    return 0


def _median(xs):
    xs = sorted(xs)
    n = len(xs)
    return None if n == 0 else (xs[n // 2] if n % 2 else 0.5 * (xs[n // 2 - 1] + xs[n // 2]))


DUMP_LIMIT_BYTES = 64_000_000


def _fit_outputs(la):
    """What ``la.fit()`` hands its caller, as (name, tensor) pairs: the loss and the curvature -- for kron the Kronecker
    factors and their eigenvalues, otherwise ``la.H`` itself (diag: [P]; last-layer full GGN: [P, P]).  The eigenvectors
    are left out: they follow from the factors, and where two eigenvalues lie close they differ from run to run (1e-2 in
    a column of the arxiv-shaped fit at a gap of 3e-4) without the fit being any different."""
    import torch
    import laplace_gnn_amd as lg

    out = [("loss", torch.as_tensor(la.loss).detach().reshape(()).double())]
    if isinstance(la.H, lg.KronDecomposed):
        for i, F in enumerate(la.H_facs.kfacs):
            for j, t in enumerate(F):
                out += [(f"kron_factor_{i}_{j}", t), (f"kron_eigenvalues_{i}_{j}", la.H.eigenvalues[i][j])]
    else:
        out.append(("hessian", la.H))
    return out


def _dump_outputs(pairs, out_dir, limit=DUMP_LIMIT_BYTES):
    """Write every (name, tensor) as ``out_dir/<name>.npy`` (float32 as computed, float64 for the loss).  Smallest first,
    each array gets an equal share of the byte budget that is left; one that does not fit its share is written as a fixed
    sample, ``<name>_sample.npy``: the rows (2-D) or entries (1-D) at sorted positions drawn by a generator seeded with 0."""
    import numpy as np
    import torch

    os.makedirs(out_dir, exist_ok=True)
    pairs = sorted(pairs, key=lambda p: p[1].numel() * p[1].element_size())
    left = limit - 4096 * len(pairs)  # (room for the .npy headers)
    written = {}
    for k, (name, t) in enumerate(pairs):
        t = t.detach()
        if t.dtype not in (torch.float32, torch.float64):
            t = t.float()
        share = left // (len(pairs) - k)
        if t.numel() * t.element_size() > share:
            row_bytes = (t[0].numel() if t.ndim > 1 else 1) * t.element_size()
            n = max(1, share // row_bytes)
            pick = torch.randperm(t.shape[0], generator=torch.Generator().manual_seed(0))[:n].sort().values
            t, name = t.index_select(0, pick.to(t.device)), name + "_sample"
        a = t.contiguous().cpu().numpy()
        np.save(os.path.join(out_dir, name + ".npy"), a)
        left -= a.nbytes
        written[name] = list(a.shape)
    return written


def _pmc_traffic(workload, structure, units_per_launch):
    """HBM-side bytes per launch of the dominant kernel from the committed rocprofv3 --pmc pass of this same command
    (counters cannot be collected inside the timed run); null when no summary for this workload is committed."""
    names = ["r04_arxiv_pmc_fused.json", "r03_arxiv_pmc_fused.json"] if (workload, structure) == ("arxiv", "kron") \
        else [f"r04_{workload}_pmc_dominant.json", f"r03_{workload}_pmc_dominant.json", f"r02_{workload}_pmc_dominant.json"]
    if structure != DEFAULT_STRUCTURE[workload]:
        names = []
    for name in names:
        path = os.path.join(ROOT, "profiles", name)
        if os.path.exists(path):
            with open(path) as fh:
                pj = json.load(fh)
            per = pj.get("planes_per_launch") or pj.get("units_per_launch") or units_per_launch
            if os.environ.get("LGNN_NO_PATHS", "") not in ("", "0") and "paths" in pj.get("kernel", ""):
                continue  # the committed counters are the path route's
            return (pj["traffic_bytes_per_launch"] * units_per_launch / per,
                    f"profiles/{name} ((2*FETCH_SIZE + WRITE_SIZE) KB, gfx950 correction)", pj)
    return None, None, None


def main():
    args = _parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world == 1 and args.gpus > 1:
        sys.exit(_launch_ranks(args))  # before anything touches the GPU
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")

    import torch
    import torch.distributed as dist

    assert torch.cuda.is_available(), "bench.py needs a GPU (no CPU fallback)"
    # one rank per GPU; LGNN_DIST_BACKEND=gloo lets several ranks share one GPU (rehearsal of the N > 1 code path on a
    # 1-GPU box: RCCL refuses two ranks on the same device)
    backend = os.environ.get("LGNN_DIST_BACKEND", "nccl")
    dev_index = local_rank if backend == "nccl" else local_rank % torch.cuda.device_count()
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    import laplace_gnn_amd as lg

    w, ei, X, train_idx, train_y = make_workload(args.workload, dev)
    torch.manual_seed(0)
    cls = lg.GraphSAGE if w.get("kind") == "sage" else lg.GCN
    model = cls(w["F"], w["H"], w["C"], w.get("layers", 2), X, ei, symmetric=True).to(dev)
    loader = lg.TensorBatchLoader(train_idx.to(dev), train_y.to(dev), batch_size=w["batch"])
    structure = args.structure or DEFAULT_STRUCTURE[args.workload]
    if structure == "lastlayer":
        la = lg.Laplace(model, "classification", subset_of_weights="last_layer", hessian_structure="full")
    else:
        la = lg.Laplace(model, "classification", subset_of_weights="all", hessian_structure=structure)
    eng = model.engine
    nnz, N, F, H, C = eng.nnz, w["N"], w["F"], w["H"], w["C"]
    # Diagonal fits are a dozen kernels of 3-40 us: a fit that repeats unchanged is captured into ONE hipGraph launch on its
    # second call (DiagLaplace.fit_graph) -- the same kernels on the same buffers, forward pass included.
    # --no-fit-graph times the launch-by-launch path.
    fit_graph = structure == "diag" and world == 1 and not args.no_fit_graph and args.emulate_world <= 1
    if fit_graph:
        la.fit_graph = True

    if args.emulate_world > 1:
        plan = la._shard_plan
        la._shard_plan = lambda tl, r, w_: plan(tl, 0, args.emulate_world)  # rank 0's share of an N-rank job

    ev = []  # (start, accumulated, end) device events per timed step, on torch's current stream = the launch stream

    red = []  # (reduce_begin, reduce_end) device events per timed step (N > 1)

    def step(timed=False):
        # A fresh fit: the forward pass and the activations' input Grams are recomputed.  What depends on the graph and X
        # only -- the padded copy of X, rowsum(P), P X and a GCN's first-layer X^T X (legal hoisting) --
        # survives lgnn_invalidate: 0.15 ms of an arxiv-shaped fit, ~0.06 ms (15 %) of a Cora-shaped one.
        eng.invalidate()
        model.__dict__.pop("_lgnn_eig_cache", None)  # no cached decomposition of a large factor (cora --structure kron)
        if timed:
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            la._on_accumulated = e[1].record
            if world > 1:
                r = {"reduce_begin": torch.cuda.Event(enable_timing=True), "reduce_end": torch.cuda.Event(enable_timing=True)}
                la._on_phase = lambda name: r[name].record()
                red.append(r)
        la.fit(loader)
        if timed:
            e[2].record()
            la._on_accumulated = None
            la._on_phase = None
            ev.append(e)

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    sync()
    if args.full and not fit_graph:
        eng.enable_kernel_timing(True)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step(timed=True)
    sync()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        _dump_outputs(_fit_outputs(la), args.dump_outputs)  # before anything below runs another fit
    kt_steps = args.steps
    launches, kern_ms, units, per_launch = 0, 0.0, 0, []
    if args.full:
        if fit_graph:
            # event records around the dominant kernel cannot live inside the replayed graph: its launch duration is measured
            # over three more fits of the launch-by-launch path right behind the timed region (same process, same buffers)
            eng.enable_kernel_timing(True)
            kt_steps = 3
            for _ in range(kt_steps):
                step()
            sync()
        launches, kern_ms, units = eng.kernel_timing()
        per_launch = eng.kernel_timing_launches() if hasattr(eng, "kernel_timing_launches") else []
        eng.enable_kernel_timing(False)
    step_ms = [e[0].elapsed_time(e[2]) for e in ev]
    acc_ms = [e[0].elapsed_time(e[1]) for e in ev]
    dist_info = None
    if world > 1:
        # evidence that the collective saw N ranks: the backend's name, an all-reduce of ones, the all-reduce's own device
        # time (events around all_reduce_flat_ on the launch stream) and the spread of the per-rank accumulate times
        ar_ms = _median([r["reduce_begin"].elapsed_time(r["reduce_end"]) for r in red])
        t = torch.tensor([elapsed, _median(step_ms), _median(acc_ms), ar_ms, -_median(acc_ms)], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed, step_med, acc_med, ar_max, neg_acc_min = (float(v) for v in t.tolist())
        ones = torch.ones(1, device=dev)
        dist.all_reduce(ones)
        dist_info = {"dist_backend": dist.get_backend(), "ranks_seen": int(round(float(ones.item()))),
                     "allreduce_ms": ar_max, "accumulate_ms_min": -neg_acc_min, "accumulate_ms_max": acc_med,
                     "allreduce_floats": (sum(i * i + o * o for i, o in eng.block_dims) + 2) if structure == "kron" else None,
                     "devices": torch.cuda.device_count()}
    else:
        step_med, acc_med = _median(step_ms), _median(acc_ms)

    if rank == 0:
        value = args.steps * w["n_train"] / elapsed
        roofline = None
        if launches > 0 and kern_ms > 0:
            avg_ms = kern_ms / launches
            upl = units / launches
            traffic, traffic_src, pmc = _pmc_traffic(args.workload, structure, upl)
            common = {"traffic": traffic, "traffic_source": traffic_src, "launches": launches, "avg_launch_ms": avg_ms,
                      "kernel_share_of_wall": (kern_ms / kt_steps) * 1e-3 / (elapsed / args.steps)}
            if fit_graph:
                common["launch_timing"] = (f"{kt_steps} launch-by-launch fits right behind the timed region (the timed fits are "
                                           "replays of one captured hipGraph, which cannot hold the event records)")
            if structure == "kron":
                # dominant kernel: fused SpMM^T -> Gram of layer 0.  ALGORITHMIC flops per class plane:
                # SpMM 2*nnz*H + Gram 2*N*H^2 (no credit for symmetry); bytes per plane (fused, nothing written):
                # nnz*8 + (N+1)*4 + N*H*4.  The MFMA floor is the higher one => "mfma" bound.
                flops = (2.0 * nnz * H + 2.0 * N * H * H) * units
                bytes_ = (nnz * 8.0 + (N + 1) * 4.0 + N * H * 4.0) * units
                ach = flops / (kern_ms * 1e-3) / 1e12
                # which route a FULL batch takes (2-layer GCN: B_0 from the batch's two-hop paths, no class planes -- unless the
                # graph's hubs make the planes cheaper; a short last batch may take the other route): one untimed accumulate
                _, pv, pl = eng.new_kfac_buffers()
                xb, yb = next(iter(loader))
                eng.kfac_accumulate(xb, yb, w["n_train"], pv, pl)
                paths = eng.last_kfac_used_paths
                # The last batch of a fit is short (arxiv: 941 of 10 000 samples): its launch is cheaper, yet SURVEY.md 8(d) credits
                # it the same N-row work.  `achieved` / `frac` therefore count the FULL batches' launches only (the stricter
                # reading: VERDICT r3 recomputed 0.77 where the blended average gave 0.82); the blended figure is kept beside it.
                T = len(loader)
                full_ms = last_ms = None
                if per_launch and len(per_launch) == args.steps * T and T > 1 and w["n_train"] % w["batch"]:
                    fl = [t for i, t in enumerate(per_launch) if i % T != T - 1]
                    ll = [t for i, t in enumerate(per_launch) if i % T == T - 1]
                    full_ms, last_ms = sum(fl) / len(fl), sum(ll) / len(ll)
                    common.update({"full_batch_launch_ms": full_ms, "last_batch_launch_ms": last_ms,
                                   "frac_all_launches": ach / PEAK_MFMA_F32_TFLOPS})
                    ach = flops / launches / (full_ms * 1e-3) / 1e12
                roofline = {"bound": "mfma", "achieved": ach, "peak": PEAK_MFMA_F32_TFLOPS, "unit": "TFLOP/s",
                            "frac": ach / PEAK_MFMA_F32_TFLOPS, **common,
                            "kernel": "paths_fused_kernel" if paths else ("spmm_gram256_kernel" if H > 128 else "spmm_gram_kernel"),
                            "planes_per_launch": upl, "algorithmic_bytes_per_launch": bytes_ / launches,
                            "algorithmic_GBps": bytes_ / (kern_ms * 1e-3) / 1e9}
                if paths:
                    # executed work: the 36 of 64 symmetric sub-tiles of every node's Gram plus the three path products
                    # (incl. their tile padding); measured, not modelled: SQ_VALU_MFMA_BUSY_CYCLES of the committed counter
                    # pass x 64 flop per busy cycle and SIMD, over this run's launch time
                    busy = (pmc or {}).get("SQ_VALU_MFMA_BUSY_CYCLES_avg")
                    per = (pmc or {}).get("planes_per_launch", upl)
                    t_ms = avg_ms
                    # the counter pass keeps the template instances apart: <false> = the full batches' launches, <true> = the
                    # short last batch's (node list); the full batches' busy cycles go over the full batches' launch time
                    inst = {("<true>" in i["kernel"]): i for i in (pmc or {}).get("instances", [])}
                    if full_ms and False in inst and "SQ_VALU_MFMA_BUSY_CYCLES_avg" in inst[False]:
                        busy, t_ms = inst[False]["SQ_VALU_MFMA_BUSY_CYCLES_avg"], full_ms
                        if True in inst and last_ms and "SQ_VALU_MFMA_BUSY_CYCLES_avg" in inst[True]:
                            roofline["last_batch_executed_frac_of_peak"] = (inst[True]["SQ_VALU_MFMA_BUSY_CYCLES_avg"] * 64.0
                                                                          / (last_ms * 1e-3) / 1e12 / PEAK_MFMA_F32_TFLOPS)
                    exe = busy * 64.0 * (upl / per) / (t_ms * 1e-3) / 1e12 if busy else None
                    roofline.update({
                        "executed_TFLOPs": exe, "executed_frac_of_peak": exe / PEAK_MFMA_F32_TFLOPS if exe else None,
                        "note": "'achieved' credits the SURVEY.md 8(d) count of what the kernel replaces (C planes x (2 nnz H + 2 N "
                                "H^2), no credit for symmetry); executed_* = matrix-pipe busy cycles (rocprofv3 counter pass of "
                                "this command, profiles/) x 64 flop, full batches' launches over their own time: the kernel runs "
                                "the upper triangle of every node's Gram plus the path products; its HBM traffic is below the algorithmic bytes because no class plane exists"})
                else:
                    roofline.update({
                        "executed_frac_of_peak": ach / PEAK_MFMA_F32_TFLOPS * 36.0 / 64.0 if H > 128 else None,
                        "note": "the kernel executes the 36 of 64 symmetric 32x32 sub-tiles of the Gram; 'achieved' "
                                "credits the full 2*N*H^2 as SURVEY.md 8(d) prescribes"
                                + ("; GraphSAGE: it also visits only the rows that can be non-zero (batch nodes and "
                                   "their neighbours), so frac can exceed 1 and executed_frac_of_peak overstates by the "
                                   "share of skipped rows" if w.get("kind") == "sage" else "")})
            elif structure == "diag":
                # dominant kernel: the first-layer contraction (GCN: diag_first_layer_tile_kernel on wide inputs, else
                # diag_first_layer_mfma_kernel; GraphSAGE:
                # diag_first_layer_kernel<1>), one launch per batch.  ALGORITHMIC bytes per launch (SURVEY.md 8(d)
                # "Diag (C2)"): N*F*4 + nnz*8 + 2*P*4; flops 2*M*dbar*H*(F+1).  HBM bound by that count (in practice latency
                # bound: ~16 MB per launch; DESIGN.md has the phase breakdown).
                P = eng.n_params
                bytes_l = N * F * 4.0 + nnz * 8.0 + 2.0 * P * 4.0
                ach = bytes_l * launches / (kern_ms * 1e-3) / 1e9
                roofline = {"bound": "hbm", "achieved": ach, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                            "frac": ach / PEAK_HBM_GBS, **common,
                            "kernel": "diag_first_layer_kernel<1>" if w.get("kind") == "sage"
                            else ("diag_first_layer_tile_kernel" if (F + 1 + 191) // 192 >= 4 and H % 4 == 0 else "diag_first_layer_mfma_kernel"),
                            "samples_per_launch": upl, "algorithmic_bytes_per_launch": bytes_l,
                            "algorithmic_TFLOPs": 2.0 * units * (nnz / N) * H * (F + 1) / (kern_ms * 1e-3) / 1e12}
            else:
                # dominant kernel: batched weighted Gram (gram_mem_kernel<128>, one launch per chunk of class pairs).
                # ALGORITHMIC flops per batch (SURVEY.md 8(d) "LL full"): 2*M*C^2*(D+1)^2, no credit for symmetry;
                # executed: C(C+1)/2 pair Grams on their upper 128x128 tile pairs, 2*M*D^2 * (ntile+1)/(2*ntile) each.
                D = eng.in_dims[-1]
                nb = len(loader)
                samples = args.steps * w["n_train"] // max(world, 1) if world > 1 else args.steps * w["n_train"]
                flops = 2.0 * samples * C * C * (D + 1.0) ** 2
                nt = -(-D // 128)
                executed = 2.0 * samples * D * D * (nt + 1) / (2.0 * nt) * (C * (C + 1) / 2)
                ach = flops / (kern_ms * 1e-3) / 1e12
                exe = executed / (kern_ms * 1e-3) / 1e12
                roofline = {"bound": "mfma", "achieved": ach, "peak": PEAK_MFMA_F32_TFLOPS, "unit": "TFLOP/s",
                            "frac": ach / PEAK_MFMA_F32_TFLOPS, **common, "kernel": "gram_mem_kernel<128> (batched, weighted)",
                            "class_pairs_per_launch": upl, "executed_TFLOPs": exe,
                            "executed_frac_of_peak": exe / PEAK_MFMA_F32_TFLOPS,
                            "algorithmic_bytes_per_launch": (w["batch"] * (D + 1 + C) * 4.0) + upl * D * D * 4.0,
                            "note": "'achieved' credits 2*M*C^2*(D+1)^2 per batch as SURVEY.md 8(d) prescribes; the kernel "
                                    "executes only the pairs c <= c' and the upper tiles of each block (about a quarter), "
                                    "so frac can exceed 1 -- executed_frac_of_peak is the matrix-pipe utilisation"}
        gname = "GraphSAGE" if w.get("kind") == "sage" else "GCN"
        out = {
            "metric": {"kron": f"la.fit() samples/sec ({gname}, KFAC)",
                       "diag": f"la.fit() samples/sec ({gname}, diag GGN)",
                       "lastlayer": f"la.fit() samples/sec ({gname}, last-layer full GGN)"}[structure],
            "value": value, "unit": "samples/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "strong",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "ms_per_step_median": step_med, "accumulate_ms": acc_med,
            "config": {
                "workload": f"{args.workload}-shaped {w.get('layers', 2)}-layer {w.get('kind', 'gcn').upper()}, "
                            f"hessian_structure={structure} "
                            + (f"(BASELINE configs[{BASELINE_CONFIG[args.workload]}])"
                               if args.workload in BASELINE_CONFIG and structure == DEFAULT_STRUCTURE[args.workload]
                               else "(not a BASELINE config)"),
                "num_nodes": N, "nnz": nnz, "features": F, "hidden": H, "classes": C,
                "n_train": w["n_train"], "batch_size": w["batch"],
                "batches": len(loader),
                **({"fit_graph": "every timed la.fit() is one replay of the hipGraph captured on the second warm-up fit "
                                 "(DiagLaplace.fit_graph): the same kernels, forward pass included"} if fit_graph else {}),
                "parallelism": f"dp{world} (" + ("(batch, class) units, contiguous balanced runs" if structure == "kron"
                                                  else "sample slices of every batch") + ")",
            },
            "roofline": roofline,
        }
        if dist_info is not None:
            out["dist"] = dist_info
        if args.full and world == 1 and not args.no_cpu_baseline and not args.emulate_world:
            Ws = [c.lin.weight.detach().cpu().numpy() for c in model.convs]
            bs = [c.lin.bias.detach().cpu().numpy() for c in model.convs]
            out["cpu_baseline"] = cpu_baseline(args.workload, ei, X, Ws, bs, train_idx, train_y, w, structure, model)
            if args.workload == "cora":
                out["cpu_baseline_dense"] = cpu_baseline_dense(ei, X, Ws, bs, train_idx, train_y, w, structure)
        else:
            out["cpu_baseline"] = None
        if args.emulate_world > 1:
            out = {"emulated_rank0_of": args.emulate_world, "ms_per_rank_step": elapsed / args.steps * 1e3,
                   "implied_samples_per_s": value, "note": "not a bench line: one rank's share, no all-reduce"}
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
