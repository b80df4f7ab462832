"""dev: the adjacency gradient under the full posterior at a Cora-like shape (N = 2 708, ~13 k stored entries, F = 1 433, H = 16,
C = 7, one batch of M = 140 samples: P = 23 063, Gamma 2.1 GB, 2 M C P^2 = 1.04 TFLOP for the product) -- DESIGN 12.17.

Device events around synchronised work, 2 warm-up rounds, median [min .. max] over the timed rounds.  Every round runs, in this
order: the Jacobians, lgnn_full_directions (Jacobians + the fused product kernel), the alternative the kernel replaces (rocBLAS
sgemm into a Z buffer + a batched K_n = Z_n J_n^T + the Lambda mix as separate passes, on the same inputs), that sgemm alone, one
lgnn_full_adjgrad_batch and the finish -- so the fused kernel and the alternative alternate inside one process.  The product
kernel's time is full_directions minus the Jacobians of the same round, the tangent / reverse chain's is the batch call minus
full_directions.  At the end two whole FullLaplace.neg_marglik_adj_grad calls.  Prints one JSON line and writes it to
$LGNN_OUT_DIR (default out/) as full_adjgrad_cora.json."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
import laplace_gnn_amd as lg  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
H, M = 16, 140


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def spread(xs):
    return dict(median_ms=statistics.median(xs), min_ms=min(xs), max_ms=max(xs), n=len(xs))


w, ei, X, tri, try_ = bench.make_workload("cora", "cuda")
torch.manual_seed(0)
model = lg.GCN(w["F"], H, w["C"], 2, X, ei, symmetric=True).to("cuda").eval()
eng = model.engine
idx, y = tri[:M].cuda(), try_[:M].cuda()
loader = lg.TensorBatchLoader(idx, y, batch_size=M)
C, P, N = w["C"], eng.n_params, w["N"]
la = lg.FullLaplace(model, "classification", prior_precision=1.0)
la.fit(loader)
t_fit = [timed(lambda: la.fit(loader))[0] for _ in range(3)]


t_gamma = []
for _ in range(2):
    ms, Gamma = timed(la._adj_gamma)
    t_gamma.append(ms)

p = torch.softmax(eng.forward(idx), 1)


def alternative(J):
    Z = torch.matmul(J.reshape(M * C, P), Gamma).reshape(M, C, P)
    Kn = torch.bmm(Z, J.transpose(1, 2))
    R = 2.0 * p[:, :, None] * (Z - (p[:, :, None] * Z).sum(1, keepdim=True))
    return Kn, R


def buffers():
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")  # noqa: E731
    return z(eng.nnz), z(N, C), z(N, H), z(N, w["F"] + 1)


eng.set_likelihood("classification")
rows = dict(jacobians=[], full_directions=[], product=[], alternative=[], sgemm_alone=[], batch=[], chain=[], finish=[], ratio=[])
check = None
for rnd in range(ROUNDS + 2):
    t_j, (J, _) = timed(lambda: eng.jacobians(idx))
    t_d, (Kn, R) = timed(lambda: eng.full_directions(idx, Gamma))
    t_a, (Ka, Ra) = timed(lambda: alternative(J))
    t_g, _ = timed(lambda: torch.matmul(J.reshape(M * C, P), Gamma))
    bufs = buffers()
    t_b, _ = timed(lambda: eng.full_adjgrad_batch(idx, y, Gamma, *bufs, loss_scale=1.0))
    t_f, grad = timed(lambda: eng.diag_adjgrad_finish(bufs[1], bufs[2], bufs[3], bufs[0]))
    if check is None:  # the two routes compute the same thing
        check = dict(R_fused_vs_alternative=float((R - Ra).norm() / Ra.norm()), K_fused_vs_alternative=float((Kn - Ka).norm() / Ka.norm()))
    del J, Kn, R, Ka, Ra
    if rnd < 2:
        continue
    for k, v in (("jacobians", t_j), ("full_directions", t_d), ("product", t_d - t_j), ("alternative", t_a), ("sgemm_alone", t_g),
                 ("batch", t_b),
                 ("chain", t_b - t_d), ("finish", t_f), ("ratio", (t_d - t_j) / t_a)):
        rows[k].append(v)
eng.check_async_errors()

flop = 2.0 * M * C * P * P
prod = spread(rows["product"])
tf = lambda ms: flop / (ms * 1e-3) / 1e12  # noqa: E731
out = dict(shape=dict(N=N, nnz=int(eng.nnz), F=w["F"], H=H, C=C, M=M, P=P, gamma_bytes=4 * P * P, product_flop=flop),
           fit=spread(t_fit), gamma_build=spread(t_gamma), **{k: spread(v) for k, v in rows.items() if k != "ratio"},
           fused_over_alternative=dict(median=statistics.median(rows["ratio"]), min=min(rows["ratio"]), max=max(rows["ratio"])),
           product_tflops=tf(prod["median_ms"]),
           product_share_of_fp32_mfma_peak=tf(prod["median_ms"]) / bench.PEAK_MFMA_F32_TFLOPS,
           alternative_tflops_incl_its_passes=tf(statistics.median(rows["alternative"])),
           sgemm_alone_tflops=tf(statistics.median(rows["sgemm_alone"])), check=check, grad_abs_sum=float(grad.abs().sum()))
odir = os.environ.get("LGNN_OUT_DIR", os.path.join(ROOT, "out"))
os.makedirs(odir, exist_ok=True)


def write():
    line = json.dumps(out)
    with open(os.path.join(odir, "full_adjgrad_cora.json"), "w") as fh:
        fh.write(line + "\n")
    return line


write()  # the rounds are on disk before the two whole calls run
del Gamma
out["neg_marglik_adj_grad"] = spread([timed(lambda: la.neg_marglik_adj_grad(loader))[0] for _ in range(2)])
eng.check_async_errors()
print(write())
