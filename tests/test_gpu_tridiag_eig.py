"""tridiag_dc_kernel (csrc/eigh.hip): Cuppen's divide and conquer with the Gu-Eisenstat vector fix on the
tridiagonal matrices that tridiag256_kernel leaves, one workgroup per matrix, in place of the rocsolver_sstedc chains.

The bounds are the project's existing ones for a decomposition (tests/test_gpu_frontend.py, tools/time_eigh.py): eigenvalues
within 1e-5 of the largest against fp64, max|Q^T Q - I| < 1e-4, relative reconstruction < 1e-5, eigenvalues ascending.

`merge_f32` below restates ONE merge in float32 numpy (tearing, sort, deflation with LAPACK's tolerance, shifted bisection
with 32 steps, the recomputed update vector, the eigenvector product): it is the specification the kernel is read against and
is held to the same three bounds without a GPU."""
import functools

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
f32 = np.float32
EPS = f32(np.finfo(np.float32).eps) / f32(2)  # LAPACK's slamch('E')
BISECT_STEPS = 32


# ---- the float32 restatement of one merge ---------------------------------------------------------------------------------
def merge_f32(lam1, Q1, lam2, Q2, e_split):
    """Eigenpairs of blockdiag(T1', T2') + rho v v^T from those of the torn halves: T1' = Q1 diag(lam1) Q1^T is the upper half
    with rho = |e_split| taken off its last diagonal entry, T2' the lower half with rho taken off its first one, v = e_last +
    sign(e_split) e_first.  Eigenvectors in columns; returns (eigenvalues, eigenvectors), NOT sorted (the next level sorts)."""
    n1, n2 = len(lam1), len(lam2)
    m = n1 + n2
    rho = f32(abs(e_split))
    sgn = f32(1.0) if e_split >= 0 else f32(-1.0)
    Q = np.zeros((m, m), f32)
    Q[:n1, :n1], Q[n1:, n1:] = Q1, Q2
    D = np.concatenate([lam1, lam2]).astype(f32)
    z = np.concatenate([Q1[-1, :], sgn * Q2[0, :]]).astype(f32)
    child = np.concatenate([np.ones(n1, np.int32), np.full(n2, 2, np.int32)])
    nrm2 = f32(np.sum(z * z, dtype=f32))
    if rho == 0 or nrm2 == 0:
        return D, Q
    z = z / np.sqrt(nrm2)
    rho = rho * nrm2
    order = np.argsort(D, kind="stable")
    D, z, Q, child = D[order], z[order], Q[:, order], child[order]
    tol = f32(8.0) * EPS * max(np.abs(D).max(), np.abs(z).max())
    # deflation: tiny components, then close pairs (one serial recurrence over the survivors)
    keep, prev = [], -1
    for p in range(m):
        if rho * abs(z[p]) <= tol:
            continue
        if prev >= 0:
            s, c = z[prev], z[p]
            t = D[p] - D[prev]
            tau2 = f32(c * c + s * s)
            if abs(t * c * s) <= tol * tau2:  # |t c s| <= tol for the rotation c / tau, -s / tau
                tau = f32(np.sqrt(tau2))
                c, s = c / tau, -s / tau
                z[p], z[prev] = tau, f32(0)
                qa, qb = Q[:, prev].copy(), Q[:, p].copy()
                Q[:, prev] = c * qa + s * qb
                Q[:, p] = c * qb - s * qa
                da, db = D[prev], D[p]
                D[prev] = da * c * c + db * s * s
                D[p] = da * s * s + db * c * c
                prev = p
                continue
            keep.append(prev)
        prev = p
    if prev >= 0:
        keep.append(prev)
    keep = np.array(keep, np.int64)
    gone = np.setdiff1d(np.arange(m), keep)
    k = len(keep)
    if k == 0:
        return D, Q
    d, zs = D[keep], z[keep]
    z2 = zs * zs
    # secular roots: root j in (d_j, d_j+1), the last in (d_k-1, d_k-1 + rho); origin = the nearer pole, unknown = the offset mu
    gap = np.concatenate([d[1:] - d[:-1], [rho]]).astype(f32)
    half = f32(0.5) * gap

    def secular(org, mu):  # 1 + rho sum_i z_i^2 / ((d_i - d_org) - mu), one row per root
        delta = (d[None, :] - d[org][:, None]) - mu[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            return f32(1.0) + rho * np.sum(z2[None, :] / delta, axis=1, dtype=f32)

    j = np.arange(k)
    with np.errstate(invalid="ignore"):
        left = secular(j, half) > 0  # the root lies in the left half: origin d_j
    left[k - 1] = True
    org = np.where(left, j, np.minimum(j + 1, k - 1))
    a = np.where(left, f32(0), -half).astype(f32)
    b = np.where(left, half, f32(0)).astype(f32)
    a[k - 1], b[k - 1] = f32(0), gap[k - 1]
    for _ in range(BISECT_STEPS):
        mid = f32(0.5) * (a + b)
        with np.errstate(invalid="ignore"):
            pos = secular(org, mid) > 0
        b = np.where(pos, mid, b)
        a = np.where(pos, a, mid)
    mu = f32(0.5) * (a + b)
    lam = d[org] + mu
    # Gu-Eisenstat: the update vector for which the computed roots are exact, as a product of ratios of shifted differences
    num = (d[org][None, :] - d[:, None]) + mu[None, :]          # lam_j - d_i, [i, j]
    den = d[None, :] - d[:, None]                               # d_j - d_i
    np.fill_diagonal(den, f32(1))
    ratio = (num / den).astype(f32)
    zh2 = np.prod(ratio, axis=1, dtype=f32) / rho
    zh = np.copysign(np.sqrt(np.abs(zh2)), zs).astype(f32)
    U = zh[:, None] / ((d[:, None] - d[org][None, :]) - mu[None, :])     # u_j[i], column j
    U = (U / np.sqrt(np.sum(U * U, axis=0, dtype=f32))).astype(f32)
    Qn = np.empty_like(Q)
    Qn[:, :k] = Q[:, keep] @ U
    Qn[:, k:] = Q[:, gone]
    return np.concatenate([lam, D[gone]]).astype(f32), Qn


def _tridiag(d, e):
    return np.diag(d) + np.diag(e, 1) + np.diag(e, -1)


def _bounds(d, e, lam, Q):
    """(eigenvalue error / largest, orthogonality, relative reconstruction) of eigenvalues lam / eigenvector COLUMNS Q against
    the fp64 decomposition of the same tridiagonal matrix."""
    T = _tridiag(np.asarray(d, np.float64), np.asarray(e, np.float64))
    ref = np.linalg.eigvalsh(T)
    lam, Q = np.asarray(lam, np.float64), np.asarray(Q, np.float64)
    scale = max(np.abs(ref).max(), 1e-300)
    nrm = max(np.linalg.norm(T), 1e-300)
    return (np.abs(lam - ref).max() / scale, np.abs(Q.T @ Q - np.eye(len(lam))).max(),
            np.linalg.norm((Q * lam) @ Q.T - T) / nrm)


def _wilkinson(m=10):
    return np.abs(np.arange(-m, m + 1)).astype(f32), np.ones(2 * m, f32)


def _cases(n, seed=0):
    """{name: (d, e)} float32, e of length n - 1."""
    g = np.random.default_rng(seed + n)
    out = {}
    d, e = g.standard_normal(n).astype(f32), g.standard_normal(max(n - 1, 0)).astype(f32)
    out["random"] = (d, e)
    ez = e.copy()
    ez[::3] = 0
    out["zeros_in_e"] = (d, ez)
    out["e_all_zero"] = (d, np.zeros_like(e))
    out["identity"] = (np.ones(n, f32), np.zeros_like(e))
    out["cluster"] = ((1 + 1e-6 * g.standard_normal(n)).astype(f32), (1e-6 * g.standard_normal(max(n - 1, 0))).astype(f32))
    grade = np.logspace(0, -3, n).astype(f32)
    out["graded"] = (grade * g.standard_normal(n).astype(f32), (grade[:-1] * g.standard_normal(max(n - 1, 0))).astype(f32))
    return out


def _special_cases():
    wd, we = _wilkinson()
    out = {"wilkinson21": (wd, we)}
    out["wilkinson_glued"] = (np.concatenate([wd, wd]), np.concatenate([we, [f32(1e-6)], we]).astype(f32))
    return out


@pytest.mark.parametrize("n", [2, 3, 7, 40, 127, 128])
def test_one_merge_in_float32_numpy_meets_the_bounds(n):
    cases = dict(_cases(n))
    if n == 40:
        cases.update(_special_cases())
    for name, (d, e) in cases.items():
        m, s = len(d), len(d) // 2
        rho = f32(abs(e[s - 1]))
        d1, d2 = d[:s].copy(), d[s:].copy()
        d1[-1] -= rho
        d2[0] -= rho
        l1, Q1 = np.linalg.eigh(_tridiag(d1.astype(np.float64), e[:s - 1].astype(np.float64)))
        l2, Q2 = np.linalg.eigh(_tridiag(d2.astype(np.float64), e[s:].astype(np.float64)))
        lam, Q = merge_f32(l1.astype(f32), Q1.astype(f32), l2.astype(f32), Q2.astype(f32), e[s - 1])
        order = np.argsort(lam, kind="stable")
        ev, orth, rec = _bounds(d, e, lam[order], Q[:, order])
        print(f"n={m} {name}: lam {ev:.1e} orth {orth:.1e} rec {rec:.1e}")
        assert ev < 1e-5 and orth < 1e-4 and rec < 1e-5, (name, ev, orth, rec)


# ---- the kernel, through lgnn_tridiag_eig ---------------------------------------------------------------------------------
def _tridiag_eig(ds, es):
    """One batched lgnn_tridiag_eig call: [(d, e)] of one size -> (eigenvalues [B, n], Z [B, n, n] (row j = vector j), info)."""
    from laplace_gnn_amd import _lib
    lib = _lib.load()
    n, B = len(ds[0]), len(ds)
    d = torch.tensor(np.stack(ds), dtype=torch.float32, device="cuda")
    e = torch.zeros(B, n, dtype=torch.float32, device="cuda")
    if n > 1:
        e[:, :n - 1] = torch.tensor(np.stack(es), dtype=torch.float32, device="cuda")
    Z = torch.full((B, n, n), float("nan"), dtype=torch.float32, device="cuda")
    info = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.lgnn_tridiag_eig(d.data_ptr(), e.data_ptr(), n, B, Z.data_ptr(), info.data_ptr(), stream), "lgnn_tridiag_eig")
    torch.cuda.synchronize()
    return d.cpu().numpy(), Z.cpu().numpy(), info.cpu().numpy()


@gpu
@pytest.mark.parametrize("n", [1, 2, 3, 5, 7, 40, 127, 128, 255, 256])
def test_tridiag_eig_meets_the_bounds(n):
    cases = _cases(n)
    names = list(cases)
    lam, Z, info = _tridiag_eig([cases[k][0] for k in names], [cases[k][1] for k in names])
    lam2, Z2, _ = _tridiag_eig([cases[k][0] for k in names], [cases[k][1] for k in names])
    assert np.array_equal(lam, lam2) and np.array_equal(Z, Z2)  # no atomics, a stable sort: two calls are bit-equal
    for b, name in enumerate(names):
        d, e = cases[name]
        assert info[b] == 0
        assert np.all(np.diff(lam[b]) >= 0), name
        ev, orth, rec = _bounds(d, e, lam[b], Z[b].T)
        print(f"n={n} {name}: lam {ev:.1e} orth {orth:.1e} rec {rec:.1e}")
        assert ev < 1e-5 and orth < 1e-4 and rec < 1e-5, (name, ev, orth, rec)


@gpu
def test_tridiag_eig_wilkinson_pairs():
    for name, (d, e) in _special_cases().items():
        lam, Z, info = _tridiag_eig([d], [e])
        assert info[0] == 0 and np.all(np.diff(lam[0]) >= 0)
        ev, orth, rec = _bounds(d, e, lam[0], Z[0].T)
        print(f"{name}: lam {ev:.1e} orth {orth:.1e} rec {rec:.1e}")
        assert ev < 1e-5 and orth < 1e-4 and rec < 1e-5, (name, ev, orth, rec)


@gpu
def test_tridiag_eig_flags_a_nan_for_its_matrix_only():
    n = 40
    cases = _cases(n)
    d0, e0 = cases["random"]
    bad = d0.copy()
    bad[17] = np.nan
    inf_e = e0.copy()
    inf_e[3] = np.inf
    lam, Z, info = _tridiag_eig([d0, bad, d0, d0], [e0, e0, inf_e, e0])
    assert info.tolist() == [0, 1, 1, 0]
    for b in (0, 3):
        ev, orth, rec = _bounds(d0, e0, lam[b], Z[b].T)
        assert ev < 1e-5 and orth < 1e-4 and rec < 1e-5
    assert np.array_equal(lam[0], lam[3]) and np.array_equal(Z[0], Z[3])


# ---- through symeig_batched_hip ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _factor_set():
    """The factors of tools/time_eigh.py: (256, 256), (256, 200) with exact dependence, (128, 128), (40, 39)."""
    torch.manual_seed(0)
    mats = []
    for n, rank in ((256, 256), (256, 200), (128, 128), (40, 39)):
        G = torch.randn(4000, n, device="cuda", dtype=torch.float64) * torch.logspace(0, -3, n, device="cuda", dtype=torch.float64)
        if rank < n:
            G[:, rank:] = G[:, :n - rank] * 0.5 + G[:, 1:n - rank + 1]
        mats.append((G.T @ G / 4000).float())
    return tuple(mats)


@gpu
def test_symeig_batched_on_the_arxiv_shaped_factor_set():
    from laplace_gnn_amd.matrix import symeig_batched_hip
    mats = list(_factor_set())
    first = symeig_batched_hip(mats)
    second = symeig_batched_hip(mats)
    for H, (lam, Q), (lam2, Q2) in zip(mats, first, second):
        assert torch.equal(lam, lam2) and torch.equal(Q, Q2)
        n = H.shape[0]
        ref = torch.linalg.eigvalsh(H.double()).clamp(min=0)
        ev = float((lam.double() - ref).abs().max() / ref.max())
        rec = float(((Q * lam) @ Q.T - H).norm() / H.norm())
        orth = float((Q.T @ Q - torch.eye(n, device="cuda")).abs().max())
        print(f"n={n}: lam {ev:.1e} orth {orth:.1e} rec {rec:.1e}")
        assert bool((lam[1:] >= lam[:-1]).all())
        assert ev < 1e-5 and orth < 1e-4 and rec < 1e-5, (n, ev, orth, rec)


@gpu
def test_short_kron_fit_eigenvalues_match_float64():
    """N = 300, F = 8, batches of 60 (the size of tests/test_gpu_alpha_bf16.py): every factor's eigenvalues of the fit's own
    decomposition within 1e-5 lambda_max of fp64 eigvalsh of la.H_facs."""
    import laplace_gnn_amd as lg
    g = torch.Generator().manual_seed(0)
    N, F, H, C, M = 300, 8, 16, 5, 120
    ei = torch.randint(0, N, (2, 900), generator=g)
    X = torch.randn(N, F, generator=g)
    torch.manual_seed(0)
    model = lg.GCN(F, H, C, 2, X, ei, symmetric=True).to("cuda")
    idx = torch.randperm(N, generator=g)[:M]
    y = torch.randint(0, C, (M,), generator=g)
    loader = lg.TensorBatchLoader(idx.to("cuda"), y.to("cuda"), batch_size=60)
    la = lg.Laplace(model, "classification", subset_of_weights="all", hessian_structure="kron")
    la.fit(loader)
    dec = la.H_facs.decompose()
    checked = 0
    for facs, lams in zip(la.H_facs.kfacs, dec.eigenvalues):
        for Hf, lam in zip(facs, lams):
            ref = torch.linalg.eigvalsh(Hf.double()).clamp(min=0)
            err = float((lam.double() - ref).abs().max() / ref.max())
            assert err < 1e-5, (tuple(Hf.shape), err)
            checked += 1
    assert checked >= 4
