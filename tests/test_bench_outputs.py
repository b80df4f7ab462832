"""``bench.py --dump-outputs`` without a GPU: what ``_fit_outputs`` takes from a fitted front (the real ``HipGGN`` backend on
the CPU oracle engine) and what ``_dump_outputs`` writes -- names, dtypes, values, the byte budget and its seeded sample."""
import os

import numpy as np
import torch
from torch.utils.data import DataLoader, TensorDataset

from conftest import GOLDEN

import bench
import laplace_gnn_amd as lg
from test_host_logic import _cpu_model


def _fit(structure):
    g = np.load(os.path.join(GOLDEN, "gcn_small_3batch_s1.npz"))
    la = lg.Laplace(_cpu_model(g), "classification", subset_of_weights="all", hessian_structure=structure,
                    backend=lg.HipGGN)
    la.fit(DataLoader(TensorDataset(torch.from_numpy(g["train_idx"]), torch.from_numpy(g["train_y"])),
                      batch_size=int(g["batch_size"]), shuffle=False))
    return la


def test_dump_outputs_of_a_kron_fit(tmp_path):
    la = _fit("kron")
    written = bench._dump_outputs(bench._fit_outputs(la), str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in written)
    loss = np.load(tmp_path / "loss.npy")
    assert loss.dtype == np.float64 and loss.shape == () and float(loss) == float(la.loss)
    n = 0
    for i, F in enumerate(la.H_facs.kfacs):
        for j, t in enumerate(F):
            f = np.load(tmp_path / f"kron_factor_{i}_{j}.npy")
            lam = np.load(tmp_path / f"kron_eigenvalues_{i}_{j}.npy")
            assert f.dtype == lam.dtype == np.float32
            assert np.array_equal(f, t.numpy()) and np.array_equal(lam, la.H.eigenvalues[i][j].numpy())
            # the factor's spectrum (symeig clamps at 0)
            ref = np.clip(np.linalg.eigvalsh(f.astype(np.float64)), 0, None)
            np.testing.assert_allclose(np.sort(lam), ref, atol=1e-4 * max(float(np.abs(f).max()), 1e-30))
            n += 1
    assert len(written) == 1 + 2 * n


def test_dump_outputs_keeps_to_the_byte_budget_with_a_seeded_sample(tmp_path):
    la = _fit("diag")
    big = torch.arange(5000 * 300, dtype=torch.float32).reshape(5000, 300)  # 6 MB: over a 1 MiB budget
    pairs = bench._fit_outputs(la) + [("big", big)]
    limit = 2 ** 20
    written = bench._dump_outputs(pairs, str(tmp_path / "a"), limit=limit)
    bench._dump_outputs(pairs, str(tmp_path / "b"), limit=limit)
    assert set(written) == {"loss", "hessian", "big_sample"}
    assert sum(os.path.getsize(tmp_path / "a" / (k + ".npy")) for k in written) <= limit
    assert np.array_equal(np.load(tmp_path / "a" / "hessian.npy"), la.H.numpy())  # small outputs are written whole
    s = np.load(tmp_path / "a" / "big_sample.npy")
    rows = s[:, 0].astype(np.int64) // 300
    assert s.shape[1] == 300 and len(rows) > 100 and (np.diff(rows) > 0).all()
    assert np.array_equal(s, big.numpy()[rows])
    assert np.array_equal(s, np.load(tmp_path / "b" / "big_sample.npy"))  # the same sample every run
