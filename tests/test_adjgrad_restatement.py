"""Pins tests/adjgrad_restatement.py, the fp64 autograd yardstick of the full posterior's adjacency gradient, to the reference:
with the diagonal log determinant it must reproduce the reference's own ``model.adj.grad`` goldens of ``DiagLaplace`` (value,
stored entries, the 200 non-edges), and its full GGN and full-posterior value must match the ``fullla_*`` goldens.  The goldens
are stored in fp32; measured <= 4.5e-7 (gradients), <= 2e-7 (H), <= 2e-8 (value), held at 1e-6."""
import glob
import os

import numpy as np
import pytest

from adjgrad_restatement import neg_marglik_adj_grad, spec_from_golden
from conftest import GOLDEN


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


CASES = sorted(p for p in glob.glob(os.path.join(GOLDEN, "*.npz")) if "adjgrad_diag_vals" in np.load(p))


@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(p)[:-4] for p in CASES])
def test_restatement_reproduces_the_reference_goldens(path):
    g = np.load(path)
    spec = spec_from_golden(g)
    prior = float(g["adjgrad_prior"])
    val, gA, H = neg_marglik_adj_grad(g["adj_nz_row"], g["adj_nz_col"], g["train_idx"], g["train_y"], prior, "diag", **spec)
    ref = float(g["adjgrad_diag_neg_marglik"])
    print(f"value {abs(val - ref) / abs(ref):.2e}  stored {rel(gA[g['adj_nz_row'], g['adj_nz_col']], g['adjgrad_diag_vals']):.2e}  "
          f"non-edges {rel(gA[g['adjgrad_ne_row'], g['adjgrad_ne_col']], g['adjgrad_diag_ne_val']):.2e}")
    assert abs(val - ref) <= 1e-6 * abs(ref)
    assert rel(gA[g["adj_nz_row"], g["adj_nz_col"]], g["adjgrad_diag_vals"]) < 1e-6
    assert rel(gA[g["adjgrad_ne_row"], g["adjgrad_ne_col"]], g["adjgrad_diag_ne_val"]) < 1e-6
    if "fullla_H" in g.files:
        print(f"H {rel(H, g['fullla_H']):.2e}")
        assert rel(H, g["fullla_H"]) < 1e-6
    if "fullla_marglik_pp07" in g.files:
        assert prior == 0.7
        vf, gF, _ = neg_marglik_adj_grad(g["adj_nz_row"], g["adj_nz_col"], g["train_idx"], g["train_y"], prior, "full", **spec)
        assert abs(vf + float(g["fullla_marglik_pp07"])) <= 1e-6 * abs(float(g["fullla_marglik_pp07"]))
        assert rel(gF, gA) > 0.1  # the full posterior's gradient is a different one
