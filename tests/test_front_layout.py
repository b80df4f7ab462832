"""The layout of the Laplace front (the package ``laplace_gnn_amd.laplace``): its import surface, the factory's keys, no
function-body imports between its modules, and the in-place accumulator protocol of the fit loop against the generic
``(loss, H)`` route on the CPU stand-ins.  No GPU."""
import ast
import glob
import os

import numpy as np
import pytest
import torch

import laplace_gnn_amd as lg
from laplace_gnn_amd import laplace as lp
from conftest import GOLDEN, ROOT
from oracle_backend import CpuForwardGCN, OracleBackend, OracleClassBackend

# ``dir(laplace_gnn_amd.laplace)`` of the one-file module this package replaced, minus dunders, imported modules and the names
# of the standard library and torch it merely imported (Any, annotations, log, pi, parameters_to_vector)
SURFACE = ["BaseLaplace", "DiagLLLaplace", "DiagLaplace", "DiagSubnetLaplace", "FullLLLaplace", "FullLaplace",
           "FullSubnetLaplace", "HipGGN", "Kron", "KronDecomposed", "KronLLLaplace", "KronLaplace", "Laplace", "LowRankLaplace",
           "ParametricLaplace", "SubnetLaplace", "TensorBatchLoader", "_GLMLinkMixin", "_LastLayerHead", "_adjacency_candidates",
           "_adjgrad_drive", "_adjgrad_scope", "_all_subclasses", "_dense_scope", "_dist_info", "_is_zero_number",
           "all_reduce_flat_"]
FACTORY = {("all", "kron"): "KronLaplace", ("all", "diag"): "DiagLaplace", ("all", "full"): "FullLaplace",
           ("all", "lowrank"): "LowRankLaplace", ("last_layer", "full"): "FullLLLaplace", ("last_layer", "kron"): "KronLLLaplace",
           ("last_layer", "diag"): "DiagLLLaplace", ("all", "gp"): "FunctionalLaplace",
           ("subnetwork", "full"): "FullSubnetLaplace", ("subnetwork", "diag"): "DiagSubnetLaplace"}
PACKAGE = os.path.join(ROOT, "laplace-gnn_amd", "laplace")


def test_import_surface_is_the_one_file_modules():
    missing = [name for name in SURFACE if not hasattr(lp, name)]
    assert missing == []
    assert lp.BaseLaplace is lg.BaseLaplace and lp.all_reduce_flat_ is lg.all_reduce_flat_


def _tiny_model():
    g = torch.Generator().manual_seed(0)
    return lg.GCN(4, 5, 3, 2, torch.randn(12, 4, generator=g), torch.randint(0, 12, (2, 30), generator=g), symmetric=True).eval()


@pytest.mark.parametrize("key", sorted(FACTORY))
def test_factory_keys_return_the_same_classes(key):
    kwargs = {("all", "gp"): {"n_subset": 4}}.get(key, {})
    if key[0] == "subnetwork":
        kwargs = {"subnetwork_indices": torch.tensor([0, 3, 7]), "backend": OracleBackend}  # (its backend is made at once)
    la = lg.Laplace(_tiny_model(), "classification", *key, **kwargs)
    assert type(la).__name__ == FACTORY[key] and type(la) is getattr(lg, FACTORY[key])


def test_no_module_of_the_package_imports_a_sibling_inside_a_function_body():
    files = sorted(glob.glob(os.path.join(PACKAGE, "*.py")))
    siblings = {os.path.basename(f)[:-3] for f in files}
    assert {"base", "fit", "kron", "diag"} <= siblings
    found = []
    for path in files:
        tree = ast.parse(open(path).read())
        for fn in ast.walk(tree):
            if not isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda)):
                continue
            for node in ast.walk(fn):
                if isinstance(node, ast.ImportFrom) and node.level == 1:
                    names = {node.module.split(".")[0]} if node.module else {a.name for a in node.names}
                    if names & siblings or node.module is None:
                        found.append((os.path.basename(path), fn.name if hasattr(fn, "name") else "lambda", node.lineno))
                elif isinstance(node, ast.Import) and any("laplace_gnn_amd.laplace" in a.name for a in node.names):
                    found.append((os.path.basename(path), getattr(fn, "name", "lambda"), node.lineno))
    assert found == []


# ---- the accumulator protocol: in-place route == generic route ---------------------------------------------------------------
# Posteriors with an in-place route on the CPU stand-ins: KronLaplace over OracleClassBackend (separate buffers, no flat one),
# and KronLaplace / DiagLaplace over the real HipGGN on tests/oracle_engine.py.  The last-layer posteriors' buffers
# (new_lastlayer_pair_buffers / new_lastlayer_kron_buffers) exist on the HIP engine only: tests/test_gpu_frontend.py covers them.
ROUTES = [("KronLaplace", "class"), ("KronLaplace", "hip"), ("DiagLaplace", "hip")]


def _fit_both_ways(cls, backend):
    g = np.load(os.path.join(GOLDEN, "gcn_small_3batch_s1.npz"))
    from test_host_logic import _cpu_model
    model = _cpu_model(g)
    assert isinstance(model, CpuForwardGCN)
    gen = torch.Generator().manual_seed(4)
    idx, y = torch.randperm(g["X"].shape[0], generator=gen)[:40], torch.randint(0, int(g["n_outputs"]), (40,), generator=gen)
    loader = lg.TensorBatchLoader(idx, y, batch_size=24)  # 24 + 16
    be = OracleClassBackend if backend == "class" else lg.HipGGN
    fast, slow = getattr(lg, cls)(model, "classification", backend=be), getattr(lg, cls)(model, "classification", backend=be)
    made, new = [], fast._new_accumulator
    fast._new_accumulator = lambda override: made.append(new(override)) or made[-1]
    slow._new_accumulator = lambda override: None  # the generic route: backend.kron / backend.diag return (loss, H)
    for override in (True, False):
        fast.fit(loader, override=override)
        slow.fit(loader, override=override)
        assert len(made) == (1 if override else 2) and made[-1] is not None and fast._acc is None
        yield fast, slow


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


@pytest.mark.parametrize("cls,backend", ROUTES)
def test_accumulator_route_equals_the_generic_route(cls, backend):
    """``fit(override=True)`` then ``fit(override=False)`` on a 24 + 16 loader: H / H_facs, loss and n_data of the in-place
    route equal those of the same posterior with ``_new_accumulator`` returning None.  The stand-ins compute both routes from
    the same oracle call per batch but add them up in a different order (into the buffers vs. into H), so the bar is the
    suite's 1e-4 relative, not bit equality."""
    for k, (fast, slow) in enumerate(_fit_both_ways(cls, backend)):
        assert fast.n_data == slow.n_data == 40 * (k + 1)
        assert abs(float(fast.loss) - float(slow.loss)) <= 1e-4 * abs(float(slow.loss))
        if cls == "KronLaplace":
            for Ff, Fs in zip(fast.H_facs.kfacs, slow.H_facs.kfacs):
                assert len(Ff) == len(Fs)
                for a, b in zip(Ff, Fs):
                    assert _rel(a, b) < 1e-4
        else:
            assert _rel(fast.H, slow.H) < 1e-4
    # what each route asked of its backend
    if backend == "class":
        assert {c[0] for c in fast.backend.calls} == {"kron_"} and {c[0] for c in slow.backend.calls} == {"kron"}


def test_diagonal_loss_slot_is_handed_out_without_a_copy_and_survives_the_next_fit():
    """``override=True``: ``loss`` is the slot of ``[H | loss]`` itself (no clone, no multiplication by a factor of 1);
    ``override=False`` zeroes the slot, so the loss handed out earlier is copied first and the sum is a tensor of its own."""
    fast, _ = next(_fit_both_ways("DiagLaplace", "hip"))  # after the override=True fit
    n = fast.n_params
    assert fast.H.data_ptr() == fast._hl.data_ptr() and fast.loss.data_ptr() == fast._hl[n:].data_ptr()
    first = float(fast.loss)
    loader = lg.TensorBatchLoader(torch.arange(6), torch.tensor([0, 1, 2, 0, 1, 2]), batch_size=4)
    fast.fit(loader, override=False)
    assert fast.loss.data_ptr() != fast._hl[n:].data_ptr() and float(fast.loss) > first and fast.n_data == 46
    assert abs(float(fast.loss) - first - float(fast._hl[n])) <= 1e-5 * float(fast.loss)
