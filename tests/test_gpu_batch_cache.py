"""The batch-structure cache (csrc/batchcache.hip): the active-row list and the two-hop path list of a batch,
kept by the library from the second accumulate of a batch on, against the same fits with ``LGNN_BATCH_CACHE_MB=0``.

A cached list holds the same paths as a rebuilt one in another order (``path_r_kernel`` hands out slots with ``atomicAdd``), so
a hit differs from a cache-off run only by the order of fp32 sums -- as two cache-off runs already do.  The bound of every
comparison is therefore measured in the test, the way ``test_gpu_split_once.py`` takes its bound: twice the difference of two
cache-off runs on the same inputs plus 1e-7.  The absolute bar against the CPU oracle (1e-4, ``test_gpu_paths.py``) is kept
where the oracle is run.
"""
import os

import numpy as np
import pytest
import torch

import gnn_laplace_oracle as O
from gpu_utils import oracle_from_arrays, rel
from test_gpu_scale import _engine, _make
from test_gpu_split_once import _batch, _check_hub, _graph

pytestmark = pytest.mark.gpu

N, F = 3000, 48
RTOL = 1e-4


class _budget:
    """LGNN_BATCH_CACHE_MB for the duration of a block (the library reads it per call); None: the default"""

    def __init__(self, mb):
        self.mb = mb

    def __enter__(self):
        self.old = os.environ.pop("LGNN_BATCH_CACHE_MB", None)
        if self.mb is not None:
            os.environ["LGNN_BATCH_CACHE_MB"] = str(self.mb)

    def __exit__(self, *exc):
        os.environ.pop("LGNN_BATCH_CACHE_MB", None)
        if self.old is not None:
            os.environ["LGNN_BATCH_CACHE_MB"] = self.old


def _fit(eng, idx, y, bs, **kw):
    """One fit over the slices of (idx, y), as TensorBatchLoader yields them: [A_0, B_0, A_1, B_1] and the loss"""
    _, views, loss = eng.new_kfac_buffers()
    n = idx.shape[0]
    for s in range(0, n, bs):
        eng.kfac_accumulate(idx[s:s + bs], y[s:s + bs], n, views, loss, **kw)
    torch.cuda.synchronize()
    return [t.cpu().numpy().astype(np.float64) for pair in views for t in pair], float(loss)


LOSS_RUNS = 30


def _off_pair(eng, idx, y, bs, **kw):
    """Cache-off fits, each from scratch: the reference (the first) and the bounds 2 x (the difference of two cache-off fits)
    + 1e-7.  Per factor the two fits are the first two.  The loss is ONE fp32 number whose workgroup sums arrive by atomicAdd
    in any order: two given fits often agree to the bit while a third lies a unit or two in the last place away (1.1e-7
    relative at 2216.47, more than the 1e-7), so with one pair the parent's library fails this comparison against itself --
    30 cache-off fits of one mid-size case with it, MI355X: four distinct losses, 11 / 14 / 3 / 2 times, three units in the
    last place apart.  For the loss the two fits are therefore the pair that differs most among LOSS_RUNS."""
    runs = []
    with _budget(0):
        for _ in range(LOSS_RUNS):
            eng.invalidate()  # the forward and the input Grams behind A are part of a fit
            r = _fit(eng, idx, y, bs, **kw)
            runs.append(r if len(runs) < 2 else (None, r[1]))
        assert eng.batch_cache_stats()["entries"] == 0
    r1, l1 = runs[0]
    return r1, l1, _bounds([runs[0][0], runs[1][0]]), _bounds([[np.float64(l)] for _, l in runs])[0]


def _bounds(runs):
    """per array: 2 x (the largest difference of two of the runs, relative to the second) + 1e-7"""
    pairs = [(i, j) for i in range(len(runs)) for j in range(len(runs)) if i != j]
    return [2 * max(rel(runs[i][k], runs[j][k]) for i, j in pairs) + 1e-7 for k in range(len(runs[0]))]


def _assert_same(got, loss, ref, ref_loss, bounds, loss_bound, what):
    for k, (a, b, bound) in enumerate(zip(got, ref, bounds)):
        d = rel(a, b)
        print(f"{what}: factor {k}: cached vs cache-off {d:.3e} (bound {bound:.3e})")
        assert np.isfinite(a).all() and d <= bound, (what, k, d, bound)
    dl = abs(loss - ref_loss) / abs(ref_loss)
    print(f"{what}: loss {dl:.3e} (bound {loss_bound:.3e})")
    assert dl <= loss_bound, (what, dl, loss_bound)


def _three_fits(eng, idx, y, bs, **kw):
    """first sight, build, hit: the third fit's result, with the counts the stats query must show"""
    nb = -(-idx.shape[0] // bs)
    s0 = eng.batch_cache_stats()
    _fit(eng, idx, y, bs, **kw)
    s1 = eng.batch_cache_stats()
    assert s1["misses"] - s0["misses"] == nb and s1["builds"] == s0["builds"] and s1["entries"] == s0["entries"]
    _fit(eng, idx, y, bs, **kw)
    s2 = eng.batch_cache_stats()
    assert s2["builds"] - s1["builds"] == nb and s2["entries"] - s1["entries"] == nb and s2["bytes"] > s1["bytes"]
    out = _fit(eng, idx, y, bs, **kw)
    s3 = eng.batch_cache_stats()
    assert s3["hits"] - s2["hits"] == nb and s3["builds"] == s2["builds"] and s3["misses"] == s2["misses"]
    return out


# id -> (nodes, H, C, batch size, batches, hub graph, LGNN_PATH_LIST_CAP)
CASES = {
    "small-full": (300, 256, 7, 120, 2, False, None),
    "mid-full": (N, 256, 40, 300, 2, False, None),         # 8 expected paths per node: paths_fused_kernel<false>
    "mid-short-list": (N, 192, 40, 60, 2, False, None),    # 1.6 expected paths per node: the node-list instance
    "mid-full-and-short": (N, 132, 64, 300, 1.2, False, None),  # a full batch and a short last batch of one loader
    "hub-full": (N, 256, 40, 300, 1, True, None),
    "hub-list": (N, 256, 40, 100, 1, True, None),
    "overflow": (N, 256, 40, 300, 2, False, 1000),         # the list does not fit: ybuild_kernel + streaming Gram, R kept
    "overflow-list": (N, 256, 40, 60, 2, False, 200),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_third_fit_hits_and_equals_the_cache_off_fit(case, monkeypatch):
    n, H, C, bs, nbatch, hub, cap = CASES[case]
    seed = sum(map(ord, case))
    if n == N:
        _, X, Ws, bs_ = _make("gcn", N, F, H, C, 1, L=2, seed=seed)
        ei = _graph(hub, seed)
        idx, y = _batch(int(bs * nbatch), hub, seed + 1)
        if hub:
            _check_hub(ei, idx)
    else:
        ei, X, Ws, bs_ = _make("gcn", n, F, H, C, 900, L=2, seed=seed)
        g = torch.Generator().manual_seed(seed)
        idx, y = torch.randperm(n, generator=g)[:int(bs * nbatch)], torch.randint(0, C, (int(bs * nbatch),), generator=g)
    y = y % C
    idx[-1] = idx[0] if hub else idx[1]  # a node listed twice (the multiplicities are part of the cached weights)
    if cap is not None:
        monkeypatch.setenv("LGNN_PATH_LIST_CAP", str(cap))
    eng = _engine("gcn", n, ei, X, Ws, bs_)
    assert eng.kfac_plan()["paths"]
    idx, y = idx.cuda(), y.cuda()
    ref, ref_loss, bounds, lb = _off_pair(eng, idx, y, bs, paths=True)
    with _budget(None):
        got, loss = _three_fits(eng, idx, y, bs, paths=True)
    assert eng.last_kfac_used_paths
    _assert_same(got, loss, ref, ref_loss, bounds, lb, case)
    om = oracle_from_arrays("gcn", n, ei.numpy(), X.numpy(), [w.numpy() for w in Ws], [b.numpy() for b in bs_], True)
    oloss, oH = O.fit_kron(om, idx.cpu().numpy(), y.cpu().numpy(), bs)
    for l in range(2):
        assert rel(got[2 * l + 1], oH[2 * l][0]) < RTOL, f"B_{l} vs oracle"
        assert rel(got[2 * l], oH[2 * l][1]) < RTOL, f"A_{l} vs oracle"
    assert abs(loss - float(oloss)) <= RTOL * abs(float(oloss))
    eng.check_async_errors()
    eng.close()


def _mid(seed=3, H=256, C=40, M=600):
    ei, X, Ws, bs = _make("gcn", N, F, H, C, 12000, L=2, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    idx = torch.randperm(N, generator=g)[:M]
    y = torch.randint(0, C, (M,), generator=g)
    eng = _engine("gcn", N, ei, X, Ws, bs)
    return eng, ei, idx.cuda(), y.cuda()


def test_weights_changed_between_fits_still_hit():
    eng, _, idx, y = _mid()
    with _budget(None):
        _three_fits(eng, idx, y, 300)
        with torch.no_grad():
            for w in eng._bound[1]:
                w.mul_(1.5).add_(0.01)  # (an optimizer step: the version counters make the engine invalidate the forward)
        before = eng.batch_cache_stats()
        got, loss = _fit(eng, idx, y, 300)
        after = eng.batch_cache_stats()
    assert after["hits"] - before["hits"] == 2 and after["builds"] == before["builds"] and after["misses"] == before["misses"]
    eng.invalidate()
    with _budget(None):
        got2, loss2 = _fit(eng, idx, y, 300)
    assert eng.batch_cache_stats()["hits"] - after["hits"] == 2
    ref, ref_loss, bounds, lb = _off_pair(eng, idx, y, 300)
    _assert_same(got, loss, ref, ref_loss, bounds, lb, "new weights")
    _assert_same(got2, loss2, ref, ref_loss, bounds, lb, "after invalidate()")
    eng.check_async_errors()
    eng.close()


def test_graph_edit_drops_every_entry_and_the_lists_are_built_again():
    eng, ei, idx, y = _mid(seed=5)
    with _budget(None):
        _three_fits(eng, idx, y, 300)
        # new edges at the batch's own nodes (and their transposes: the stored adjacency stays symmetric)
        a, b = idx[:40].clone(), idx[300:340].clone()
        keep = a != b
        a, b = a[keep], b[keep]
        eng.update_adjacency(torch.cat([a, b]), torch.cat([b, a]), torch.ones(2 * a.numel(), dtype=torch.uint8))
        assert eng.batch_cache_stats()["entries"] == 0 and eng.batch_cache_stats()["bytes"] == 0
        got, loss = _three_fits(eng, idx, y, 300)  # no stale hit: first sight, build, hit again
    ref, ref_loss, bounds, lb = _off_pair(eng, idx, y, 300)
    _assert_same(got, loss, ref, ref_loss, bounds, lb, "edited graph")
    eng.check_async_errors()
    eng.close()


def test_ids_changed_through_torch_miss_and_behind_its_back_raise():
    from laplace_gnn_amd._lib import HipLibraryError

    eng, _, idx, y = _mid(seed=7)
    other = int(((torch.arange(N, device="cuda")[:, None] == idx[None, :]).sum(1) == 0).nonzero()[0])  # a node not in the batch
    with _budget(None):
        _three_fits(eng, idx, y, 300)
        idx[5] = other  # in place through torch: the version counter moves, every slice of the tensor is a new batch
        before = eng.batch_cache_stats()
        got, loss = _fit(eng, idx, y, 300)
        after = eng.batch_cache_stats()
    assert after["misses"] - before["misses"] == 2 and after["hits"] == before["hits"]
    ref, ref_loss, bounds, lb = _off_pair(eng, idx, y, 300)
    _assert_same(got, loss, ref, ref_loss, bounds, lb, "id changed in place")
    eng.check_async_errors()
    with _budget(None):
        _fit(eng, idx, y, 300)
        _fit(eng, idx, y, 300)
        eng.check_async_errors()
        changed = idx.clone()
        changed[310] = int(idx[5])
        changed[5] = int(idx[311])
        idx.data.copy_(changed)  # a raw copy into the storage: no version counter sees it
        _fit(eng, idx, y, 300)
        with pytest.raises(HipLibraryError, match="cached structure"):
            eng.check_async_errors()
        eng.batch_cache_clear()
        got, loss = _fit(eng, idx, y, 300)
    ref, ref_loss, bounds, lb = _off_pair(eng, idx, y, 300)
    _assert_same(got, loss, ref, ref_loss, bounds, lb, "after batch_cache_clear()")
    eng.check_async_errors()
    eng.close()


def test_a_freed_tensor_and_another_one_in_its_place():
    eng, _, idx, y = _mid(seed=9)
    g = torch.Generator().manual_seed(1)
    with _budget(None):
        a = idx.clone()
        _three_fits(eng, a, y, 300)
        ptr = a.data_ptr()
        del a
        b = torch.randperm(N, generator=g)[:600].cuda()  # same length, other contents; the allocator may hand out the same block
        print("same address:", b.data_ptr() == ptr)
        before = eng.batch_cache_stats()
        got, loss = _fit(eng, b, y, 300)
        after = eng.batch_cache_stats()
    assert after["hits"] == before["hits"]
    ref, ref_loss, bounds, lb = _off_pair(eng, b, y, 300)
    _assert_same(got, loss, ref, ref_loss, bounds, lb, "new tensor")
    eng.check_async_errors()
    eng.close()


def test_two_loaders_alternate_a_small_budget_evicts_and_budget_zero_is_off():
    eng, _, idx, y = _mid(seed=11, M=1200)
    tr, ytr, va, yva = idx[:600], y[:600], idx[600:], y[600:]
    ref_t, lt, bt, lbt = _off_pair(eng, tr, ytr, 300)
    ref_v, lv, bv, lbv = _off_pair(eng, va, yva, 300)
    with _budget(None):
        for _ in range(3):
            got_t, loss_t = _fit(eng, tr, ytr, 300)
            got_v, loss_v = _fit(eng, va, yva, 300)
        st = eng.batch_cache_stats()
        assert st["entries"] == 4 and st["hits"] == 4 and st["builds"] == 4 and st["misses"] == 4
        _assert_same(got_t, loss_t, ref_t, lt, bt, lbt, "train loader")
        _assert_same(got_v, loss_v, ref_v, lv, bv, lbv, "validation loader")
        per_entry = st["bytes"] / 4
        print("bytes per entry:", per_entry)
    assert 4 * per_entry > (1 << 20) > per_entry, "the case needs four entries that do not fit one MiB together"
    with _budget(1):  # one MiB: not all four entries fit
        for _ in range(3):
            got_t, loss_t = _fit(eng, tr, ytr, 300)
            got_v, loss_v = _fit(eng, va, yva, 300)
        st = eng.batch_cache_stats()
        assert 0 < st["entries"] < 4 and st["bytes"] <= (1 << 20)
        _assert_same(got_t, loss_t, ref_t, lt, bt, lbt, "train loader, small budget")
        _assert_same(got_v, loss_v, ref_v, lv, bv, lbv, "validation loader, small budget")
    with _budget(0):
        before = eng.batch_cache_stats()
        got_t, loss_t = _fit(eng, tr, ytr, 300)
        after = eng.batch_cache_stats()
        assert after["entries"] == 0 and after["bytes"] == 0
        assert (after["hits"], after["misses"], after["builds"]) == (before["hits"], before["misses"], before["builds"])
        _assert_same(got_t, loss_t, ref_t, lt, bt, lbt, "budget 0")
    eng.check_async_errors()
    eng.close()


@pytest.mark.parametrize("paths", [None, False])
def test_class_ranges_and_node_shares_of_a_cached_batch_add_up(paths):
    eng, _, idx, y = _mid(seed=13, C=10)
    C = 10
    with _budget(None):
        whole, wl = _three_fits(eng, idx, y, 300, paths=paths)
        assert eng.last_kfac_used_paths == (paths is None)
        before = eng.batch_cache_stats()
        calls = 0
        for mode, count, cuts in (("classes", C, [0, 1, 4, C]), ("share", C, [0, 1, 4, 9, C]), ("share", 25, [0, 2, 11, 12, 25])):
            flat, views, loss = eng.new_kfac_buffers()
            for s in (0, 300):
                for a, b in zip(cuts[:-1], cuts[1:]):
                    kw = {"classes": (a, b)} if mode == "classes" else {"share": (a, b, count)}
                    eng.kfac_accumulate(idx[s:s + 300], y[s:s + 300], 600, views, loss, paths=paths, **kw)
                    calls += 1
            torch.cuda.synchronize()
            parts = [t.cpu().numpy().astype(np.float64) for pair in views for t in pair]
            for k, (a, b) in enumerate(zip(parts, whole)):
                assert rel(a, b) < 1e-5, (mode, count, k)
            assert abs(float(loss) - wl) <= 1e-5 * abs(wl)
        after = eng.batch_cache_stats()
    assert after["builds"] == before["builds"] and after["misses"] == before["misses"]
    # (a part without a class column returns before the route is entered: it is not counted)
    assert 0 < after["hits"] - before["hits"] <= calls
    eng.check_async_errors()
    eng.close()


def test_fisher_plane_route_and_diag_are_unaffected():
    eng, _, idx, y = _mid(seed=15, C=10)

    def others():
        out = []
        _, views, loss = eng.new_kfac_buffers()
        for s in (0, 300):
            eng.kfac_accumulate_fisher(idx[s:s + 300], y[s:s + 300], y[s:s + 300], 600, views, loss)
        out += [t.clone() for pair in views for t in pair] + [loss.clone()]
        diag = torch.zeros(eng.n_params, device="cuda")
        dl = torch.zeros(1, device="cuda")
        for s in (0, 300):
            eng.diag_accumulate(idx[s:s + 300], y[s:s + 300], diag, dl)
        out += [diag, dl]
        torch.cuda.synchronize()
        return [t.cpu().numpy().astype(np.float64) for t in out]

    refs = []
    with _budget(0):
        for _ in range(LOSS_RUNS):
            eng.invalidate()
            refs.append(others())
    # (arrays: the first two runs; the two losses, entries 4 and 6: the most different pair of all runs, see _off_pair)
    bounds = _bounds(refs[:2])
    for k in (4, 6):
        bounds[k] = _bounds([[r[k]] for r in refs])[0]
    with _budget(None):
        _three_fits(eng, idx, y, 300)
        before = eng.batch_cache_stats()
        got = others()
        assert eng.batch_cache_stats() == before  # neither takes part in the cache
        plane, pl = _fit(eng, idx, y, 300, paths=False)  # the plane route reads the cached active rows
        assert not eng.last_kfac_used_paths and eng.batch_cache_stats()["hits"] - before["hits"] == 2
    for k, (a, b) in enumerate(zip(got, refs[0])):
        assert rel(a, b) <= bounds[k], (k, rel(a, b), bounds[k])
    r, rl, bounds, lb = _off_pair(eng, idx, y, 300, paths=False)
    _assert_same(plane, pl, r, rl, bounds, lb, "plane route")
    eng.check_async_errors()
    eng.close()
