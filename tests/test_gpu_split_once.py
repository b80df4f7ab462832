"""The node tile of paths_fused_kernel as bf16 pieces, split once by the product wave that forms a value (csrc/paths_fused.hip,
DESIGN 12.11), against the fp32 Gram role (LGNN_GRAM_F32=1, read per call) on the shapes the piece layout can break: classes
per launch R = 1, 7, 8, 9, 40, 41, 48 (a chunk of 8 tile rows partly filled, the row pair of a dword half filled, every row), a
second launch for the classes past 48, widths 132 / 192 (the last product wave has no columns) / 256, GCN and GraphSAGE, a
graph with a hub of more than 64 paths (several chunks of one node) and with nodes that have no path (their tile is never
written), and batches that take the node-list instance.

The bound of every case is twice the figure of the SAME case before the change (the Gram waves splitting the fp32 tile
themselves) plus 1e-7: the pieces are bit for bit the same, only the order of the fp32 sums inside an MFMA and of the atomic
adds differs.  PARENT holds those figures (relative Frobenius difference of B_0, default role against fp32 role), measured
on an MI355X with the parent commit's library; `figure(case)` is what was run there and what is run here.
"""
import numpy as np
import pytest
import torch

from gpu_utils import rel
from test_gpu_scale import _engine, _make
from test_gpu_split_gram import _accumulate

pytestmark = pytest.mark.gpu

N, F = 3000, 48
RS = (1, 7, 8, 9, 40, 41, 48)

# id -> (kind, H, C, class range, batch size, hub graph)
CASES = {}
for _R in RS:
    CASES[f"gcn-H256-R{_R}"] = ("gcn", 256, 64, (3, 3 + _R), 300, False)
    CASES[f"sage-H132-R{_R}"] = ("sage", 132, 64, (3, 3 + _R), 300, False)
for _R in (9, 41):
    CASES[f"gcn-H192-R{_R}-list"] = ("gcn", 192, 64, (5, 5 + _R), 60, False)
    CASES[f"sage-H256-R{_R}-list"] = ("sage", 256, 64, (5, 5 + _R), 60, False)
# classes past 48: a second launch over the fourth class tile of the coefficient slots, with 1, 9 and 16 classes
CASES["gcn-H192-C49"] = ("gcn", 192, 64, (0, 49), 300, False)
CASES["gcn-H132-C57"] = ("gcn", 132, 64, (0, 57), 300, False)
CASES["gcn-H256-C64"] = ("gcn", 256, 64, (0, 64), 300, False)
CASES["sage-H256-C57"] = ("sage", 256, 64, (0, 57), 300, False)
CASES["sage-H192-C64-list"] = ("sage", 192, 64, (0, 64), 60, False)
for _kind in ("gcn", "sage"):
    CASES[f"{_kind}-H256-hub"] = (_kind, 256, 40, (0, 40), 300, True)
    CASES[f"{_kind}-H256-hub-list"] = (_kind, 256, 40, (0, 40), 100, True)
    CASES[f"{_kind}-H132-hub-R9"] = (_kind, 132, 40, (2, 11), 300, True)

# parent commit, MI355X: rel(B_0 default role, B_0 fp32 role) per case
PARENT = {
    "gcn-H132-C57": 2.423e-07,
    "gcn-H132-hub-R9": 2.047e-07,
    "gcn-H192-C49": 2.309e-07,
    "gcn-H192-R41-list": 2.016e-07,
    "gcn-H192-R9-list": 2.087e-07,
    "gcn-H256-C64": 2.362e-07,
    "gcn-H256-R1": 1.905e-07,
    "gcn-H256-R40": 2.195e-07,
    "gcn-H256-R41": 2.159e-07,
    "gcn-H256-R48": 2.280e-07,
    "gcn-H256-R7": 2.015e-07,
    "gcn-H256-R8": 2.063e-07,
    "gcn-H256-R9": 1.948e-07,
    "gcn-H256-hub": 2.092e-07,
    "gcn-H256-hub-list": 4.463e-07,
    "sage-H132-R1": 1.198e-07,
    "sage-H132-R40": 1.574e-07,
    "sage-H132-R41": 1.629e-07,
    "sage-H132-R48": 1.828e-07,
    "sage-H132-R7": 1.452e-07,
    "sage-H132-R8": 1.349e-07,
    "sage-H132-R9": 1.359e-07,
    "sage-H132-hub-R9": 1.528e-07,
    "sage-H192-C64-list": 1.504e-07,
    "sage-H256-C57": 1.539e-07,
    "sage-H256-R41-list": 1.270e-07,
    "sage-H256-R9-list": 1.048e-07,
    "sage-H256-hub": 2.687e-07,
    "sage-H256-hub-list": 1.520e-07,
}


def _graph(hub, seed):
    """Random edges; `hub`: a sparser graph whose node 0 neighbours the nodes 1 .. 200 (the batch takes 1 .. 100: node 0 has
    more than 64 one-hop and two-hop paths) and whose last 100 nodes have no edge at all (no path unless in the batch)."""
    g = torch.Generator().manual_seed(seed)
    if not hub:
        return torch.randint(0, N, (2, 12000), generator=g)
    ei = torch.randint(201, N - 100, (2, 5000), generator=g)
    spokes = torch.stack([torch.zeros(200, dtype=torch.long), torch.arange(1, 201)])
    return torch.cat([ei, spokes], dim=1)


def _batch(M, hub, seed):
    g = torch.Generator().manual_seed(seed)
    if hub:
        rest = 201 + torch.randperm(N - 301, generator=g)[:M - 100]
        idx = torch.cat([torch.arange(1, 101), rest])
    else:
        idx = torch.randperm(N, generator=g)[:M]
    return idx, torch.randint(0, 64, (M,), generator=g)


def _check_hub(ei, idx):
    """node 0 has more than 64 paths of either family and some node has none (counted on the symmetrised graph with self
    loops, which is what the GCN's propagation matrix connects; GraphSAGE's one-hop paths are a subset)"""
    A = torch.zeros(N, N)
    A[ei[0], ei[1]] = 1.0
    A = ((A + A.T + torch.eye(N)) > 0).float()
    b = torch.zeros(N)
    b[idx] = 1.0
    one = (A - torch.eye(N)) @ b
    two = A @ (A @ b)
    assert one[0] > 64 and two[0] > 64
    assert int((two == 0).sum()) > 0


def figure(case):
    """rel(B_0 under the default role, B_0 under the fp32 role) of one case, and the two factors"""
    kind, H, C, classes, M, hub = CASES[case]
    seed = sum(map(ord, case))
    _, X, Ws, bs = _make(kind, N, F, H, C, 1, L=2, seed=seed)
    ei = _graph(hub, seed)
    idx, y = _batch(M, hub, seed + 1)
    y = y % C
    if hub:
        _check_hub(ei, idx)
    eng = _engine(kind, N, ei, X, Ws, bs)
    assert eng.kfac_plan()["paths"]
    calls = [(idx.cuda(), y.cuda(), M, {"classes": classes})]
    s0, _, _ = _accumulate(eng, False, calls)
    f0, _, _ = _accumulate(eng, True, calls)
    assert eng.last_kfac_used_paths
    eng.check_async_errors()
    eng.close()
    return rel(s0, f0), s0, f0


@pytest.mark.parametrize("case", sorted(CASES))
def test_pieces_written_once_match_the_fp32_role(case):
    d, s0, f0 = figure(case)
    print(f"{case}: default role vs fp32 role {d:.3e} (parent {PARENT[case]:.3e})")
    assert np.isfinite(f0).all() and np.abs(f0).max() > 0
    assert d <= 2 * PARENT[case] + 1e-7


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("cls", [3, 50])
def test_non_finite_tile_value_gives_a_non_finite_factor_under_both_roles(bad, cls):
    """W_1[cls, 17] non-finite: a tile value of the first (cls = 3) or of the second launch (cls = 50) is; H = 192, so the
    piece planes of the fourth product wave stay the zeros of the kernel's start"""
    H, C = 192, 64
    ei, X, Ws, bs = _make("gcn", N, F, H, C, 12000, L=2, seed=4)
    Ws[1][cls, 17] = bad
    eng = _engine("gcn", N, ei, X, Ws, bs)
    g = torch.Generator().manual_seed(9)
    idx = torch.randperm(N, generator=g)[:300].cuda()
    y = torch.randint(0, C, (300,), generator=g).cuda()
    for f32 in (False, True):
        s0, _, _ = _accumulate(eng, f32, [(idx, y, 300, {})])
        assert not np.isfinite(s0).all(), f"fp32 role: {f32}"
    eng.close()
