"""The host side of the batch-structure cache: which index tensors name the same batch (engine.BatchTagMap).  CPU tensors
behave like device tensors in everything the key reads (base, data pointer, offset, shape, version counter)."""
import torch

from laplace_gnn_amd.data import TensorBatchLoader
from laplace_gnn_amd.engine import BatchTagMap


def test_slices_of_one_loader_repeat_their_tags_pass_after_pass():
    idx, y = torch.arange(25), torch.zeros(25, dtype=torch.int64)
    loader = TensorBatchLoader(idx, y, batch_size=10)
    tags = BatchTagMap()
    first = [tags.tag(b) for b, _ in loader]
    second = [tags.tag(b) for b, _ in loader]
    assert first == second and len(set(first)) == 3 and 0 not in first
    assert len(tags) == 3


def test_equal_contents_in_other_tensors_are_other_batches():
    a = torch.arange(10)
    tags = BatchTagMap()
    assert tags.tag(a) != tags.tag(a.clone())
    assert tags.tag(a[:5]) != tags.tag(a[5:])      # same base, other offset
    assert tags.tag(a[:5]) != tags.tag(a[:6])      # same base and offset, other length
    assert tags.tag(a[:5]) == tags.tag(a[0:5])


def test_an_in_place_write_through_torch_is_a_new_batch_for_every_view():
    a = torch.arange(10)
    tags = BatchTagMap()
    t_whole, t_view = tags.tag(a), tags.tag(a[2:7])
    a[9] = 3  # outside the view: the version counter is shared by a base and its views
    assert tags.tag(a) != t_whole and tags.tag(a[2:7]) != t_view
    t2 = tags.tag(a[2:7])
    a[2:7].add_(1)
    assert tags.tag(a[2:7]) != t2
    t3 = tags.tag(a)
    a.data.mul_(1)  # through .data: no counter moves -- the library's device-side guard covers this
    assert tags.tag(a) == t3


def test_the_key_keeps_the_tensor_alive_so_its_address_cannot_be_reused():
    tags = BatchTagMap()
    seen = set()
    for _ in range(20):
        t = torch.arange(1000)
        tag = tags.tag(t)
        assert tag not in seen
        seen.add(tag)
        del t  # (the map still holds it: the next tensor cannot take its place)
    assert len(seen) == 20


def test_copies_and_unsupported_layouts_are_never_cached():
    tags = BatchTagMap()
    a = torch.arange(20)
    strided = a[::2]
    assert tags.tag(strided) == 0
    assert tags.tag(strided.contiguous(), copied=True) == 0
    assert tags.tag(a.view(4, 5)) == 0
    assert len(tags) == 0


def test_the_map_is_bounded_and_reports_what_it_drops():
    dropped = []
    tags = BatchTagMap(capacity=3, on_drop=dropped.append)
    ts = [torch.arange(4) for _ in range(5)]
    got = [tags.tag(t) for t in ts[:3]]
    assert tags.tag(ts[0]) == got[0]          # touched: the least recently used is now ts[1]
    tags.tag(ts[3])
    assert dropped == [got[1]] and len(tags) == 3
    tags.tag(ts[4])
    assert dropped == [got[1], got[2]]
    assert tags.tag(ts[0]) == got[0]
    assert tags.tag(ts[1]) not in got         # dropped keys come back under a new tag
    tags.clear()
    assert len(tags) == 0
