"""The process group of a fit: rank / world and the one flat all-reduce."""
import torch
import torch.distributed as dist


def _dist_info(process_group):
    if process_group is None and not (dist.is_available() and dist.is_initialized()):
        return 0, 1
    return dist.get_rank(process_group), dist.get_world_size(process_group)


def all_reduce_flat_(tensors: list[torch.Tensor], process_group=None):
    """Sum a list of tensors over the group with one collective on a flat buffer (in place)."""
    rank, world = _dist_info(process_group)
    if world == 1:
        return
    big = [t for t in tensors if t.numel() >= (1 << 24)]
    if len(tensors) == 1 or big:
        # a large contiguous tensor (the 2.3 GB last-layer H at the products shape) is reduced where it lives --
        # no second buffer, no copy back; the small rest (loss scalars) still travels as one flat message
        for t in big if big else tensors:
            if not t.is_contiguous():
                raise ValueError("all_reduce_flat_ needs contiguous tensors")
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=process_group)
        tensors = [t for t in tensors if t.numel() < (1 << 24)] if big else []
        if not tensors:
            return
    flat = torch.cat([t.reshape(-1) for t in tensors])
    dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=process_group)
    off = 0
    for t in tensors:
        n = t.numel()
        t.copy_(flat[off:off + n].view_as(t))
        off += n
