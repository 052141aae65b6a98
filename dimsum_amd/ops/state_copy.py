"""native.state_pool_table / native.state_copy_slots written out in plain torch (same signatures, same refusals, same skips): what the tests
compare the kernel with and what CPU tests put in its place; never a fallback: nothing in the package calls it."""
import torch

from .. import native


def state_pool_table_torch(pool):
    """native.state_pool_table without the device table: the pool's own checks, on any device"""
    return native.StatePoolTable(*native.state_pool_tensors(pool))


def state_copy_slots_torch(table, pairs):
    """native.state_copy_slots: slot dst := slot src of every tensor of the pool for every pair; a pair with a negative index or one
    >= num_slots is skipped. A host list goes through the wrapper's checks; a tensor is taken as is (a host read: test infrastructure).
    Every source row is read before any row is written, so the answer is the defined one whenever the kernel's is."""
    assert isinstance(table, native.StatePoolTable)
    if not torch.is_tensor(pairs):
        pairs = native.state_copy_pairs(pairs, table.num_slots)
    assert pairs.dtype == torch.int32 and pairs.dim() == 2 and pairs.shape[1] == 2
    live = [(s, d) for s, d in pairs.tolist() if 0 <= s < table.num_slots and 0 <= d < table.num_slots and s != d]
    for t in table.tensors:
        rows = [t[s].clone() for s, _ in live]
        for (_, d), row in zip(live, rows):
            t[d].copy_(row)
