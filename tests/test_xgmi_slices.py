"""The xGMI engine's bucket slices against the sharded optimizer's owned chunks (pure layout
arithmetic, no GPU): for FlatParams.relayout's padded layout the engine's slice r is exactly
GradReducer.owned(b) of rank r; a layout without the padding is rejected."""
import pytest
import torch

from pyrecover_amd.parallel.xgmi import sharded_slices, slice_cuts


def _flat():
    from pyrecover_amd.config import get_preset
    from pyrecover_amd.models.llama import Transformer

    torch.manual_seed(0)
    m = Transformer(get_preset("llama-micro", seq_len=64))
    return m, m.flatten_()


def _as_rank(red, rank, world, ranges):
    """A view of reducer `red` as rank `rank` of `world` over the padded `ranges` (owned() reads only
    these fields)."""
    from pyrecover_amd.parallel.ddp import GradReducer

    r = object.__new__(GradReducer)
    r.shard, r.rank, r.world, r.ranges = True, rank, world, ranges
    r.chunks = [(hi - lo) // world for lo, hi in ranges]
    return r


@pytest.mark.parametrize("world", [2, 3, 4, 8])
def test_engine_slices_equal_owned_chunks_of_a_padded_layout(world):
    from pyrecover_amd.parallel.ddp import GradReducer

    _, flat = _flat()
    red = GradReducer(flat, bucket_cap_mb=0.05, first_bucket_mb=0.02)  # one process: buckets only
    assert red.num_buckets > 3
    ranges = flat.relayout(red.bucket_slots, 64 * world)  # what GradReducer does at W > 1
    slices = sharded_slices(ranges, world)
    assert len(slices) == len(ranges)
    for rank in range(world):
        view = _as_rank(red, rank, world, ranges)
        for b in range(len(ranges)):
            assert view.owned(b) == [slices[b][rank]], (world, rank, b)
    for b, (lo, hi) in enumerate(ranges):
        cuts = slice_cuts(lo, hi, world)
        assert cuts[0] == lo and cuts[-1] == hi and all(c % 64 == 0 for c in cuts)
        assert len({cuts[r + 1] - cuts[r] for r in range(world)}) == 1  # W equal chunks


@pytest.mark.parametrize("world", [2, 3, 4, 8])
def test_unpadded_layout_is_rejected(world):
    from pyrecover_amd.parallel.ddp import GradReducer
    from pyrecover_amd.parallel.flat import FlatParams

    # groups of 200, 72 and 1000 elements, one bucket each: the one-process layout has no padding
    ps = [torch.nn.Parameter(torch.zeros(n)) for n in (200, 72, 1000)]
    flat = FlatParams([[(f"p{i}", p)] for i, p in enumerate(ps)])
    red = GradReducer(flat, bucket_cap_mb=1e-4, first_bucket_mb=1e-4)
    assert red.num_buckets == 3 and all((hi - lo) % (64 * world) for lo, hi in red.ranges)
    with pytest.raises(ValueError, match="not .* equal 64-element-aligned chunks"):
        sharded_slices(red.ranges, world)
    # the padded layout of the same groups passes
    assert sharded_slices(flat.relayout(red.bucket_slots, 64 * world), world)
    # equal 8-aligned thirds whose chunk is no multiple of 64: also not the sharded layout
    with pytest.raises(ValueError, match="unpadded layout"):
        sharded_slices([(0, 24 * world)], world)


def test_slice_cuts_keep_the_all_reduce_boundaries():
    """The factored cut function is the engine's formula: 16-B aligned cuts, the remainder in the
    last slice."""
    assert slice_cuts(0, 100, 3) == [0, 32, 64, 100]
    assert slice_cuts(64, 64 + 1024, 4) == [64, 320, 576, 832, 1088]
    assert slice_cuts(0, 7, 2) == [0, 0, 7]
