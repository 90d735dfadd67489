"""``shard_layout`` / ``shard_slices`` (tokenpacker_amd/optim.py), the flat index space of ``ShardedMainGradAdamW``: pure host
arithmetic, checked by marking every element a rank's slices name.  Also what a machine without a GPU can hold of the sharded
step's C ABI: the header declares the two calls, the binding names them."""
import itertools
import os

import pytest

from tests import optim_ref as R
from tokenpacker_amd import _capi, optim, shard_layout, shard_slices

NUMELS = (1, 3, 63, 64, 65, 4095, 4096, 4097, 2 * 4096 + 4, 70_000)
WORLDS = (1, 2, 3, 8)
TABLES = [NUMELS, tuple(reversed(NUMELS)), (1,), (70_000,), (65, 1, 4097)] + [(n,) for n in NUMELS]


def check(numels, world, align=64, chunk=optim.CHUNK):
    lay = shard_layout(numels, world, align=align, chunk=chunk)
    assert lay["world"] == world and lay["numels"] == list(numels) and len(lay["offsets"]) == len(numels)
    assert lay["total"] % (world * chunk) == 0 and lay["shard"] * world == lay["total"] and lay["total"] > 0
    end = 0
    for off, n in zip(lay["offsets"], numels):
        assert off % align == 0 and off >= end, "aligned starts, no overlap, tensor order"
        end = off + n
    assert end <= lay["total"] < end + align + world * chunk, "no more padding than the two roundings ask for"
    owner = [[0] * n for n in numels]              # how many slices name each element of each tensor
    flat = [0] * lay["total"]                      # how many slices name each flat index
    for rank in range(world):
        covered = 0
        for i, start, length, off in shard_slices(lay, rank):
            assert length > 0 and 0 <= start and start + length <= numels[i] and 0 <= off and off + length <= lay["shard"]
            assert off >= covered, "slices of a shard in order, not overlapping"
            covered = off + length
            assert rank * lay["shard"] + off == lay["offsets"][i] + start, "the two addresses of a slice agree"
            for k in range(length):
                owner[i][start + k] += 1
                flat[rank * lay["shard"] + off + k] += 1
    assert all(c == 1 for t in owner for c in t), "every element in exactly one rank's slices"
    assert sum(flat) == sum(numels) and max(flat) == 1, "padding in none"
    return lay


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("numels", TABLES, ids=lambda t: "x".join(map(str, t)) if len(t) < 4 else f"{len(t)}tensors_{t[0]}first")
def test_every_element_in_exactly_one_shard(numels, world):
    check(numels, world)


@pytest.mark.parametrize("world", WORLDS)
def test_unaligned_and_small_chunk_layouts(world):
    lay = check(NUMELS, world, align=1)
    assert lay["offsets"] == list(itertools.accumulate((0,) + NUMELS[:-1])), "align = 1 packs the tensors back to back"
    check(NUMELS, world, align=4, chunk=16)              # many shard boundaries inside tensors


def test_a_world_larger_than_the_data_leaves_ranks_empty():
    lay = check((1, 3, 63), 8)
    assert lay["shard"] == optim.CHUNK and [len(shard_slices(lay, r)) for r in range(8)] == [3, 0, 0, 0, 0, 0, 0, 0]
    lay = check((optim.CHUNK + 1,), 3)
    assert [len(shard_slices(lay, r)) for r in range(3)] == [1, 1, 0]


def test_bad_arguments_are_named():
    for kw in (dict(world=0), dict(world=2, align=0), dict(world=2, chunk=0)):
        with pytest.raises(ValueError, match="shard_layout"):
            shard_layout((4,), **kw)
    with pytest.raises(ValueError, match="at least one element"):
        shard_layout((4, 0), 2)
    with pytest.raises(ValueError, match="rank 2"):
        shard_slices(shard_layout((4,), 2), 2)


def test_the_chunk_is_the_kernels_chunk():
    assert optim.CHUNK == R.CHUNK


def test_the_header_and_the_binding_name_the_two_calls():
    header = open(os.path.join(R.ROOT, "include", "tokenpacker.h")).read()
    for name in ("tp_optim_sumsq", "tp_optim_apply"):
        assert f"int {name}(const tp_optim_tensor* t, int n," in header and name in _capi.EXPORTED_SYMBOLS
    assert "float grad_scale" in header and "const double* sums, int nsums" in header and "double* sumsq_out" in header
    assert callable(_capi.sharded_optim_supported)
    if os.path.exists(_capi.LIB_PATH):                   # (loading needs no GPU)
        assert _capi.sharded_optim_supported()
