"""The streaming driver's device-free parts (stream.py): the slab geometry against shard's
bounds and by hand, the output layout, and the buffer table with the memory fit that sums it
(the byte arithmetic of test_gpu_k0batch.py::test_flowstream_fits_device_memory, no GPU)."""
from functools import partial

import numpy as np
import pytest

from opticalflow3d_dev_amd import radii
from opticalflow3d_dev_amd.shard import halo_planes, zslab_bounds
from opticalflow3d_dev_amd.stream import _fit_device_memory, _Slab, buffer_table, device_bytes, output_layout

VOL = (30, 20, 24)
U16, F32, F64, I64 = (np.dtype(t) for t in (np.uint16, np.float32, np.float64, np.int64))


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("rd,rw", [radii(2, 2, 5)[::3], (1, 2)])  # (6, 15): a halo past the volume; (1, 2): within
def test_slab_geometry(rd, rw, world, axis):
    nz, ny, nx = VOL
    n = VOL[axis]
    covered = 0
    for rank in range(world):
        g = _Slab.of(VOL, 3, (rank, world, None, axis), rd, rw)
        a0, a1 = zslab_bounds(n, rank, world)
        ai0, ai1 = halo_planes(n, a0, a1, rd, rw)
        assert (g.axis, g.n, g.a0, g.a1, g.ai0, g.ai1) == (axis, n, a0, a1, ai0, ai1)
        assert ai0 == max(a0 - rd - rw, 0) and ai1 == min(a1 + rd + rw, n)
        covered += g.a1 - g.a0
        if axis == 0:  # planes: contiguous in a slot, the plan of the whole volume told its planes
            assert g.shape == (a1 - a0, ny, nx) and g.nvox == (a1 - a0) * ny * nx
            assert g.nblock == (ai1 - ai0) * ny * nx and g.own0 == (a0 - ai0) * ny * nx
            assert (g.plan_dims, g.max_out_planes, g.rows) == (VOL, a1 - a0, None)
            assert (g.frame_z0, g.zo0, g.zo1) == (ai0, a0, a1)
        else:  # rows: a plan of the rows + halo as a volume of its own, all of its planes
            assert g.shape == (nz, a1 - a0, nx) and g.nvox == nz * (a1 - a0) * nx
            assert g.nblock == nz * (ai1 - ai0) * nx and g.own0 == 0
            assert (g.plan_dims, g.max_out_planes, g.rows) == ((nz, ai1 - ai0, nx), 0, (a0 - ai0, a1 - ai0))
            assert (g.frame_z0, g.zo0, g.zo1) == (0, 0, nz)
        # the views: a slot numbered by global (z, y, x); the block has the split axis first
        ext = (ai1 - ai0, ny, nx) if axis == 0 else (nz, ai1 - ai0, nx)
        lo = (ai0, 0, 0) if axis == 0 else (0, ai0, 0)
        z, y, x = np.meshgrid(*(np.arange(l, l + e) for l, e in zip(lo, ext)), indexing="ij")
        slot = np.concatenate([((z * ny + y) * nx + x).reshape(-1), [-1, -1]])  # longer than the block
        want = np.arange(nz * ny * nx).reshape(VOL)
        own = want[a0:a1] if axis == 0 else want[:, a0:a1]
        assert g.own(slot).shape == g.shape and np.array_equal(g.own(slot), own)
        blk = g.block(slot)
        assert blk.shape[0] == ai1 - ai0 and np.shares_memory(blk, slot)
        assert np.array_equal(blk, want[ai0:ai1] if axis == 0 else want[:, ai0:ai1].swapaxes(0, 1))
    assert covered == n


def test_slab_geometry_by_hand():
    # 30 planes over 3 ranks with a halo of 1 + 2: rank 1 owns [10, 20) and reads [7, 23)
    g = _Slab.of(VOL, 3, (1, 3, None), 1, 2)
    assert g == (0, 30, 10, 20, 7, 23, (10, 20, 24), 4800, 7680, 1440, VOL, 10, None, 7, 10, 20)
    # 20 rows over 3 ranks (7, 7, 6): rank 2 owns [14, 20) and reads [11, 20), its rows 3 .. 8 of 9
    g = _Slab.of(VOL, 3, (2, 3, None, 1), 1, 2)
    assert g == (1, 20, 14, 20, 11, 20, (30, 6, 24), 4320, 6480, 0, (30, 9, 24), 0, (3, 9), 0, 0, 30)
    whole = _Slab.of(VOL, 3, None, 6, 15)
    assert whole == (0, 30, 0, 30, 0, 30, VOL, 14400, 14400, 0, VOL, 0, None, 0, 0, 30)
    flat = _Slab.of((40, 48), 2, None, 6, 15)  # 2-D: one plane, frames pushed as (ny, nx)
    assert flat == (0, 1, 0, 1, 0, 1, (40, 48), 1920, 1920, 0, (1, 40, 48), 0, None, 0, 0, 1)
    assert flat.own(np.arange(1921)).shape == (40, 48)
    empty = _Slab.of((0, 5, 6), 3, None, 1, 2)
    assert empty.nvox == 0 and empty.block(np.zeros(1)) is None


def test_slab_split_errors():
    with pytest.raises(ValueError, match="slab split of 20 planes over 21 ranks leaves empty slabs"):
        _Slab.of(VOL, 3, (0, 21, None, 1), 6, 15)
    with pytest.raises(ValueError, match="slab split of 30 planes over 31 ranks leaves empty slabs"):
        _Slab.of(VOL, 3, (30, 31, None), 6, 15)
    with pytest.raises(ValueError, match="z-slabs need a 3D volume"):
        _Slab.of((40, 48), 2, (0, 2, None), 6, 15)


@pytest.mark.parametrize("ndim,precision,rel_fp64,want", [
    (3, "fp64", False, (4, F64, F32)), (3, "fp64", True, (4, F64, F64)),
    (2, "fp64", False, (3, F64, F64)), (2, "fp64", True, (3, F64, F64)),
    (3, "fp32", False, (4, F32, F32)), (2, "fp32", False, (3, F32, F32)),
    (3, "fp32", True, (4, F32, F32)), (2, "fp32", True, (3, F32, F32))])
def test_output_layout(ndim, precision, rel_fp64, want):
    assert output_layout(ndim, precision, rel_fp64) == want


def test_output_layout_refuses_other_precisions():
    with pytest.raises(ValueError, match="precision must be 'fp64'"):
        output_layout(3, "fp16", False)


NWIN = 13
SHAPE = (24, 40, 48)
VOX = 24 * 40 * 48
SLOT, OSET = VOX * 2, VOX * (3 * 8 + 4)  # as test_flowstream_fits_device_memory counts them


def _whole_table(**kw):
    return partial(buffer_table, _Slab.of(SHAPE, 3, None, 6, 15), NWIN, U16, output_layout(3, "fp64", False), **kw)


def test_buffer_table_whole_volume():
    table = _whole_table()
    for depth in (1, 2, 3):
        for L in (0, 1, 4):
            assert device_bytes(table(depth, L)) == SLOT * (NWIN + 1 + L) + depth * OSET
    rows = {b.name: b for b in table(3, 4)}
    assert sorted(rows) == ["dout", "hout", "ring", "stage"]
    assert rows["ring"] == ("ring", False, NWIN + 5, VOX, (U16,))
    assert rows["stage"] == ("stage", True, 2, VOX, (U16,))
    assert rows["dout"] == ("dout", False, 3, VOX, (F64, F64, F64, F32))
    assert rows["hout"] == rows["dout"]._replace(name="hout", pinned=True)
    assert rows["hout"].nbytes == 3 * OSET


@pytest.mark.parametrize("extra,want", [(None, (3, 5, 4)), (1, (1, 2, 1)), (0, (1, 0, 0))])
def test_fit_device_memory(extra, want):
    """Fewer output sets first, then K0 batching 5 -> 2 -> none: the free sizes of
    test_flowstream_fits_device_memory (less its 1 GiB margin)."""
    free = 1 << 40 if extra is None else SLOT * (NWIN + 1 + extra) + OSET + 1024
    assert _fit_device_memory(_whole_table(), 3, 5, 4, free) == want
    assert _fit_device_memory(_whole_table(), 3, 0, 1, free) == (want[0], 0, min(want[2], 1))  # frame pipelining


def test_fit_device_memory_raises_below_one_set():
    free = SLOT * (NWIN + 1) + OSET - 1
    with pytest.raises(MemoryError, match=r"FlowStream: 0\.0 GiB of frames and outputs do not fit the 0\.0 GiB "
                                          r"left on device 2"):
        _fit_device_memory(_whole_table(), 3, 5, 4, free, 2)
    assert _fit_device_memory(_whole_table(), 3, 5, 4, free + 1) == (1, 0, 0)


def test_buffer_table_row_slab_charges_dfull_only_when_allocated():
    g = _Slab.of(VOL, 3, (1, 3, None, 1), 1, 2)  # rows [7, 14) of 20, reads [4, 17)
    layout = output_layout(3, "fp64", False)
    direct = buffer_table(g, NWIN, U16, layout, 2, 0)
    fallback = buffer_table(g, NWIN, U16, layout, 2, 0, dfull=True)
    block = 30 * 13 * 24
    assert g.nblock == block and g.nvox == 30 * 7 * 24
    assert device_bytes(fallback) - device_bytes(direct) == block * (3 * 8 + 4)  # one sub-volume output set
    assert [b for b in fallback if b not in direct] == [("dfull", False, 1, block, (F64, F64, F64, F32))]
    # ring slots of the block, one device staging buffer and the output sets of the own rows
    assert device_bytes(direct) == (NWIN + 1) * block * 2 + g.nvox * 2 + 2 * g.nvox * 28
    planes = buffer_table(_Slab.of(VOL, 3, (1, 3, None, 0), 1, 2), NWIN, U16, layout, 2, 0)
    assert "dstage" not in [b.name for b in planes]


def test_buffer_table_without_full_size_fields():
    none = _whole_table(fields=False)(3, 4)
    assert sorted(b.name for b in none) == ["dout", "ring", "stage"]
    assert [b.name for b in none if b.pinned] == ["stage"]
    spec = _whole_table(fields=False, export_bytes=4096)(3, 4)
    assert [(b.name, b.count, b.elems, b.dtypes) for b in spec if b.pinned] == [
        ("stage", 2, VOX, (U16,)), ("hexport", 3, 512, (I64,))]
    assert device_bytes(spec) == device_bytes(none) + 3 * 4096  # one export block per output set
