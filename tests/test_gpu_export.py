"""The field export on the device (analysis.export_fields, csrc/kt_export.hip) against the numpy
restatement (tests/export_ref.py): every value bit for bit where it is not NaN, NaNs in the same
places; mode None compared as bytes.  The shapes are the smallest at which the kernel's
partition can go wrong: odd x0 and dx (every row starts elsewhere inside a 16-byte group of
output), several workgroups, a ragged tail, rows shorter than a group, one voxel.

Non-vacuity is asserted on the reference in every masked case: 0 < inside < voxels for every
exported ROI of more than one voxel (a one-voxel box cannot be partly masked)."""
import functools

import numpy as np
import pytest

import export_ref as er
import quiver_ref as qr
import summary_ref as sr
from opticalflow3d_dev_amd import FieldSpec, export_fields

pytestmark = pytest.mark.gpu

KW = dict(rel_percentile=60, xyscale=0.3, zscale=1.2, tscale=0.5)
MASKS = [None, "nan", "zero", "summary"]
DTYPES = [None, "float32"]

# (volume, ROIs, exported ROI indices)
SEAMS = [
    ((6, 50, 301), [(1, 5, 3, 47, 7, 290)], (1, 0)),   # several workgroups; and the whole volume as box 0
    ((2, 3, 70), [(0, 2, 1, 3, 3, 70)], (1,)),         # one workgroup, ragged tail
    ((3, 7, 5), [(0, 3, 1, 7, 0, 5)], (1,)),           # rows shorter than a store group
    ((4, 9, 11), [(2, 3, 4, 5, 6, 7)], (1,)),          # one voxel
]
FLAT = [
    ((33, 45), [(3, 25, 2, 17), (32, 33, 0, 45)], (1, 2)),
    ((2, 20000), [(1, 2, 19990, 20000)], (1,)),
]


@functools.lru_cache(maxsize=None)
def fields_of(shape, v_dtype=np.float64, rel_dtype=np.float32):
    return tuple(qr.planted_fields(shape, 21, v_dtype=v_dtype, rel_dtype=rel_dtype))  # shared: never written to


def reference(f, rois, export_rois, mask, dtype, fields=None, physical=True, **kw):
    ref = er.export_ref(*f, **dict(KW, **kw), rois=rois, export_rois=export_rois, fields=fields, mask=mask,
                        physical=physical, dtype=dtype)
    if mask is not None:
        for blk, n in zip(ref["blocks"], ref["inside"]):
            size = int(np.prod([blk["box"][2 * a + 1] - blk["box"][2 * a] for a in range(3)]))
            assert size == 1 or 0 < n < size, (blk["roi"], n, size)
    return ref


def run(f, rois, export_rois, mask, dtype, fields=None, physical=True, **kw):
    spec = FieldSpec(rois=export_rois, mask=mask, dtype=dtype, physical=physical,
                     **({} if fields is None else {"fields": fields}))
    got = export_fields(*f, **dict(KW, **kw), rois=rois, spec=spec)
    ref = reference(f, rois, export_rois, mask, dtype, fields, physical, **kw)
    er.assert_blocks(got, ref, bytes_exact=mask is None and not physical)
    return got, ref


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mask", MASKS)
def test_partition_and_alignment_seams(mask, dtype):
    for shape, rois, export_rois in SEAMS:
        got, _ = run(fields_of(shape), rois, export_rois, mask, dtype)
        for blk in got["blocks"]:
            assert blk["vx"].dtype == (np.float32 if dtype else np.float64) and blk["rel"].dtype == np.float32
            assert blk["vx"].shape == tuple(blk["box"][2 * a + 1] - blk["box"][2 * a] for a in range(3))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mask", MASKS)
def test_plain_crops_are_bit_copies(mask, dtype):
    """Without physical units: mode None in the fields' own types is the slice's bytes."""
    shape, rois, export_rois = SEAMS[0]
    run(fields_of(shape), rois, export_rois, mask, dtype, physical=False)
    run(fields_of(shape, np.float32, np.float64), rois, export_rois, mask, dtype, physical=False)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mask", ["nan", "summary"])
@pytest.mark.parametrize("v_dtype,rel_dtype", [(np.float32, np.float64), (np.float64, np.float32),
                                               (np.float32, np.float32), (np.float64, np.float64)])
def test_field_types(v_dtype, rel_dtype, mask, dtype):
    shape, rois, export_rois = (5, 11, 37), [(1, 4, 2, 11, 3, 36)], (1,)
    got, _ = run(fields_of(shape, v_dtype, rel_dtype), rois, export_rois, mask, dtype)
    blk = got["blocks"][0]
    assert blk["vx"].dtype == (np.float32 if dtype or v_dtype == np.float32 else np.float64)
    assert blk["rel"].dtype == (np.float32 if dtype else rel_dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mask", MASKS)
def test_2d(mask, dtype):
    for shape, rois, export_rois in FLAT:
        got, _ = run(fields_of(shape, np.float64, np.float64), rois, export_rois, mask, dtype)
        for blk in got["blocks"]:
            assert list(blk) == ["roi", "box", "vx", "vy", "rel"] and blk["vx"].ndim == 2
    with pytest.raises(ValueError, match="no vz"):
        export_fields(*fields_of((33, 45), np.float64, np.float64), spec=FieldSpec(fields=("vx", "vz")))


def special_fields():
    """(4, 6, 10) float64 fields with -0.0, inf, -inf, a NaN with a payload and exact zeros planted
    in vx both inside and outside the mask rel > 0.5 (x < 5 is inside)."""
    rng = np.random.default_rng(3)
    shape = (4, 6, 10)
    vx, vy, vz = (rng.standard_normal(shape) for _ in range(3))
    rel = np.where(np.arange(10) < 5, 0.75, 0.25).astype(np.float32) * np.ones(shape, np.float32)
    payload = np.array([0x7FF8000000000123, 0xFFF80000DEADBEEF], dtype=np.uint64).view(np.float64)
    for x in (2, 7):  # inside, outside
        vx[1, 1, x], vx[1, 2, x], vx[1, 3, x], vx[1, 4, x] = -0.0, np.inf, -np.inf, 0.0
        vx[2, 1, x], vx[2, 2, x], vx[2, 3, x] = payload[0], payload[1], -3.0
    return vx, vy, vz, rel


@pytest.mark.parametrize("dtype", DTYPES)
def test_special_values(dtype):
    f = special_fields()
    rois = [(1, 3, 1, 5, 1, 9)]
    kw = dict(threshold=0.5)
    got = {}
    for mask in MASKS:
        for physical in (False, True):
            got[mask, physical] = run(f, rois, (1,), mask, dtype, physical=physical, **kw)[0]["blocks"][0]["vx"]
    # the box starts at (1, 1, 1): vx[1, y, x] is block [0, y - 1, x - 1]
    inside, outside = 1, 6
    if dtype is None:  # the bit copy keeps the payloads and the sign of zero
        want = np.ascontiguousarray(f[0][1:3, 1:5, 1:9])
        assert got[None, False].tobytes() == want.tobytes()
        assert got[None, False].view(np.uint64)[1, 0, inside] == 0x7FF8000000000123
        assert got[None, False].view(np.uint64)[1, 1, outside] == 0xFFF80000DEADBEEF
    zero = got["zero", False]
    assert zero[1, 2, outside] == 0 and np.signbit(zero[1, 2, outside])   # -3.0 * 0.0 is -0.0
    assert zero[1, 2, inside] == -3.0
    assert np.isnan(zero[0, 1, outside]) and np.isnan(zero[0, 2, outside])  # inf * 0.0 is NaN
    assert zero[0, 1, inside] == np.inf and zero[0, 2, inside] == -np.inf
    assert zero[0, 0, inside] == 0 and np.signbit(zero[0, 0, inside])      # -0.0 * 1.0
    assert zero[0, 3, inside] == 0 and not np.signbit(zero[0, 3, inside])
    summary = got["summary", False]
    assert np.isnan(summary[0, 0, inside]) and np.isnan(summary[0, 3, inside])  # exact zeros -> NaN
    assert np.isnan(summary[1, 2, outside]) and summary[1, 2, inside] == -3.0
    nan = got["nan", True]
    want = -3.0 * KW["xyscale"] / KW["tscale"]
    assert np.isnan(nan[:, :, 4:]).all() and nan[1, 2, inside] == (np.float32(want) if dtype else want)
    assert nan[0, 3, inside] == 0  # "nan" keeps a zero inside the mask


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mask", ["nan", "zero", "summary"])
def test_opened_masks_are_read_per_box(mask, dtype):
    """min_size drops components, and two overlapping ROIs, whose opened masks differ on the
    overlap (a component is cut differently by each box), each get their own bit of the keep
    volume; ROI 0 is listed and skipped."""
    shape, rois = (5, 20, 40), [(0, 5, 0, 20, 0, 25), (0, 5, 0, 20, 15, 40)]
    f = fields_of(shape)
    kw = dict(rel_percentile=80, min_size=4, connectivity=6)
    boxes = sr.boxes_of(shape, rois)
    thresh, opened = er.masks_of(f[3], boxes, 80, None, 4, 6)
    plain = f[3] > thresh
    overlap = (slice(None), slice(None), slice(15, 25))
    assert (opened[1][overlap] != opened[2][overlap]).any()
    for r in (1, 2):
        sl = tuple(slice(boxes[r][2 * a], boxes[r][2 * a + 1]) for a in range(3))
        assert 0 < opened[r][sl].sum() < plain[sl].sum()  # the opening dropped components, and kept some
    run(f, rois, (1, 2), mask, dtype, **kw)
    run(f, rois, (2,), mask, dtype, **kw)


def sixteen_boxes():
    out = []
    for k in range(15):
        z0, y0, x0 = k % 3, k % 4, (3 * k) % 7
        out.append((z0, z0 + 2 + k % 2, y0, y0 + 5 + k % 3, x0, x0 + 4 + k % 5))
    return out


@pytest.mark.parametrize("mask,dtype", [("nan", None), ("summary", "float32")])
def test_sixteen_boxes_at_once(mask, dtype):
    got, _ = run(fields_of((5, 10, 15)), sixteen_boxes(), tuple(range(16)), mask, dtype)
    assert [b["roi"] for b in got["blocks"]] == list(range(16))
    run(fields_of((5, 10, 15)), sixteen_boxes(), (15, 3, 8), mask, dtype, min_size=1)


@pytest.mark.parametrize("mask,dtype", [("zero", None), ("nan", "float32")])
def test_field_subset(mask, dtype):
    shape, rois, export_rois = SEAMS[0]
    got, _ = run(fields_of(shape), rois, export_rois, mask, dtype, fields=("vz", "rel"))
    assert all(list(b) == ["roi", "box", "vz", "rel"] for b in got["blocks"])
    got, _ = run(fields_of(shape), rois, (1,), mask, dtype, fields=("rel",))
    assert list(got["blocks"][0]) == ["roi", "box", "rel"]


@pytest.mark.parametrize("mask,dtype", [("nan", None), ("summary", "float32"), (None, None)])
def test_torch_inputs_stay_on_the_device(mask, dtype):
    import torch

    shape, rois, export_rois = SEAMS[0]
    f = fields_of(shape)
    spec = FieldSpec(rois=export_rois, mask=mask, dtype=dtype)
    host = export_fields(*f, **KW, rois=rois, spec=spec)
    dev = export_fields(*(torch.from_numpy(a.copy()).cuda() for a in f), **KW, rois=rois, spec=spec)
    assert dev["threshold"] == host["threshold"]
    for h, d in zip(host["blocks"], dev["blocks"]):
        assert h["roi"] == d["roi"] and h["box"] == d["box"]
        for name in ("vx", "vy", "vz", "rel"):
            assert isinstance(d[name], torch.Tensor) and d[name].is_cuda and isinstance(h[name], np.ndarray)
            assert d[name].cpu().numpy().tobytes() == h[name].tobytes() and tuple(d[name].shape) == h[name].shape
