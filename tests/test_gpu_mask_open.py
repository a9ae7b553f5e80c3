"""analysis.reliability_mask (of3d_mask_open) against the CPU labelling of mask_ref.open_ref:
the keep bits of every ROI and the four counts are integers fixed by the input, so every
comparison is exact."""
import numpy as np
import pytest
from scipy import ndimage

import mask_ref as mr
from opticalflow3d_dev_amd import reliability_mask

pytestmark = pytest.mark.gpu

CONN = {2: (4, 8), 3: (6, 18, 26)}


def rois_for(shape):
    """Two overlapping boxes with odd offsets (beside ROI 0, the whole volume)."""
    ny, nx = shape[-2:]
    a, b = (3, ny - 5, 5, nx - 7), (11, ny, 33, nx)
    if len(shape) == 2:
        return [a, b]
    nz = shape[0]
    return [(0, max(nz - 1, 1)) + a, (1, nz) + b]


def check(rel, min_size, connectivity, rois=None, **kw):
    """reliability_mask == open_ref: keep (so every ROI's bit plane) and the counts; returns both."""
    got = reliability_mask(rel, min_size=min_size, connectivity=connectivity, rois=rois, **kw)
    boxes = mr.boxes_of(rel.shape, rois)
    keep, counts = mr.open_ref(rel, got["threshold"], boxes, min_size, connectivity)
    assert np.array_equal(got["rois"], boxes)
    assert got["keep"].dtype == np.uint16 and got["keep"].shape == rel.shape
    for k in mr.COUNTS:
        assert got[k].dtype == np.int64 and np.array_equal(got[k], counts[k]), (k, got[k], counts[k])
    for r in range(len(boxes)):
        assert np.array_equal(got["mask"](r), (keep >> r) & 1 == 1), r
    assert np.array_equal(got["keep"], keep)
    return got, counts


@pytest.mark.parametrize("shape, dtype", [((37, 131), np.float32), ((5, 37, 131), np.float32),
                                          ((5, 37, 131), np.float64), ((24, 40, 72), np.float32)])
@pytest.mark.parametrize("percentile", [40, 70, 90])
def test_random_fields(shape, dtype, percentile):
    rel = np.random.default_rng(31).random(shape).astype(dtype)
    for conn in CONN[len(shape)]:
        for min_size in (1, 2, 5, 50):
            got, counts = check(rel, min_size, conn, rois_for(shape), rel_percentile=percentile)
            assert got["threshold"] == np.percentile(rel, percentile) and got["threshold"].dtype == dtype
            if min_size == 1:
                assert np.array_equal(got["n_kept"], got["n_mask"])
                assert np.array_equal(got["mask"](0), rel > got["threshold"])
    assert counts["n_components"][0] >= 1  # 40th percentile, 26 neighbours: one giant component


def test_smooth_blobs():
    rel = ndimage.gaussian_filter(np.random.default_rng(3).standard_normal((24, 40, 72)), 1.5).astype(np.float32)
    got, counts = check(rel, 10, 26, rois_for(rel.shape), rel_percentile=80)
    kept, removed = counts["n_components_kept"][0], counts["n_components"][0] - counts["n_components_kept"][0]
    print("components kept / removed:", kept, removed)
    assert kept >= 5 and removed >= 5


def test_checkerboard():
    rel = mr.checkerboard()
    got, _ = check(rel, 2, 6, threshold=0.5)
    assert got["n_components"] == 60 and got["n_kept"] == 0 and got["threshold"] == np.float32(0.5)
    for conn in (18, 26):
        got, _ = check(rel, 60, conn, threshold=0.5)
        assert got["n_components"] == 1 and got["n_kept"] == 60
        got, _ = check(rel, 61, conn, threshold=0.5)
        assert got["n_components"] == 1 and got["n_kept"] == 0


def test_serpentine():
    """Two snakes (planes 0 and 2) of 17 full rows joined alternately at either end: long
    union-find chains, and runs that cross waves and workgroups."""
    nz, ny, nx = 3, 33, 130
    rel = np.zeros((nz, ny, nx), np.float32)
    rel[0::2, 0::2, :] = 1
    rel[0::2, 1::4, nx - 1] = 1
    rel[0::2, 3::4, 0] = 1
    size = 17 * nx + 16
    got, _ = check(rel, size, 6, threshold=0.5)
    assert got["n_components"] == 2 and got["n_mask"] == 2 * size and got["n_kept"] == 2 * size
    got, _ = check(rel, size + 1, 6, threshold=0.5)
    assert got["n_components"] == 2 and got["n_components_kept"] == 0 and got["n_kept"] == 0


def test_no_wrap_around():
    """Voxels adjacent in linear index but not in space stay apart."""
    rel = np.zeros((6, 8), np.float32)
    rel[1, 7] = rel[2, 0] = rel[3, 7] = rel[4, 0] = 1
    got, _ = check(rel, 2, 8, threshold=0.5)
    assert got["n_components"] == 4 and got["n_kept"] == 0
    rel = np.zeros((3, 5, 6), np.float32)
    rel[0, 4, 1] = rel[1, 0, 1] = rel[1, 4, 4] = rel[2, 0, 4] = 1
    got, _ = check(rel, 2, 26, threshold=0.5)
    assert got["n_components"] == 4 and got["n_kept"] == 0


def test_box_truncation():
    rel, boxes = mr.u_shape()
    got, _ = check(rel, 15, 26, [tuple(boxes[1])], threshold=0.5)  # a = 10 < 15 <= 2a + base = 31
    assert got["n_components"].tolist() == [1, 2] and got["n_kept"].tolist() == [31, 0]
    assert np.array_equal(got["mask"](0), rel > 0.5) and not got["mask"](1).any()


def test_degenerate_cases():
    ones = np.ones((5, 7, 9), np.float32)
    got, _ = check(ones, 315, 26, threshold=0.5)
    assert got["n_components"] == 1 and got["n_kept"] == 315
    got, _ = check(ones, 316, 6, threshold=0.5)  # min_size larger than the volume
    assert got["n_components"] == 1 and got["n_kept"] == 0 and not got["keep"].any()
    got, _ = check(np.zeros((5, 7, 9), np.float64), 1, 18, threshold=0.5)
    assert got["n_mask"] == 0 and got["n_components"] == 0
    got, _ = check(ones, 1, 26, threshold=float("nan"))
    assert np.isnan(got["threshold"]) and got["n_mask"] == 0 and not got["keep"].any()
    rng = np.random.default_rng(8)
    rel = rng.random((5, 37, 131)).astype(np.float32)
    rel[rng.random(rel.shape) < 0.05] = np.nan
    rel[rng.random(rel.shape) < 0.05] = np.inf
    rel[rng.random(rel.shape) < 0.05] = -np.inf
    got, _ = check(rel, 3, 26, rois_for(rel.shape), threshold=0.6)
    assert 0 < got["n_kept"][0] < got["n_mask"][0]
    got, _ = check(rel, 3, 26, rel_percentile=50)  # a NaN percentile: nothing above it
    assert np.isnan(got["threshold"]) and got["n_mask"] == 0


def test_bad_arguments_raise():
    rel = np.zeros((4, 5, 6), np.float32)
    with pytest.raises(ValueError, match="connectivity"):
        reliability_mask(rel, connectivity=8)
    with pytest.raises(ValueError, match="connectivity"):
        reliability_mask(rel[0], connectivity=26)
    with pytest.raises(ValueError, match="min_size"):
        reliability_mask(rel, min_size=0)
    with pytest.raises(ValueError, match="outside the volume"):
        reliability_mask(rel, rois=[(0, 5, 0, 5, 0, 6)])


def test_deterministic_and_boxes_independent():
    import torch

    rel = np.random.default_rng(32).random((24, 40, 72)).astype(np.float32)
    t = torch.as_tensor(rel).cuda()
    a = reliability_mask(t, 70, min_size=5, rois=rois_for(rel.shape))
    b = reliability_mask(t, 70, min_size=5, rois=rois_for(rel.shape))
    alone = reliability_mask(t, 70, min_size=5)
    assert a["keep"].is_cuda and a["keep"].dtype == torch.uint16 and a["mask"](1).dtype == torch.bool
    ka, kb = a["keep"].cpu().numpy(), b["keep"].cpu().numpy()
    assert ka.tobytes() == kb.tobytes()
    assert np.array_equal(a["mask"](0).cpu().numpy(), alone["mask"](0).cpu().numpy())
    assert np.array_equal(alone["keep"].cpu().numpy(), ka & 1)
    for k in mr.COUNTS:
        assert np.array_equal(a[k], b[k]) and a[k][0] == alone[k][0], k
