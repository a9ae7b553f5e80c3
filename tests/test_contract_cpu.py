"""The contractility reference itself (tests/contract_ref.py), without a GPU: its largest
component is the notebook's sort-and-zero procedure, ties keep the lower label, and the inputs of
the GPU tests meet the conditions those tests rely on — no NaN that only the unclamped arccos
yields, no |dot| above 1 - 1e-6, no value within the margin of a bin edge."""
import numpy as np
import pytest
from scipy import ndimage

import contract_ref as cr
import mask_ref as mr


@pytest.mark.parametrize("name", ["random", "smooth", "checkerboard", "tie", "empty", "truncated"])
def test_largest_ref_is_the_notebooks_sort_and_zero(name):
    rel, boxes, thresh = cr.label_masks()[name]
    keep, counts = cr.largest_ref(rel, thresh, boxes, 26)
    for r, (z0, z1, y0, y1, x0, x1) in enumerate(boxes):
        crop = rel[z0:z1, y0:y1, x0:x1] > thresh
        assert np.array_equal((keep[z0:z1, y0:y1, x0:x1] >> r & 1).astype(bool), cr.notebook_largest(crop)), (name, r)
        assert counts["n_mask"][r] == crop.sum() and counts["n_kept"][r] <= crop.sum()
    outside = np.ones(rel.shape, bool)
    z0, z1, y0, y1, x0, x1 = boxes[1]
    outside[z0:z1, y0:y1, x0:x1] = False
    assert not (keep[outside] >> 1 & 1).any()


def test_2d_largest_ref_is_the_notebooks_procedure():
    rel, boxes, thresh = cr.label_masks_2d()["random2d"]
    keep, counts = cr.largest_ref(rel, thresh, boxes, 8)
    assert np.array_equal((keep & 1).astype(bool), cr.notebook_largest(rel > thresh))
    assert counts["n_components"][0] > 1 and counts["n_components_kept"][0] == 1


def test_a_tie_keeps_the_lower_label():
    rel, boxes, thresh = cr.label_masks()["tie"]
    keep, counts = cr.largest_ref(rel, thresh, boxes, 26)
    assert counts["n_components"].tolist() == [2, 1] and counts["n_kept"].tolist() == [6, 6]
    assert (keep[1] & 1).sum() == 6 and not (keep[3] & 1).any()  # the component met first in raster order
    assert (keep[3] >> 1 & 1).sum() == 6  # alone in its box, the other one is the largest
    rel, boxes, thresh = cr.label_masks()["truncated"]
    keep, counts = cr.largest_ref(rel, thresh, boxes, 26)
    assert counts["n_components"].tolist() == [1, 2] and counts["n_kept"].tolist() == [31, 10]
    assert (keep[2, :, 10] >> 1 & 1).sum() == 10 and not (keep[2, :, 20] >> 1 & 1).any()
    # every component of the checkerboard is one voxel at connectivity 6: the first voxel wins
    rel, boxes, thresh = cr.label_masks()["checkerboard"]
    keep, counts = cr.largest_ref(rel, thresh, boxes, 6)
    assert counts["n_kept"].tolist() == [1, 1] and keep[0, 0, 0] == 1 and keep[0, 1, 1] == 2


def test_an_empty_mask_keeps_nothing():
    rel, boxes, thresh = cr.label_masks()["empty"]
    keep, counts = cr.largest_ref(rel, thresh, boxes, 18)
    assert not keep.any() and all(not counts[k].any() for k in mr.COUNTS)


def _gpu_inputs():
    """(name, fields, keep, boxes, scales, center) of every contractility reduction the GPU tests
    compare against the reference."""
    for name, (f, rois, per) in (("general3d", cr.general3d()), ("general2d", cr.general2d())):
        boxes = cr.boxes_of(np.shape(f[0]), rois)
        for mode in ("largest", "summary"):
            yield name + "/" + mode, f, cr.mask_of(f[3], per, boxes, mode)[0], boxes, cr.SCALES, None
    f = cr.cube()
    boxes = cr.boxes_of(f[0].shape, [])
    yield "cube", f, cr.mask_of(f[3], 50, boxes, "largest")[0], boxes, dict(xyscale=1.0, zscale=1.0, tscale=1.0), None


@pytest.mark.parametrize("case", list(_gpu_inputs()), ids=lambda c: c[0])
def test_gpu_inputs_are_clear_of_the_edges_and_of_dot_1(case):
    name, f, keep, boxes, scales, center = case
    ref = cr.contract_ref(*f[:3], keep, boxes, **scales, center=center, bins=cr.BINS)
    raw = cr.contract_ref(*f[:3], keep, boxes, **scales, center=center, bins=cr.BINS, clamp=False)
    assert np.array_equal(ref["n_angle"], raw["n_angle"])  # the clamp removes no NaN on these inputs
    assert ref["n_angle"].sum() > 0
    for r in range(len(boxes)):
        assert np.all(np.abs(ref["dot"][r]) <= cr.DOT_LIMIT), (name, r)
        for k in cr.QUANTITIES:
            v = ref["values"][r][k]
            if v.size:
                assert np.min(np.abs(v[:, None] - cr.BINS[k][None, :])) > cr.EDGE_MARGIN, (name, r, k)
    slack = (180.0 / np.pi) * cr.K_DOT * cr.U / np.sqrt(1.0 - cr.DOT_LIMIT ** 2) + 16 * cr.U * 180.0
    assert slack < cr.EDGE_MARGIN


def test_the_cube_and_the_aligned_case_are_what_the_gpu_tests_expect():
    f = cr.cube()
    boxes = cr.boxes_of(f[0].shape, [])
    ref = cr.contract_ref(*f[:3], cr.mask_of(f[3], 50, boxes, "largest")[0], boxes)
    assert ref["moments"][0].tolist() == [27, 27 * 4, 27 * 3, 27 * 2] and ref["centroid"][0].tolist() == [4.0, 3.0, 2.0]
    assert ref["n_valid"][0] == 27 and ref["n_angle"][0] == 26  # the centroid voxel has no direction
    f, c, n_to, n_away = cr.aligned()
    boxes = cr.boxes_of(f[0].shape, [])
    keep = cr.mask_of(f[3], 50, boxes, "summary")[0]
    for clamp in (True, False):  # dot is exactly +-1: nothing for the clamp to do
        ref = cr.contract_ref(*f[:3], keep, boxes, 0.5, 2.0, 1.0, center=c, clamp=clamp)
        assert ref["n_valid"][0] == n_to + n_away + 1 and ref["n_angle"][0] == n_to + n_away
        assert sorted(set(ref["dot"][0].tolist())) == [-1.0, 1.0]
        assert sorted(set(ref["values"][0]["angle"].tolist())) == [0.0, 180.0]
        assert ref["sum_angle"][0] == 180.0 * n_away and ref["sum_dot"][0] == n_to - n_away


def test_center_of_mass_is_one_division_of_exact_integers():
    f, rois, per = cr.general3d()
    boxes = cr.boxes_of(f[0].shape, rois)
    keep = cr.mask_of(f[3], per, boxes, "largest")[0]
    ref = cr.contract_ref(*f[:3], keep, boxes, **cr.SCALES)
    m = ref["moments"].astype(np.float64)
    assert np.array_equal(ref["centroid"], m[:, 1:] / m[:, :1])
    with np.errstate(invalid="ignore"):
        assert np.isnan(ndimage.center_of_mass(np.zeros((2, 2, 2), int))).all()  # an empty mask: NaN
