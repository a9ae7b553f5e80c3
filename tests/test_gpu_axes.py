"""The mask's principal axes and the projected flow on the device (of3d_mask_axes) against
axes_ref: integer moments exactly, the covariance against exact fractions, the
eigen-decomposition against the device's own covariance and np.linalg.eigh, the projection's
histograms exactly with the host restating the device's expression tree on the downloaded
axes, given axes, determinism, degenerate masks, and that nothing else moved.

Shapes: (9, 23, 70) — rows of 70 split over two 64-lane segments, the whole volume spans two
workgroups of the projection — with the ROI (1, 8, 3, 21, 5, 69), and the 2D (23, 70)."""
from fractions import Fraction

import numpy as np
import pytest
from scipy import ndimage

import axes_ref as ar
import mask_ref as mr
from conftest import bits_equal
from opticalflow3d_dev_amd import SummarySpec, analysis, calc_flow3D, flow_summary, principal_axes, process_flow
from opticalflow3d_dev_amd import tiff as tf
from opticalflow3d_dev_amd.analysis import AXIS_NAMES, CSV_AXES_COLUMNS, CSV_COLUMNS, read_summary_csv

pytestmark = pytest.mark.gpu

SHAPE3, ROI3 = (9, 23, 70), (1, 8, 3, 21, 5, 69)
SHAPE2, ROI2 = (23, 70), (3, 21, 5, 69)
PCT = 70
SCALES = dict(xyscale=0.1, zscale=0.3, tscale=2.0)


def smooth(seed, shape, dtype=np.float64):
    return ndimage.gaussian_filter(np.random.default_rng(seed).standard_normal(shape), 1.5).astype(dtype)


@pytest.fixture(scope="module")
def vol3():
    """rel (float64 blob; float32 copies are taken per test), vx, vy, vz of SHAPE3."""
    return ar.blob(SHAPE3, 7), smooth(70, SHAPE3), smooth(71, SHAPE3), smooth(72, SHAPE3)


@pytest.fixture(scope="module")
def vol2():
    return ar.blob(SHAPE2, 7), smooth(80, SHAPE2), smooth(81, SHAPE2)


def ref_masks(rel, rois, min_size, connectivity):
    """(boxes, threshold, [cropped boolean mask per box]) of the host: rel > percentile, opened."""
    boxes = mr.boxes_of(rel.shape, rois)
    thresh = np.percentile(rel, PCT)
    if min_size:
        keep, _ = mr.open_ref(rel, thresh, boxes, min_size, connectivity)
        keep = keep.reshape((1,) + keep.shape) if keep.ndim == 2 else keep
        masks = [((ar.box_mask(keep, b) >> np.uint16(r)) & np.uint16(1)).astype(bool) for r, b in enumerate(boxes)]
    else:
        masks = [ar.box_mask(rel > thresh, b) for b in boxes]
    return boxes, thresh, masks


def check_mask_part(got, boxes, masks):
    """Moments exactly; centroid within 2 ulp and covariance within 1e-14 of the fractions; the
    eigen-decomposition against the device's own covariance."""
    for r, (box, m) in enumerate(zip(boxes, masks)):
        mom = ar.int_moments(m)
        assert got["moments"].dtype == np.uint64 and [int(v) for v in got["moments"][r]] == mom, (r, mom)
        assert int(got["n_axes_mask"][r]) == mom[0]
        cen, cov = ar.exact_stats(mom, box)
        for i in range(3):
            d = ar.ulp_distance(got["centroid"][r, i], cen[i])
            print("roi", r, "centroid", "xyz"[i], "ulp", d)
            assert d <= 2
            for j in range(3):
                g, want = got["covariance"][r, i, j], cov[i][j]
                if want == 0:
                    assert g == 0.0, (r, i, j, g)
                else:
                    err = abs(Fraction(float(g)) - want) / abs(want)
                    print("roi", r, "cov", i, j, "rel err", float(err))
                    assert err <= Fraction(1, 10 ** 14), (r, i, j, float(err))
        check_eigen(got["covariance"][r], got["axis_values"][r], got["axis_vectors"][r])


def check_eigen(C, lam, vec, compare_vectors=False):
    l1 = lam[0]
    assert lam[0] >= lam[1] >= lam[2] >= 0
    for k in range(3):
        res = np.linalg.norm(C @ vec[k] - lam[k] * vec[k])
        assert res <= 1e-10 * l1, (k, res)
        for j in range(3):
            assert abs(vec[j] @ vec[k] - (j == k)) <= 1e-10, (j, k)
        big = np.argmax(np.abs(vec[k]))
        assert vec[k][big] > 0
    w, v = ar.eigh_axes(C)
    assert np.all(np.abs(lam - w) <= 1e-10 * max(l1, w[0]))
    if compare_vectors:
        # meaningful only for a separated spectrum and a sign rule away from a tie: asserted on the reference
        assert w[0] - w[1] >= 0.05 * w[0] and w[1] - w[2] >= 0.05 * w[0]
        srt = np.sort(np.abs(v), axis=1)
        assert np.all(srt[:, 2] - srt[:, 1] >= 0.5)
        print("eigh gaps", (w[0] - w[1]) / w[0], (w[1] - w[2]) / w[0], "max |dv|", np.max(np.abs(vec - v)))
        assert np.all(np.abs(vec - v) <= 1e-10)


# ---- integer moments, covariance, centroid, eigen-decomposition --------------------------------
@pytest.mark.parametrize("rel_dtype", [np.float32, np.float64])
@pytest.mark.parametrize("min_size,connectivity", [(0, None), (1, 26), (50, 26), (50, 6)])
def test_mask_part_3d(vol3, rel_dtype, min_size, connectivity):
    rel = vol3[0].astype(rel_dtype)
    boxes, thresh, masks = ref_masks(rel, [ROI3], min_size, connectivity)
    got = principal_axes(rel, PCT, min_size=min_size, connectivity=connectivity, rois=[ROI3])
    assert got["threshold"] == thresh and np.array_equal(got["rois"], boxes)
    check_mask_part(got, boxes, masks)
    for r in range(2):
        check_eigen(got["covariance"][r], got["axis_values"][r], got["axis_vectors"][r], compare_vectors=True)
    if min_size:
        assert np.array_equal(got["n_kept"], got["n_axes_mask"])
    if connectivity == 6:
        assert np.all(got["n_components"] > got["n_components_kept"])  # the opening removed something


@pytest.mark.parametrize("min_size,connectivity", [(0, None), (6, 8), (6, 4)])
def test_mask_part_2d(vol2, min_size, connectivity):
    rel = vol2[0].astype(np.float32)
    boxes, _, masks = ref_masks(rel, [ROI2], min_size, connectivity)
    got = principal_axes(rel, PCT, min_size=min_size, connectivity=connectivity, rois=[ROI2])
    check_mask_part(got, boxes, masks)
    for r in range(2):  # the same code in 2D: the third axis is z with eigenvalue 0
        assert got["axis_values"][r, 2] == 0.0 and got["axis_vectors"][r, 2].tolist() == [0.0, 0.0, 1.0]
        assert got["axis_vectors"][r, 0, 2] == 0.0 and got["axis_vectors"][r, 1, 2] == 0.0


def test_covariance_is_not_a_float_shortcut():
    """A slab 3 voxels thick at x in [2900, 2902]: variance 2/3 under a squared mean of 8.4e6;
    sum(xx)/n - mean^2 in float64 is off by about 1e-9 relative there."""
    rel = np.zeros((2, 3, 3000), np.float32)
    rel[:, :, 2900:2903] = 1
    got = principal_axes(rel, threshold=0.5)
    boxes = mr.boxes_of(rel.shape, None)
    check_mask_part(got, boxes, [rel > 0.5])
    assert got["covariance"][0, 0, 0] == 2 / 3 and got["covariance"][0, 1, 1] == 2 / 3
    assert got["covariance"][0, 2, 2] == 0.25
    assert got["centroid"][0].tolist() == [2901.0, 1.0, 0.5]
    n, sx, sxx = (float(v) for v in got["moments"][0][[0, 1, 4]])
    naive = sxx / n - (sx / n) ** 2
    assert abs(naive - 2 / 3) / (2 / 3) > 1e-12  # the shortcut this test is built to expose


def test_physical_axes(vol3):
    rel = vol3[0].astype(np.float32)
    plain = principal_axes(rel, PCT, rois=[ROI3])
    phys = principal_axes(rel, PCT, rois=[ROI3], physical=True, xyscale=0.1, zscale=0.3)
    s = np.array([0.1, 0.1, 0.3])
    assert bits_equal(plain["moments"], phys["moments"]) and bits_equal(plain["centroid"], phys["centroid"])
    for r in range(2):
        want = np.triu((s[:, None] * plain["covariance"][r]) * s[None, :])  # (s_a * C_ab) * s_b for a <= b
        assert np.array_equal(np.triu(phys["covariance"][r]), want)
        assert np.array_equal(phys["covariance"][r], phys["covariance"][r].T)
        check_eigen(phys["covariance"][r], phys["axis_values"][r], phys["axis_vectors"][r])


# ---- the projection ----------------------------------------------------------------------------
def axis_bins_for(a, nbins):
    return np.linspace(-a, a, nbins + 1)


def check_projection(vx, vy, vz, rel, rois, min_size, connectivity, axis_bins, axes="mask"):
    got = flow_summary(vx, vy, vz, rel, PCT, rois=rois, min_size=min_size, connectivity=connectivity, axes=axes,
                       axis_bins=axis_bins, **SCALES)
    boxes, _, masks = ref_masks(rel, rois, min_size, connectivity)
    check_mask_part(got, boxes, masks)
    ref = ar.projection_ref(vx, vy, vz, masks, boxes, got["axes_used"], bins=axis_bins, **SCALES)
    assert np.array_equal(got["n_axes_valid"], ref["n_valid"]) and np.array_equal(got["n_axes_valid"], got["n_valid"])
    assert np.all(got["n_valid"] > 0)
    for a in AXIS_NAMES:
        bound = (ref["n_valid"] + 16) * 2.0 ** -53 * ref["abs_sum_" + a]  # summary_ref.sum_bound's rule
        err = np.abs(got["sum_" + a] - ref["sum_" + a])
        print(a, "max err / bound", float(np.max(err / np.maximum(bound, 1e-300))))
        assert np.all(err <= bound), (a, err, bound)
        assert np.array_equal(got["mean_" + a], got["sum_" + a] / got["n_valid"])
    assert set(ref["hist"]) == set(axis_bins)
    for a in axis_bins:
        assert got["hist"][a].dtype == np.uint64 and np.array_equal(got["hist"][a], ref["hist"][a]), a
        assert np.array_equal(got["edges"][a], axis_bins[a])
        assert got["hist"][a].sum() > 0
    return got


@pytest.mark.parametrize("v_dtype", [np.float64, np.float32])
@pytest.mark.parametrize("min_size,connectivity", [(0, None), (50, 6)])
def test_projection_3d(vol3, v_dtype, min_size, connectivity):
    rel, vx, vy, vz = vol3
    cast = lambda a: a.astype(v_dtype)
    bins = {"axis1": axis_bins_for(0.004, 14), "axis2": axis_bins_for(0.003, 14), "axis3": axis_bins_for(0.01, 256)}
    got = check_projection(cast(vx), cast(vy), cast(vz), rel.astype(np.float32), [ROI3], min_size, connectivity, bins)
    assert np.all(got["axes_used"] == got["axis_vectors"])


@pytest.mark.parametrize("v_dtype", [np.float64, np.float32])
def test_projection_2d(vol2, v_dtype):
    rel, vx, vy = vol2
    bins = {"axis1": axis_bins_for(0.004, 256), "axis2": axis_bins_for(0.003, 14)}
    check_projection(vx.astype(v_dtype), vy.astype(v_dtype), None, rel, [ROI2], 0, None, bins)
    check_projection(vx.astype(v_dtype), vy.astype(v_dtype), None, rel.astype(np.float32), [ROI2], 6, 8, bins)


def test_given_axes_identity(vol3):
    rel, vx, vy, vz = vol3
    rel = rel.astype(np.float32)
    e = {"x": np.linspace(-0.004, 0.004, 15), "y": np.linspace(-0.003, 0.003, 15), "z": np.linspace(-0.01, 0.01, 257)}
    got = flow_summary(vx, vy, vz, rel, PCT, rois=[ROI3], bins={"vx": e["x"], "vy": e["y"], "vz": e["z"]},
                       axes=np.eye(3), axis_bins={"axis1": e["x"], "axis2": e["y"], "axis3": e["z"]}, **SCALES)
    own = flow_summary(vx, vy, vz, rel, PCT, rois=[ROI3], axes="mask", **SCALES)
    for a, c in zip(AXIS_NAMES, "xyz"):
        assert np.array_equal(got["hist"][a], got["hist"]["v" + c]) and got["hist"][a].sum() > 0
        assert bits_equal(got["sum_" + a], got["sum_v" + c])
    assert np.array_equal(got["axes_used"], np.broadcast_to(np.eye(3), (2, 3, 3)))
    assert bits_equal(got["axis_vectors"], own["axis_vectors"]) and bits_equal(own["axes_used"], own["axis_vectors"])
    assert np.all(np.abs(got["axis_vectors"][:, 0, 0]) > 0.9)
    # a movie keeps one frame's axes: a permutation with a sign moves the projections with it
    swap = flow_summary(vx, vy, vz, rel, PCT, rois=[ROI3], axes=[[0, -1, 0], [0, 0, 1], [1, 0, 0]], **SCALES)
    assert np.array_equal(swap["sum_axis1"], -got["sum_vy"]) and bits_equal(swap["sum_axis2"], got["sum_vz"])


def test_deterministic_and_independent_of_other_boxes(vol3):
    rel, vx, vy, vz = vol3
    rel = rel.astype(np.float32)
    bins = {"axis1": axis_bins_for(0.004, 14), "axis3": axis_bins_for(0.01, 31)}

    def words(rois):
        spec = SummarySpec(rois, None, PCT, min_size=50, axes="mask", axis_bins=bins, **SCALES)
        import torch
        dev = torch.device("cuda", 0)
        t = [torch.as_tensor(a).to(dev) for a in (vx, vy, vz, rel)]
        call = analysis._SummaryCall(spec, SHAPE3, t[3].dtype, dev)
        res = call.new_result(dev)
        call.enqueue((t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), False), res.data_ptr(),
                     torch.cuda.current_stream(dev).cuda_stream)
        per_box = call.axes.result_bytes // 8 // len(call.boxes)
        return res.cpu().numpy()[call.axes_off // 8:], per_box

    a, n = words([ROI3, (0, 9, 2, 20, 10, 40)])
    b, _ = words([ROI3, (0, 9, 2, 20, 10, 40)])
    alone, n1 = words(None)
    assert n == n1 == 44 + 14 + 31 and a.size == 3 * n
    assert np.array_equal(a, b)                 # every word, run to run
    assert np.array_equal(a[:n], alone)         # ROI 0 with and without the other boxes
    assert a[0] > 0 and a[40] > 0


# ---- degenerate masks --------------------------------------------------------------------------
def test_empty_mask(vol3):
    rel, vx, vy, vz = vol3
    bins = {"axis1": axis_bins_for(0.004, 14)}
    got = flow_summary(vx, vy, vz, rel, 100, rois=[ROI3], axes="mask", axis_bins=bins)  # rel > max: nothing
    assert not got["moments"].any() and not got["n_axes_mask"].any() and not got["n_axes_valid"].any()
    for k in ("centroid", "covariance", "axis_values", "axis_vectors", "axes_used", "mean_axis1"):
        assert np.all(np.isnan(got[k])), k
    for a in AXIS_NAMES:
        assert bits_equal(got["sum_" + a], np.zeros(2))
    assert not got["hist"]["axis1"].any()
    given = flow_summary(vx, vy, vz, rel, 100, axes=np.eye(3))
    assert np.array_equal(given["axes_used"][0], np.eye(3)) and np.all(np.isnan(given["axis_vectors"]))


def test_one_voxel_and_planar_masks():
    rel = np.zeros((5, 6, 70), np.float32)
    rel[3, 2, 66] = 1
    got = principal_axes(rel, threshold=0.5, rois=[(2, 5, 1, 6, 60, 70)])
    for r in range(2):
        assert got["n_axes_mask"][r] == 1 and got["centroid"][r].tolist() == [66.0, 2.0, 3.0]
        assert not got["covariance"][r].any() and got["axis_values"][r].tolist() == [0.0, 0.0, 0.0]
        assert np.array_equal(got["axis_vectors"][r], np.eye(3))
    assert got["moments"][1].tolist() == [1, 6, 1, 1, 36, 1, 1, 6, 6, 1]
    # a tilted ellipse in the plane z = 2: the third eigenvalue is exactly 0, the third axis z
    rel = np.zeros((5, 23, 70), np.float32)
    rel[2] = ar.blob((23, 70), 3) > 0.6
    got = principal_axes(rel, threshold=0.5)
    check_mask_part(got, mr.boxes_of(rel.shape, None), [rel > 0.5])
    assert got["axis_values"][0, 2] == 0.0 and got["axis_vectors"][0, 2].tolist() == [0.0, 0.0, 1.0]
    assert got["axis_values"][0, 1] > 1 and got["centroid"][0, 2] == 2.0
    # a plane x = 3 of a 3D volume: the zero eigenvalue belongs to x
    rel = np.zeros((5, 9, 8), np.float32)
    rel[:, 1:8, 3] = 1
    got = principal_axes(rel, threshold=0.5)
    assert got["axis_values"][0].tolist() == [4.0, 2.0, 0.0]
    assert got["axis_vectors"][0].tolist() == [[0, 1, 0], [0, 0, 1], [1, 0, 0]]


# ---- nothing else moved ------------------------------------------------------------------------
def test_default_spec_is_todays_summary(vol3):
    import torch

    rel, vx, vy, vz = vol3
    rel = rel.astype(np.float32)
    bins = {"vx": np.linspace(-0.004, 0.004, 13), "theta": np.linspace(-np.pi, np.pi, 9)}
    lib = analysis._lib.load()
    for extra in (dict(), dict(min_size=50)):
        plain = SummarySpec([ROI3], bins, PCT, **SCALES, **extra)
        call = analysis._SummaryCall(plain, SHAPE3, torch.float32, torch.device("cuda", 0))
        assert call.axes is None
        assert call.result_bytes == lib.of3d_flow_summary_result_bytes(2, call.nb_arr) + (64 if extra else 0)
        base = flow_summary(vx, vy, vz, rel, PCT, rois=[ROI3], bins=bins, **SCALES, **extra)
        same = flow_summary(vx, vy, vz, rel, PCT, rois=[ROI3], bins=bins, axes=None, axes_physical=False,
                            axis_bins=None, **SCALES, **extra)
        with_axes = flow_summary(vx, vy, vz, rel, PCT, rois=[ROI3], bins=bins, axes="mask",
                                 axis_bins={"axis1": axis_bins_for(0.004, 14)}, **SCALES, **extra)
        assert set(base) == set(same) and "axes_used" not in base and "axes_used" in with_axes
        for k in base:
            for other in (same, with_axes):
                if k in ("hist", "edges"):
                    assert all(bits_equal(other[k][q], base[k][q]) for q in base[k]), k
                else:
                    assert bits_equal(np.asarray(other[k]), np.asarray(base[k])), k


D_ROIS = [(1, 5, 3, 14, 2, 17)]
D_BINS = {"magnitude": np.linspace(0.0, 0.5, 11)}
D_AXIS_BINS = {"axis1": np.linspace(-0.3, 0.3, 15)}


def test_process_flow_and_flowstream_carry_the_axes(tmp_path):
    from opticalflow3d_dev_amd.stream import FlowStream

    series = np.random.default_rng(61).integers(0, 4096, size=(9, 6, 16, 20)).astype(np.uint16)
    kw = dict(rois=D_ROIS, bins=D_BINS, rel_percentile=70, min_size=20, connectivity=18, **SCALES)
    specs = {"plain": SummarySpec(**kw), "axes": SummarySpec(axes="mask", axis_bins=D_AXIS_BINS, **kw)}
    want = [flow_summary(*calc_flow3D(series[i:i + 7], 1, 1, 2), 70, rois=D_ROIS, bins=D_BINS, min_size=20,
                         connectivity=18, axes="mask", axis_bins=D_AXIS_BINS, **SCALES) for i in range(3)]
    runs = {}
    for name, spec in specs.items():
        d = tmp_path / name
        d.mkdir()
        tf.imwrite(d / "cells.tif", series, imagej=True)
        process_flow(str(d), "cells", "OneTif", 3, 1, 1, 2, summary=spec)
        runs[name] = d / "OpticalFlow3D" / "cells"
    tiffs = sorted(p.name for p in runs["plain"].glob("*.tif*"))
    assert tiffs and tiffs == sorted(p.name for p in runs["axes"].glob("*.tif*"))
    for t in tiffs:
        assert (runs["plain"] / t).read_bytes() == (runs["axes"] / t).read_bytes(), t
    plain, axes = (read_summary_csv(runs[k] / "cells_summary.csv") for k in ("plain", "axes"))
    header = (runs["axes"] / "cells_summary.csv").read_text().splitlines()[0].split(",")
    assert header == list(CSV_COLUMNS + analysis.CSV_OPEN_COLUMNS + CSV_AXES_COLUMNS)
    assert list(plain) == list(CSV_COLUMNS + analysis.CSV_OPEN_COLUMNS)
    for k in plain:
        assert bits_equal(plain[k], axes[k]), k
    npz = np.load(runs["axes"] / "cells_summary_hist.npz")
    for i, w in enumerate(want):
        rows = slice(2 * i, 2 * i + 2)
        assert np.array_equal(axes["n_axes_mask"][rows], w["n_axes_mask"]) and np.all(w["n_axes_mask"] > 0)
        assert np.array_equal(axes["mom_xx"][rows], w["moments"][:, 4].astype(np.int64))
        for j, c in enumerate("xyz"):
            assert np.array_equal(axes["centroid_" + c][rows], w["centroid"][:, j])
            assert np.array_equal(axes["axis1_" + c][rows], w["axis_vectors"][:, 0, j])
            assert np.array_equal(axes["used3_" + c][rows], w["axes_used"][:, 2, j])
        assert np.array_equal(axes["cov_xy"][rows], w["covariance"][:, 0, 1])
        for a in AXIS_NAMES:
            assert np.array_equal(axes["sum_" + a][rows], w["sum_" + a])
        assert np.array_equal(npz["counts_axis1"][i], w["hist"]["axis1"]) and npz["counts_axis1"][i].sum() > 0
    # the stream itself, without field downloads
    fs = FlowStream(3, series.shape[1:], series.dtype, 1, 1, 2, summary=specs["axes"], fields=False)
    try:
        for f in series[:7 + fs.lookahead]:
            fs.push(f)
        p = fs.submit()
        s = p.summary()
        p.release()
    finally:
        fs.close()
    assert set(s) == set(want[0])
    for k in s:
        if k in ("hist", "edges"):
            assert all(bits_equal(s[k][q], want[0][k][q]) for q in s[k]), k
        else:
            assert bits_equal(np.asarray(s[k]), np.asarray(want[0][k])), k
