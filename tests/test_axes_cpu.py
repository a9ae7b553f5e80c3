"""Host side of the mask axes (no GPU): SummarySpec's validation of the new fields, the
overflow guard of of3d_mask_axes_workspace_bytes (host arithmetic), the CSV / npz round trip
with and without the axes columns, and the tests' own reference (axes_ref) on hand-made masks
with known answers."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import axes_ref as ar
from opticalflow3d_dev_amd import SummarySpec, _lib, analysis


# ---- SummarySpec ------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,shape,message", [
    (dict(axes="body"), (4, 5, 6), "summary: axes 'body' is not 'mask' or a 3x3 array"),
    (dict(axes=object()), (4, 5, 6), "is not 'mask' or a 3x3 array"),
    (dict(axes=np.eye(2)), (4, 5, 6), r"summary: axes must be a 3x3 array, got shape \(2, 2\)"),
    (dict(axes=np.arange(9.0)), (4, 5, 6), r"summary: axes must be a 3x3 array, got shape \(9,\)"),
    (dict(axes=np.diag([1.0, np.inf, 1.0])), (4, 5, 6), "summary: axes must be finite"),
    (dict(axes=np.diag([1.0, np.nan, 1.0])), (4, 5, 6), "summary: axes must be finite"),
    (dict(axis_bins={"axis1": [0.0, 1.0]}), (4, 5, 6), "summary: axis_bins needs axes"),
    (dict(axes="mask", axis_bins={"axis3": [0.0, 1.0]}), (5, 6), "summary: an axis3 histogram needs a 3D volume"),
    (dict(axes="mask", axis_bins={"axis4": [0.0, 1.0]}), (4, 5, 6), "summary: unknown axis histogram 'axis4'"),
    (dict(axes="mask", axis_bins={"axis1": [0.0, 1.0, 1.0]}), (4, 5, 6), "summary: axis1 bin edges must be strictly"),
    (dict(axes="mask", axis_bins={"axis2": [0.0, np.nan, 1.0]}), (4, 5, 6), "summary: axis2 bin edges must be strictly"),
    (dict(axes="mask", axis_bins={"axis1": [0.0]}), (4, 5, 6), "summary: axis1 edges must be a 1-D array of 2 to 257"),
    (dict(axes="mask", axis_bins={"axis1": np.arange(258.0)}), (4, 5, 6), "of 2 to 257 values"),
])
def test_spec_rejects(kw, shape, message):
    with pytest.raises(ValueError, match=message):
        SummarySpec(**kw).axes_request(len(shape))


def test_spec_accepts_and_resolve_is_unchanged():
    plain = SummarySpec(rois=[(1, 3, 0, 4, 2, 5)], bins={"theta": [-1.0, 0.0, 2.0]})
    assert plain.axes is None and plain.axes_physical is False and plain.axis_bins is None
    assert plain.axes_request(3) is None
    both = SummarySpec(rois=[(1, 3, 0, 4, 2, 5)], bins={"theta": [-1.0, 0.0, 2.0]}, axes="mask", axes_physical=True,
                       axis_bins={"axis2": [-1.0, 0.0, 1.0, 3.0]})
    a, b = plain.resolve((4, 5, 6)), both.resolve((4, 5, 6))
    assert len(a) == len(b) == 3 and np.array_equal(a[0], b[0]) and a[1] == b[1]
    assert all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a[2], b[2]))
    given, nbins, edges = both.axes_request(3)
    assert given is None and nbins == [0, 3, 0] and edges[1].tolist() == [-1.0, 0.0, 1.0, 3.0] and edges[0] is None
    given, nbins, _ = SummarySpec(axes=[[0, 1, 0], [1, 0, 0], [0, 0, 1]]).axes_request(2)
    assert given.dtype == np.float64 and given.tolist() == [0, 1, 0, 1, 0, 0, 0, 0, 1] and nbins == [0, 0, 0]
    # the existing fields are still the first positional ones
    s = SummarySpec(None, None, 80, 0.1, 0.3, 2.0, 5, 6)
    assert (s.rel_percentile, s.tscale, s.min_size, s.connectivity, s.axes) == (80, 2.0, 5, 6, None)


# ---- the overflow guard: voxels * (L - 1)^2 < 2^63 ---------------------------------------------
def ws_bytes(*boxes):
    arr = np.array(boxes, dtype=np.int64)
    return _lib.load().of3d_mask_axes_workspace_bytes(arr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(arr))


def test_workspace_bytes_guards_the_moments_range():
    assert ws_bytes((0, 9, 0, 23, 0, 70)) > 0
    assert ws_bytes((0, 2048, 0, 1024, 0, 1024)) > 0          # BASELINE c5: 2^31 voxels, L = 2048
    # a (1, 1, L) rod: L * (L - 1)^2 against 2^63
    L = 2097152                                               # 2^21: 2^21 * (2^21 - 1)^2 < 2^63
    assert L * (L - 1) ** 2 < 2 ** 63 <= (L + 1) * L ** 2
    assert ws_bytes((0, 1, 0, 1, 0, L)) > 0
    assert ws_bytes((0, 1, 0, 1, 0, L + 1)) == 0
    assert "too large" in _lib.last_error()
    # a cube of edge a: a^3 * (a - 1)^2 against 2^63
    a = next(a for a in range(2, 10 ** 5) if (a + 1) ** 3 * a ** 2 >= 2 ** 63)
    assert a ** 3 * (a - 1) ** 2 < 2 ** 63
    assert ws_bytes((0, a, 0, a, 0, a)) > 0
    assert ws_bytes((0, a + 1, 0, a + 1, 0, a + 1)) == 0
    assert ws_bytes((5, a + 6, 0, a + 1, 7, a + 8)) == 0      # the extent counts, not the origin
    assert ws_bytes((0, 2 ** 31 - 1, 0, 2 ** 31 - 1, 0, 2 ** 31 - 1)) == 0  # 2^93 voxels: no wrap-around
    assert ws_bytes((0, 0, 0, 4, 0, 4)) == 0 and ws_bytes((0, 4, 0, 4, 4, 2)) == 0   # invalid boxes
    assert ws_bytes((0, 4, 0, 4, 0, 4), (0, 1, 0, 1, 0, L + 1)) == 0                 # any bad box


def test_result_bytes():
    lib = _lib.load()
    nb = lambda *v: (ctypes.c_int * 3)(*v)
    assert lib.of3d_mask_axes_result_bytes(1, nb(0, 0, 0)) == 44 * 8
    assert lib.of3d_mask_axes_result_bytes(3, nb(14, 0, 256)) == 3 * (44 + 270) * 8
    assert lib.of3d_mask_axes_result_bytes(0, nb(0, 0, 0)) == 0
    assert lib.of3d_mask_axes_result_bytes(17, nb(0, 0, 0)) == 0
    assert lib.of3d_mask_axes_result_bytes(1, nb(257, 0, 0)) == 0


# ---- writer round trip -------------------------------------------------------------------------
def _fake_summary(seed, n_roi=2, axes=False):
    rng = np.random.default_rng(seed)
    s = {"threshold": np.float32(rng.random()), "rois": rng.integers(0, 9, size=(n_roi, 6)),
         "n_valid": rng.integers(0, 99, n_roi), "n_voxels": rng.integers(99, 999, n_roi)}
    for k in analysis.CSV_COLUMNS[11:]:
        s[k] = rng.standard_normal(n_roi)
    s["hist"] = {"magnitude": rng.integers(0, 50, (n_roi, 4)).astype(np.uint64)}
    s["edges"] = {"magnitude": np.linspace(0.0, 1.0, 5)}
    if axes:
        s["moments"] = rng.integers(0, 2 ** 62, (n_roi, 10)).astype(np.uint64)
        s["n_axes_mask"] = s["moments"][:, 0].astype(np.int64)
        s["n_axes_valid"] = rng.integers(0, 99, n_roi)
        s["centroid"], s["axis_values"] = rng.standard_normal((n_roi, 3)), rng.standard_normal((n_roi, 3))
        c = rng.standard_normal((n_roi, 3, 3))
        s["covariance"] = c + c.transpose(0, 2, 1)
        s["axis_vectors"], s["axes_used"] = rng.standard_normal((n_roi, 3, 3)), rng.standard_normal((n_roi, 3, 3))
        s["axis_vectors"][1] = np.nan  # an empty mask's row
        for a in analysis.AXIS_NAMES:
            s["sum_" + a], s["mean_" + a] = rng.standard_normal(n_roi), rng.standard_normal(n_roi)
        s["hist"]["axis1"] = rng.integers(0, 50, (n_roi, 14)).astype(np.uint64)
        s["edges"]["axis1"] = np.linspace(-2.0, 2.0, 15)
    return s


def test_csv_and_npz_round_trip_with_and_without_axes(tmp_path):
    for axes in (False, True):
        frames, summaries = [3, 4], [_fake_summary(10, axes=axes), _fake_summary(11, axes=axes)]
        prefix = str(tmp_path / f"run{int(axes)}")
        analysis.write_summaries(prefix, frames, summaries)
        header = open(prefix + "_summary.csv").readline().strip().split(",")
        assert header == list(analysis.CSV_COLUMNS + (analysis.CSV_AXES_COLUMNS if axes else ()))
        csv, npz = analysis.read_summary_csv(prefix + "_summary.csv"), np.load(prefix + "_summary_hist.npz")
        assert csv["frame"].tolist() == [3, 3, 4, 4] and csv["roi"].tolist() == [0, 1, 0, 1]
        assert sorted(npz.files) == sorted(["frames", "edges_magnitude", "counts_magnitude"]
                                           + (["edges_axis1", "counts_axis1"] if axes else []))
        if not axes:
            continue
        for i, s in enumerate(summaries):
            rows = slice(2 * i, 2 * i + 2)
            assert csv["n_axes_mask"].dtype == np.int64 and np.array_equal(csv["n_axes_mask"][rows], s["n_axes_mask"])
            assert np.array_equal(csv["n_axes_valid"][rows], s["n_axes_valid"])
            for j, m in enumerate(ar.MOMENTS[1:], 1):
                assert np.array_equal(csv["mom_" + m][rows], s["moments"][:, j].astype(np.int64)), m
            for j, c in enumerate("xyz"):
                assert np.array_equal(csv["centroid_" + c][rows], s["centroid"][:, j])
                assert np.array_equal(csv[f"axis_value{j + 1}"][rows], s["axis_values"][:, j])
                for k in range(3):
                    assert np.array_equal(csv[f"axis{k + 1}_{c}"][rows], s["axis_vectors"][:, k, j], equal_nan=True)
                    assert np.array_equal(csv[f"used{k + 1}_{c}"][rows], s["axes_used"][:, k, j])
            for name, (a, b) in {"cov_xx": (0, 0), "cov_yy": (1, 1), "cov_zz": (2, 2), "cov_xy": (0, 1),
                                 "cov_xz": (0, 2), "cov_yz": (1, 2)}.items():
                assert np.array_equal(csv[name][rows], s["covariance"][:, a, b]), name
            for a in analysis.AXIS_NAMES:
                assert np.array_equal(csv["sum_" + a][rows], s["sum_" + a])
                assert np.array_equal(csv["mean_" + a][rows], s["mean_" + a])
            assert np.array_equal(npz["counts_axis1"][i], s["hist"]["axis1"])
        assert np.array_equal(npz["edges_axis1"], np.linspace(-2.0, 2.0, 15))


# ---- the reference on masks with known answers ------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 7, 30])
def test_rod_along_x(k):
    m = np.zeros((3, 4, 40), bool)
    m[1, 2, 5:5 + k] = True
    box = (0, 3, 0, 4, 0, 40)
    mom = ar.int_moments(m)
    assert mom[0] == k and mom[1] == sum(range(5, 5 + k)) and mom[4] == sum(x * x for x in range(5, 5 + k))
    cen, cov = ar.exact_stats(mom, box)
    assert cen == [Fraction(2 * 5 + k - 1, 2), Fraction(2), Fraction(1)]
    assert cov[0][0] == Fraction(k * k - 1, 12) and all(cov[i][j] == 0 for i in range(3) for j in range(3) if (i, j) != (0, 0))
    w, v = ar.eigh_axes([[float(c) for c in row] for row in cov])
    assert w.tolist() == [(k * k - 1) / 12, 0.0, 0.0]
    if k > 1:
        assert v[0].tolist() == [1.0, 0.0, 0.0]


def test_brick_has_the_textbook_variances():
    m = np.zeros((9, 12, 20), bool)
    m[2:7, 1:9, 3:19] = True  # 5 x 8 x 16
    box = (1, 9, 0, 12, 2, 20)  # a box with an origin: local coordinates, volume centroid
    mom = ar.int_moments(ar.box_mask(m, box))
    cen, cov = ar.exact_stats(mom, box)
    assert mom[0] == 5 * 8 * 16
    assert cen == [Fraction(3 + 18, 2), Fraction(1 + 8, 2), Fraction(2 + 6, 2)]
    assert [cov[i][i] for i in range(3)] == [Fraction(16 * 16 - 1, 12), Fraction(8 * 8 - 1, 12), Fraction(5 * 5 - 1, 12)]
    assert all(cov[i][j] == 0 for i in range(3) for j in range(3) if i != j)
    w, v = ar.eigh_axes([[float(c) for c in row] for row in cov])
    assert np.allclose(w, [255 / 12, 63 / 12, 24 / 12], rtol=1e-15) and np.array_equal(np.abs(v), np.eye(3))


def test_sign_rule():
    assert ar.sign_rule([-0.9, 0.3, 0.1]).tolist() == [0.9, -0.3, -0.1]
    assert ar.sign_rule([0.2, -0.9, 0.1]).tolist() == [-0.2, 0.9, -0.1]
    assert ar.sign_rule([0.2, 0.3, 0.9]).tolist() == [0.2, 0.3, 0.9]
    # a tie goes to the first of x, y, z
    assert ar.sign_rule([-0.5, 0.5, 0.1]).tolist() == [0.5, -0.5, -0.1]
    assert ar.sign_rule([0.1, 0.5, -0.5]).tolist() == [0.1, 0.5, -0.5]
    d = np.diag([1.0, 3.0, 2.0])
    w, v = ar.eigh_axes(d)
    assert w.tolist() == [3.0, 2.0, 1.0] and v.tolist() == [[0, 1, 0], [0, 0, 1], [1, 0, 0]]


def test_ulp_distance():
    assert ar.ulp_distance(0.5, Fraction(1, 2)) == 0
    assert ar.ulp_distance(np.nextafter(3.0, 4.0), Fraction(3)) == 1
