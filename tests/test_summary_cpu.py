"""Host side of the device frame summaries (no GPU): SummarySpec validation, the factored
percentile rank/weight helper against np.percentile, the CSV / npz writer round trip, and the
tests' own numpy restatement (summary_ref) against the notebook arithmetic."""
import numpy as np
import pytest

import summary_ref as sr
from opticalflow3d_dev_amd import SummarySpec, analysis


# ---- SummarySpec validation -------------------------------------------------------------------
def test_spec_resolves_whole_volume_first():
    boxes, nbins, edges = SummarySpec(rois=[(1, 3, 0, 4, 2, 5)], bins={"theta": [-1.0, 0.0, 2.0]}).resolve((4, 5, 6))
    assert boxes.dtype == np.int64 and boxes.tolist() == [[0, 4, 0, 5, 0, 6], [1, 3, 0, 4, 2, 5]]
    assert nbins == [0, 0, 0, 0, 2, 0] and edges[4].tolist() == [-1.0, 0.0, 2.0] and edges[0] is None
    boxes, _, _ = SummarySpec(rois=[(1, 3, 2, 5)]).resolve((5, 6))
    assert boxes.tolist() == [[0, 1, 0, 5, 0, 6], [0, 1, 1, 3, 2, 5]]


@pytest.mark.parametrize("kw,shape,word", [
    (dict(rois=[(0, 5, 0, 5, 0, 6)]), (4, 5, 6), "outside"),          # z1 past the volume
    (dict(rois=[(2, 2, 0, 5, 0, 6)]), (4, 5, 6), "empty"),            # empty box
    (dict(rois=[(-1, 2, 0, 5, 0, 6)]), (4, 5, 6), "outside"),         # negative origin
    (dict(rois=[(0, 5, 0, 6)]), (4, 5, 6), "6 bounds"),               # a 2D box for a 3D volume
    (dict(rois=[(0, 1, 0, 5, 0, 6)]), (5, 6), "4 bounds"),            # a 3D box for a 2D frame
    (dict(rois=[(0, 1.5, 0, 5, 0, 6)]), (4, 5, 6), "non-integer"),
    (dict(rois=[(0, 1, 0, 1, 0, 1)] * 16), (4, 5, 6), "at most 15"),
    (dict(bins={"theta": [0.0, 1.0, 1.0]}), (4, 5, 6), "ascending"),
    (dict(bins={"theta": [0.0, 2.0, 1.0]}), (4, 5, 6), "ascending"),
    (dict(bins={"theta": [0.0, np.nan, 1.0]}), (4, 5, 6), "ascending"),
    (dict(bins={"theta": [0.0]}), (4, 5, 6), "2 to 257"),
    (dict(bins={"theta": np.arange(258.0)}), (4, 5, 6), "2 to 257"),
    (dict(bins={"speed": [0.0, 1.0]}), (4, 5, 6), "unknown"),
    (dict(bins={"phi": [0.0, 1.0]}), (5, 6), "3D"),
    (dict(rel_percentile=101), (4, 5, 6), "rel_percentile"),
])
def test_spec_rejects(kw, shape, word):
    with pytest.raises(ValueError, match=word):
        SummarySpec(**kw).resolve(shape)


# ---- the rank / weight helper shared by percentile_threshold and percentile_threshold_device ---
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [1, 2, 7, 100003])
def test_linear_ranks_reproduce_numpy(dtype, n):
    a = np.random.default_rng(n).standard_normal(n).astype(dtype)
    dt = np.dtype(dtype)
    for pct in (0, 50, 90, 99.5, 100):
        lo, hi, gamma = analysis._linear_ranks(n, pct, dt)
        assert 0 <= lo <= hi <= n - 1 and hi - lo <= 1 and gamma.dtype == dt
        part = np.partition(a, sorted({lo, hi}))
        got = analysis._lerp(part[lo], part[hi], gamma, dt)
        want = np.percentile(a, pct)
        assert got == want and got.dtype == want.dtype, (n, pct)


# ---- writer round trip -------------------------------------------------------------------------
def _fake_summary(seed, n_roi=3):
    rng = np.random.default_rng(seed)
    s = {"threshold": np.float32(rng.random()), "rois": rng.integers(0, 9, size=(n_roi, 6)),
         "n_valid": rng.integers(0, 100, size=n_roi), "n_voxels": rng.integers(100, 200, size=n_roi)}
    for k in analysis.CSV_COLUMNS[11:]:
        s[k] = rng.standard_normal(n_roi)
    s["n_valid"][1] = 0
    s["mean_magnitude"][1] = s["theta_mean"][1] = np.nan
    s["edges"] = {"vx": np.linspace(-1, 1, 5), "theta": np.linspace(-3, 3, 8)}
    s["hist"] = {k: rng.integers(0, 2 ** 40, size=(n_roi, e.size - 1)).astype(np.uint64) for k, e in s["edges"].items()}
    return s


def test_writer_round_trip(tmp_path):
    frames, sums = [3, 4, 5, 6], [_fake_summary(i) for i in range(4)]
    prefix = str(tmp_path / "cells")
    analysis.write_summaries(prefix, frames, sums)
    header = open(prefix + "_summary.csv").readline().strip().split(",")
    assert tuple(header) == analysis.CSV_COLUMNS and header[:3] == ["frame", "roi", "z0"]
    csv = analysis.read_summary_csv(prefix + "_summary.csv")
    assert csv["frame"].tolist() == [f for f in frames for _ in range(3)]
    assert csv["roi"].tolist() == [0, 1, 2] * 4
    for i, s in enumerate(sums):
        rows = slice(3 * i, 3 * i + 3)
        assert np.array_equal(np.stack([csv[k][rows] for k in ("z0", "z1", "y0", "y1", "x0", "x1")], 1), s["rois"])
        assert np.array_equal(csv["n_valid"][rows], s["n_valid"]) and np.array_equal(csv["n_voxels"][rows], s["n_voxels"])
        assert np.all(csv["threshold"][rows] == np.float64(s["threshold"]))
        for k in analysis.CSV_COLUMNS[11:]:
            assert np.array_equal(csv[k][rows], s[k], equal_nan=True), k  # repr round-trips float64 exactly
    npz = np.load(prefix + "_summary_hist.npz")
    assert npz["frames"].tolist() == frames
    for k in ("vx", "theta"):
        assert np.array_equal(npz["edges_" + k], sums[0]["edges"][k])
        assert npz["counts_" + k].dtype == np.uint64 and npz["counts_" + k].shape == (4, 3, sums[0]["edges"][k].size - 1)
        assert np.array_equal(npz["counts_" + k], np.stack([s["hist"][k] for s in sums]))


# ---- summary_ref against the notebook arithmetic ------------------------------------------------
def test_summary_ref_matches_notebook_arithmetic():
    rng = np.random.default_rng(11)
    shape = (3, 5, 7)
    vx, vy, vz = (rng.standard_normal(shape) for _ in range(3))
    rel = rng.random(shape).astype(np.float32)
    vx[1, 2, 3] = 0.0
    rel[1, 2, 3] = 2.0  # passes the mask, but vx == 0 -> NaN -> not valid
    roi = (1, 3, 0, 4, 2, 7)
    edges = np.linspace(-np.pi, np.pi, 9)
    ref = sr.summary_ref(vx, vy, vz, rel, 60, 0.5, 2.0, 4.0, rois=[roi], bins={"theta": edges, "magnitude": [0.0, 0.2, 5.0]})
    # the notebook's cells 4-6 and the figures' reductions, written out directly
    thresh = np.percentile(rel, 60)
    m = rel > thresh
    with np.errstate(invalid="ignore"):
        x, y, z = vx * m, vy * m, vz * m
        for v in (x, y, z):
            v[v == 0] = np.nan
        x, y, z = x * 0.5 / 4.0, y * 0.5 / 4.0, z * 2.0 / 4.0
        mag = np.sqrt(x ** 2 + y ** 2 + z ** 2)
        theta = np.arctan2(y, x)
    assert ref["threshold"] == thresh
    for r, sl in enumerate([np.s_[:, :, :], np.s_[1:3, 0:4, 2:7]]):
        good = ~np.isnan(mag[sl])
        assert ref["n_valid"][r] == good.sum() and ref["n_voxels"][r] == good.size
        assert good.sum() == m[sl].sum() - 1  # the planted zero passes the mask but is not valid
        np.testing.assert_allclose(ref["mean_magnitude"][r], np.nanmean(mag[sl]), rtol=1e-13)
        t = theta[sl][good]
        np.testing.assert_allclose(ref["theta_mean"][r], np.arctan2(np.mean(np.sin(t)), np.mean(np.cos(t))), rtol=1e-12)
        w = mag[sl][good]
        np.testing.assert_allclose(ref["theta_mean_weighted"][r],
                                   np.arctan2(np.sum(w * np.sin(t)), np.sum(w * np.cos(t))), rtol=1e-12)
        assert np.array_equal(ref["hist"]["theta"][r], np.histogram(t, bins=edges)[0])
        assert ref["hist"]["magnitude"][r].sum() == np.sum((w >= 0) & (w <= 5.0))
    assert np.all(sr.sum_bound(ref, "sum_magnitude") > 0)


def test_summary_ref_2d_and_empty_box():
    rng = np.random.default_rng(12)
    vx, vy = rng.standard_normal((6, 8)), rng.standard_normal((6, 8))
    rel = rng.random((6, 8))
    rel[0, 0] = np.nan  # NaN threshold: nothing passes
    ref = sr.summary_ref(vx, vy, None, rel, 90, rois=[(1, 3, 2, 5)])
    assert ref["rois"].tolist() == [[0, 1, 0, 6, 0, 8], [0, 1, 1, 3, 2, 5]]
    assert np.isnan(ref["threshold"]) and ref["n_valid"].tolist() == [0, 0] and ref["n_voxels"].tolist() == [48, 6]
    assert np.all(np.isnan(ref["mean_magnitude"])) and np.all(ref["sum_vz"] == 0)
