"""Summaries over the opened reliability mask (min_size >= 1): flow_summary against
mask_ref.summary_ref_masked on open_ref's mask, min_size = 1 against today's summary bit for
bit, and the FlowStream / process_flow drivers with the four extra counts."""
import numpy as np
import pytest
from scipy import ndimage

import mask_ref as mr
import summary_ref as sr
from conftest import bits_equal
from opticalflow3d_dev_amd import SummarySpec, calc_flow3D, flow_summary, process_flow
from opticalflow3d_dev_amd import tiff as tf
from opticalflow3d_dev_amd.analysis import CSV_COLUMNS, CSV_OPEN_COLUMNS, SUMS, read_summary_csv

pytestmark = pytest.mark.gpu

SCALES = dict(xyscale=0.1, zscale=0.3, tscale=2.0)
ROIS3 = [(0, 23, 3, 35, 5, 65), (1, 24, 11, 40, 33, 72)]
BINS = {"vx": np.linspace(-0.02, 0.02, 13), "magnitude": np.linspace(0.0, 0.05, 11),
        "theta": -np.pi + (np.arange(13) + (np.sqrt(2.0) - 1.0)) * (2 * np.pi / 12),
        "phi": -np.pi / 2 + (np.arange(9) + (np.sqrt(3.0) - 1.0)) * (np.pi / 8)}


def smooth(seed, shape, dtype=np.float64):
    return ndimage.gaussian_filter(np.random.default_rng(seed).standard_normal(shape), 1.5).astype(dtype)


@pytest.fixture(scope="module")
def fields():
    shape = (24, 40, 72)
    return smooth(40, shape), smooth(41, shape), smooth(42, shape), smooth(43, shape, np.float32)


def check_against_ref(vx, vy, vz, rel, rois, bins, min_size, connectivity, percentile=80):
    got = flow_summary(vx, vy, vz, rel, percentile, rois=rois, bins=bins, min_size=min_size,
                       connectivity=connectivity, **SCALES)
    boxes = mr.boxes_of(np.shape(vx), rois)
    thresh = np.percentile(rel, percentile)
    keep, counts = mr.open_ref(rel, thresh, boxes, min_size, connectivity)
    ref = mr.summary_ref_masked(vx, vy, vz, keep, thresh, boxes, bins=bins, **SCALES)
    sr.assert_clear_of_edges(ref, [k for k in bins if k in ("theta", "phi")])
    sr.assert_matches(got, ref, list(bins))
    for k in mr.COUNTS:
        assert got[k].dtype == np.int64 and np.array_equal(got[k], counts[k]), k
    return got, counts


@pytest.mark.parametrize("v_dtype", [np.float64, np.float32])
def test_3d_against_reference(fields, v_dtype):
    vx, vy, vz, rel = fields
    got, counts = check_against_ref(vx.astype(v_dtype), vy.astype(v_dtype), vz.astype(v_dtype), rel, ROIS3, BINS, 10,
                                    26)
    assert np.all(counts["n_components_kept"] >= 3) and np.all(counts["n_components"] > counts["n_components_kept"])
    assert np.all(got["n_valid"] > 0) and np.all(got["n_valid"] <= got["n_kept"])


@pytest.mark.parametrize("v_dtype", [np.float64, np.float32])
def test_2d_against_reference(v_dtype):
    shape = (40, 72)
    vx, vy, rel = smooth(50, shape).astype(v_dtype), smooth(51, shape).astype(v_dtype), smooth(52, shape)
    bins = {k: BINS[k] for k in ("vx", "magnitude", "theta")}
    got, counts = check_against_ref(vx, vy, None, rel, [(3, 35, 5, 65), (11, 40, 33, 72)], bins, 6, 8)
    assert 0 < counts["n_components_kept"][0] < counts["n_components"][0]
    check_against_ref(vx, vy, None, rel, None, bins, 6, 4)


def test_min_size_1_is_todays_summary_bit_for_bit(fields):
    vx, vy, vz, rel = fields
    kw = dict(rois=ROIS3, bins=BINS, **SCALES)
    plain = flow_summary(vx, vy, vz, rel, 80, **kw)
    for extra in (dict(min_size=0), dict(min_size=1), dict(min_size=1, connectivity=6)):
        got = flow_summary(vx, vy, vz, rel, 80, **kw, **extra)
        assert set(got) - set(plain) == (set(mr.COUNTS) if extra["min_size"] else set())
        for k in plain:
            if k in ("hist", "edges"):
                assert all(bits_equal(got[k][q], plain[k][q]) for q in plain[k]), k
            else:
                assert bits_equal(np.asarray(got[k]), np.asarray(plain[k])), k
        if extra["min_size"]:
            assert np.array_equal(got["n_kept"], got["n_mask"])
            assert np.array_equal(got["n_components_kept"], got["n_components"])


def test_min_size_above_the_volume(fields):
    vx, vy, vz, rel = fields
    got = flow_summary(vx, vy, vz, rel, 80, rois=ROIS3, bins=BINS, min_size=vx.size + 1)
    assert np.all(got["n_valid"] == 0) and np.all(got["n_kept"] == 0) and np.all(got["n_mask"] > 0)
    assert np.all(np.isnan(got["mean_magnitude"])) and np.all(np.isnan(got["theta_mean"]))
    assert all(not h.any() for h in got["hist"].values())


# ---- drivers: a tiny 3D series, 9 frames, tSig = 1 (three windows of 7) ----
D_ROIS = [(1, 5, 3, 14, 2, 17)]
D_BINS = {"magnitude": np.linspace(0.0, 0.5, 11)}
D_SPEC = SummarySpec(rois=D_ROIS, bins=D_BINS, rel_percentile=70, min_size=20, connectivity=18, **SCALES)


@pytest.fixture(scope="module")
def series():
    return np.random.default_rng(61).integers(0, 4096, size=(9, 6, 16, 20)).astype(np.uint16)


@pytest.fixture(scope="module")
def per_frame(series):
    """flow_summary of each window's calc_flow3D outputs: what the drivers must reproduce."""
    return [flow_summary(*calc_flow3D(series[i:i + 7], 1, 1, 2), 70, rois=D_ROIS, bins=D_BINS, min_size=20,
                         connectivity=18, **SCALES) for i in range(3)]


def same_summary(a, b):
    assert set(a) == set(b)
    for k in a:
        if k in ("hist", "edges"):
            assert set(a[k]) == set(b[k]) and all(bits_equal(a[k][q], b[k][q]) for q in a[k]), k
        else:
            assert bits_equal(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.mark.parametrize("with_fields", [True, False])
def test_flowstream_summary(series, per_frame, with_fields):
    from opticalflow3d_dev_amd.stream import FlowStream

    fs = FlowStream(3, series.shape[1:], series.dtype, 1, 1, 2, summary=D_SPEC, fields=with_fields)
    try:
        pushed = 0
        for i in range(3):
            while pushed < min(i + 7 + fs.lookahead, len(series)):
                fs.push(series[pushed])
                pushed += 1
            p = fs.submit()
            s = p.summary()
            p.release()
            same_summary(s, per_frame[i])
        assert per_frame[0]["n_components"][0] > per_frame[0]["n_components_kept"][0] > 0
    finally:
        fs.close()


def test_process_flow_writes_the_counts(series, per_frame, tmp_path):
    runs = {}
    for name, spec in (("opened", D_SPEC), ("zero", SummarySpec(rois=D_ROIS, bins=D_BINS, rel_percentile=70,
                                                               min_size=0, connectivity=18, **SCALES)),
                       ("unset", SummarySpec(rois=D_ROIS, bins=D_BINS, rel_percentile=70, **SCALES))):
        d = tmp_path / name
        d.mkdir()
        tf.imwrite(d / "cells.tif", series, imagej=True)
        process_flow(str(d), "cells", "OneTif", 3, 1, 1, 2, summary=spec, save_fields=False)
        runs[name] = d / "OpticalFlow3D" / "cells"
    text = {k: (v / "cells_summary.csv").read_text() for k, v in runs.items()}
    assert text["zero"] == text["unset"]  # min_size = 0: the file of a spec without the new fields
    assert text["unset"].splitlines()[0].split(",") == list(CSV_COLUMNS)
    assert text["opened"].splitlines()[0].split(",") == list(CSV_COLUMNS + CSV_OPEN_COLUMNS)
    a, b = np.load(runs["zero"] / "cells_summary_hist.npz"), np.load(runs["unset"] / "cells_summary_hist.npz")
    assert sorted(a.files) == sorted(b.files) and all(bits_equal(a[k], b[k]) for k in a.files)
    csv, npz = read_summary_csv(runs["opened"] / "cells_summary.csv"), np.load(runs["opened"] / "cells_summary_hist.npz")
    assert csv["frame"].tolist() == [3, 3, 4, 4, 5, 5]
    for i, want in enumerate(per_frame):
        rows = slice(2 * i, 2 * i + 2)
        for k in CSV_OPEN_COLUMNS + ("n_valid", "n_voxels"):
            assert csv[k].dtype == np.int64 and np.array_equal(csv[k][rows], want[k]), k
        for k in SUMS + ("mean_magnitude", "theta_mean"):
            assert np.array_equal(csv[k][rows], want[k], equal_nan=True), k
        assert np.array_equal(npz["counts_magnitude"][i], want["hist"]["magnitude"])
