"""Mask opening without a GPU: the spec's validation of min_size / connectivity, the CPU
reference on hand-made masks with known answers, and the summary CSV with and without the
opening's four columns."""
import numpy as np
import pytest

import mask_ref as mr
from opticalflow3d_dev_amd import SummarySpec
from opticalflow3d_dev_amd.analysis import (CSV_COLUMNS, CSV_OPEN_COLUMNS, SUMS, read_summary_csv,
                                            write_summaries)


@pytest.mark.parametrize("kw, shape, match", [
    (dict(min_size=-1), (4, 5, 6), "min_size"),
    (dict(min_size=2.5), (4, 5, 6), "min_size"),
    (dict(min_size=True), (4, 5, 6), "min_size"),
    (dict(min_size=3, connectivity=26), (5, 6), "connectivity"),
    (dict(min_size=3, connectivity=8), (4, 5, 6), "connectivity"),
    (dict(min_size=3, connectivity=7), (4, 5, 6), "connectivity"),
    (dict(min_size=3, connectivity=7), (5, 6), "connectivity"),
    (dict(connectivity=6.0), (4, 5, 6), "connectivity"),
])
def test_spec_rejects_bad_opening(kw, shape, match):
    with pytest.raises(ValueError, match="summary: " + match):
        SummarySpec(**kw).resolve(shape)


def test_spec_defaults_and_valid_values():
    assert SummarySpec().opening(3) == (0, 26) and SummarySpec().opening(2) == (0, 8)
    assert SummarySpec(min_size=np.int64(7), connectivity=18).opening(3) == (7, 18)
    assert SummarySpec(min_size=1, connectivity=4).opening(2) == (1, 4)
    boxes, nbins, edges = SummarySpec(min_size=5).resolve((4, 5, 6))  # resolve's result is unchanged
    assert boxes.tolist() == [[0, 4, 0, 5, 0, 6]] and nbins == [0] * 6 and edges == [None] * 6
    assert CSV_OPEN_COLUMNS == mr.COUNTS


def test_open_ref_checkerboard():
    rel = mr.checkerboard()
    boxes = mr.boxes_of(rel.shape, None)
    assert rel.sum() == 60
    keep, c = mr.open_ref(rel, 0.5, boxes, 2, 6)
    assert not keep.any() and (c["n_mask"], c["n_components"], c["n_components_kept"], c["n_kept"]) == (60, 60, 0, 0)
    for conn in (18, 26):
        keep, c = mr.open_ref(rel, 0.5, boxes, 60, conn)
        assert np.array_equal(keep, rel.astype(np.uint16)) and c["n_components"] == 1 and c["n_kept"] == 60
        keep, c = mr.open_ref(rel, 0.5, boxes, 61, conn)
        assert not keep.any() and c["n_components"] == 1 and c["n_components_kept"] == 0


def test_open_ref_u_shape():
    rel, boxes = mr.u_shape()
    keep, c = mr.open_ref(rel, 0.5, boxes, 15, 26)
    assert c["n_mask"].tolist() == [31, 20] and c["n_components"].tolist() == [1, 2]
    assert c["n_components_kept"].tolist() == [1, 0] and c["n_kept"].tolist() == [31, 0]
    assert np.array_equal(keep, rel.astype(np.uint16))  # bit 0 on the whole U, bit 1 nowhere
    keep, c = mr.open_ref(rel, 0.5, boxes, 10, 26)
    assert c["n_kept"].tolist() == [31, 20] and keep[2, 5, 10] == 3 and keep[2, 15, 12] == 1


def test_open_ref_2d_and_nan():
    rel = np.array([[1, 0, np.nan, 1], [0, 1, 0, np.inf], [0, 0, 0, -np.inf]], np.float64)
    boxes = mr.boxes_of(rel.shape, None)
    keep, c = mr.open_ref(rel, 0.5, boxes, 2, 4)
    assert keep.tolist() == [[0, 0, 0, 1], [0, 0, 0, 1], [0, 0, 0, 0]] and c["n_components"] == 3
    keep, c = mr.open_ref(rel, 0.5, boxes, 2, 8)
    assert keep.tolist() == [[1, 0, 0, 1], [0, 1, 0, 1], [0, 0, 0, 0]] and c["n_components_kept"] == 2
    keep, c = mr.open_ref(rel, np.nan, boxes, 1, 8)
    assert not keep.any() and c["n_mask"] == 0


def _summaries(opened):
    rng = np.random.default_rng(5)
    out = []
    for f in range(2):
        s = {"rois": np.array([[0, 4, 0, 5, 0, 6], [1, 3, 0, 5, 2, 6]]), "threshold": np.float32(rng.random()),
             "n_valid": rng.integers(0, 90, 2), "n_voxels": np.array([120, 40]), "hist": {}, "edges": {}}
        for k in CSV_COLUMNS[11:]:
            s[k] = rng.standard_normal(2)
        if opened:
            for k in CSV_OPEN_COLUMNS:
                s[k] = rng.integers(0, 2 ** 40, 2)
        out.append(s)
    return out


@pytest.mark.parametrize("opened", [False, True])
def test_csv_round_trip(tmp_path, opened):
    summ = _summaries(opened)
    write_summaries(str(tmp_path / "s"), [3, 4], summ)
    header = (tmp_path / "s_summary.csv").read_text().splitlines()[0].split(",")
    assert header == list(CSV_COLUMNS + (CSV_OPEN_COLUMNS if opened else ()))
    csv = read_summary_csv(tmp_path / "s_summary.csv")
    assert list(csv) == header and csv["frame"].tolist() == [3, 3, 4, 4]
    for i, s in enumerate(summ):
        rows = slice(2 * i, 2 * i + 2)
        for k in SUMS + ("mean_magnitude", "theta_mean"):
            assert np.array_equal(csv[k][rows], s[k]), k
        for k in CSV_OPEN_COLUMNS if opened else ():
            assert csv[k].dtype == np.int64 and np.array_equal(csv[k][rows], s[k]), k
