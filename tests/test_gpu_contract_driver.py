"""Contractility through the drivers: process_flow(summary=, contract=, save_fields=False)'s CSV
and npz against analysis.contractility on the same frames' fields, with the summary route's own
files byte-identical whether or not a contract is requested; FlowStream(contract=) with the
summary's opened mask against the numpy restatement (tests/contract_ref.py)."""
import numpy as np
import pytest

import contract_ref as cr
import mask_ref as mr
from opticalflow3d_dev_amd import ContractSpec, SummarySpec, calc_flow3D, contractility, process_flow
from opticalflow3d_dev_amd import tiff as tf
from opticalflow3d_dev_amd.analysis import CONTRACT_CSV_COLUMNS, read_contract_csv
from opticalflow3d_dev_amd.stream import FlowStream

pytestmark = pytest.mark.gpu

D_KW = dict(rel_percentile=70, xyscale=0.1, zscale=0.3, tscale=2.0)
BINS = {"angle": np.linspace(0.0, 180.0, 19), "inward": np.linspace(-0.05, 0.05, 21)}


def test_process_flow_writes_the_contract_files_and_nothing_else_changes(tmp_path):
    series = np.random.default_rng(81).integers(0, 4096, size=(9, 6, 16, 20)).astype(np.uint16)
    rois = [(1, 5, 3, 14, 2, 17)]
    kw = dict(rois=rois, bins={"magnitude": np.linspace(0.0, 0.5, 11)}, min_size=3)
    request = ContractSpec(connectivity=18, bins=BINS)
    for name in ("with", "without"):
        (tmp_path / name).mkdir()
        tf.imwrite(tmp_path / name / "cells.tif", series, imagej=True)
    process_flow(str(tmp_path / "with"), "cells", "OneTif", 3, 1, 1, 2, summary=SummarySpec(**kw, **D_KW),
                 save_fields=False, contract=request)
    process_flow(str(tmp_path / "without"), "cells", "OneTif", 3, 1, 1, 2, summary=SummarySpec(**kw, **D_KW),
                 save_fields=False)
    out, out0 = (tmp_path / name / "OpticalFlow3D" / "cells" for name in ("with", "without"))
    common = ["cells_parameters.csv", "cells_summary.csv", "cells_summary_hist.npz"]
    assert sorted(p.name for p in out0.iterdir()) == common
    assert sorted(p.name for p in out.iterdir()) == sorted(common + ["cells_contract.csv", "cells_contract_hist.npz"])
    for name in common[1:]:
        assert (out / name).read_bytes() == (out0 / name).read_bytes(), name
    rows = read_contract_csv(out / "cells_contract.csv")
    assert tuple(rows) == CONTRACT_CSV_COLUMNS and rows["frame"].tolist() == [3, 3, 4, 4, 5, 5]
    npz = np.load(out / "cells_contract_hist.npz")
    assert sorted(npz.files) == ["counts_angle", "counts_inward", "edges_angle", "edges_inward", "frames"]
    assert npz["frames"].tolist() == [3, 4, 5] and npz["counts_angle"].shape == (3, 2, 18)
    for i in range(3):
        want = contractility(*calc_flow3D(series[i:i + 7], 1, 1, 2), **D_KW, rois=rois, spec=request)
        assert np.all(want["n_angle"] > 0)
        sl = slice(2 * i, 2 * i + 2)
        for k in ("n_mask", "n_components", "n_kept", "n_valid", "n_angle", "n_inward"):
            assert np.array_equal(rows[k][sl], want[k]), (i, k)
        for k in ("mean_angle", "mean_dot", "mean_inward", "mean_speed", "inward_fraction", "sum_angle", "sum_dot",
                  "sum_inward", "sum_speed"):
            assert rows[k][sl].tobytes() == want[k].tobytes(), (i, k)
        for a, c in enumerate("xyz"):
            assert rows["centroid_" + c][sl].tobytes() == want["centroid"][:, a].tobytes(), (i, c)
            assert rows["center_" + c][sl].tobytes() == want["center_used"][:, a].tobytes(), (i, c)
        assert np.array_equal(np.stack([rows[k][sl] for k in ("z0", "z1", "y0", "y1", "x0", "x1")], 1), want["rois"])
        for k in BINS:
            assert np.array_equal(npz["counts_" + k][i], want["hist"][k]) and np.array_equal(npz["edges_" + k], BINS[k])
    with pytest.raises(ValueError, match="contract needs a summary"):
        process_flow(str(tmp_path / "without"), "cells", "OneTif", 3, 1, 1, 2, contract=request)


def test_flowstream_contract_over_the_summarys_opened_mask():
    shape = (6, 16, 20)
    series = np.random.default_rng(82).integers(0, 4096, size=(9,) + shape).astype(np.uint16)
    rois = [(1, 5, 3, 14, 2, 17)]
    spec = SummarySpec(rois=rois, min_size=4, connectivity=6, **D_KW)
    fs = FlowStream(3, shape, series.dtype, 1, 1, 2, summary=spec, contract=ContractSpec(mask="summary"), fields=False)
    scales = {k: D_KW[k] for k in ("xyscale", "zscale", "tscale")}
    try:
        pushed = 0
        for i in range(2):
            while pushed < min(i + 7 + fs.lookahead, len(series)):
                fs.push(series[pushed])
                pushed += 1
            p = fs.submit()
            summary, got = p.summary(), p.contract()
            p.release()
            vx, vy, vz, rel = calc_flow3D(series[i:i + 7], 1, 1, 2)
            boxes, thresh = mr.boxes_of(shape, rois), np.percentile(rel, D_KW["rel_percentile"])
            keep, counts = mr.open_ref(rel, thresh, boxes, 4, 6)
            ref = cr.contract_ref(vx, vy, vz, keep, boxes, **scales)
            assert got["threshold"] == thresh == summary["threshold"]
            assert np.array_equal(got["moments"], ref["moments"]) and np.array_equal(got["n_kept"], counts["n_kept"])
            assert np.array_equal(summary["n_kept"], counts["n_kept"]) and np.any(counts["n_kept"] < counts["n_mask"])
            for k in ("n_valid", "n_angle", "n_inward"):
                assert np.array_equal(got[k], ref[k]), k
            assert np.array_equal(got["n_valid"], summary["n_valid"])
            for k in cr.SUMS:
                assert np.all(np.abs(got[k] - ref[k]) <= cr.sum_bound(ref, k)), k
            with pytest.raises(RuntimeError, match="quiver"):
                p.quiver()
    finally:
        fs.close()
    with pytest.raises(ValueError, match="contract needs a summary"):
        FlowStream(3, shape, series.dtype, 1, 1, 2, contract=ContractSpec())
