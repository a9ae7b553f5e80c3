"""The quiver samples through the drivers: FlowStream(summary=, quiver=, fields=False) against
quiver_sample on the fields of a fields=True stream, and process_flow(quiver=)'s npz files against
the numpy restatement (tests/quiver_ref.py) — all exact — with the summary route's own files
byte-identical whether or not a quiver is requested."""
import numpy as np
import pytest

import mask_ref as mr
import quiver_ref as qr
from opticalflow3d_dev_amd import QuiverSpec, SummarySpec, calc_flow3D, process_flow, quiver_sample
from opticalflow3d_dev_amd import tiff as tf
from opticalflow3d_dev_amd.stream import FlowStream

pytestmark = pytest.mark.gpu

D_KW = dict(rel_percentile=70, xyscale=0.1, zscale=0.3, tscale=2.0)


def _same_samples(got, want):
    assert len(got) == len(want)
    for r, (g, w) in enumerate(zip(got, want)):
        assert set(g) == set(w), r
        assert g["n_valid"] == w["n_valid"] and g["n_lattice"] == w["n_lattice"] and g["truncated"] == w["truncated"], r
        assert np.array_equal(g["zyx"], w["zyx"]), r
        for k in ("v", "magnitude", "theta", "phi"):
            assert g[k].dtype == np.float64 and g[k].tobytes() == w[k].tobytes(), (r, k)


def _run(fs, series, frames):
    """Submit `frames` windows of 7 frames; per window (summary or None, quiver or None, fields or None)."""
    out, pushed = [], 0
    try:
        for i in range(frames):
            while pushed < min(i + 7 + fs.lookahead, len(series)):
                fs.push(series[pushed])
                pushed += 1
            p = fs.submit()
            out.append((p.summary() if fs.summary is not None else None,
                        p.quiver() if fs.summary is not None and fs.summary.quiver is not None else None,
                        [a.copy() for a in p.result()] if fs.fields else None))
            p.release()
    finally:
        fs.close()
    return out


def test_flowstream_quiver_equals_quiver_sample_on_the_fields():
    shape = (24, 40, 64)
    series = np.random.default_rng(70).integers(0, 4096, size=(9,) + shape).astype(np.uint16)  # 2 rt + 3 frames
    rois = [(2, 22, 5, 37, 3, 60), (10, 24, 0, 20, 30, 64)]
    spec = SummarySpec(rois=rois, min_size=5, **D_KW)
    request = QuiverSpec(gap=(2, 3, 4), max_vectors=300)
    lists = _run(FlowStream(3, shape, series.dtype, 1, 1, 2, summary=spec, quiver=request, fields=False), series, 3)
    fields = _run(FlowStream(3, shape, series.dtype, 1, 1, 2), series, 3)
    plain = _run(FlowStream(3, shape, series.dtype, 1, 1, 2, summary=spec, fields=False), series, 3)
    truncated = 0
    for (summary, got, _), (_, _, f), (summary0, _, _) in zip(lists, fields, plain):
        want = quiver_sample(*f, **D_KW, gap=(2, 3, 4), rois=rois, min_size=5, max_vectors=300)
        _same_samples(got, want["samples"])
        assert want["threshold"] == summary["threshold"]
        assert want["samples"][1]["n_lattice"] == 10 * 11 * 15
        assert 0 < want["samples"][2]["n_valid"] < want["samples"][2]["n_lattice"] == 7 * 7 * 9
        truncated += want["samples"][0]["truncated"]
        assert not want["samples"][2]["truncated"]
        # the summary is what it is without the quiver request
        assert set(summary) == set(summary0)
        for k in ("n_valid", "n_kept", "sum_magnitude", "sum_vx", "threshold"):
            assert np.asarray(summary[k]).tobytes() == np.asarray(summary0[k]).tobytes(), k
    assert truncated == 3  # the whole volume's list (12 x 14 x 16 lattice points) overflows 300 in every frame
    with pytest.raises(RuntimeError, match="quiver"):
        fs = FlowStream(3, (6, 16, 20), series.dtype, 1, 1, 2, summary=SummarySpec(**D_KW), fields=False)
        try:
            for k in range(min(7 + fs.lookahead, len(series))):
                fs.push(series[k][:6, :16, :20])
            p = fs.submit()
            p.quiver()
        finally:
            fs.close()


def test_process_flow_writes_the_quiver_files_and_nothing_else_changes(tmp_path):
    series = np.random.default_rng(71).integers(0, 4096, size=(9, 6, 16, 20)).astype(np.uint16)
    rois = [(1, 5, 3, 14, 2, 17)]
    kw = dict(rois=rois, bins={"magnitude": np.linspace(0.0, 0.5, 11)}, min_size=3)
    for name in ("with", "without"):
        (tmp_path / name).mkdir()
        tf.imwrite(tmp_path / name / "cells.tif", series, imagej=True)
    process_flow(str(tmp_path / "with"), "cells", "OneTif", 3, 1, 1, 2, summary=SummarySpec(**kw, **D_KW),
                 save_fields=False, quiver=QuiverSpec(gap=(1, 2, 3)))
    process_flow(str(tmp_path / "without"), "cells", "OneTif", 3, 1, 1, 2, summary=SummarySpec(**kw, **D_KW),
                 save_fields=False)
    out, out0 = (tmp_path / name / "OpticalFlow3D" / "cells" for name in ("with", "without"))
    common = ["cells_parameters.csv", "cells_summary.csv", "cells_summary_hist.npz"]
    assert sorted(p.name for p in out0.iterdir()) == common
    assert sorted(p.name for p in out.iterdir()) == sorted(common + [f"cells_quiver_t{t:04d}.npz" for t in (3, 4, 5)])
    for name in common[1:]:
        assert (out / name).read_bytes() == (out0 / name).read_bytes(), name
    for i in range(3):
        vx, vy, vz, rel = calc_flow3D(series[i:i + 7], 1, 1, 2)
        boxes, thresh = mr.boxes_of(vx.shape, rois), np.percentile(rel, D_KW["rel_percentile"])
        keep, _ = mr.open_ref(rel, thresh, boxes, 3, 26)
        ref = qr.quiver_ref(vx, vy, vz, rel, **D_KW, gap=(1, 2, 3), rois=rois, keep=keep)
        npz = np.load(out / f"cells_quiver_t{i + 3:04d}.npz")
        assert sorted(npz.files) == sorted(["gap", "rois", "threshold"] + [f"{k}_{r}" for r in range(2) for k in
                                                                           ("zyx", "v", "n_valid", "n_lattice")])
        assert npz["gap"].tolist() == [1, 2, 3] and np.array_equal(npz["rois"], boxes)
        assert npz["threshold"].dtype == rel.dtype and npz["threshold"] == thresh
        for r, s in enumerate(ref["samples"]):
            assert 0 < s["n_valid"] < s["n_lattice"], (i, r)
            assert int(npz[f"n_valid_{r}"]) == s["n_valid"] and int(npz[f"n_lattice_{r}"]) == s["n_lattice"]
            assert np.array_equal(npz[f"zyx_{r}"], s["zyx"]) and npz[f"zyx_{r}"].dtype == np.int64
            assert npz[f"v_{r}"].dtype == np.float64 and npz[f"v_{r}"].tobytes() == s["v"].tobytes(), (i, r)
