"""process_flow / FlowStream with a device-side summary: the CSV and npz rows equal
flow_summary of each window's fields, no field TIFFs with save_fields=False, the reference's
stdout lines and (with save_fields=True) the TIFFs unchanged."""
import contextlib
import io

import numpy as np
import pytest

import summary_ref as sr
from conftest import bits_equal
from opticalflow3d_dev_amd import SummarySpec, calc_flow2D, calc_flow3D, flow_summary, process_flow
from opticalflow3d_dev_amd import tiff as tf
from opticalflow3d_dev_amd.analysis import SUMS, read_summary_csv

pytestmark = pytest.mark.gpu

ROIS = [(0, 8, 0, 24, 0, 40), (2, 3, 5, 6, 7, 8), (1, 7, 3, 20, 5, 8), (4, 8, 10, 24, 21, 40)]
BINS = {"vx": np.linspace(-0.3, 0.3, 13), "magnitude": np.linspace(0.0, 0.5, 11),
        "theta": -np.pi + (np.arange(13) + (np.sqrt(2.0) - 1.0)) * (2 * np.pi / 12)}
SPEC = SummarySpec(rois=ROIS, bins=BINS, rel_percentile=80, xyscale=0.1, zscale=0.3, tscale=2.0)


def _lines(text):
    """stdout without the timestamps and durations."""
    return [l.split(" - ", 1)[-1].split("  Duration")[0] for l in text.splitlines()]


def _run(path, **kw):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        process_flow(str(path), "cells", "OneTif", 3, 1, 1, 2, **kw)
    return buf.getvalue()


@pytest.fixture(scope="module")
def runs3d(tmp_path_factory):
    stack = np.random.default_rng(21).integers(0, 4096, size=(9, 8, 24, 40)).astype(np.uint16)
    out = {"stack": stack}
    for mode, kw in (("plain", {}), ("summary_only", dict(summary=SPEC, save_fields=False)),
                     ("both", dict(summary=SPEC))):
        d = tmp_path_factory.mktemp(mode)
        tf.imwrite(d / "cells.tif", stack, imagej=True)
        out[mode] = (d / "OpticalFlow3D" / "cells", _run(d, **kw))
    return out


def _check_rows(csv, npz, frame_rows, frame_i, got, ref):
    """One frame's CSV rows and npz counts against flow_summary's dict (exact) and summary_ref."""
    rows = slice(frame_rows * frame_i, frame_rows * (frame_i + 1))
    assert np.array_equal(np.stack([csv[k][rows] for k in ("z0", "z1", "y0", "y1", "x0", "x1")], 1), got["rois"])
    assert np.all(csv["threshold"][rows] == np.float64(got["threshold"])) and got["threshold"] == ref["threshold"]
    for k in ("n_valid", "n_voxels"):
        assert np.array_equal(csv[k][rows], got[k]) and np.array_equal(got[k], ref[k]), k
    for k in SUMS:
        assert np.all(np.abs(csv[k][rows] - ref[k]) <= sr.sum_bound(ref, k)), k
    for k in ("mean_magnitude", "theta_mean", "theta_mean_weighted") + SUMS:
        assert np.array_equal(csv[k][rows], got[k], equal_nan=True), k  # the same kernels on the same fields
    for k in got["hist"]:
        assert np.array_equal(npz["counts_" + k][frame_i], got["hist"][k]), k
        assert np.array_equal(npz["edges_" + k], got["edges"][k])
    for k in ("vx", "magnitude"):
        assert np.array_equal(got["hist"][k], ref["hist"][k]), k


def test_summary_only_3d(runs3d):
    out, _ = runs3d["summary_only"]
    assert not list(out.glob("*.tiff")) and not list(out.glob("*.tif"))
    assert sorted(p.name for p in out.iterdir()) == ["cells_parameters.csv", "cells_summary.csv",
                                                    "cells_summary_hist.npz"]
    csv, npz = read_summary_csv(out / "cells_summary.csv"), np.load(out / "cells_summary_hist.npz")
    assert csv["frame"].tolist() == [f for f in (3, 4, 5) for _ in ROIS + [0]]
    assert csv["roi"].tolist() == list(range(len(ROIS) + 1)) * 3 and npz["frames"].tolist() == [3, 4, 5]
    assert npz["counts_theta"].shape == (3, len(ROIS) + 1, 12) and npz["counts_theta"].dtype == np.uint64
    kw = dict(rois=ROIS, bins=BINS)
    for i in range(3):
        f = calc_flow3D(runs3d["stack"][i:i + 7], 1, 1, 2)
        got = flow_summary(*f, 80, 0.1, 0.3, 2.0, **kw)
        ref = sr.summary_ref(*f, 80, 0.1, 0.3, 2.0, **kw)
        assert ref["n_valid"][0] > 0
        _check_rows(csv, npz, len(ROIS) + 1, i, got, ref)


def test_stdout_lines_are_the_same_in_every_mode(runs3d):
    plain = _lines(runs3d["plain"][1])
    assert "Processing frame 3..." in plain and "Frame 5 saved." in plain
    assert _lines(runs3d["summary_only"][1]) == plain
    assert _lines(runs3d["both"][1]) == plain


def test_fields_unchanged_beside_a_summary(runs3d):
    plain, both, only = runs3d["plain"][0], runs3d["both"][0], runs3d["summary_only"][0]
    names = sorted(p.name for p in plain.glob("*.tiff"))
    assert len(names) == 12 and names == sorted(p.name for p in both.glob("*.tiff"))
    for n in names:
        assert bits_equal(tf.imread(plain / n), tf.imread(both / n)), n
    assert (both / "cells_summary.csv").read_text() == (only / "cells_summary.csv").read_text()
    a, b = np.load(both / "cells_summary_hist.npz"), np.load(only / "cells_summary_hist.npz")
    assert sorted(a.files) == sorted(b.files) and all(np.array_equal(a[k], b[k]) for k in a.files)


def test_summary_2d_sequence(tmp_path):
    stack = np.random.default_rng(22).integers(0, 4096, size=(8, 30, 26)).astype(np.uint16)
    for t in range(8):
        tf.imwrite(tmp_path / f"img_t{t}_ch0.tif", stack[t])
    rois, bins = [(0, 30, 0, 26), (3, 4, 5, 6), (10, 30, 7, 10)], {"vy": np.linspace(-1.0, 1.0, 9)}
    spec = SummarySpec(rois=rois, bins=bins, rel_percentile=75)
    process_flow(str(tmp_path), "img_t.*_ch0", "SequenceT", 2, 1, 1, 3, summary=spec, save_fields=False)
    out = tmp_path / "OpticalFlow2D" / "img_t_ch0"
    assert not list(out.glob("*.tiff"))
    csv, npz = read_summary_csv(out / "img_t_ch0_summary.csv"), np.load(out / "img_t_ch0_summary_hist.npz")
    assert csv["frame"].tolist() == [3] * 4 + [4] * 4
    for i in range(2):
        vx, vy, rel = calc_flow2D(stack[i:i + 7], 1, 1, 3)
        got = flow_summary(vx, vy, None, rel, 75, rois=rois, bins=bins)
        ref = sr.summary_ref(vx, vy, None, rel, 75, rois=rois, bins=bins)
        rows = slice(4 * i, 4 * i + 4)
        assert np.array_equal(csv["n_valid"][rows], ref["n_valid"]) and ref["n_valid"][0] > 0
        assert np.all(csv["threshold"][rows] == ref["threshold"])
        for k in SUMS:
            assert np.all(np.abs(csv[k][rows] - ref[k]) <= sr.sum_bound(ref, k)), k
            assert np.array_equal(csv[k][rows], got[k]), k
        assert np.array_equal(npz["counts_vy"][i], ref["hist"]["vy"])


def test_fp32_and_matlab_output_modes(tmp_path):
    """The other ring modes: float32 fields, and matlab_output's float64 rel."""
    stack = np.random.default_rng(23).integers(0, 4096, size=(7, 4, 16, 18)).astype(np.uint16)
    from opticalflow3d_dev_amd import calc_flow3D_fp32
    from opticalflow3d_dev_amd.calc_flow import _flow3d

    for sub, kw, flow in (("a", dict(precision="fp32"), lambda: calc_flow3D_fp32(stack, 1, 1, 2)),
                          ("b", dict(matlab_output=True), lambda: _flow3d(stack, 1, 1, 2, rel_fp64=True))):
        d = tmp_path / sub
        d.mkdir()
        tf.imwrite(d / "s.tif", stack, imagej=True)
        process_flow(str(d), "s", "OneTif", 3, 1, 1, 2, summary=SummarySpec(rois=[(1, 3, 2, 9, 3, 6)]),
                     save_fields=False, **kw)
        csv = read_summary_csv(d / "OpticalFlow3D" / "s" / "s_summary.csv")
        got = flow_summary(*flow(), rois=[(1, 3, 2, 9, 3, 6)])
        assert csv["frame"].tolist() == [3, 3] and np.array_equal(csv["n_valid"], got["n_valid"])
        assert np.all(csv["threshold"] == np.float64(got["threshold"]))
        for k in SUMS:
            assert np.array_equal(csv[k], got[k]), k


def test_pending_result_raises_without_fields():
    from opticalflow3d_dev_amd.stream import FlowStream

    stack = np.random.default_rng(24).integers(0, 250, size=(7, 20, 22)).astype(np.uint8)
    with pytest.raises(ValueError, match="fields=False needs a summary"):
        FlowStream(2, (20, 22), np.uint8, 1, 1, 2, fields=False)
    fs = FlowStream(2, (20, 22), np.uint8, 1, 1, 2, summary=SummarySpec(), fields=False)
    try:
        assert all(h is None for h in fs.hout)  # no pinned field buffers
        for t in range(7):
            fs.push(stack[t])
        p = fs.submit()
        with pytest.raises(RuntimeError, match="fields=False"):
            p.result()
        s = p.summary()
        p.release()
    finally:
        fs.close()
    vx, vy, rel = calc_flow2D(stack, 1, 1, 2)
    want = flow_summary(vx, vy, None, rel)
    assert s["n_valid"].tolist() == want["n_valid"].tolist() and s["threshold"] == want["threshold"]
    assert np.array_equal(s["sum_magnitude"], want["sum_magnitude"])


def test_several_ranks_with_a_summary_raise(tmp_path, monkeypatch):
    import importlib

    cf = importlib.import_module("opticalflow3d_dev_amd.calc_flow")  # the module, not the calc_flow alias
    stack = np.random.default_rng(25).integers(0, 4096, size=(7, 3, 12, 14)).astype(np.uint16)
    tf.imwrite(tmp_path / "s.tif", stack, imagej=True)
    monkeypatch.setattr(cf, "_dist_context", lambda: (0, 2))
    with pytest.raises(ValueError, match="sharded"):
        process_flow(str(tmp_path), "s", "OneTif", 3, 1, 1, 2, summary=SummarySpec())
    assert not (tmp_path / "OpticalFlow3D").exists()  # refused before anything is written
    monkeypatch.undo()
    with pytest.raises(ValueError, match="device-ring"):
        process_flow(str(tmp_path), "s", "OneTif", 3, 1, 1.2, 2, summary=SummarySpec())
    with pytest.raises(ValueError, match="needs a summary"):
        process_flow(str(tmp_path), "s", "OneTif", 3, 1, 1, 2, save_fields=False)
