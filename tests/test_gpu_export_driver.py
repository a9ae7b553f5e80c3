"""The field export through the drivers: FlowStream(summary=, fields=FieldSpec) against the numpy
restatement (tests/export_ref.py) applied to the fields of a fields=True stream, in all three
d2h modes, and process_flow(save_fields=FieldSpec)'s ROI TIFFs against the crops of a
save_fields=True run's TIFFs — values bitwise where not NaN, NaNs in the same places — with
every other file and the stdout lines what they are without it."""
import contextlib
import io

import numpy as np
import pytest

import export_ref as er
from opticalflow3d_dev_amd import FieldSpec, SummarySpec, process_flow
from opticalflow3d_dev_amd import tiff as tf
from opticalflow3d_dev_amd.stream import FlowStream

pytestmark = pytest.mark.gpu

D_KW = dict(rel_percentile=70, xyscale=0.1, zscale=0.3, tscale=2.0)
SHAPE = (8, 24, 40)
ROIS = [(1, 7, 3, 22, 5, 38), (4, 8, 0, 12, 21, 40)]


@pytest.fixture(scope="module")
def series():
    return np.random.default_rng(80).integers(0, 4096, size=(9,) + SHAPE).astype(np.uint16)  # 2 rt + 3 frames


def _stream(series, frames, **kw):
    """Submit `frames` windows of 7 frames; per window the copied full-size fields or export blocks."""
    fs = FlowStream(3, SHAPE, series.dtype, 1, 1, 2, **kw)
    out, pushed = [], 0
    try:
        for i in range(frames):
            while pushed < min(i + 7 + fs.lookahead, len(series)):
                fs.push(series[pushed])
                pushed += 1
            p = fs.submit()
            if fs.field_spec is None:
                out.append([a.copy() for a in p.result()])
            else:
                with pytest.raises(RuntimeError, match="fields()"):
                    p.result()
                assert all(h is None for h in fs.hout)  # no full-size pinned buffer
                blocks = p.fields()
                out.append(([{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in b.items()} for b in blocks],
                            p.summary()))
            p.release()
    finally:
        fs.close()
    return out


@pytest.fixture(scope="module")
def full_fields(series):
    return _stream(series, 3)


def _reference(f, request, min_size):
    names = request.resolve(3, len(ROIS) + 1)[1]
    ref = er.export_ref(*f, **D_KW, rois=ROIS, export_rois=request.resolve(3, len(ROIS) + 1)[0], fields=names,
                        mask=request.mask, physical=request.physical, dtype=request.dtype, min_size=min_size,
                        connectivity=26)
    if request.mask is not None:
        for blk, n in zip(ref["blocks"], ref["inside"]):
            assert 0 < n < blk[names[0]].size, (blk["roi"], n)
    return ref


@pytest.mark.parametrize("d2h,request_,min_size", [
    ("dma", FieldSpec(dtype="float32"), 3),
    ("kernel", FieldSpec(rois=(2, 0), mask="summary"), 0),
    ("runtime", FieldSpec(fields=("vy", "rel"), mask="zero", physical=False), 3),
])
def test_flowstream_fields_equal_the_restatement_on_the_full_fields(series, full_fields, d2h, request_, min_size):
    spec = SummarySpec(rois=ROIS, min_size=min_size, **D_KW)
    got = _stream(series, 3, summary=spec, fields=request_, d2h=d2h)
    for (blocks, summary), f in zip(got, full_fields):
        ref = _reference(f, request_, min_size)
        er.assert_blocks({"rois": summary["rois"], "threshold": summary["threshold"], "blocks": blocks}, ref)
    with pytest.raises(RuntimeError, match="FieldSpec"):
        fs = FlowStream(3, SHAPE, series.dtype, 1, 1, 2, summary=SummarySpec(**D_KW), fields=False)
        try:
            for k in range(min(7 + fs.lookahead, len(series))):
                fs.push(series[k])
            fs.submit().fields()
        finally:
            fs.close()


def _lines(text):
    """stdout without the timestamps and durations."""
    return [l.split(" - ", 1)[-1].split("  Duration")[0] for l in text.splitlines()]


def _run(path, **kw):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        process_flow(str(path), "cells", "OneTif", 3, 1, 1, 2, **kw)
    return buf.getvalue()


def test_process_flow_writes_the_roi_files_and_nothing_else_changes(series, tmp_path):
    request = FieldSpec(rois=(1, 2), dtype="float32")
    spec = SummarySpec(rois=ROIS, min_size=3, **D_KW)
    for name in ("roi", "full"):
        (tmp_path / name).mkdir()
        tf.imwrite(tmp_path / name / "cells.tif", series, imagej=True)
    text = _run(tmp_path / "roi", summary=spec, save_fields=request)
    text0 = _run(tmp_path / "full", summary=spec, save_fields=True)
    out, out0 = (tmp_path / name / "OpticalFlow3D" / "cells" for name in ("roi", "full"))
    assert _lines(text) == _lines(text0) and "Frame 5 saved." in _lines(text)
    common = ["cells_parameters.csv", "cells_summary.csv", "cells_summary_hist.npz"]
    names = ("vx", "vy", "vz", "rel")
    # the save_fields=True run writes exactly the files it always did
    assert sorted(p.name for p in out0.iterdir()) == sorted(
        common + [f"cells_{n}_t{t:04d}.tiff" for n in names for t in (3, 4, 5)])
    assert sorted(p.name for p in out.iterdir()) == sorted(
        common + ["cells_fields.csv"] + [f"cells_{n}_roi{r}_t{t:04d}.tiff" for n in names for r in (1, 2)
                                          for t in (3, 4, 5)])
    assert not list(out.glob("cells_vx_t*.tiff"))
    for name in common:
        assert (out / name).read_bytes() == (out0 / name).read_bytes(), name
    rows = (out / "cells_fields.csv").read_text().splitlines()
    assert rows[0] == "roi,z0,z1,y0,y1,x0,x1,mask,physical,dtype,xyscale,zscale,tscale"
    assert rows[1:] == ["1,1,7,3,22,5,38,nan,True,float32,0.1,0.3,2.0", "2,4,8,0,12,21,40,nan,True,float32,0.1,0.3,2.0"]
    for t in (3, 4, 5):
        f = [tf.imread(out0 / f"cells_{n}_t{t:04d}.tiff") for n in names]
        assert f[0].dtype == np.float64 and f[3].dtype == np.float32
        ref = _reference(f, request, 3)
        for blk in ref["blocks"]:
            for n in names:
                got = tf.imread(out / f"cells_{n}_roi{blk['roi']}_t{t:04d}.tiff")
                assert er.same(got, blk[n]), (t, blk["roi"], n)
