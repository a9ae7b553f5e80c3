"""The projection maps through the drivers: FlowStream(summary=, project=, fields=False) against
projection_maps on the fields of a fields=True stream with the series' centre frames as the image,
and process_flow(project=)'s npz files against the stream's results — all exact — with the
summary route's own words and files byte-identical whether or not a projection is requested."""
import numpy as np
import pytest

from opticalflow3d_dev_amd import ProjectionSpec, SummarySpec, process_flow, projection_maps
from opticalflow3d_dev_amd import tiff as tf
from opticalflow3d_dev_amd.analysis import read_projections
from opticalflow3d_dev_amd.stream import FlowStream

pytestmark = pytest.mark.gpu

D_KW = dict(rel_percentile=70, xyscale=0.1, zscale=0.3, tscale=2.0)
SHAPE = (24, 40, 64)
ROIS = [(2, 22, 5, 37, 3, 60), (10, 24, 0, 20, 30, 64)]
REQUEST = ProjectionSpec(axes=("z", "x"), image=True)


def _series(seed, shape=SHAPE, frames=9):
    """uint16 frames with values above 32767 (the ring keeps them in int16 storage)."""
    s = np.random.default_rng(seed).integers(30000, 65536, size=(frames,) + shape).astype(np.uint16)
    assert (s > 32767).mean() > 0.5
    return s


def _same_maps(got, want):
    assert got["axes"] == want["axes"] and np.array_equal(got["rois"], want["rois"])
    assert got["threshold"] == want["threshold"] and len(got["maps"]) == len(want["maps"])
    for g, w in zip(got["maps"], want["maps"]):
        assert g["roi"] == w["roi"] and g["box"] == w["box"]
        for a in got["axes"]:
            assert sorted(g[a]) == sorted(w[a])
            for name, v in g[a].items():
                assert v.dtype == w[a][name].dtype and v.tobytes() == w[a][name].tobytes(), (g["roi"], a, name)


def _run(fs, series, frames):
    """Submit `frames` windows of 7 frames; per window (summary words, projections, fields)."""
    out, pushed = [], 0
    try:
        for i in range(frames):
            while pushed < min(i + 7 + fs.lookahead, len(series)):
                fs.push(series[pushed])
                pushed += 1
            p = fs.submit()
            project = fs.summary is not None and fs.summary.project is not None
            if fs.summary is not None:
                p.summary()
            out.append((fs.hsum[p.b].numpy().copy() if fs.summary is not None else None,
                        p.projections() if project else None,
                        [a.copy() for a in p.result()] if fs.fields else None))
            p.release()
    finally:
        fs.close()
    return out


def test_flowstream_projections_equal_projection_maps_on_the_fields():
    series = _series(80)
    spec = SummarySpec(rois=ROIS, min_size=5, **D_KW)
    maps = _run(FlowStream(3, SHAPE, np.uint16, 1, 1, 2, summary=spec, project=REQUEST, fields=False), series, 3)
    fields = _run(FlowStream(3, SHAPE, np.uint16, 1, 1, 2), series, 3)
    plain = _run(FlowStream(3, SHAPE, np.uint16, 1, 1, 2, summary=spec, fields=False), series, 3)
    for i, ((words, got, _), (_, _, f), (words0, _, _)) in enumerate(zip(maps, fields, plain)):
        want = projection_maps(*f, image=series[i + 3], spec=REQUEST, rois=ROIS, min_size=5, **D_KW)
        _same_maps(got, want)
        assert [e["roi"] for e in got["maps"]] == [1, 2] and got["maps"][0]["z"]["max_image"].shape == (32, 57)
        assert got["maps"][0]["z"]["max_image"].min() > 32767 and got["maps"][1]["x"]["max_image"].min() > 32767
        assert 0 < got["maps"][0]["x"]["n_valid"].sum() <= got["maps"][0]["x"]["n_mask"].sum()
        assert words.tobytes() == words0.tobytes()  # the summary is what it is without the request


def test_project_needs_a_summary_and_a_request():
    with pytest.raises(ValueError, match="FlowStream: project needs a summary"):
        FlowStream(3, (6, 16, 20), np.uint16, 1, 1, 2, project=REQUEST)
    series = _series(81, (6, 16, 20))
    fs = FlowStream(3, (6, 16, 20), np.uint16, 1, 1, 2, summary=SummarySpec(**D_KW), fields=False)
    try:
        for k in range(min(7 + fs.lookahead, len(series))):
            fs.push(series[k])
        p = fs.submit()
        with pytest.raises(RuntimeError, match="project"):
            p.projections()
    finally:
        fs.close()


def test_process_flow_writes_the_projection_files_and_nothing_else_changes(tmp_path):
    shape = (6, 16, 20)
    series = _series(82, shape)
    rois = [(1, 5, 3, 14, 2, 17)]
    kw = dict(rois=rois, bins={"magnitude": np.linspace(0.0, 0.5, 11)}, min_size=3)
    request = ProjectionSpec(axes=("z", "y", "x"), rois=(0, 1), image=True)
    for name in ("with", "without"):
        (tmp_path / name).mkdir()
        tf.imwrite(tmp_path / name / "cells.tif", series, imagej=True)
    with pytest.raises(ValueError, match="^project needs a summary"):
        process_flow(str(tmp_path / "with"), "cells", "OneTif", 3, 1, 1, 2, project=request)
    process_flow(str(tmp_path / "with"), "cells", "OneTif", 3, 1, 1, 2, summary=SummarySpec(**kw, **D_KW),
                 save_fields=False, project=request)
    process_flow(str(tmp_path / "without"), "cells", "OneTif", 3, 1, 1, 2, summary=SummarySpec(**kw, **D_KW),
                 save_fields=False)
    out, out0 = (tmp_path / name / "OpticalFlow3D" / "cells" for name in ("with", "without"))
    common = ["cells_parameters.csv", "cells_summary.csv", "cells_summary_hist.npz"]
    assert sorted(p.name for p in out0.iterdir()) == common
    assert sorted(p.name for p in out.iterdir()) == sorted(common + [f"cells_project_t{t:04d}.npz" for t in (3, 4, 5)])
    for name in common[1:]:
        assert (out / name).read_bytes() == (out0 / name).read_bytes(), name
    stream = _run(FlowStream(3, shape, np.uint16, 1, 1, 2, summary=SummarySpec(**kw, **D_KW), project=request,
                             fields=False), series, 3)
    for i, (_, want, _) in enumerate(stream):
        got = read_projections(out / f"cells_project_t{i + 3:04d}.npz")
        _same_maps(got, want)
        assert got["maps"][1]["z"]["sum_image"].shape == (11, 15) and got["maps"][0]["x"]["n_mask"].shape == (6, 16)
