"""of3d_rel_select / of3d_rel_profile on the GPU against numpy on the crops (relsel_ref.py), and the
percentile_box / percentile_method / rel_profile options through the analysis functions and the
series driver.  Every comparison is exact: selected values, integer counts and float64 edges."""

import contextlib
import ctypes
import io

import numpy as np
import pytest

import relsel_ref as rr
from opticalflow3d_dev_amd import (RelProfileSpec, SummarySpec, calc_flow3D, channel_compare, contractility,
                                   flow_summary, joint_reliability_mask, largest_component_mask,
                                   percentile_threshold_device, principal_axes, process_flow, quiver_sample,
                                   reliability_mask, reliability_profile, reliability_thresholds)
from opticalflow3d_dev_amd import _lib
from opticalflow3d_dev_amd import analysis as an
from opticalflow3d_dev_amd import tiff as tf

pytestmark = pytest.mark.gpu

SHAPE = (7, 37, 131)
PCTS = (0, 50, 85, 90, 95, 99.5, 100, 90)  # unsorted, a duplicate, the extremes
BOXES = [None,
         (4, 5, 20, 21, 77, 78),      # one voxel
         (4, 7, 30, 37, 100, 131),    # ends at the last voxel
         (0, 7, 0, 37, 33, 36),       # odd x origin, 3 voxels wide
         (0, 7, 0, 37, 130, 131)]     # one column
BIG_SHAPE, BIG_BOX = (9, 40, 300), (1, 9, 2, 39, 7, 290)  # 83768 voxels: several workgroups
SHAPE_2D, BOX_2D = (40, 44), (5, 25, 5, 30)
ROIS = [(4, 5, 20, 21, 77, 78), (4, 7, 30, 37, 100, 131), (0, 7, 0, 37, 33, 36), (1, 6, 5, 25, 10, 90),
        (0, 7, 2, 36, 5, 125)]  # one voxel, an end box, 3 wide, two overlapping, the last of several workgroups


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _select(a, ps, box, method):
    return reliability_thresholds(_cuda(a), ps, box=box, method=method).cpu().numpy()


def _volume(kind, shape, dtype):
    return rr.dataset(kind, int(np.prod(shape)), dtype).reshape(shape)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("method", ["linear", "hazen"])
def test_select_equals_numpy_on_the_crop(method, dtype):
    for kind in rr.KINDS:
        cases = [(_volume(kind, SHAPE, dtype), b) for b in BOXES]
        cases += [(_volume(kind, BIG_SHAPE, dtype), BIG_BOX), (_volume(kind, SHAPE_2D, dtype), BOX_2D)]
        for a, box in cases:
            got = _select(a, PCTS, box, method)
            want = rr.percentiles(a, box, PCTS, method)
            assert got.dtype == a.dtype and rr.same_values(got, want), (kind, box, got, want)
            assert got[3].tobytes() == got[7].tobytes()  # the duplicate


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_outside_of_the_box_is_never_counted(dtype):
    a = _volume("normal", SHAPE, dtype)
    for box in BOXES[1:]:
        want = rr.percentiles(a, box, PCTS, "hazen")
        inside = np.zeros(SHAPE, bool)
        inside[box[0]:box[1], box[2]:box[3], box[4]:box[5]] = True
        for poison in (np.nan, np.inf):
            b = np.where(inside, a, dtype(poison))
            assert rr.same_values(_select(b, PCTS, box, "hazen"), want), (box, poison)
        b = a.copy()
        b[box[1] - 1, box[3] - 1, box[5] - 1] = np.nan  # the box's last voxel
        assert np.all(np.isnan(_select(b, PCTS, box, "hazen"))), box
    b = a.copy()
    b[3, 11, 17] = np.nan
    assert np.all(np.isnan(_select(b, PCTS, None, "linear")))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_whole_volume_linear_is_the_flat_select(dtype):
    for kind in rr.KINDS:
        dev = _cuda(_volume(kind, SHAPE, dtype))
        for p in (0, 37.5, 90, 100):
            got = reliability_thresholds(dev, [p]).cpu().numpy()
            want = percentile_threshold_device(dev, p).cpu().numpy()
            assert got.tobytes() == want.tobytes() or (np.isnan(got[0]) and np.isnan(want[0])), (kind, p, got, want)


def test_the_same_call_twice_gives_the_same_bytes_and_out_is_used():
    import torch

    dev = _cuda(_volume("normal", BIG_SHAPE, np.float32))
    out = torch.empty(len(PCTS), dtype=dev.dtype, device=dev.device)
    first = reliability_thresholds(dev, PCTS, box=BIG_BOX, method="hazen", out=out)
    assert first is out
    a = out.cpu().numpy().tobytes()
    assert reliability_thresholds(dev, PCTS, box=BIG_BOX, method="hazen").cpu().numpy().tobytes() == a


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_views_off_a_16_byte_boundary(dtype):
    a = _volume("normal", SHAPE, dtype)
    n = a.size
    for off in (1, 3):
        buf = _cuda(np.concatenate([np.full(off, np.nan, dtype), a.ravel(), np.full(4, np.nan, dtype)]))
        view = buf[off:off + n].view(SHAPE)
        assert view.data_ptr() % 16 == (off * a.itemsize) % 16
        for box in (None, BOXES[2], BOXES[3]):
            got = reliability_thresholds(view, PCTS, box=box, method="hazen").cpu().numpy()
            assert rr.same_values(got, rr.percentiles(a, box, PCTS, "hazen")), (off, box)


def test_c_abi_refusals():
    import torch

    lib = _lib.load()
    rel = torch.zeros(SHAPE, dtype=torch.float32, device="cuda")
    out = torch.zeros(8, dtype=torch.float32, device="cuda")
    ws = torch.empty(lib.of3d_rel_select_workspace_bytes(0), dtype=torch.uint8, device="cuda")
    I, D = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
    n = int(np.prod(SHAPE))

    def call(n_q=1, lo=(0,), hi=(0,), gamma=(0.0,), box=None):
        arr = lambda v, t: np.array(v, dtype=t)
        lo, hi, gamma = arr(lo, np.int64), arr(hi, np.int64), arr(gamma, np.float64)
        b = arr(box, np.int64).ctypes.data_as(I) if box is not None else None
        rc = lib.of3d_rel_select(rel.data_ptr(), 0, *SHAPE, b, n_q, lo.ctypes.data_as(I), hi.ctypes.data_as(I),
                                 gamma.ctypes.data_as(D), out.data_ptr(), ws.data_ptr(), None)
        return rc, _lib.last_error()

    assert call()[0] == 0
    for n_q in (0, 9):
        rc, msg = call(n_q=n_q, lo=(0,) * 9, hi=(0,) * 9, gamma=(0.0,) * 9)
        assert rc < 0 and "1 to 8 percentiles" in msg
    for lo, hi, box in ((-1, 0, None), (2, 1, None), (0, n, None), (0, 3 * 4 * 5, (0, 3, 0, 4, 0, 5))):
        rc, msg = call(lo=(lo,), hi=(hi,), box=box)
        assert rc < 0 and "0 <= lo <= hi <= n_box-1" in msg, (lo, hi, msg)
    assert call(lo=(59,), hi=(59,), box=(0, 3, 0, 4, 0, 5))[0] == 0
    for box in ((2, 2, 0, 4, 0, 5), (0, 8, 0, 4, 0, 5), (0, 3, -1, 4, 0, 5), (0, 3, 0, 4, 0, 132)):
        rc, msg = call(box=box)
        assert rc < 0 and "ROI 0 is empty or outside the volume" in msg, (box, msg)
    rc, msg = call(gamma=(1.5,))
    assert rc < 0 and "gamma" in msg
    torch.cuda.synchronize()


# ---- profile --------------------------------------------------------------------------------------
def _check_profile(got, rel, rois, ps, method, box, edges):
    want_t = rr.percentiles(rel, box, list(ps) + [0, 100], method)
    assert rr.same_values(got["thresholds"], want_t[:-2])
    assert rr.same_values(np.array([got["min"], got["max"]]), want_t[-2:])
    assert got["edges"].dtype == np.float64 and np.array_equal(got["edges"], edges, equal_nan=True)
    ref = rr.profile(rel, rois, got["thresholds"], edges)
    for k in ("n_voxels", "n_nan", "n_above", "hist"):
        assert np.array_equal(got[k], ref[k]), (k, got[k], ref[k])
    assert got["hist"].dtype == np.uint64 and got["hist"].shape == (len(rois) + 1, len(edges) - 1)
    assert np.array_equal(got["fraction_above"], ref["n_above"] / ref["n_voxels"][:, None])
    return ref


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nbins", [1, 50, 256])
def test_profile_equals_numpy(nbins, dtype):
    rel = _volume("normal", SHAPE, dtype)
    rel[2, 3, 4] = np.nan  # in ROI 0 alone: counted, and dropped from the histogram
    box = (3, 5, 4, 20, 9, 60)  # a twentieth of the volume: the tails of the rest lie outside its range
    ps = (85, 90, 95)
    got = reliability_profile(rel, ps, box=box, method="hazen", rois=ROIS, bins=nbins)
    lo, hi = rr.percentiles(rel, box, [0, 100], "hazen")
    ref = _check_profile(got, rel, ROIS, ps, "hazen", box, np.linspace(float(lo), float(hi), nbins + 1))
    assert ref["n_nan"].tolist() == [1, 0, 0, 0, 0, 0] and ref["hist"][0].sum() < rel.size - 1  # some fall outside
    # 2D, the whole field, numpy input and resident tensor alike
    rel2 = _volume("five_levels", SHAPE_2D, dtype)
    got2 = reliability_profile(rel2, (50,), rois=[BOX_2D, (7, 8, 9, 10)], bins=nbins)
    _check_profile(got2, rel2, [BOX_2D, (7, 8, 9, 10)], (50,), "linear", None, np.linspace(-1.0, 1.0, nbins + 1))
    dev = reliability_profile(_cuda(rel2), (50,), rois=[BOX_2D, (7, 8, 9, 10)], bins=nbins)
    assert all(np.array_equal(got2[k], dev[k]) for k in ("hist", "n_above", "edges", "thresholds"))


def test_profile_values_on_the_edges_float64():
    """Values exactly on lo, on hi and on an interior edge: half-open bins, the last one closed."""
    rng = np.random.default_rng(5)
    rel = rng.uniform(1.0, 3.0, SHAPE)
    edges = np.linspace(1.0, 3.0, 9)  # exact in binary
    assert edges[3] == 1.75
    rel[0, 0, 0:3] = 1.0
    rel[6, 36, 128:131] = 3.0
    rel[3, 10, 33:36] = 1.75
    rel[4, 20, 77] = 1.75
    got = reliability_profile(rel, (90,), rois=ROIS, bins=8)
    ref = _check_profile(got, rel, ROIS, (90,), "linear", None, edges)
    assert ref["hist"][1].tolist() == [0, 0, 0, 1, 0, 0, 0, 0] and ref["hist"][0].sum() == rel.size


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_profile_constant_and_infinite(dtype):
    rel = np.full(SHAPE, 1.25, dtype)
    got = reliability_profile(rel, (85, 95), rois=ROIS[:2], bins=4)
    ref = _check_profile(got, rel, ROIS[:2], (85, 95), "linear", None, np.linspace(0.75, 1.75, 5))
    assert ref["hist"][0].tolist() == [0, 0, rel.size, 0] and not got["n_above"].any()
    rel = _volume("normal", SHAPE, dtype)
    rel[1, 2, 3] = np.inf
    got = reliability_profile(rel, (50,), rois=ROIS[:2], bins=4)
    assert np.all(np.isnan(got["edges"])) and not got["hist"].any() and np.isnan(got["max"])  # inf - inf in _lerp
    assert np.array_equal(got["n_above"], rr.profile(rel, ROIS[:2], got["thresholds"], got["edges"])["n_above"])


def test_profile_given_edges_and_box_independence():
    rel = _volume("normal", SHAPE, np.float32)
    edges = np.array([-1.0, -0.25, 0.0, float(rel[4, 20, 77]), 2.0])
    edges = np.unique(edges)
    got = reliability_profile(rel, (85, 90, 95), rois=ROIS, edges=edges)
    ref = _check_profile(got, rel, ROIS, (85, 90, 95), "linear", None, edges)
    assert ref["hist"][0].sum() < rel.size  # values outside the given edges are dropped
    for r in (1, 4):  # a box's words do not depend on the other boxes
        alone = reliability_profile(rel, (85, 90, 95), rois=[ROIS[r - 1]], edges=edges)
        for k in ("n_voxels", "n_nan", "n_above", "hist"):
            assert alone[k][1].tobytes() == got[k][r].tobytes(), (r, k)
    again = reliability_profile(rel, (85, 90, 95), rois=ROIS, edges=edges)
    assert all(again[k].tobytes() == got[k].tobytes() for k in ("n_above", "hist", "edges", "thresholds"))


# ---- wiring ---------------------------------------------------------------------------------------
PBOX = (1, 7, 3, 20, 5, 30)
WROIS = [(2, 3, 5, 6, 7, 8), (1, 7, 3, 20, 5, 8), (4, 8, 10, 24, 21, 40)]


@pytest.fixture(scope="module")
def series():
    stack = np.random.default_rng(21).integers(0, 4096, size=(9, 8, 24, 40)).astype(np.uint16)
    fields = [np.ascontiguousarray(a) for a in calc_flow3D(stack[0:7], 1, 1, 2)]
    other = [np.ascontiguousarray(a) for a in calc_flow3D(stack[1:8], 1, 1, 2)]
    return stack, fields, other


def _crop_threshold(rel, p):
    return rr.percentiles(rel, PBOX, [p], "hazen")[0]


def test_functions_with_a_box_equal_the_given_threshold(series):
    _, f, g = series
    rel = f[3]
    t = _crop_threshold(rel, 80)
    assert t != np.percentile(rel, 80)  # the crop and the definition matter here
    kw = dict(percentile_box=PBOX, percentile_method="hazen")

    def same(a, b, keys):
        for k in keys:
            x, y = a[k], b[k]
            assert np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True), k

    counts = ("n_mask", "n_components", "n_components_kept", "n_kept")
    a = reliability_mask(rel, 80, min_size=3, rois=WROIS, **kw)
    b = reliability_mask(rel, 80, threshold=float(t), min_size=3, rois=WROIS)
    assert a["threshold"].tobytes() == t.tobytes()
    same(a, b, ("keep", "threshold") + counts)
    a = principal_axes(rel, 80, rois=WROIS, **kw)
    b = principal_axes(rel, 80, threshold=float(t), rois=WROIS)
    same(a, b, ("threshold", "moments", "centroid", "covariance", "axis_values", "axis_vectors"))
    a = quiver_sample(*f, 80, gap=1, rois=WROIS, **kw)
    b = quiver_sample(*f, 80, gap=1, rois=WROIS, threshold=float(t))
    assert a["threshold"].tobytes() == t.tobytes()
    for sa, sb in zip(a["samples"], b["samples"]):
        same(sa, sb, ("zyx", "v", "n_valid"))
    a = largest_component_mask(rel, 80, rois=WROIS, **kw)
    b = largest_component_mask(rel, 80, threshold=float(t), rois=WROIS)
    same(a, b, ("keep", "threshold", "n_mask", "n_kept"))
    # no threshold= on these three: their threshold is numpy's of the crop, and their masks are
    # those of the functions above at that threshold
    s = flow_summary(*f, 80, rois=WROIS, min_size=3, **kw)
    assert s["threshold"].tobytes() == t.tobytes()
    same(s, reliability_mask(rel, 80, threshold=float(t), min_size=3, rois=WROIS), counts)
    s1 = flow_summary(*f, 80, rois=WROIS, **kw)
    assert np.array_equal(s1["n_valid"], [x["n_valid"] for x in quiver_sample(*f, 80, gap=1, rois=WROIS,
                                                                           threshold=float(t))["samples"]])
    c = contractility(*f, 80, rois=WROIS, **kw)
    assert c["threshold"].tobytes() == t.tobytes()
    same(c, b, ("n_mask", "n_kept"))
    t1 = _crop_threshold(g[3], 80)
    j = joint_reliability_mask(rel, g[3], 80, min_size=2, rois=WROIS, **kw)
    jt = joint_reliability_mask(rel, g[3], 80, thresholds=[float(t), float(t1)], min_size=2, rois=WROIS)
    assert j["thresholds"].tobytes() == np.array([t, t1]).tobytes()
    same(j, jt, ("keep",) + counts)
    cc = channel_compare(f, g, 80, min_size=2, rois=WROIS, **kw)
    assert cc["thresholds"].tobytes() == np.array([t, t1]).tobytes()
    same(cc, jt, counts)


def test_summary_with_a_profile_equals_the_single_calls(series):
    _, f, _ = series
    prof = RelProfileSpec(percentiles=(70, 80, 95), bins=20)
    s = flow_summary(*f, 80, rois=WROIS, percentile_box=PBOX, percentile_method="hazen", rel_profile=prof)
    plain = flow_summary(*f, 80, rois=WROIS, percentile_box=PBOX, percentile_method="hazen")
    assert s["threshold"].tobytes() == _crop_threshold(f[3], 80).tobytes() == plain["threshold"].tobytes()
    for k in ("n_valid",) + an.SUMS:
        assert np.array_equal(s[k], plain[k], equal_nan=True), k
    p = reliability_profile(f[3], (70, 80, 95), box=PBOX, method="hazen", rois=WROIS, bins=20)
    for k in p:
        assert np.asarray(s["rel_profile"][k]).tobytes() == np.asarray(p[k]).tobytes(), k
    lo, hi = rr.percentiles(f[3], PBOX, [0, 100], "hazen")
    _check_profile(p, f[3], WROIS, (70, 80, 95), "hazen", PBOX, np.linspace(float(lo), float(hi), 21))
    # the summary's own percentile outside the profile's: one more rank in the same select
    s2 = flow_summary(*f, 60, rois=WROIS, percentile_box=PBOX, percentile_method="hazen", rel_profile=prof)
    assert s2["threshold"].tobytes() == _crop_threshold(f[3], 60).tobytes()
    assert all(np.asarray(s2["rel_profile"][k]).tobytes() == np.asarray(p[k]).tobytes() for k in p)
    # without the new options: the flat select, as before
    assert flow_summary(*f, 80)["threshold"] == np.percentile(f[3], 80)


def test_series_driver_writes_the_profile(series, tmp_path):
    stack, _, _ = series
    spec = SummarySpec(rois=WROIS, rel_percentile=80, xyscale=0.1, zscale=0.3, tscale=2.0, percentile_box=PBOX,
                       percentile_method="hazen", rel_profile=RelProfileSpec(percentiles=(70, 80, 95), bins=20))
    tf.imwrite(tmp_path / "cells.tif", stack, imagej=True)
    with contextlib.redirect_stdout(io.StringIO()):
        process_flow(str(tmp_path), "cells", "OneTif", 3, 1, 1, 2, summary=spec, save_fields=False)
    out = tmp_path / "OpticalFlow3D" / "cells"
    csv, npz = an.read_summary_csv(out / "cells_summary.csv"), np.load(out / "cells_summary_hist.npz")
    n_roi = len(WROIS) + 1
    assert npz["counts_rel"].shape == (3, n_roi, 20) and npz["edges_rel"].shape == (3, 21)
    for i in range(3):
        f = calc_flow3D(stack[i:i + 7], 1, 1, 2)
        s = flow_summary(*f, 80, 0.1, 0.3, 2.0, rois=WROIS, percentile_box=PBOX, percentile_method="hazen",
                         rel_profile=spec.rel_profile)
        p = reliability_profile(np.ascontiguousarray(f[3]), (70, 80, 95), box=PBOX, method="hazen", rois=WROIS,
                                bins=20)
        rows = slice(n_roi * i, n_roi * (i + 1))
        assert np.all(csv["threshold"][rows] == np.float64(_crop_threshold(f[3], 80)))
        assert np.array_equal(csv["n_valid"][rows], s["n_valid"])
        assert np.all(csv["rel_min"][rows] == np.float64(p["min"])) and np.all(csv["rel_max"][rows] == np.float64(p["max"]))
        assert np.array_equal(csv["rel_n_nan"][rows], p["n_nan"])
        for k, name in enumerate(("70", "80", "95")):
            assert np.all(csv["rel_p" + name][rows] == np.float64(p["thresholds"][k]))
            assert np.array_equal(csv["n_above_p" + name][rows], p["n_above"][:, k])
        assert np.array_equal(npz["counts_rel"][i], p["hist"]) and np.array_equal(npz["edges_rel"][i], p["edges"])
