"""The device analysis under a poisoned allocator: no pass may rely on what torch.empty returns.

analysis.py and stream.py allocate every workspace, threshold, count and result buffer with
torch.empty; the caching allocator usually hands back zeros or an earlier call's (correct)
words.  Here torch.empty returns 0xFF bytes on the device (poison.poisoned_empty) for one
representative call of every public analysis function, at the small shapes the functions' own
GPU tests use (3D with two ROIs beside the whole volume, and one 2D call each).  For each call:

  * the decoded result passes the reference check of the function's own test (summary_ref,
    mask_ref, axes_ref, whist_ref, spread_ref, relsel_ref, pair_ref, quiver_ref, contract_ref,
    through those tests' check helpers: no new tolerance);
  * it equals, bit for bit, the same call made without the poisoned allocator (the headers
    promise equal bits for equal inputs; only what the decoders return is compared, so not a
    quiver block's words past n_stored);
  * the wrapper poisoned at least one device allocation during the call."""
import numpy as np
import pytest

import contract_ref as cr
import mask_ref as mr
import pair_ref as pr
import poison
import quiver_ref as qr
import relsel_ref as rr
import spread_ref as spr
import summary_ref as sr
import whist_ref as wr
from opticalflow3d_dev_amd import (ContractSpec, RelProfileSpec, calc_flow2D, calc_flow3D, channel_compare,
                                   contractility, flow_summary, joint_reliability_mask, largest_component_mask,
                                   principal_axes, quiver_sample, reliability_profile, reliability_thresholds)
from opticalflow3d_dev_amd.analysis import flow_statistics
from oracle import cpu_ref

import test_gpu_analysis as t_stats
import test_gpu_axes as t_axes
import test_gpu_contract as t_contract
import test_gpu_mask_open as t_open
import test_gpu_pair as t_pair
import test_gpu_quiver as t_quiver
import test_gpu_relsel as t_relsel
import test_gpu_spread as t_spread
import test_gpu_summary_mask as t_smask
import test_gpu_whist as t_whist

pytestmark = pytest.mark.gpu


def assert_same_bits(a, b, path="result"):
    """Two decoded results, bit for bit: dicts by key, sequences by item, tensors and arrays by
    dtype, shape and bytes (NaN payloads included); the mask accessors (callables) are views of
    `keep`, which is compared."""
    import torch

    if isinstance(a, dict):
        assert isinstance(b, dict) and sorted(map(str, a)) == sorted(map(str, b)), (path, sorted(a), sorted(b))
        for k in a:
            assert_same_bits(a[k], b[k], f"{path}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert type(a) is type(b) and len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            assert_same_bits(x, y, f"{path}[{i}]")
    elif callable(a) and not isinstance(a, (np.generic, np.ndarray)):
        assert callable(b), path
    else:
        if isinstance(a, torch.Tensor):
            assert isinstance(b, torch.Tensor) and a.device == b.device, path
            a, b = a.cpu().numpy(), b.cpu().numpy()
        x, y = np.asarray(a), np.asarray(b)
        assert x.dtype == y.dtype and x.shape == y.shape, (path, x.dtype, y.dtype, x.shape, y.shape)
        assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), f"{path} differs"


def both(call, monkeypatch):
    """call() without and with the poisoned allocator: equal bits; returns the poisoned result."""
    plain = call()
    with poison.poisoned_empty(monkeypatch) as counter:
        hostile = call()
    assert counter.device_allocations >= 1, "the wrapper poisoned nothing: torch.empty is no longer what allocates"
    assert_same_bits(hostile, plain)
    return hostile


# ---- flow_summary and its options --------------------------------------------------------------------
@pytest.fixture(scope="module")
def smooth3():
    shape = (24, 40, 72)
    return [t_smask.smooth(40 + i, shape) for i in range(3)] + [t_smask.smooth(43, shape, np.float32)]


def test_flow_summary_plain(smooth3, monkeypatch):
    kw = dict(rois=t_smask.ROIS3, bins=t_smask.BINS)
    got = both(lambda: flow_summary(*smooth3, 80, **t_smask.SCALES, **kw), monkeypatch)
    ref = sr.summary_ref(*smooth3, 80, *t_smask.SCALES.values(), **kw)
    assert np.all(ref["n_valid"] > 1000)
    sr.assert_clear_of_edges(ref, ("theta", "phi"))
    sr.assert_matches(got, ref, list(t_smask.BINS))


def test_flow_summary_2d(monkeypatch):
    img = np.random.default_rng(4).integers(0, 4096, size=(7, 40, 44)).astype(np.uint16)
    vx, vy, rel = (np.ascontiguousarray(a) for a in calc_flow2D(img, 1, 1, 2))
    bins = {"magnitude": [0.0, 0.01, 0.1, 1.0, 1e3]}
    rois = [(5, 25, 5, 30), (15, 35, 20, 44)]
    got = both(lambda: flow_summary(vx, vy, None, rel, 50, 0.065, 0.2, 0.75, rois=rois, bins=bins), monkeypatch)
    ref = sr.summary_ref(vx, vy, None, rel, 50, 0.065, 0.2, 0.75, rois=rois, bins=bins)
    assert np.all(ref["n_valid"] > 0)
    sr.assert_matches(got, ref, ("magnitude",))


def test_flow_summary_min_size(smooth3, monkeypatch):
    vx, vy, vz, rel = smooth3
    call = lambda: t_smask.check_against_ref(vx, vy, vz, rel, t_smask.ROIS3, t_smask.BINS, 10, 26)[0]
    got = both(call, monkeypatch)  # (the helper checks against mask_ref inside, both times)
    assert np.all(got["n_components"] > got["n_components_kept"]) and np.all(got["n_valid"] > 0)


def test_flow_summary_min_size_2d(monkeypatch):
    shape = (40, 72)
    vx, vy, rel = t_smask.smooth(50, shape), t_smask.smooth(51, shape), t_smask.smooth(52, shape)
    bins = {k: t_smask.BINS[k] for k in ("vx", "magnitude", "theta")}
    both(lambda: t_smask.check_against_ref(vx, vy, None, rel, [(3, 35, 5, 65), (11, 40, 33, 72)], bins, 6, 8)[0],
         monkeypatch)


AXES_ROIS = [t_axes.ROI3, (2, 9, 0, 23, 20, 70)]  # overlapping


def test_flow_summary_axes_mask(monkeypatch):
    rel, vx, vy, vz = t_axes.ar.blob(t_axes.SHAPE3, 7), *[t_axes.smooth(70 + i, t_axes.SHAPE3) for i in range(3)]
    bins = {"axis1": t_axes.axis_bins_for(0.004, 14), "axis2": t_axes.axis_bins_for(0.003, 14),
            "axis3": t_axes.axis_bins_for(0.01, 256)}
    got = both(lambda: t_axes.check_projection(vx, vy, vz, rel.astype(np.float32), AXES_ROIS, 50, 6, bins), monkeypatch)
    assert np.all(got["axes_used"] == got["axis_vectors"])


def test_flow_summary_axes_mask_2d(monkeypatch):
    rel, vx, vy = t_axes.ar.blob(t_axes.SHAPE2, 7), t_axes.smooth(80, t_axes.SHAPE2), t_axes.smooth(81, t_axes.SHAPE2)
    bins = {"axis1": t_axes.axis_bins_for(0.004, 256), "axis2": t_axes.axis_bins_for(0.003, 14)}
    both(lambda: t_axes.check_projection(vx, vy, None, rel.astype(np.float32), [t_axes.ROI2], 6, 8, bins), monkeypatch)


def test_flow_summary_weighted_bins(monkeypatch):
    f = wr.exact_case()
    ref = wr.whist_ref(*f, 50, rois=wr.EXACT_ROIS, weighted_bins=wr.EXACT_BINS)
    assert ref["n_valid"].tolist() == [4221, 2083, 53]
    got = both(lambda: flow_summary(*f, 50, rois=wr.EXACT_ROIS, weighted_bins=wr.EXACT_BINS), monkeypatch)
    t_whist.assert_bitwise(got, ref, ("phi", "theta", "magnitude"))
    for k in wr.EXACT_BINS:
        assert got["hist_weighted"][k].sum(axis=1).tobytes() == got["sum_magnitude"].tobytes(), k


EXACT2D_ROIS = [(3, 25, 5, 40), (10, 30, 20, 45)]  # overlapping


def _exact2d():
    """test_gpu_whist's exact 2D frame: vx, vy from the triples, None, a random float64 rel."""
    rng = np.random.default_rng(9)
    vx, vy = wr.exact_fields((33, 45), rng, ndim=2)
    return [vx, vy, None, rng.random((33, 45))]


def test_flow_summary_weighted_bins_2d(monkeypatch):
    f, rois = _exact2d(), EXACT2D_ROIS
    bins = {"theta": np.linspace(-np.pi, np.pi, 11) + 0.01, "magnitude": np.array([0.0, 4.0, 16.0, 128.0])}
    ref = wr.whist_ref(*f, 50, rois=rois, weighted_bins=bins)
    assert np.all(ref["n_valid"] > 100)
    sr.assert_clear_of_edges(wr.with_bins(ref, bins), ("theta",))
    got = both(lambda: flow_summary(*f, 50, rois=rois, weighted_bins=bins), monkeypatch)
    t_whist.assert_bitwise(got, ref, ("theta", "magnitude"))


def test_flow_summary_spread_mean(monkeypatch):
    """spread="mean" on the exact fields: the centre is the call's own sum / n, and the sums about
    it are within spread_ref's bound (test_gpu_spread.test_general_case_within_the_sum_bound's
    checks); the extremes bit for bit."""
    f = wr.exact_case()
    ref = sr.summary_ref(*f, 50, rois=wr.EXACT_ROIS)
    got = both(lambda: flow_summary(*f, 50, rois=wr.EXACT_ROIS, spread="mean"), monkeypatch)
    assert np.array_equal(got["n_valid"], ref["n_valid"]) and ref["n_valid"].tolist() == [4221, 2083, 53]
    nv = got["n_valid"].astype(np.float64)
    want = np.stack([got["sum_" + k] / nv for k in spr.COMPONENTS], axis=1)
    assert got["spread_center"].tobytes() == want.tobytes()
    sref = spr.spread_ref(ref, got["spread_center"])
    for k in spr.SUMS:
        err, bound = np.abs(got[k] - sref[k]), spr.sum_bound(sref, k)
        assert np.all(err <= bound), (k, err, bound)
    t_spread.assert_bitwise(got, sref, [f"{m}_{k}" for m in ("min", "max") for k in spr.COMPONENTS])


def test_flow_summary_spread_mean_2d(monkeypatch):
    f, rois = _exact2d(), EXACT2D_ROIS
    ref = sr.summary_ref(*f, 50, rois=rois)
    got = both(lambda: flow_summary(*f, 50, rois=rois, spread="mean"), monkeypatch)
    assert np.array_equal(got["n_valid"], ref["n_valid"]) and np.all(ref["n_valid"] > 0)
    sref = spr.spread_ref(ref, got["spread_center"])
    for k in spr.SUMS:
        assert np.all(np.abs(got[k] - sref[k]) <= spr.sum_bound(sref, k)), k


@pytest.fixture(scope="module")
def flow3():
    stack = np.random.default_rng(21).integers(0, 4096, size=(9, 8, 24, 40)).astype(np.uint16)
    return [np.ascontiguousarray(a) for a in calc_flow3D(stack[0:7], 1, 1, 2)]


def test_flow_summary_rel_profile(flow3, monkeypatch):
    prof = RelProfileSpec(percentiles=(70, 80, 95), bins=20)
    kw = dict(rois=t_relsel.WROIS, percentile_box=t_relsel.PBOX, percentile_method="hazen")
    got = both(lambda: flow_summary(*flow3, 80, rel_profile=prof, **kw), monkeypatch)
    assert got["threshold"].tobytes() == t_relsel._crop_threshold(flow3[3], 80).tobytes()
    lo, hi = rr.percentiles(flow3[3], t_relsel.PBOX, [0, 100], "hazen")
    t_relsel._check_profile(got["rel_profile"], flow3[3], t_relsel.WROIS, (70, 80, 95), "hazen", t_relsel.PBOX,
                            np.linspace(float(lo), float(hi), 21))
    plain = flow_summary(*flow3, 80, **kw)
    for k in ("n_valid", "sum_vx", "sum_magnitude"):
        assert np.array_equal(got[k], plain[k], equal_nan=True), k


# ---- masks ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,min_size,conn", [((24, 40, 72), 10, 26), ((37, 131), 5, 8)])
def test_reliability_mask(shape, min_size, conn, monkeypatch):
    from scipy import ndimage

    rel = ndimage.gaussian_filter(np.random.default_rng(3).standard_normal(shape), 1.5).astype(np.float32)
    call = lambda: t_open.check(rel, min_size, conn, t_open.rois_for(shape), rel_percentile=80)[0]
    got = both(call, monkeypatch)
    assert np.all(got["n_components"] > got["n_components_kept"]) and np.all(got["n_kept"] > 0)


@pytest.mark.parametrize("ndim", [3, 2])
def test_largest_component_mask(ndim, monkeypatch):
    rel, boxes, thresh = cr.label_masks()["smooth"] if ndim == 3 else cr.label_masks_2d()["random2d"]
    conn = 18 if ndim == 3 else 8
    keep, counts = cr.largest_ref(rel, thresh, boxes, conn)
    rois = t_contract._rois(boxes, ndim)
    got = both(lambda: largest_component_mask(rel, threshold=thresh, connectivity=conn, rois=rois), monkeypatch)
    assert got["keep"].dtype == np.uint16 and np.array_equal(got["keep"], keep)
    for k in mr.COUNTS:
        assert np.array_equal(got[k], counts[k]), (k, got[k], counts[k])
    assert counts["n_components"][0] > 1


def test_principal_axes(monkeypatch):
    rel = t_axes.ar.blob(t_axes.SHAPE3, 7).astype(np.float32)
    boxes, thresh, masks = t_axes.ref_masks(rel, AXES_ROIS, 50, 6)
    got = both(lambda: principal_axes(rel, t_axes.PCT, min_size=50, connectivity=6, rois=AXES_ROIS), monkeypatch)
    assert got["threshold"] == thresh and np.array_equal(got["rois"], boxes)
    t_axes.check_mask_part(got, boxes, masks)
    assert got["n_components"][0] > got["n_components_kept"][0]  # the opening removed something


def test_principal_axes_2d(monkeypatch):
    rel = t_axes.ar.blob(t_axes.SHAPE2, 7).astype(np.float32)
    boxes, _, masks = t_axes.ref_masks(rel, [t_axes.ROI2], 0, None)
    got = both(lambda: principal_axes(rel, t_axes.PCT, rois=[t_axes.ROI2]), monkeypatch)
    t_axes.check_mask_part(got, boxes, masks)


# ---- two channels --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def general():
    return pr.general_case()


def test_joint_reliability_mask(general, monkeypatch):
    rel0, rel1 = general[0][3], general[1][3]
    rois = [(0, 4, 2, 30, 3, 50), (1, 5, 10, 37, 30, 67)]  # overlapping
    kw = dict(rel_percentile=80, connectivity=6, min_size=5)
    ref = t_pair._open_ref(rel0, rel1, rois, **kw)
    assert np.all(ref[3]["n_components"] > ref[3]["n_components_kept"]) and np.all(ref[3]["n_kept"] > 0)
    t_pair._assert_opening(both(lambda: joint_reliability_mask(rel0, rel1, rois=rois, **kw), monkeypatch), *ref)


def test_joint_reliability_mask_2d(general, monkeypatch):
    rel0, rel1 = general[0][3][2], general[1][3][2]
    kw = dict(rel_percentile=75, connectivity=8, min_size=4)
    ref = t_pair._open_ref(rel0, rel1, [(1, 36, 3, 64)], **kw)
    t_pair._assert_opening(both(lambda: joint_reliability_mask(rel0, rel1, rois=[(1, 36, 3, 64)], **kw), monkeypatch),
                           *ref)


def test_channel_compare(general, monkeypatch):
    ch0, ch1 = general
    rois = [(0, 4, 2, 30, 3, 50), (1, 5, 10, 37, 30, 67)]
    ref, t, counts = t_pair._pair_ref(ch0, ch1, rois, pr.G_SCALES, pr.G_BINS, **t_pair.SETTINGS["sparse"])
    assert np.all(ref["n_valid"] > 500)
    got = both(lambda: channel_compare(ch0, ch1, 80, *pr.G_SCALES, rois=rois, bins=pr.G_BINS, min_size=5,
                                       connectivity=6), monkeypatch)
    t_pair._assert_pair(got, ref, t, counts)


def test_channel_compare_2d(general, monkeypatch):
    ch0, ch1 = ((c[0][1], c[1][1], None, c[3][1]) for c in general)
    rois = [(1, 36, 3, 64), (5, 6, 0, 67)]
    ref, t, counts = t_pair._pair_ref(ch0, ch1, rois, pr.G_SCALES, pr.G_BINS, rel_percentile=60, connectivity=4,
                                      min_size=3)
    got = both(lambda: channel_compare(ch0, ch1, 60, *pr.G_SCALES, rois=rois, bins=pr.G_BINS, min_size=3,
                                       connectivity=4), monkeypatch)
    t_pair._assert_pair(got, ref, t, counts)


# ---- quiver, contractility ----------------------------------------------------------------------------
def test_quiver_sample_truncated(monkeypatch):
    """A capacity below n_valid: the blocks hold the first records; the words past n_stored of the
    short third block are not part of the result (the decoder returns n_stored records)."""
    f = qr.planted_fields(t_quiver.T_SHAPE, 29)
    kw = dict(**t_quiver.SCALES, gap=t_quiver.T_GAP, rois=t_quiver.T_ROIS)
    ref = qr.quiver_ref(*f, 60, **kw)
    cap = 700
    n_valid = [s["n_valid"] for s in ref["samples"]]
    assert n_valid[0] > cap and n_valid[1] > cap and n_valid[2] < 100
    got = both(lambda: quiver_sample(*f, 60, max_vectors=cap, **kw), monkeypatch)
    t_quiver.assert_same(got, ref, capacity=[cap, cap, 100])
    assert [s["truncated"] for s in got["samples"]] == [True, True, False]


def test_quiver_sample_opened_overlapping_rois(monkeypatch):
    from scipy import ndimage

    shape = (8, 30, 70)
    rel = ndimage.gaussian_filter(np.random.default_rng(31).standard_normal(shape), 1.5).astype(np.float32)
    vx, vy, vz = qr.planted_fields(shape, 32)[:3]
    boxes, thresh = mr.boxes_of(shape, t_quiver.M_ROIS), np.percentile(rel, 80)
    keep, _ = mr.open_ref(rel, thresh, boxes, 20, 18)
    kw = dict(**t_quiver.SCALES, gap=(1, 1, 2), rois=t_quiver.M_ROIS)
    ref = qr.quiver_ref(vx, vy, vz, rel, 80, keep=keep, **kw)
    t_quiver.assert_not_vacuous(ref)
    got = both(lambda: quiver_sample(vx, vy, vz, rel, 80, min_size=20, connectivity=18, **kw), monkeypatch)
    t_quiver.assert_same(got, ref)


def test_quiver_sample_2d(monkeypatch):
    f = qr.planted_fields((33, 45), 24, rel_dtype=np.float64)
    kw = dict(xyscale=0.3, tscale=0.5, gap=(2, 3), rois=[(3, 25, 2, 17), (32, 33, 0, 45)])
    ref = qr.quiver_ref(*f, 50, **kw)
    t_quiver.assert_not_vacuous(ref)
    t_quiver.assert_same(both(lambda: quiver_sample(*f, 50, **kw), monkeypatch), ref)


@pytest.mark.parametrize("name", ["general3d", "general2d"])
def test_contractility(name, monkeypatch):
    f, rois, per = cr.general3d() if name == "general3d" else cr.general2d()
    boxes = cr.boxes_of(np.shape(f[0]), rois)
    keep, counts, thresh = cr.mask_of(f[3], per, boxes, "largest")
    ref = cr.contract_ref(*f[:3], keep, boxes, **cr.SCALES, bins=cr.BINS)
    assert np.all(ref["n_angle"] > 100)
    got = both(lambda: contractility(*f, per, **cr.SCALES, rois=rois, spec=ContractSpec(mask="largest", bins=cr.BINS)),
               monkeypatch)
    assert got["threshold"] == thresh
    t_contract._assert_matches(got, ref, counts)


# ---- thresholds and the profile -------------------------------------------------------------------------
@pytest.mark.parametrize("shape,box", [(t_relsel.BIG_SHAPE, t_relsel.BIG_BOX), (t_relsel.SHAPE_2D, t_relsel.BOX_2D)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_reliability_thresholds(shape, box, dtype, monkeypatch):
    a = t_relsel._volume("normal", shape, dtype)
    dev = t_relsel._cuda(a)
    got = both(lambda: reliability_thresholds(dev, t_relsel.PCTS, box=box, method="hazen"), monkeypatch).cpu().numpy()
    want = rr.percentiles(a, box, t_relsel.PCTS, "hazen")
    assert got.dtype == a.dtype and rr.same_values(got, want), (got, want)


def test_reliability_profile(monkeypatch):
    rel = t_relsel._volume("normal", t_relsel.SHAPE, np.float32)
    rel[2, 3, 4] = np.nan
    box, ps = (3, 5, 4, 20, 9, 60), (85, 90, 95)
    got = both(lambda: reliability_profile(rel, ps, box=box, method="hazen", rois=t_relsel.ROIS, bins=50), monkeypatch)
    lo, hi = rr.percentiles(rel, box, [0, 100], "hazen")
    ref = t_relsel._check_profile(got, rel, t_relsel.ROIS, ps, "hazen", box, np.linspace(float(lo), float(hi), 51))
    assert ref["n_nan"].tolist() == [1, 0, 0, 0, 0, 0]


def test_reliability_profile_2d(monkeypatch):
    rel2 = t_relsel._volume("five_levels", t_relsel.SHAPE_2D, np.float64)
    rois = [t_relsel.BOX_2D, (7, 8, 9, 10)]
    got = both(lambda: reliability_profile(rel2, (50,), rois=rois, bins=50), monkeypatch)
    t_relsel._check_profile(got, rel2, rois, (50,), "linear", None, np.linspace(-1.0, 1.0, 51))


# ---- the one-shot statistics and the streaming driver ---------------------------------------------------
def test_flow_statistics(monkeypatch):
    img = np.random.default_rng(3).integers(0, 4096, size=(7, 8, 30, 34)).astype(np.uint16)
    vx, vy, vz, rel = calc_flow3D(img, 1, 1, 2)
    vx[0, 0, :3] = 0.0
    ref = cpu_ref.analysis_reference(vx.copy(), vy.copy(), vz.copy(), rel, 90, 0.065, 0.2, 0.75)
    got = both(lambda: flow_statistics(vx, vy, vz, rel, 90, 0.065, 0.2, 0.75), monkeypatch)
    assert got["threshold"] == ref["threshold"] and got["threshold"].dtype == ref["threshold"].dtype
    for k in ("vx", "vy", "vz", "magnitude"):
        assert got[k].tobytes() == ref[k].tobytes(), k
    for k in ("theta", "phi"):
        same_nan, u = t_stats._ulps(got[k], ref[k])
        assert same_nan and u <= 4, (k, u)


def test_flow_statistics_2d(monkeypatch):
    img = np.random.default_rng(4).integers(0, 4096, size=(7, 40, 44)).astype(np.uint16)
    vx, vy, rel = calc_flow2D(img, 1, 1, 2)
    ref = cpu_ref.analysis_reference(vx.copy(), vy.copy(), None, rel, 90)
    got = both(lambda: flow_statistics(vx, vy, None, rel, 90), monkeypatch)
    assert got["threshold"] == ref["threshold"] and "phi" not in got
    for k in ("vx", "vy", "magnitude"):
        assert np.asarray(got[k]).tobytes() == ref[k].tobytes(), k


def test_flowstream_summary_without_fields(monkeypatch):
    """One short FlowStream run with summary= and fields=False, the stream built and run under the
    poisoned allocator (its slots, outputs and summary buffers are torch.empty): every window's
    summary equals flow_summary of calc_flow3D's outputs bit for bit, as test_flowstream_summary
    has it, and the unpoisoned stream's."""
    from opticalflow3d_dev_amd.stream import FlowStream

    series = np.random.default_rng(61).integers(0, 4096, size=(9, 6, 16, 20)).astype(np.uint16)
    per_frame = [flow_summary(*calc_flow3D(series[i:i + 7], 1, 1, 2), 70, rois=t_smask.D_ROIS, bins=t_smask.D_BINS,
                              min_size=20, connectivity=18, **t_smask.SCALES) for i in range(3)]
    assert per_frame[0]["n_components"][0] > per_frame[0]["n_components_kept"][0] > 0

    def run():
        fs = FlowStream(3, series.shape[1:], series.dtype, 1, 1, 2, summary=t_smask.D_SPEC, fields=False)
        try:
            out, pushed = [], 0
            for i in range(3):
                while pushed < min(i + 7 + fs.lookahead, len(series)):
                    fs.push(series[pushed])
                    pushed += 1
                p = fs.submit()
                out.append(p.summary())
                p.release()
            return out
        finally:
            fs.close()

    got = both(run, monkeypatch)
    for s, want in zip(got, per_frame):
        t_smask.same_summary(s, want)
