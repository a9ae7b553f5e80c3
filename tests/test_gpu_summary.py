"""Device-side frame summaries (csrc/kt_summary.hip): of3d_quantile against np.percentile,
analysis.flow_summary against the numpy restatement tests/summary_ref.py, determinism."""
import warnings

import numpy as np
import pytest

import summary_ref as sr
from opticalflow3d_dev_amd import (SummarySpec, calc_flow2D, calc_flow3D, calc_flow3D_fp32, flow_summary,
                                   percentile_threshold_device)
from opticalflow3d_dev_amd.analysis import _SummaryCall

pytestmark = pytest.mark.gpu

NS = (1, 2, 257, 100003)
PCTS = (0, 50, 90, 99.5, 100)


def _dataset(kind, n, dtype):
    rng = np.random.default_rng(1000 + n)
    dt = np.dtype(dtype)
    if kind == "normal":
        return rng.standard_normal(n).astype(dt)
    if kind == "equal":
        return np.full(n, 1.25, dtype=dt)
    if kind == "five_levels":  # heavy ties, zero and both signs among the levels
        return (rng.integers(0, 5, n) * 0.5 - 1.0).astype(dt)
    if kind == "low_bits":  # equal but for the lowest 10 (float32) / 11 (float64) bits: the last pass decides
        it, nb = (np.uint32, 10) if dt == np.float32 else (np.uint64, 11)
        base = np.array(1.5, dtype=dt).view(it)
        return (base + rng.integers(0, 1 << nb, n).astype(it)).view(dt)
    if kind == "signs_zero_inf":
        a = rng.standard_normal(n).astype(dt)
        special = np.array([-0.0, np.inf, 0.0, -np.inf], dtype=dt)
        pos = rng.permutation(n)[:4]
        a[pos] = special[:len(pos)]
        return a
    if kind == "nan_last":
        a = rng.standard_normal(n).astype(dt)
        a[-1] = np.nan
        return a
    raise AssertionError(kind)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["normal", "equal", "five_levels", "low_bits", "signs_zero_inf", "nan_last"])
def test_quantile_equals_numpy(kind, dtype):
    import torch

    for n in NS:
        a = _dataset(kind, n, dtype)
        dev = torch.from_numpy(a).cuda()
        out = torch.empty(1, dtype=dev.dtype, device=dev.device)
        for pct in PCTS:
            with np.errstate(invalid="ignore"), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                want = np.percentile(a, pct)
            got_t = percentile_threshold_device(dev, pct, out=out)
            assert got_t is out and got_t.is_cuda
            got = got_t.cpu().numpy()[0]
            assert got.dtype == want.dtype == np.dtype(dtype)
            assert got == want or (np.isnan(got) and np.isnan(want)), (kind, n, pct, got, want)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_quantile_of_an_unaligned_slice(dtype):
    """Arrays that do not start on a 16-byte boundary (the kernel's vector loads start later)."""
    import torch

    a = _dataset("normal", 100003, dtype)
    dev = torch.from_numpy(a).cuda()
    for off in (1, 3):
        for pct in (0, 37.5, 100):
            got = percentile_threshold_device(dev[off:off + 1029], pct).cpu().numpy()[0]
            assert got == np.percentile(a[off:off + 1029], pct), (off, pct)
        assert percentile_threshold_device(dev[off:off + 2], 50).cpu().numpy()[0] == np.percentile(a[off:off + 2], 50)


# ---- flow_summary against summary_ref ---------------------------------------------------------
SCALES = (0.065, 0.2, 0.75)
ROIS_3D = [(4, 5, 20, 21, 77, 78),      # one voxel
           (6, 9, 30, 37, 100, 131),    # ends at the last voxel
           (0, 9, 0, 37, 33, 36),       # odd x origin, 3 voxels wide
           (1, 6, 5, 25, 10, 90),       # two overlapping boxes ...
           (0, 8, 2, 36, 5, 125)]       # ... the second of several workgroups (like the whole volume)
ROIS_2D = [(7, 8, 9, 10), (30, 40, 40, 44), (0, 40, 11, 14), (5, 25, 5, 30), (15, 35, 20, 44)]
THETA_EDGES = -np.pi + (np.arange(37) + (np.sqrt(2.0) - 1.0)) * (2 * np.pi / 36)
PHI_EDGES = -np.pi / 2 + (np.arange(37) + (np.sqrt(3.0) - 1.5)) * (np.pi / 36)


def _plant_zeros(fields):
    """Exact zeros at voxels that pass the 90th-percentile mask: they turn NaN, not valid."""
    rel = fields[-1]
    top = np.argsort(rel.ravel())[-4:]
    fields[0].ravel()[top[0]] = 0.0
    fields[1].ravel()[top[1]] = 0.0
    fields[-2].ravel()[top[2]] = 0.0


def _edges_from(vals, n_lin, frac):
    """Edges over the central part of the values (the rest is dropped), two of them exactly data
    values, so the half-open / closed-last-bin rules are exercised."""
    v = np.sort(vals)
    lo, hi = v[int(frac * (v.size - 1))], v[int((1 - frac) * (v.size - 1))]
    return np.unique(np.concatenate([np.linspace(lo, hi, n_lin), v[[v.size // 3, v.size // 2]]]))


@pytest.fixture(scope="module")
def fields3d():
    img = np.random.default_rng(3).integers(0, 4096, size=(7, 9, 37, 131)).astype(np.uint16)
    out = [np.ascontiguousarray(a) for a in calc_flow3D(img, 1, 1, 2)]
    _plant_zeros(out)
    return out


@pytest.fixture(scope="module")
def fields2d():
    img = np.random.default_rng(4).integers(0, 4096, size=(7, 40, 44)).astype(np.uint16)
    out = [np.ascontiguousarray(a) for a in calc_flow2D(img, 1, 1, 2)]
    _plant_zeros(out)
    return out


def _bins_for(fields, ndim, pct=90):
    plain = sr.summary_ref(*(fields if ndim == 3 else (fields[0], fields[1], None, fields[2])), pct, *SCALES)
    v = plain["values"][0]
    bins = {"vx": _edges_from(v["vx"], 30, 0.1), "vy": _edges_from(v["vy"], 7, 0.0),
            "magnitude": _edges_from(v["magnitude"], 30, 0.0), "theta": THETA_EDGES}
    if ndim == 3:
        bins["vz"] = _edges_from(v["vz"], 255, 0.05)[:257]
        bins["phi"] = PHI_EDGES
    return bins


@pytest.fixture(scope="module")
def ref3d(fields3d):
    bins = _bins_for(fields3d, 3)
    return bins, sr.summary_ref(*fields3d, 90, *SCALES, rois=ROIS_3D, bins=bins)


def test_summary_3d(fields3d, ref3d):
    bins, ref = ref3d
    assert 1000 < ref["n_valid"][0] < ref["n_voxels"][0] // 9  # about a tenth passes the mask
    sr.assert_clear_of_edges(ref, ("theta", "phi"))
    got = flow_summary(*fields3d, 90, *SCALES, rois=ROIS_3D, bins=bins)
    sr.assert_matches(got, ref, ("vx", "vy", "vz", "magnitude", "theta", "phi"))
    np.testing.assert_allclose(got["mean_magnitude"], ref["mean_magnitude"], rtol=1e-12, equal_nan=True)
    np.testing.assert_allclose(got["theta_mean"], ref["theta_mean"], rtol=0, atol=1e-9, equal_nan=True)
    np.testing.assert_allclose(got["theta_mean_weighted"], ref["theta_mean_weighted"], rtol=0, atol=1e-9, equal_nan=True)


@pytest.mark.parametrize("pct", [50, 99.5])
def test_summary_3d_other_percentiles(fields3d, pct):
    ref = sr.summary_ref(*fields3d, pct, *SCALES, rois=ROIS_3D[:3], bins={"magnitude": [0.0, 0.01, 0.1, 1.0, 1e3]})
    got = flow_summary(*fields3d, pct, *SCALES, rois=ROIS_3D[:3], bins={"magnitude": [0.0, 0.01, 0.1, 1.0, 1e3]})
    sr.assert_matches(got, ref, ("magnitude",))


def test_summary_2d_float64_rel_and_resident_tensors(fields2d):
    import torch

    vx, vy, rel = fields2d
    assert rel.dtype == np.float64
    bins = _bins_for(fields2d, 2)
    ref = sr.summary_ref(vx, vy, None, rel, 90, *SCALES, rois=ROIS_2D, bins=bins)
    sr.assert_clear_of_edges(ref, ("theta",))
    dev = [torch.from_numpy(a).cuda() for a in (vx, vy, rel)]
    got = flow_summary(dev[0], dev[1], None, dev[2], 90, *SCALES, rois=ROIS_2D, bins=bins)
    sr.assert_matches(got, ref, ("vx", "vy", "magnitude", "theta"))
    assert np.all(got["sum_vz"] == 0) and "phi" not in got["hist"]


def test_summary_fp32_fields():
    img = np.random.default_rng(3).integers(0, 4096, size=(7, 9, 37, 131)).astype(np.uint16)
    f = [np.ascontiguousarray(a) for a in calc_flow3D_fp32(img, 1, 1, 2)]
    assert f[0].dtype == np.float32 and f[3].dtype == np.float32
    _plant_zeros(f)
    bins = _bins_for(f, 3)
    ref = sr.summary_ref(*f, 90, *SCALES, rois=ROIS_3D, bins=bins)
    sr.assert_clear_of_edges(ref, ("theta", "phi"))
    got = flow_summary(*f, 90, *SCALES, rois=ROIS_3D, bins=bins)
    sr.assert_matches(got, ref, ("vx", "vy", "vz", "magnitude", "theta", "phi"))


def test_nan_threshold_gives_empty_summary(fields2d):
    vx, vy, rel = fields2d
    rel = rel.copy()
    rel[3, 5] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = flow_summary(vx, vy, None, rel, 90, rois=ROIS_2D[:2], bins={"magnitude": [0.0, 1.0, 2.0]})
    assert np.isnan(got["threshold"]) and got["threshold"].dtype == np.float64
    assert got["n_valid"].tolist() == [0, 0, 0] and got["n_voxels"].tolist() == [40 * 44, 1, 40]
    for k in ("mean_magnitude", "mean_vx", "mean_vy", "mean_vz", "theta_mean", "theta_mean_weighted"):
        assert np.all(np.isnan(got[k])), k
    assert not got["hist"]["magnitude"].any()


def test_bad_box_and_edges_raise(fields2d):
    vx, vy, rel = fields2d
    with pytest.raises(ValueError, match="outside"):
        flow_summary(vx, vy, None, rel, rois=[(0, 41, 0, 44)])
    with pytest.raises(ValueError, match="ascending"):
        flow_summary(vx, vy, None, rel, bins={"vx": [0.0, 0.0, 1.0]})


# ---- determinism --------------------------------------------------------------------------------
def _raw(fields, spec):
    """The raw device result words of one summary call."""
    import torch

    dev = [torch.from_numpy(a).cuda() for a in fields]
    call = _SummaryCall(spec, fields[0].shape, dev[-1].dtype, dev[0].device)
    res = call.new_result(dev[0].device)
    call.enqueue((dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), False), res.data_ptr(),
                 torch.cuda.current_stream().cuda_stream)
    return call, res.cpu().numpy()


def test_same_call_twice_same_bytes(fields3d, ref3d):
    spec = SummarySpec(rois=ROIS_3D, bins=ref3d[0], xyscale=0.065, zscale=0.2, tscale=0.75)
    (_, a), (_, b) = _raw(fields3d, spec), _raw(fields3d, spec)
    assert a.tobytes() == b.tobytes()


def test_whole_volume_row_independent_of_other_rois(fields3d, ref3d):
    kw = dict(bins=ref3d[0], xyscale=0.065, zscale=0.2, tscale=0.75)
    (c1, alone), (c2, many) = _raw(fields3d, SummarySpec(**kw)), _raw(fields3d, SummarySpec(rois=ROIS_3D, **kw))
    words = 10 + sum(c1.nbins)
    assert alone.size == 8 + words and many.size == 8 + 6 * words
    assert alone[0] == many[0]  # the threshold
    assert alone[8:8 + words].tobytes() == many[8:8 + words].tobytes()
    # and a box's row does not depend on its position in the list
    (_, swapped) = _raw(fields3d, SummarySpec(rois=ROIS_3D[::-1], **kw))
    assert swapped[8 + words:8 + 2 * words].tobytes() == many[8 + 5 * words:8 + 6 * words].tobytes()
