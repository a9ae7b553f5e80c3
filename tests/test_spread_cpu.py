"""Host side of the spread block (no GPU): the numpy restatement tests/spread_ref.py against
np.std and scipy.stats.circstd, SummarySpec.spread's validation, the C ABI's host arithmetic and
the CSV writer's round trip of CSV_SPREAD_COLUMNS."""
import ctypes

import numpy as np
import pytest
from scipy import stats

import spread_ref as spr
import summary_ref as sr
from opticalflow3d_dev_amd import SummarySpec, _lib, analysis

SHAPE, SCALES, ROIS = (5, 37, 67), (0.3, 1.2, 0.5), [(0, 5, 1, 36, 3, 64)]


@pytest.fixture(scope="module")
def general():
    rng = np.random.default_rng(100)
    f = [rng.standard_normal(SHAPE) for _ in range(3)] + [rng.random(SHAPE, dtype=np.float32)]
    ref = sr.summary_ref(*f, 60, *SCALES, rois=ROIS)
    return ref, spr.spread_ref(ref, "mean")


# ---- the reference itself ---------------------------------------------------------------------------
def test_reference_std_is_numpys(general):
    ref, s = general
    assert ref["n_valid"][1] > 1000
    for r, vals in enumerate(ref["values"]):
        for k in spr.COMPONENTS:
            want = np.std(vals[k])
            assert abs(s["std_" + k][r] - want) <= 1e-13 * want, (r, k)
        cov = np.cov(np.stack([vals[k] for k in ("vx", "vy", "vz")]), ddof=0)
        assert np.allclose(s["velocity_covariance"][r], cov, rtol=1e-12, atol=0)
        for k in spr.COMPONENTS:
            assert s["min_" + k][r] == vals[k].min() and s["max_" + k][r] == vals[k].max()


def test_reference_circular_std_is_scipys(general):
    ref, s = general
    for r, vals in enumerate(ref["values"]):
        want = stats.circstd(vals["theta"], high=np.pi, low=-np.pi)
        assert abs(s["theta_std"][r] - want) <= 1e-12, r
        want = stats.circstd(vals["phi"], high=np.pi, low=-np.pi)  # sin / cos of phi = vz / mag, h / mag
        assert abs(s["phi_std"][r] - want) <= 1e-12, r
        assert abs(s["phi_mean"][r] - stats.circmean(vals["phi"], high=np.pi, low=-np.pi)) <= 1e-12
        # the notebook's R divides by the array's size, NaNs included
        n_all = ref["n_voxels"][r]
        R = np.hypot(np.sin(vals["theta"]).sum(), np.cos(vals["theta"]).sum()) / n_all
        assert abs(s["theta_std_all"][r] - np.sqrt(-2 * np.log(R))) <= 1e-12


def test_reference_about_a_given_centre_is_the_rms_error(general):
    ref, _ = general
    c = (0.1, -0.2, 0.3, 1.0)
    s = spr.spread_ref(ref, c)
    for r, vals in enumerate(ref["values"]):
        assert s["spread_center"][r].tolist() == list(c)
        for q, k in enumerate(spr.COMPONENTS):
            want = np.sqrt(np.mean((vals[k] - c[q]) ** 2))
            assert abs(s["std_" + k][r] - want) <= 1e-13 * want


def test_reference_of_an_empty_roi_is_nan_without_warnings():
    import warnings

    vx = np.ones((4, 6))
    rel = np.zeros((4, 6), np.float32)
    rel[0, 0] = 1.0
    ref = sr.summary_ref(vx, 2 * vx, None, rel, 50, rois=[(2, 4, 2, 5)])
    assert ref["n_valid"].tolist() == [1, 0]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        s = spr.spread_ref(ref, "mean")
    assert np.all(np.isnan(s["spread_center"][1])) and np.isnan(s["min_vx"][1]) and np.isnan(s["std_vx"][1])
    assert s["ss_vx"][1] == 0 and s["sum_sin_phi"].tolist() == [0, 0] and "phi_std" not in s
    assert s["std_vx"][0] == 0 and s["spread_center"][0].tolist() == [1.0, 2.0, 0.0, np.sqrt(5.0)]


# ---- SummarySpec.spread -----------------------------------------------------------------------------
def test_spec_resolves_spread():
    assert SummarySpec().spread_request(3) is None
    assert SummarySpec(spread="mean").spread_request(2) == (None,)
    (g,) = SummarySpec(spread=(1, 2, 3, 4)).spread_request(3)
    assert g.dtype == np.float64 and g.tolist() == [1.0, 2.0, 3.0, 4.0]
    (g,) = SummarySpec(spread=np.array([1.5, -2.0, 4.0])).spread_request(2)  # vx vy magnitude: vz = 0
    assert g.tolist() == [1.5, -2.0, 0.0, 4.0]
    SummarySpec(spread=(1, 2, 3, 4)).resolve((4, 5, 6))
    SummarySpec(spread="mean", rois=[(1, 3, 1, 4)]).resolve((5, 6))


@pytest.mark.parametrize("spread,shape", [
    ((1.0, 2.0, 3.0), (4, 5, 6)),            # a wrong length
    ((1.0, 2.0, 3.0, 4.0, 5.0), (4, 5, 6)),
    ((1.0, np.nan, 3.0, 4.0), (4, 5, 6)),    # a NaN
    ((1.0, np.inf, 4.0), (5, 6)),
    ("median", (4, 5, 6)),                   # a string other than "mean"
    ((1.0, 2.0, 3.0, 4.0), (5, 6)),          # four numbers for a 2D volume
    (((1.0, 2.0), (3.0, 4.0)), (5, 6)),
    (object(), (5, 6)),
    (True, (5, 6)),
])
def test_spec_rejects_spread(spread, shape):
    with pytest.raises(ValueError, match="summary: spread"):
        SummarySpec(spread=spread).resolve(shape)


# ---- the C ABI's host arithmetic --------------------------------------------------------------------
def test_c_abi_sizes_and_refusals():
    lib = _lib.load()
    I = ctypes.POINTER(ctypes.c_int64)
    assert lib.of3d_flow_spread_result_bytes(1) == 22 * 8 and lib.of3d_flow_spread_result_bytes(16) == 16 * 22 * 8
    assert lib.of3d_flow_spread_result_bytes(0) == 0 and lib.of3d_flow_spread_result_bytes(17) == 0
    # workgroups as of3d_flow_summary's: ceil(voxels / 8192), at most the rows; 17 words each
    rois = np.array([[0, 6, 0, 21, 0, 67], [0, 1, 0, 2, 0, 20000], [2, 3, 4, 9, 7, 30]], dtype=np.int64)
    assert lib.of3d_flow_spread_workspace_bytes(rois.ctypes.data_as(I), 3) == (2 + 2 + 1) * 17 * 8
    bad = np.array([[0, 6, 5, 5, 0, 67]], dtype=np.int64)
    assert lib.of3d_flow_spread_workspace_bytes(bad.ctypes.data_as(I), 1) == 0
    assert "empty or outside" in _lib.last_error()
    assert lib.of3d_flow_spread_workspace_bytes(rois.ctypes.data_as(I), 17) == 0
    assert "1 to 16" in _lib.last_error()

    # argument errors are reported before anything is enqueued (the pointers are never read)
    one = ctypes.c_void_p(8)
    c = (ctypes.c_double * 4)(0, 0, 0, 0)
    nb = (ctypes.c_int * 6)()
    call = lambda **kw: lib.of3d_flow_spread(*[kw.get(k, v) for k, v in dict(
        vx=one, vy=one, vz=one, rel=one, v_f32=0, rel_f64=0, nz=6, ny=21, nx=67, thresh=one, sxy=1.0, sz=1.0, st=1.0,
        rois=rois.ctypes.data_as(I), n_roi=1, keep=None, summary=one, nbins=nb, center=c, result=one, ws=one,
        stream=None).items()])
    for kw, word in ((dict(vx=None), "null"), (dict(result=None), "null"), (dict(rel=None), "null"),
                     (dict(nz=0), "dims"), (dict(vz=None), "2D"), (dict(center=None, summary=None), "center"),
                     (dict(center=None, nbins=None), "nbins"), (dict(n_roi=0), "1 to 16")):
        assert call(**kw) != 0 and word in _lib.last_error(), (kw, _lib.last_error())


# ---- the CSV columns --------------------------------------------------------------------------------
def _decoded(ndim):
    """A decoded dict from made-up result words: what _SpreadCall.decode adds to a summary's."""
    n_roi = 2
    call = object.__new__(analysis._SpreadCall)
    call.boxes, call.ndim = np.zeros((n_roi, 6), np.int64), ndim
    rng = np.random.default_rng(5)
    f = rng.random((n_roi, 21)) + 0.1
    words = np.concatenate([np.array([[7], [0]], np.int64), f.view(np.int64)], axis=1).reshape(-1)
    out = {"threshold": np.float32(0.5), "rois": np.array([[0, 1, 0, 4, 0, 5], [0, 1, 1, 2, 1, 3]]),
           "n_valid": np.array([7, 0]), "n_voxels": np.array([20, 2])}
    for i, k in enumerate(analysis.SUMS):
        out[k] = np.array([0.3 + i, 0.0])
    for k in ("mean_magnitude", "mean_vx", "mean_vy", "mean_vz", "theta_mean", "theta_mean_weighted"):
        out[k] = np.array([0.25, np.nan])
    out["hist"], out["edges"] = {}, {}
    return call.decode(words, out), f


@pytest.mark.parametrize("ndim", [2, 3])
def test_decode_and_csv_round_trip(tmp_path, ndim):
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("error")
        s, f = _decoded(ndim)
    assert s["spread_center"].tobytes() == f[:, :4].tobytes() and s["ss_vx_vz"][0] == f[0, 9]
    assert s["min_vx"][1] == f[1, 13] and s["max_magnitude"][0] == f[0, 20]
    assert s["std_vy"][0] == np.sqrt(f[0, 5] / 7) and np.isnan(s["std_vy"][1])
    assert s["velocity_covariance"].shape == (2, 3, 3) and s["velocity_covariance"][0, 1, 2] == f[0, 10] / 7
    assert np.array_equal(s["velocity_covariance"][0], s["velocity_covariance"][0].T)
    assert ("phi_std" in s) == ("phi_mean" in s) == ("phi_std_all" in s) == (ndim == 3)
    assert np.isnan(s["theta_std"][1]) and s["theta_std"][0] >= 0
    analysis.write_summaries(str(tmp_path / "a"), [4], [s])
    got = analysis.read_summary_csv(str(tmp_path / "a_summary.csv"))
    cols = open(tmp_path / "a_summary.csv").readline().strip().split(",")
    assert tuple(cols) == analysis.CSV_COLUMNS + analysis.CSV_SPREAD_COLUMNS
    for k in ("ss_vx", "sum_cos_phi", "min_vz", "max_magnitude", "std_magnitude", "theta_std", "theta_std_all"):
        assert got[k].tobytes() == np.asarray(s[k], np.float64).tobytes(), k
    assert got["spread_center_vz"].tobytes() == s["spread_center"][:, 2].tobytes()
    assert got["vcov_xz"].tobytes() == s["velocity_covariance"][:, 0, 2].tobytes()
    if ndim == 3:
        assert got["phi_std"].tobytes() == s["phi_std"].tobytes()
    else:
        assert np.all(np.isnan(got["phi_std"]))
    plain = {k: v for k, v in s.items() if k in ("threshold", "rois", "n_valid", "n_voxels", "hist", "edges")
             or k in analysis.CSV_COLUMNS}
    analysis.write_summaries(str(tmp_path / "b"), [4], [plain])
    assert tuple(open(tmp_path / "b_summary.csv").readline().strip().split(",")) == analysis.CSV_COLUMNS
