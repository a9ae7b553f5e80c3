"""Reliability thresholds, host side: the ranks of both percentile definitions against numpy, the
validation of the new options, and the CSV / npz round trip of a summary with a profile."""

import dataclasses
import warnings

import numpy as np
import pytest

from opticalflow3d_dev_amd import RelProfileSpec, SummarySpec, reliability_profile, reliability_thresholds
from opticalflow3d_dev_amd import analysis as an

NS = (1, 2, 3, 10, 257, 4099, 100003)
PCTS = sorted({0.0, 0.001, 1.0, 2.5, 5.0, 10.0, 12.5, 20.0, 25.0, 30.0, 33.3, 37.5, 40.0, 45.0, 50.0, 55.0, 60.0, 62.5,
               66.6, 70.0, 75.0, 80.0, 85.0, 87.5, 90.0, 92.5, 95.0, 97.5, 99.0, 99.5, 99.9, 99.999, 100.0}
              | {float(v) for v in np.linspace(0.7, 99.3, 16)})


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("method", ["linear", "hazen"])
def test_ranks_and_lerp_equal_numpy(method, dtype):
    dt = np.dtype(dtype)
    assert len(PCTS) == 49
    for n in NS:
        a = np.sort(np.random.default_rng(n).standard_normal(n).astype(dt))
        for p in PCTS:
            lo, hi, gamma = an._percentile_ranks(n, p, dt, method)
            assert 0 <= lo <= hi <= n - 1 and 0.0 <= float(gamma) <= 1.0, (n, p, lo, hi, gamma)
            got = an._lerp(a[lo], a[hi], gamma, dt)
            want = np.percentile(a, p, method=method)
            assert got.dtype == want.dtype == dt
            assert got.tobytes() == want.tobytes(), (method, dt, n, p, got, want)


def test_an_infinite_order_statistic_gives_numpys_nan():
    a = np.array([-np.inf, 0.0, 1.0, np.inf])
    for method in ("linear", "hazen"):
        for p in (0.0, 100.0):
            lo, hi, gamma = an._percentile_ranks(4, p, a.dtype, method)
            with np.errstate(invalid="ignore"), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                got, want = an._lerp(a[lo], a[hi], gamma, a.dtype), np.percentile(a, p, method=method)
            assert np.isnan(got) and np.isnan(want), (method, p, got, want)


def test_linear_is_linear_ranks():
    for dt in (np.dtype(np.float32), np.dtype(np.float64)):
        for n in NS:
            for p in PCTS:
                a, b = an._percentile_ranks(n, p, dt, "linear"), an._linear_ranks(n, p, dt)
                assert a[:2] == b[:2] and a[2].tobytes() == b[2].tobytes() and a[2].dtype == b[2].dtype


def test_the_short_hazen_form_is_not_numpys():
    """n*q - 0.5 is not what numpy evaluates: float32, n = 3, p = 33.3 differs in the last bit."""
    dt, n, p = np.dtype(np.float32), 3, 33.3
    q = np.true_divide(p, dt.type(100))
    lo, _, gamma = an._percentile_ranks(n, p, dt, "hazen")
    assert dt.type(n * q - dt.type(0.5) - lo).tobytes() != gamma.tobytes()


def test_bad_method():
    with pytest.raises(ValueError, match="percentile_method"):
        an._percentile_ranks(10, 50, np.dtype(np.float32), "nearest")
    with pytest.raises(ValueError, match="percentile_method"):
        SummarySpec(percentile_method="matlab").resolve((4, 5, 6))
    with pytest.raises(ValueError, match="percentile_method"):
        SummarySpec(percentile_method=None).resolve((4, 5, 6))


@pytest.mark.parametrize("ps", [(), tuple(range(9))])
def test_percentile_count(ps):
    with pytest.raises(ValueError, match="percentiles needs 1 to 8"):
        an._check_percentiles(ps, "percentiles")


@pytest.mark.parametrize("p", [-0.5, 100.5, float("nan")])
def test_percentile_range(p):
    with pytest.raises(ValueError, match="percentiles .* outside"):
        an._check_percentiles((50, p), "percentiles")
    with pytest.raises(ValueError, match="rel_profile percentiles .* outside"):
        RelProfileSpec(percentiles=(p,)).resolve()


@pytest.mark.parametrize("box, what", [((0, 4, 0, 5), "needs 6 bounds"), ((0, 4, 0, 5, 0, 6, 1), "needs 6 bounds"),
                                       ((1, 1, 0, 5, 0, 6), "empty or outside"), ((0, 4, 0, 5, 0, 7), "empty or outside"),
                                       ((-1, 4, 0, 5, 0, 6), "empty or outside"), ((0, 4, 0, 5, 0.5, 6), "non-integer"),
                                       (5, "is not a box")])
def test_bad_percentile_box(box, what):
    with pytest.raises(ValueError, match="percentile_box.*" + what):
        SummarySpec(percentile_box=box).resolve((4, 5, 6))


def test_percentile_box_2d_and_good_values():
    spec = SummarySpec(percentile_box=(1, 4, 2, 6), percentile_method="hazen", rel_profile=RelProfileSpec())
    box, method, profile = spec.threshold_request((5, 6))
    assert box == (0, 1, 1, 4, 2, 6) and method == "hazen" and profile == ([85.0, 90.0, 95.0], 50, None)
    assert SummarySpec().threshold_request((4, 5, 6)) == (None, "linear", None)
    with pytest.raises(ValueError, match="percentile_box.*needs 4 bounds"):
        SummarySpec(percentile_box=(0, 1, 1, 4, 2, 6)).resolve((5, 6))


@pytest.mark.parametrize("bins", [0, 257, 2.5, True])
def test_profile_bins(bins):
    with pytest.raises(ValueError, match="rel_profile bins"):
        RelProfileSpec(bins=bins).resolve()


@pytest.mark.parametrize("edges", [[0.0], [0.0, 0.0], [1.0, 0.5], [0.0, np.nan, 1.0], np.arange(258.0)])
def test_profile_edges(edges):
    with pytest.raises(ValueError, match="rel_profile"):
        RelProfileSpec(edges=edges).resolve()


def test_profile_spec_resolves_and_rides_on_the_summary_spec():
    ps, nbins, edges = RelProfileSpec(percentiles=(50,), edges=[0.0, 0.5, 2.0]).resolve()
    assert ps == [50.0] and nbins == 2 and edges.dtype == np.float64 and edges.tolist() == [0.0, 0.5, 2.0]
    assert RelProfileSpec(bins=np.int64(256)).resolve()[1] == 256
    with pytest.raises(ValueError, match="percentiles needs 1 to 6"):
        RelProfileSpec(percentiles=tuple(range(7))).resolve()
    with pytest.raises(ValueError, match="rel_profile .* is not a RelProfileSpec"):
        SummarySpec(rel_profile={"bins": 5}).resolve((4, 5, 6))


def test_spec_fields():
    names = [f.name for f in dataclasses.fields(SummarySpec)]
    assert names[-1] == "weighted_bins" and names[-2] == "spread"
    assert names[-5:-2] == ["percentile_box", "percentile_method", "rel_profile"]
    s = SummarySpec()
    assert s.percentile_box is None and s.percentile_method == "linear" and s.rel_profile is None


def test_public_functions_validate_before_the_device():
    """The wrappers refuse bad arguments by name (a numpy array is no CUDA tensor: TypeError)."""
    with pytest.raises(TypeError, match="CUDA tensor"):
        reliability_thresholds(np.zeros((2, 3, 4), np.float32), [50])
    with pytest.raises(ValueError, match="percentiles needs 1 to 6"):
        reliability_profile(np.zeros((2, 3, 4), np.float32), percentiles=range(7))
    with pytest.raises(ValueError, match="percentile_box"):
        reliability_profile(np.zeros((2, 3, 4), np.float32), box=(0, 3, 0, 3, 0, 4))
    with pytest.raises(ValueError, match="percentile_method"):
        reliability_profile(np.zeros((2, 3, 4), np.float32), method="midpoint")
    with pytest.raises(ValueError, match="rel_profile bins"):
        reliability_profile(np.zeros((2, 3, 4), np.float32), bins=0)


def _hand_made(frame, with_profile):
    n_roi = 2
    rng = np.random.default_rng(frame)
    s = {"threshold": np.float32(0.1 + frame), "rois": np.array([[0, 2, 0, 3, 0, 4], [0, 1, 1, 2, 2, 3]]),
         "n_valid": np.array([5, 1]), "n_voxels": np.array([24, 1]), "hist": {}, "edges": {}}
    for k in an.CSV_COLUMNS[11:]:
        s[k] = rng.standard_normal(n_roi)
    if with_profile:
        s["rel_profile"] = {"percentiles": np.array([85.0, 90.0, 99.5]),
                            "thresholds": rng.standard_normal(3).astype(np.float32),
                            "min": np.float32(-1.5 - frame), "max": np.float32(7.25), "rois": s["rois"],
                            "n_voxels": s["n_voxels"], "n_nan": np.array([2, 0]),
                            "n_above": rng.integers(0, 24, (n_roi, 3)),
                            "hist": rng.integers(0, 9, (n_roi, 4)).astype(np.uint64),
                            "edges": np.linspace(-1.5 - frame, 7.25, 5)}
    return s


def test_csv_and_npz_round_trip_with_a_profile(tmp_path):
    frames, sums = [3, 4], [_hand_made(3, True), _hand_made(4, True)]
    an.write_summaries(str(tmp_path / "p"), frames, sums)
    with open(tmp_path / "p_summary.csv") as f:
        header = f.readline().strip().split(",")
    extra = ("rel_min", "rel_max", "rel_n_nan", "rel_p85", "n_above_p85", "rel_p90", "n_above_p90", "rel_p99.5",
             "n_above_p99.5")
    assert tuple(header) == an.CSV_COLUMNS + extra
    assert an.profile_columns([85, 90, 99.5]) == extra and an.CSV_PROFILE_COLUMNS == extra[:3]
    csv, npz = an.read_summary_csv(tmp_path / "p_summary.csv"), np.load(tmp_path / "p_summary_hist.npz")
    for i, s in enumerate(sums):
        p, rows = s["rel_profile"], slice(2 * i, 2 * i + 2)
        assert np.all(csv["rel_min"][rows] == np.float64(p["min"])) and np.all(csv["rel_max"][rows] == 7.25)
        assert csv["rel_n_nan"].dtype == np.int64 and np.array_equal(csv["rel_n_nan"][rows], p["n_nan"])
        for k, name in enumerate(("85", "90", "99.5")):
            assert np.all(csv["rel_p" + name][rows] == np.float64(p["thresholds"][k]))
            assert csv["n_above_p" + name].dtype == np.int64
            assert np.array_equal(csv["n_above_p" + name][rows], p["n_above"][:, k])
        assert np.array_equal(npz["counts_rel"][i], p["hist"]) and npz["counts_rel"].dtype == np.uint64
        assert np.array_equal(npz["edges_rel"][i], p["edges"])
    assert npz["counts_rel"].shape == (2, 2, 4) and npz["edges_rel"].shape == (2, 5)


def test_header_without_a_profile_is_unchanged(tmp_path):
    an.write_summaries(str(tmp_path / "q"), [3], [_hand_made(3, False)])
    with open(tmp_path / "q_summary.csv") as f:
        assert tuple(f.readline().strip().split(",")) == an.CSV_COLUMNS
    assert sorted(np.load(tmp_path / "q_summary_hist.npz").files) == ["frames"]


def test_exports_and_abi():
    import opticalflow3d_dev_amd as pkg
    from opticalflow3d_dev_amd import _lib

    for name in ("reliability_thresholds", "reliability_profile", "RelProfileSpec"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    for name in ("of3d_rel_select", "of3d_rel_select_workspace_bytes", "of3d_rel_profile",
                 "of3d_rel_profile_result_bytes"):
        assert name in _lib.EXPORTED and hasattr(_lib.load(), name)
    lib = _lib.load()
    assert lib.of3d_rel_profile_result_bytes(2, 5, 50) == (3 + 5 + 51 + 2 * (2 + 5 + 50)) * 8
    assert lib.of3d_rel_profile_result_bytes(17, 5, 50) == 0 and lib.of3d_rel_profile_result_bytes(1, 9, 50) == 0
    assert lib.of3d_rel_profile_result_bytes(1, 1, 0) == 0 and lib.of3d_rel_profile_result_bytes(1, 1, 257) == 0
    assert lib.of3d_rel_select_workspace_bytes(0) == lib.of3d_rel_select_workspace_bytes(1) > 0
