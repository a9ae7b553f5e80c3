"""The spread block of the device-side frame summary (csrc/kt_spread.hip: of3d_flow_spread)
against the numpy restatement tests/spread_ref.py: bitwise on fields whose deviation products
sum exactly in any order, within the sum bound on general fields; the cancellation a one-pass
variance fails, determinism, the shapes that break walks, the opened mask and the drivers."""
import warnings

import numpy as np
import pytest

import mask_ref as mr
import spread_ref as spr
import summary_ref as sr
import whist_ref as wr
from conftest import bits_equal
from opticalflow3d_dev_amd import SummarySpec, calc_flow2D, calc_flow3D, flow_summary, process_flow
from opticalflow3d_dev_amd import analysis
from opticalflow3d_dev_amd import tiff as tf
from opticalflow3d_dev_amd.analysis import _SummaryCall
from test_gpu_whist import M_ROIS, _ramp_fields, blobs  # noqa: F401  (blobs: that module's fixture)

pytestmark = pytest.mark.gpu

CENTER = (0.75, -1.5, 2.25, 5.0)  # multiples of 2^-2, as every exact component and magnitude


def assert_bitwise(got, ref, keys=spr.EXACT):
    """flow_summary's spread keys against spread_ref's, bit for bit (NaN bits included)."""
    assert np.array_equal(got["n_valid"], ref["n_valid"]), (got["n_valid"], ref["n_valid"])
    for k in keys:
        g, w = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64)
        assert g.shape == w.shape and bits_equal(g, w), (k, g, w)


# ---- 1. the exact case: any summation order gives the reference's bits ------------------------------
@pytest.fixture(scope="module")
def exact():
    f = wr.exact_case()
    ref = sr.summary_ref(*f, 50, rois=wr.EXACT_ROIS)
    return f, ref, spr.spread_ref(ref, CENTER)


def test_exact_case_is_the_reference_bit_for_bit(exact):
    f, ref, sref = exact
    assert ref["n_valid"].tolist() == [4221, 2083, 53]
    # every product is a multiple of 2^-4 below 2^12: every partial sum is exact in any order
    assert all(np.all(sref["abs_" + k] < 2.0 ** 12 * ref["n_valid"]) for k in spr.SUMS[:7])
    got = flow_summary(*f, 50, rois=wr.EXACT_ROIS, spread=CENTER)
    assert_bitwise(got, sref)
    assert bits_equal(got["spread_center"], np.tile(np.array(CENTER), (3, 1)))
    for k in ("sum_sin_phi", "sum_cos_phi"):
        assert np.all(np.abs(got[k] - sref[k]) <= spr.sum_bound(sref, k)), k
    assert np.all(got["min_magnitude"] > 0) and np.all(got["max_vx"] > got["min_vx"])


def test_exact_case_with_float32_fields_and_float64_rel(exact):
    (vx, vy, vz, rel), _, _ = exact
    f = [a.astype(np.float32) for a in (vx, vy, vz)] + [rel.astype(np.float64)]  # the values are exact in float32
    ref = sr.summary_ref(*f, 50, rois=wr.EXACT_ROIS)
    assert_bitwise(flow_summary(*f, 50, rois=wr.EXACT_ROIS, spread=CENTER), spr.spread_ref(ref, CENTER))


# ---- 2. the general case ---------------------------------------------------------------------------
G_SHAPE, G_SCALES, G_ROIS = (5, 37, 67), (0.3, 1.2, 0.5), [(0, 5, 1, 36, 3, 64)]


@pytest.mark.parametrize("seed", [100, 101, 102, 103])
def test_general_case_within_the_sum_bound(seed):
    rng = np.random.default_rng(seed)
    f = [rng.standard_normal(G_SHAPE) for _ in range(3)] + [rng.random(G_SHAPE, dtype=np.float32)]
    bins = {"theta": np.linspace(-np.pi, np.pi, 9), "magnitude": np.linspace(0, 4, 17)}
    ref = sr.summary_ref(*f, 60, *G_SCALES, rois=G_ROIS)
    got = flow_summary(*f, 60, *G_SCALES, rois=G_ROIS, bins=bins, spread="mean")
    assert np.array_equal(got["n_valid"], ref["n_valid"]) and ref["n_valid"][1] > 1000
    # the centre is the dict's own sum / n, one IEEE division
    nv = got["n_valid"].astype(np.float64)
    want = np.stack([got["sum_" + k] / nv for k in spr.COMPONENTS], axis=1)
    assert bits_equal(got["spread_center"], want)
    # the sums about that reported centre
    sref = spr.spread_ref(ref, got["spread_center"])
    for k in spr.SUMS:
        err, bound = np.abs(got[k] - sref[k]), spr.sum_bound(sref, k)
        print(k, "max err / bound:", float(np.max(err / np.maximum(bound, 1e-300))))
        assert np.all(err <= bound), (k, err, bound)
    assert_bitwise(got, sref, [f"{m}_{k}" for m in ("min", "max") for k in spr.COMPONENTS])
    # the std against the two-pass fsum std: moving the centre by its own rounding error changes
    # the sum only in second order
    two_pass = spr.spread_ref(ref, "mean")
    for k in spr.COMPONENTS:
        rel_err = np.abs(got["std_" + k] - two_pass["std_" + k]) / two_pass["std_" + k]
        print("std_" + k, "rel err / bound:", float(np.max(rel_err / ((nv + 32) * 2.0 ** -53))))
        assert np.all(rel_err <= (nv + 32) * 2.0 ** -53), (k, rel_err)
    for k in ("velocity_covariance", "theta_std", "theta_resultant", "phi_mean", "phi_std", "phi_resultant",
              "theta_std_all", "phi_std_all"):
        assert np.allclose(got[k], two_pass[k], rtol=1e-12, atol=1e-14), k
    # keys, hists and the eight old sums are those of the same call without spread
    plain = flow_summary(*f, 60, *G_SCALES, rois=G_ROIS, bins=bins)
    new = ({"spread_center", "velocity_covariance", "theta_resultant", "theta_std", "theta_std_all", "phi_mean",
            "phi_resultant", "phi_std", "phi_std_all"} | set(spr.SUMS)
           | {f"{m}_{k}" for m in ("min", "max", "std") for k in spr.COMPONENTS})
    assert set(got) - set(plain) == new and set(plain) <= set(got)
    for k in plain:
        if k in ("hist", "edges"):
            assert all(bits_equal(got[k][q], plain[k][q]) for q in plain[k]), k
        else:
            assert bits_equal(np.asarray(got[k]), np.asarray(plain[k])), k


# ---- 3. cancellation ---------------------------------------------------------------------------------
def test_uniform_translation_has_no_spread():
    """std << |mean|: a one-pass E[x^2] - E[x]^2 leaves ~sqrt(n) ulp of |v|, or the root of a
    negative number, here."""
    shape, v = (3, 40, 256), (0.1, -0.3, 0.7)
    rel = _ramp_fields(shape, 3)[3]
    f = [np.full(shape, c) for c in v] + [rel]
    got = flow_summary(*f, 0, spread="mean")
    n = got["n_valid"][0]
    assert n == 3 * 40 * 256 - 1
    mag = np.sqrt(np.power(v[0], 2) + np.power(v[1], 2) + np.power(v[2], 2))
    for k, a in zip(spr.COMPONENTS, v + (mag,)):
        print("std_" + k, got["std_" + k][0], "bound", (n + 16) * 2.0 ** -53 * abs(a))
        assert got["std_" + k][0] <= (n + 16) * 2.0 ** -53 * abs(a), k  # NaN fails this too
        assert got["min_" + k][0] == got["max_" + k][0] == a
    assert np.all(np.abs(got["velocity_covariance"][0]) <= ((n + 16) * 2.0 ** -53 * mag) ** 2)


# ---- 4. determinism ----------------------------------------------------------------------------------
def _raw(fields, spec):
    """The call and the raw device result words of one summary call."""
    import torch

    dev = [torch.from_numpy(a).cuda() for a in fields]
    call = _SummaryCall(spec, fields[0].shape, dev[-1].dtype, dev[0].device)
    res = call.new_result(dev[0].device)
    call.enqueue((dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), False), res.data_ptr(),
                 torch.cuda.current_stream().cuda_stream)
    return call, res.cpu().numpy()


@pytest.mark.parametrize("spread", ["mean", (0.1, -0.2, 0.3, 1.5)])
def test_same_bits_twice_and_independent_of_other_rois(spread):
    rng = np.random.default_rng(7)
    f = [rng.standard_normal(G_SHAPE) for _ in range(3)] + [rng.random(G_SHAPE, dtype=np.float32)]
    kw = dict(rel_percentile=60, xyscale=0.3, zscale=1.2, tscale=0.5, spread=spread)
    rois = G_ROIS + [(1, 4, 0, 37, 10, 11), (0, 5, 0, 37, 0, 67)]
    (c, a), (_, b) = (_raw(f, SummarySpec(rois=rois, **kw)) for _ in range(2))
    assert a.tobytes() == b.tobytes()
    block = lambda call, words: words[call.spread_off // 8:].reshape(len(call.boxes), -1)
    many = block(c, a)
    assert many.shape == (4, 22) and c.spread_off == c.result_bytes - 4 * 22 * 8
    assert many[0].tobytes() == many[3].tobytes()  # the whole volume again, as the last box
    c1, alone = _raw(f, SummarySpec(**kw))
    assert block(c1, alone)[0].tobytes() == many[0].tobytes()
    assert np.all(many[:, 0] > 0) and many[0, 0] > 1000


# ---- 5. shapes that break walks ----------------------------------------------------------------------
def test_two_long_rows_and_boxes_narrower_than_a_wave():
    """(2, 20000) in 2D: 5 workgroups by size, capped at the 2 rows; then boxes of 1 to 3 columns.
    Every voxel holds k times the triple (3, 4, 5), k <= 256: the products are multiples of 2^-4
    below 2^22, 40000 of them sum exactly."""
    f = _ramp_fields((2, 20000), 2)
    rois = [(0, 2, 7, 10), (1, 2, 19999, 20000), (0, 2, 0, 63), (0, 1, 1, 20000)]
    ref = sr.summary_ref(*f, 0, rois=rois)
    assert ref["n_valid"].tolist() == [39999, 6, 0, 126, 19999]
    center = (0.75, -1.5, 5.0)
    sref = spr.spread_ref(ref, (0.75, -1.5, 0.0, 5.0))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = flow_summary(*f, 0, rois=rois, spread=center)
    assert_bitwise(got, sref)
    assert np.isnan(got["min_vx"][2]) and np.isnan(got["max_magnitude"][2]) and np.isnan(got["std_vx"][2])
    assert got["spread_center"][2].tolist() == [0.75, -1.5, 0.0, 5.0]
    for k in ("ss_vz", "ss_vx_vz", "ss_vy_vz", "sum_sin_phi", "sum_cos_phi", "min_vz", "max_vz"):
        assert not np.nan_to_num(got[k]).any(), k  # 2D: every vz term and both phi sums are 0
    assert "phi_std" not in got and "phi_mean" not in got and "theta_std_all" in got


def test_ragged_tails_in_3d():
    """(3, 40, 256): 4 workgroups of 30 rows; a box of 64 columns (2 workgroups) and one row."""
    f = _ramp_fields((3, 40, 256), 3)
    rois = [(0, 3, 0, 40, 0, 64), (1, 2, 3, 4, 0, 256), (0, 3, 1, 40, 5, 252)]
    ref = sr.summary_ref(*f, 0, rois=rois)
    assert ref["n_valid"].tolist() == [3 * 40 * 256 - 1, 3 * 40 * 64, 256, 3 * 39 * 247]
    got = flow_summary(*f, 0, rois=rois, spread=CENTER)
    assert_bitwise(got, spr.spread_ref(ref, CENTER))


def test_empty_roi_and_nan_threshold():
    rng = np.random.default_rng(9)
    vx, vy = wr.exact_fields((33, 45), rng, ndim=2)
    rel = rng.random((33, 45))
    rel[4:6, 7:10] = 0.0  # a box below any positive threshold: no valid voxel
    rois = [(4, 6, 7, 10), (0, 33, 44, 45)]
    ref = sr.summary_ref(vx, vy, None, rel, 50, rois=rois)
    assert ref["n_valid"][1] == 0 and ref["n_valid"][2] > 0
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = flow_summary(vx, vy, None, rel, 50, rois=rois, spread="mean")
    assert np.array_equal(got["n_valid"], ref["n_valid"])
    assert np.all(np.isnan(got["spread_center"][1]))  # 0 / 0 on the device
    for k in spr.COMPONENTS:
        assert np.isnan(got["min_" + k][1]) and np.isnan(got["max_" + k][1]) and np.isnan(got["std_" + k][1])
    for k in spr.SUMS:
        assert got[k][1] == 0.0, k
    assert np.isnan(got["theta_std"][1]) and np.all(np.isnan(got["velocity_covariance"][1]))
    sref = spr.spread_ref(ref, got["spread_center"])
    for k in spr.SUMS:
        ok = np.abs(got[k] - sref[k]) <= spr.sum_bound(sref, k)
        assert ok[0] and ok[2], k
    rel[0, 0] = np.nan  # a NaN threshold: nothing is valid
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = flow_summary(vx, vy, None, rel, 50, rois=rois, spread="mean")
    assert np.isnan(got["threshold"]) and got["n_valid"].tolist() == [0, 0, 0]
    assert np.all(np.isnan(got["spread_center"])) and np.all(np.isnan(got["max_vx"])) and not got["ss_vx"].any()
    with pytest.raises(ValueError, match="summary: spread"):
        flow_summary(vx, vy, None, rel, 50, spread=CENTER)  # four numbers for a 2D frame


# ---- 6. the masked route ---------------------------------------------------------------------------
def test_min_size_1_has_the_unmasked_bits(blobs):
    for spread in ("mean", CENTER):
        plain = flow_summary(*blobs, 70, rois=M_ROIS, spread=spread)
        for extra in (dict(min_size=1), dict(min_size=1, connectivity=6)):
            got = flow_summary(*blobs, 70, rois=M_ROIS, spread=spread, **extra)
            for k in ("spread_center",) + spr.SUMS + spr.EXACT:
                assert bits_equal(got[k], plain[k]), k
    assert np.all(plain["n_valid"] > 100)


def test_opened_mask_against_the_labelled_reference(blobs):
    vx, vy, vz, rel = blobs
    boxes, thresh = mr.boxes_of(vx.shape, M_ROIS), np.percentile(rel, 80)
    keep, counts = mr.open_ref(rel, thresh, boxes, 20, 18)
    assert np.all(counts["n_components_kept"] > 0) and np.all(counts["n_components"] > counts["n_components_kept"])
    masked = mr.summary_ref_masked(vx, vy, vz, keep, thresh, boxes)
    got = flow_summary(vx, vy, vz, rel, 80, rois=M_ROIS, spread=CENTER, min_size=20, connectivity=18)
    assert np.array_equal(got["n_kept"], counts["n_kept"]) and np.all(got["n_kept"] < got["n_mask"])
    assert_bitwise(got, spr.spread_ref(masked, CENTER))


# ---- 7. the drivers ----------------------------------------------------------------------------------
D_KW = dict(rel_percentile=70, xyscale=0.1, zscale=0.3, tscale=2.0)


@pytest.mark.parametrize("ndim", [2, 3])
def test_flowstream_gives_flow_summary_bits_per_frame(ndim):
    from opticalflow3d_dev_amd.stream import FlowStream

    shape = (6, 16, 20) if ndim == 3 else (30, 26)
    series = np.random.default_rng(60 + ndim).integers(0, 4096, size=(9,) + shape).astype(np.uint16)
    rois = [(1, 5, 3, 14, 2, 17)] if ndim == 3 else [(3, 25, 2, 17)]
    kw = dict(rois=rois, bins={"vx": np.linspace(-0.3, 0.3, 13)}, min_size=3 if ndim == 3 else 0, spread="mean")
    fs = FlowStream(ndim, shape, series.dtype, 1, 1, 2, summary=SummarySpec(**kw, **D_KW), fields=False)
    try:
        pushed = 0
        for i in range(3):
            while pushed < min(i + 7 + fs.lookahead, len(series)):
                fs.push(series[pushed])
                pushed += 1
            p = fs.submit()
            s = p.summary()
            p.release()
            if ndim == 3:
                f = calc_flow3D(series[i:i + 7], 1, 1, 2)
            else:
                vx, vy, rel = calc_flow2D(series[i:i + 7], 1, 1, 2)
                f = (vx, vy, None, rel)
            want = flow_summary(*f, **kw, **D_KW)
            assert set(s) == set(want) and "std_vx" in s and ("phi_std" in s) == (ndim == 3)
            for k in want:
                if k in ("hist", "edges"):
                    assert all(bits_equal(s[k][q], want[k][q]) for q in want[k]), k
                else:
                    assert bits_equal(np.asarray(s[k]), np.asarray(want[k])), k
            assert np.all(want["std_magnitude"] > 0)
    finally:
        fs.close()


def test_process_flow_writes_the_spread_columns(tmp_path):
    series = np.random.default_rng(63).integers(0, 4096, size=(9, 6, 16, 20)).astype(np.uint16)
    kw = dict(rois=[(1, 5, 3, 14, 2, 17)], bins={"magnitude": np.linspace(0.0, 0.5, 11)}, spread="mean")
    tf.imwrite(tmp_path / "cells.tif", series, imagej=True)
    process_flow(str(tmp_path), "cells", "OneTif", 3, 1, 1, 2, summary=SummarySpec(**kw, **D_KW), save_fields=False)
    out = tmp_path / "OpticalFlow3D" / "cells"
    assert sorted(p.name for p in out.iterdir()) == ["cells_parameters.csv", "cells_summary.csv",
                                                    "cells_summary_hist.npz"]
    assert sorted(np.load(out / "cells_summary_hist.npz").files) == ["counts_magnitude", "edges_magnitude", "frames"]
    assert tuple(open(out / "cells_summary.csv").readline().strip().split(",")) == (analysis.CSV_COLUMNS
                                                                                   + analysis.CSV_SPREAD_COLUMNS)
    rows = analysis.read_summary_csv(str(out / "cells_summary.csv"))
    assert rows["frame"].size == 6
    for i in range(3):
        want = flow_summary(*calc_flow3D(series[i:i + 7], 1, 1, 2), **kw, **D_KW)
        sel = slice(2 * i, 2 * i + 2)
        for k in analysis._SPREAD_CSV_KEYS:  # floats written as repr read back as the same floats
            assert bits_equal(rows[k][sel], np.asarray(want[k], np.float64)), k
        for q, k in enumerate(spr.COMPONENTS):
            assert bits_equal(rows["spread_center_" + k][sel], want["spread_center"][:, q]), k
        assert bits_equal(rows["vcov_xy"][sel], want["velocity_covariance"][:, 0, 1])
        assert bits_equal(rows["sum_magnitude"][sel], want["sum_magnitude"])
