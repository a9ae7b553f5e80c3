"""Magnitude-weighted histograms of the device-side frame summary (csrc/kt_whist.hip:
of3d_flow_whist) against the numpy restatement tests/whist_ref.py: bitwise on fields whose
magnitudes sum exactly in any order, within the per-bin sum bound on general fields;
determinism, the lane patterns of the accumulation, the opened mask, dtypes and the drivers."""
import warnings

import numpy as np
import pytest

import mask_ref as mr
import summary_ref as sr
import whist_ref as wr
from conftest import bits_equal
from opticalflow3d_dev_amd import SummarySpec, calc_flow2D, calc_flow3D, flow_summary, process_flow
from opticalflow3d_dev_amd import tiff as tf
from opticalflow3d_dev_amd.analysis import _SummaryCall

pytestmark = pytest.mark.gpu


def assert_bitwise(got, ref, names):
    """flow_summary's weighted histograms against whist_ref's, bit for bit."""
    assert np.array_equal(got["n_valid"], ref["n_valid"]), (got["n_valid"], ref["n_valid"])
    assert sorted(got["hist_weighted"]) == sorted(names) == sorted(got["edges_weighted"])
    for k in names:
        g, w = got["hist_weighted"][k], ref["hist_weighted"][k]
        assert g.dtype == np.float64 and g.shape == w.shape, k
        assert g.tobytes() == w.tobytes(), (k, g, w)
        assert np.array_equal(got["edges_weighted"][k], ref["edges_weighted"][k])


# ---- 1. the exact case: any summation order gives numpy's bits ------------------------------------
@pytest.fixture(scope="module")
def exact():
    f = wr.exact_case()
    return f, wr.whist_ref(*f, 50, rois=wr.EXACT_ROIS, weighted_bins=wr.EXACT_BINS)


def test_exact_case_is_numpy_bit_for_bit(exact):
    f, ref = exact
    assert ref["n_valid"].tolist() == [4221, 2083, 53]  # two workgroups with a ragged tail; mostly idle waves
    got = flow_summary(*f, 50, rois=wr.EXACT_ROIS, weighted_bins=wr.EXACT_BINS)
    assert_bitwise(got, ref, ("phi", "theta", "magnitude"))
    for k in wr.EXACT_BINS:  # every valid voxel lies in a bin: nothing lost, nothing doubled
        assert got["hist_weighted"][k].sum(axis=1).tobytes() == got["sum_magnitude"].tobytes(), k
    assert got["hist"] == {} and got["edges"] == {}


# ---- 2. the general case ---------------------------------------------------------------------------
G_SHAPE, G_SCALES, G_ROIS = (5, 37, 67), (0.3, 1.2, 0.5), [(0, 5, 1, 36, 3, 64)]
G_BINS = {"phi": np.linspace(-np.pi / 2, np.pi / 2, 37), "vx": np.linspace(-3, 3, 257)}


@pytest.mark.parametrize("seed", [100, 101, 102, 103])
def test_general_case_within_the_per_bin_bound(seed):
    rng = np.random.default_rng(seed)
    f = [rng.standard_normal(G_SHAPE) for _ in range(3)] + [rng.random(G_SHAPE, dtype=np.float32)]
    plain_bins = {"theta": np.linspace(-np.pi, np.pi, 9), "magnitude": np.linspace(0, 4, 17)}
    ref = wr.whist_ref(*f, 60, *G_SCALES, rois=G_ROIS, weighted_bins=G_BINS)
    sr.assert_clear_of_edges(wr.with_bins(ref, G_BINS), tuple(G_BINS))
    got = flow_summary(*f, 60, *G_SCALES, rois=G_ROIS, bins=plain_bins, weighted_bins=G_BINS)
    assert np.array_equal(got["n_valid"], ref["n_valid"]) and ref["n_valid"][1] > 1000
    for k in G_BINS:
        err, bound = np.abs(got["hist_weighted"][k] - ref["fsum_weighted"][k]), wr.bin_bound(ref, k)
        print(k, "max err / bound:", float(np.max(err / np.maximum(bound, 1e-300))))
        assert np.all(err <= bound), (k, err, bound)
        assert np.all((got["hist_weighted"][k] == 0) == (ref["count_weighted"][k] == 0)), k
    # the plain histograms and the eight sums are those of a call without weighted_bins
    plain = flow_summary(*f, 60, *G_SCALES, rois=G_ROIS, bins=plain_bins)
    assert set(got) - set(plain) == {"hist_weighted", "edges_weighted"}
    for k in plain:
        if k in ("hist", "edges"):
            assert all(bits_equal(got[k][q], plain[k][q]) for q in plain[k]), k
        else:
            assert bits_equal(np.asarray(got[k]), np.asarray(plain[k])), k


# ---- 3. determinism ----------------------------------------------------------------------------------
def _raw(fields, spec):
    """The call and the raw device result words of one summary call."""
    import torch

    dev = [torch.from_numpy(a).cuda() for a in fields]
    call = _SummaryCall(spec, fields[0].shape, dev[-1].dtype, dev[0].device)
    res = call.new_result(dev[0].device)
    call.enqueue((dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), False), res.data_ptr(),
                 torch.cuda.current_stream().cuda_stream)
    return call, res.cpu().numpy()


def test_same_bits_twice_and_independent_of_other_rois_and_quantities():
    rng = np.random.default_rng(7)
    f = [rng.standard_normal(G_SHAPE) for _ in range(3)] + [rng.random(G_SHAPE, dtype=np.float32)]
    six = dict(G_BINS, vy=np.linspace(-2, 2, 11), vz=np.linspace(-5, 5, 6), magnitude=np.linspace(0, 6, 31),
               theta=np.linspace(-np.pi, np.pi, 13))
    kw = dict(rel_percentile=60, xyscale=0.3, zscale=1.2, tscale=0.5)
    rois = G_ROIS + [(1, 4, 0, 37, 10, 11), (0, 5, 0, 37, 0, 67)]
    (c, a), (_, b) = (_raw(f, SummarySpec(rois=rois, weighted_bins=six, **kw)) for _ in range(2))
    assert a.tobytes() == b.tobytes()
    block = lambda call, words: words[call.whist_off // 8:].reshape(len(call.boxes), -1)
    many = block(c, a)
    assert many.shape == (4, 1 + sum(e.size - 1 for e in six.values()))
    assert many[0].tobytes() == many[3].tobytes()  # the whole volume again, as the last box
    c1, alone = _raw(f, SummarySpec(weighted_bins=six, **kw))
    assert block(c1, alone)[0].tobytes() == many[0].tobytes()
    # one quantity alone: the same bits as among six (the order is QUANTITIES')
    off = 1
    for name in ("vx", "vy", "vz", "magnitude", "theta", "phi"):
        n = six[name].size - 1
        c2, one = _raw(f, SummarySpec(rois=rois, weighted_bins={name: six[name]}, **kw))
        assert block(c2, one)[:, 1:].tobytes() == np.ascontiguousarray(many[:, off:off + n]).tobytes(), name
        assert np.array_equal(block(c2, one)[:, 0], many[:, 0])
        off += n


# ---- 4. lane patterns of the accumulation ------------------------------------------------------------
def _ramp_fields(shape, ndim):
    """Voxel i (C order) holds k = i % 256 + 1 times a quadruple / triple: vx = k or 3k, an
    integer magnitude, so consecutive voxels — the lanes of a wave — differ in vx."""
    k = (np.arange(int(np.prod(shape))) % 256 + 1).astype(np.float64).reshape(shape)
    rel = np.ones(shape, np.float32)
    rel.flat[-1] = 0.0  # percentile 0: everything but this voxel passes
    return ([k, 2 * k, 2 * k] if ndim == 3 else [3 * k, 4 * k, None]) + [rel]


def test_64_lanes_in_64_bins_and_all_lanes_in_one_bin():
    f = _ramp_fields((3, 40, 256), 3)
    bins = {"vx": np.arange(257) + 0.5, "magnitude": np.array([0.0, 1000.0]), "vy": np.array([0.0, 300.0, 600.0])}
    rois = [(0, 3, 0, 40, 0, 64), (1, 2, 3, 4, 0, 256)]
    ref = wr.whist_ref(*f, 0, rois=rois, weighted_bins=bins)
    assert ref["n_valid"].tolist() == [3 * 40 * 256 - 1, 3 * 40 * 64, 256]
    assert np.all(ref["count_weighted"]["vx"][0] >= 119) and np.all(ref["count_weighted"]["vx"][2] == 1)
    assert np.count_nonzero(ref["count_weighted"]["vx"][1]) == 64
    got = flow_summary(*f, 0, rois=rois, weighted_bins=bins)
    assert_bitwise(got, ref, ("vx", "vy", "magnitude"))
    assert got["hist_weighted"]["magnitude"][:, 0].tobytes() == got["sum_magnitude"].tobytes()


def test_two_long_rows_and_boxes_narrower_than_a_wave():
    """(2, 20000) in 2D: 5 workgroups by size, capped at the 2 rows; then boxes of 1 to 3 columns."""
    f = _ramp_fields((2, 20000), 2)
    bins = {"vx": np.arange(0, 257 * 3, 3) + 1.5, "theta": np.array([-np.pi, 0.0, np.pi])}
    rois = [(0, 2, 7, 10), (1, 2, 19999, 20000), (0, 2, 0, 63), (0, 1, 1, 20000)]
    ref = wr.whist_ref(*f, 0, rois=rois, weighted_bins=bins)
    assert ref["n_valid"].tolist() == [39999, 6, 0, 126, 19999]
    got = flow_summary(*f, 0, rois=rois, weighted_bins=bins)
    assert_bitwise(got, ref, ("vx", "theta"))
    assert not got["hist_weighted"]["vx"][2].any()


# ---- 5. the masked route ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blobs():
    """Exact velocities under a smooth reliability, so the mask has components of many sizes."""
    from scipy import ndimage

    shape = (8, 30, 70)
    rng = np.random.default_rng(31)
    rel = ndimage.gaussian_filter(rng.standard_normal(shape), 1.5).astype(np.float32)
    return wr.exact_fields(shape, rng) + [rel]


M_ROIS = [(0, 8, 2, 28, 3, 50), (1, 7, 10, 30, 30, 70)]  # overlapping: each uses its own bit of keep
M_BINS = {"magnitude": wr.EXACT_BINS["magnitude"], "phi": wr.EXACT_BINS["phi"]}


def test_min_size_1_has_the_unmasked_bits(blobs):
    plain = flow_summary(*blobs, 70, rois=M_ROIS, weighted_bins=M_BINS)
    for extra in (dict(min_size=1), dict(min_size=1, connectivity=6)):
        got = flow_summary(*blobs, 70, rois=M_ROIS, weighted_bins=M_BINS, **extra)
        for k in M_BINS:
            assert got["hist_weighted"][k].tobytes() == plain["hist_weighted"][k].tobytes(), k
    assert np.all(plain["n_valid"] > 100)


def test_opened_mask_against_the_labelled_reference(blobs):
    vx, vy, vz, rel = blobs
    boxes, thresh = mr.boxes_of(vx.shape, M_ROIS), np.percentile(rel, 80)
    keep, counts = mr.open_ref(rel, thresh, boxes, 20, 18)
    assert np.all(counts["n_components_kept"] > 0) and np.all(counts["n_components"] > counts["n_components_kept"])
    both = keep[1:7, 10:28, 30:50]  # the boxes' overlap: some voxels are kept by one box only
    assert np.any((both >> 1 & 1) != (both >> 2 & 1))
    masked = mr.summary_ref_masked(vx, vy, vz, keep, thresh, boxes)
    ref = wr.whist_ref(None, None, None, None, ref=masked, weighted_bins=M_BINS)
    sr.assert_clear_of_edges(wr.with_bins(ref, M_BINS), tuple(M_BINS))
    got = flow_summary(vx, vy, vz, rel, 80, rois=M_ROIS, weighted_bins=M_BINS, min_size=20, connectivity=18)
    assert np.array_equal(got["n_kept"], counts["n_kept"]) and np.all(got["n_kept"] < got["n_mask"])
    assert_bitwise(got, ref, ("magnitude", "phi"))


# ---- 6. dtypes and dimensions ------------------------------------------------------------------------
def test_float32_fields_and_float64_rel(exact):
    (vx, vy, vz, rel), _ = exact
    f = [a.astype(np.float32) for a in (vx, vy, vz)] + [rel.astype(np.float64)]  # the values are exact in float32
    ref = wr.whist_ref(*f, 50, rois=wr.EXACT_ROIS, weighted_bins=wr.EXACT_BINS)
    assert_bitwise(flow_summary(*f, 50, rois=wr.EXACT_ROIS, weighted_bins=wr.EXACT_BINS), ref, tuple(wr.EXACT_BINS))


def test_2d_frame_empty_roi_and_nan_threshold():
    rng = np.random.default_rng(9)
    vx, vy = wr.exact_fields((33, 45), rng, ndim=2)
    rel = rng.random((33, 45))
    rel[4:6, 7:10] = 0.0  # a box below any positive threshold: no valid voxel
    bins = {"theta": np.linspace(-np.pi, np.pi, 11) + 0.01, "magnitude": np.array([0.0, 4.0, 16.0, 128.0])}
    rois = [(4, 6, 7, 10), (0, 33, 44, 45)]
    ref = wr.whist_ref(vx, vy, None, rel, 50, rois=rois, weighted_bins=bins)
    assert ref["n_valid"][1] == 0 and ref["n_valid"][2] > 0
    sr.assert_clear_of_edges(wr.with_bins(ref, bins), ("theta",))
    got = flow_summary(vx, vy, None, rel, 50, rois=rois, weighted_bins=bins)
    assert_bitwise(got, ref, ("theta", "magnitude"))
    assert not got["hist_weighted"]["theta"][1].any() and not got["hist_weighted"]["magnitude"][1].any()
    with pytest.raises(ValueError, match="3D"):
        flow_summary(vx, vy, None, rel, 50, weighted_bins={"phi": [0.0, 1.0]})
    rel[0, 0] = np.nan  # a NaN threshold: nothing is valid
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = flow_summary(vx, vy, None, rel, 50, rois=rois, weighted_bins=bins)
    assert np.isnan(got["threshold"]) and got["n_valid"].tolist() == [0, 0, 0]
    assert all(h.shape == (3, e.size - 1) and not h.any() for h, e in ((got["hist_weighted"][k], bins[k]) for k in bins))


# ---- 7. the drivers ----------------------------------------------------------------------------------
D_KW = dict(rel_percentile=70, xyscale=0.1, zscale=0.3, tscale=2.0)


def _same_weighted(a, b):
    assert set(a) == set(b)
    for k in ("hist_weighted", "edges_weighted", "hist"):
        assert set(a[k]) == set(b[k]) and all(bits_equal(a[k][q], b[k][q]) for q in a[k]), k
    for k in ("n_valid", "sum_magnitude", "threshold"):
        assert bits_equal(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.mark.parametrize("ndim", [2, 3])
def test_flowstream_gives_flow_summary_bits_per_frame(ndim):
    from opticalflow3d_dev_amd.stream import FlowStream

    shape = (6, 16, 20) if ndim == 3 else (30, 26)
    series = np.random.default_rng(60 + ndim).integers(0, 4096, size=(9,) + shape).astype(np.uint16)
    wb = {"magnitude": np.linspace(0.0, 0.5, 11), "theta": np.linspace(-np.pi, np.pi, 13)}
    rois = [(1, 5, 3, 14, 2, 17)] if ndim == 3 else [(3, 25, 2, 17)]
    if ndim == 3:
        wb["phi"] = np.linspace(-np.pi / 2, np.pi / 2, 37)
    kw = dict(rois=rois, bins={"vx": np.linspace(-0.3, 0.3, 13)}, weighted_bins=wb, min_size=3 if ndim == 3 else 0)
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
            _same_weighted(s, want)
            assert want["hist_weighted"]["magnitude"][0].sum() > 0
    finally:
        fs.close()


def test_process_flow_writes_the_weights(tmp_path):
    series = np.random.default_rng(63).integers(0, 4096, size=(9, 6, 16, 20)).astype(np.uint16)
    wb = {"phi": np.linspace(-np.pi / 2, np.pi / 2, 37), "magnitude": np.linspace(0.0, 0.5, 11)}
    kw = dict(rois=[(1, 5, 3, 14, 2, 17)], bins={"magnitude": np.linspace(0.0, 0.5, 11)}, weighted_bins=wb)
    tf.imwrite(tmp_path / "cells.tif", series, imagej=True)
    process_flow(str(tmp_path), "cells", "OneTif", 3, 1, 1, 2, summary=SummarySpec(**kw, **D_KW), save_fields=False)
    out = tmp_path / "OpticalFlow3D" / "cells"
    assert sorted(p.name for p in out.iterdir()) == ["cells_parameters.csv", "cells_summary.csv",
                                                    "cells_summary_hist.npz"]
    npz = np.load(out / "cells_summary_hist.npz")
    assert sorted(npz.files) == ["counts_magnitude", "edges_magnitude", "frames", "wedges_magnitude", "wedges_phi",
                                 "weights_magnitude", "weights_phi"]
    assert npz["weights_phi"].shape == (3, 2, 36) and npz["weights_phi"].dtype == np.float64
    for i in range(3):
        want = flow_summary(*calc_flow3D(series[i:i + 7], 1, 1, 2), **kw, **D_KW)
        for k in wb:
            assert npz["weights_" + k][i].tobytes() == want["hist_weighted"][k].tobytes(), k
            assert np.array_equal(npz["wedges_" + k], wb[k])
        assert np.array_equal(npz["counts_magnitude"][i], want["hist"]["magnitude"])
