"""The two-channel comparison on the device (csrc/kt_ccl.hip: of3d_mask_open_pair,
csrc/kt_pair.hip: of3d_flow_pair) against the numpy restatement tests/pair_ref.py: the joint
opening exactly, the counts and histograms exactly, the 24 sums within the summation bound
(bitwise where any order is exact), consistency with the single-channel passes, determinism,
the workgroup partition and the resident route."""
import ctypes
import warnings

import numpy as np
import pytest

import pair_ref as pr
import summary_ref as sr
import whist_ref as wr
from conftest import bits_equal
from opticalflow3d_dev_amd import _lib, channel_compare, joint_reliability_mask, reliability_mask
from opticalflow3d_dev_amd.analysis import _PairCall

pytestmark = pytest.mark.gpu

SETTINGS = {"sparse": dict(rel_percentile=80, connectivity=6, min_size=5),   # 1107 components, 167 kept
            "one": dict(rel_percentile=40, connectivity=26, min_size=1)}      # one component of 6742 voxels


@pytest.fixture(scope="module")
def general():
    return pr.general_case()


def _open_ref(rel0, rel1, rois, rel_percentile, connectivity, min_size, floor=0.0, combine="or", thresholds=None):
    boxes = pr.boxes_of(rel0.shape, rois)
    t = pr.thresholds_of(rel0, rel1, rel_percentile) if thresholds is None else np.asarray(thresholds, rel0.dtype)
    keep, counts = pr.joint_open_ref(rel0, rel1, t[0], t[1], boxes, min_size, connectivity, floor, combine)
    return boxes, t, keep, counts


def _assert_opening(got, boxes, t, keep, counts):
    assert np.array_equal(got["rois"], boxes)
    assert got["thresholds"].dtype == t.dtype and got["thresholds"].tobytes() == t.tobytes()
    for k in pr.mr.COUNTS:
        assert got[k].dtype == np.int64 and np.array_equal(got[k], counts[k]), (k, got[k], counts[k])
    assert got["keep"].dtype == np.uint16 and np.array_equal(got["keep"], keep)
    assert np.array_equal(got["mask"](len(boxes) - 1), (keep >> np.uint16(len(boxes) - 1) & 1).astype(bool))


# ---- 1. the joint opening ---------------------------------------------------------------------------
@pytest.mark.parametrize("combine", ["or", "and"])
@pytest.mark.parametrize("setting", ["sparse", "one"])
def test_joint_opening_is_the_labelled_reference(general, setting, combine):
    rel0, rel1 = general[0][3], general[1][3]
    kw = dict(SETTINGS[setting], combine=combine)
    ref = _open_ref(rel0, rel1, pr.G_ROIS, **kw)
    if (setting, combine) == ("sparse", "or"):
        assert ref[3]["n_mask"].tolist() == [3272, 2824] and ref[3]["n_kept"].tolist() == [1896, 1663]
    assert np.all(ref[3]["n_mask"] > 0)
    _assert_opening(joint_reliability_mask(rel0, rel1, rois=pr.G_ROIS, **kw), *ref)


def test_joint_opening_float64_rel_floor_off_and_overlapping_rois(general):
    rel0, rel1 = general[0][3].astype(np.float64) ** 3, general[1][3].astype(np.float64) * 1.5  # not float32 values
    rois = [(0, 4, 2, 30, 3, 50), (1, 5, 10, 37, 30, 67)]
    for floor in (0.0, -np.inf, 0.2):
        kw = dict(rel_percentile=90, connectivity=6, min_size=4, floor=floor)
        ref = _open_ref(rel0, rel1, rois, **kw)
        both = ref[2][1:4, 10:30, 30:50]  # the boxes' overlap: some voxels are kept by one box only
        assert np.any((both >> 1 & 1) != (both >> 2 & 1))
        _assert_opening(joint_reliability_mask(rel0, rel1, rois=rois, **kw), *ref)
    assert ref[1].dtype == np.float64


@pytest.mark.parametrize("connectivity", [4, 8])
def test_joint_opening_2d(general, connectivity):
    rel0, rel1 = general[0][3][2], general[1][3][2]
    kw = dict(rel_percentile=75, connectivity=connectivity, min_size=4)
    ref = _open_ref(rel0, rel1, [(1, 36, 3, 64)], **kw)
    assert ref[3]["n_components"][0] > ref[3]["n_components_kept"][0] > 0
    _assert_opening(joint_reliability_mask(rel0, rel1, rois=[(1, 36, 3, 64)], **kw), *ref)


def test_a_nan_in_either_rel_fails_its_voxel(general):
    rel0, rel1 = general[0][3].copy(), general[1][3].copy()
    t = pr.thresholds_of(rel0, rel1, 40)
    rel0[2, 10, 20], rel1[3, 11, 21], rel0[1, 5, 5] = np.nan, np.nan, -np.inf
    for floor in (0.0, -np.inf):
        kw = dict(rel_percentile=40, connectivity=26, min_size=2, floor=floor, thresholds=[float(v) for v in t])
        ref = _open_ref(rel0, rel1, pr.G_ROIS, **kw)
        assert not ref[2][2, 10, 20] and not ref[2][3, 11, 21] and not ref[2][1, 5, 5]
        _assert_opening(joint_reliability_mask(rel0, rel1, rois=pr.G_ROIS, **kw), *ref)
    # through the percentile a channel with a NaN gets a NaN threshold: its test fails everywhere
    clean1 = general[1][3]
    got = joint_reliability_mask(rel0, clean1, 40, floor=-np.inf, connectivity=6, min_size=1)
    want = (clean1 > np.percentile(clean1, 40)) & ~np.isnan(rel0) & (rel0 > -np.inf)
    assert np.isnan(got["thresholds"][0]) and got["thresholds"][1] == np.percentile(clean1, 40)
    assert np.array_equal(got["mask"](0), want) and want.sum() == got["n_mask"][0] > 1000
    assert not joint_reliability_mask(rel0, clean1, 40, floor=-np.inf, combine="and")["keep"].any()


def test_equal_channels_without_floor_give_mask_open_bits(general):
    rel = general[0][3]
    for kw in (dict(connectivity=6, min_size=5), dict(connectivity=26, min_size=1)):
        one = reliability_mask(rel, 80, rois=pr.G_ROIS, **kw)
        for combine in ("or", "and"):
            two = joint_reliability_mask(rel, rel, 80, floor=-np.inf, combine=combine, rois=pr.G_ROIS, **kw)
            assert bits_equal(two["keep"], one["keep"])
            assert two["thresholds"].tolist() == [one["threshold"]] * 2
            assert all(np.array_equal(two[k], one[k]) for k in pr.mr.COUNTS)
    assert one["n_kept"][0] > 1000


def test_joint_opening_of_cuda_tensors_stays_on_the_device(general):
    import torch

    rel0, rel1 = general[0][3], general[1][3]
    ref = _open_ref(rel0, rel1, pr.G_ROIS, **SETTINGS["sparse"])
    got = joint_reliability_mask(torch.from_numpy(rel0).cuda(), torch.from_numpy(rel1).cuda(), rois=pr.G_ROIS,
                                 **SETTINGS["sparse"])
    assert got["keep"].is_cuda and np.array_equal(got["keep"].cpu().numpy(), ref[2])
    assert np.array_equal(got["mask"](1).cpu().numpy(), (ref[2] >> 1 & 1).astype(bool))
    assert np.array_equal(got["n_kept"], ref[3]["n_kept"])


# ---- 2. the pair summary, general case ------------------------------------------------------------------
def _pair_ref(ch0, ch1, rois, scales, bins, in_plane=False, **kw):
    boxes, t, keep, counts = _open_ref(ch0[3], ch1[3], rois, **kw)
    ref = pr.pair_ref(ch0, ch1, keep, boxes, *scales, bins=bins, in_plane=in_plane)
    sr.assert_clear_of_edges(ref, tuple(bins or ()))
    return ref, t, counts


def _assert_pair(got, ref, t, counts, **kw):
    pr.assert_matches(got, ref, **kw)
    assert got["thresholds"].tobytes() == t.tobytes()
    for k in pr.mr.COUNTS:
        assert np.array_equal(got[k], counts[k]), k


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_general_case(general, dtype):
    ch0, ch1 = ([a.astype(dtype) for a in c[:3]] + [c[3]] for c in general)
    ref, t, counts = _pair_ref(ch0, ch1, pr.G_ROIS, pr.G_SCALES, pr.G_BINS, **SETTINGS["sparse"])
    assert ref["n_valid"].tolist() == [1896, 1663]
    got = channel_compare(ch0, ch1, 80, *pr.G_SCALES, rois=pr.G_ROIS, bins=pr.G_BINS, min_size=5, connectivity=6)
    _assert_pair(got, ref, t, counts)
    assert got["hist"]["dot"][0].sum() < 1896 == got["hist"]["dtheta"][0].sum()  # the drop rule: dot beyond +-6
    # the derived values
    n = got["n_valid"].astype(np.float64)
    assert np.array_equal(got["mean_dot"], got["sum_dot"] / n) and np.array_equal(got["mean_diff"], got["sum_diff"] / n)
    assert np.array_equal(got["dtheta_mean"], np.arctan2(got["sum_sin_dtheta"] / n, got["sum_cos_dtheta"] / n))
    assert np.array_equal(got["ch1"]["theta_mean_weighted"],
                          np.arctan2(got["ch1"]["sum_mag_sin"] / n, got["ch1"]["sum_mag_cos"] / n))
    m0, m1 = (ref["values"][0]["ch_terms"][c]["sum_magnitude"] for c in (0, 1))
    assert abs(got["magnitude_correlation"][0] - np.corrcoef(m0, m1)[0, 1]) < 1e-12


def test_in_plane_mode_on_a_3d_volume(general):
    ch0, ch1 = general
    ref, t, counts = _pair_ref(ch0, ch1, pr.G_ROIS, pr.G_SCALES, pr.G_BINS, in_plane=True, **SETTINGS["one"])
    assert ref["n_valid"].tolist() == [6742, 5802]
    kw = dict(rois=pr.G_ROIS, bins=pr.G_BINS, min_size=1, connectivity=26)
    got = channel_compare(ch0, ch1, 40, *pr.G_SCALES, in_plane=True, **kw)
    _assert_pair(got, ref, t, counts)
    assert not got["ch0"]["sum_vz"].any() and not got["ch1"]["sum_vz"].any()
    flat = lambda c: (c[0], c[1], None, c[3])  # vz absent: the same mode
    again = channel_compare(flat(ch0), flat(ch1), 40, *pr.G_SCALES, in_plane=True, **kw)
    assert all(bits_equal(again[k], got[k]) for k in pr.PAIR_SUMS)
    full = channel_compare(ch0, ch1, 40, *pr.G_SCALES, **kw)
    assert np.all(full["ch0"]["sum_magnitude"] > got["ch0"]["sum_magnitude"])


def test_2d_fields(general):
    ch0, ch1 = ((c[0][1], c[1][1], None, c[3][1]) for c in general)
    rois = [(1, 36, 3, 64), (5, 6, 0, 67)]
    kw = dict(rel_percentile=60, connectivity=4, min_size=3)
    ref, t, counts = _pair_ref(ch0, ch1, rois, pr.G_SCALES, pr.G_BINS, **kw)
    assert ref["n_valid"][0] > 300 and ref["n_valid"][2] > 0
    got = channel_compare(ch0, ch1, 60, *pr.G_SCALES, rois=rois, bins=pr.G_BINS, min_size=3, connectivity=4)
    _assert_pair(got, ref, t, counts)


def test_empty_box_gives_nan_means_without_warnings(general):
    ch0, ch1 = general
    rel0 = ch0[3].copy()
    rel0[1:3, 4:9, 7:30] = -0.1  # below the floor: the box keeps nothing
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = channel_compare((*ch0[:3], rel0), ch1, 80, rois=[(1, 3, 4, 9, 7, 30)], bins=pr.G_BINS)
    assert got["n_valid"][1] == 0 and got["n_voxels"][1] == 2 * 5 * 23 and got["n_valid"][0] > 0
    for k in ("mean_dot", "mean_cosine", "dtheta_mean", "mean_diff", "magnitude_correlation"):
        assert np.isnan(got[k][1]) and not np.isnan(got[k][0]), k
    assert np.isnan(got["ch0"]["mean_magnitude"][1]) and np.isnan(got["ch1"]["theta_mean"][1])
    assert got["sum_dot"][1] == 0 and not any(h[1].any() for h in got["hist"].values())


# ---- 3. the exact case ----------------------------------------------------------------------------------
def test_exact_case_is_numpy_bit_for_bit():
    e0, e1 = pr.exact_case()
    kw = dict(rel_percentile=80, connectivity=26, min_size=1)
    ref, t, counts = _pair_ref(e0, e1, wr.EXACT_ROIS, (1.0, 1.0, 1.0), None, **kw)
    assert ref["n_valid"].tolist() == [2187, 1063, 31]
    got = channel_compare(e0, e1, 80, rois=wr.EXACT_ROIS)
    _assert_pair(got, ref, t, counts, bitwise=pr.EXACT_CH_SUMS + pr.EXACT_PAIR_SUMS)
    assert got["hist"] == {} and got["edges"] == {}


# ---- 4. consistency with what exists ----------------------------------------------------------------------
def _raw(ch0, ch1, stream=None, **kw):
    """The call and the raw device result words of one comparison on CUDA copies of the fields."""
    import torch

    dev = [[None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in c] for c in (ch0, ch1)]
    call = _PairCall(ch0[0].shape, dev[0][3].dtype, dev[0][3].device, **kw)
    ptrs = lambda c: tuple(None if a is None else a.data_ptr() for a in c)
    res = call.enqueue(ptrs(dev[0]), ptrs(dev[1]), ch0[0].dtype == np.float32,
                       stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return call, res.cpu().numpy(), dev


G_KW = dict(rel_percentile=80, xyscale=0.3, zscale=1.2, tscale=0.5, rois=pr.G_ROIS, min_size=5, connectivity=6)


def test_a_channel_against_itself(general):
    ch0 = general[0]
    got = channel_compare(ch0, ch0, 80, *pr.G_SCALES, rois=pr.G_ROIS, bins=pr.G_BINS, min_size=5, connectivity=6)
    n = got["n_valid"]
    assert np.all(n > 500)
    for k in sr.SUMS:
        assert got["ch0"][k].tobytes() == got["ch1"][k].tobytes(), k
    assert not got["sum_diff"].any() and not got["sum_sin_dtheta"].any()
    # every cosine is 1 to within an ulp or two of the divide and the roots: |t| <= 1 + 2^-50
    assert np.all(np.abs(got["sum_cosine"] - n) <= (n + 16) * 2.0 ** -53 * n * (1 + 2.0 ** -50))
    assert np.all(np.abs(got["sum_cos_dtheta"] - n) <= (n + 16) * 2.0 ** -53 * n * (1 + 2.0 ** -50))
    assert got["sum_mag0_mag1"].tobytes() == got["sum_mag0_sq"].tobytes() == got["sum_mag1_sq"].tobytes()
    assert got["hist"]["dmagnitude"][:, 16].tolist() == n.tolist()  # all in the bin [0, 0.5)
    assert np.all(np.abs(got["magnitude_correlation"] - 1) < 1e-12)


@pytest.mark.parametrize("shape", [pr.G_SHAPE, (9, 40, 131)])
def test_channel_block_is_flow_summary_masked_bit_for_bit(shape):
    """Normal deviates are never zero, so every kept voxel is valid in both channels: channel 0's
    sums must be those of the single-channel pass for the same keep (the same partition, the
    same per-thread order, the same trees)."""
    import torch

    ch0, ch1 = pr.general_case(seed=12, shape=shape)
    kw = dict(G_KW, rois=[(0, shape[0], 1, shape[1] - 1, 3, shape[2] - 3)])
    call, words, dev = _raw(ch0, ch1, **kw)
    lib, n_roi = _lib.load(), len(call.boxes)
    nb = (ctypes.c_int * 6)()
    res = torch.zeros(lib.of3d_flow_summary_result_bytes(n_roi, nb) // 8, dtype=torch.int64, device="cuda")
    ws = torch.empty(lib.of3d_flow_summary_workspace_bytes(), dtype=torch.uint8, device="cuda")
    pair = words[:n_roi * 26].reshape(n_roi, 26)
    for c in (0, 1):
        vx, vy, vz, rel = dev[c]
        _lib.check(lib.of3d_flow_summary_masked(
            vx.data_ptr(), vy.data_ptr(), vz.data_ptr(), rel.data_ptr(), 0, 0, *shape,
            call.result.data_ptr() + call.thresh_off + 8 * c, 0.3, 1.2, 0.5, call.roi_arr, n_roi, nb, None,
            res.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream, call.keep.data_ptr()))
        single = res.cpu().numpy()[8:8 + n_roi * 10].reshape(n_roi, 10)
        assert np.array_equal(single[:, 0], pair[:, 0]) and np.all(pair[:, 0] > 500)  # n_valid
        assert np.array_equal(single[:, 2:10], pair[:, 2 + 8 * c:10 + 8 * c]), c


# ---- 5. determinism ---------------------------------------------------------------------------------------
def test_same_bits_twice_and_independent_of_other_rois_and_histograms(general):
    ch0, ch1 = general
    rois = pr.G_ROIS + [(1, 4, 0, 37, 10, 11), (0, 5, 0, 37, 0, 67)]
    (c, a, _), (_, b, _) = (_raw(ch0, ch1, **dict(G_KW, rois=rois, bins=pr.G_BINS)) for _ in range(2))
    assert a.tobytes() == b.tobytes()
    ntot = sum(e.size - 1 for e in pr.G_BINS.values())
    many = a[:4 * (26 + ntot)].reshape(4, 26 + ntot)
    assert many[0].tobytes() == many[3].tobytes() and many[0, 0] == 1896  # the whole volume again, as the last box
    _, alone, _ = _raw(ch0, ch1, **dict(G_KW, rois=None, bins=pr.G_BINS))
    assert alone[:26 + ntot].tobytes() == many[0].tobytes()
    _, plain, _ = _raw(ch0, ch1, **dict(G_KW, rois=rois))
    assert plain[:4 * 26].reshape(4, 26).tobytes() == np.ascontiguousarray(many[:, :26]).tobytes()
    one = dict(G_KW, rois=rois, bins={"dtheta": pr.G_BINS["dtheta"]})
    _, d, _ = _raw(ch0, ch1, **one)
    d = d[:4 * 38].reshape(4, 38)  # dot 24 bins, cosine 20, then dtheta's 12
    assert d[:, 26:].tobytes() == np.ascontiguousarray(many[:, 26 + 44:26 + 56]).tobytes()


# ---- 6. the partition and the final pass ---------------------------------------------------------------------
def test_six_workgroups_with_a_ragged_tail():
    ch0, ch1 = pr.general_case(seed=21, shape=(9, 40, 131))  # 47160 voxels: 6 workgroups of 60 rows
    rois = [(1, 9, 0, 39, 2, 131)]
    kw = dict(rel_percentile=70, connectivity=18, min_size=2)
    ref, t, counts = _pair_ref(ch0, ch1, rois, pr.G_SCALES, pr.G_BINS, **kw)
    assert ref["n_valid"][0] > 10000
    got = channel_compare(ch0, ch1, 70, *pr.G_SCALES, rois=rois, bins=pr.G_BINS, min_size=2, connectivity=18)
    _assert_pair(got, ref, t, counts)


def test_the_maximum_of_1024_workgroups():
    """(64, 256, 512) = 1024 x 8192 voxels, in-plane float32 fields, the whole volume, min_size 1
    (keep = the mask itself: no labelling needed for the reference)."""
    shape = (64, 256, 512)
    rng = np.random.default_rng(33)
    rel0, rel1 = pr.rel_pair(shape, rng)
    v = [rng.standard_normal(shape, dtype=np.float32) for _ in range(4)]
    ch0, ch1 = (v[0], v[1], None, rel0), (v[2], v[3], None, rel1)
    t = pr.thresholds_of(rel0, rel1, 99)
    keep = pr.joint_mask(rel0, rel1, t[0], t[1]).astype(np.uint16)
    bins = {"cosine": np.linspace(-1.001, 1.001, 8), "dtheta": np.linspace(-np.pi, np.pi, 6)}
    ref = pr.pair_ref(ch0, ch1, keep, pr.boxes_of(shape, None), *pr.G_SCALES, bins=bins, in_plane=True)
    sr.assert_clear_of_edges(ref, tuple(bins))
    assert 100000 < ref["n_valid"][0] == int(keep.sum())
    got = channel_compare(ch0, ch1, 99, *pr.G_SCALES, bins=bins, in_plane=True, connectivity=6)
    pr.assert_matches(got, ref)
    assert got["thresholds"].tobytes() == t.tobytes()
    assert got["n_mask"][0] == got["n_kept"][0] == ref["n_valid"][0] and got["n_voxels"][0] == 1024 * 8192


# ---- 7. the resident route -----------------------------------------------------------------------------------
def test_resident_tensors_on_a_side_stream_give_channel_compare_bits(general):
    import torch

    ch0, ch1 = general
    want = channel_compare(ch0, ch1, 80, *pr.G_SCALES, rois=pr.G_ROIS, bins=pr.G_BINS, min_size=5, connectivity=6)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        call, words, _ = _raw(ch0, ch1, stream=side.cuda_stream, **dict(G_KW, bins=pr.G_BINS))
    got = call.decode(words)
    assert set(got) == set(want)
    for k in want:
        if k in ("ch0", "ch1", "hist", "edges"):
            assert set(got[k]) == set(want[k]) and all(bits_equal(got[k][q], want[k][q]) for q in want[k]), k
        else:
            assert bits_equal(np.asarray(got[k]), np.asarray(want[k])), k
    assert np.array_equal(call.keep.cpu().numpy() & 1, _open_ref(ch0[3], ch1[3], None, **SETTINGS["sparse"])[2] & 1)


def test_two_flowstreams_feed_the_pair_call_from_their_resident_outputs():
    """INTEGRATION §1's snippet: nothing full-size leaves the device."""
    import torch

    from opticalflow3d_dev_amd import SummarySpec, calc_flow3D
    from opticalflow3d_dev_amd.stream import FlowStream

    shape = (6, 16, 20)
    series = [np.random.default_rng(70 + c).integers(0, 4096, size=(9,) + shape).astype(np.uint16) for c in (0, 1)]
    kw = dict(rel_percentile=60, xyscale=0.1, zscale=0.3, tscale=2.0, rois=[(1, 5, 3, 14, 2, 17)],
              bins={"dtheta": np.linspace(-np.pi, np.pi, 13), "cosine": np.linspace(-1.0001, 1.0001, 9)},
              min_size=3, connectivity=6)
    fss = [FlowStream(3, shape, np.uint16, 1, 1, 2, summary=SummarySpec(), fields=False) for _ in (0, 1)]
    fs0, fs1 = fss
    try:
        call = _PairCall(shape, torch.float32, fs0.dev, **kw)
        pushed = 0
        for i in range(2):
            while pushed < min(i + 7 + fs0.lookahead, 9):
                for fs, frames in zip(fss, series):
                    fs.push(frames[pushed])
                pushed += 1
            p0, p1 = fs0.submit(), fs1.submit()
            ptrs = lambda fs, p: tuple(t.data_ptr() for t in fs.dout[p.b])
            fs0.comp.wait_stream(fs1.comp)
            words = call.enqueue(ptrs(fs0, p0), ptrs(fs1, p1), fs0.precision == "fp32", fs0.comp.cuda_stream)
            with torch.cuda.stream(fs0.comp):
                host = words.cpu()
            fs1.comp.wait_stream(fs0.comp)
            got = call.decode(host.numpy())
            p0.release(), p1.release()
            want = channel_compare(calc_flow3D(series[0][i:i + 7], 1, 1, 2), calc_flow3D(series[1][i:i + 7], 1, 1, 2),
                                   **kw)
            assert want["n_valid"][0] > 100
            for k in ("n_valid", "thresholds", "n_kept") + pr.PAIR_SUMS:
                assert bits_equal(np.asarray(got[k]), np.asarray(want[k])), (i, k)
            assert all(bits_equal(got["ch1"][k], want["ch1"][k]) for k in sr.SUMS)
            assert all(bits_equal(got["hist"][k], want["hist"][k]) for k in want["hist"])
    finally:
        for fs in fss:
            fs.close()


# ---- 8. bad input --------------------------------------------------------------------------------------------
def test_bad_input_raises_before_anything_is_launched(general):
    ch0, ch1 = general
    with pytest.raises(ValueError, match="ROI 1"):
        channel_compare(ch0, ch1, rois=[(0, 6, 0, 37, 0, 67)])
    with pytest.raises(ValueError, match="ascending"):
        channel_compare(ch0, ch1, bins={"dot": [0.0, 0.0, 1.0]})
    with pytest.raises(ValueError, match="unknown pair histogram quantity"):
        channel_compare(ch0, ch1, bins={"phi": [0.0, 1.0]})
    with pytest.raises(ValueError, match="shape"):
        channel_compare(ch0, tuple(a[:, :, :66] for a in ch1))
    with pytest.raises(ValueError, match="shape"):
        channel_compare(ch0, (ch1[0][:4], *ch1[1:]))
    with pytest.raises(TypeError, match="float"):
        channel_compare(ch0, (ch1[0].astype(np.float32), *ch1[1:]))
    with pytest.raises(TypeError, match="rel"):
        channel_compare(ch0, (*ch1[:3], ch1[3].astype(np.float64)))
    with pytest.raises(ValueError, match="vz"):
        channel_compare(ch0, (ch1[0], ch1[1], None, ch1[3]))
    with pytest.raises(ValueError, match="in_plane"):
        channel_compare((ch0[0], ch0[1], None, ch0[3]), (ch1[0], ch1[1], None, ch1[3]))
    with pytest.raises(ValueError, match="combine"):
        channel_compare(ch0, ch1, combine="xor")
    with pytest.raises(ValueError, match="connectivity"):
        joint_reliability_mask(ch0[3], ch1[3], connectivity=8)
    with pytest.raises(ValueError, match="shape"):
        joint_reliability_mask(ch0[3], ch1[3][:4])
    with pytest.raises(TypeError, match="float"):
        joint_reliability_mask(ch0[3], ch1[3].astype(np.float16))
