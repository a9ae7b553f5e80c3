"""Quiver samples on the device (csrc/kt_quiver.hip: of3d_quiver_sample) against the numpy
restatement tests/quiver_ref.py.  Every comparison is exact: the coordinates by array_equal, the
velocities bit for bit (they are copies through non-fused multiplies and divides)."""
import numpy as np
import pytest

import mask_ref as mr
import quiver_ref as qr
from opticalflow3d_dev_amd import QuiverSpec, quiver_sample
from opticalflow3d_dev_amd.analysis import _QuiverCall

pytestmark = pytest.mark.gpu

SCALES = dict(xyscale=0.3, zscale=1.2, tscale=0.5)


def assert_same(got, ref, capacity=None):
    """quiver_sample's dict against quiver_ref's, record for record; capacity: per ROI, where the
    device's blocks were smaller than the reference's lists."""
    assert got["threshold"].dtype == np.asarray(ref["threshold"]).dtype
    assert got["threshold"] == ref["threshold"] or (np.isnan(got["threshold"]) and np.isnan(ref["threshold"]))
    assert np.array_equal(got["rois"], ref["rois"]) and tuple(got["gap"]) == tuple(ref["gap"])
    assert len(got["samples"]) == len(ref["samples"])
    for r, (g, w) in enumerate(zip(got["samples"], ref["samples"])):
        if capacity is not None:
            w = qr.truncated(w, capacity[r])
        assert g["n_lattice"] == w["n_lattice"] and g["n_valid"] == w["n_valid"], (r, g["n_valid"], w["n_valid"])
        assert g["truncated"] == (w["n_valid"] > len(w["zyx"])), r
        assert g["zyx"].dtype == np.int64 and g["zyx"].shape == w["zyx"].shape, (r, g["zyx"].shape, w["zyx"].shape)
        assert np.array_equal(g["zyx"], w["zyx"]), r
        assert g["v"].dtype == np.float64 and g["v"].shape == w["v"].shape, r
        assert g["v"].tobytes() == w["v"].tobytes(), r
        vx, vy, vz = g["v"].T
        assert g["magnitude"].tobytes() == np.sqrt(np.power(vx, 2) + np.power(vy, 2) + np.power(vz, 2)).tobytes()
        assert g["theta"].tobytes() == np.arctan2(vy, vx).tobytes()


def assert_not_vacuous(ref, rois=None):
    for r in (range(len(ref["samples"])) if rois is None else rois):
        s = ref["samples"][r]
        assert 0 < s["n_valid"] < s["n_lattice"], (r, s["n_valid"], s["n_lattice"])


# ---- 1. the seams of the partition --------------------------------------------------------------------
@pytest.mark.parametrize("shape,gap,rois,lattice0", [
    ((6, 50, 301), (1, 2, 3), [(1, 5, 3, 47, 7, 290)], 6 * 25 * 101),  # two workgroups, ragged rows (101 % 64)
    ((5, 40, 300), 1, [(1, 4, 5, 40, 11, 299)], 60000),  # eight workgroups
    ((2, 3, 70), 1, [(0, 2, 1, 3, 3, 70)], 420),  # one workgroup, 52.5 points per wave: sub-runs partly empty
    ((3, 7, 5), (2, 3, 2), [(0, 3, 1, 7, 0, 5)], 2 * 3 * 3),  # fewer points than waves: empty sub-runs
])
def test_partition_seams(shape, gap, rois, lattice0):
    f = qr.planted_fields(shape, 21)
    ref = qr.quiver_ref(*f, 60, **SCALES, gap=gap, rois=rois)
    assert ref["samples"][0]["n_lattice"] == lattice0
    assert_not_vacuous(ref)
    assert_same(quiver_sample(*f, 60, **SCALES, gap=gap, rois=rois), ref)


def test_gap_larger_than_the_box_gives_one_point_per_axis():
    f = qr.planted_fields((4, 9, 11), 22)
    for a in f[:3]:
        a[0, 0, 0] = 1.5  # the whole volume's single lattice point is valid ...
    f[3][0, 0, 0] = 2.0
    f[0][1, 2, 3] = 0.0  # ... and the ROI's is not
    rois = [(1, 4, 2, 9, 3, 11), (2, 3, 4, 5, 6, 7)]
    ref = qr.quiver_ref(*f, 60, **SCALES, gap=(100, 9, 11), rois=rois)
    assert [s["n_lattice"] for s in ref["samples"]] == [1, 1, 1]
    assert [s["n_valid"] for s in ref["samples"]][:2] == [1, 0] and ref["samples"][0]["zyx"].tolist() == [[0, 0, 0]]
    assert_same(quiver_sample(*f, 60, **SCALES, gap=(100, 9, 11), rois=rois), ref)


# ---- 2. dtypes and dimensions -------------------------------------------------------------------------
def test_float32_fields_and_float64_rel():
    f = qr.planted_fields((5, 21, 67), 23, v_dtype=np.float32, rel_dtype=np.float64)
    rois = [(1, 5, 3, 20, 7, 60)]
    ref = qr.quiver_ref(*f, 70, **SCALES, gap=(1, 2, 2), rois=rois)
    assert_not_vacuous(ref)
    got = quiver_sample(*f, 70, **SCALES, gap=(1, 2, 2), rois=rois)
    assert got["threshold"].dtype == np.float64
    assert_same(got, ref)


@pytest.mark.parametrize("shape,gap,rois", [
    ((33, 45), (2, 3), [(3, 25, 2, 17), (32, 33, 0, 45)]),
    ((2, 20000), 1, [(1, 2, 19990, 20000)]),  # 5 workgroups by size, capped at the 2 rows
    ((2, 20000), (1, 7), [(0, 2, 3, 19999)]),
])
def test_2d(shape, gap, rois):
    f = qr.planted_fields(shape, 24, rel_dtype=np.float64)
    ref = qr.quiver_ref(*f, 50, xyscale=0.3, tscale=0.5, gap=gap, rois=rois)
    assert_not_vacuous(ref)
    got = quiver_sample(*f, 50, xyscale=0.3, tscale=0.5, gap=gap, rois=rois)
    assert_same(got, ref)
    for s in got["samples"]:
        assert "phi" not in s and not s["v"][:, 2].any() and not s["zyx"][:, 0].any()
        assert np.all(np.signbit(s["v"][:, 2]) == 0)  # vz is +0.0
    with pytest.raises(ValueError, match="2 integers"):
        quiver_sample(*f, 50, gap=(1, 2, 3))


def test_torch_input_stays_on_the_device_and_matches_numpy_input():
    import torch

    f = qr.planted_fields((4, 20, 70), 25)
    a = quiver_sample(*f, 60, **SCALES, gap=2)
    b = quiver_sample(*(torch.from_numpy(x).cuda() for x in f), 60, **SCALES, gap=2)
    assert_same(b, a)
    assert_same(a, qr.quiver_ref(*f, 60, **SCALES, gap=2))


# ---- 3. NaN in rel, and the extremes ---------------------------------------------------------------------
def test_nan_in_rel_with_a_given_threshold():
    f = qr.planted_fields((4, 20, 70), 26)
    f[3].reshape(-1)[::5] = np.nan
    ref = qr.quiver_ref(*f, **SCALES, gap=(1, 1, 2), threshold=0.4)
    assert_not_vacuous(ref)
    nan_lattice = np.isnan(f[3][:, :, ::2])
    assert nan_lattice.any() and not nan_lattice.all()
    got = quiver_sample(*f, **SCALES, gap=(1, 1, 2), threshold=0.4)
    assert_same(got, ref)
    assert not np.isnan(f[3][tuple(got["samples"][0]["zyx"].T)]).any()
    # the percentile of a field with a NaN is NaN, and nothing passes a NaN threshold
    got = quiver_sample(*f, 60, **SCALES, gap=(1, 1, 2))
    assert np.isnan(got["threshold"]) and got["samples"][0]["n_valid"] == 0 and got["samples"][0]["zyx"].shape == (0, 3)


def test_percentile_100_stores_nothing():
    f = qr.planted_fields((4, 20, 70), 27)
    rois = [(1, 3, 2, 19, 5, 66)]
    ref = qr.quiver_ref(*f, 100, **SCALES, gap=2, rois=rois)
    assert [s["n_valid"] for s in ref["samples"]] == [0, 0] and ref["samples"][0]["n_lattice"] == 2 * 10 * 35
    got = quiver_sample(*f, 100, **SCALES, gap=2, rois=rois)
    assert_same(got, ref)
    assert all(s["zyx"].shape == (0, 3) and s["v"].shape == (0, 3) and not s["truncated"] for s in got["samples"])


def test_threshold_minus_inf_keeps_every_nonzero_lattice_voxel():
    f = qr.planted_fields((4, 20, 70), 28)
    ref = qr.quiver_ref(*f, **SCALES, gap=(2, 1, 3), threshold=-np.inf)
    sl = (slice(None, None, 2), slice(None), slice(None, None, 3))
    clean = np.ones(f[0][sl].shape, bool)
    for a in f[:3]:
        clean &= (a[sl] != 0) & ~np.isnan(a[sl])
    assert ref["samples"][0]["n_valid"] == clean.sum() and 0 < clean.sum() < clean.size
    got = quiver_sample(*f, **SCALES, gap=(2, 1, 3), threshold=-np.inf)
    assert got["threshold"] == -np.inf
    assert_same(got, ref)


# ---- 4. the opened mask ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blobs():
    """Planted velocities under a smooth reliability, so the mask has components of many sizes."""
    from scipy import ndimage

    shape = (8, 30, 70)
    rel = ndimage.gaussian_filter(np.random.default_rng(31).standard_normal(shape), 1.5).astype(np.float32)
    return qr.planted_fields(shape, 32)[:3] + [rel]


M_ROIS = [(0, 8, 2, 28, 3, 50), (1, 7, 10, 30, 30, 70)]  # overlapping: each uses its own bit of keep


def test_opened_mask_against_the_labelled_reference(blobs):
    vx, vy, vz, rel = blobs
    boxes, thresh = mr.boxes_of(vx.shape, M_ROIS), np.percentile(rel, 80)
    keep, counts = mr.open_ref(rel, thresh, boxes, 20, 18)
    assert np.all(counts["n_components_kept"] > 0) and np.all(counts["n_components"] > counts["n_components_kept"])
    both = keep[1:7, 10:28, 30:50:2]  # the boxes' overlap: some voxels are kept by one box only
    assert np.any((both >> 1 & 1) != (both >> 2 & 1))
    kw = dict(**SCALES, gap=(1, 1, 2), rois=M_ROIS)
    ref = qr.quiver_ref(vx, vy, vz, rel, 80, keep=keep, **kw)
    assert_not_vacuous(ref)
    unopened = qr.quiver_ref(vx, vy, vz, rel, 80, **kw)
    assert all(o["n_valid"] < u["n_valid"] for o, u in zip(ref["samples"], unopened["samples"]))
    got = quiver_sample(vx, vy, vz, rel, 80, min_size=20, connectivity=18, **kw)
    assert_same(got, ref)
    # min_size 1 keeps every mask voxel: the unopened lists
    assert_same(quiver_sample(vx, vy, vz, rel, 80, min_size=1, **kw), unopened)
    assert_same(quiver_sample(vx, vy, vz, rel, 80, **kw), unopened)
    # a ROI's records do not depend on the other ROIs requested beside it
    for k, roi in enumerate(M_ROIS):
        alone = quiver_sample(vx, vy, vz, rel, 80, min_size=20, connectivity=18, **dict(kw, rois=[roi]))
        for mine, among in ((alone["samples"][0], got["samples"][0]), (alone["samples"][1], got["samples"][1 + k])):
            assert mine["n_valid"] == among["n_valid"] and mine["n_lattice"] == among["n_lattice"]
            assert np.array_equal(mine["zyx"], among["zyx"]) and mine["v"].tobytes() == among["v"].tobytes()


# ---- 5. truncation, the block bounds and determinism (the raw words) -----------------------------------------
CANARY = np.int64(0x5A5A5A5A5A5A5A5A)
TAIL = 64


def _raw(f, rois, gap, max_vectors, percentile=60):
    """One of3d_quiver_sample call into a canary-filled buffer with TAIL words beyond the result:
    (call, words)."""
    import torch

    from opticalflow3d_dev_amd.analysis import percentile_threshold_device

    dev = [torch.from_numpy(a).cuda() for a in f]
    boxes = mr.boxes_of(f[0].shape, rois)
    call = _QuiverCall(boxes, f[0].shape, dev[3].dtype == torch.float64, QuiverSpec(gap, max_vectors), 3,
                       tuple(SCALES.values()), dev[0].device)
    res = torch.full((call.result_bytes // 8 + TAIL,), int(CANARY), dtype=torch.int64, device=dev[0].device)
    thresh = percentile_threshold_device(dev[3], percentile)
    call.enqueue((dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), False), thresh.data_ptr(),
                 None, res.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return call, res.cpu().numpy()


T_SHAPE, T_GAP, T_ROIS = (5, 40, 150), (1, 2, 1), [(1, 4, 3, 37, 7, 140), (0, 5, 0, 40, 149, 150)]


def test_truncation_keeps_the_first_records_and_the_block_bounds():
    f = qr.planted_fields(T_SHAPE, 29)
    ref = qr.quiver_ref(*f, 60, **SCALES, gap=T_GAP, rois=T_ROIS)
    n_valid = [s["n_valid"] for s in ref["samples"]]
    cap = 700  # ROI 0 (two workgroups) and ROI 1 overflow it, ROI 2 (100 lattice points) does not
    assert n_valid[0] > 3000 and n_valid[1] > cap and n_valid[2] < ref["samples"][2]["n_lattice"] == 100 < cap
    call, words = _raw(f, T_ROIS, T_GAP, cap)
    assert call.capacity.tolist() == [cap, cap, 100]
    n = call.result_bytes // 8
    assert n == 6 + 4 * 3 + 4 * (cap + cap + 100)
    assert np.all(words[n:] == CANARY) and words[n:].size == TAIL  # nothing past the last block
    assert words[1:6].tolist() == [3, 1, 2, 1, 1]
    head = words[6:18].reshape(3, 4)
    assert head[:, 0].tolist() == [s["n_lattice"] for s in ref["samples"]]
    assert head[:, 1].tolist() == n_valid  # the full counts
    assert head[:, 2].tolist() == [cap, cap, n_valid[2]]
    assert head[:, 3].tolist() == [18, 18 + 4 * cap, 18 + 8 * cap]
    # a block is followed at once by the next one, so a record past a block's capacity would land
    # in the next ROI's indices: the comparison of every ROI's records covers the bounds between
    # the blocks.  Inside ROI 2's block the words past n_stored are left as they were.
    got = {"threshold": np.float32(words[:1].view(np.float64)[0]), "rois": call.boxes, "gap": call.gap,
           "samples": call.decode(words)}
    assert_same(got, ref, capacity=call.capacity)
    assert [s["truncated"] for s in got["samples"]] == [True, True, False]
    last = words[18 + 8 * cap:n].reshape(4, 100)
    assert np.all(last[:, n_valid[2]:] == CANARY)
    # and through the public call
    assert_same(quiver_sample(*f, 60, **SCALES, gap=T_GAP, rois=T_ROIS, max_vectors=cap), ref, capacity=call.capacity)
    zero = quiver_sample(*f, 60, **SCALES, gap=T_GAP, rois=T_ROIS, max_vectors=0)  # counts alone
    assert [s["n_valid"] for s in zero["samples"]] == n_valid and all(len(s["zyx"]) == 0 for s in zero["samples"])


def test_same_words_twice():
    f = qr.planted_fields(T_SHAPE, 30)
    (c, a), (_, b) = (_raw(f, T_ROIS, T_GAP, 2500) for _ in range(2))
    assert a[:18].tobytes() == b[:18].tobytes()  # the header
    assert a[7] > 2500 > a[11] > 0  # ROI 0 truncated, ROI 1 not
    for r in range(3):
        n_stored, off, cap = int(a[6 + 4 * r + 2]), int(a[6 + 4 * r + 3]), int(c.capacity[r])
        for k in range(4):
            lo = off + k * cap
            assert a[lo:lo + n_stored].tobytes() == b[lo:lo + n_stored].tobytes(), (r, k)
    assert a.tobytes() == b.tobytes()  # and every other word is untouched in both
