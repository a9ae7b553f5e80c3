"""Contractility on the device (csrc/kt_ccl.hip: of3d_mask_largest; csrc/kt_contract.hip:
of3d_flow_contract) against the scipy / numpy restatement tests/contract_ref.py: the keep bits,
the counts, the integer sums, the centroid and the histograms exactly, the four sums within the
summation bound; determinism, independence of the boxes, the given centre, the masked summary
over the largest component, the canary behind the result and every refusal."""
import ctypes

import numpy as np
import pytest

import contract_ref as cr
import mask_ref as mr
import summary_ref as sr
from conftest import bits_equal
from opticalflow3d_dev_amd import ContractSpec, _lib, contractility, largest_component_mask
from opticalflow3d_dev_amd.analysis import _ContractCall, _LargestCall, percentile_threshold_device

pytestmark = pytest.mark.gpu

CANARY, TAIL = -0x0123456789ABCDEF, 64


# ---- 1. the largest component ----------------------------------------------------------------------
def _rois(boxes, ndim):
    return [tuple(int(v) for v in b[6 - 2 * ndim:]) for b in boxes[1:]]


@pytest.mark.parametrize("connectivity", [6, 18, 26])
@pytest.mark.parametrize("name", ["random", "smooth", "checkerboard", "tie", "empty", "truncated"])
def test_largest_component_equals_the_host_labelling(name, connectivity):
    rel, boxes, thresh = cr.label_masks()[name]
    keep, counts = cr.largest_ref(rel, thresh, boxes, connectivity)
    got = largest_component_mask(rel, threshold=thresh, connectivity=connectivity, rois=_rois(boxes, 3))
    assert got["keep"].dtype == np.uint16 and np.array_equal(got["keep"], keep), name
    for k in mr.COUNTS:
        assert np.array_equal(got[k], counts[k]), (name, k, got[k], counts[k])
    assert np.array_equal(got["mask"](1), (keep >> 1 & 1).astype(bool))
    if name == "smooth":  # two overlapping boxes: somewhere one keeps a voxel that the other drops
        both = keep[1:8, 10:38, 30:66]
        assert np.any((both >> 1 & 1) != (both >> 2 & 1))


@pytest.mark.parametrize("connectivity", [4, 8])
def test_largest_component_2d_float64(connectivity):
    rel, boxes, thresh = cr.label_masks_2d()["random2d"]
    keep, counts = cr.largest_ref(rel, thresh, boxes, connectivity)
    got = largest_component_mask(rel, threshold=thresh, connectivity=connectivity, rois=_rois(boxes, 2))
    assert np.array_equal(got["keep"], keep)
    for k in mr.COUNTS:
        assert np.array_equal(got[k], counts[k]), (k, got[k], counts[k])
    assert counts["n_components"][0] > 10 and counts["n_components_kept"].tolist() == [1, 1]


def test_a_tie_goes_to_the_lower_root():
    rel, boxes, thresh = cr.label_masks()["tie"]
    got = largest_component_mask(rel, threshold=thresh, rois=_rois(boxes, 3))
    assert (got["keep"][1] & 1).sum() == 6 and not (got["keep"][3] & 1).any()
    assert (got["keep"][3] >> 1 & 1).sum() == 6 and got["n_kept"].tolist() == [6, 6]


# ---- 2. the reduction against the reference --------------------------------------------------------
def _assert_matches(got, ref, counts):
    assert got["moments"].dtype == np.uint64 and np.array_equal(got["moments"], ref["moments"])
    origin = ref["rois"][:, [4, 2, 0]].astype(np.float64)
    assert bits_equal(got["centroid"], origin + ref["centroid"])  # center_of_mass, bit for bit
    assert bits_equal(got["center_used"], origin + ref["center_used"])
    for k in ("n_valid", "n_angle", "n_inward"):
        assert np.array_equal(got[k], ref[k]), (k, got[k], ref[k])
    for k in cr.QUANTITIES:
        assert got["hist"][k].dtype == np.uint64 and np.array_equal(got["hist"][k], ref["hist"][k]), k
        assert np.array_equal(got["edges"][k], ref["edges"][k])
    for k in cr.SUMS:
        err, bound = np.abs(got[k] - ref[k]), cr.sum_bound(ref, k)
        print(k, "max err / bound:", float(np.max(err / np.maximum(bound, 1e-300))))
        assert np.all(err <= bound), (k, err, bound)
    if counts is not None:
        for k in ("n_mask", "n_components", "n_kept"):
            assert np.array_equal(got[k], counts[k]), k
    else:
        assert np.array_equal(got["n_mask"], ref["moments"][:, 0].astype(np.int64))
        assert got["n_components"].tolist() == [-1] * len(ref["rois"])
    na = ref["n_angle"].astype(np.float64)
    assert np.array_equal(got["mean_angle"], got["sum_angle"] / na)
    assert np.array_equal(got["inward_fraction"], got["n_inward"] / na)


@pytest.fixture(scope="module")
def general():
    return {"general3d": cr.general3d(), "general2d": cr.general2d()}


@pytest.mark.parametrize("mode", ["largest", "summary"])
@pytest.mark.parametrize("name", ["general3d", "general2d"])
def test_contractility_against_the_reference(general, name, mode):
    f, rois, per = general[name]
    boxes = cr.boxes_of(np.shape(f[0]), rois)
    keep, counts, thresh = cr.mask_of(f[3], per, boxes, mode)
    ref = cr.contract_ref(*f[:3], keep, boxes, **cr.SCALES, bins=cr.BINS)
    assert np.all(ref["n_angle"] > 100)
    got = contractility(*f, per, **cr.SCALES, rois=rois, spec=ContractSpec(mask=mode, bins=cr.BINS))
    assert got["threshold"] == thresh and got["threshold"].dtype == f[3].dtype
    _assert_matches(got, ref, counts)


def test_float32_fields_and_float64_rel(general):
    f, rois, per = general["general3d"]
    f = [a.astype(np.float32) for a in f[:3]] + [f[3].astype(np.float64)]
    boxes = cr.boxes_of(f[0].shape, rois)
    keep, counts, _ = cr.mask_of(f[3], per, boxes, "largest", 18)
    ref = cr.contract_ref(*f[:3], keep, boxes, **cr.SCALES, bins={"inward": cr.BINS["inward"]})
    got = contractility(*f, per, **cr.SCALES, rois=rois,
                        spec=ContractSpec(connectivity=18, bins={"inward": cr.BINS["inward"]}))
    assert np.array_equal(got["moments"], ref["moments"]) and np.array_equal(got["n_angle"], ref["n_angle"])
    assert np.array_equal(got["hist"]["inward"], ref["hist"]["inward"]) and "angle" not in got["hist"]
    for k in cr.SUMS:
        assert np.all(np.abs(got[k] - ref[k]) <= cr.sum_bound(ref, k)), k
    for k in ("n_mask", "n_components", "n_kept"):
        assert np.array_equal(got[k], counts[k]), k


def test_the_centroid_voxel_counts_as_valid_but_has_no_angle():
    f = cr.cube()
    got = contractility(*f, 50)
    assert got["moments"][0].tolist() == [27, 108, 81, 54] and got["centroid"][0].tolist() == [4.0, 3.0, 2.0]
    assert got["n_valid"][0] == 27 and got["n_angle"][0] == 26
    ref = cr.contract_ref(*f[:3], cr.mask_of(f[3], 50, cr.boxes_of(f[0].shape, []), "largest")[0],
                          cr.boxes_of(f[0].shape, []))
    for k in cr.SUMS:
        assert np.all(np.abs(got[k] - ref[k]) <= cr.sum_bound(ref, k)), k


def test_an_empty_mask_has_a_nan_centroid_and_no_angle():
    f = cr.cube()
    f[3][:] = 0.0
    got = contractility(*f, 50, spec=ContractSpec(bins=cr.BINS))
    assert np.isnan(got["centroid"]).all() and np.isnan(got["center_used"]).all() and np.isnan(got["mean_angle"][0])
    assert got["n_valid"][0] == got["n_angle"][0] == got["n_mask"][0] == got["n_kept"][0] == 0
    assert not got["hist"]["angle"].any() and not got["moments"].any()


def test_aligned_flow_is_exactly_0_and_180_degrees():
    f, c, n_to, n_away = cr.aligned()
    edges = np.linspace(0.0, 180.0, 10)
    got = contractility(*f, 50, 0.5, 2.0, 1.0, spec=ContractSpec(mask="summary", center=c, bins={"angle": edges}))
    assert got["center_used"][0].tolist() == list(c) and got["centroid"][0].tolist() == list(c)  # the lines' own centre too
    assert got["n_valid"][0] == n_to + n_away + 1 and got["n_angle"][0] == n_to + n_away
    assert got["n_inward"][0] == n_to
    assert got["sum_dot"][0] == n_to - n_away  # every dot is exactly +-1
    assert got["sum_angle"][0] == 180.0 * n_away
    hist = got["hist"]["angle"][0]
    assert hist[0] == n_to and hist[-1] == n_away and hist[1:-1].sum() == 0  # 180 lands in the closed last bin
    ref = cr.contract_ref(*f[:3], cr.mask_of(f[3], 50, cr.boxes_of(f[0].shape, []), "summary")[0],
                          cr.boxes_of(f[0].shape, []), 0.5, 2.0, 1.0, center=c)
    assert got["sum_speed"][0] == ref["sum_speed"][0] and got["sum_inward"][0] == ref["sum_inward"][0]


# ---- 3. raw words: determinism, independence, the given centre, the canary ------------------------
def _raw(f, rois, per, spec, scales=cr.SCALES):
    """One contract call into a canary-filled buffer with TAIL words beyond the result: (call, words)."""
    import torch

    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None else None for a in f]
    shape = f[0].shape
    boxes = cr.boxes_of(shape, rois)
    call = _ContractCall(boxes, shape if len(shape) == 3 else (1,) + shape, dev[3].dtype == torch.float64, spec,
                         len(shape), tuple(scales.values()), dev[0].device)
    res = torch.full((call.result_bytes // 8 + TAIL,), CANARY, dtype=torch.int64, device=dev[0].device)
    thresh = percentile_threshold_device(dev[3], per)
    call.enqueue((dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr() if dev[2] is not None else None,
                  dev[3].data_ptr(), False), thresh.data_ptr(), None, res.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return call, res.cpu().numpy()


def _box(call, words, r):
    w = 17 + sum(call.nbins)
    return words[r * w:(r + 1) * w]


@pytest.mark.parametrize("mode", ["largest", "summary"])
def test_same_words_twice_alone_and_beside_and_with_the_centroid_given(general, mode):
    f, rois, per = general["general3d"]
    spec = ContractSpec(mask=mode, bins=cr.BINS)
    (c, a), (_, b) = (_raw(f, rois, per, spec) for _ in range(2))
    assert a.tobytes() == b.tobytes()
    assert np.all(a[c.result_bytes // 8:] == CANARY) and len(a) == c.result_bytes // 8 + TAIL
    assert c.result_bytes == 8 * (3 * (17 + 36 + 48) + (12 if mode == "largest" else 0))
    # a ROI alone and beside others: the whole volume, and ROI 1 without ROI 2
    c0, alone = _raw(f, [], per, spec)
    assert _box(c0, alone, 0).tobytes() == _box(c, a, 0).tobytes()
    c1, one = _raw(f, rois[:1], per, spec)
    assert _box(c1, one, 1).tobytes() == _box(c, a, 1).tobytes()
    assert np.all(alone[c0.result_bytes // 8:] == CANARY)
    # the reported centroid given back: the same words
    centroid = _box(c0, alone, 0)[4:7].copy().view(np.float64)
    cg, given = _raw(f, [], per, ContractSpec(mask=mode, center=tuple(centroid), bins=cr.BINS))
    assert given.tobytes() == alone.tobytes()
    # another centre: other sums, the mask's own centroid still reported
    cs, shifted = _raw(f, [], per, ContractSpec(mask=mode, center=tuple(centroid + 1.5), bins=cr.BINS))
    assert _box(cs, shifted, 0)[:7].tobytes() == _box(c0, alone, 0)[:7].tobytes()
    assert _box(cs, shifted, 0)[7:10].view(np.float64).tolist() == (centroid + 1.5).tolist()
    assert _box(cs, shifted, 0)[13:17].tobytes() != _box(c0, alone, 0)[13:17].tobytes()


def test_masked_summary_over_the_largest_component(general):
    import torch

    f, rois, per = general["general3d"]
    boxes = cr.boxes_of(f[0].shape, rois)
    keep, counts, thresh = cr.mask_of(f[3], per, boxes, "largest")
    ref = mr.summary_ref_masked(*f[:3], keep, thresh, boxes, **cr.SCALES)
    dev = [torch.from_numpy(a).cuda() for a in f]
    lib, n_roi = _lib.load(), len(boxes)
    call = _LargestCall(boxes, f[0].shape, False, 26, dev[0].device)
    t = percentile_threshold_device(dev[3], per)
    cnt = torch.empty((n_roi, 4), dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    call.enqueue(dev[3].data_ptr(), t.data_ptr(), cnt.data_ptr(), stream)
    nb = (ctypes.c_int * 6)()
    res = torch.zeros(lib.of3d_flow_summary_result_bytes(n_roi, nb) // 8, dtype=torch.int64, device="cuda")
    ws = torch.empty(lib.of3d_flow_summary_workspace_bytes(), dtype=torch.uint8, device="cuda")
    _lib.check(lib.of3d_flow_summary_masked(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(),
                                            0, 0, *f[0].shape, t.data_ptr(), *cr.SCALES.values(), call.roi_arr, n_roi,
                                            nb, None, res.data_ptr(), ws.data_ptr(), stream, call.keep.data_ptr()))
    assert np.array_equal(call.keep.cpu().numpy(), keep)
    assert np.array_equal(cnt.cpu().numpy()[:, 3], counts["n_kept"])
    body = res.cpu().numpy()[8:].reshape(n_roi, 10)
    assert np.array_equal(body[:, 0], ref["n_valid"]) and np.array_equal(body[:, 1], ref["n_voxels"])
    sums = np.ascontiguousarray(body[:, 2:]).view(np.float64)
    for i, k in enumerate(sr.SUMS):
        assert np.all(np.abs(sums[:, i] - ref[k]) <= sr.sum_bound(ref, k)), k


# ---- 4. refusals -----------------------------------------------------------------------------------
def test_every_refusal_returns_non_zero_with_a_message():
    import torch

    lib = _lib.load()
    I64, D = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
    v = torch.ones((2, 3, 4), dtype=torch.float64, device="cuda")
    rel = torch.ones((2, 3, 4), dtype=torch.float32, device="cuda")
    t = torch.zeros(1, dtype=torch.float32, device="cuda")
    out = torch.zeros(4096, dtype=torch.int64, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    keep = torch.zeros((2, 3, 4), dtype=torch.uint16, device="cuda")
    whole = [0, 2, 0, 3, 0, 4]

    def contract(vx=v.data_ptr(), vz=v.data_ptr(), dims=(2, 3, 4), rois=whole, n_roi=1, nbins=(0, 0), edges=(None, None),
                 center=None):
        r = (ctypes.c_int64 * len(rois))(*rois)
        nb = (ctypes.c_int * 2)(*nbins)
        arrs = [None if e is None else np.asarray(e, np.float64) for e in edges]
        e = (D * 2)(*[None if a is None else a.ctypes.data_as(D) for a in arrs])
        c = None if center is None else (ctypes.c_double * 3)(*center)
        return lib.of3d_flow_contract(vx, v.data_ptr(), vz, rel.data_ptr(), 0, 0, *dims, t.data_ptr(), 1.0, 1.0, 1.0,
                                      ctypes.cast(r, I64), n_roi, None, c, nb, e, out.data_ptr(), ws.data_ptr(), None)

    def refused(rc, text):
        assert rc != 0 and text in _lib.last_error(), (rc, _lib.last_error())

    refused(contract(vx=None), "null")
    refused(contract(rois=[0, 2, 0, 3, 0, 5]), "outside the volume")
    refused(contract(rois=[1, 1, 0, 3, 0, 4]), "empty")
    refused(contract(rois=whole * 17, n_roi=17), "1 to 16")
    refused(contract(nbins=(257, 0)), "256 bins")
    refused(contract(nbins=(2, 0), edges=([0.0, 2.0, 1.0], None)), "ascend")
    refused(contract(nbins=(0, 1), edges=(None, None)), "without edges")
    refused(contract(center=(1.0, np.inf, 0.0)), "finite")
    refused(contract(center=(np.nan, 0.0, 0.0)), "finite")
    refused(contract(dims=(1, 3, 4), rois=[0, 1, 0, 3, 0, 4]), "2D")
    refused(contract(vz=None), "nz == 1")
    # 2^32 voxels with an edge of 2^24: the coordinate sums could pass 2^63 (nothing is launched)
    long_box = [0, 1, 0, 256, 0, 1 << 24]
    refused(contract(vz=None, dims=(1, 256, 1 << 24), rois=long_box), "64-bit moments")
    r = (ctypes.c_int64 * 6)(*long_box)
    nb = (ctypes.c_int * 2)()
    assert lib.of3d_flow_contract_workspace_bytes(ctypes.cast(r, I64), 1, nb) == 0 and "64-bit" in _lib.last_error()
    assert lib.of3d_flow_contract_result_bytes(17, nb) == 0
    assert contract() == 0  # the same arguments unmodified are accepted

    def largest(rel_ptr=rel.data_ptr(), rois=whole, n_roi=1, connectivity=26, dims=(2, 3, 4)):
        r = (ctypes.c_int64 * len(rois))(*rois)
        return lib.of3d_mask_largest(rel_ptr, 0, *dims, t.data_ptr(), ctypes.cast(r, I64), n_roi, connectivity,
                                     keep.data_ptr(), out.data_ptr(), ws.data_ptr(), None)

    refused(largest(rel_ptr=None), "null")
    refused(largest(connectivity=8), "connectivity")
    refused(largest(connectivity=26, dims=(1, 6, 4), rois=[0, 1, 0, 6, 0, 4]), "connectivity")
    refused(largest(rois=[0, 3, 0, 3, 0, 4]), "outside the volume")
    refused(largest(rois=whole * 17, n_roi=17), "1 to 16")
    assert lib.of3d_mask_largest_workspace_bytes(ctypes.cast((ctypes.c_int64 * 6)(0, 0, 0, 3, 0, 4), I64), 1) == 0
    assert largest() == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="mask"):
        contractility(*cr.cube(), 50, spec=ContractSpec(mask="open"))
    with pytest.raises(ValueError, match="connectivity"):
        contractility(*cr.cube(), 50, spec=ContractSpec(connectivity=8))
    with pytest.raises(ValueError, match="center"):
        contractility(*cr.cube(), 50, spec=ContractSpec(center=(1.0, 2.0)))
    with pytest.raises(ValueError, match="finite"):
        contractility(*cr.cube(), 50, spec=ContractSpec(center=(1.0, 2.0, np.nan)))
    with pytest.raises(ValueError, match="unknown histogram quantity"):
        contractility(*cr.cube(), 50, spec=ContractSpec(bins={"phi": [0.0, 1.0]}))
    with pytest.raises(ValueError, match="ascending"):
        contractility(*cr.cube(), 50, spec=ContractSpec(bins={"angle": [0.0, 0.0, 1.0]}))
