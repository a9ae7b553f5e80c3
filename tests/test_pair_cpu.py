"""Host side of the two-channel comparison (no GPU): the facts about the general and the exact
case that tests/test_gpu_pair.py relies on, re-derived with the numpy restatement (pair_ref);
channel_compare's validation; the C ABI's host arithmetic and refusals; the exports."""
import ctypes
import math

import numpy as np
import pytest

import pair_ref as pr
import summary_ref as sr
import whist_ref as wr
import opticalflow3d_dev_amd as pkg
from opticalflow3d_dev_amd import SummarySpec, _lib, analysis


# ---- the general case ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def general():
    ch0, ch1 = pr.general_case()
    boxes = pr.boxes_of(pr.G_SHAPE, pr.G_ROIS)
    t = pr.thresholds_of(ch0[3], ch1[3], 80)
    keep, counts = pr.joint_open_ref(ch0[3], ch1[3], t[0], t[1], boxes, 5, 6)
    return ch0, ch1, boxes, t, keep, counts, pr.pair_ref(ch0, ch1, keep, boxes, *pr.G_SCALES, bins=pr.G_BINS)


def test_general_case_counts(general):
    ch0, ch1, boxes, t, keep, counts, ref = general
    assert ch0[3].dtype == np.float32 and t.dtype == np.float32 and ch0[0].dtype == np.float64
    assert boxes.tolist() == [[0, 5, 0, 37, 0, 67], [0, 5, 1, 36, 3, 64]]
    assert counts["n_mask"].tolist() == [3272, 2824]
    assert counts["n_components"].tolist() == [1107, 932]
    assert counts["n_kept"].tolist() == [1896, 1663] and counts["n_components_kept"][0] == 167
    assert ref["n_valid"].tolist() == [1896, 1663]  # normal deviates are never zero: kept = valid
    assert ref["n_voxels"].tolist() == [5 * 37 * 67, 5 * 35 * 61]


def test_every_clause_of_the_predicate_decides_something(general):
    ch0, ch1, _, t, _, _, _ = general
    r0, r1 = ch0[3], ch1[3]
    m_or = pr.joint_mask(r0, r1, t[0], t[1], 0.0, "or")
    no_floor = pr.joint_mask(r0, r1, t[0], t[1], -np.inf, "or")
    assert int(no_floor.sum() - m_or.sum()) == 1219 and np.all(no_floor[m_or])
    assert int(((r0 > t[0]) ^ (r1 > t[1])).sum()) == 4024
    m_and = pr.joint_mask(r0, r1, t[0], t[1], 0.0, "and")
    assert np.array_equal(m_and, (r0 > t[0]) & (r1 > t[1])) and 0 < m_and.sum() < m_or.sum()
    # a NaN fails the voxel whatever the floor; -inf fails the floor -inf as well
    r0n = r0.copy()
    r0n[2, 3, 4], r0n[2, 3, 5] = np.nan, -np.inf
    big = np.float32(-1)
    m = pr.joint_mask(r0n, r1, big, big, -np.inf, "or")
    assert not m[2, 3, 4] and not m[2, 3, 5] and m.sum() == m.size - 2


def test_one_component_setting(general):
    ch0, ch1, boxes, _, _, _, _ = general
    t = pr.thresholds_of(ch0[3], ch1[3], 40)
    _, counts = pr.joint_open_ref(ch0[3], ch1[3], t[0], t[1], boxes, 1, 26)
    assert counts["n_mask"].tolist() == counts["n_kept"].tolist() == [6742, 5802]
    assert counts["n_components"].tolist() == [1, 1]


def test_general_values_clear_of_edges_and_the_drop_rule_is_exercised(general):
    ref = general[-1]
    sr.assert_clear_of_edges(ref, pr.QUANTITIES)
    for k, e in pr.G_BINS.items():
        for vals in ref["values"]:
            assert np.min(np.abs(vals[k][:, None] - e[None, :])) > 1e-6, k
    dot, e = ref["values"][0]["dot"], pr.G_BINS["dot"]
    assert int(((dot < e[0]) | (dot > e[-1])).sum()) == 385
    assert ref["hist"]["dot"][0].sum() == 1896 - 385
    assert ref["hist"]["cosine"][0].sum() == ref["hist"]["dtheta"][0].sum() == 1896


def test_summation_orders_stay_far_inside_the_bound(general):
    """Four orders (forward, backward, shuffled, numpy's pairwise) of all eight cross sums: the
    bound (n + 16) u sum|t| leaves the device's tree order a wide margin."""
    ref = general[-1]
    rng = np.random.default_rng(5)
    worst = 0.0
    for r, vals in enumerate(ref["values"]):
        for k, t in vals["terms"].items():
            sums = [float(np.sum(t))]
            for order in (np.arange(t.size), np.arange(t.size)[::-1], rng.permutation(t.size)):
                s = 0.0
                for x in t[order].tolist():
                    s += x
                sums.append(s)
            worst = max(worst, max(abs(s - ref[k][r]) for s in sums) / pr.pair_bound(ref, k)[r])
    print("worst err / bound over the orders:", worst)
    assert worst < 0.05


def test_in_plane_reference_differs_only_where_it_should(general):
    ch0, ch1, boxes, _, keep, _, ref = general
    flat = pr.pair_ref(ch0, ch1, keep, boxes, *pr.G_SCALES, in_plane=True)
    assert np.array_equal(flat["n_valid"], ref["n_valid"])
    assert not flat["ch0"]["sum_vz"].any() and not flat["ch1"]["sum_vz"].any()
    for k in ("sum_vx", "sum_vy", "sum_sin", "sum_cos"):
        assert flat["ch0"][k].tobytes() == ref["ch0"][k].tobytes()
    assert flat["sum_sin_dtheta"].tobytes() == ref["sum_sin_dtheta"].tobytes()
    assert np.all(flat["ch0"]["sum_magnitude"] < ref["ch0"]["sum_magnitude"])


# ---- the exact case --------------------------------------------------------------------------------
def test_exact_case_sums_are_exact_in_any_order():
    e0, e1 = pr.exact_case()
    assert e0[0].shape == wr.EXACT_SHAPE and e0[3].dtype == np.float32
    boxes = pr.boxes_of(wr.EXACT_SHAPE, wr.EXACT_ROIS)
    t = pr.thresholds_of(e0[3], e1[3], 80)
    keep, counts = pr.joint_open_ref(e0[3], e1[3], t[0], t[1], boxes, 1, 26)
    ref = pr.pair_ref(e0, e1, keep, boxes)
    assert ref["n_valid"].tolist() == counts["n_kept"].tolist() == [2187, 1063, 31]
    rng = np.random.default_rng(5)
    for r, vals in enumerate(ref["values"]):
        for c in (0, 1):
            mag = vals["ch_terms"][c]["sum_magnitude"]
            assert np.array_equal(mag * 4, np.round(mag * 4)) and mag.min() >= 0.75
        perm = rng.permutation(ref["n_valid"][r])
        terms = [(k, vals["terms"][k], ref[k][r]) for k in pr.EXACT_PAIR_SUMS]
        terms += [(k, vals["ch_terms"][c][k], ref[f"ch{c}"][k][r]) for c in (0, 1) for k in pr.EXACT_CH_SUMS]
        assert len(terms) == 12
        for k, t, want in terms:
            for order in (np.arange(t.size), np.arange(t.size)[::-1], perm):
                s = 0.0
                for x in t[order].tolist():
                    s += x
                assert s == want == math.fsum(t.tolist()), (r, k)
            assert float(np.sum(t)) == want, (r, k)


# ---- validation ------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins,word", [
    ({"dot": [0.0, 1.0, 1.0]}, "pair dot bin edges must be strictly ascending"),
    ({"cosine": [0.0, np.nan, 1.0]}, "pair cosine bin edges must be strictly ascending"),
    ({"dtheta": [0.0]}, "pair dtheta edges must be a 1-D array of 2 to 257 values"),
    ({"dmagnitude": np.arange(258.0)}, "pair dmagnitude edges must be a 1-D array of 2 to 257 values"),
    ({"theta": [0.0, 1.0]}, "unknown pair histogram quantity 'theta'"),
])
def test_pair_bins_are_validated_with_the_summary_messages(bins, word):
    with pytest.raises(ValueError, match=word):
        SummarySpec._quantity_bins(bins, 3, "pair ", analysis.PAIR_QUANTITIES)


def test_pair_bins_accepted():
    nb, ed = SummarySpec._quantity_bins({"dtheta": [-1, 0, 2], "dot": np.arange(257.0)}, 2, "pair ",
                                        analysis.PAIR_QUANTITIES)
    assert nb == [256, 0, 2, 0] and ed[2].tolist() == [-1.0, 0.0, 2.0] and ed[2].dtype == np.float64 and ed[1] is None
    assert SummarySpec._quantity_bins(None, 3, "pair ", analysis.PAIR_QUANTITIES) == ([0] * 4, [None] * 4)
    assert analysis.PAIR_QUANTITIES == pr.QUANTITIES and analysis.PAIR_SUMS == pr.PAIR_SUMS


def test_combine_and_floor_handling():
    assert analysis._pair_options(0.0, "or") == (0.0, 0) and analysis._pair_options(-np.inf, "and") == (-np.inf, 1)
    assert analysis._pair_options(np.float32(0.5), "or") == (0.5, 0)
    for bad in ("xor", "OR", 0, None):
        with pytest.raises(ValueError, match="combine"):
            analysis._pair_options(0.0, bad)
    for bad in (np.nan, "low", None):
        with pytest.raises(ValueError, match="floor"):
            analysis._pair_options(bad, "or")


def test_rois_connectivity_and_min_size_go_through_summary_spec():
    boxes, dims, m, c = analysis._pair_spec((37, 67), 80, [(1, 36, 3, 64)], 1, None)
    assert boxes.tolist() == [[0, 1, 0, 37, 0, 67], [0, 1, 1, 36, 3, 64]] and dims == (1, 37, 67) and (m, c) == (1, 8)
    assert analysis._pair_spec((5, 37, 67), 80, None, 7, 6)[2:] == (7, 6)
    with pytest.raises(ValueError, match="ROI 1"):
        analysis._pair_spec((5, 37, 67), 80, [(0, 6, 0, 37, 0, 67)], 1, None)
    with pytest.raises(ValueError, match="connectivity"):
        analysis._pair_spec((5, 37, 67), 80, None, 1, 8)
    with pytest.raises(ValueError, match="min_size"):
        analysis._pair_spec((5, 37, 67), 80, None, 0, None)
    with pytest.raises(ValueError, match="rel_percentile"):
        analysis._pair_spec((5, 37, 67), 101, None, 1, None)


# ---- the C ABI's host arithmetic -------------------------------------------------------------------
def test_c_abi_sizes_and_refusals():
    lib = _lib.load()
    nb = (ctypes.c_int * 4)(36, 0, 12, 5)
    boxes = np.array([[0, 128, 0, 512, 0, 512], [2, 3, 4, 9, 7, 30], [0, 1, 0, 2, 0, 20000]], dtype=np.int64)
    rois = boxes.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    assert lib.of3d_flow_pair_result_bytes(3, nb) == 3 * (26 + 53) * 8
    # workgroups: 1024 (the cap), 1 (115 voxels), 2 (5 by size, capped by the 2 rows); 37 + 13 + 6 edges
    assert lib.of3d_flow_pair_workspace_bytes(rois, 3, nb) == ((1024 + 1 + 2) * 24 + 56) * 8
    none = (ctypes.c_int * 4)()  # unlike the weighted histograms': no bins at all is legal
    assert lib.of3d_flow_pair_result_bytes(3, none) == 3 * 26 * 8
    assert lib.of3d_flow_pair_workspace_bytes(rois, 3, none) == (1024 + 1 + 2) * 24 * 8
    boxes[1, 1] = 2  # an empty box
    assert lib.of3d_flow_pair_workspace_bytes(rois, 3, nb) == 0 and "ROI 1" in _lib.last_error()
    boxes[1, 1] = 3
    boxes[0] = [0, 2 ** 31 - 1, 0, 1, 0, 2 ** 31 - 1]  # one row per workgroup of 2^31 - 1 voxels
    assert lib.of3d_flow_pair_workspace_bytes(rois, 3, nb) == 0 and "too large" in _lib.last_error()
    boxes[0] = [0, 128, 0, 512, 0, 512]
    assert lib.of3d_flow_pair_workspace_bytes(rois, 17, nb) == 0 and "16 ROI" in _lib.last_error()
    assert lib.of3d_flow_pair_result_bytes(17, nb) == 0 and lib.of3d_flow_pair_result_bytes(0, nb) == 0
    many = (ctypes.c_int * 4)(0, 257, 0, 0)
    assert lib.of3d_flow_pair_result_bytes(1, many) == 0
    assert lib.of3d_flow_pair_workspace_bytes(rois, 3, many) == 0 and "256 bins" in _lib.last_error()
    assert lib.of3d_flow_pair_workspace_bytes(None, 3, nb) == 0 and "null" in _lib.last_error()


def test_bad_arguments_are_errors_not_crashes():
    """Everything refused here is refused before a pointer is touched or a kernel launched."""
    lib = _lib.load()
    p = ctypes.c_void_p(4096)  # never dereferenced
    boxes = np.array([[0, 2, 0, 3, 0, 4]], dtype=np.int64)
    rois = boxes.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    open_args = lambda **kw: [kw.get(k, v) for k, v in dict(
        rel0=p, t0=p, rel1=p, t1=p, f64=0, floor=0.0, combine=0, nz=2, ny=3, nx=4, rois=rois, n_roi=1, min_size=1,
        conn=26, keep=p, counts=p, ws=p, stream=None).items()]
    for k in ("rel0", "t0", "rel1", "t1", "rois", "keep", "counts", "ws"):
        assert lib.of3d_mask_open_pair(*open_args(**{k: None})) != 0 and "null" in _lib.last_error(), k
    for c in (2, -1):
        assert lib.of3d_mask_open_pair(*open_args(combine=c)) != 0 and "combine" in _lib.last_error()
    assert lib.of3d_mask_open_pair(*open_args(floor=float("nan"))) != 0 and "floor" in _lib.last_error()
    assert lib.of3d_mask_open_pair(*open_args(min_size=0)) != 0 and "min_size" in _lib.last_error()
    assert lib.of3d_mask_open_pair(*open_args(conn=8)) != 0 and "connectivity" in _lib.last_error()
    assert lib.of3d_mask_open_pair(*open_args(n_roi=17)) != 0 and "16 ROI" in _lib.last_error()

    nb = (ctypes.c_int * 4)(2, 0, 0, 0)
    D = ctypes.POINTER(ctypes.c_double)
    e = np.array([0.0, 1.0, 2.0])
    edges = (D * 4)(e.ctypes.data_as(D), None, None, None)
    pair_args = lambda **kw: [kw.get(k, v) for k, v in dict(
        vx0=p, vy0=p, vz0=p, vx1=p, vy1=p, vz1=p, f32=0, nz=2, ny=3, nx=4, sxy=1.0, sz=1.0, st=1.0, rois=rois,
        n_roi=1, keep=p, nbins=nb, edges=edges, result=p, ws=p, stream=None).items()]
    for k in ("vx0", "vy0", "vx1", "vy1", "rois", "keep", "result", "ws"):
        assert lib.of3d_flow_pair(*pair_args(**{k: None})) != 0 and "null" in _lib.last_error(), k
    for k in ("vz0", "vz1"):
        assert lib.of3d_flow_pair(*pair_args(**{k: None})) != 0 and "vz of both" in _lib.last_error(), k
    assert lib.of3d_flow_pair(*pair_args(nbins=None)) != 0 and "bins" in _lib.last_error()
    assert lib.of3d_flow_pair(*pair_args(nbins=(ctypes.c_int * 4)(0, 0, 300, 0))) != 0 and "bins" in _lib.last_error()
    assert lib.of3d_flow_pair(*pair_args(edges=None)) != 0 and "without edges" in _lib.last_error()
    bad = np.array([0.0, 2.0, 1.0])
    assert lib.of3d_flow_pair(*pair_args(edges=(D * 4)(bad.ctypes.data_as(D), None, None, None))) != 0
    assert "ascend" in _lib.last_error()
    assert lib.of3d_flow_pair(*pair_args(nz=0)) != 0 and "dims" in _lib.last_error()
    boxes[0, 1] = 3  # outside the volume
    assert lib.of3d_flow_pair(*pair_args()) != 0 and "ROI 0" in _lib.last_error()


# ---- exports ----------------------------------------------------------------------------------------
def test_package_exports():
    for name in ("channel_compare", "joint_reliability_mask"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(analysis, name)
    for name in ("of3d_mask_open_pair", "of3d_flow_pair", "of3d_flow_pair_result_bytes",
                 "of3d_flow_pair_workspace_bytes"):
        assert name in _lib.EXPORTED and hasattr(_lib.load(), name)
    assert [f.name for f in __import__("dataclasses").fields(SummarySpec)][-1] == "weighted_bins"
