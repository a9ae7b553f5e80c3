"""Host side of the magnitude-weighted histograms (no GPU): SummarySpec.weighted_bins'
validation, the npz writer's round trip of weights_<name>, and the facts about the exact case
that tests/test_gpu_whist.py relies on, checked with the numpy restatement (whist_ref)."""
import ctypes
import dataclasses

import numpy as np
import pytest

import summary_ref as sr
import whist_ref as wr
from opticalflow3d_dev_amd import SummarySpec, _lib, analysis
from test_summary_cpu import _fake_summary


# ---- SummarySpec.weighted_bins ------------------------------------------------------------------
def test_spec_accepts_weighted_bins_as_last_field():
    spec = SummarySpec(bins={"theta": [-1.0, 0.0, 2.0]}, weighted_bins={"phi": [-1.0, 0.0, 0.5, 1.0], "vx": [0, 1]})
    assert [f.name for f in dataclasses.fields(SummarySpec)][-1] == "weighted_bins"
    boxes, nbins, edges = spec.resolve((4, 5, 6))  # the plain bins' triple is unchanged
    assert nbins == [0, 0, 0, 0, 2, 0] and boxes.tolist() == [[0, 4, 0, 5, 0, 6]]
    wn, we = spec.weighted(3)
    assert wn == [1, 0, 0, 0, 0, 3] and we[5].tolist() == [-1.0, 0.0, 0.5, 1.0] and we[5].dtype == np.float64
    assert we[1] is None
    assert SummarySpec().weighted(3) == ([0] * 6, [None] * 6)


@pytest.mark.parametrize("wb,shape,word", [
    ({"theta": [0.0, 1.0, 1.0]}, (4, 5, 6), "ascending"),
    ({"theta": [0.0, 2.0, 1.0]}, (4, 5, 6), "ascending"),
    ({"theta": [0.0, np.nan, 1.0]}, (4, 5, 6), "ascending"),
    ({"theta": [0.0]}, (4, 5, 6), "2 to 257"),
    ({"theta": np.arange(258.0)}, (4, 5, 6), "2 to 257"),
    ({"speed": [0.0, 1.0]}, (4, 5, 6), "unknown weighted"),
    ({"phi": [0.0, 1.0]}, (5, 6), "weighted phi histogram needs a 3D"),
    ({"vz": [0.0, 1.0]}, (5, 6), "weighted vz histogram needs a 3D"),
])
def test_spec_rejects_weighted_bins(wb, shape, word):
    with pytest.raises(ValueError, match=word):
        SummarySpec(weighted_bins=wb).resolve(shape)
    with pytest.raises(ValueError, match=word):
        SummarySpec(weighted_bins=wb).weighted(len(shape))


def test_spec_accepts_256_weighted_bins():
    assert SummarySpec(weighted_bins={"vx": np.arange(257.0)}).weighted(2)[0][0] == 256


# ---- the C ABI's host arithmetic -------------------------------------------------------------------
def test_c_abi_sizes_and_refusals():
    """The two *_bytes entry points: exactly the slots the boxes need, plus the edges."""
    lib = _lib.load()
    nb = (ctypes.c_int * 6)(0, 0, 0, 5, 0, 36)
    boxes = np.array([[0, 128, 0, 512, 0, 512], [2, 3, 4, 9, 7, 30], [0, 1, 0, 2, 0, 20000]], dtype=np.int64)
    rois = boxes.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    assert lib.of3d_flow_whist_result_bytes(3, nb) == 3 * (1 + 41) * 8
    # workgroups: 1024 (the cap), 1 (115 voxels), 2 (5 by size, capped by the 2 rows); 6 + 37 edges
    assert lib.of3d_flow_whist_workspace_bytes(rois, 3, nb) == ((1024 + 1 + 2) * 41 + 43) * 8
    boxes[1, 1] = 2  # an empty box
    assert lib.of3d_flow_whist_workspace_bytes(rois, 3, nb) == 0 and "ROI 1" in _lib.last_error()
    boxes[1, 1] = 3
    boxes[0] = [0, 2 ** 31 - 1, 0, 1, 0, 2 ** 31 - 1]  # one row per workgroup of 2^31 - 1 voxels
    assert lib.of3d_flow_whist_workspace_bytes(rois, 3, nb) == 0 and "too large" in _lib.last_error()
    boxes[0] = [0, 128, 0, 512, 0, 512]
    assert lib.of3d_flow_whist_workspace_bytes(rois, 3, (ctypes.c_int * 6)()) == 0 and "bins" in _lib.last_error()
    assert lib.of3d_flow_whist_workspace_bytes(rois, 17, nb) == 0 and "16 ROI" in _lib.last_error()
    assert lib.of3d_flow_whist_result_bytes(17, nb) == 0
    assert lib.of3d_flow_whist_result_bytes(1, (ctypes.c_int * 6)(257, 0, 0, 0, 0, 0)) == 0


# ---- writer round trip ---------------------------------------------------------------------------
def _fake_weighted(seed):
    s = _fake_summary(seed)
    rng = np.random.default_rng(1000 + seed)
    s["edges_weighted"] = {"phi": np.linspace(-1.5, 1.5, 7), "vx": np.linspace(-1, 1, 4)}
    # every float64 bit pattern class that a sum can take: tiny, huge, zero, many mantissa bits
    s["hist_weighted"] = {k: rng.standard_normal((3, e.size - 1)) * 10.0 ** rng.integers(-300, 300, (3, e.size - 1))
                          for k, e in s["edges_weighted"].items()}
    s["hist_weighted"]["phi"][1] = 0.0
    return s


def test_writer_round_trips_weights_bit_exactly(tmp_path):
    frames, sums = [3, 4, 5, 6], [_fake_weighted(i) for i in range(4)]
    prefix = str(tmp_path / "cells")
    analysis.write_summaries(prefix, frames, sums)
    assert tuple(open(prefix + "_summary.csv").readline().strip().split(",")) == analysis.CSV_COLUMNS
    npz = np.load(prefix + "_summary_hist.npz")
    assert sorted(npz.files) == sorted(["frames", "edges_vx", "counts_vx", "edges_theta", "counts_theta", "wedges_phi",
                                        "weights_phi", "wedges_vx", "weights_vx"])
    for k in ("phi", "vx"):
        want = np.stack([s["hist_weighted"][k] for s in sums])
        got = npz["weights_" + k]
        assert got.dtype == np.float64 and got.shape == (4, 3, sums[0]["edges_weighted"][k].size - 1)
        assert got.tobytes() == want.tobytes()
        assert np.array_equal(npz["wedges_" + k], sums[0]["edges_weighted"][k])
    assert np.array_equal(npz["counts_vx"], np.stack([s["hist"]["vx"] for s in sums]))


def test_files_without_weighted_bins_are_as_before(tmp_path):
    frames, plain = [3, 4], [_fake_summary(i) for i in range(2)]
    analysis.write_summaries(str(tmp_path / "a"), frames, plain)
    analysis.write_summaries(str(tmp_path / "b"), frames, [_fake_weighted(i) for i in range(2)])
    a, b = np.load(tmp_path / "a_summary_hist.npz"), np.load(tmp_path / "b_summary_hist.npz")
    assert sorted(a.files) == ["counts_theta", "counts_vx", "edges_theta", "edges_vx", "frames"]
    assert sorted(set(b.files) - set(a.files)) == ["wedges_phi", "wedges_vx", "weights_phi", "weights_vx"]
    for k in a.files:  # and the weighted arrays come on top of them, changing none
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
    assert (tmp_path / "a_summary.csv").read_text() == (tmp_path / "b_summary.csv").read_text()


# ---- the exact case of test_gpu_whist.py ---------------------------------------------------------
def test_exact_case_is_exact_in_any_order():
    vx, vy, vz, rel = wr.exact_case()
    assert vx.shape == (6, 21, 67) and rel.dtype == np.float32
    spec = SummarySpec(rois=wr.EXACT_ROIS, weighted_bins=wr.EXACT_BINS, rel_percentile=50)
    assert spec.resolve(vx.shape)[0].shape == (3, 6) and spec.weighted(3)[0] == [0, 0, 0, 5, 12, 14]
    ref = wr.whist_ref(vx, vy, vz, rel, 50, rois=wr.EXACT_ROIS, weighted_bins=wr.EXACT_BINS)
    assert ref["n_valid"].tolist() == [4221, 2083, 53]
    sr.assert_clear_of_edges(wr.with_bins(ref, wr.EXACT_BINS), tuple(wr.EXACT_BINS))
    rng = np.random.default_rng(5)
    for r, vals in enumerate(ref["values"]):
        perm = rng.permutation(vals["magnitude"].size)
        for k, e in wr.EXACT_BINS.items():
            shuffled = np.histogram(vals[k][perm], bins=e, weights=vals["magnitude"][perm])[0]
            assert shuffled.tobytes() == ref["hist_weighted"][k][r].tobytes(), (r, k)
            assert ref["fsum_weighted"][k][r].tobytes() == ref["hist_weighted"][k][r].tobytes(), (r, k)
            # every valid voxel lies in a bin: a row's total is the sum of the magnitudes
            assert ref["count_weighted"][k][r].sum() == ref["n_valid"][r]
            assert ref["hist_weighted"][k][r].sum() == ref["sum_magnitude"][r]


def test_whist_ref_bins_as_numpy_does():
    """whist_ref's own bin rule (for the per-bin fsum) against np.histogram's, values on edges
    and outside included."""
    e = SummarySpec(weighted_bins={"vx": [-1, 0, 0.5, 2]}).weighted(2)[1][0]  # as the device gets them
    vals = {"magnitude": np.array([1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0]),
            "vx": np.array([-1.0, 0.0, 0.25, 2.0, 2.5, -1.5, 0.5])}
    ref = wr.whist_ref(None, None, None, None, ref={"values": [vals]}, weighted_bins={"vx": e})
    assert ref["hist_weighted"]["vx"].tolist() == [[1.0, 6.0, 72.0]]
    assert ref["fsum_weighted"]["vx"].tolist() == [[1.0, 6.0, 72.0]]
    assert ref["count_weighted"]["vx"].tolist() == [[1, 2, 2]]
    assert np.array_equal(wr.bin_bound(ref, "vx"), np.array([[17 * 1.0, 18 * 6.0, 18 * 72.0]]) * 2.0 ** -53)
