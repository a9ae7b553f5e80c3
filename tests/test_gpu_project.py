"""Projection maps on the device (csrc/kt_project.hip: of3d_flow_project) against the numpy
restatement tests/project_ref.py.  Every comparison is exact: the counts by array_equal, the
float maps bit for bit — the sums are the same loop on both sides.  Two things the arithmetic
standard leaves open are compared by value instead: the image maximum (the sign of a zero
maximum is unspecified), and a NaN, which must sit in the same element but may carry another
sign or payload (inf - inf is -NaN on the host and +NaN on the device)."""
import numpy as np
import pytest

import mask_ref as mr
import project_ref as pj
import quiver_ref as qr
from opticalflow3d_dev_amd import ProjectionSpec, flow_summary, projection_maps
from opticalflow3d_dev_amd import _lib
from opticalflow3d_dev_amd.analysis import _ProjectCall, _cuda_device

pytestmark = pytest.mark.gpu

SCALES = dict(xyscale=0.3, zscale=1.2, tscale=0.5)
ALL = ProjectionSpec(axes=("z", "y", "x"), rois=None, image=True)
SHAPE = (7, 37, 131)
ROIS = [(1, 6, 3, 21, 5, 70), (0, 7, 0, 37, 1, 131)]  # dx 65 and 130, odd x0; overlapping


def same_floats(a, b):
    """Equal NaN positions, equal bytes elsewhere (so the sign of a zero counts)."""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return (a.dtype == b.dtype == np.float64 and a.shape == b.shape and np.array_equal(nan, np.isnan(b))
            and np.where(nan, 0.0, a).tobytes() == np.where(nan, 0.0, b).tobytes())


def assert_same(got, ref, names=None):
    """projection_maps' dict against project_ref's (which holds every ROI and map)."""
    assert got["threshold"].dtype == np.asarray(ref["threshold"]).dtype
    assert got["threshold"] == ref["threshold"] or (np.isnan(got["threshold"]) and np.isnan(ref["threshold"]))
    assert np.array_equal(got["rois"], ref["rois"])
    for e in got["maps"]:
        w = ref["maps"][e["roi"]]
        assert e["box"] == w["box"]
        for a in got["axes"]:
            if names is None:
                assert set(e[a]) == set(w[a]), (e["roi"], a, sorted(e[a]), sorted(w[a]))
            else:
                assert set(names) <= set(e[a]) <= set(w[a]), (e["roi"], a, sorted(e[a]))
            for name, v in e[a].items():
                want, where = w[a][name], (e["roi"], a, name)
                assert v.shape == want.shape and v.dtype == want.dtype, where + (v.shape, want.shape, v.dtype)
                if name in ("n_mask", "n_valid"):
                    assert v.dtype == np.int64 and np.array_equal(v, want), where
                elif name == "max_image":
                    assert np.array_equal(v, want, equal_nan=True), where
                else:
                    assert same_floats(v, want), where


def image_of(shape, seed, dtype=np.uint16):
    """An image with values in the upper half of an unsigned type's range."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    if dtype.kind == "f":
        return (rng.standard_normal(shape) * 1000).astype(dtype)
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max, size=shape, endpoint=True, dtype=np.int64).astype(dtype)


# ---- 1. odd boxes, every axis, every map, the four dtype pairs ----------------------------------------
@pytest.mark.parametrize("v_dtype,rel_dtype", [(np.float64, np.float32), (np.float64, np.float64),
                                               (np.float32, np.float32), (np.float32, np.float64)])
def test_odd_boxes_all_axes(v_dtype, rel_dtype):
    f, img = qr.planted_fields(SHAPE, 41, v_dtype=v_dtype, rel_dtype=rel_dtype), image_of(SHAPE, 42)
    ref = pj.project_ref(*f, image=img, rel_percentile=60, **SCALES, rois=ROIS)
    got = projection_maps(*f, image=img, spec=ProjectionSpec(axes=("z", "y", "x"), rois=(0, 1, 2), image=True),
                          rel_percentile=60, **SCALES, rois=ROIS)
    assert got["axes"] == ("z", "y", "x") and [e["roi"] for e in got["maps"]] == [0, 1, 2]
    assert got["maps"][1]["z"]["n_mask"].shape == (18, 65) and got["maps"][2]["x"]["sum_vx"].shape == (7, 37)
    assert got["maps"][1]["y"]["max_image"].shape == (5, 65)
    for e in ref["maps"]:
        for a in "zyx":
            assert 0 < e[a]["n_valid"].sum() < e[a]["n_mask"].sum()  # the planted zeros
    assert_same(got, ref)


def test_default_spec_is_along_z_for_every_roi_after_0():
    f = qr.planted_fields(SHAPE, 43)
    got = projection_maps(*f, rel_percentile=60, rois=ROIS)
    assert got["axes"] == ("z",) and [e["roi"] for e in got["maps"]] == [1, 2]
    assert sorted(got["maps"][0]["z"]) == sorted(pj.FLOW_MAPS + ("mean_vx", "mean_vy", "mean_vz", "mean_magnitude"))
    assert_same(got, pj.project_ref(*f, rel_percentile=60, rois=ROIS))


def test_lines_of_length_one():
    f, img = qr.planted_fields(SHAPE, 44), image_of(SHAPE, 45)
    rois = [(3, 4, 0, 37, 0, 131), (0, 7, 5, 6, 0, 131), (0, 7, 0, 37, 64, 65), (2, 3, 4, 5, 6, 7)]
    ref = pj.project_ref(*f, image=img, rel_percentile=50, **SCALES, rois=rois)
    assert_same(projection_maps(*f, image=img, spec=ALL, rel_percentile=50, **SCALES, rois=rois), ref)


# ---- 2. special values ----------------------------------------------------------------------------------
def special_fields():
    shape = (6, 21, 70)
    rng = np.random.default_rng(46)
    vx, vy, vz = (rng.standard_normal(shape) for _ in range(3))
    rel = (rng.random(shape) * 0.5 + 0.5).astype(np.float32)  # all above 0.5 ...
    rel.reshape(-1)[rng.choice(rel.size, rel.size // 3, replace=False)] = 0.25  # ... but a third
    inside = np.argwhere(rel > 0.4)
    outside = np.argwhere(rel < 0.4)
    put = lambda a, where, v: a.__setitem__(tuple(where), v)
    for i, v in enumerate((0.0, -0.0, np.inf, -np.inf, np.nan, 0.0, -0.0, np.inf, -np.inf, np.nan) * 6):
        put((vx, vy, vz)[i % 3], inside[7 * i + 3], v)
        put((vx, vy, vz)[(i + 1) % 3], outside[5 * i + 2], v)
    for a in (vx, vy, vz):  # +inf and -inf on one line of every axis: their sum is NaN
        a[1, 2, 3], a[4, 2, 3], a[1, 9, 3], a[1, 2, 40] = np.inf, -np.inf, -np.inf, -np.inf
    rel[1, 2, 3] = rel[4, 2, 3] = rel[1, 9, 3] = rel[1, 2, 40] = 1.0
    rel[:, 5, 6] = rel[2, :, 7] = rel[3, 8, :] = 0.125  # whole lines below the threshold
    return [vx, vy, vz, rel]


def test_special_values():
    f = special_fields()
    ref = pj.project_ref(*f, threshold=0.4, **SCALES, rois=[(1, 6, 1, 20, 3, 68)])
    got = projection_maps(*f, spec=ProjectionSpec(axes=("z", "y", "x"), rois=(0, 1)), threshold=0.4, **SCALES,
                          rois=[(1, 6, 1, 20, 3, 68)])
    assert_same(got, ref)
    whole = got["maps"][0]
    for a in "zyx":
        assert np.any(whole[a]["n_mask"] > whole[a]["n_valid"])  # exact zeros, NaNs inside the mask
        assert np.any(np.isinf(whole[a]["sum_vx"])) and np.any(np.isinf(whole[a]["max_magnitude"]))
    assert np.isnan(whole["z"]["sum_vx"][2, 3]) and np.isnan(whole["y"]["sum_vy"][1, 3])
    assert np.isnan(whole["x"]["sum_vz"][1, 2]) and whole["x"]["max_magnitude"][1, 2] == np.inf
    zero = np.float64(0.0).tobytes()
    for a, at in (("z", (5, 6)), ("y", (2, 7)), ("x", (3, 8))):  # the lines below the threshold
        m = whole[a]
        assert m["n_mask"][at] == 0 and m["n_valid"][at] == 0 and np.isnan(m["max_magnitude"][at])
        assert np.isnan(m["mean_vx"][at])
        for k in ("sum_vx", "sum_vy", "sum_vz", "sum_magnitude"):
            assert m[k][at].tobytes() == zero, (a, k)


def test_threshold_minus_infinity_and_percentile_100():
    f = special_fields()
    spec = ProjectionSpec(axes=("z", "y", "x"), rois=(0,))
    ref = pj.project_ref(*f, threshold=-np.inf, **SCALES)
    assert np.all(ref["maps"][0]["z"]["n_mask"] == 6)
    assert_same(projection_maps(*f, spec=spec, threshold=-np.inf, **SCALES), ref)
    ref = pj.project_ref(*f, rel_percentile=100, **SCALES)
    got = projection_maps(*f, spec=spec, rel_percentile=100, **SCALES)
    assert_same(got, ref)
    for a in "zyx":
        m = got["maps"][0][a]
        assert not m["n_mask"].any() and not m["n_valid"].any() and np.all(np.isnan(m["max_magnitude"]))
        assert m["sum_magnitude"].tobytes() == np.zeros_like(m["sum_magnitude"]).tobytes()


# ---- 3. the opened mask ---------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [None, 6])
def test_opened_mask_of_overlapping_rois(connectivity):
    from scipy import ndimage

    shape = (8, 30, 70)
    rel = ndimage.gaussian_filter(np.random.default_rng(47).standard_normal(shape), 1.0).astype(np.float32)
    vx, vy, vz = qr.planted_fields(shape, 48)[:3]
    rois = [(1, 7, 2, 25, 3, 50), (0, 8, 10, 30, 31, 70)]
    boxes, thresh = mr.boxes_of(shape, rois), np.percentile(rel, 85)
    keep, counts = mr.open_ref(rel, thresh, boxes, 3, connectivity or 26)
    assert np.all(counts["n_kept"] < counts["n_mask"]) and np.all(counts["n_kept"] > 0)
    inter = keep[1:7, 10:25, 31:50]
    assert np.any((inter >> 1 & 1) != (inter >> 2 & 1))  # bit r matters where the boxes overlap
    ref = pj.project_ref(vx, vy, vz, rel, rel_percentile=85, **SCALES, rois=rois, keep=keep)
    got = projection_maps(vx, vy, vz, rel, spec=ProjectionSpec(axes=("z", "y", "x"), rois=(0, 1, 2)),
                          rel_percentile=85, **SCALES, rois=rois, min_size=3, connectivity=connectivity)
    assert_same(got, ref)
    for r in range(3):
        assert got["maps"][r]["x"]["n_mask"].sum() == counts["n_kept"][r]


# ---- 4. skip bits -----------------------------------------------------------------------------------------
def test_one_roi_of_three_equals_its_maps_in_the_full_request():
    f, img = qr.planted_fields(SHAPE, 49), image_of(SHAPE, 50)
    kw = dict(image=img, rel_percentile=60, **SCALES, rois=ROIS, min_size=2)
    full = projection_maps(*f, spec=ProjectionSpec(axes=("z", "y", "x"), rois=(0, 1, 2), image=True), **kw)
    one = projection_maps(*f, spec=ProjectionSpec(axes=("z", "y", "x"), rois=(2,), image=True), **kw)
    assert [e["roi"] for e in one["maps"]] == [2]
    for a in "zyx":
        assert sorted(one["maps"][0][a]) == sorted(full["maps"][2][a])
        for name, v in one["maps"][0][a].items():
            assert v.tobytes() == full["maps"][2][a][name].tobytes(), (a, name)


def test_fifteen_rois_work_and_sixteen_raise():
    f = qr.planted_fields((5, 20, 40), 51)
    rois = [(0, 5, i, i + 4, 2 * i + 1, 2 * i + 9) for i in range(15)]
    ref = pj.project_ref(*f, rel_percentile=50, rois=rois)
    got = projection_maps(*f, spec=ProjectionSpec(axes=("x", "z"), rois=(15, 3)), rel_percentile=50, rois=rois)
    assert [e["roi"] for e in got["maps"]] == [15, 3]
    assert_same(got, ref)
    with pytest.raises((ValueError, RuntimeError)):
        projection_maps(*f, rel_percentile=50, rois=rois + [(0, 5, 0, 20, 0, 40)])


# ---- 5. the image ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64])
def test_image_dtypes(dtype):
    shape = (5, 12, 70)
    f, img = qr.planted_fields(shape, 52), image_of(shape, 53, dtype)
    if np.dtype(dtype).kind == "f":
        img[:, 3, 4] = img[1, :, 5] = img[2, 6, :] = np.nan  # all-NaN lines along every axis
        img[0, 0, :5] = np.nan
        img[3, 1, 1] = -0.0
    rois = [(1, 5, 2, 11, 3, 68)]
    spec = ProjectionSpec(axes=("z", "y", "x"), maps=("max_image", "sum_image", "n_mask"), rois=(0, 1), image=True)
    ref = pj.project_ref(*f, image=img, rel_percentile=50, rois=rois)
    got = projection_maps(*f, image=img, spec=spec, rel_percentile=50, rois=rois)
    assert_same(got, ref, names=("max_image", "sum_image", "mean_image", "n_mask"))
    assert "sum_vx" not in got["maps"][0]["z"]
    top = got["maps"][0]["z"]["max_image"]
    if dtype is np.uint16:
        assert top.max() >= 32768 and np.any(got["maps"][1]["x"]["max_image"] >= 32768)
    if dtype is np.uint32:
        assert top.max() >= 2 ** 31 and np.any(got["maps"][1]["x"]["max_image"] >= 2 ** 31)
    if np.dtype(dtype).kind == "f":
        assert np.isnan(top[3, 4]) and np.isnan(got["maps"][0]["y"]["max_image"][1, 5])
        assert np.isnan(got["maps"][0]["x"]["max_image"][2, 6]) and not np.isnan(got["maps"][0]["x"]["max_image"][0, 0])
        assert np.isnan(got["maps"][0]["x"]["sum_image"][0, 0])


def test_image_argument_and_spec_must_agree():
    f = qr.planted_fields((3, 8, 9), 54)
    with pytest.raises(ValueError, match="^project: an image"):
        projection_maps(*f, spec=ProjectionSpec(image=True))
    with pytest.raises(ValueError, match="^project: an image"):
        projection_maps(*f, image=np.zeros((3, 8, 9), np.uint8))
    with pytest.raises(ValueError, match="^project: image shape"):
        projection_maps(*f, image=np.zeros((3, 8, 8), np.uint8), spec=ProjectionSpec(image=True))
    with pytest.raises(TypeError, match="^project: image dtype"):
        projection_maps(*f, image=np.zeros((3, 8, 9), np.int8), spec=ProjectionSpec(image=True))


# ---- 6. 2D ------------------------------------------------------------------------------------------------
def test_2d_profiles():
    shape = (23, 70)
    f, img = qr.planted_fields(shape, 55, rel_dtype=np.float64), image_of(shape, 56, np.int16)
    rois = [(2, 19, 3, 68)]
    ref = pj.project_ref(*f, image=img, rel_percentile=55, xyscale=0.3, tscale=0.5, rois=rois)
    got = projection_maps(*f, image=img, spec=ProjectionSpec(rois=(0, 1), image=True), rel_percentile=55,
                          xyscale=0.3, tscale=0.5, rois=rois)
    assert got["axes"] == ("y", "x") and "sum_vz" not in got["maps"][0]["y"]
    assert got["maps"][1]["y"]["n_mask"].shape == (65,) and got["maps"][1]["x"]["sum_vx"].shape == (17,)
    assert 0 < ref["maps"][1]["x"]["n_valid"].sum() < ref["maps"][1]["x"]["n_mask"].sum()
    assert_same(got, ref)
    with pytest.raises(ValueError, match="^project: a 2D volume has no z axis"):
        projection_maps(*f, spec=ProjectionSpec(axes=("z",)))


# ---- 7. consistency with the frame summary --------------------------------------------------------------
def test_counts_add_up_to_the_summary():
    f = qr.planted_fields(SHAPE, 57)
    s = flow_summary(*f, 60, **SCALES, rois=ROIS)
    got = projection_maps(*f, spec=ProjectionSpec(axes=("z", "y", "x"), rois=(0, 1, 2)), rel_percentile=60, **SCALES,
                          rois=ROIS)
    assert got["threshold"] == s["threshold"]
    for e in got["maps"]:
        z0, z1, y0, y1, x0, x1 = e["box"]
        n_mask = int((f[3] > got["threshold"])[z0:z1, y0:y1, x0:x1].sum())
        for a in "zyx":
            assert e[a]["n_valid"].sum() == s["n_valid"][e["roi"]] and e[a]["n_mask"].sum() == n_mask, (e["roi"], a)


# ---- 8. many workgroups, lines longer than any tile -----------------------------------------------------
def test_larger_volume():
    shape = (40, 150, 300)
    f, img = qr.planted_fields(shape, 58, v_dtype=np.float32), image_of(shape, 59)
    rois = [(3, 38, 7, 149, 11, 296)]
    ref = pj.project_ref(*f, image=img, rel_percentile=70, **SCALES, rois=rois)
    got = projection_maps(*f, image=img, spec=ProjectionSpec(axes=("z", "y", "x"), rois=(0, 1), image=True),
                          rel_percentile=70, **SCALES, rois=rois)
    assert_same(got, ref)


# ---- 9. inputs, repeatability, guards -------------------------------------------------------------------
def test_numpy_and_device_inputs_give_the_same_bits():
    import torch

    f, img = qr.planted_fields(SHAPE, 60), image_of(SHAPE, 61, np.int32)
    kw = dict(spec=ALL, rel_percentile=60, **SCALES, rois=ROIS)
    a = projection_maps(*f, image=img, **kw)
    dev = _cuda_device(None)
    b = projection_maps(*(torch.as_tensor(x).to(dev) for x in f), image=torch.as_tensor(img).to(dev), **kw)
    c = projection_maps(*f, image=img, **kw)
    for other in (b, c):
        assert other["threshold"] == a["threshold"]
        for e, w in zip(other["maps"], a["maps"]):
            for ax in "zyx":
                assert sorted(e[ax]) == sorted(w[ax])
                for name, v in e[ax].items():
                    assert v.tobytes() == w[ax][name].tobytes(), (ax, name)


@pytest.mark.parametrize("masked", [False, True])
def test_every_byte_of_the_block_is_written_and_nothing_outside_it(masked):
    """The result block between 64 guard words on either side, all filled with 0xA5, then with
    0x5A: the guards stay, the block's words are the same after both (so none kept its fill), and
    they decode to the reference.  The pass has no workspace."""
    import torch

    f, img = qr.planted_fields(SHAPE, 62), image_of(SHAPE, 63)
    boxes = mr.boxes_of(SHAPE, ROIS + [(2, 5, 7, 30, 9, 40)])  # plane sizes 23 * 31, 3 * 31, 3 * 23: odd ones, padded
    thresh = np.float32(0.5)
    keep = mr.open_ref(f[3], thresh, boxes, 2, 26)[0] if masked else None
    dev = _cuda_device(None)
    t = [torch.as_tensor(a).to(dev) for a in f + [img.view(np.int16)]]
    tk = torch.as_tensor(keep.view(np.int16)).to(dev) if masked else None
    thr = torch.tensor([thresh], dtype=torch.float32, device=dev)
    call = _ProjectCall(boxes, SHAPE, False, ProjectionSpec(axes=("z", "y", "x"), rois=(0, 2, 3), image=True), 3,
                        tuple(SCALES.values()))
    call.bind_image(t[4].data_ptr(), _lib.OF3D_U16)
    n, blocks = call.result_bytes // 8, []
    for fill in (0xA5, 0x5A):
        buf = torch.full(((n + 128) * 8,), fill, dtype=torch.uint8, device=dev)
        assert buf.data_ptr() % 16 == 0
        call.enqueue(tuple(x.data_ptr() for x in t[:4]) + (False,), thr.data_ptr(), tk.data_ptr() if masked else None,
                     buf.data_ptr() + 64 * 8, torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        raw = buf.cpu().numpy()
        assert np.all(raw[:64 * 8] == fill) and np.all(raw[-64 * 8:] == fill), "a guard word was written"
        blocks.append(raw[64 * 8:-64 * 8].copy())
    assert blocks[0].tobytes() == blocks[1].tobytes(), "a byte of the block kept its fill"
    words = blocks[0].view(np.int64)
    assert words[6] == n and words[7] == 0
    got = {"threshold": np.float32(words[:1].view(np.float64)[0]), "rois": boxes, "axes": call.axes,
           "maps": call.decode(words)}
    assert_same(got, pj.project_ref(*f, image=img, threshold=thresh, **SCALES, rois=ROIS + [(2, 5, 7, 30, 9, 40)],
                                    keep=keep))
