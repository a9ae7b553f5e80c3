"""Host side of the projection maps (no GPU): ProjectionSpec.resolve's defaults and refusals,
the public names, write_projections' round trip, and project_ref's loops against independent
numpy expressions of the same maps."""
import dataclasses

import numpy as np
import pytest

import project_ref as pj
import quiver_ref as qr
from opticalflow3d_dev_amd import ProjectionSpec, SummarySpec, analysis


# ---- ProjectionSpec -------------------------------------------------------------------------------
def test_spec_fields():
    assert [f.name for f in dataclasses.fields(ProjectionSpec)] == ["axes", "maps", "rois", "image"]
    assert [f.name for f in dataclasses.fields(SummarySpec)][-1] == "weighted_bins"


def test_public_names():
    import opticalflow3d_dev_amd as pkg

    for name in ("ProjectionSpec", "projection_maps"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(analysis, name)
    assert analysis.PROJECT_MAPS == pj.FLOW_MAPS + pj.IMAGE_MAPS and analysis.PROJECT_AXES == pj.AXES


def test_defaults_3d():
    rois, axes, abits, maps, mbits = ProjectionSpec().resolve(3, 3)
    assert rois == (1, 2) and axes == ("z",) and abits == 1
    assert maps == pj.FLOW_MAPS and mbits == 0x7F
    assert ProjectionSpec().resolve(3, 1)[0] == (0,)
    _, _, _, maps, mbits = ProjectionSpec(image=True).resolve(3, 2)
    assert maps == pj.FLOW_MAPS + pj.IMAGE_MAPS and mbits == 0x1FF


def test_defaults_2d():
    rois, axes, abits, maps, mbits = ProjectionSpec().resolve(2, 2)
    assert rois == (1,) and axes == ("y", "x") and abits == 6
    assert maps == tuple(n for n in pj.FLOW_MAPS if n != "sum_vz") and mbits == 0x6F
    assert ProjectionSpec(image=True).resolve(2, 2)[4] == 0x1EF


def test_names_come_back_in_bit_order():
    _, axes, abits, maps, mbits = ProjectionSpec(axes=["x", "z"], maps=("max_image", "n_valid"), rois=[2, 0],
                                                 image=True).resolve(3, 3)
    assert axes == ("z", "x") and abits == 5 and maps == ("n_valid", "max_image") and mbits == 0x82


@pytest.mark.parametrize("kw,ndim,word", [
    (dict(axes=("z",)), 2, "no z axis"),
    (dict(axes="z"), 3, "not a sequence"),
    (dict(axes=()), 3, "no name"),
    (dict(axes=("w",)), 3, "unknown name"),
    (dict(axes=("y", "y")), 3, "duplicate"),
    (dict(axes=3), 3, "not a sequence"),
    (dict(maps=("sum_vz",)), 2, "no sum_vz"),
    (dict(maps=("max_image",)), 3, "image=True"),
    (dict(maps=("sum_image", "n_mask")), 3, "image=True"),
    (dict(maps=("speed",)), 3, "unknown name"),
    (dict(maps=()), 3, "no name"),
    (dict(maps="n_mask"), 3, "not a sequence"),
    (dict(rois=(3,)), 3, "out of range"),
    (dict(rois=()), 3, "non-empty"),
    (dict(rois=(1, 1)), 3, "duplicate"),
    (dict(rois=(1.5,)), 3, "ROI indices"),
    (dict(rois=4), 3, "not a sequence"),
])
def test_spec_refuses(kw, ndim, word):
    with pytest.raises(ValueError, match="^project: .*" + word):
        ProjectionSpec(**kw).resolve(ndim, 3)


def test_field_spec_messages_keep_their_prefix():
    with pytest.raises(ValueError, match="^fields: ROI index out of range"):
        analysis.FieldSpec(rois=(7,)).resolve(3, 2)


# ---- write_projections ----------------------------------------------------------------------------
def _fields(shape, seed):
    f = qr.planted_fields(shape, seed)
    img = np.random.default_rng(seed + 1).integers(0, 65536, size=shape).astype(np.uint16)
    return f, img


def test_write_projections_round_trip(tmp_path):
    f, img = _fields((5, 9, 14), 3)
    ref = pj.project_ref(*f, image=img, rel_percentile=60, rois=[(1, 4, 2, 9, 3, 12)], axes=("z", "x"))
    path = tmp_path / "p.npz"
    analysis.write_projections(path, ref)
    back = analysis.read_projections(path)
    assert back["threshold"] == ref["threshold"] and np.array_equal(back["rois"], ref["rois"])
    assert back["axes"] == ref["axes"] and [e["roi"] for e in back["maps"]] == [0, 1]
    for e, want in zip(back["maps"], ref["maps"]):
        assert e["box"] == want["box"]
        for a in ref["axes"]:
            assert sorted(e[a]) == sorted(want[a])
            for name, v in want[a].items():
                assert e[a][name].dtype == v.dtype and e[a][name].tobytes() == v.tobytes(), (a, name)


# ---- project_ref against independent expressions ----------------------------------------------------
@pytest.mark.parametrize("shape,rois", [((6, 11, 17), [(1, 5, 2, 11, 3, 16)]), ((13, 19), [(2, 12, 1, 18)])])
def test_ref_agrees_with_reductions(shape, rois):
    f, img = _fields(shape, 11)
    vx, vy, vz, rel = f
    scales = dict(xyscale=0.5, zscale=2.0, tscale=0.25)
    ref = pj.project_ref(vx, vy, vz, rel, image=img, rel_percentile=55, rois=rois, **scales)
    t = ref["threshold"]
    vol = lambda a: a.reshape((1,) + shape) if len(shape) == 2 else a
    x, y, z, mag = qr.physical_fields(vx, vy, vz, rel > t, *scales.values())
    valid = vol(~np.isnan(mag))
    assert 0 < valid.sum() < (rel > t).sum()  # planted zeros inside the mask
    for e in ref["maps"]:
        z0, z1, y0, y1, x0, x1 = e["box"]
        sl = (slice(z0, z1), slice(y0, y1), slice(x0, x1))
        for a in ref["axes"]:
            k, m = pj.AXES.index(a), e[a]
            shp = m["n_mask"].shape
            assert np.array_equal(m["n_mask"], vol(rel > t)[sl].sum(k).reshape(shp))
            assert np.array_equal(m["n_valid"], valid[sl].sum(k).reshape(shp))
            assert np.array_equal(m["max_image"], np.fmax.reduce(vol(img)[sl].astype(np.float64), k).reshape(shp))
            assert np.array_equal(m["sum_image"], vol(img)[sl].astype(np.float64).sum(k).reshape(shp))  # integers: exact
            with np.errstate(invalid="ignore"):
                want = np.fmax.reduce(np.where(valid[sl], vol(mag)[sl], np.nan), k).reshape(shp)
            assert np.array_equal(m["max_magnitude"], want, equal_nan=True)
            assert np.array_equal(np.isnan(m["max_magnitude"]), m["n_valid"] == 0)
            s = np.where(valid[sl], vol(x)[sl], 0.0).sum(k).reshape(shp)  # another order: close, not equal
            assert np.allclose(m["sum_vx"], s, rtol=1e-12, atol=1e-12)
            assert m["mean_image"].tobytes() == (m["sum_image"] / float(e["box"][2 * k + 1] - e["box"][2 * k])).tobytes()


def test_ref_special_lines():
    """A line without a valid voxel: NaN maximum, +0.0 sums; an all-NaN image line: NaN maximum and sum."""
    shape = (4, 5, 6)
    vx, vy, vz = (np.ones(shape) for _ in range(3))
    rel = np.ones(shape, np.float32)
    rel[:, 2, 3] = 0.0
    img = np.ones(shape, np.float32)
    img[:, 1, 1] = np.nan
    img[0, 0, 0] = np.nan
    m = pj.project_ref(vx, vy, vz, rel, image=img, threshold=0.5, axes=("z",))["maps"][0]["z"]
    assert m["n_mask"][2, 3] == 0 and np.isnan(m["max_magnitude"][2, 3]) and np.isnan(m["mean_vx"][2, 3])
    assert m["sum_vx"][2, 3].tobytes() == np.float64(0.0).tobytes()
    assert np.isnan(m["max_image"][1, 1]) and np.isnan(m["sum_image"][1, 1])
    assert m["max_image"][0, 0] == 1.0 and np.isnan(m["sum_image"][0, 0])
    assert m["sum_vx"][0, 0] == 4.0 and m["max_magnitude"][0, 0] == np.sqrt(3.0)
