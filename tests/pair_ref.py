"""numpy restatement of the two-channel comparison (tests only): figure 3's joint reliability
mask (plot_figure3_ROIfigures.m:93-96) opened per ROI with scipy.ndimage.label as
mask_ref.open_ref does, and channel_compare's sums and histograms over the jointly valid voxels
(plot_figure3_ROIfigures.m:98-193).  Sums with math.fsum (the correctly rounded sum), besides
each its sum of absolute terms for the tests' error bound; histograms with np.histogram."""
import math

import numpy as np

import mask_ref as mr
import whist_ref as wr
from summary_ref import SUMS, boxes_of  # noqa: F401  (boxes_of: re-exported for the tests)

QUANTITIES = ("dot", "cosine", "dtheta", "dmagnitude")
PAIR_SUMS = ("sum_dot", "sum_cosine", "sum_mag0_mag1", "sum_mag0_sq", "sum_mag1_sq", "sum_sin_dtheta",
             "sum_cos_dtheta", "sum_diff")

# ---- the general case ---------------------------------------------------------------------------
G_SHAPE, G_SCALES, G_ROIS = (5, 37, 67), (0.3, 1.2, 0.5), [(0, 5, 1, 36, 3, 64)]
G_BINS = {"dtheta": np.linspace(-np.pi, np.pi, 13), "cosine": np.linspace(-1, 1, 21),
          "dmagnitude": np.linspace(-8, 8, 33), "dot": np.linspace(-6, 6, 25)}


def rel_pair(shape, rng):
    """Two float32 reliabilities in [-0.25, 0.75): a quarter of each lies below the floor 0."""
    return [rng.random(shape, dtype=np.float32) - np.float32(0.25) for _ in range(2)]


def general_case(seed=11, shape=G_SHAPE):
    """(ch0, ch1), each (vx, vy, vz float64, rel float32): the rels drawn first, then the six
    velocity fields in the order vx0 vy0 vz0 vx1 vy1 vz1."""
    rng = np.random.default_rng(seed)
    rel0, rel1 = rel_pair(shape, rng)
    v = [rng.standard_normal(shape) for _ in range(6)]
    return (v[0], v[1], v[2], rel0), (v[3], v[4], v[5], rel1)


def exact_case():
    """Channels of whist_ref's exact fields (every magnitude a multiple of 1/4, scales 1) under
    the general case's kind of rel: the sums of magnitude, vx, vy, vz, dot, mag0*mag1, mag0^2 and
    mag1^2 are exact in any order."""
    f0 = wr.exact_fields(wr.EXACT_SHAPE, np.random.default_rng(3197))
    f1 = wr.exact_fields(wr.EXACT_SHAPE, np.random.default_rng(3198))
    rel0, rel1 = rel_pair(wr.EXACT_SHAPE, np.random.default_rng(11))
    return (f0[0], f0[1], f0[2], rel0), (f1[0], f1[1], f1[2], rel1)


EXACT_CH_SUMS = ("sum_magnitude", "sum_vx", "sum_vy", "sum_vz")
EXACT_PAIR_SUMS = ("sum_dot", "sum_mag0_mag1", "sum_mag0_sq", "sum_mag1_sq")


# ---- the joint mask -----------------------------------------------------------------------------
def thresholds_of(rel0, rel1, percentile):
    return np.array([np.percentile(rel0, percentile), np.percentile(rel1, percentile)], dtype=np.asarray(rel0).dtype)


def joint_mask(rel0, rel1, t0, t1, floor=0.0, combine="or"):
    """C(rel0 > t0, rel1 > t1) & (rel0 > floor) & (rel1 > floor); NaN compares false."""
    rel0, rel1 = np.asarray(rel0), np.asarray(rel1)
    with np.errstate(invalid="ignore"):
        a, b = rel0 > rel0.dtype.type(t0), rel1 > rel1.dtype.type(t1)
        c = (a | b) if combine == "or" else (a & b)
        return c & (rel0.astype(np.float64) > floor) & (rel1.astype(np.float64) > floor)


def joint_open_ref(rel0, rel1, t0, t1, boxes, min_size, connectivity, floor=0.0, combine="or"):
    """mask_ref.open_ref's (keep, counts) for the joint mask: labelled per cropped box with
    scipy.ndimage.label."""
    assert combine in ("or", "and")
    m = joint_mask(rel0, rel1, t0, t1, floor, combine)
    return mr.open_ref(m.astype(np.float32), 0.5, boxes, min_size, connectivity)


# ---- the pair summary ---------------------------------------------------------------------------
def _fsum(t):
    return math.fsum(t.tolist())


def pair_ref(ch0, ch1, keep, boxes, xyscale=1.0, zscale=1.0, tscale=1.0, bins=None, in_plane=False):
    """channel_compare's dict for a given keep volume (bit r: box r): n_valid, n_voxels, ch0 / ch1
    (the eight SUMS with abs_<sum>), the eight PAIR_SUMS with abs_<sum> and fsum_<sum> (the same
    correctly rounded value), hist / edges, and values: per ROI the four quantities' arrays."""
    shape = np.shape(ch0[0])
    vol = lambda f: np.array(f, dtype=np.float64).reshape((1,) + shape if len(shape) == 2 else shape)
    three = ch0[2] is not None and not in_plane
    f = [[vol(c[0]), vol(c[1]), vol(c[2]) if three else None] for c in (ch0, ch1)]
    keep = np.asarray(keep).reshape(f[0][0].shape)
    edges = {k: np.asarray(e, np.float64) for k, e in (bins or {}).items()}
    out = {"rois": np.asarray(boxes, dtype=np.int64), "n_valid": [], "n_voxels": [], "values": [],
           "hist": {k: [] for k in edges}, "edges": edges, "ch0": {}, "ch1": {}}
    for d in (out["ch0"], out["ch1"]):
        for k in SUMS:
            d[k], d["abs_" + k] = [], []
    for k in PAIR_SUMS:
        out[k], out["abs_" + k] = [], []

    def masked(v, m, scale):  # example_analysis_script.ipynb cell 5
        v = v * m
        v[v == 0] = np.nan
        return v * scale / tscale

    for r, (z0, z1, y0, y1, x0, x1) in enumerate(out["rois"]):
        sl = (slice(z0, z1), slice(y0, y1), slice(x0, x1))
        m = ((keep[sl] >> np.uint16(r)) & np.uint16(1)).astype(bool)
        with np.errstate(invalid="ignore", divide="ignore"):
            comp = []
            for c in range(2):
                x, y = masked(f[c][0][sl], m, xyscale), masked(f[c][1][sl], m, xyscale)
                z = masked(f[c][2][sl], m, zscale) if three else np.zeros_like(x)
                xy2 = x * x + y * y
                comp.append((x, y, z, np.sqrt(xy2 + z * z) if three else np.sqrt(xy2)))
        ok = ~(np.isnan(comp[0][3]) | np.isnan(comp[1][3]))  # badRows = isnan(theta) | isnan(theta1)
        out["n_valid"].append(int(ok.sum()))
        out["n_voxels"].append(int(ok.size))
        ch = []
        for c in range(2):
            x, y, z, mag = (a[ok] for a in comp[c])
            h = np.sqrt(x * x + y * y)
            sn, cs = y / h, x / h
            ch.append((x, y, z, mag, sn, cs))
            for k, t in zip(SUMS, (mag, x, y, z, sn, cs, mag * sn, mag * cs)):
                out[f"ch{c}"][k].append(_fsum(t))
                out[f"ch{c}"]["abs_" + k].append(_fsum(np.abs(t)))
        (x0_, y0_, z0_, m0, sn0, cs0), (x1_, y1_, z1_, m1, sn1, cs1) = ch
        dxy = x0_ * x1_ + y0_ * y1_
        dot = dxy + z0_ * z1_ if three else dxy
        cosine = dot / (m0 * m1)
        cosd, sind = cs0 * cs1 + sn0 * sn1, cs0 * sn1 - sn0 * cs1
        exy = (x1_ - x0_) ** 2 + (y1_ - y0_) ** 2
        diff = np.sqrt(exy + (z1_ - z0_) ** 2) if three else np.sqrt(exy)
        for k, t in zip(PAIR_SUMS, (dot, cosine, m0 * m1, m0 * m0, m1 * m1, sind, cosd, diff)):
            out[k].append(_fsum(t))
            out["abs_" + k].append(_fsum(np.abs(t)))
        vals = {"dot": dot, "cosine": cosine, "dtheta": np.arctan2(sind, cosd), "dmagnitude": m1 - m0,
                "terms": dict(zip(PAIR_SUMS, (dot, cosine, m0 * m1, m0 * m0, m1 * m1, sind, cosd, diff))),
                "ch_terms": [dict(zip(SUMS[:4], (c[3], c[0], c[1], c[2]))) for c in ch]}
        out["values"].append(vals)
        for k in edges:
            out["hist"][k].append(np.histogram(vals[k], bins=edges[k])[0].astype(np.uint64))
    for k in ("n_valid", "n_voxels"):
        out[k] = np.array(out[k], dtype=np.int64)
    for d in (out["ch0"], out["ch1"]):
        for k in list(d):
            d[k] = np.array(d[k])
    for k in PAIR_SUMS:
        out[k], out["abs_" + k] = np.array(out[k]), np.array(out["abs_" + k])
        out["fsum_" + k] = out[k]
    out["hist"] = {k: np.stack(v) for k, v in out["hist"].items()}
    return out


def pair_bound(ref, key, ch=None):
    """summary_ref.sum_bound's rule, (n_valid + 16) * 2^-53 * sum |term| per ROI: any summation
    order stays within n*u of the exact sum, and 16 ulp per term cover the device's sqrt / divide
    against the host's.  ch: 0 / 1 for a channel's sum, None for a cross sum."""
    a = ref["abs_" + key] if ch is None else ref[f"ch{ch}"]["abs_" + key]
    return (ref["n_valid"] + 16) * 2.0 ** -53 * a


def assert_matches(got, ref, exact_hists=QUANTITIES, bitwise=()):
    """channel_compare's dict against pair_ref's: the counts and the listed histograms exactly,
    all 24 sums within pair_bound (those named in `bitwise` bit for bit)."""
    assert np.array_equal(got["rois"], ref["rois"])
    assert np.array_equal(got["n_valid"], ref["n_valid"]), (got["n_valid"], ref["n_valid"])
    assert np.array_equal(got["n_voxels"], ref["n_voxels"])
    worst = 0.0
    for c in (0, 1):
        for k in SUMS:
            g, w = got[f"ch{c}"][k], ref[f"ch{c}"][k]
            if k in bitwise:
                assert g.tobytes() == w.tobytes(), (c, k, g, w)
            err, bound = np.abs(g - w), pair_bound(ref, k, c)
            worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
            assert np.all(err <= bound), (c, k, err, bound)
    for k in PAIR_SUMS:
        if k in bitwise:
            assert got[k].tobytes() == ref[k].tobytes(), (k, got[k], ref[k])
        err, bound = np.abs(got[k] - ref[k]), pair_bound(ref, k)
        print(k, "max err / bound:", float(np.max(err / np.maximum(bound, 1e-300))))
        assert np.all(err <= bound), (k, err, bound)
    print("channel sums: max err / bound:", worst)
    for k in exact_hists:
        if k in ref["hist"]:
            assert got["hist"][k].dtype == np.uint64 and got["hist"][k].shape == ref["hist"][k].shape
            assert np.array_equal(got["hist"][k], ref["hist"][k]), k
            assert np.array_equal(got["edges"][k], ref["edges"][k])
    assert sorted(got["hist"]) == sorted(ref["hist"])
