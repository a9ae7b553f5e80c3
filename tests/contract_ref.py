"""CPU restatement of the contractility analysis (tests only): plot_figure2_movie.ipynb cell 1 of
the reference with scipy / numpy.

largest_ref: the largest connected component of (rel > thresh) cropped to every ROI, by
scipy.ndimage.label, np.bincount and argmax (the first maximum = the lowest raster-order label,
which is what the notebook's stable descending sort keeps).
contract_ref: center_of_mass of the integer mask and, per valid voxel, the notebook's expressions
for the angle between the velocity and the direction to that centre — with np.clip before arccos,
the stated deviation of of3d_flow_contract —, reduced as summary_ref reduces: math.fsum sums with
their sums of absolute terms, np.histogram counts.
The inputs of the GPU tests are built here too, so that tests/test_contract_cpu.py can check the
conditions they must meet (clear of the bin edges, |dot| away from 1) without a GPU."""
import math

import numpy as np
from scipy import ndimage

import mask_ref as mr
from summary_ref import boxes_of  # noqa: F401  (re-exported for the tests)

SUMS = ("sum_angle", "sum_dot", "sum_inward", "sum_speed")
QUANTITIES = ("angle", "inward")
U = 2.0 ** -53
# Rounded operations in the expression tree of `dot` from the scaled velocities and the integer
# coordinates (3D; 2D has fewer): dx dy dz 3 x (two products, one difference) = 9; nd three
# squares, two sums, one root = 6; speed likewise 6; three v/speed, three -d/nd, three products,
# two sums = 11.  After the two normalisations every intermediate is at most 1 in magnitude, so
# each rounding moves dot by at most 2^-53: |dot_device - dot_exact| <= K_DOT * 2^-53.
K_DOT = 9 + 6 + 6 + 11
DOT_LIMIT = 1.0 - 1e-6  # no reference |dot| above this but in the constructed aligned case
EDGE_MARGIN = 1e-9      # >= (180/pi) * K_DOT * 2^-53 / sqrt(1 - DOT_LIMIT^2) + 16 ulp of 180 = 1.5e-10


def largest_ref(rel, thresh, boxes, connectivity):
    """keep (uint16, rel's shape; bit r: in box r and in the largest component of (rel > thresh)
    cropped to box r) and a dict of of3d_mask_open's four int64 count arrays."""
    rel = np.asarray(rel)
    vol = rel.reshape((1,) + rel.shape) if rel.ndim == 2 else rel
    assert connectivity in ((4, 8) if rel.ndim == 2 else (6, 18, 26))
    with np.errstate(invalid="ignore"):
        mask = vol > thresh
    keep = np.zeros(vol.shape, np.uint16)
    counts = {k: [] for k in mr.COUNTS}
    for r, (z0, z1, y0, y1, x0, x1) in enumerate(np.asarray(boxes)):
        sl = (slice(z0, z1), slice(y0, y1), slice(x0, x1))
        m = mask[sl]
        if rel.ndim == 2:
            lab, n = ndimage.label(m[0], ndimage.generate_binary_structure(2, mr._RANK[connectivity]))
            lab = lab[None]
        else:
            lab, n = ndimage.label(m, ndimage.generate_binary_structure(3, mr._RANK[connectivity]))
        sizes = np.bincount(lab.ravel(), minlength=n + 1)
        sizes[0] = 0  # label 0 is the background
        kept = (lab == int(np.argmax(sizes))) & (lab != 0) if n else np.zeros(m.shape, bool)
        keep[sl] |= kept.astype(np.uint16) << np.uint16(r)
        counts["n_mask"].append(int(m.sum()))
        counts["n_components"].append(int(n))
        counts["n_components_kept"].append(int(n > 0))
        counts["n_kept"].append(int(kept.sum()))
    return keep.reshape(rel.shape), {k: np.array(v, dtype=np.int64) for k, v in counts.items()}


def notebook_largest(mask):
    """The notebook's own procedure on one cropped 3D mask, with scipy.ndimage.label at full
    connectivity in place of skimage.measure.label (the same raster-order labels): sort the
    regions by area, descending and stable, and zero all but the first."""
    lab, n = ndimage.label(mask, ndimage.generate_binary_structure(mask.ndim, mask.ndim))
    regions = [(int((lab == i).sum()), i) for i in range(1, n + 1)]
    regions.sort(key=lambda x: x[0], reverse=True)
    for _, i in regions[1:]:
        lab[lab == i] = 0
    lab[lab != 0] = 1
    return lab.astype(bool)


def dot_terms(x, y, z, m, xyscale, zscale, center, clamp=True):
    """The notebook's per-voxel quantities of one cropped box: physical velocities x, y, z (z None
    in 2D; NaN where masked out), the integer mask m, center = (cx, cy, cz) in the box's index
    coordinates.  Returns speed, dot, angle (degrees), inward."""
    kz, ky, kx = np.indices(m.shape).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        dxc = kx * xyscale - center[0] * xyscale
        dyc = ky * xyscale - center[1] * xyscale
        if z is not None:
            dzc = kz * zscale - center[2] * zscale
            nd = np.sqrt((dxc * dxc + dyc * dyc) + dzc * dzc)
            speed = np.sqrt(np.power(x, 2) + np.power(y, 2) + np.power(z, 2))
            dot = ((x / speed) * (-dxc / nd) + (y / speed) * (-dyc / nd)) + (z / speed) * (-dzc / nd)
        else:
            nd = np.sqrt(dxc * dxc + dyc * dyc)
            speed = np.sqrt(np.power(x, 2) + np.power(y, 2))
            dot = (x / speed) * (-dxc / nd) + (y / speed) * (-dyc / nd)
        angle = np.degrees(np.arccos(np.clip(dot, -1.0, 1.0) if clamp else dot))
        return speed, dot, angle, speed * dot


def contract_ref(vx, vy, vz, keep, boxes, xyscale=1.0, zscale=1.0, tscale=1.0, center=None, bins=None, clamp=True):
    """of3d_flow_contract's result per box, with the mask of box r taken from bit r of `keep`
    (uint16, the fields' shape).  center: None (the mask's centroid) or (x, y, z) box-local."""
    shape = np.shape(vx)
    vol = lambda f: np.array(f, dtype=np.float64).reshape((1,) + shape if len(shape) == 2 else shape)
    fx, fy, fz = vol(vx), vol(vy), (vol(vz) if vz is not None else None)
    keep = np.asarray(keep).reshape(fx.shape)
    bins = {k: np.asarray(e, np.float64) for k, e in (bins or {}).items()}
    out = {"rois": np.asarray(boxes, dtype=np.int64), "moments": [], "centroid": [], "center_used": [],
           "n_valid": [], "n_angle": [], "n_inward": [], "hist": {k: [] for k in bins}, "edges": bins,
           "values": [], "dot": [], "angle_slack": []}
    for k in SUMS:
        out[k], out["abs_" + k] = [], []

    def masked(v, m, scale):  # example_analysis_script.ipynb cell 5, as the figure's cell does
        v = v * m
        v[v == 0] = np.nan
        return v * scale / tscale

    for r, (z0, z1, y0, y1, x0, x1) in enumerate(out["rois"]):
        sl = (slice(z0, z1), slice(y0, y1), slice(x0, x1))
        m = ((keep[sl] >> np.uint16(r)) & np.uint16(1)).astype(np.int64)
        kz, ky, kx = np.indices(m.shape)
        out["moments"].append([int(m.sum()), int((m * kx).sum()), int((m * ky).sum()), int((m * kz).sum())])
        with np.errstate(invalid="ignore", divide="ignore"):
            com = ndimage.center_of_mass(m)  # (z, y, x); NaN for an empty mask
        centroid = np.array([com[2], com[1], com[0]], dtype=np.float64)
        used = centroid if center is None else np.asarray(center, dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            x, y = masked(fx[sl], m, xyscale), masked(fy[sl], m, xyscale)
            z = masked(fz[sl], m, zscale) if fz is not None else None
        speed, dot, angle, inward = dot_terms(x, y, z, m, xyscale, zscale, used, clamp)
        valid = ~np.isnan(speed)
        has = valid & ~np.isnan(angle)
        out["centroid"].append(centroid)
        out["center_used"].append(used)
        out["n_valid"].append(int(valid.sum()))
        out["n_angle"].append(int(has.sum()))
        with np.errstate(invalid="ignore"):
            out["n_inward"].append(int((has & (dot > 0)).sum()))
        terms = dict(zip(SUMS, (angle[has], dot[has], inward[has], speed[has])))
        for k, t in terms.items():
            out[k].append(math.fsum(t.tolist()))
            out["abs_" + k].append(math.fsum(np.abs(t).tolist()))
        out["dot"].append(dot[has])
        with np.errstate(divide="ignore"):  # |dot| == 1 (the aligned case): no bound from this formula
            out["angle_slack"].append(math.fsum(((180.0 / np.pi) * K_DOT * U / np.sqrt(1.0 - dot[has] ** 2)).tolist()))
        vals = {"angle": angle[has], "inward": inward[has]}
        out["values"].append(vals)
        for k in bins:
            out["hist"][k].append(np.histogram(vals[k], bins=bins[k])[0].astype(np.uint64))
    for k in ("n_valid", "n_angle", "n_inward"):
        out[k] = np.array(out[k], dtype=np.int64)
    out["moments"] = np.array(out["moments"], dtype=np.uint64)
    out["centroid"], out["center_used"] = np.array(out["centroid"]), np.array(out["center_used"])
    for k in SUMS:
        out[k], out["abs_" + k] = np.array(out[k]), np.array(out["abs_" + k])
    out["angle_slack"] = np.array(out["angle_slack"])
    out["hist"] = {k: np.stack(v) for k, v in out["hist"].items()}
    return out


def sum_bound(ref, key):
    """summary_ref.sum_bound's form over the voxels with an angle: (n_angle + 16) * 2^-53 * sum
    |term| (any summation order stays within n*u of the exact sum; 16 ulp per term cover the
    device's sqrt / divide / acos against the host's).  sum_angle also gets the arccosine's
    amplification of the roundings of its argument, per term (180/pi) * K_DOT * 2^-53 /
    sqrt(1 - dot^2)."""
    b = (ref["n_angle"] + 16) * U * ref["abs_" + key]
    return b + ref["angle_slack"] if key == "sum_angle" else b


def mask_of(rel, percentile, boxes, mode, connectivity=None):
    """(keep, counts or None, threshold) for mode "largest" / "summary" (the plain threshold mask,
    every bit of a voxel above the threshold set)."""
    rel = np.asarray(rel)
    thresh = np.percentile(rel, percentile)
    if mode == "largest":
        keep, counts = largest_ref(rel, thresh, boxes, connectivity or (26 if rel.ndim == 3 else 8))
        return keep, counts, thresh
    with np.errstate(invalid="ignore"):
        return np.where(rel > thresh, np.uint16(0xFFFF), np.uint16(0)), None, thresh


# ---------------------------------------------------------------------------------------------
# The inputs of the GPU tests
# ---------------------------------------------------------------------------------------------
BINS = {"angle": np.linspace(0.0, 180.0, 37), "inward": np.linspace(-6.0, 6.0, 49)}
SCALES = dict(xyscale=0.3, zscale=1.2, tscale=0.5)


def general3d(seed=5):
    """12 x 40 x 70 = 33 600 voxels (several workgroups per box at 8 192 voxels each; a width that
    is no multiple of 64): random velocities under a smooth reliability, two overlapping ROIs."""
    shape = (12, 40, 70)
    rng = np.random.default_rng(seed)
    f = [rng.standard_normal(shape) for _ in range(3)]
    rel = ndimage.gaussian_filter(rng.standard_normal(shape), 1.5).astype(np.float32)
    return f + [rel], [(1, 11, 3, 38, 5, 66), (0, 8, 10, 40, 30, 70)], 70


def general2d(seed=9):
    """1 x 37 x 53: a 2D frame with a float64 reliability.  In the plane about one direction in a
    thousand lies within 1 - 1e-6 of the centre's: the seed is one without such a voxel
    (test_contract_cpu.py checks it)."""
    shape = (37, 53)
    rng = np.random.default_rng(seed)
    f = [rng.standard_normal(shape) for _ in range(2)] + [None]
    rel = ndimage.gaussian_filter(rng.standard_normal(shape), 1.5)
    return f + [rel], [(2, 35, 4, 50)], 60


def cube():
    """A 3 x 3 x 3 solid cube inside 5 x 7 x 9: its centroid voxel (2, 3, 4) is valid."""
    rel = np.zeros((5, 7, 9), np.float32)
    rel[1:4, 2:5, 3:6] = 1.0
    rng = np.random.default_rng(8)
    return [rng.standard_normal(rel.shape) for _ in range(3)] + [rel]


def aligned():
    """(fields, centre, n_towards, n_away): a flow that points exactly at, and away from, the
    voxel (x, y, z) = (6, 5, 4) of a 9 x 11 x 13 volume, along the three lines through it.  The
    masking turns an exact zero component into NaN, so the two off-axis components are 2^-600:
    their squares underflow to zero, the speed is exactly the axis component's magnitude and the
    off-axis terms of the dot product are exactly -0.  Towards the centre on the lower side of
    every line, away from it on the upper side."""
    shape, c = (9, 11, 13), (6, 5, 4)
    tiny = 2.0 ** -600
    vx, vy, vz = (np.full(shape, tiny) for _ in range(3))
    rel = np.zeros(shape, np.float32)
    kz, ky, kx = np.indices(shape)
    lines = ((vx, kx, c[0], (ky == c[1]) & (kz == c[2])), (vy, ky, c[1], (kx == c[0]) & (kz == c[2])),
             (vz, kz, c[2], (kx == c[0]) & (ky == c[1])))
    for v, k, ck, on in lines:
        rel[on] = 1.0
        v[on & (k < ck)] = 2.0   # below the centre, pointing up: towards it
        v[on & (k > ck)] = 0.75  # above the centre, pointing up: away from it
    n_towards, n_away = c[0] + c[1] + c[2], (12 - c[0]) + (10 - c[1]) + (8 - c[2])
    return [vx, vy, vz, rel], c, n_towards, n_away


def label_masks():
    """name -> (rel, boxes, threshold): the masks of the largest-component tests."""
    rng = np.random.default_rng(40)
    out = {}
    out["random"] = ((rng.random((12, 40, 70)) > 0.62).astype(np.float32), [(1, 11, 3, 38, 5, 66)])
    out["smooth"] = (ndimage.gaussian_filter(rng.standard_normal((12, 40, 70)), 1.5).astype(np.float32) > 0.05,
                     [(0, 8, 10, 40, 30, 70), (1, 11, 3, 38, 5, 66)])  # overlapping: each its own bit of keep
    out["checkerboard"] = (mr.checkerboard(), [(0, 4, 1, 5, 0, 5)])
    two = np.zeros((5, 7, 9), np.float32)  # two components of 6 voxels: the lower root wins
    two[3, 4:6, 5:8] = 1
    two[1, 1:3, 1:4] = 1
    out["tie"] = (two, [(0, 5, 0, 7, 4, 9)])  # the box holds the later one alone
    out["empty"] = (np.zeros((3, 5, 7), np.float32), [(0, 2, 1, 4, 2, 6)])
    u, boxes = mr.u_shape()  # box 1 ends above the base: the two arms are separate there, equal in size
    out["truncated"] = (u, [tuple(int(v) for v in boxes[1])])
    return {k: (np.asarray(rel, np.float32), boxes_of(np.shape(rel), rois), 0.5) for k, (rel, rois) in out.items()}


def label_masks_2d():
    rng = np.random.default_rng(41)
    rel = (rng.random((37, 53)) > 0.55).astype(np.float64)
    return {"random2d": (rel, boxes_of(rel.shape, [(2, 35, 4, 50)]), 0.5)}
