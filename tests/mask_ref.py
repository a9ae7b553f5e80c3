"""CPU restatement of the mask opening and of the summaries over an opened mask (tests only).

open_ref: MATLAB's bwareaopen(rel > thresh, min_size, connectivity) on every cropped ROI
(plot_figure4_timeTraces.m:72-79) with scipy.ndimage.label and np.bincount.
summary_ref_masked: example_analysis_script.ipynb cells 5-6 with a given boolean mask per box
(v * mask, zeros -> NaN, scale, magnitude, theta, phi), reduced as summary_ref.summary_ref
reduces the threshold mask: math.fsum sums, np.histogram counts."""
import math

import numpy as np
from scipy import ndimage

from summary_ref import SUMS, boxes_of  # noqa: F401  (boxes_of: re-exported for the tests)

COUNTS = ("n_mask", "n_components", "n_components_kept", "n_kept")
_RANK = {4: 1, 8: 2, 6: 1, 18: 2, 26: 3}  # generate_binary_structure's connectivity rank


def open_ref(rel, thresh, boxes, min_size, connectivity):
    """keep (uint16, rel's shape; bit r: in box r and in a component of >= min_size voxels of
    (rel > thresh) cropped to box r) and a dict of the four int64 count arrays."""
    rel = np.asarray(rel)
    vol = rel.reshape((1,) + rel.shape) if rel.ndim == 2 else rel
    assert connectivity in ((4, 8) if rel.ndim == 2 else (6, 18, 26))
    with np.errstate(invalid="ignore"):
        mask = vol > thresh
    keep = np.zeros(vol.shape, np.uint16)
    counts = {k: [] for k in COUNTS}
    for r, (z0, z1, y0, y1, x0, x1) in enumerate(np.asarray(boxes)):
        sl = (slice(z0, z1), slice(y0, y1), slice(x0, x1))
        m = mask[sl]
        if rel.ndim == 2:
            lab, n = ndimage.label(m[0], ndimage.generate_binary_structure(2, _RANK[connectivity]))
            lab = lab[None]
        else:
            lab, n = ndimage.label(m, ndimage.generate_binary_structure(3, _RANK[connectivity]))
        sizes = np.bincount(lab.ravel(), minlength=n + 1)
        sizes[0] = 0  # label 0 is the background
        big = sizes >= min_size
        big[0] = False
        kept = big[lab]
        keep[sl] |= kept.astype(np.uint16) << np.uint16(r)
        counts["n_mask"].append(int(m.sum()))
        counts["n_components"].append(int(n))
        counts["n_components_kept"].append(int(big.sum()))
        counts["n_kept"].append(int(kept.sum()))
    return keep.reshape(rel.shape), {k: np.array(v, dtype=np.int64) for k, v in counts.items()}


def checkerboard():
    z, y, x = np.indices((4, 5, 6))
    return ((z + y + x) % 2 == 0).astype(np.float32)


def u_shape():
    """(6, 20, 40): two arms of 10 voxels along y and a base of 11 along x at y = 15, in plane 2;
    box 1 ends at y = 15, so it holds the arms only."""
    rel = np.zeros((6, 20, 40), np.float32)
    rel[2, 5:15, 10] = rel[2, 5:15, 20] = 1
    rel[2, 15, 10:21] = 1
    return rel, boxes_of(rel.shape, [(0, 6, 0, 15, 0, 40)])


def summary_ref_masked(vx, vy, vz, keep, threshold, boxes, xyscale=1.0, zscale=1.0, tscale=1.0, bins=None):
    """summary_ref.summary_ref's dict with the mask of box r taken from bit r of `keep`."""
    shape = np.shape(vx)
    vol = lambda f: np.array(f, dtype=np.float64).reshape((1,) + shape if len(shape) == 2 else shape)
    fx, fy, fz = vol(vx), vol(vy), (vol(vz) if vz is not None else None)
    keep = np.asarray(keep).reshape(fx.shape)
    out = {"threshold": threshold, "rois": np.asarray(boxes, dtype=np.int64), "n_valid": [], "n_voxels": [],
           "hist": {k: [] for k in (bins or {})}, "edges": {k: np.asarray(e, np.float64) for k, e in (bins or {}).items()},
           "values": []}
    for k in SUMS:
        out[k], out["abs_" + k] = [], []

    def masked(v, m, scale):  # cell 5
        v = v * m
        v[v == 0] = np.nan
        return v * scale / tscale

    for r, (z0, z1, y0, y1, x0, x1) in enumerate(out["rois"]):
        sl = (slice(z0, z1), slice(y0, y1), slice(x0, x1))
        m = ((keep[sl] >> np.uint16(r)) & np.uint16(1)).astype(bool)
        with np.errstate(invalid="ignore", divide="ignore"):
            x, y = masked(fx[sl], m, xyscale), masked(fy[sl], m, xyscale)
            if fz is not None:
                z = masked(fz[sl], m, zscale)
                mag = np.sqrt(np.power(x, 2) + np.power(y, 2) + np.power(z, 2))  # cell 6
                phi = np.arctan(z / np.sqrt(np.power(x, 2) + np.power(y, 2)))
            else:
                z, phi = np.zeros_like(x), None
                mag = np.sqrt(np.power(x, 2) + np.power(y, 2))
            theta = np.arctan2(y, x)
        ok = ~np.isnan(mag)
        bx, by, bz, bm = x[ok], y[ok], z[ok], mag[ok]
        h = np.sqrt(bx * bx + by * by)
        sn, cs = by / h, bx / h
        terms = dict(zip(SUMS, (bm, bx, by, bz, sn, cs, bm * sn, bm * cs)))
        out["n_valid"].append(int(ok.sum()))
        out["n_voxels"].append(int(ok.size))
        for k, t in terms.items():
            out[k].append(math.fsum(t.tolist()))
            out["abs_" + k].append(math.fsum(np.abs(t).tolist()))
        vals = {"vx": bx, "vy": by, "vz": bz, "magnitude": bm, "theta": theta[ok]}
        if phi is not None:
            vals["phi"] = phi[ok]
        out["values"].append(vals)
        for k in out["hist"]:
            out["hist"][k].append(np.histogram(vals[k], bins=out["edges"][k])[0].astype(np.uint64))
    for k in ("n_valid", "n_voxels"):
        out[k] = np.array(out[k], dtype=np.int64)
    for k in SUMS:
        out[k], out["abs_" + k] = np.array(out[k]), np.array(out["abs_" + k])
    out["hist"] = {k: np.stack(v) for k, v in out["hist"].items()}
    return out
