"""numpy restatement of analysis.projection_maps (tests only), written as the loop the header
states: per ROI and axis one vectorised step per index along the axis — ``s = np.where(valid,
s + q, s)`` for the flow sums, ``np.fmax`` for the image maximum, ``s + img`` for the image sum —
so every map is reproduced bit for bit.  The masking is example_analysis_script.ipynb cells 4-5
step by step (v * mask, exact zeros -> NaN, (v * scale) / tscale) on float64 copies, validity is
~isnan(magnitude); the masks come from mask_ref (boxes_of, and open_ref's keep volume for an
opened mask: box r keeps bit r)."""
import numpy as np

import mask_ref as mr

AXES = ("z", "y", "x")
FLOW_MAPS = ("n_mask", "n_valid", "sum_vx", "sum_vy", "sum_vz", "sum_magnitude", "max_magnitude")
IMAGE_MAPS = ("max_image", "sum_image")


def _physical(v, m, scale, tscale):
    """Cell 5 for one component: v * m, exact zeros -> NaN, (v * scale) / tscale."""
    v = np.array(v, dtype=np.float64) * m
    v[v == 0] = np.nan
    return (v * scale) / tscale


def line_maps(x, y, z, m, img, axis):
    """The maps of one box along `axis` (0 z, 1 y, 2 x) from its cropped (dz, dy, dx) physical
    velocities (z None in 2D), boolean mask m and image (or None): the loops."""
    with np.errstate(invalid="ignore", over="ignore"):
        sq = x * x + y * y
        if z is not None:
            sq = sq + z * z
        mag = np.sqrt(sq)
        valid = ~np.isnan(mag)
        plane = tuple(e for i, e in enumerate(x.shape) if i != axis)
        out = {"n_mask": np.zeros(plane, np.int64), "n_valid": np.zeros(plane, np.int64)}
        sums = {"sum_vx": x, "sum_vy": y, "sum_magnitude": mag}
        if z is not None:
            sums["sum_vz"] = z
        for name in sums:
            out[name] = np.zeros(plane, np.float64)
        out["max_magnitude"] = np.full(plane, np.nan)
        if img is not None:
            out["max_image"], out["sum_image"] = np.full(plane, np.nan), np.zeros(plane, np.float64)
        for k in range(x.shape[axis]):
            at = lambda a: np.take(a, k, axis=axis)
            ok = at(valid)
            out["n_mask"] = out["n_mask"] + at(m)
            out["n_valid"] = out["n_valid"] + ok
            for name, q in sums.items():
                out[name] = np.where(ok, out[name] + at(q), out[name])
            out["max_magnitude"] = np.where(ok, np.fmax(out["max_magnitude"], at(mag)), out["max_magnitude"])
            if img is not None:
                v = at(img).astype(np.float64)
                out["max_image"] = np.fmax(out["max_image"], v)
                out["sum_image"] = out["sum_image"] + v
    return {k: out[k] for k in FLOW_MAPS + IMAGE_MAPS if k in out}


def add_means(m, length):
    """The host's means, as analysis._projection_means forms them."""
    with np.errstate(invalid="ignore", divide="ignore"):
        nv = m["n_valid"].astype(np.float64)
        nv[nv == 0] = np.nan
        for k in ("vx", "vy", "vz", "magnitude"):
            if "sum_" + k in m:
                m["mean_" + k] = m["sum_" + k] / nv
        if "sum_image" in m:
            m["mean_image"] = m["sum_image"] / float(length)
    return m


def project_ref(vx, vy, vz, rel, image=None, rel_percentile=90, threshold=None, xyscale=1.0, zscale=1.0, tscale=1.0,
                rois=None, keep=None, axes=None):
    """analysis.projection_maps' dict for every ROI (0, the whole volume, included) and `axes`
    (default: all the volume has).  threshold: used instead of the percentile, as one element
    of rel's dtype; keep (uint16, rel's shape): the mask of box r is bit r of it."""
    shape = np.shape(vx)
    ndim = len(shape)
    axes = tuple(axes) if axes is not None else (AXES if ndim == 3 else AXES[1:])
    boxes = mr.boxes_of(shape, rois)
    rel = np.asarray(rel)
    thresh = rel.dtype.type(threshold) if threshold is not None else np.percentile(rel, rel_percentile)
    vol = lambda a: None if a is None else np.asarray(a).reshape((1,) + shape if ndim == 2 else shape)
    with np.errstate(invalid="ignore"):
        plain = vol(rel > thresh)
    out = []
    for r, box in enumerate(boxes):
        z0, z1, y0, y1, x0, x1 = (int(v) for v in box)
        sl = (slice(z0, z1), slice(y0, y1), slice(x0, x1))
        m = plain[sl] if keep is None else ((vol(keep)[sl] >> np.uint16(r)) & np.uint16(1)).astype(bool)
        with np.errstate(invalid="ignore", over="ignore"):
            x, y = (_physical(vol(f)[sl], m, xyscale, tscale) for f in (vx, vy))
            z = _physical(vol(vz)[sl], m, zscale, tscale) if vz is not None else None
        entry = {"roi": r, "box": tuple(int(v) for v in box)}
        for a in axes:
            k = AXES.index(a)
            maps = line_maps(x, y, z, m, None if image is None else vol(image)[sl], k)
            if ndim == 2:
                maps = {name: v.reshape(v.shape[1:]) for name, v in maps.items()}
            entry[a] = add_means(maps, box[2 * k + 1] - box[2 * k])
        out.append(entry)
    return {"threshold": thresh, "rois": boxes, "axes": axes, "maps": out}
