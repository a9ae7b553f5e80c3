"""numpy restatement of analysis.quiver_sample (tests only): the masking exactly as
summary_ref.masked_fields (example_analysis_script.ipynb cells 4-6 on float64 copies of the
fields), then what the figure scripts do before quiver / quiver3 (plot_figure4_Movies.m:121-143):
strided slices of every ROI anchored at its origin, ~isnan(magnitude), the survivors in C order
(np.argwhere).  With a given threshold or a keep volume (mask_ref.open_ref) the mask of cell 4
is replaced and cell 5 restated here.  lattice_mask_records is the same result by another
road, for the CPU test: a boolean lattice over the whole volume, indexed in C order."""
import numpy as np

import summary_ref as sr


def gap3_of(gap, ndim):
    """gap as (gz, gy, gx): an int for every axis, or ndim values; gz = 1 in 2D."""
    g = (int(gap),) * ndim if np.ndim(gap) == 0 else tuple(int(v) for v in gap)
    assert len(g) == ndim
    return g if ndim == 3 else (1,) + g


def _masked(v, m, scale, tscale):
    """Cell 5 for one component with a given boolean mask."""
    v = np.array(v, dtype=np.float64) * m
    v[v == 0] = np.nan
    return v * scale / tscale


def physical_fields(vx, vy, vz, mask, xyscale=1.0, zscale=1.0, tscale=1.0):
    """(vx, vy, vz or None, magnitude) in physical units under a boolean mask (cells 5-6)."""
    with np.errstate(invalid="ignore"):
        x, y = _masked(vx, mask, xyscale, tscale), _masked(vy, mask, xyscale, tscale)
        if vz is None:
            return x, y, None, np.sqrt(np.power(x, 2) + np.power(y, 2))
        z = _masked(vz, mask, zscale, tscale)
        return x, y, z, np.sqrt(np.power(x, 2) + np.power(y, 2) + np.power(z, 2))


def _vol(f, shape):
    return None if f is None else f.reshape((1,) + tuple(shape) if len(shape) == 2 else shape)


def lattice_records(x, y, z, mag, box, gap3):
    """One box's records from (nz, ny, nx) physical fields (z None in 2D): strided slices,
    ~isnan(magnitude), argwhere in C order."""
    z0, z1, y0, y1, x0, x1 = (int(v) for v in box)
    sl = (slice(z0, z1, gap3[0]), slice(y0, y1, gap3[1]), slice(x0, x1, gap3[2]))
    ok = ~np.isnan(mag[sl])
    zyx = np.argwhere(ok).astype(np.int64) * np.array(gap3, dtype=np.int64) + np.array([z0, y0, x0], dtype=np.int64)
    vz = z[sl][ok] if z is not None else np.zeros(int(ok.sum()))
    v = np.stack([x[sl][ok], y[sl][ok], vz], axis=1)
    return {"zyx": zyx.reshape(-1, 3), "v": v.reshape(-1, 3), "n_lattice": int(ok.size), "n_valid": int(ok.sum())}


def lattice_mask_records(x, y, z, mag, box, gap3):
    """lattice_records by a boolean lattice mask over the whole volume, indexed in C order."""
    z0, z1, y0, y1, x0, x1 = (int(v) for v in box)
    lattice = np.zeros(mag.shape, dtype=bool)
    lattice[z0:z1:gap3[0], y0:y1:gap3[1], x0:x1:gap3[2]] = True
    idx = np.flatnonzero(lattice & ~np.isnan(mag))  # flat order is C order
    zyx = np.stack(np.unravel_index(idx, mag.shape), axis=1).astype(np.int64)
    cols = [f.reshape(-1)[idx] for f in (x, y)] + [z.reshape(-1)[idx] if z is not None else np.zeros(idx.size)]
    return {"zyx": zyx.reshape(-1, 3), "v": np.stack(cols, axis=1).reshape(-1, 3), "n_lattice": int(lattice.sum()),
            "n_valid": int(idx.size)}


def quiver_ref(vx, vy, vz, rel, rel_percentile=90, xyscale=1.0, zscale=1.0, tscale=1.0, gap=2, rois=None,
               threshold=None, keep=None, records=lattice_records):
    """analysis.quiver_sample's dict without a capacity (every valid record).  threshold: used
    instead of the percentile, as one element of rel's dtype; keep (uint16, rel's shape): the mask
    of box r is bit r of it (mask_ref.open_ref), the threshold then only reported."""
    shape = np.shape(vx)
    gap3, boxes = gap3_of(gap, len(shape)), sr.boxes_of(shape, rois)
    rel = np.asarray(rel)
    if threshold is None and keep is None:
        a = sr.masked_fields(vx, vy, vz, rel, rel_percentile, xyscale, zscale, tscale)
        thresh = a["threshold"]
        per_box = [(a["vx"], a["vy"], a.get("vz"), a["magnitude"])] * len(boxes)
    else:
        thresh = rel.dtype.type(threshold) if threshold is not None else np.percentile(rel, rel_percentile)
        if keep is None:
            with np.errstate(invalid="ignore"):
                per_box = [physical_fields(vx, vy, vz, rel > thresh, xyscale, zscale, tscale)] * len(boxes)
        else:
            bit = lambda r: ((np.asarray(keep) >> np.uint16(r)) & np.uint16(1)).astype(bool)
            per_box = [physical_fields(vx, vy, vz, bit(r), xyscale, zscale, tscale) for r in range(len(boxes))]
    samples = [records(*(_vol(f, shape) for f in per_box[r]), boxes[r], gap3) for r in range(len(boxes))]
    return {"threshold": thresh, "rois": boxes, "gap": gap3, "samples": samples}


def truncated(sample, capacity):
    """A ROI's sample as a block of `capacity` records holds it: the first ones, n_valid in full."""
    n = min(sample["n_valid"], capacity)
    return dict(sample, zyx=sample["zyx"][:n], v=sample["v"][:n])


def planted_fields(shape, seed, v_dtype=np.float64, rel_dtype=np.float32):
    """Random fields with what the masking must cope with planted: exact zeros in single
    components (the voxel's magnitude is then NaN), NaNs in the velocities, and rel values tied
    across many voxels.  (vx, vy, vz or None, rel); 2D shapes give vz None."""
    rng = np.random.default_rng(seed)
    f = [rng.standard_normal(shape).astype(v_dtype) for _ in range(len(shape))]
    for k, a in enumerate(f):
        flat = a.reshape(-1)
        flat[rng.choice(flat.size, flat.size // 11, replace=False)] = 0.0
        flat[rng.choice(flat.size, flat.size // 17, replace=False)] = np.nan
        flat[(3 + k) % flat.size] = -0.0
    rel = np.round(rng.random(shape) * 64).astype(rel_dtype) / rel_dtype(64)  # ties at the threshold
    return f + ([None] if len(shape) == 2 else []) + [rel]
