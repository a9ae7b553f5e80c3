"""numpy restatement of analysis.flow_summary (tests only): the masking exactly as
oracle.cpu_ref.analysis_reference (example_analysis_script.ipynb cells 4-6) on float64 copies
of the fields, the figures' badRows = isnan(magnitude) as validity, sums with math.fsum (the
correctly rounded sum), histograms with np.histogram(values, bins=edges).  Besides each sum its
sum of absolute terms, for the tests' error bound."""
import math

import numpy as np

from oracle import cpu_ref

SUMS = ("sum_magnitude", "sum_vx", "sum_vy", "sum_vz", "sum_sin", "sum_cos", "sum_mag_sin", "sum_mag_cos")


def masked_fields(vx, vy, vz, rel, rel_percentile=90, xyscale=1.0, zscale=1.0, tscale=1.0):
    """analysis_reference's dict on float64 copies of the velocities (the device kernels widen
    float32 fields to float64 before the masking, as of3d_flow_stats does)."""
    f64 = lambda a: None if a is None else np.array(a, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return cpu_ref.analysis_reference(f64(vx), f64(vy), f64(vz), np.asarray(rel), rel_percentile, xyscale, zscale,
                                          tscale)


def boxes_of(shape, rois):
    """ROI 0 = the whole volume, then `rois`; 2D boxes get z = (0, 1).  (n_roi, 6) int64."""
    dims = tuple(shape) if len(shape) == 3 else (1,) + tuple(shape)
    out = [(0, dims[0], 0, dims[1], 0, dims[2])]
    for r in rois or ():
        out.append(tuple(r) if len(shape) == 3 else (0, 1) + tuple(r))
    return np.array(out, dtype=np.int64)


def summary_ref(vx, vy, vz, rel, rel_percentile=90, xyscale=1.0, zscale=1.0, tscale=1.0, rois=None, bins=None):
    a = masked_fields(vx, vy, vz, rel, rel_percentile, xyscale, zscale, tscale)
    shape = np.shape(vx)
    vol = lambda f: f.reshape((1,) + shape) if len(shape) == 2 else f
    x, y, mag, theta = vol(a["vx"]), vol(a["vy"]), vol(a["magnitude"]), vol(a["theta"])
    z = vol(a["vz"]) if vz is not None else np.zeros_like(x)
    phi = vol(a["phi"]) if vz is not None else None
    boxes = boxes_of(shape, rois)
    out = {"threshold": a["threshold"], "rois": boxes, "n_valid": [], "n_voxels": [],
           "hist": {k: [] for k in (bins or {})}, "edges": {k: np.asarray(e, np.float64) for k, e in (bins or {}).items()},
           "values": []}
    for k in SUMS:
        out[k], out["abs_" + k] = [], []
    for z0, z1, y0, y1, x0, x1 in boxes:
        sl = (slice(z0, z1), slice(y0, y1), slice(x0, x1))
        ok = ~np.isnan(mag[sl])
        bx, by, bz, bm = x[sl][ok], y[sl][ok], z[sl][ok], mag[sl][ok]
        h = np.sqrt(bx * bx + by * by)
        sn, cs = by / h, bx / h
        terms = dict(zip(SUMS, (bm, bx, by, bz, sn, cs, bm * sn, bm * cs)))
        out["n_valid"].append(int(ok.sum()))
        out["n_voxels"].append(int(ok.size))
        for k, t in terms.items():
            out[k].append(math.fsum(t.tolist()))
            out["abs_" + k].append(math.fsum(np.abs(t).tolist()))
        vals = {"vx": bx, "vy": by, "vz": bz, "magnitude": bm, "theta": theta[sl][ok]}
        if phi is not None:
            vals["phi"] = phi[sl][ok]
        out["values"].append(vals)
        for k in out["hist"]:
            out["hist"][k].append(np.histogram(vals[k], bins=out["edges"][k])[0].astype(np.uint64))
    for k in ("n_valid", "n_voxels"):
        out[k] = np.array(out[k], dtype=np.int64)
    for k in SUMS:
        out[k], out["abs_" + k] = np.array(out[k]), np.array(out["abs_" + k])
    out["hist"] = {k: np.stack(v) for k, v in out["hist"].items()}
    nv = out["n_valid"].astype(np.float64)
    nv[nv == 0] = np.nan
    out["mean_magnitude"] = out["sum_magnitude"] / nv
    out["theta_mean"] = np.arctan2(out["sum_sin"] / nv, out["sum_cos"] / nv)
    out["theta_mean_weighted"] = np.arctan2(out["sum_mag_sin"] / nv, out["sum_mag_cos"] / nv)
    return out


def sum_bound(ref, key):
    """(n_valid + 16) * 2^-53 * sum |term| per ROI: any summation order stays within n*u of the
    exact sum, and 16 ulp per term cover the device's sqrt / divide / atan2 against the host's."""
    return (ref["n_valid"] + 16) * 2.0 ** -53 * ref["abs_" + key]


def assert_matches(got, ref, exact_hists):
    """flow_summary's dict against summary_ref's: counts, the threshold and the listed
    histograms exactly, every sum within sum_bound."""
    assert got["threshold"].dtype == np.asarray(ref["threshold"]).dtype
    assert got["threshold"] == ref["threshold"] or (np.isnan(got["threshold"]) and np.isnan(ref["threshold"]))
    assert np.array_equal(got["rois"], ref["rois"])
    assert np.array_equal(got["n_valid"], ref["n_valid"]), (got["n_valid"], ref["n_valid"])
    assert np.array_equal(got["n_voxels"], ref["n_voxels"])
    for k in SUMS:
        err, bound = np.abs(got[k] - ref[k]), sum_bound(ref, k)
        print(k, "max err / bound:", float(np.max(err / np.maximum(bound, 1e-300))))
        assert np.all(err <= bound), (k, err, bound)
    for k in exact_hists:
        assert got["hist"][k].dtype == np.uint64 and got["hist"][k].shape == ref["hist"][k].shape
        assert np.array_equal(got["hist"][k], ref["hist"][k]), k
        assert np.array_equal(got["edges"][k], ref["edges"][k])


def assert_clear_of_edges(ref, names, margin=1e-9):
    """No reference value of the named quantities lies within `margin` of a bin edge (so the
    device's atan2 / atan, a few ulp off the host's, cannot move a value across an edge)."""
    for k in names:
        e = ref["edges"][k]
        for vals in ref["values"]:
            if vals[k].size:
                assert np.min(np.abs(vals[k][:, None] - e[None, :])) > margin, k
