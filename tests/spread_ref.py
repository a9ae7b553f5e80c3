"""numpy restatement of flow_summary's spread block (tests only), built on the valid values of
summary_ref.summary_ref (or mask_ref.summary_ref_masked): per ROI, about a centre, the correctly
rounded sum (math.fsum) of every term list with its sum of absolute terms for the tests' error
bound, the extremes, and the derived values formed as analysis._SpreadCall.decode forms them."""
import math

import numpy as np

COMPONENTS = ("vx", "vy", "vz", "magnitude")
SUMS = ("ss_vx", "ss_vy", "ss_vz", "ss_magnitude", "ss_vx_vy", "ss_vx_vz", "ss_vy_vz", "sum_sin_phi", "sum_cos_phi")
EXACT = SUMS[:7] + tuple(f"{m}_{k}" for m in ("min", "max") for k in COMPONENTS)  # bitwise on exact fields


def spread_ref(ref, center="mean"):
    """ref: summary_ref's dict (its `values`, n_valid, n_voxels, sum_sin, sum_cos).  center:
    "mean" (every ROI about fsum / n of its own values), 4 numbers vx vy vz magnitude for every
    ROI, or an (n_roi, 4) array.  Returns a dict of arrays per ROI: spread_center, each of SUMS
    with abs_<name>, min_ / max_ of COMPONENTS, std_*, velocity_covariance, theta_resultant,
    theta_std, theta_std_all and (3D) phi_mean, phi_resultant, phi_std, phi_std_all."""
    n_roi = len(ref["values"])
    is3 = "phi" in ref["values"][0]
    out = {"n_valid": np.asarray(ref["n_valid"]), "spread_center": np.empty((n_roi, 4))}
    for k in SUMS:
        out[k], out["abs_" + k] = np.empty(n_roi), np.empty(n_roi)
    for k in COMPONENTS:
        out["min_" + k], out["max_" + k] = np.full(n_roi, np.nan), np.full(n_roi, np.nan)
    for r, vals in enumerate(ref["values"]):
        comps = [np.asarray(vals[k], dtype=np.float64) for k in COMPONENTS]
        n = comps[0].size
        if isinstance(center, str):
            assert center == "mean"
            c = [math.fsum(v.tolist()) / n if n else np.nan for v in comps]
        else:
            c = np.broadcast_to(np.asarray(center, dtype=np.float64), (n_roi, 4))[r]
        out["spread_center"][r] = c
        dx, dy, dz, dm = (v - cq for v, cq in zip(comps, c))
        x, y, z, mag = comps
        zero = np.zeros(n)
        with np.errstate(invalid="ignore", divide="ignore"):
            terms = (dx * dx, dy * dy, dz * dz, dm * dm, dx * dy, dx * dz, dy * dz,
                     z / mag if is3 else zero, np.sqrt(x * x + y * y) / mag if is3 else zero)
        for k, t in zip(SUMS, terms):
            out[k][r] = math.fsum(t.tolist())
            out["abs_" + k][r] = math.fsum(np.abs(t).tolist())
        if n:
            for k, v in zip(COMPONENTS, comps):
                out["min_" + k][r], out["max_" + k][r] = np.min(v), np.max(v)
    nv = out["n_valid"].astype(np.float64)
    nv[nv == 0] = np.nan
    for k in COMPONENTS:
        out["std_" + k] = np.sqrt(out["ss_" + k] / nv)
    c = np.stack([out[k] for k in SUMS[:7]], axis=1) / nv[:, None]
    out["velocity_covariance"] = c[:, [0, 4, 5, 4, 1, 6, 5, 6, 2]].reshape(n_roi, 3, 3)
    n_all = np.asarray(ref["n_voxels"], dtype=np.float64)
    pairs = [("theta", np.asarray(ref["sum_sin"]), np.asarray(ref["sum_cos"]))]
    if is3:
        pairs.append(("phi", out["sum_sin_phi"], out["sum_cos_phi"]))
        out["phi_mean"] = np.arctan2(out["sum_sin_phi"] / nv, out["sum_cos_phi"] / nv)
    with np.errstate(divide="ignore"):
        for name, sn, cs in pairs:
            r = np.hypot(sn, cs) / nv
            out[name + "_resultant"] = r
            out[name + "_std"] = np.sqrt(np.maximum(0.0, -2.0 * np.log(r)))
            out[name + "_std_all"] = np.sqrt(np.maximum(0.0, -2.0 * np.log(r * nv / n_all)))
    return out


def sum_bound(sref, key):
    """summary_ref.sum_bound's rule: (n_valid + 16) * 2^-53 * sum |term| per ROI."""
    return (sref["n_valid"] + 16) * 2.0 ** -53 * sref["abs_" + key]
