"""Host reference of the mask's principal axes and the projected flow (tests only).

Moments: numpy integer sums over box-local coordinates.  Centroid and covariance: exact, with
fractions.Fraction, from those integers.  Axes: np.linalg.eigh of the float64 covariance,
descending, with the device's sign rule (largest-magnitude component positive, a tie to the
first of x, y, z).  Projection: example_analysis_script.ipynb cell 5's masking (as
mask_ref.summary_ref_masked), then p_k = (vx*e_k.x + vy*e_k.y) + vz*e_k.z in numpy (no FMA:
the device's expression tree), math.fsum sums and np.histogram counts."""
import math
from fractions import Fraction

import numpy as np

MOMENTS = ("n", "x", "y", "z", "xx", "yy", "zz", "xy", "xz", "yz")
AXIS_NAMES = ("axis1", "axis2", "axis3")


def blob(shape, seed, noise=0.02):
    """A tilted anisotropic Gaussian blob (long axis near x, turned 0.12 rad towards y and
    0.03 towards z; the second axis near y) plus `noise` of seeded white noise, float64."""
    dims = shape if len(shape) == 3 else (1,) + tuple(shape)
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in dims), indexing="ij")
    cz, cy, cx = ((n - 1) / 2 for n in dims)
    u, v, w = x - cx - 2.0, y - cy + 1.0, z - cz
    a, b = 0.12, 0.03
    p = math.cos(a) * u + math.sin(a) * v + b * w      # along the long axis
    q = -math.sin(a) * u + math.cos(a) * v             # across, in the plane
    r = w - b * u
    f = np.exp(-0.5 * ((p / (0.30 * dims[2])) ** 2 + (q / (0.35 * dims[1])) ** 2 + (r / max(0.5 * dims[0], 1.0)) ** 2))
    f += noise * np.random.default_rng(seed).standard_normal(dims)
    return f.reshape(shape)


def box_mask(mask, box):
    z0, z1, y0, y1, x0, x1 = (int(v) for v in box)
    m = np.asarray(mask)
    m = m.reshape((1,) + m.shape) if m.ndim == 2 else m
    return m[z0:z1, y0:y1, x0:x1]


def int_moments(m):
    """The ten integer sums of a cropped boolean mask (nz, ny, nx), as Python ints."""
    z, y, x = (c.astype(np.int64) for c in np.nonzero(m))
    s = lambda a: int(a.sum(dtype=np.int64))
    return [int(x.size), s(x), s(y), s(z), s(x * x), s(y * y), s(z * z), s(x * y), s(x * z), s(y * z)]


def exact_stats(mom, box):
    """(centroid [3 Fractions, volume coordinates x y z], covariance [3][3] Fractions)."""
    n, sx, sy, sz, sxx, syy, szz, sxy, sxz, syz = (int(v) for v in mom)
    z0, _, y0, _, x0, _ = (int(v) for v in box)
    s1 = (sx, sy, sz)
    s2 = ((sxx, sxy, sxz), (sxy, syy, syz), (sxz, syz, szz))
    cen = [Fraction(o) + Fraction(s, n) for o, s in zip((x0, y0, z0), s1)]
    cov = [[Fraction(n * s2[i][j] - s1[i] * s1[j], n * n) for j in range(3)] for i in range(3)]
    return cen, cov


def sign_rule(e):
    """The device's sign convention for one vector (x, y, z)."""
    e = np.asarray(e, dtype=np.float64)
    big = 0
    for i in (1, 2):
        if abs(e[i]) > abs(e[big]):
            big = i
    return -e if e[big] < 0 else e


def eigh_axes(cov):
    """(values descending, vectors as rows e_k = x y z with sign_rule) of a float64 3x3."""
    w, v = np.linalg.eigh(np.asarray(cov, dtype=np.float64))
    order = np.argsort(-w, kind="stable")
    return w[order], np.stack([sign_rule(v[:, k]) for k in order])


def ulp_distance(got, frac):
    """|got - frac| in units of the last place of the float64 nearest frac."""
    want = float(frac)
    return float(abs(Fraction(float(got)) - frac) / Fraction(np.spacing(abs(want)) if want else 5e-324))


def projection_ref(vx, vy, vz, masks, boxes, axes_used, xyscale=1.0, zscale=1.0, tscale=1.0, bins=None):
    """Per box: n_valid, sum_axis*, abs_sum_axis*, hist[axis] from the boolean mask of each box
    (masks[r]: cropped to box r) and the axes the device used (axes_used[r]: rows e_k)."""
    shape = np.shape(vx)
    vol = lambda f: np.array(f, dtype=np.float64).reshape((1,) + shape if len(shape) == 2 else shape)
    fx, fy, fz = vol(vx), vol(vy), (vol(vz) if vz is not None else None)
    bins = {k: np.asarray(e, np.float64) for k, e in (bins or {}).items()}
    out = {"n_valid": [], "hist": {k: [] for k in bins}, "edges": bins}
    for a in AXIS_NAMES:
        out["sum_" + a], out["abs_sum_" + a] = [], []

    def masked(v, m, scale):
        v = v * m
        v[v == 0] = np.nan
        return v * scale / tscale

    for r, box in enumerate(np.asarray(boxes)):
        z0, z1, y0, y1, x0, x1 = (int(v) for v in box)
        sl = (slice(z0, z1), slice(y0, y1), slice(x0, x1))
        m = np.asarray(masks[r], dtype=bool)
        with np.errstate(invalid="ignore"):
            x, y = masked(fx[sl], m, xyscale), masked(fy[sl], m, xyscale)
            if fz is not None:
                z = masked(fz[sl], m, zscale)
                mag2 = (x * x + y * y) + z * z
            else:
                z, mag2 = None, x * x + y * y
        ok = ~np.isnan(mag2)
        out["n_valid"].append(int(ok.sum()))
        for k, a in enumerate(AXIS_NAMES):
            e = axes_used[r][k]
            p = x[ok] * e[0] + y[ok] * e[1]
            if z is not None:
                p = p + z[ok] * e[2]
            out["sum_" + a].append(math.fsum(p.tolist()))
            out["abs_sum_" + a].append(math.fsum(np.abs(p).tolist()))
            if a in bins:
                out["hist"][a].append(np.histogram(p, bins=bins[a])[0].astype(np.uint64))
    out["n_valid"] = np.array(out["n_valid"], dtype=np.int64)
    for a in AXIS_NAMES:
        out["sum_" + a], out["abs_sum_" + a] = np.array(out["sum_" + a]), np.array(out["abs_sum_" + a])
    out["hist"] = {k: np.stack(v) for k, v in out["hist"].items()}
    return out
