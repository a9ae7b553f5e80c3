"""numpy restatements of what of3d_rel_select and of3d_rel_profile compute (csrc/kt_relsel.hip):
the percentile of a crop, one np.percentile call per percentile with a Python float (numpy returns
float64 for a float32 array when q is an np.float64 scalar or a list), and the profile of a crop:
counts above each threshold in rel's dtype and np.histogram of the float64 values."""

import warnings

import numpy as np


def dataset(kind, n, dtype):
    """The data kinds of test_gpu_summary.py's select tests, restated."""
    rng = np.random.default_rng(1000 + n)
    dt = np.dtype(dtype)
    if kind == "normal":
        return rng.standard_normal(n).astype(dt)
    if kind == "equal":
        return np.full(n, 1.25, dtype=dt)
    if kind == "five_levels":  # heavy ties, zero and both signs among the levels
        return (rng.integers(0, 5, n) * 0.5 - 1.0).astype(dt)
    if kind == "low_bits":  # equal but for the lowest 10 (float32) / 11 (float64) bits: the last pass decides
        it, nb = (np.uint32, 10) if dt == np.float32 else (np.uint64, 11)
        base = np.array(1.5, dtype=dt).view(it)
        return (base + rng.integers(0, 1 << nb, n).astype(it)).view(dt)
    if kind == "signs_zero_inf":
        a = rng.standard_normal(n).astype(dt)
        special = np.array([-0.0, np.inf, 0.0, -np.inf], dtype=dt)
        pos = rng.permutation(n)[:4]
        a[pos] = special[:len(pos)]
        return a
    raise AssertionError(kind)


KINDS = ("normal", "equal", "five_levels", "low_bits", "signs_zero_inf")


def crop(a, box):
    """The box (6 bounds, or 4 for a 2D array; None: everything) of an array."""
    if box is None:
        return a
    if a.ndim == 2:
        return a[box[0]:box[1], box[2]:box[3]]
    return a[box[0]:box[1], box[2]:box[3], box[4]:box[5]]


def percentiles(a, box, ps, method):
    """np.percentile(crop, p, method=method) per percentile, as an array of a's dtype."""
    c = crop(a, box)
    out = []
    with np.errstate(invalid="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for p in ps:
            v = np.percentile(c, float(p), method=method)
            assert v.dtype == a.dtype, (v.dtype, a.dtype)
            out.append(v)
    return np.array(out, dtype=a.dtype)


def same_values(got, want):
    """Bitwise equality of two arrays of one dtype, but that any NaN equals any NaN and -0.0
    equals +0.0: the select has one key for the two zeros, and the order numpy's sort leaves
    them in is not specified."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    it = np.uint32 if got.dtype == np.float32 else np.uint64
    bits = got.view(it) == want.view(it)
    return bool(np.all(bits | (np.isnan(got) & np.isnan(want)) | ((got == 0) & (want == 0))))


def auto_edges(lo, hi, nbins):
    """The edges of the profile's auto histogram: np.histogram's outer edges (lo == hi widened by
    0.5 to both sides) and np.linspace between them in float64; NaN edges for a non-finite end."""
    lo, hi = float(lo), float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi)):
        return np.full(nbins + 1, np.nan)
    if lo == hi:
        lo, hi = lo - 0.5, hi + 0.5
    return np.linspace(lo, hi, nbins + 1)


def profile(rel, rois, thresholds, edges):
    """Per ROI (ROI 0: the whole volume) n_voxels, n_nan, n_above (rel > t in rel's dtype) and
    np.histogram(crop.astype(float64), bins=edges)[0]; NaN edges: all-zero counts."""
    boxes = [None] + list(rois)
    thresholds = np.asarray(thresholds, dtype=rel.dtype)
    out = {"n_voxels": [], "n_nan": [], "n_above": [], "hist": []}
    for b in boxes:
        c = crop(rel, b).ravel()
        out["n_voxels"].append(c.size)
        out["n_nan"].append(int(np.isnan(c).sum()))
        with np.errstate(invalid="ignore"):
            out["n_above"].append([int((c > t).sum()) for t in thresholds])
        if np.any(np.isnan(edges)):
            out["hist"].append(np.zeros(len(edges) - 1, dtype=np.uint64))
        else:
            v = c.astype(np.float64)
            out["hist"].append(np.histogram(v[~np.isnan(v)], bins=edges)[0].astype(np.uint64))
    return {k: np.array(v) for k, v in out.items()}
