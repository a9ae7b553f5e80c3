"""numpy restatement of flow_summary's magnitude-weighted histograms (tests only): per ROI and
quantity np.histogram(values, bins=edges, weights=magnitude)[0] over summary_ref's valid
values, and per bin the correctly rounded sum (math.fsum), the sum of absolute terms and the
count, for the tests' error bound."""
import math

import numpy as np

import summary_ref as sr


# Pythagorean quadruples / triples (a, b, c[, d]): every magnitude is an integer, and with
# power-of-two or small integer factors every partial sum of magnitudes is exact in float64, so
# any summation order gives the same bits
QUADRUPLES = ((1, 2, 2), (2, 3, 6), (1, 4, 8), (4, 4, 7), (2, 6, 9), (6, 6, 7), (3, 4, 12), (2, 10, 11))
TRIPLES = ((3, 4), (5, 12), (8, 15), (7, 24))


def exact_fields(shape, rng, ndim=3):
    """vx, vy[, vz] of `shape` drawn from the quadruples (triples in 2D): the components
    permuted, random signs, a random factor 2^-2 .. 2^2."""
    n = int(np.prod(shape))
    table = np.array(QUADRUPLES if ndim == 3 else TRIPLES, dtype=np.float64)
    q = rng.permuted(table[rng.integers(0, len(table), n)], axis=1)
    q *= rng.choice([-1.0, 1.0], size=q.shape)
    q *= 2.0 ** rng.integers(-2, 3, size=(n, 1))
    return [np.ascontiguousarray(q[:, i].reshape(shape)) for i in range(ndim)]


EXACT_SHAPE = (6, 21, 67)
EXACT_ROIS = [(1, 5, 3, 20, 5, 66), (2, 3, 4, 9, 7, 30)]
EXACT_BINS = {"phi": np.linspace(-np.pi / 2, np.pi / 2, 15), "theta": np.linspace(-np.pi, np.pi, 13),
              "magnitude": np.array([0, 2.6, 5.7, 10.3, 20.9, 61])}
EXACT_SEED = 3197  # the first seed with n_valid 4221 / 2083 / 53 (test_whist_cpu.py checks the counts)


def exact_case(seed=EXACT_SEED):
    """The exact case's fields (vx, vy, vz float64, rel float32): percentile 50, scales 1."""
    rng = np.random.default_rng(seed)
    return exact_fields(EXACT_SHAPE, rng) + [rng.random(EXACT_SHAPE, dtype=np.float32)]


def whist_ref(vx, vy, vz, rel, rel_percentile=90, xyscale=1.0, zscale=1.0, tscale=1.0, rois=None,
              weighted_bins=None, ref=None):
    """summary_ref's dict (computed here, or `ref` from the same fields and ROIs) with
    hist_weighted / edges_weighted and fsum_weighted, abs_weighted, count_weighted, each
    name -> (n_roi, nbins)."""
    if ref is None:
        ref = sr.summary_ref(vx, vy, vz, rel, rel_percentile, xyscale, zscale, tscale, rois=rois)
    out = dict(ref)
    edges = {k: np.asarray(e, np.float64) for k, e in (weighted_bins or {}).items()}
    out["edges_weighted"] = edges
    for key in ("hist_weighted", "fsum_weighted", "abs_weighted", "count_weighted"):
        out[key] = {k: [] for k in edges}
    for vals in ref["values"]:
        mag = vals["magnitude"]
        for k, e in edges.items():
            v = vals[k]
            out["hist_weighted"][k].append(np.histogram(v, bins=e, weights=mag)[0])
            # np.histogram's bin rule: e[i] <= v < e[i+1], the last bin closed
            idx = np.searchsorted(e, v, side="right") - 1
            idx[v == e[-1]] = e.size - 2
            idx[(v < e[0]) | (v > e[-1])] = -1
            terms = [mag[idx == b].tolist() for b in range(e.size - 1)]
            out["fsum_weighted"][k].append([math.fsum(t) for t in terms])
            out["abs_weighted"][k].append([math.fsum(abs(x) for x in t) for t in terms])
            out["count_weighted"][k].append([len(t) for t in terms])
    for key, dt in (("hist_weighted", np.float64), ("fsum_weighted", np.float64), ("abs_weighted", np.float64),
                    ("count_weighted", np.int64)):
        out[key] = {k: np.array(v, dtype=dt).reshape(len(ref["values"]), -1) for k, v in out[key].items()}
    return out


def bin_bound(ref, name):
    """summary_ref.sum_bound's rule per bin: (n_bin + 16) * 2^-53 * sum_bin |term|."""
    return (ref["count_weighted"][name] + 16) * 2.0 ** -53 * ref["abs_weighted"][name]


def with_bins(ref, names):
    """`ref` with edges[name] = edges_weighted[name] for `names`, for sr.assert_clear_of_edges."""
    out = dict(ref)
    out["edges"] = {k: ref["edges_weighted"][k] for k in names}
    return out
