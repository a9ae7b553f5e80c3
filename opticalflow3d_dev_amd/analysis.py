"""Downstream statistics on the flow outputs.

The reference post-processes the saved TIFFs in
``src/Python/example_analysis_script.ipynb``: cell 4 thresholds the
reliability at a percentile (``np.percentile(rel, relPer)``, ``rel >
thresh``), cell 5 masks vx/vy/vz, turns exact zeros into NaN and scales to
physical units, cell 6 forms the magnitude and the angles theta (in the xy
plane) and phi (against the z axis).  Here that runs on outputs still
resident in HBM (FlowStream / plans): the percentile from two order
statistics selected on the GPU, the rest in one fused HIP pass
(``of3d_flow_stats``).
"""

from __future__ import annotations

import ctypes
import dataclasses

import numpy as np

from . import _lib


def _dtype_name(a):
    """'float32', ... of a numpy array or a torch tensor."""
    return str(a.dtype).replace("torch.", "")


def _np_dtype(t):
    return np.dtype(_dtype_name(t))


def _dims(shape):
    """(nz, ny, nx) of a volume's shape: a 2D field is one plane."""
    return shape if len(shape) == 3 else (1,) + shape


def _cuda_device(device):
    """The torch device of an entry's `device` argument (None: the library's default)."""
    import torch

    return torch.device("cuda", _lib.device_index() if device is None else device)


def _to_device(a, host, dev):
    """A field as a contiguous tensor: a numpy array (host) uploaded to dev, a tensor where it is;
    None stays None."""
    import torch

    if a is None:
        return None
    return torch.as_tensor(np.ascontiguousarray(a)).to(dev) if host else a.contiguous()


def _linear_ranks(n, percentile, dt):
    """numpy's 'linear' percentile of n values of dtype dt as two 0-based ranks and a weight:
    (lo, hi, gamma) with lo <= hi <= n-1 and gamma of dtype dt, numpy's arithmetic in the array's
    dtype (numpy/lib/_function_base_impl.py: percentile -> _quantile, method 'linear': virtual
    index (n-1)*q, gamma); the value is _lerp(a, b, gamma) (see _lerp) of the order statistics."""
    q = np.asanyarray(np.true_divide(percentile, dt.type(100)))
    vi = (n - 1) * q
    if vi >= n - 1:
        lo = hi = n - 1
    elif vi < 0:
        lo = hi = 0
    else:
        lo = int(np.floor(vi))
        hi = lo + 1
    gamma = np.asanyarray(vi - lo, dtype=dt)
    return lo, hi, gamma


PERCENTILE_METHODS = ("linear", "hazen")
SELECT_MAX = 8  # percentiles of one of3d_rel_select call (OF3D_SELECT_MAX)


def _percentile_ranks(n, percentile, dt, method="linear"):
    """_linear_ranks for either percentile definition: (lo, hi, gamma) of the `percentile`-th
    percentile of n values of dtype dt.  method "linear": numpy's default.  method "hazen":
    numpy's method='hazen', which is MATLAB's prctile — the sorted values sit at the
    100 * (i - 0.5) / n percentiles (i = 1..n), linear in between, clamped to the extremes beyond
    the first and the last.  numpy's arithmetic, term by term in the array's dtype
    (_compute_virtual_index with alpha = beta = 0.5): n*q + (0.5 + q*(1 - 0.5 - 0.5)) - 1; the
    shorter n*q - 0.5 differs from it in the last bit for some (n, percentile).  Clamped as
    _linear_ranks clamps (vi >= n - 1: the last value, vi < 0: the first), with gamma 0 there:
    lo == hi makes _lerp's result independent of it."""
    if method == "linear":
        return _linear_ranks(n, percentile, dt)
    if method != "hazen":
        raise ValueError(f"summary: percentile_method {method!r} is not one of {PERCENTILE_METHODS}")
    q = np.asanyarray(np.true_divide(percentile, dt.type(100)))
    vi = np.asanyarray(n * q + (0.5 + q * (1 - 0.5 - 0.5)) - 1)
    if vi >= n - 1:
        return n - 1, n - 1, np.asanyarray(0, dtype=dt)
    if vi < 0:
        return 0, 0, np.asanyarray(0, dtype=dt)
    lo = int(np.floor(vi))
    return lo, lo + 1, np.asanyarray(vi - lo, dtype=dt)


def _check_percentiles(percentiles, what, most=SELECT_MAX):
    """1 to `most` percentiles in [0, 100] as a list of Python floats; ValueError naming `what`."""
    try:
        ps = [float(p) for p in percentiles]
    except (TypeError, ValueError):
        raise ValueError(f"summary: {what} {percentiles!r} is not a sequence of numbers") from None
    if not 1 <= len(ps) <= most:
        raise ValueError(f"summary: {what} needs 1 to {most} values, got {len(ps)}")
    for p in ps:
        if not 0 <= p <= 100:  # a NaN fails both comparisons
            raise ValueError(f"summary: {what} {p} outside [0, 100]")
    return ps


def _check_method(method):
    if not isinstance(method, str) or method not in PERCENTILE_METHODS:
        raise ValueError(f"summary: percentile_method {method!r} is not one of {PERCENTILE_METHODS}")
    return method


def _lerp(a, b, gamma, dt):
    """numpy's _lerp of two order statistics in the array's dtype."""
    diff = np.subtract(b, a)
    res = np.add(a, diff * gamma) if gamma < 0.5 else np.subtract(b, diff * (1 - gamma))
    return dt.type(res)


def percentile_threshold(rel, percentile):
    """``np.percentile(rel, percentile)`` (method 'linear') of a tensor, any device.

    The two order statistics around the virtual index come from
    torch.kthvalue on the tensor's device; the interpolation repeats
    numpy's (``a + (b-a)*g``, or ``b - (b-a)*(1-g)`` for g >= 0.5, in the
    array's dtype), so the value equals numpy's.  NaN in -> NaN out."""
    import torch

    flat = rel.reshape(-1)
    n = flat.numel()
    if n == 0:
        raise ValueError("percentile of an empty array")
    dt = _np_dtype(flat)
    if bool(torch.isnan(flat).any()):
        return dt.type(np.nan)
    lo, hi, gamma = _linear_ranks(n, percentile, dt)
    a = dt.type(flat.kthvalue(lo + 1).values.item())
    b = dt.type(flat.kthvalue(hi + 1).values.item()) if hi != lo else a
    return _lerp(a, b, gamma, dt)


def flow_statistics(vx, vy, vz, rel, rel_percentile=90, xyscale=1.0, zscale=1.0, tscale=1.0, device=None):
    """Masked physical velocities, magnitude and angles of one output frame.

    vx, vy, vz, rel: numpy arrays or torch tensors (CUDA tensors stay on
    their device); vz None for 2D.  Returns a dict: threshold, vx, vy, [vz,]
    magnitude, theta, [phi] — torch tensors on the GPU (numpy arrays when the
    inputs were numpy).  Matches example_analysis_script.ipynb cells 4-6:
    bitwise for the threshold, the mask, the velocities and the magnitude;
    theta/phi to the last bits of atan2/atan (device libm vs the host's)."""
    import torch

    host = isinstance(vx, np.ndarray)
    dev = _cuda_device(device)
    tx, ty, tz, tr = (_to_device(a, host, dev) for a in (vx, vy, vz, rel))
    if tx.dtype not in (torch.float64, torch.float32) or tr.dtype not in (torch.float32, torch.float64):
        raise TypeError("vx/vy/vz must be float64 or float32, rel float32 or float64")
    shape = tuple(tx.shape)
    n = tx.numel()
    thresh = percentile_threshold(tr, rel_percentile)
    out = {k: torch.empty(shape, dtype=torch.float64, device=tx.device)
           for k in (("vx", "vy", "vz", "magnitude", "theta", "phi") if tz is not None
                     else ("vx", "vy", "magnitude", "theta"))}
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    stream = torch.cuda.current_stream(tx.device).cuda_stream
    _lib.check(_lib.load().of3d_flow_stats(
        ptr(tx), ptr(ty), ptr(tz), ptr(tr), int(tx.dtype == torch.float32), int(tr.dtype == torch.float64), n,
        float(thresh), float(xyscale), float(zscale), float(tscale), ptr(out["vx"]), ptr(out["vy"]),
        ptr(out.get("vz")), ptr(out["magnitude"]), ptr(out["theta"]), ptr(out.get("phi")), stream))
    if host:
        torch.cuda.synchronize(tx.device)
        out = {k: v.cpu().numpy() for k, v in out.items()}
    out["threshold"] = thresh
    return out


# ---------------------------------------------------------------------------
# Device-side frame summaries (csrc/kt_summary.hip): what the reference's figure
# scripts reduce the saved TIFFs to (plot_figure4_timeTraces.m:82-126,
# plot_figure3_ROIfigures.m:114-193, plot_FigureS2_dt.m:199-222, notebook cells 4-6)
# — a reliability percentile, then per ROI the valid count, the mean magnitude, the
# (magnitude-weighted) circular mean of theta and histograms — computed on the
# resident fields.  `bins` gives plain counts; the magnitude-weighted phi distribution
# of figure 4 (plot_figure4_timeTraces.m:128-138, distPhiW) is `weighted_bins`: float64
# sums of the magnitude per bin, by a deterministic pass of its own (csrc/kt_whist.hip:
# of3d_flow_whist; no floating-point atomics).  The scripts' clean-up of the mask first,
# bwareaopen(rel > thresh, minSize) (plot_figure4_timeTraces.m:75-79, plot_figure5.m:87-88),
# is min_size / connectivity (csrc/kt_ccl.hip: of3d_mask_open, then
# of3d_flow_summary_masked).
# ---------------------------------------------------------------------------
QUANTITIES = ("vx", "vy", "vz", "magnitude", "theta", "phi")
SUMS = ("sum_magnitude", "sum_vx", "sum_vy", "sum_vz", "sum_sin", "sum_cos", "sum_mag_sin", "sum_mag_cos")
MAX_ROI, MAX_BINS = 16, 256
_HEAD, _ROI_HEAD = 8, 10  # result words before the boxes / before a box's histograms (include/of3d.h)
CONNECTIVITIES = {2: (4, 8), 3: (6, 18, 26)}  # bwareaopen's, the default last
OPEN_COUNTS = ("n_mask", "n_components", "n_components_kept", "n_kept")  # of3d_mask_open's d_counts
# of3d_mask_axes (csrc/kt_axes.hip): the mask's principal axes (regionprops3's EigenVectors /
# EigenValues, plot_figure5.m:132-149, plot_figure5_Movie.m:128-143) and the flow projected on them
AXIS_NAMES = ("axis1", "axis2", "axis3")
MOMENTS = ("n", "x", "y", "z", "xx", "yy", "zz", "xy", "xz", "yz")  # the integer sums of a box's result
_AX_HEAD = 44  # a box's result words before its histograms (include/of3d.h)
# of3d_flow_pair (csrc/kt_pair.hip): two channels over the joint mask (figure 3)
PAIR_QUANTITIES = ("dot", "cosine", "dtheta", "dmagnitude")
PAIR_SUMS = ("sum_dot", "sum_cosine", "sum_mag0_mag1", "sum_mag0_sq", "sum_mag1_sq", "sum_sin_dtheta",
             "sum_cos_dtheta", "sum_diff")
_PAIR_HEAD = 26  # a box's result words before its histograms (include/of3d.h)
COMBINE = {"or": 0, "and": 1}  # of3d_mask_open_pair's combine
# of3d_flow_contract (csrc/kt_contract.hip): the flow against the direction to the mask's centroid
# (figure 2 / movie S2, plot_figure2_movie.ipynb cell 1)
CONTRACT_QUANTITIES = ("angle", "inward")
CONTRACT_SUMS = ("sum_angle", "sum_dot", "sum_inward", "sum_speed")
_CT_HEAD = 17  # a box's result words before its histograms (include/of3d.h)
# of3d_flow_spread (csrc/kt_spread.hip): second moments about a centre, phi sums, extremes (the
# validation figure S1, plot_FigureS1_translation.ipynb cell "Calculations over time")
SPREAD_COMPONENTS = ("vx", "vy", "vz", "magnitude")  # the centre's, the extremes' and the stds' order
SPREAD_SUMS = ("ss_vx", "ss_vy", "ss_vz", "ss_magnitude", "ss_vx_vy", "ss_vx_vz", "ss_vy_vz", "sum_sin_phi",
               "sum_cos_phi")
_SPREAD_WORDS = 22  # a box's result words (include/of3d.h)


def percentile_threshold_device(rel, percentile, out=None):
    """``np.percentile(rel, percentile)`` of a CUDA tensor as a 1-element tensor of rel's dtype
    on rel's device: of3d_quantile (radix select) on the current stream, no host
    synchronisation — the value is ready for the next kernel on that stream."""
    import torch

    if not rel.is_cuda or rel.dtype not in (torch.float32, torch.float64):
        raise TypeError("rel must be a float32 or float64 CUDA tensor")
    flat = rel.contiguous().reshape(-1)
    n = flat.numel()
    if n == 0:
        raise ValueError("percentile of an empty array")
    lo, hi, gamma = _linear_ranks(n, percentile, _np_dtype(flat))
    if out is None:
        out = torch.empty(1, dtype=flat.dtype, device=flat.device)
    elif out.dtype != flat.dtype or out.device != flat.device or out.numel() != 1:
        raise ValueError("out must be one element of rel's dtype on rel's device")
    lib = _lib.load()
    f64 = int(flat.dtype == torch.float64)
    ws = torch.empty(lib.of3d_quantile_workspace_bytes(f64), dtype=torch.uint8, device=flat.device)
    _lib.check(lib.of3d_quantile(flat.data_ptr(), f64, n, lo, hi, float(gamma), out.data_ptr(), ws.data_ptr(),
                                 torch.cuda.current_stream(flat.device).cuda_stream))
    return out


@dataclasses.dataclass
class RelProfileSpec:
    """The reliability profile asked of SummarySpec(rel_profile=) (reliability_profile gives the
    same for one frame): what plot_figureS3_reliability.ipynb cells 4-8 look at to choose the
    percentile.  percentiles: 1 to 6 percentiles whose thresholds and kept-voxel counts are
    reported (they take the summary's percentile_box and percentile_method).  bins: the number of
    equal bins of the histogram of rel between the minimum and the maximum of the selection box
    (1 to 256), as plt.hist(rel.flatten(), bins); edges: ascending edges to use instead (2 to 257
    values), np.histogram(rel, bins=edges) semantics."""
    percentiles: tuple = (85, 90, 95)
    bins: int = 50
    edges: object = None

    def resolve(self):
        """Validated (percentiles [floats], nbins, edges float64 array or None); ValueError on a
        bad value."""
        ps = _check_percentiles(self.percentiles, "rel_profile percentiles", SELECT_MAX - 2)
        if self.edges is not None:
            e = SummarySpec._bin_edges(self.edges, "rel_profile")
            return ps, e.size - 1, e
        b = self.bins
        if isinstance(b, bool) or not isinstance(b, (int, np.integer)) or not 1 <= b <= MAX_BINS:
            raise ValueError(f"summary: rel_profile bins {b!r} is not an integer in 1..{MAX_BINS}")
        return ps, int(b), None


@dataclasses.dataclass
class SummarySpec:
    """What flow_summary / FlowStream(summary=) / process_flow(summary=) reduce a frame to.

    rois: boxes (z0, z1, y0, y1, x0, x1), half-open, or (y0, y1, x0, x1) in 2D; the whole
    volume is always ROI 0 and these follow it (at most 15).  bins: quantity name (vx, vy,
    vz, magnitude, theta, phi) -> ascending bin edges (at most 256 bins),
    np.histogram(values, bins=edges) semantics.  Scales and percentile as flow_statistics.
    min_size >= 1: the mask of every ROI is opened first, MATLAB's bwareaopen(rel > thresh,
    min_size, connectivity) on the cropped mask (components of fewer than min_size voxels are
    dropped; of3d_mask_open), and the summaries carry n_mask, n_components, n_components_kept
    and n_kept; 0: no opening.  connectivity: 6, 18 or 26 in 3D (default 26), 4 or 8 in 2D
    (default 8).
    axes: "mask" — the principal axes of every ROI's (opened) mask, regionprops3's EigenVectors /
    EigenValues (of3d_mask_axes), and the flow projected onto them — or a 3x3 array (rows e1 e2
    e3, each x y z) to project on instead, e.g. an earlier frame's axis_vectors, so that no
    sign flips along a movie; the mask's own axes are reported either way.  axes_physical: the
    covariance in physical units (xyscale, xyscale, zscale) before the decomposition.
    axis_bins: "axis1" / "axis2" / "axis3" -> ascending bin edges of the projections'
    histograms (at most 256 bins; axis3 in 3D only).  None: nothing of this is computed.
    weighted_bins: quantity name -> ascending bin edges, as `bins`, for magnitude-weighted
    histograms, np.histogram(values, bins=edges, weights=magnitude) (of3d_flow_whist); the same
    quantity may appear in both.
    spread: "mean" — the second moments of vx, vy, vz and the magnitude about every ROI's own
    mean (std_*, velocity_covariance), the circular spread of theta and phi and the extremes
    (of3d_flow_spread, a centred pass after the summary's) — or ndim + 1 finite numbers (vx, vy[,
    vz], magnitude; physical units) to measure the deviations from instead, e.g. the translation
    that was applied to the images (std_* is then the RMS error against it).  None: nothing of
    this is computed.
    percentile_box: one box (as a ROI's bounds) whose voxels alone form the threshold — the
    figure scripts' ``prctile(relCrop(:), relPer)`` of the cropped rel (plot_figure5.m:80-84) —
    read in place (of3d_rel_select); one box and one threshold for the call, whatever `rois`.
    percentile_method: "linear" (np.percentile's default) or "hazen" (MATLAB's prctile).
    rel_profile: a RelProfileSpec — the summary also carries rel_profile, reliability_profile's
    dict (thresholds at several percentiles, the voxels each keeps, the histogram of rel per ROI).
    With none of the three the threshold is of3d_quantile's of the whole volume."""
    rois: list | None = None
    bins: dict | None = None
    rel_percentile: float = 90
    xyscale: float = 1.0
    zscale: float = 1.0
    tscale: float = 1.0
    min_size: int = 0
    connectivity: int | None = None
    axes: object = None
    axes_physical: bool = False
    axis_bins: dict | None = None
    percentile_box: object = None
    percentile_method: str = "linear"
    rel_profile: object = None
    spread: object = None  # before weighted_bins, which stays the last field
    weighted_bins: dict | None = None

    @staticmethod
    def _box(r, ndim, dims, label):
        """One box (2 * ndim half-open bounds) validated against dims (nz, ny, nx) as 6 ints
        (z0, z1, y0, y1, x0, x1); label: what the messages call it."""
        r = tuple(r)
        if len(r) != 2 * ndim:
            raise ValueError(f"summary: {label} {r} needs {2 * ndim} bounds for a {ndim}D volume")
        if any(int(v) != v for v in r):
            raise ValueError(f"summary: {label} {r} has non-integer bounds")
        r = tuple(int(v) for v in r)
        r = r if ndim == 3 else (0, 1) + r
        for a in range(3):
            if not (0 <= r[2 * a] < r[2 * a + 1] <= dims[a]):
                raise ValueError(f"summary: {label} {r} is empty or outside the volume {dims} "
                                 f"(axis {'zyx'[a]}: need 0 <= {r[2 * a]} < {r[2 * a + 1]} <= {dims[a]})")
        return r

    def threshold_request(self, shape):
        """How the threshold is formed: validated (box, method, profile) for a volume of `shape`
        — box None (the whole volume) or 6 ints, method "linear" / "hazen", profile None or
        RelProfileSpec.resolve()'s triple; ValueError on a bad value.  All None / "linear": the
        flat select (of3d_quantile); anything else goes through of3d_rel_select."""
        shape = tuple(int(v) for v in shape)
        ndim, dims = len(shape), _dims(shape)
        box = None
        if self.percentile_box is not None:
            try:
                r = tuple(self.percentile_box)
            except TypeError:
                raise ValueError(f"summary: percentile_box {self.percentile_box!r} is not a box") from None
            try:
                box = self._box(r, ndim, dims, "percentile_box")
            except TypeError:
                raise ValueError(f"summary: percentile_box {r} has non-integer bounds") from None
        method = _check_method(self.percentile_method)
        profile = None
        if self.rel_profile is not None:
            if not isinstance(self.rel_profile, RelProfileSpec):
                raise ValueError(f"summary: rel_profile {self.rel_profile!r} is not a RelProfileSpec")
            profile = self.rel_profile.resolve()
        return box, method, profile

    @staticmethod
    def _bin_edges(e, label):
        """One histogram's edges as a validated float64 array (label: what the messages call it)."""
        e = np.ascontiguousarray(e, dtype=np.float64)
        if e.ndim != 1 or e.size < 2 or e.size > MAX_BINS + 1:
            raise ValueError(f"summary: {label} edges must be a 1-D array of 2 to {MAX_BINS + 1} values")
        if np.any(np.isnan(e)) or not np.all(e[1:] > e[:-1]):
            raise ValueError(f"summary: {label} bin edges must be strictly ascending")
        return e

    @staticmethod
    def _quantity_bins(bins, ndim, kind="", names=QUANTITIES):
        """Validated (nbins [6], edges [6 arrays or None]) of a `bins` / `weighted_bins` dict
        (kind: "" / "weighted ", for the messages); with names=PAIR_QUANTITIES (kind "pair ") the
        four of channel_compare's `bins`."""
        nbins, edges = [0] * len(names), [None] * len(names)
        for name, e in (bins or {}).items():
            if name not in names:
                raise ValueError(f"summary: unknown {kind}histogram quantity {name!r} (one of {names})")
            if ndim == 2 and name in ("vz", "phi"):
                raise ValueError(f"summary: a {kind}{name} histogram needs a 3D volume")
            q = names.index(name)
            edges[q] = SummarySpec._bin_edges(e, kind + name)
            nbins[q] = edges[q].size - 1
        return nbins, edges

    def weighted(self, ndim):
        """Validated (nbins [6], edges [6 arrays or None]) of weighted_bins for an ndim-D volume
        (all 0 / None without any); ValueError on a bad name or bad edges."""
        return self._quantity_bins(self.weighted_bins, ndim, "weighted ")

    def spread_request(self, ndim):
        """None without spread, else a validated 1-tuple (given,): given = None for "mean" or the
        4 float64 values vx vy vz magnitude (vz = 0 in 2D); ValueError on a bad value."""
        if self.spread is None:
            return None
        what = f"'mean' or {ndim + 1} numbers (vx, vy{', vz' if ndim == 3 else ''}, magnitude)"
        if isinstance(self.spread, str):
            if self.spread != "mean":
                raise ValueError(f"summary: spread {self.spread!r} is not {what}")
            return (None,)
        try:
            given = np.ascontiguousarray(self.spread, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"summary: spread {self.spread!r} is not {what}") from None
        if given.shape != (ndim + 1,):
            raise ValueError(f"summary: spread must be {what} for a {ndim}D volume, got shape {given.shape}")
        if not np.all(np.isfinite(given)):
            raise ValueError("summary: spread centre must be finite")
        return (np.array([given[0], given[1], given[2] if ndim == 3 else 0.0, given[-1]]),)

    def axes_request(self, ndim):
        """None without axes, else validated (given, nbins3, edges3): given = None for "mask" or
        the 9 float64 values of the 3x3 array; ValueError on a bad value."""
        if self.axes is None:
            if self.axis_bins:
                raise ValueError("summary: axis_bins needs axes")
            return None
        given = None
        if isinstance(self.axes, str):
            if self.axes != "mask":
                raise ValueError(f"summary: axes {self.axes!r} is not 'mask' or a 3x3 array")
        else:
            try:
                given = np.ascontiguousarray(self.axes, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError(f"summary: axes {self.axes!r} is not 'mask' or a 3x3 array") from None
            if given.shape != (3, 3):
                raise ValueError(f"summary: axes must be a 3x3 array, got shape {given.shape}")
            if not np.all(np.isfinite(given)):
                raise ValueError("summary: axes must be finite")
            given = given.reshape(9).copy()
        nbins, edges = [0] * 3, [None] * 3
        for name, e in (self.axis_bins or {}).items():
            if name not in AXIS_NAMES:
                raise ValueError(f"summary: unknown axis histogram {name!r} (one of {AXIS_NAMES})")
            if ndim == 2 and name == "axis3":
                raise ValueError("summary: an axis3 histogram needs a 3D volume")
            k = AXIS_NAMES.index(name)
            edges[k] = self._bin_edges(e, name)
            nbins[k] = edges[k].size - 1
        return given, nbins, edges

    def opening(self, ndim):
        """Validated (min_size, connectivity) for an ndim-D volume; ValueError on a bad value."""
        m = self.min_size
        if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or m < 0:
            raise ValueError(f"summary: min_size {m!r} is not a non-negative integer")
        allowed = CONNECTIVITIES[ndim]
        c = allowed[-1] if self.connectivity is None else self.connectivity
        if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or c not in allowed:
            raise ValueError(f"summary: connectivity {c!r} is not one of {allowed} for a {ndim}D volume")
        return int(m), int(c)

    def resolve(self, shape):
        """Validated (boxes int64 (n_roi, 6), nbins [6], edges [6 arrays or None]) for a volume
        of `shape` ((nz, ny, nx) or (ny, nx)); ValueError on a bad box, bad edges or a bad
        min_size / connectivity."""
        shape = tuple(int(v) for v in shape)
        if len(shape) not in (2, 3) or min(shape) < 1:
            raise ValueError(f"summary: volume shape {shape} is not 2D or 3D")
        ndim = len(shape)
        self.opening(ndim)
        dims = _dims(shape)
        if not (0 <= float(self.rel_percentile) <= 100):
            raise ValueError(f"summary: rel_percentile {self.rel_percentile} outside [0, 100]")
        boxes = [(0, dims[0], 0, dims[1], 0, dims[2])]
        for i, r in enumerate(self.rois or ()):
            boxes.append(self._box(r, ndim, dims, f"ROI {i + 1}"))
        if len(boxes) > MAX_ROI:
            raise ValueError(f"summary: at most {MAX_ROI - 1} ROIs beside the whole volume, got {len(boxes) - 1}")
        nbins, edges = self._quantity_bins(self.bins, ndim)
        self.weighted(ndim)
        self.spread_request(ndim)
        self.threshold_request(shape)
        return np.array(boxes, dtype=np.int64), nbins, edges


def _decode_hists(body, off, names, nbins, edges, view_dtype, hist, edges_out):
    """The histograms of a result block: body (n_roi, words) int64, the requested ones of `names`
    one after the other from column `off`; hist[name] (n_roi, nbins) viewed as view_dtype and
    edges_out[name] filled."""
    for q, name in enumerate(names):
        if nbins[q]:
            hist[name] = np.ascontiguousarray(body[:, off:off + nbins[q]]).view(view_dtype)
            edges_out[name] = edges[q].copy()
            off += nbins[q]


def _decode_open_counts(words, n_roi, out):
    """of3d_mask_open's d_counts (4 int64 words per box, from words[0]) as out[name] per box."""
    counts = np.asarray(words[:4 * n_roi]).reshape(n_roi, 4)
    for i, name in enumerate(OPEN_COUNTS):
        out[name] = counts[:, i].copy()


def _word_threshold(words, rel_f64):
    """The threshold a pass left in the first word of its result (a double) as a numpy scalar of
    rel's dtype."""
    return (np.float64 if rel_f64 else np.float32)(words[:1].view(np.float64)[0])


class _BoxCall:
    """What every summary pass is bound to: the library, the boxes (int64 (n_roi, 6)) with their
    ctypes view, the volume's dims (nz, ny, nx), whether rel is float64 and, for the passes over
    physical velocities, the scales (xyscale, zscale, tscale) as floats.

    The passes that follow the threshold on a frame (_AxesCall, _WhistCall, _SpreadCall,
    _ProfileCall, _QuiverCall, _ContractCall, _ExportCall) share one calling convention:
    ``enqueue(fields, thresh_ptr, keep_ptr, result_ptr, stream)`` — fields: the frame's device
    pointers and velocity type (vx, vy, vz or None, rel, v_f32), _Frame.fields; thresh_ptr: the
    threshold on the device; keep_ptr: the opened mask's keep volume or None; result_ptr: where
    the pass's result_bytes go (new_result allocates them)."""

    def __init__(self, boxes, dims, rel_f64, scales=None):
        self.lib, self.dims, self.rel_f64 = _lib.load(), tuple(dims), int(rel_f64)
        self.scales = None if scales is None else tuple(float(v) for v in scales)
        self.boxes = np.ascontiguousarray(boxes, dtype=np.int64)
        self.roi_arr = self.boxes.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))

    def new_result(self, device):
        """The result block (result_bytes) on `device`, 16-byte aligned as of3d_field_export asks."""
        import torch

        res = torch.empty(self.result_bytes // 8, dtype=torch.int64, device=device)
        assert res.data_ptr() % 16 == 0
        return res

    def _bind_bins(self, nbins, edges):
        """nbins / edges (one entry per quantity, None without bins) kept, with their ctypes arrays."""
        self.nbins, self.edges = list(nbins), list(edges)
        D = ctypes.POINTER(ctypes.c_double)
        self.nb_arr = (ctypes.c_int * len(self.nbins))(*self.nbins)
        self.edge_arr = (D * len(self.edges))(*[e.ctypes.data_as(D) if e is not None else None for e in self.edges])

    @staticmethod
    def _workspace(nbytes, device):
        """A workspace of the size a *_workspace_bytes function gave; 0 is its refusal of the boxes."""
        import torch

        if nbytes == 0:
            raise ValueError("of3d: " + _lib.last_error())
        return torch.empty(nbytes, dtype=torch.uint8, device=device)


class _OpenCall(_BoxCall):
    """of3d_mask_open bound to boxes and a device: the keep volume and the label / size
    workspace, allocated once."""

    def __init__(self, boxes, dims, rel_f64, min_size, connectivity, device):
        import torch

        super().__init__(boxes, dims, rel_f64)
        self.min_size, self.connectivity = int(min_size), int(connectivity)
        self.ws = self._workspace(self.lib.of3d_mask_open_workspace_bytes(self.roi_arr, len(self.boxes)), device)
        self.keep = torch.empty(self.dims, dtype=torch.uint16, device=device)
        self.result_bytes = 32 * len(self.boxes)  # d_counts

    def enqueue(self, rel, thresh_ptr, counts_ptr, stream):
        _lib.check(self.lib.of3d_mask_open(rel, self.rel_f64, *self.dims, thresh_ptr, self.roi_arr, len(self.boxes),
                                           self.min_size, self.connectivity, self.keep.data_ptr(), counts_ptr,
                                           self.ws.data_ptr(), stream or None))

    def decode(self, words, out):
        _decode_open_counts(words, len(self.boxes), out)
        return out

    def enqueue_pair(self, rel0, thresh0_ptr, rel1, thresh1_ptr, floor, combine, counts_ptr, stream):
        """of3d_mask_open_pair: the joint mask of two channels, opened like the single one."""
        _lib.check(self.lib.of3d_mask_open_pair(rel0, thresh0_ptr, rel1, thresh1_ptr, self.rel_f64, float(floor),
                                                int(combine), *self.dims, self.roi_arr, len(self.boxes),
                                                self.min_size, self.connectivity, self.keep.data_ptr(), counts_ptr,
                                                self.ws.data_ptr(), stream or None))


class _AxesCall(_BoxCall):
    """of3d_mask_axes bound to boxes and a device: sizes, the workspace and the decoding."""

    def __init__(self, boxes, dims, rel_f64, request, physical, scales, device):
        super().__init__(boxes, dims, rel_f64, scales)
        self.given = request[0]
        self._bind_bins(*request[1:])
        self.physical = int(bool(physical))
        self.given_arr = (self.given.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
                          if self.given is not None else None)
        self.ws = self._workspace(self.lib.of3d_mask_axes_workspace_bytes(self.roi_arr, len(self.boxes)), device)
        self.result_bytes = self.lib.of3d_mask_axes_result_bytes(len(self.boxes), self.nb_arr)

    def enqueue(self, fields, thresh_ptr, keep_ptr, result_ptr, stream):
        """Moments, axes and (vx given) projection kernels on `stream` (device pointers)."""
        vx, vy, vz, rel, v_f32 = fields
        _lib.check(self.lib.of3d_mask_axes(vx or None, vy or None, vz or None, rel, int(v_f32), self.rel_f64,
                                           *self.dims, thresh_ptr, *self.scales, self.roi_arr, len(self.boxes),
                                           keep_ptr or None, self.given_arr, self.physical, self.nb_arr,
                                           self.edge_arr, result_ptr, self.ws.data_ptr(), stream or None))

    def decode(self, words, out, projected=True):
        """The block's words (host int64) added to the dict `out` (flow_summary's keys)."""
        n_roi, ntot = len(self.boxes), sum(self.nbins)
        body = np.ascontiguousarray(words[:n_roi * (_AX_HEAD + ntot)], dtype=np.int64).reshape(n_roi, _AX_HEAD + ntot)
        f = lambda a, b: np.ascontiguousarray(body[:, a:b]).view(np.float64)
        out["moments"] = np.ascontiguousarray(body[:, :10]).view(np.uint64)
        out["n_axes_mask"] = body[:, 0].copy()
        out["centroid"] = f(10, 13)
        c = f(13, 19)
        out["covariance"] = c[:, [0, 3, 4, 3, 1, 5, 4, 5, 2]].reshape(n_roi, 3, 3)
        out["axis_values"] = f(19, 22)
        out["axis_vectors"] = f(22, 31).reshape(n_roi, 3, 3)
        out["axes_used"] = f(31, 40).reshape(n_roi, 3, 3)
        if not projected:
            return out
        out["n_axes_valid"] = body[:, 40].copy()
        sums = f(41, 44)
        nv = out["n_axes_valid"].astype(np.float64)
        nv[nv == 0] = np.nan
        for k, name in enumerate(AXIS_NAMES):
            out["sum_" + name] = sums[:, k].copy()
            out["mean_" + name] = sums[:, k] / nv
        _decode_hists(body, _AX_HEAD, AXIS_NAMES, self.nbins, self.edges, np.uint64, out["hist"], out["edges"])
        return out


class _WhistCall(_BoxCall):
    """of3d_flow_whist bound to boxes and a device: sizes, the workspace and the decoding."""

    def __init__(self, boxes, dims, rel_f64, nbins, edges, scales, device):
        super().__init__(boxes, dims, rel_f64, scales)
        self._bind_bins(nbins, edges)
        self.ws = self._workspace(
            self.lib.of3d_flow_whist_workspace_bytes(self.roi_arr, len(self.boxes), self.nb_arr), device)
        self.result_bytes = self.lib.of3d_flow_whist_result_bytes(len(self.boxes), self.nb_arr)

    def enqueue(self, fields, thresh_ptr, keep_ptr, result_ptr, stream):
        """The accumulation and final kernels on `stream` (device pointers)."""
        vx, vy, vz, rel, v_f32 = fields
        _lib.check(self.lib.of3d_flow_whist(vx, vy, vz or None, rel, int(v_f32), self.rel_f64, *self.dims,
                                            thresh_ptr, *self.scales, self.roi_arr, len(self.boxes),
                                            keep_ptr or None, self.nb_arr, self.edge_arr, result_ptr,
                                            self.ws.data_ptr(), stream or None))

    def decode(self, words, out):
        """The block's words (host int64) added to the dict `out` (flow_summary's keys)."""
        n_roi, ntot = len(self.boxes), sum(self.nbins)
        body = np.ascontiguousarray(words[:n_roi * (1 + ntot)], dtype=np.int64).reshape(n_roi, 1 + ntot)
        assert np.array_equal(body[:, 0], out["n_valid"]), (body[:, 0], out["n_valid"])
        out["hist_weighted"], out["edges_weighted"] = {}, {}
        _decode_hists(body, 1, QUANTITIES, self.nbins, self.edges, np.float64, out["hist_weighted"],
                      out["edges_weighted"])
        return out


class _SpreadCall(_BoxCall):
    """of3d_flow_spread bound to boxes and a device: sizes, the workspace and the decoding.
    given: None (every box about its own mean, read on the device from the summary's result) or
    the 4 float64 values of SummarySpec.spread_request.  It follows a summary in the summary's own
    result block: summary_nbins are that summary's ctypes nbins, and its words begin
    summary_before bytes ahead of the spread's."""

    def __init__(self, boxes, dims, rel_f64, given, ndim, scales, device, summary_nbins, summary_before):
        super().__init__(boxes, dims, rel_f64, scales)
        self.given, self.ndim = given, int(ndim)
        self.summary_nbins, self.summary_before = summary_nbins, int(summary_before)
        self.given_arr = given.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if given is not None else None
        self.ws = self._workspace(self.lib.of3d_flow_spread_workspace_bytes(self.roi_arr, len(self.boxes)), device)
        self.result_bytes = self.lib.of3d_flow_spread_result_bytes(len(self.boxes))

    def enqueue(self, fields, thresh_ptr, keep_ptr, result_ptr, stream):
        """The accumulation and final kernels on `stream` (device pointers), after the summary
        whose result lies summary_before bytes ahead of result_ptr."""
        vx, vy, vz, rel, v_f32 = fields
        _lib.check(self.lib.of3d_flow_spread(vx, vy, vz or None, rel, int(v_f32), self.rel_f64, *self.dims,
                                             thresh_ptr, *self.scales, self.roi_arr, len(self.boxes),
                                             keep_ptr or None, result_ptr - self.summary_before, self.summary_nbins,
                                             self.given_arr, result_ptr, self.ws.data_ptr(), stream or None))

    def decode(self, words, out):
        """The block's words (host int64) added to the dict `out` (flow_summary's keys)."""
        n_roi = len(self.boxes)
        body = np.ascontiguousarray(words[:n_roi * _SPREAD_WORDS], dtype=np.int64).reshape(n_roi, _SPREAD_WORDS)
        assert np.array_equal(body[:, 0], out["n_valid"]), (body[:, 0], out["n_valid"])
        f = np.ascontiguousarray(body[:, 1:]).view(np.float64)
        out["spread_center"] = f[:, 0:4].copy()
        for i, k in enumerate(SPREAD_SUMS):
            out[k] = f[:, 4 + i].copy()
        for i, k in enumerate(SPREAD_COMPONENTS):
            out["min_" + k], out["max_" + k] = f[:, 13 + i].copy(), f[:, 17 + i].copy()
        nv = out["n_valid"].astype(np.float64)
        nv[nv == 0] = np.nan  # empty box: NaN, no division warnings
        for k in SPREAD_COMPONENTS:
            out["std_" + k] = np.sqrt(out["ss_" + k] / nv)  # ddof 0, as np.nanstd
        c = np.stack([out[k] for k in SPREAD_SUMS[:7]], axis=1) / nv[:, None]
        out["velocity_covariance"] = c[:, [0, 4, 5, 4, 1, 6, 5, 6, 2]].reshape(n_roi, 3, 3)
        n_all = out["n_voxels"].astype(np.float64)

        def circular(prefix, sn, cs):
            # the notebook's (scipy.stats.circstd's) sqrt(-2 ln R); rounding can leave R an ulp above 1
            with np.errstate(divide="ignore"):
                r = np.hypot(sn, cs) / nv
                out[prefix + "_resultant"] = r
                out[prefix + "_std"] = np.sqrt(np.maximum(0.0, -2.0 * np.log(r)))
                # the notebook divides its sums by the array's size, NaNs included: R * n_valid / n_voxels
                out[prefix + "_std_all"] = np.sqrt(np.maximum(0.0, -2.0 * np.log(r * nv / n_all)))

        circular("theta", out["sum_sin"], out["sum_cos"])
        if self.ndim == 3:
            out["phi_mean"] = np.arctan2(out["sum_sin_phi"] / nv, out["sum_cos_phi"] / nv)
            circular("phi", out["sum_sin_phi"], out["sum_cos_phi"])
        return out


@dataclasses.dataclass
class QuiverSpec:
    """The vectors of a quiver plot of every ROI, asked of quiver_sample / FlowStream(quiver=) /
    process_flow(quiver=): what the figure scripts hand to quiver / quiver3
    (plot_figure4_Movies.m:121-143: every gap-th voxel of the ROI whose masked velocity is not NaN).

    gap: an int (every axis), or (gz, gy, gx) — (gy, gx) in 2D — each >= 1; the lattice is
    anchored at each ROI's origin.  max_vectors: the records kept per ROI at most (the first ones
    in C order; n_valid still counts all of them), >= 0."""
    gap: object = 2
    max_vectors: int = 65536

    def resolve(self, ndim):
        """Validated ((gz, gy, gx), max_vectors) for an ndim-D volume (2D: gz = 1); ValueError on
        a bad value."""
        is_int = lambda v: not isinstance(v, bool) and isinstance(v, (int, np.integer))
        g = self.gap
        if is_int(g):
            g = (g,) * ndim
        else:
            try:
                g = tuple(g)
            except TypeError:
                raise ValueError(f"quiver: gap {self.gap!r} is not an integer or {ndim} integers") from None
        if len(g) != ndim or not all(is_int(v) for v in g):
            raise ValueError(f"quiver: gap {self.gap!r} is not an integer or {ndim} integers for a {ndim}D volume")
        if min(g) < 1:
            raise ValueError(f"quiver: gap {self.gap!r} must be at least 1 on every axis")
        m = self.max_vectors
        if not is_int(m) or m < 0:
            raise ValueError(f"quiver: max_vectors {m!r} is not a non-negative integer")
        g = tuple(int(v) for v in g)
        return (g if ndim == 3 else (1,) + g), int(m)


def _quiver_entry(zyx, v, ndim, n_lattice, n_valid):
    """One ROI's entry of a quiver sample from its stored volume coordinates (int64 (n, 3)) and
    physical velocities (float64 (n, 3)): with them magnitude, theta and (3D) phi, formed here on
    the host with example_analysis_script.ipynb cell 6's expressions."""
    vx, vy, vz = v[:, 0], v[:, 1], v[:, 2]
    out = {"zyx": zyx, "v": v, "n_lattice": int(n_lattice), "n_valid": int(n_valid),
           "truncated": int(n_valid) > len(zyx)}
    with np.errstate(invalid="ignore", divide="ignore"):
        if ndim == 3:
            out["magnitude"] = np.sqrt(np.power(vx, 2) + np.power(vy, 2) + np.power(vz, 2))
            out["phi"] = np.arctan(vz / np.sqrt(np.power(vx, 2) + np.power(vy, 2)))
        else:
            out["magnitude"] = np.sqrt(np.power(vx, 2) + np.power(vy, 2))
        out["theta"] = np.arctan2(vy, vx)
    return out


class _QuiverCall(_BoxCall):
    """of3d_quiver_sample bound to boxes and a device: the capacities, sizes, the workspace and
    the decoding."""

    def __init__(self, boxes, dims, rel_f64, quiver, ndim, scales, device):
        super().__init__(boxes, dims, rel_f64, scales)
        self.ndim = int(ndim)
        self.gap, self.max_vectors = quiver.resolve(self.ndim)
        ext = self.boxes[:, 1::2] - self.boxes[:, 0::2]
        self.n_lattice = np.prod((ext - 1) // np.array(self.gap, dtype=np.int64) + 1, axis=1).astype(np.int64)
        self.capacity = np.ascontiguousarray(np.minimum(self.n_lattice, self.max_vectors), dtype=np.int64)
        I = ctypes.POINTER(ctypes.c_int64)
        self.gap_arr = (ctypes.c_int64 * 3)(*self.gap)
        self.cap_arr = self.capacity.ctypes.data_as(I)
        self.ws = self._workspace(self.lib.of3d_quiver_workspace_bytes(self.roi_arr, len(self.boxes), self.gap_arr),
                                  device)
        self.result_bytes = self.lib.of3d_quiver_result_bytes(len(self.boxes), self.cap_arr)
        if self.result_bytes == 0:
            raise ValueError("of3d: " + _lib.last_error())

    def enqueue(self, fields, thresh_ptr, keep_ptr, result_ptr, stream):
        """The count, scan and emit kernels on `stream` (device pointers)."""
        vx, vy, vz, rel, v_f32 = fields
        _lib.check(self.lib.of3d_quiver_sample(vx, vy, vz or None, rel, int(v_f32), self.rel_f64, *self.dims,
                                               thresh_ptr, *self.scales, self.roi_arr, len(self.boxes),
                                               self.gap_arr, self.cap_arr, keep_ptr or None, result_ptr,
                                               self.ws.data_ptr(), stream or None))

    def decode(self, words):
        """The result words (host int64 array) as the per-ROI list of quiver_sample."""
        words = np.ascontiguousarray(words, dtype=np.int64)
        n_roi = len(self.boxes)
        assert words[1] == n_roi and tuple(words[2:5]) == self.gap and words[5] == (self.ndim == 3), words[:6]
        out = []
        for r in range(n_roi):
            n_lattice, n_valid, n_stored, off = (int(v) for v in words[6 + 4 * r:10 + 4 * r])
            cap = int(self.capacity[r])
            assert n_lattice == self.n_lattice[r] and n_stored == min(n_valid, cap), (r, n_lattice, n_valid, n_stored)
            block = words[off:off + 4 * cap].reshape(4, cap)
            v = np.ascontiguousarray(block[1:, :n_stored].T).view(np.float64)
            zyx = np.stack(np.unravel_index(block[0, :n_stored], self.dims), axis=1).astype(np.int64).reshape(-1, 3)
            out.append(_quiver_entry(zyx, v, self.ndim, n_lattice, n_valid))
        return out


EXPORT_FIELDS = ("vx", "vy", "vz", "rel")  # of3d_field_export's field bits, in order
EXPORT_MASKS = {None: 0, "nan": 1, "zero": 2, "summary": 3}  # its mask_mode
_EXPORT_HEAD, _EXPORT_ROI, _EXPORT_SKIP = 8, 6, 16  # OF3D_EXPORT_HEAD_WORDS, _ROI_WORDS, _SKIP_SHIFT


@dataclasses.dataclass
class FieldSpec:
    """The fields themselves, cropped to ROIs of the summary, asked of export_fields /
    FlowStream(fields=) / process_flow(save_fields=): what the figure scripts keep of the four
    full-size outputs (``vx(y1:y2,x1:x2,z1:z2)``, then ``vx.*relMask./relMask*xyscale/tscale``).

    rois: indices into the summary's ROI list (0 = the whole volume); None: every ROI after 0,
    or (0,) when there are none.  fields: names among vx, vy, vz, rel (2D: vz is dropped from the
    default, and an error if named).  mask — what the (opened) reliability mask m does to a
    velocity: None: nothing (the plain crop); "nan": ``(v*m)/m``, the figures' ``v.*relMask./relMask``;
    "zero": ``v*m`` (plot_FigureS2_dt.m:123); "summary": ``v*m`` with exact zeros -> NaN, the
    notebooks' and flow_summary's masking.  rel is always the plain crop.  physical: velocities
    then become ``(v*xyscale)/tscale`` (vz: zscale).  dtype: None — every block in its field's own
    type — or "float32": every value narrowed once, from the float64 it was computed in."""
    rois: tuple | None = None
    fields: tuple = EXPORT_FIELDS
    mask: str | None = "nan"
    physical: bool = True
    dtype: str | None = None

    @staticmethod
    def _roi_indices(given, n_roi, what):
        """A `rois` request (FieldSpec's, ProjectionSpec's) as validated indices into the
        summary's n_roi boxes; `what` begins the messages."""
        is_int = lambda v: not isinstance(v, bool) and isinstance(v, (int, np.integer))
        if given is None:
            return tuple(range(1, n_roi)) or (0,)
        try:
            rois = tuple(given)
        except TypeError:
            raise ValueError(f"{what}: rois {given!r} is not a sequence of ROI indices") from None
        if not rois or not all(is_int(r) for r in rois):
            raise ValueError(f"{what}: rois {given!r} is not a non-empty sequence of ROI indices")
        if any(not 0 <= r < n_roi for r in rois):
            raise ValueError(f"{what}: ROI index out of range in {rois} (the summary has ROIs 0..{n_roi - 1})")
        if len(set(rois)) != len(rois):
            raise ValueError(f"{what}: duplicate ROI index in {rois}")
        return tuple(int(r) for r in rois)

    def resolve(self, ndim, n_roi):
        """Validated (rois, names, field bits, mask_mode, physical, out_f32) for an ndim-D volume
        whose summary has n_roi boxes (the whole volume included); ValueError on a bad value."""
        rois = self._roi_indices(self.rois, n_roi, "fields")
        if self.fields is EXPORT_FIELDS:
            names = tuple(n for n in EXPORT_FIELDS if ndim == 3 or n != "vz")
        else:
            if isinstance(self.fields, str):
                raise ValueError(f"fields: fields {self.fields!r} is not a sequence of names among {EXPORT_FIELDS}")
            try:
                names = tuple(self.fields)
            except TypeError:
                raise ValueError(f"fields: fields {self.fields!r} is not a sequence of names among "
                                 f"{EXPORT_FIELDS}") from None
            if not names:
                raise ValueError("fields: no field named")
            for n in names:
                if n not in EXPORT_FIELDS:
                    raise ValueError(f"fields: unknown field name {n!r} (one of {EXPORT_FIELDS})")
            if len(set(names)) != len(names):
                raise ValueError(f"fields: duplicate field name in {names}")
            if ndim == 2 and "vz" in names:
                raise ValueError("fields: a 2D volume has no vz to export")
        if self.mask is not None and (not isinstance(self.mask, str) or self.mask not in EXPORT_MASKS):
            raise ValueError(f"fields: mask {self.mask!r} is not None, 'nan', 'zero' or 'summary'")
        if self.dtype is not None and (not isinstance(self.dtype, str) or self.dtype != "float32"):
            raise ValueError(f"fields: dtype {self.dtype!r} is not None or 'float32'")
        bits = sum(1 << EXPORT_FIELDS.index(n) for n in names)
        return rois, names, bits, EXPORT_MASKS[self.mask], bool(self.physical), self.dtype == "float32"


class _ExportCall(_BoxCall):
    """of3d_field_export bound to the summary's boxes, of which spec.rois are exported (the
    others are listed and skipped, so every box keeps its bit of the keep volume): the size, the
    launch and the decoding.  v_f32: whether the velocity fields are float32."""

    def __init__(self, boxes, dims, rel_f64, v_f32, spec, ndim, scales):
        super().__init__(boxes, dims, rel_f64, scales)
        self.ndim, self.v_f32 = int(ndim), int(bool(v_f32))
        self.rois, self.names, _, self.mask_mode, self.physical, self.out_f32 = spec.resolve(self.ndim,
                                                                                             len(self.boxes))
        self.fields, self.result_bytes = self.size(self.boxes, self.rel_f64, self.v_f32, spec, self.ndim)
        self.v_dtype = np.dtype(np.float32 if self.out_f32 or self.v_f32 else np.float64)
        self.rel_dtype = np.dtype(np.float32 if self.out_f32 or not self.rel_f64 else np.float64)

    @staticmethod
    def size(boxes, rel_f64, v_f32, spec, ndim):
        """(of3d_field_export's `fields` word, its result bytes) for spec (a FieldSpec) over boxes:
        what a block costs, known from the boxes, the types and the spec alone — FlowStream sizes
        its buffers with it before any call exists."""
        boxes = np.ascontiguousarray(boxes, dtype=np.int64)
        rois, _, bits, _, _, out_f32 = spec.resolve(int(ndim), len(boxes))
        f = bits | sum(1 << (_EXPORT_SKIP + r) for r in range(len(boxes)) if r not in rois)
        f = f - (1 << 32) if f >> 31 else f  # as a C int
        nbytes = _lib.load().of3d_field_export_result_bytes(boxes.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                                            len(boxes), f, int(bool(v_f32)), int(bool(rel_f64)),
                                                            int(out_f32))
        if nbytes == 0:
            raise ValueError("of3d: " + _lib.last_error())
        return f, nbytes

    def enqueue(self, fields, thresh_ptr, keep_ptr, result_ptr, stream):
        """The export kernel and its header on `stream` (device pointers)."""
        vx, vy, vz, rel, v_f32 = fields
        if self.v_f32 != int(bool(v_f32)):
            raise ValueError("summary: the export was sized for the other velocity type")
        _lib.check(self.lib.of3d_field_export(vx, vy, vz or None, rel, self.v_f32, self.rel_f64, *self.dims,
                                              thresh_ptr, *self.scales, self.roi_arr, len(self.boxes), self.fields,
                                              self.mask_mode, int(self.physical), int(self.out_f32),
                                              keep_ptr or None, result_ptr, stream or None))

    def decode(self, words):
        """The result words as export_fields' `blocks`: views of `words`, a host int64 array or
        an int64 tensor (which stays where it is; only its header is read on the host)."""
        n_roi, host = len(self.boxes), isinstance(words, np.ndarray)
        nhead = _EXPORT_HEAD + _EXPORT_ROI * n_roi
        head = words[:nhead] if host else words[:nhead].cpu().numpy()
        assert (head[1] == n_roi and head[2] == self.fields & 0xFFFFFFFF and head[3] == self.mask_mode
                and head[6] == (self.ndim == 3) and head[7] * 8 == self.result_bytes), head[:8]
        out = []
        for r in self.rois:
            box = tuple(int(v) for v in self.boxes[r])
            n, sizes, *offs = (int(v) for v in head[_EXPORT_HEAD + _EXPORT_ROI * r:_EXPORT_HEAD + _EXPORT_ROI * (r + 1)])
            shape = tuple(box[2 * a + 1] - box[2 * a] for a in range(3))
            assert n == int(np.prod(shape)) and sizes == self.v_dtype.itemsize + 256 * self.rel_dtype.itemsize
            entry = {"roi": r, "box": box}
            for name in self.names:
                dt = self.rel_dtype if name == "rel" else self.v_dtype
                off = offs[EXPORT_FIELDS.index(name)]
                flat = words[off:off + (n * dt.itemsize + 7) // 8]
                if host:
                    flat = flat.view(dt)[:n]
                else:
                    import torch

                    flat = flat.view(getattr(torch, dt.name))[:n]
                entry[name] = flat.reshape(shape if self.ndim == 3 else shape[1:])
            out.append(entry)
        return out


PROJECT_AXES = ("z", "y", "x")  # of3d_flow_project's axis bits, in order
PROJECT_MAPS = ("n_mask", "n_valid", "sum_vx", "sum_vy", "sum_vz", "sum_magnitude", "max_magnitude", "max_image",
                "sum_image")  # its map bits, in order
PROJECT_IMAGE_MAPS = PROJECT_MAPS[7:]
_PROJECT_HEAD, _PROJECT_ROI, _PROJECT_SKIP = 8, 6, 16  # OF3D_PROJECT_HEAD_WORDS, _ROI_WORDS, _SKIP_SHIFT


@dataclasses.dataclass
class ProjectionSpec:
    """Projection maps of ROIs of the summary, asked of projection_maps / FlowStream(project=) /
    process_flow(project=): one value per line of a ROI along an axis — the picture the figure
    scripts draw their vectors on (``max(myo,[],3)``), the mask's footprint (``sum(relMask,3)``)
    and the depth-summed flow.

    axes: names among "z", "y", "x" (the axis projected away); None: ("z",) in 3D, ("y", "x") in
    2D, where "z" is an error.  maps: names among PROJECT_MAPS; None: n_mask, n_valid, sum_vx,
    sum_vy, sum_vz (3D), sum_magnitude, max_magnitude and, with image, max_image and sum_image.
    rois: as FieldSpec.rois.  image: an image volume is projected too (projection_maps' image=;
    in a stream the window's centre frame)."""
    axes: tuple | None = None
    maps: tuple | None = None
    rois: tuple | None = None
    image: bool = False

    @staticmethod
    def _names(given, allowed, what):
        if isinstance(given, str):
            raise ValueError(f"project: {what} {given!r} is not a sequence of names among {allowed}")
        try:
            names = tuple(given)
        except TypeError:
            raise ValueError(f"project: {what} {given!r} is not a sequence of names among {allowed}") from None
        if not names:
            raise ValueError(f"project: no name in {what}")
        for n in names:
            if n not in allowed:
                raise ValueError(f"project: unknown name {n!r} in {what} (one of {allowed})")
        if len(set(names)) != len(names):
            raise ValueError(f"project: duplicate name in {what} {names}")
        return tuple(n for n in allowed if n in names)  # in bit order

    def resolve(self, ndim, n_roi):
        """Validated (rois, axes, axis bits, maps, map bits) for an ndim-D volume whose summary
        has n_roi boxes (the whole volume included), the names in bit order; ValueError on a bad
        value."""
        rois = FieldSpec._roi_indices(self.rois, n_roi, "project")
        if self.axes is None:
            axes = ("z",) if ndim == 3 else ("y", "x")
        else:
            axes = self._names(self.axes, PROJECT_AXES, "axes")
            if ndim == 2 and "z" in axes:
                raise ValueError("project: a 2D volume has no z axis to project along")
        image = bool(self.image)
        if self.maps is None:
            maps = tuple(n for n in PROJECT_MAPS[:7] if ndim == 3 or n != "sum_vz") + (PROJECT_IMAGE_MAPS if image
                                                                                     else ())
        else:
            maps = self._names(self.maps, PROJECT_MAPS, "maps")
            if ndim == 2 and "sum_vz" in maps:
                raise ValueError("project: a 2D volume has no sum_vz")
            if not image and any(n in PROJECT_IMAGE_MAPS for n in maps):
                raise ValueError("project: max_image and sum_image need image=True")
        return (rois, axes, sum(1 << PROJECT_AXES.index(a) for a in axes), maps,
                sum(1 << PROJECT_MAPS.index(n) for n in maps))


class _ProjectCall(_BoxCall):
    """of3d_flow_project bound to the summary's boxes, of which spec.rois are projected (the
    others are listed and skipped, so every box keeps its bit of the keep volume): the size, the
    launch and the decoding.  The image changes per frame: bind_image names it before enqueue."""

    def __init__(self, boxes, dims, rel_f64, spec, ndim, scales):
        super().__init__(boxes, dims, rel_f64, scales)
        self.ndim = int(ndim)
        self.rois, self.axes, self.axis_bits, self.names, _ = spec.resolve(self.ndim, len(self.boxes))
        self.needs_image = any(n in PROJECT_IMAGE_MAPS for n in self.names)
        self.maps, self.result_bytes = self.size(self.boxes, spec, self.ndim)
        self.image_ptr, self.image_code = None, 0

    @staticmethod
    def size(boxes, spec, ndim):
        """(of3d_flow_project's `maps` word, its result bytes) for spec (a ProjectionSpec) over
        boxes: known from the boxes and the spec alone — FlowStream sizes its buffers with it
        before any call exists.  The image's dtype does not change the layout."""
        boxes = np.ascontiguousarray(boxes, dtype=np.int64)
        rois, _, axis_bits, names, bits = spec.resolve(int(ndim), len(boxes))
        m = bits | sum(1 << (_PROJECT_SKIP + r) for r in range(len(boxes)) if r not in rois)
        m = m - (1 << 32) if m >> 31 else m  # as a C int
        image = _lib.OF3D_F64 if any(n in PROJECT_IMAGE_MAPS for n in names) else 0
        nbytes = _lib.load().of3d_flow_project_result_bytes(boxes.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                                            len(boxes), axis_bits, m, int(ndim == 3), image)
        if nbytes == 0:
            raise ValueError("of3d: " + _lib.last_error())
        return m, nbytes

    def bind_image(self, ptr, code):
        """The image volume of the next enqueue: its device pointer and of3d_dtype code."""
        self.image_ptr, self.image_code = ptr, int(code)

    def enqueue(self, fields, thresh_ptr, keep_ptr, result_ptr, stream):
        """The line kernels and the header on `stream` (device pointers)."""
        vx, vy, vz, rel, v_f32 = fields
        if self.needs_image and not self.image_ptr:
            raise ValueError("project: the image maps need an image (bind_image)")
        _lib.check(self.lib.of3d_flow_project(vx, vy, vz or None, rel, int(v_f32), self.rel_f64, *self.dims,
                                              thresh_ptr, *self.scales, self.roi_arr, len(self.boxes),
                                              self.axis_bits, self.maps, self.image_ptr if self.needs_image else None,
                                              self.image_code if self.needs_image else 0, keep_ptr or None,
                                              result_ptr, stream or None))

    def decode(self, words):
        """The result words (host int64 array) as projection_maps' `maps`: per projected ROI a
        dict roi, box and per axis a dict of map arrays with the plane's shape — views of
        `words`, no copy —, the means formed here on the host."""
        words = np.ascontiguousarray(words, dtype=np.int64)
        n_roi = len(self.boxes)
        assert (words[1] == n_roi and words[2] == self.axis_bits and words[3] == self.maps & 0xFFFFFFFF
                and words[4] == (self.ndim == 3) and words[6] * 8 == self.result_bytes), words[:8]
        out = []
        for r in self.rois:
            box = tuple(int(v) for v in self.boxes[r])
            ext = tuple(box[2 * a + 1] - box[2 * a] for a in range(3))
            head = words[_PROJECT_HEAD + _PROJECT_ROI * r:_PROJECT_HEAD + _PROJECT_ROI * (r + 1)]
            entry = {"roi": r, "box": box}
            for axis in self.axes:
                a = PROJECT_AXES.index(axis)
                shape = tuple(e for i, e in enumerate(ext) if i != a)
                n, off = int(head[2 * a]), int(head[2 * a + 1])
                assert n == int(np.prod(shape)) and off > 0, (r, axis, n, off)
                step, m = (n + 1) & ~1, {}
                for i, name in enumerate(self.names):
                    flat = words[off + i * step:off + i * step + n]
                    flat = flat if name in PROJECT_MAPS[:2] else flat.view(np.float64)
                    m[name] = flat.reshape(shape if self.ndim == 3 else shape[1:])
                _projection_means(m, ext[a])
                entry[axis] = m
            out.append(entry)
        return out


def _projection_means(m, length):
    """The host's part of one (ROI, axis): mean_vx, mean_vy, mean_vz, mean_magnitude = sum /
    n_valid (NaN where 0) and mean_image = sum_image / the line's length, for the sums present."""
    if "n_valid" in m:
        nv = m["n_valid"].astype(np.float64)
        nv[nv == 0] = np.nan
        for k in ("vx", "vy", "vz", "magnitude"):
            if "sum_" + k in m:
                m["mean_" + k] = m["sum_" + k] / nv
    if "sum_image" in m:
        m["mean_image"] = m["sum_image"] / float(length)


@dataclasses.dataclass
class ContractSpec:
    """The contractility of every ROI, asked of contractility / FlowStream(contract=) /
    process_flow(contract=): the centroid of the ROI's mask and, over its valid voxels, the angle
    between the flow and the direction to that centroid (plot_figure2_movie.ipynb cell 1; 0
    degrees: straight towards the centroid, 180: straight away).

    mask: "largest" — the figure's route: rel > threshold, then the largest connected component
    of every ROI's cropped mask (largest_component_mask) — or "summary": the mask the summary
    itself reduces over (the threshold mask, or its opening when the SummarySpec has min_size >= 1).
    connectivity ("largest" only): 6, 18 or 26 in 3D (default 26), 4 or 8 in 2D (default 8).
    center: "mask" — every ROI's own centroid — or (x, y, z) ((x, y) in 2D) to measure from
    instead, in each ROI's own index coordinates (the notebook's crop-local com: a centroid this
    module reports, minus the ROI's origin), the same for every ROI; e.g. an earlier frame's, to
    hold the centre still along a movie.  The mask's own centroid is reported either way.
    bins: "angle" (degrees) and / or "inward" (the physical velocity component towards the
    centre) -> ascending bin edges (at most 256 bins), np.histogram semantics."""
    mask: str = "largest"
    connectivity: int | None = None
    center: object = "mask"
    bins: dict | None = None

    def resolve(self, ndim):
        """Validated (mask, connectivity, given, nbins [2], edges [2 arrays or None]) for an
        ndim-D volume: given = None for "mask" or the 3 float64 values x y z (z = 0 in 2D);
        ValueError on a bad value."""
        if self.mask not in ("largest", "summary"):
            raise ValueError(f"contract: mask {self.mask!r} is not 'largest' or 'summary'")
        allowed = CONNECTIVITIES[ndim]
        c = allowed[-1] if self.connectivity is None else self.connectivity
        if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or c not in allowed:
            raise ValueError(f"contract: connectivity {c!r} is not one of {allowed} for a {ndim}D volume")
        if self.mask == "summary" and self.connectivity is not None:
            raise ValueError("contract: connectivity goes with mask='largest' (the summary's mask has its own)")
        given = None
        if isinstance(self.center, str):
            if self.center != "mask":
                raise ValueError(f"contract: center {self.center!r} is not 'mask' or {ndim} coordinates")
        else:
            try:
                given = np.ascontiguousarray(self.center, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError(f"contract: center {self.center!r} is not 'mask' or {ndim} coordinates") from None
            if given.shape != (ndim,):
                raise ValueError(f"contract: center must be {ndim} coordinates (x, y{', z' if ndim == 3 else ''}), "
                                 f"got shape {given.shape}")
            if not np.all(np.isfinite(given)):
                raise ValueError("contract: center must be finite")
            given = np.concatenate([given, np.zeros(3 - ndim)])
        nbins, edges = [0] * 2, [None] * 2
        for name, e in (self.bins or {}).items():
            if name not in CONTRACT_QUANTITIES:
                raise ValueError(f"contract: unknown histogram quantity {name!r} (one of {CONTRACT_QUANTITIES})")
            q = CONTRACT_QUANTITIES.index(name)
            edges[q] = SummarySpec._bin_edges(e, "contract " + name)
            nbins[q] = edges[q].size - 1
        return self.mask, int(c), given, nbins, edges


class _LargestCall(_BoxCall):
    """of3d_mask_largest bound to boxes and a device: the keep volume and the workspace,
    allocated once."""

    def __init__(self, boxes, dims, rel_f64, connectivity, device):
        import torch

        super().__init__(boxes, dims, rel_f64)
        self.connectivity = int(connectivity)
        self.ws = self._workspace(self.lib.of3d_mask_largest_workspace_bytes(self.roi_arr, len(self.boxes)), device)
        self.keep = torch.empty(self.dims, dtype=torch.uint16, device=device)

    def enqueue(self, rel, thresh_ptr, counts_ptr, stream):
        _lib.check(self.lib.of3d_mask_largest(rel, self.rel_f64, *self.dims, thresh_ptr, self.roi_arr,
                                              len(self.boxes), self.connectivity, self.keep.data_ptr(), counts_ptr,
                                              self.ws.data_ptr(), stream or None))


class _ContractCall(_BoxCall):
    """of3d_flow_contract bound to boxes and a device, with of3d_mask_largest in front of it for
    mask="largest": sizes, the workspaces and the decoding.  The result block: the contract
    words, then ("largest") of3d_mask_largest's 4 counts per box."""

    def __init__(self, boxes, dims, rel_f64, request, ndim, scales, device):
        super().__init__(boxes, dims, rel_f64, scales)
        self.mask, connectivity, self.given, nbins, edges = request.resolve(int(ndim))
        self._bind_bins(nbins, edges)
        self.given_arr = (self.given.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
                          if self.given is not None else None)
        self.ws = self._workspace(
            self.lib.of3d_flow_contract_workspace_bytes(self.roi_arr, len(self.boxes), self.nb_arr), device)
        self.contract_bytes = self.lib.of3d_flow_contract_result_bytes(len(self.boxes), self.nb_arr)
        self.largest = (_LargestCall(self.boxes, self.dims, self.rel_f64, connectivity, device)
                        if self.mask == "largest" else None)
        self.result_bytes = self.contract_bytes + (32 * len(self.boxes) if self.largest is not None else 0)

    def enqueue(self, fields, thresh_ptr, keep_ptr, result_ptr, stream):
        """("largest") the labelling and selection, then the moment, centre, reduction and final
        kernels on `stream` (device pointers); keep_ptr: the summary's mask for mask="summary"."""
        vx, vy, vz, rel, v_f32 = fields
        if self.largest is not None:
            self.largest.enqueue(rel, thresh_ptr, result_ptr + self.contract_bytes, stream)
            keep_ptr = self.largest.keep.data_ptr()
        _lib.check(self.lib.of3d_flow_contract(vx, vy, vz or None, rel, int(v_f32), self.rel_f64, *self.dims,
                                               thresh_ptr, *self.scales, self.roi_arr, len(self.boxes),
                                               keep_ptr or None, self.given_arr, self.nb_arr, self.edge_arr,
                                               result_ptr, self.ws.data_ptr(), stream or None))

    def decode(self, words):
        """The result words (host int64 array) as contractility's dict but for the threshold."""
        words = np.ascontiguousarray(words, dtype=np.int64)
        n_roi, ntot = len(self.boxes), sum(self.nbins)
        body = words[:n_roi * (_CT_HEAD + ntot)].reshape(n_roi, _CT_HEAD + ntot)
        f = lambda a, b: np.ascontiguousarray(body[:, a:b]).view(np.float64)
        origin = self.boxes[:, [4, 2, 0]].astype(np.float64)  # x y z
        out = {"rois": self.boxes.copy(), "moments": np.ascontiguousarray(body[:, :4]).view(np.uint64),
               "centroid": origin + f(4, 7), "center_used": origin + f(7, 10),
               "n_valid": body[:, 10].copy(), "n_angle": body[:, 11].copy(), "n_inward": body[:, 12].copy()}
        if self.largest is not None:
            counts = words[self.contract_bytes // 8:][:4 * n_roi].reshape(n_roi, 4)
            out["n_mask"], out["n_components"], out["n_kept"] = (counts[:, i].copy() for i in (0, 1, 3))
        else:  # no labelling of this request's own: the mask reduced over, as it came
            out["n_mask"] = out["n_kept"] = body[:, 0].copy()
            out["n_components"] = np.full(n_roi, -1, dtype=np.int64)
        sums = f(13, 17)
        na = out["n_angle"].astype(np.float64)
        na[na == 0] = np.nan  # no voxel with an angle: NaN means, no division warnings
        for i, k in enumerate(CONTRACT_SUMS):
            out[k] = sums[:, i].copy()
            out["mean_" + k[4:]] = sums[:, i] / na
        out["inward_fraction"] = out["n_inward"] / na
        out["hist"], out["edges"] = {}, {}
        _decode_hists(body, _CT_HEAD, CONTRACT_QUANTITIES, self.nbins, self.edges, np.uint64, out["hist"],
                      out["edges"])
        return out


class _SelectCall:
    """of3d_rel_select bound to a volume, one box (None: the whole volume), percentiles and a
    method: the ranks (relative to the box's voxel count) and the workspace, formed once."""

    def __init__(self, dims, rel_f64, box, percentiles, method, device):
        import torch

        self.lib, self.dims, self.rel_f64 = _lib.load(), tuple(int(v) for v in dims), int(rel_f64)
        dt = np.dtype(np.float64 if rel_f64 else np.float32)
        b = (0, self.dims[0], 0, self.dims[1], 0, self.dims[2]) if box is None else tuple(int(v) for v in box)
        self.n_box = (b[1] - b[0]) * (b[3] - b[2]) * (b[5] - b[4])
        ranks = [_percentile_ranks(self.n_box, p, dt, method) for p in percentiles]
        self.n_q = len(ranks)
        self.lo = np.array([r[0] for r in ranks], dtype=np.int64)
        self.hi = np.array([r[1] for r in ranks], dtype=np.int64)
        self.gamma = np.array([float(r[2]) for r in ranks], dtype=np.float64)
        self.box = None if box is None else np.array(b, dtype=np.int64)
        self.ws = torch.empty(self.lib.of3d_rel_select_workspace_bytes(self.rel_f64), dtype=torch.uint8,
                              device=device)

    def enqueue(self, rel, out_ptr, stream):
        """The select's kernels on `stream`: n_q elements of rel's dtype from out_ptr."""
        I, D = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)
        _lib.check(self.lib.of3d_rel_select(rel, self.rel_f64, *self.dims,
                                            self.box.ctypes.data_as(I) if self.box is not None else None, self.n_q,
                                            self.lo.ctypes.data_as(I), self.hi.ctypes.data_as(I),
                                            self.gamma.ctypes.data_as(D), out_ptr, self.ws.data_ptr(),
                                            stream or None))


class _ProfileCall(_BoxCall):
    """of3d_rel_profile bound to boxes: sizes and the decoding.  Its thresholds are the n_p
    percentiles' and then the selection box's minimum and maximum (percentiles 0 and 100 of the
    same select), so that one block holds everything the profile reports; the last two also are
    the range of the auto edges.  thresholds: the device tensor the select leaves them in (n_p + 2
    elements of rel's dtype, or more: the first n_p + 2 count) — the pass reads these, whatever
    single threshold the frame's other passes share."""

    def __init__(self, boxes, dims, rel_f64, percentiles, nbins, edges, thresholds):
        super().__init__(boxes, dims, rel_f64)
        self.percentiles, self.nbins, self.edges, self.thresholds = list(percentiles), int(nbins), edges, thresholds
        self.n_t = len(self.percentiles) + 2
        self.result_bytes = self.lib.of3d_rel_profile_result_bytes(len(self.boxes), self.n_t, self.nbins)
        if self.result_bytes == 0:
            raise ValueError("of3d: bad reliability profile sizes")

    def enqueue(self, fields, thresh_ptr, keep_ptr, result_ptr, stream):
        """The profile kernel on `stream`, of rel (fields[3]) alone, against self.thresholds."""
        thresh_ptr = self.thresholds.data_ptr()
        given = self.edges.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if self.edges is not None else None
        range_ptr = None if self.edges is not None else thresh_ptr + (self.n_t - 2) * self.thresholds.element_size()
        _lib.check(self.lib.of3d_rel_profile(fields[3], self.rel_f64, *self.dims, self.roi_arr, len(self.boxes),
                                             thresh_ptr, self.n_t, self.nbins, given, range_ptr, result_ptr,
                                             stream or None))

    def decode(self, words, summary=None):
        """The block's words (host int64) as reliability_profile's dict (also summary["rel_profile"])."""
        words = np.ascontiguousarray(words, dtype=np.int64)
        n_roi, n_p, nb = len(self.boxes), self.n_t - 2, self.nbins
        assert tuple(words[:3]) == (n_roi, self.n_t, nb), words[:3]
        rel_dt = np.dtype(np.float64 if self.rel_f64 else np.float32)
        thr = words[3:3 + self.n_t].view(np.float64).astype(rel_dt)  # exact: they were rel_dt values
        head = 3 + self.n_t + nb + 1
        rw = 2 + self.n_t + nb
        body = words[head:head + n_roi * rw].reshape(n_roi, rw)
        out = {"percentiles": np.array(self.percentiles, dtype=np.float64), "thresholds": thr[:n_p].copy(),
               "min": thr[n_p], "max": thr[n_p + 1], "rois": self.boxes.copy(),
               "n_voxels": body[:, 0].copy(), "n_nan": body[:, 1].copy(), "n_above": body[:, 2:2 + n_p].copy(),
               "hist": np.ascontiguousarray(body[:, 2 + self.n_t:]).view(np.uint64),
               "edges": words[3 + self.n_t:head].view(np.float64).copy()}
        out["fraction_above"] = out["n_above"] / out["n_voxels"][:, None].astype(np.float64)
        if summary is not None:
            summary["rel_profile"] = out
        return out


def _pair_options(floor, combine):
    """Validated (floor, combine code) of the joint mask; ValueError on a bad value."""
    if not isinstance(combine, str) or combine not in COMBINE:
        raise ValueError(f"summary: combine {combine!r} is not one of {tuple(COMBINE)}")
    try:
        floor = float(floor)
    except (TypeError, ValueError):
        raise ValueError(f"summary: floor {floor!r} is not a number") from None
    if np.isnan(floor):
        raise ValueError("summary: floor must not be NaN (-inf switches the clause off)")
    return floor, COMBINE[combine]


def _pair_spec(shape, rel_percentile, rois, min_size, connectivity, percentile_box=None, percentile_method="linear"):
    """(boxes, dims, min_size, connectivity) of a two-channel call, validated by SummarySpec."""
    spec = SummarySpec(rois=rois, rel_percentile=rel_percentile, min_size=min_size, connectivity=connectivity,
                       percentile_box=percentile_box, percentile_method=percentile_method)
    boxes = spec.resolve(shape)[0]
    min_size, connectivity = spec.opening(len(shape))
    if min_size < 1:
        raise ValueError("summary: the joint mask needs min_size >= 1 (1: no opening)")
    return boxes, _dims(tuple(int(v) for v in shape)), min_size, connectivity


class _PairCall(_BoxCall):
    """The two-channel comparison of one frame bound to boxes and a device: two of3d_quantile
    (with a percentile_box or another percentile_method: two of3d_rel_select),
    of3d_mask_open_pair, then of3d_flow_pair.  Holds the boxes, sizes, workspaces, the keep volume
    and the result tensor: of3d_flow_pair's words, then the opening's 4 counts per box, then the
    two thresholds (one word each, in rel's dtype) — one small download."""

    def __init__(self, shape, rel_dtype, device, rel_percentile=90, xyscale=1.0, zscale=1.0, tscale=1.0, rois=None,
                 bins=None, floor=0.0, combine="or", min_size=1, connectivity=None, percentile_box=None,
                 percentile_method="linear"):
        import torch

        boxes, dims, min_size, connectivity = _pair_spec(shape, rel_percentile, rois, min_size, connectivity,
                                                         percentile_box, percentile_method)
        self.floor, self.combine = _pair_options(floor, combine)
        super().__init__(boxes, dims, rel_dtype == torch.float64, (xyscale, zscale, tscale))
        self._bind_bins(*SummarySpec._quantity_bins(bins, len(shape), "pair ", PAIR_QUANTITIES))
        lib = self.lib
        self.rel_dt = np.dtype(np.float64 if self.rel_f64 else np.float32)
        self.open = _OpenCall(self.boxes, self.dims, self.rel_f64, min_size, connectivity, device)
        self.ws = self._workspace(lib.of3d_flow_pair_workspace_bytes(self.roi_arr, len(self.boxes), self.nb_arr),
                                  device)
        self.qws = torch.empty(lib.of3d_quantile_workspace_bytes(self.rel_f64), dtype=torch.uint8, device=device)
        self.pair_bytes = lib.of3d_flow_pair_result_bytes(len(self.boxes), self.nb_arr)
        self.counts_off = self.pair_bytes
        self.thresh_off = self.counts_off + 32 * len(self.boxes)
        # zeros for the padding beside float32 thresholds (every other byte is written per call);
        # a blocking upload, so that no fill is pending on another stream than enqueue's
        self.result = torch.zeros((self.thresh_off + 16) // 8, dtype=torch.int64).to(device)
        self.n = int(np.prod(self.dims))
        self.ranks = _linear_ranks(self.n, rel_percentile, self.rel_dt)
        # a crop or MATLAB's definition: each channel's own percentile over the same box, in place
        self.select = None
        if percentile_box is not None or percentile_method != "linear":
            box = SummarySpec(percentile_box=percentile_box).threshold_request(shape)[0]
            self.select = _SelectCall(self.dims, self.rel_f64, box, [float(rel_percentile)], percentile_method, device)

    @property
    def keep(self):
        """The joint mask's keep volume (uint16, bit r: box r), as the last enqueue left it."""
        return self.open.keep

    def enqueue(self, ptrs0, ptrs1, v_f32, stream):
        """Both channels' quantiles, the joint opening and the pair pass on `stream`.  ptrs0 /
        ptrs1: device pointers (vx, vy, vz or None, rel) of the channels; vz None in both: the
        in-plane mode.  Returns the result tensor (decode its host copy)."""
        lo, hi, gamma = self.ranks
        lib, res = self.lib, self.result.data_ptr()
        t0, t1 = res + self.thresh_off, res + self.thresh_off + 8
        for rel, t in ((ptrs0[3], t0), (ptrs1[3], t1)):
            if self.select is not None:
                self.select.enqueue(rel, t, stream)
                continue
            _lib.check(lib.of3d_quantile(rel, self.rel_f64, self.n, lo, hi, float(gamma), t, self.qws.data_ptr(),
                                         stream or None))
        self.open.enqueue_pair(ptrs0[3], t0, ptrs1[3], t1, self.floor, self.combine, res + self.counts_off, stream)
        _lib.check(lib.of3d_flow_pair(ptrs0[0], ptrs0[1], ptrs0[2] or None, ptrs1[0], ptrs1[1], ptrs1[2] or None,
                                      int(v_f32), *self.dims, *self.scales, self.roi_arr, len(self.boxes),
                                      self.open.keep.data_ptr(), self.nb_arr, self.edge_arr, res, self.ws.data_ptr(),
                                      stream or None))
        return self.result

    def decode(self, words):
        """The result words (host int64 array) as channel_compare's dict."""
        words = np.ascontiguousarray(words, dtype=np.int64)
        n_roi, ntot = len(self.boxes), sum(self.nbins)
        body = words[:n_roi * (_PAIR_HEAD + ntot)].reshape(n_roi, _PAIR_HEAD + ntot)
        th = words[self.thresh_off // 8:self.thresh_off // 8 + 2]
        out = {"rois": self.boxes.copy(), "thresholds": np.array([th[i:i + 1].view(self.rel_dt)[0] for i in (0, 1)]),
               "n_valid": body[:, 0].copy(), "n_voxels": body[:, 1].copy()}
        _decode_open_counts(words[self.counts_off // 8:], n_roi, out)
        sums = np.ascontiguousarray(body[:, 2:_PAIR_HEAD]).view(np.float64)
        nv = out["n_valid"].astype(np.float64)
        nv[nv == 0] = np.nan  # empty box: NaN means, no division warnings
        for c in (0, 1):
            ch = {k: sums[:, 8 * c + i].copy() for i, k in enumerate(SUMS)}
            ch["mean_magnitude"] = ch["sum_magnitude"] / nv
            ch["theta_mean"] = np.arctan2(ch["sum_sin"] / nv, ch["sum_cos"] / nv)
            ch["theta_mean_weighted"] = np.arctan2(ch["sum_mag_sin"] / nv, ch["sum_mag_cos"] / nv)
            out[f"ch{c}"] = ch
        for i, k in enumerate(PAIR_SUMS):
            out[k] = sums[:, 16 + i].copy()
        out["mean_dot"] = out["sum_dot"] / nv
        out["mean_cosine"] = out["sum_cosine"] / nv
        out["dtheta_mean"] = np.arctan2(out["sum_sin_dtheta"] / nv, out["sum_cos_dtheta"] / nv)
        out["mean_diff"] = out["sum_diff"] / nv
        # Pearson's r of the two magnitudes from the five magnitude sums
        s0, s1 = out["ch0"]["sum_magnitude"], out["ch1"]["sum_magnitude"]
        cov = nv * out["sum_mag0_mag1"] - s0 * s1
        var = (nv * out["sum_mag0_sq"] - s0 * s0) * (nv * out["sum_mag1_sq"] - s1 * s1)
        with np.errstate(invalid="ignore", divide="ignore"):
            out["magnitude_correlation"] = cov / np.sqrt(np.where(var > 0, var, np.nan))
        out["hist"], out["edges"] = {}, {}
        _decode_hists(body, _PAIR_HEAD, PAIR_QUANTITIES, self.nbins, self.edges, np.uint64, out["hist"], out["edges"])
        return out


class _SummaryCall(_BoxCall):
    """One resolved spec bound to a device: sizes, workspaces and the kernel launches, as two
    ordered lists of (name, call, where its result goes).

    parts — what shares the summary's result block, (name, call, byte offset), in the block's
    order: "summary" (this call's own words, offset 0, no call of their own), "open" (min_size >= 1: of3d_mask_open's
    counts), "axes", "whist", "spread", "profile" (each with its request in the spec).  One
    download brings all of them.

    addons — what follows into a result block of its own, (name, call, None), in launch order:
    "quiver" (a QuiverSpec: of3d_quiver_sample), "contract" (a ContractSpec: of3d_flow_contract;
    the quiver keeps the summary's mask whatever the contract's), "project" (a ProjectionSpec:
    of3d_flow_project; its image is bound per frame, call.project.bind_image) and "export" (a FieldSpec:
    of3d_field_export, last; v_f32: whether the velocity fields it will be given are float32 —
    its block is sized at construction).  All take the summary's boxes, threshold and opened
    mask; enqueue's `blocks` names a device block for each.  In a FlowStream the export's block
    alone travels on the fields' download path, the others are copied behind the summary's words.

    A part or add-on is read by name — call.open, call.spread, call.quiver, ... (None without
    it) — and a part's offset as call.spread_off, ...  The next pass is one more line in
    __init__: part(...) or an entry of `addons`."""

    def __init__(self, spec, shape, rel_dtype, device, quiver=None, contract=None, export=None, v_f32=False,
                 project=None):
        import torch

        self.spec, self.shape = spec, tuple(int(v) for v in shape)
        ndim = len(self.shape)
        boxes, nbins, edges = spec.resolve(shape)
        for request, args in ((quiver, (ndim,)), (contract, (ndim,)), (export, (ndim, len(boxes))),
                              (project, (ndim, len(boxes)))):
            if request is not None:
                request.resolve(*args)  # a bad request fails before anything is allocated
        min_size, connectivity = spec.opening(ndim)
        super().__init__(boxes, _dims(self.shape), rel_dtype == torch.float64,
                         (spec.xyscale, spec.zscale, spec.tscale))
        self._bind_bins(nbins, edges)
        lib, bound, scales = self.lib, (self.boxes, self.dims, self.rel_f64), self.scales
        self.parts, self.result_bytes = [], 0

        def part(name, call, nbytes):
            self.parts.append((name, call, self.result_bytes))
            self.result_bytes += nbytes

        part("summary", None, lib.of3d_flow_summary_result_bytes(len(self.boxes), self.nb_arr))  # this call's own
        if min_size:
            opening = _OpenCall(*bound, min_size, connectivity, device)
            part("open", opening, opening.result_bytes)
        self.keep_ptr = opening.keep.data_ptr() if min_size else None
        self.followers = len(self.parts)  # the parts from here on follow the summary's kernel
        request = spec.axes_request(ndim)
        if request is not None:
            call = _AxesCall(*bound, request, spec.axes_physical, scales, device)
            part("axes", call, call.result_bytes)
        wnbins, wedges = spec.weighted(ndim)
        if any(wnbins):
            call = _WhistCall(*bound, wnbins, wedges, scales, device)
            part("whist", call, call.result_bytes)
        request = spec.spread_request(ndim)
        if request is not None:
            call = _SpreadCall(*bound, request[0], ndim, scales, device, self.nb_arr, self.result_bytes)
            part("spread", call, call.result_bytes)
        self.ws = torch.empty(lib.of3d_flow_summary_workspace_bytes(), dtype=torch.uint8, device=device)
        self.qws = torch.empty(lib.of3d_quantile_workspace_bytes(self.rel_f64), dtype=torch.uint8, device=device)
        self.thresh = torch.empty(1, dtype=rel_dtype, device=device)
        self.n = int(np.prod(self.dims))
        self.ranks = _linear_ranks(self.n, spec.rel_percentile, _np_dtype(self.thresh))
        self.thresh_ptr = self.thresh.data_ptr()
        # a crop, MATLAB's definition or a profile: one of3d_rel_select for the profile's
        # percentiles, the box's minimum and maximum and the summary's own percentile; then
        # (rel_profile) of3d_rel_profile's block after the spread's
        box, method, profile = spec.threshold_request(self.shape)
        self.select = None
        if box is not None or method != "linear" or profile is not None:
            own = float(spec.rel_percentile)
            sel = (list(profile[0]) + [0.0, 100.0]) if profile is not None else []
            if own not in sel[:-2]:
                sel.append(own)
            if len(sel) > SELECT_MAX:
                raise ValueError(f"summary: rel_percentile, the rel_profile percentiles and the extremes are "
                                 f"{len(sel)} percentiles, one select takes {SELECT_MAX}: name rel_percentile among "
                                 "the profile's")
            self.select = _SelectCall(self.dims, self.rel_f64, box, sel, method, device)
            self.thresh = torch.empty(len(sel), dtype=rel_dtype, device=device)
            self.thresh_ptr = self.thresh.data_ptr() + sel.index(own) * self.thresh.element_size()
            if profile is not None:
                call = _ProfileCall(*bound, *profile, self.thresh)
                part("profile", call, call.result_bytes)
        self.addons = []
        if quiver is not None:
            self.addons.append(("quiver", _QuiverCall(*bound, quiver, ndim, scales, device), None))
        if contract is not None:
            self.addons.append(("contract", _ContractCall(*bound, contract, ndim, scales, device), None))
        if project is not None:
            self.addons.append(("project", _ProjectCall(*bound, project, ndim, scales), None))
        if export is not None:
            self.addons.append(("export", _ExportCall(*bound, v_f32, export, ndim, scales), None))

    def __getattr__(self, name):
        """call.<name> of a part or add-on (None without it), call.<name>_off of a part."""
        listed = {n: (call, off) for n, call, off in self.__dict__.get("parts", []) + self.__dict__.get("addons", [])}
        if name in ("open", "axes", "whist", "spread", "profile", "quiver", "contract", "project", "export"):
            return listed.get(name, (None, None))[0]
        if name.endswith("_off") and name[:-4] in listed:
            return listed[name[:-4]][1]
        raise AttributeError(name)

    def enqueue(self, fields, result_ptr, stream, blocks=None):
        """Quantile + summary kernels on `stream`, then the other parts' and the add-ons' — fields:
        (vx, vy, vz, rel, v_f32), device pointers (vz 0/None for 2D) and whether the velocities are
        float32; blocks: add-on name -> device pointer of its result block, for exactly the
        add-ons that were requested."""
        blocks = blocks or {}
        if set(blocks) != {name for name, _, _ in self.addons}:
            raise ValueError(f"summary: result blocks for {sorted(blocks)}, but the requests are "
                             f"{[name for name, _, _ in self.addons]}")
        vx, vy, vz, rel, v_f32 = fields
        lo, hi, gamma = self.ranks
        lib, thresh_ptr, keep_ptr = self.lib, self.thresh_ptr, self.keep_ptr
        if self.select is None:
            _lib.check(lib.of3d_quantile(rel, self.rel_f64, self.n, lo, hi, float(gamma), thresh_ptr,
                                         self.qws.data_ptr(), stream or None))
        else:
            self.select.enqueue(rel, self.thresh.data_ptr(), stream)
        args = (vx, vy, vz or None, rel, int(v_f32), self.rel_f64, *self.dims, thresh_ptr, *self.scales,
                self.roi_arr, len(self.boxes), self.nb_arr, self.edge_arr, result_ptr, self.ws.data_ptr(),
                stream or None)
        if keep_ptr is None:
            _lib.check(lib.of3d_flow_summary(*args))
        else:
            _, opening, off = self.parts[1]
            opening.enqueue(rel, thresh_ptr, result_ptr + off, stream)
            _lib.check(lib.of3d_flow_summary_masked(*args, keep_ptr))
        for _, call, off in self.parts[self.followers:]:
            call.enqueue(fields, thresh_ptr, keep_ptr, result_ptr + off, stream)
        for name, call, _ in self.addons:
            call.enqueue(fields, thresh_ptr, keep_ptr, blocks[name], stream)

    def decode(self, words):
        """The result words (host int64 array) as flow_summary's dict."""
        words = np.ascontiguousarray(words, dtype=np.int64)
        n_roi, ntot = len(self.boxes), sum(self.nbins)
        body = words[_HEAD:_HEAD + n_roi * (_ROI_HEAD + ntot)].reshape(n_roi, _ROI_HEAD + ntot)
        out = {"threshold": _word_threshold(words, self.rel_f64), "rois": self.boxes.copy(),
               "n_valid": body[:, 0].copy(), "n_voxels": body[:, 1].copy()}
        sums = np.ascontiguousarray(body[:, 2:_ROI_HEAD]).view(np.float64)
        for i, k in enumerate(SUMS):
            out[k] = sums[:, i].copy()
        nv = out["n_valid"].astype(np.float64)
        nv[nv == 0] = np.nan  # empty box: NaN means, no division warnings
        out["mean_magnitude"] = out["sum_magnitude"] / nv
        for k in ("vx", "vy", "vz"):
            out["mean_" + k] = out["sum_" + k] / nv
        out["theta_mean"] = np.arctan2(out["sum_sin"] / nv, out["sum_cos"] / nv)
        out["theta_mean_weighted"] = np.arctan2(out["sum_mag_sin"] / nv, out["sum_mag_cos"] / nv)
        out["hist"], out["edges"] = {}, {}
        _decode_hists(body, _ROI_HEAD, QUANTITIES, self.nbins, self.edges, np.uint64, out["hist"], out["edges"])
        for _, call, off in self.parts[1:]:
            call.decode(words[off // 8:], out)
        return out


class _Frame:
    """The inputs of one public entry — (vx, vy, vz or None, rel), or rel alone (vx None) — and
    the only place that knows how they become device state.

    The constructor validates what the host objects show (a TypeError for the dtypes, a
    ValueError for the dimensions against vz; `name`, the entry's, is what the messages say) and
    settles host (numpy input: results come back as numpy), dev (numpy: the default or given
    device; tensors: their own), shape, ndim, dims (nz, ny, nx), rel_dtype (torch), rel_f64 and
    v_f32 — enough to validate the entry's other arguments and to bind its _*Call objects before
    anything is uploaded.  ``with frame:`` then uploads (numpy) or makes contiguous (tensors) the
    fields, enters the device and holds tx, ty, tz, tr, `fields` (the passes' (vx, vy, vz, rel,
    v_f32) of device pointers, None for an absent field) and `stream`, the current stream."""

    def __init__(self, name, vx, vy, vz, rel, device, check=True):
        import torch

        self.inputs, first = (vx, vy, vz, rel), rel if vx is None else vx
        self.host = isinstance(rel, np.ndarray)
        if check and vx is None and _dtype_name(rel) not in ("float32", "float64"):
            raise TypeError("rel must be float32 or float64")
        if check and vx is not None and not {_dtype_name(vx), _dtype_name(rel)} <= {"float32", "float64"}:
            raise TypeError("vx/vy/vz must be float64 or float32, rel float32 or float64")
        self.shape = shape = tuple(int(v) for v in first.shape)
        if check and vx is None and len(shape) not in (2, 3):
            raise ValueError(f"{name} needs a (nz, ny, nx) or (ny, nx) field")
        if check and vx is not None and len(shape) != (3 if vz is not None else 2):
            raise ValueError(f"{name} needs (nz, ny, nx) fields with vz, (ny, nx) fields without")
        self.dev = _cuda_device(device) if self.host else first.device
        self.ndim, self.dims = len(shape), _dims(shape)
        self.rel_dtype = getattr(torch, _dtype_name(rel))
        self.rel_f64, self.v_f32 = self.rel_dtype == torch.float64, vx is not None and _dtype_name(vx) == "float32"

    def __enter__(self):
        import torch

        self.tx, self.ty, self.tz, self.tr = t = [_to_device(a, self.host, self.dev) for a in self.inputs]
        self.fields = tuple(a.data_ptr() if a is not None else None for a in t) + (self.v_f32,)
        self.device_guard = torch.cuda.device(self.dev)
        self.device_guard.__enter__()
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream
        return self

    def __exit__(self, *exc):
        return self.device_guard.__exit__(*exc)

    def threshold(self, rel_percentile, threshold=None, percentile_box=None, percentile_method="linear"):
        """The entry's threshold as a 1-element device tensor of rel's dtype: `threshold` if
        given, else the percentile, selected on the device (_thresholds_device)."""
        return _thresholds_device([self.tr], rel_percentile, None if threshold is None else [threshold],
                                  percentile_box, percentile_method)

    def threshold_value(self, thresh):
        """That tensor's value as a numpy scalar of rel's dtype (a synchronising download)."""
        return _np_dtype(self.tr).type(thresh.cpu().numpy()[0])

    def open_mask(self, boxes, min_size, connectivity, thresh, counts_ptr=None):
        """The optional opening ahead of a pass: with min_size >= 1 an _OpenCall over `boxes`,
        enqueued on the stream (its counts at counts_ptr, or in a tensor of its own); returns the
        keep volume's device pointer, None without an opening."""
        import torch

        if not min_size:
            return None
        self.opening = _OpenCall(boxes, self.dims, self.rel_f64, min_size, connectivity, self.dev)
        if counts_ptr is None:
            self.counts = torch.empty((len(boxes), 4), dtype=torch.int64, device=self.dev)
            counts_ptr = self.counts.data_ptr()
        self.opening.enqueue(self.fields[3], thresh.data_ptr(), counts_ptr, self.stream)
        return self.opening.keep.data_ptr()


def _thresholds_device(rels, rel_percentile, given, percentile_box=None, percentile_method="linear"):
    """One threshold per rel field as a tensor of their dtype on their device: the `given` values,
    or each field's rel_percentile-th percentile selected on the device (nothing goes to the
    host) — of the whole field by of3d_quantile, or with a percentile_box / another
    percentile_method of that box of each field by of3d_rel_select."""
    import torch

    t = rels[0]
    box, method, _ = SummarySpec(percentile_box=percentile_box,
                                 percentile_method=percentile_method).threshold_request(tuple(t.shape))
    if given is not None:
        return torch.tensor([float(v) for v in given], dtype=t.dtype).to(t.device)
    thresh = torch.empty(len(rels), dtype=t.dtype, device=t.device)
    for i, r in enumerate(rels):
        if box is None and method == "linear":
            percentile_threshold_device(r, rel_percentile, out=thresh[i:i + 1])
        else:
            reliability_thresholds(r, [rel_percentile], box=percentile_box, method=method, out=thresh[i:i + 1])
    return thresh


def reliability_thresholds(rel, percentiles, box=None, method="linear", out=None):
    """Percentiles of one box of rel as a tensor of len(percentiles) values of rel's dtype on rel's
    device: the figure scripts' ``prctile(relCrop(:), relPer)`` of the cropped reliability
    (plot_figure5.m:80-84, plot_figure3_ROIfigures.m:70-84) by of3d_rel_select — the volume is read
    in place, all percentiles in one select, on the current stream with no synchronisation, so
    every element is ready as a threshold for the next kernel on that stream.

    rel: a float32 or float64 CUDA tensor, (nz, ny, nx) or (ny, nx).  percentiles: 1 to 8 values in
    [0, 100], in any order (0 and 100 are the box's exact minimum and maximum).  box:
    (z0, z1, y0, y1, x0, x1), or (y0, y1, x0, x1) in 2D, half-open; None: the whole volume.
    method: "linear" (np.percentile's default) or "hazen" — np.percentile(..., method='hazen'),
    which is MATLAB's prctile.  Each value equals ``np.percentile(crop, p, method=method)`` bit for
    bit (-0.0 counts as +0.0); a NaN inside the box makes every value NaN, one outside is ignored."""
    import torch

    if not isinstance(rel, torch.Tensor) or not rel.is_cuda or rel.dtype not in (torch.float32, torch.float64):
        raise TypeError("rel must be a float32 or float64 CUDA tensor")
    if rel.dim() not in (2, 3) or rel.numel() == 0:
        raise ValueError("reliability_thresholds needs a non-empty (nz, ny, nx) or (ny, nx) field")
    ps = _check_percentiles(percentiles, "percentiles")
    shape = tuple(rel.shape)
    b, method, _ = SummarySpec(percentile_box=box, percentile_method=method).threshold_request(shape)
    tr = rel.contiguous()
    if out is None:
        out = torch.empty(len(ps), dtype=tr.dtype, device=tr.device)
    elif (out.dtype != tr.dtype or out.device != tr.device or out.numel() != len(ps) or out.dim() != 1
          or not out.is_contiguous()):
        raise ValueError("out must be len(percentiles) contiguous elements of rel's dtype on rel's device")
    call = _SelectCall(_dims(shape), tr.dtype == torch.float64, b, ps, method, tr.device)
    call.enqueue(tr.data_ptr(), out.data_ptr(), torch.cuda.current_stream(tr.device).cuda_stream)
    return out


def reliability_profile(rel, percentiles=(85, 90, 95), box=None, method="linear", rois=None, bins=50, edges=None,
                        device=None):
    """What one needs to choose the reliability percentile (plot_figureS3_reliability.ipynb cells
    4-8), reduced on the device: one select of `percentiles` plus 0 and 100 over `box`
    (reliability_thresholds), then per ROI the voxels above each threshold and the histogram of rel
    (of3d_rel_profile); one small download.

    rel: numpy array or torch tensor, (nz, ny, nx) or (ny, nx), float32 or float64.  percentiles:
    1 to 6 values; box and method as reliability_thresholds (the selection box; None: the whole
    volume); rois as flow_summary (ROI 0 is the whole volume).  bins: the histogram's number of
    equal bins (1 to 256) between the selection box's minimum and maximum,
    ``np.histogram(rel.astype(float64), bins=np.linspace(float(min), float(max), bins + 1))`` — a
    ROI's values outside that range are dropped, as np.histogram's `range` drops them; min == max
    widens to min - 0.5, max + 0.5; a NaN or infinite min / max (a NaN in the selection box, an
    infinite value) gives NaN edges and all-zero counts where numpy would raise.  edges: ascending
    edges to use instead of `bins`.
    Returns a dict of numpy values: percentiles, thresholds (rel's dtype), min and max of the
    selection box, rois, per ROI n_voxels, n_nan, n_above (n_roi, n_percentiles: the voxels with
    rel > threshold, compared in rel's dtype), fraction_above = n_above / n_voxels, hist
    (n_roi, nbins) uint64 and edges (nbins + 1, float64).  Integer counts only: the same inputs
    give the same bits on every run."""
    import torch

    shape = tuple(int(v) for v in rel.shape)
    spec = SummarySpec(rois=rois, percentile_box=box, percentile_method=method,
                       rel_profile=RelProfileSpec(percentiles=tuple(percentiles), bins=bins, edges=edges))
    boxes = spec.resolve(shape)[0]  # its message for a field that is not 2D or 3D, ahead of the frame's
    b, method, profile = spec.threshold_request(shape)
    f = _Frame("reliability_profile", None, None, None, rel, device)
    select = _SelectCall(f.dims, f.rel_f64, b, list(profile[0]) + [0.0, 100.0], method, f.dev)
    thresh = torch.empty(select.n_q, dtype=f.rel_dtype, device=f.dev)
    call = _ProfileCall(boxes, f.dims, f.rel_f64, *profile, thresh)
    with f:
        res = call.new_result(f.dev)
        select.enqueue(f.fields[3], thresh.data_ptr(), f.stream)
        call.enqueue(f.fields, None, None, res.data_ptr(), f.stream)
        return call.decode(res.cpu().numpy())


def _mask_dict(keep, host, boxes, counts):
    """reliability_mask's dict but for the threshold(s): keep (numpy for host input), mask, rois
    and the opening's counts per ROI (counts: the device tensor (n_roi, 4))."""
    import torch

    k = keep.cpu().numpy() if host else keep
    out = {"keep": k, "rois": boxes.copy()}
    if host:
        out["mask"] = lambda r: ((k >> np.uint16(r)) & np.uint16(1)).astype(bool)
    else:
        out["mask"] = lambda r: ((k.view(torch.int16) >> r) & 1).bool()  # uint16 has no shifts in torch
    _decode_open_counts(counts.cpu().numpy().reshape(-1), len(boxes), out)
    return out


def _mask_entry(f, call, boxes, thresh):
    """reliability_mask's / largest_component_mask's launch and dict: call (an _OpenCall or a
    _LargestCall over boxes) on the entered frame f at the device threshold thresh."""
    import torch

    counts = torch.empty((len(boxes), 4), dtype=torch.int64, device=f.dev)
    call.enqueue(f.fields[3], thresh.data_ptr(), counts.data_ptr(), f.stream)
    out = _mask_dict(call.keep.view(f.tr.shape), f.host, boxes, counts)
    out["threshold"] = f.threshold_value(thresh)
    return out


def reliability_mask(rel, rel_percentile=90, threshold=None, min_size=1, connectivity=None, rois=None, device=None,
                     percentile_box=None, percentile_method="linear"):
    """The opened reliability mask of one frame, per ROI: MATLAB's
    ``bwareaopen(rel > relThresh, min_size, connectivity)`` of the reference's figure scripts
    (plot_figure5.m:87-88; principal_axes gives the regionprops3 step that follows it there) on
    the device (of3d_mask_open).

    rel: numpy array or torch tensor, (nz, ny, nx) or (ny, nx), float32 or float64.  The
    threshold is the rel_percentile-th percentile of rel (selected on the device) unless
    `threshold` (a Python float, used as one element of rel's dtype) is given.  min_size >= 1;
    connectivity 6 / 18 / 26 in 3D (default 26), 4 / 8 in 2D (default 8).  ROI 0 is the whole
    volume, `rois` follow (SummarySpec's boxes); each box's mask is cropped first, then opened.
    Returns a dict: keep (uint16, rel's shape; bit r set where the voxel lies in box r and in a
    component of at least min_size voxels of that box's mask; a torch tensor, numpy for numpy
    input), mask (r -> that bit plane as bool), rois, threshold and per ROI n_mask,
    n_components, n_components_kept, n_kept (int64).
    percentile_box, percentile_method (see SummarySpec): the percentile of that one box of rel,
    read in place, by "linear" or "hazen" (MATLAB's prctile) — plot_figure5.m:80-84's
    ``prctile(relCrop(:), relPer)`` (of3d_rel_select); the default is the whole field, "linear"."""
    f = _Frame("reliability_mask", None, None, None, rel, device)
    spec = SummarySpec(rois=rois, rel_percentile=rel_percentile, min_size=min_size, connectivity=connectivity)
    boxes = spec.resolve(f.shape)[0]
    min_size, connectivity = spec.opening(f.ndim)
    if min_size < 1:
        raise ValueError("summary: reliability_mask needs min_size >= 1")
    call = _OpenCall(boxes, f.dims, f.rel_f64, min_size, connectivity, f.dev)
    with f:
        return _mask_entry(f, call, boxes, f.threshold(rel_percentile, threshold, percentile_box, percentile_method))


def _frame_pair(what, ch0, ch1, device):
    """The frames of two channels ((vx, vy, vz or None, rel) each; rel alone: vx None) whose rel
    fields are of one kind, dtype and shape, on one device; `what`'s own TypeError / ValueError
    otherwise, before anything reaches the device.  The velocities are the caller's to check."""
    rel0, rel1 = ch0[3], ch1[3]
    host = isinstance(rel0, np.ndarray)
    if host != isinstance(rel1, np.ndarray):
        raise TypeError(f"{what}: both channels must be numpy arrays or both torch tensors")
    names = {_dtype_name(a) for a in (rel0, rel1)}
    if len(names) != 1 or not names <= {"float32", "float64"}:
        raise TypeError(f"{what}: both rel fields must be float32, or both float64")
    if tuple(rel0.shape) != tuple(rel1.shape) or len(rel0.shape) not in (2, 3):
        raise ValueError(f"{what}: the rel fields must share one (nz, ny, nx) or (ny, nx) shape, got "
                         f"{tuple(rel0.shape)} and {tuple(rel1.shape)}")
    f0, f1 = _Frame(what, *ch0, device, check=False), _Frame(what, *ch1, device, check=False)
    f1.dev = f0.dev
    return f0, f1


def joint_reliability_mask(rel0, rel1, rel_percentile=90, thresholds=None, floor=0.0, combine="or", min_size=1,
                           connectivity=None, rois=None, device=None, percentile_box=None,
                           percentile_method="linear"):
    """The opened JOINT reliability mask of two channels of one frame, per ROI: figure 3's
    ``relMask = (rel > prctile(rel(:),relPer)) | (rel1 > prctile(rel1(:),relPer)); relMask =
    relMask & (rel > 0) & (rel1 > 0); relMask = bwareaopen(relMask, 10^5)``
    (plot_figure3_ROIfigures.m:93-96) on the device (of3d_mask_open_pair).

    rel0, rel1: numpy arrays or CUDA tensors of one shape and dtype.  Each channel's threshold is
    its own rel_percentile-th percentile (percentile_threshold_device; nothing goes to the host
    before the counts) unless `thresholds` (two Python floats) is given.  floor: both fields must
    exceed it (the scripts' 0; -inf switches the clause off); combine: "or" (the scripts') or
    "and" of the two threshold tests.  A NaN in a field fails there; it also makes that channel's
    percentile NaN, whose test then fails everywhere.  min_size, connectivity, rois and the
    returned dict as reliability_mask, with `thresholds` (2 values of rel's dtype) in place of
    `threshold`.  keep has reliability_mask's format: it feeds the same consumers.
    percentile_box, percentile_method as reliability_mask: each channel's own percentile over the
    same box (plot_figure3_ROIfigures.m:70-84)."""
    import torch

    f0, f1 = _frame_pair("joint_reliability_mask", (None, None, None, rel0), (None, None, None, rel1), device)
    boxes, dims, min_size, connectivity = _pair_spec(f0.shape, rel_percentile, rois, min_size, connectivity,
                                                     percentile_box, percentile_method)
    floor, combine = _pair_options(floor, combine)
    if thresholds is not None and len(thresholds) != 2:
        raise ValueError("joint_reliability_mask: thresholds must be two values, one per channel")
    call = _OpenCall(boxes, dims, f0.rel_f64, min_size, connectivity, f0.dev)
    with f0, f1:
        thresh = _thresholds_device([f0.tr, f1.tr], rel_percentile, thresholds, percentile_box, percentile_method)
        counts = torch.empty((len(boxes), 4), dtype=torch.int64, device=f0.dev)
        esz = thresh.element_size()
        call.enqueue_pair(f0.fields[3], thresh.data_ptr(), f1.fields[3], thresh.data_ptr() + esz, floor, combine,
                          counts.data_ptr(), f0.stream)
        out = _mask_dict(call.keep.view(f0.tr.shape), f0.host, boxes, counts)
        out["thresholds"] = thresh.cpu().numpy().astype(_np_dtype(f0.tr))
    return out


def channel_compare(ch0, ch1, rel_percentile=90, xyscale=1.0, zscale=1.0, tscale=1.0, rois=None, bins=None, floor=0.0,
                    combine="or", min_size=1, connectivity=None, in_plane=False, device=None, percentile_box=None,
                    percentile_method="linear"):
    """Two channels' flows of one frame compared over the same voxels, reduced on the device to
    a few kilobytes (one small device->host copy): figure 3 of the reference
    (plot_figure3_ROIfigures.m:67-193, plot_figure3_ChannelCompare.m:111-164).

    ch0, ch1: (vx, vy, vz or None, rel) of each channel, numpy arrays or CUDA tensors; all six
    velocity fields share one dtype (float64 / float32) and the fields one shape, both rel one
    dtype.  The mask is joint_reliability_mask's (rel_percentile per channel, floor, combine,
    min_size, connectivity, rois); a voxel is valid when it is kept and both channels' magnitudes
    are not NaN, so both channels are averaged over the same voxels.  in_plane: ignore vz
    (magnitude = sqrt(vx^2 + vy^2), as the figure's scripts on their 3-slice volumes); 2D fields
    are in-plane by nature.  bins: "dot" | "cosine" | "dtheta" | "dmagnitude" -> ascending edges
    (np.histogram semantics, at most 256 bins).  The cosine is not clamped: rounding may leave it
    a few ulp past +-1, outside edges that end exactly there.
    Returns a dict of numpy values: rois, thresholds (2), per ROI n_valid, n_voxels, n_mask,
    n_components, n_components_kept, n_kept; ch0 and ch1, each a dict of flow_summary's eight
    sums (sum_magnitude .. sum_mag_cos) with mean_magnitude, theta_mean, theta_mean_weighted (the
    scripts' ch0_theta / ch0_thetaW); the cross sums sum_dot, sum_cosine, sum_mag0_mag1,
    sum_mag0_sq, sum_mag1_sq, sum_sin_dtheta, sum_cos_dtheta (of dtheta = theta1 - theta0),
    sum_diff (|v1 - v0|); the derived mean_dot, mean_cosine, dtheta_mean = atan2(sum_sin_dtheta,
    sum_cos_dtheta), mean_diff and magnitude_correlation (Pearson's r of the two magnitudes);
    hist[name] (n_roi, nbins) uint64 with edges[name].  An empty box gives NaN means.
    percentile_box, percentile_method as joint_reliability_mask.
    Bit-reproducible: the same inputs give the same bits on every run."""
    ch0, ch1 = tuple(ch0), tuple(ch1)
    if len(ch0) != 4 or len(ch1) != 4:
        raise ValueError("channel_compare: a channel is (vx, vy, vz or None, rel)")
    if in_plane:
        ch0, ch1 = (ch0[0], ch0[1], None, ch0[3]), (ch1[0], ch1[1], None, ch1[3])
    f0, f1 = _frame_pair("channel_compare", ch0, ch1, device)
    host = f0.host
    if (ch0[2] is None) != (ch1[2] is None):
        raise ValueError("channel_compare: vz of both channels or of neither")
    shape = tuple(ch0[3].shape)
    if ch0[2] is None and len(shape) == 3 and not in_plane:
        raise ValueError("channel_compare: (nz, ny, nx) fields need vz, or in_plane=True")
    if ch0[2] is not None and len(shape) == 2:
        raise ValueError("channel_compare: (ny, nx) fields take no vz")
    fields = [a for a in ch0[:3] + ch1[:3] if a is not None]
    if any(isinstance(a, np.ndarray) != host for a in fields):
        raise TypeError("channel_compare: all fields must be numpy arrays or all torch tensors")
    names = {_dtype_name(a) for a in fields}
    if len(names) != 1 or not names <= {"float32", "float64"}:
        raise TypeError("channel_compare: all velocity fields must be float64, or all float32")
    if any(tuple(a.shape) != shape for a in fields):
        raise ValueError(f"channel_compare: every field must have the shape {shape}")
    call = _PairCall(shape, f0.rel_dtype, f0.dev, rel_percentile, xyscale, zscale, tscale, rois, bins, floor, combine,
                     min_size, connectivity, percentile_box, percentile_method)
    with f0, f1:
        res = call.enqueue(f0.fields[:4], f1.fields[:4], f0.v_f32, f0.stream)
        return call.decode(res.cpu().numpy())


def principal_axes(rel, rel_percentile=90, threshold=None, min_size=0, connectivity=None, rois=None, physical=False,
                   xyscale=1.0, zscale=1.0, device=None, percentile_box=None, percentile_method="linear"):
    """The principal axes of one frame's reliability mask, per ROI: what the reference's
    plot_figure5.m:132-149 takes from ``regionprops3(relMask, 'EigenVectors', 'EigenValues')``,
    on the device (of3d_mask_axes); the mask-only part of flow_summary(axes="mask").

    rel, rel_percentile, threshold, connectivity and rois as reliability_mask; min_size >= 1
    opens the mask first, 0 (the default) takes rel > threshold as it is.  physical: the
    covariance in physical units, diag(xyscale, xyscale, zscale) on both sides.  Returns a dict of
    numpy values per ROI: rois, threshold, n_axes_mask (the mask's voxels), moments (uint64
    (n_roi, 10): n and the sums of x y z xx yy zz xy xz yz over box-local coordinates), centroid
    (x, y, z in volume coordinates), covariance (3, 3; population, exact numerators),
    axis_values (descending), axis_vectors (row k: e_k as x y z; largest component positive) and,
    with min_size >= 1, the opening's counts.  An empty mask gives NaN.  percentile_box,
    percentile_method as reliability_mask."""
    import torch

    f = _Frame("principal_axes", None, None, None, rel, device)
    spec = SummarySpec(rois=rois, rel_percentile=rel_percentile, min_size=min_size, connectivity=connectivity,
                       axes="mask", axes_physical=physical)
    boxes = spec.resolve(f.shape)[0]
    min_size, connectivity = spec.opening(f.ndim)
    call = _AxesCall(boxes, f.dims, f.rel_f64, spec.axes_request(f.ndim), physical, (xyscale, zscale, 1.0), f.dev)
    with f:
        thresh = f.threshold(rel_percentile, threshold, percentile_box, percentile_method)
        res = torch.empty(call.result_bytes // 8 + 4 * len(boxes), dtype=torch.int64, device=f.dev)
        keep_ptr = f.open_mask(boxes, min_size, connectivity, thresh, res.data_ptr() + call.result_bytes)
        call.enqueue(f.fields, thresh.data_ptr(), keep_ptr, res.data_ptr(), f.stream)
        words = res.cpu().numpy()
        out = {"rois": boxes.copy(), "threshold": f.threshold_value(thresh)}
    call.decode(words, out, projected=False)
    del out["axes_used"]
    if min_size:
        _decode_open_counts(words[call.result_bytes // 8:], len(boxes), out)
    return out


def flow_summary(vx, vy, vz, rel, rel_percentile=90, xyscale=1.0, zscale=1.0, tscale=1.0, rois=None, bins=None,
                 device=None, min_size=0, connectivity=None, axes=None, axes_physical=False, axis_bins=None,
                 weighted_bins=None, spread=None, percentile_box=None, percentile_method="linear", rel_profile=None):
    """One frame reduced on the device to a few kilobytes (one small device->host copy).

    Inputs as flow_statistics (numpy arrays or torch tensors, vz None for 2D).  The masking is
    flow_statistics' (rel > the rel_percentile-th percentile; zeros -> NaN; physical units); a
    voxel is valid when its magnitude is not NaN.  Returns a dict of numpy values: threshold,
    rois (n_roi, 6; ROI 0 is the whole volume, `rois` follow), per ROI n_valid, n_voxels and
    the raw sums sum_magnitude, sum_vx, sum_vy, sum_vz, sum_sin, sum_cos, sum_mag_sin,
    sum_mag_cos (sin/cos of theta = atan2(vy, vx)), the derived mean_magnitude, mean_vx/vy/vz,
    theta_mean = atan2(sum_sin/n, sum_cos/n), theta_mean_weighted (NaN where n_valid == 0), and
    hist[name] (n_roi, nbins) uint64 with edges[name] for every quantity in `bins`.
    min_size >= 1 (with connectivity, see SummarySpec): every ROI's mask is opened first
    (reliability_mask), n_valid then counts the kept voxels with a non-NaN magnitude, and the
    dict also holds n_mask, n_components, n_components_kept and n_kept (int64 per ROI).
    axes ("mask" or a 3x3 array), axes_physical, axis_bins (see SummarySpec): per ROI also the
    mask's integer moments (moments, n_axes_mask), centroid, covariance (3, 3), axis_values,
    axis_vectors (row k: e_k as x y z), axes_used (those, or the given array), and the flow
    projected on axes_used: n_axes_valid, sum_axis1..3, mean_axis1..3, hist["axis1"]...
    weighted_bins (quantity -> edges, as bins): hist_weighted[name] (n_roi, nbins) float64 =
    np.histogram(values, bins=edges, weights=magnitude)[0] over the valid voxels (the same mask,
    opened when min_size >= 1), with edges_weighted[name].  Figure 4's magnitude-weighted phi
    trace (plot_figure4_timeTraces.m:128-138, distPhiW) is hist_weighted["phi"] / n_valid[:, None].
    The script bins -phi into phiBins: pass weighted_bins={"phi": -phiBins[::-1]} and reverse
    the bins (hist_weighted["phi"][:, ::-1]); the bins are then right-closed where discretize's
    are left-closed, which differs only for a value exactly on an edge.
    spread ("mean", or vx, vy[, vz], magnitude to measure from; see SummarySpec): per ROI also
    spread_center (n_roi, 4: vx vy vz magnitude, the centre used); with d = value - centre over
    the valid voxels the raw sums ss_vx, ss_vy, ss_vz, ss_magnitude (of d^2), ss_vx_vy, ss_vx_vz,
    ss_vy_vz (of the products), sum_sin_phi, sum_cos_phi (sin phi = vz / magnitude; 0 in 2D);
    min_ and max_ of vx, vy, vz, magnitude; and, formed here from the sums, std_* = sqrt(ss / n)
    (np.nanstd's, ddof 0, for "mean"; the RMS deviation for a given centre), velocity_covariance
    (n_roi, 3, 3) = ss / n, theta_resultant R = hypot(sum_sin, sum_cos) / n, theta_std =
    sqrt(max(0, -2 ln R)) (scipy.stats.circstd's), in 3D phi_mean, phi_resultant, phi_std likewise,
    and theta_std_all / phi_std_all with R * n_valid / n_voxels (the validation notebook divides by
    the array's size, NaNs included).  NaN where n_valid == 0.  By a centred pass of its own
    (of3d_flow_spread): std << |mean| loses nothing.
    percentile_box, percentile_method (see SummarySpec): the threshold is the percentile of that
    one box of rel, by "linear" or "hazen" (MATLAB's prctile), whatever `rois`.  rel_profile (a
    RelProfileSpec): the dict also holds rel_profile, reliability_profile's dict for the same box
    and method, from the same select.  Without the three the threshold is of3d_quantile's.
    Bit-reproducible: the same inputs give the same bits on every run."""
    f = _Frame("flow_summary", vx, vy, vz, rel, device)
    spec = SummarySpec(rois, bins, rel_percentile, xyscale, zscale, tscale, min_size, connectivity, axes,
                       axes_physical, axis_bins, weighted_bins=weighted_bins, spread=spread,
                       percentile_box=percentile_box, percentile_method=percentile_method, rel_profile=rel_profile)
    call = _SummaryCall(spec, f.shape, f.rel_dtype, f.dev)
    with f:
        res = call.new_result(f.dev)
        call.enqueue(f.fields, res.data_ptr(), f.stream)
        return call.decode(res.cpu().numpy())


def _one_pass(f, call, boxes, min_size, connectivity, thresh):
    """One pass of the common calling convention on the entered frame f at the device threshold
    thresh, behind the optional opening of the mask: its result tensor, still on the device."""
    res = call.new_result(f.dev)
    call.enqueue(f.fields, thresh.data_ptr(), f.open_mask(boxes, min_size, connectivity, thresh), res.data_ptr(),
                 f.stream)
    return res


# ---------------------------------------------------------------------------
# Quiver samples (csrc/kt_quiver.hip): the vector lists the figure scripts hand to quiver /
# quiver3 (example_analysis_script.m:64-66,121-135, plot_figure4_Movies.m:121-143,
# plot_figure5.m:119-156, plot_FigureS2_dt.m:99-143, plot_figure3_ChannelCompare.m:181) —
# every gap-th voxel of a ROI whose masked velocity is not NaN — compacted on the device in C
# order, so that a series run with save_fields=False can still be drawn.  Rendering stays with
# the caller.
# ---------------------------------------------------------------------------
def quiver_sample(vx, vy, vz, rel, rel_percentile=90, xyscale=1.0, zscale=1.0, tscale=1.0, gap=2, rois=None,
                  min_size=0, connectivity=None, threshold=None, max_vectors=65536, device=None, percentile_box=None,
                  percentile_method="linear"):
    """The quiver vectors of one frame, per ROI: the voxels of the gap lattice
    ``[z0:z1:gz, y0:y1:gy, x0:x1:gx]`` of every ROI whose masked physical velocity is not NaN
    (flow_summary's validity), in C order, by of3d_quiver_sample; only the lists leave the device.

    Inputs, scales, rois, min_size and connectivity as flow_summary (numpy arrays or torch
    tensors, vz None for 2D; ROI 0 is the whole volume); gap and max_vectors as QuiverSpec.  The
    threshold is the rel_percentile-th percentile of rel (percentile_threshold_device) unless
    `threshold` (a Python float, used as one element of rel's dtype) is given; min_size >= 1
    opens every ROI's mask first (reliability_mask); percentile_box, percentile_method as
    reliability_mask.
    Returns a dict: threshold, rois (n_roi, 6), gap (gz, gy, gx) and samples, a list with one
    dict per ROI: zyx (int64 (n, 3), volume coordinates; z = 0 in 2D), v (float64 (n, 3): vx,
    vy, vz in physical units, vz 0.0 in 2D), magnitude, theta and (3D) phi (float64 (n,), formed
    on the host from v with the notebook's expressions), n_lattice, n_valid (the full count) and
    truncated (n_valid > n = min(n_valid, n_lattice, max_vectors): only the first n in C order
    are held).  For each field f in physical units, v's column equals
    ``f[z0:z1:gz, y0:y1:gy, x0:x1:gx][valid]`` bit for bit.
    Bit-reproducible: the same inputs give the same bits, in the same order, on every run."""
    f = _Frame("quiver_sample", vx, vy, vz, rel, device)
    spec = SummarySpec(rois=rois, rel_percentile=rel_percentile, min_size=min_size, connectivity=connectivity)
    boxes = spec.resolve(f.shape)[0]
    min_size, connectivity = spec.opening(f.ndim)
    call = _QuiverCall(boxes, f.dims, f.rel_f64, QuiverSpec(gap=gap, max_vectors=max_vectors), f.ndim,
                       (xyscale, zscale, tscale), f.dev)
    with f:
        words = _one_pass(f, call, boxes, min_size, connectivity,
                          f.threshold(rel_percentile, threshold, percentile_box, percentile_method)).cpu().numpy()
    return {"threshold": _word_threshold(words, f.rel_f64), "rois": boxes.copy(), "gap": call.gap,
            "samples": call.decode(words)}


def export_fields(vx, vy, vz, rel, rel_percentile=90, threshold=None, xyscale=1.0, zscale=1.0, tscale=1.0, rois=None,
                  spec=None, min_size=0, connectivity=None, percentile_box=None, percentile_method="linear",
                  device=None):
    """The fields of one frame cropped to ROIs, masked and scaled as the figure scripts do right
    after loading them, by of3d_field_export: compact blocks, formed on the device.

    Inputs, scales, rois, min_size and connectivity as flow_summary (numpy arrays or torch
    tensors, vz None for 2D; ROI 0 is the whole volume); threshold, percentile_box and
    percentile_method as quiver_sample.  spec: a FieldSpec (default FieldSpec(): every ROI after
    0, all fields, mask "nan", physical units, the fields' own types); min_size >= 1 opens every
    ROI's mask first (reliability_mask), and ROI r is masked by its own opened mask.
    Returns a dict: threshold, rois (n_roi, 6) and blocks, a list with one dict per exported ROI:
    roi (its index), box (6 ints) and per exported field an array of shape (dz, dy, dx) — (dy, dx)
    in 2D.  numpy inputs give numpy arrays, torch inputs device tensors; all of them view one
    result block.  With mask None, physical False and dtype None a block is ``f[z0:z1, y0:y1,
    x0:x1]`` bit for bit."""
    f = _Frame("export_fields", vx, vy, vz, rel, device)
    summary = SummarySpec(rois=rois, rel_percentile=rel_percentile, min_size=min_size, connectivity=connectivity)
    boxes = summary.resolve(f.shape)[0]
    min_size, connectivity = summary.opening(f.ndim)
    call = _ExportCall(boxes, f.dims, f.rel_f64, f.v_f32, FieldSpec() if spec is None else spec, f.ndim,
                       (xyscale, zscale, tscale))
    with f:
        words = _one_pass(f, call, boxes, min_size, connectivity,
                          f.threshold(rel_percentile, threshold, percentile_box, percentile_method))
        head = words[:1].cpu().numpy()
        words = words.cpu().numpy() if f.host else words
    return {"threshold": _word_threshold(head, f.rel_f64), "rois": boxes.copy(), "blocks": call.decode(words)}


# ---------------------------------------------------------------------------
# Projection maps (csrc/kt_project.hip): the image every figure script draws its vectors on —
# max(myo,[],3) (plot_figure3_ROIfigures.m:298,313, plot_figure3_ChannelCompare.m:64,69,
# plot_figure5.m:915-917), the mask's footprint sum(relMask,3) (plot_figure4_timeTraces.m:103,
# plot_figure5.m:90, plot_figure5_Movie.m:91) — and the flow reduced along an axis, on the
# resident fields, so that a series run with save_fields=False can still return a picture.
# Rendering stays with the caller.
# ---------------------------------------------------------------------------
def _image_frame(image, f):
    """projection_maps' image argument checked against the entered frame f: (tensor on the
    frame's device, of3d_dtype code).  uint16 / uint32 travel as their signed views, as the
    frame ring keeps them."""
    import torch

    dt = _np_dtype(image)
    if dt not in _lib.DTYPE_CODES:
        raise TypeError(f"project: image dtype {dt} is not one of {[d.name for d in _lib.DTYPE_CODES]}")
    if tuple(int(v) for v in image.shape) != f.shape:
        raise ValueError(f"project: image shape {tuple(image.shape)} != the fields' {f.shape}")
    if isinstance(image, np.ndarray):
        a = np.ascontiguousarray(image)
        signed = {"uint16": np.int16, "uint32": np.int32}.get(dt.name)
        t = torch.as_tensor(a.view(signed) if signed else a).to(f.dev)
    else:
        t = image.to(f.dev).contiguous()
    return t, _lib.DTYPE_CODES[dt]


def projection_maps(vx, vy, vz, rel, image=None, spec=None, rel_percentile=90, threshold=None, xyscale=1.0,
                    zscale=1.0, tscale=1.0, rois=None, min_size=0, connectivity=None, percentile_box=None,
                    percentile_method="linear", device=None):
    """Projection maps of one frame, per ROI and axis, by of3d_flow_project: one value per line
    of the ROI along the axis, only the maps leave the device.

    Inputs, scales, rois, min_size and connectivity as flow_summary (numpy arrays or torch
    tensors, vz None for 2D; ROI 0 is the whole volume); threshold, percentile_box and
    percentile_method as quiver_sample.  spec: a ProjectionSpec (default ProjectionSpec(): every
    ROI after 0, along z — 2D: along y and x —, the seven flow maps).  image: a numpy array or
    tensor of the volume's shape in one of the seven input dtypes, required iff the spec names an
    image map (ProjectionSpec(image=True)).
    Returns a dict: threshold, rois (n_roi, 6), axes (the names) and maps, a list with one dict
    per projected ROI: roi (its index), box (6 ints) and per axis a dict of arrays of the plane's
    shape — axis z (dy, dx), y (dz, dx), x (dz, dy); 2D: 1-D profiles —: n_mask and n_valid
    (int64), sum_vx, sum_vy, sum_vz, sum_magnitude, max_magnitude, max_image, sum_image
    (float64) as requested, and formed on the host mean_vx, mean_vy, mean_vz, mean_magnitude
    (sum / n_valid, NaN where 0) and mean_image (sum_image / the line's length).  A sum is the
    loop ``s = 0.0; for k ascending along the axis: if valid: s = s + v`` bit for bit.
    Bit-reproducible: the same inputs give the same bits on every run."""
    f = _Frame("projection_maps", vx, vy, vz, rel, device)
    summary = SummarySpec(rois=rois, rel_percentile=rel_percentile, min_size=min_size, connectivity=connectivity)
    boxes = summary.resolve(f.shape)[0]
    min_size, connectivity = summary.opening(f.ndim)
    call = _ProjectCall(boxes, f.dims, f.rel_f64, ProjectionSpec() if spec is None else spec, f.ndim,
                        (xyscale, zscale, tscale))
    if call.needs_image != (image is not None):
        raise ValueError("project: an image is needed by max_image / sum_image (ProjectionSpec(image=True)), "
                         "and only by them")
    with f:
        if image is not None:
            timg, code = _image_frame(image, f)
            call.bind_image(timg.data_ptr(), code)
        words = _one_pass(f, call, boxes, min_size, connectivity,
                          f.threshold(rel_percentile, threshold, percentile_box, percentile_method)).cpu().numpy()
    return {"threshold": _word_threshold(words, f.rel_f64), "rois": boxes.copy(), "axes": call.axes,
            "maps": call.decode(words)}


def write_projections(path, result):
    """One frame's projection maps (projection_maps' dict) as an npz: threshold, rois, axes, the
    projected ROIs' indices (projected) and per ROI r, axis a and map m the array <m>_<a>_<r>,
    the host's means included."""
    arrays = {"threshold": np.asarray(result["threshold"]), "rois": np.asarray(result["rois"], dtype=np.int64),
              "axes": np.asarray(list(result["axes"])),
              "projected": np.asarray([e["roi"] for e in result["maps"]], dtype=np.int64)}
    for e in result["maps"]:
        for a in result["axes"]:
            for name, v in e[a].items():
                arrays[f"{name}_{a}_{e['roi']}"] = np.asarray(v)
    np.savez(path, **arrays)


def read_projections(path):
    """write_projections' file as projection_maps' dict."""
    with np.load(path) as f:
        rois, axes = f["rois"], tuple(str(a) for a in f["axes"])
        out = {"threshold": f["threshold"][()], "rois": rois, "axes": axes, "maps": []}
        for r in (int(v) for v in f["projected"]):
            entry = {"roi": r, "box": tuple(int(v) for v in rois[r])}
            for a in axes:
                tail = f"_{a}_{r}"
                entry[a] = {k[:-len(tail)]: f[k] for k in f.files if k.endswith(tail)}
            out["maps"].append(entry)
    return out


_SPLIT_COLUMNS = {"vx": 0, "vy": 1, "vz": 2}


def quiver_split(sample, quantity, edges):
    """The figure scripts' colour slices of one ROI's quiver sample (plot_figure4_Movies.m:132-142:
    one quiver call per slice ``(c >= e(j)) & (c < e(j+1))``): a list of len(edges) - 1 index
    arrays into the sample's records.  quantity: "vx" | "vy" | "vz" | "magnitude" | "theta" |
    "phi"; edges: ascending, left-closed slices, so a last edge of inf takes everything from the
    edge before it.  Host only."""
    if quantity in _SPLIT_COLUMNS:
        c = np.asarray(sample["v"])[:, _SPLIT_COLUMNS[quantity]]
    elif quantity in ("magnitude", "theta", "phi") and quantity in sample:
        c = np.asarray(sample[quantity])
    else:
        raise ValueError(f"quiver: unknown quantity {quantity!r} of this sample (one of {QUANTITIES})")
    e = np.asarray(edges, dtype=np.float64)
    if e.ndim != 1 or e.size < 2 or np.any(np.isnan(e)) or not np.all(e[1:] >= e[:-1]):
        raise ValueError("quiver: edges must be a 1-D ascending array of at least 2 values without NaN")
    return [np.flatnonzero((c >= e[j]) & (c < e[j + 1])) for j in range(e.size - 1)]


def write_quiver(path, sample):
    """One frame's quiver sample (quiver_sample's dict) as an npz: gap (int64 (3,)), rois,
    threshold and per ROI r zyx_<r>, v_<r>, n_valid_<r>, n_lattice_<r>; the derived quantities are
    not stored (read_quiver forms them again)."""
    arrays = {"gap": np.asarray(sample["gap"], dtype=np.int64), "rois": np.asarray(sample["rois"], dtype=np.int64),
              "threshold": np.asarray(sample["threshold"])}
    for r, s in enumerate(sample["samples"]):
        arrays[f"zyx_{r}"] = np.asarray(s["zyx"], dtype=np.int64).reshape(-1, 3)
        arrays[f"v_{r}"] = np.asarray(s["v"], dtype=np.float64).reshape(-1, 3)
        arrays[f"n_valid_{r}"] = np.int64(s["n_valid"])
        arrays[f"n_lattice_{r}"] = np.int64(s["n_lattice"])
    np.savez(path, **arrays)


def read_quiver(path, ndim=3):
    """write_quiver's file as quiver_sample's dict (ndim 2: no phi, a 2-term magnitude)."""
    with np.load(path) as f:
        rois = f["rois"]
        out = {"threshold": f["threshold"][()], "rois": rois, "gap": tuple(int(v) for v in f["gap"]), "samples": []}
        for r in range(len(rois)):
            out["samples"].append(_quiver_entry(f[f"zyx_{r}"], f[f"v_{r}"], ndim, f[f"n_lattice_{r}"],
                                                f[f"n_valid_{r}"]))
    return out


# ---------------------------------------------------------------------------
# Contractility (csrc/kt_contract.hip, csrc/kt_ccl.hip: of3d_mask_largest): figure 2 / movie S2
# of the reference (plot_figure2_movie.ipynb cell 1) — the largest connected component of the
# cropped reliability mask, its centre of mass, and per voxel the angle between the flow and the
# direction to that centre — on the resident fields, so that a series run with
# save_fields=False still yields the figure's distributions.
# ---------------------------------------------------------------------------
def largest_component_mask(rel, rel_percentile=90, threshold=None, connectivity=None, rois=None, device=None,
                           percentile_box=None, percentile_method="linear"):
    """The largest connected component of the reliability mask of one frame, per ROI: the
    notebook's measure.label / sort by area / zero all but the first, on the device
    (of3d_mask_largest).  Among components of equal size the one holding the smallest linear
    index of the ROI is kept (the lowest label of a raster-order labelling, what the notebook's
    stable sort keeps); an empty mask keeps nothing.

    Arguments but min_size as reliability_mask's, and so is the returned dict: keep (uint16,
    rel's shape; bit r set where the voxel lies in box r and in that box's largest component),
    mask (r -> that bit plane as bool), rois, threshold and per ROI n_mask, n_components,
    n_components_kept (0 or 1), n_kept (int64).  percentile_box, percentile_method as
    reliability_mask."""
    f = _Frame("largest_component_mask", None, None, None, rel, device)
    boxes = SummarySpec(rois=rois, rel_percentile=rel_percentile).resolve(f.shape)[0]
    connectivity = ContractSpec(connectivity=connectivity).resolve(f.ndim)[1]
    call = _LargestCall(boxes, f.dims, f.rel_f64, connectivity, f.dev)
    with f:
        return _mask_entry(f, call, boxes, f.threshold(rel_percentile, threshold, percentile_box, percentile_method))


def contractility(vx, vy, vz, rel, rel_percentile=90, xyscale=1.0, zscale=1.0, tscale=1.0, rois=None, spec=None,
                  device=None, percentile_box=None, percentile_method="linear"):
    """One frame's contractility per ROI (ROI 0 is the whole volume, `rois` follow), reduced on
    the device to a few hundred bytes: the mask's centroid and, over the valid voxels (the masked
    velocity's magnitude is not NaN, flow_summary's validity), the angle in degrees between the
    physical velocity and the direction from the voxel to the centre, by of3d_flow_contract.

    Inputs and scales as flow_summary (numpy arrays or torch tensors, vz None for 2D); spec: a
    ContractSpec (default: the largest component, its own centroid, no histograms; mask="summary"
    is the threshold mask here).  Returns a dict of numpy values: threshold, rois and per ROI
    centroid and center_used (x y z, volume coordinates; NaN for an empty mask), moments (uint64
    n, Sx, Sy, Sz of the mask in the ROI's own coordinates), n_mask, n_components, n_kept (the
    labelling's counts; with mask="summary" n_mask = n_kept = the mask reduced over and
    n_components = -1), n_valid, n_angle (the valid voxels with a direction: all but the centre's
    own voxel), n_inward (cosine > 0), the raw sums sum_angle, sum_dot, sum_inward, sum_speed over
    the voxels with an angle, mean_angle, mean_dot, mean_inward, mean_speed (formed here from the
    sums; NaN where n_angle == 0), inward_fraction = n_inward / n_angle, and hist[name]
    (n_roi, nbins) uint64 with edges[name] for every quantity in spec.bins.
    percentile_box, percentile_method as reliability_mask.
    A cosine that rounding left a last bit beyond +-1 gives exactly 0 or 180 degrees where the
    notebook's arccos gives NaN.  Bit-reproducible: the same inputs give the same bits on every run."""
    f = _Frame("contractility", vx, vy, vz, rel, device)
    boxes = SummarySpec(rois=rois, rel_percentile=rel_percentile).resolve(f.shape)[0]
    call = _ContractCall(boxes, f.dims, f.rel_f64, ContractSpec() if spec is None else spec, f.ndim,
                         (xyscale, zscale, tscale), f.dev)
    with f:
        thresh = f.threshold(rel_percentile, None, percentile_box, percentile_method)
        out = call.decode(_one_pass(f, call, boxes, 0, None, thresh).cpu().numpy())
        out["threshold"] = f.threshold_value(thresh)
    return out


def centroid_angle(sample, center, xyscale, zscale):
    """The movie's quiver colour: for the records of one ROI's quiver sample (an entry of
    quiver_sample's ``samples``) the angle in degrees between each vector and the direction to
    `center` (x, y, z in volume coordinates, e.g. contractility's center_used of that ROI; z is
    ignored for a 2D sample), with the notebook's numpy expressions — NaN where arccos gives
    NaN.  Host only: the lists are small."""
    zyx = np.asarray(sample["zyx"], dtype=np.float64).reshape(-1, 3)
    v = np.asarray(sample["v"], dtype=np.float64).reshape(-1, 3)
    cx, cy, cz = (float(c) for c in center)
    with np.errstate(invalid="ignore", divide="ignore"):
        dxc = zyx[:, 2] * xyscale - cx * xyscale
        dyc = zyx[:, 1] * xyscale - cy * xyscale
        dzc = zyx[:, 0] * zscale - cz * zscale if "phi" in sample else np.zeros(len(zyx))
        normalc = np.stack([-dxc, -dyc, -dzc], axis=-1)
        normalc = normalc / np.linalg.norm(normalc, axis=-1, keepdims=True)
        speed = np.sqrt(np.power(v[:, 0], 2) + np.power(v[:, 1], 2) + np.power(v[:, 2], 2))
        vnorm = v / speed[:, None]
        return np.degrees(np.arccos(np.sum(vnorm * normalc, axis=-1)))


CONTRACT_CSV_INT_COLUMNS = ("frame", "roi", "z0", "z1", "y0", "y1", "x0", "x1", "n_mask", "n_components", "n_kept",
                            "n_valid", "n_angle", "n_inward")
CONTRACT_CSV_COLUMNS = CONTRACT_CSV_INT_COLUMNS + (
    "centroid_x", "centroid_y", "centroid_z", "center_x", "center_y", "center_z", "mean_angle", "mean_dot",
    "mean_inward", "mean_speed", "inward_fraction") + CONTRACT_SUMS


def write_contract(prefix, frames, results):
    """<prefix>_contract.csv (one row per frame and ROI, CONTRACT_CSV_COLUMNS; floats as repr, so
    they read back exactly) and <prefix>_contract_hist.npz (frames, edges_<name>, counts_<name> of
    shape (frames, n_roi, nbins)) from contractility dicts of consecutive frames."""
    with open(prefix + "_contract.csv", "w", newline="") as f:
        f.write(",".join(CONTRACT_CSV_COLUMNS) + "\n")
        for frame, c in zip(frames, results):
            for r in range(len(c["rois"])):
                row = [int(frame), r] + [int(v) for v in c["rois"][r]]
                row += [int(c[k][r]) for k in CONTRACT_CSV_INT_COLUMNS[8:]]
                floats = list(c["centroid"][r]) + list(c["center_used"][r])
                floats += [c[k][r] for k in CONTRACT_CSV_COLUMNS[len(CONTRACT_CSV_INT_COLUMNS) + 6:]]
                f.write(",".join(str(v) for v in row + [repr(float(v)) for v in floats]) + "\n")
    arrays = {"frames": np.asarray(list(frames), dtype=np.int64)}
    if results:
        for name, e in results[0]["edges"].items():
            arrays["edges_" + name] = e
            arrays["counts_" + name] = np.stack([c["hist"][name] for c in results])
    np.savez(prefix + "_contract_hist.npz", **arrays)


def read_contract_csv(path):
    """The rows of a <prefix>_contract.csv as a dict of numpy columns (int64 / float64)."""
    with open(path) as f:
        cols = f.readline().strip().split(",")
        rows = [line.strip().split(",") for line in f if line.strip()]
    ints = set(CONTRACT_CSV_INT_COLUMNS)
    return {c: np.array([int(r[i]) if c in ints else float(r[i]) for r in rows],
                        dtype=np.int64 if c in ints else np.float64) for i, c in enumerate(cols)}


CSV_COLUMNS = ("frame", "roi", "z0", "z1", "y0", "y1", "x0", "x1", "threshold", "n_valid", "n_voxels",
               "mean_magnitude", "mean_vx", "mean_vy", "mean_vz", "theta_mean", "theta_mean_weighted") + SUMS


CSV_OPEN_COLUMNS = OPEN_COUNTS  # appended when the summaries carry the opening's counts (min_size >= 1)


# appended when the summaries carry the axes block (SummarySpec.axes): the integer columns, then
# the float64 ones (vectors as x y z)
CSV_AXES_INT_COLUMNS = ("n_axes_mask",) + tuple("mom_" + m for m in MOMENTS[1:]) + ("n_axes_valid",)
CSV_AXES_COLUMNS = CSV_AXES_INT_COLUMNS + (
    ("centroid_x", "centroid_y", "centroid_z", "cov_xx", "cov_yy", "cov_zz", "cov_xy", "cov_xz", "cov_yz",
     "axis_value1", "axis_value2", "axis_value3")
    + tuple(f"{a}_{c}" for a in AXIS_NAMES for c in "xyz") + tuple(f"used{k}_{c}" for k in "123" for c in "xyz")
    + tuple("sum_" + a for a in AXIS_NAMES) + tuple("mean_" + a for a in AXIS_NAMES))


# appended when the summaries carry the spread block (SummarySpec.spread): float64 columns (the
# phi columns NaN in 2D)
_SPREAD_CSV_KEYS = (SPREAD_SUMS + tuple(f"{m}_{k}" for m in ("min", "max", "std") for k in SPREAD_COMPONENTS)
                    + ("theta_resultant", "theta_std", "phi_mean", "phi_resultant", "phi_std", "theta_std_all",
                       "phi_std_all"))
CSV_SPREAD_COLUMNS = (tuple("spread_center_" + k for k in SPREAD_COMPONENTS) + _SPREAD_CSV_KEYS
                      + ("vcov_xx", "vcov_yy", "vcov_zz", "vcov_xy", "vcov_xz", "vcov_yz"))


# appended when the summaries carry a reliability profile (SummarySpec.rel_profile): these, then
# per percentile p of the profile rel_p<p> (its threshold) and n_above_p<p> (int), <p> = format(p, "g")
CSV_PROFILE_COLUMNS = ("rel_min", "rel_max", "rel_n_nan")


def profile_columns(percentiles):
    """The CSV columns of a reliability profile with these percentiles."""
    return CSV_PROFILE_COLUMNS + tuple(f"{k}_p{format(float(p), 'g')}" for p in percentiles
                                       for k in ("rel", "n_above"))


def _profile_row(s, r):
    """The profile_columns values of ROI r of a summary dict."""
    p = s["rel_profile"]
    row = [repr(float(p["min"])), repr(float(p["max"])), int(p["n_nan"][r])]
    for k in range(len(p["percentiles"])):
        row += [repr(float(p["thresholds"][k])), int(p["n_above"][r][k])]
    return row


def _spread_row(s, r):
    """The CSV_SPREAD_COLUMNS values of ROI r of a summary dict."""
    c = s["velocity_covariance"][r]
    floats = list(s["spread_center"][r]) + [s[k][r] if k in s else np.nan for k in _SPREAD_CSV_KEYS]
    floats += [c[0, 0], c[1, 1], c[2, 2], c[0, 1], c[0, 2], c[1, 2]]
    return [repr(float(v)) for v in floats]


def _axes_row(s, r):
    """The CSV_AXES_COLUMNS values of ROI r of a summary dict."""
    c = s["covariance"][r]
    ints = [int(s["n_axes_mask"][r])] + [int(v) for v in s["moments"][r][1:]] + [int(s["n_axes_valid"][r])]
    floats = list(s["centroid"][r]) + [c[0, 0], c[1, 1], c[2, 2], c[0, 1], c[0, 2], c[1, 2]]
    floats += list(s["axis_values"][r]) + list(s["axis_vectors"][r].ravel()) + list(s["axes_used"][r].ravel())
    floats += [s["sum_" + a][r] for a in AXIS_NAMES] + [s["mean_" + a][r] for a in AXIS_NAMES]
    return ints + [repr(float(v)) for v in floats]


def write_summaries(prefix, frames, summaries):
    """<prefix>_summary.csv (one row per frame and ROI; floats as repr, so they read back
    exactly; the columns CSV_COLUMNS, then CSV_OPEN_COLUMNS when the summaries were made with
    min_size >= 1, then CSV_AXES_COLUMNS when they were made with axes, then CSV_SPREAD_COLUMNS
    when they were made with spread, then profile_columns(percentiles) when they were made with
    rel_profile) and <prefix>_summary_hist.npz (frames, edges_<name>, counts_<name> of shape
    (frames, n_roi, nbins), with weighted_bins wedges_<name>, weights_<name> float64 of that
    shape, and with rel_profile counts_rel (frames, n_roi, nbins) and edges_rel (frames,
    nbins + 1): the auto edges differ from frame to frame) from flow_summary dicts of
    consecutive frames."""
    opened = bool(summaries) and all(k in summaries[0] for k in CSV_OPEN_COLUMNS)
    with_axes = bool(summaries) and "axes_used" in summaries[0]
    with_spread = bool(summaries) and "spread_center" in summaries[0]
    with_profile = bool(summaries) and "rel_profile" in summaries[0]
    with open(prefix + "_summary.csv", "w", newline="") as f:
        f.write(",".join(CSV_COLUMNS + (CSV_OPEN_COLUMNS if opened else ())
                         + (CSV_AXES_COLUMNS if with_axes else ())
                         + (CSV_SPREAD_COLUMNS if with_spread else ())
                         + (profile_columns(summaries[0]["rel_profile"]["percentiles"]) if with_profile else ()))
                + "\n")
        for frame, s in zip(frames, summaries):
            for r in range(len(s["rois"])):
                row = [int(frame), r] + [int(v) for v in s["rois"][r]] + [repr(float(s["threshold"]))]
                row += [int(s["n_valid"][r]), int(s["n_voxels"][r])]
                row += [repr(float(s[k][r])) for k in CSV_COLUMNS[11:]]
                if opened:
                    row += [int(s[k][r]) for k in CSV_OPEN_COLUMNS]
                if with_axes:
                    row += _axes_row(s, r)
                if with_spread:
                    row += _spread_row(s, r)
                if with_profile:
                    row += _profile_row(s, r)
                f.write(",".join(str(v) for v in row) + "\n")
    arrays = {"frames": np.asarray(list(frames), dtype=np.int64)}
    if summaries:
        for name, e in summaries[0]["edges"].items():
            arrays["edges_" + name] = e
            arrays["counts_" + name] = np.stack([s["hist"][name] for s in summaries])
        for name, e in summaries[0].get("edges_weighted", {}).items():
            arrays["wedges_" + name] = e
            arrays["weights_" + name] = np.stack([s["hist_weighted"][name] for s in summaries])
        if with_profile:
            arrays["counts_rel"] = np.stack([s["rel_profile"]["hist"] for s in summaries])
            arrays["edges_rel"] = np.stack([s["rel_profile"]["edges"] for s in summaries])
    np.savez(prefix + "_summary_hist.npz", **arrays)


def read_summary_csv(path):
    """The rows of a <prefix>_summary.csv as a dict of numpy columns (int64 / float64)."""
    with open(path) as f:
        cols = f.readline().strip().split(",")
        rows = [line.strip().split(",") for line in f if line.strip()]
    ints = set(CSV_COLUMNS[:8]) | {"n_valid", "n_voxels"} | set(CSV_OPEN_COLUMNS) | set(CSV_AXES_INT_COLUMNS)
    ints |= {"rel_n_nan"} | {c for c in cols if c.startswith("n_above_p")}
    return {c: np.array([int(r[i]) if c in ints else float(r[i]) for r in rows],
                        dtype=np.int64 if c in ints else np.float64) for i, c in enumerate(cols)}
