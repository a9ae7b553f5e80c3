"""numpy restatement of analysis.export_fields (tests only), written straight from the
expressions of the reference's scripts: the crop ``vx(y1:y2,x1:x2,z1:z2)``, then
``vx.*relMask./relMask*xyscale/tscale`` (plot_figure3 / 4 / 5), ``vx.*relMask``
(plot_FigureS2_dt.m:123) or ``vx*relMask; vx[vx==0]=nan`` (the notebooks) — on float64 copies of
the velocities, as the device widens a float32 field first —, ``.astype(np.float32)`` last.  The
mask is ``rel > np.percentile(rel, p)`` (or a given threshold), opened per ROI by
mask_ref.open_ref when min_size >= 1.  same() is the tests' comparison: values bitwise where
not NaN, NaNs in the same places (their sign and payload out of 0/0 differ between CPU and GPU)."""
import numpy as np

import mask_ref as mr
import summary_ref as sr

FIELDS = ("vx", "vy", "vz", "rel")


def masks_of(rel, boxes, rel_percentile=90, threshold=None, min_size=0, connectivity=None):
    """(threshold, [boolean mask of box r over the whole volume, as (nz, ny, nx)])."""
    rel = np.asarray(rel)
    thresh = rel.dtype.type(threshold) if threshold is not None else np.percentile(rel, rel_percentile)
    vol = rel.reshape((1,) + rel.shape) if rel.ndim == 2 else rel
    if min_size >= 1:
        c = connectivity if connectivity is not None else (8 if rel.ndim == 2 else 26)
        keep, _ = mr.open_ref(rel, thresh, boxes, min_size, c)
        keep = keep.reshape(vol.shape)
        return thresh, [((keep >> np.uint16(r)) & np.uint16(1)).astype(bool) for r in range(len(boxes))]
    with np.errstate(invalid="ignore"):
        return thresh, [vol > thresh] * len(boxes)


def export_block(v, m, sl, mask, physical, scale, tscale, dtype):
    """One velocity block: v (nz, ny, nx) cropped to sl, masked by the boolean m (same shape as
    v) in mode `mask`, scaled, narrowed."""
    if mask is None and not physical:
        out = v[sl].copy()
    else:
        w = np.array(v, dtype=np.float64)
        with np.errstate(all="ignore"):
            if mask == "nan":
                out = w[sl] * m[sl] / m[sl]
            elif mask == "zero":
                out = w[sl] * m[sl]
            elif mask == "summary":
                out = w[sl] * m[sl]
                out[out == 0] = np.nan
            else:
                assert mask is None, mask
                out = w[sl]
            if physical:
                out = out * scale / tscale
    return out.astype(np.float32) if dtype == "float32" or v.dtype == np.float32 else out


def export_ref(vx, vy, vz, rel, rel_percentile=90, threshold=None, xyscale=1.0, zscale=1.0, tscale=1.0, rois=None,
               export_rois=None, fields=None, mask="nan", physical=True, dtype=None, min_size=0, connectivity=None):
    """analysis.export_fields' dict; export_rois, fields, mask, physical, dtype as FieldSpec's.
    Besides it "inside": per exported ROI the voxels of the box inside its mask."""
    shape = np.shape(rel)
    ndim = len(shape)
    boxes = sr.boxes_of(shape, rois)
    if export_rois is None:
        export_rois = tuple(range(1, len(boxes))) or (0,)
    if fields is None:
        fields = tuple(n for n in FIELDS if ndim == 3 or n != "vz")
    thresh, masks = masks_of(rel, boxes, rel_percentile, threshold, min_size, connectivity)
    vol = lambda f: None if f is None else np.asarray(f).reshape((1,) + shape if ndim == 2 else shape)
    src = dict(zip(FIELDS, (vol(vx), vol(vy), vol(vz), vol(rel))))
    blocks, inside = [], []
    for r in export_rois:
        z0, z1, y0, y1, x0, x1 = (int(v) for v in boxes[r])
        sl = (slice(z0, z1), slice(y0, y1), slice(x0, x1))
        entry = {"roi": r, "box": (z0, z1, y0, y1, x0, x1)}
        for name in fields:
            if name == "rel":
                out = src["rel"][sl].astype(np.float32) if dtype == "float32" else src["rel"][sl].copy()
            else:
                out = export_block(src[name], masks[r], sl, mask, physical, zscale if name == "vz" else xyscale,
                                   tscale, dtype)
            entry[name] = out if ndim == 3 else out[0]
        blocks.append(entry)
        inside.append(int(masks[r][sl].sum()))
    return {"threshold": thresh, "rois": boxes, "blocks": blocks, "inside": inside}


def same(got, ref):
    """got is ref: dtype, shape, NaNs in the same places, every other value bit for bit."""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.dtype != ref.dtype or got.shape != ref.shape:
        return False
    nan = np.isnan(ref)
    bits = np.dtype("u%d" % ref.dtype.itemsize)
    return bool(np.array_equal(np.isnan(got), nan) and
                np.array_equal(np.ascontiguousarray(got).view(bits)[~nan], np.ascontiguousarray(ref).view(bits)[~nan]))


def assert_blocks(got, ref, bytes_exact=False):
    """export_fields' dict against export_ref's; bytes_exact (mode None): tobytes() throughout."""
    assert np.array_equal(got["rois"], ref["rois"])
    assert np.asarray(got["threshold"]).dtype == np.asarray(ref["threshold"]).dtype
    assert got["threshold"] == ref["threshold"] or (np.isnan(got["threshold"]) and np.isnan(ref["threshold"]))
    assert len(got["blocks"]) == len(ref["blocks"])
    for g, w in zip(got["blocks"], ref["blocks"]):
        assert list(g) == list(w), (list(g), list(w))
        assert g["roi"] == w["roi"] and tuple(g["box"]) == tuple(w["box"])
        for name in list(w)[2:]:
            a, b = np.asarray(g[name]), w[name]
            if bytes_exact:
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (w["roi"], name)
            else:
                assert same(a, b), (w["roi"], name)
