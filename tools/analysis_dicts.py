"""The decoded dictionaries of every public analysis entry and of a FlowStream with every add-on,
for a bit-for-bit comparison of two versions of the Python host.

tools/summary_words.py pins the device words; this pins what analysis.py and stream.py make of
them: every public entry of analysis.py and a FlowStream with summary=, quiver=, contract= and
fields=FieldSpec run on summary_words.py's seeded fields, and every returned dict is flattened to
path -> array (lists become indexed paths, tensors are copied to the host, the `mask` lambdas are
evaluated for every ROI).  Two versions of the host agree when the two mappings have the same
paths and every array has the same dtype, shape and bytes (tests/test_gpu_analysis_dicts.py holds
the tree's to tests/golden/summary/analysis_dicts.npz).

Cases a (5, 37, 67) and c (37, 67) of summary_words.py, each with ROI 0 and the interior box.
Per case the velocity entries (flow_summary, quiver_sample, export_fields, contractility,
channel_compare) run with velocities float64 / float32 x rel float32 / float64 x min_size 0 / 3
on numpy input, and two of those runs again on CUDA tensors; the rel-only entries
(reliability_mask, largest_component_mask, principal_axes, reliability_profile,
joint_reliability_mask, reliability_thresholds) once per rel dtype, min_size and input kind.  The
threshold comes by turns from the plain percentile, from percentile_box with
percentile_method="hazen" (flow_summary then with a rel_profile: the select path and its
threshold index) and from an explicit threshold=.  The streams (3D fp64 with an opened, boxed,
profiled summary; 2D fp32 plain) submit two frames each of seeded uint16 images at
xyzSig = tSig = wSig = 1.  Only the interior box is exported, and max_vectors is small.

The file: a flattened mapping has thousands of arrays of a few bytes, and a zip member costs a
few hundred bytes however small, so the arrays are packed — `paths`, `dtypes`, `shapes` (one
string per array) and `data` (their bytes, one after the other) — beside the meta_* entries;
pack() / unpack() convert.

    python tools/analysis_dicts.py --out dicts.npz [--commit ID]
"""

import argparse
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from summary_words import CASES, GIVEN_AXES, SCALES, SEED, SPREAD_CENTER, fields  # noqa: E402

CASES = {k: CASES[k] for k in ("a", "c")}
DTYPES = ((np.float64, np.float32), (np.float32, np.float32), (np.float64, np.float64), (np.float32, np.float64))
TORCH_RUNS = ((np.float64, np.float32, 3), (np.float32, np.float64, 0))  # (velocity, rel, min_size) run on tensors too
THRESHOLD = {3: 2.125, 2: 1.5}  # the explicit threshold=: near rel's 80th percentile, exact in float32
BINS = {"vx": np.linspace(-1.0, 1.0, 5), "vz": np.linspace(-3.0, 3.0, 4), "magnitude": np.linspace(0.0, 3.0, 6),
        "theta": np.linspace(-np.pi, np.pi, 9), "phi": np.linspace(-np.pi / 2, np.pi / 2, 7)}
WEIGHTED_BINS = {"vy": np.linspace(-1.0, 1.0, 6), "phi": np.linspace(-np.pi / 2, np.pi / 2, 5)}
AXIS_BINS = {"axis1": np.linspace(-2.0, 2.0, 5), "axis3": np.linspace(-3.0, 3.0, 4)}
PAIR_BINS = {"cosine": np.linspace(-1.0001, 1.0001, 7), "dmagnitude": np.linspace(-1.0, 1.0, 4)}
CONTRACT_BINS = {"angle": np.linspace(0.0, 180.0, 7), "inward": np.linspace(-1.0, 1.0, 4)}
CONTRACT_CENTER = (20.5, 11.25, 1.5)  # x y z, box-local (2D: x y)
QUIVER = dict(gap=(2, 3, 2), max_vectors=16)  # gz gy gx (2D: gy gx = 3 2)
EDGES = np.linspace(0.0, 4.0, 9)  # reliability_profile's given edges
STREAM_FRAMES = 2


def flatten(obj, path, out):
    """obj (a dict, list, tensor, array, scalar or a `mask` function beside `rois`) into out[path]."""
    if isinstance(obj, dict):
        for k, v in obj.items():
            if callable(v):
                v = [v(r) for r in range(len(obj["rois"]))]
            flatten(v, f"{path}/{k}", out)
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            flatten(v, f"{path}/{i}", out)
    else:
        assert path not in out, path
        out[path] = np.array(obj.cpu().numpy() if hasattr(obj, "cpu") else obj)


def pack(arrays):
    """path -> array as the four arrays of the file."""
    paths = sorted(arrays)
    return {"paths": np.array(paths), "dtypes": np.array([arrays[p].dtype.str for p in paths]),
            "shapes": np.array([",".join(str(n) for n in arrays[p].shape) for p in paths]),
            "data": np.frombuffer(b"".join(np.ascontiguousarray(arrays[p]).tobytes() for p in paths), dtype=np.uint8)}


def unpack(f):
    """The file's four arrays (an open npz) as path -> array."""
    out, data, off = {}, f["data"], 0
    for p, dt, shape in zip(f["paths"], f["dtypes"], f["shapes"]):
        dt, shape = np.dtype(str(dt)), tuple(int(n) for n in str(shape).split(",") if n)
        n = dt.itemsize * int(np.prod(shape, dtype=np.int64))
        out[str(p)] = data[off:off + n].view(dt).reshape(shape).copy()
        off += n
    assert off == data.size
    return out


def entries(out, tag, ch0, ch1, nd, box, min_size, source, rel_only):
    """Every public entry on the channels ch0 / ch1 ((vx, vy, vz or None, rel), numpy or CUDA), the
    threshold from `source` ("plain" / "box" / "given"); rel_only: the entries of rel alone too."""
    from opticalflow3d_dev_amd import analysis as an

    pick = lambda d: {k: e for k, e in d.items() if nd == 3 or k not in ("vz", "phi", "axis3")}
    rois = [box]
    pct = dict(rel_percentile=80)
    if source == "box":
        pct = dict(rel_percentile=85, percentile_box=box, percentile_method="hazen")
    thr = dict(pct, threshold=THRESHOLD[nd]) if source == "given" else pct
    centre = SPREAD_CENTER if nd == 3 else SPREAD_CENTER[:2] + SPREAD_CENTER[3:]
    extra = {"plain": dict(axes="mask", axis_bins=pick(AXIS_BINS), weighted_bins=pick(WEIGHTED_BINS)),
             "box": dict(spread="mean", rel_profile=an.RelProfileSpec(percentiles=(85, 90), bins=8)),
             "given": dict(spread=centre, axes=GIVEN_AXES, axes_physical=True)}[source]
    flatten(an.flow_summary(*ch0, rois=rois, bins=pick(BINS), min_size=min_size, **SCALES, **pct, **extra),
            f"{tag}/flow_summary", out)
    flatten(an.quiver_sample(*ch0, gap=QUIVER["gap"][3 - nd:], max_vectors=QUIVER["max_vectors"], rois=rois,
                             min_size=min_size, **SCALES, **thr), f"{tag}/quiver_sample", out)
    request = {"plain": an.FieldSpec(rois=(1,), fields=("vx", "rel"), mask="nan"),
               "box": an.FieldSpec(rois=(1,), fields=("vy",), mask="summary", dtype="float32"),
               "given": an.FieldSpec(rois=(1,), fields=("vz",) if nd == 3 else ("vx",), mask="zero", physical=False)}
    flatten(an.export_fields(*ch0, rois=rois, spec=request[source], min_size=min_size, **SCALES, **thr),
            f"{tag}/export_fields", out)
    if not min_size:
        spec = an.ContractSpec(bins=CONTRACT_BINS) if source == "plain" else an.ContractSpec(
            mask="summary", center=CONTRACT_CENTER[:nd])
        flatten(an.contractility(*ch0, rois=rois, spec=spec, **SCALES, **pct), f"{tag}/contractility", out)
    flatten(an.channel_compare(ch0, ch1, rois=rois, bins=PAIR_BINS, floor=0.9, min_size=max(min_size, 1),
                               combine="and" if source == "box" else "or", in_plane=source == "given", **SCALES,
                               **pct), f"{tag}/channel_compare", out)
    if not rel_only:
        return
    rel0, rel1 = ch0[3], ch1[3]
    flatten(an.reliability_mask(rel0, min_size=max(min_size, 1), rois=rois, **thr), f"{tag}/reliability_mask", out)
    if not min_size:
        flatten(an.largest_component_mask(rel0, rois=rois, **thr), f"{tag}/largest_component_mask", out)
    flatten(an.principal_axes(rel0, min_size=min_size, rois=rois, physical=source != "plain", xyscale=0.4, zscale=1.5,
                              **thr), f"{tag}/principal_axes", out)
    sel = dict(box=box, method="hazen") if source == "box" else {}
    hist = dict(edges=EDGES) if source == "given" else dict(bins=8)
    flatten(an.reliability_profile(rel0, rois=rois, **sel, **hist), f"{tag}/reliability_profile", out)
    two = dict(thresholds=(THRESHOLD[nd], THRESHOLD[nd] - 0.25)) if source == "given" else {}
    flatten(an.joint_reliability_mask(rel0, rel1, floor=0.9, combine="and" if source == "box" else "or",
                                      min_size=max(min_size, 1), rois=rois, **pct, **two),
            f"{tag}/joint_reliability_mask", out)
    if not isinstance(rel0, np.ndarray):
        flatten(an.reliability_thresholds(rel0, [10, 50, 90], **sel), f"{tag}/reliability_thresholds", out)


def streams(out):
    """Two frames each of a 3D fp64 and a 2D fp32 FlowStream with every add-on."""
    from opticalflow3d_dev_amd import analysis as an
    from opticalflow3d_dev_amd.stream import FlowStream

    runs = {
        "a": dict(precision="fp64", summary=an.SummarySpec(
            rois=[CASES["a"][1]], bins={"magnitude": BINS["magnitude"]}, rel_percentile=85, min_size=3,
            percentile_box=CASES["a"][1], percentile_method="hazen", spread="mean", axes="mask",
            weighted_bins=WEIGHTED_BINS, rel_profile=an.RelProfileSpec(percentiles=(85, 90), bins=8), **SCALES),
            quiver=an.QuiverSpec(**QUIVER), contract=an.ContractSpec(bins=CONTRACT_BINS),
            fields=an.FieldSpec(rois=(1,), mask="nan")),
        "c": dict(precision="fp32", summary=an.SummarySpec(rois=[CASES["c"][1]], rel_percentile=80, **SCALES),
                  quiver=an.QuiverSpec(gap=QUIVER["gap"][1:], max_vectors=QUIVER["max_vectors"]),
                  contract=an.ContractSpec(mask="summary", center=CONTRACT_CENTER[:2]),
                  fields=an.FieldSpec(rois=(1,), fields=("vx", "rel"), mask="summary"))}
    for case, kw in runs.items():
        shape = CASES[case][0]
        fs = FlowStream(len(shape), shape, np.uint16, 1, 1, 1, depth=2, **kw)
        series = np.random.default_rng([SEED, 7, len(shape)]).integers(
            0, 4096, size=(fs.nwin + STREAM_FRAMES - 1,) + shape).astype(np.uint16)
        pushed = 0
        try:
            for i in range(STREAM_FRAMES):
                while pushed < min(i + fs.nwin + fs.lookahead, len(series)):
                    fs.push(series[pushed])
                    pushed += 1
                p = fs.submit()
                for name in ("summary", "quiver", "contract", "fields"):
                    flatten(getattr(p, name)(), f"stream/{case}/{i}/{name}", out)
                p.release()
        finally:
            fs.close()


def generate():
    """path -> array of every run; needs a GPU."""
    import torch

    dev = torch.device("cuda", 0)
    out = {}
    for case, (shape, box) in CASES.items():
        rng = np.random.default_rng([SEED, len(shape), shape[-2]])
        host = fields(shape, rng), fields(shape, rng)
        nd = len(shape)
        for vdt, rdt in DTYPES:
            cast = [[None if a is None else np.ascontiguousarray(a.astype(rdt if i == 3 else vdt))
                     for i, a in enumerate(ch)] for ch in host]
            for min_size in (0, 3):
                kinds = [("numpy", cast)]
                if (vdt, rdt, min_size) in TORCH_RUNS:
                    kinds.append(("torch", [[None if a is None else torch.as_tensor(a).to(dev) for a in ch]
                                            for ch in cast]))
                for kind, (ch0, ch1) in kinds:
                    source = "given" if kind == "torch" else "box" if min_size else "plain"
                    tag = f"{case}/v{np.dtype(vdt).itemsize * 8}r{np.dtype(rdt).itemsize * 8}/m{min_size}/{kind}"
                    entries(out, tag, ch0, ch1, nd, box, min_size, source, vdt == np.float64 or kind == "torch")
    streams(out)
    return out


def error_strings():
    """The error table of tests/test_gpu_analysis_dicts.py as name -> "Type: message"."""
    tests = os.path.join(os.path.dirname(HERE), "tests")
    sys.path.insert(0, tests)
    spec = importlib.util.spec_from_file_location("test_gpu_analysis_dicts",
                                                  os.path.join(tests, "test_gpu_analysis_dicts.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return {name: module.raised(call) for name, call in module.error_cases().items()}


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", default="", help="recorded in the file: the commit the package was taken from")
    args = ap.parse_args()
    arrays = generate()
    for name, text in error_strings().items():
        arrays["error/" + name] = np.array(text)
    packed = pack(arrays)
    packed["meta_commit"] = np.array(args.commit)
    packed["meta_rocm"] = np.array(str(torch.version.hip))
    packed["meta_device"] = np.array(torch.cuda.get_device_name(0))
    packed["meta_numpy"] = np.array(np.__version__)
    np.savez_compressed(args.out, **packed)
    print(f"{len(arrays)} arrays, {packed['data'].size} bytes -> {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
