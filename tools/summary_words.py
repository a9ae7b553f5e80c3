"""The raw result words of every device-side summary pass, for a byte-for-byte comparison of two
builds.

The summary passes are tested against CPU references at a relative tolerance, which a change of
the summation order would pass.  This tool runs of3d_flow_summary (plain and masked, with the
of3d_mask_axes and of3d_flow_whist blocks), of3d_mask_axes alone, of3d_mask_open,
of3d_mask_open_pair and of3d_flow_pair on small seeded fields through the `_*Call` classes of
analysis.py and writes the int64 result words and the uint16 keep volumes, untouched, to one
.npz.  Two builds of the library agree when every array of their files is byte-equal
(tests/test_gpu_summary_words.py holds one build's file to the committed one).

Cases (all with ROI 0, the whole volume, and one interior box):
  a  (5, 37, 67)    2 workgroups for the volume; 185 rows do not divide by 2, 67 does not divide
                    512, a ragged tail
  b  (9, 61, 131)   9 workgroups
  c  (37, 67)       2D, one workgroup
each with velocities float64 / float32 x rel float32 / float64, unmasked and opened (min_size 3),
all six quantities binned plain (two edge uploads: more than 384 edges) and weighted, the three
axis histograms with axes="mask" and with a given 3x3, and the pair pass in 3D and in-plane with
both `combine` values.  Zeros and NaNs are planted in the velocities.

The later passes ride on the same cases and dtype pairs through `_SummaryCall(spec, quiver=,
contract=)` with `SummarySpec(spread=)`, unmasked and opened: of3d_flow_spread about the box mean
and about a given centre; of3d_quiver_sample with gap 1 and with an anisotropic gap, at a capacity
that truncates the volume's list but not the box's (QUIVER_MAX); of3d_flow_contract over the summary's mask
and (unmasked summary only) over of3d_mask_largest's, about the mask's centroid and a given
centre, both histograms binned, with of3d_mask_largest's keep volume.  The quiver's and the
contract's result tensors are zeroed first: the kernels leave the records past n_stored alone.

    python tools/summary_words.py --out words.npz [--commit ID] [--skip b] [--beside old.npz]
"""

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEED = 20240611
CASES = {"a": ((5, 37, 67), (1, 4, 3, 30, 5, 66)), "b": ((9, 61, 131), (2, 9, 0, 47, 17, 130)),
         "c": ((37, 67), (3, 30, 5, 66))}
SCALES = dict(xyscale=0.4, zscale=1.5, tscale=2.0)
GIVEN_AXES = ((0.6, 0.8, 0.0), (-0.8, 0.6, 0.0), (0.0, 0.0, 1.0))
BINS = {"vx": np.linspace(-1.0, 1.0, 12), "vy": np.linspace(-1.0, 1.0, 14), "vz": np.linspace(-3.0, 3.0, 12),
        "magnitude": np.linspace(0.0, 3.0, 17), "theta": np.linspace(-np.pi, np.pi, 201),
        "phi": np.linspace(-np.pi / 2, np.pi / 2, 191)}
WEIGHTED_BINS = {"vx": np.linspace(-0.5, 1.5, 9), "vy": np.linspace(-1.0, 1.0, 6), "vz": np.linspace(-2.0, 3.0, 8),
                 "magnitude": np.linspace(0.0, 2.0, 11), "theta": np.linspace(-np.pi, np.pi, 37),
                 "phi": np.linspace(-np.pi / 2, np.pi / 2, 19)}
AXIS_BINS = {"axis1": np.linspace(-2.0, 2.0, 21), "axis2": np.linspace(-1.0, 1.0, 11),
             "axis3": np.linspace(-3.0, 3.0, 16)}
PAIR_BINS = {"dot": np.linspace(-1.0, 1.0, 21), "cosine": np.linspace(-1.0001, 1.0001, 37),
             "dtheta": np.linspace(-np.pi, np.pi, 37), "dmagnitude": np.linspace(-1.0, 1.0, 12)}
CONTRACT_BINS = {"angle": np.linspace(0.0, 180.0, 19), "inward": np.linspace(-1.0, 1.0, 12)}
SPREAD_CENTER = (0.1, -0.2, 0.3, 0.5)  # vx vy vz magnitude (2D: without vz)
CONTRACT_CENTER = (20.5, 11.25, 1.5)   # x y z, box-local (2D: x y)
QUIVER_GAP = (2, 3, 2)                 # gz gy gx (2D: gy gx = 3 2)
# max_vectors at gap 1 and at QUIVER_GAP.  In QUIVER_SPLIT's run the capacity lies between the valid lattice
# points of the interior box and of the volume, so the volume's list truncates and the box's does
# not: a and c at gap 1 (a 865 / 2134, past the volume's first workgroup; c 268 / 438 unmasked,
# opened a few less), b at QUIVER_GAP (645 / 1147).  b at gap 1 (nine workgroups, 6485 / 12330)
# truncates both: a record is four incompressible words and the file has 1 MiB.
QUIVER_MAX = {"a": (1200, 65536), "b": (600, 900), "c": (320, 65536)}
QUIVER_SPLIT = {"a": "g1", "b": "aniso", "c": "g1"}  # where one list truncates and the other does not


def fields(shape, rng):
    """One channel (vx, vy, vz or None, rel) of float64 arrays: normal velocities with exact zeros
    and NaNs planted, a smooth positive rel so that the mask has components of many sizes."""
    v = [rng.normal(0.0, 2.0, shape) for _ in range(len(shape))]
    for a in v:
        a[rng.random(shape) < 0.03] = 0.0
        a[rng.random(shape) < 0.02] = np.nan
    rel = rng.random(shape)
    for ax in range(len(shape)):
        rel = rel + 0.5 * np.roll(rel, 1, axis=ax)
    vx, vy = v[0], v[1]
    return [vx, vy, v[2] if len(shape) == 3 else None, rel]


def generate(skip=()):
    """name -> array of every case; needs a GPU."""
    import torch

    from opticalflow3d_dev_amd.analysis import (ContractSpec, QuiverSpec, SummarySpec, _AxesCall, _PairCall,
                                                _SummaryCall)

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    out = {}
    up = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a.astype(dt))).to(dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    for case, (shape, box) in CASES.items():
        if case in skip:
            continue
        rng = np.random.default_rng([SEED, len(shape), shape[-2]])
        ch0, ch1 = fields(shape, rng), fields(shape, rng)
        nd = len(shape)
        pick = lambda d: {k: e for k, e in d.items() if nd == 3 or k not in ("vz", "phi", "axis3")}
        for vdt, rdt in ((np.float64, np.float32), (np.float32, np.float32), (np.float64, np.float64),
                         (np.float32, np.float64)):
            tag = f"{case}/v{np.dtype(vdt).itemsize * 8}r{np.dtype(rdt).itemsize * 8}"
            t0 = [up(a, vdt) for a in ch0[:3]] + [up(ch0[3], rdt)]
            t1 = [up(a, vdt) for a in ch1[:3]] + [up(ch1[3], rdt)]
            v_f32 = vdt == np.float32
            for min_size in (0, 3):
                for axes_name, axes in (("mask", "mask"), ("given", GIVEN_AXES)):
                    spec = SummarySpec(rois=[box], bins=pick(BINS), rel_percentile=80, min_size=min_size, axes=axes,
                                       axes_physical=axes_name == "given", axis_bins=pick(AXIS_BINS),
                                       weighted_bins=pick(WEIGHTED_BINS), **SCALES)
                    call = _SummaryCall(spec, shape, t0[3].dtype, dev)
                    res = call.new_result(dev)
                    call.enqueue((ptr(t0[0]), ptr(t0[1]), ptr(t0[2]), ptr(t0[3]), v_f32), res.data_ptr(), stream)
                    out[f"{tag}/summary/m{min_size}/{axes_name}"] = res.cpu().numpy()
                    if min_size and axes_name == "mask" and not v_f32:
                        out[f"{case}/r{np.dtype(rdt).itemsize * 8}/keep"] = call.open.keep.cpu().numpy()
                        # the mask's part of of3d_mask_axes alone (principal_axes' call): no fields
                        alone = _AxesCall(call.boxes, call.dims, call.rel_f64,
                                          SummarySpec(axes="mask").axes_request(nd), True, (0.4, 1.5, 1.0), dev)
                        ares = torch.empty(alone.result_bytes // 8, dtype=torch.int64, device=dev)
                        alone.enqueue((None, None, None, ptr(t0[3]), 0), call.thresh.data_ptr(),
                                      call.open.keep.data_ptr(), ares.data_ptr(), stream)
                        out[f"{case}/r{np.dtype(rdt).itemsize * 8}/axes_alone"] = ares.cpu().numpy()
            # spread, quiver and contract: (spread, quiver, contract mask, contract centre) per run
            runs = [("mean", "g1", "summary", "mask"), ("given", "aniso", "summary", "given")]
            for min_size in (0, 3):
                for sp, qv, cmask, centre in runs + ([(None, None, "largest", "mask"),
                                                      (None, None, "largest", "given")] if not min_size else []):
                    given = SPREAD_CENTER if nd == 3 else SPREAD_CENTER[:2] + SPREAD_CENTER[3:]
                    spread = None if sp is None else "mean" if sp == "mean" else given
                    quiver = None if qv is None else (QuiverSpec(gap=1, max_vectors=QUIVER_MAX[case][0]) if qv == "g1"
                                                      else QuiverSpec(gap=QUIVER_GAP[3 - nd:],
                                                                      max_vectors=QUIVER_MAX[case][1]))
                    contract = ContractSpec(mask=cmask, center="mask" if centre == "mask" else CONTRACT_CENTER[:nd],
                                            bins=CONTRACT_BINS)
                    spec = SummarySpec(rois=[box], rel_percentile=80, min_size=min_size, spread=spread, **SCALES)
                    call = _SummaryCall(spec, shape, t0[3].dtype, dev, quiver=quiver, contract=contract)
                    res = call.new_result(dev)
                    qres = None if quiver is None else torch.zeros_like(call.quiver.new_result(dev))
                    cres = torch.zeros_like(call.contract.new_result(dev))
                    blocks = {"contract": cres.data_ptr()} | ({} if quiver is None else {"quiver": qres.data_ptr()})
                    call.enqueue((ptr(t0[0]), ptr(t0[1]), ptr(t0[2]), ptr(t0[3]), v_f32), res.data_ptr(), stream, blocks)
                    out[f"{tag}/contract/{cmask}/m{min_size}/{centre}"] = cres.cpu().numpy()
                    if spread is not None:
                        out[f"{tag}/spread/m{min_size}/{sp}"] = res[call.spread_off // 8:].cpu().numpy()
                    if quiver is not None:
                        words = out[f"{tag}/quiver/m{min_size}/{qv}"] = qres.cpu().numpy()
                        if qv == QUIVER_SPLIT[case]:  # n_valid against the capacity: the volume truncates, the box does not
                            assert words[7] > call.quiver.capacity[0] and words[11] <= call.quiver.capacity[1], words[:14]
                    if cmask == "largest" and centre == "mask" and not v_f32:
                        out[f"{case}/r{np.dtype(rdt).itemsize * 8}/largest_keep"] = call.contract.largest.keep.cpu().numpy()
            for combine in ("or", "and"):
                for in_plane in ((False, True) if nd == 3 else (True,)):
                    call = _PairCall(shape, t0[3].dtype, dev, rel_percentile=70, rois=[box], bins=PAIR_BINS, floor=0.9,
                                     combine=combine, min_size=3, **SCALES)
                    p0 = (ptr(t0[0]), ptr(t0[1]), None if in_plane else ptr(t0[2]), ptr(t0[3]))
                    p1 = (ptr(t1[0]), ptr(t1[1]), None if in_plane else ptr(t1[2]), ptr(t1[3]))
                    res = call.enqueue(p0, p1, v_f32, stream)
                    out[f"{tag}/pair/{combine}/{'plane' if in_plane else 'full'}"] = res.cpu().numpy()
                    if not v_f32 and in_plane == (nd == 2):
                        out[f"{case}/r{np.dtype(rdt).itemsize * 8}/pair_keep/{combine}"] = call.keep.cpu().numpy()
    return out


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", default="", help="recorded in the file: the commit the library was built from")
    ap.add_argument("--skip", default="", help="comma-separated cases to leave out (a, b, c)")
    ap.add_argument("--beside", default="", help="an earlier file: write only the arrays it does not hold")
    args = ap.parse_args()
    arrays = generate(tuple(s for s in args.skip.split(",") if s))
    if args.beside:
        with np.load(args.beside) as f:
            arrays = {k: a for k, a in arrays.items() if k not in f.files}
    arrays["meta_commit"] = np.array(args.commit)
    arrays["meta_rocm"] = np.array(str(torch.version.hip))
    arrays["meta_device"] = np.array(torch.cuda.get_device_name(0))
    np.savez_compressed(args.out, **arrays)
    print(f"{len(arrays)} arrays, {sum(a.nbytes for a in arrays.values())} bytes -> {args.out} "
          f"({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
