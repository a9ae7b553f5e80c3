"""Device-side contractility: what it costs.

On the resident outputs of one FlowStream step of --config (default c3, 512x512x128), 90th
percentile, connectivity 26, whole volume; device events over --iters calls after 3 warm-ups, the
routes alternating:

  a  the host route the feature replaces: fields and rel device -> host, scipy.ndimage.label,
     the largest component, center_of_mass, the notebook's numpy angle
  b  select + of3d_mask_largest + of3d_flow_contract, with and without the two histograms; and
     of3d_mask_largest and of3d_flow_contract (given the keep volume) alone
  c  of3d_mask_open at min_size 1000 in the same run: the yardstick of the labelling part, which
     of3d_mask_largest shares but for its selection phase
  d  the same run's device-to-device copy rate and the byte floor of the reduction pass: per
     voxel the three velocity fields and the mask source read once — 26 B with a keep volume
     (fp64 fields), 28 B with a float32 rel; the moment pass's own read of the mask is left out

and the counts and the centroid of (a) and (b) compared.  One JSON line per figure.
"""

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from summary_bench import SCALES, emit, event_ms, resident_fields  # noqa: E402

from bench import CONFIGS  # noqa: E402
from opticalflow3d_dev_amd import ContractSpec  # noqa: E402
from opticalflow3d_dev_amd.analysis import _ContractCall, _OpenCall, percentile_threshold_device  # noqa: E402

BINS = {"angle": np.linspace(0.0, 180.0, 37), "inward": np.linspace(-2.0, 2.0, 257)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(CONFIGS))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=20, help="calls of the host route (seconds each at c3)")
    args = ap.parse_args()

    import torch
    from scipy import ndimage

    fs, (vx, vy, vz, rel) = resident_fields(args.config)
    nvox, dims = rel.numel(), tuple(rel.shape)
    stream = torch.cuda.current_stream().cuda_stream
    boxes = np.array([(0, dims[0], 0, dims[1], 0, dims[2])], dtype=np.int64)
    scales = tuple(SCALES.values())
    rel_f64 = rel.dtype == torch.float64
    thresh = torch.empty(1, dtype=rel.dtype, device=rel.device)
    select = lambda: percentile_threshold_device(rel, 90, out=thresh)
    select()
    calls = {name: _ContractCall(boxes, dims, rel_f64, ContractSpec(bins=bins), 3, scales, rel.device)
             for name, bins in (("hist", BINS), ("plain", None))}
    results = {name: c.new_result(rel.device) for name, c in calls.items()}
    ptrs = (vx.data_ptr(), vy.data_ptr(), vz.data_ptr(), rel.data_ptr(), vx.dtype == torch.float32)

    def route_b(name):
        select()
        calls[name].enqueue(ptrs, thresh.data_ptr(), None, results[name].data_ptr(), stream)

    hist = calls["hist"]
    counts = torch.empty((1, 4), dtype=torch.int64, device=rel.device)
    run_largest = lambda: hist.largest.enqueue(rel.data_ptr(), thresh.data_ptr(), counts.data_ptr(), stream)
    lib = hist.lib
    run_reduce = lambda: lib.of3d_flow_contract(*ptrs[:4], int(ptrs[4]), hist.rel_f64, *dims, thresh.data_ptr(), *scales,
                                                hist.roi_arr, 1, hist.largest.keep.data_ptr(), None, hist.nb_arr,
                                                hist.edge_arr, results["hist"].data_ptr(), hist.ws.data_ptr(), stream)
    oc = _OpenCall(boxes, dims, rel_f64, 1000, 26, rel.device)
    run_open = lambda: oc.enqueue(rel.data_ptr(), thresh.data_ptr(), counts.data_ptr(), stream)

    host = {}

    def route_a():
        fx, fy, fz, r = (a.cpu().numpy() for a in (vx, vy, vz, rel))
        t = np.percentile(r, 90)
        lab, n = ndimage.label(r > t, ndimage.generate_binary_structure(3, 3))
        sizes = np.bincount(lab.ravel(), minlength=n + 1)
        sizes[0] = 0
        m = lab == int(np.argmax(sizes)) if n else np.zeros(lab.shape, bool)
        com = ndimage.center_of_mass(m)
        with np.errstate(invalid="ignore", divide="ignore"):
            v = []
            for f, s in ((fx, SCALES["xyscale"]), (fy, SCALES["xyscale"]), (fz, SCALES["zscale"])):
                f = f * m
                f[f == 0] = np.nan
                v.append(f * s / SCALES["tscale"])
            speed = np.sqrt(np.power(v[0], 2) + np.power(v[1], 2) + np.power(v[2], 2))
            kz, ky, kx = np.meshgrid(*(np.arange(d, dtype=np.float64) for d in dims), indexing="ij", sparse=True)
            d = [kx * SCALES["xyscale"] - com[2] * SCALES["xyscale"], ky * SCALES["xyscale"] - com[1] * SCALES["xyscale"],
                 kz * SCALES["zscale"] - com[0] * SCALES["zscale"]]
            nd = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            dot = ((v[0] / speed) * (-d[0] / nd) + (v[1] / speed) * (-d[1] / nd)) + (v[2] / speed) * (-d[2] / nd)
            angle = np.degrees(np.arccos(dot))
        host.update(n_mask=int((lab > 0).sum()), n_components=int(n), n_kept=int(m.sum()), centroid=[com[2], com[1], com[0]],
                    n_angle=int((~np.isnan(angle)).sum()), mean_angle=float(np.nanmean(angle)))

    route_a()
    route_b("hist")
    dev = hist.decode(results["hist"].cpu().numpy())
    emit(name="routes_agree", config=args.config,
         device={k: int(dev[k][0]) for k in ("n_mask", "n_components", "n_kept", "n_angle")} |
         {"centroid": dev["centroid"][0].tolist(), "mean_angle": float(dev["mean_angle"][0])}, host=host)

    src = torch.empty(1 << 28, dtype=torch.float32, device=rel.device).normal_()  # 1 GiB
    dst = torch.empty_like(src)
    fns = [lambda: route_b("hist"), lambda: route_b("plain"), run_largest, run_reduce, run_open, lambda: dst.copy_(src)]
    tbh, tbp, tl, tr, to, tc = event_ms(torch, fns, args.iters)
    (ta,) = event_ms(torch, [route_a], args.host_iters, warmup=1)
    copy_tbs = 2 * src.numel() * 4 / (tc[0] * 1e-3) / 1e12
    per_voxel = 3 * vx.element_size() + 2  # the reduction pass with a keep volume
    floor_ms = nvox * per_voxel / (copy_tbs * 1e12) * 1e3
    emit(name="copy_bandwidth", tb_per_s=round(copy_tbs, 3), ms=round(tc[0], 4), bytes=2 * src.numel() * 4)
    emit(name="a_host_route", config=args.config, iters=args.host_iters, ms_median=round(ta[0], 3), ms_min=round(ta[1], 3))
    for name, t in (("b_select_largest_contract_hist", tbh), ("b_select_largest_contract", tbp),
                    ("b_mask_largest", tl), ("b_flow_contract_keep_hist", tr), ("c_mask_open_1000", to)):
        emit(name=name, config=args.config, iters=args.iters, ms_median=round(t[0], 4), ms_min=round(t[1], 4))
    emit(name="b_over_a", ratio=round(tbh[0] / ta[0], 6), speedup=round(ta[0] / tbh[0], 1))
    emit(name="largest_over_open", ratio=round(tl[0] / to[0], 3))
    emit(name="d_reduce_vs_byte_floor", bytes_per_voxel=per_voxel, floor_ms=round(floor_ms, 4),
         reduce_over_floor=round(tr[0] / floor_ms, 2))
    fs.close()


if __name__ == "__main__":
    main()
