"""Device-side magnitude-weighted histograms: what they cost.

On the resident outputs of one FlowStream step of --config (default c3, 512x512x128), 90th
percentile, whole volume; device events over --iters calls after 3 warm-ups, the routes
alternating:

  a  the host route the feature replaces: the three fields and rel device -> host, numpy
     masking (the threshold taken from the device), np.histogram(phi, weights=magnitude)
  b  of3d_flow_whist for phi alone, 36 bins (the threshold already on the device)
  c  of3d_flow_whist for all six quantities, 36 bins each (six passes over the fields)
  d  the same run's device-to-device copy rate, for the byte floor: a requested quantity's
     pass reads the three fields and rel, 28 B per voxel in fp64 with a float32 rel

and the results of (a) and (b) compared.  One JSON line per figure.
"""

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from summary_bench import SCALES, emit, event_ms, resident_fields  # noqa: E402

from bench import CONFIGS  # noqa: E402
from opticalflow3d_dev_amd import SummarySpec  # noqa: E402
from opticalflow3d_dev_amd.analysis import QUANTITIES, _SummaryCall, _WhistCall  # noqa: E402


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(CONFIGS))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=20, help="calls of the host route (about a second each at c3)")
    args = ap.parse_args()

    fs, (vx, vy, vz, rel) = resident_fields(args.config)
    nvox, dims = rel.numel(), tuple(rel.shape)
    stream = torch.cuda.current_stream().cuda_stream
    phi_edges = np.linspace(-np.pi / 2, np.pi / 2, 37)
    six = {"vx": np.linspace(-0.05, 0.05, 37), "vy": np.linspace(-0.05, 0.05, 37), "vz": np.linspace(-0.05, 0.05, 37),
           "magnitude": np.linspace(0.0, 0.1, 37), "theta": np.linspace(-np.pi, np.pi, 37), "phi": phi_edges}
    spec = SummarySpec(weighted_bins={"phi": phi_edges}, **SCALES)
    call = _SummaryCall(spec, dims, rel.dtype, rel.device)
    res = call.new_result(rel.device)
    call.enqueue((vx.data_ptr(), vy.data_ptr(), vz.data_ptr(), rel.data_ptr(), vx.dtype == torch.float32),
                 res.data_ptr(), stream)  # leaves the threshold on the device
    summary = call.decode(res.cpu().numpy())
    thresh, one = call.thresh, call.whist
    scales = (spec.xyscale, spec.zscale, spec.tscale)
    all_spec = SummarySpec(weighted_bins=six)
    allq = _WhistCall(call.boxes, dims, call.rel_f64, *all_spec.weighted(3), scales, rel.device)
    out_one = torch.empty(one.result_bytes // 8, dtype=torch.int64, device=rel.device)
    out_all = torch.empty(allq.result_bytes // 8, dtype=torch.int64, device=rel.device)
    v_f32 = vx.dtype == torch.float32
    run = lambda c, out: c.enqueue((vx.data_ptr(), vy.data_ptr(), vz.data_ptr(), rel.data_ptr(), v_f32),
                                   thresh.data_ptr(), None, out.data_ptr(), stream)
    route_b, route_c = (lambda: run(one, out_one)), (lambda: run(allq, out_all))
    host = {}

    def route_a():
        t = thresh.cpu().numpy()[0]
        r = rel.cpu().numpy()
        f = [a.cpu().numpy() for a in (vx, vy, vz)]
        m = r > t  # the valid voxels alone go through the arithmetic: what a careful script does
        x, y, z = (a[m].astype(np.float64) for a in f)
        ok = (x != 0) & (y != 0) & (z != 0)  # v * mask == 0 -> NaN -> not valid
        x, y, z = x[ok] * spec.xyscale / spec.tscale, y[ok] * spec.xyscale / spec.tscale, z[ok] * spec.zscale / spec.tscale
        xy2 = x * x + y * y
        mag, phi = np.sqrt(xy2 + z * z), np.arctan(z / np.sqrt(xy2))
        host.update(n_valid=int(mag.size), hist=np.histogram(phi, bins=phi_edges, weights=mag)[0],
                    total=float(mag.sum()))

    route_a()
    dev = summary["hist_weighted"]["phi"][0]
    emit(name="routes_agree", config=args.config, n_valid=int(summary["n_valid"][0]),
         n_valid_equal=bool(host["n_valid"] == int(summary["n_valid"][0])),
         max_rel_diff=float(np.max(np.abs(dev - host["hist"]) / np.maximum(np.abs(host["hist"]), 1e-300))),
         device_total=float(dev.sum()), host_total=host["total"], sum_magnitude=float(summary["sum_magnitude"][0]))

    src = torch.empty(1 << 28, dtype=torch.float32, device=rel.device).normal_()  # 1 GiB
    dst = torch.empty_like(src)
    tb, tc, td = event_ms(torch, [route_b, route_c, lambda: dst.copy_(src)], args.iters)
    (ta,) = event_ms(torch, [route_a], args.host_iters, warmup=1)
    copy_tbs = 2 * src.numel() * 4 / (td[0] * 1e-3) / 1e12
    pass_bytes = nvox * (3 * vx.element_size() + rel.element_size())
    floor = pass_bytes / (copy_tbs * 1e12) * 1e3
    emit(name="d_copy_bandwidth", tb_per_s=round(copy_tbs, 3), ms=round(td[0], 4), bytes=2 * src.numel() * 4)
    emit(name="a_host_route", config=args.config, iters=args.host_iters, ms_median=round(ta[0], 3), ms_min=round(ta[1], 3))
    emit(name="b_whist_phi", config=args.config, iters=args.iters, bins=36, ms_median=round(tb[0], 4),
         ms_min=round(tb[1], 4), bytes_per_voxel=pass_bytes / nvox, floor_ms=round(floor, 4),
         over_floor=round(tb[0] / floor, 2), workspace_bytes=int(one.ws.numel()))
    emit(name="c_whist_six", config=args.config, iters=args.iters, quantities=list(QUANTITIES), bins=36,
         ms_median=round(tc[0], 4), ms_min=round(tc[1], 4), floor_ms=round(6 * floor, 4),
         over_floor=round(tc[0] / (6 * floor), 2), workspace_bytes=int(allq.ws.numel()))
    emit(name="b_over_a", ratio=round(tb[0] / ta[0], 6), speedup=round(ta[0] / tb[0], 1))
    fs.close()


if __name__ == "__main__":
    main()
