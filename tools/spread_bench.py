"""Device-side spread of the flow (std, covariance, circular std, extremes): what it costs
(DESIGN.md §8l).

On the resident outputs of one FlowStream step of --config (default c3, 512x512x128), 90th
percentile, whole volume (one box of 1024 workgroups); device events over --iters calls after 3
warm-ups, the routes alternating:

  a  the host route the feature replaces: the three fields and rel device -> host, numpy
     masking (the threshold taken from the device), np.std of vx, vy, vz and the speed, the
     circular std of theta and phi (the validation notebook's numbers)
  b  of3d_flow_spread alone about the box's mean (the summary's result already on the device),
     over the threshold mask: it reads the three fields and rel once, 28 B per voxel in fp64
     with a float32 rel
  c  the same over an opened mask (min_size 1): the three fields and the keep volume, 26 B
  d  the summary without and with spread=, whole calls (quantile, summary, spread)
  e  the same run's device-to-device copy rate, for the byte floors

and the results of (a) and (b) compared.  One JSON line per figure, on stdout and in --out
(default profiles/spread_bench_<config>.jsonl).
"""

import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from summary_bench import SCALES, event_ms, resident_fields  # noqa: E402

from bench import CONFIGS  # noqa: E402
from opticalflow3d_dev_amd import SummarySpec  # noqa: E402
from opticalflow3d_dev_amd.analysis import SPREAD_COMPONENTS, _OpenCall, _SummaryCall  # noqa: E402


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(CONFIGS))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=5, help="calls of the host route (seconds each at c3)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out_path = args.out or os.path.join(REPO, "profiles", f"spread_bench_{args.config}.jsonl")
    out_file = open(out_path, "w")

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        out_file.write(line + "\n")
        out_file.flush()

    fs, (vx, vy, vz, rel) = resident_fields(args.config)
    nvox, dims = rel.numel(), tuple(rel.shape)
    stream = torch.cuda.current_stream().cuda_stream
    v_f32 = vx.dtype == torch.float32
    ptrs = (vx.data_ptr(), vy.data_ptr(), vz.data_ptr(), rel.data_ptr(), v_f32)
    plain = _SummaryCall(SummarySpec(**SCALES), dims, rel.dtype, rel.device)
    call = _SummaryCall(SummarySpec(spread="mean", **SCALES), dims, rel.dtype, rel.device)
    res_plain, res = plain.new_result(rel.device), call.new_result(rel.device)
    call.enqueue(ptrs, res.data_ptr(), stream)  # leaves the threshold and the summary's words on the device
    summary = call.decode(res.cpu().numpy())
    thresh, spread = call.thresh, call.spread
    opening = _OpenCall(call.boxes, dims, call.rel_f64, 1, 26, rel.device)
    counts = torch.empty((len(call.boxes), 4), dtype=torch.int64, device=rel.device)
    opening.enqueue(rel.data_ptr(), thresh.data_ptr(), counts.data_ptr(), stream)

    def run(keep_ptr):  # into its own part of res, behind the summary's words it reads
        spread.enqueue(ptrs, thresh.data_ptr(), keep_ptr, res.data_ptr() + call.spread_off, stream)

    route_b, route_c = (lambda: run(None)), (lambda: run(opening.keep.data_ptr()))
    route_d0 = lambda: plain.enqueue(ptrs, res_plain.data_ptr(), stream)
    route_d1 = lambda: call.enqueue(ptrs, res.data_ptr(), stream)
    host = {}

    def route_a():
        t = thresh.cpu().numpy()[0]
        r = rel.cpu().numpy()
        f = [a.cpu().numpy() for a in (vx, vy, vz)]
        m = r > t  # the valid voxels alone go through the arithmetic: what a careful script does
        x, y, z = (a[m].astype(np.float64) for a in f)
        ok = (x != 0) & (y != 0) & (z != 0)  # v * mask == 0 -> NaN -> not valid
        s = SCALES
        x, y, z = (x[ok] * s["xyscale"] / s["tscale"], y[ok] * s["xyscale"] / s["tscale"],
                   z[ok] * s["zscale"] / s["tscale"])
        xy2 = x * x + y * y
        mag, theta, phi = np.sqrt(xy2 + z * z), np.arctan2(y, x), np.arctan(z / np.sqrt(xy2))
        circstd = lambda a: float(np.sqrt(-2 * np.log(np.hypot(np.sin(a).mean(), np.cos(a).mean()))))
        host.update(n_valid=int(mag.size), std=[float(np.std(a)) for a in (x, y, z, mag)],
                    theta_std=circstd(theta), phi_std=circstd(phi),
                    extremes=[float(v) for a in (x, y, z, mag) for v in (a.min(), a.max())])

    route_a()
    dev_std = [float(summary["std_" + k][0]) for k in SPREAD_COMPONENTS]
    dev_ext = [float(summary[m + k][0]) for k in SPREAD_COMPONENTS for m in ("min_", "max_")]
    emit(name="routes_agree", config=args.config, n_valid=int(summary["n_valid"][0]),
         n_valid_equal=bool(host["n_valid"] == int(summary["n_valid"][0])),
         std_max_rel_diff=float(np.max(np.abs(np.array(dev_std) - host["std"]) / np.array(host["std"]))),
         extremes_equal=bool(dev_ext == host["extremes"]),
         theta_std_diff=abs(float(summary["theta_std"][0]) - host["theta_std"]),
         phi_std_diff=abs(float(summary["phi_std"][0]) - host["phi_std"]), device_std=dev_std, host_std=host["std"])

    src = torch.empty(1 << 28, dtype=torch.float32, device=rel.device).normal_()  # 1 GiB
    dst = torch.empty_like(src)
    tb, tc, td0, td1, te = event_ms(torch, [route_b, route_c, route_d0, route_d1, lambda: dst.copy_(src)], args.iters)
    (ta,) = event_ms(torch, [route_a], args.host_iters, warmup=1)
    copy_tbs = 2 * src.numel() * 4 / (te[0] * 1e-3) / 1e12
    bytes_b = nvox * (3 * vx.element_size() + rel.element_size())
    bytes_c = nvox * (3 * vx.element_size() + 2)
    floor_b, floor_c = (b / (copy_tbs * 1e12) * 1e3 for b in (bytes_b, bytes_c))
    nb = -(-nvox // 8192)
    box = f"one box of {nvox} voxels, {min(nb, 1024)} workgroups"
    emit(name="e_copy_bandwidth", tb_per_s=round(copy_tbs, 3), ms=round(te[0], 4), bytes=2 * src.numel() * 4)
    emit(name="a_host_route", config=args.config, iters=args.host_iters, ms_median=round(ta[0], 3), ms_min=round(ta[1], 3))
    emit(name="b_spread_pass", config=args.config, box=box, iters=args.iters, ms_median=round(tb[0], 4),
         ms_min=round(tb[1], 4), bytes_per_voxel=bytes_b / nvox, floor_ms=round(floor_b, 4),
         over_floor=round(tb[0] / floor_b, 2), workspace_bytes=int(spread.ws.numel()))
    emit(name="c_spread_pass_keep", config=args.config, box=box, iters=args.iters, ms_median=round(tc[0], 4),
         ms_min=round(tc[1], 4), bytes_per_voxel=bytes_c / nvox, floor_ms=round(floor_c, 4),
         over_floor=round(tc[0] / floor_c, 2))
    emit(name="d_summary_calls", config=args.config, iters=args.iters, plain_ms_median=round(td0[0], 4),
         with_spread_ms_median=round(td1[0], 4), added_ms=round(td1[0] - td0[0], 4))
    emit(name="b_over_a", ratio=round(tb[0] / ta[0], 6), speedup=round(ta[0] / tb[0], 1))
    out_file.close()
    fs.close()


if __name__ == "__main__":
    main()
