"""Device-side two-channel comparison: what it costs.

On the resident outputs of one FlowStream step of --config (default c3, 512x512x128) as channel
0; channel 1 is channel 0's four fields rolled by (1, 3, 5) voxels (resident_fields makes one
synthetic series, so there is no second one to take).  80th percentile per channel, OR, floor 0,
min_size 1 (connectivity 26), whole volume; device events over --iters calls after 3 warm-ups,
the routes alternating:

  a  the host route the feature replaces: the eight fields device -> host, then the joint mask
     and the sums in numpy (the thresholds taken from the device)
  b  of3d_mask_open_pair alone (the thresholds already on the device)
  c  of3d_flow_pair alone, four 36-bin histograms (the keep volume already on the device)
  d  the same run's device-to-device copy rate, for (c)'s byte floor: the pass reads six fields
     and 2 B of keep per voxel, 50 B in fp64

and the results of (a) and (c) compared.  One JSON line per figure.
"""

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from summary_bench import SCALES, emit, event_ms, resident_fields  # noqa: E402

from bench import CONFIGS  # noqa: E402
from opticalflow3d_dev_amd import _lib  # noqa: E402
from opticalflow3d_dev_amd.analysis import PAIR_QUANTITIES, _PairCall  # noqa: E402


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(CONFIGS))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=20, help="calls of the host route (seconds each at c3)")
    args = ap.parse_args()

    fs, ch0 = resident_fields(args.config)
    ch1 = [torch.roll(a, shifts=(1, 3, 5), dims=(0, 1, 2)).contiguous() for a in ch0]
    (vx0, vy0, vz0, rel0), (vx1, vy1, vz1, rel1) = ch0, ch1
    nvox, dims = rel0.numel(), tuple(rel0.shape)
    stream = torch.cuda.current_stream().cuda_stream
    bins = {"dot": np.linspace(-0.01, 0.01, 37), "cosine": np.linspace(-1.0001, 1.0001, 37),
            "dtheta": np.linspace(-np.pi, np.pi, 37), "dmagnitude": np.linspace(-0.1, 0.1, 37)}
    call = _PairCall(dims, rel0.dtype, rel0.device, rel_percentile=80, bins=bins, min_size=1, connectivity=26, **SCALES)
    ptrs = lambda c: tuple(a.data_ptr() for a in c)
    v_f32 = vx0.dtype == torch.float32
    res = call.enqueue(ptrs(ch0), ptrs(ch1), v_f32, stream)  # leaves the thresholds and keep on the device
    dev = call.decode(res.cpu().numpy())
    lib, base = call.lib, call.result.data_ptr()
    t0, t1 = base + call.thresh_off, base + call.thresh_off + 8
    route_b = lambda: call.open.enqueue_pair(rel0.data_ptr(), t0, rel1.data_ptr(), t1, call.floor, call.combine,
                                             base + call.counts_off, stream)
    route_c = lambda: _lib.check(lib.of3d_flow_pair(
        vx0.data_ptr(), vy0.data_ptr(), vz0.data_ptr(), vx1.data_ptr(), vy1.data_ptr(), vz1.data_ptr(), int(v_f32),
        *dims, *call.scales, call.roi_arr, 1, call.keep.data_ptr(), call.nb_arr, call.edge_arr, base,
        call.ws.data_ptr(), stream))
    host = {}
    sxy, sz, st = call.scales

    def route_a():
        th = call.result[call.thresh_off // 8:].cpu().numpy()
        ta, tb = (th[i:i + 1].view(call.rel_dt)[0] for i in (0, 1))
        f = [a.cpu().numpy() for a in ch0 + ch1]
        r0, r1 = f[3], f[7]
        m = ((r0 > ta) | (r1 > tb)) & (r0 > 0) & (r1 > 0)
        # the mask's voxels alone go through the arithmetic: what a careful script does
        x0, y0, z0, x1, y1, z1 = (a[m].astype(np.float64) for a in (f[0], f[1], f[2], f[4], f[5], f[6]))
        ok = (x0 != 0) & (y0 != 0) & (z0 != 0) & (x1 != 0) & (y1 != 0) & (z1 != 0)  # v * mask == 0 -> NaN
        x0, y0, x1, y1 = (a[ok] * sxy / st for a in (x0, y0, x1, y1))
        z0, z1 = z0[ok] * sz / st, z1[ok] * sz / st
        m0, m1 = np.sqrt(x0 * x0 + y0 * y0 + z0 * z0), np.sqrt(x1 * x1 + y1 * y1 + z1 * z1)
        h0, h1 = np.sqrt(x0 * x0 + y0 * y0), np.sqrt(x1 * x1 + y1 * y1)
        dot = x0 * x1 + y0 * y1 + z0 * z1
        cosine = dot / (m0 * m1)
        dth = np.arctan2((x0 * y1 - y0 * x1) / (h0 * h1), (x0 * x1 + y0 * y1) / (h0 * h1))
        host.update(n_valid=int(dot.size), sum_dot=float(dot.sum()), sum_cosine=float(cosine.sum()),
                    sum_mag0=float(m0.sum()), sum_mag1=float(m1.sum()),
                    theta0=float(np.arctan2((y0 / h0).sum(), (x0 / h0).sum())),
                    hist_dtheta=np.histogram(dth, bins=bins["dtheta"])[0],
                    hist_cosine=np.histogram(cosine, bins=bins["cosine"])[0])

    route_a()
    rel_diff = lambda a, b: float(abs(a - b) / max(abs(b), 1e-300))
    emit(name="routes_agree", config=args.config, second_channel="channel 0 rolled by (1, 3, 5) voxels",
         n_valid=int(dev["n_valid"][0]), n_valid_equal=bool(host["n_valid"] == int(dev["n_valid"][0])),
         n_mask=int(dev["n_mask"][0]), n_voxels=int(dev["n_voxels"][0]),
         sum_dot_rel_diff=rel_diff(dev["sum_dot"][0], host["sum_dot"]),
         sum_cosine_rel_diff=rel_diff(dev["sum_cosine"][0], host["sum_cosine"]),
         sum_mag0_rel_diff=rel_diff(dev["ch0"]["sum_magnitude"][0], host["sum_mag0"]),
         sum_mag1_rel_diff=rel_diff(dev["ch1"]["sum_magnitude"][0], host["sum_mag1"]),
         theta0_abs_diff=float(abs(dev["ch0"]["theta_mean"][0] - host["theta0"])),
         hist_cosine_equal=bool(np.array_equal(dev["hist"]["cosine"][0], host["hist_cosine"])),
         hist_dtheta_moved=int(np.abs(dev["hist"]["dtheta"][0].astype(np.int64) - host["hist_dtheta"]).sum()))

    src = torch.empty(1 << 28, dtype=torch.float32, device=rel0.device).normal_()  # 1 GiB
    dst = torch.empty_like(src)
    tb, tc, td = event_ms(torch, [route_b, route_c, lambda: dst.copy_(src)], args.iters)
    (ta,) = event_ms(torch, [route_a], args.host_iters, warmup=1)
    copy_tbs = 2 * src.numel() * 4 / (td[0] * 1e-3) / 1e12
    pass_bytes = nvox * (6 * vx0.element_size() + 2)
    floor = pass_bytes / (copy_tbs * 1e12) * 1e3
    emit(name="d_copy_bandwidth", tb_per_s=round(copy_tbs, 3), ms=round(td[0], 4), bytes=2 * src.numel() * 4)
    emit(name="a_host_route", config=args.config, iters=args.host_iters, ms_median=round(ta[0], 3), ms_min=round(ta[1], 3),
         bytes_downloaded=sum(a.numel() * a.element_size() for a in ch0 + ch1))
    emit(name="b_mask_open_pair", config=args.config, iters=args.iters, min_size=1, connectivity=26,
         ms_median=round(tb[0], 4), ms_min=round(tb[1], 4), workspace_bytes=int(call.open.ws.numel()))
    emit(name="c_flow_pair", config=args.config, iters=args.iters, quantities=list(PAIR_QUANTITIES), bins=36,
         ms_median=round(tc[0], 4), ms_min=round(tc[1], 4), bytes_per_voxel=pass_bytes / nvox,
         floor_ms=round(floor, 4), over_floor=round(tc[0] / floor, 2), workspace_bytes=int(call.ws.numel()),
         valid_fraction=round(int(dev["n_valid"][0]) / nvox, 4))
    emit(name="c_over_a", ratio=round(tc[0] / ta[0], 6), speedup=round(ta[0] / tc[0], 1),
         b_plus_c_speedup=round(ta[0] / (tb[0] + tc[0]), 1))
    fs.close()


if __name__ == "__main__":
    main()
