"""Device-side mask axes and projected flow: what they cost.

On the resident outputs of one FlowStream step of --config (default c3, 512x512x128), 90th
percentile, the mask opened with --min-size (default 1000), connectivity 26, whole volume;
device events over --iters calls after 3 warm-ups, the routes alternating:

  a  the host route the feature replaces: keep and the three fields device -> host, numpy
     integer moments, np.linalg.eigh, the masked projections and their histograms on the host
  b  of3d_mask_axes (the threshold and keep already on the device), per phase:
       b_mask_keep   moments + axes from keep (no fields): 2 B per voxel
       b_mask_rel    moments + axes from rel > threshold (no keep): rel's element per voxel
       b_full        moments + axes + projection with three 14-bin histograms
       b_projection  b_full - b_mask_keep: 26 B per voxel in fp64 (three fields and keep)
  d  the same run's device-to-device copy rate, for the byte floors

and the integer moments and histograms of (a) and (b) compared.  One JSON line per figure.
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
from opticalflow3d_dev_amd.analysis import AXIS_NAMES, _AxesCall, _SummaryCall  # noqa: E402


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(CONFIGS))
    ap.add_argument("--min-size", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=20, help="calls of the host route (seconds each at c3)")
    args = ap.parse_args()

    fs, (vx, vy, vz, rel) = resident_fields(args.config)
    nvox, dims = rel.numel(), tuple(rel.shape)
    stream = torch.cuda.current_stream().cuda_stream
    half = [0.05, 0.05, 0.05]
    bins = {a: np.linspace(-h, h, 15) for a, h in zip(AXIS_NAMES, half)}
    spec = SummarySpec(min_size=args.min_size, connectivity=26, axes="mask", axis_bins=bins, **SCALES)
    call = _SummaryCall(spec, dims, rel.dtype, rel.device)
    res = call.new_result(rel.device)
    call.enqueue((vx.data_ptr(), vy.data_ptr(), vz.data_ptr(), rel.data_ptr(), vx.dtype == torch.float32),
                 res.data_ptr(), stream)  # leaves the threshold and keep on the device
    summary = call.decode(res.cpu().numpy())
    thresh, keep, ax = call.thresh, call.open.keep, call.axes
    scales = (spec.xyscale, spec.zscale, spec.tscale)
    mask_only = _AxesCall(call.boxes, dims, call.rel_f64, SummarySpec(axes="mask").axes_request(3), False, scales,
                          rel.device)
    out_full = torch.empty(ax.result_bytes // 8, dtype=torch.int64, device=rel.device)
    out_mask = torch.empty(mask_only.result_bytes // 8, dtype=torch.int64, device=rel.device)
    v_f32 = vx.dtype == torch.float32
    b_full = lambda: ax.enqueue((vx.data_ptr(), vy.data_ptr(), vz.data_ptr(), rel.data_ptr(), v_f32),
                                thresh.data_ptr(), keep.data_ptr(), out_full.data_ptr(), stream)
    b_mask_keep = lambda: mask_only.enqueue((None, None, None, rel.data_ptr(), 0), thresh.data_ptr(), keep.data_ptr(),
                                            out_mask.data_ptr(), stream)
    b_mask_rel = lambda: mask_only.enqueue((None, None, None, rel.data_ptr(), 0), thresh.data_ptr(), None,
                                           out_mask.data_ptr(), stream)
    host = {}

    def route_a():
        k = (keep.cpu().numpy() & 1).astype(bool)
        f = [t.cpu().numpy().astype(np.float64) for t in (vx, vy, vz)]
        z, y, x = (c.astype(np.int64) for c in np.nonzero(k))
        n = x.size
        s1 = np.array([x.sum(), y.sum(), z.sum()], dtype=np.int64)
        s2 = np.array([[(a * b).sum() for b in (x, y, z)] for a in (x, y, z)], dtype=np.int64)
        cov = (s2 / n) - np.outer(s1 / n, s1 / n)
        w, v = np.linalg.eigh(cov)
        vec = v[:, ::-1].T
        hists = []
        with np.errstate(invalid="ignore"):
            p = []
            for fld, sc in zip(f, (spec.xyscale, spec.xyscale, spec.zscale)):
                m = fld * k
                m[m == 0] = np.nan
                p.append(m * sc / spec.tscale)
            ok = ~np.isnan(p[0] * p[0] + p[1] * p[1] + p[2] * p[2])
            used = summary["axes_used"][0]  # the device's axes: the histograms compare exactly
            for e, a in zip(used, AXIS_NAMES):
                proj = (p[0][ok] * e[0] + p[1][ok] * e[1]) + p[2][ok] * e[2]
                hists.append(np.histogram(proj, bins=bins[a])[0])
        host.update(n=int(n), sx=int(s1[0]), sxx=int(s2[0, 0]), syz=int(s2[1, 2]), values=w[::-1].tolist(), vec=vec,
                    hists=hists, n_valid=int(ok.sum()))

    route_a()
    mom = summary["moments"][0]
    emit(name="routes_agree", config=args.config, min_size=args.min_size,
         moments_equal=bool([host["n"], host["sx"], host["sxx"], host["syz"]] == [int(mom[0]), int(mom[1]), int(mom[4]),
                                                                                  int(mom[9])]),
         n_mask=host["n"], n_valid_equal=bool(host["n_valid"] == int(summary["n_axes_valid"][0])),
         hists_equal=bool(all(np.array_equal(h, summary["hist"][a][0]) for h, a in zip(host["hists"], AXIS_NAMES))),
         hist_total=int(sum(int(h.sum()) for h in host["hists"])),
         axis_values=summary["axis_values"][0].tolist(), host_axis_values=host["values"],
         max_abs_cos_to_host=[round(float(abs(summary["axis_vectors"][0][k] @ host["vec"][k])), 12) for k in range(3)])

    src = torch.empty(1 << 28, dtype=torch.float32, device=rel.device).normal_()  # 1 GiB
    dst = torch.empty_like(src)
    tf_, tk, tr, tc = event_ms(torch, [b_full, b_mask_keep, b_mask_rel, lambda: dst.copy_(src)], args.iters)
    (ta,) = event_ms(torch, [route_a], args.host_iters, warmup=1)
    copy_tbs = 2 * src.numel() * 4 / (tc[0] * 1e-3) / 1e12
    floor = lambda nbytes: nbytes / (copy_tbs * 1e12) * 1e3
    proj_ms = tf_[0] - tk[0]
    proj_bytes = nvox * (3 * vx.element_size() + 2)
    emit(name="copy_bandwidth", tb_per_s=round(copy_tbs, 3), ms=round(tc[0], 4), bytes=2 * src.numel() * 4)
    emit(name="a_host_route", config=args.config, iters=args.host_iters, ms_median=round(ta[0], 3), ms_min=round(ta[1], 3))
    emit(name="b_full", config=args.config, iters=args.iters, ms_median=round(tf_[0], 4), ms_min=round(tf_[1], 4))
    emit(name="b_mask_keep", ms_median=round(tk[0], 4), ms_min=round(tk[1], 4), bytes_per_voxel=2,
         floor_ms=round(floor(nvox * 2), 4), over_floor=round(tk[0] / floor(nvox * 2), 2))
    emit(name="b_mask_rel", ms_median=round(tr[0], 4), ms_min=round(tr[1], 4), bytes_per_voxel=rel.element_size(),
         floor_ms=round(floor(nvox * rel.element_size()), 4),
         over_floor=round(tr[0] / floor(nvox * rel.element_size()), 2))
    emit(name="b_projection", ms_median_difference=round(proj_ms, 4), bytes_per_voxel=proj_bytes / nvox,
         floor_ms=round(floor(proj_bytes), 4), over_floor=round(proj_ms / floor(proj_bytes), 2))
    emit(name="b_over_a", ratio=round(tf_[0] / ta[0], 6), speedup=round(ta[0] / tf_[0], 1))
    fs.close()


if __name__ == "__main__":
    main()
