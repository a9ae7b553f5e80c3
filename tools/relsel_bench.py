"""Reliability thresholds on the device (box percentiles, prctile, profile): what they cost
(DESIGN.md §8m).

On the resident rel of one FlowStream step of --config (default c3, 512x512x128); device events
over --iters calls after 3 warm-ups, the routes alternating:

  a  the host route: rel device -> host, np.percentile x 3 and np.histogram(rel, 50)
  b  the device route before of3d_rel_select: three of3d_quantile calls (85, 90, 95), whole volume
  c  of3d_rel_select, the three percentiles in one call, whole volume
  d  the same with 0 and 100 added (five percentiles, ten ranks)
  e  a box of the central half on each axis: of3d_rel_select in place, against
     rel[box].contiguous() + three of3d_quantile calls
  f  of3d_rel_profile, whole volume plus two ROIs, five thresholds, 50 auto bins
  g  the same run's device-to-device copy rate (1 GiB), for the byte floors

and the values of (b), (c) and (e) compared.  One JSON line per figure, on stdout and in --out
(default profiles/relsel_bench_<config>.jsonl).
"""

import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from summary_bench import event_ms, resident_fields  # noqa: E402

from bench import CONFIGS  # noqa: E402
from opticalflow3d_dev_amd import percentile_threshold_device  # noqa: E402
from opticalflow3d_dev_amd.analysis import _ProfileCall, _SelectCall  # noqa: E402

PCTS = [85.0, 90.0, 95.0]


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(CONFIGS))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=3, help="calls of the host route (seconds each at c3)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out_path = args.out or os.path.join(REPO, "profiles", f"relsel_bench_{args.config}.jsonl")
    out_file = open(out_path, "w")

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        out_file.write(line + "\n")
        out_file.flush()

    fs, (_, _, _, rel) = resident_fields(args.config)
    nvox, dims = rel.numel(), tuple(rel.shape)
    esz, f64 = rel.element_size(), rel.dtype == torch.float64
    passes = 6 if f64 else 3
    stream = torch.cuda.current_stream().cuda_stream
    box = tuple(v for n in dims for v in (n // 4, n // 4 + n // 2))
    nbox = int(np.prod([box[2 * a + 1] - box[2 * a] for a in range(3)]))
    rois = np.array([(0, dims[0], 0, dims[1], 0, dims[2]), box,
                     (0, dims[0] // 2, 0, dims[1] // 2, 0, dims[2] // 2)], dtype=np.int64)

    out3, out5 = (torch.empty(n, dtype=rel.dtype, device=rel.device) for n in (3, 5))
    out_q, out_e, out_eq = (torch.empty(3, dtype=rel.dtype, device=rel.device) for _ in range(3))
    sel3 = _SelectCall(dims, f64, None, PCTS, "linear", rel.device)
    sel5 = _SelectCall(dims, f64, None, PCTS + [0.0, 100.0], "linear", rel.device)
    selbox = _SelectCall(dims, f64, box, PCTS, "linear", rel.device)
    prof = _ProfileCall(rois, dims, f64, PCTS, 50, None, out5)
    res_f = torch.empty(prof.result_bytes // 8, dtype=torch.int64, device=rel.device)

    def route_b(src=rel, out=out_q):
        for k, p in enumerate(PCTS):
            percentile_threshold_device(src, p, out=out[k:k + 1])

    route_c = lambda: sel3.enqueue(rel.data_ptr(), out3.data_ptr(), stream)
    route_d = lambda: sel5.enqueue(rel.data_ptr(), out5.data_ptr(), stream)
    route_e = lambda: selbox.enqueue(rel.data_ptr(), out_e.data_ptr(), stream)
    crop = lambda: rel[box[0]:box[1], box[2]:box[3], box[4]:box[5]].contiguous()
    route_e_copy = lambda: route_b(crop(), out_eq)
    route_f = lambda: prof.enqueue((None, None, None, rel.data_ptr(), 0), None, None, res_f.data_ptr(), stream)
    host = {}

    def route_a():
        r = rel.cpu().numpy()
        host["thresholds"] = [float(np.percentile(r, p)) for p in PCTS]
        host["hist"] = np.histogram(r.ravel(), 50)[0]

    for fn in (route_a, route_b, route_c, route_d, route_e, route_e_copy, route_f):
        fn()
    torch.cuda.synchronize()
    p = prof.decode(res_f.cpu().numpy())
    emit(name="routes_agree", config=args.config, thresholds=[float(v) for v in out3.cpu().numpy()],
         select_equals_quantile=bool(out3.cpu().numpy().tobytes() == out_q.cpu().numpy().tobytes()),
         select_equals_numpy=bool([float(v) for v in out3.cpu().numpy()] == host["thresholds"]),
         five_equal_three=bool(out5[:3].cpu().numpy().tobytes() == out3.cpu().numpy().tobytes()),
         box_in_place_equals_copy=bool(out_e.cpu().numpy().tobytes() == out_eq.cpu().numpy().tobytes()),
         hist_equals_numpy_float32_edges=bool(np.array_equal(p["hist"][0], host["hist"])),
         hist_differences=int(np.abs(p["hist"][0].astype(np.int64) - host["hist"]).sum()),
         fraction_above=[float(v) for v in p["fraction_above"][0]])

    src = torch.empty(1 << 28, dtype=torch.float32, device=rel.device).normal_()  # 1 GiB
    dst = torch.empty_like(src)
    tb, tc, td, te, tec, tf_, tg = event_ms(
        torch, [route_b, route_c, route_d, route_e, route_e_copy, route_f, lambda: dst.copy_(src)], args.iters)
    (ta,) = event_ms(torch, [route_a], args.host_iters, warmup=1)
    copy_tbs = 2 * src.numel() * 4 / (tg[0] * 1e-3) / 1e12
    floor = lambda nbytes: nbytes / (copy_tbs * 1e12) * 1e3
    emit(name="g_copy_bandwidth", tb_per_s=round(copy_tbs, 3), ms=round(tg[0], 4), bytes=2 * src.numel() * 4)
    emit(name="a_host_route", config=args.config, iters=args.host_iters, ms_median=round(ta[0], 3), ms_min=round(ta[1], 3))

    def line(name, t, nbytes, **kw):
        emit(name=name, config=args.config, iters=args.iters, ms_median=round(t[0], 4), ms_min=round(t[1], 4),
             bytes=int(nbytes), floor_ms=round(floor(nbytes), 4), over_floor=round(t[0] / floor(nbytes), 2), **kw)

    line("b_three_quantile_calls", tb, 3 * passes * nvox * esz, passes=3 * passes)
    line("c_select_3", tc, passes * nvox * esz, passes=passes, ranks=6)
    line("d_select_5", td, passes * nvox * esz, passes=passes, ranks=10)
    line("e_select_box_in_place", te, passes * nbox * esz, passes=passes, box=list(box), box_voxels=nbox)
    line("e_crop_copy_three_quantile", tec, (2 + 3 * passes) * nbox * esz, box=list(box), box_voxels=nbox)
    line("f_profile", tf_, int(sum(np.prod(r[1::2] - r[0::2]) for r in rois)) * esz, n_roi=len(rois), thresholds=5,
         nbins=50)
    emit(name="c_over_b", ratio=round(tc[0] / tb[0], 4), speedup=round(tb[0] / tc[0], 2))
    emit(name="e_in_place_over_copy", ratio=round(te[0] / tec[0], 4), speedup=round(tec[0] / te[0], 2))
    emit(name="c_plus_f_over_a", ratio=round((td[0] + tf_[0]) / ta[0], 6), speedup=round(ta[0] / (td[0] + tf_[0]), 1))
    out_file.close()
    fs.close()


if __name__ == "__main__":
    main()
