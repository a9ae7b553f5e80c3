"""Device-side mask opening: what it costs.

Part 1, on the resident outputs of one FlowStream step of --config (default c3, 512x512x128),
90th percentile, --min-size (default 1000), connectivity 26, whole volume; device events over
--iters calls after 3 warm-ups, the routes alternating:

  a  the host route the feature replaces: rel device -> host, scipy.ndimage.label + np.bincount
     + the kept mask on the host, mask host -> device
  b  of3d_mask_open alone (the threshold already on the device)
  c  select + summary as without an opening, and select + open + masked summary
  d  the same run's device-to-device copy rate and (b)'s byte floor from its own traffic: per
     voxel 2 B keep cleared, rel read, label and size written (init), label read (merge), label
     read (count), label read (write) = 22 B + rel's element; the traffic that grows with the
     foreground (neighbour labels, compressed labels, sizes, keep bits) is left out

and the counts of (a) and (b) compared.  Part 2: per-frame wall time of process_flow(summary=,
save_fields=False) on a synthetic OneTif series of --e2e-config (default c2) without and with
min_size.  Part 3 (--parts 3, for a kernel trace of its own): of3d_mask_open --iters times,
nothing else after the set-up.

One JSON line per figure.
"""

import argparse
import contextlib
import io
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from summary_bench import SCALES, emit, event_ms, resident_fields, synthetic_frames  # noqa: E402

from bench import CONFIGS  # noqa: E402
from opticalflow3d_dev_amd import SummarySpec, process_flow, radii  # noqa: E402
from opticalflow3d_dev_amd import tiff as tf  # noqa: E402
from opticalflow3d_dev_amd.analysis import OPEN_COUNTS, _OpenCall, _SummaryCall  # noqa: E402


def part1(args, trace_only=False):
    import torch
    from scipy import ndimage

    fs, (vx, vy, vz, rel) = resident_fields(args.config)
    nvox, dims = rel.numel(), tuple(rel.shape)
    stream = torch.cuda.current_stream().cuda_stream
    plain = _SummaryCall(SummarySpec(**SCALES), dims, rel.dtype, rel.device)
    opened = _SummaryCall(SummarySpec(min_size=args.min_size, connectivity=26, **SCALES), dims, rel.dtype, rel.device)
    res_p, res_o = plain.new_result(rel.device), opened.new_result(rel.device)
    enq = lambda call, res: call.enqueue((vx.data_ptr(), vy.data_ptr(), vz.data_ptr(), rel.data_ptr(),
                                          vx.dtype == torch.float32), res.data_ptr(), stream)
    run_plain, run_opened = (lambda: enq(plain, res_p)), (lambda: enq(opened, res_o))
    run_opened()  # leaves the threshold on the device
    thresh = opened.thresh
    oc = _OpenCall(opened.boxes, dims, opened.rel_f64, args.min_size, 26, rel.device)
    counts = torch.empty((1, 4), dtype=torch.int64, device=rel.device)
    run_open = lambda: oc.enqueue(rel.data_ptr(), thresh.data_ptr(), counts.data_ptr(), stream)
    if trace_only:
        for _ in range(args.iters):
            run_open()
        torch.cuda.synchronize()
        fs.close()
        return

    host = {}

    def route_a():
        r = rel.cpu().numpy()
        lab, n = ndimage.label(r > thresh.cpu().numpy()[0], ndimage.generate_binary_structure(3, 3))
        sizes = np.bincount(lab.ravel(), minlength=n + 1)
        sizes[0] = 0
        big = sizes >= args.min_size
        keep = big[lab]
        host.update(n_mask=int((lab > 0).sum()), n_components=int(n), n_components_kept=int(big.sum()),
                    n_kept=int(keep.sum()), keep=keep)
        return torch.as_tensor(keep).to(rel.device)

    route_a()
    run_open()
    dev = dict(zip(OPEN_COUNTS, counts.cpu().numpy()[0].tolist()))
    emit(name="routes_agree", config=args.config, min_size=args.min_size, device=dev,
         host={k: host[k] for k in OPEN_COUNTS},
         keep_equal=bool(np.array_equal(oc.keep.cpu().numpy() == 1, host["keep"])))

    src = torch.empty(1 << 28, dtype=torch.float32, device=rel.device).normal_()  # 1 GiB
    dst = torch.empty_like(src)
    tb, tp, to, tc = event_ms(torch, [run_open, run_plain, run_opened, lambda: dst.copy_(src)], args.iters)
    (ta,) = event_ms(torch, [route_a], args.host_iters, warmup=1)
    copy_tbs = 2 * src.numel() * 4 / (tc[0] * 1e-3) / 1e12
    bytes_b = nvox * (22 + rel.element_size())
    floor_ms = bytes_b / (copy_tbs * 1e12) * 1e3
    emit(name="copy_bandwidth", tb_per_s=round(copy_tbs, 3), ms=round(tc[0], 4), bytes=2 * src.numel() * 4)
    emit(name="a_host_route", config=args.config, iters=args.host_iters, ms_median=round(ta[0], 3),
         ms_min=round(ta[1], 3))
    emit(name="b_mask_open", config=args.config, iters=args.iters, ms_median=round(tb[0], 4), ms_min=round(tb[1], 4))
    emit(name="c_select_summary", config=args.config, ms_median=round(tp[0], 4), ms_min=round(tp[1], 4))
    emit(name="c_select_open_masked_summary", config=args.config, ms_median=round(to[0], 4), ms_min=round(to[1], 4))
    emit(name="b_over_a", ratio=round(tb[0] / ta[0], 6), speedup=round(ta[0] / tb[0], 1))
    emit(name="b_vs_byte_floor", bytes_per_voxel=bytes_b / nvox, floor_ms=round(floor_ms, 4),
         b_over_floor=round(tb[0] / floor_ms, 2))
    fs.close()


def part2(args):
    nt0, nz, ny, nx, s, t, w, _ = CONFIGS[args.e2e_config]
    rt = radii(s, t, w)[2]
    nt = 2 * rt + 1 + args.frames - 1
    root = tempfile.mkdtemp(dir=args.dir)
    try:
        tf.imwrite(os.path.join(root, "series.tif"), synthetic_frames(nt, nz, ny, nx, seed=0), imagej=True)
        kw = dict(rois=[(nz // 4, nz // 2, ny // 4, ny // 2, nx // 4, nx // 2)],
                  bins={"magnitude": np.linspace(0, 2, 37), "theta": np.linspace(-np.pi, np.pi, 37)}, **SCALES)
        modes = (("summary_without_fields", SummarySpec(**kw)),
                 ("summary_without_fields_min_size", SummarySpec(min_size=args.min_size, **kw)))
        for rep in range(args.reps + 1):  # rep 0 warms up (code objects, page cache of the input)
            for name, spec in modes:
                shutil.rmtree(os.path.join(root, "OpticalFlow3D"), ignore_errors=True)
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    process_flow(root, "series", "OneTif", 3, s, t, w, summary=spec, save_fields=False)
                dt = time.perf_counter() - t0
                if rep:
                    emit(name="process_flow_" + name, config=args.e2e_config, rep=rep, frames=args.frames,
                         min_size=spec.min_size, ms_per_frame=round(dt / args.frames * 1e3, 3))
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(CONFIGS))
    ap.add_argument("--e2e-config", default="c2", choices=sorted(CONFIGS))
    ap.add_argument("--min-size", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=20, help="calls of the host route (seconds each at c3)")
    ap.add_argument("--frames", type=int, default=12, help="output frames of the process_flow runs")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--dir", default=None, help="where the synthetic series is written (default: the temp dir)")
    ap.add_argument("--parts", default="1,2")
    args = ap.parse_args()
    parts = args.parts.split(",")
    if "1" in parts:
        part1(args)
    if "2" in parts:
        part2(args)
    if "3" in parts:
        part1(args, trace_only=True)


if __name__ == "__main__":
    main()
