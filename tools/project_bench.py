"""Projection maps on the device: what they cost.

Part 1, on the resident outputs of one FlowStream step of --config (default c3, 512x512x128,
float64 velocities, float32 rel), device events over --iters calls after 3 warm-ups, the
callables alternating:

  axis_z / axis_y / axis_x   of3d_flow_project of the whole volume along one axis, maps 0-6
  copy                       torch copy_ of the three fields and rel between device tensors — the
                             bytes an axis reads, read and written once, in the same process
  half_z / half_y / half_x   a box of half the extent per axis with an odd x0 (export_bench's)
  thin_z                     a 16 x 16 box over the whole depth along z: 256 lines, one workgroup
                             marching 128 voxels in sequence — the price of the sequential sums
  host                       the fields downloaded and the same maps formed with numpy (wall time)

Part 2, steady wall time per frame of a FlowStream (fields=False) over --frames output frames of
--stream-configs (default c3 and c2): without a request, and with ProjectionSpec(axes=("z",),
image=True) over the whole volume — once with a consumer that only waits for the frame's words
(the device's share: kernels and the block's copy), once with one that copies and decodes them
in the submitting thread —; with the block's bytes and, from device events, the compute-stream
copy of that block to pinned memory alone.  --stream-reps alternates the three.

One JSON line per figure.
"""

import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from export_bench import half_box  # noqa: E402
from summary_bench import SCALES, emit, event_ms, resident_fields, synthetic_frames  # noqa: E402

from bench import CONFIGS  # noqa: E402
from opticalflow3d_dev_amd import ProjectionSpec, SummarySpec  # noqa: E402
from opticalflow3d_dev_amd.analysis import _ProjectCall, percentile_threshold_device  # noqa: E402
from opticalflow3d_dev_amd.stream import FlowStream  # noqa: E402

FLOW_MAPS = ("n_mask", "n_valid", "sum_vx", "sum_vy", "sum_vz", "sum_magnitude", "max_magnitude")


def host_route(fields, thresh):
    """The maps along z as a numpy user forms them from downloaded fields (a pairwise sum: the
    values differ from the device's loop in the last bits)."""
    vx, vy, vz, rel = (f.cpu().numpy() for f in fields)
    m = rel > thresh
    comps = []
    for v, s in ((vx, SCALES["xyscale"]), (vy, SCALES["xyscale"]), (vz, SCALES["zscale"])):
        v = v * m
        v[v == 0] = np.nan
        comps.append(v * s / SCALES["tscale"])
    mag = np.sqrt(comps[0] ** 2 + comps[1] ** 2 + comps[2] ** 2)
    ok = ~np.isnan(mag)
    out = [m.sum(0), ok.sum(0), np.fmax.reduce(np.where(ok, mag, np.nan), 0)]
    return out + [np.where(ok, q, 0.0).sum(0) for q in comps + [mag]]


def part1(args):
    import torch

    fs, (vx, vy, vz, rel) = resident_fields(args.config)
    dims = tuple(rel.shape)
    stream = torch.cuda.current_stream().cuda_stream
    thresh = percentile_threshold_device(rel, 90)
    scales = (SCALES["xyscale"], SCALES["zscale"], SCALES["tscale"])
    thin = (0, dims[0], dims[1] // 2, dims[1] // 2 + 16, dims[2] // 2 + 1, dims[2] // 2 + 17)
    boxes = np.array([[0, dims[0], 0, dims[1], 0, dims[2]], half_box(dims), thin], dtype=np.int64)
    v_f32, rel_f64 = vx.dtype == torch.float32, rel.dtype == torch.float64
    in_bytes = lambda n: n * (3 * vx.element_size() + rel.element_size())

    def bound(roi, axis):
        call = _ProjectCall(boxes, dims, rel_f64, ProjectionSpec(axes=(axis,), maps=FLOW_MAPS, rois=(roi,)), 3, scales)
        out = call.new_result(rel.device)
        run = lambda: call.enqueue((vx.data_ptr(), vy.data_ptr(), vz.data_ptr(), rel.data_ptr(), v_f32),
                                   thresh.data_ptr(), None, out.data_ptr(), stream)
        return call, out, run

    cases = ([("axis_" + a, 0, a) for a in "zyx"] + [("half_" + a, 1, a) for a in "zyx"] + [("thin_z", 2, "z")])
    runs = [bound(r, a) for _, r, a in cases]
    src = [vx, vy, vz, rel]
    dst = [torch.empty_like(t) for t in src]

    def copy():
        for d, s in zip(dst, src):
            d.copy_(s)

    times = event_ms(torch, [r[2] for r in runs] + [copy], args.iters)
    tc = times[-1]
    nvox = int(np.prod(dims))
    copy_tbs = 2 * in_bytes(nvox) / (tc[0] * 1e-3) / 1e12
    emit(name="copy", config=args.config, iters=args.iters, ms_median=round(tc[0], 4), ms_min=round(tc[1], 4),
         bytes_read=in_bytes(nvox), bytes_moved=2 * in_bytes(nvox), tb_per_s=round(copy_tbs, 3))
    by_name = {}
    for (name, r, axis), (call, _, _), t in zip(cases, runs, times):
        n = int(np.prod(boxes[r, 1::2] - boxes[r, 0::2]))
        read = in_bytes(n)
        by_name[name] = t[0]
        emit(name="project_" + name, config=args.config, iters=args.iters, box=[int(v) for v in boxes[r]], axis=axis,
             ms_median=round(t[0], 4), ms_min=round(t[1], 4), bytes_read=int(read),
             result_bytes=int(call.result_bytes), read_tb_per_s=round(read / (t[0] * 1e-3) / 1e12, 3),
             copy_of_those_bytes_ms=round(tc[0] * n / nvox, 4), over_copy=round(t[0] / (tc[0] * n / nvox), 3))
    emit(name="x_over_z", config=args.config, whole=round(by_name["axis_x"] / by_name["axis_z"], 3),
         half=round(by_name["half_x"] / by_name["half_z"], 3))
    t0 = time.perf_counter()
    host_route(src, thresh.cpu().numpy()[0])
    emit(name="host_route_z", config=args.config, wall_ms=round((time.perf_counter() - t0) * 1e3, 1),
         downloaded_bytes=in_bytes(nvox))
    fs.close()


def stream_case(cfg, frames, project, decode=True):
    """Steady wall ms per frame of a summary-only FlowStream over `frames` output frames (the
    first two left out); with a request also the block's bytes.  decode False: the consumer
    waits for the frame's words and leaves them in pinned memory (the device's share alone);
    True: it also copies and decodes them, in the thread that submits."""
    import torch

    _, nz, ny, nx, s, t, w, _ = CONFIGS[cfg]
    fs = FlowStream(3, (nz, ny, nx), np.uint16, s, t, w, summary=SummarySpec(**SCALES), fields=False, project=project)
    series = synthetic_frames(fs.nwin + frames - 1, nz, ny, nx, seed=0)
    pushed, pend, stamps = 0, [], []

    def take(p):
        if project is not None and decode:
            p.projections()
        elif project is not None:
            p.sum_event.synchronize()
        else:
            p.summary()
        p.release()
        stamps.append(time.perf_counter())

    try:
        for i in range(frames):
            while pushed < min(i + fs.nwin + fs.lookahead, len(series)):
                fs.push(series[pushed])
                pushed += 1
            pend.append(fs.submit())
            if len(pend) == fs.depth:
                take(pend.pop(0))
        for p in pend:
            take(p)
        torch.cuda.synchronize()
        block = fs.summary.project.result_bytes if project is not None else 0
        copy_ms = None
        if project is not None:  # the block's copy to pinned memory alone, by device events
            d, h = fs.addon["project"][0]
            copy_ms = event_ms(torch, [lambda: h.copy_(d, non_blocking=True)], 10)[0][0]
    finally:
        fs.close()
    return float(np.median(np.diff(stamps[2:]))) * 1e3, block, copy_ms


def part2(args):
    request = ProjectionSpec(axes=("z",), rois=(0,), image=True)
    for cfg in args.stream_configs:
        for rep in range(args.stream_reps):
            for name, project, decode in (("plain", None, True), ("project_z_image_words", request, False),
                                          ("project_z_image_decoded", request, True)):
                ms, block, copy_ms = stream_case(cfg, args.frames, project, decode)
                line = dict(name="stream_" + name, config=cfg, rep=rep, frames=args.frames, ms_per_frame=round(ms, 3))
                if project is not None:
                    line.update(block_bytes=int(block), block_copy_ms=round(copy_ms, 4))
                emit(**line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(CONFIGS))
    ap.add_argument("--stream-configs", nargs="+", default=["c3", "c2"], choices=sorted(CONFIGS))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frames", type=int, default=16, help="output frames of the stream runs")
    ap.add_argument("--stream-reps", type=int, default=2)
    ap.add_argument("--parts", default="1,2")
    args = ap.parse_args()
    if "1" in args.parts.split(","):
        part1(args)
    if "2" in args.parts.split(","):
        part2(args)


if __name__ == "__main__":
    main()
