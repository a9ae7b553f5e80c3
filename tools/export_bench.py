"""Field export on the device: what it costs.

Part 1, on the resident outputs of one FlowStream step of --config (default c3, 512x512x128),
device events over --iters calls after 3 warm-ups, the callables alternating:

  whole   of3d_field_export of the whole volume, mask None, no scaling, the fields' own types —
          the same bytes read and written as a device-to-device copy of the four fields
  copy    torch copy_ of the four fields between device tensors, in the same process
  half    a box of half the extent per axis with an odd x0 (1/8 of the voxels), the same mode
  nan32   that box with mask "nan", physical units, float32 blocks

and the ratios of each export to the copy of the bytes it moves (read + written).

Part 2, steady wall time per frame of a FlowStream over --frames output frames of --stream-configs
(default c3 and c2: 512x512x128 and 256x256x64, uint16): fields=True, fields=False (summary
only) and fields=FieldSpec(float32, mask "nan") over one ROI of half the extent per axis; with
the export bytes per frame, the D2H rate the fields=True line shows, and the download thread's
own accounting (fs.stats).

One JSON line per figure.
"""

import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from summary_bench import SCALES, emit, event_ms, resident_fields, synthetic_frames  # noqa: E402

from bench import CONFIGS  # noqa: E402
from opticalflow3d_dev_amd import FieldSpec, SummarySpec  # noqa: E402
from opticalflow3d_dev_amd.analysis import _ExportCall, percentile_threshold_device  # noqa: E402
from opticalflow3d_dev_amd.stream import FlowStream  # noqa: E402


def half_box(dims):
    """Half the extent per axis, centred, x0 made odd."""
    z0, y0, x0 = (d // 4 for d in dims)
    x0 |= 1
    return (z0, z0 + dims[0] // 2, y0, y0 + dims[1] // 2, x0, x0 + dims[2] // 2)


def part1(args):
    import torch

    fs, (vx, vy, vz, rel) = resident_fields(args.config)
    dims = tuple(rel.shape)
    stream = torch.cuda.current_stream().cuda_stream
    thresh = percentile_threshold_device(rel, 90)
    scales = (SCALES["xyscale"], SCALES["zscale"], SCALES["tscale"])
    boxes = np.array([[0, dims[0], 0, dims[1], 0, dims[2]], half_box(dims)], dtype=np.int64)
    v_f32, rel_f64 = vx.dtype == torch.float32, rel.dtype == torch.float64
    in_bytes = lambda n: n * (3 * vx.element_size() + rel.element_size())

    def bound(spec):
        call = _ExportCall(boxes, dims, rel_f64, v_f32, spec, 3, scales)
        out = call.new_result(rel.device)
        run = lambda: call.enqueue((vx.data_ptr(), vy.data_ptr(), vz.data_ptr(), rel.data_ptr(), v_f32), thresh.data_ptr(),
                                   None, out.data_ptr(), stream)
        return call, out, run

    cases = [("whole", FieldSpec(rois=(0,), mask=None, physical=False), 0, 0),
             ("half", FieldSpec(rois=(1,), mask=None, physical=False), 1, 0),
             ("nan32", FieldSpec(rois=(1,), mask="nan", dtype="float32"), 1, 3 * rel.element_size())]
    runs = [bound(spec) for _, spec, _, _ in cases]
    # the whole-volume plain export is the fields, bit for bit
    call, out, run = runs[0]
    run()
    blk = call.decode(out)[0]
    as_bytes = lambda t: t.reshape(-1).view(torch.uint8)
    emit(name="whole_is_a_bit_copy", equal=bool(all(torch.equal(as_bytes(blk[n]), as_bytes(f))
                                                   for n, f in zip(("vx", "vy", "vz", "rel"), (vx, vy, vz, rel)))))
    del blk
    src = [vx, vy, vz, rel]
    dst = [torch.empty_like(t) for t in src]

    def copy():
        for d, s in zip(dst, src):
            d.copy_(s)

    times = event_ms(torch, [r[2] for r in runs] + [copy], args.iters)
    tc = times[-1]
    nvox = int(np.prod(dims))
    copy_bytes = 2 * in_bytes(nvox)
    copy_tbs = copy_bytes / (tc[0] * 1e-3) / 1e12
    emit(name="copy", config=args.config, iters=args.iters, ms_median=round(tc[0], 4), ms_min=round(tc[1], 4),
         bytes=copy_bytes, tb_per_s=round(copy_tbs, 3))
    for (name, spec, r, mask_bytes), (call, out, _), t in zip(cases, runs, times):
        n = int(np.prod(boxes[r, 1::2] - boxes[r, 0::2]))
        moved = in_bytes(n) + n * mask_bytes + call.result_bytes  # the mask source is read once per velocity
        floor = moved / (copy_tbs * 1e12) * 1e3
        emit(name="export_" + name, config=args.config, iters=args.iters, box=[int(v) for v in boxes[r]],
             ms_median=round(t[0], 4), ms_min=round(t[1], 4), result_bytes=int(call.result_bytes), bytes_moved=int(moved),
             tb_per_s=round(moved / (t[0] * 1e-3) / 1e12, 3), copy_of_the_same_bytes_ms=round(floor, 4),
             over_copy=round(t[0] / floor, 3))
    fs.close()


def stream_case(cfg, frames, **kw):
    """Steady wall ms per frame of a FlowStream over `frames` output frames (the first two left
    out), with the stream's own download accounting."""
    import torch

    _, nz, ny, nx, s, t, w, _ = CONFIGS[cfg]
    fs = FlowStream(3, (nz, ny, nx), np.uint16, s, t, w, **kw)
    series = synthetic_frames(fs.nwin + frames - 1, nz, ny, nx, seed=0)
    pushed, pend, stamps = 0, [], []

    def take(p):  # the consumer: wait for the frame, then hand its buffer set back
        if fs.field_spec is not None:
            p.fields()
        elif fs.fields:
            p.result()
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
        stats = dict(fs.stats)
        export_bytes = fs.summary.export.result_bytes if fs.field_spec else 0
    finally:
        fs.close()
    steady = np.diff(stamps[2:])
    return float(np.median(steady)) * 1e3, stats, export_bytes


def part2(args):
    for cfg in args.stream_configs:
        _, nz, ny, nx, *_ = CONFIGS[cfg]
        box = half_box((nz, ny, nx))
        spec = SummarySpec(rois=[box], **SCALES)
        full_bytes = nz * ny * nx * (3 * 8 + 4)
        rate = None
        for name, kw in (("fields_true", dict(summary=spec)), ("fields_false", dict(summary=spec, fields=False)),
                         ("field_spec", dict(summary=spec, fields=FieldSpec(dtype="float32", mask="nan")))):
            ms, stats, export_bytes = stream_case(cfg, args.frames, **kw)
            line = dict(name="stream_" + name, config=cfg, frames=args.frames, ms_per_frame=round(ms, 3))
            if stats["dl_n"]:
                line["dl_copy_ms"] = round(stats["dl_copy_s"] / stats["dl_n"] * 1e3, 3)
                line["dl_wait_ms"] = round(stats["dl_wait_s"] / stats["dl_n"] * 1e3, 3)
            if name == "fields_true":
                rate = full_bytes / (stats["dl_copy_s"] / stats["dl_n"])  # bytes per second of the D2H itself
                line.update(d2h_bytes=full_bytes, d2h_gb_per_s=round(rate / 1e9, 2))
            if name == "field_spec":
                line.update(box=list(box), export_bytes=int(export_bytes),
                            export_transfer_ms_at_that_rate=round(export_bytes / rate * 1e3, 3))
            emit(**line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(CONFIGS))
    ap.add_argument("--stream-configs", nargs="+", default=["c3", "c2"], choices=sorted(CONFIGS))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frames", type=int, default=16, help="output frames of the stream runs")
    ap.add_argument("--parts", default="1,2")
    args = ap.parse_args()
    if "1" in args.parts.split(","):
        part1(args)
    if "2" in args.parts.split(","):
        part2(args)


if __name__ == "__main__":
    main()
