"""Device-side frame summaries: what they cost (DESIGN.md "Device-side frame summaries").

Part 1, on resident fields of one FlowStream step of --config (default c3, 512x512x128), timed
with device events over --iters calls after a warm-up, the two routes alternating:

  a  existing route: percentile_threshold (two torch.kthvalue + isnan().any(), host
     synchronisations) + flow_statistics (six more full-size fp64 fields) + the torch
     reductions that form the same sums as the summary
  b  new route: percentile_threshold_device + of3d_flow_summary (no histograms: the same
     outputs as a), and b_hist: the same with vx, vy, vz, magnitude, theta, phi histograms

and (b) against its byte floor, (3 select passes * 4 B + 28 B) per voxel over the copy
bandwidth measured in the same run (a device-to-device torch copy, read + write bytes).

Part 2, per-frame wall time of process_flow on a synthetic OneTif series of --e2e-config
(default c2, 256x256x64): fields only (the behaviour without a summary), summary with fields,
summary without fields.

One JSON line per figure.
"""

import argparse
import contextlib
import io
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import CONFIGS  # noqa: E402
from opticalflow3d_dev_amd import SummarySpec, flow_statistics, process_flow, radii  # noqa: E402
from opticalflow3d_dev_amd import tiff as tf  # noqa: E402
from opticalflow3d_dev_amd.analysis import _SummaryCall  # noqa: E402
from opticalflow3d_dev_amd.stream import FlowStream  # noqa: E402

SCALES = dict(xyscale=0.065, zscale=0.2, tscale=0.75)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def event_ms(torch, fns, iters, warmup=3):
    """Median and min device-event time (ms) of each callable, the callables alternating."""
    times = [[] for _ in fns]
    for it in range(warmup + iters):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if it >= warmup:
                times[i].append(a.elapsed_time(b))
    return [(float(np.median(t)), float(np.min(t))) for t in times]


def synthetic_frames(nt, nz, ny, nx, seed=0):
    """bench.synthetic_frames' family (translated separable sinusoids + bounded noise, uint16),
    generated on the device: the host version takes minutes at 512x512x128."""
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    rng = np.random.default_rng(seed)
    k, ph = rng.uniform(2 * np.pi / 24, 2 * np.pi / 6, size=(3, 3)), rng.uniform(0, 2 * np.pi, size=(3, 3))
    ax = [torch.arange(n, dtype=torch.float64, device="cuda") for n in (nx, ny, nz)]
    vel = (0.3, -0.2, -0.1)
    out = np.empty((nt, nz, ny, nx), np.uint16)
    for t in range(nt):
        s = torch.zeros((nz, ny, nx), dtype=torch.float64, device="cuda")
        for q in range(3):
            fx, fy, fz = (torch.sin(k[q, i] * (ax[i] - vel[i] * t) + ph[q, i]) for i in range(3))
            s += fz[:, None, None] * fy[None, :, None] * fx[None, None, :]
        noise = torch.randint(-8, 9, (nz, ny, nx), generator=g, device="cuda")
        out[t] = (1000 + 300 * s + noise).clamp_(0, 65535).to(torch.int32).cpu().numpy().astype(np.uint16)
    return out


def resident_fields(cfg):
    """The device outputs of one FlowStream step on synthetic frames (kept resident)."""
    nt, nz, ny, nx, s, t, w, _ = CONFIGS[cfg]
    fs = FlowStream(3, (nz, ny, nx), np.uint16, s, t, w, depth=1, summary=SummarySpec(), fields=False)
    frames = synthetic_frames(fs.nwin + fs.lookahead, nz, ny, nx, seed=0)
    for f in frames:
        fs.push(f)
    p = fs.submit()
    p.summary()
    shape = (nz, ny, nx)
    return fs, [d.view(shape) for d in fs.dout[0]]


def part1(args):
    import torch

    fs, (vx, vy, vz, rel) = resident_fields(args.config)
    nvox = vx.numel()
    stream = torch.cuda.current_stream().cuda_stream

    def route_a():
        o = flow_statistics(vx, vy, vz, rel, 90, **SCALES)
        mag = o["magnitude"]
        ok = ~torch.isnan(mag)
        sn, cs = torch.sin(o["theta"]), torch.cos(o["theta"])
        zero = torch.zeros((), dtype=mag.dtype, device=mag.device)
        tot = lambda f: torch.where(ok, f, zero).sum()
        return torch.stack([ok.sum().double(), tot(mag), tot(o["vx"]), tot(o["vy"]), tot(o["vz"]), tot(sn), tot(cs),
                            tot(mag * sn), tot(mag * cs)]).cpu()

    def new_route(bins):
        call = _SummaryCall(SummarySpec(bins=bins, **SCALES), tuple(vx.shape), rel.dtype, vx.device)
        res = call.new_result(vx.device)
        run = lambda: call.enqueue((vx.data_ptr(), vy.data_ptr(), vz.data_ptr(), rel.data_ptr(),
                                    vx.dtype == torch.float32), res.data_ptr(), stream)
        return call, res, run

    lin = lambda a, b: np.linspace(a, b, 37)
    bins = {"vx": lin(-1, 1), "vy": lin(-1, 1), "vz": lin(-1, 1), "magnitude": lin(0, 2), "theta": lin(-np.pi, np.pi),
            "phi": lin(-np.pi / 2, np.pi / 2)}
    call_b, res_b, run_b = new_route(None)
    _, _, run_bh = new_route(bins)
    q_only = lambda: call_b.lib.of3d_quantile(rel.data_ptr(), call_b.rel_f64, nvox, *call_b.ranks[:2],
                                              float(call_b.ranks[2]), call_b.thresh.data_ptr(),
                                              call_b.qws.data_ptr(), stream)
    # the same numbers by both routes (reordered sums: last bits)
    a = route_a().numpy()
    run_b()
    b = call_b.decode(res_b.cpu().numpy())
    got = np.array([b["n_valid"][0]] + [b[k][0] for k in ("sum_magnitude", "sum_vx", "sum_vy", "sum_vz", "sum_sin",
                                                          "sum_cos", "sum_mag_sin", "sum_mag_cos")], dtype=np.float64)
    emit(name="routes_agree", n_valid=int(b["n_valid"][0]), n_voxels=int(b["n_voxels"][0]),
         max_rel_diff=float(np.max(np.abs(a - got) / np.maximum(np.abs(a), 1e-300))))

    src = torch.empty(1 << 28, dtype=torch.float32, device=vx.device).normal_()  # 1 GiB
    dst = torch.empty_like(src)
    (ta, tb, tbh, tq, tc) = event_ms(torch, [route_a, run_b, run_bh, q_only, lambda: dst.copy_(src)], args.iters)
    copy_tbs = 2 * src.numel() * 4 / (tc[0] * 1e-3) / 1e12
    v_sz, r_sz = vx.element_size(), rel.element_size()
    bytes_b = nvox * (3 * r_sz + 3 * v_sz + r_sz)
    floor_ms = bytes_b / (copy_tbs * 1e12) * 1e3
    emit(name="copy_bandwidth", tb_per_s=round(copy_tbs, 3), ms=round(tc[0], 4), bytes=2 * src.numel() * 4)
    emit(name="a_existing_route", config=args.config, ms_median=round(ta[0], 4), ms_min=round(ta[1], 4))
    emit(name="b_new_route", config=args.config, ms_median=round(tb[0], 4), ms_min=round(tb[1], 4),
         quantile_ms=round(tq[0], 4), summary_ms=round(tb[0] - tq[0], 4))
    emit(name="b_new_route_6_histograms", config=args.config, ms_median=round(tbh[0], 4), ms_min=round(tbh[1], 4))
    emit(name="b_over_a", ratio=round(tb[0] / ta[0], 5), speedup=round(ta[0] / tb[0], 2))
    emit(name="b_vs_byte_floor", bytes_per_voxel=bytes_b / nvox, floor_ms=round(floor_ms, 4),
         b_over_floor=round(tb[0] / floor_ms, 2), b_hist_over_floor=round(tbh[0] / floor_ms, 2))
    fs.close()


def part2(args):
    nt0, nz, ny, nx, s, t, w, _ = CONFIGS[args.e2e_config]
    rt = radii(s, t, w)[2]
    nt = 2 * rt + 1 + args.frames - 1
    root = tempfile.mkdtemp(dir=args.dir)
    try:
        tf.imwrite(os.path.join(root, "series.tif"), synthetic_frames(nt, nz, ny, nx, seed=0), imagej=True)
        spec = SummarySpec(rois=[(nz // 4, nz // 2, ny // 4, ny // 2, nx // 4, nx // 2)],
                           bins={"magnitude": np.linspace(0, 2, 37), "theta": np.linspace(-np.pi, np.pi, 37)}, **SCALES)
        modes = (("fields_only", {}), ("summary_with_fields", dict(summary=spec)),
                 ("summary_without_fields", dict(summary=spec, save_fields=False)))
        for rep in range(args.reps + 1):  # rep 0 warms up (code objects, page cache of the input)
            for name, kw in modes:
                out = os.path.join(root, "OpticalFlow3D")
                shutil.rmtree(out, ignore_errors=True)
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    process_flow(root, "series", "OneTif", 3, s, t, w, **kw)
                dt = time.perf_counter() - t0
                if rep:
                    emit(name="process_flow_" + name, config=args.e2e_config, rep=rep, frames=args.frames,
                         ms_per_frame=round(dt / args.frames * 1e3, 3))
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(CONFIGS))
    ap.add_argument("--e2e-config", default="c2", choices=sorted(CONFIGS))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frames", type=int, default=12, help="output frames of the process_flow runs")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--dir", default=None, help="where the synthetic series is written (default: the temp dir)")
    ap.add_argument("--parts", default="1,2")
    args = ap.parse_args()
    if "1" in args.parts.split(","):
        part1(args)
    if "2" in args.parts.split(","):
        part2(args)


if __name__ == "__main__":
    main()
