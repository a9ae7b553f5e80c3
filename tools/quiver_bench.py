"""Device-side quiver samples: what they cost.

On the resident outputs of one FlowStream step of --config (default c3, 512x512x128), 90th
percentile (10 % of the voxels valid), whole volume; device events over --iters calls after 3
warm-ups, the routes alternating, for the gaps 4, 2 and 1:

  a  the route without the feature: flow_statistics (the masked physical fields, full size, on
     the device), torch strided slicing of the gap lattice, boolean indexing by ~isnan(magnitude),
     the lists (coordinates and three velocities) to the host
  b  of3d_quiver_sample (the threshold already on the device) and the copy of its block — sized
     by a counting call to hold exactly the valid records — to a pinned host buffer; and its
     three kernels alone
  d  the same run's device-to-device copy rate, for the kernels' distance from a byte model: both
     passes read, per field, every 64-byte sector that holds a lattice voxel (with gx elements of
     e bytes between lattice voxels a sector holds max(1, 64 / (gx e)) of them), and the emit pass
     writes 32 bytes per record

and the lists of (a) and (b) compared.  One JSON line per figure.
"""

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from summary_bench import SCALES, emit, event_ms, resident_fields  # noqa: E402

from bench import CONFIGS  # noqa: E402
from opticalflow3d_dev_amd import QuiverSpec, flow_statistics  # noqa: E402
from opticalflow3d_dev_amd.analysis import _QuiverCall, percentile_threshold_device  # noqa: E402

SECTOR = 64


def model_bytes(dims, gap, sizes, n_records):
    """The byte model of one of3d_quiver_sample call over the whole volume: two passes over the
    sectors of the four fields (element sizes `sizes`) that hold lattice voxels, and the records."""
    lz, ly = ((d - 1) // g + 1 for d, g in zip(dims[:2], gap[:2]))
    lx = (dims[2] - 1) // gap[2] + 1
    per_row = sum(min(lx, -(-dims[2] * e // SECTOR)) for e in sizes) * SECTOR
    return 2 * lz * ly * per_row + 32 * n_records


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(CONFIGS))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--gaps", type=int, nargs="+", default=[4, 2, 1])
    args = ap.parse_args()

    fs, (vx, vy, vz, rel) = resident_fields(args.config)
    dims = tuple(rel.shape)
    stream = torch.cuda.current_stream().cuda_stream
    thresh = percentile_threshold_device(rel, 90)
    scales = (SCALES["xyscale"], SCALES["zscale"], SCALES["tscale"])
    boxes = np.array([[0, dims[0], 0, dims[1], 0, dims[2]]], dtype=np.int64)
    sizes = [vx.element_size()] * 3 + [rel.element_size()]
    v_f32 = vx.dtype == torch.float32

    src = torch.empty(1 << 28, dtype=torch.float32, device=rel.device).normal_()  # 1 GiB
    dst = torch.empty_like(src)
    for gap in args.gaps:
        make = lambda cap: _QuiverCall(boxes, dims, rel.dtype == torch.float64, QuiverSpec(gap, cap), 3, scales, rel.device)
        call = make(0)  # the count alone first: the block is then sized to hold every valid record, no more
        out = call.new_result(rel.device)
        call.enqueue((vx.data_ptr(), vy.data_ptr(), vz.data_ptr(), rel.data_ptr(), v_f32), thresh.data_ptr(), None,
                     out.data_ptr(), stream)
        call = make(call.decode(out.cpu().numpy())[0]["n_valid"])
        out = call.new_result(rel.device)
        pinned = torch.empty(call.result_bytes // 8, dtype=torch.int64, pin_memory=True)
        got, lists = {}, {}

        def kernels_b():
            call.enqueue((vx.data_ptr(), vy.data_ptr(), vz.data_ptr(), rel.data_ptr(), v_f32), thresh.data_ptr(), None,
                         out.data_ptr(), stream)

        def route_b():
            kernels_b()
            pinned.copy_(out, non_blocking=True)

        def route_a():
            st = flow_statistics(vx, vy, vz, rel, 90, **SCALES)
            sl = (slice(None, None, gap),) * 3
            ok = ~torch.isnan(st["magnitude"][sl])
            lists["zyx"] = (torch.nonzero(ok) * gap).cpu().numpy()
            lists["v"] = torch.stack([st[k][sl][ok] for k in ("vx", "vy", "vz")], dim=1).cpu().numpy()

        route_b()
        torch.cuda.synchronize()
        got = call.decode(pinned.numpy().copy())[0]
        route_a()
        emit(name="routes_agree", config=args.config, gap=gap, n_lattice=got["n_lattice"], n_valid=got["n_valid"],
             zyx_equal=bool(np.array_equal(lists["zyx"], got["zyx"])),
             v_bits_equal=bool(lists["v"].tobytes() == got["v"].tobytes()))
        del lists["zyx"], lists["v"]
        tb, tk, ta, td = event_ms(torch, [route_b, kernels_b, route_a, lambda: dst.copy_(src)], args.iters)
        copy_tbs = 2 * src.numel() * 4 / (td[0] * 1e-3) / 1e12
        mbytes = model_bytes(dims, (gap,) * 3, sizes, got["n_valid"])
        floor = mbytes / (copy_tbs * 1e12) * 1e3
        emit(name="d_copy_bandwidth", gap=gap, tb_per_s=round(copy_tbs, 3), ms=round(td[0], 4), bytes=2 * src.numel() * 4)
        emit(name="a_torch_route", config=args.config, gap=gap, iters=args.iters, ms_median=round(ta[0], 4),
             ms_min=round(ta[1], 4), list_bytes=48 * got["n_valid"])
        emit(name="b_quiver_sample", config=args.config, gap=gap, iters=args.iters, ms_median=round(tb[0], 4),
             ms_min=round(tb[1], 4), block_bytes=int(call.result_bytes), workspace_bytes=int(call.ws.numel()))
        emit(name="b_kernels_alone", config=args.config, gap=gap, iters=args.iters, ms_median=round(tk[0], 4),
             ms_min=round(tk[1], 4), model_bytes=int(mbytes), floor_ms=round(floor, 4),
             over_floor=round(tk[0] / floor, 2))
        emit(name="b_over_a", gap=gap, ratio=round(tb[0] / ta[0], 6), speedup=round(ta[0] / tb[0], 1))
        del call, out, pinned
    fs.close()


if __name__ == "__main__":
    main()
