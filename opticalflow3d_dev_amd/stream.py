"""Streaming driver for time series.

The reference's process_flow loads all NtChunk = 6*tSig+1 frames of every
window for every output frame (calc_flow.py:518, :571-574), computes, then
writes four TIFFs synchronously (:526-529).  Here:

* the input frames live in a device ring of 2*rt+1 slots: each output frame
  costs ONE host->device frame upload (the plan takes a table of frame
  pointers, so the ring is never shifted);
* uploads, compute and downloads run on their own HIP streams, ordered by
  events (upload of frame t+1 overlaps compute of frame t);
* outputs land in pinned host buffers and are handed to a writer thread, so
  TIFF writing overlaps the next frames' transfer and compute.

Results are the same kernels as calc_flow3D/calc_flow2D (bit-identical).
"""

from __future__ import annotations

import queue
import threading
import time
from collections import namedtuple
from functools import partial

import numpy as np

from . import _lib
from .shard import check_slab_split, halo_planes, zslab_bounds
from .taps import make_taps, radii

K0_BATCH_RADII = (3, 6, 9)  # temporal radii with a batched K0 instance (csrc/kt_grad.hip k0m_fn)
MAX_FRAMES = 65  # frame pointers per plan call (kMaxT in csrc/of3d_host.hip)

# torch storage type holding each kernel-native input dtype (same width; the kernels read the bits)
_TORCH_VIEW = {
    np.dtype(np.uint8): "uint8",
    np.dtype(np.uint16): "int16",
    np.dtype(np.int16): "int16",
    np.dtype(np.uint32): "int32",
    np.dtype(np.int32): "int32",
    np.dtype(np.float32): "float32",
    np.dtype(np.float64): "float64",
}


def require_summary(summary, fields, quiver, contract, prefix, fields_name, project=None):
    """The add-ons that ride on a summary refuse to go without one.  FlowStream and process_flow
    share the checks; `prefix` and the name of their fields argument keep each one's messages."""
    from .analysis import FieldSpec

    if isinstance(fields, FieldSpec) and summary is None:
        raise ValueError(f"{prefix}{fields_name}=FieldSpec needs a summary")
    if not fields and summary is None:
        raise ValueError(f"{prefix}{fields_name}=False needs a summary")
    if quiver is not None and summary is None:
        raise ValueError(f"{prefix}quiver needs a summary")
    if contract is not None and summary is None:
        raise ValueError(f"{prefix}contract needs a summary")
    if project is not None and summary is None:
        raise ValueError(f"{prefix}project needs a summary")


def output_layout(ndim, precision, rel_fp64):
    """(number of fields, velocity dtype, rel dtype) of a stream's outputs (numpy dtypes): every
    torch dtype, byte size and rel_f64 / v_f32 flag of the outputs derives from this."""
    if precision not in ("fp64", "fp32"):
        raise ValueError("precision must be 'fp64' (bit-exact) or 'fp32'")
    v_t = np.float32 if precision == "fp32" else np.float64
    rel_t = np.float64 if precision == "fp64" and (ndim == 2 or rel_fp64) else np.float32
    return (4 if ndim == 3 else 3), np.dtype(v_t), np.dtype(rel_t)


class _Slab(namedtuple("_Slab", "axis n a0 a1 ai0 ai1 shape nvox nblock own0 plan_dims max_out_planes rows "
                                "frame_z0 zo0 zo1")):
    """The part of every frame one stream holds, as plain numbers (no device): the whole volume,
    planes [a0, a1) of its n (axis 0) or rows [a0, a1) of the n of every plane (axis 1), with the
    input range [ai0, ai1) along that axis that the own part's stencils reach (shard.halo_planes).
    shape: what is pushed / returned, of nvox elements; nblock: elements of own part + halo, what
    a ring slot holds, the own planes from own0 in it (row slabs: strided, from 0).  plan_dims,
    max_out_planes: what the plan is created with; rows: a row slab's own rows within its plan's
    volume (of3d_plan_set_rows), else None; frame_z0, zo0, zo1: the plan call's first frame plane
    and output planes."""
    __slots__ = ()

    @classmethod
    def of(cls, vol_shape, ndim, zslab, rd, rw):
        """zslab = None (whole volume) or (rank, world, group[, axis]) as FlowStream takes it."""
        nz, ny, nx = vol_shape if ndim == 3 else (1,) + tuple(vol_shape)
        if zslab is None:
            return cls(0, nz, 0, nz, 0, nz, tuple(vol_shape), nz * ny * nx, nz * ny * nx, 0,
                       (nz, ny, nx), 0, None, 0, 0, nz)
        if ndim != 3:
            raise ValueError("z-slabs need a 3D volume")
        rank, world = zslab[:2]
        axis = zslab[3] if len(zslab) > 3 else 0
        n = (nz, ny)[axis]
        check_slab_split(n, world)  # every rank owns planes (rows)
        a0, a1 = zslab_bounds(n, rank, world)
        ai0, ai1 = halo_planes(n, a0, a1, rd, rw)
        if axis == 0:
            plane = ny * nx
            return cls(0, n, a0, a1, ai0, ai1, (a1 - a0, ny, nx), (a1 - a0) * plane,
                       (ai1 - ai0) * plane, (a0 - ai0) * plane, (nz, ny, nx), a1 - a0, None, ai0, a0, a1)
        # row slabs run the plan on the rank's rows + halo as a volume of its own
        return cls(1, n, a0, a1, ai0, ai1, (nz, a1 - a0, nx), nz * (a1 - a0) * nx,
                   nz * (ai1 - ai0) * nx, 0, (nz, ai1 - ai0, nx), 0, (a0 - ai0, a1 - ai0), 0, 0, nz)

    def block(self, buf):
        """A ring slot as the halo exchange takes it: (ai1 - ai0, ...) with the split axis first
        (row slabs: a strided view); None for an empty block."""
        if not self.nblock:
            return None
        nz, ny, nx = self.plan_dims
        if self.axis == 0:
            return buf[:self.nblock].reshape(self.ai1 - self.ai0, ny, nx)
        return buf[:self.nblock].reshape(nz, ny, nx).swapaxes(0, 1)

    def own(self, buf):
        """The own part, of `shape`, of a ring slot or of an output buffer of a whole block."""
        if self.rows is None:
            return buf[self.own0:self.own0 + self.nvox].reshape(self.shape)
        return buf[:self.nblock].reshape(self.plan_dims)[:, self.rows[0]:self.rows[1]]


class _Buf(namedtuple("_Buf", "name pinned count elems dtypes")):
    """One row of a stream's buffer table: `count` allocations, each one tensor of `elems`
    elements per dtype, on the device or in pinned host memory."""
    __slots__ = ()
    nbytes = property(lambda self: self.count * self.elems * sum(d.itemsize for d in self.dtypes))


def buffer_table(slab, nwin, in_dtype, layout, depth, L, fields=True, export_bytes=0, dfull=False, project_bytes=0):
    """Every buffer of a stream with `depth` output sets and L frames of lookahead, as _Buf rows;
    FlowStream allocates from it what _fit_device_memory counted.  fields: full-size pinned
    sets; export_bytes / project_bytes: one export / projection block (device and pinned) per
    set; dfull: a row-slab plan without row ranges writes a whole block's outputs here first."""
    nout, v_t, rel_t = layout
    outs = (v_t,) * (nout - 1) + (rel_t,)
    nv, nb = max(slab.nvox, 1), max(slab.nblock, 1)
    # nwin + 1 (+ lookahead) slots: a new frame's upload (and halo exchange) goes to the slot
    # the frame before last read, so it overlaps the previous frame's compute
    rows = [_Buf("ring", False, nwin + 1 + L, nb, (in_dtype,)),
            _Buf("stage", True, 2, nv, (in_dtype,)),
            _Buf("dout", False, depth, nv, outs)]
    if slab.rows is not None:  # strided own part: the upload lands here, a device copy spreads it
        rows.append(_Buf("dstage", False, 1, nv, (in_dtype,)))
    if fields:
        rows.append(_Buf("hout", True, depth, nv, outs))
    if export_bytes:
        rows += [_Buf(name, pin, depth, export_bytes // 8, (np.dtype(np.int64),))
                 for name, pin in (("export", False), ("hexport", True))]
    if project_bytes:
        rows += [_Buf(name, pin, depth, project_bytes // 8, (np.dtype(np.int64),))
                 for name, pin in (("project", False), ("hproject", True))]
    if dfull:
        rows.append(_Buf("dfull", False, 1, nb, outs))
    return rows


def device_bytes(rows):
    return sum(b.nbytes for b in rows if not b.pinned)


def _fit_device_memory(table, depth, batch, L, free, device=0):
    """(depth, batch, L) that fit `free` bytes of device memory beside the plan's workspace
    (already allocated), table(depth, L) being the buffers: fewer output sets first, then K0
    batching M -> 2 -> none (frame pipelining: -> none); raises only when even one set and no
    lookahead do not fit."""
    need = lambda d, lk: device_bytes(table(d, lk))
    while depth > 1 and need(depth, L) > free:
        depth -= 1
    while L and need(depth, L) > free:
        batch, L = (2, 1) if batch > 2 else (0, 0)
    if need(depth, L) > free:
        raise MemoryError(f"FlowStream: {need(depth, L) / 2**30:.1f} GiB of frames and outputs do not fit "
                          f"the {free / 2**30:.1f} GiB left on device {device}")
    return depth, batch, L


class FlowStream:
    """Device-resident sliding window over a frame sequence.

    push(frame) uploads one frame (shape vol_shape); once 2*rt+1 frames are
    resident, submit() computes the flow of the window's centre frame (the oldest
    2*rt+1 resident frames; the oldest is then retired) and returns a Pending whose
    .result() gives host arrays (vx, vy, [vz,] rel); .release() hands the buffer set
    back (at most `depth` frames in flight).  With lookahead, push `lookahead` frames more
    than the window BEFORE submit() (fewer at a series' end): they pipeline the next windows'
    temporal derivative.  windows(load, first, count) does all of that for a series:

        with FlowStream(3, shape, dtype, xyzSig, tSig, wSig) as fs:
            for k, p in fs.windows(load, 0, n_frames - fs.nwin + 1):
                vx, vy, vz, rel = p.result()  # window k: frames k .. k + nwin - 1
                p.release()

    k0_batch=M (2..5; default 5 for whole-volume 3D streams unless `lookahead` is given): M-1
    frames of lookahead, one K0 pass forms the temporal derivatives of M consecutive windows.
    lookahead=True (with k0_batch unset or < 2): frame pipelining instead, one frame of
    lookahead.  Bit-identical either way.
    zslab=(rank, world, group[, axis]): this process holds one slab of every frame (3D only) —
    axis 0 (default): planes shard.zslab_bounds(nz, rank, world); axis 1: those rows of every
    plane.  push() takes the rank's own part and fetches the halo from its neighbours
    (torch.distributed P2P) on the upload stream; results are the rank's part (no gather).
    summary=SummarySpec: the frame is also reduced on the device (.summary() gives
    analysis.flow_summary's dict); fields=False: only that, no field downloads;
    fields=FieldSpec: the fields cropped to ROIs, masked and scaled on the device (.fields());
    quiver=QuiverSpec, contract=ContractSpec, project=ProjectionSpec: .quiver(), .contract(),
    .projections() (the image projected is the window's centre frame).  Whole-volume streams
    only; each add-on is described in DESIGN.md §8a–§8o and §8q, the driver itself in §8p."""

    def __init__(self, ndim, vol_shape, dtype, xyzSig, tSig, wSig, device=None, depth=3, d2h="dma",
                 d2h_blocks=64, precision="fp64", rel_fp64=False, zslab=None, lookahead=None, k0_batch=None,
                 summary=None, fields=True, quiver=None, contract=None, project=None):
        import torch

        from .analysis import FieldSpec

        # validate (no device call before the last of these)
        self.torch = torch
        self.ndim = ndim
        self.field_spec = fields if isinstance(fields, FieldSpec) else None
        if summary is not None and zslab is not None:
            raise ValueError("FlowStream: summaries of slab streams are not supported (whole volumes only)")
        require_summary(summary, fields, quiver, contract, "FlowStream: ", "fields", project=project)
        self.fields = bool(fields) and self.field_spec is None  # full-size downloads
        self.device = _lib.device_index() if device is None else device
        self.dev = torch.device("cuda", self.device)
        dt = np.dtype(dtype)
        if dt not in _TORCH_VIEW:
            dt = np.dtype(np.float64)
        self.np_dtype = dt
        self.code = _lib.DTYPE_CODES[dt]
        self.rd, self.rs, self.rt, self.rw = radii(xyzSig, tSig, wSig)
        self.nwin = 2 * self.rt + 1
        self.batch = 0
        if k0_batch is None:  # default: K0 batching of 5 windows for whole-volume 3D streams
            k0_batch = 5 if lookahead is None else 0
        # batched K0 instances exist for rt 3, 6, 9 (tSig 1, 2, 3: csrc/kt_grad.hip k0m_fn) and
        # 2rt+M frames within the plan's 65-frame table; elsewhere the ring holds no lookahead
        if (k0_batch >= 2 and ndim == 3 and zslab is None and self.rt in K0_BATCH_RADII
                and self.nwin + min(int(k0_batch), 5) - 1 <= MAX_FRAMES):
            self.batch = min(int(k0_batch), 5)
            lookahead = False
        elif k0_batch >= 2 and lookahead is None:
            lookahead = False  # asked for batching: no frame pipelining in its place
        if lookahead is None:
            lookahead = ndim == 3 and zslab is None
        self.L = self.batch - 1 if self.batch else (1 if lookahead else 0)
        # geometry
        self.rank, self.world, self.group = zslab[:3] if zslab is not None else (0, 1, None)
        self.slab = slab = _Slab.of(vol_shape, ndim, zslab, self.rd, self.rw)
        self.shape, self.nvox = slab.shape, slab.nvox
        layout = output_layout(ndim, precision, rel_fp64)
        v_f32, rel_f64 = layout[1].itemsize == 4, layout[2].itemsize == 8
        if d2h not in ("dma", "kernel", "runtime"):
            raise ValueError("d2h must be 'dma', 'kernel' or 'runtime'")
        # plan
        self.plan, self.rows_direct = None, False
        if slab.nvox > 0:
            mode = (_lib.OF3D_FP32 if v_f32 else 0) | (_lib.OF3D_REL_F64 if rel_fp64 else 0)
            self.plan = _lib.Plan(ndim, *slab.plan_dims, make_taps(xyzSig, tSig, wSig), device=self.device, mode=mode,
                                  max_out_planes=slab.max_out_planes)
            if slab.max_out_planes:
                assert self.plan.input_range(slab.a0, slab.a1) == (slab.ai0, slab.ai1)
            if slab.rows is not None:
                try:  # the plan writes only the own rows (of3d_plan_set_rows)
                    self.plan.set_rows(*slab.rows)
                    self.rows_direct = True
                except RuntimeError:  # kernels without row ranges: whole sub-volume, then a slice
                    pass
        # buffer table (after the plan: rows_direct decides dfull), and what of it fits the device
        export_bytes = 0
        if self.field_spec is not None:  # sized ahead of the buffers: _SummaryCall allocates on the device
            from .analysis import _ExportCall

            export_bytes = _ExportCall.size(summary.resolve(self.shape)[0], rel_f64, v_f32, self.field_spec, ndim)[1]
        project_bytes = 0
        if project is not None:
            from .analysis import _ProjectCall

            project_bytes = _ProjectCall.size(summary.resolve(self.shape)[0], project, ndim)[1]
        table = partial(buffer_table, slab, self.nwin, dt, layout, fields=self.fields, export_bytes=export_bytes,
                        dfull=slab.rows is not None and not self.rows_direct, project_bytes=project_bytes)
        free = torch.cuda.mem_get_info(self.dev)[0] - (1 << 30)  # a margin for the runtime and the summary
        self.depth, self.batch, self.L = _fit_device_memory(table, depth, self.batch, self.L, free, self.device)
        # allocate
        bufs = {b.name: self._alloc(b) for b in table(self.depth, self.L)}
        self.ring = bufs["ring"]  # one allocation: the slots are its rows
        self.order = []  # ring slots of the resident frames, oldest first
        self.free = list(range(len(self.ring)))
        self.dstage = bufs["dstage"][0][0] if "dstage" in bufs else None
        self.stage = [s[0] for s in bufs["stage"]]
        self.stage_np = [t.numpy().view(dt)[:self.nvox].reshape(self.shape) for t in self.stage]
        self.stage_evt = [None, None]
        self.stage_i = 0
        self.dout = bufs["dout"]
        self.hout = bufs.get("hout", [None] * self.depth)
        self.dfull = bufs["dfull"][0] if "dfull" in bufs else None
        # Downloads (d2h):
        #   "dma"     of3d_dma_copy on the SDMA engines from a download thread
        #             once the frame's kernels are done: no CU time, and the
        #             next frame's kernels run at full speed meanwhile;
        #   "kernel"  of3d_copy_async, d2h_blocks workgroups on a stream of its
        #             own priority (hence its own hardware queue);
        #   "runtime" torch copy_ — HIP's device->host path is a blit kernel
        #             over the whole GPU.
        # Kernel-driven PCIe writes (the last two) back up the memory pipeline
        # shared with the compute kernels and slow them several-fold.
        self.d2h_mode = d2h
        self.d2h_blocks = d2h_blocks
        self.h2d = torch.cuda.Stream(device=self.dev)
        self.comp = torch.cuda.Stream(device=self.dev)
        self.d2h = torch.cuda.Stream(device=self.dev, priority=-1)
        self.dl_q = None
        self.stats = {"dl_wait_s": 0.0, "dl_copy_s": 0.0, "dl_n": 0}
        self.trace = None  # list -> (time, event) records of the download thread
        if d2h == "dma":
            self.dl_q = queue.Queue()
            self.dl_thread = threading.Thread(target=self._download_loop, daemon=True)
            self.dl_thread.start()
        self.precision, self.v_f32 = precision, v_f32
        self.summary, self.addon = None, {}
        if summary is not None:
            from .analysis import _SummaryCall

            self.summary = _SummaryCall(summary, self.shape, getattr(torch, layout[2].name), self.dev, quiver=quiver,
                                        contract=contract, export=self.field_spec, v_f32=v_f32, project=project)
            self.dsum = [self.summary.new_result(self.dev) for _ in range(self.depth)]
            self.hsum = [torch.empty(self.summary.result_bytes // 8, dtype=torch.int64, pin_memory=True)
                         for _ in range(self.depth)]
            # the add-ons' own blocks per buffer set, name -> (device, pinned): copied behind the
            # summary's words on the compute stream — but for "export", whose block (the table's)
            # travels on the fields' download path in their place (submit); the projection's
            # blocks are the table's too (counted against the device's memory), copied like the others
            self.addon = {name: [(call.new_result(self.dev),
                                  torch.empty(call.result_bytes // 8, dtype=torch.int64, pin_memory=True))
                                 for _ in range(self.depth)]
                          for name, call, _ in self.summary.addons if name not in ("export", "project")}
            if project is not None:
                assert self.summary.project.result_bytes == project_bytes
                self.addon["project"] = [(d[0], h[0]) for d, h in zip(bufs["project"], bufs["hproject"])]
                assert all(d.data_ptr() % 16 == 0 for d, _ in self.addon["project"])  # as of3d_flow_project asks
            if self.field_spec is not None:
                assert self.summary.export.result_bytes == export_bytes
                self.addon["export"] = [(d[0], h[0]) for d, h in zip(bufs["export"], bufs["hexport"])]
                assert all(d.data_ptr() % 16 == 0 for d, _ in self.addon["export"])  # as of3d_field_export asks
        self.host_free = [threading.Event() for _ in range(self.depth)]  # set: writer released the set
        for e in self.host_free:
            e.set()
        self.slot_evt = {}               # ring slot -> event of the last compute that read it
        self.k = 0

    def _alloc(self, b):
        """The tensors of one buffer-table row: per allocation one tensor per dtype; the ring is
        one (slots, elements) tensor."""
        torch = self.torch
        new = lambda shape, d: torch.empty(shape, dtype=getattr(torch, _TORCH_VIEW.get(d, d.name)),
                                           device=None if b.pinned else self.dev, pin_memory=b.pinned)
        if b.name == "ring":
            return new((b.count, b.elems), b.dtypes[0])
        return [[new(b.elems, d) for d in b.dtypes] for _ in range(b.count)]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def push(self, frame):
        torch = self.torch
        frame = np.asarray(frame)
        if frame.shape != self.shape:
            raise ValueError(f"frame shape {frame.shape} != stream shape {self.shape}")
        if not self.free:
            raise RuntimeError("FlowStream: every ring slot holds a frame of an unsubmitted window")
        slot = self.free.pop(0)  # the slot freed longest ago (its last reader is furthest done)
        st = self.stage[self.stage_i]
        if self.stage_evt[self.stage_i] is not None:
            self.stage_evt[self.stage_i].synchronize()  # pinned staging buffer free again
        # one host pass: (byte-swap / astype(float64) as _device_array) into pinned memory
        np.copyto(self.stage_np[self.stage_i], frame, casting="unsafe")
        with torch.cuda.stream(self.h2d):
            if slot in self.slot_evt:
                self.h2d.wait_event(self.slot_evt[slot])  # no compute still reads this slot
            if self.nvox and self.dstage is None:
                self.slab.own(self.ring[slot]).copy_(st[:self.nvox].view(self.shape), non_blocking=True)
            elif self.nvox:
                self.dstage.copy_(st, non_blocking=True)
                self.slab.own(self.ring[slot]).copy_(self.dstage[:self.nvox].view(self.shape))
            if self.world > 1:  # this frame's halo planes from / to the z-neighbours
                self.exchange(slot)
            ev = torch.cuda.Event()
            ev.record(self.h2d)
        self.stage_evt[self.stage_i] = ev
        self.stage_i ^= 1
        self.order.append(slot)

    def exchange(self, slot):
        """Halo planes (rows) of the frame in ring slot `slot` (slab streams): issued on the
        current stream (the upload stream in push); every rank calls it for the same frame."""
        from .shard import exchange_frame_halo

        g = self.slab
        exchange_frame_halo(g.block(self.ring[slot]), g.ai0, g.a0, g.a1, g.n, self.rd + self.rw, self.rank,
                            self.world, self.group)

    @property
    def ready(self):
        return len(self.order) >= self.nwin

    @property
    def lookahead(self):
        """Frames past the window to push before submit (frame pipelining: 1; K0 batching: M-1)."""
        return self.L

    def windows(self, load, first, count):
        """The push-ahead protocol for the windows first .. first + count - 1 of a series (window
        k: frames k .. k + nwin - 1): generates (k, Pending).  load(i) is called once per frame
        those windows need, in increasing order, each frame resident `lookahead` submits early
        (fewer at the series' end).  The ring must be empty (RuntimeError once iterated)."""
        if self.order:
            raise RuntimeError("FlowStream.windows: the ring already holds frames")
        pushed, end = first, first + count + self.nwin - 1  # next frame to upload, one past the last
        for k in range(first, first + count):
            while pushed < min(k + self.nwin + self.L, end):
                self.push(load(pushed))
                pushed += 1
            yield k, self.submit()

    def submit(self):
        torch = self.torch
        assert self.ready
        b = self.k % self.depth
        self.k += 1
        self.host_free[b].wait()  # previous user of this set has released its host buffers,
        self.host_free[b].clear()  # which also means its D2H (and so its compute) finished
        dout, hout = self.dout[b], self.hout[b]
        self.comp.wait_stream(self.h2d)
        g = self.slab
        ptrs = [self.ring[s].data_ptr() for s in self.order[:self.nwin]]
        look = {}
        if g.rows is None:  # a row slab's plan sees a volume of its own: no lookahead through it
            # frame pipelining: the next window (one frame on) is resident too -> its dt0 formed in
            # this call; K0 batching: the resident frames past the window (up to M-1; fewer at a
            # series' end)
            nxt = [self.ring[s].data_ptr() for s in self.order[1:self.nwin + 1]] \
                if self.L and not self.batch and len(self.order) == self.nwin + 1 else None
            ahead = [self.ring[s].data_ptr() for s in self.order[self.nwin:self.nwin + self.L]] if self.batch else None
            look = dict(next_ptrs=nxt, pipelined=bool(self.L) and not self.batch, ahead_ptrs=ahead)
        vz = dout[2].data_ptr() if self.ndim == 3 else 0
        if self.plan is not None:
            # row slabs without row ranges: the plan writes all rows of its sub-volume to dfull,
            # the own rows are copied out
            to = [t.data_ptr() for t in (self.dfull or dout)]
            self.plan.execute(ptrs, self.code, g.frame_z0, g.zo0, g.zo1, to[0], to[1], to[2] if self.ndim == 3 else 0,
                              to[-1], self.comp.cuda_stream, **look)
            if self.dfull is not None:
                with torch.cuda.stream(self.comp):
                    for d, f in zip(dout, self.dfull):
                        d[:self.nvox].view(self.shape).copy_(g.own(f))
        pending = Pending(self, b)
        if self.summary is not None:
            # on the compute stream: behind this frame's kernels and ahead of every later frame's,
            # so a later submit() that reuses this set's device outputs (after its release()) is
            # ordered behind these reads by the stream itself
            if "project" in self.addon:  # the image under the maps: the window's centre frame
                self.summary.project.bind_image(self.ring[self.order[self.rt]].data_ptr(), self.code)
            self.summary.enqueue((dout[0].data_ptr(), dout[1].data_ptr(), vz, dout[-1].data_ptr(), self.v_f32),
                                 self.dsum[b].data_ptr(), self.comp.cuda_stream,
                                 blocks={name: sets[b][0].data_ptr() for name, sets in self.addon.items()})
            with torch.cuda.stream(self.comp):
                self.hsum[b].copy_(self.dsum[b], non_blocking=True)
                for name, sets in self.addon.items():
                    if name != "export":
                        sets[b][1].copy_(sets[b][0], non_blocking=True)
                pending.sum_event = torch.cuda.Event()
                pending.sum_event.record(self.comp)
        cev = torch.cuda.Event()
        cev.record(self.comp)
        for s in self.order[:self.nwin + self.L]:  # the window and (lookahead) the next frame
            self.slot_evt[s] = cev
        self.free.append(self.order.pop(0))  # the window's oldest frame is done with (after cev)
        if self.field_spec is not None:  # the export block travels as the fields would
            dout, hout = ([t] for t in self.addon["export"][b])
        elif not self.fields:
            return pending
        if self.d2h_mode == "dma":
            self.dl_q.put((cev, hout, dout, pending))
            return pending
        with torch.cuda.stream(self.d2h):
            self.d2h.wait_event(cev)
            for h, d in zip(hout, dout):
                if self.d2h_mode == "kernel":
                    _lib.copy_async(h.data_ptr(), d.data_ptr(), d.numel() * d.element_size(), self.d2h_blocks,
                                    self.d2h.cuda_stream)
                else:
                    h.copy_(d, non_blocking=True)
            pending.event = torch.cuda.Event()
            pending.event.record(self.d2h)
        return pending

    def _download_loop(self):
        while True:
            job = self.dl_q.get()
            if job is None:
                return
            cev, hout, dout, pending = job
            try:
                t0 = time.perf_counter()
                cev.synchronize()
                t1 = time.perf_counter()
                if self.nvox:
                    _lib.dma_copy([h.data_ptr() for h in hout], [d.data_ptr() for d in dout],
                                  [d.numel() * d.element_size() for d in dout])
                t2 = time.perf_counter()
                self.stats["dl_wait_s"] += t1 - t0
                self.stats["dl_copy_s"] += t2 - t1
                self.stats["dl_n"] += 1
                if self.trace is not None:
                    self.trace += [(t0, "dl_get"), (t1, "dl_cev"), (t2, "dl_done")]
            except BaseException as e:  # re-raised by Pending.result()
                pending.error = e
            pending.done.set()

    def close(self):
        if self.dl_q is not None:
            self.dl_q.put(None)
            self.dl_thread.join()
            self.dl_q = None
        self.torch.cuda.synchronize(self.dev)
        if self.plan is not None:
            self.plan.close()


class Pending:
    def __init__(self, fs, b):
        self.fs, self.b = fs, b
        self.event = None               # D2H on a stream: completion event
        self.done = threading.Event()   # D2H by the download thread
        self.error = None
        self.sum_event = None           # summary kernels + the copy of their result

    def summary(self):
        """analysis.flow_summary's dict of this frame (streams created with summary=)."""
        if self.sum_event is None:
            raise RuntimeError("FlowStream was created without a summary")
        self.sum_event.synchronize()
        return self.fs.summary.decode(self.fs.hsum[self.b].numpy().copy())

    def _addon(self, name):
        """The decoded block of the add-on `name` of this frame, from a copy of its pinned words,
        once the summary's copies are done."""
        if self.sum_event is None or name not in self.fs.addon:
            raise RuntimeError(f"FlowStream was created without a {name} request")
        self.sum_event.synchronize()
        return getattr(self.fs.summary, name).decode(self.fs.addon[name][self.b][1].numpy().copy())

    def quiver(self):
        """analysis.quiver_sample's per-ROI list of this frame (streams created with quiver=)."""
        return self._addon("quiver")

    def projections(self):
        """analysis.projection_maps' dict of this frame (streams created with project=); the
        image under max_image / sum_image is the window's centre frame."""
        from .analysis import _word_threshold

        maps = self._addon("project")
        call = self.fs.summary.project
        return {"threshold": _word_threshold(self.fs.hsum[self.b].numpy(), call.rel_f64), "rois": call.boxes.copy(),
                "axes": call.axes, "maps": maps}

    def contract(self):
        """analysis.contractility's dict of this frame (streams created with contract=)."""
        from .analysis import _word_threshold

        out = self._addon("contract")
        out["threshold"] = _word_threshold(self.fs.hsum[self.b].numpy(), self.fs.summary.rel_f64)
        return out

    def _wait_download(self):
        if self.event is not None:
            self.event.synchronize()
        else:
            self.done.wait()
            if self.error is not None:
                raise self.error

    def fields(self):
        """analysis.export_fields' `blocks` of this frame (streams created with fields=FieldSpec):
        views of the pinned block, valid until release()."""
        if self.fs.field_spec is None:
            raise RuntimeError("FlowStream was created without a FieldSpec")
        self._wait_download()
        return self.fs.summary.export.decode(self.fs.addon["export"][self.b][1].numpy())

    def result(self):
        """Host arrays: views of pinned buffers, valid until release()."""
        if self.fs.field_spec is not None:
            raise RuntimeError("FlowStream(fields=FieldSpec) downloads no full-size fields: use fields()")
        if not self.fs.fields:
            raise RuntimeError("FlowStream(fields=False) downloads no fields: use summary()")
        self._wait_download()
        shp, n = self.fs.shape, self.fs.nvox
        return [t.numpy()[:n].reshape(shp) for t in self.fs.hout[self.b]]

    def release(self):
        self.fs.host_free[self.b].set()


class Writer:
    """Background TIFF writer; jobs run in submission order."""

    def __init__(self, write_fn):
        self.q = queue.Queue(maxsize=4)
        self.write_fn = write_fn
        self.err = None
        self.t = threading.Thread(target=self._run, daemon=True)
        self.t.start()

    def _run(self):
        while True:
            job = self.q.get()
            if job is None:
                return
            try:
                self.write_fn(*job)
            except BaseException as e:  # surfaced on close()
                self.err = e
            finally:
                self.q.task_done()

    def put(self, *job):
        if self.err:
            raise self.err
        self.q.put(job)

    def close(self):
        self.q.put(None)
        self.t.join()
        if self.err:
            raise self.err
