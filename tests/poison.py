"""Hostile memory for the GPU tests: nothing a kernel touches may start out plausible.

A kernel that reads memory nobody wrote in this call, leaves output elements unwritten or
writes just outside its output passes any test whose buffers happen to hold zeros or an
earlier run's correct results (the caching allocator hands the block a test just freed to the
next one).  The helpers here take that luck away:

  * guarded()        an output between two guard runs, every element a sentinel NaN that no
                     kernel of the pipeline can produce; check() reads the bits back;
  * guarded_frames() input frames between guard planes of a loud value;
  * run_plan()       one plan execution into guarded outputs of exactly the compact size;
  * poisoned_empty() torch.empty on the device returns 0xFF bytes (NaN in fp32 and fp64, -1
                     or the largest value in the integer types) for the duration of a test.

The device workspace itself is reached through Plan.poison() / _lib.cache_poison()
(of3d_plan_poison).  A plain module like summary_ref.py: no fixtures, no pytest settings."""
import contextlib

import numpy as np

# Quiet NaNs with a payload: the 2D rel is the canonical NaN (0x7FF8000000000000 / 0x7FC00000,
# either sign) where the discriminant rounds negative, and no arithmetic forms these payloads.
SENTINEL_BITS = {"float64": 0x7FF80F3D0F3D0F3D, "float32": 0x7FC0F3D1}
LOUD_FLOAT = 1e30  # guard planes of float frames (integer frames: all bits set, 0xFFFF in uint16)


def _torch_float(dtype):
    """(torch float dtype, the integer dtype of its bits, the sentinel) for a torch / numpy dtype."""
    import torch

    name = str(dtype).replace("torch.", "") if isinstance(dtype, torch.dtype) else np.dtype(dtype).name
    if name not in SENTINEL_BITS:
        raise TypeError(f"guarded: float32 or float64 outputs, not {dtype!r}")
    ft, it = (torch.float64, torch.int64) if name == "float64" else (torch.float32, torch.int32)
    return ft, it, SENTINEL_BITS[name]


def guarded(n, dtype, device, guard=4096):
    """(view, check): `view` is n elements of `dtype` in the middle of ONE allocation of
    guard + n + guard elements, all set to the sentinel.  check(what="") asserts on the bits
    that both guards still hold the sentinel (nothing wrote outside the view) and that no
    element of the view does (everything was written); a failure names the count and the first
    index of the offenders.  A canonical NaN in the view is a value, not an offender.
    check.buffer is the whole allocation as `dtype` (the CPU tests write to the guards)."""
    import torch

    ft, it, s = _torch_float(dtype)
    n, guard = int(n), int(guard)
    bits = torch.full((guard + n + guard,), s, dtype=it, device=device)
    buf = bits.view(ft)
    view = buf[guard:guard + n]

    def offenders(mask):
        cnt = int(mask.sum())
        return cnt, (int(torch.nonzero(mask)[0, 0]) if cnt else -1)

    def check(what=""):
        tag = f"{what}: " if what else ""
        for name, lo, hi in (("below", 0, guard), ("above", guard + n, guard + n + guard)):
            cnt, first = offenders(bits[lo:hi] != s)
            assert cnt == 0, (f"{tag}{cnt} guard elements {name} the output overwritten, the first at "
                              f"{first + lo - guard} (output indices: [0, {n}))")
        cnt, first = offenders(bits[guard:guard + n] == s)
        assert cnt == 0, f"{tag}{cnt} of {n} output elements never written (still the sentinel), the first at {first}"

    check.buffer = buf
    return view, check


def guarded_set(n, dtypes, device, names=("vx", "vy", "vz", "rel"), guard=4096):
    """guarded() once per dtype -> (views, check_all); check_all(used=None, what="") runs the
    checks of the views whose indices are in `used` (default all) under their names: one call
    after every execution (a 2D plan takes no vz: where a buffer is passed for it anyway, it
    is left out of `used`)."""
    pairs = [guarded(n, dt, device, guard) for dt in dtypes]
    views = [v for v, _ in pairs]

    def check_all(used=None, what=""):
        for i, (_, check) in enumerate(pairs):
            if used is None or i in used:
                check(f"{what}{' ' if what else ''}{names[i] if i < len(names) else i}")

    return views, check_all


def guarded_frames(stack_window, device="cuda", guard_planes=4, misaligned=False):
    """The frames of stack_window ((nframes, planes, ny, nx), or (nframes, ny, nx): one plane
    each; any input dtype) in ONE device buffer, every frame between guard planes of a loud
    value (all bits set for integers: 0xFFFF in uint16; 1e30 for floats): a read outside the
    planes a frame holds changes the result.  Pass exactly the planes of of3d_plan_input_range
    with the matching frame_z0 to hold a slab plan to its promise.  Every frame starts on a
    16-byte boundary (K12's LDS DMA, the vectorised K0); misaligned=True puts every frame one
    element past one instead (the scalar K0, K1c + K2c).  Returns the frames as 1-D device
    tensors (views of the buffer; integer frames as their signed type, as torch has no
    unsigned 16- and 32-bit arithmetic)."""
    import torch

    a = np.ascontiguousarray(stack_window)
    if a.ndim == 3:
        a = a[:, None]
    nf, npl, ny, nx = a.shape
    signed = {"uint16": np.int16, "uint32": np.int32}.get(a.dtype.name)
    a = a.view(signed) if signed else a
    es = a.dtype.itemsize
    al = max(16 // es, 1)  # elements per 16 bytes
    n = npl * ny * nx
    g = -(-int(guard_planes) * ny * nx // al) * al  # guard run, whole 16-byte groups
    pitch = g + -(-(n + 1) // al) * al  # (+ 1: room for the misaligned variant)
    t = torch.from_numpy(a.reshape(nf, n))
    loud = LOUD_FLOAT if a.dtype.kind == "f" else (255 if a.dtype == np.uint8 else -1)
    buf = torch.full((nf * pitch + g + al,), loud, dtype=t.dtype, device=device)
    base = (-buf.data_ptr() % 16) // es  # elements to the first 16-byte boundary
    out = []
    for i in range(nf):
        o = base + i * pitch + g + (1 if misaligned else 0)
        buf[o:o + n].copy_(t[i])
        out.append(buf[o:o + n])
        assert (out[-1].data_ptr() % 16 == 0) == (not misaligned)
    return out


def out_dtypes(ndim, mode):
    """(flow dtype, rel dtype) of a plan's outputs: float64 flow (OF3D_FP32: float32); rel float32
    in 3D (OF3D_REL_F64: float64) and the flow's type in 2D."""
    import torch

    from opticalflow3d_dev_amd import _lib

    vt = torch.float32 if mode & _lib.OF3D_FP32 else torch.float64
    if ndim == 2:
        return vt, vt
    return vt, (torch.float64 if mode & _lib.OF3D_REL_F64 else torch.float32)


def run_plan(plan, frames, dtype_code, frame_z0, z0, z1, mode, rows=None, call="execute", next_frames=None,
             ahead_frames=(), device="cuda", guard=4096):
    """One execution of `plan` over output planes [z0, z1) into guarded outputs of exactly the
    compact size, (z1 - z0) * (yb - ya) * nx (rows = (ya, yb): what plan.set_rows was given;
    None: all rows).  call: "execute", "next" (of3d_plan_execute_next, next_frames: the next
    window's frames or None) or "ahead" (of3d_plan_execute_ahead, ahead_frames: the frames past
    the window).  frames: device tensors.  Synchronises, runs every check(), and returns
    (outputs, kernels, geometry): the host arrays vx, vy, (vz,) rel shaped (planes, rows, nx),
    plan.kernels() and plan.geometry()."""
    import torch

    ndim, ny, nx = plan.ndim, plan.ny, plan.nx
    ya, yb = rows if rows is not None else (0, ny)
    shape = (z1 - z0, yb - ya, nx)
    n = int(np.prod(shape))
    vt, rt = out_dtypes(ndim, mode)
    names = ("vx", "vy", "vz", "rel") if ndim == 3 else ("vx", "vy", "rel")
    bufs = [guarded(n, rt if name == "rel" else vt, device, guard) for name in names]
    ptr = {name: v.data_ptr() for name, (v, _) in zip(names, bufs)}
    fp = [f.data_ptr() for f in frames]
    args = (fp, dtype_code, frame_z0, z0, z1, ptr["vx"], ptr["vy"], ptr.get("vz", 0), ptr["rel"])
    if call == "execute":
        plan.execute(*args)
    elif call == "next":
        plan.execute(*args, next_ptrs=None if next_frames is None else [f.data_ptr() for f in next_frames],
                     pipelined=True)
    elif call == "ahead":
        plan.execute(*args, ahead_ptrs=[f.data_ptr() for f in ahead_frames])
    else:
        raise ValueError(call)
    torch.cuda.synchronize()
    for name, (_, check) in zip(names, bufs):
        check(f"{name} of planes [{z0}, {z1}) rows [{ya}, {yb})")
    outs = [v.cpu().numpy().reshape(shape) for v, _ in bufs]
    return outs, plan.kernels(), plan.geometry()


class _Counter:
    """What poisoned_empty() poisoned so far."""
    device_allocations = 0
    bytes = 0


@contextlib.contextmanager
def poisoned_empty(monkeypatch):
    """While active, torch.empty is a wrapper that calls the real function and, for tensors on
    a device (not CPU, pinned or not), fills their bytes with 0xFF.  Yields a counter
    (device_allocations, bytes); leaving the block restores torch.empty (so does monkeypatch's
    own teardown, should the test fail inside)."""
    import torch

    real = torch.empty
    counter = _Counter()

    def empty(*args, **kwargs):
        t = real(*args, **kwargs)
        if t.device.type != "cpu" and t.numel():
            assert t.is_contiguous()
            t.view(-1).view(torch.uint8).fill_(0xFF)
            counter.device_allocations += 1
            counter.bytes += t.numel() * t.element_size()
        return t

    monkeypatch.setattr(torch, "empty", empty)
    try:
        yield counter
    finally:
        monkeypatch.setattr(torch, "empty", real)
