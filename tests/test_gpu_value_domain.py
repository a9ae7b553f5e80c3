"""Every kernel family on saturated, zero-filled, full-range frames (domain_frames.py).

The other GPU tests draw seeded uint16 noise below 4096, on which no gradient, product or
windowed sum is ever exactly zero and bit 15 of a voxel is never set.  Two kinds of error pass
all of them:

  * the sign of an exact zero.  Inside a constant block every pass sums terms +-0, and the sign
    of the sum follows from the order of the additions and from the value the accumulator starts
    from (scipy starts from the first product, not from +0.0); the solve then forms -R * (...) on
    tensors that are zero throughout.  The oracle defines the pattern (thousands of -0.0 and
    hundreds of +0.0 per component: test_value_domain_cpu.py pins the counts);
  * the high bits of the frames: an int16 / uint16 mix-up in one row of a dispatch table, or a
    permuted unpack in the LDS-DMA staging, changes nothing below 32768.

Here the fused readers (K0c k_tderiv_c, batched K0 k_tderiv_multi, the next-frame K0 inside
k_wz_solve_c_next, K1c k_grad_xy_c, K12 k_grad_xyz_c) and every forced variant of K34 / K5c and
the W-xy layouts run on such frames through a plan, which reports its kernels and geometry.

Contracts are the suite's existing ones, no new tolerance:
  fp64        vx, vy, vz bit-identical to oracle.cpu_ref (scipy backend), every sign of zero
              included; rel within 1e-6 lambda_max of fp64 eigvalsh
  OF3D_FP32   test_gpu_fp32_exact._check3d / _check2d against the float32 oracle
  2D fp64     vx, vy, rel bit-identical
and, stated on its own so that a failure names the cause: rel is exactly 0 wherever the oracle's
lambda_max is exactly 0 (the all-zero tensors)."""
import numpy as np
import pytest

import poison
from conftest import assert_rel_within, bits_equal, oracle3d
from domain_frames import CASES_2D, CASES_3D, block_frames, case_frames
from opticalflow3d_dev_amd import _lib, calc_flow2D, calc_flow3D, make_taps, radii
from oracle import cpu_ref
from test_gpu_fp32_exact import VARIANT_ENV, VARIANTS, _check2d, _check3d, assert_family_ran
from test_gpu_kernel_families import _run

pytestmark = pytest.mark.gpu

REL_TOL = 1e-6  # float32 rel against fp64 eigvalsh

_FRAMES = {}  # (case, dtype) -> the stack
_ORACLE = {}  # (case ..., precision) -> oracle outputs: one per (shape, precision), shared by the variants


def _frames(case, dtype=np.uint16):
    key = (case, np.dtype(dtype).str)
    if key not in _FRAMES:
        _FRAMES[key] = case_frames(case, dtype)[0]
    return _FRAMES[key]


def _oracle(key, img, sig, ndim, fp32):
    """fp64: (vx, vy, vz, lmin, lmax) / 2D (vx, vy, rel) of the scipy-backend oracle; fp32: the
    float32 oracle's."""
    key = key + ("fp32" if fp32 else "fp64",)
    if key not in _ORACLE:
        if fp32:
            fn = cpu_ref.calc_flow3D_fp32_oracle if ndim == 3 else cpu_ref.calc_flow2D_fp32_oracle
            _ORACLE[key] = fn(img, *sig)
        elif ndim == 3:
            _ORACLE[key] = oracle3d(img, *sig)
        else:
            _ORACLE[key] = cpu_ref.calc_flow2D(img, *sig, backend="scipy")
    return _ORACLE[key]


def _explain(name, got, want):
    """On a mismatch: how many of the differing voxels are zero in the oracle, and the first index."""
    got = np.ascontiguousarray(got).reshape(want.shape)
    it = np.uint64 if want.dtype == np.float64 else np.uint32
    if got.dtype != want.dtype:
        return f"{name}: dtype {got.dtype}, oracle {want.dtype}"
    bad = got.view(it) != want.view(it)
    if not bad.any():
        return None
    i0 = tuple(int(i) for i in np.argwhere(bad)[0])
    nz = int((bad & (want == 0)).sum())
    sign_only = int((bad & (want == 0) & (got == 0)).sum())
    msg = (f"{name}: {int(bad.sum())} of {bad.size} voxels differ from the oracle; {nz} of them are zero in the "
           f"oracle ({sign_only} differ in the sign of zero only); first at {i0}: got {got[i0]!r} want {want[i0]!r}")
    print(msg)
    return msg


def _check(got, want, ndim, fp32):
    names = ("vx", "vy", "vz")[:ndim]
    msgs = [m for m in (_explain(n, a, b) for n, a, b in zip(names, got, want)) if m]
    assert not msgs, "; ".join(msgs)
    if ndim == 2:
        if fp32:
            _check2d(got, want)
        else:
            for name, a, b in zip(("vx", "vy", "rel"), got, want):
                assert bits_equal(np.ascontiguousarray(a).reshape(b.shape), b), name
        return
    lmin, lmax = want[3], want[4]
    rel = np.asarray(got[3]).reshape(lmax.shape)
    flat = lmax == 0
    assert flat.any()  # the frames hold all-zero tensors
    off = flat & (rel != 0)
    assert not off.any(), (f"rel: {int(off.sum())} of the {int(flat.sum())} voxels whose tensor is exactly zero are not "
                           f"0; first at {tuple(int(i) for i in np.argwhere(off)[0])}: {rel[off][0]!r}")
    if fp32:
        _check3d(got, want)
    else:
        for name, a, b in zip(names, got, want):
            assert a.dtype == np.float64 and bits_equal(a.reshape(b.shape), b), name
        assert rel.dtype == np.float32
        assert_rel_within(rel, lmin, lmax, REL_TOL)


def _run_variant(img, sig, ndim, fp32, variant, monkeypatch):
    """One execution of a fresh plan under a forced variant of test_gpu_fp32_exact.VARIANTS
    -> (outputs, plan.kernels(), plan.geometry())."""
    force = VARIANTS[variant]
    for k, v in VARIANT_ENV.get(variant, {}).items():  # switches outside FAMILY_ENV: _run would not restore them
        monkeypatch.setenv(k, v)
    kernels, geom = [], {}
    out = _run(img, *sig, ndim, _lib.OF3D_FP32 if fp32 else 0, old=force is None, force=force, kernels=kernels,
               geometry=geom)
    print(f"{img.shape} {img.dtype} {sig} {'fp32' if fp32 else 'fp64'} {variant}: kernels {kernels} geometry {geom}")
    return out, kernels, geom


def _variant_params(cases, ndim):
    out = []
    for case, variants in cases:
        for fp32 in (False, True):
            for v in variants:
                if v == "k34_uq3" and not fp32:
                    continue  # the packed kernel is fp32 only
                out.append(pytest.param(case, v, fp32, id=f"{case}-{'fp32' if fp32 else 'fp64'}-{v}"))
    return out


# ---- a. every kernel family, 3D ---------------------------------------------------------------------
ALL_3D = [v for v in VARIANTS if not v.startswith("k12_zc")]
# B1f, B2f: the bright block fading (domain_frames.block_frames(fade=...)): whole windows of tx, ty,
# tz sum to -0 there, which a W accumulator started at +0.0 would turn into +0 (and vx, vy, vz
# from +0 into -0); with the constant blocks every windowed sum of zeros is +0
FAMILIES_3D = [("B1", list(VARIANTS)),  # the forced K12 march lengths: on the rd 3 volume
               ("B2", ALL_3D),
               ("B3", ["default", "k12", "k5c_nw8"]),
               ("B1f", ALL_3D),
               ("B2f", ALL_3D)]


@pytest.mark.parametrize("case,variant,fp32", _variant_params(FAMILIES_3D, 3))
def test_families_3d(case, variant, fp32, monkeypatch):
    shape, sig, _ = CASES_3D[case.rstrip("f")]
    img = _frames(case)
    out, kernels, geom = _run_variant(img, sig, 3, fp32, variant, monkeypatch)
    assert_family_ran(variant, kernels, geom, shape, sig, 3, fp32)
    if variant.startswith("k12"):
        assert "k_grad_xyz_c" in kernels, kernels  # rd 3 / 6 and 16-byte rows: an instance in both precisions
    if variant != "old":
        assert "k_tderiv_c" in kernels and "k_wz_solve_c" in kernels, kernels
    _check(out, _oracle((case,), img, sig, 3, fp32), 3, fp32)


# ---- b. the series paths ----------------------------------------------------------------------------
def _call(plan, frames, k, nwin, vol, vt, **kw):
    """Window k (frames k .. k + nwin - 1) of a series into guarded outputs."""
    import torch

    outs, check_all = poison.guarded_set(int(np.prod(vol)), [vt, vt, vt, torch.float32], "cuda")
    plan.execute([f.data_ptr() for f in frames[k:k + nwin]], _lib.OF3D_U16, 0, 0, vol[0],
                 *[o.data_ptr() for o in outs], **kw)
    torch.cuda.synchronize()
    check_all(what=f"window {k}")  # everything written, nothing beside it
    return [o.cpu().numpy().reshape(vol) for o in outs]


@pytest.mark.parametrize("fp32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("case", ["B2", "B3"])
def test_series_batched_and_next_frame_k0(case, fp32, monkeypatch):
    """A series of nwin + 5 block frames (the blocks constant in time: dt0 is exactly zero in them,
    full-range outside).  With 4 frames of lookahead window 0 forms five windows' dt0 in one
    k_tderiv_multi pass; then the same series through of3d_plan_execute_next, where the W z /
    solve kernel of window k forms window k + 1's dt0.  Each checked window against the oracle of
    its own 2 rt + 1 frames."""
    import torch

    monkeypatch.setenv("OF3D_K12", "1")  # batching rides on the fused gradient kernel's workspace
    shape, sig, seed = CASES_3D[case]
    vol = shape[1:]
    nwin = 2 * radii(*sig)[2] + 1
    assert nwin == shape[0]
    stack = block_frames((nwin + 5,) + vol, seed + 1)
    frames = [torch.from_numpy(stack[i].view(np.int16)).to("cuda") for i in range(stack.shape[0])]  # the bits
    vt = torch.float32 if fp32 else torch.float64
    mode = _lib.OF3D_FP32 if fp32 else 0
    want = lambda k: _oracle((case, "series", k), stack[k:k + nwin], sig, 3, fp32)
    plan = _lib.Plan(3, *vol, make_taps(*sig), device=0, mode=mode)
    try:
        for k in range(5):
            ahead = [f.data_ptr() for f in frames[k + nwin:k + nwin + 4]]
            got = _call(plan, frames, k, nwin, vol, vt, ahead_ptrs=ahead)
            if k == 0:
                assert plan.geometry()["k0_batch"] == 5, plan.geometry()
                assert "k_tderiv_multi" in plan.kernels(), plan.kernels()
            if k in (0, 2, 4):
                _check(got, want(k), 3, fp32)
        # one batched pass fed all five windows: no other K0 launch
        assert "k_grad_xyz_c" in plan.kernels() and not {"k_tderiv_c", "k_tderiv"} & set(plan.kernels()), plan.kernels()
    finally:
        plan.close()
    plan = _lib.Plan(3, *vol, make_taps(*sig), device=0, mode=mode)
    try:
        for k in range(3):
            nxt = [f.data_ptr() for f in frames[k + 1:k + 1 + nwin]] if k < 2 else None
            got = _call(plan, frames, k, nwin, vol, vt, next_ptrs=nxt, pipelined=True)
            if k == 0:
                assert "k_wz_solve_c_next" in plan.kernels(), plan.kernels()
            else:  # windows whose dt0 the previous call's W z / solve kernel formed
                _check(got, want(k), 3, fp32)
        assert "k_tderiv_multi" not in plan.kernels(), plan.kernels()
    finally:
        plan.close()


# ---- c. the input types with fused instances ----------------------------------------------------------
@pytest.mark.parametrize("fp32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("variant", ["default", "k12"])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["uint8", "float32"])
def test_fused_input_types(dtype, variant, fp32, monkeypatch):
    """B1 as uint8 (whole range, saturated at 255) and as float32 (the uint16 stack, the noise
    0.25 off the integers): the (K0c, K1c, K12) x (u8, f32) rows of the dispatch tables."""
    shape, sig, _ = CASES_3D["B1"]
    img = _frames("B1", dtype)
    out, kernels, geom = _run_variant(img, sig, 3, fp32, variant, monkeypatch)
    assert_family_ran(variant, kernels, geom, shape, sig, 3, fp32)  # (nx 96: 16-byte rows in every type)
    assert "k_tderiv_c" in kernels, kernels
    assert ("k_grad_xyz_c" if variant == "k12" else "k_grad_xy_c") in kernels, kernels
    _check(out, _oracle(("B1", np.dtype(dtype).str), img, sig, 3, fp32), 3, fp32)


def test_int16_runs_legacy_gradients():
    """int16 frames (both signs, the blocks at 32767 and 0) have no fused K0 / K1c / K12 instance:
    the plan must report the runtime-radius kernels, and match the oracle."""
    shape, sig, _ = CASES_3D["B1"]
    img = _frames("B1", np.int16)
    assert img.min() == -32768 and img.max() == 32767
    kernels = []
    out = _run(img, *sig, 3, 0, old=False, kernels=kernels)
    assert not {"k_grad_xy_c", "k_grad_xyz_c", "k_tderiv_c"} & set(kernels), kernels
    assert {"k_grad_xy", "k_tderiv"} <= set(kernels), kernels
    _check(out, _oracle(("B1", "int16"), img, sig, 3, False), 3, False)


# ---- d. 2D ----------------------------------------------------------------------------------------------
FAMILIES_2D = [(c, ["default", "old", "k34_uq0", "k34_uq1", "k34_uq2", "k34_uq3"]) for c in list(CASES_2D) + ["P1f"]]


@pytest.mark.parametrize("case,variant,fp32", _variant_params(FAMILIES_2D, 2))
def test_families_2d(case, variant, fp32, monkeypatch):
    shape, sig, _ = CASES_2D[case.rstrip("f")]
    img = _frames(case)
    out, kernels, geom = _run_variant(img, sig, 2, fp32, variant, monkeypatch)
    assert_family_ran(variant, kernels, geom, shape, sig, 2, fp32)
    assert "k_solve2d" in kernels, kernels
    _check(out, _oracle((case,), img, sig, 2, fp32), 2, fp32)


def test_host_entry_2d():
    shape, sig, _ = CASES_2D["P1"]
    img = _frames("P1")
    _check(calc_flow2D(img, *sig), _oracle(("P1",), img, sig, 2, False), 2, False)


def test_host_entry_3d():
    shape, sig, _ = CASES_3D["B1"]
    img = _frames("B1")
    _check(calc_flow3D(img, *sig), _oracle(("B1",), img, sig, 3, False), 3, False)
