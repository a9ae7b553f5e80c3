"""The runtime-radius kernels (k_grad_xy, k_grad_z, k_prod_wy + k_wx, k_wz_solve_dma /
k_wz_solve) on every radius rung they serve, against the oracle.

Parameter sets without a fused instance (K1c / K12 at (rd, rs) = (3,1), (6,2), (9,3); K34 /
K5c at rw 9, 12, 15, 18, 21) and below the general path's limits (rd <= 24, rw <= 48) run
these kernels by default (wSig 8, xyzSig 4, ...).  Their getters pick a template instance and
a block geometry from the radius; of3d_plan_geometry reports the pick as "runtime_radius"
(from the functions the getters switch on), and every case here asserts the kernel families
that ran, the exact rung, and that the general path ran only where it is meant to.

Contracts (the suite's existing ones, no new tolerance):
  fp64        vx, vy, vz bit-identical to oracle.cpu_ref (scipy backend), rel within
              1e-6 lambda_max of fp64 eigvalsh; OF3D_REL_F64: rel within 1e-10 lambda_max
  OF3D_FP32   bit-identical to the float32 oracle (test_gpu_fp32_exact._check3d / _check2d)
  2D fp64     vx, vy, rel bit-identical

Inputs are seeded uniform integers over the whole range of the dtype (bit 15 of uint16 set,
both signs of the signed types, uint32 above 2^31), floats uniform in (-5e4, 6.5e4).

Rung -> case (rw / rd are asserted against radii() of the case's sigmas):
  k_grad_xy NJ 8        rd 2 (test_small_end), rd 8 (test_d_ladder)
  k_grad_xy NJ 12       rd 10, 16 (test_d_ladder); rd 16, every dtype (test_d_dtypes)
  k_grad_xy NJ 16       rd 17, 24 (test_d_ladder); rd 24, every dtype (test_d_dtypes)
  k_prod_wy TJ 8        rw 2 (test_small_end), rw 16 (test_w_ladder)
  k_prod_wy TJ 12       rw 17, 24
  k_prod_wy TJ 24       rw 25 .. 48
  k_wx TJ 1 / 2 / 3     rw 2, 16 / rw 17, 24, 25, 32 / rw 33 .. 48
  k_wz_solve R 8 NJ 12  rw 2, 16 (nx 65 / 71: rows no 16-byte multiple)
  k_wz_solve R 8 NJ 14  rw 17, 24 (nx 71)
  k_wz_solve R 4 NJ 12  rw 25, 32 (nx 71)
  k_wz_solve R 4 NJ 16  rw 33, 39, 40, 48 (nx 71)
  k_wz_solve_dma fp64   R 8: NJ2 6 rw 2, 16; NJ2 7 rw 17, 22, 24; two buffers at rw 22, 24
                        R 4: NJ2 6 rw 25, 32; NJ2 7 rw 33, 37 .. 40; NJ2 8 rw 41, 48;
                        three buffers up to rw 37, two from rw 38 (test_w_dma_seams_fp64)
  k_wz_solve_dma fp32   R 8: NJ2 3 rw 2, 16; NJ2 4 rw 17, 24   R 4: NJ2 3 rw 25, 32; NJ2 4 rw 33 .. 48
  tiled -> general      (24, 6, 3, 48) tiled; rw 49 and rd 25 general (test_switch_to_general)
(k_wz_solve<.., 10, 4, 8> is compiled but no radius reaches it: R = 4 starts at rw 25, where
the window already needs 11 rows per thread.)"""
import numpy as np
import pytest

import poison
from conftest import assert_rel_within, bits_equal, oracle3d
from opticalflow3d_dev_amd import _lib, make_taps, radii
from oracle import cpu_ref
from test_gpu_fp32_exact import _check2d, _check3d

pytestmark = pytest.mark.gpu

REL_TOL = 1e-6        # float32 rel against fp64 eigvalsh
REL_TOL_FP64 = 1e-10  # OF3D_REL_F64

ALL_DTYPES = (np.uint8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64)

_ORACLE = {}  # key -> oracle outputs of the cases several tests share


def _full_range(shape, dtype, seed):
    """Seeded uniform values over the whole range of an integer dtype; floats in (-5e4, 6.5e4)."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return rng.uniform(-5e4, 6.5e4, size=shape).astype(dt)
    ii = np.iinfo(dt)
    img = rng.integers(ii.min, ii.max, size=shape, dtype=dt, endpoint=True)
    assert img.max() > ii.max - (ii.max - ii.min) // 64 and img.min() < ii.min + (ii.max - ii.min) // 64
    return img


def _oracle(img, sig, ndim, fp32, taps=None, key=None):
    """fp64: (vx, vy, vz, lmin, lmax) / 2D (vx, vy, rel) of the scipy-backend oracle; fp32: the
    float32 oracle's.  key: kept for the other tests of the same case."""
    if key is not None and key in _ORACLE:
        return _ORACLE[key]
    if fp32:
        fn = cpu_ref.calc_flow3D_fp32_oracle if ndim == 3 else cpu_ref.calc_flow2D_fp32_oracle
        out = fn(img, *sig, taps=taps)
    elif ndim == 2:
        out = cpu_ref.calc_flow2D(img, *sig, backend="scipy")
    elif taps is None:
        out = oracle3d(img, *sig)
    else:
        st = cpu_ref.structure_tensor3d(img, *sig, backend="scipy", taps=taps)
        out = cpu_ref.solve3d(st) + cpu_ref.eig_fp64_3d(st)
    if key is not None:
        _ORACLE[key] = out
    return out


def _run(img, taps, ndim, mode, zout=None, max_out_planes=0):
    """One execution of a fresh plan on img's centre window (any input dtype), output planes
    zout (default all) -> (outputs, plan.kernels(), plan.geometry(), plan.input_range(*zout))."""
    import torch

    dev = torch.device("cuda", 0)
    vol = img.shape[1:] if ndim == 3 else (1,) + img.shape[1:]
    nz, ny, nx = vol
    rt = len(taps["tderiv"]) // 2
    c = img.shape[0] // 2
    win = np.ascontiguousarray(img[c - rt:c + rt + 1])
    d_in = torch.from_numpy(win.view(np.uint8).reshape(2 * rt + 1, -1)).to(dev)
    z0, z1 = zout or (0, nz)
    fp32 = bool(mode & _lib.OF3D_FP32)
    vt = torch.float32 if fp32 else torch.float64
    if ndim == 2:
        rt_ = vt
    else:
        rt_ = torch.float64 if mode & _lib.OF3D_REL_F64 else torch.float32
    n = (z1 - z0) * ny * nx
    (*outs, rel), check_all = poison.guarded_set(n, [vt, vt, vt, rt_], dev)
    plan = _lib.Plan(ndim, nz, ny, nx, taps, device=0, mode=mode, max_out_planes=max_out_planes)
    try:
        zin = plan.input_range(z0, z1)
        plan.execute([d_in[i].data_ptr() for i in range(2 * rt + 1)], _lib.DTYPE_CODES[img.dtype], 0, z0, z1,
                     outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), rel.data_ptr())
        torch.cuda.synchronize(dev)
        check_all(used=(0, 1, 2, 3) if ndim == 3 else (0, 1, 3))  # everything written, nothing beside it
        kernels, geom = plan.kernels(), plan.geometry()
    finally:
        plan.close()
    shape = (z1 - z0, ny, nx) if ndim == 3 else (ny, nx)
    res = [o.cpu().numpy().reshape(shape) for o in outs[:ndim]] + [rel.cpu().numpy().reshape(shape)]
    return res, kernels, geom, zin


def _check(got, want, ndim, fp32, rel_tol=REL_TOL):
    if fp32:
        (_check3d if ndim == 3 else _check2d)(got, want)
    elif ndim == 2:
        for name, a, b in zip(("vx", "vy", "rel"), got, want):
            assert bits_equal(a, b), name
    else:
        for name, a, b in zip(("vx", "vy", "vz"), got[:3], want[:3]):
            assert a.dtype == np.float64 and bits_equal(a, b), name
        assert got[3].dtype == (np.float64 if rel_tol == REL_TOL_FP64 else np.float32)
        assert_rel_within(got[3], want[3], want[4], rel_tol)


# ---- which kernels and rungs a case must report -------------------------------------------------
FUSED = {"k_grad_xy_c", "k_grad_xyz_c", "k_grad_z_c", "k_prod_wyx", "k_prod_wyx_ws", "k_prod_wyx_pk", "k_wz_solve_c",
         "k_wz_solve_c_next"}
FUSED_W = {k for k in FUSED if k.startswith(("k_prod_wyx", "k_wz_solve_c"))}
FUSED_D = FUSED - FUSED_W

# window radius -> (k_prod_wy TJ, k_wx TJ, (k_wz_solve R, NJ), fp64 k_wz_solve_dma (NB, NJ2), fp32 (NB, NJ2)),
# worked out by hand from the kernels' staging (rows per thread x threads >= rows of the window;
# NB buffers of ceil((8 R + 2 rw) / (16 B / sizeof F)) KiB within 160 KiB), not from the getters
W_RUNGS = {
    2: (8, 1, (8, 12), (3, 6), (3, 3)),
    16: (8, 1, (8, 12), (3, 6), (3, 3)),
    17: (12, 2, (8, 14), (3, 7), (3, 4)),
    22: (12, 2, (8, 14), (2, 7), (3, 4)),
    24: (12, 2, (8, 14), (2, 7), (3, 4)),
    25: (24, 2, (4, 12), (3, 6), (3, 3)),
    32: (24, 2, (4, 12), (3, 6), (3, 3)),
    33: (24, 3, (4, 16), (3, 7), (3, 4)),
    37: (24, 3, (4, 16), (3, 7), (3, 4)),
    38: (24, 3, (4, 16), (2, 7), (3, 4)),
    39: (24, 3, (4, 16), (2, 7), (3, 4)),
    40: (24, 3, (4, 16), (2, 7), (3, 4)),
    41: (24, 3, (4, 16), (2, 8), (3, 4)),
    48: (24, 3, (4, 16), (2, 8), (3, 4)),
}
D_RUNGS = {2: 8, 3: 8, 8: 8, 10: 12, 16: 12, 17: 16, 24: 16}  # gradient radius -> k_grad_xy NJ


def _assert_tiled(kernels, geom):
    rr = geom["runtime_radius"]
    assert "general" not in kernels and geom["general"] == 0 and rr["general"] is False, (kernels, geom)
    return rr


def _assert_w_rung(kernels, geom, rw, ndim, nx, fp32):
    """The runtime-radius W kernels ran, on rw's rung; 3D: the LDS-DMA W z where rows are 16-byte
    multiples of the pass type, else the register-staged one."""
    rr = _assert_tiled(kernels, geom)
    k3, k4, k5, dma64, dma32 = W_RUNGS[rw]
    assert {"k_prod_wy", "k_wx"} <= set(kernels) and not FUSED_W & set(kernels), kernels
    assert (rr["k3_tj"], rr["k4_tj"]) == (k3, k4), rr
    if ndim == 2:
        assert "k_solve2d" in kernels and not {"k_wz_solve_dma", "k_wz_solve"} & set(kernels), kernels
        return
    assert (rr["k5"]["r"], rr["k5"]["nj"]) == k5, rr
    dma = nx % (4 if fp32 else 2) == 0
    assert ("k_wz_solve_dma" in kernels) == dma and ("k_wz_solve" in kernels) == (not dma), (kernels, nx)
    want = (dma32 if fp32 else dma64) if dma else (0, 0)
    assert (rr["k5_dma"]["nb"], rr["k5_dma"]["nj2"]) == want, rr


def _assert_d_rung(kernels, geom, rd, ndim):
    """k_grad_xy (+ k_grad_z in 3D) ran, on rd's rung, and no fused gradient kernel."""
    rr = _assert_tiled(kernels, geom)
    assert "k_grad_xy" in kernels and not FUSED_D & set(kernels), kernels
    assert ndim == 2 or "k_grad_z" in kernels, kernels
    assert rr["k1_nj"] == D_RUNGS[rd], rr


# ---- W ladder -----------------------------------------------------------------------------------
# xyzSig 1, tSig 1 (fused gradients), uint16, nt 7.  ny 70: above K4_ROWS = 64, two K3_STEP = 32
# marches and a tail; nz 66 up to rw 24: two 64-plane R = 8 blocks; nz 36 from rw 25: two 32-plane
# R = 4 blocks.  nx 72: 16-byte rows in both precisions (LDS-DMA W z); nx 71: the register-staged one.
W_LADDER = [(5.3, 16), (5.5, 17), (8, 24), (8.2, 25), (10.5, 32), (11, 33), (13, 39), (13.2, 40), (16, 48)]


def _w_shape(rw, nx):
    return (7, 66 if rw <= 24 else 36, 70, nx)


def _w_case(wsig, rw, nx, fp32, mode=0, key=None):
    sig = (1, 1, wsig)
    assert radii(*sig) == (3, 1, 3, rw)
    shape = _w_shape(rw, nx)
    img = _full_range(shape, np.uint16, 5000 + shape[1] + nx)
    got, kernels, geom, _ = _run(img, make_taps(*sig), 3, mode | (_lib.OF3D_FP32 if fp32 else 0))
    print(f"{shape} {sig}: {kernels} {geom['runtime_radius']}")
    _assert_w_rung(kernels, geom, rw, 3, nx, fp32)
    return got, _oracle(img, sig, 3, fp32, key=key)


@pytest.mark.parametrize("fp32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("nx", [72, 71])
@pytest.mark.parametrize("wsig,rw", W_LADDER)
def test_w_ladder(wsig, rw, nx, fp32):
    keep = ("w", rw) if (rw in (25, 48) and nx == 72 and not fp32) else None  # test_w_rel_fp64's too
    got, want = _w_case(wsig, rw, nx, fp32, key=keep)
    _check(got, want, 3, fp32)


@pytest.mark.parametrize("wsig,rw", [(7.2, 22), (12.3, 37), (12.5, 38), (13.5, 41)])
def test_w_dma_seams_fp64(wsig, rw):
    """The fp64 LDS-DMA W z at the radii the ladder leaves between its window-buffer and row-group
    steps: three buffers up to rw 21 / 37 and two from 22 / 38; NJ2 8 from rw 41."""
    got, want = _w_case(wsig, rw, 72, False)
    _check(got, want, 3, False)


@pytest.mark.parametrize("wsig,rw", [(8.2, 25), (16, 48)])
def test_w_rel_fp64(wsig, rw):
    got, want = _w_case(wsig, rw, 72, False, mode=_lib.OF3D_REL_F64, key=("w", rw))
    _check(got, want, 3, False, rel_tol=REL_TOL_FP64)


@pytest.mark.parametrize("fp32", [False, True], ids=["fp64", "fp32"])
def test_w_thin_volume_all_clamped(fp32):
    """(3, 5, 20) voxels under a rw 48 window: every tap of every W pass clamps."""
    sig = (1, 1, 16)
    assert radii(*sig) == (3, 1, 3, 48)
    img = _full_range((7, 3, 5, 20), np.uint16, 5100)
    got, kernels, geom, _ = _run(img, make_taps(*sig), 3, _lib.OF3D_FP32 if fp32 else 0)
    _assert_w_rung(kernels, geom, 48, 3, 20, fp32)
    _check(got, _oracle(img, sig, 3, fp32), 3, fp32)


# ---- D ladder -----------------------------------------------------------------------------------
# wSig 4, tSig 1 (fused W kernels), nt 7.  (20, 40, 40): 2-3 column strips at rd 16 and 24 (strips
# of 64 - 2 rd outputs), three row tiles with a partial last one, five K1_NZB groups, two K2_ZC blocks.
D_LADDER = [(2.6, 8, 2), (3.2, 10, 3), (5.3, 16, 4), (5.5, 17, 5), (8, 24, 6)]


def _d_case(xsig, rd, rs, shape, dtype, fp32):
    sig = (xsig, 1, 4)
    assert radii(*sig) == (rd, rs, 3, 12)
    img = _full_range(shape, dtype, 5200 + rd + np.dtype(dtype).num)
    got, kernels, geom, _ = _run(img, make_taps(*sig), 3, _lib.OF3D_FP32 if fp32 else 0)
    print(f"{shape} {sig} {np.dtype(dtype)}: {kernels} {geom['runtime_radius']}")
    _assert_d_rung(kernels, geom, rd, 3)
    assert FUSED_W & set(kernels) and not {"k_prod_wy", "k_wx"} & set(kernels), kernels
    _check(got, _oracle(img, sig, 3, fp32), 3, fp32)


@pytest.mark.parametrize("fp32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("xsig,rd,rs", D_LADDER)
def test_d_ladder(xsig, rd, rs, fp32):
    _d_case(xsig, rd, rs, (7, 20, 40, 40), np.uint16, fp32)


def _d_dtype_params():
    out = []
    for xsig, rd, rs in ((5.3, 16, 4), (8, 24, 6)):  # NJ 12, NJ 16
        out += [pytest.param(xsig, rd, rs, dt, False, id=f"rd{rd}-{np.dtype(dt)}-fp64") for dt in ALL_DTYPES]
        out += [pytest.param(xsig, rd, rs, dt, True, id=f"rd{rd}-{np.dtype(dt)}-fp32")
                for dt in (np.uint8, np.float32, np.int32)]
    return out


@pytest.mark.parametrize("xsig,rd,rs,dtype,fp32", _d_dtype_params())
def test_d_dtypes(xsig, rd, rs, dtype, fp32):
    """k_grad_xy is templated on the input type: every type on the NJ 12 and NJ 16 rungs."""
    _d_case(xsig, rd, rs, (7, 6, 40, 40), dtype, fp32)


# ---- the switch to the general path ---------------------------------------------------------------
@pytest.mark.parametrize("fp32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("sig,rad,general", [((8, 1, 16), (24, 6, 3, 48), False),
                                             ((8, 1, 16.2), (24, 6, 3, 49), True),
                                             ((8.2, 1, 16), (25, 7, 3, 48), True)])
def test_switch_to_general(sig, rad, general, fp32):
    """The largest radii of the tiled kernels, (24, 6, 3, 48): every runtime-radius kernel on its
    top rung at once; one more in rw or in rd: the general path, and nothing else."""
    assert radii(*sig) == rad
    shape = (7, 36, 70, 72)
    img = _full_range(shape, np.uint16, 5300)
    got, kernels, geom, _ = _run(img, make_taps(*sig), 3, _lib.OF3D_FP32 if fp32 else 0)
    rr = geom["runtime_radius"]
    if general:
        assert kernels == ["general"] and geom["general"] == 1 and rr["general"] is True, (kernels, geom)
        assert (rr["k1_nj"], rr["k3_tj"], rr["k4_tj"], rr["k5"]["nj"], rr["k5_dma"]["nb"]) == (0, 0, 0, 0, 0), rr
    else:
        _assert_d_rung(kernels, geom, 24, 3)
        _assert_w_rung(kernels, geom, 48, 3, 72, fp32)
        assert not FUSED & set(kernels), kernels
    _check(got, _oracle(img, sig, 3, fp32), 3, fp32)


# ---- the small end --------------------------------------------------------------------------------
@pytest.mark.parametrize("fp32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("nx", [65, 64])
def test_small_end(nx, fp32):
    """Sigmas (0.5, 0.5, 0.5), radii (2, 1, 2, 2): the lowest rung of every kernel and a temporal
    radius the compile-time K0 has no instance for (nx 64: the LDS-DMA W z; 65: register-staged)."""
    sig = (0.5, 0.5, 0.5)
    assert radii(*sig) == (2, 1, 2, 2)
    img = _full_range((5, 9, 33, nx), np.uint16, 5400 + nx)
    got, kernels, geom, _ = _run(img, make_taps(*sig), 3, _lib.OF3D_FP32 if fp32 else 0)
    _assert_d_rung(kernels, geom, 2, 3)
    _assert_w_rung(kernels, geom, 2, 3, nx, fp32)
    assert "k_tderiv" in kernels and not FUSED & set(kernels) and "k_tderiv_c" not in kernels, kernels
    _check(got, _oracle(img, sig, 3, fp32), 3, fp32)


# ---- 2D: five products, k_solve2d -------------------------------------------------------------------
def _2d_params():
    out = []
    for wsig, rw in ((8.2, 25), (11, 33), (16, 48)):
        out += [pytest.param((1, 1, wsig), (3, 1, 3, rw), (7, 70, nx), id=f"rw{rw}-nx{nx}") for nx in (72, 71)]
    out += [pytest.param((xs, 1, 4), (rd, rs, 3, 12), (7, 40, 40), id=f"rd{rd}")
            for xs, rd, rs in ((5.5, 17, 5), (8, 24, 6))]
    return out


@pytest.mark.parametrize("fp32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("sig,rad,shape", _2d_params())
def test_2d(sig, rad, shape, fp32):
    assert radii(*sig) == rad
    img = _full_range(shape, np.uint16, 5500 + shape[-1])
    got, kernels, geom, _ = _run(img, make_taps(*sig), 2, _lib.OF3D_FP32 if fp32 else 0)
    print(f"{shape} {sig}: {kernels} {geom['runtime_radius']}")
    assert "k_solve2d" in kernels, kernels
    if rad[0] == 3:
        _assert_w_rung(kernels, geom, rad[3], 2, shape[-1], fp32)
    else:
        _assert_d_rung(kernels, geom, rad[0], 2)
        assert FUSED_W & set(kernels) and not {"k_prod_wy", "k_wx"} & set(kernels), kernels
    _check(got, _oracle(img, sig, 2, fp32), 2, fp32)


# ---- z-slabs on this band ---------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_zslabs(world, monkeypatch):
    """Slabs thinner than the rd + rw = 35 halo, every plane range clamped at the volume's edge:
    bit-identical to the oracle of the whole volume, every slab on the NJ 12 / R = 4 rungs."""
    from opticalflow3d_dev_amd.shard import flow3d_zslabs_host

    sig = (3.2, 1, 8.2)
    assert radii(*sig) == (10, 3, 3, 25)
    img = _full_range((7, 40, 24, 28), np.uint16, 5600)
    seen = []
    close = _lib.Plan.close

    def recording_close(plan):
        if getattr(plan, "handle", None):
            seen.append((plan.kernels(), plan.geometry()))
        close(plan)

    monkeypatch.setattr(_lib.Plan, "close", recording_close)
    got = flow3d_zslabs_host(img, *sig, world)
    assert len(seen) == world
    for kernels, geom in seen:
        _assert_d_rung(kernels, geom, 10, 3)
        _assert_w_rung(kernels, geom, 25, 3, 28, False)
    _check(got, _oracle(img, sig, 3, False, key="zslabs"), 3, False)


# ---- caller-made taps with rs > rd --------------------------------------------------------------------
@pytest.mark.parametrize("fp32", [False, True], ids=["fp64", "fp32"])
def test_smooth_radius_above_gradient_radius(fp32):
    """Taps the C ABI accepts but make_taps never builds: gauss / deriv of xyzSig 1 (rd 3) with the
    smooth of sigma 1.5 (rs 5).  The tiled gradient kernels stage an rd halo only, so such a plan
    takes the general path; a plane range's input halo is rw + max(rd, rs)."""
    taps = dict(make_taps(1, 1, 2), smooth=make_taps(6, 1, 2)["smooth"])
    assert [len(taps[k]) // 2 for k in ("gauss", "deriv", "smooth", "tderiv", "window")] == [3, 3, 5, 3, 6]
    img = _full_range((7, 20, 21, 37), np.uint16, 5700)
    mode = _lib.OF3D_FP32 if fp32 else 0
    want = _oracle(img, (1, 1, 2), 3, fp32, taps=taps)
    got, kernels, geom, _ = _run(img, taps, 3, mode)
    assert kernels == ["general"] and geom["runtime_radius"]["general"] is True, (kernels, geom)
    _check(got, want, 3, fp32)
    # output planes [0, 4): gradients on [0, 10), whose z smooth reads input planes up to 14
    part, kernels, _, zin = _run(img, taps, 3, mode, zout=(0, 4), max_out_planes=4)
    assert kernels == ["general"] and zin == (0, 15), (kernels, zin)
    _check(part, tuple(w[:4] for w in want), 3, fp32)
