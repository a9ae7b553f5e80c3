"""The fp32 mode (OF3D_FP32, configs[4]) against the float32 restatement of the oracle
(oracle.cpu_ref, dtype float32), bit for bit.

The mode is fully specified: frames cast to float32, taps rounded to nearest float32, every
pass and product in float32 in the scipy symmetric order with no FMA contraction, the solve
and the eigenvalue in fp64 on the promoted float32 tensor, results rounded to float32.  So
every kernel instance of the mode is held to the oracle at every voxel:

  * vx, vy, vz: bit-identical (signed zeros included);
  * 2D rel: bit-identical, NaN at the same pixels;
  * 3D rel (float32): within 1e-6 * lambda_max of fp64 eigvalsh of the promoted tensor.

Each forced kernel family also proves through plan.kernels() / plan.geometry() that it ran
(or, where the shape makes it ineligible on purpose, that the fallback ran).  The max-norm
tests (test_gpu_fp32.py, test_gpu_oracle_paths.py) pin the accuracy against fp64: another
claim."""
import numpy as np
import pytest

from conftest import assert_rel_within, bits_equal, golden_cases, load_golden, oracle3d
from opticalflow3d_dev_amd import _lib, calc_flow2D_fp32, calc_flow3D, calc_flow3D_fp32, make_taps, radii
from oracle import cpu_ref
from test_gpu_k0batch import NX, NY, NZ
from test_gpu_k0batch import _call as _batch_call
from test_gpu_k0batch import _series as _batch_series
from test_gpu_kernel_families import CASES, W_RADII, _run
from test_gpu_parity import SEEDED_2D, SEEDED_3D, _rand
from test_gpu_pipeline import _run as _pipe_run
from test_gpu_pipeline import _series as _pipe_series

pytestmark = pytest.mark.gpu

REL_TOL = 1e-6

_ORACLE = {}  # key -> the float32 oracle's outputs: computed once, shared by the forced variants


def _oracle(key, img, sig, ndim):
    if key not in _ORACLE:
        fn = cpu_ref.calc_flow3D_fp32_oracle if ndim == 3 else cpu_ref.calc_flow2D_fp32_oracle
        _ORACLE[key] = fn(img, *sig)
    return _ORACLE[key]


def _same_bits(name, got, want):
    got = np.ascontiguousarray(got).reshape(want.shape)
    assert got.dtype == np.float32 and want.dtype == np.float32, (name, got.dtype, want.dtype)
    if bits_equal(got, want):
        return
    bad = got.view(np.uint32) != want.view(np.uint32)
    idx = np.argwhere(bad)
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    ulp = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    i0 = tuple(idx[0])
    raise AssertionError(
        f"{name}: {bad.sum()} of {bad.size} values differ from the float32 oracle; max |d| {np.nanmax(d):.3e} "
        f"(max |v| {np.nanmax(np.abs(want)):.3e}), max distance {ulp[bad].max()} ulp; first at {i0}: got "
        f"{got[i0]!r} want {want[i0]!r}; index box {idx.min(axis=0).tolist()} .. {idx.max(axis=0).tolist()}")


def _check3d(got, want):
    vx, vy, vz, lmin, lmax = want
    for name, a, b in zip(("vx", "vy", "vz"), got[:3], (vx, vy, vz)):
        _same_bits(name, a, b)
    rel = np.asarray(got[3])
    assert rel.dtype == np.float32
    assert_rel_within(rel.reshape(lmin.shape), lmin, lmax, REL_TOL)


def _check2d(got, want):
    for name, a, b in zip(("vx", "vy"), got[:2], want[:2]):
        _same_bits(name, a, b)
    rel = np.ascontiguousarray(got[2]).reshape(want[2].shape)
    assert rel.dtype == np.float32
    nan = np.isnan(want[2])
    assert np.array_equal(np.isnan(rel), nan), "rel: NaN at other pixels"
    _same_bits("rel", np.where(nan, np.float32(0), rel), np.where(nan, np.float32(0), want[2]))


# ---- 1. the goldens -------------------------------------------------------------------------
@pytest.mark.parametrize("name", golden_cases("c3d"))
def test_golden_3d_fp32_exact(name):
    g = load_golden(name)
    sig = (g["sig"], g["tsig"], g["wsig"])
    _check3d(calc_flow3D_fp32(g["images"], *sig), _oracle(("golden", name), g["images"], sig, 3))


@pytest.mark.parametrize("name", golden_cases("c2d"))
def test_golden_2d_fp32_exact(name):
    g = load_golden(name)
    sig = (g["sig"], g["tsig"], g["wsig"])
    _check2d(calc_flow2D_fp32(g["images"], *sig), _oracle(("golden", name), g["images"], sig, 2))


# ---- 2. shapes and input dtypes ---------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(SEEDED_3D)))
def test_seeded_3d_fp32_exact(case):
    shape, sig, dt = SEEDED_3D[case]
    img = _rand(shape, dt, 100 + case)
    _check3d(calc_flow3D_fp32(img, *sig), _oracle(("seeded3", case), img, sig, 3))


@pytest.mark.parametrize("case", range(len(SEEDED_2D)))
def test_seeded_2d_fp32_exact(case):
    shape, sig, dt = SEEDED_2D[case]
    img = _rand(shape, dt, 200 + case)
    _check2d(calc_flow2D_fp32(img, *sig), _oracle(("seeded2", case), img, sig, 2))


@pytest.mark.parametrize("dtype", cpu_ref.CAST_DTYPES)
def test_input_cast_fp32_exact(dtype):
    """Inputs a float32 cannot hold (integers above 2^24, float64 fractions): the device casts
    each frame to float32 first, rounding to nearest, as the oracle's astype does."""
    img = cpu_ref.cast_case_images((7, 6, 20, 24), dtype, 78)
    assert (img.astype(np.float32).astype(np.float64) != img.astype(np.float64)).mean() > 0.3
    sig = (1, 1, 2)
    _check3d(calc_flow3D_fp32(img, *sig), _oracle(("cast3", np.dtype(dtype).str), img, sig, 3))
    _check2d(calc_flow2D_fp32(img[:, 3], *sig), _oracle(("cast2", np.dtype(dtype).str), img[:, 3], sig, 2))


# ---- 3. degenerate 3D extents ------------------------------------------------------------------
DEGENERATE = [(7, 1, 12, 16), (7, 6, 1, 16), (7, 6, 12, 1), (7, 1, 1, 1)]


@pytest.mark.parametrize("shape", DEGENERATE)
@pytest.mark.parametrize("fp32", [True, False])
def test_degenerate_extents(shape, fp32):
    """One-voxel extents along z, y, x and all three, sigma (1, 1, 2): every tap clamps to the
    one plane / row / column.  fp32 against the float32 oracle, fp64 against the fp64 oracle."""
    sig = (1, 1, 2)
    img = np.random.default_rng(sum(shape)).integers(0, 4096, size=shape).astype(np.uint16)
    if fp32:
        _check3d(calc_flow3D_fp32(img, *sig), _oracle(("degenerate", shape), img, sig, 3))
    else:
        vx, vy, vz, lmin, lmax = oracle3d(img, *sig)
        got = calc_flow3D(img, *sig)
        for a, b in zip(got[:3], (vx, vy, vz)):
            assert bits_equal(a, b)
        assert_rel_within(got[3], lmin, lmax, REL_TOL)


# ---- 4. every fp32 kernel family against the oracle -------------------------------------------
def _aligned(shape):
    """nx rounded up to a multiple of 32: 16-byte rows for K12 (uint16 frames: nx % 8) and K5c
    (float fields: nx % 4), whole 32-column tiles for the z-tiled W-xy layout."""
    return shape[:-1] + ((shape[-1] + 31) // 32 * 32,)


# (shape, sigmas, ndim): the kernel-family shapes, each radius set with an aligned nx and with
# the original nx, which is not (266, 530: no K12, no K5c, no tiles; 140, 268: K5c but no K12;
# 200: K12 and K5c but no tiles)
FAMILY_SHAPES = (
    [(_aligned(s), sig, nd) for s, sig, nd in CASES] + list(CASES) +
    [(_aligned(s), sig, nd) for s, sig, nd in W_RADII] + list(W_RADII) +
    [((13, 45, 70, 232), (1, 2, 5), 3)]
)

K5C_RW = (9, 12, 15, 18, 21)  # window radii with a compiled K5c / fused K34 instance
# (the old family of test_gpu_kernel_families.FAMILY_ENV keeps the compile-time K0 and the z march K2c)
NEW_NAMES = ("k_grad_xy_c", "k_grad_xyz_c", "k_prod_wyx", "k_prod_wyx_ws", "k_prod_wyx_pk", "k_wz_solve_c",
             "k_wz_solve_c_next")

VARIANTS = {
    "default": {},
    "old": None,
    "k12": {"OF3D_K12": "1"},
    "k12_zc16": {"OF3D_K12": "1", "OF3D_K12_ZC": "16"},
    "k12_zc40": {"OF3D_K12": "1", "OF3D_K12_ZC": "40"},
    "k34_uq0": {"OF3D_K34_UQ": "0"},
    "k34_uq1": {"OF3D_K34_UQ": "1"},
    "k34_uq2": {"OF3D_K34_UQ": "2"},
    "k34_uq3": {"OF3D_K34_UQ": "3"},
    "k5c_nw8": {"OF3D_K5C_NW": "8"},
    "wxy_plain": {"OF3D_WXY_TILE": "0"},
    "wxy_tiled": {"OF3D_WXY_TILE": "1"},
}
# OF3D_K34_UQ=2 leaves the wave-specialised and the packed candidates to the autotune, which is
# free to time the packed one faster: without the packed ones it has to be k_prod_wyx_ws
# (OF3D_K34_UQ=1 likewise drops only the duplicate-staging candidates: without the wave-specialised
# and the packed ones the unique-staging instance is all that is left)
VARIANT_ENV = {"k34_uq1": {"OF3D_K34_PK": "0", "OF3D_K34_WS": "0"}, "k34_uq2": {"OF3D_K34_PK": "0"}}


def _family_params():
    out = []
    for i, (shape, sig, nd) in enumerate(FAMILY_SHAPES):
        for v in VARIANTS:
            if v in ("k12_zc16", "k12_zc40") and radii(*sig)[0] != 3:
                continue  # the forced march lengths: on the rd 3 volume
            if nd == 2 and (v.startswith("k12") or v.startswith("k5c") or v.startswith("wxy")):
                continue  # 3D kernels
            out.append(pytest.param(i, v, id=f"{'x'.join(map(str, shape))}-{v}"))
    return out


def _run_plan(img, sig, ndim, force, old=False, env=None, monkeypatch=None):
    """test_gpu_kernel_families._run in fp32 plus the plan's kernel list and geometry."""
    kernels, geom = [], {}
    for k, v in (env or {}).items():  # switches outside FAMILY_ENV: _run would not restore them
        monkeypatch.setenv(k, v)
    out = _run(img, *sig, ndim, _lib.OF3D_FP32, old=old, force=force, kernels=kernels, geometry=geom)
    return out, kernels, geom


def _family_image(i):
    shape, sig, nd = FAMILY_SHAPES[i]
    img = np.random.default_rng(1000 + i).integers(0, 4096, size=shape).astype(np.uint16)
    return img[:, 0] if nd == 2 else img


def assert_family_ran(variant, kernels, geom, shape, sig, nd, fp32):
    """The forced variant ran the kernels it names, or, where the shape makes it ineligible on
    purpose, the fallback did: from plan.kernels() and plan.geometry() after an execution on
    shape (uint16 frames) at sigmas sig, in the fp32 mode or in fp64."""
    rd, rs, rt, rw = radii(*sig)
    nx = shape[-1]
    force = VARIANTS[variant]
    # which kernels this shape can run (uint16 frames: 16-byte rows at nx % 8; fields of the pass
    # type: at nx % 4 in float32, nx % 2 in fp64; K12 has no fp64 instance at rd 9; of3d_host.hip)
    k12_ok = nd == 3 and nx % 8 == 0 and rd in ((3, 6, 9) if fp32 else (3, 6))
    k5c_ok = nd == 3 and nx % (4 if fp32 else 2) == 0 and rw in K5C_RW
    assert "general" not in kernels and geom["general"] == 0 and geom["fp32"] == int(fp32)
    if variant == "old":
        assert not set(kernels) & set(NEW_NAMES), kernels
        assert {"k_grad_xy", "k_prod_wy", "k_wx"} <= set(kernels), kernels
        assert nd == 2 or (set(kernels) & {"k_grad_z", "k_grad_z_c"} and
                           set(kernels) & {"k_wz_solve_dma", "k_wz_solve"}), kernels
    else:
        assert any(k.startswith("k_prod_wyx") for k in kernels), kernels
        assert not {"k_prod_wy", "k_wx"} & set(kernels), kernels
        assert nd == 2 or ("k_wz_solve_c" in kernels) == k5c_ok, (kernels, k5c_ok)
    if variant.startswith("k12"):
        assert ("k_grad_xyz_c" in kernels) == k12_ok, (kernels, k12_ok)
        if k12_ok:
            assert not {"k_grad_xy_c", "k_grad_z_c", "k_grad_xy", "k_grad_z"} & set(kernels), kernels
            zc = int(force.get("OF3D_K12_ZC", 0))
            assert geom["k12"]["march"] == zc if zc else geom["k12"]["march"] >= 16, geom
            if zc:
                assert geom["k12"]["grid"][1] == -(-shape[1] // zc), geom
        else:  # rows not 16-byte aligned: K1c + K2c, on purpose
            assert "k_grad_xy_c" in kernels, kernels
    if variant == "k34_uq0":
        assert "k_prod_wyx" in kernels and geom["k34"]["threads"] == geom["k34"]["cw"] <= 256, (kernels, geom)
    if variant == "k34_uq1":  # unique staging: 4- or 8-wave blocks, not the duplicate-staging column stride
        k34 = geom["k34"]
        assert "k_prod_wyx" in kernels and not {"k_prod_wyx_ws", "k_prod_wyx_pk"} & set(kernels), kernels
        assert k34["threads"] == k34["cw"] >= 256 and k34["tx"] != (k34["cw"] - 2 * rw) & ~3, geom
    if variant == "k34_uq2":
        assert "k_prod_wyx_ws" in kernels and geom["k34"]["threads"] == 2 * geom["k34"]["cw"], (kernels, geom)
    if variant == "k34_uq3":
        assert "k_prod_wyx_pk" in kernels, kernels
    if variant == "k5c_nw8":
        assert geom["k5c"]["nw"] == (8 if k5c_ok else 0), geom
    if variant == "wxy_plain":
        assert geom["wxy_zt"] == 0, geom
    if variant == "wxy_tiled":
        assert (geom["wxy_zt"] != 0) == (k5c_ok and nx % 32 == 0), geom
        if geom["wxy_zt"]:
            assert geom["wxy_zt"] == geom["cap_planes"] == shape[1], geom


@pytest.mark.parametrize("i,variant", _family_params())
def test_family_fp32_exact(i, variant, monkeypatch):
    shape, sig, nd = FAMILY_SHAPES[i]
    img = _family_image(i)
    force = VARIANTS[variant]
    out, kernels, geom = _run_plan(img, sig, nd, force, old=force is None, env=VARIANT_ENV.get(variant),
                                   monkeypatch=monkeypatch)
    print(f"{shape} {sig} {variant}: kernels {kernels} geometry {geom}")
    assert_family_ran(variant, kernels, geom, shape, sig, nd, fp32=True)
    (_check3d if nd == 3 else _check2d)(out, _oracle(("family", i), img, sig, nd))


@pytest.mark.parametrize("i", [0, 1, 3, 4, 13, 14, len(FAMILY_SHAPES) - 1])
def test_general_path_fp32_exact(i, monkeypatch):
    """OF3D_GENERAL=1: the general-radius passes (k_corr_gen; of3d_plan_kernels reports the
    path as "general" and nothing else), in float32 against the oracle."""
    shape, sig, nd = FAMILY_SHAPES[i]
    img = _family_image(i)
    out, kernels, geom = _run_plan(img, sig, nd, {}, env={"OF3D_GENERAL": "1"}, monkeypatch=monkeypatch)
    assert kernels == ["general"] and geom["general"] == 1, (kernels, geom)
    (_check3d if nd == 3 else _check2d)(out, _oracle(("family", i), img, sig, nd))


# ---- 5. batched K0 and the pipelined next-frame K0 ---------------------------------------------
@pytest.mark.parametrize("sig", [(2, 2, 5), (2, 3, 7)])  # rt 6, 9
def test_batched_k0_fp32_exact(sig, monkeypatch):
    """of3d_plan_execute_ahead on an fp32 plan: window 0 forms four windows' dt0 in one
    k_tderiv_multi pass, windows 1..3 use them; every window against the float32 oracle."""
    import torch

    monkeypatch.setenv("OF3D_K12", "1")  # batching rides on the fused gradient kernel's workspace
    nwin = 2 * radii(*sig)[2] + 1
    stack, frames = _batch_series(nwin + 3, *sig, 21)
    plan = _lib.Plan(3, NZ, NY, NX, make_taps(*sig), device=0, mode=_lib.OF3D_FP32)
    try:
        for k in range(4):
            got = _batch_call(plan, frames, k, nwin, 3 - k, torch.float32, torch.float32)
            if k == 0:
                assert plan.geometry()["k0_batch"] == 4, plan.geometry()
                assert "k_tderiv_c" not in plan.kernels(), plan.kernels()
            _check3d(got, _oracle(("batch", sig, k), stack[k:k + nwin], sig, 3))
        # one batched pass fed all four windows: no other K0 launch
        assert "k_tderiv_multi" in plan.kernels() and "k_grad_xyz_c" in plan.kernels(), plan.kernels()
        assert not {"k_tderiv_c", "k_tderiv"} & set(plan.kernels()), plan.kernels()
    finally:
        plan.close()


@pytest.mark.parametrize("sig", [(2, 2, 5), (2, 3, 7)])
def test_execute_next_fp32_exact(sig):
    """of3d_plan_execute_next on an fp32 plan: the W-z / solve kernel of window k forms window
    k + 1's dt0 (k_wz_solve_c_next); every window against the float32 oracle."""
    import torch

    rt = radii(*sig)[2]
    stack, wins, rt = _pipe_series((2 * rt + 1 + 2, NZ, NY, NX), *sig, 22)
    plan = _lib.Plan(3, NZ, NY, NX, make_taps(*sig), device=0, mode=_lib.OF3D_FP32)
    try:
        calls = [(k, k + 1 if k + 1 < len(wins) else None, True) for k in range(len(wins))]
        got = _pipe_run(plan, wins, None, (0, NZ), (NZ, NY, NX), torch.float32, calls)
        assert "k_wz_solve_c_next" in plan.kernels(), plan.kernels()
        for k, g in enumerate(got):
            _check3d(g, _oracle(("next", sig, k), stack[k:k + 2 * rt + 1], sig, 3))
    finally:
        plan.close()


# ---- 6. float32 subnormals -----------------------------------------------------------------------
def _tiny_images(shape, seed):
    """float32 frames of amplitude 1e-18: gradients around 1e-19, so a good part of the float32
    products (and of the 2D rel) is subnormal while the windowed sums stay normal."""
    rng = np.random.default_rng(seed)
    grids = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    s = sum(np.sin(0.5 * g + 0.9 * k) for k, g in enumerate(grids))
    return ((1000 + 300 * s + rng.integers(-8, 9, size=shape)) * 1e-21).astype(np.float32)


def _stream_fp32(img, ndim, sig):
    """calc_flow*_fp32's route (the streaming driver, one window) plus the plan's kernel list."""
    from opticalflow3d_dev_amd.stream import FlowStream

    fs = FlowStream(ndim, img.shape[1:], img.dtype, *sig, depth=1, precision="fp32")
    try:
        for frame in img:
            fs.push(frame)
        pend = fs.submit()
        out = tuple(o.copy() for o in pend.result())
        pend.release()
        return out, fs.plan.kernels()
    finally:
        fs.close()


@pytest.mark.parametrize("env,kernel", [({}, None), ({"OF3D_K12": "1"}, "k_grad_xyz_c"),
                                        ({"OF3D_K34_UQ": "0"}, "k_prod_wyx"), ({"OF3D_K34_UQ": "3"}, "k_prod_wyx_pk"),
                                        ({"OF3D_K34": "0", "OF3D_K5C": "0", "OF3D_K1C": "0"}, "k_grad_xy"),
                                        ({"OF3D_GENERAL": "1"}, "general")])
def test_subnormal_products_fp32_exact(env, kernel, monkeypatch):
    """Subnormal float32 products and sums are kept, not flushed to zero, by every kernel family
    (numpy on the host keeps them): a quarter of the products here is subnormal, so a flush in
    any pass moves the 3D rel by percents and the 2D rel's bits.  (vx, vy, vz are signed zeros
    here: the determinant is far below the reference's epsilon.)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sig = (1, 1, 3)
    img = _tiny_images((7, 8, 24, 32), 5)
    tp = cpu_ref.make_taps(*sig)
    cor = lambda a, w, ax: cpu_ref.correlate1d_restated(a, w, ax, np.float32)
    dx = cor(cor(cor(img[3], tp["smooth"], 1), tp["deriv"], 2), tp["smooth"], 0)
    sub = (dx * dx != 0) & (dx * dx < np.finfo(np.float32).tiny)
    assert sub.mean() > 0.2, sub.mean()  # the case is what it says
    out, used = _stream_fp32(img, 3, sig)
    assert kernel is None or kernel in used, used
    want = _oracle(("tiny3",), img, sig, 3)
    assert want[4].max() > 1e-38 and (want[3] > 0).all()  # nothing flushed on the host either
    _check3d(out, want)
    out2, used2 = _stream_fp32(img[:, 2], 2, sig)
    assert kernel in (None, "k_grad_xyz_c") or kernel in used2, used2
    want2 = _oracle(("tiny2",), img[:, 2], sig, 2)
    assert (np.abs(want2[2]) < np.finfo(np.float32).tiny).mean() > 0.05
    _check2d(out2, want2)
