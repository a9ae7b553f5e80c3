"""The float32 restatement of the oracle (oracle/cpu_ref.py, dtype=np.float32): the checker
the GPU tests hold the library's fp32 mode to, bit for bit (tests/test_gpu_fp32_exact.py).
Pinned here, on the CPU: its float64 instance is the golden-pinned oracle itself, its
float32 instance stays within a measured distance of the fp64 goldens, agrees with a
scalar loop written without NumPy array arithmetic, and casts its inputs first."""
import numpy as np
import pytest

from conftest import bits_equal, golden_cases, load_golden
from oracle import cpu_ref


# ---- the float64 instance of the generic code: still the reference's bits -----------------
@pytest.mark.parametrize("name", golden_cases("c3d"))
def test_generic_float64_3d_bitwise(name):
    g = load_golden(name)
    st = cpu_ref.structure_tensor3d(g["images"], g["sig"], g["tsig"], g["wsig"], "restated", dtype=np.float64)
    for a, k in zip(cpu_ref.solve3d(st), ("vx", "vy", "vz")):
        assert bits_equal(a, g[k]), k


@pytest.mark.parametrize("name", golden_cases("c2d"))
def test_generic_float64_2d_bitwise(name):
    g = load_golden(name)
    st = cpu_ref.structure_tensor2d(g["images"], g["sig"], g["tsig"], g["wsig"], "restated", dtype=np.float64)
    for a, k in zip(cpu_ref.solve2d(st), ("vx", "vy", "rel")):
        assert bits_equal(a, g[k]), k


# ---- float32 accuracy against the fp64 goldens ----------------------------------------------
# max|dv| / max|v| of the float32 oracle against the golden fp64 vx / vy / vz, measured over
# every c3d* and c2d* golden (the largest of the components):
#   c3d_big_wsig17 9.9e-7      c3d_big_xyzsig9 9.9e-7     c3d_default_params 1.3e-6
#   c3d_float32_nt11 5.6e-7    c3d_frac_sigmas 2.9e-7     c3d_iso_smoothed_noise 2.8e-7
#   c3d_nonsquare_odd 3.3e-7   c3d_nz2 4.1e-7   c3d_nz3 3.3e-7   c3d_nz4 4.7e-7
#   c3d_pub_s3t1w4_nz4 4.7e-7  c3d_rand_c2params 8.2e-7   c3d_rand_c3params 5.7e-7
#   c3d_rand_s1 2.8e-7         c3d_smooth_translate 1.32e-5   c3d_wsig3 2.9e-7   c3d_wsig6 4.3e-7
#   c2d_big_sigmas 4.1e-7      c2d_c1params 1.9e-7        c2d_c2params 2.8e-7
#   c2d_float32 3.7e-7         c2d_nonsquare 2.3e-7       c2d_smooth_translate 3.7e-7
#   c2d_tiny_s3 4.6e-7
#   c3d_flat, c3d_nz1, c3d_ramp_xy_planar, c3d_wave_planar, c2d_flat: v == 0 everywhere, error 0
#   c3d_ramp_xyz_rank1: 0.637
# The largest is c3d_smooth_translate's 1.32e-5 (a smooth stack: small determinants), so the
# bound is 4 x 1.32e-5 = 5.3e-5.  It guards the oracle against a gross mistake (a dropped tap, a
# pass in the wrong precision that matters); it is not what the device is held to.
FP32_ORACLE_BOUND = 4 * 1.32e-5
# c3d_ramp_xyz_rank1 is singular by construction (a linear ramp: the tensor has rank 1, its
# determinant is rounding noise, and the golden fp64 v is that noise divided by det + eps), so
# float32 passes give other noise: measured 0.637 of max|v|.  Held to 4 x that; all it says is
# that the result stays finite and of the golden's magnitude.
FP32_ORACLE_BOUND_SINGULAR = {"c3d_ramp_xyz_rank1": 4 * 0.637}
# c3d_flat_blocks / c2d_flat_blocks hold a block saturated at 65535.  Inside it the smoothing
# passes return values near 65535, where a float32 ulp is 2^-8, and the derivative pass that
# follows takes differences of them: what is left of the gradient deep in the block (the far
# tails of the noise outside) is of that size, so the float32 tensor there is a few 1e-4 off
# in relative terms and v with it.  The largest errors sit at such voxels (|v| of the order of
# max|v|, e.g. (11, 13, 11) and (7, 12)): measured 5.9e-4 (3D, vz) and 1.2e-4 (2D, vx) of
# max|v|.  Held to 4 x that, as above; outside the blocks the float32 oracle is as close as on
# noise.  Its zeros, and their signs, are the fp64 oracle's exactly (test_value_domain_cpu.py).
FP32_ORACLE_BOUND_SINGULAR.update({"c3d_flat_blocks": 4 * 5.9e-4, "c2d_flat_blocks": 4 * 1.2e-4})


@pytest.mark.parametrize("name", golden_cases("c3d") + golden_cases("c2d"))
def test_float32_oracle_close_to_fp64_golden(name):
    g = load_golden(name)
    if name.startswith("c3d"):
        out = cpu_ref.calc_flow3D_fp32_oracle(g["images"], g["sig"], g["tsig"], g["wsig"])[:3]
        keys = ("vx", "vy", "vz")
    else:
        out = cpu_ref.calc_flow2D_fp32_oracle(g["images"], g["sig"], g["tsig"], g["wsig"])
        keys = ("vx", "vy")
        assert out[2].dtype == np.float32 and out[2].shape == g["rel"].shape
    bound = FP32_ORACLE_BOUND_SINGULAR.get(name, FP32_ORACLE_BOUND)
    for a, k in zip(out, keys):
        assert a.dtype == np.float32 and a.shape == g[k].shape
        vmax = np.abs(g[k]).max()
        err = np.abs(a.astype(np.float64) - g[k]).max()
        print(f"{name} {k}: max|dv| {err:.3e}  max|v| {vmax:.3e}  ratio {err / vmax if vmax else 0:.3e}")
        assert err <= bound * vmax, (k, err, vmax)


# ---- the float32 passes against a scalar loop -------------------------------------------------
def _correlate_scalar_f32(a, w, anti):
    """One line, mode='nearest', scipy's symmetric order, every operation on np.float32 scalars."""
    r = len(w) // 2
    n = len(a)
    a = [np.float32(v) for v in a]
    w = [np.float32(v) for v in w]  # round to nearest
    out = []
    for i in range(n):
        o = a[i] * w[r]
        for j in range(-r, 0):
            lo, hi = a[min(max(i + j, 0), n - 1)], a[min(max(i - j, 0), n - 1)]
            o = o + ((lo - hi) if anti else (lo + hi)) * w[r + j]
        assert type(o) is np.float32
        out.append(o)
    return np.array(out, np.float32)


@pytest.mark.parametrize("r", [1, 3, 6, 21])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_restated_float32_matches_scalar_loop(r, axis):
    rng = np.random.default_rng(40 + 3 * r + axis)
    a = (rng.normal(size=(4, 5, 6)) * 1000).astype(np.float32)
    x = np.arange(-r, r + 1)
    sym = np.exp(-x * x / 2 / (r / 3) ** 2) / 7
    for w, anti in ((sym, False), (sym * x, True)):
        got = cpu_ref.correlate1d_restated(a, w, axis, dtype=np.float32)
        assert got.dtype == np.float32
        want = np.apply_along_axis(_correlate_scalar_f32, axis, a, w, anti)
        assert bits_equal(got, want)
        # taps rounded to nearest, not truncated, and not left in float64
        assert not bits_equal(got, cpu_ref.correlate1d_restated(a, w, axis).astype(np.float32))


def test_scipy_backend_refuses_float32():
    img = np.zeros((7, 3, 8, 8), np.uint16)
    with pytest.raises(ValueError):
        cpu_ref.structure_tensor3d(img, 1, 1, 2, backend="scipy", dtype=np.float32)
    with pytest.raises(ValueError):
        cpu_ref.structure_tensor2d(img[:, 0], 1, 1, 2, backend="scipy", dtype=np.float32)
    with pytest.raises(ValueError):
        cpu_ref.structure_tensor3d(img, 1, 1, 2, dtype=np.float16)


# ---- inputs a float32 cannot hold ------------------------------------------------------------
@pytest.mark.parametrize("dtype", cpu_ref.CAST_DTYPES)
def test_float32_oracle_casts_inputs_first(dtype):
    img = cpu_ref.cast_case_images((7, 5, 12, 16), dtype, 77)
    rounded = img.astype(np.float32)
    lost = rounded.astype(np.float64) != img.astype(np.float64)
    assert lost.mean() > 0.3, lost.mean()  # the cast really rounds
    if np.dtype(dtype).kind != "f":
        assert np.abs(img.astype(np.int64)).min() > (1 << 24)
    got = cpu_ref.calc_flow3D_fp32_oracle(img, 1, 1, 2)
    want = cpu_ref.calc_flow3D_fp32_oracle(rounded, 1, 1, 2)
    for a, b in zip(got, want):
        assert bits_equal(a, b)
    got2 = cpu_ref.calc_flow2D_fp32_oracle(img[:, 2], 1, 1, 2)
    for a, b in zip(got2, cpu_ref.calc_flow2D_fp32_oracle(rounded[:, 2], 1, 1, 2)):
        assert bits_equal(a, b)
    # and it is not the fp64 oracle rounded at the end
    st = cpu_ref.structure_tensor3d(img, 1, 1, 2)
    assert not bits_equal(got[0], cpu_ref.solve3d(st)[0].astype(np.float32))
