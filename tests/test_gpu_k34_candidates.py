"""Every K34 autotune candidate at every compiled window radius (wSig 3..7: rw 9, 12, 15, 18, 21),
fp64 and fp32, against the separate-pass kernels (OF3D_K34=0: k_prod_wy + k_wx) on the same plan:
every output bit-identical.  The forced-family tests reach each family at rw 12, 15, 21 and the
candidate sweeps of test_gpu_bench_geometry.py run rw 15 and 21 only, so the deeper-prefetch and
9-producer-wave instances at rw 9, 12 and every rw 18 instance otherwise run only where the
autotune happens to time them fastest.

Volume 7 x 6 x 42 x 544 (uint16, xyzSig 1, tSig 1): 42 rows leave a partial last tile at every
tile height (4, 8, 16); nx = 544 is a multiple of 32 (K5c and the z-tiled hand-off run), is more
than the 512 staged columns of an 8-wave block (two column blocks with a seam and both edge pads
for the unique-staging and wave-specialised families), fits one 576-column block (the
9-producer-wave candidate exists in fp64) and gives the 1-wave duplicate-staging blocks of 20 to
44 outputs many seams.  One 2D case (five products): wSig 5 on a 300 x 544 plane.

The default plan of each parameter set is also held to the oracle (fp64: vx, vy, vz bitwise; fp32:
the float32 oracle as test_gpu_fp32_exact.py), which pins the reference kernels themselves."""
import numpy as np
import pytest

from conftest import bits_equal, oracle3d
from opticalflow3d_dev_amd import _lib, make_taps, radii
from oracle import cpu_ref
from test_gpu_bench_geometry import env
from test_gpu_fp32_exact import _check2d, _check3d
from test_gpu_kernel_families import _run

pytestmark = pytest.mark.gpu

SHAPE_3D = (7, 6, 42, 544)
SHAPE_2D = (7, 300, 544)
# (ndim, wSig)
PARAMS = [(3, w) for w in (3, 4, 5, 6, 7)] + [(2, 5)]


def _candidates(ndim, vol, taps, mode):
    """Number of K34 candidates of the plan shape, counted as test_gpu_bench_geometry.k34_candidates
    does (a pin past the end fails under OF3D_K34_CAND_STRICT=1)."""
    n = 0
    while n < 64:
        with env(OF3D_K34_CAND=n, OF3D_K34_CAND_STRICT=1):
            try:
                _lib.Plan(ndim, *vol, taps, device=0, mode=mode).close()
            except RuntimeError as e:
                assert "OF3D_K34_CAND out of range" in str(e)
                return n
        n += 1
    return n


@pytest.mark.parametrize("fp32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("ndim,w", PARAMS, ids=[f"{nd}d-w{w}" for nd, w in PARAMS])
def test_every_k34_candidate_bit_identical(ndim, w, fp32):
    sig = (1, 1, w)
    rw = radii(*sig)[3]
    assert rw == 3 * w
    shape = SHAPE_3D if ndim == 3 else SHAPE_2D
    img = np.random.default_rng(3400 + 10 * w + ndim).integers(0, 4096, size=shape).astype(np.uint16)
    vol = shape[1:] if ndim == 3 else (1,) + shape[1:]
    mode = _lib.OF3D_FP32 if fp32 else 0

    ks_ref = []
    ref = _run(img, *sig, ndim, mode, old=False, force={"OF3D_K34": "0"}, kernels=ks_ref)
    assert {"k_prod_wy", "k_wx"} <= set(ks_ref) and not any(k.startswith("k_prod_wyx") for k in ks_ref), ks_ref

    # the default plan against the oracle: the reference kernels are pinned through it
    ks_def = []
    out = _run(img, *sig, ndim, mode, old=False, kernels=ks_def)
    assert any(k.startswith("k_prod_wyx") for k in ks_def), ks_def
    for a, b in zip(out, ref):
        assert bits_equal(a, b), ("default", ks_def)
    if fp32:
        if ndim == 3:
            _check3d(out, cpu_ref.calc_flow3D_fp32_oracle(img, *sig))
        else:
            _check2d(out, cpu_ref.calc_flow2D_fp32_oracle(img, *sig))
    else:
        want = oracle3d(img, *sig)[:3] if ndim == 3 else cpu_ref.calc_flow2D(img, *sig, backend="scipy")[:2]
        for name, a, b in zip(("vx", "vy", "vz"), out, want):
            assert bits_equal(a.reshape(b.shape), b), name

    ncand = _candidates(ndim, vol, make_taps(*sig), mode)
    shapes, names = set(), set()
    for i in range(ncand):
        ks, geo = [], {}
        with env(OF3D_K34_CAND=i):
            out = _run(img, *sig, ndim, mode, old=False, kernels=ks, geometry=geo)
        k34 = geo["k34"]
        print(f"rw {rw} {'fp32' if fp32 else 'fp64'} cand {i}/{ncand}: {[k for k in ks if 'prod' in k]} {k34}")
        assert k34["candidates"] == ncand, geo
        shapes.add((k34["threads"], k34["cw"]))
        names.update(ks)
        for name, a, b in zip(("vx", "vy", "vz", "rel") if ndim == 3 else ("vx", "vy", "rel"), out, ref):
            assert bits_equal(a, b), (i, name, ks, k34)
    # the sweep was not empty: the families it is meant to reach were among the candidates
    assert any(t == cw <= 256 for t, cw in shapes), shapes  # duplicate staging
    assert any(t == 2 * cw for t, cw in shapes), shapes  # wave-specialised
    if fp32:
        assert "k_prod_wyx_pk" in names, names
    else:
        assert any(cw == 576 for _, cw in shapes), shapes  # 9 producer waves
