"""The block frames of domain_frames.py, from the oracle alone (no GPU): the properties
test_gpu_value_domain.py relies on, so that a change to the generator cannot hollow it out.

Per shape: whole structure tensors that are exactly zero (as many as the geometry says: the
voxels rd + rw inside each block), velocities of both signs of zero, every output finite, the
restated and the scipy backend equal bit for bit, the float32 oracle's zeros where (and as)
the fp64 oracle's are, saturated frames whose noise sets bit 15 in about half the voxels.  The
counts these tests print are the ones DESIGN.md's table carries."""
import numpy as np
import pytest

from conftest import bits_equal, golden_cases, load_golden
from domain_frames import CASES_2D, CASES_3D, FADE, block_frames, block_slices, noise_mask, zero_signs, zero_tensor
from opticalflow3d_dev_amd import radii
from oracle import cpu_ref

MIN_ZERO_TENSORS = 400
MIN_EACH_SIGN = 100


def _interior(spatial, margin):
    """Voxels at least margin inside a block, both blocks: where every window sees the block only."""
    return sum(int(np.prod([max(s.stop - s.start - 2 * margin, 0) for s in blk])) for blk in block_slices(spatial))


def _frames_ok(img, shape):
    ii = np.iinfo(img.dtype)
    noise = img[:, noise_mask(shape[1:])]
    assert img.max() == ii.max and img.min() == 0
    assert (noise >= 32768).mean() > 0.4, (noise >= 32768).mean()  # bit 15
    sat, zero = block_slices(shape[1:])
    assert (img[(slice(None),) + sat] == ii.max).all() and (img[(slice(None),) + zero] == 0).all()


@pytest.mark.parametrize("name", CASES_3D)
def test_block_frames_3d(name):
    shape, sig, seed = CASES_3D[name]
    rd, rs, rt, rw = radii(*sig)
    assert shape[0] == 2 * rt + 1 and shape[-1] % 32 == 0
    img = block_frames(shape, seed)
    assert img.dtype == np.uint16 and img.shape == shape
    _frames_ok(img, shape)
    st = cpu_ref.structure_tensor3d(img, *sig, backend="scipy")
    rst = cpu_ref.structure_tensor3d(img, *sig, backend="restated")
    for k in st:
        assert bits_equal(st[k], rst[k]), k
    nzt = int(zero_tensor(st).sum())
    assert nzt == _interior(shape[1:], rd + rw) >= MIN_ZERO_TENSORS, nzt
    v = cpu_ref.solve3d(st)
    lmin, lmax = cpu_ref.eig_fp64_3d(st)
    assert all(np.isfinite(a).all() for a in v + (lmin, lmax))
    assert int((lmax == 0).sum()) == nzt and (lmin[lmax == 0] == 0).all()
    st32 = cpu_ref.structure_tensor3d(img, *sig, backend="restated", dtype=np.float32)
    assert int(zero_tensor(st32).sum()) == nzt
    v32 = cpu_ref.calc_flow3D_fp32_oracle(img, *sig)
    assert all(np.isfinite(a).all() for a in v32)
    signs = [zero_signs(a) for a in v]
    print(f"{name} {shape} {sig} radii {(rd, rs, rt, rw)}: {nzt} zero tensors; (-0, +0) per component {signs}")
    for (neg, pos), a32 in zip(signs, v32[:3]):
        assert neg >= MIN_EACH_SIGN and pos >= MIN_EACH_SIGN, signs
        assert zero_signs(a32) == (neg, pos), (zero_signs(a32), neg, pos)


@pytest.mark.parametrize("name", CASES_2D)
def test_block_frames_2d(name):
    shape, sig, seed = CASES_2D[name]
    rd, rs, rt, rw = radii(*sig)
    assert shape[0] == 2 * rt + 1 and shape[-1] % 32 == 0
    img = block_frames(shape, seed)
    _frames_ok(img, shape)
    st = cpu_ref.structure_tensor2d(img, *sig, backend="scipy")
    rst = cpu_ref.structure_tensor2d(img, *sig, backend="restated")
    for k in st:
        assert bits_equal(st[k], rst[k]), k
    nzt = int(zero_tensor(st).sum())
    assert nzt == _interior(shape[1:], rd + rw) >= MIN_ZERO_TENSORS, nzt
    out = cpu_ref.solve2d(st)
    out32 = cpu_ref.calc_flow2D_fp32_oracle(img, *sig)
    assert all(np.isfinite(a).all() for a in out + out32)  # rel: no NaN
    signs = [zero_signs(a) for a in out[:2]]
    print(f"{name} {shape} {sig}: {nzt} zero tensors; (-0, +0) of vx, vy {signs}; rel {zero_signs(out[2])}")
    for (neg, pos), a32 in zip(signs, out32[:2]):
        assert neg >= MIN_EACH_SIGN and pos >= MIN_EACH_SIGN, signs
        assert zero_signs(a32) == (neg, pos)
    assert (out[2][zero_tensor(st)] == 0).all()


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.float32])
def test_block_frames_other_dtypes(dtype):
    """The B1 stack in the other input types: same blocks, same count of zero tensors, the
    integer types over their whole range, the float frames no integers outside the blocks."""
    shape, sig, seed = CASES_3D["B1"]
    rd, rs, rt, rw = radii(*sig)
    img = block_frames(shape, seed, dtype)
    assert img.dtype == np.dtype(dtype)
    sat, zero = block_slices(shape[1:])
    top = 65535 if img.dtype.kind == "f" else np.iinfo(dtype).max
    assert (img[(slice(None),) + sat] == top).all() and (img[(slice(None),) + zero] == 0).all()
    noise = img[:, noise_mask(shape[1:])]
    if img.dtype.kind == "f":
        assert (noise % 1 == 0.25).all() and bits_equal((noise - np.float32(0.25)).astype(np.uint16),
                                                         block_frames(shape, seed)[:, noise_mask(shape[1:])])
    else:
        ii = np.iinfo(dtype)
        assert noise.min() == ii.min and noise.max() == ii.max
    st = cpu_ref.structure_tensor3d(img, *sig, backend="scipy")
    assert int(zero_tensor(st).sum()) == _interior(shape[1:], rd + rw)
    for a in cpu_ref.solve3d(st):  # (the uint16 stack's counts are pinned above; here: both signs occur)
        assert np.isfinite(a).all() and zero_signs(a)[0] >= MIN_EACH_SIGN and zero_signs(a)[1] > 0, zero_signs(a)


def _neg_zeros(a):
    return int(((a == 0) & np.signbit(a)).sum())


@pytest.mark.parametrize("case", ["B1", "B2"])
def test_fading_block_is_what_sees_an_accumulator_started_at_plus_zero(case):
    """With the constant blocks the zero products are of both signs and every windowed sum of
    them is +0: a W pass whose accumulator starts at +0.0 instead of at the first product gives
    the same bits (shown here, so nobody relies on B1 .. B3 for it).  In the fading block the
    products with dt are -0 throughout, whole windows sum to -0, and the same mistake in any of
    the three W passes changes vx, vy and vz at hundreds of voxels: the B1f / B2f / P1f cases of
    test_gpu_value_domain.py."""
    from scipy.ndimage import correlate1d

    shape, sig, seed = CASES_3D[case]
    cor = lambda a, w, ax: correlate1d(a, w, axis=ax, mode="nearest")
    changed = {}
    for fade in (0, FADE):
        img = block_frames(shape, seed, fade=fade)
        tp = cpu_ref.make_taps(*sig)
        G, D, S, T, W = tp["gauss"], tp["deriv"], tp["smooth"], tp["tderiv"], tp["window"]
        I = img[shape[0] // 2].astype(np.float64)
        dt = cor(cor(cor(cpu_ref._tderiv_centre(img, shape[0] // 2, T, np.float64), G, 1), G, 2), G, 0)
        dy = cor(cor(cor(I, D, 1), S, 2), S, 0)
        dx = cor(cor(cor(I, S, 1), D, 2), S, 0)
        dz = cor(cor(cor(I, S, 1), S, 2), D, 0)
        prods = {"tx": dx * dt, "ty": dy * dt, "tz": dz * dt, "xy": dx * dy, "xz": dx * dz, "x2": dx * dx,
                 "yz": dy * dz, "y2": dy * dy, "z2": dz * dz}
        assert _neg_zeros(prods["tx"]) > 1000  # negative zeros enter the W passes either way

        def flow(lossy_pass):
            """solve3d of the windowed products; lossy_pass (0, 1, 2 or None): that W pass's result
            + 0.0, which is all an accumulator started at +0.0 changes (-0 becomes +0)."""
            st = {}
            for k, p in prods.items():
                for n, ax in enumerate((1, 2, 0)):
                    p = cor(p, W, ax)
                    if n == lossy_pass:
                        p = p + 0.0
                st[k] = p
            return st, cpu_ref.solve3d(st)

        st, ref = flow(None)
        want = cpu_ref.structure_tensor3d(img, *sig, backend="scipy")
        assert all(bits_equal(st[k], want[k]) for k in st)  # this restatement is the oracle's
        nneg = {k: _neg_zeros(a) for k, a in st.items()}
        changed[fade] = [int((a.view(np.uint64) != b.view(np.uint64)).sum())
                         for n in range(3) for a, b in zip(flow(n)[1], ref)]
        print(f"{case} fade {fade}: -0 among the windowed sums {nneg}; voxels of vx, vy, vz a +0.0 start of W y / "
              f"W x / W z changes: {changed[fade]}; (-0, +0) per component {[zero_signs(a) for a in ref]}")
        if fade:
            assert min(nneg["tx"], nneg["ty"], nneg["tz"]) >= MIN_ZERO_TENSORS, nneg
            assert all(np.isfinite(a).all() and min(zero_signs(a)) >= MIN_ZERO_TENSORS for a in ref)
            v32 = cpu_ref.calc_flow3D_fp32_oracle(img, *sig)
            assert [zero_signs(a) for a in v32[:3]] == [zero_signs(a) for a in ref]
        else:
            assert not any(nneg.values()), nneg
    assert not any(changed[0]) and min(changed[FADE]) >= MIN_ZERO_TENSORS, changed


def test_fading_block_2d():
    shape, sig, seed = CASES_2D["P1"]
    st = cpu_ref.structure_tensor2d(block_frames(shape, seed, fade=FADE), *sig, backend="scipy")
    assert min(_neg_zeros(st["tx"]), _neg_zeros(st["ty"])) >= MIN_ZERO_TENSORS
    out = cpu_ref.solve2d(st)
    assert all(np.isfinite(a).all() for a in out) and all(min(zero_signs(a)) >= MIN_EACH_SIGN for a in out[:2])


def test_flat_block_fixtures():
    """The two reference fixtures of this input class hold what they are for: bit 15, saturated
    voxels, exactly zero tensors, and velocities of both signs of zero in the reference's outputs."""
    assert "c3d_flat_blocks" in golden_cases("c3d") and "c2d_flat_blocks" in golden_cases("c2d")
    for name, fn in (("c3d_flat_blocks", cpu_ref.structure_tensor3d), ("c2d_flat_blocks", cpu_ref.structure_tensor2d)):
        g = load_golden(name)
        img = g["images"]
        assert img.dtype == np.uint16 and img.max() == 65535 and (img >= 32768).mean() > 0.3
        st = fn(img, g["sig"], g["tsig"], g["wsig"], backend="scipy")
        assert zero_tensor(st).sum() >= 4, name
        neg, pos = zero_signs(g["vx"])
        assert neg > 0 and pos > 0, (name, neg, pos)
        assert np.isfinite(g["vx"]).all() and np.isfinite(g["rel"]).all()
