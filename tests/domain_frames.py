"""Test frames with saturated and zero-filled blocks in full-range noise (tests only).

The suite's seeded frames are noise below 4096: no gradient, product or windowed sum on them
is ever exactly zero, and bit 15 of a uint16 voxel is never set.  block_frames builds the other
kind of input this workload meets: noise over the whole range of the input type (bit 15 set in
half the voxels) around two blocks that are constant in time, one at the type's maximum (a
saturated camera) and one at zero (the wedge a deskewed stack is padded with).  Each block is
wider than 2 (rd + rw) + 1 in every direction at the shapes in CASES_3D / CASES_2D, so inside
it every pass sums terms like (v[-k] - v[+k]) * h[k] = +-0, whole structure tensors are exactly
zero, and the sign of each zero velocity is set by the order of the additions and by the value
each accumulator starts from: what the oracle defines and a kernel has to reproduce."""
import numpy as np

# id -> (frames' shape, (xyzSig, tSig, wSig), seed); the radii (rd, rs, rt, rw) are
# B1 (3, 1, 3, 9), B2 (6, 2, 6, 15), B3 (6, 2, 9, 21: the headline's parameters)
CASES_3D = {
    "B1": ((7, 40, 48, 96), (1, 1, 3), 7000),
    "B2": ((13, 52, 56, 128), (2, 2, 5), 7000),
    "B3": ((19, 64, 64, 160), (2, 3, 7), 7000),
}
CASES_2D = {
    "P1": ((7, 96, 128), (1, 1, 3), 7100),
    "P2": ((13, 120, 160), (2, 2, 5), 7100),
}


FADE = 256  # counts per frame the bright block of the "f" cases loses (B1f, B2f, P1f: block_frames(fade=FADE))


def case_frames(case, dtype=np.uint16):
    """(frames, sigmas) of a case id of CASES_3D / CASES_2D; with an "f" appended: its fading form."""
    shape, sig, seed = (CASES_3D | CASES_2D)[case.rstrip("f")]
    return block_frames(shape, seed, dtype, fade=FADE if case.endswith("f") else 0), sig


def block_slices(spatial, zm=2, ym=4, xm=4):
    """(saturated block, zero block) as index tuples over the spatial axes ([nz,] ny, nx): the
    left and right halves of x, each zm / ym / xm voxels inside the volume and the half."""
    *zy, nx = spatial
    half = nx // 2
    lead = [slice(m, n - m) for n, m in zip(zy, (zm, ym) if len(zy) == 2 else (ym,))]
    return tuple(lead) + (slice(xm, half - xm),), tuple(lead) + (slice(half + xm, nx - xm),)


def noise_mask(spatial, **margins):
    """True where a voxel is noise (outside both blocks)."""
    m = np.ones(spatial, bool)
    for s in block_slices(spatial, **margins):
        m[s] = False
    return m


def block_frames(shape, seed, dtype=np.uint16, fade=0, **margins):
    """A stack (nt, [nz,] ny, nx) of seeded uniform noise over the whole range of an integer
    dtype with the two constant blocks of block_slices.  dtype float32: the uint16 stack with 0.25
    added to the noise voxels (so the frames are no integers) and the blocks left exact.

    fade > 0: the bright block is flat in space but loses `fade` counts per frame (a bleaching flat
    region: max - fade * t).  Its spatial gradients stay +0 while its temporal derivative is
    negative, so the products tx, ty, tz are -0 throughout and whole windows sum to -0: the one
    place where a windowed sum is a negative zero, which an accumulator started at +0.0 loses
    (with constant blocks the products are of both signs of zero and every windowed sum is +0)."""
    dt = np.dtype(dtype)
    it = np.dtype(np.uint16) if dt.kind == "f" else dt
    ii = np.iinfo(it)
    img = np.random.default_rng(seed).integers(ii.min, ii.max, size=shape, dtype=it, endpoint=True)
    sat, zero = block_slices(shape[1:], **margins)
    for t in range(shape[0]):
        img[(t,) + sat] = ii.max - fade * t
    img[(slice(None),) + zero] = 0
    if dt.kind == "f":
        img = img.astype(dt)
        img[:, noise_mask(shape[1:], **margins)] += dt.type(0.25)
    return img


def zero_tensor(st):
    """Voxels whose windowed products (the dict of structure_tensor3d / 2d) are all exactly 0."""
    return np.logical_and.reduce([v == 0 for v in st.values()])


def zero_signs(v):
    """(number of -0.0, number of +0.0) in v."""
    z = v == 0
    neg = np.signbit(v)
    return int((z & neg).sum()), int((z & ~neg).sum())
