"""The flow pipeline on hostile memory: no kernel may rely on stale or unwritten memory.

Every case here runs with the plan's workspace filled with 0xFF bytes (of3d_plan_poison: a NaN
in every fp64 and fp32 element, every pre-formed dt0 dropped), its outputs between guard runs
of a sentinel NaN (poison.guarded: nothing outside written, nothing inside left), and its
input frames between guard planes of a loud value (poison.guarded_frames: a read outside the
planes of of3d_plan_input_range changes the result).  The comparisons are the project's own:

  * vx, vy, vz and every 2D output bit-identical to oracle.cpu_ref (scipy backend in fp64, the
    float32 restatement in OF3D_FP32);
  * 3D rel within REL_TOL_REF (float32 rel) / REL_TOL_FP64 (OF3D_REL_F64) times lambda_max of
    cpu_ref.eig_fp64_3d, as test_gpu_parity has it, and finite.

Volumes: the smallest that give every tiled dimension two blocks and a partial last one,
asserted from plan.geometry() in every case: the K5c z blocks, the K12 column tiles and z
marches, and the K34 column blocks.  The K34 autotune is free to pick a one-block geometry, so
every plan pins (OF3D_K34_CAND) the first candidate of the variant's form with two column
blocks or more and a partial last one; the unique-staging, wave-specialised and packed forms
stage up to 512 columns, so their variants run on 604-column volumes (WA, WB).  The series
and host-entry cases run A-sized frames at B's sigmas (volume S): only (rw, rt) = (15, 6) and
(21, 9) have the K5c instance that forms the next window's dt0.  Each case asserts from
plan.kernels() / plan.geometry() that the kernel it is about ran, and prints both (pytest -s:
the POISON lines are the coverage table).  of3d_plan_kernels names not reached here: k_wz_solve_c2 (the packed-fp32 K5c was
removed; the name only keeps the bit positions)."""
import numpy as np
import pytest

import poison
from conftest import assert_rel_within, bits_equal, oracle3d
from opticalflow3d_dev_amd import _lib, calc_flow2D, calc_flow3D, make_taps
from oracle import cpu_ref
from test_gpu_fp32_exact import K5C_RW, NEW_NAMES, VARIANT_ENV
from test_gpu_kernel_families import FAMILY_ENV
from test_gpu_parity import REL_TOL_FP64, REL_TOL_REF

pytestmark = pytest.mark.gpu

# name -> sigmas, frames of a window, (nz, ny, nx), windows of the series (full-volume cases: window 0)
VOLS = {
    # nx 192 (not 160 / 96): two K12 column tiles in fp64 (186 / 180 outputs per tile) with a partial
    # last one, still whole 32-column K5c tiles; B's nz 52: a partial last 16-plane K12 march
    "A": dict(sig=(1, 1, 3), nt=7, shape=(72, 37, 192), nwins=1, seed=9101),
    "A150": dict(sig=(1, 1, 3), nt=7, shape=(72, 37, 150), nwins=1, seed=9102),  # rows of no 16-byte multiple
    "B": dict(sig=(2, 2, 5), nt=13, shape=(52, 33, 192), nwins=1, seed=9103),
    # A-sized frames at B's sigmas: (rw, rt) = (15, 6) has the K5c instance that forms the next dt0
    "S": dict(sig=(2, 2, 5), nt=13, shape=(72, 37, 192), nwins=4, seed=9104),
    # the K34 forms that stage up to 512 columns per block: 604 columns are two blocks of 304 and 300
    "WA": dict(sig=(1, 1, 3), nt=7, shape=(40, 21, 604), nwins=1, seed=9105),
    "WB": dict(sig=(2, 2, 5), nt=13, shape=(40, 17, 604), nwins=1, seed=9106),
    # the deep K12 instance marches 128 planes: 136 planes are two marches, the last one of 8
    "D": dict(sig=(2, 2, 5), nt=13, shape=(136, 33, 192), nwins=1, seed=9107),
}
RADII = {"A": (3, 1, 3, 9), "A150": (3, 1, 3, 9), "B": (6, 2, 6, 15), "S": (6, 2, 6, 15), "WA": (3, 1, 3, 9),
         "WB": (6, 2, 6, 15), "D": (6, 2, 6, 15)}
MODES = {"fp64": 0, "fp32": _lib.OF3D_FP32, "rel64": _lib.OF3D_REL_F64}

OLD = {k: "0" for k in FAMILY_ENV}
VARIANTS = {
    "default": {},
    "old": OLD,
    "oldest": OLD | {"OF3D_K2C": "0", "OF3D_K0C": "0"},  # the runtime-radius K2 and K0 too
    "k12": {"OF3D_K12": "1"},
    "k12_zc16": {"OF3D_K12": "1", "OF3D_K12_ZC": "16"},
    "k12_deep": {"OF3D_K12": "1", "OF3D_K12_ZC": "128"},  # the three-DMA-slot instance: fp64, rd 6
    "k5c_nw8": {"OF3D_K5C_NW": "8"},
    "wxy_plain": {"OF3D_WXY_TILE": "0"},
    "wxy_tiled": {"OF3D_WXY_TILE": "1"},
    "k34_off": {"OF3D_K34": "0"},
    "k34_uq0": {"OF3D_K34_UQ": "0"},
    "k34_uq1": {"OF3D_K34_UQ": "1"} | VARIANT_ENV["k34_uq1"],
    "k34_uq2": {"OF3D_K34_UQ": "2"} | VARIANT_ENV["k34_uq2"],
    "k34_uq3": {"OF3D_K34_UQ": "3"},  # the packed-fp32 K34: fp32 plans only
    "general": {"OF3D_GENERAL": "1"},
}
SWITCHES = sorted({k for env in VARIANTS.values() for k in env} | {"OF3D_K34_CAND", "OF3D_K34_TUNE", "OF3D_K5C_R",
                                                                    "OF3D_PIPE", "OF3D_ZCHUNK", "OF3D_K2C", "OF3D_K0C",
                                                                    "OF3D_K34_CAND_STRICT"})
NO_K34 = ("old", "oldest", "k34_off", "general")  # variants that do not run the fused K34

_STACK, _ORACLE = {}, {}


def _stack(vol):
    """The volume's uint16 series, random in [0, 4096): nt + nwins - 1 frames."""
    if vol not in _STACK:
        v = VOLS[vol]
        shape = (v["nt"] + v["nwins"] - 1,) + v["shape"]
        _STACK[vol] = np.random.default_rng(v["seed"]).integers(0, 4096, size=shape).astype(np.uint16)
    return _STACK[vol]


def _oracle(vol, fp32, k=0):
    """(vx, vy, vz, lambda_min, lambda_max) of window k of the volume's series: computed once
    per (volume, precision, window), never written to, sliced for sub-ranges."""
    key = (vol, bool(fp32), k)
    if key not in _ORACLE:
        v = VOLS[vol]
        img = _stack(vol)[k:k + v["nt"]]
        out = cpu_ref.calc_flow3D_fp32_oracle(img, *v["sig"]) if fp32 else oracle3d(img, *v["sig"])
        for a in out:
            a.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


def _set_env(monkeypatch, variant):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in VARIANTS[variant].items():
        monkeypatch.setenv(k, v)


_PIN = {}  # (variant, plan arguments) -> the pinned K34 candidate


def _pinned_plan(monkeypatch, variant, ndim, shape, sig, mode, max_out_planes=0):
    """A plan under the variant's switches whose fused K34 is pinned (OF3D_K34_CAND, strict: a
    pin past the candidates is an error) to the first candidate of the variant's form with >= 2
    column blocks and a partial last one.  No candidate like that fails the case: enlarge nx."""
    _set_env(monkeypatch, variant)
    make = lambda: _lib.Plan(ndim, *shape, make_taps(*sig), device=0, mode=mode, max_out_planes=max_out_planes)
    if variant in NO_K34:
        return make()
    key = (variant, ndim, shape, sig, mode, max_out_planes)
    monkeypatch.setenv("OF3D_K34_CAND_STRICT", "1")
    seen = []
    for i in ([_PIN[key]] if key in _PIN else range(64)):
        monkeypatch.setenv("OF3D_K34_CAND", str(i))
        try:
            plan = make()
        except RuntimeError as e:  # past the last candidate
            raise AssertionError(f"{variant} {shape}: no K34 candidate with two column blocks and a partial last "
                                 f"one among {seen} ({e})") from None
        k = plan.geometry()["k34"]
        if k["nbx"] >= 2 and shape[-1] % k["tx"]:
            _PIN[key] = i
            return plan
        seen.append((k["cw"], k["tx"], k["nbx"]))
        plan.close()
    raise AssertionError(f"{variant} {shape}: more than 64 K34 candidates")


def _check3d(got, want, mode, z=slice(None), y=slice(None), what=""):
    fp32 = bool(mode & _lib.OF3D_FP32)
    ft = np.float32 if fp32 else np.float64
    for name, a, b in zip(("vx", "vy", "vz"), got[:3], want[:3]):
        b = np.ascontiguousarray(b[z, y])
        assert a.dtype == ft and b.dtype == ft and a.shape == b.shape, (what, name, a.dtype, a.shape, b.shape)
        if not bits_equal(a, b):
            it = np.uint32 if fp32 else np.uint64
            bad = np.argwhere(a.view(it) != b.view(it))
            raise AssertionError(f"{what}: {name}: {len(bad)} of {a.size} values differ from the oracle "
                                 f"({int(np.isnan(a).sum())} NaN); index box {bad.min(axis=0).tolist()} .. "
                                 f"{bad.max(axis=0).tolist()} of shape {a.shape}")
    rel = got[3]
    assert rel.dtype == (np.float64 if mode & _lib.OF3D_REL_F64 else np.float32), rel.dtype
    assert np.isfinite(rel).all(), f"{what}: rel: {int((~np.isfinite(rel)).sum())} values not finite"
    tol = REL_TOL_FP64 if mode & _lib.OF3D_REL_F64 else REL_TOL_REF
    assert_rel_within(rel, want[3][z, y], want[4][z, y], tol)


def _expect(variant, vol, fp32, kernels, geom, aligned=True, z=None):
    """The kernels the variant is about ran (or, where the shape rules them out on purpose, the
    stated fallback did): of3d_host.hip's eligibility rules for uint16 frames."""
    rd, rs, rt, rw = RADII[vol]
    nz, ny, nx = VOLS[vol]["shape"]
    es = 4 if fp32 else 8
    ks = set(kernels)
    k12_ok = aligned and nx % 8 == 0 and (rd in (3, 6) or (rd == 9 and fp32))
    k5c_ok = nx % (16 // es) == 0 and rw in K5C_RW
    assert geom["fp32"] == int(fp32) and (geom["nz"], geom["ny"], geom["nx"]) == (nz, ny, nx), geom
    if variant == "general":
        assert kernels == ["general"] and geom["general"] == 1, (kernels, geom)
        return
    assert "general" not in ks and geom["general"] == 0, (kernels, geom)
    if variant in ("old", "oldest"):
        assert not ks & set(NEW_NAMES), kernels
        assert {"k_grad_xy", "k_prod_wy", "k_wx"} <= ks, kernels
        assert ("k_grad_z" if variant == "oldest" else "k_grad_z_c") in ks, kernels
        # the LDS-DMA K5 stages 16-byte rows of the pass type; else the register-staged one
        if nx % (16 // es):
            assert "k_wz_solve" in ks and "k_wz_solve_dma" not in ks, kernels
        else:
            assert ks & {"k_wz_solve_dma", "k_wz_solve"}, kernels
        if variant == "oldest":
            assert "k_tderiv" in ks and "k_tderiv_c" not in ks, kernels
    elif variant == "k34_off":
        assert {"k_prod_wy", "k_wx"} <= ks and not any(k.startswith("k_prod_wyx") for k in ks), kernels
    else:
        assert any(k.startswith("k_prod_wyx") for k in ks) and not {"k_prod_wy", "k_wx"} & ks, kernels
    if variant not in ("old", "oldest"):
        assert ("k_wz_solve_c" in ks) == k5c_ok, (kernels, k5c_ok)
        if not k5c_ok:
            assert ks & {"k_wz_solve_dma", "k_wz_solve"}, kernels
    if variant.startswith("k12"):
        assert ("k_grad_xyz_c" in ks) == k12_ok, (kernels, k12_ok)
        if k12_ok:
            assert not {"k_grad_xy_c", "k_grad_z_c", "k_grad_xy", "k_grad_z"} & ks, kernels
            zc = int(VARIANTS[variant].get("OF3D_K12_ZC", 0))
            assert geom["k12"]["march"] == zc if zc else geom["k12"]["march"] >= 16, geom
            assert geom["k12"]["deep"] == int(variant == "k12_deep"), geom
            if z is None:  # a whole volume in one schedule: >= 2 z marches, a partial last one
                assert geom["k12"]["grid"][1] >= 2 and nz % geom["k12"]["march"], (nz, geom)
        else:  # rows or frames not 16-byte aligned: K1c + K2c, on purpose, and the plan says so
            assert {"k_grad_xy_c", "k_grad_z_c"} <= ks, kernels
    elif variant not in ("old", "oldest") and "k_grad_xyz_c" not in ks:
        assert {"k_grad_xy_c", "k_grad_z_c"} <= ks, kernels
    if "k_grad_xyz_c" in ks:
        # K12 tiles: 4 rows by 192 (fp64) / 128 (fp32) staged columns less the 2 rd halo (of3d_k12.hpp);
        # >= 2 column tiles and row tiles with partial last ones, and the grid is that many tiles in 8s
        tx12 = (128 if fp32 else 192) - 2 * rd
        nb12, nr12 = -(-nx // tx12), -(-ny // 4)
        assert nb12 >= 2 and nx % tx12 and nr12 >= 2 and ny % 4, (nx, ny, tx12)
        assert geom["k12"]["grid"][0] == 8 * -(-nb12 * nr12 // 8), (nb12, nr12, geom)
    if aligned and variant != "oldest" and z is None:
        assert "k_tderiv_c" in ks, kernels  # whole volumes are whole groups of four voxels
    if not aligned:
        assert "k_tderiv" in ks, kernels  # the scalar K0
    k34 = geom["k34"]
    if variant not in NO_K34:  # the pinned geometry: >= 2 column blocks, a partial last one
        assert k34["nbx"] >= 2 and nx % k34["tx"] and k34["nbx"] == -(-nx // k34["tx"]), (nx, geom)
    if variant == "k34_uq0":
        assert "k_prod_wyx" in ks and k34["threads"] == k34["cw"] <= 256, (kernels, geom)
    if variant == "k34_uq1":
        assert "k_prod_wyx" in ks and not {"k_prod_wyx_ws", "k_prod_wyx_pk"} & ks, kernels
        assert k34["threads"] == k34["cw"] >= 256 and k34["tx"] != (k34["cw"] - 2 * rw) & ~3, geom
    if variant == "k34_uq2":
        assert "k_prod_wyx_ws" in ks and k34["threads"] == 2 * k34["cw"], (kernels, geom)
    if variant == "k34_uq3":
        assert "k_prod_wyx_pk" in ks, kernels
    if variant == "k5c_nw8":
        assert geom["k5c"]["nw"] == (8 if k5c_ok else 0), geom
    if variant == "wxy_plain":
        assert geom["wxy_zt"] == 0, geom
    if variant == "wxy_tiled":
        assert (geom["wxy_zt"] != 0) == (k5c_ok and nx % 32 == 0), geom
        if geom["wxy_zt"]:
            assert geom["wxy_zt"] == geom["cap_planes"], geom
    if variant == "default" and k5c_ok and z is None:
        # K5c: blocks of zc planes by 32 columns (of3d_k5.hpp k5c_zc): >= 2 z blocks with a partial
        # last one, >= 2 column tiles (A150: a partial last one)
        zc = 2 * geom["k5c"]["nw"] * geom["k5c"]["r"]
        assert nz > zc and nz % zc and nx > 32, (nz, nx, zc, geom)


# every name of3d_plan_kernels can report (of3d_host.hip kKernelNames) but k_wz_solve_c2, whose kernel was removed
KERNEL_NAMES = {"k_tderiv_c", "k_tderiv", "k_tderiv_multi", "k_grad_xy_c", "k_grad_xy", "k_grad_xyz_c", "k_grad_z_c",
                "k_grad_z", "k_prod_wyx", "k_prod_wyx_ws", "k_prod_wyx_pk", "k_prod_wy", "k_wx", "k_wz_solve_c",
                "k_wz_solve_c_next", "k_wz_solve_dma", "k_wz_solve", "k_solve2d", "general"}
_SEEN = {"cases": set(), "kernels": set(), "k12_deep": False}


def _report(case, kernels, geom):
    _SEEN["cases"].add(case.split()[0])
    _SEEN["kernels"] |= set(kernels)
    _SEEN["k12_deep"] |= bool(geom["k12"]["deep"])
    g = {k: geom[k] for k in ("cap_planes", "wxy_zt", "k34", "k5c", "k12", "k0_batch")}
    print(f"POISON {case}: kernels {','.join(kernels)} geometry {g}")


def _plan(monkeypatch, variant, vol, mode, max_out_planes=0):
    v = VOLS[vol]
    return _pinned_plan(monkeypatch, variant, 3, v["shape"], v["sig"], mode, max_out_planes)


def _slab_frames(plan, vol, z0, z1, k=0, extra=0, misaligned=False):
    """Window k (+ extra frames past it) holding only the planes of of3d_plan_input_range."""
    zi0, zi1 = plan.input_range(z0, z1)
    nt = VOLS[vol]["nt"]
    return poison.guarded_frames(_stack(vol)[k:k + nt + extra, zi0:zi1], misaligned=misaligned), zi0


# ---- 1. full volumes: every kernel family, fresh plan, poisoned workspace -----------------------
def _full_params():
    out = []
    for variant in VARIANTS:
        if variant in ("k34_uq1", "k34_uq2", "k34_uq3"):
            vols = ("WA", "WB")  # forms of up to 512 staged columns: A's and B's sigmas on 604 columns
        elif variant == "k12_deep":
            vols = ("D",)  # marches of 128 planes
        else:
            vols = ("A", "B", "A150")
        for vol in vols:
            for mode in ("fp64", "fp32", "rel64"):
                if mode == "rel64" and (variant not in ("default", "old") or vol == "A150"):
                    continue
                if variant == "k34_uq3" and mode != "fp32":
                    continue  # the packed kernel is float2 arithmetic: no fp64 instance
                if variant == "k12_deep" and mode != "fp64":
                    continue  # the deep instance: fp64, rd 6
                if vol == "A150" and variant not in ("default", "old", "oldest", "k12", "k5c_nw8", "wxy_tiled",
                                                     "general"):
                    continue  # the fallbacks of misaligned rows; the K34 forms do not depend on them
                out.append(pytest.param(vol, variant, mode, id=f"{vol}-{variant}-{mode}"))
    return out


@pytest.mark.parametrize("vol,variant,mode", _full_params())
def test_full_volume_poisoned(vol, variant, mode, monkeypatch):
    m = MODES[mode]
    nz = VOLS[vol]["shape"][0]
    plan = _plan(monkeypatch, variant, vol, m)
    try:
        frames, zi0 = _slab_frames(plan, vol, 0, nz)
        plan.poison()
        got, kernels, geom = poison.run_plan(plan, frames, _lib.OF3D_U16, zi0, 0, nz, m)
    finally:
        plan.close()
    _report(f"full {vol} {variant} {mode}", kernels, geom)
    _expect(variant, vol, mode == "fp32", kernels, geom)
    _check3d(got, _oracle(vol, mode == "fp32"), m, what=f"{vol} {variant} {mode}")


@pytest.mark.parametrize("vol", ["A", "A150"])
@pytest.mark.parametrize("variant", ["default", "k12"])
@pytest.mark.parametrize("mode", ["fp64", "fp32"])
def test_full_volume_misaligned_frames_poisoned(vol, variant, mode, monkeypatch):
    """Frames one element past a 16-byte boundary: the scalar K0, and K1c + K2c where K12 was
    asked for; the plan must say so."""
    m = MODES[mode]
    nz = VOLS[vol]["shape"][0]
    plan = _plan(monkeypatch, variant, vol, m)
    try:
        frames, zi0 = _slab_frames(plan, vol, 0, nz, misaligned=True)
        plan.poison()
        got, kernels, geom = poison.run_plan(plan, frames, _lib.OF3D_U16, zi0, 0, nz, m)
    finally:
        plan.close()
    _report(f"misaligned {vol} {variant} {mode}", kernels, geom)
    _expect(variant, vol, mode == "fp32", kernels, geom, aligned=False)
    _check3d(got, _oracle(vol, mode == "fp32"), m, what=f"{vol} {variant} {mode} misaligned")


# ---- 2. plane ranges on one plan -----------------------------------------------------------------
RANGES = {"A": [(0, 72), (0, 20), (30, 50), (52, 72), (71, 72), (0, 1)], "B": [(0, 52), (22, 26), (44, 52)]}
RANGE_VARIANTS = [("default", "fp64"), ("default", "fp32"), ("old", "fp64"), ("k12", "fp64"), ("wxy_tiled", "fp64"),
                  ("general", "fp64")]


@pytest.mark.parametrize("vol", ["A", "B"])
@pytest.mark.parametrize("variant,mode", RANGE_VARIANTS)
def test_plane_ranges_poisoned(vol, variant, mode, monkeypatch):
    """Output plane ranges on ONE plan, the workspace poisoned before each (so a range finds
    neither zeros nor the previous range's fields), the frames holding only the planes of
    of3d_plan_input_range between loud guard planes.  (30, 50) of A clamps neither halo."""
    m = MODES[mode]
    want = _oracle(vol, mode == "fp32")
    plan = _plan(monkeypatch, variant, vol, m)
    try:
        for z0, z1 in RANGES[vol]:
            frames, zi0 = _slab_frames(plan, vol, z0, z1)
            plan.poison()
            got, kernels, geom = poison.run_plan(plan, frames, _lib.OF3D_U16, zi0, z0, z1, m)
            _report(f"range {vol} {variant} {mode} [{z0}, {z1})", kernels, geom)
            _expect(variant, vol, mode == "fp32", kernels, geom, z=(z0, z1))
            _check3d(got, want, m, z=slice(z0, z1), what=f"{vol} {variant} {mode} planes [{z0}, {z1})")
    finally:
        plan.close()


@pytest.mark.parametrize("variant", ["default", "k12", "wxy_tiled"])
def test_partial_plan_poisoned(variant, monkeypatch):
    """A plan of max_out_planes = 20 (a workspace of 20 + 2 (rw + rd) planes) over planes
    [30, 50) of A, then [0, 20) and [52, 72) on the same plan."""
    want = _oracle("A", False)
    plan = _plan(monkeypatch, variant, "A", 0, max_out_planes=20)
    try:
        assert plan.geometry()["cap_planes"] == 20 + 2 * (9 + 3)
        for z0, z1 in ((30, 50), (0, 20), (52, 72)):
            frames, zi0 = _slab_frames(plan, "A", z0, z1)
            plan.poison()
            got, kernels, geom = poison.run_plan(plan, frames, _lib.OF3D_U16, zi0, z0, z1, 0)
            _report(f"partial A {variant} [{z0}, {z1})", kernels, geom)
            _expect(variant, "A", False, kernels, geom, z=(z0, z1))
            _check3d(got, want, 0, z=slice(z0, z1), what=f"partial plan {variant} planes [{z0}, {z1})")
    finally:
        plan.close()


# ---- 3. row ranges and the overlap schedule ---------------------------------------------------------
@pytest.mark.parametrize("variant", ["default", "k12"])
@pytest.mark.parametrize("mode", ["fp64", "fp32"])
def test_set_rows_poisoned(variant, mode, monkeypatch):
    """set_rows(5, 21) on A: compact, guarded outputs of 16 rows; then set_rows(0, ny) gives the
    full result again on the same plan."""
    m = MODES[mode]
    nz, ny, nx = VOLS["A"]["shape"]
    want = _oracle("A", mode == "fp32")
    plan = _plan(monkeypatch, variant, "A", m)
    try:
        frames, zi0 = _slab_frames(plan, "A", 0, nz)
        for rows in ((5, 21), (0, ny), (30, ny)):
            plan.set_rows(*rows)
            plan.poison()
            got, kernels, geom = poison.run_plan(plan, frames, _lib.OF3D_U16, zi0, 0, nz, m, rows=rows)
            _report(f"rows A {variant} {mode} {rows}", kernels, geom)
            _expect(variant, "A", mode == "fp32", kernels, geom)
            _check3d(got, want, m, y=slice(*rows), what=f"rows {rows} {variant} {mode}")
    finally:
        plan.close()


@pytest.mark.parametrize("variant", ["default", "k12", "wxy_tiled"])
def test_overlap_chunks_poisoned(variant, monkeypatch):
    """set_overlap(16) on A (five chunks, the last one short; two streams): poison and execute
    three times on one plan, bitwise against the oracle each time."""
    nz = VOLS["A"]["shape"][0]
    want = _oracle("A", False)
    plan = _plan(monkeypatch, variant, "A", 0)
    try:
        plan.set_overlap(16)
        frames, zi0 = _slab_frames(plan, "A", 0, nz)
        for rep in range(3):
            plan.poison()
            got, kernels, geom = poison.run_plan(plan, frames, _lib.OF3D_U16, zi0, 0, nz, 0)
            _expect(variant, "A", False, kernels, geom, z=(0, nz))  # (z: K12 marches per chunk, not per volume)
            _check3d(got, want, 0, what=f"overlap {variant} run {rep}")
        _report(f"overlap A {variant}", kernels, geom)
    finally:
        plan.close()


# ---- 4. series: execute_next and execute_ahead ---------------------------------------------------
def _series_call(plan, frames, k, call, m):
    nt, nwins, nz = VOLS["S"]["nt"], VOLS["S"]["nwins"], VOLS["S"]["shape"][0]
    if call == "next":
        nxt = frames[k + 1:k + 1 + nt] if k + 1 < nwins else None
        return poison.run_plan(plan, frames[k:k + nt], _lib.OF3D_U16, 0, 0, nz, m, call="next", next_frames=nxt)
    return poison.run_plan(plan, frames[k:k + nt], _lib.OF3D_U16, 0, 0, nz, m, call="ahead",
                           ahead_frames=frames[k + nt:nt + nwins - 1])


@pytest.mark.parametrize("call", ["next", "ahead"])
@pytest.mark.parametrize("mode", ["fp64", "fp32"])
@pytest.mark.parametrize("repoison", [False, True])
def test_series_poisoned(call, mode, repoison, monkeypatch):
    """Four windows of A-sized frames (volume S) through of3d_plan_execute_next (window k's K5c forms
    window k + 1's dt0) and of3d_plan_execute_ahead (OF3D_K12=1: window 0's batched K0 forms
    all four), poisoned once before the first call: every window exact, the fused / batched
    kernels reported.  repoison: poison again between windows 1 and 2, which destroys the
    pending dt0 — the entry dropped its tags, so window 2 recomputes and is exact (a stale tag
    would read NaN)."""
    variant = "k12" if call == "ahead" else "default"
    m = MODES[mode]
    plan = _plan(monkeypatch, variant, "S", m)
    try:
        frames = poison.guarded_frames(_stack("S"))
        plan.poison()
        for k in range(VOLS["S"]["nwins"]):
            if repoison and k == 2:
                plan.poison()
            before = set(plan.kernels())
            got, kernels, geom = _series_call(plan, frames, k, call, m)
            _report(f"series {call} {mode} repoison={int(repoison)} window {k}", kernels, geom)
            assert geom["k34"]["nbx"] >= 2 and VOLS["S"]["shape"][2] % geom["k34"]["tx"], geom  # (the pinned K34)
            _check3d(got, _oracle("S", mode == "fp32", k), m, what=f"{call} {mode} window {k}")
            if call == "ahead" and k == 0:
                assert geom["k0_batch"] == 4 and {"k_tderiv_multi", "k_grad_xyz_c"} <= set(kernels), (kernels, geom)
                assert not {"k_tderiv_c", "k_tderiv"} & set(kernels), kernels
            if call == "ahead" and k == 2:
                # repoison dropped the slots: window 2 formed its own dt0 (and window 3's) again
                assert geom["k0_batch"] == (2 if repoison else 4), geom
            if call == "next" and k == 0:
                assert "k_wz_solve_c_next" in kernels and "k_tderiv_c" in kernels, kernels
            if call == "next" and not repoison and k == 1:
                assert before == set(kernels), (before, kernels)
        if call == "ahead" and not repoison:  # one batched pass fed all four windows
            assert not {"k_tderiv_c", "k_tderiv"} & set(plan.kernels()), plan.kernels()
    finally:
        plan.close()


# ---- 5. 2D batches -----------------------------------------------------------------------------------
_ORACLE2D = {}


def _series2d(nx):
    return np.random.default_rng(9200 + nx).integers(0, 4096, size=(9, 37, nx)).astype(np.uint16)


def _oracle2d(nx, fp32, b):
    key = (nx, bool(fp32), b)
    if key not in _ORACLE2D:
        img = _series2d(nx)[b:b + 7]
        _ORACLE2D[key] = (cpu_ref.calc_flow2D_fp32_oracle(img, 1, 1, 3) if fp32
                          else cpu_ref.calc_flow2D(img, 1, 1, 3, backend="scipy"))
    return _ORACLE2D[key]


def _check2d(got, want, fp32, what):
    for name, a, b in zip(("vx", "vy", "rel"), got, want):
        assert a.dtype == b.dtype == (np.float32 if fp32 else np.float64), (what, name, a.dtype, b.dtype)
        if fp32 and name == "rel":  # as test_gpu_fp32_exact: NaN at the same pixels, equal bits elsewhere
            nan = np.isnan(b)
            assert np.array_equal(np.isnan(a), nan), f"{what}: rel: NaN at other pixels"
            a, b = np.where(nan, np.float32(0), a), np.where(nan, np.float32(0), b)
        assert bits_equal(a, b), f"{what}: {name} differs from the oracle ({int(np.isnan(a).sum())} NaN)"


@pytest.mark.parametrize("nx", [160, 150])
@pytest.mark.parametrize("variant", ["default", "old", "general"])
@pytest.mark.parametrize("mode", ["fp64", "fp32"])
def test_batch_2d_poisoned(nx, variant, mode, monkeypatch):
    """A 2D plan over a batch of three output frames (plane b: the image of window b; the frame
    pointers are the series shifted by 0 .. 2 rt frames), whole and as the sub-range [1, 3)
    with the frames holding only those planes."""
    m = MODES[mode]
    fp32 = mode == "fp32"
    series = _series2d(nx)
    nwin, nout = 7, 3
    plan = _pinned_plan(monkeypatch, variant, 2, (nout, 37, nx), (1, 1, 3), m)
    try:
        for z0, z1 in ((0, nout), (1, 3)):
            assert plan.input_range(z0, z1) == (z0, z1)
            frames = poison.guarded_frames(np.stack([series[j + z0:j + z1] for j in range(nwin)]))
            plan.poison()
            got, kernels, geom = poison.run_plan(plan, frames, _lib.OF3D_U16, z0, z0, z1, m)
            _report(f"2d nx {nx} {variant} {mode} [{z0}, {z1})", kernels, geom)
            if variant == "general":
                assert kernels == ["general"], kernels
            else:
                assert "k_solve2d" in kernels and "general" not in kernels, kernels
                assert ("k_grad_xy" in kernels) == (variant == "old"), kernels
                assert any(k.startswith("k_prod_wyx") for k in kernels) == (variant == "default"), kernels
            if variant == "default":  # the pinned K34: >= 2 column blocks, a partial last one
                assert geom["k34"]["nbx"] >= 2 and nx % geom["k34"]["tx"], geom
            for b in range(z0, z1):
                _check2d([g[b - z0] for g in got], _oracle2d(nx, fp32, b), fp32,
                         f"2D nx {nx} {variant} {mode} plane {b}")
    finally:
        plan.close()


def test_every_kernel_name_ran_poisoned():
    """Where this whole file ran (every group of cases above reported), every kernel name
    of3d_plan_kernels can report appeared in a poisoned case, the deep K12 instance included."""
    groups = {"full", "misaligned", "range", "partial", "rows", "overlap", "series", "2d"}
    if _SEEN["cases"] >= groups:  # (a selection of cases with -k proves nothing about the rest)
        assert _SEEN["kernels"] >= KERNEL_NAMES, sorted(KERNEL_NAMES - _SEEN["kernels"])
        assert _SEEN["k12_deep"]
        print(f"POISON coverage: checked, {len(_SEEN['kernels'])} kernel names")
    else:  # visible in the run's warnings summary: a pass here says nothing about coverage
        import warnings

        warnings.warn(f"kernel coverage NOT checked: only the groups {sorted(_SEEN['cases'])} ran in this process "
                      f"(of {sorted(groups)})")
    assert not _SEEN["kernels"] - KERNEL_NAMES, sorted(_SEEN["kernels"] - KERNEL_NAMES)  # a new name: cover it here


# ---- 6. the host entry points' cached plans and staging ----------------------------------------------
@pytest.mark.parametrize("poisoned", [True, False])
def test_host_entry_3d_second_call(poisoned):
    """calc_flow3D(A), then calc_flow3D(B) of the same shape: the cached plan's workspace and
    staging start from A's fields (or, poisoned, from 0xFF bytes); B's result is B's oracle."""
    a, b = _stack("S")[0:13], _stack("S")[1:14]
    calc_flow3D(a, *VOLS["S"]["sig"])
    if poisoned:  # the entry met the plan calc_flow3D keeps (the cache holds its last two shapes)
        assert 1 <= _lib.cache_poison() <= 2
    got = calc_flow3D(b, *VOLS["S"]["sig"])
    _check3d(list(got), _oracle("S", False, 1), 0, what=f"calc_flow3D second call (poisoned={poisoned})")


@pytest.mark.parametrize("poisoned", [True, False])
def test_host_entry_2d_second_call(poisoned):
    series = _series2d(150)
    calc_flow2D(series[0:7], 1, 1, 3)
    if poisoned:
        assert 1 <= _lib.cache_poison() <= 2
    got = calc_flow2D(series[1:8], 1, 1, 3)
    _check2d(list(got), _oracle2d(150, False, 1), False, f"calc_flow2D second call (poisoned={poisoned})")


def test_cache_poison_with_an_empty_cache():
    _lib.cache_clear()
    assert _lib.cache_poison() == 0 and _lib.cache_poison(0) == 0
    calc_flow2D(_series2d(150)[0:7], 1, 1, 3)
    assert _lib.cache_poison() == 1  # exactly the plan that call cached
