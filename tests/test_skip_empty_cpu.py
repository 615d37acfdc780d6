"""Empty-space skipping without a GPU: the entry points exist and refuse bad arguments on the host before any HIP call
(csrc/skip_empty_kernels.hip), the numpy restatement (tests/skip_empty_ref.py) agrees with brute force, and the Python layer refuses bad
knobs before it touches a tensor."""
import ctypes
import itertools

import numpy as np
import pytest

import skip_empty_ref as R

INVALID, UNSUPPORTED = -1, -2
FAKE = ctypes.c_void_p(0x1000)
ODD = ctypes.c_void_p(0x1001)


def _lib():
    from nerfdet_amd import _lib
    return _lib, _lib.load()


def _i3(*v):
    return (ctypes.c_int * 3)(*v)


def test_entry_points_exist():
    L, lib = _lib()
    for name in ("ndet_occupancy_bits", "ndet_cull_blocks", "ndet_cull_count", "ndet_cull_write", "ndet_ray_view_count_bank"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert L.NDET_OUTSIDE == {"keep": 0, "cull": 1}
    from nerfdet_amd import ops, rays, streaming
    assert callable(ops.occupancy_bits) and callable(rays.cull_points) and callable(rays.ray_view_count_bank)
    assert hasattr(rays, "OccupancyGrid") and hasattr(streaming.SceneStream, "occupancy") and hasattr(streaming.SceneGroup, "occupancy")
    # a block of points is 512 points: the counts array of a cull
    assert [lib.ndet_cull_blocks(n) for n in (-3, 0, 1, 512, 513, 3 * 1024 + 17)] == [0, 0, 1, 1, 2, 7]


def test_occupancy_bits_host_checks():
    _, lib = _lib()
    ok = dict(alpha=FAKE, count=FAKE, nx=4, ny=4, nz=4, threshold=1e-3, dilate=1, bits=FAKE)

    def call(**bad):
        a = dict(ok, **bad)
        return lib.ndet_occupancy_bits(a["alpha"], a["count"], a["nx"], a["ny"], a["nz"], a["threshold"], a["dilate"], a["bits"], None)

    for key in ("alpha", "count", "bits"):
        assert call(**{key: None}) == INVALID and b"null" in lib.ndet_last_error()
    for key in ("nx", "ny", "nz"):
        assert call(**{key: 0}) == INVALID and call(**{key: -2}) == INVALID
    for d in (-1, 3):
        assert call(dilate=d) == INVALID and b"dilate" in lib.ndet_last_error()
    for t in (float("nan"), float("inf"), -float("inf")):
        assert call(threshold=t) == INVALID and b"threshold" in lib.ndet_last_error()
    assert call(nx=2048, ny=1024, nz=1024) == UNSUPPORTED and b"2^31" in lib.ndet_last_error()
    for key in ("alpha", "count", "bits"):
        assert call(**{key: ODD}) == UNSUPPORTED and b"misaligned" in lib.ndet_last_error()
    assert call(count=ctypes.c_void_p(0x1004)) == UNSUPPORTED       # int64 counts: 8-byte aligned


@pytest.mark.parametrize("write", [False, True])
def test_cull_host_checks(write):
    _, lib = _lib()
    from nerfdet_amd._lib import float3
    ok = dict(pts=FAKE, n=100, bits=FAKE, nv=_i3(4, 4, 4), p0=float3([0, 0, 0]), vs=float3([.1, .1, .1]), outside=0, a=FAKE, b=FAKE, c=FAKE)

    def call(**bad):
        a = dict(ok, **bad)
        if write:
            return lib.ndet_cull_write(a["pts"], a["n"], a["bits"], a["nv"], a["p0"], a["vs"], a["outside"], a["a"], a["b"], a["c"], None)
        return lib.ndet_cull_count(a["pts"], a["n"], a["bits"], a["nv"], a["p0"], a["vs"], a["outside"], a["a"], None)

    for key in ("pts", "bits", "nv", "p0", "vs", "a") + (("b", "c") if write else ()):
        assert call(**{key: None}) == INVALID and b"null" in lib.ndet_last_error(), key
    assert call(n=0) == INVALID and call(n=-1) == INVALID
    assert call(nv=_i3(4, 0, 4)) == INVALID
    for vs in ([.1, 0.0, .1], [.1, .1, -1.0], [float("nan"), .1, .1], [.1, float("inf"), .1]):
        assert call(vs=float3(vs)) == INVALID and b"voxel size" in lib.ndet_last_error()
    assert call(p0=float3([0, float("nan"), 0])) == INVALID
    for outside in (-1, 2):
        assert call(outside=outside) == INVALID and b"outside" in lib.ndet_last_error()
    assert call(n=1 << 31) == UNSUPPORTED and b"2^31" in lib.ndet_last_error()
    assert call(nv=_i3(2048, 1024, 1024)) == UNSUPPORTED
    for key in ("pts", "bits", "a") + (("b", "c") if write else ()):
        assert call(**{key: ODD}) == UNSUPPORTED and b"misaligned" in lib.ndet_last_error(), key


def test_count_bank_host_checks():
    _, lib = _lib()
    ok = dict(pts=FAKE, n=100, views=FAKE, n_views=3, pm=FAKE, vc=FAKE)

    def call(**bad):
        a = dict(ok, **bad)
        return lib.ndet_ray_view_count_bank(a["pts"], a["n"], a["views"], a["n_views"], 64.0, 96.0, a["pm"], a["vc"], None)

    for key in ("pts", "views", "pm", "vc"):
        assert call(**{key: None}) == INVALID and b"null" in lib.ndet_last_error()
    assert call(n=0) == INVALID and call(n_views=0) == INVALID
    assert call(n=1 << 31) == UNSUPPORTED and b"2^31" in lib.ndet_last_error()
    assert call(views=ctypes.c_void_p(0x1004)) == UNSUPPORTED
    for key in ("pts", "vc"):
        assert call(**{key: ODD}) == UNSUPPORTED and b"misaligned" in lib.ndet_last_error()
    # (the 2^24-workgroup bound of the three launchers lies beyond 2^31 points or voxels, which are refused first: it guards the block sizes)


# ---- the restatement against brute force ----
def _brute_bits(alpha, count, nv, thr, dilate):
    nx, ny, nz = nv
    n_all = nx * ny * nz
    words = np.zeros((n_all + 31) // 32, dtype=np.uint32)
    flat = lambda x, y, z: (x * ny + y) * nz + z
    for x, y, z in itertools.product(range(nx), range(ny), range(nz)):
        hit = False
        for dx, dy, dz in itertools.product(range(-dilate, dilate + 1), repeat=3):
            u, v, w = x + dx, y + dy, z + dz
            if 0 <= u < nx and 0 <= v < ny and 0 <= w < nz:
                a = alpha[flat(u, v, w)]
                hit = hit or (not (a <= np.float32(thr))) or count[flat(u, v, w)] == 0
        if hit:
            n = flat(x, y, z)
            words[n >> 5] |= np.uint32(1) << np.uint32(n & 31)
    return words.view(np.int32)


@pytest.mark.parametrize("dilate", [0, 1, 2])
def test_restatement_of_the_grid_against_brute_force(dilate):
    nv = (5, 3, 7)
    alpha, count, thr = R.grid_case(nv, 3)
    with np.errstate(invalid="ignore"):
        got = R.occupancy_bits(alpha, count, nv, thr, dilate)
        want = _brute_bits(alpha, count, nv, thr, dilate)
    assert got.dtype == np.int32 and got.shape == (4,) and np.array_equal(got, want)
    frac = np.unpackbits(got.view(np.uint8)).sum() / 105
    assert 0 < frac < 1, frac
    assert (got.view(np.uint32)[-1] >> np.uint32(105 - 96)) == 0         # the ragged word's spare bits


def test_restatement_of_the_cull_against_brute_force():
    nv, p0, vs = (5, 3, 7), np.float32([-0.4, 0.3, 1.0]), np.float32([0.16, 0.2, 0.1])
    alpha, count, thr = R.grid_case(nv, 5)
    bits = R.occupancy_bits(alpha, count, nv, thr, 0)
    rng = np.random.RandomState(7)
    lattice = np.stack(np.meshgrid(*[np.arange(-1, n + 1) for n in nv], indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    pts = np.concatenate([lattice * vs + p0, (lattice + np.float32(0.5)) * vs + p0, (rng.rand(200, 3).astype(np.float32) * 9 - 2) * vs + p0,
                          np.float32([[np.nan, 0.5, 1.2], [0.0, np.inf, 1.2], [0.0, 0.5, -np.inf]])]).astype(np.float32)
    for outside in ("keep", "cull"):
        idx, kept = R.cull(pts, bits, nv, p0, vs, outside)
        want = []
        for j, p in enumerate(pts):
            with np.errstate(invalid="ignore", over="ignore"):
                f = [np.floor(np.float32(np.float32((p[k] - p0[k]) / vs[k]) + np.float32(0.5))) for k in range(3)]
            inside = all(np.isfinite(p)) and all(0 <= f[k] < nv[k] for k in range(3))
            if inside:
                n = (int(f[0]) * nv[1] + int(f[1])) * nv[2] + int(f[2])
                keep = bool((bits.view(np.uint32)[n >> 5] >> np.uint32(n & 31)) & 1)
            else:
                keep = outside == "keep"
            if keep:
                want.append(j)
        assert idx.dtype == np.int32 and np.array_equal(idx, np.int32(want)) and np.array_equal(kept, pts[want], equal_nan=True)
        assert 0 < len(want) < len(pts)


# ---- the Python layer refuses before it touches a tensor ----
def test_knobs_are_checked_before_any_launch():
    import torch
    from nerfdet_amd import rays, streaming
    for bad in (dict(threshold=float("nan")), dict(threshold="x"), dict(threshold=True), dict(dilate=3), dict(dilate=1.0), dict(outside="drop")):
        with pytest.raises(ValueError):
            streaming._check_occupancy_knobs(**dict(streaming.SKIP_EMPTY_DEFAULTS, **bad))
    assert streaming._check_occupancy_knobs(0, np.int64(2), "cull") == (0.0, 2, "cull")
    import types
    nv, dev = (5, 3, 7), torch.device("cpu")
    det = types.SimpleNamespace(n_voxels=list(nv))
    assert streaming._skip_knobs(None, None, dev, "render_rays") is None and streaming._skip_knobs(False, None, dev, "render_rays") is None
    assert streaming._skip_knobs(True, det, dev, "render_rays") == streaming.SKIP_EMPTY_DEFAULTS
    assert streaming._skip_knobs(dict(dilate=0), det, dev, "render_rays") == dict(threshold=1e-3, dilate=0, outside="keep")
    for bad in (dict(dilate=5), dict(treshold=0.1), 3, "yes"):
        with pytest.raises(ValueError):
            streaming._skip_knobs(bad, det, dev, "render_rays")
    bits = torch.zeros(4, dtype=torch.int32)
    grid = rays.OccupancyGrid(bits, nv, (0.0, 0.0, 0.0), (0.1, 0.1, 0.1), "cull")
    assert grid.n_voxels == nv and grid.outside == "cull" and grid.voxel_size == tuple(float(np.float32(0.1)) for _ in range(3))
    with pytest.raises(ValueError, match="n_voxels"):
        streaming._skip_knobs(grid, types.SimpleNamespace(n_voxels=(5, 3, 8)), dev, "render_rays")
    with pytest.raises(RuntimeError, match="GPU"):
        streaming._skip_knobs(grid, det, dev, "render_rays")            # a grid whose bits lie in host memory
    for bad in (dict(bits=torch.zeros(3, dtype=torch.int32)), dict(bits=bits.to(torch.int64)), dict(voxel_size=(0.1, 0.0, 0.1)), dict(outside="x"),
                dict(p0=(0.0, float("inf"), 0.0)), dict(n_voxels=(5, 3))):
        args = dict(dict(bits=bits, n_voxels=nv, p0=(0.0, 0.0, 0.0), voxel_size=(0.1, 0.1, 0.1), outside="keep"), **bad)
        with pytest.raises(ValueError):
            rays.OccupancyGrid(**args)
    with pytest.raises(RuntimeError, match="GPU"):
        rays.cull_points(torch.zeros(4, 3), grid)
