"""Space carving without a GPU: the two entry points exist and refuse bad arguments on the host before any HIP call
(csrc/carve_kernels.hip), the Python layer refuses bad knobs before it touches a tensor, rays.CarveStore follows a scene's chunks, the
shared inputs of the GPU tests hold the cases they are meant to hold, and the DEFINITION itself (tests/carve_ref.py) carves a wall scene
as float64 geometry says it should."""
import ctypes
import types

import numpy as np
import pytest
import torch

import carve_ref as C

INVALID, UNSUPPORTED = -1, -2
FAKE = ctypes.c_void_p(0x1000)
ODD = ctypes.c_void_p(0x1001)


def _lib():
    from nerfdet_amd import _lib
    return _lib, _lib.load()


def test_entry_points_exist():
    L, lib = _lib()
    for name in ("ndet_carve_accumulate", "ndet_carve_bits"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    from nerfdet_amd import ops, rays, streaming
    assert callable(ops.carve_accumulate) and callable(ops.carve_bits) and hasattr(rays, "CarveStore")
    for cls in (streaming.SceneStream, streaming.SceneGroup):
        assert hasattr(cls, "carve_counts")
    assert ops.carve_lattice((40, 40, 16), (0.16, 0.16, 0.2), 4) == ((160, 160, 64), tuple(float(np.float32(v) / np.float32(4)) for v in (0.16, 0.16, 0.2)))
    assert ops.carve_lattice((5, 3, 7), (0.16, 0.16, 0.2), 1)[1] == tuple(float(np.float32(v)) for v in (0.16, 0.16, 0.2))
    for bad in (3, 0, True, 2.0):
        with pytest.raises(ValueError, match="refine"):
            ops.carve_lattice((4, 4, 4), (0.1, 0.1, 0.1), bad)


def test_carve_accumulate_host_checks():
    _, lib = _lib()
    ok = dict(points=FAKE, nx=4, ny=4, nz=4, proj=FAKE, k=3, depth=FAKE, dtype=0, vp=24 * 32, rp=32, H=24, W=32, band=0.25, counts=FAKE)

    def call(**bad):
        a = dict(ok, **bad)
        return lib.ndet_carve_accumulate(a["points"], a["nx"], a["ny"], a["nz"], a["proj"], a["k"], a["depth"], a["dtype"], a["vp"], a["rp"], a["H"],
                                         a["W"], a["band"], a["counts"], None)

    for key in ("points", "proj", "depth", "counts"):
        assert call(**{key: None}) == INVALID and b"null" in lib.ndet_last_error(), key
    for key in ("nx", "ny", "nz", "k", "H", "W"):
        assert call(**{key: 0}) == INVALID and call(**{key: -2}) == INVALID, key
    for band in (0.0, -1.0, float("nan"), float("inf")):
        assert call(band=band) == INVALID and b"band" in lib.ndet_last_error()
    assert call(dtype=2) == INVALID and b"dtype" in lib.ndet_last_error()
    assert call(rp=31) == INVALID and call(vp=24 * 32 - 1) == INVALID and b"pitches" in lib.ndet_last_error()
    assert call(nx=2048, ny=1024, nz=1024) == UNSUPPORTED and b"2^31" in lib.ndet_last_error()
    for key in ("points", "proj", "depth", "counts"):
        assert call(**{key: ODD}) == UNSUPPORTED and b"misaligned" in lib.ndet_last_error(), key
    assert call(depth=ctypes.c_void_p(0x1004), dtype=1) == UNSUPPORTED           # a float64 map: 8-byte aligned
    # (the 2^24-workgroup bound lies beyond 2^31 voxels, which are refused first: it guards the block size)


def test_carve_bits_host_checks():
    _, lib = _lib()

    def segs(n, ptr=0x1000):
        return (ctypes.c_void_p * max(n, 1))(*([ptr] * n))

    ok = dict(segs=segs(2), n=2, min_free=2, dilate=1, nx=4, ny=4, nz=4, coarse=None, refine=1, scratch=None, bits=FAKE)

    def call(**bad):
        a = dict(ok, **bad)
        return lib.ndet_carve_bits(a["segs"], a["n"], a["min_free"], a["dilate"], a["nx"], a["ny"], a["nz"], a["coarse"], a["refine"], a["scratch"],
                                   a["bits"], None)

    assert call(segs=None) == INVALID and call(bits=None) == INVALID and b"null" in lib.ndet_last_error()
    assert call(segs=segs(2, 0)) == INVALID and b"null" in lib.ndet_last_error()
    for n in (0, -1, 65):
        assert call(segs=segs(65), n=n) == INVALID and b"segments" in lib.ndet_last_error()
    for key in ("nx", "ny", "nz"):
        assert call(**{key: 0}) == INVALID and call(**{key: -2}) == INVALID
    for m in (0, -3):
        assert call(min_free=m) == INVALID and b"min_free" in lib.ndet_last_error()
    for d in (-1, 3):
        assert call(dilate=d) == INVALID and b"dilate" in lib.ndet_last_error()
    for r in (0, 3, 8):
        assert call(refine=r) == INVALID and b"refine" in lib.ndet_last_error()
    assert call(coarse=FAKE, refine=4, nz=6) == INVALID and b"multiples" in lib.ndet_last_error()
    assert call(scratch=FAKE, bits=FAKE) == INVALID
    assert call(nx=2048, ny=1024, nz=1024) == UNSUPPORTED and b"2^31" in lib.ndet_last_error()
    for bad in (dict(bits=ODD), dict(coarse=ODD), dict(scratch=ODD), dict(segs=segs(2, 0x1002))):
        assert call(**bad) == UNSUPPORTED and b"misaligned" in lib.ndet_last_error(), bad


def test_knobs_are_checked_before_any_launch():
    from nerfdet_amd import rays, streaming
    vs = types.SimpleNamespace(voxel_size=(0.16, 0.16, 0.2))
    assert streaming._carve_knobs(None, vs) is None and streaming._carve_knobs(False, vs) is None
    assert streaming._carve_knobs(True, vs) == (2, 0.2) and streaming._carve_knobs(dict(refine=4), vs) == (4, 0.2)
    assert streaming._carve_knobs(dict(refine=1, band=0.05), vs) == (1, 0.05)
    for bad in (dict(refine=3), dict(refine=2.0), dict(refine=True), dict(band=0.0), dict(band=-1), dict(band=float("nan")), dict(band="x"),
                dict(rafine=2), 2, "yes"):
        with pytest.raises(ValueError):
            streaming._carve_knobs(bad, vs)
    assert streaming._check_source_knobs("depth", np.int64(3)) == ("depth", 3)
    for bad in (("gamma", 2), ("depth", 0), ("depth", 1.0), ("both", True), ("alpha", 65536)):
        with pytest.raises(ValueError):
            streaming._check_source_knobs(*bad)
    # skip_empty=: the new keys are carried only when the caller gave them
    dev = torch.device("cpu")
    det = types.SimpleNamespace(n_voxels=[5, 3, 7])
    assert streaming._skip_knobs(True, det, dev, "render_rays") == streaming.SKIP_EMPTY_DEFAULTS == dict(threshold=1e-3, dilate=1, outside="keep")
    assert streaming._skip_knobs(dict(dilate=0), det, dev, "render_rays") == dict(threshold=1e-3, dilate=0, outside="keep")
    assert streaming._skip_knobs(dict(source="depth"), det, dev, "r") == dict(threshold=1e-3, dilate=1, outside="keep", source="depth")
    assert streaming._skip_knobs(dict(min_free=3, dilate=2), det, dev, "r") == dict(threshold=1e-3, dilate=2, outside="keep", min_free=3)
    for bad in (dict(source="sensor"), dict(min_free=0), dict(source="depth", min_free=2.5), dict(sauce="depth")):
        with pytest.raises(ValueError):
            streaming._skip_knobs(bad, det, dev, "render_rays")
    # a source that needs a carve, on a scene without one
    with pytest.raises(ValueError, match="carve"):
        streaming._need_carve(None, "depth", "occupancy")
    streaming._need_carve(None, "alpha", "occupancy")


def test_the_relaxed_lattice_rule():
    """A caller's grid may refine the detector's lattice by 1, 2 or 4 on all three axes; anything else is refused, naming n_voxels."""
    from nerfdet_amd import rays, streaming
    dev = torch.device("cpu")
    nv = (5, 3, 7)
    det = types.SimpleNamespace(n_voxels=list(nv))

    def grid(n):
        return rays.OccupancyGrid(torch.zeros(((n[0] * n[1] * n[2] + 31) // 32,), dtype=torch.int32), n, (0.0, 0.0, 0.0), (0.1, 0.1, 0.1), "cull")

    for r in (1, 2, 4):
        assert streaming._grid_refine(tuple(r * v for v in nv), nv) == r
        with pytest.raises(RuntimeError, match="GPU"):            # accepted as a lattice; its bits lie in host memory
            streaming._skip_knobs(grid(tuple(r * v for v in nv)), det, dev, "render_rays")
    for other in ((15, 9, 21), (10, 6, 7), (10, 3, 14), (5, 3, 8), (40, 24, 56), (20, 12, 14)):
        assert streaming._grid_refine(other, nv) is None
        with pytest.raises(ValueError, match="n_voxels"):
            streaming._skip_knobs(grid(other), det, dev, "render_rays")


def test_carve_store_life_cycle():
    from nerfdet_amd import rays
    n = 12
    one = lambda v: torch.full((n,), v, dtype=torch.int32)
    # windowed: a segment per chunk, spares reused
    st = rays.CarveStore(n, "cpu", windowed=True)
    assert st.segments == [] and st.nbytes() == 0
    a = st.target()
    assert a.dtype == torch.int32 and tuple(a.shape) == (n,) and not a.any() and st.segments == []
    a += 1
    st.push(a)
    b = st.target()
    assert b is not a and not b.any()
    b += 2
    st.push(b)
    assert [int(s[0]) for s in st.segments] == [1, 2] and st.nbytes() == 8 * n
    st.drop_oldest(1)
    assert [int(s[0]) for s in st.segments] == [2]
    c = st.target()
    assert c is a and not c.any()                                  # the dropped segment, zeroed: nothing is allocated
    c += 3
    st.give_back(c)                                                # a chunk that failed
    assert [int(s[0]) for s in st.segments] == [2] and st.target() is a and not a.any()
    with pytest.raises(ValueError):
        st.give_back(b)                                            # held
    st.push(a)                                                     # a chunk without depth: all zero
    assert [int(s[0]) for s in st.segments] == [2, 0]
    for bad in (-1, 3, True, 1.0):
        with pytest.raises(ValueError):
            st.drop_oldest(bad)
    st.drop_oldest(0)
    st.clear()
    assert st.segments == [] and st.nbytes() == 8 * n and all(not s.any() for s in st._spare)
    with pytest.raises(ValueError):
        st.push(torch.zeros(n + 1, dtype=torch.int32))
    with pytest.raises(ValueError):
        st.push(torch.zeros(n, dtype=torch.int64))
    # unwindowed: one segment that accumulates
    st = rays.CarveStore(n, "cpu", windowed=False)
    a = st.target()
    a += 1
    st.push(a)
    assert st.target() is a
    a += 1
    st.push(a)
    assert len(st.segments) == 1 and int(st.segments[0][0]) == 2
    with pytest.raises(ValueError):
        st.push(one(5))
    st.clear()
    assert st.segments == [] and st.target() is a and not a.any()
    with pytest.raises(ValueError):
        rays.CarveStore(0, "cpu", True)


# ---- the restatement and the shared inputs ----
LATTICES = [(5, 3, 7), (8, 8, 40)]


@pytest.mark.parametrize("nv", LATTICES)
@pytest.mark.parametrize("refine", [1, 2, 4])
def test_the_shared_views_hold_every_case(nv, refine):
    """What the GPU counter tests rely on: holes, a negative and a NaN depth under accepted pixels, points outside the image and behind a
    camera, camera depths exactly on d - band and d + band, and all three of free, hit and behind."""
    from oracle import nerfdet_oracle as O
    pts = C.fine_points(nv, refine)
    assert tuple(pts.shape[1:]) == tuple(refine * v for v in nv)
    coarse = C.fine_points(nv, 1)
    lo, hi = pts.reshape(3, -1).min(1).values, pts.reshape(3, -1).max(1).values
    assert torch.allclose((lo + hi) / 2 + torch.tensor(C.VS) / (2 * refine), (coarse.reshape(3, -1).min(1).values + coarse.reshape(3, -1).max(1).values) / 2
                          + torch.tensor(C.VS) / 2, atol=1e-6)                  # the same box, the same centre
    for k in (1, 3):
        proj, depth = C.views_case(nv, k, np.float64)
        free, hit = C.evidence(pts, proj, depth, C.BAND, C.HW)
        with np.errstate(all="ignore"):
            fu, fv, z = (t.numpy() for t in O.project_voxels(pts, proj))
            x, y = np.rint(fu), np.rint(fv)
            ok = (x >= 0) & (y >= 0) & (x < C.HW[1]) & (y < C.HW[0]) & (z > 0)
            d = depth[np.arange(k)[:, None], np.where(ok, y, 0).astype(int), np.where(ok, x, 0).astype(int)]
        assert (ok & (d == 0)).any() and (ok & (d < 0)).any() and (ok & np.isnan(d)).any()
        assert not (free & hit).any() and not ((free | hit) & ~(ok & (d > 0))).any()
        assert (z[0] == d[0] - C.BAND)[ok[0]].any() and (z[0] == d[0] + C.BAND)[ok[0]].any(), "the dyadic view misses an edge"
        assert free[0][ok[0] & (z[0] == d[0] - C.BAND)].all() and not hit[0][ok[0] & (z[0] == d[0] + C.BAND)].any()
        assert not free[0][ok[0] & (z[0] == d[0] + C.BAND)].any()
        if k > 1:
            assert (~ok & (z > 0)).any() and (z <= 0).any()
            behind = ok & (d > 0) & ~free & ~hit
            assert free.any() and hit.any() and behind.any()
        f32 = C.evidence(pts, proj, depth.astype(np.float32), C.BAND, C.HW)
        assert f32[0].shape == free.shape


def test_counters_saturate_and_chunk():
    nv = (5, 3, 7)
    pts = C.fine_points(nv, 2)
    proj, depth = C.views_case(nv, 6, np.float64)
    n = pts[0].numel()
    zero = np.zeros(n, dtype=np.int32)
    whole = C.accumulate(zero, pts, proj, depth, C.BAND, C.HW)
    parts = C.accumulate(C.accumulate(zero, pts, proj[:2], depth[:2], C.BAND, C.HW), pts, proj[2:], depth[2:], C.BAND, C.HW)
    assert np.array_equal(whole, parts) and whole.any()
    full = C.pack(np.full(n, 65534), np.full(n, 65535))
    after = C.accumulate(full, pts, proj[:3], depth[:3], C.BAND, C.HW)
    f, h = C.unpack(after)
    assert f.max() == 65535 and f.min() == 65534 and (h == 65535).all()


def test_restated_bits_against_brute_force():
    import itertools
    nv, r = (4, 2, 6), 2
    n = nv[0] * nv[1] * nv[2]
    segs = C.segments_case(n, 3, 5)
    coarse = C.pack_bits(np.random.RandomState(3).rand(n // 8) < 0.6)
    free = sum(C.unpack(s)[0] for s in segs)
    hit = sum(C.unpack(s)[1] for s in segs)
    for min_free, dilate, cb in itertools.product((1, 3), (0, 1, 2), (None, coarse)):
        want = np.zeros(n, dtype=bool)
        for x, y, z in itertools.product(*[range(v) for v in nv]):
            for dx, dy, dz in itertools.product(range(-dilate, dilate + 1), repeat=3):
                u, v, w = x + dx, y + dy, z + dz
                if 0 <= u < nv[0] and 0 <= v < nv[1] and 0 <= w < nv[2]:
                    m = (u * nv[1] + v) * nv[2] + w
                    solid = not (free[m] >= min_free and hit[m] == 0)
                    if cb is not None:
                        p = ((u // r) * (nv[1] // r) + v // r) * (nv[2] // r) + w // r
                        solid = solid and bool((cb.view(np.uint32)[p >> 5] >> np.uint32(p & 31)) & 1)
                    want[(x * nv[1] + y) * nv[2] + z] |= solid
        got = C.bits(segs, nv, min_free, dilate, cb, r)
        assert np.array_equal(got, C.pack_bits(want)), (min_free, dilate, cb is not None)


# ---- the definition against float64 geometry: a wall ----
def test_the_definition_carves_a_wall_scene():
    """Wall plane x = 1.5 m, 6 cameras within about 20 degrees of its normal with analytic float64 depth maps, a 48 x 64 image, lattice
    (16, 16, 8) at 0.25 m refined by 2.  (a) no fine voxel with x >= 1.5 - band is empty; (b) away from a decision boundary -- the band
    edge, the image border, z = 0 -- the empty set is the analytic one: in front of the wall, along the voxel's own ray, by more than
    the band in at least min_free views, and within the band in none; (c) at most 10 % of the voxels are left out as too close to a
    boundary.  Margins: the map holds the wall's depth along the PIXEL CENTRE's ray while (b) takes the voxel's own ray; half a pixel
    off, at up to 44 degrees from the normal and 5 m, the depth differs by at most 0.5 / 64 x 5 m x tan 44 < 0.04 m: 0.04 m on the band
    edges; 0.05 pixel on the border (the rounding boundary itself is exact: only the float32 projection's error, about 1e-5 pixel,
    moves it) and 0.05 m on z."""
    from oracle import nerfdet_oracle as O
    nv, vs, r, band, min_free = (16, 16, 8), (0.25, 0.25, 0.25), 2, 0.25, 2
    hw = (48, 64)
    origin = (0.05, 0.0, 0.0)          # no fine layer lies exactly at x = 1.5 - band
    pts = O.get_points([r * v for v in nv], [v / r for v in vs], origin)
    proj, depth, exts, kk = C.wall_scene(6, hw)
    for e in exts:
        assert np.degrees(np.arccos(e[2, 0])) < 20.0       # the viewing direction against the wall's normal
    words = C.accumulate(np.zeros(pts[0].numel(), dtype=np.int32), pts, proj, depth, band, hw)
    free, hit = C.unpack(words)
    empty = (free >= min_free) & (hit == 0)
    p = pts.reshape(3, -1).numpy().astype(np.float64)
    assert not empty[p[0] >= C.WALL_X - band].any()
    assert (p[0] >= C.WALL_X - band).sum() > 1000 and empty.sum() > 1000
    # float64 geometry
    a_free = np.zeros(p.shape[1], dtype=np.int64)
    a_hit = np.zeros(p.shape[1], dtype=np.int64)
    near = np.zeros(p.shape[1], dtype=bool)
    for e in exts:
        c = e[:, :3] @ p + e[:, 3:]
        z = c[2]
        eye = -e[:, :3].T @ e[:, 3]
        with np.errstate(all="ignore"):
            u, v = kk[0, 0] * c[0] / z + kk[0, 2], kk[1, 1] * c[1] / z + kk[1, 2]
            d = z * (C.WALL_X - eye[0]) / (p[0] - eye[0])        # the wall's camera depth along the voxel's own ray
        inside = (z > 0) & (u >= -0.5) & (u < hw[1] - 0.5) & (v >= -0.5) & (v < hw[0] - 0.5)
        a_free += inside & (z < d - band)
        a_hit += inside & (z > d - band) & (z < d + band)
        border = (np.abs(u + 0.5) < 0.05) | (np.abs(u - (hw[1] - 0.5)) < 0.05) | (np.abs(v + 0.5) < 0.05) | (np.abs(v - (hw[0] - 0.5)) < 0.05)
        almost = (z > -0.05) & (u > -1.5) & (u < hw[1] + 0.5) & (v > -1.5) & (v < hw[0] + 0.5)
        near |= almost & ((np.abs(z - (d - band)) < 0.04) | (np.abs(z - (d + band)) < 0.04) | border | (np.abs(z) < 0.05))
    a_empty = (a_free >= min_free) & (a_hit == 0)
    share = near.mean()
    print(f"wall: {empty.sum()} empty of {empty.size}, analytic {a_empty.sum()}, left out {share:.4f}, differ {(empty != a_empty)[~near].sum()}")
    assert share <= 0.10
    assert np.array_equal(empty[~near], a_empty[~near])
