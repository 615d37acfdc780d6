"""The point cloud of a streamed RGB-D scene without a GPU: the four entry points exist and refuse bad arguments on the host before any
HIP call (csrc/cloud_kernels.hip), the Python layer refuses bad knobs before it touches a tensor, rays.CloudStore follows a scene's
chunks and folds at its pixel budget, pipeline.write_ply writes what numpy reads back, and the DEFINITION itself (tests/cloud_ref.py)
puts the standard case's points where float64 geometry says they are."""
import ctypes

import numpy as np
import pytest
import torch

import cloud_ref as C

INVALID, UNSUPPORTED = -1, -2
FAKE = ctypes.c_void_p(0x1000)
ODD = ctypes.c_void_p(0x1001)


def _lib():
    from nerfdet_amd import _lib
    return _lib, _lib.load()


def _f3(*v):
    return (ctypes.c_float * 3)(*v)


def test_entry_points_exist():
    L, lib = _lib()
    for name in ("ndet_cloud_accumulate", "ndet_cloud_blocks", "ndet_cloud_count", "ndet_cloud_write", "ndet_label_points"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    from nerfdet_amd import ops, pipeline, rays, streaming
    for fn in (ops.cloud_accumulate, ops.cloud_points, ops.cloud_sums, pipeline.label_points, pipeline.write_ply):
        assert callable(fn)
    assert hasattr(rays, "CloudStore") and isinstance(ops.CLOUD_WAVE_MERGE, bool)
    for cls in (streaming.SceneStream, streaming.SceneGroup):
        assert hasattr(cls, "points") and hasattr(cls, "cloud_sums")
    assert lib.ndet_cloud_blocks(0) == 0 and lib.ndet_cloud_blocks(512) == 1 and lib.ndet_cloud_blocks(513) == 2


def test_cloud_accumulate_host_checks():
    _, lib = _lib()
    ok = dict(depth=FAKE, dtype=0, vp=24 * 40, rp=40, rgb=FAKE, cv=3 * 24 * 40, cp=24 * 40, cr=40, kn=FAKE, rot=FAKE, lpos=FAKE, k=3, H=24, W=40,
              p0=_f3(0, 0, 0), vs=_f3(0.1, 0.1, 0.1), nx=4, ny=4, nz=4, max_depth=0.0, merge=1, sums=FAKE)

    def call(**bad):
        a = dict(ok, **bad)
        return lib.ndet_cloud_accumulate(a["depth"], a["dtype"], a["vp"], a["rp"], a["rgb"], a["cv"], a["cp"], a["cr"], a["kn"], a["rot"], a["lpos"],
                                         a["k"], a["H"], a["W"], a["p0"], a["vs"], a["nx"], a["ny"], a["nz"], a["max_depth"], a["merge"], a["sums"],
                                         None)

    for key in ("depth", "rgb", "kn", "rot", "lpos", "p0", "vs", "sums"):
        assert call(**{key: None}) == INVALID and b"null" in lib.ndet_last_error(), key
    for key in ("nx", "ny", "nz", "k", "H", "W"):
        assert call(**{key: 0}) == INVALID and call(**{key: -2}) == INVALID, key
    assert call(dtype=2) == INVALID and b"dtype" in lib.ndet_last_error()
    assert call(rp=39) == INVALID and call(vp=24 * 40 - 1) == INVALID and b"depth pitches" in lib.ndet_last_error()
    for bad in (dict(cr=39), dict(cp=24 * 40 - 1), dict(cv=3 * 24 * 40 - 1)):
        assert call(**bad) == INVALID and b"colour pitches" in lib.ndet_last_error(), bad
    for vs in ((0.1, 0.0, 0.1), (0.1, 0.1, -1.0), (float("nan"), 0.1, 0.1), (0.1, float("inf"), 0.1)):
        assert call(vs=_f3(*vs)) == INVALID and b"voxel sizes" in lib.ndet_last_error(), vs
    assert call(p0=_f3(0, float("nan"), 0)) == INVALID
    assert call(max_depth=float("nan")) == INVALID and b"max_depth" in lib.ndet_last_error()
    assert call(nx=2048, ny=1024, nz=1024) == UNSUPPORTED and b"2^31" in lib.ndet_last_error()
    # k H W = 2^24 exactly is refused, one pixel fewer passes the host checks' size part (and is refused for its odd pointer instead)
    big = dict(k=16, H=1024, W=1024, vp=1024 * 1024, rp=1024, cv=3 * 1024 * 1024, cp=1024 * 1024, cr=1024)
    assert call(**big) == UNSUPPORTED and b"2^24" in lib.ndet_last_error()
    below = dict(k=1, H=4095, W=4097, vp=4095 * 4097, rp=4097, cv=3 * 4095 * 4097, cp=4095 * 4097, cr=4097)        # 2^24 - 1
    assert 4095 * 4097 == 2 ** 24 - 1
    assert call(sums=ODD, **below) == UNSUPPORTED and b"misaligned" in lib.ndet_last_error()
    for key in ("depth", "rgb", "kn", "rot", "lpos", "sums"):
        assert call(**{key: ODD}) == UNSUPPORTED and b"misaligned" in lib.ndet_last_error(), key
    assert call(depth=ctypes.c_void_p(0x1004), dtype=1) == UNSUPPORTED           # a float64 map: 8-byte aligned


def _segs(n, ptr=0x1000):
    return (ctypes.c_void_p * max(n, 1))(*([ptr] * n))


@pytest.mark.parametrize("which", ["count", "write"])
def test_cloud_emit_host_checks(which):
    _, lib = _lib()
    ok = dict(segs=_segs(2), n=2, nx=4, ny=4, nz=4, p0=_f3(0, 0, 0), vs=_f3(0.1, 0.1, 0.1), min_points=1, a=FAKE, xyz=FAKE, bgr=FAKE, count=FAKE,
              voxel=FAKE)

    def call(**bad):
        a = dict(ok, **bad)
        head = (a["segs"], a["n"], a["nx"], a["ny"], a["nz"], a["p0"], a["vs"], a["min_points"], a["a"])
        if which == "count":
            return lib.ndet_cloud_count(*head, None)
        return lib.ndet_cloud_write(*head, a["xyz"], a["bgr"], a["count"], a["voxel"], None)

    for key in ("segs", "p0", "vs", "a") + (("xyz", "bgr", "count", "voxel") if which == "write" else ()):
        assert call(**{key: None}) == INVALID and b"null" in lib.ndet_last_error(), key
    assert call(segs=_segs(2, 0)) == INVALID and b"null" in lib.ndet_last_error()
    for n in (0, -1, 65):
        assert call(segs=_segs(65), n=n) == INVALID and b"segments" in lib.ndet_last_error()
    for key in ("nx", "ny", "nz"):
        assert call(**{key: 0}) == INVALID and call(**{key: -2}) == INVALID
    for m in (0, -3):
        assert call(min_points=m) == INVALID and b"min_points" in lib.ndet_last_error()
    assert call(vs=_f3(0.1, float("nan"), 0.1)) == INVALID and b"voxel sizes" in lib.ndet_last_error()
    assert call(nx=2048, ny=1024, nz=1024) == UNSUPPORTED and b"2^31" in lib.ndet_last_error()
    odd = [dict(a=ODD), dict(segs=_segs(2, 0x1002))] + ([dict(xyz=ODD), dict(count=ODD), dict(voxel=ODD)] if which == "write" else [])
    for bad in odd:
        assert call(**bad) == UNSUPPORTED and b"misaligned" in lib.ndet_last_error(), bad


def test_label_points_host_checks():
    _, lib = _lib()
    call = lambda pts=FAKE, m=10, boxes=FAKE, n=3, labels=FAKE: lib.ndet_label_points(pts, m, boxes, n, labels, None)
    for bad in (dict(pts=None), dict(boxes=None), dict(labels=None)):
        assert call(**bad) == INVALID and b"null" in lib.ndet_last_error()
    for bad in (dict(m=0), dict(m=-1), dict(n=0), dict(n=-4)):
        assert call(**bad) == INVALID and b"positive" in lib.ndet_last_error()
    assert call(n=32768) == UNSUPPORTED and b"int16" in lib.ndet_last_error()
    assert call(m=2 ** 31) == UNSUPPORTED and b"2^31" in lib.ndet_last_error()
    for bad in (dict(pts=ODD), dict(boxes=ODD), dict(labels=ODD)):
        assert call(**bad) == UNSUPPORTED and b"misaligned" in lib.ndet_last_error()


def test_knobs_are_checked_before_any_launch():
    from nerfdet_amd import ops, pipeline, streaming
    assert streaming._cloud_knobs(None) is None and streaming._cloud_knobs(False) is None
    assert streaming._cloud_knobs(True) == (2, None) and streaming._cloud_knobs(dict(refine=4)) == (4, None)
    assert streaming._cloud_knobs(dict(refine=1, max_depth=3)) == (1, 3.0)
    for bad in (dict(refine=3), dict(refine=2.0), dict(refine=True), dict(max_depth=0.0), dict(max_depth=-1), dict(max_depth=float("nan")),
                dict(max_depth=float("inf")), dict(max_depth="x"), dict(max_depth=True), dict(rafine=2), 2, "yes"):
        with pytest.raises(ValueError):
            streaming._cloud_knobs(bad)
    for bad in (0, -1, 1.0, True, "2", 2 ** 31):
        with pytest.raises(ValueError, match="min_points"):
            streaming._check_min_points(bad)
    with pytest.raises(ValueError, match=r"begin_scene\(img_meta, cloud=True\)"):
        streaming._need_cloud(None, "points")
    # the wrappers: wrong shapes and dtypes are ValueErrors, CPU tensors RuntimeErrors, all before a launch
    nv, p0, vs = (2, 2, 2), (0.0, 0.0, 0.0), (0.5, 0.5, 0.5)
    sums = torch.zeros((8, 8), dtype=torch.int32)
    d, rgb = torch.ones((1, 4, 6)), torch.zeros((1, 3, 4, 6))
    kk, c2w = np.eye(3), np.eye(4)[None]
    for bad in (dict(sums=torch.zeros((8, 7), dtype=torch.int32)), dict(sums=sums.float()), dict(d=d.half()), dict(d=d[0]), dict(rgb=rgb[:, :2]),
                dict(rgb=rgb.double()), dict(kk=np.eye(2)), dict(c2w=np.eye(4)), dict(max_depth=0.0), dict(vs=(0.5, 0.0, 0.5)),
                dict(d=torch.ones((4, 2048, 2048)), rgb=torch.empty((4, 3, 2048, 2048), device="meta"))):
        a = dict(dict(sums=sums, d=d, rgb=rgb, kk=kk, c2w=c2w, max_depth=None, vs=vs), **bad)
        with pytest.raises(ValueError):
            ops.cloud_accumulate(a["sums"], nv, p0, a["vs"], a["d"], a["rgb"], a["kk"], a["c2w"], a["max_depth"])
    with pytest.raises(RuntimeError, match="GPU"):
        ops.cloud_accumulate(sums, nv, p0, vs, d, rgb, kk, c2w)
    for bad in (dict(segs=[]), dict(segs=[sums] * 65), dict(segs=[sums.view(-1)]), dict(min_points=0), dict(min_points=1.5)):
        a = dict(dict(segs=[sums], min_points=1), **bad)
        with pytest.raises(ValueError):
            ops.cloud_points(a["segs"], nv, p0, vs, a["min_points"])
    with pytest.raises(RuntimeError, match="GPU"):
        ops.cloud_points([sums], nv, p0, vs)
    got = ops.cloud_sums([sums, sums + 1], nv)                                    # torch arithmetic: runs anywhere
    assert set(got) == set(C.FIELDS) and got["n"].dtype == torch.int64 and tuple(got["r"].shape) == nv and int(got["g"].sum()) == 8
    assert int(ops.cloud_sums([torch.full((8, 8), -1, dtype=torch.int32)], nv)["n"][0, 0, 0]) == 2 ** 32 - 1      # the words are unsigned
    xyz = torch.zeros((5, 3))
    for bad in (dict(xyz=xyz.double()), dict(xyz=xyz[:, :2]), dict(xyz=xyz.T), dict(bf=np.zeros((2, 7), dtype=np.float32)),
                dict(bf=np.zeros((32768, 8), dtype=np.float32)), dict(bf=np.zeros((2, 8), dtype=np.int32))):
        a = dict(dict(xyz=xyz, bf=np.zeros((2, 8), dtype=np.float32)), **bad)
        with pytest.raises(ValueError):
            pipeline.label_points(a["xyz"], a["bf"])
    with pytest.raises(RuntimeError, match="GPU"):
        pipeline.label_points(xyz, np.zeros((2, 8), dtype=np.float32))


def test_cloud_store_life_cycle():
    from nerfdet_amd import ops, rays
    n = 6
    full = lambda v: torch.full((n, ops.CLOUD_WORDS), v, dtype=torch.int32)
    # windowed: a segment per chunk, spares reused, a pixel total per segment
    st = rays.CloudStore(n, "cpu", windowed=True, budget=100)
    a = st.target(40)
    assert tuple(a.shape) == (n, ops.CLOUD_WORDS) and a.dtype == torch.int32 and not a.any() and st.segments == []
    a += 1
    st.push(a, 40)
    b = st.target(0)
    assert b is not a
    st.push(b, 0)                                            # a chunk without depth: an empty segment
    assert st.pixels == [40, 0] and st.nbytes() == 2 * 32 * n and not st.segments[1].any()
    c = st.target(100)
    c += 3
    st.give_back(c)                                          # the chunk failed: zeroed, spare again
    assert not c.any() and st.pixels == [40, 0] and st.target(1) is c
    st.give_back(c)
    with pytest.raises(ValueError):
        st.give_back(a)
    with pytest.raises(ValueError, match="101 pixels"):
        st.target(101)
    st.drop_oldest(1)
    assert st.pixels == [0] and st.segments[0] is b and not a.any() and st.nbytes() == 3 * 32 * n
    with pytest.raises(ValueError):
        st.drop_oldest(2)
    st.clear()
    assert st.segments == [] and st.pixels == [] and st.nbytes() == 3 * 32 * n
    # unwindowed: chunks accumulate into the newest segment until the next one would pass the budget
    st = rays.CloudStore(n, "cpu", windowed=False, budget=100)
    a = st.target(60)
    st.push(a, 60)
    assert st.target(40) is a
    st.push(a, 40)
    assert st.pixels == [100] and len(st.segments) == 1
    b = st.target(1)                                         # 101 > 100: a further segment
    assert b is not a and len(st.segments) == 1
    st.push(b, 1)
    assert st.pixels == [100, 1] and st.target(0) is b
    with pytest.raises(ValueError):
        st.push(a, 1)                                        # only the newest segment takes chunks
    with pytest.raises(ValueError):
        st.push(full(0), 5)                                  # b still has room: a further segment is not what target() hands out
    # refused, whole, at 64 segments; the store is unchanged
    st = rays.CloudStore(n, "cpu", windowed=False, budget=10)
    for _ in range(64):
        t = st.target(10)
        st.push(t, 10)
    assert len(st.segments) == 64 and st.pixels == [10] * 64
    before = [s.clone() for s in st.segments]
    for call in (lambda: st.check(1), lambda: st.target(1)):
        with pytest.raises(ValueError, match="64 segments"):
            call()
    st.check(0)
    assert st.target(0) is st.segments[-1]                  # a chunk without depth still joins
    assert len(st.segments) == 64 and st.pixels == [10] * 64 and all(torch.equal(x, y) for x, y in zip(st.segments, before))
    st.clear()
    assert st.segments == [] and st.pixels == [] and st.target(10) is not None
    for bad in (dict(n=0), dict(budget=0), dict(budget=2 ** 24), dict(budget=True)):
        with pytest.raises(ValueError):
            rays.CloudStore(**dict(dict(n=4, device="cpu", windowed=False), **bad))
    assert rays.CloudStore(4, "cpu", False).budget == 2 ** 24 - 1


@pytest.mark.parametrize("with_labels", [False, True])
def test_write_ply_reads_back(tmp_path, with_labels):
    from nerfdet_amd import pipeline
    rng = np.random.RandomState(5)
    m = 37
    xyz = rng.randn(m, 3).astype(np.float32)
    bgr = rng.randint(0, 256, (m, 3)).astype(np.uint8)
    labels = rng.randint(-1, 4, m).astype(np.int16) if with_labels else None
    path = tmp_path / "cloud.ply"
    pipeline.write_ply(path, torch.from_numpy(xyz), bgr, None if labels is None else torch.from_numpy(labels))
    raw = path.read_bytes()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    header = raw[:end].decode("ascii").split("\n")[:-1]
    props = ["property float x", "property float y", "property float z", "property uchar red", "property uchar green", "property uchar blue"]
    assert header == ["ply", "format binary_little_endian 1.0", f"element vertex {m}"] + props + (["property short label"] if with_labels else []) \
        + ["end_header"]
    dt = [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")] + ([("label", "<i2")] if with_labels else [])
    rows = np.frombuffer(raw[end:], dtype=np.dtype(dt))
    assert rows.shape == (m,) and rows.dtype.itemsize == (17 if with_labels else 15)
    assert np.array_equal(np.stack([rows["x"], rows["y"], rows["z"]], 1), xyz)
    assert np.array_equal(np.stack([rows["blue"], rows["green"], rows["red"]], 1), bgr)          # B and R swapped
    if with_labels:
        assert np.array_equal(rows["label"], labels)
    for bad in (dict(xyz=xyz[:, :2]), dict(bgr=bgr.astype(np.int32)), dict(bgr=bgr[:-1]), dict(labels=np.zeros(m, dtype=np.int32))):
        a = dict(dict(xyz=xyz, bgr=bgr, labels=labels), **bad)
        with pytest.raises(ValueError):
            pipeline.write_ply(tmp_path / "bad.ply", a["xyz"], a["bgr"], a["labels"])
    pipeline.write_ply(tmp_path / "empty.ply", np.zeros((0, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.uint8))
    assert (tmp_path / "empty.ply").read_bytes().endswith(b"end_header\n")


# ---- the definition on the standard case, in float64 ----
@pytest.mark.parametrize("refine", [1, 2, 4])
def test_the_restatement_on_the_standard_case(refine):
    """Every contributing pixel's point projects back through the chunk's stride-1 ops.compute_projection to within 0.01 px of the
    centre of its own pixel -- (x + 0.5, y + 0.5): the rays are camera_rays', which look through pixel centres -- with z within 1e-5 d
    of d; every emitted point lies inside its voxel's cell; and the fixture holds what the GPU tests rely on."""
    from nerfdet_amd import ops
    case = C.standard_case(np.float64)
    nv, p0, vs = C.lattice(C.NV, C.VS, C.ORIGIN, refine)
    assert nv == tuple(refine * v for v in C.NV)
    assert ops.carve_lattice(C.NV, C.VS, refine) == (nv, tuple(float(v) for v in vs))
    ok, pts, d = C.pixel_points(case["depth"], case["krows"], case["c2w"])
    depth = case["depth"]
    assert (depth == 0).any() and np.isnan(depth).any() and np.isinf(depth).any() and (depth < 0).any()
    assert not ok[np.isnan(depth) | np.isinf(depth) | (depth <= 0)].any() and ok[np.isfinite(depth) & (depth > 0)].all()
    proj = ops.compute_projection(C.meta_of(case), 1).numpy().astype(np.float64)              # (k, 3, 4)
    vv, uu = np.mgrid[0:C.HW[0], 0:C.HW[1]]
    for v in range(depth.shape[0]):
        p = pts[v][ok[v]].astype(np.float64)
        uvz = np.concatenate([p, np.ones((len(p), 1))], 1) @ proj[v].T
        dd = d[v][ok[v]].astype(np.float64)
        assert np.abs(uvz[:, 0] / uvz[:, 2] - (uu[ok[v]] + 0.5)).max() <= 0.01 and np.abs(uvz[:, 1] / uvz[:, 2] - (vv[ok[v]] + 0.5)).max() <= 0.01
        assert (np.abs(uvz[:, 2] - dd) <= 1e-5 * dd).all()
    inside, flat, q = C.voxel_of(pts, nv, p0, vs)
    use = ok & inside
    assert (ok & ~inside).any(), "no point leaves the lattice"
    assert use.mean() >= 0.30, f"only {use.mean():.3f} of the pixels contribute"
    assert q[use].min() >= 0 and q[use].max() <= 255
    sums = C.accumulate(C.zero_sums(nv), nv, p0, vs, depth, case["rgb"], case["krows"], case["c2w"])
    assert sums[:, 0].sum() == use.sum()
    out = C.emit(sums, nv, p0, vs)
    m = len(out["voxel"])
    assert m >= 20 and (np.diff(out["voxel"]) > 0).all() and out["count"].sum() == use.sum()
    vox = out["voxel"].astype(np.int64)
    idx = np.stack([vox // (nv[1] * nv[2]), (vox // nv[2]) % nv[1], vox % nv[2]], 1).astype(np.float64)
    centre = p0.astype(np.float64) + vs.astype(np.float64) * idx
    half = 0.5 * vs.astype(np.float64)
    # the offsets stop at (255.5 / 256 - 0.5) vs = 0.498 vs from the centre: 0.002 vs, far more than a float32 rounding, inside the cell
    assert (np.abs(out["xyz"].astype(np.float64) - centre) < half).all(), "an emitted point lies outside its voxel's cell"
    # the emitted mean is the mean of the pixels' points to within the quantisation: half a step of vs / 256, and float32 rounding
    sx = np.zeros((sums.shape[0], 3))
    np.add.at(sx, flat[use], pts[use].astype(np.float64))
    mean = sx[vox] / out["count"][:, None]
    assert np.abs(out["xyz"] - mean).max() <= vs.max() / 256 * 0.5 + 1e-5
    # min_points cuts, an impossible one empties
    three = C.emit(sums, nv, p0, vs, 3)
    assert 0 < len(three["voxel"]) < m or refine == 4
    assert len(C.emit(sums, nv, p0, vs, 10 ** 6)["voxel"]) == 0
    # a max_depth that cuts the floor
    cut = C.accumulate(C.zero_sums(nv), nv, p0, vs, depth, case["rgb"], case["krows"], case["c2w"], max_depth=2.0)
    assert 0 < cut[:, 0].sum() < sums[:, 0].sum()


def test_the_merge_fixtures_hold_their_corners():
    nv1, p01, vs1 = C.lattice(C.NV, C.VS, C.ORIGIN, 1)
    nv4, p04, vs4 = C.lattice(C.NV, C.VS, C.ORIGIN, 4)
    keys, most = C.keys_per_wave(C.wall_case(0.1, (8, 64)), nv1, p01, vs1)
    assert keys == [1] * 8 and most == 512                  # whole waves share one voxel, which takes far more than 64 pixels of 8 waves
    keys, most = C.keys_per_wave(C.oblique_case(), nv4, p04, vs4)
    assert min(keys) > 48 and most <= 3                     # most lanes of a wave hold a voxel of their own
    keys, _ = C.keys_per_wave(C.wall_case(0.0, (16, 16), grazing=True), nv4, p04, vs4)
    assert min(keys) >= 16
    keys, _ = C.keys_per_wave(C.standard_case(), *C.lattice(C.NV, C.VS, C.ORIGIN, 2))
    # 24 x 40: waves straddle rows, but a view is 15 whole waves; the 23 x 40 variant of the GPU tests (C.ODD_HW) also straddles views and
    # ends in a partial wave
    assert len(keys) == 45 and 40 % 64 != 0 and 24 * 40 % 64 == 0
    assert C.ODD_HW[0] * C.ODD_HW[1] % 64 != 0 and 3 * C.ODD_HW[0] * C.ODD_HW[1] % 64 != 0


def test_colour_bytes_and_labels():
    x = np.array([-0.1, 0.0, 0.5 / 255, 0.49 / 255, 1.0, 1.5, np.nan, 254.5 / 255, np.inf], dtype=np.float32)
    assert C.colour_bytes(x).tolist() == [0, 0, 1, 0, 255, 255, 0, 255, 255]
    from nerfdet_amd.boxes import box_frames
    bf = box_frames(C.boxes7())
    pts = np.array([[0.625, -0.28, 0.0], [0.85, -0.1, 0.0], [2.5, 2.5, 0.2], [9.0, 9.0, 9.0], [np.nan, 0.0, 0.0]], dtype=np.float32)
    assert C.label_points(pts, bf).tolist() == [1, 2, 0, -1, -1]               # the overlap goes to the higher index
    assert C.label_points(pts, np.zeros((0, 8), dtype=np.float32)).tolist() == [-1] * 5
