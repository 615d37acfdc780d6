"""GPU checks of the point cloud of a streamed RGB-D scene (csrc/cloud_kernels.hip, ops.cloud_accumulate / cloud_points / cloud_sums,
pipeline.label_points, rays.CloudStore, ``begin_scene(cloud=)``, ``scene.points()``): sums, points and labels against the numpy
restatement (tests/cloud_ref.py) bit for bit, the merged and the unmerged kernel against each other, and the store following streams,
windows and groups."""
import numpy as np
import pytest
import torch

import cloud_ref as C

pytestmark = pytest.mark.gpu

_CACHE = {}
POINT_KEYS = ("xyz", "bgr", "count", "voxel")


def _lattice(refine):
    key = ("lattice", refine)
    if key not in _CACHE:
        _CACHE[key] = C.lattice(C.NV, C.VS, C.ORIGIN, refine)
    return _CACHE[key]


def _want(name, case, refine, max_depth=None):
    """The restated sums of one chunk over zeroed records; made once per case."""
    key = ("want", name, refine, max_depth)
    if key not in _CACHE:
        nv, p0, vs = _lattice(refine)
        _CACHE[key] = C.accumulate(C.zero_sums(nv), nv, p0, vs, case["depth"], case["rgb"], case["krows"], case["c2w"], max_depth)
    return _CACHE[key]


def _zeros(nv, device):
    from nerfdet_amd import ops
    return torch.zeros((nv[0] * nv[1] * nv[2], ops.CLOUD_WORDS), dtype=torch.int32, device=device)


def _run(case, refine, device, depth=None, rgb=None, max_depth=None, merge=None, sums=None, views=slice(None)):
    from nerfdet_amd import ops
    nv, p0, vs = _lattice(refine)
    sums = _zeros(nv, device) if sums is None else sums
    depth = C.to_torch(case["depth"], device) if depth is None else depth
    rgb = C.to_torch(case["rgb"], device) if rgb is None else rgb
    out = ops.cloud_accumulate(sums, nv, p0, vs, depth[views], rgb[views], case["intrinsic"], case["c2w"][views], max_depth, merge=merge)
    assert out is sums
    return sums


def _stacked(sums, refine):
    from nerfdet_amd import ops
    return C.stack_sums(ops.cloud_sums([sums], _lattice(refine)[0]))


def _same_points(a, b):
    return all(a[key].dtype == b[key].dtype and a[key].shape == b[key].shape and torch.equal(a[key], b[key]) for key in POINT_KEYS)


def _points_equal_ref(got, want, what):
    for key in POINT_KEYS:
        g = got[key].cpu().numpy()
        assert g.dtype == want[key].dtype and g.shape == want[key].shape, f"{what}: {key} {g.shape} {g.dtype} vs {want[key].shape} {want[key].dtype}"
        assert np.array_equal(g.view(np.uint8), want[key].view(np.uint8)), f"{what}: {key} differs"


# ---- 1. sums against the restatement ----
@pytest.mark.parametrize("hw", [C.HW, C.ODD_HW])
@pytest.mark.parametrize("refine", [1, 2, 4])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_sums_equal_the_restatement(device, dtype, refine, hw):
    """The standard case -- holes, a NaN, an Inf, a negative depth, points that leave the lattice, colours below 0, above 1 and NaN -- as
    a contiguous and a pitched map, contiguous and pitched colour planes (the crop of a padded tensor), with and without a max_depth that
    cuts the floor, merged and unmerged; 23 x 40 frames also straddle views and end in a partial wave."""
    from nerfdet_amd import ops
    name = ("standard", np.dtype(dtype).name, hw)
    if ("case",) + name not in _CACHE:
        _CACHE[("case",) + name] = C.standard_case(dtype, hw=hw)
    case = _CACHE[("case",) + name]
    k, (h, w) = 3, hw
    d = C.to_torch(case["depth"], device)
    pitched = torch.full((k, h + 3, w + 5), 1.5, dtype=d.dtype, device=device)
    pitched[:, :h, :w] = d
    pitched = pitched[:, :h, :w]
    padded = torch.full((k, 3, 32, 48), 0.25, dtype=torch.float32, device=device)
    padded[:, :, :h, :w] = C.to_torch(case["rgb"], device)
    crop = padded[:, :, :h, :w]
    assert not pitched.is_contiguous() and not crop.is_contiguous()
    for max_depth in (None, 2.0):
        want = _want(name, case, refine, max_depth)
        for depth, rgb, merge in ((d, None, True), (d, None, False), (pitched, crop, True), (pitched, crop, False), (d, crop, None)):
            got = _stacked(_run(case, refine, device, depth=depth, rgb=rgb, max_depth=max_depth, merge=merge), refine)
            assert np.array_equal(got, want), f"{name} r{refine} max_depth {max_depth} merge {merge} pitched {depth is pitched}"
    full, cut = _want(name, case, refine, None), _want(name, case, refine, 2.0)
    assert 0 < cut[:, 0].sum() < full[:, 0].sum()
    print(f"{name} r{refine}: {int(full[:, 0].sum())} of {k * h * w} pixels in {int((full[:, 0] > 0).sum())} voxels, most in one {int(full[:, 0].max())}")
    # a second chunk adds to the first: the spare word stays 0
    sums = _run(case, refine, device)
    _run(case, refine, device, sums=sums)
    assert np.array_equal(_stacked(sums, refine), 2 * full) and not sums[:, 7].any()
    assert isinstance(ops.CLOUD_WAVE_MERGE, bool)


# ---- 2. the merge's corners ----
CORNERS = {   # name -> (case, refine)
    "near_wall_r1": (lambda: C.wall_case(0.1, (8, 64)), 1),            # whole waves share one voxel; one voxel takes 512 pixels of 8 waves; W = 64
    "near_wall_r4": (lambda: C.wall_case(0.1, (8, 64), k=2), 4),
    "grazing_r4": (lambda: C.wall_case(0.0, (16, 16), grazing=True), 4),
    "oblique_r4": (lambda: C.oblique_case(), 4),                       # most lanes of a wave hold a voxel of their own
}


@pytest.mark.parametrize("name", list(CORNERS))
def test_the_merge_corners(device, name):
    make, refine = CORNERS[name]
    case = make()
    want = _want(name, case, refine)
    assert want[:, 0].sum() > 0
    for merge in (True, False):
        assert np.array_equal(_stacked(_run(case, refine, device, merge=merge), refine), want), f"{name} merge {merge}"
    keys, most = C.keys_per_wave(case, *_lattice(refine))
    print(f"{name}: {min(keys)} .. {max(keys)} voxels a wave, {most} pixels in one voxel")


@pytest.mark.parametrize("merge", [True, False])
def test_a_frame_of_holes_adds_nothing(device, merge):
    case = dict(C.standard_case(np.float32))
    case["depth"] = np.zeros_like(case["depth"])
    case["depth"][1] = np.nan
    case["depth"][2] = -1.0
    assert not _run(case, 2, device, merge=merge).any()
    start = torch.arange(16 * 16 * 8 * 8, dtype=torch.int32, device=device).view(-1, 8).contiguous()
    assert torch.equal(_run(case, 2, device, merge=merge, sums=start.clone()), start)


# ---- 3. chunk invariance ----
def test_any_chunking_leaves_the_same_bytes(device):
    from nerfdet_amd import ops
    case = C.standard_case(np.float64, k=6)
    nv, p0, vs = _lattice(2)
    want = _want("six", case, 2)
    got = {}
    for merge in (True, False):
        for sizes in ([6], [2, 2, 2], [1] * 6):
            sums, v = _zeros(nv, device), 0
            for s in sizes:
                _run(case, 2, device, merge=merge, sums=sums, views=slice(v, v + s))
                v += s
            got[(merge, len(sizes))] = (sums, ops.cloud_points([sums], nv, p0, vs, 1))
    first = got[(True, 1)]
    assert np.array_equal(_stacked(first[0], 2), want)
    for key, (sums, pts) in got.items():
        assert torch.equal(sums, first[0]) and _same_points(pts, first[1]), key
    # ... and as six segments of one view each
    segs = [_run(case, 2, device, views=slice(v, v + 1)) for v in range(6)]
    assert _same_points(ops.cloud_points(segs, nv, p0, vs, 1), first[1])


# ---- 4. emit ----
def _record_segments(n, n_segs, seed):
    """``n_segs`` record segments (n, 8) int32 with per voxel a total count from {0, 0, 1, 2, 3, 7, 300} dealt over the segments at random,
    offsets and colours within 255 per contribution; voxel 1 holds 2^31 pixels in every segment (the count saturates, sums pass 2^32),
    voxel 2 a segment budget's worth (2^24 - 1 pixels of 255)."""
    rng = np.random.RandomState(seed)
    tot = rng.choice([0, 0, 1, 2, 3, 7, 300], n)
    rec = np.zeros((n_segs, n, 8), dtype=np.int64)
    for _ in range(int(tot.max())):
        live = np.nonzero(tot > 0)[0]
        seg = rng.randint(0, n_segs, len(live))
        rec[seg, live, 0] += 1
        rec[seg, live, 1:7] += rng.randint(0, 256, (len(live), 6))
        tot[live] -= 1
    if n > 2:
        rec[:, 1] = [2 ** 31, 2 ** 32 - 1, 0, 2 ** 31, 2 ** 32 - 1, 5, 2 ** 31 + 1, 0]
        rec[:, 2] = [2 ** 24 - 1] + [255 * (2 ** 24 - 1)] * 6 + [0]
    return [r.astype(np.uint32).view(np.int32) for r in rec], rec.sum(0)[:, :7]


@pytest.mark.parametrize("nv", [(5, 3, 7), (32, 32, 16), (7, 9, 41)])
def test_points_equal_the_restatement(device, nv):
    """105 voxels (a partial wave), 16384 (eight workgroups), 2583 (a partial workgroup and a partial 512-voxel block); 1, 2 and 64
    segments; min_points 1 and 3; ascending voxels; two calls give the same bytes."""
    from nerfdet_amd import ops
    n = nv[0] * nv[1] * nv[2]
    p0, vs = np.float32([-0.4, 1.3, 0.05]), np.float32([0.1, 0.07, 0.3])
    for n_segs in (1, 2, 64):
        segs, total = _record_segments(n, n_segs, seed=n_segs)
        dev = [C.to_torch(s, device) for s in segs]
        assert np.array_equal(C.stack_sums(ops.cloud_sums(dev, nv)), total)
        for min_points in (1, 3):
            want = C.emit(total, nv, p0, vs, min_points)
            got = ops.cloud_points(dev, nv, p0, vs, min_points)
            _points_equal_ref(got, want, f"{nv} segs {n_segs} min_points {min_points}")
            assert _same_points(ops.cloud_points(dev, nv, p0, vs, min_points), got), "a second call gives other bytes"
            v = got["voxel"].cpu().numpy()
            assert len(v) > 0 and (np.diff(v) > 0).all()
        if n_segs > 1:
            assert int(got["count"].max()) == 2 ** 31 - 1
    # nothing to emit: M = 0 tensors of the right shapes and no write launch
    few = torch.full((n, 8), 2, dtype=torch.int32, device=device)            # two pixels in every voxel of every segment
    for segs, min_points in (([torch.zeros((n, 8), dtype=torch.int32, device=device)], 1), ([few], 3), ([few] * 3, 7), ([few], 2 ** 31 - 1)):
        got = ops.cloud_points(segs, nv, p0, vs, min_points)
        assert [tuple(got[key].shape) for key in POINT_KEYS] == [(0, 3), (0, 3), (0,), (0,)]
        assert [got[key].dtype for key in POINT_KEYS] == [torch.float32, torch.uint8, torch.int32, torch.int32]


def test_points_of_the_standard_case(device):
    from nerfdet_amd import ops
    case = C.standard_case(np.float64)
    for refine in (1, 2, 4):
        nv, p0, vs = _lattice(refine)
        sums = _run(case, refine, device)
        for min_points in (1, 3):
            _points_equal_ref(ops.cloud_points([sums], nv, p0, vs, min_points), C.emit(_want("std64", case, refine), nv, p0, vs, min_points),
                              f"r{refine} min_points {min_points}")


# ---- 5. labels ----
def test_labels_equal_the_restatement(device):
    from nerfdet_amd import ops, pipeline
    from nerfdet_amd.boxes import box_frames
    case = C.standard_case(np.float64)
    nv, p0, vs = _lattice(4)
    pts = ops.cloud_points([_run(case, 4, device)], nv, p0, vs, 1)
    bf = box_frames(C.boxes7())
    got = pipeline.label_points(pts["xyz"], bf)
    want = C.label_points(pts["xyz"].cpu().numpy(), bf)
    assert got.dtype == torch.int16 and tuple(got.shape) == (pts["xyz"].shape[0],) and np.array_equal(got.cpu().numpy(), want)
    assert (want == 1).any() and (want == 2).any() and (want == -1).any() and not (want == 0).any()
    print("labels: " + ", ".join(f"{int(v)}: {int(c)}" for v, c in zip(*np.unique(want, return_counts=True))))
    none = pipeline.label_points(pts["xyz"], np.zeros((0, 8), dtype=np.float32))            # no box at all
    assert none.dtype == torch.int16 and bool((none == -1).all()) and none.shape == got.shape
    assert tuple(pipeline.label_points(pts["xyz"][:0], bf).shape) == (0,)
    # more boxes than one LDS batch holds, the highest index wins
    many = np.concatenate([bf[1:2]] * 300 + [bf[2:3]], 0)
    got = pipeline.label_points(pts["xyz"], many).cpu().numpy()
    assert np.array_equal(got, np.where(want == 2, 300, np.where(want == 1, 299, -1)))


def test_labels_of_a_frames_points_are_label_frames(device):
    """ray_o + d ray_d of pipeline.camera_rays for a millimetre-exact depth frame: label_points returns label_frames' labels."""
    from nerfdet_amd import pipeline
    from nerfdet_amd.boxes import box_frames
    case = C.standard_case(np.float64)
    mm = np.clip(np.rint(np.nan_to_num(case["depth"], nan=0.0, posinf=0.0) * 1000.0), 0, 65535).astype(np.uint16)
    k, h, w = mm.shape
    bf = box_frames(C.boxes7())
    window = (0, 0, h, w)
    frames = pipeline.label_frames(C.to_torch(mm, device), case["intrinsic"], case["c2w"], bf, window)
    ray_o, ray_d = pipeline.camera_rays(case["intrinsic"], case["c2w"], window, device=device)
    d = (C.to_torch(mm, device).to(torch.float32) / 1000.0).view(k, h * w, 1)
    pts = torch.addcmul(ray_o, d, ray_d).view(-1, 3).contiguous()
    got = pipeline.label_points(pts, bf).view(k, h, w)
    got = torch.where(C.to_torch(mm, device) != 0, got, torch.full_like(got, -1))           # a hole is no point
    assert torch.equal(got, frames) and int((frames >= 0).sum()) > 50


# ---- 6. scenes ----
def _raw(device):
    """The raw scene of tests/test_raw_frames_gpu.py on the small detector, with millimetre depth frames of the floor z = 0 (5 % holes);
    made once."""
    key = ("raw", str(device))
    if key not in _CACHE:
        from depth_gate_ref import plane_depth
        from test_detector_gpu import _small_detector
        from test_raw_frames_gpu import _raw_scene
        frames, meta, _, _ = _raw_scene(device, 21)
        metres = plane_depth(meta, (60, 80), 0.0, noise=0.01, seed=3, missing=0.05).numpy()
        mm = np.clip(np.rint(metres * 1000.0), 0, 65535).astype(np.uint16)
        _CACHE[key] = dict(det=_small_detector(device), frames=frames, meta=meta, mm=C.to_torch(mm, device).unsqueeze(0))
    return _CACHE[key]


def _scene_want(c, v0, v1, refine, max_depth=None, sums=None):
    """The restated sums of the raw scene's views v0 .. v1 over the chunk's own depth_r and rgb, remade with the public pieces."""
    from nerfdet_amd import ops, pipeline
    from test_raw_frames_gpu import PAD, SCALE
    det, meta = c["det"], c["meta"]
    hh, ww = meta["img_shape"][:2]
    _, denorm = pipeline.prepare_frames(c["frames"][0, v0:v1], SCALE, PAD)
    depth = pipeline.prepare_depth_frames(c["mm"][0, v0:v1].contiguous(), (hh, ww))
    gate = ops.depth_gate(depth, det.voxel_size, (hh // 4, ww // 4), (hh, ww))
    kk = np.array(meta["lidar2img"]["intrinsic"], dtype=np.float32)
    kk[:2] = kk[:2] / (meta["ori_shape"][0] / meta["img_shape"][0])
    nv, p0, vs = C.lattice([int(v) for v in det.n_voxels], [float(v) for v in det.voxel_size], meta["lidar2img"]["origin"], refine)
    sums = C.zero_sums(nv) if sums is None else sums
    return C.accumulate(sums, nv, p0, vs, gate.depth_r.cpu().numpy(), denorm[:, :, :hh, :ww].cpu().numpy(), C.krows_of(kk),
                        C.c2w_of_extrinsics(meta["lidar2img"]["extrinsic"][v0:v1]), max_depth), (nv, p0, vs)


def test_scene_points_equal_the_restatement(device):
    from nerfdet_amd.boxes import box_frames, drawing_order
    from test_streaming_gpu import _chunk_meta
    c = _raw(device)
    det, meta = c["det"], c["meta"]
    scene = det.begin_scene(dict(meta), cloud=True)
    assert scene.cloud.refine == 2 and scene.cloud.max_depth is None and scene.cloud.store.segments == []
    empty = scene.points()
    assert [tuple(empty[key].shape) for key in POINT_KEYS] == [(0, 3), (0, 3), (0,), (0,)] and not any(v.any() for v in scene.cloud_sums().values())
    scene.add_frames(c["frames"][:, 0:4], _chunk_meta(meta, 0, 4), depth_frames=c["mm"][:, 0:4].contiguous())
    want, (nv, p0, vs) = _scene_want(c, 0, 4, 2)
    assert scene.cloud.n_voxels == nv and np.array_equal(np.float32(scene.cloud.p0), p0) and np.array_equal(np.float32(scene.cloud.vs), vs)
    assert np.array_equal(C.stack_sums(scene.cloud_sums()), want) and len(scene.cloud.store.segments) == 1
    assert scene.cloud.store.pixels == [4 * 63 * 96]
    pts = scene.points()
    _points_equal_ref(pts, C.emit(want, nv, p0, vs, 1), "scene.points()")
    _points_equal_ref(scene.points(min_points=3), C.emit(want, nv, p0, vs, 3), "scene.points(min_points=3)")
    m = pts["xyz"].shape[0]
    print(f"scene: {int(want[:, 0].sum())} of {4 * 63 * 96} pixels in {m} of {want.shape[0]} fine voxels")
    assert m > 100
    # a second chunk accumulates into the same segment; max_depth cuts
    scene.add_frames(c["frames"][:, 4:6], _chunk_meta(meta, 4, 6), depth_frames=c["mm"][:, 4:6].contiguous())
    both, _ = _scene_want(c, 4, 6, 2, sums=want)
    assert np.array_equal(C.stack_sums(scene.cloud_sums()), both) and scene.cloud.store.pixels == [6 * 63 * 96]
    near = det.begin_scene(dict(meta), cloud=dict(refine=1, max_depth=2.5))
    near.add_frames(c["frames"][:, 0:4], _chunk_meta(meta, 0, 4), depth_frames=c["mm"][:, 0:4].contiguous())
    cut, (nv1, _, _) = _scene_want(c, 0, 4, 1, max_depth=2.5)
    assert near.cloud.n_voxels == nv1 and np.array_equal(C.stack_sums(near.cloud_sums()), cut) and 0 < cut[:, 0].sum() < want[:, 0].sum()
    # labels: a detect() result, and one made by hand around the floor so that points are held; ids index kept
    result = scene.detect()[0]
    by_hand = dict(boxes_3d=torch.tensor([[0.0, 0.0, -0.5, 2.0, 2.0, 1.0, 0.3], [0.5, 0.5, -0.2, 1.5, 1.0, 0.5, 0.0], [9.0, 9.0, 0.0, 1.0, 1.0, 1.0, 0.0],
                                          [-1.0, 0.5, -0.3, 1.0, 3.0, 0.6, 1.0]]), scores_3d=torch.tensor([0.9, 0.4, 0.95, 0.2]),
                   labels_3d=torch.tensor([1, 0, 2, 1]))
    pts = scene.points()
    for res, thr in ((result, 0.0), (result, float(result["scores_3d"].median())), (by_hand, 0.0), (by_hand, 0.3), (by_hand, 2.0)):
        got = scene.points(result=res, score_thr=thr)
        assert _same_points(got, pts)
        boxes = getattr(res["boxes_3d"], "tensor", res["boxes_3d"]).cpu().numpy()
        kept = drawing_order(res["scores_3d"], thr)
        assert got["kept"].dtype == torch.int64 and np.array_equal(got["kept"].numpy(), kept)
        want_ids = C.label_points(pts["xyz"].cpu().numpy(), box_frames(boxes[kept])) if len(kept) else np.full(pts["xyz"].shape[0], -1, dtype=np.int16)
        assert got["ids"].dtype == torch.int16 and np.array_equal(got["ids"].cpu().numpy(), want_ids)
        if res is by_hand and thr == 0.0:
            assert kept.tolist() == [3, 1, 0, 2] and (want_ids == 2).any() and (want_ids == 1).any() and not (want_ids == 3).any()
    with pytest.raises(ValueError, match="min_points"):
        scene.points(min_points=0)
    with pytest.raises(ValueError):
        scene.points(result=dict(boxes_3d=by_hand["boxes_3d"]))
    plain = det.begin_scene(dict(meta))
    for call in (plain.points, plain.cloud_sums):
        with pytest.raises(ValueError, match=r"begin_scene\(img_meta, cloud=True\)"):
            call()
    for bad in (dict(refine=3), dict(max_depth=0.0), 5):
        with pytest.raises(ValueError):
            det.begin_scene(dict(meta), cloud=bad)
        with pytest.raises(ValueError):
            det.begin_scenes([dict(meta)], cloud=bad)


def test_a_chunk_past_the_pixel_limit_is_refused_before_any_device_work(device):
    """A cloud scene refuses a chunk of 2^24 pixels or more, and an unwindowed store folds into a further segment at its budget."""
    from test_streaming_gpu import _chunk_meta
    c = _raw(device)
    det, meta = c["det"], c["meta"]
    scene = det.begin_scene(dict(meta), cloud=True)
    scene.cloud.store.budget = 5 * 63 * 96
    feed = lambda v0, v1: scene.add_frames(c["frames"][:, v0:v1], _chunk_meta(meta, v0, v1), depth_frames=c["mm"][:, v0:v1].contiguous())
    with pytest.raises(ValueError, match="pixels"):
        feed(0, 6)
    assert scene.n_views == 0 and scene.cloud.store.segments == []
    feed(0, 3)
    feed(3, 5)
    feed(5, 6)                                               # 6 views pass the budget of 5: a further segment
    assert scene.cloud.store.pixels == [5 * 63 * 96, 63 * 96] and len(scene.cloud.store.segments) == 2 and scene.n_views == 6
    whole = det.begin_scene(dict(meta), cloud=True)
    whole.add_frames(c["frames"], meta, depth_frames=c["mm"])
    assert _same_points(scene.points(), whole.points())
    for key, v in scene.cloud_sums().items():
        assert torch.equal(v, whole.cloud_sums()[key]), key


# ---- 7. windows ----
def _carved(device):
    from test_carve_gpu import _carved as carved
    return carved(device)


def _feed(scene, c, splits, depth=True):
    from test_carve_gpu import _feed as feed
    return feed(scene, c, splits, depth)


def _same_sums(a, b):
    return all(torch.equal(a[key], b[key]) for key in C.FIELDS)


def test_a_window_follows_the_chunks(device):
    """S + 2 chunks through a window of S = 2 leave what a fresh stream fed the last S holds; drop_oldest and reset leave no trace; a chunk
    without depth adds an empty segment that drops with its state; a refused call changes nothing."""
    from test_stream_render_gpu import _chunk_meta
    c = _carved(device)
    det = c["det"]
    begin = lambda: det.begin_scene(dict(c["meta"]), window=2, cloud=dict(refine=2))
    scene = _feed(begin(), c, [(0, 2), (2, 3), (3, 5), (5, 6)])
    fresh = _feed(begin(), c, [(3, 5), (5, 6)])
    assert len(scene.cloud.store.segments) == 2 == scene.n_chunks and scene.cloud.store.pixels == [2 * 64 * 96, 64 * 96]
    assert _same_sums(scene.cloud_sums(), fresh.cloud_sums()) and int(scene.cloud_sums()["n"].sum()) > 0
    assert _same_points(scene.points(), fresh.points()) and scene.points()["xyz"].shape[0] > 0
    owned = scene.cloud.store.nbytes()
    sums = scene.cloud_sums()
    with pytest.raises(ValueError):
        scene.add_views(c["img"][:, 0:2], c["dn"][:, 0:2], _chunk_meta(c["meta"], 0, 3), depth=c["depth"][:, 0:2])     # 3 extrinsics for 2 views
    assert _same_sums(scene.cloud_sums(), sums) and len(scene.cloud.store.segments) == 2 and scene.cloud.store.nbytes() == owned
    scene.drop_oldest(1)
    only = _feed(begin(), c, [(5, 6)])
    assert _same_sums(scene.cloud_sums(), only.cloud_sums()) and _same_points(scene.points(), only.points())
    _feed(scene, c, [(0, 2)], depth=False)                                      # no depth: an empty segment
    assert len(scene.cloud.store.segments) == 2 and not scene.cloud.store.segments[-1].any() and scene.cloud.store.pixels == [64 * 96, 0]
    assert _same_sums(scene.cloud_sums(), only.cloud_sums())
    _feed(scene, c, [(2, 3)])                                                   # evicts (5, 6)
    assert scene.cloud.store.nbytes() == owned                                 # a window that has slid allocates nothing
    _feed(scene, c, [(3, 5)])                                                   # evicts the empty segment with its state
    two = _feed(begin(), c, [(2, 3), (3, 5)])
    assert _same_sums(scene.cloud_sums(), two.cloud_sums()) and scene.cloud.store.pixels == [64 * 96, 2 * 64 * 96]
    scene.reset()
    assert scene.cloud.store.segments == [] and not any(v.any() for v in scene.cloud_sums().values())
    _feed(scene, c, [(3, 5), (5, 6)])
    assert _same_sums(scene.cloud_sums(), fresh.cloud_sums())
    # an unwindowed scene: one segment for all chunks, any chunking, and reset leaves no trace
    plain = _feed(det.begin_scene(dict(c["meta"]), cloud=True), c, [(0, 3)])
    plain.reset()
    _feed(plain, c, [(3, 5), (5, 6)])
    assert len(plain.cloud.store.segments) == 1 and _same_sums(plain.cloud_sums(), fresh.cloud_sums())
    assert _same_points(plain.points(), fresh.points())


# ---- 8. groups ----
@pytest.mark.parametrize("window", [None, 2])
def test_a_group_of_one_scene_is_the_stream(device, window):
    from test_stream_render_gpu import _chunk_meta
    c = _carved(device)
    det = c["det"]
    splits = [(0, 2), (2, 3), (3, 5), (5, 6)]
    scene = _feed(det.begin_scene(dict(c["meta"]), window=window, cloud=True), c, splits)
    group = det.begin_scenes([dict(c["meta"])], window=window, cloud=True)
    for v0, v1 in splits:
        group.add_views(c["img"][:, v0:v1], c["dn"][:, v0:v1], [_chunk_meta(c["meta"], v0, v1)], depth=c["depth"][:, v0:v1])
    assert _same_sums(group.cloud_sums()[0], scene.cloud_sums()) and int(scene.cloud_sums()["n"].sum()) > 0
    assert len(group.clouds[0].store.segments) == len(scene.cloud.store.segments) and group.clouds[0].store.pixels == scene.cloud.store.pixels
    for a, b in zip(group.clouds[0].store.segments, scene.cloud.store.segments):
        assert torch.equal(a, b)
    assert _same_points(group.points()[0], scene.points())
    result = scene.detect()
    got, want = group.points(min_points=2, results=result, score_thr=0.0)[0], scene.points(min_points=2, result=result[0])
    assert _same_points(got, want) and torch.equal(got["ids"], want["ids"]) and torch.equal(got["kept"], want["kept"])
    with pytest.raises(ValueError, match="cloud=True"):
        det.begin_scenes([dict(c["meta"])]).points()


def test_a_subset_call_touches_only_the_listed_scenes(device):
    from depth_gate_ref import plane_depth
    from test_group_render_gpu import _chunk_meta, _det_scenes
    det, scenes = _det_scenes(device)
    depth = [plane_depth(scenes[s]["meta"], (64, 96), 0.0, noise=0.01, seed=s, missing=0.05).unsqueeze(0).to(device) for s in (0, 1)]
    group = det.begin_scenes([dict(scenes[s]["meta"]) for s in (0, 1)], window=2, cloud=True)

    def add(rows, a, b):
        group.add_views(torch.cat([scenes[s]["img"][:, a:b] for s in rows]), torch.cat([scenes[s]["dn"][:, a:b] for s in rows]),
                        [_chunk_meta(scenes[s]["meta"], a, b) for s in rows], scenes=rows, depth=torch.cat([depth[s][:, a:b] for s in rows]))

    add([0, 1], 0, 3)
    streams = []
    for s in (0, 1):
        st = det.begin_scene(dict(scenes[s]["meta"]), window=2, cloud=True)
        st.add_views(scenes[s]["img"][:, 0:3], scenes[s]["dn"][:, 0:3], _chunk_meta(scenes[s]["meta"], 0, 3), depth=depth[s][:, 0:3])
        streams.append(st)
    for s in (0, 1):                       # the sums depend on the depth maps, images and cameras alone: each scene's are its stream's
        assert _same_sums(group.cloud_sums()[s], streams[s].cloud_sums())
    assert not _same_sums(group.cloud_sums()[0], group.cloud_sums()[1])
    zero = group.cloud_sums(scenes=[0])[0]
    add([1], 3, 6)
    assert _same_sums(group.cloud_sums(scenes=[0])[0], zero) and len(group.clouds[0].store.segments) == 1
    assert len(group.clouds[1].store.segments) == 2
    streams[1].add_views(scenes[1]["img"][:, 3:6], scenes[1]["dn"][:, 3:6], _chunk_meta(scenes[1]["meta"], 3, 6), depth=depth[1][:, 3:6])
    assert _same_sums(group.cloud_sums()[1], streams[1].cloud_sums()) and _same_points(group.points(scenes=[1])[0], streams[1].points())
    assert len(group.points()) == 2 and _same_points(group.points()[0], streams[0].points())
    group.drop_oldest(1, scenes=[1])
    assert len(group.clouds[1].store.segments) == 1 and len(group.clouds[0].store.segments) == 1
    group.reset(scenes=[0])
    assert group.clouds[0].store.segments == [] and len(group.clouds[1].store.segments) == 1


# ---- 9. nothing changes without it ----
def test_without_cloud_nothing_changes(device):
    """cloud=None: no k_cloud* launch and exactly the plain scene's kernel names; cloud=True: one k_cloud_accumulate span per chunk, and
    the volume and detect() output of the plain scene bit for bit."""
    from nerfdet_amd import trace
    c = _carved(device)
    det = c["det"]
    trace.recorder = trace.Recorder()
    try:
        plain = _feed(det.begin_scene(dict(c["meta"])), c, [(0, 2), (2, 6)])
        names_plain = {s[0] for s in trace.recorder.spans}
        trace.recorder = trace.Recorder()
        none = _feed(det.begin_scene(dict(c["meta"]), cloud=None), c, [(0, 2), (2, 6)])
        names_none = {s[0] for s in trace.recorder.spans}
        trace.recorder = trace.Recorder()
        cloud = _feed(det.begin_scene(dict(c["meta"]), cloud=True), c, [(0, 2), (2, 6)])
        spans = [s for s in trace.recorder.spans if s[0].startswith("k_cloud")]
        names_cloud = {s[0] for s in trace.recorder.spans}
        trace.recorder = trace.Recorder()
        cloud.points()
        names_points = [s[0] for s in trace.recorder.spans]
    finally:
        trace.recorder = None
    assert not any(n.startswith("k_cloud") for n in names_plain | names_none) and names_none == names_plain
    assert plain.cloud is None and none.cloud is None
    assert [s[0] for s in spans] == ["k_cloud_accumulate"] * 2 and names_cloud - {"k_cloud_accumulate"} == names_plain
    assert names_points == ["k_cloud_count", "k_cloud_write"]
    for a, b in zip(plain.volume(), cloud.volume()):
        assert torch.equal(a, b)
    ra, rb = plain.detect()[0], cloud.detect()[0]
    assert torch.equal(ra["boxes_3d"].tensor, rb["boxes_3d"].tensor) and torch.equal(ra["scores_3d"], rb["scores_3d"])
    assert torch.equal(ra["labels_3d"], rb["labels_3d"]) and len(ra["scores_3d"]) > 0
    # cloud= is independent of carve= and keep_views
    both = _feed(det.begin_scene(dict(c["meta"]), carve=True, cloud=True, keep_views=True), c, [(0, 2), (2, 6)])
    carved = _feed(det.begin_scene(dict(c["meta"]), carve=True), c, [(0, 2), (2, 6)])
    assert _same_sums(both.cloud_sums(), cloud.cloud_sums())
    assert all(torch.equal(a, b) for a, b in zip(both.carve_counts(), carved.carve_counts()))
