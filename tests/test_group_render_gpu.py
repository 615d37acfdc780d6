"""GPU checks of view banks and rendering for scene groups: the grouped bank sampler (csrc/ray_stats_kernels.hip: k_ray_stats_bank_group,
rays.ray_view_stats_bank_group) against the single-bank sampler run per scene on the same banks -- the two kernels share one body, so
once against the packed and the generic kernels, which do not -- and SceneGroup(keep_views=True)
(nerf-det_amd/streaming.py): banks that follow the states, render_rays / render against the one-shot ray branch and SceneStream."""
import numpy as np
import pytest
import torch

from oracle import nerfdet_oracle as O

pytestmark = pytest.mark.gpu

ATOL = 2e-5      # tests/test_stream_render_gpu.py: the one-pass statistics against the generic (two-pass) kernel on identical fp32 coordinates
R, S = 257, 19   # 4883 samples: not a multiple of any samples-per-block

_CACHE = {}


def _inputs(device, n_v, d, hw, seed=0):
    """The recipe of tests/test_stream_render_gpu.py::_inputs (ring cameras, random maps, rays towards the ring's centre), made once per
    shape and seed and never changed.  ``seed`` gives scenes of the same shape their own maps, images, cameras (the ring turned) and points."""
    key = (str(device), n_v, d, hw, seed)
    if key not in _CACHE:
        from nerfdet_amd import rays
        gen = torch.Generator().manual_seed(n_v * 100 + d + 7919 * seed)
        meta = O.ring_scene_meta(n_v, hw)
        ext = meta["lidar2img"]["extrinsic"]
        meta["lidar2img"]["extrinsic"] = ext[seed % n_v:] + ext[:seed % n_v]
        feat = torch.randn(n_v, d, hw[0] // 4, hw[1] // 4, generator=gen).to(device).contiguous(memory_format=torch.channels_last)
        img = torch.rand(n_v, 3, *hw, generator=gen).to(device)
        ang = torch.rand(R, generator=gen) * 2 * np.pi
        ray_o = torch.stack([2.0 * torch.cos(ang), 2.0 * torch.sin(ang), 1.0 + 0.3 * torch.rand(R, generator=gen)], -1)
        ray_d = -ray_o / ray_o.norm(dim=-1, keepdim=True) + 0.35 * torch.randn(R, 3, generator=gen)
        pts, _ = rays.sample_along_camera_ray(ray_o.to(device), ray_d.to(device), [0.2, 8.0], S, det=True)
        _CACHE[key] = dict(meta=meta, feat=feat, img=img, pts=pts)
    return _CACHE[key]


def _chunk_meta(meta, v0, v1):
    m = dict(meta)
    m["lidar2img"] = dict(meta["lidar2img"], extrinsic=list(meta["lidar2img"]["extrinsic"][v0:v1]))
    return m


def _bank(d, sizes):
    from nerfdet_amd import rays
    bank, v = rays.ViewBank(), 0
    for k in sizes:
        bank.append(d["feat"][v:v + k], d["img"][v:v + k], _chunk_meta(d["meta"], v, v + k))
        v += k
    assert v == d["feat"].shape[0] and bank.n_views == v and len(bank.segments) == len(sizes)
    return bank


def _equal(got, want, what):
    for a, b, name in zip(got, want, ("globalfeat", "pixel_mask", "view_count")):
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {name} {tuple(a.shape)} {a.dtype} vs {tuple(b.shape)} {b.dtype}"
        assert torch.equal(a, b), f"{what}: {name} differs, max |diff| {float((a.float() - b.float()).abs().max()):.3e}"


def _singles(pts, banks):
    """The reference of every kernel-level comparison: the single-bank sampler, scene by scene, on the same banks and points."""
    from nerfdet_amd import rays
    return [rays.ray_view_stats_bank(p, b) for p, b in zip(pts, banks)]


def _samples_per_block(d):
    g = 64 // (d // 4 + 1)
    while g > 1 and 4 * g * 64 * 8 + 1024 > 64 * 1024:      # the host's LDS rule: d = 4 gives 31, not 32
        g -= 1
    return 4 * g


# ---- K-a: rounds, count pass and barrier positions differ between the blocks of one launch ----
def test_view_rounds_differ_between_blocks_of_one_launch(device):
    """1, 64, 65 and 130 views: zero, one, two and three rounds of 64, with and without the count pass, in one launch."""
    from nerfdet_amd import rays
    segs = [[1], [63, 1], [2, 63], [64, 2, 64]]
    inps = [_inputs(device, sum(s), 8, (32, 48), seed=i) for i, s in enumerate(segs)]
    banks = [_bank(inp, s) for inp, s in zip(inps, segs)]
    pts = [inp["pts"] for inp in inps]
    want = _singles(pts, banks)
    got = rays.ray_view_stats_bank_group(pts, banks)
    assert len(got) == 4
    for i, (g, w) in enumerate(zip(got, want)):
        _equal(g, w, f"scene {i} with {sum(segs[i])} views")
    assert not got[0][1].any() and int(got[0][2].max()) <= 1, "a single view never makes pixel_mask (more than one view) true"
    for i in (1, 2, 3):
        assert got[i][1].any() and 0.02 < got[i][1].float().mean() < 0.98
    assert int(got[3][2].max()) <= 130 and int(got[1][2].max()) <= 64


# ---- K-b: point counts: padding blocks of grid.x leave, tiles end in the middle of a wave ----
@pytest.mark.parametrize("d,hw,spb", [(8, (60, 80), 84), (32, (64, 96), 28), (4, (60, 80), 124)])
def test_point_counts_pad_the_grid_and_end_mid_wave(device, d, hw, spb):
    from nerfdet_amd import rays
    assert _samples_per_block(d) == spb
    counts = [1, spb - 1, spb + 1, R * S]
    views = [[3], [2, 3], [9], [4, 1, 7]]
    inps = [_inputs(device, sum(v), d, hw, seed=i) for i, v in enumerate(views)]
    banks = [_bank(inp, v) for inp, v in zip(inps, views)]
    pts = [inp["pts"].reshape(-1, 3)[R * S // 2 - c // 2:][:c] for inp, c in zip(inps, counts)]
    assert [p.shape[0] for p in pts] == counts
    want = _singles(pts, banks)
    got = rays.ray_view_stats_bank_group(pts, banks)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[0].shape == (counts[i], 2 * (3 + d)) and g[1].shape == (counts[i],)
        _equal(g, w, f"d={d}: scene {i} with {counts[i]} points")
    assert got[3][1].any() and not got[3][1].all()
    # shapes are kept: (R, S, 3) points give (R, S, ...) outputs, views into the call's buffers
    one = rays.ray_view_stats_bank_group([inps[3]["pts"], pts[1]], [banks[3], banks[1]])
    assert one[0][0].shape == (R, S, 2 * (3 + d)) and one[0][1].shape == (R, S) and one[1][2].shape == (counts[1],)
    assert one[1][0].data_ptr() == one[0][0].data_ptr() + 4 * R * S * 2 * (3 + d)
    _equal([t.reshape(w.shape) for t, w in zip(one[0], want[3])], want[3], "shaped points")
    _equal(one[1], want[1], "second of two")


# ---- K-c: a scene's rows do not depend on the call ----
def test_a_scenes_rows_do_not_depend_on_the_other_scenes(device):
    from nerfdet_amd import rays
    views = [[5], [40], [2, 10], [70]]
    inps = [_inputs(device, sum(v), 32, (64, 96), seed=10 + i) for i, v in enumerate(views)]
    banks = [_bank(inp, v) for inp, v in zip(inps, views)]
    pts = [inp["pts"].reshape(-1, 3)[:c] for inp, c in zip(inps, (4883, 300, 1001, 29))]
    want = _singles(pts, banks)

    def run(order):
        return rays.ray_view_stats_bank_group([pts[i] for i in order], [banks[i] for i in order])

    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [2, 0], [1, 3, 0], [0], [1], [2], [3]):
        for i, g in zip(order, run(order)):
            _equal(g, want[i], f"scene {i} in call {order}")
    # banks of another size or device, wrong list lengths: refused before anything is launched
    other = _bank(_inputs(device, 3, 8, (60, 80)), [3])
    with pytest.raises(ValueError, match="differs"):
        rays.ray_view_stats_bank_group([pts[0], pts[1]], [banks[0], other])
    with pytest.raises(ValueError):
        rays.ray_view_stats_bank_group([pts[0]], [banks[0], banks[1]])
    with pytest.raises(ValueError):
        rays.ray_view_stats_bank_group([], [])
    with pytest.raises(ValueError, match="at least one point"):
        rays.ray_view_stats_bank_group([pts[0], pts[1][:0]], [banks[0], banks[1]])
    with pytest.raises(RuntimeError, match="no views"):
        rays.ray_view_stats_bank_group([pts[0], pts[1]], [banks[0], rays.ViewBank()])


# ---- K-d: the full scene count ----
def test_sixty_four_scenes_in_one_launch(device):
    from nerfdet_amd import rays
    inps = [_inputs(device, 2, 8, (32, 48), seed=i) for i in range(64)]
    banks = [_bank(inp, [1, 1] if i % 2 else [2]) for i, inp in enumerate(inps)]
    pts = [inp["pts"].reshape(-1, 3)[37 * (i % 5):][:100] for i, inp in enumerate(inps)]
    want = _singles(pts, banks)
    got = rays.ray_view_stats_bank_group(pts, banks)
    assert len(got) == 64
    for i, (g, w) in enumerate(zip(got, want)):
        _equal(g, w, f"scene {i} of 64")
    assert any(g[1].any() for g in got)
    assert not torch.equal(got[0][0], got[2][0]), "the scenes differ"
    with pytest.raises(ValueError):
        rays.ray_view_stats_bank_group(pts + pts[:1], banks + banks[:1])


# ---- K-e: repeated calls ----
def test_repeated_calls_leave_tables_and_banks_unchanged(device):
    from nerfdet_amd import rays
    views = [[4, 1, 7], [2, 3], [9]]
    inps = [_inputs(device, sum(v), 32, (64, 96), seed=20 + i) for i, v in enumerate(views)]
    banks = [_bank(inp, v) for inp, v in zip(inps, views)]
    pts = [inp["pts"] for inp in inps]
    before = [[(s.feat.clone(), s.rgb4.clone(), s.ke.clone(), s.feat.data_ptr(), s.rgb4.data_ptr()) for s in b.segments] for b in banks]
    tables = [b.table()[0] for b in banks]
    rows = [t.clone() for t in tables]
    a = rays.ray_view_stats_bank_group(pts, banks)
    b = rays.ray_view_stats_bank_group(pts, banks)
    for x, y in zip(a, b):
        _equal(y, x, "second call")
    for bank, table, row, segs in zip(banks, tables, rows, before):
        assert bank.table()[0] is table and bank.table()[0].data_ptr() == table.data_ptr(), "the device table is cached until the segment list changes"
        assert torch.equal(table, row)
        for s, (f, i, k, fp, ip) in zip(bank.segments, segs):
            assert torch.equal(s.feat, f) and torch.equal(s.rgb4, i) and torch.equal(s.ke, k) and (s.feat.data_ptr(), s.rgb4.data_ptr()) == (fp, ip)
    _equal(rays.ray_view_stats_bank(pts[0], banks[0]), a[0], "the single-bank sampler after the grouped calls")


# ---- K-f: against kernels that do not share the bank samplers' body ----
@pytest.mark.parametrize("d,hw,spb", [(8, (60, 80), 84), (32, (64, 96), 28)])
def test_grouped_sampler_equals_the_packed_and_generic_kernels(device, d, hw, spb):
    """One launch over banks of 9, 40, 64, 100 and 130 views, with 1, 4G - 1 or 4G + 1 points each, every scene against rays.ray_view_stats
    over the concatenated segments.  Where that call takes k_ray_stats_packed the scene is its bits: 9, 40 and 64 views (no count pass, one
    round, a round of exactly 64) and, at d = 32, 100 views (count pass, two rounds).  Where it takes the generic kernel -- 130 views, and 100
    views at d = 8, whose records for two rounds of 21 samples a wave exceed the packed kernel's 64 KB of LDS -- the masks and counts are
    equal and the statistics within ATOL (tests/test_stream_render_gpu.py::test_more_than_128_views_match_generic_kernel).  Neither
    reference runs rb_walk."""
    from nerfdet_amd import rays, trace
    assert _samples_per_block(d) == spb
    segs = [[4, 5], [40], [63, 1], [63, 2, 35], [64, 2, 64]]
    counts = [spb + 1, 1, spb - 1, spb + 1, spb - 1]
    inps = [_inputs(device, sum(s), d, hw, seed=30 + i) for i, s in enumerate(segs)]
    banks = [_bank(inp, s) for inp, s in zip(inps, segs)]
    pts = [inp["pts"].reshape(-1, 3)[R * S // 2 - c // 2:][:c] for inp, c in zip(inps, counts)]
    assert [p.shape[0] for p in pts] == counts and [b.n_views for b in banks] == [9, 40, 64, 100, 130]
    prev, trace.recorder = trace.recorder, trace.Recorder()
    try:
        got = rays.ray_view_stats_bank_group(pts, banks)
        want = [rays.ray_view_stats(p, inp["img"], rays._compute_projection(inp["meta"]), inp["feat"]) for p, inp in zip(pts, inps)]
        names = [sp[0] for sp in trace.recorder.spans]
    finally:
        trace.recorder = prev
    packed = [rays.packed_ok(b.n_views, d) for b in banks]
    assert packed == [True, True, True, d == 32, False]
    assert names == ["k_ray_stats_bank_group"] + ["k_ray_stats_packed" if p else "k_ray_view_stats" for p in packed], names
    for i, (g, w) in enumerate(zip(got, want)):
        what = f"d={d}: {banks[i].n_views} views, {counts[i]} points"
        assert g[0].shape == w[0].shape == (counts[i], 2 * (3 + d))
        if packed[i]:
            _equal(g, w, what + " against the packed kernel")
            continue
        print(f"{what}: max |group - generic| = {float((g[0] - w[0]).abs().max()):.3e} (bound {ATOL:.0e})")
        assert torch.equal(g[1], w[1]) and torch.equal(g[2], w[2]), what + " against the generic kernel: masks or counts differ"
        torch.testing.assert_close(g[0], w[0], rtol=0, atol=ATOL)
    assert any(bool(g[1].any()) for g in got), "no sample of the call is seen by more than one view"


# ---- detector level ----
def _det_scenes(device):
    """_small_detector and three scenes of synth.train_scene(6, (64, 96), t_views=2) with their own seeds, origins and cameras; made once."""
    key = ("det", str(device))
    if key not in _CACHE:
        from nerfdet_amd import synth
        from test_detector_gpu import _small_detector
        det = _small_detector(device)
        scenes = []
        for i in range(3):
            batch = synth.batch_to(synth.train_scene(6, (64, 96), t_views=2, n_boxes=2, seed=4 + i), device)
            meta = batch["img_metas"][0]
            meta["lidar2img"]["origin"] = np.asarray(meta["lidar2img"]["origin"], dtype=np.float32) + np.float32([0.2 * i, -0.1 * i, 0.0])
            ext = meta["lidar2img"]["extrinsic"]
            meta["lidar2img"]["extrinsic"] = ext[2 * i:] + ext[:2 * i]
            scenes.append(dict(img=batch["img"], dn=batch["denorm_images"], meta=meta, rb=det._ray_batch(batch)))
        _CACHE[key] = (det, scenes)
    return _CACHE[key]


def _feed(group, scenes, calls):
    """``calls``: per add_views call a list of (scene, v0, v1), every row with the same number of views."""
    for call in calls:
        rows = [s for s, _, _ in call]
        group.add_views(torch.cat([scenes[s]["img"][:, a:b] for s, a, b in call]), torch.cat([scenes[s]["dn"][:, a:b] for s, a, b in call]),
                        [_chunk_meta(scenes[s]["meta"], a, b) for s, a, b in call], scenes=rows)
        _books(group)
    return group


def _books(group):
    """The banks hold the chunks the states hold.  An unwindowed scene reports its views as one chunk (``chunk_views`` is ``[n_views]``) while
    its bank keeps a segment per add_views call, so there the totals are compared; a windowed scene's lists are equal entry for entry."""
    for s in range(group.n_scenes):
        segs = [seg.n_views for seg in group.banks[s].segments]
        if group.window is None:
            assert sum(segs) == sum(group.chunk_views[s]) == group.n_views[s], (s, segs, group.chunk_views[s])
        else:
            assert segs == group.chunk_views[s] and len(segs) <= group.window, (s, segs, group.chunk_views[s])


def _rays_of(scene, n):
    o, d = scene["rb"]["ray_o"].view(-1, 3), scene["rb"]["ray_d"].view(-1, 3)
    while o.shape[0] < n:
        o, d = torch.cat([o, o]), torch.cat([d, d.flip(0)])
    return o[:n].contiguous(), d[:n].contiguous()


def _one_shot(det, bank, fed_meta, ray_o, ray_d):
    """rays.render_rays_func(det=True) over the concatenation of the bank's own segments, in passes of RENDER_TESTING_RAYS rays (the D-b
    comparison of tests/test_stream_render_gpu.py).  ``fed_meta``: the scene's meta with the extrinsics of the views held, oldest first."""
    from nerfdet_amd import rays
    feat = torch.cat([s.feat for s in bank.segments]).permute(0, 3, 1, 2)
    rgb = torch.cat([s.rgb4 for s in bank.segments])[..., :3].permute(0, 3, 1, 2)
    assert rays.packed_ok(feat.shape[0], feat.shape[1])
    assert len(fed_meta["lidar2img"]["extrinsic"]) == feat.shape[0]
    outs = []
    with torch.no_grad():
        for i in range(0, ray_o.shape[0], rays.RENDER_TESTING_RAYS):
            o, d = ray_o[i:i + rays.RENDER_TESTING_RAYS], ray_d[i:i + rays.RENDER_TESTING_RAYS]
            outs.append(rays.render_rays_func(o, d, None, None, feat, rgb, det.aabb, det.near_far_range, det.N_samples, det.N_rand, det.nerf_mlp,
                                              fed_meta, None, "image", det=True)["outputs_coarse"])
    return {k: torch.cat([o[k] for o in outs]) for k in ("rgb", "depth", "mask")}


def _fed_meta(scene, ranges):
    """The scene's meta with the extrinsics of the views fed, in the order they were fed."""
    ext = scene["meta"]["lidar2img"]["extrinsic"]
    m = dict(scene["meta"])
    m["lidar2img"] = dict(scene["meta"]["lidar2img"], extrinsic=[e for a, b in ranges for e in ext[a:b]])
    return m


def _same_render(got, want, what):
    for key in ("rgb", "depth", "mask"):
        assert got[key].shape == want[key].shape and torch.equal(got[key], want[key]), f"{what}: {key} differs"


CALLS = [[(2, 0, 2), (0, 0, 2)], [(1, 0, 3)], [(0, 2, 3), (1, 3, 4), (2, 2, 3)], [(2, 3, 6), (0, 3, 6)], [(1, 4, 6)]]
FED = {0: [(0, 2), (2, 3), (3, 6)], 1: [(0, 3), (3, 4), (4, 6)], 2: [(0, 2), (2, 3), (3, 6)]}


@pytest.mark.parametrize("window", [None, 2])
def test_banks_follow_the_states(device, window):
    """Subsets and per-scene chunkings, unwindowed and window=2 (where every scene's third chunk evicts its first): after every call a scene's
    bank holds the chunks its states hold; drop_oldest and reset take the listed scenes' segments along."""
    det, scenes = _det_scenes(device)
    group = det.begin_scenes([dict(sc["meta"]) for sc in scenes], window=window, keep_views=True)
    assert len(group.banks) == 3 and all(b.n_views == 0 for b in group.banks)
    _feed(group, scenes, CALLS)
    if window is None:
        assert group.n_views == [6, 6, 6] and [[s.n_views for s in b.segments] for b in group.banks] == [[2, 1, 3], [3, 1, 2], [2, 1, 3]]
        with pytest.raises(ValueError):
            group.drop_oldest(1, scenes=[1])
    else:
        assert group.chunk_views == [[1, 3], [1, 2], [1, 3]] == [[s.n_views for s in b.segments] for b in group.banks]
        kept = group.banks[1].segments[1]
        group.drop_oldest(1, scenes=[1])
        _books(group)
        assert group.chunk_views == [[1, 3], [2], [1, 3]] and group.banks[1].segments == [kept]
        with pytest.raises(ValueError):
            group.drop_oldest(2, scenes=[0, 1])          # refused whole: scene 1 holds one chunk
        _books(group)
        assert group.chunk_views == [[1, 3], [2], [1, 3]]
    group.reset(scenes=[0])
    _books(group)
    assert group.n_views[0] == 0 and group.banks[0].segments == [] and group.banks[1].n_views > 0 and group.banks[2].n_views == 4 + 2 * (window is None)
    o, d = _rays_of(scenes[0], 16)
    with pytest.raises(RuntimeError, match="no views"):
        group.render_rays([o, o], [d, d], scenes=[1, 0])
    _feed(group, scenes, [[(0, 1, 4)]])
    assert group.banks[0].n_views == 3


def test_a_window_renders_what_a_fresh_window_renders(device):
    """window=2 fed a, b, c renders bit for bit what a fresh windowed group fed b, c renders: the evicted chunk leaves no trace in a bank."""
    det, scenes = _det_scenes(device)
    metas = [dict(sc["meta"]) for sc in scenes]
    a, b, c = [[(s, v0, v1) for s in range(3)] for v0, v1 in ((0, 2), (2, 4), (4, 6))]
    group = _feed(det.begin_scenes(metas, window=2, keep_views=True), scenes, [a, b, c])
    fresh = _feed(det.begin_scenes(metas, window=2, keep_views=True), scenes, [b, c])
    assert group.chunk_views == fresh.chunk_views == [[2, 2]] * 3
    rays_ = [_rays_of(sc, 2048) for sc in scenes]
    o, d = [r[0] for r in rays_], [r[1] for r in rays_]
    got, want = group.render_rays(o, d), fresh.render_rays(o, d)
    for s in range(3):
        _same_render(got[s], want[s], f"scene {s}")
        assert got[s]["mask"].any()
    # and its detections: the banks are beside the states, not in their way
    for g, w in zip(group.detect(), fresh.detect()):
        assert torch.equal(g["scores_3d"], w["scores_3d"]) and torch.equal(g["boxes_3d"].tensor, w["boxes_3d"].tensor)


@pytest.mark.parametrize("window", [None, 2])
def test_a_failed_add_views_changes_nothing(device, window, monkeypatch):
    """add_views that raises before, between and after the segments are made leaves every bank, state and window as it was."""
    from nerfdet_amd import ops
    det, scenes = _det_scenes(device)
    group = _feed(det.begin_scenes([dict(sc["meta"]) for sc in scenes], window=window, keep_views=True), scenes, CALLS[:3])

    def books():
        return ([list(b.segments) for b in group.banks], list(group.n_views), [list(c) for c in group.chunk_views],
                None if window is None else [list(segs) for segs in group.pool.segs],
                [b._table for b in group.banks])

    def unchanged(before, what):
        after = books()
        for s in range(3):
            assert len(after[0][s]) == len(before[0][s]) and all(x is y for x, y in zip(after[0][s], before[0][s])), f"{what}: bank {s} changed"
            assert after[4][s] is before[4][s], f"{what}: bank {s}'s table was dropped"
        assert after[1] == before[1] and after[2] == before[2], what
        if window is not None:
            assert all(x is y for a, b in zip(after[3], before[3]) for x, y in zip(a, b)) and [len(a) for a in after[3]] == [len(b) for b in before[3]], what
        _books(group)

    for b in group.banks:
        b.table()
    o, d = zip(*[_rays_of(sc, 512) for sc in scenes])
    want = group.render_rays(list(o), list(d))
    before = books()
    call = [(0, 3, 5), (1, 4, 6), (2, 3, 5)]
    args = (torch.cat([scenes[s]["img"][:, a:b] for s, a, b in call]), torch.cat([scenes[s]["dn"][:, a:b] for s, a, b in call]))
    metas = [_chunk_meta(scenes[s]["meta"], a, b) for s, a, b in call]
    # a wrong extrinsic count on the last row
    with pytest.raises(ValueError, match="extrinsics"):
        group.add_views(*args, metas[:2] + [_chunk_meta(scenes[2]["meta"], 3, 6)])
    unchanged(before, "wrong extrinsic count")
    # the last listed scene's make_segment raises after the others' segments were made
    made = []
    real = group.banks[2].make_segment
    monkeypatch.setattr(group.banks[0], "make_segment", lambda *a, **k: made.append(0) or type(group.banks[0]).make_segment(group.banks[0], *a, **k))

    def refuse(*a, **k):
        made.append(2)
        raise ValueError("refused for the test")
    monkeypatch.setattr(group.banks[2], "make_segment", refuse)
    with pytest.raises(ValueError, match="refused for the test"):
        group.add_views(*args, metas)
    assert made == [0, 2]
    unchanged(before, "a later scene's make_segment raised")
    monkeypatch.setattr(group.banks[2], "make_segment", real)
    # the grouped accumulate raises after every segment was made
    name = "scene_accumulate_group" if window is None else "scene_accumulate_group_ring"

    def fail(*a, **k):
        raise RuntimeError("accumulate failed for the test")
    monkeypatch.setattr(ops, name, fail)
    with pytest.raises(RuntimeError, match="accumulate failed"):
        group.add_views(*args, metas)
    unchanged(before, "the accumulate raised")
    monkeypatch.undo()
    got = group.render_rays(list(o), list(d))
    for s in range(3):
        _same_render(got[s], want[s], f"scene {s} after the failed calls")
    group.add_views(*args, metas)
    _books(group)
    assert [b.n_views for b in group.banks] == ([5, 6, 5] if window is None else [3, 3, 3])


def test_render_rays_equals_the_one_shot_ray_branch_per_scene(device):
    """Ray counts 1, 2048 and RENDER_TESTING_RAYS + 5 (two passes, two scenes finishing early), scenes listed out of order: every scene is
    bit for bit rays.render_rays_func(det=True) over the concatenation of its own bank segments."""
    from nerfdet_amd import rays
    det, scenes = _det_scenes(device)
    group = _feed(det.begin_scenes([dict(sc["meta"]) for sc in scenes], keep_views=True), scenes, CALLS)
    listed = [2, 0, 1]
    counts = [1, 2048, rays.RENDER_TESTING_RAYS + 5]
    rr = [_rays_of(scenes[s], n) for s, n in zip(listed, counts)]
    got = group.render_rays([r[0] for r in rr], [r[1] for r in rr], scenes=listed)
    assert len(got) == 3
    for (o, d), s, n, g in zip(rr, listed, counts, got):
        want = _one_shot(det, group.banks[s], _fed_meta(scenes[s], FED[s]), o, d)
        assert g["rgb"].shape == (n, 3) and g["depth"].shape == (n,) and g["mask"].shape == (n,) and g["mask"].dtype == torch.bool
        _same_render(g, want, f"scene {s} with {n} rays")
        if n > 1:
            assert g["mask"].any() and float(g["rgb"].abs().max()) > 0
    # a scene's render does not depend on the call it is listed in
    alone = group.render_rays([rr[2][0]], [rr[2][1]], scenes=[1])
    _same_render(alone[0], got[2], "scene 1 alone")


def test_group_of_one_is_a_scene_stream(device):
    """One scene, one chunk: render_rays and render are SceneStream(keep_views=True)'s bit for bit, and keeping the views does not change detect()."""
    from nerfdet_amd import rays
    det, scenes = _det_scenes(device)
    sc = scenes[1]
    call = [[(0, 0, 6)]]
    one = [dict(img=sc["img"], dn=sc["dn"], meta=sc["meta"])]
    det.render_testing = True
    try:
        with pytest.raises(NotImplementedError):
            det.begin_scenes([dict(sc["meta"])])
        group = _feed(det.begin_scenes([dict(sc["meta"])], keep_views=True), one, call)
    finally:
        det.render_testing = False
    stream = det.begin_scene(dict(sc["meta"]), keep_views=True)
    stream.add_views(sc["img"], sc["dn"], _chunk_meta(sc["meta"], 0, 6))
    o, d = sc["rb"]["ray_o"].view(-1, 3), sc["rb"]["ray_d"].view(-1, 3)
    for batched in (False, True):
        got = group.render_rays([o], [d], batched=batched)
        assert len(got) == 1
        _same_render(got[0], stream.render_rays(o, d), f"render_rays(batched={batched})")
    assert got[0]["mask"].any()
    got, want = group.render([sc["rb"]]), stream.render(sc["rb"])
    assert len(got) == 1 and set(got[0]) == set(want)
    for key in ("rgb", "depth"):
        assert got[0]["outputs_coarse"][key].shape == want["outputs_coarse"][key].shape
        assert torch.equal(got[0]["outputs_coarse"][key], want["outputs_coarse"][key]), key
    assert torch.equal(got[0]["gt_rgb"], want["gt_rgb"]) and torch.equal(got[0]["gt_depth"], want["gt_depth"])
    psnr, ssim, err = rays.rendering_metrics(got[0])
    assert torch.isfinite(psnr) and torch.isfinite(ssim)
    plain = _feed_plain(det, one, call)
    a, b = group.detect()[0], plain.detect()[0]
    assert torch.equal(a["labels_3d"], b["labels_3d"]) and torch.equal(a["scores_3d"], b["scores_3d"]) and torch.equal(a["boxes_3d"].tensor, b["boxes_3d"].tensor)
    assert len(a["scores_3d"]) > 0


def _feed_plain(det, scenes, calls):
    group = det.begin_scenes([dict(sc["meta"]) for sc in scenes])
    assert group.banks is None
    for call in calls:
        group.add_views(torch.cat([scenes[s]["img"][:, a:b] for s, a, b in call]), torch.cat([scenes[s]["dn"][:, a:b] for s, a, b in call]),
                        [_chunk_meta(scenes[s]["meta"], a, b) for s, a, b in call], scenes=[s for s, _, _ in call])
    return group


def test_batched_render_shares_the_scales_within_the_chunking_contract(device):
    """batched=True: one nerf_mlp and one raw2outputs call per pass; the scenes share linear_rows' per-tensor fp16-pair scales.  Masks are
    bit-equal, rgb within 1e-4 absolute, depth within 1e-4 x near_far_range[1] of batched=False; one listed scene is batched=False bit for bit."""
    from nerfdet_amd import rays
    det, scenes = _det_scenes(device)
    group = _feed(det.begin_scenes([dict(sc["meta"]) for sc in scenes], window=2, keep_views=True), scenes, CALLS)
    counts = [3000, 2048, rays.RENDER_TESTING_RAYS + 5]
    rr = [_rays_of(sc, n) for sc, n in zip(scenes, counts)]
    o, d = [r[0] for r in rr], [r[1] for r in rr]
    want = group.render_rays(o, d)
    got = group.render_rays(o, d, batched=True)
    far = float(det.near_far_range[1])
    for s in range(3):
        e_rgb = float((got[s]["rgb"] - want[s]["rgb"]).abs().max())
        e_depth = float((got[s]["depth"] - want[s]["depth"]).abs().max())
        print(f"scene {s}: {counts[s]} rays, batched against unbatched: max |rgb| {e_rgb:.3e} (bound 1e-4), max |depth| {e_depth:.3e} "
              f"(bound {1e-4 * far:.3e}), mask mean {float(want[s]['mask'].float().mean()):.3f}")
        assert got[s]["rgb"].shape == want[s]["rgb"].shape and got[s]["depth"].shape == want[s]["depth"].shape
        assert torch.equal(got[s]["mask"], want[s]["mask"]) and want[s]["mask"].any()
        assert e_rgb <= 1e-4 and e_depth <= 1e-4 * far
    one = group.render_rays(o[1:2], d[1:2], scenes=[1], batched=True)
    _same_render(one[0], want[1], "one listed scene, batched")


def test_render_returns_what_scene_stream_render_returns(device):
    from nerfdet_amd import rays
    det, scenes = _det_scenes(device)
    group = _feed(det.begin_scenes([dict(sc["meta"]) for sc in scenes], keep_views=True), scenes, CALLS)
    listed = [1, 2]
    got = group.render([scenes[s]["rb"] for s in listed], scenes=listed)
    bat = group.render([scenes[s]["rb"] for s in listed], scenes=listed, batched=True)
    t, hh, ww = 2, 44, 76
    far = float(det.near_far_range[1])
    for s, g, b in zip(listed, got, bat):
        assert g["outputs_coarse"]["rgb"].shape == (t, hh, ww, 3) and g["outputs_coarse"]["depth"].shape == (t, hh, ww, 1)
        assert g["gt_rgb"].shape == (t, hh, ww, 3) and g["gt_depth"].shape == (t, hh, ww, 1)
        assert torch.equal(g["gt_rgb"], scenes[s]["rb"]["gt_rgb"].view(t, hh, ww, 3))
        o, d = scenes[s]["rb"]["ray_o"].view(-1, 3), scenes[s]["rb"]["ray_d"].view(-1, 3)
        flat = group.render_rays([o], [d], scenes=[s])[0]
        assert torch.equal(g["outputs_coarse"]["rgb"].view(-1, 3), flat["rgb"]) and torch.equal(g["outputs_coarse"]["depth"].view(-1), flat["depth"])
        psnr, ssim, err = rays.rendering_metrics(g)
        assert torch.isfinite(psnr) and torch.isfinite(ssim) and err.shape == (hh, ww, 1)
        assert float((b["outputs_coarse"]["rgb"] - g["outputs_coarse"]["rgb"]).abs().max()) <= 1e-4
        assert float((b["outputs_coarse"]["depth"] - g["outputs_coarse"]["depth"]).abs().max()) <= 1e-4 * far
    with pytest.raises(ValueError, match="ray batches"):
        group.render([scenes[0]["rb"]], scenes=listed)
