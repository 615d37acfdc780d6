"""GPU checks of scene groups (nerf-det_amd/streaming.py::SceneGroup, ops.scene_accumulate_group / density_finish_group /
volume_finish_group): a scene's state after a grouped accumulate against ops.scene_accumulate on that scene alone, the grouped finishes
against the single-state ones -- all bit for bit -- and SceneGroup against SceneStream and simple_test."""
import numpy as np
import pytest
import torch

from test_streaming_gpu import _chunk_meta, _close, _gate, _inputs, _one_shot, _same, _splits, _stream

pytestmark = pytest.mark.gpu

ORIGINS = [(-0.4, 0.0, 0.5), (0.0, 0.3, 0.6), (0.4, 0.6, 0.7)]        # every scene sees part of its grid only (checked below)
FAR_ORIGINS = [(0.4, 0.6, 0.7), (-0.6, 0.5, 0.8)]                      # the same for the 70-view ring at 32 x 48
SIDE_ORIGINS = [(1.2, 0.0, 1.5), (-1.2, 0.0, 0.5)]                     # a 3 x 3 x 2 grid beside a 24 x 32 ring: 3 views see part of it
TENSORS = ("k1_sum", "k1_count", "k2_sum", "k2_count")


def _scenes(device, n_v, origins, seed0, **kw):
    """One ``_inputs`` set per scene: its own seed (features, mapped maps, images, depth), its own origin (points) and its own cameras --
    scene s takes the views v + s of a ring of ``n_v + len(origins) - 1`` cameras (``_views``), so no two listed scenes of a call share a
    projection, a feature map, an image or a depth map."""
    from nerfdet_amd import ops
    ds = []
    for i, org in enumerate(origins):
        d = _inputs(device, n_v + len(origins) - 1, seed=seed0 + i, **kw)
        d["points"] = ops.get_points(d["grid"], d["vs"], np.float32(org), device)
        d["shift"] = i
        ds.append(d)
    assert all(not torch.equal(a["proj"][a["shift"]:a["shift"] + n_v], b["proj"][b["shift"]:b["shift"] + n_v]) for a, b in zip(ds, ds[1:]))
    return ds


def _views(d, key, v0, v1):
    """The scene's views v0 .. v1 of ``key``: the ring's cameras v0 + shift .. v1 + shift."""
    return d[key][v0 + d["shift"]:v1 + d["shift"]]


def _new_group(ds):
    from nerfdet_amd import ops
    d0 = ds[0]
    return ops.SceneGroupState(d0["grid"], d0["feats"].shape[1], d0["mapped"].shape[1], [d["points"] for d in ds], d0["feats"].device)


def _new_refs(ds):
    from nerfdet_amd import ops
    d0 = ds[0]
    return [ops.SceneState(d0["grid"], d0["feats"].shape[1], d0["mapped"].shape[1], d0["feats"].device) for _ in ds]


def _feed(group, refs, ds, listed, v0, v1, gated):
    """The views v0 .. v1 of every listed scene: one grouped call, and the same slices through ops.scene_accumulate per scene."""
    from nerfdet_amd import ops
    bias = ds[0]["bias"]                      # the group's one Linear bias (K2's pivot); every scene keeps its own mapped maps
    rows = listed if listed is not None else list(range(len(ds)))
    cat = lambda key: torch.cat([_views(ds[s], key, v0, v1) for s in rows])
    d0 = ds[0]
    gate = ops.depth_gate(cat("depth"), d0["vs"], (d0["h"], d0["w"]), d0["hw"]) if gated else None
    ops.scene_accumulate_group(group, listed, cat("feats"), cat("mapped"), bias, cat("rgb"), cat("proj"), cat("rgb_proj"), depth_gate=gate)
    for s in rows:
        d = ds[s]
        ops.scene_accumulate(refs[s], _views(d, "feats", v0, v1), _views(d, "mapped", v0, v1), bias, _views(d, "rgb", v0, v1), d["points"],
                             _views(d, "proj", v0, v1), _views(d, "rgb_proj", v0, v1), depth_gate=_gate(d, v0 + d["shift"], v1 + d["shift"], gated))


def _snapshot(group):
    return [[getattr(st, t).clone() for t in TENSORS] for st in group.states]


def _assert_states(group, refs, what):
    for s, (st, ref) in enumerate(zip(group.states, refs)):
        assert st.n_views == ref.n_views, (what, s)
        for t in TENSORS:
            assert torch.equal(getattr(st, t), getattr(ref, t)), f"{what}: scene {s}'s {t} differs from ops.scene_accumulate on that scene alone"


def _assert_finishes(group, refs, bias, listed, seed=3):
    from nerfdet_amd import ops
    rows_of = listed if listed is not None else list(range(len(refs)))
    n_vox = refs[0].n_voxels
    before = _snapshot(group)
    rows = ops.density_finish_group(group, bias, listed)
    assert rows.shape == (len(rows_of) * n_vox, 2 * (3 + refs[0].cm))
    alpha = torch.rand(len(rows_of) * n_vox, generator=torch.Generator().manual_seed(seed)).to(rows.device)
    mean, cnt = ops.volume_finish_group(group, None, listed)
    vol, cnt2 = ops.volume_finish_group(group, alpha, listed)
    assert mean.shape == (len(rows_of), refs[0].c) + refs[0].grid and cnt.shape == (len(rows_of), 1) + refs[0].grid and cnt.dtype == torch.int64
    for i, s in enumerate(rows_of):
        assert torch.equal(rows[i * n_vox:(i + 1) * n_vox], ops.density_finish(refs[s], bias)), f"density rows of scene {s} (listed {i})"
        want_mean, want_cnt = ops.volume_finish(refs[s])
        want_vol, _ = ops.volume_finish(refs[s], alpha[i * n_vox:(i + 1) * n_vox])
        assert torch.equal(mean[i], want_mean) and torch.equal(vol[i], want_vol), f"volume of scene {s} (listed {i})"
        assert torch.equal(cnt[i], want_cnt) and torch.equal(cnt2[i], want_cnt), f"counts of scene {s} (listed {i})"
        assert mean[i].stride() == want_mean.stride()          # channels-last memory, as the single-state finish hands it to neck_3d
    for a, b in zip(before, _snapshot(group)):
        assert all(torch.equal(x, y) for x, y in zip(a, b)), "finishing changed a state"


@pytest.mark.parametrize("gated,c", [(False, 64), (True, 64), (False, 320), (True, 320)])
def test_group_accumulate_and_finishes_match_single_scene(device, gated, c):
    """S = 3, N = 315 (a ragged tail for the 4-voxel K2 blocks and the 16-voxel K1 tile); c = 320 takes NCHUNK = 2."""
    ds = _scenes(device, 5, ORIGINS, seed0=11, grid=(7, 9, 5), c=c)
    group, refs = _new_group(ds), _new_refs(ds)
    bias = ds[0]["bias"]
    _feed(group, refs, ds, None, 0, 3, gated)               # k = 3 for every scene
    _assert_states(group, refs, "k=3, all scenes")
    _feed(group, refs, ds, None, 3, 5, gated)               # then k = 2
    _assert_states(group, refs, "k=2, all scenes")
    assert group.n_views == [5, 5, 5]
    _assert_finishes(group, refs, bias, None)
    keep = [getattr(group.states[1], t).clone() for t in TENSORS]
    _feed(group, refs, ds, [2, 0], 1, 3, gated)             # a subset, listed order against slot order
    _assert_states(group, refs, "k=2, scenes [2, 0]")
    assert group.n_views == [7, 5, 7]
    assert all(torch.equal(getattr(group.states[1], t), k) for t, k in zip(TENSORS, keep)), "an unlisted scene changed"
    _assert_finishes(group, refs, bias, None)               # view totals now differ between the scenes
    _assert_finishes(group, refs, bias, [2, 0])
    _assert_finishes(group, refs, bias, [1])
    for s, ref in enumerate(refs):
        seen = int((ref.k1_count != 0).sum())
        assert 0 < seen < ref.n_voxels, f"scene {s}: {seen} of {ref.n_voxels} voxels seen -- the case needs seen and unseen voxels"
    if gated:
        ungated = _new_refs(ds)
        _feed(_new_group(ds), ungated, ds, None, 0, 5, False)
        assert all(int(a.k1_count.sum()) < int(b.k1_count.sum()) for a, b in zip(refs, ungated)), "the gate dropped nothing"


def test_group_accumulate_two_view_rounds(device):
    """k = 70: two 64-view rounds in K1's walk and in the packed K2 walk."""
    ds = _scenes(device, 70, FAR_ORIGINS, seed0=21, hw=(32, 48), grid=(8, 8, 4))
    group, refs = _new_group(ds), _new_refs(ds)
    _feed(group, refs, ds, [1, 0], 0, 70, False)
    _assert_states(group, refs, "k=70")
    _assert_finishes(group, refs, ds[0]["bias"], None)
    for s, ref in enumerate(refs):
        seen = int((ref.k1_count != 0).sum())
        assert 0 < seen < ref.n_voxels and int(ref.k1_count.max()) > 64, f"scene {s}: {seen} voxels seen, at most {int(ref.k1_count.max())} views"


@pytest.mark.parametrize("gated", [False, True])
def test_four_channel_chunks(device, gated):
    """C = 516 takes the accumulate kernels' NCHUNK = 4 (C > 512): c4 = 129 is the first quad of the third 64-lane chunk, so the ``ci < c4``
    guard cuts inside a chunk.  N = 18: one full 16-voxel K1 tile and one with 2 live voxels.  Two scenes, 3 views each as chunks of 2 and
    1: the single states against one launch over the 3 views, the group's states against the single states, and the four volume finishes
    against each other over one-segment rings."""
    from nerfdet_amd import ops
    ds = _scenes(device, 3, SIDE_ORIGINS, seed0=51, hw=(24, 32), grid=(3, 3, 2), c=516)
    d0 = ds[0]
    assert d0["feats"].shape[1:] == (516, 6, 8)
    group, refs = _new_group(ds), _new_refs(ds)
    _feed(group, refs, ds, None, 0, 2, gated)
    _feed(group, refs, ds, None, 2, 3, gated)
    _assert_states(group, refs, "chunks of 2 and 1")
    # a windowed pool holding each scene's 3 views as one chunk: K1's sums do not depend on the chunking, so its states are one-segment
    # rings over the same sums
    pool = ops.SceneGroupRingState(d0["grid"], 516, d0["mapped"].shape[1], [d["points"] for d in ds], 2, device)
    cat = lambda key: torch.cat([_views(d, key, 0, 3) for d in ds])
    ops.scene_accumulate_group_ring(pool, None, cat("feats"), cat("mapped"), d0["bias"], cat("rgb"), cat("proj"), cat("rgb_proj"),
                                    depth_gate=ops.depth_gate(cat("depth"), d0["vs"], (d0["h"], d0["w"]), d0["hw"]) if gated else None)
    assert pool.n_chunks == [1, 1]
    n_vox = refs[0].n_voxels
    assert n_vox == 18
    for alpha in (None, torch.rand(2 * n_vox, generator=torch.Generator().manual_seed(3)).to(device)):
        group_mean, group_cnt = ops.volume_finish_group(group, alpha)
        pool_mean, pool_cnt = ops.volume_finish_group_ring(pool, alpha)
        for s, (d, ref) in enumerate(zip(ds, refs)):
            a = None if alpha is None else alpha[s * n_vox:(s + 1) * n_vox]
            seg, = pool.segs[s]
            assert torch.equal(seg.k1_sum, ref.k1_sum) and torch.equal(seg.k1_count, ref.k1_count), f"scene {s}: one chunk of 3 against 2 + 1"
            want_mean, want_cnt = ops.backproject_aggregate(_views(d, "feats", 0, 3), d["points"], _views(d, "proj", 0, 3), alpha=a,
                                                            depth_gate=_gate(d, d["shift"], d["shift"] + 3, gated))
            mean, cnt = ops.volume_finish(ref, a)
            assert torch.equal(cnt, want_cnt) and torch.equal(mean, want_mean), f"scene {s}: K1 sums differ from one launch over the 3 views"
            ring_mean, ring_cnt = ops.volume_finish_ring([ref], a)
            assert torch.equal(ring_mean, mean) and torch.equal(ring_cnt, cnt), f"scene {s}: ring of one state"
            assert torch.equal(group_mean[s], mean) and torch.equal(group_cnt[s], cnt), f"scene {s}: group finish"
            assert torch.equal(pool_mean[s], mean) and torch.equal(pool_cnt[s], cnt), f"scene {s}: group ring finish"
    for s, ref in enumerate(refs):
        seen = int((ref.k1_count != 0).sum())
        assert 0 < seen < n_vox, f"scene {s}: {seen} of {n_vox} voxels seen -- the case needs seen and unseen voxels"
    assert int(refs[1].k1_count[16:].min()) > 0, "no view sees the 2 voxels of the ragged tile"
    if gated:
        ungated = _new_refs(ds)
        _feed(_new_group(ds), ungated, ds, None, 0, 3, False)
        assert all(int(a.k1_count.sum()) < int(b.k1_count.sum()) for a, b in zip(refs, ungated)), "the gate dropped nothing"


def test_group_ops_refuse_bad_calls(device):
    from nerfdet_amd import ops
    ds = _scenes(device, 4, ORIGINS[:2], seed0=31, grid=(7, 9, 5))
    group, refs = _new_group(ds), _new_refs(ds)
    with pytest.raises(ValueError, match="no views"):
        ops.density_finish_group(group, ds[0]["bias"])
    _feed(group, refs, ds, [1], 0, 2, False)
    before = _snapshot(group)
    with pytest.raises(ValueError, match="no views"):
        ops.volume_finish_group(group, None, [1, 0])
    d = ds[0]
    for scenes in ([0, 0], [2], [-1], []):
        with pytest.raises(ValueError):
            ops.scene_accumulate_group(group, scenes, d["feats"][:2], d["mapped"][:2], d["bias"], d["rgb"][:2], d["proj"][:2], d["rgb_proj"][:2])
    with pytest.raises(ValueError, match="same"):      # 3 views for 2 scenes
        ops.scene_accumulate_group(group, None, d["feats"][:3], d["mapped"][:3], d["bias"], d["rgb"][:3], d["proj"][:3], d["rgb_proj"][:3])
    for a, b in zip(before, _snapshot(group)):
        assert all(torch.equal(x, y) for x, y in zip(a, b)), "a refused call changed a state"
    assert group.n_views == [0, 2]
    _assert_states(group, refs, "after refused calls")


# ---- detector level ----
def _det_scenes(device, seeds, n_v=10):
    from test_detector_gpu import _scene, _small_detector
    det = _small_detector(device)
    scenes = []
    for i, seed in enumerate(seeds):
        img, dn, meta, rays = _scene(device, seed, n_v=n_v)
        meta["lidar2img"]["origin"] = np.asarray(meta["lidar2img"]["origin"], dtype=np.float32) + np.float32([0.2 * i, -0.1 * i, 0.0])
        ext = meta["lidar2img"]["extrinsic"]            # its own cameras too: the ring turned by 3 i places, so that the scenes' chunks
        meta["lidar2img"]["extrinsic"] = ext[3 * i:] + ext[:3 * i]      # of one call never share a projection
        scenes.append((img, dn, meta, rays))
    return det, scenes


def _group_feed(group, scenes, rows, sizes):
    for v0, v1 in _splits(scenes[0][0].shape[1], sizes):
        group.add_views(torch.cat([scenes[s][0][:, v0:v1] for s in rows]), torch.cat([scenes[s][1][:, v0:v1] for s in rows]),
                        [_chunk_meta(scenes[s][2], v0, v1) for s in rows], scenes=rows)


def test_group_of_one_equals_stream_and_simple_test(device):
    det, scenes = _det_scenes(device, [4])
    img, dn, meta, rays = scenes[0]
    want = _one_shot(det, img, dn, meta, rays)
    assert len(want["scores_3d"]) > 5
    group = det.begin_scenes([dict(meta)])
    _group_feed(group, scenes, [0], [10])
    assert group.n_views == [10]
    got = group.detect()
    assert isinstance(got, list) and len(got) == 1
    _same(got[0], _stream(det, img, dn, meta, [10]).detect())
    _same(got[0], want)
    (vol, valid), = group.volume()
    svol, svalid = _stream(det, img, dn, meta, [10]).volume()
    assert torch.equal(vol, svol) and torch.equal(valid, svalid)


def test_group_of_three_matches_separate_streams(device):
    from nerfdet_amd import conv3d as C
    det, scenes = _det_scenes(device, [4, 5, 6])
    before = C.guard_trips
    group = det.begin_scenes([dict(sc[2]) for sc in scenes])
    _group_feed(group, scenes, [0, 1, 2], [5, 5])
    assert group.n_views == [10, 10, 10]
    streams = [_stream(det, img, dn, meta, [5, 5]) for img, dn, meta, _ in scenes]
    want = [s.detect() for s in streams]
    assert all(len(w[0]["scores_3d"]) > 5 for w in want)
    got = group.detect()
    assert len(got) == 3
    for g, w in zip(got, want):
        _close(g, w)
    _close(group.detect(scenes=[1])[0], want[1])
    sub = group.detect(scenes=[2, 0])
    _close(sub[0], want[2])
    _close(sub[1], want[0])
    # the state is the scene's own whatever the batch: counts are exact, and detect() leaves the states alone
    for st, s in zip(group.group.states, streams):
        assert torch.equal(st.k1_count, s.state.k1_count) and torch.equal(st.k2_count, s.state.k2_count)
    for (vol, valid), s in zip(group.volume(), streams):
        assert torch.equal(valid, s.volume()[1])
    # reset(scenes=[0]) empties scene 0 only
    group.reset(scenes=[0])
    assert group.n_views == [0, 10, 10] and not group.group.states[0].k1_sum.any() and not group.group.states[0].k2_count.any()
    with pytest.raises(ValueError, match="no views"):
        group.detect()
    with pytest.raises(ValueError, match="no views"):
        group.volume(scenes=[0])
    rest = group.detect(scenes=[1, 2])
    _close(rest[0], want[1])
    _close(rest[1], want[2])
    # a subset call refills it: cameras do not tick together
    _group_feed(group, scenes, [0], [5, 5])
    _close(group.detect(scenes=[0])[0], want[0])
    assert C.guard_trips == before, "an ordinary scene must stay on the fp16-pair arithmetic"


def test_group_guard_trip_redoes_the_call_on_bf16x3(device):
    """cfg2's detector with the bright region of test_adversarial_gpu in scene 0's chunk: the call's backbone is redone on bf16x3 before any state
    is touched, once for the call; a plain call trips nothing."""
    from nerfdet_amd import conv3d as C
    from test_adversarial_gpu import _adversarial_detector, _bench
    bench = _bench()
    w = bench.WORKLOADS["cfg2"]
    det = _adversarial_detector(bench, w).to(device)
    batch = bench.to_device(bench.synth_batch(w, 0), device)
    meta = batch["img_metas"][0]
    img, dn = batch["img"].clone(), batch["denorm_images"]
    img[:, :4, :, 60:140, 100:220] *= 1.0e6
    metas = [dict(meta), dict(meta)]
    call = lambda g, v: g.add_views(torch.cat([img[:, v:v + 5], img[:, v + 5:v + 10]]), torch.cat([dn[:, v:v + 5], dn[:, v + 5:v + 10]]),
                                    [_chunk_meta(meta, v, v + 5), _chunk_meta(meta, v + 5, v + 10)])
    assert C.ARITHMETIC == "f16x2"
    with torch.no_grad():
        before = C.guard_trips
        group = det.begin_scenes(metas)
        call(group, 0)
        assert C.guard_trips == before + 1, "the bright call was not redone, or was counted per scene"
        exact = det.begin_scenes(metas)
        prev = C.set_arithmetic("bf16x3")
        try:
            call(exact, 0)
        finally:
            C.set_arithmetic(prev)
        assert C.guard_trips == before + 1
        for st, ref in zip(group.group.states, exact.group.states):
            for t in TENSORS:
                assert torch.equal(getattr(st, t), getattr(ref, t)), f"{t}: the states do not hold the bf16x3 features"
        call(group, 10)
        assert C.guard_trips == before + 1, "a plain call tripped the guard"
        assert group.n_views == [10, 10]


def _same_bits(a, b):
    """``_same`` on the bit patterns: the blown-up scene's boxes may hold inf and NaN, which must match too (NaN != NaN under torch.equal)."""
    assert torch.equal(a["labels_3d"], b["labels_3d"])
    for x, y in ((a["scores_3d"], b["scores_3d"]), (a["boxes_3d"].tensor, b["boxes_3d"].tensor)):
        assert x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


@pytest.mark.parametrize("fused", [True, False])
def test_group_detect_guard_trip_repeats_the_call_on_bf16x3(device, fused, monkeypatch):
    """A few voxels of scene 1's feature sums made 1e10 times larger: neck_3d's first fp16-pair launch on that volume raises the guard word.  No
    f16x2 result may get out: the call is repeated on bf16x3 from the finished volumes, counted once.  The group's states are copies of two
    streams' states, so every scene must come out as its stream's own detect() does, bit for bit -- the tripped scene through the stream's
    repeat, the other one through a repeat its stream did not need (checked against the stream's own repeat).  ``fused=False``: a head that
    cannot take the fused tail does not carry the word with its picks; the group then reads it once."""
    from nerfdet_amd import conv3d as C
    det, scenes = _det_scenes(device, [4, 5])
    if not fused:
        monkeypatch.setattr(det.bbox_head, "can_fuse", lambda x: False)
    streams = [_stream(det, img, dn, meta, [10]) for img, dn, meta, _ in scenes]
    group = det.begin_scenes([dict(sc[2]) for sc in scenes])
    seen = torch.nonzero(streams[1].state.k1_count)[:8, 0]
    assert len(seen) == 8
    streams[1].state.k1_sum[seen] *= 1.0e10
    for st, s in zip(group.group.states, streams):
        for t in TENSORS:
            getattr(st, t).copy_(getattr(s.state, t))
        st.n_views = s.state.n_views
    assert C.ARITHMETIC == "f16x2"
    before = C.guard_trips
    plain = streams[0].detect()
    assert C.guard_trips == before, "the ordinary scene must not trip"
    want1 = streams[1].detect()
    assert C.guard_trips == before + 1, "the test's scene did not trip the guard in detect()"
    vol0, valid0 = streams[0].volume()
    want0 = streams[0]._repeat_tail(vol0, valid0, [dict(scenes[0][2])])      # the stream's own bf16x3 repeat from its finished volume
    _close(want0, plain)
    before = C.guard_trips
    got = group.detect()
    assert C.guard_trips == before + 1, "the tripped call was not repeated, or was counted per scene"
    _same_bits(got[1], want1[0])
    _same(got[0], want0)
    # scene 0 alone trips nothing and stays on the fp16-pair arithmetic
    _same(group.detect(scenes=[0])[0], plain)
    assert C.guard_trips == before + 1
