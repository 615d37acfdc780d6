"""GPU checks of windowed scene groups (nerf-det_amd/streaming.py::SceneGroup(window=), ops.SceneGroupRingState, scene_accumulate_group_ring /
density_finish_group_ring / volume_finish_group_ring): every state a grouped call fills through its front table against ops.scene_accumulate
into a fresh state, the grouped ring finishes against the single-scene ring finishes -- all bit for bit -- and a windowed SceneGroup against
windowed SceneStreams."""
import numpy as np
import pytest
import torch

from test_scene_group_gpu import FAR_ORIGINS, ORIGINS, TENSORS, _det_scenes, _scenes, _views
from test_streaming_gpu import _chunk_meta, _close, _gate, _same

pytestmark = pytest.mark.gpu


def _new_pool(ds, window):
    from nerfdet_amd import ops
    d0 = ds[0]
    return ops.SceneGroupRingState(d0["grid"], d0["feats"].shape[1], d0["mapped"].shape[1], [d["points"] for d in ds], window, d0["feats"].device)


def _feed(pool, refs, ds, listed, v0, v1, gated):
    """The views v0 .. v1 of every listed scene as one chunk each: one grouped call into the pool, and per scene the same slices through
    ops.scene_accumulate into a fresh state that joins ``refs[s]`` (a list per scene, kept as the pool keeps its windows)."""
    from nerfdet_amd import ops
    d0 = ds[0]
    bias = d0["bias"]
    rows = listed if listed is not None else list(range(len(ds)))
    cat = lambda key: torch.cat([_views(ds[s], key, v0, v1) for s in rows])
    gate = ops.depth_gate(cat("depth"), d0["vs"], (d0["h"], d0["w"]), d0["hw"]) if gated else None
    ops.scene_accumulate_group_ring(pool, listed, cat("feats"), cat("mapped"), bias, cat("rgb"), cat("proj"), cat("rgb_proj"), depth_gate=gate)
    if refs is None:
        return
    for s in rows:
        d = ds[s]
        st = ops.SceneState(d0["grid"], d0["feats"].shape[1], d0["mapped"].shape[1], d0["feats"].device)
        ops.scene_accumulate(st, _views(d, "feats", v0, v1), _views(d, "mapped", v0, v1), bias, _views(d, "rgb", v0, v1), d["points"],
                             _views(d, "proj", v0, v1), _views(d, "rgb_proj", v0, v1), depth_gate=_gate(d, v0 + d["shift"], v1 + d["shift"], gated))
        if len(refs[s]) == pool.window:
            del refs[s][0]
        refs[s].append(st)


def _snapshot(pool):
    return [[getattr(st, t).clone() for t in TENSORS] for st in pool.states]


def _unchanged(pool, before, what):
    for st, a in zip(pool.states, before):          # states allocated since the snapshot are not in it
        assert all(torch.equal(getattr(st, t), x) for t, x in zip(TENSORS, a)), what


def _assert_states(pool, refs, what):
    assert pool.n_chunks == [len(r) for r in refs] and pool.chunk_views == [[st.n_views for st in r] for r in refs], what
    for s, (segs, ref) in enumerate(zip(pool.segs, refs)):
        for j, (st, want) in enumerate(zip(segs, ref)):
            for t in TENSORS:
                assert torch.equal(getattr(st, t), getattr(want, t)), \
                    f"{what}: scene {s} segment {j}'s {t} differs from ops.scene_accumulate into a fresh state"


def _assert_finishes(pool, bias, listed, seed=3):
    """The grouped ring finishes over the listed scenes against the single-scene ring finishes over each scene's list."""
    from nerfdet_amd import ops
    rows_of = listed if listed is not None else list(range(len(pool)))
    n_vox, n = pool.n_voxels, len(rows_of)
    before = _snapshot(pool)
    rows = ops.density_finish_group_ring(pool, bias, listed)
    assert rows.shape == (n * n_vox, 2 * (3 + pool.cm))
    alpha = torch.rand(n * n_vox, generator=torch.Generator().manual_seed(seed)).to(rows.device)
    mean, cnt = ops.volume_finish_group_ring(pool, None, listed)
    vol, cnt2 = ops.volume_finish_group_ring(pool, alpha, listed)
    assert mean.shape == (n, pool.c) + pool.grid and cnt.shape == (n, 1) + pool.grid and cnt.dtype == torch.int64
    for i, s in enumerate(rows_of):
        segs = pool.segs[s]
        a = alpha[i * n_vox:(i + 1) * n_vox]
        assert torch.equal(rows[i * n_vox:(i + 1) * n_vox], ops.density_finish_ring(segs, bias)), f"density rows of scene {s} (listed {i})"
        want_mean, want_cnt = ops.volume_finish_ring(segs)
        want_vol, _ = ops.volume_finish_ring(segs, a)
        assert torch.equal(mean[i], want_mean) and torch.equal(vol[i], want_vol), f"volume of scene {s} (listed {i})"
        assert torch.equal(cnt[i], want_cnt) and torch.equal(cnt2[i], want_cnt), f"counts of scene {s} (listed {i})"
        assert mean[i].stride() == want_mean.stride() and vol[i].stride() == want_vol.stride()      # channels-last, as neck_3d takes it
        if len(segs) == 1:
            assert torch.equal(rows[i * n_vox:(i + 1) * n_vox], ops.density_finish(segs[0], bias))
            one_mean, one_cnt = ops.volume_finish(segs[0])
            assert torch.equal(mean[i], one_mean) and torch.equal(cnt[i], one_cnt) and torch.equal(vol[i], ops.volume_finish(segs[0], a)[0])
    _unchanged(pool, before, "finishing changed a state")
    assert len(before) == len(pool.states)


@pytest.mark.parametrize("gated,c", [(False, 64), (True, 64), (False, 320), (True, 320)])
def test_group_ring_finishes_match_single_scene_ring_finishes(device, gated, c):
    """S = 3, N = 315 (a ragged tail for the 256-thread blocks), windows of 1, 3 and 6 segments: no trip of the segment loop, a partial
    batch of 4, a full batch and a padded one.  Chunks of 1 to 3 views; c = 320 takes the accumulate's NCHUNK = 2."""
    from nerfdet_amd import ops
    ds = _scenes(device, 12, ORIGINS, seed0=41, grid=(7, 9, 5), c=c)
    pool, refs = _new_pool(ds, 8), [[], [], []]
    bias = ds[0]["bias"]
    _feed(pool, refs, ds, None, 0, 2, gated)                # k = 2, every scene
    _assert_states(pool, refs, "k=2, all scenes")
    _feed(pool, refs, ds, [2, 0], 2, 5, gated)              # k = 3, a subset, listed order against scene order
    _assert_states(pool, refs, "k=3, scenes [2, 0]")
    pool.drop_oldest(1, [0])                                # scene 0 keeps its second chunk only
    del refs[0][0]
    _feed(pool, refs, ds, [1, 2], 5, 6, gated)              # k = 1
    _feed(pool, refs, ds, [2, 1], 6, 8, gated)
    _feed(pool, refs, ds, [2], 8, 9, gated)
    _feed(pool, refs, ds, [2], 9, 12, gated)
    _assert_states(pool, refs, "after six calls")
    assert pool.n_chunks == [1, 3, 6] and pool.n_views == [3, 5, 12]
    assert pool.chunk_views == [[3], [2, 1, 2], [2, 3, 1, 2, 1, 3]]
    # what the comparison needs to see: seen and unseen voxels in every scene, and in the 6-segment scene voxels that some segment sees and
    # another does not (the rows the kernels skip), in K1's counts and in both of K2's
    for s, segs in enumerate(pool.segs):
        seen = int((sum(st.k1_count for st in segs) != 0).sum())
        assert 0 < seen < pool.n_voxels, f"scene {s}: {seen} of {pool.n_voxels} voxels seen -- the case needs seen and unseen voxels"
    k1 = torch.stack([st.k1_count for st in pool.segs[2]])
    k2 = torch.stack([st.k2_count for st in pool.segs[2]])
    mixed1, mixed2 = (k1 == 0).any(0) & (k1 != 0).any(0), (k2 == 0).any(0) & (k2 != 0).any(0)
    assert bool(mixed1.any()) and bool(mixed2[:, 0].any()) and bool(mixed2[:, 1].any()), "no voxel that one segment sees and another does not"
    _assert_finishes(pool, bias, None)
    _assert_finishes(pool, bias, [2, 0])
    _assert_finishes(pool, bias, [1])
    # the comparison can see the order of the adds
    fwd, _ = ops.volume_finish_ring(pool.segs[2])
    rev, _ = ops.volume_finish_ring(pool.segs[2][::-1])
    assert not torch.equal(fwd, rev), "reversing the 6 segments changed no bit: the case cannot see the summation order"
    if gated:
        loose = _new_pool(ds, 8)
        _feed(loose, None, ds, None, 0, 2, False)
        assert all(int(a[0].k1_count.sum()) < int(b[0].k1_count.sum()) for a, b in zip(refs[1:], loose.segs[1:])), "the gate dropped nothing"


def test_group_ring_two_view_rounds(device):
    """k = 70: two 64-view rounds in K1's walk and in the packed K2 walk, through the front table; two segments a scene."""
    ds = _scenes(device, 70, FAR_ORIGINS, seed0=51, hw=(32, 48), grid=(8, 8, 4))
    pool, refs = _new_pool(ds, 2), [[], []]
    _feed(pool, refs, ds, [1, 0], 0, 70, False)
    _feed(pool, refs, ds, [1, 0], 3, 8, False)
    _assert_states(pool, refs, "k=70 then k=5")
    assert pool.chunk_views == [[70, 5], [70, 5]]
    _assert_finishes(pool, ds[0]["bias"], [1, 0])
    _assert_finishes(pool, ds[0]["bias"], None)
    for s, segs in enumerate(pool.segs):
        seen = int((segs[0].k1_count != 0).sum())
        assert 0 < seen < pool.n_voxels and int(segs[0].k1_count.max()) > 64, f"scene {s}: {seen} voxels seen, at most {int(segs[0].k1_count.max())} views"


def test_a_dropped_chunk_leaves_no_trace(device):
    """A window of 2 slid over 4 rounds of 2 views, the scenes served in different rounds, against a fresh pool fed only the chunks each
    scene still holds."""
    from nerfdet_amd import ops
    ds = _scenes(device, 8, ORIGINS, seed0=61, grid=(7, 9, 5))
    pool, refs = _new_pool(ds, 2), [[], [], []]
    served = [None, [2, 0], [1, 2], [0, 2]]
    held = [[], [], []]
    for r, listed in enumerate(served):
        _feed(pool, refs, ds, listed, 2 * r, 2 * r + 2, r % 2 == 1)
        for s in (listed if listed is not None else [0, 1, 2]):
            held[s] = (held[s] + [r])[-2:]
        assert all(pool.owned(s) <= 3 for s in range(3))
    assert held == [[1, 3], [0, 2], [2, 3]] and pool.n_chunks == [2, 2, 2]
    _assert_states(pool, refs, "after four rounds")
    fresh = _new_pool(ds, 2)
    for s in (1, 0, 2):
        for r in held[s]:
            _feed(fresh, None, ds, [s], 2 * r, 2 * r + 2, r % 2 == 1)
    assert len(fresh.states) == 6 and len(pool.states) <= 9
    bias = ds[0]["bias"]
    alpha = torch.rand(3 * pool.n_voxels, generator=torch.Generator().manual_seed(5)).to(device)
    assert torch.equal(ops.density_finish_group_ring(pool, bias), ops.density_finish_group_ring(fresh, bias))
    for got, want in zip(ops.volume_finish_group_ring(pool, alpha), ops.volume_finish_group_ring(fresh, alpha)):
        assert torch.equal(got, want)
    _assert_finishes(pool, bias, [2, 0])


# ---- detector level ----
def _group_add(group, scenes, rows, v0, v1):
    group.add_views(torch.cat([scenes[s][0][:, v0:v1] for s in rows]), torch.cat([scenes[s][1][:, v0:v1] for s in rows]),
                    [_chunk_meta(scenes[s][2], v0, v1) for s in rows], scenes=rows)


def test_windowed_group_of_one_equals_windowed_stream(device):
    det, scenes = _det_scenes(device, [4], n_v=16)
    img, dn, meta, _ = scenes[0]
    group = det.begin_scenes([dict(meta)], window=3)
    stream = det.begin_scene(dict(meta), window=3)
    assert group.window == 3 and (group.n_views, group.n_chunks, group.chunk_views) == ([0], [0], [[]])
    for v0 in range(0, 16, 4):                              # the fourth chunk evicts the first
        _group_add(group, scenes, [0], v0, v0 + 4)
        stream.add_views(img[:, v0:v0 + 4], dn[:, v0:v0 + 4], _chunk_meta(meta, v0, v0 + 4))
    assert group.chunk_views == [stream.chunk_views] == [[4, 4, 4]] and group.n_views == [12] and group.n_chunks == [3]
    want = stream.detect()
    assert len(want[0]["scores_3d"]) > 5
    got = group.detect()
    assert isinstance(got, list) and len(got) == 1
    _same(got[0], want)
    (vol, valid), = group.volume()
    svol, svalid = stream.volume()
    assert torch.equal(vol, svol) and torch.equal(valid, svalid) and vol.stride() == svol.stride()
    assert group.pool.owned(0) == 4


ROUNDS = [((0, 4), [0, 1, 2]), ((4, 8), [2, 0]), ((8, 12), [0, 1, 2])]


@pytest.fixture(scope="module")
def three(device):
    """Three scenes and, once for the tests below, three separate windowed streams fed ROUNDS' chunks, with their detections."""
    det, scenes = _det_scenes(device, [4, 5, 6], n_v=12)
    streams = [det.begin_scene(dict(sc[2]), window=2) for sc in scenes]
    for (v0, v1), rows in ROUNDS:
        for s in rows:
            img, dn, meta, _ = scenes[s]
            streams[s].add_views(img[:, v0:v1], dn[:, v0:v1], _chunk_meta(meta, v0, v1))
    want = [s.detect() for s in streams]
    assert all(len(w[0]["scores_3d"]) > 5 for w in want)
    return det, scenes, streams, want


def _assert_matches_streams(group, streams, want):
    assert group.n_chunks == [s.n_chunks for s in streams] == [2, 2, 2]
    assert group.chunk_views == [s.chunk_views for s in streams] and group.n_views == [s.n_views for s in streams] == [8, 8, 8]
    got = group.detect()
    assert len(got) == 3
    for g, w in zip(got, want):
        _close(g, w)                    # the chunking contract: same labels in the same order, scores and boxes to 1e-4


def test_windowed_group_of_three_matches_separate_windowed_streams(three, monkeypatch):
    from nerfdet_amd import conv3d as C, trace
    det, scenes, streams, want = three
    before = C.guard_trips
    group = det.begin_scenes([dict(sc[2]) for sc in scenes], window=2)
    for (v0, v1), rows in ROUNDS:
        _group_add(group, scenes, rows, v0, v1)
    _assert_matches_streams(group, streams, want)
    # one detect: two finish launches and one sigma-MLP call, whatever the number of scenes
    mlp_calls = []
    for name in ("alpha_from_points", "raw_sigma_from_rows"):
        if hasattr(det.nerf_mlp, name):
            monkeypatch.setattr(det.nerf_mlp, name, (lambda f: lambda *a, **k: (mlp_calls.append(1), f(*a, **k))[1])(getattr(det.nerf_mlp, name)))
    monkeypatch.setattr(trace, "recorder", trace.Recorder())
    group.detect()
    finishes = [sp[0] for sp in trace.recorder.spans if sp[0].startswith(("k_density_finish", "k_volume_finish"))]
    monkeypatch.undo()
    assert sorted(finishes) == ["k_density_finish_group_ring", "k_volume_finish_group_ring"] and len(mlp_calls) == 1
    sub = group.detect(scenes=[2, 0])
    _close(sub[0], want[2])
    _close(sub[1], want[0])
    # counts are exact whatever the batch
    for segs, s in zip(group.pool.segs, streams):
        for st, ref in zip(segs, s._segs):
            assert torch.equal(st.k1_count, ref.k1_count) and torch.equal(st.k2_count, ref.k2_count)
    # given equal states, detect is the stream's bit for bit
    for segs, s in zip(group.pool.segs, streams):
        for st, ref in zip(segs, s._segs):
            for t in TENSORS:
                getattr(st, t).copy_(getattr(ref, t))
    for g, w in zip(group.detect(), want):
        _same(g, w)
    _same(group.detect(scenes=[1])[0], want[1])
    assert C.guard_trips == before, "an ordinary scene must stay on the fp16-pair arithmetic"
    assert all(group.pool.owned(s) <= 3 for s in range(3))


def test_refused_calls_leave_the_windows_as_they_were(three):
    from nerfdet_amd import ops
    det, scenes, streams, want = three
    device = scenes[0][0].device
    group = det.begin_scenes([dict(sc[2]) for sc in scenes], window=2)
    for (v0, v1), rows in ROUNDS[:2]:
        _group_add(group, scenes, rows, v0, v1)
    pool = group.pool
    assert group.chunk_views == [[4, 4], [4], [4, 4]]
    before, segs, views = _snapshot(pool), [list(s) for s in pool.segs], group.chunk_views

    def untouched(what):
        _unchanged(pool, before, what)
        assert group.chunk_views == views and all(len(a) == len(b) and all(x is y for x, y in zip(a, b)) for a, b in zip(pool.segs, segs)), what
        for st in pool.states[len(before):]:            # a state the refused call took: back among the spares, zeroed
            assert st.n_views == 0 and not any(bool(getattr(st, t).any()) for t in TENSORS), what
            assert any(st is x for x in pool.spare[pool.owner[st.row]]), what

    rows = [0, 1, 2]
    cat = lambda j: torch.cat([scenes[s][j][:, 8:12] for s in rows])
    with pytest.raises(ValueError, match="extrinsics"):
        group.add_views(cat(0), cat(1), [_chunk_meta(scenes[s][2], 8, 12 if s else 11) for s in rows])
    untouched("a chunk meta with the wrong number of views")
    for bad in ([0, 0, 1], [0, 1, 3]):
        with pytest.raises(ValueError):
            group.add_views(cat(0), cat(1), [_chunk_meta(scenes[s][2], 8, 12) for s in rows], scenes=bad)
    untouched("a bad scenes list")
    c, cm = pool.c, pool.cm
    g = torch.Generator().manual_seed(7)
    proj = ops.compute_projection(_chunk_meta(scenes[1][2], 8, 10), 4, device)
    with pytest.raises(AssertionError, match=f"C={c}"):
        ops.scene_accumulate_group_ring(pool, [1, 0], torch.randn(4, c + 4, 16, 24, generator=g).to(device), torch.randn(4, cm, 16, 24, generator=g).to(device),
                                        torch.zeros(cm, device=device), torch.rand(4, 3, 64, 96, generator=g).to(device), torch.cat([proj, proj]),
                                        torch.cat([proj, proj]))
    assert len(pool.states) == len(before) + 2          # scene 0's window was full, scene 1 had no spare: both states were allocated
    untouched("an accumulate with mismatched C")
    (v0, v1), rows = ROUNDS[2]
    _group_add(group, scenes, rows, v0, v1)
    _assert_matches_streams(group, streams, want)


def test_windowed_group_guard_trip_redoes_the_call_on_bf16x3(device):
    """test_scene_group_gpu's guard case on a windowed group: the bright call's backbone is redone on bf16x3 before any window changes, once
    for the call, and the windows gain exactly one chunk per listed scene."""
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
        group = det.begin_scenes(metas, window=2)
        call(group, 0)
        assert C.guard_trips == before + 1, "the bright call was not redone, or was counted per scene"
        assert group.chunk_views == [[5], [5]]
        exact = det.begin_scenes(metas, window=2)
        prev = C.set_arithmetic("bf16x3")
        try:
            call(exact, 0)
        finally:
            C.set_arithmetic(prev)
        assert C.guard_trips == before + 1
        for segs, refs in zip(group.pool.segs, exact.pool.segs):
            for t in TENSORS:
                assert torch.equal(getattr(segs[0], t), getattr(refs[0], t)), f"{t}: the states do not hold the bf16x3 features"
        call(group, 10)
        assert C.guard_trips == before + 1, "a plain call tripped the guard"
        assert group.chunk_views == [[5, 5], [5, 5]] and group.n_views == [10, 10] and len(group.pool.states) == 4
