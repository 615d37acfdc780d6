"""SceneGroup.detect(batched=True) (nerf-det_amd/streaming.py): the finished volumes of the listed scenes through neck_3d and the head's convolutions
as ONE batch -- FastIndoorImVoxelNeck.forward_batched and ScanNetImVoxelHeadV2.raws_batched, one ndet_conv_split_batch launch per layer and
level -- then every scene's own tail.  The reference runs the same modules on a batch axis (mmdet3d/models/necks/imvoxelnet.py:22-67,233-260,
dense_heads/imvoxel_head_v2.py:45-49,216-285).  The scenes of a batched call share the 3D part's fp16-pair scales, so the contract is the
chunking contract (``_close``: same labels in the same order, scores and boxes to 1e-4); everything that does not go through a shared scale is
held to bits."""
import pytest
import torch

from test_group_window_gpu import ROUNDS, _group_add
from test_scene_group_gpu import TENSORS, _det_scenes, _group_feed, _same_bits
from test_streaming_gpu import _chunk_meta, _close, _same, _stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def three(device):
    """Three scenes in one group and, once for the tests below, three separate streams with their detections."""
    det, scenes = _det_scenes(device, [4, 5, 6])
    group = det.begin_scenes([dict(sc[2]) for sc in scenes])
    _group_feed(group, scenes, [0, 1, 2], [5, 5])
    want = [_stream(det, img, dn, meta, [5, 5]).detect() for img, dn, meta, _ in scenes]
    assert all(len(w[0]["scores_3d"]) > 5 for w in want)
    return det, scenes, group, want


def _count(fn):
    """(result, names of the convolution launches ``fn()`` made)."""
    from nerfdet_amd import conv3d as C
    names = []

    def hook(flops, thunk, name):
        names.append(name)
        return thunk()
    prev = C.launch_hook
    try:
        C.launch_hook = hook
        out = fn()
    finally:
        C.launch_hook = prev
    return out, names


def test_batched_detect_agrees_with_separate_streams(three):
    from nerfdet_amd import conv3d as C
    det, scenes, group, want = three
    before = C.guard_trips
    snapshot = [[getattr(st, t).clone() for t in TENSORS] for st in group.group.states]
    got = group.detect(batched=True)
    assert len(got) == 3
    for g, w in zip(got, want):
        _close(g, w)
    sub = group.detect(scenes=[2, 0], batched=True)
    assert len(sub) == 2
    _close(sub[0], want[2])
    _close(sub[1], want[0])
    assert C.guard_trips == before, "an ordinary batched call must stay on the fp16-pair arithmetic"
    for st, snap in zip(group.group.states, snapshot):          # detect leaves the states alone, batched or not
        assert all(torch.equal(getattr(st, t), s) for t, s in zip(TENSORS, snap))


def test_batched_detect_of_a_windowed_group(device):
    det, scenes = _det_scenes(device, [4, 5, 6], n_v=12)
    streams = [det.begin_scene(dict(sc[2]), window=2) for sc in scenes]
    group = det.begin_scenes([dict(sc[2]) for sc in scenes], window=2)
    for (v0, v1), rows in ROUNDS:
        _group_add(group, scenes, rows, v0, v1)
        for s in rows:
            streams[s].add_views(scenes[s][0][:, v0:v1], scenes[s][1][:, v0:v1], _chunk_meta(scenes[s][2], v0, v1))
    want = [s.detect() for s in streams]
    assert all(len(w[0]["scores_3d"]) > 5 for w in want)
    for g, w in zip(group.detect(batched=True), want):
        _close(g, w)
    sub = group.detect(scenes=[2, 0], batched=True)
    _close(sub[0], want[2])
    _close(sub[1], want[0])


def test_batched_detect_is_one_launch_per_layer(three):
    """As many convolution launches for three scenes as for one (the sigma MLP's, which serve all the listed scenes in any case, included); the
    unbatched call makes neck_3d's and the head's three times."""
    det, scenes, group, want = three
    _, mlp = _count(lambda: group.volume())                      # what comes before neck_3d: the same launches for any number of scenes
    _, one = _count(lambda: group.detect(scenes=[1]))
    _, bat = _count(lambda: group.detect(batched=True))
    _, unb = _count(lambda: group.detect())
    neck_head = len(one) - len(mlp)
    assert neck_head >= 10, (len(one), len(mlp))
    assert len(bat) == len(one), (len(bat), len(one))
    assert len(unb) - len(mlp) == 3 * neck_head, (len(unb), len(mlp), neck_head)
    assert sum(nm.endswith("/batch") for nm in bat) == neck_head and not any(nm.endswith("/batch") for nm in one + unb)


def test_batched_detect_of_one_scene_is_the_unbatched_call(three):
    det, scenes, group, want = three
    _same(group.detect(scenes=[1], batched=True)[0], group.detect(scenes=[1]))
    _, names = _count(lambda: group.detect(scenes=[1], batched=True))
    assert not any(nm.endswith("/batch") for nm in names)


@pytest.mark.parametrize("fused", [True, False])
def test_batched_detect_guard_trip_is_the_unbatched_repeat(device, fused, monkeypatch):
    """The 1e10-voxel setup of test_group_detect_guard_trip_repeats_the_call_on_bf16x3: the batched call trips once, is repeated by the same
    per-scene bf16x3 repeat and returns the unbatched tripped call's results bit for bit; an ordinary batched call trips nothing."""
    from nerfdet_amd import conv3d as C
    det, scenes = _det_scenes(device, [4, 5])
    if not fused:
        monkeypatch.setattr(det.bbox_head, "can_fuse", lambda x: False)
    streams = [_stream(det, img, dn, meta, [10]) for img, dn, meta, _ in scenes]
    group = det.begin_scenes([dict(sc[2]) for sc in scenes])
    plain = det.begin_scenes([dict(sc[2]) for sc in scenes])
    for g in (group, plain):
        for st, s in zip(g.group.states, streams):
            for t in TENSORS:
                getattr(st, t).copy_(getattr(s.state, t))
            st.n_views = s.state.n_views
    seen = torch.nonzero(group.group.states[1].k1_count)[:8, 0]
    assert len(seen) == 8
    group.group.states[1].k1_sum[seen] *= 1.0e10
    assert C.ARITHMETIC == "f16x2"
    before = C.guard_trips
    ordinary = plain.detect(batched=True)
    assert C.guard_trips == before, "an ordinary batched call tripped the guard"
    for g, s in zip(ordinary, streams):
        _close(g, s.detect())
    assert C.guard_trips == before
    want = group.detect()
    assert C.guard_trips == before + 1, "the test's scene did not trip the unbatched call"
    got = group.detect(batched=True)
    assert C.guard_trips == before + 2, "the tripped batched call was not repeated, or was counted per scene"
    for g, w in zip(got, want):
        _same_bits(g, w)


def test_batched_detect_on_bf16x3_and_f32(three):
    """bf16x3 set globally: the batched launches run in that arithmetic (exact operands, no shared scale left) and agree with the unbatched call;
    "f32" has no batched kernels: batched=True falls back to the unbatched path."""
    from nerfdet_amd import conv3d as C
    det, scenes, group, want = three
    prev = C.set_arithmetic("bf16x3")
    try:
        unb = group.detect()
        bat, names = _count(lambda: group.detect(batched=True))
    finally:
        C.set_arithmetic(prev)
    assert any(nm.endswith("/batch") for nm in names) and not any("/f16x2" in nm for nm in names)
    for b, u in zip(bat, unb):
        _close(b, u)
    prev = C.set_arithmetic("f32")
    try:
        unb = group.detect()
        bat, names = _count(lambda: group.detect(batched=True))
    finally:
        C.set_arithmetic(prev)
    assert not any(nm.endswith("/batch") for nm in names)
    for b, u in zip(bat, unb):
        _same(b, u)
