"""Sliding-window streaming without a GPU: the ring finishes (ndet_scene_density_finish_ring / ndet_scene_volume_finish_ring) reject a bad
segment list or output before any HIP call and name the field and the segment at fault; SceneStream rejects a bad window and
``drop_oldest`` on an unwindowed stream."""
import ctypes

import pytest


def _seg(**bad):
    from nerfdet_amd import _lib
    fields = dict(size=ctypes.sizeof(_lib.NdetSceneAccum), N=64, C=32, cm=8, n_views=3, k1_sum=0x1000, k1_pitch=32, k1_count=0x2000,
                  k2_sum=0x3000, k2_pitch=36, k2_count=0x4000)
    fields.update(bad)
    return _lib.NdetSceneAccum(**fields)


def _ring(*segs):
    from nerfdet_amd import _lib
    return (_lib.NdetSceneAccum * len(segs))(*segs)


def test_ring_finishes_are_bound():
    from nerfdet_amd import _lib, ops
    lib = _lib.load()
    for name in ("ndet_scene_density_finish_ring", "ndet_scene_volume_finish_ring"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert ops.RING_MAX == 64


def test_ring_finishes_reject_bad_arguments_without_a_gpu():
    from nerfdet_amd import _lib
    lib = _lib.load()
    f = ctypes.c_void_p(0x1000)

    def dfin(segs, n, bias=f, out=f):
        return lib.ndet_scene_density_finish_ring(segs, n, bias, out, None)

    def vfin(segs, n, out=f, count=f):
        return lib.ndet_scene_volume_finish_ring(segs, n, None, out, count, None)

    def err():
        return lib.ndet_last_error()

    for call in (dfin, vfin):
        assert call(None, 1) == -1 and b"null segs" in err()
        three = _ring(_seg(), _seg(), _seg())
        assert call(three, 0) == -1 and b"n_segs=0" in err()
        assert call(three, 65) == -1 and b"n_segs=65" in err()
        assert call(three, -1) == -1 and b"n_segs" in err()
        # one bad block in the list: the message names what is wrong and which segment
        assert call(_ring(_seg(), _seg(size=ctypes.sizeof(_lib.NdetSceneAccum) - 8), _seg()), 3) == -1
        assert b"size" in err() and b"segs[1]" in err()
        assert call(_ring(_seg(), _seg(), _seg(k2_sum=None)), 3) == -1 and b"segs[2]" in err()
        assert call(_ring(_seg(k1_sum=0x1004), _seg()), 2) == -2 and b"segs[0]" in err()
        assert call(_ring(_seg(), _seg(C=30)), 2) == -2 and b"C=30" in err() and b"segs[1]" in err()
        # blocks that disagree
        assert call(_ring(_seg(), _seg(N=128)), 2) == -1 and b"segs[1].N=128" in err()
        assert call(_ring(_seg(), _seg(), _seg(C=64, k1_pitch=64)), 3) == -1 and b"segs[2].C=64" in err()
        assert call(_ring(_seg(), _seg(cm=16, k2_pitch=60)), 2) == -1 and b"segs[1].cm=16" in err()
        # the view total must fit int32
        assert call(_ring(_seg(n_views=0x7fffffff), _seg(n_views=0), _seg(n_views=1)), 3) == -2
        assert b"n_views" in err() and b"segs[0..2]" in err()
        assert call(_ring(_seg(n_views=0x40000000), _seg(n_views=0x40000000)), 2) == -2 and b"n_views" in err()
    # outputs
    two = _ring(_seg(), _seg())
    assert dfin(two, 2, bias=None) == -1 and b"null bias" in err()
    assert dfin(two, 2, out=None) == -1 and b"null global_feat" in err()
    assert dfin(two, 2, out=ctypes.c_void_p(0x1004)) == -2 and b"global_feat" in err()
    assert vfin(two, 2, out=None) == -1 and b"null out" in err()
    assert vfin(two, 2, count=None) == -1 and b"null count" in err()
    assert vfin(two, 2, out=ctypes.c_void_p(0x1008)) == -2 and b"out must be 16-byte aligned" in err()
    assert vfin(two, 2, count=ctypes.c_void_p(0x1004)) == -2 and b"count must be 8-byte aligned" in err()


class _Det:
    training = False
    render_testing = False


def test_window_and_drop_oldest_are_validated():
    from nerfdet_amd.detector import nerfdet
    from nerfdet_amd.streaming import SceneStream
    from nerfdet_amd.synth import ring_scene_meta
    import inspect
    meta = ring_scene_meta(4, (64, 96))
    for bad in (0, 65, -1, 2.0, True):
        with pytest.raises(ValueError, match="window"):
            SceneStream(_Det(), meta, window=bad)
    assert inspect.signature(nerfdet.begin_scene).parameters["window"].default is None
    s = SceneStream.__new__(SceneStream)          # an unwindowed stream, no device touched
    s.det, s.meta, s.window = _Det(), meta, None
    with pytest.raises(ValueError, match="windowed"):
        s.drop_oldest()
    w = SceneStream.__new__(SceneStream)          # an empty window
    w.det, w.meta, w.window, w._segs, w._spare = _Det(), meta, 2, [], []
    with pytest.raises(ValueError, match="k=1"):
        w.drop_oldest(1)
    w.drop_oldest(0)
    assert w.n_chunks == 0 and w.n_views == 0 and w.chunk_views == []
    with pytest.raises(RuntimeError):
        w.volume()


def test_a_failing_chunk_leaves_the_window_as_it_was(monkeypatch):
    """The oldest chunk leaves a full window only once the new chunk's accumulation has succeeded; the state of a chunk that fails goes
    back to the spares, zeroed."""
    import torch
    from nerfdet_amd import ops
    from nerfdet_amd.streaming import SceneStream
    from nerfdet_amd.synth import ring_scene_meta

    class Lin:
        in_features, out_features = 8, 4

    class Det(_Det):
        n_voxels = (2, 2, 2)

    def fill(state, *chunk, depth_gate=None):
        if chunk[0] == "bad":
            state.k1_sum.fill_(1.0)
            raise RuntimeError("boom")
        state.n_views += chunk[0]

    monkeypatch.setattr(ops, "scene_accumulate", fill)
    w = SceneStream.__new__(SceneStream)
    w.det, w.meta, w.window, w._segs, w._spare, w._lin, w.device = Det(), ring_scene_meta(4, (64, 96)), 2, [], [], Lin(), torch.device("cpu")
    w._accumulate(3)
    w._accumulate(5)
    assert w.chunk_views == [3, 5]
    oldest = w._segs[0]
    with pytest.raises(RuntimeError, match="boom"):
        w._accumulate("bad")
    assert w.chunk_views == [3, 5] and w._segs[0] is oldest
    assert len(w._spare) == 1 and not w._spare[0].k1_sum.any() and w._spare[0].n_views == 0
    w._accumulate(7)
    assert w.chunk_views == [5, 7] and w._spare == [oldest] and oldest.n_views == 0
    w._accumulate(2)                        # steady state: the state that left is the one filled next, nothing is allocated
    assert w.chunk_views == [7, 2] and w._segs[1] is oldest and len(w._spare) == 1
