"""The raw-frame path without a GPU: the new entry point is exported and refuses what its header says before any device work, the size
arithmetic of pipeline.rescale_size / frame_meta is datasets.Resize's, the oracle helper (tests/raw_frames_ref.py) stands on the host
function, and add_frames refuses frames that its scene's meta does not describe before anything touches a device."""
import ctypes

import numpy as np
import pytest
import torch

import raw_frames_ref as R


def test_the_library_exports_the_new_entry_point():
    from nerfdet_amd import _lib
    lib = _lib.load()
    assert "ndet_resize_normalize_views" in _lib.SIGNATURES and hasattr(lib, "ndet_resize_normalize_views")
    assert len(_lib.SIGNATURES["ndet_resize_normalize_views"][0]) == 15


def test_resize_normalize_views_refuses_bad_arguments_without_a_gpu():
    from nerfdet_amd import _lib
    lib = _lib.load()
    f = ctypes.c_void_p(0x1000)
    err = lib.ndet_last_error
    mean_ok, std_ok = (ctypes.c_double * 3)(123.675, 116.28, 103.53), (ctypes.c_double * 3)(58.395, 57.12, 57.375)

    def call(frames=f, ids=f, n_sel=2, Hs=37, Ws=53, Hr=22, Wr=32, H=24, W=32, mean=mean_ok, std=std_ok, img=f, denorm=f, u8=f):
        return lib.ndet_resize_normalize_views(frames, ids, n_sel, Hs, Ws, Hr, Wr, H, W, mean, std, img, denorm, u8, None)

    for null in ("frames", "mean", "std", "img", "denorm"):
        assert call(**{null: None}) == -1 and b"null pointer" in err(), null
    for bad in ("n_sel", "Hs", "Ws", "Hr", "Wr", "H", "W"):
        for v in (0, -3):
            assert call(**{bad: v}) == -1 and b"sizes must be positive" in err(), (bad, v)
    for bad in ((58.395, 0.0, 57.375), (-1.0, 57.12, 57.375), (58.395, 57.12, float("nan"))):
        assert call(std=(ctypes.c_double * 3)(*bad)) == -1 and b"std must be positive" in err(), bad
    assert call(Hr=25) == -1 and b"does not fit the pad" in err()
    assert call(Wr=33) == -1 and b"does not fit the pad" in err()
    # one frame of 2^31 bytes or more; one view's output planes of 2^31 elements or more
    assert 32768 * 21846 * 3 >= 1 << 31 > 32768 * 21845 * 3
    assert call(Hs=32768, Ws=21846) == -2 and b"frame" in err() and b"2^31" in err()
    assert call(Hr=32768, Wr=21846, H=32768, W=21846) == -2 and b"planes" in err() and b"2^31" in err()
    # ids and resized_bgr may be null: with them null the next refusal is still the one reported
    assert call(ids=None, u8=None, Hr=25) == -1 and b"does not fit the pad" in err()


def test_the_codes_become_the_usual_exceptions():
    from nerfdet_amd import _lib
    f = ctypes.c_void_p(0x1000)
    ms = (ctypes.c_double * 3)(1.0, 1.0, 1.0)
    with pytest.raises(AssertionError, match="does not fit the pad"):
        _lib.check(_lib.load().ndet_resize_normalize_views(f, None, 1, 8, 8, 9, 8, 8, 8, ms, ms, f, f, None, None), "resize_normalize_views")
    with pytest.raises(ValueError, match="2\\^31"):
        _lib.check(_lib.load().ndet_resize_normalize_views(f, None, 1, 32768, 21846, 8, 8, 8, 8, ms, ms, f, f, None, None), "resize_normalize_views")


RESCALE = [((968, 1296), (320, 240), (239, 320)), ((480, 640), (320, 240), (240, 320)), ((128, 194), (96, 64), (63, 96)),
           ((19, 23), (32, 24), (24, 29))]


@pytest.mark.parametrize("size,scale,want", RESCALE)
def test_rescale_size_is_the_datasets_resize(size, scale, want):
    from nerfdet_amd import pipeline as P
    assert P.rescale_size(size, scale) == want
    assert R.resized_size(size, scale) == want
    assert P.rescale_size(size, scale[::-1]) == want            # mmcv.imrescale reads the scale as (long edge, short edge)


def test_rescale_size_on_the_kernel_test_sizes():
    from nerfdet_amd import pipeline as P
    for size, scale, want, pad in R.SIZES.values():
        assert P.rescale_size(size, scale) == want == R.resized_size(size, scale)
        assert want[0] <= pad[0] and want[1] <= pad[1]


def test_frame_meta_and_the_refusal_of_a_frame_that_does_not_fit():
    from nerfdet_amd import pipeline as P
    from nerfdet_amd.synth import ring_scene_meta
    l2i = ring_scene_meta(3, (240, 320))["lidar2img"]
    m = P.frame_meta(l2i, (968, 1296), (320, 240), (240, 320))
    assert (m["ori_shape"], m["img_shape"], m["pad_shape"]) == ((968, 1296, 3), (239, 320, 3), (240, 320, 3))
    assert m["lidar2img"]["intrinsic"] is l2i["intrinsic"] and len(m["lidar2img"]["extrinsic"]) == 3
    with pytest.raises(ValueError, match="does not fit"):       # a portrait frame into a landscape pad
        P.frame_meta(l2i, (1296, 968), (320, 240), (240, 320))
    with pytest.raises(ValueError, match="does not fit"):
        P.prepare_frames(torch.zeros(1, 1296, 968, 3, dtype=torch.uint8), (320, 240), (240, 320))
    with pytest.raises(ValueError, match="uint8"):
        P.prepare_frames(torch.zeros(1, 37, 53, 3), (32, 24), (24, 32))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        P.prepare_frames(torch.zeros(1, 37, 53, 3, dtype=torch.uint8), (32, 24), (24, 32))
    with pytest.raises(ValueError, match="go together"):
        P.MultiViewPipeline(4, img_scale=(32, 24))


def test_the_host_resize_is_not_float_bilinear():
    """What the every-byte GPU test rests on: on each non-copy size the host function differs from exact bilinear interpolation with
    round-to-nearest in some bytes (each by one grey level), so a kernel that interpolated in floating point could not pass it."""
    from nerfdet_amd.datasets import imresize_linear
    from test_pipeline_edges_gpu import _frames
    for name, (size, scale, (hr, wr), pad) in R.SIZES.items():
        fr = _frames(size, n=2)
        a, b = R.float_bilinear(fr[0], (wr, hr)), imresize_linear(fr[0], (wr, hr))
        d = np.abs(a.astype(np.int64) - b.astype(np.int64))
        assert d.max() <= 1
        assert (int((d != 0).sum()) > 0) == ("copy" not in name), (name, int((d != 0).sum()))


def test_the_oracle_pads_after_normalising():
    mean, std = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
    fr = np.full((1, 37, 53, 3), 200, np.uint8)
    ref = R.prepare(fr, (32, 24), (24, 32), mean, std)
    assert ref["resized_hw"] == (22, 32) and not ref["img"][:, :, 22:].any() and not ref["u8"][:, 22:].any()
    assert np.array_equal(ref["denorm"][0, :, 23, 0], np.array([103, 116, 123], np.float32) / np.float32(255.0))      # BGR planes
    assert np.array_equal(ref["u8"][0, :22], np.full((22, 32, 3), 200, np.uint8))


# ---- add_frames refuses before any device work ----
class _Det:
    training = False


def _raw_meta(n_v=6):
    from nerfdet_amd import pipeline as P
    from nerfdet_amd.synth import ring_scene_meta
    return P.frame_meta(ring_scene_meta(n_v, (64, 97))["lidar2img"], (128, 194), (96, 64), (64, 96))


def _chunk(meta, k):
    m = dict(meta)
    m["lidar2img"] = dict(meta["lidar2img"], extrinsic=meta["lidar2img"]["extrinsic"][:k])
    return m


def test_stream_add_frames_refuses_frames_its_meta_does_not_describe():
    from nerfdet_amd.detector import nerfdet
    from nerfdet_amd.streaming import SceneStream
    assert callable(getattr(SceneStream, "add_frames")) and "mean" in nerfdet.begin_scene.__code__.co_varnames
    meta = _raw_meta()
    assert (meta["ori_shape"], meta["img_shape"], meta["pad_shape"]) == ((128, 194, 3), (63, 96, 3), (64, 96, 3))
    s = SceneStream.__new__(SceneStream)      # the checks below run before anything touches a device
    s.det, s.meta = _Det(), meta
    ok = torch.zeros(1, 2, 128, 194, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="ori_shape"):
        s.add_frames(torch.zeros(1, 2, 127, 194, 3, dtype=torch.uint8), _chunk(meta, 2))
    with pytest.raises(ValueError, match="raw uint8 BGR frames"):
        s.add_frames(ok.float(), _chunk(meta, 2))
    with pytest.raises(ValueError, match="raw uint8 BGR frames"):
        s.add_frames(ok[0], _chunk(meta, 2))
    with pytest.raises(ValueError, match="raw uint8 BGR frames"):
        s.add_frames(torch.zeros(2, 2, 128, 194, 3, dtype=torch.uint8), _chunk(meta, 2))
    with pytest.raises(ValueError, match="extrinsics"):
        s.add_frames(ok, _chunk(meta, 3))
    with pytest.raises(ValueError, match="depth"):
        s.add_frames(ok, _chunk(meta, 2), depth=torch.zeros(1, 3, 8, 8))
    m = _chunk(meta, 2)
    m["pad_shape"] = (64, 128, 3)
    with pytest.raises(ValueError, match="pad_shape"):
        s.add_frames(ok, m)
    # a scene whose img_shape is not what the resize gives: 64 rows instead of 63; and one without pad_shape (= img_shape), whose box the
    # frame fills to 63 x 95
    s.meta = dict(meta, img_shape=(64, 96, 3))
    with pytest.raises(ValueError, match="img_shape"):
        s.add_frames(ok, _chunk(s.meta, 2))
    s.meta = {k: v for k, v in meta.items() if k != "pad_shape"}
    with pytest.raises(ValueError, match="img_shape"):
        s.add_frames(ok, _chunk(s.meta, 2))
    # a described chunk passes every check and stops where the device work would begin
    s.meta = meta
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        s.add_frames(ok, _chunk(meta, 2))


def test_group_add_frames_refuses_frames_its_meta_does_not_describe():
    from nerfdet_amd.streaming import SceneGroup
    meta = _raw_meta()
    g = SceneGroup.__new__(SceneGroup)
    g.det, g.metas = _Det(), [dict(meta) for _ in range(3)]
    ok = torch.zeros(2, 2, 128, 194, 3, dtype=torch.uint8)
    chunks = [_chunk(meta, 2), _chunk(meta, 2)]
    with pytest.raises(ValueError, match="ori_shape"):
        g.add_frames(torch.zeros(2, 2, 128, 193, 3, dtype=torch.uint8), chunks, scenes=[2, 0])
    with pytest.raises(ValueError, match="raw uint8 BGR frames"):
        g.add_frames(ok, chunks)                                    # three scenes listed, two rows
    with pytest.raises(ValueError, match="chunk metas"):
        g.add_frames(ok, chunks[:1], scenes=[2, 0])
    with pytest.raises(ValueError, match="extrinsics"):
        g.add_frames(ok, [_chunk(meta, 2), _chunk(meta, 1)], scenes=[2, 0])
    with pytest.raises(ValueError):
        g.add_frames(ok, chunks, scenes=[0, 0])
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        g.add_frames(ok, chunks, scenes=[2, 0])
