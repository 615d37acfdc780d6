"""Streaming scenes without a GPU: the NdetSceneAccum entry points reject bad arguments before any HIP call, and SceneStream.add_views
rejects a chunk whose camera rig differs from the scene's."""
import ctypes

import numpy as np
import pytest
import torch


def _state(**bad):
    from nerfdet_amd import _lib
    fields = dict(size=ctypes.sizeof(_lib.NdetSceneAccum), N=64, C=32, cm=8, n_views=0, k1_sum=0x1000, k1_pitch=32, k1_count=0x2000,
                  k2_sum=0x3000, k2_pitch=36, k2_count=0x4000)
    fields.update(bad)
    return _lib.NdetSceneAccum(**fields)


def _gate(n_views):
    from nerfdet_amd import _lib
    return _lib.NdetDepthGate(size=ctypes.sizeof(_lib.NdetDepthGate), dtype=0, n_views=n_views, h=4, w=4, H=16, W=16, depth_f=0x5000,
                              f_view_pitch=16, f_row_pitch=4, depth_r=0x6000, r_view_pitch=256, r_row_pitch=16, band=0.5)


def test_scene_entry_points_reject_bad_arguments_without_a_gpu():
    from nerfdet_amd import _lib
    lib = _lib.load()
    assert lib.ndet_version() == 110
    f = ctypes.c_void_p(0x1000)

    def acc(s, n_views=2, gate=None):
        # features (n,4,4,32) channels-last, mapped (n,4,4,8), rgb (n,3,16,16)
        return lib.ndet_scene_accumulate(None if s is None else ctypes.byref(s), f, n_views, 4, 4, 512, 128, f, 128, 32, f, f, 16, 16, 768, 256, 16,
                                         f, f, f, None if gate is None else ctypes.byref(gate), None)

    def dfin(s):
        return lib.ndet_scene_density_finish(None if s is None else ctypes.byref(s), f, f, None)

    def vfin(s):
        return lib.ndet_scene_volume_finish(None if s is None else ctypes.byref(s), None, f, f, None)

    for call in (acc, dfin, vfin):
        assert call(None) == -1 and b"null scene state" in lib.ndet_last_error()
        assert call(_state(size=ctypes.sizeof(_lib.NdetSceneAccum) - 8)) == -1 and b"size" in lib.ndet_last_error()
        assert call(_state(k2_sum=None)) == -1
        assert call(_state(C=30, k1_pitch=32)) == -2                       # C not a multiple of 4
        assert call(_state(cm=6, k2_pitch=36)) == -2                       # cm not a multiple of 4
        assert call(_state(k1_sum=0x1004)) == -2                           # misaligned state rows
        assert call(_state(k2_pitch=20)) == -1                             # pitch smaller than a row
        assert call(_state(k1_pitch=1 << 31)) == -2                        # pitch beyond int32
    # a gate for another number of views than the chunk's
    assert acc(_state(), 2, _gate(3)) == -1 and b"depth maps for 3 views" in lib.ndet_last_error()
    bad = _gate(2)
    bad.size = 8
    assert acc(_state(), 2, bad) == -1
    # chunk inputs: null pointer, feature pitch below a row, misaligned mapped quads
    assert lib.ndet_scene_accumulate(ctypes.byref(_state()), None, 2, 4, 4, 512, 128, f, 128, 32, f, f, 16, 16, 768, 256, 16, f, f, f, None, None) == -1
    assert lib.ndet_scene_accumulate(ctypes.byref(_state()), f, 2, 4, 4, 512, 64, f, 128, 32, f, f, 16, 16, 768, 256, 16, f, f, f, None, None) == -1
    assert lib.ndet_scene_accumulate(ctypes.byref(_state()), f, 2, 4, 4, 512, 128, ctypes.c_void_p(0x1004), 128, 32, f, f, 16, 16, 768, 256, 16,
                                     f, f, f, None, None) == -2
    assert lib.ndet_scene_accumulate(ctypes.byref(_state(n_views=0x7fffffff)), f, 2, 4, 4, 512, 128, f, 128, 32, f, f, 16, 16, 768, 256, 16,
                                     f, f, f, None, None) == -2


class _Det:
    training = False


def _stream(meta):
    from nerfdet_amd.streaming import SceneStream
    s = SceneStream.__new__(SceneStream)      # the checks below run before anything touches a device
    s.det, s.meta = _Det(), meta
    return s


def test_add_views_rejects_another_rig():
    from nerfdet_amd.synth import ring_scene_meta
    meta = ring_scene_meta(6, (64, 96))
    s = _stream(meta)
    img = torch.zeros(1, 2, 3, 64, 96)

    def chunk(**lidar):
        m = dict(meta)
        m["lidar2img"] = dict(meta["lidar2img"], extrinsic=meta["lidar2img"]["extrinsic"][:2], **lidar)
        return m

    with pytest.raises(ValueError, match="origin"):
        s.add_views(img, img, chunk(origin=np.asarray(meta["lidar2img"]["origin"]) + 0.1))
    intr = np.array(meta["lidar2img"]["intrinsic"], dtype=np.float32)
    intr[0, 0] *= 1.01
    with pytest.raises(ValueError, match="intrinsic"):
        s.add_views(img, img, chunk(intrinsic=intr))
    m = chunk()
    m["img_shape"] = (60, 96, 3)
    with pytest.raises(ValueError, match="img_shape"):
        s.add_views(img, img, m)
    m = chunk()
    m["ori_shape"] = (120, 192, 3)
    with pytest.raises(ValueError, match="ori_shape"):
        s.add_views(img, img, m)
    with pytest.raises(ValueError, match="extrinsics"):
        s.add_views(torch.zeros(1, 3, 3, 64, 96), torch.zeros(1, 3, 3, 64, 96), chunk())
    with pytest.raises(ValueError, match="one scene"):
        s.add_views(torch.zeros(2, 2, 3, 64, 96), torch.zeros(2, 2, 3, 64, 96), chunk())
    with pytest.raises(ValueError, match="depth"):
        s.add_views(img, img, chunk(), depth=torch.zeros(1, 3, 8, 8))
