"""Rendering from a streamed scene without a GPU: ndet_ray_view_stats_bank rejects bad arguments before any HIP call, and a SceneStream
without kept views refuses to render."""
import ctypes

import pytest
import torch


def test_bank_entry_point_rejects_bad_arguments_without_a_gpu():
    from nerfdet_amd import _lib
    lib = _lib.load()
    assert lib.ndet_version() == 110
    assert ctypes.sizeof(_lib.NdetBankView) == 64
    assert _lib.NdetBankView.ke.offset == 16 and _lib.NdetBankView.rgb4.offset == 8
    f = ctypes.c_void_p(0x1000)

    def call(pts=f, n_points=100, views=f, n_views=3, H=16, W=16, d=8, hf=4, wf=4, glob=f, pm=f, vc=f):
        return lib.ndet_ray_view_stats_bank(pts, n_points, views, n_views, 16.0, 16.0, H, W, d, hf, wf, glob, pm, vc, None)

    for null in ("pts", "views", "glob", "pm"):
        assert call(**{null: None}) == -1 and b"null pointer" in lib.ndet_last_error(), null
    for bad in (dict(n_points=0), dict(n_points=-5), dict(n_views=0), dict(n_views=-1), dict(d=0), dict(H=1), dict(W=1), dict(hf=1), dict(wf=1),
                dict(H=0), dict(wf=-3)):
        assert call(**bad) == -1 and b"bad sizes" in lib.ndet_last_error(), bad
    assert call(d=6) == -2 and b"multiple of 4" in lib.ndet_last_error()
    assert call(d=132) == -2
    assert call(views=ctypes.c_void_p(0x1004)) == -2 and b"8-byte" in lib.ndet_last_error()
    assert call(glob=ctypes.c_void_p(0x1002)) == -2 and b"global_feat" in lib.ndet_last_error()
    assert call(n_points=2 ** 31 - 1) == -2 and b"too many points" in lib.ndet_last_error()
    assert call(H=1 << 15, W=1 << 15) == -2                               # one image beyond 2^31 floats
    # the null checks come first, whatever else is wrong
    assert call(pts=None, d=6, n_views=0) == -1


class _Det:
    training = False
    render_testing = False


def test_streams_without_kept_views_do_not_render():
    from nerfdet_amd.detector import nerfdet
    from nerfdet_amd.streaming import SceneStream
    from nerfdet_amd.synth import ring_scene_meta
    meta = ring_scene_meta(6, (64, 96))
    s = SceneStream.__new__(SceneStream)          # as the other CPU tests build one: no device touched
    s.det, s.meta = _Det(), meta
    assert s.bank is None
    rays = torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match="keep_views"):
        s.render_rays(rays, rays)
    with pytest.raises(RuntimeError, match="keep_views"):
        s.render(dict(ray_o=rays.view(1, 1, 5, 3), ray_d=rays.view(1, 1, 5, 3), gt_rgb=rays.view(1, 1, 5, 3), gt_depth=[],
                      nerf_sizes=[torch.tensor([[1, 5, 3]])]))
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="keep_views"):
            nerfdet.begin_scene(_Det(), meta, keep_views=bad)
        with pytest.raises(ValueError, match="keep_views"):
            SceneStream(_Det(), meta, window=2, keep_views=bad)


def test_an_empty_bank_has_no_table():
    from nerfdet_amd.rays import ViewBank
    bank = ViewBank()
    assert bank.n_views == 0 and bank.segments == [] and bank.nbytes() == 0
    bank.clear()
    bank.drop_oldest(0)
    with pytest.raises(ValueError):
        bank.drop_oldest(1)
    with pytest.raises(RuntimeError, match="no views"):
        bank.table()
