"""View banks and rendering for scene groups without a GPU: ndet_ray_view_stats_bank_group rejects bad arguments on the host before any HIP
call, and a SceneGroup without kept views refuses to render before it touches a device."""
import ctypes
import inspect
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sel(n=3, n_views=(3, 1, 70), n_points=(100, 1, 4883), views=None, size=None):
    from nerfdet_amd import _lib
    sel = _lib.NdetBankGroupSel()
    sel.size = ctypes.sizeof(_lib.NdetBankGroupSel) if size is None else size
    sel.n = n
    for i in range(min(max(n, 0), 64)):
        sel.views[i] = 0x1000 + 64 * i if views is None else views[i]
        sel.n_views[i] = n_views[i % len(n_views)]
        sel.n_points[i] = n_points[i % len(n_points)]
    return sel


def test_selection_block_mirrors_the_header():
    from nerfdet_amd import _lib
    header = open(os.path.join(ROOT, "include", "nerfdet_hip.h")).read()
    assert "typedef struct NdetBankGroupSel {" in header
    body = header[header.index("typedef struct NdetBankGroupSel {"):header.index("} NdetBankGroupSel;")]
    for field in ("int32_t size;", "int32_t n;", "const NdetBankView* views[NDET_GROUP_MAX];", "int32_t n_views[NDET_GROUP_MAX];",
                  "int32_t n_points[NDET_GROUP_MAX];"):
        assert field in body, field
    s = _lib.NdetBankGroupSel
    assert [f[0] for f in s._fields_] == ["size", "n", "views", "n_views", "n_points"]
    assert ctypes.sizeof(s) == 8 + 64 * 8 + 2 * 64 * 4 == 1032        # with the library's 256-byte prefix: under the 4 KiB of kernel arguments
    assert (s.views.offset, s.n_views.offset, s.n_points.offset) == (8, 520, 776)


def test_group_entry_point_rejects_bad_arguments_without_a_gpu():
    from nerfdet_amd import _lib
    lib = _lib.load()
    assert "ndet_ray_view_stats_bank_group" in _lib.SIGNATURES and hasattr(lib, "ndet_ray_view_stats_bank_group")
    f = ctypes.c_void_p(0x1000)

    def call(pts=f, sel=None, H=16, W=16, d=8, hf=4, wf=4, glob=f, pm=f, vc=f, null_sel=False):
        block = _sel() if sel is None else sel
        return lib.ndet_ray_view_stats_bank_group(pts, None if null_sel else ctypes.byref(block), 16.0, 16.0, H, W, d, hf, wf, glob, pm, vc, None)

    err = lib.ndet_last_error
    for null in ("pts", "glob", "pm"):
        assert call(**{null: None}) == -1 and b"null pointer" in err(), null
    assert call(null_sel=True) == -1 and b"null pointer" in err()
    for size in (ctypes.sizeof(_lib.NdetBankGroupSel) - 4, ctypes.sizeof(_lib.NdetBankGroupSel) + 8, 0):
        assert call(sel=_sel(size=size)) == -1 and b"size" in err(), size
    for n in (0, 65, -1):
        assert call(sel=_sel(n=n)) == -1 and b"listed scenes" in err(), n
    assert call(sel=_sel(n_views=(3, 0, 5))) == -1 and b"listed scene 1" in err() and b"0 views" in err()
    assert call(sel=_sel(n_views=(3, 4, -2))) == -1 and b"listed scene 2" in err()
    assert call(sel=_sel(n_points=(100, 7, 0))) == -1 and b"listed scene 2" in err() and b"0 points" in err()
    assert call(sel=_sel(views=[0x1000, 0, 0x2000])) == -1 and b"null pointer" in err() and b"listed scene 1" in err()
    for bad in (dict(H=1), dict(W=1), dict(hf=1), dict(wf=1), dict(d=0), dict(H=0), dict(wf=-3)):
        assert call(**bad) == -1 and b"bad sizes" in err(), bad
    assert call(d=6) == -2 and b"multiple of 4" in err()
    assert call(d=132) == -2 and b"at most 128" in err()
    assert call(sel=_sel(views=[0x1000, 0x1040, 0x1084])) == -2 and b"8-byte" in err() and b"listed scene 2" in err()
    assert call(glob=ctypes.c_void_p(0x1002)) == -2 and b"global_feat" in err()
    assert call(H=1 << 15, W=1 << 15) == -2 and b"2^31" in err()                       # one image beyond 2^31 floats
    assert call(sel=_sel(n_points=(100, 2 ** 31 - 1, 5))) == -2 and b"too many points" in err()
    assert call(sel=_sel(n_points=(2 ** 30, 2 ** 30, 5))) == -2 and b"too many points" in err() and b"in all" in err()
    # scenes beyond n are not looked at; the null checks come first, whatever else is wrong
    sel = _sel(n=2)
    sel.n_views[2], sel.views[2] = 0, 0
    assert call(sel=sel, d=6) == -2
    assert call(pts=None, d=6, sel=_sel(n=0)) == -1 and b"null pointer" in err()
    with pytest.raises(AssertionError):
        _lib.check(call(sel=_sel(n=65)), "x")
    with pytest.raises(ValueError):
        _lib.check(call(d=6), "x")


class _Det:
    training = False
    render_testing = False


def _metas(n):
    from nerfdet_amd.synth import ring_scene_meta
    return [ring_scene_meta(6, (64, 96), origin=(0.1 * i, 0.0, 0.5)) for i in range(n)]


def test_groups_without_kept_views_do_not_render():
    from nerfdet_amd.detector import nerfdet
    from nerfdet_amd.streaming import SceneGroup
    params = inspect.signature(nerfdet.begin_scenes).parameters
    assert params["keep_views"].default is False and params["window"].default is None
    assert inspect.signature(SceneGroup.__init__).parameters["keep_views"].default is False
    g = SceneGroup.__new__(SceneGroup)          # as the other CPU tests build one: no device touched
    g.det, g.metas = _Det(), _metas(2)
    assert g.banks is None
    rays = [torch.zeros(5, 3), torch.zeros(2, 3)]
    for batched in (False, True):
        with pytest.raises(RuntimeError, match="keep_views"):
            g.render_rays(rays, rays, batched=batched)
        with pytest.raises(RuntimeError, match="keep_views"):
            g.render_rays(rays[:1], rays[:1], scenes=[1], batched=batched)
    rb = dict(ray_o=rays[0].view(1, 1, 5, 3), ray_d=rays[0].view(1, 1, 5, 3), gt_rgb=rays[0].view(1, 1, 5, 3), gt_depth=[],
              nerf_sizes=[torch.tensor([[1, 5, 3]])])
    with pytest.raises(RuntimeError, match="keep_views"):
        g.render([rb, rb])
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="keep_views"):
            nerfdet.begin_scenes(_Det(), _metas(2), keep_views=bad)
        with pytest.raises(ValueError, match="keep_views"):
            SceneGroup(_Det(), _metas(2), window=2, keep_views=bad)
    # a render_testing detector is still refused without keep_views
    det = _Det()
    det.render_testing = True
    with pytest.raises(NotImplementedError, match="keep_views"):
        SceneGroup(det, _metas(2))


def test_kept_views_refuse_bad_ray_lists_before_any_launch():
    """A group with (empty) banks on the CPU: scenes without views and wrong ray lists are refused on the host."""
    from nerfdet_amd.rays import ViewBank
    from nerfdet_amd.streaming import SceneGroup
    g = SceneGroup.__new__(SceneGroup)
    g.det, g.metas = _Det(), _metas(2)
    g.banks = [ViewBank(), ViewBank()]
    rays = [torch.zeros(5, 3), torch.zeros(2, 3)]
    with pytest.raises(RuntimeError, match="no views"):
        g.render_rays(rays, rays)
    with pytest.raises(ValueError):
        g.render_rays(rays, rays, scenes=[0, 0])

    class _Held(ViewBank):
        n_views = 3
    g.banks = [_Held(), _Held()]
    for o, d, scenes in ((rays[:1], rays[:1], None), (rays, rays[:1], None), (rays, rays, [1]), (rays[0], rays[0], [0]),
                         ([torch.zeros(5, 4), rays[1]], [torch.zeros(5, 4), rays[1]], None), ([torch.zeros(0, 3), rays[1]], [torch.zeros(0, 3), rays[1]], None),
                         (rays, [rays[0], torch.zeros(3, 3)], None), ([torch.zeros(5), rays[1]], [torch.zeros(5), rays[1]], None)):
        with pytest.raises(ValueError, match="render_rays"):
            g.render_rays(o, d, scenes=scenes)
    with pytest.raises(ValueError, match="ray batches"):
        g.render([dict()])
