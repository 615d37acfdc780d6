"""CPU side of the frames-out path (csrc/frames_out_kernels.hip, pipeline.camera_rays / pack_frames / frame_errors,
SceneStream / SceneGroup.render_frames and score_frames): the entry points exist and refuse bad arguments before any device work, the
references of tests/frames_out_ref.py are what they claim to be, and the streams refuse what they must without touching a device."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

import frames_out_ref as R

F = np.float32


def test_entry_points_exist():
    from nerfdet_amd import _lib, pipeline, streaming
    lib = _lib.load()
    for name in ("ndet_camera_rays", "ndet_pack_frames", "ndet_frame_errors"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    for fn in ("camera_rays", "pack_frames", "frame_errors"):
        assert callable(getattr(pipeline, fn))
    for cls in (streaming.SceneStream, streaming.SceneGroup):
        assert callable(cls.render_frames) and callable(cls.score_frames)


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from nerfdet_amd import _lib
    lib = _lib.load()
    f, odd, err = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1001), lib.ndet_last_error

    def rays(k=f, rot=f, lp=f, n=3, x0=3, y0=3, s=1, h=14, w=22, o=f, d=f):
        return lib.ndet_camera_rays(k, rot, lp, n, x0, y0, s, h, w, o, d, None)
    for null in ("k", "rot", "lp", "o", "d"):
        assert rays(**{null: None}) == -1 and b"null" in err(), null
    for bad in (dict(n=0), dict(h=0), dict(w=-1), dict(s=0), dict(s=-2), dict(x0=-1), dict(y0=-1)):
        assert rays(**bad) == -1, bad
    for name in ("k", "rot", "lp", "o", "d"):
        assert rays(**{name: odd}) == -2 and b"aligned" in err(), name
    assert rays(n=1 << 10, h=1 << 10, w=1 << 10) == -2 and b"2^31" in err()          # 3 * 2^30 elements
    assert rays(n=1, h=1 << 16, w=1 << 15) == -2
    assert rays(x0=(1 << 31) - 10, w=22) == -2 and rays(s=1 << 28, h=14) == -2         # a pixel coordinate of 2^31 or more

    def pack(rgb=f, dep=f, mask=f, n=100, b=f, mm=f):
        return lib.ndet_pack_frames(rgb, dep, mask, n, b, mm, None)
    for null in ("rgb", "dep", "b", "mm"):
        assert pack(**{null: None}) == -1 and b"null" in err(), null
    assert pack(n=0) == -1 and pack(n=-7) == -1
    assert pack(n=(1 << 31) // 3 + 1) == -2 and pack(n=1 << 40) == -2
    for name in ("rgb", "dep", "mm"):
        assert pack(**{name: odd}) == -2 and b"aligned" in err(), name

    def errs(a=f, b=f, da=f, db=f, n=2, px=6144, out=f):
        return lib.ndet_frame_errors(a, b, da, db, n, px, out, None)
    for null in ("a", "b", "da", "out"):
        assert errs(**{null: None}) == -1 and b"null" in err(), null
    assert errs(n=0) == -1 and errs(px=0) == -1 and errs(px=-3) == -1
    assert errs(n=1, px=1 << 31) == -2 and errs(n=1 << 10, px=1 << 20) == -2
    for name in ("da", "db"):
        assert errs(**{name: odd}) == -2 and b"aligned" in err(), name
    assert errs(out=ctypes.c_void_p(0x1004)) == -2
    with pytest.raises(AssertionError):
        _lib.check(pack(n=0), "x")
    with pytest.raises(ValueError):
        _lib.check(errs(n=1, px=1 << 31), "x")


def test_camera_rays_ref_agrees_with_get_dtu_raydir():
    """2e-7 relative, the bound of tests/test_pipeline_edges_gpu.py, against the reference helper in float64."""
    from nerfdet_amd.pipeline import get_dtu_raydir
    krows, rot, lpos = R.cameras(3)
    ray_o, ray_d = R.camera_rays_ref(krows, rot, lpos, (3, 3, 14, 22))
    assert ray_o.dtype == F and ray_d.dtype == F and ray_d.shape == (3, 14 * 22, 3)
    k = np.eye(3)
    k[:2] = krows.astype(np.float64)
    px, py = np.meshgrid(np.arange(3, 25).astype(np.float64), np.arange(3, 17).astype(np.float64))
    coords = np.stack([px, py], axis=-1).reshape(-1, 2)
    for c in range(3):
        want = get_dtu_raydir(coords, k, rot[c].astype(np.float64))
        assert np.abs(ray_d[c] - want).max() <= 2e-7 * max(1.0, np.abs(want).max())
        assert np.array_equal(ray_o[c], np.tile(lpos[c], (14 * 22, 1)))


def test_strided_reference_is_the_subsample_of_the_full_one():
    krows, rot, lpos = R.cameras(2, seed=1)
    full_o, full_d = R.camera_rays_ref(krows, rot, lpos, (0, 0, 20, 28))
    for (y0, x0), s in (((1, 1), 3), ((2, 2), 4), ((0, 5), 7)):
        h, w = len(range(y0, 20, s)), len(range(x0, 28, s))
        o, d = R.camera_rays_ref(krows, rot, lpos, (y0, x0, h, w), s)
        assert np.array_equal(d.reshape(2, h, w, 3), full_d.reshape(2, 20, 28, 3)[:, y0::s, x0::s])
        assert np.array_equal(o, full_o[:, :h * w])


def _byte_exact(x):
    """The byte rule on one float32 in exact rationals: every float32 step rounded once."""
    if np.isnan(x):
        return 0
    if np.isinf(x):
        return 255 if x > 0 else 0
    v = R.rn32(Fraction(float(x)) * 255)
    if v < 0:
        return 0
    if v > 255:
        return 255
    return int(R.rn32(Fraction(float(v)) + Fraction(1, 2)))


def _mm_exact(x):
    if np.isnan(x):
        return 0
    if np.isinf(x):
        return 65535 if x > 0 else 0
    v = R.rn32(Fraction(float(x)) * 1000)
    if v < 0:
        return 0
    if v > 65535:
        return 65535
    return int(R.rn32(Fraction(float(v)) + Fraction(1, 2)))


def test_pack_frames_ref_on_the_edge_vector():
    rgb = R.edge_rgb()
    n = len(R.SPECIAL_RGB)
    got, _ = R.pack_frames_ref(rgb, np.zeros(len(rgb), dtype=F))
    assert got.dtype == np.uint8
    assert got[:n].tolist() == [0, 255, 0, 0, 0, 255, 255, 255, 255, 0, 0, got[11], got[12], 255, 255, 0, 0, 255]
    assert np.array_equal(got[n:n + 256], np.arange(256)), "k / 255 gives k back"
    ties = got[n + 256:].astype(int)
    assert np.all((ties == np.arange(256)) | (ties == np.minimum(np.arange(256) + 1, 255))) and ties[255] == 255
    assert len(set((ties - np.arange(256)).tolist())) == 2, "float32 (k + 0.5) / 255 * 255 lands on both sides of the tie"
    assert got.tolist() == [_byte_exact(x) for x in rgb]
    depth = R.edge_depth()
    mask = np.ones(len(depth), dtype=bool)
    _, mm = R.pack_frames_ref(np.zeros((len(depth), 3), dtype=F), depth, mask)
    assert mm.dtype == np.uint16 and mm.tolist() == [_mm_exact(x) for x in depth]
    s = dict(zip(R.SPECIAL_DEPTH, mm.tolist()))
    assert s[0.0004] == 0 and s[0.0005] in (0, 1) and s[65.5349] == 65535 and s[65.536] == 65535 and s[100.0] == 65535 and s[-1.0] == 0
    assert s[0.0015] in (1, 2) and s[3.2765] in (3276, 3277)
    mask[::2] = False
    _, mm2 = R.pack_frames_ref(np.zeros((len(depth), 3), dtype=F), depth, mask)
    assert np.array_equal(mm2[1::2], mm[1::2]) and not mm2[::2].any() and mm[::2].any()
    c, d, m = R.pack_inputs()
    assert c.shape[1] == 3 and c.shape[0] == d.shape[0] == m.shape[0] and c.shape[0] * 3 >= len(rgb) + 1000 and 0 < m.sum() < len(m)


def test_frame_errors_ref_against_a_brute_force_loop():
    for n, h, w in ((1, 1, 1), (3, 1, 257), (2, 8, 12)):
        a, b, da, db = R.errors_inputs(n, h, w)
        want = np.zeros((n, 4), dtype=object)
        for f in range(n):
            for y in range(h):
                for x in range(w):
                    if int(da[f, y, x]) == 0:
                        continue
                    want[f, 0] += sum((int(a[f, y, x, c]) - int(b[f, y, x, c])) ** 2 for c in range(3))
                    want[f, 1] += 1
                    if int(db[f, y, x]) != 0:
                        want[f, 2] += abs(int(da[f, y, x]) - int(db[f, y, x]))
                        want[f, 3] += 1
        got = R.frame_errors_ref(a, b, da, db)
        assert got.dtype == np.int64 and got.tolist() == want.tolist(), (n, h, w)
        none = R.frame_errors_ref(a, b, da)
        assert none[:, :2].tolist() == got[:, :2].tolist() and not none[:, 2:].any()
    p = R.psnr_ref(np.array([0, 0, 195075]), np.array([4, 0, 1]))
    assert p[0] == np.inf and np.isnan(p[1]) and p[2] == 0.0


def test_depth_to_mm_is_packs_rule():
    from nerfdet_amd.pipeline import depth_to_mm
    _, d, _ = R.pack_inputs()
    got = depth_to_mm(torch.from_numpy(d).to(torch.float64))          # the float64 maps of prepare_depth_frames, rounded to float32 first
    assert got.dtype == torch.uint16
    assert np.array_equal(got.numpy(), R.pack_frames_ref(np.zeros((len(d), 3), dtype=F), d)[1])


# ---- streams and groups on the CPU ----
class _Det:
    training = False
    render_testing = False


def _metas(n):
    from nerfdet_amd.synth import ring_scene_meta
    return [ring_scene_meta(6, (64, 96), origin=(0.1 * i, 0.0, 0.5)) for i in range(n)]


def _streams(held):
    """A SceneStream and a SceneGroup of two scenes as the other CPU tests build them (no device touched), with banks that hold
    ``held`` views each, or without banks (``held`` None)."""
    from nerfdet_amd.rays import ViewBank
    from nerfdet_amd.streaming import SceneGroup, SceneStream

    class _Held(ViewBank):
        n_views = held
    s = SceneStream.__new__(SceneStream)
    s.det, s.meta, s.device = _Det(), _metas(1)[0], None
    g = SceneGroup.__new__(SceneGroup)
    g.det, g.metas, g.device = _Det(), _metas(2), None
    if held is not None:
        s.bank, g.banks = _Held(), [_Held(), _Held()]
    return s, g


def test_streams_without_kept_views_do_not_render_frames():
    s, g = _streams(None)
    ext = s.meta["lidar2img"]["extrinsic"]
    frames = torch.zeros((1, 2, 128, 192, 3), dtype=torch.uint8)
    chunk = dict(s.meta, lidar2img=dict(s.meta["lidar2img"], extrinsic=ext[:2]))
    with pytest.raises(RuntimeError, match="keep_views"):
        s.render_frames(extrinsic=ext[:2])
    with pytest.raises(RuntimeError, match="keep_views"):
        s.score_frames(frames, chunk)
    with pytest.raises(RuntimeError, match="keep_views"):
        g.render_frames(extrinsic=[ext[:1], ext[:2]])
    with pytest.raises(RuntimeError, match="keep_views"):
        g.score_frames(torch.cat([frames, frames]), [chunk, chunk])
    s, g = _streams(0)
    with pytest.raises(RuntimeError, match="no views"):
        s.render_frames(extrinsic=ext[:2])
    with pytest.raises(RuntimeError, match="no views"):
        g.render_frames(extrinsic=[ext[:1], ext[:2]])


def test_bad_arguments_are_refused_before_any_launch():
    s, g = _streams(3)
    ext = s.meta["lidar2img"]["extrinsic"]
    c2w = [np.linalg.inv(e) for e in ext[:2]]
    for kw in (dict(), dict(c2w=c2w, extrinsic=ext[:2]), dict(c2w=c2w, stride=0), dict(c2w=c2w, stride=-1), dict(c2w=c2w, stride=1.5),
               dict(c2w=c2w, window=(0, 0, 0, 96)), dict(c2w=c2w, window=(0, 0, 64, 0)), dict(c2w=c2w, window=(-1, 0, 4, 4)),
               dict(c2w=c2w, window=(0, 0, 64)), dict(c2w=c2w, stride=200), dict(c2w=[]), dict(c2w=[np.eye(3)]), dict(extrinsic=np.eye(4)),
               dict(c2w=c2w, n_importance=-1), dict(c2w=c2w, n_importance=300)):
        with pytest.raises(ValueError):
            s.render_frames(**kw)
        gkw = {k: ([v, v] if k in ("c2w", "extrinsic") else v) for k, v in kw.items()}
        with pytest.raises(ValueError):
            g.render_frames(**gkw)
    for kw in (dict(c2w=[c2w]), dict(c2w=[c2w, c2w, c2w]), dict(c2w=[c2w, c2w], scenes=[1]), dict(c2w=[c2w, c2w], scenes=[0, 0]),
               dict(c2w=[c2w, []])):
        with pytest.raises(ValueError):
            g.render_frames(**kw)
    # score_frames: frames of another size, dtype or count, depth frames of another count
    chunk = dict(s.meta, lidar2img=dict(s.meta["lidar2img"], extrinsic=ext[:2]))
    good = torch.zeros((1, 2, 128, 192, 3), dtype=torch.uint8)
    for frames, meta, kw in ((good[:, :, :100], chunk, {}), (good.float(), chunk, {}), (good[:, :1], chunk, {}), (good[0], chunk, {}),
                             (good, chunk, dict(stride=0)), (good, chunk, dict(depth_frames=torch.zeros((1, 3, 60, 80), dtype=torch.uint16)))):
        with pytest.raises(ValueError):
            s.score_frames(frames, meta, **kw)
    with pytest.raises(ValueError):
        g.score_frames(torch.cat([good, good]), [chunk])
    with pytest.raises(ValueError):
        g.score_frames(good, [chunk, chunk])
    # what is left once the arguments are good is the device: no CPU fallback
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):
            s.render_frames(c2w=c2w)


def test_pipeline_wrappers_refuse_wrong_shapes_and_cpu_tensors():
    from nerfdet_amd import pipeline as P
    krows, rot, lpos = R.cameras(2)
    k = np.eye(3, dtype=F)
    k[:2] = krows
    c2w = R.c2w_of(rot, lpos)
    for bad in (dict(intrinsic=np.eye(2)), dict(c2w=c2w[0]), dict(c2w=np.zeros((2, 3, 4))), dict(window=(0, 0, 0, 5)), dict(stride=0)):
        args = dict(intrinsic=k, c2w=c2w, window=(0, 0, 4, 5), stride=1)
        args.update(bad)
        with pytest.raises(ValueError):
            P.camera_rays(**args)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):
            P.camera_rays(k, c2w, (0, 0, 4, 5))
        with pytest.raises(RuntimeError, match="GPU"):
            P.camera_rays(k, torch.from_numpy(c2w), (0, 0, 4, 5), device="cpu")
    rgb, depth, mask = torch.zeros(24, 3), torch.zeros(24), torch.ones(24, dtype=torch.bool)
    for bad in ((rgb[:23], depth, mask, (2, 3, 4)), (rgb, depth[:5], mask, (2, 3, 4)), (rgb, depth, mask.float(), (2, 3, 4)),
                (rgb.double(), depth, mask, (2, 3, 4)), (rgb, depth, mask, (2, 3)), (rgb, depth, mask, (2, 0, 12)), (rgb.view(-1), depth, None, (2, 3, 4))):
        with pytest.raises(ValueError):
            P.pack_frames(*bad)
    with pytest.raises(RuntimeError, match="GPU"):
        P.pack_frames(rgb, depth, mask, (2, 3, 4))
    with pytest.raises(RuntimeError, match="GPU"):
        P.pack_frames(rgb, depth, None, (2, 3, 4))
    a = torch.zeros((2, 3, 4, 3), dtype=torch.uint8)
    da = torch.zeros((2, 3, 4), dtype=torch.uint16)
    for bad in ((a, a[:1], da), (a.float(), a.float(), da), (a, a, da.to(torch.int32)), (a, a, da[:1]), (a[..., :2], a[..., :2], da), (a, a, da, da[:, :2]),
                (a, a, None)):
        with pytest.raises(ValueError):
            P.frame_errors(*bad)
    with pytest.raises(RuntimeError, match="GPU"):
        P.frame_errors(a, a, da)
    with pytest.raises(RuntimeError, match="GPU"):
        P.frame_errors(a, a, da, da)
