"""CPU side of the frame SSIM (csrc/frame_ssim_kernels.hip, pipeline.frame_ssim, rays.ssim_views, score_frames(ssim=True)): the entry point
exists and refuses bad arguments before any device work, the wrappers refuse what they must, and the numpy restatement of
tests/frame_ssim_ref.py -- what the GPU tests hold the kernel to, bit for bit -- is the reference's metric: it agrees with the independent
oracle/render_eval_oracle.py on every input the GPU tests use."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import frame_ssim_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# quantisation (2^-41 a window) plus the oracle's own float64 rounding over C2 = 3.6e-3: two decades of margin; a wrong constant or window
# count shows at 1e-3 or more
ORACLE_TOL = 1e-10


def test_entry_point_exists_and_the_version_stays():
    from nerfdet_amd import _lib, pipeline, rays, streaming
    lib = _lib.load()
    assert "ndet_frame_ssim" in _lib.SIGNATURES and hasattr(lib, "ndet_frame_ssim")
    assert lib.ndet_version() == 110, "an added entry point does not move the ABI version"
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nerfdet_hip.h")).read(), flags=re.S)
    decl = re.search(r"int\s+ndet_frame_ssim\s*\(([^)]*)\)\s*;", txt)
    assert decl and decl.group(1).count(",") + 1 == len(_lib.SIGNATURES["ndet_frame_ssim"][0]) == 9
    assert callable(pipeline.frame_ssim) and callable(rays.ssim_views)
    src = open(os.path.join(ROOT, "nerf-det_amd", "csrc", "frame_ssim_kernels.hip")).read()
    th, tw = (int(re.search(rf"#define {name} (\d+)", src).group(1)) for name in ("SSIM_TH", "SSIM_TW"))
    assert pipeline.SSIM_TILE == (th, tw) == S.TILE
    for c, name in ((S.C1_U8, "SSIM_C1_U8"), (S.C2_U8, "SSIM_C2_U8"), (S.C1_F32, "SSIM_C1_F32"), (S.C2_F32, "SSIM_C2_F32")):
        assert float.fromhex(re.search(rf"#define {name} (\S+)", src).group(1)) == c, name
    import inspect
    for cls in (streaming.SceneStream, streaming.SceneGroup):
        assert inspect.signature(cls.score_frames).parameters["ssim"].default is False
    assert inspect.signature(rays.rendering_metrics).parameters["fused"].default is False


def test_entry_point_refuses_bad_arguments_without_a_gpu():
    from nerfdet_amd import _lib
    lib = _lib.load()
    f, odd, err = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1001), lib.ndet_last_error

    def ssim(a=f, b=f, da=f, kind=0, n=2, h=39, w=70, out=f):
        return lib.ndet_frame_ssim(a, b, da, kind, n, h, w, out, None)
    for null in ("a", "b", "out"):
        assert ssim(**{null: None}) == -1 and b"null" in err(), null
    for bad in (dict(n=0), dict(n=-1), dict(h=6), dict(w=6), dict(h=0), dict(w=-3), dict(kind=2), dict(kind=-1)):
        assert ssim(**bad) == -1, bad
    assert ssim(n=1, h=2054, w=2054) == -2 and b"2^22" in err()                      # 2048 * 2048 windows
    assert ssim(n=1 << 12, h=512, w=512) == -2 and b"2^31" in err()                  # 3 * 2^30 elements
    assert ssim(da=odd) == -2 and b"aligned" in err()
    assert ssim(out=ctypes.c_void_p(0x1004)) == -2 and b"aligned" in err()
    assert ssim(kind=1, a=ctypes.c_void_p(0x1002)) == -2 and b"aligned" in err()
    assert ssim(kind=1, b=odd) == -2 and b"aligned" in err()
    with pytest.raises(AssertionError):
        _lib.check(ssim(h=6), "x")
    with pytest.raises(ValueError):
        _lib.check(ssim(n=1, h=2054, w=2054), "x")


def test_wrappers_refuse_wrong_shapes_and_cpu_tensors():
    from nerfdet_amd import pipeline as P, rays
    a = torch.zeros((2, 9, 12, 3), dtype=torch.uint8)
    da = torch.ones((2, 9, 12), dtype=torch.uint16)
    for bad in ((a, a[:1]), (a, a.float()), (a.double(), a.double()), (a.to(torch.int32), a.to(torch.int32)), (a[..., :2], a[..., :2]), (a[0], a[0]),
                (a, a, da.to(torch.int32)), (a, a, da[:1]), (a, a, da[:, :, :7]), (a[:, :6], a[:, :6]), (a[:, :, :6], a[:, :, :6]),
                (a[:, :, ::2], a[:, :, ::2]), (a.numpy(), a.numpy()), (a.float(), a.float(), da.float())):
        with pytest.raises(ValueError):
            P.frame_ssim(*bad)
    with pytest.raises(RuntimeError, match="GPU"):
        P.frame_ssim(a, a)
    with pytest.raises(RuntimeError, match="GPU"):
        P.frame_ssim(a.float(), a.float(), da)
    with pytest.raises(ValueError):
        rays.ssim_views(a, a)
    with pytest.raises(ValueError):
        rays.ssim_views(a.float()[:, :6], a.float()[:, :6])
    with pytest.raises(RuntimeError, match="GPU"):
        rays.ssim_views(a.float(), a.float())


def _streams(held=3):
    """A SceneStream and a SceneGroup of two scenes with banks of ``held`` views each, built without touching a device."""
    from nerfdet_amd.rays import ViewBank
    from nerfdet_amd.streaming import SceneGroup, SceneStream
    from nerfdet_amd.synth import ring_scene_meta

    class _Det:
        training = False
        render_testing = False

    class _Held(ViewBank):
        n_views = held
    metas = [ring_scene_meta(6, (64, 96), origin=(0.1 * i, 0.0, 0.5)) for i in range(2)]
    s = SceneStream.__new__(SceneStream)
    s.det, s.meta, s.device, s.bank = _Det(), metas[0], None, _Held()
    g = SceneGroup.__new__(SceneGroup)
    g.det, g.metas, g.device, g.banks = _Det(), metas, None, [_Held(), _Held()]
    return s, g


def test_score_frames_refuses_ssim_on_a_thumbnail_below_one_window():
    """64 x 96 content at stride 16 leaves 4 x 6 pixels: a ValueError before anything touches a device (a launch without a GPU would be a
    RuntimeError here); the same stride without ssim gets past the argument checks."""
    s, g = _streams(3)
    ext = s.meta["lidar2img"]["extrinsic"]
    chunk = dict(s.meta, lidar2img=dict(s.meta["lidar2img"], extrinsic=ext[:2]))
    chunks = [dict(m, lidar2img=dict(m["lidar2img"], extrinsic=m["lidar2img"]["extrinsic"][:2])) for m in g.metas]
    good = torch.zeros((1, 2, 128, 192, 3), dtype=torch.uint8)
    for stride in (16, 10):                      # 4 x 6 and 6 x 9
        with pytest.raises(ValueError, match="ssim"):
            s.score_frames(good, chunk, stride=stride, ssim=True)
        with pytest.raises(ValueError, match="ssim"):
            g.score_frames(torch.cat([good, good]), chunks, stride=stride, ssim=True)
    with pytest.raises(ValueError, match="ssim"):
        s.score_frames(good, chunk, ssim=1)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            s.score_frames(good, chunk, stride=16)


def _oracle(a, b):
    from oracle import render_eval_oracle as O
    return np.array([O.ssim(a[f], b[f]) for f in range(a.shape[0])])


@pytest.mark.parametrize("content", S.CONTENTS)
def test_the_restatement_is_the_oracles_ssim_on_the_gpu_tests_inputs(content):
    worst = 0.0
    for h, w in S.shapes():
        for n in (1, 3):
            a, b = S.frames(content, n, h, w)
            out = S.frame_ssim_ref(a, b)
            assert out.dtype == np.int64 and (out[:, 3] == (h - 6) * (w - 6)).all()
            ch, ssim = S.ssim_of(out)
            want = _oracle(a.astype(np.float64) / 255.0, b.astype(np.float64) / 255.0)
            worst = max(worst, np.abs(ssim - want).max())
            assert np.abs(ssim - want).max() <= ORACLE_TOL, (content, h, w, n, ssim, want)
            if content == "equal":
                assert (out[:, :3] == out[:, 3:] * 2 ** 40).all() and (ssim == 1.0).all()
            if content == "inverted" and h * w > 49:
                assert (out[:, :3] < 0).all()
            if content == "extremes":
                assert (out[:, :3] > 0).all() and (ssim < 1e-3).all()
    print(f"{content}: max |restatement - oracle| {worst:.3e} (bound {ORACLE_TOL:.0e})")


def test_the_float_restatement_is_the_oracles_ssim():
    for h, w in S.shapes():
        p, t = S.float_frames(3, h, w)
        ssim = S.ssim_of(S.frame_ssim_f32_ref(p, t))[1]
        assert np.abs(ssim - _oracle(p, t)).max() <= ORACLE_TOL, (h, w)


def test_the_restatement_agrees_with_the_definition_per_channel():
    from oracle import render_eval_oracle as O
    for content in ("random", "smooth", "channels"):
        a, b = S.frames(content, 1, 8, 13)
        ch = S.ssim_of(S.frame_ssim_ref(a, b))[0][0]
        for c in range(3):
            want = O.ssim_by_definition(a[0, ..., c] / 255.0, b[0, ..., c] / 255.0)
            assert abs(ch[c] - want) <= ORACLE_TOL, (content, c, ch[c], want)
    a, b = S.frames("channels", 1, 8, 13)
    ch = S.ssim_of(S.frame_ssim_ref(a, b))[0][0]
    assert ch[0] == 1.0 and ch[1] < -0.5 and abs(ch[2]) < 0.5, "the three channels differ strongly"


def test_the_hole_rule_against_a_loop_over_windows():
    """The cumulative-sum count against 49 explicit depth values per window, and the masks are neither vacuous nor total."""
    th, tw = S.TILE
    for kind in S.HOLES:
        for h, w in ((39, 70), (th + 7, 2 * tw + 7), (2 * th + 6, tw + 6)):
            d = S.holes(kind, 3, h, w)
            cnt = S.counting((3, h, w), d)
            want = np.array([[[bool((d[f, y:y + 7, x:x + 7] != 0).all()) for x in range(w - 6)] for y in range(h - 6)] for f in range(3)])
            assert np.array_equal(cnt, want), (kind, h, w)
            per = cnt.reshape(3, -1).sum(1)
            total = (h - 6) * (w - 6)
            if kind == "frame":
                assert per.tolist() == [total, 0, total]
            else:
                assert ((0 < per) & (per < total)).all(), (kind, h, w, per)
            if kind == "corner":
                assert (per == total - 1).all()
            if kind == "seam" and (h, w) == (39, 70):
                assert (per == total - 49).all() and not cnt[0, th - 4:th + 3, tw - 4:tw + 3].any()
