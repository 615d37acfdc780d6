"""GPU checks of the frames-out path: k_camera_rays, k_pack_frames and k_frame_errors (csrc/frames_out_kernels.hip) against the numpy
references of tests/frames_out_ref.py and against k_target_rays, and SceneStream / SceneGroup.render_frames and score_frames
(nerf-det_amd/streaming.py) against render_rays on the generated rays and frame_errors of the hand-composed held-out frames.

Every comparison is bit for bit: the kernels' arithmetic is fixed operation by operation (include/nerfdet_hip.h), the error sums are
integers, and the stream methods promise the bits of the calls they are made of."""
from ctypes import c_void_p

import numpy as np
import pytest
import torch

import frames_out_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
# psnr is the float64 formula evaluated by torch on the device: the quotient is correctly rounded on both sides, log10 is within a few
# ulp of the exact value in the device's and in the host's library alike, so the two agree to a few parts in 10^16; inf and nan must match
PSNR_RTOL = 1e-14


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _k33(krows):
    k = np.eye(3, dtype=F)
    k[:2] = krows
    return k


# ---- rays ----
def test_camera_rays_equal_target_rays_and_the_reference(device):
    """3 cameras, a 20 x 28 grid with margin 3: window (3, 3, 14, 22) gives k_target_rays' raydirs and lightpos, and the reference's bits;
    924 rays a launch, not a multiple of 256."""
    from nerfdet_amd import _lib, pipeline as P
    from nerfdet_amd._lib import _ptr, check
    krows, rot, lpos = R.cameras(3)
    n, h, w, m = 3, 20, 28, 3
    got_o, got_d = P.camera_rays(_k33(krows), R.c2w_of(rot, lpos), (m, m, h - 2 * m, w - 2 * m), device=device)
    assert got_o.shape == got_d.shape == (n, 14 * 22, 3) and got_d.dtype == torch.float32 and (n * 14 * 22) % 256 != 0
    frames = torch.zeros((n, h, w, 3), dtype=torch.uint8, device=device)
    tids = torch.arange(n, dtype=torch.int32, device=device)
    raydirs = torch.empty((n, 14 * 22, 3), dtype=torch.float32, device=device)
    lightpos, gt = torch.empty_like(raydirs), torch.empty_like(raydirs)
    mean, std = np.asarray(P.IMG_MEAN, dtype=np.float64), np.asarray(P.IMG_STD, dtype=np.float64)
    kd, rd, ld = _dev(krows, device), _dev(rot, device), _dev(lpos, device)
    check(_lib.load().ndet_target_rays(_ptr(frames), _ptr(tids), n, h, w, m, _ptr(kd), _ptr(rd), _ptr(ld), mean.ctypes.data_as(c_void_p),
                                       std.ctypes.data_as(c_void_p), _ptr(raydirs), _ptr(lightpos), _ptr(gt), c_void_p(_lib.raw_stream(device))),
          "target_rays")
    assert torch.equal(got_d, raydirs) and torch.equal(got_o, lightpos)
    ref_o, ref_d = R.camera_rays_ref(krows, rot, lpos, (m, m, 14, 22))
    assert np.array_equal(got_d.cpu().numpy(), ref_d) and np.array_equal(got_o.cpu().numpy(), ref_o)
    assert float(got_d.abs().max()) > 0.3


def test_strided_rays_are_the_subsample_and_a_single_ray(device):
    from nerfdet_amd import pipeline as P
    krows, rot, lpos = R.cameras(2, seed=1)
    k, c2w = _k33(krows), R.c2w_of(rot, lpos)
    full_o, full_d = P.camera_rays(k, c2w, (0, 0, 20, 28), device=device)
    o, d = P.camera_rays(k, c2w, (1, 1, 7, 9), 3, device=device)
    assert d.shape == (2, 63, 3)
    assert torch.equal(d.view(2, 7, 9, 3), full_d.view(2, 20, 28, 3)[:, 1::3, 1::3]) and torch.equal(o, full_o[:, :63])
    assert np.array_equal(d.cpu().numpy(), R.camera_rays_ref(krows, rot, lpos, (1, 1, 7, 9), 3)[1])
    # one ray, outside any image: no bound
    o1, d1 = P.camera_rays(k, torch.from_numpy(c2w[1:]), (500, 700, 1, 1), 5, device=device)
    ref = R.camera_rays_ref(krows, rot[1:], lpos[1:], (500, 700, 1, 1), 5)
    assert o1.shape == d1.shape == (1, 1, 3) and np.array_equal(d1.cpu().numpy(), ref[1]) and np.array_equal(o1.cpu().numpy(), ref[0])
    # a 4 x 4 intrinsic and a list of tensors are taken as well
    k44 = np.eye(4, dtype=F)
    k44[:3, :3] = k
    o2, d2 = P.camera_rays(torch.from_numpy(k44), [torch.from_numpy(m) for m in c2w], (0, 0, 20, 28), device=device)
    assert torch.equal(d2, full_d) and torch.equal(o2, full_o)


# ---- pack ----
@pytest.mark.parametrize("with_mask", [False, True])
def test_pack_frames_equals_the_reference(device, with_mask):
    """The edge vector plus 1000 seeded values, walked in calls of R = 255 and R = 257 rows; R = 1 on every row of specials."""
    from nerfdet_amd import pipeline as P
    c, d, m = R.pack_inputs()
    want_b, want_d = R.pack_frames_ref(c, d, m if with_mask else None)
    assert want_d[:18].any() and (not with_mask or not want_d[18:36].any())
    cd, dd, md = _dev(c, device), _dev(d, device), _dev(m, device)
    rows = c.shape[0]
    spans = [(at, min(at + r, rows)) for r in (255, 257) for at in range(0, rows, r)] + [(i, i + 1) for i in range(36)]
    assert {b - a for a, b in spans} >= {1, 255, 257}
    for a, b in spans:
        frames, mm = P.pack_frames(cd[a:b], dd[a:b], md[a:b] if with_mask else None, (1, 1, b - a))
        assert frames.shape == (1, 1, b - a, 3) and frames.dtype == torch.uint8 and mm.shape == (1, 1, b - a) and mm.dtype == torch.uint16
        assert np.array_equal(frames.cpu().numpy().reshape(-1, 3), want_b[a:b]), (a, b)
        assert np.array_equal(mm.cpu().numpy().reshape(-1), want_d[a:b]), (a, b)
    # shapes: (n, h, w) over flat rows
    frames, mm = P.pack_frames(cd[:24], dd[:24], None, (2, 3, 4))
    assert frames.shape == (2, 3, 4, 3) and np.array_equal(frames.cpu().numpy().reshape(-1, 3), want_b[:24])


# ---- errors ----
@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (3, 1, 257), (2, 64, 96)])
def test_frame_errors_equal_the_reference(device, n, h, w):
    from nerfdet_amd import pipeline as P
    a, b, da, db = R.errors_inputs(n, h, w)
    if n > 1:
        da[1] = 0                                           # a frame the render has no depth for: four zeros
    want = R.frame_errors_ref(a, b, da, db)
    ad, bd, dad, dbd = (_dev(x, device) for x in (a, b, da, db))
    got = P.frame_errors(ad, bd, dad, dbd)
    out = np.stack([got[k].cpu().numpy() for k in ("sse", "n_px", "depth_sad_mm", "n_depth")], axis=1)
    assert out.dtype == np.int64 and np.array_equal(out, want), (out, want)
    assert got["psnr"].dtype == torch.float64
    np.testing.assert_allclose(got["psnr"].cpu().numpy(), R.psnr_ref(want[:, 0], want[:, 1]), rtol=PSNR_RTOL, atol=0)
    if n > 1:
        assert not out[1].any() and np.isnan(got["psnr"][1].item()) and out[0].all()
    again = P.frame_errors(ad, bd, dad, dbd)
    assert all(torch.equal(again[k], got[k]) for k in ("sse", "n_px", "depth_sad_mm", "n_depth")), "two calls write the same bytes"
    none = P.frame_errors(ad, bd, dad)
    assert np.array_equal(torch.stack([none["sse"], none["n_px"]], 1).cpu().numpy(), want[:, :2])
    assert not none["depth_sad_mm"].any() and not none["n_depth"].any()
    same = P.frame_errors(ad, ad.clone(), dad, dad.clone())
    assert not same["sse"].any() and not same["depth_sad_mm"].any() and torch.equal(same["n_px"], got["n_px"])
    assert torch.equal(same["n_depth"], same["n_px"])
    seen = same["n_px"] > 0
    assert bool(torch.isinf(same["psnr"][seen]).all()) and bool(torch.isnan(same["psnr"][~seen]).all())


# ---- streams ----
def _scenes(device):
    from test_group_render_gpu import _det_scenes
    return _det_scenes(device)


def _chunk_meta(meta, v0, v1):
    m = dict(meta)
    m["lidar2img"] = dict(meta["lidar2img"], extrinsic=list(meta["lidar2img"]["extrinsic"][v0:v1]))
    return m


def _stream(det, sc, splits=((0, 2), (2, 3), (3, 6)), **kw):
    scene = det.begin_scene(dict(sc["meta"]), keep_views=True, **kw)
    for v0, v1 in splits:
        scene.add_views(sc["img"][:, v0:v1], sc["dn"][:, v0:v1], _chunk_meta(sc["meta"], v0, v1))
    return scene


def _k_scaled(meta):
    k = np.array(meta["lidar2img"]["intrinsic"], dtype=F)
    k[:2] = k[:2] / (meta["ori_shape"][0] / meta["img_shape"][0])
    return k


def _c2w(ext):
    return np.linalg.inv(np.stack(ext).astype(np.float64)).astype(F)


def _same(got, want, what, keys=("rgb", "depth", "mask")):
    for key in keys:
        assert got[key].shape == want[key].shape and got[key].dtype == want[key].dtype, f"{what}: {key} {tuple(got[key].shape)} vs {tuple(want[key].shape)}"
        assert torch.equal(got[key], want[key]), f"{what}: {key} differs"


def _packed(out, what):
    """``frames`` / ``depth_frames`` of a render_frames dict are the reference's pack of its float outputs."""
    b, d = R.pack_frames_ref(out["rgb"].cpu().numpy(), out["depth"].cpu().numpy(), out["mask"].cpu().numpy())
    assert out["frames"].dtype == torch.uint8 and out["depth_frames"].dtype == torch.uint16
    assert np.array_equal(out["frames"].cpu().numpy(), b), f"{what}: frames"
    assert np.array_equal(out["depth_frames"].cpu().numpy(), d), f"{what}: depth_frames"
    assert not d[~out["mask"].cpu().numpy()].any() and d.any() and b.any()


def test_render_frames_equals_render_rays_on_the_camera_rays(device):
    """Two cameras of 64 x 96: 12 288 rays, two passes.  The detections and the bank are what they were."""
    from nerfdet_amd import pipeline as P, rays
    det, scenes = _scenes(device)
    sc = scenes[0]
    scene = _stream(det, sc)
    ext = sc["meta"]["lidar2img"]["extrinsic"][1:3]
    before = [(s.feat.clone(), s.rgb4.clone(), s.ke.clone()) for s in scene.bank.segments]
    det_before = scene.detect()
    out = scene.render_frames(extrinsic=ext)
    o, d = P.camera_rays(_k_scaled(sc["meta"]), _c2w(ext), (0, 0, 64, 96), device=device)
    assert o.shape[0] * o.shape[1] == 12288 > rays.RENDER_TESTING_RAYS
    want = scene.render_rays(o.view(-1, 3), d.view(-1, 3))
    assert list(out) == ["frames", "depth_frames", "rgb", "depth", "mask"]
    assert out["frames"].shape == (2, 64, 96, 3) and out["depth_frames"].shape == (2, 64, 96) and out["rgb"].shape == (2, 64, 96, 3)
    _same({k: out[k].reshape(want[k].shape) for k in want}, want, "render_frames")
    _packed(out, "render_frames")
    assert out["mask"].any()
    _same(scene.render_frames(c2w=_c2w(ext)), out, "c2w instead of extrinsic", keys=("frames", "depth_frames", "rgb", "depth", "mask"))
    det_after = scene.detect()
    for a, b in zip(det_before, det_after):
        assert torch.equal(a["labels_3d"], b["labels_3d"]) and torch.equal(a["scores_3d"], b["scores_3d"]) and torch.equal(a["boxes_3d"].tensor, b["boxes_3d"].tensor)
    assert len(scene.bank.segments) == len(before) == 3
    for s, (f, i, k) in zip(scene.bank.segments, before):
        assert torch.equal(s.feat, f) and torch.equal(s.rgb4, i) and torch.equal(s.ke, k)


def test_render_frames_fine_pass_and_thumbnail(device):
    from nerfdet_amd import pipeline as P
    det, scenes = _scenes(device)
    sc = scenes[0]
    scene = _stream(det, sc)
    ext = sc["meta"]["lidar2img"]["extrinsic"][1:3]
    k, c2w = _k_scaled(sc["meta"]), _c2w(ext)
    o, d = P.camera_rays(k, c2w, (0, 0, 64, 96), device=device)
    fine = scene.render_frames(extrinsic=ext, n_importance=8)
    want = scene.render_rays(o.view(-1, 3), d.view(-1, 3), n_importance=8)
    assert list(fine) == ["frames", "depth_frames", "rgb", "depth", "mask", "coarse"] and list(fine["coarse"]) == list(fine)[:5]
    _same({key: fine[key].reshape(want[key].shape) for key in ("rgb", "depth", "mask")}, want, "fine pass")
    _same({key: fine["coarse"][key].reshape(want["coarse"][key].shape) for key in ("rgb", "depth", "mask")}, want["coarse"], "coarse pass")
    _packed(fine, "fine pass")
    _packed(fine["coarse"], "coarse pass")
    assert not torch.equal(fine["rgb"], fine["coarse"]["rgb"])
    # stride 4: a 16 x 24 thumbnail through pixels 2, 6, ...
    thumb = scene.render_frames(extrinsic=ext, stride=4)
    assert thumb["frames"].shape == (2, 16, 24, 3) and thumb["depth_frames"].shape == (2, 16, 24) and thumb["mask"].shape == (2, 16, 24)
    to, td = P.camera_rays(k, c2w, (2, 2, 16, 24), 4, device=device)
    assert torch.equal(td.view(2, 16, 24, 3), d.view(2, 64, 96, 3)[:, 2::4, 2::4]) and torch.equal(to, o[:, :16 * 24])
    want = scene.render_rays(to.view(-1, 3), td.view(-1, 3))
    _same({key: thumb[key].reshape(want[key].shape) for key in want}, want, "thumbnail")
    _packed(thumb, "thumbnail")
    # a window of its own, partly outside the image
    win = scene.render_frames(c2w=c2w[:1], window=(60, 90, 5, 9), stride=2)
    wo, wd = P.camera_rays(k, c2w[:1], (60, 90, 5, 9), 2, device=device)
    want = scene.render_rays(wo.view(-1, 3), wd.view(-1, 3))
    assert win["frames"].shape == (1, 5, 9, 3)
    _same({key: win[key].reshape(want[key].shape) for key in want}, want, "window")


@pytest.mark.parametrize("stride", [1, 4])
def test_score_frames_equals_frame_errors_of_the_hand_composed_frames(device, stride):
    """Two held-out 128 x 192 frames with 60 x 80 depth frames against the render of their poses."""
    from nerfdet_amd import pipeline as P
    det, scenes = _scenes(device)
    sc = scenes[0]
    scene = _stream(det, sc)
    rs = np.random.RandomState(5)
    frames = _dev(rs.randint(0, 256, (1, 2, 128, 192, 3)).astype(np.uint8), device)
    depth_np = (rs.randint(300, 6000, (1, 2, 60, 80)) * (rs.rand(1, 2, 60, 80) > 0.2)).astype(np.uint16)
    depth_frames = _dev(depth_np, device)
    chunk = _chunk_meta(sc["meta"], 4, 6)
    n_before = scene.n_views
    got = scene.score_frames(frames, chunk, depth_frames=depth_frames, stride=stride)
    assert scene.n_views == n_before == scene.bank.n_views
    o = stride // 2
    u8 = P.prepare_frames(frames[0], (96, 64), (64, 96), want_u8=True)[2][:, o:64:stride, o:96:stride].contiguous()
    metres = P.prepare_depth_frames(depth_frames[0], (64, 96))[:, o::stride, o::stride]
    held_mm = R.pack_frames_ref(np.zeros(metres.shape + (3,), dtype=F), metres.cpu().numpy().astype(F))[1]
    out = scene.render_frames(extrinsic=chunk["lidar2img"]["extrinsic"], stride=stride)
    assert out["frames"].shape == u8.shape == (2, 64 // stride, 96 // stride, 3)
    want = P.frame_errors(out["frames"], u8, out["depth_frames"], _dev(held_mm, device))
    ref = R.frame_errors_ref(out["frames"].cpu().numpy(), u8.cpu().numpy(), out["depth_frames"].cpu().numpy(), held_mm)
    for i, key in enumerate(("sse", "n_px", "depth_sad_mm", "n_depth")):
        assert got[key].dtype == torch.int64 and torch.equal(got[key], want[key]), key
        assert np.array_equal(got[key].cpu().numpy(), ref[:, i]), key
    np.testing.assert_allclose(got["psnr"].cpu().numpy(), R.psnr_ref(ref[:, 0], ref[:, 1]), rtol=PSNR_RTOL, atol=0)
    print(f"stride {stride}: sse {ref[:, 0].tolist()}, n_px {ref[:, 1].tolist()}, sad_mm {ref[:, 2].tolist()}, n_depth {ref[:, 3].tolist()}, "
          f"psnr {got['psnr'].tolist()}")
    assert ref[:, 1].all() and ref[:, 3].all() and (ref[:, 3] <= ref[:, 1]).all() and np.isfinite(got["psnr"].cpu().numpy()).all()
    no_depth = scene.score_frames(frames, chunk, stride=stride)
    assert torch.equal(no_depth["sse"], got["sse"]) and torch.equal(no_depth["n_px"], got["n_px"]) and not no_depth["n_depth"].any()


# ---- groups ----
def test_group_render_frames_equals_group_render_rays(device):
    """Scenes 2 and 0 with 2 and 1 cameras: per scene the bits of group.render_rays on its generated rays; and scored frames per scene."""
    from nerfdet_amd import pipeline as P
    from test_group_render_gpu import CALLS, _feed
    det, scenes = _scenes(device)
    group = _feed(det.begin_scenes([dict(sc["meta"]) for sc in scenes], keep_views=True), scenes, CALLS)
    listed = [2, 0]
    exts = [scenes[2]["meta"]["lidar2img"]["extrinsic"][0:2], scenes[0]["meta"]["lidar2img"]["extrinsic"][3:4]]
    got = group.render_frames(extrinsic=exts, scenes=listed)
    rays_ = [P.camera_rays(_k_scaled(scenes[s]["meta"]), _c2w(e), (0, 0, 64, 96), device=device) for s, e in zip(listed, exts)]
    want = group.render_rays([o.view(-1, 3) for o, _ in rays_], [d.view(-1, 3) for _, d in rays_], scenes=listed)
    assert len(got) == 2 and got[0]["frames"].shape == (2, 64, 96, 3) and got[1]["frames"].shape == (1, 64, 96, 3)
    for i, s in enumerate(listed):
        _same({k: got[i][k].reshape(want[i][k].shape) for k in want[i]}, want[i], f"scene {s}")
        _packed(got[i], f"scene {s}")
    alone = group.render_frames(c2w=[_c2w(exts[0])], scenes=[2])
    _same(alone[0], got[0], "scene 2 alone", keys=("frames", "depth_frames", "rgb", "depth", "mask"))
    # score_frames: one row of 2 held-out frames per listed scene
    rs = np.random.RandomState(6)
    frames = _dev(rs.randint(0, 256, (2, 2, 128, 192, 3)).astype(np.uint8), device)
    depth_frames = _dev((rs.randint(300, 6000, (2, 2, 60, 80)) * (rs.rand(2, 2, 60, 80) > 0.2)).astype(np.uint16), device)
    metas = [_chunk_meta(scenes[s]["meta"], 1, 3) for s in listed]
    scored = group.score_frames(frames, metas, scenes=listed, depth_frames=depth_frames, stride=4)
    outs = group.render_frames(extrinsic=[m["lidar2img"]["extrinsic"] for m in metas], scenes=listed, stride=4)
    u8 = P.prepare_frames(frames.view(4, 128, 192, 3), (96, 64), (64, 96), want_u8=True)[2][:, 2:64:4, 2:96:4].contiguous()
    mm = P.depth_to_mm(P.prepare_depth_frames(depth_frames.view(4, 60, 80), (64, 96))[:, 2::4, 2::4].contiguous())
    for i in range(2):
        want_i = P.frame_errors(outs[i]["frames"], u8[2 * i:2 * i + 2], outs[i]["depth_frames"], mm[2 * i:2 * i + 2])
        for key in ("sse", "n_px", "depth_sad_mm", "n_depth"):
            assert torch.equal(scored[i][key], want_i[key]), (i, key)
        assert scored[i]["n_px"].all()


def test_group_of_one_is_a_scene_stream(device):
    from test_group_render_gpu import _feed
    det, scenes = _scenes(device)
    sc = scenes[1]
    group = _feed(det.begin_scenes([dict(sc["meta"])], keep_views=True), [sc], [[(0, 0, 6)]])
    stream = _stream(det, sc, splits=((0, 6),))
    ext = sc["meta"]["lidar2img"]["extrinsic"][2:4]
    keys = ("frames", "depth_frames", "rgb", "depth", "mask")
    for kw in (dict(), dict(stride=4, n_importance=8)):
        got, want = group.render_frames(extrinsic=[ext], **kw)[0], stream.render_frames(extrinsic=ext, **kw)
        assert list(got) == list(want)
        _same(got, want, f"group of one {kw}", keys=keys)
        if "coarse" in want:
            _same(got["coarse"], want["coarse"], "group of one, coarse", keys=keys)
    assert want["mask"].any()


def test_a_windowed_group_renders_frames_as_a_fresh_one(device):
    """window=2 fed a, b, c renders the frames a fresh windowed group fed b, c renders."""
    from test_group_render_gpu import _feed
    det, scenes = _scenes(device)
    metas = [dict(sc["meta"]) for sc in scenes]
    a, b, c = [[(s, v0, v1) for s in range(3)] for v0, v1 in ((0, 2), (2, 4), (4, 6))]
    group = _feed(det.begin_scenes(metas, window=2, keep_views=True), scenes, [a, b, c])
    fresh = _feed(det.begin_scenes(metas, window=2, keep_views=True), scenes, [b, c])
    exts = [sc["meta"]["lidar2img"]["extrinsic"][0:1 + s % 2] for s, sc in enumerate(scenes)]
    got, want = group.render_frames(extrinsic=exts, stride=2), fresh.render_frames(extrinsic=exts, stride=2)
    for s in range(3):
        assert got[s]["frames"].shape == (1 + s % 2, 32, 48, 3)
        _same(got[s], want[s], f"scene {s}", keys=("frames", "depth_frames", "rgb", "depth", "mask"))
        assert got[s]["mask"].any()
