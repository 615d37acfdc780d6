"""The frame SSIM on the device (csrc/frame_ssim_kernels.hip): pipeline.frame_ssim's byte form against the numpy restatement of
tests/frame_ssim_ref.py BIT FOR BIT (every box sum is an integer, the window expression five float64 lines, the frame's sum an integer of
2^-40), its float form and rays.ssim_views against oracle/render_eval_oracle.py and rays.compute_ssim to 1e-10, and
SceneStream / SceneGroup.score_frames(ssim=True) against frame_ssim of the hand-composed frames.

The float bound: the float64 box sums carry at most 49 * 2^-53 relative error on terms of O(49); divided by C2 * 49 * 48 = 8.5 that is below
1e-13 a window, the quantisation adds 2^-41, the oracle's own float64 rounding over C2 = 3.6e-3 about as much: 1e-10 leaves two decades."""
import numpy as np
import pytest
import torch

import frame_ssim_ref as S

pytestmark = pytest.mark.gpu
F = np.float32
FLOAT_TOL = 1e-10
_CACHE = {}


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _np(out):
    return np.concatenate([out["ssim_sum"].cpu().numpy(), out["n_windows"].cpu().numpy()[:, None]], axis=1)


def _check_bits(got, want, what):
    """``got``: a frame_ssim dict; ``want``: the restatement's (n, 4).  Sums and counts to the bit, the float64 outputs exactly, nan matching."""
    assert got["ssim_sum"].dtype == torch.int64 and got["n_windows"].dtype == torch.int64
    assert got["ssim_channels"].dtype == torch.float64 and got["ssim"].dtype == torch.float64
    g = _np(got)
    assert np.array_equal(g, want), f"{what}: sums\n{g}\nwant\n{want}"
    ch, ssim = S.ssim_of(want)
    assert np.array_equal(got["ssim_channels"].cpu().numpy(), ch, equal_nan=True), f"{what}: ssim_channels"
    assert np.array_equal(got["ssim"].cpu().numpy(), ssim, equal_nan=True), f"{what}: ssim"


def test_the_tile_is_the_one_the_shapes_are_made_for():
    from nerfdet_amd import pipeline as P
    assert P.SSIM_TILE == S.TILE
    th, tw = P.SSIM_TILE
    assert (th + 7, 2 * tw + 7) in S.shapes() and (2 * th + 6, tw + 6) in S.shapes()


@pytest.mark.parametrize("content", S.CONTENTS)
@pytest.mark.parametrize("h,w", S.shapes())
def test_bytes_equal_the_restatement_bit_for_bit(device, h, w, content):
    from nerfdet_amd import pipeline as P
    for n in (3, 1):
        a, b = S.frames(content, n, h, w)
        want = S.frame_ssim_ref(a, b)
        got = P.frame_ssim(_dev(a, device), _dev(b, device))
        _check_bits(got, want, f"{content} {n} x {h} x {w}")
        assert (want[:, 3] == (h - 6) * (w - 6)).all()
        if content == "equal":
            assert (want[:, :3] == want[:, 3:] * 2 ** 40).all() and bool((got["ssim"] == 1.0).all())
        if content == "inverted" and h * w > 49:
            assert (want[:, :3] < 0).all(), "negative q"
        if content == "extremes":
            assert (want[:, :3] > 0).all() and bool((got["ssim"] < 1e-3).all())
    if content == "smooth" and (h, w) == (39, 70):
        print(f"smooth 39 x 70: ssim {got['ssim'].tolist()}")
        assert 0.9 < float(got["ssim"][0]) < 1.0


@pytest.mark.parametrize("kind", S.HOLES)
@pytest.mark.parametrize("h,w", [(39, 70), (S.TILE[0] + 7, 2 * S.TILE[1] + 7), (2 * S.TILE[0] + 6, S.TILE[1] + 6)])
def test_holes_remove_the_windows_that_touch_them(device, h, w, kind):
    from nerfdet_amd import pipeline as P
    th, tw = P.SSIM_TILE
    total = (h - 6) * (w - 6)
    for content in ("random", "inverted"):
        a, b = S.frames(content, 3, h, w)
        d = S.holes(kind, 3, h, w)
        want = S.frame_ssim_ref(a, b, d)
        got = P.frame_ssim(_dev(a, device), _dev(b, device), _dev(d, device))
        _check_bits(got, want, f"{kind} {content} {h} x {w}")
        n_w = want[:, 3]
        if kind == "frame":
            assert n_w.tolist() == [total, 0, total]
            assert bool(torch.isnan(got["ssim"][1])) and bool(torch.isnan(got["ssim_channels"][1]).all()) and not want[1].any()
            whole = S.frame_ssim_ref(a, b)
            assert np.array_equal(want[[0, 2]], whole[[0, 2]]), "the neighbours of the empty frame are unaffected"
        else:
            assert ((0 < n_w) & (n_w < total)).all(), "the mask is neither vacuous nor total"
        if kind == "corner":
            assert (n_w == total - 1).all()
        if kind == "seam" and (h, w) == (39, 70):
            assert (n_w == total - 49).all()
    none = P.frame_ssim(_dev(a, device), _dev(b, device), _dev(np.ones((3, h, w), dtype=np.uint16), device))
    _check_bits(none, S.frame_ssim_ref(a, b), "a depth frame without holes")


def test_two_calls_and_any_place_in_the_batch_give_the_same_bytes(device):
    from nerfdet_amd import pipeline as P
    th, tw = P.SSIM_TILE
    h, w = th + 7, 2 * tw + 7
    a, b = S.frames("random", 3, h, w)
    d = S.holes("seam", 3, h, w)
    ad, bd, dd = _dev(a, device), _dev(b, device), _dev(d, device)
    first, second = P.frame_ssim(ad, bd, dd), P.frame_ssim(ad, bd, dd)
    for key in ("ssim_sum", "n_windows"):
        assert torch.equal(first[key], second[key]), key
    alone = P.frame_ssim(ad[2:3].contiguous(), bd[2:3].contiguous(), dd[2:3].contiguous())
    assert torch.equal(alone["ssim_sum"][0], first["ssim_sum"][2]) and torch.equal(alone["n_windows"][0], first["n_windows"][2])
    assert not torch.equal(first["ssim_sum"][0], first["ssim_sum"][2]), "the frames differ"


# ---- float form ----
def _oracle(p, t):
    from oracle import render_eval_oracle as O
    return np.array([O.ssim(p[f], t[f]) for f in range(p.shape[0])])


@pytest.mark.parametrize("h,w", S.shapes())
def test_float_views_against_the_oracle_and_compute_ssim(device, h, w):
    from nerfdet_amd import pipeline as P, rays
    p, t = S.float_frames(3, h, w)
    pd, td = _dev(p, device), _dev(t, device)
    got = rays.ssim_views(pd, td)
    assert got.dtype == torch.float64 and got.shape == (3,)
    want = _oracle(p, t)
    glue = torch.stack([rays.compute_ssim(pd[v], td[v]) for v in range(3)]).cpu().numpy()
    e_oracle, e_glue = np.abs(got.cpu().numpy() - want).max(), np.abs(got.cpu().numpy() - glue).max()
    print(f"{h} x {w}: ssim {got.tolist()}, |fused - oracle| {e_oracle:.3e}, |fused - compute_ssim| {e_glue:.3e} (bound {FLOAT_TOL:.0e})")
    assert e_oracle <= FLOAT_TOL and e_glue <= FLOAT_TOL
    full = P.frame_ssim(pd, td)
    assert (full["n_windows"] == (h - 6) * (w - 6)).all()
    ref = S.ssim_of(S.frame_ssim_f32_ref(p, t))[0]
    assert np.abs(full["ssim_channels"].cpu().numpy() - ref).max() <= FLOAT_TOL
    # the same bytes call to call and at any place in the batch
    again = P.frame_ssim(pd, td)
    alone = P.frame_ssim(pd[2:3].contiguous(), td[2:3].contiguous())
    assert torch.equal(full["ssim_sum"], again["ssim_sum"]) and torch.equal(alone["ssim_sum"][0], full["ssim_sum"][2])
    # a byte frame scored as floats x / 255 is the byte form within the bound
    a, b = S.frames("smooth", 2, h, w)
    as_float = P.frame_ssim(_dev(a.astype(F) / F(255), device), _dev(b.astype(F) / F(255), device))["ssim"].cpu().numpy()
    assert np.abs(as_float - _oracle(a.astype(F) / F(255), b.astype(F) / F(255))).max() <= FLOAT_TOL


def test_float_views_with_holes(device):
    from nerfdet_amd import pipeline as P
    th, tw = P.SSIM_TILE
    h, w = th + 7, 2 * tw + 7
    p, t = S.float_frames(3, h, w)
    for kind in ("seam", "frame"):
        d = S.holes(kind, 3, h, w)
        got = P.frame_ssim(_dev(p, device), _dev(t, device), _dev(d, device))
        want = S.frame_ssim_f32_ref(p, t, d)
        assert np.array_equal(got["n_windows"].cpu().numpy(), want[:, 3])
        ch = S.ssim_of(want)[0]
        gch = got["ssim_channels"].cpu().numpy()
        assert np.array_equal(np.isnan(gch), np.isnan(ch)) and np.nanmax(np.abs(gch - ch)) <= FLOAT_TOL
        if kind == "frame":
            assert np.isnan(gch[1]).all() and want[1, 3] == 0
        else:
            assert ((0 < want[:, 3]) & (want[:, 3] < (h - 6) * (w - 6))).all()


def test_rendering_metrics_fused_against_the_loop(device):
    from nerfdet_amd import rays
    p, t = S.float_frames(3, 39, 70)
    rs = np.random.RandomState(3)
    rendered = {"outputs_coarse": {"rgb": _dev(p, device), "depth": _dev(rs.rand(3, 39, 70, 1).astype(F), device)},
                "gt_rgb": _dev(t, device), "gt_depth": _dev(rs.rand(3, 39, 70, 1).astype(F), device)}
    psnr, ssim, err = rays.rendering_metrics(rendered)
    psnr_f, ssim_f, err_f = rays.rendering_metrics(rendered, fused=True)
    assert torch.equal(psnr, psnr_f) and torch.equal(err, err_f)
    assert abs(float(ssim) - float(ssim_f)) <= FLOAT_TOL and 0.0 < float(ssim_f) < 1.0
    rendered["gt_depth"] = None
    assert rays.rendering_metrics(rendered, fused=True)[2] is None


# ---- streams and groups: the small streamed rig of the frames-out tests, rebuilt here ----
def _rig(device):
    """A small detector and three scenes of synth.train_scene(6, (64, 96)) with their own seeds, origins and cameras; made once."""
    key = str(device)
    if key not in _CACHE:
        from nerfdet_amd import synth
        from nerfdet_amd.config import _wrap
        from nerfdet_amd.presets import nerfdet_cfg
        from nerfdet_amd.registry import build_detector
        torch.manual_seed(0)
        cfg = _wrap(nerfdet_cfg(50, n_voxels=(16, 16, 8), voxel_size=(0.4, 0.4, 0.4)))
        cfg["test_cfg"]["nms_pre"] = 200
        det = build_detector(cfg["model"], train_cfg=cfg["train_cfg"], test_cfg=cfg["test_cfg"])
        with torch.no_grad():
            det.neck.fpn_convs[0].conv.weight.mul_(1 / 30.0)
            det.nerf_mlp.mlp.sigma_layer.output_layer.bias.fill_(2.0)
        det = det.to(device).eval()
        scenes = []
        for i in range(3):
            batch = synth.batch_to(synth.train_scene(6, (64, 96), t_views=2, n_boxes=2, seed=4 + i), device)
            meta = batch["img_metas"][0]
            meta["lidar2img"]["origin"] = np.asarray(meta["lidar2img"]["origin"], dtype=F) + F([0.2 * i, -0.1 * i, 0.0])
            ext = meta["lidar2img"]["extrinsic"]
            meta["lidar2img"]["extrinsic"] = ext[2 * i:] + ext[:2 * i]
            scenes.append(dict(img=batch["img"], dn=batch["denorm_images"], meta=meta))
        _CACHE[key] = (det, scenes)
    return _CACHE[key]


def _chunk_meta(meta, v0, v1):
    m = dict(meta)
    m["lidar2img"] = dict(meta["lidar2img"], extrinsic=list(meta["lidar2img"]["extrinsic"][v0:v1]))
    return m


def _stream(det, sc, splits=((0, 2), (2, 3), (3, 6))):
    scene = det.begin_scene(dict(sc["meta"]), keep_views=True)
    for v0, v1 in splits:
        scene.add_views(sc["img"][:, v0:v1], sc["dn"][:, v0:v1], _chunk_meta(sc["meta"], v0, v1))
    return scene


def _held_frames(device, n, seed):
    rs = np.random.RandomState(seed)
    frames = _dev(rs.randint(0, 256, (n, 2, 128, 192, 3)).astype(np.uint8), device)
    depth = _dev((rs.randint(300, 6000, (n, 2, 60, 80)) * (rs.rand(n, 2, 60, 80) > 0.2)).astype(np.uint16), device)
    return frames, depth


SSIM_KEYS = ("ssim", "ssim_channels", "n_windows")
ERROR_KEYS = ("sse", "n_px", "depth_sad_mm", "n_depth", "psnr")


def _same_scores(got, want, keys, what):
    for key in keys:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (what, key)
        assert np.array_equal(got[key].cpu().numpy(), want[key].cpu().numpy(), equal_nan=True), (what, key)


@pytest.mark.parametrize("stride", [1, 4])
def test_score_frames_with_ssim_equals_frame_ssim_of_the_hand_composed_frames(device, stride):
    from nerfdet_amd import pipeline as P
    det, scenes = _rig(device)
    sc = scenes[0]
    scene = _stream(det, sc)
    frames, depth_frames = _held_frames(device, 1, 5)
    chunk = _chunk_meta(sc["meta"], 4, 6)
    plain = scene.score_frames(frames, chunk, depth_frames=depth_frames, stride=stride)
    got = scene.score_frames(frames, chunk, depth_frames=depth_frames, stride=stride, ssim=True)
    assert list(plain) == list(ERROR_KEYS) and list(got) == list(ERROR_KEYS + SSIM_KEYS)
    _same_scores(got, plain, ERROR_KEYS, "ssim=True leaves the other keys")
    o = stride // 2
    held = P.prepare_frames(frames[0], (96, 64), (64, 96), want_u8=True)[2][:, o:64:stride, o:96:stride].contiguous()
    out = scene.render_frames(extrinsic=chunk["lidar2img"]["extrinsic"], stride=stride)
    want = P.frame_ssim(out["frames"], held, out["depth_frames"])
    _same_scores(got, want, SSIM_KEYS, "score_frames(ssim=True)")
    ref = S.frame_ssim_ref(out["frames"].cpu().numpy(), held.cpu().numpy(), out["depth_frames"].cpu().numpy())
    assert np.array_equal(_np(want), ref)
    print(f"stride {stride}: n_windows {ref[:, 3].tolist()} of {(64 // stride - 6) * (96 // stride - 6)}, ssim {got['ssim'].tolist()}")
    assert (ref[:, 3] >= 1).all() and np.isfinite(got["ssim"].cpu().numpy()).all()
    _same_scores(scene.score_frames(frames, chunk, stride=stride, ssim=True), want, SSIM_KEYS, "without held-out depth")


def test_group_score_frames_with_ssim(device):
    from nerfdet_amd import pipeline as P
    det, scenes = _rig(device)
    group = det.begin_scenes([dict(sc["meta"]) for sc in scenes], keep_views=True)
    for v0, v1 in ((0, 2), (2, 3), (3, 6)):
        group.add_views(torch.cat([sc["img"][:, v0:v1] for sc in scenes]), torch.cat([sc["dn"][:, v0:v1] for sc in scenes]),
                        [_chunk_meta(sc["meta"], v0, v1) for sc in scenes])
    listed = [2, 0]
    frames, depth_frames = _held_frames(device, 2, 6)
    metas = [_chunk_meta(scenes[s]["meta"], 1, 3) for s in listed]
    plain = group.score_frames(frames, metas, scenes=listed, depth_frames=depth_frames)
    got = group.score_frames(frames, metas, scenes=listed, depth_frames=depth_frames, ssim=True)
    outs = group.render_frames(extrinsic=[m["lidar2img"]["extrinsic"] for m in metas], scenes=listed)
    held = P.prepare_frames(frames.view(4, 128, 192, 3), (96, 64), (64, 96), want_u8=True)[2][:, 0:64, 0:96].contiguous()
    assert len(got) == len(plain) == 2
    for i in range(2):
        assert list(got[i]) == list(ERROR_KEYS + SSIM_KEYS) and list(plain[i]) == list(ERROR_KEYS)
        _same_scores(got[i], plain[i], ERROR_KEYS, f"scene {listed[i]}: the other keys")
        want = P.frame_ssim(outs[i]["frames"], held[2 * i:2 * i + 2], outs[i]["depth_frames"])
        _same_scores(got[i], want, SSIM_KEYS, f"scene {listed[i]}")
        assert bool((got[i]["n_windows"] >= 1).all())
    # a group of one scene is the stream
    sc = scenes[1]
    one = det.begin_scenes([dict(sc["meta"])], keep_views=True)
    one.add_views(sc["img"], sc["dn"], [_chunk_meta(sc["meta"], 0, 6)])
    stream = _stream(det, sc, splits=((0, 6),))
    chunk = _chunk_meta(sc["meta"], 2, 4)
    g = one.score_frames(frames[:1], [chunk], depth_frames=depth_frames[:1], ssim=True)[0]
    s = stream.score_frames(frames[:1], chunk, depth_frames=depth_frames[:1], ssim=True)
    _same_scores(g, s, ERROR_KEYS + SSIM_KEYS, "a group of one")
    assert bool((s["n_windows"] >= 1).all())


def test_ssim_on_a_thumbnail_below_one_window_launches_nothing(device, monkeypatch):
    from nerfdet_amd import streaming
    det, scenes = _rig(device)
    sc = scenes[0]
    scene = _stream(det, sc)
    frames, depth_frames = _held_frames(device, 1, 5)
    chunk = _chunk_meta(sc["meta"], 4, 6)

    def refuse(*args, **kwargs):
        raise AssertionError("a launch in front of the ValueError")
    for name in ("prepare_frames", "prepare_depth_frames", "camera_rays", "pack_frames", "frame_errors", "frame_ssim"):
        monkeypatch.setattr(streaming, name, refuse)
    with pytest.raises(ValueError, match="ssim"):
        scene.score_frames(frames, chunk, depth_frames=depth_frames, stride=10, ssim=True)       # 6 x 9 pixels
    with pytest.raises(ValueError, match="ssim"):
        scene.score_frames(frames, chunk, stride=16, ssim=True)                                  # 4 x 6 pixels
