"""GPU checks of the depth-tested, labelled overlay: k_project_boxes_w and k_draw_overlay (csrc/detections_out_kernels.hip) against
tests/overlay_ref.py and against the kernels they extend, and the new keywords of SceneStream / SceneGroup.draw_detections
(nerf-det_amd/streaming.py) against the composed pipeline calls and against a flat wall one can reason about without the reference.

Every comparison is exact -- bytes, integers, float32 bit patterns: the edge's depth is fixed statement by statement
(include/nerfdet_hip.h), the line rule and the plates are integer rules.  tests/test_overlay_cpu.py checks that the inputs made here
(overlay_ref.projected_ref / depth_case / plate_case) reach every case of the rule."""
import numpy as np
import pytest
import torch

import detections_out_ref as D
import overlay_ref as O
from test_detections_out_gpu import _bits, _dev, _k33, _k_scaled, _result, _scenes

pytestmark = pytest.mark.gpu
F = np.float32


def _projected(device, **extra):
    """overlay_ref.projected_ref() on the device, as pipeline.project_boxes returns it."""
    ref = O.projected_ref()
    out = {key: _dev(ref[key], device) for key in ("edges", "edge_mask", "rect", "zrange", "edge_w")}
    out.update(window=O.WINDOW, stride=1, **extra)
    return out


# ---- the projection with reciprocal depths ----
@pytest.mark.parametrize("stride", [1, 2])
def test_projection_with_depths_equals_the_old_entry_and_the_reference(device, stride):
    from nerfdet_amd import pipeline as P
    krows, w2c, corners = O.projection_case()
    assert corners.shape == (36, 8, 3) and w2c.shape[0] == 2
    old = P.project_boxes(_k33(krows), corners, O.WINDOW, stride, extrinsic=w2c, device=device)
    new = P.project_boxes(_k33(krows), corners, O.WINDOW, stride, extrinsic=w2c, device=device, depths=True)
    assert "edge_w" not in old and list(new)[:len(old)] == list(old)
    for key in ("edges", "edge_mask", "rect", "zrange"):
        assert np.array_equal(_bits(new[key]), _bits(old[key])), key
    want = O.projected_ref(stride)
    assert np.array_equal(_bits(new["edges"]), want["edges"]) and np.array_equal(_bits(new["edge_mask"]), want["edge_mask"])
    w = new["edge_w"]
    assert w.dtype == torch.float32 and w.shape == (2, 36, 12, 2) and np.array_equal(_bits(w), _bits(want["edge_w"]))
    alive = ((want["edge_mask"][..., None] >> np.arange(12)) & 1).astype(bool)
    w = w.cpu().numpy()
    assert (w[alive] > 0).all() and not w[~alive].any() and (~alive).any() and (w[alive] == F(1.0) / F(0.1)).any(), "clipped ends lie on the near plane"


# ---- drawing ----
def test_overlay_without_its_groups_equals_draw_boxes(device):
    """37 x 53 is no multiple of the tile; 360 edges are more than one batch."""
    from nerfdet_amd import pipeline as P
    frames, (edges, mask) = O.case_frames(), D.hand_edge_table(2, 37, 53, n=30)
    col = O.case_colours(30)
    fd, proj = _dev(frames, device), dict(edges=_dev(edges, device), edge_mask=_dev(mask, device))
    before = fd.clone()
    for t in (1, 3, 5):
        want = P.draw_boxes(fd, proj, col, t)
        got = P.draw_overlay(fd, proj, col, t)
        assert got.dtype == torch.uint8 and got.data_ptr() != fd.data_ptr() and torch.equal(got, want), t
        assert torch.equal(P.draw_overlay(fd, proj, col, t, occluded="dim", depth_bias=1.0, text_scale=3), want), "options without their groups"
        assert torch.equal(fd, before) and not torch.equal(got, fd)


@pytest.mark.parametrize("thickness", [1, 5])
@pytest.mark.parametrize("bias_mm", [0.0, 50.0])
def test_depth_test_equals_the_reference(device, thickness, bias_mm):
    """Depth frames built from the reference's own e_mm: pixels one millimetre on either side of the threshold, holes, 65535, a random
    field; hide and dim."""
    from nerfdet_amd import pipeline as P
    ref = O.projected_ref()
    frames, col = O.case_frames(), O.case_colours(36)
    depth, _ = O.depth_case(thickness, bias_mm)
    fd, dd, proj = _dev(frames, device), _dev(depth, device), _projected(device)
    plain = P.draw_boxes(fd, proj, col, thickness)
    for mode, name in ((0, "hide"), (1, "dim")):
        want = O.overlay_ref(frames, ref["edges"], ref["edge_mask"], col, thickness, depth, ref["edge_w"], bias_mm, mode)
        got = P.draw_overlay(fd, proj, col, thickness, depth_frames=dd, occluded=name, depth_bias=bias_mm / 1000.0)
        assert float(np.float32(bias_mm / 1000.0 * 1000.0)) == bias_mm
        diff = got.cpu().numpy() != want
        assert not diff.any(), (name, int(diff.sum()), np.argwhere(diff)[:5].tolist())
        assert not torch.equal(got, plain)
    # holes everywhere: nothing is in front of anything
    assert torch.equal(P.draw_overlay(fd, proj, col, thickness, depth_frames=torch.zeros_like(dd)), plain)


@pytest.mark.parametrize("scale", [1, 2, 3])
def test_plates_equal_the_reference(device, scale):
    """300 boxes, a plate on every fourth: both LDS batches hold plates; lengths 0, 1, 32, beyond 32 and below 0, codes >= 128."""
    from nerfdet_amd import _lib, pipeline as P
    import ctypes
    edges, mask, rect, codes, lens = O.plate_case()
    frames, col = O.case_frames(), O.case_colours(300)
    want = O.overlay_ref(frames, edges, mask, col, 1, rect=rect, text=codes, text_len=lens, font=P.FONT_5X7, text_scale=scale)
    # the raw buffers go to the entry point as they are: encode_texts would neither make a length of 40 nor a code of 200
    fd, ed, md, cd, rd = (_dev(a, device) for a in (frames, edges, mask, col, rect))
    td, ld, fo = _dev(codes, device), _dev(lens, device), _dev(P.FONT_5X7, device)
    out = torch.empty_like(fd)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(_lib.load().ndet_draw_overlay(ptr(fd), ptr(ed), ptr(md), ptr(cd), None, None, 0.0, 0, ptr(rd), ptr(td), ptr(ld), ptr(fo), scale, 2, 37, 53,
                                             300, 1, ptr(out), ctypes.c_void_p(_lib.raw_stream(fd.device))), "draw_overlay")
    diff = out.cpu().numpy() != want
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:5].tolist())
    # and through the wrapper, with strings: what encode_texts makes of them
    texts = ["", "W", "abcdefghijklmnopqrstuvwxyz0123456789", "café 0.50"] + [f"c{i} 0.{i % 100:02d}"[:i % 9] for i in range(4, 300)]
    codes2, lens2 = P.encode_texts(texts)
    want2 = O.overlay_ref(frames, edges, mask, col, 3, rect=rect, text=codes2, text_len=lens2, font=P.FONT_5X7, text_scale=scale)
    got2 = P.draw_overlay(fd, dict(edges=ed, edge_mask=md, rect=rd), col, 3, texts=texts, text_scale=scale)
    assert np.array_equal(got2.cpu().numpy(), want2)


@pytest.mark.parametrize("mode", ["hide", "dim"])
def test_plates_with_the_depth_test_equal_the_reference(device, mode):
    from nerfdet_amd import pipeline as P
    ref = O.projected_ref()
    frames, col = O.case_frames(), O.case_colours(36)
    depth, _ = O.depth_case(5, 50.0)
    texts = ["chair 0.87", "", "x", "a much longer name than any class has, cut", "täble 1.00", "~"] + [f"box {i}" for i in range(6, 36)]
    codes, lens = P.encode_texts(texts)
    assert lens[:6].tolist() == [10, 0, 1, 32, 10, 1] and codes[4, 1] == 127
    for scale in (1, 2):
        want = O.overlay_ref(frames, ref["edges"], ref["edge_mask"], col, 5, depth, ref["edge_w"], 50.0, P.OCCLUDED[mode], rect=ref["rect"], text=codes,
                             text_len=lens, font=P.FONT_5X7, text_scale=scale)
        got = P.draw_overlay(_dev(frames, device), _projected(device), col, 5, depth_frames=_dev(depth, device), occluded=mode, depth_bias=0.05, texts=texts,
                             text_scale=scale)
        diff = got.cpu().numpy() != want
        assert not diff.any(), (scale, int(diff.sum()), np.argwhere(diff)[:5].tolist())


# ---- streams ----
def _box_result(meta, ext, near, far):
    """One box in front of camera ``ext`` (world-to-camera), wholly between ``near`` and ``far`` metres of camera z, on the optical axis."""
    from nerfdet_amd.boxes import DepthInstance3DBoxes
    c2w = np.linalg.inv(np.asarray(ext, dtype=np.float64))
    size = (far - near) / 2.0                               # a cube of half the gap, its diagonal 0.87 of it: any orientation stays inside
    centre = c2w[:3, 3] + c2w[:3, 2] * (near + far) / 2.0
    box = np.array([[centre[0], centre[1], centre[2] - size / 2, size, size, size, 0.3]], dtype=F)
    return dict(boxes_3d=DepthInstance3DBoxes(torch.from_numpy(box)), scores_3d=torch.tensor([0.9]), labels_3d=torch.tensor([4]))


def test_a_flat_wall_hides_what_is_behind_it(device):
    """No reference here: a wall at 2000 mm.  A box between 3 m and 4 m is not drawn at all (hide) or is exactly the blend (dim); a box
    between 1 m and 1.5 m is drawn as draw_detections draws it today."""
    from nerfdet_amd.pipeline import class_palette
    det, scenes = _scenes(device)
    meta = scenes[0]["meta"]
    scene = det.begin_scene(dict(meta))
    ext = meta["lidar2img"]["extrinsic"][1:2]
    hr, wr = meta["img_shape"][:2]
    frames = _dev(np.random.RandomState(21).randint(0, 256, (1, hr, wr, 3)).astype(np.uint8), device)
    wall = torch.full((1, hr, wr), 2000, dtype=torch.uint16, device=device)
    far, near = _box_result(meta, ext[0], 3.0, 4.0), _box_result(meta, ext[0], 1.0, 1.5)
    for res in (far, near):
        plain = scene.draw_detections(frames, res, extrinsic=ext, thickness=3)
        z = plain["zrange"].cpu().numpy()[0, 0]
        assert (res is far and 3.0 < z[0] < z[1] < 4.0) or (res is near and 1.0 < z[0] < z[1] < 1.5), z
        drawn = (plain["frames"] != frames).any(dim=-1)
        assert int(drawn.sum()) > 50, "the box is in the picture"
        hide = scene.draw_detections(frames, res, extrinsic=ext, thickness=3, depth_frames=wall)
        dim = scene.draw_detections(frames, res, extrinsic=ext, thickness=3, depth_frames=wall, occluded="dim")
        assert list(hide) == list(plain) and torch.equal(hide["rect"], plain["rect"]) and torch.equal(hide["zrange"], plain["zrange"])
        if res is near:
            assert torch.equal(hide["frames"], plain["frames"]) and torch.equal(dim["frames"], plain["frames"])
        else:
            assert torch.equal(hide["frames"], frames) and hide["frames"].data_ptr() != frames.data_ptr()
            blend = ((3 * frames.to(torch.int32) + torch.from_numpy(class_palette(18)[4].astype(np.int32)).to(device) + 2) >> 2).to(torch.uint8)
            assert torch.equal(dim["frames"][drawn], blend[drawn]) and torch.equal(dim["frames"][~drawn], frames[~drawn])
            # a hole in the wall shows the far box through it
            holed = wall.clone()
            holed[:, : hr // 2] = 0
            half = scene.draw_detections(frames, res, extrinsic=ext, thickness=3, depth_frames=holed)["frames"]
            assert torch.equal(half[:, : hr // 2], plain["frames"][:, : hr // 2]) and torch.equal(half[:, hr // 2:], frames[:, hr // 2:])


def test_draw_detections_equals_the_composed_calls(device, monkeypatch):
    from nerfdet_amd import pipeline as P
    from nerfdet_amd.boxes import box_corners, drawing_order
    det, scenes = _scenes(device)
    meta = scenes[0]["meta"]
    scene = det.begin_scene(dict(meta))
    ext = meta["lidar2img"]["extrinsic"][1:3]
    res = _result(meta)
    names = [f"class{i}" for i in range(18)]
    hr, wr = meta["img_shape"][:2]
    hs, ws = meta["ori_shape"][:2]
    rs = np.random.RandomState(12)
    calls = []
    real = P.draw_overlay
    monkeypatch.setattr(P, "draw_overlay", lambda *a, **kw: calls.append(kw) or real(*a, **kw))
    for kw, shape, intrinsic, window in ((dict(), (hr, wr), _k_scaled(meta), (0, 0, hr, wr)),
                                         (dict(capture=True, thickness=3), (hs, ws), np.array(meta["lidar2img"]["intrinsic"], dtype=F), (0, 0, hs, ws))):
        frames = _dev(rs.randint(0, 256, (2,) + tuple(shape) + (3,)).astype(np.uint8), device)
        depth = _dev((rs.randint(500, 4000, (2,) + tuple(shape)) * (rs.rand(2, *shape) > 0.2)).astype(np.uint16), device)
        t = kw.get("thickness", 1)
        # the new keywords at their defaults: today's two launches, today's bytes, no ndet_draw_overlay
        kept = drawing_order(res["scores_3d"], 0.0)
        corners = box_corners(res["boxes_3d"].tensor.numpy()[kept])
        col = P.class_palette(18)[res["labels_3d"].numpy()[kept]]
        old = P.draw_boxes(frames, P.project_boxes(intrinsic, corners, window, 1, extrinsic=np.stack(ext), device=device), col, t)
        plain = scene.draw_detections(frames, res, extrinsic=ext, **kw)
        assert not calls and torch.equal(plain["frames"], old)
        same = scene.draw_detections(frames, res, extrinsic=ext, depth_frames=None, occluded="hide", depth_bias=0.05, text=None, text_scale=1, **kw)
        assert not calls and torch.equal(same["frames"], old)
        # depth frames and names: the composed calls
        got = scene.draw_detections(frames, res, extrinsic=ext, depth_frames=depth, text=names, occluded="dim", depth_bias=0.1, text_scale=2, **kw)
        assert len(calls) == 1
        proj = P.project_boxes(intrinsic, corners, window, 1, extrinsic=np.stack(ext), device=device, depths=True)
        texts = [f"{names[int(lab)]} {float(s):.2f}" for lab, s in zip(res["labels_3d"].numpy()[kept], res["scores_3d"].numpy()[kept])]
        want = real(frames, proj, col, t, depth_frames=depth, occluded="dim", depth_bias=0.1, texts=texts, text_scale=2)
        assert list(got) == ["frames", "rect", "zrange", "kept"] and got["kept"].tolist() == kept.tolist()
        assert torch.equal(got["frames"], want) and torch.equal(got["rect"], proj["rect"]) and torch.equal(got["zrange"], proj["zrange"]), kw
        assert not torch.equal(got["frames"], old) and not torch.equal(got["frames"], frames)
        ref = O.overlay_ref(frames.cpu().numpy(), *(proj[key].cpu().numpy() for key in ("edges", "edge_mask")), col, t, depth.cpu().numpy(),
                            proj["edge_w"].cpu().numpy(), F(100.0), 1, proj["rect"].cpu().numpy(), *P.encode_texts(texts), P.FONT_5X7, 2) if not kw else None
        assert ref is None or np.array_equal(got["frames"].cpu().numpy(), ref)
        # text alone: the old projection entry, no depth test
        label_only = scene.draw_detections(frames, res, extrinsic=ext, text=True, **kw)
        numbers = [f"{int(lab)} {float(s):.2f}" for lab, s in zip(res["labels_3d"].numpy()[kept], res["scores_3d"].numpy()[kept])]
        assert len(calls) == 2 and calls[-1]["depth_frames"] is None and calls[-1]["texts"] == numbers
        assert torch.equal(label_only["frames"], real(frames, P.project_boxes(intrinsic, corners, window, 1, extrinsic=np.stack(ext), device=device), col, t,
                                                      texts=numbers))
        # nothing kept: a copy, no launch
        del calls[:]
        empty = scene.draw_detections(frames, res, extrinsic=ext, depth_frames=depth, text=names, score_thr=2.0, **kw)
        assert not calls and torch.equal(empty["frames"], frames) and empty["frames"].data_ptr() != frames.data_ptr() and empty["rect"].shape == (2, 0, 4)
    with pytest.raises(ValueError):
        scene.draw_detections(frames, res, extrinsic=ext, capture=True, text=names[:3])


def test_a_group_of_one_scene_is_the_stream(device):
    det, scenes = _scenes(device)
    metas = [dict(sc["meta"]) for sc in scenes]
    hr, wr = metas[0]["img_shape"][:2]
    rs = np.random.RandomState(13)
    one, stream = det.begin_scenes([dict(metas[1])]), det.begin_scene(dict(metas[1]))
    ext = metas[1]["lidar2img"]["extrinsic"][2:4]
    res = _result(metas[1], seed=4)
    frames = _dev(rs.randint(0, 256, (2, hr, wr, 3)).astype(np.uint8), device)
    depth = _dev((rs.randint(500, 4000, (2, hr, wr)) * (rs.rand(2, hr, wr) > 0.2)).astype(np.uint16), device)
    kw = dict(depth_frames=depth, occluded="dim", text=True, text_scale=2, thickness=3)
    got = one.draw_detections([frames], [res], extrinsic=[ext], **dict(kw, depth_frames=[depth]))[0]
    want = stream.draw_detections(frames, res, extrinsic=ext, **kw)
    assert all(torch.equal(got[key], want[key]) for key in ("frames", "rect", "zrange", "kept"))
    assert not torch.equal(want["frames"], stream.draw_detections(frames, res, extrinsic=ext, thickness=3)["frames"])
    # two scenes, one of them without a depth frame: each is its stream
    group = det.begin_scenes(metas)
    exts = [metas[2]["lidar2img"]["extrinsic"][0:2], metas[0]["lidar2img"]["extrinsic"][3:4]]
    results = [_result(metas[2], seed=2), _result(metas[0], n=5, seed=3)]
    fr = [frames, frames[:1].clone()]
    outs = group.draw_detections(fr, results, extrinsic=exts, scenes=[2, 0], depth_frames=[depth, None], text=True)
    for i, s in enumerate((2, 0)):
        want = det.begin_scene(dict(metas[s])).draw_detections(fr[i], results[i], extrinsic=exts[i], depth_frames=[depth, None][i], text=True)
        assert all(torch.equal(outs[i][key], want[key]) for key in ("frames", "rect", "zrange", "kept")), s
