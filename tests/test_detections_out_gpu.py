"""GPU checks of the detections-out path: k_project_boxes, k_draw_boxes and k_label_frames (csrc/detections_out_kernels.hip) against the
references of tests/detections_out_ref.py, and SceneStream / SceneGroup.draw_detections and label_detections (nerf-det_amd/streaming.py)
against the hand-composed pipeline calls.

Every comparison is exact -- integers, bytes, float32 bit patterns: the kernels' arithmetic is fixed statement by statement
(include/nerfdet_hip.h), the line rule and the label choice are integer rules, and the stream methods promise the bits of the calls they
are made of."""
import numpy as np
import pytest
import torch

import detections_out_ref as D
import frames_out_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
GRID = (37, 53)
_CACHE = {}


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _k33(krows):
    k = np.eye(3, dtype=F)
    k[:2] = krows
    return k


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.int32) if a.dtype == F else a


def _projection_case():
    """``frames_out_ref.cameras(3)``, 20 random boxes in front of camera 0 (6 yawed) and the six constructed ones; made once."""
    if "proj" not in _CACHE:
        from nerfdet_amd.boxes import box_corners
        krows, rot, lpos = R.cameras(3)
        corners = np.concatenate([box_corners(D.random_boxes(20, 6, centre=lpos[0] + 4 * rot[0][:, 2])), D.constructed_corners(rot, lpos)])
        _CACHE["proj"] = (krows, rot, lpos, D.w2c_of(rot, lpos), corners)
    return _CACHE["proj"]


# ---- projection ----
@pytest.mark.parametrize("window,stride", [((0, 0) + GRID, 1), ((2, 3, 9, 13), 4)])
def test_projection_equals_the_reference(device, window, stride):
    """3 poses x 26 boxes: every output bit for bit, so the dropped edges are exactly the reference's."""
    from nerfdet_amd import pipeline as P
    krows, rot, lpos, w2c, corners = _projection_case()
    want = D.project_boxes_ref(krows, w2c[:, :3], corners, window, stride)
    got = P.project_boxes(_k33(krows), corners, window, stride, extrinsic=w2c, device=device)
    assert got["edges"].shape == (3, 26, 12, 4) and got["edges"].dtype == torch.int32 and got["zrange"].dtype == torch.float32
    for key in ("edge_mask", "edges", "rect", "zrange"):
        assert np.array_equal(_bits(got[key]), _bits(want[key])), key
    m = want["edge_mask"]
    assert (m[:, :20] == 0xFFF).sum() >= 20 and m[0, 21] == 0 and 0 < m[0, 22] < 0xFFF and m[0, 23] == 0xFFF and bin(int(m[0, 25])).count("1") == 9
    assert (want["rect"][0, 21] == -1).all() and (want["rect"][:, :20] >= 0).any()
    if stride == 1:
        assert np.abs(want["edges"][0, 24]).max() == D.CLAMP
    # camera-to-world matrices give the same tables when their float64 inverse rounds to the same float32 matrices; near is a parameter
    far = P.project_boxes(_k33(krows), corners, window, stride, extrinsic=w2c, near=2.0, device=device)
    want_far = D.project_boxes_ref(krows, w2c[:, :3], corners, window, stride, near=2.0)
    assert np.array_equal(_bits(far["edges"]), want_far["edges"]) and np.array_equal(_bits(far["edge_mask"]), want_far["edge_mask"])
    assert not np.array_equal(want_far["edge_mask"], want["edge_mask"])
    again = P.project_boxes(_k33(krows), torch.from_numpy(corners), window, stride, c2w=np.linalg.inv(w2c.astype(np.float64)), device=device)
    assert np.array_equal(_bits(again["edges"]), want["edges"]) and np.array_equal(_bits(again["zrange"]), _bits(want["zrange"]))


@pytest.mark.parametrize("window,stride", [((0, 0) + GRID, 1), ((2, 3, 9, 13), 4)])
def test_a_ray_point_lands_on_its_pixel(device, window, stride):
    """For every pixel of pipeline.camera_rays on the same cameras and window the point ray_o + 2.0 ray_d, given as a zero-size box to its
    own camera, lands on that pixel: all 12 edges survive with both ends there."""
    from nerfdet_amd import pipeline as P
    krows, rot, lpos, _, _ = _projection_case()
    c2w = R.c2w_of(rot, lpos)
    h, w = window[2], window[3]
    ray_o, ray_d = P.camera_rays(_k33(krows), c2w, window, stride, device=device)
    pts = (ray_o + 2.0 * ray_d).cpu().numpy()
    jj, ii = np.meshgrid(np.arange(w), np.arange(h))
    want = np.stack([jj, ii, jj, ii], axis=-1).reshape(h * w, 1, 4).astype(np.int32)
    for c in range(3):
        corners = np.repeat(pts[c][:, None, :], 8, axis=1)
        got = P.project_boxes(_k33(krows), corners, window, stride, c2w=c2w[c:c + 1], device=device)
        assert (got["edge_mask"] == 0xFFF).all()
        assert np.array_equal(got["edges"][0].cpu().numpy(), np.broadcast_to(want, (h * w, 12, 4))), c
        assert np.array_equal(got["rect"][0].cpu().numpy(), want[:, 0, :])
        z = got["zrange"].cpu().numpy()
        assert np.array_equal(z[..., 0], z[..., 1]) and np.abs(z - 2.0).max() < 1e-5


# ---- drawing ----
@pytest.mark.parametrize("k,h,w", [(1, 1, 1), (1, 16, 16), (1, 17, 33), (3, 37, 53)])
def test_drawing_equals_the_reference(device, k, h, w):
    """Random bytes under a hand-made table of 30 boxes (360 edges, two batches): the octants in both orders, edges outside, edges crossing
    with both ends outside, masked-off edges; t = 1, 3, 5.  The input tensor is unchanged."""
    from nerfdet_amd import pipeline as P
    rs = np.random.RandomState(40 + h * w)
    frames = rs.randint(0, 256, (k, h, w, 3)).astype(np.uint8)
    edges, mask = D.hand_edge_table(k, h, w)
    if (h, w) == (1, 1):
        edges[0, 7, 2] = (0, 0, 0, 0)                           # the only pixel, as a point
        edges[0, 9, 4] = (-5, -5, 5, 5)
    col = rs.randint(0, 256, (30, 3)).astype(np.uint8)
    fd, ed, md = _dev(frames, device), _dev(edges, device), _dev(mask, device)
    before = fd.clone()
    for t in (1, 3, 5):
        want = D.draw_boxes_ref(frames, edges, mask, col, t)
        got = P.draw_boxes(fd, dict(edges=ed, edge_mask=md), col, t)
        assert got.dtype == torch.uint8 and got.shape == fd.shape and got.data_ptr() != fd.data_ptr()
        assert np.array_equal(got.cpu().numpy(), want), (t, int((got.cpu().numpy() != want).sum()))
        assert torch.equal(fd, before), "the input frames are only read"
        assert (want != frames).any()
        if h * w > 1 and t == 1:
            assert (want == frames).all(axis=-1).any(), "some pixels keep their input bytes"
    none = P.draw_boxes(fd, dict(edges=ed, edge_mask=torch.zeros_like(md)), _dev(col, device), 5)
    assert torch.equal(none, fd), "no surviving edge: a copy"


def test_the_higher_index_wins_shared_pixels(device):
    from nerfdet_amd import pipeline as P
    frames = np.zeros((1, 20, 40, 3), dtype=np.uint8)
    edges = np.zeros((1, 2, 12, 4), dtype=np.int32)
    edges[0, 0, 0], edges[0, 0, 1] = (2, 10, 37, 10), (3, 2, 30, 18)
    edges[0, 1, 5], edges[0, 1, 11] = (20, 1, 20, 19), (36, 18, 4, 3)
    mask = np.array([[0b11, (1 << 5) | (1 << 11)]], dtype=np.int32)
    col = np.array([[10, 20, 30], [200, 210, 220]], dtype=np.uint8)
    for t in (1, 3):
        for order in ((0, 1), (1, 0)):
            o = list(order)
            got = P.draw_boxes(_dev(frames, device), dict(edges=_dev(edges[:, o], device), edge_mask=_dev(mask[:, o], device)), col[o], t).cpu().numpy()
            assert np.array_equal(got, D.draw_boxes_ref(frames, edges[:, o], mask[:, o], col[o], t))
            top = col[o][1]
            mine = D.edge_pixels(*edges[0, o[1], {0: 0, 1: 5}[o[1]]].tolist(), (t - 1) // 2, 0, 39, 0, 19)
            assert mine and all(got[0, y, x].tolist() == top.tolist() for x, y in mine), "every pixel of the higher box's edge has its colour"
            assert (got[0] == col[o][0]).all(axis=-1).any()


# ---- labels ----
def test_labels_equal_the_reference(device):
    """3 x (37 x 53) depth frames with a third holes; 12 boxes: nested, yawed, far away, and one that exactly touches a constructed point."""
    from nerfdet_amd import pipeline as P
    from nerfdet_amd.boxes import box_frames
    krows, rot, lpos, _, _ = _projection_case()
    window = (0, 0) + GRID
    rs = np.random.RandomState(77)
    depth = (rs.randint(500, 6000, (3,) + GRID) * (rs.rand(3, *GRID) > 1 / 3)).astype(np.uint16)
    depth[1, 20, 30] = 3000
    pts = D.frame_points_ref(depth, krows, rot, lpos, window)
    mid = pts[0][depth[0] > 0].astype(np.float64).mean(0)
    boxes = np.zeros((12, 7), dtype=F)
    boxes[0] = [mid[0], mid[1], mid[2] - 4, 8, 8, 8, 0]                      # a large one ...
    boxes[1] = [mid[0], mid[1], mid[2] - 2, 4, 4, 4, 0.5]                    # ... with nested ones inside, yawed
    boxes[2] = [mid[0], mid[1], mid[2] - 1, 2, 2, 2, -1.1]
    boxes[3] = [mid[0], mid[1], mid[2] - 0.4, 0.8, 0.8, 0.8, 2.0]
    boxes[4:10] = D.random_boxes(6, 4, seed=3, centre=mid, spread=3.0)
    boxes[10] = [100, 100, 100, 1, 1, 1, 0]                                  # holds nothing
    bf = box_frames(boxes)
    # the last box touches the point of pixel (20, 30) of frame 1 exactly: centred half a metre off along x, hx = |dx| to the bit
    p = pts[1, 20, 30]
    cx = F(p[0] - F(0.5))
    bf[11] = [cx, p[1], p[2], abs(F(p[0] - cx)), 0.25, 0.25, 1.0, 0.0]
    want = D.label_frames_ref(depth, krows, rot, lpos, bf, window)
    assert want[1, 20, 30] == 11 and (want[depth == 0] == -1).all() and len(set(want.ravel().tolist())) >= 6 and (want == -1).sum() > (depth == 0).sum()
    shrunk = bf.copy()
    shrunk[11, 3] = np.nextafter(shrunk[11, 3], F(0))
    assert D.label_frames_ref(depth, krows, rot, lpos, shrunk, window)[1, 20, 30] != 11, "one ulp less and the point is outside: <= holds"
    got = P.label_frames(_dev(depth, device), _k33(krows), R.c2w_of(rot, lpos), bf, window)
    assert got.dtype == torch.int16 and got.shape == (3,) + GRID
    assert np.array_equal(got.cpu().numpy(), want), int((got.cpu().numpy() != want).sum())
    got_s = P.label_frames(_dev(depth, device), _k33(krows), R.c2w_of(rot, lpos), shrunk, window).cpu().numpy()
    assert np.array_equal(got_s, D.label_frames_ref(depth, krows, rot, lpos, shrunk, window))
    # a window with a stride, and more boxes than one LDS batch (300: the first 12 repeated, so the highest copy wins)
    win, s = (2, 3, 9, 13), 4
    sub = np.ascontiguousarray(depth[:, :9, :13])
    many = np.tile(bf, (25, 1))
    want_m = D.label_frames_ref(sub, krows, rot, lpos, many, win, s)
    got_m = P.label_frames(_dev(sub, device), _k33(krows), R.c2w_of(rot, lpos), many, win, s)
    assert np.array_equal(got_m.cpu().numpy(), want_m) and want_m.max() >= 288


# ---- streams ----
def _scenes(device):
    from test_group_render_gpu import _det_scenes
    return _det_scenes(device)


def _k_scaled(meta):
    k = np.array(meta["lidar2img"]["intrinsic"], dtype=F)
    k[:2] = k[:2] / (meta["ori_shape"][0] / meta["img_shape"][0])
    return k


def _result(meta, n=9, seed=0):
    """A detection result as detect()[0] returns it, on the host: n boxes about the scene's origin, scores with a tie, labels below 18."""
    from nerfdet_amd.boxes import DepthInstance3DBoxes
    rs = np.random.RandomState(50 + seed)
    boxes = D.random_boxes(n, 3, seed=seed, centre=np.asarray(meta["lidar2img"]["origin"], dtype=F), spread=1.2)
    scores = rs.rand(n).astype(F)
    scores[2] = scores[n - 1]
    return dict(boxes_3d=DepthInstance3DBoxes(torch.from_numpy(boxes)), scores_3d=torch.from_numpy(scores), labels_3d=torch.from_numpy(rs.randint(0, 18, n)))


def _hand_drawn(frames, result, intrinsic, ext, window, stride, score_thr=0.0, thickness=1):
    from nerfdet_amd import pipeline as P
    from nerfdet_amd.boxes import box_corners, drawing_order
    kept = drawing_order(result["scores_3d"], score_thr)
    proj = P.project_boxes(intrinsic, box_corners(result["boxes_3d"].tensor.numpy()[kept]), window, stride, extrinsic=np.stack(ext), device=frames.device)
    col = P.class_palette(18)[result["labels_3d"].numpy()[kept]]
    return P.draw_boxes(frames, proj, col, thickness), proj, kept


def test_draw_detections_equals_the_hand_composed_calls(device):
    det, scenes = _scenes(device)
    meta = scenes[0]["meta"]
    scene = det.begin_scene(dict(meta))                                   # no keep_views, no views: the meta is all it needs
    ext = meta["lidar2img"]["extrinsic"][1:3]
    res = _result(meta)
    hr, wr = meta["img_shape"][:2]
    hs, ws = meta["ori_shape"][:2]
    rs = np.random.RandomState(8)
    for kw, shape, intrinsic, window, stride in ((dict(), (hr, wr), _k_scaled(meta), (0, 0, hr, wr), 1),
                                                 (dict(stride=4), (hr // 4, wr // 4), _k_scaled(meta), (2, 2, hr // 4, wr // 4), 4),
                                                 (dict(capture=True, thickness=3), (hs, ws), np.array(meta["lidar2img"]["intrinsic"], dtype=F), (0, 0, hs, ws), 1)):
        frames = _dev(rs.randint(0, 256, (2,) + tuple(shape) + (3,)).astype(np.uint8), device)
        before = frames.clone()
        got = scene.draw_detections(frames, res, extrinsic=ext, **kw)
        want, proj, kept = _hand_drawn(frames, res, intrinsic, ext, window, stride, thickness=kw.get("thickness", 1))
        assert list(got) == ["frames", "rect", "zrange", "kept"] and got["kept"].tolist() == kept.tolist() and len(kept) == 9
        assert torch.equal(got["frames"], want) and torch.equal(got["rect"], proj["rect"]) and torch.equal(got["zrange"], proj["zrange"]), kw
        assert torch.equal(frames, before) and not torch.equal(got["frames"], frames) and (got["rect"] >= 0).any(), kw
        ref = D.draw_boxes_ref(frames.cpu().numpy(), proj["edges"].cpu().numpy(), proj["edge_mask"].cpu().numpy(),
                               _palette_rows(res, kept), kw.get("thickness", 1))
        assert np.array_equal(got["frames"].cpu().numpy(), ref), kw
        c2w = np.linalg.inv(np.stack(ext).astype(np.float64))
        same = scene.draw_detections(frames, res, c2w=c2w, **kw)
        assert same["rect"].shape == got["rect"].shape
    # score_thr keeps fewer, in drawing order; nothing kept: the frames copied, empty tables
    thr = float(np.sort(res["scores_3d"].numpy())[4])
    got = scene.draw_detections(frames, res, extrinsic=ext, capture=True, score_thr=thr)
    want, proj, kept = _hand_drawn(frames, res, np.array(meta["lidar2img"]["intrinsic"], dtype=F), ext, (0, 0, hs, ws), 1, score_thr=thr)
    assert 0 < len(kept) < 9 and got["kept"].tolist() == kept.tolist() and torch.equal(got["frames"], want) and got["rect"].shape == (2, len(kept), 4)
    scores = res["scores_3d"].numpy()[kept]
    assert (np.diff(scores) >= 0).all() and scores.min() >= thr
    empty = scene.draw_detections(frames, res, extrinsic=ext, capture=True, score_thr=2.0)
    assert torch.equal(empty["frames"], frames) and empty["frames"].data_ptr() != frames.data_ptr()
    assert empty["rect"].shape == (2, 0, 4) and empty["zrange"].shape == (2, 0, 2) and empty["kept"].shape == (0,)
    none = dict(boxes_3d=res["boxes_3d"].tensor[:0], scores_3d=res["scores_3d"][:0], labels_3d=res["labels_3d"][:0])
    assert torch.equal(scene.draw_detections(frames, none, extrinsic=ext, capture=True)["frames"], frames)
    assert scene.n_views == 0


def _palette_rows(res, kept):
    from nerfdet_amd.pipeline import class_palette
    return class_palette(18)[res["labels_3d"].numpy()[kept]]


def test_label_detections_equals_the_hand_composed_call(device):
    from nerfdet_amd import pipeline as P
    from nerfdet_amd.boxes import box_frames, drawing_order
    det, scenes = _scenes(device)
    meta = scenes[1]["meta"]
    scene = det.begin_scene(dict(meta))
    ext = meta["lidar2img"]["extrinsic"][0:2]
    c2w = np.linalg.inv(np.stack(ext).astype(np.float64)).astype(F)
    res = _result(meta, seed=1)
    hr, wr = meta["img_shape"][:2]
    hs, ws = meta["ori_shape"][:2]
    rs = np.random.RandomState(9)
    for kw, shape, intrinsic, window, stride in ((dict(), (hr, wr), _k_scaled(meta), (0, 0, hr, wr), 1),
                                                 (dict(stride=4, score_thr=0.3), (hr // 4, wr // 4), _k_scaled(meta), (2, 2, hr // 4, wr // 4), 4),
                                                 (dict(capture=True), (hs, ws), np.array(meta["lidar2img"]["intrinsic"], dtype=F), (0, 0, hs, ws), 1)):
        depth = _dev((rs.randint(500, 4000, (2,) + tuple(shape)) * (rs.rand(2, *shape) > 0.3)).astype(np.uint16), device)
        got = scene.label_detections(depth, res, extrinsic=ext, **kw)
        kept = drawing_order(res["scores_3d"], kw.get("score_thr", 0.0))
        bf = box_frames(res["boxes_3d"].tensor.numpy()[kept])
        want = P.label_frames(depth, intrinsic, c2w, bf, window, stride)
        assert got.dtype == torch.int16 and torch.equal(got, want), kw
        assert torch.equal(scene.label_detections(depth, res, c2w=c2w, **kw), want)
        assert (got[depth == 0] == -1).all() and (got >= 0).any() and int(got.max()) < len(kept), kw
        if stride == 4:
            ref = D.label_frames_ref(depth.cpu().numpy(), intrinsic[:2, :3], c2w[:, :3, :3], c2w[:, :3, 3], bf, window, stride)
            assert np.array_equal(got.cpu().numpy(), ref)
    empty = scene.label_detections(depth, res, extrinsic=ext, capture=True, score_thr=2.0)
    assert empty.dtype == torch.int16 and empty.shape == depth.shape and (empty == -1).all()


def test_groups_equal_their_streams(device):
    """Scenes 2 and 0 with 2 and 1 poses: the group's lists are the per-scene streams'; a group of one is the stream."""
    det, scenes = _scenes(device)
    metas = [dict(sc["meta"]) for sc in scenes]
    group = det.begin_scenes(metas)
    listed = [2, 0]
    exts = [metas[2]["lidar2img"]["extrinsic"][0:2], metas[0]["lidar2img"]["extrinsic"][3:4]]
    results = [_result(metas[2], seed=2), _result(metas[0], n=5, seed=3)]
    hr, wr = metas[0]["img_shape"][:2]
    hs, ws = metas[0]["ori_shape"][:2]
    rs = np.random.RandomState(10)
    for kw, shape in ((dict(thickness=5), (hr, wr)), (dict(stride=4, score_thr=0.2), (hr // 4, wr // 4)), (dict(capture=True), (hs, ws))):
        frames = [_dev(rs.randint(0, 256, (len(e),) + tuple(shape) + (3,)).astype(np.uint8), device) for e in exts]
        got = group.draw_detections(frames, results, extrinsic=exts, scenes=listed, **kw)
        lkw = {k: v for k, v in kw.items() if k != "thickness"}
        depths = [_dev((rs.randint(500, 4000, (len(e),) + tuple(shape)) * (rs.rand(len(e), *shape) > 0.3)).astype(np.uint16), device) for e in exts]
        labels = group.label_detections(depths, results, extrinsic=exts, scenes=listed, **lkw)
        assert len(got) == len(labels) == 2
        for i, s in enumerate(listed):
            stream = det.begin_scene(dict(metas[s]))
            want = stream.draw_detections(frames[i], results[i], extrinsic=exts[i], **kw)
            assert list(got[i]) == list(want) and got[i]["kept"].tolist() == want["kept"].tolist()
            for key in ("frames", "rect", "zrange"):
                assert torch.equal(got[i][key], want[key]), (kw, s, key)
            assert not torch.equal(got[i]["frames"], frames[i])
            assert torch.equal(labels[i], stream.label_detections(depths[i], results[i], extrinsic=exts[i], **lkw)), (kw, s)
    one = det.begin_scenes([dict(metas[1])])
    stream = det.begin_scene(dict(metas[1]))
    ext = metas[1]["lidar2img"]["extrinsic"][2:4]
    res = _result(metas[1], seed=4)
    frames = _dev(rs.randint(0, 256, (2, hr, wr, 3)).astype(np.uint8), device)
    depth = _dev(rs.randint(0, 4000, (2, hr, wr)).astype(np.uint16), device)
    got, want = one.draw_detections([frames], [res], extrinsic=[ext])[0], stream.draw_detections(frames, res, extrinsic=ext)
    assert all(torch.equal(got[key], want[key]) for key in ("frames", "rect", "zrange", "kept"))
    assert torch.equal(one.label_detections([depth], [res], extrinsic=[ext])[0], stream.label_detections(depth, res, extrinsic=ext))
