"""CPU side of the detections-out path (csrc/detections_out_kernels.hip, nerfdet_amd.boxes.box_corners / box_frames / drawing_order,
pipeline.project_boxes / draw_boxes / label_frames / class_palette, SceneStream / SceneGroup.draw_detections and label_detections): the
entry points exist and refuse bad arguments before any device work, the host-side box geometry is the reference's, the references of
tests/detections_out_ref.py are what they claim to be, and the streams refuse what they must without touching a device."""
import ctypes
import os

import numpy as np
import pytest
import torch

import detections_out_ref as D
import frames_out_ref as R

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_entry_points_exist():
    from nerfdet_amd import _lib, boxes, pipeline, streaming
    lib = _lib.load()
    for name in ("ndet_project_boxes", "ndet_draw_boxes", "ndet_label_frames"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    for fn in ("project_boxes", "draw_boxes", "label_frames", "class_palette"):
        assert callable(getattr(pipeline, fn))
    for fn in ("box_corners", "box_frames", "drawing_order"):
        assert callable(getattr(boxes, fn))
    for cls in (streaming.SceneStream, streaming.SceneGroup):
        assert callable(cls.draw_detections) and callable(cls.label_detections)
    assert lib.ndet_version() >= 100


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from nerfdet_amd import _lib
    lib = _lib.load()
    f, g, odd, err = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x100000), ctypes.c_void_p(0x1001), lib.ndet_last_error

    def proj(kn=f, e=f, c=f, k=3, n=20, x0=2, y0=3, s=1, h=37, w=53, near=0.1, ed=f, m=f, r=f, z=f):
        return lib.ndet_project_boxes(kn, e, c, k, n, x0, y0, s, h, w, near, ed, m, r, z, None)
    for null in ("kn", "e", "c", "ed", "m", "r", "z"):
        assert proj(**{null: None}) == -1 and b"null" in err(), null
    for bad in (dict(k=0), dict(n=0), dict(n=-3), dict(h=0), dict(w=-1), dict(s=0), dict(s=-2), dict(x0=-1), dict(y0=-1), dict(near=0.0),
                dict(near=-0.1), dict(near=float("nan"))):
        assert proj(**bad) == -1, bad
    for name in ("kn", "e", "c", "ed", "m", "r", "z"):
        assert proj(**{name: odd}) == -2 and b"aligned" in err(), name
    assert proj(ed=ctypes.c_void_p(0x1004)) == -2 and proj(r=ctypes.c_void_p(0x1008)) == -2          # edges and rect: 16 bytes
    assert proj(k=1 << 13, n=1 << 13) == -2 and b"2^31" in err()                                       # 48 * 2^26 edge elements

    def draw(fi=f, ed=f, m=f, col=f, k=3, h=37, w=53, n=30, t=1, fo=g):
        return lib.ndet_draw_boxes(fi, ed, m, col, k, h, w, n, t, fo, None)
    for null in ("fi", "ed", "m", "col", "fo"):
        assert draw(**{null: None}) == -1 and b"null" in err(), null
    for bad in (dict(k=0), dict(h=0), dict(w=-5), dict(n=0), dict(t=0), dict(t=2), dict(t=4), dict(t=7), dict(t=-1)):
        assert draw(**bad) == -1, bad
    assert draw(fo=f) == -1 and b"overlaps" in err()                                                    # in place
    assert draw(fo=ctypes.c_void_p(0x1000 + 37 * 53 * 3)) == -1                                         # the second frame of the input
    assert draw(k=1, h=1 << 15, w=1 << 15) == -2 and b"2^31" in err()
    assert draw(k=1 << 13, n=1 << 13, h=1, w=1) == -2
    assert draw(ed=ctypes.c_void_p(0x1004)) == -2 and b"aligned" in err() and draw(m=odd) == -2

    def lab(d=f, kn=f, rot=f, lp=f, bf=f, k=3, h=37, w=53, n=12, x0=0, y0=0, s=1, out=f):
        return lib.ndet_label_frames(d, kn, rot, lp, bf, k, h, w, n, x0, y0, s, out, None)
    for null in ("d", "kn", "rot", "lp", "bf", "out"):
        assert lab(**{null: None}) == -1 and b"null" in err(), null
    for bad in (dict(k=0), dict(h=-1), dict(w=0), dict(n=0), dict(s=0), dict(x0=-1), dict(y0=-4)):
        assert lab(**bad) == -1, bad
    assert lab(n=32768) == -2 and b"int16" in err()
    assert lab(k=1, h=1 << 16, w=1 << 15) == -2 and b"2^31" in err()
    assert lab(x0=(1 << 31) - 10) == -2
    for name in ("d", "kn", "rot", "lp", "bf", "out"):
        assert lab(**{name: odd}) == -2 and b"aligned" in err(), name
    with pytest.raises(AssertionError):
        _lib.check(draw(t=2), "x")
    with pytest.raises(ValueError):
        _lib.check(lab(n=32768), "x")


# ---- host-side box geometry ----
def test_box_corners_equal_the_reference_bit_for_bit():
    """tests/golden/box_corners.npz (make_golden_boxes.py): the reference's DepthInstance3DBoxes.corners on 12 boxes, 6 of them yawed."""
    from nerfdet_amd.boxes import BOX_EDGES, CORNER_OFFSETS, box_corners
    g = np.load(os.path.join(GOLDEN, "box_corners.npz"))
    boxes, want = g["boxes"], g["corners"]
    assert boxes.shape == (12, 7) and (boxes[:6, 6] == 0).all() and (boxes[6:, 6] != 0).all()
    got = box_corners(boxes)
    assert got.dtype == F and got.shape == (12, 8, 3)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.array_equal(box_corners(torch.from_numpy(boxes)).view(np.int32), want.view(np.int32))
    # the reference's own float32 run rounds at every step: within a few float32 ulp of the box's extent
    assert np.abs(got - g["corners_f32"]).max() <= 4 * np.finfo(F).eps * np.abs(boxes[:, :6]).max()
    # the order and the yaw sign, on a box one can check by hand: yaw pi/2 turns +x into -y (x' = x cos + y sin, y' = -x sin + y cos)
    c = box_corners(np.array([[0, 0, 0, 2, 4, 6, 0.0]]))[0]
    assert c.tolist() == [[(ox - 0.5) * 2, (oy - 0.5) * 4, oz * 6] for ox, oy, oz in CORNER_OFFSETS]
    t = box_corners(np.array([[0, 0, 0, 2, 4, 6, np.pi / 2]]))[0]
    assert np.allclose(t[4], [-2, -1, 0], atol=1e-6) and np.allclose(t[0], [-2, 1, 0], atol=1e-6)
    assert BOX_EDGES == D.EDGES and len(set(BOX_EDGES)) == 12
    for a, b in BOX_EDGES:                                       # an edge joins corners that differ in one offset
        assert sum(x != y for x, y in zip(CORNER_OFFSETS[a], CORNER_OFFSETS[b])) == 1
    for bad in (np.zeros((3, 6)), np.zeros(7), np.zeros((2, 7, 1))):
        with pytest.raises(ValueError):
            box_corners(bad)


def test_box_frames_invert_the_corners():
    """Each corner, turned into its box's frame in float64 with box_frames' float32 entries, lands on +-half within 1 ulp of float32 -- the
    ulp of the box's largest corner coordinate (the corners and the frame's entries are each rounded once, half an ulp of their own)."""
    from nerfdet_amd.boxes import CORNER_OFFSETS, box_corners, box_frames
    g = np.load(os.path.join(GOLDEN, "box_corners.npz"))
    boxes = np.concatenate([g["boxes"], D.random_boxes(20, 8)])
    fr, cn = box_frames(boxes), box_corners(boxes).astype(np.float64)
    assert fr.dtype == F and fr.shape == (len(boxes), 8)
    b64 = boxes.astype(np.float64)
    assert np.array_equal(fr[:, 3:6], (b64[:, 3:6] / 2).astype(F)) and np.array_equal(fr[:, 2], (b64[:, 2] + b64[:, 5] / 2).astype(F))
    assert np.array_equal(fr[:, 6], np.cos(b64[:, 6]).astype(F)) and np.array_equal(fr[:, 7], np.sin(b64[:, 6]).astype(F))
    f64 = fr.astype(np.float64)
    sign = np.asarray(CORNER_OFFSETS, dtype=np.float64) * 2 - 1
    for i in range(len(boxes)):
        d = cn[i] - f64[i, :3]
        lx = d[:, 0] * f64[i, 6] - d[:, 1] * f64[i, 7]
        ly = d[:, 0] * f64[i, 7] + d[:, 1] * f64[i, 6]
        local = np.stack([lx, ly, d[:, 2]], axis=1)
        ulp = np.spacing(F(np.abs(cn[i]).max())).astype(np.float64)
        assert np.abs(local - sign * f64[i, 3:6]).max() <= ulp, i
    with pytest.raises(ValueError):
        box_frames(np.zeros((3, 8)))


def test_palette_and_drawing_order_are_pinned():
    from nerfdet_amd.boxes import drawing_order
    from nerfdet_amd.pipeline import PALETTE_BGR, class_palette
    p = class_palette(18)
    assert p.dtype == np.uint8 and p.shape == (18, 3) and len({tuple(r) for r in p.tolist()}) == 18
    assert p[0].tolist() == [75, 25, 230] and p[1].tolist() == [75, 180, 60] and p[17].tolist() == [180, 215, 255]
    assert p.tolist() == [list(c) for c in PALETTE_BGR]
    q = class_palette(40)
    assert np.array_equal(q[:18], p) and np.array_equal(q[18:36], p) and np.array_equal(q[36:], p[:4])
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            class_palette(bad)
    scores = np.array([0.9, 0.2, 0.5, 0.2, 0.9, 0.1, 0.5], dtype=F)
    assert drawing_order(scores).tolist() == [5, 1, 3, 2, 6, 0, 4]                 # ascending, ties in the result's order: the later comes last
    assert drawing_order(torch.from_numpy(scores), 0.2).tolist() == [1, 3, 2, 6, 0, 4]
    assert drawing_order(scores, 0.5).tolist() == [2, 6, 0, 4] and drawing_order(scores, 0.95).tolist() == []
    assert drawing_order(scores).dtype == np.int64 and drawing_order(np.zeros(0, dtype=F)).shape == (0,)
    with pytest.raises(ValueError):
        drawing_order(np.zeros((2, 2)))


# ---- the references ----
def test_vector_fmaf_is_the_rational_one():
    rs = np.random.RandomState(3)
    a, b = rs.randn(3000).astype(F), rs.randn(3000).astype(F)
    c = (rs.randn(3000) * 10.0 ** rs.randint(-6, 3, 3000)).astype(F)
    # ties of the float64 sum: c = a float32 midpoint's neighbourhood, so that a * b + c lies a hair off the middle of two float32
    one = F(1.0)
    eps = np.spacing(one)
    ta = np.array([F(2.0 ** -30), F(-2.0 ** -30), F(2.0 ** -40), F(3.0), F(1.0)], dtype=F)
    tb = np.array([F(2.0 ** -30), F(2.0 ** -30), F(2.0 ** -40), eps / 2, eps / 2], dtype=F)
    tc = np.array([one + eps, one + eps, -one, one, one], dtype=F)
    # exact midpoints plus a far smaller product: a = 2^-12 (1 + 2^-12) squared reaches below float64's last bit of the sum
    ma = np.array([F(2.0 ** -12) * (one + F(2.0 ** -12))] * 2 + [F(2.0 ** -50)] * 2, dtype=F)
    mb = np.array([F(2.0 ** -12) * (one + F(2.0 ** -12)), -F(2.0 ** -12) * (one + F(2.0 ** -12)), F(2.0 ** -50), -F(2.0 ** -50)], dtype=F)
    a, b, c = np.concatenate([a, ta, ma]), np.concatenate([b, tb, mb]), np.concatenate([c, tc, np.full(4, one, dtype=F)])
    got = D.fmaf_v(a, b, c)
    want = np.array([R.fmaf(x, y, z) for x, y, z in zip(a, b, c)], dtype=F)
    assert got.dtype == F and np.array_equal(got.view(np.int32), want.view(np.int32))
    # a case where rounding twice goes wrong: 1 + eps/2 exactly (a tie in float64 after the sum is rounded) plus a little
    x = D.fmaf_v(F(2.0 ** -60), F(1.0), F(1.0))
    assert x == one
    # 1 + eps/2 is a tie that goes to even (1); the least product on top of it must tip it over, which rounding twice would miss
    assert D.fmaf_v(eps / 2, one, one) == one and D.fmaf_v(eps / 2, one + eps, one) == one + eps
    assert D.fmaf_v(F(2.0 ** -60), F(2.0 ** -60), one + eps) == one + eps
    # a * b = 2^-24 - 2^-70: the float64 sum with 1 + eps is exactly the middle of 1 + eps and 1 + 2 eps, the even one is the wrong one
    lo, hi = F(2.0 ** -12) * (one - eps), F(2.0 ** -12) * (one + eps)
    assert np.float64(lo) * np.float64(hi) + np.float64(one + eps) == 1.0 + 1.5 * np.float64(eps)
    assert D.fmaf_v(lo, hi, one + eps) == one + eps == R.fmaf(lo, hi, one + eps)
    assert D.fmaf_v(-lo, hi, -(one + eps)) == -(one + eps) and D.fmaf_v(lo, hi, one) == one
    assert np.isnan(D.fmaf_v(F(np.nan), one, one)) and np.isinf(D.fmaf_v(F(np.inf), one, one))


def test_the_integer_line_rule_equals_the_exact_rational_line():
    """All eight octants, both endpoint orders (the same pixels), the axes, |a| = |b|, a = b = 0, at t = 1, 3, 5; and ends at +-2^20."""
    win = (0, 40, 0, 28)
    for e in D.octant_edges():
        for r in (0, 1, 2):
            fwd, back = D.edge_pixels(*e, r, *win), D.edge_pixels(e[2], e[3], e[0], e[1], r, *win)
            assert fwd == back, (e, r)
            assert fwd == D.edge_pixels_brute(*e, r, *win), (e, r)
            assert (e[0], e[1]) in fwd and (e[2], e[3]) in fwd
    assert D.edge_pixels(20, 14, 20, 14, 2, *win) == {(20, y) for y in range(12, 17)}
    assert D.edge_pixels(20, 14, 26, 20, 0, *win) == {(20 + i, 14 + i) for i in range(7)}                     # |a| = |b|: x-major
    assert D.edge_pixels(20, 14, 22, 15, 0, *win) == {(20, 14), (21, 15), (22, 15)}                           # 14.5 rounds half up
    assert D.edge_pixels(22, 15, 20, 14, 0, *win) == {(20, 14), (21, 15), (22, 15)}
    big = D.CLAMP
    small = (0, 36, 0, 52)
    for e in ((-big, -big, big, big), (big, -big, -big, big), (-big, 7, big, 30), (11, -big, 17, big), (-big, -big + 3, big, big - 5),
              (big, 20, -big, 21)):
        for r in (0, 2):
            got = D.edge_pixels(*e, r, *small)
            assert got == D.edge_pixels(e[2], e[3], e[0], e[1], r, *small) == D.edge_pixels_brute(*e, r, *small), (e, r)
            assert got, e
    # the largest numerator of the rule stays far inside int64
    assert 2 * (2 * big) * (2 * big) + 2 * big < 2 ** 62


def test_draw_ref_paints_the_highest_index_last():
    frames = np.zeros((1, 9, 12, 3), dtype=np.uint8)
    edges = np.zeros((1, 3, 12, 4), dtype=np.int32)
    edges[0, 0, 0], edges[0, 1, 0], edges[0, 2, 1] = (1, 4, 10, 4), (5, 0, 5, 8), (0, 0, 11, 8)
    mask = np.array([[1, 1, 0]], dtype=np.int32)                          # box 2's edge is masked off: it does not paint
    col = np.array([[1, 1, 1], [2, 2, 2], [3, 3, 3]], dtype=np.uint8)
    out = D.draw_boxes_ref(frames, edges, mask, col)
    assert out[0, 4, 5].tolist() == [2, 2, 2] and out[0, 4, 4].tolist() == [1, 1, 1] and out[0, 0, 5].tolist() == [2, 2, 2]
    assert int((out[0, :, :, 0] == 1).sum()) == 9 and int((out[0, :, :, 0] == 2).sum()) == 9 and not (out == 3).any() and not frames.any()
    e, m = D.hand_edge_table(3, 37, 53)
    assert e.shape == (3, 30, 12, 4) and e.dtype == np.int32 and 12 * 30 > 256 and np.abs(e).max() == D.CLAMP and (m[:, 5] == 0).all()


def test_label_ref_on_points_one_can_check_by_hand():
    krows, rot, lpos = R.cameras(1)
    depth = np.array([[[1000, 0], [2000, 500]]], dtype=np.uint16)
    pts = D.frame_points_ref(depth, krows, rot, lpos, (4, 6, 2, 2), 3)
    _, d = R.camera_rays_ref(krows, rot, lpos, (4, 6, 2, 2), 3)
    d = d.reshape(1, 2, 2, 3).astype(np.float64)
    want = lpos[0].astype(np.float64) + depth[..., None] / 1000.0 * d
    assert pts.dtype == F and np.abs(pts - want).max() <= 1e-6
    p = pts[0, 1, 0].astype(np.float64)
    boxes = np.array([[p[0], p[1], p[2] - 0.5, 1, 1, 1, 0.4], [p[0], p[1], p[2] - 0.05, 0.1, 0.1, 0.1, -1.0], [50, 50, 50, 1, 1, 1, 0]], dtype=F)
    from nerfdet_amd.boxes import box_frames
    lab = D.label_frames_ref(depth, krows, rot, lpos, box_frames(boxes), (4, 6, 2, 2), 3)
    assert lab.dtype == np.int16 and lab[0, 1, 0] == 1 and lab[0, 0, 1] == -1 and lab[0, 0, 0] == -1
    assert D.label_frames_ref(depth, krows, rot, lpos, box_frames(boxes[:1]), (4, 6, 2, 2), 3)[0, 1, 0] == 0


def test_projection_ref_agrees_with_float64_geometry():
    """The reference's pixels against a plain float64 pinhole projection of the same corners: the same cell wherever the float64 coordinate
    is further than 1e-3 from a pixel border; what lies behind the camera is dropped, what straddles is clipped onto the near plane."""
    krows, rot, lpos = R.cameras(3)
    w2c = D.w2c_of(rot, lpos)
    from nerfdet_amd.boxes import box_corners
    corners = np.concatenate([box_corners(D.random_boxes(20, 6, centre=lpos[0] + 4 * rot[0][:, 2])), D.constructed_corners(rot, lpos)])
    out = D.project_boxes_ref(krows, w2c[:, :3], corners, (2, 3, 34, 50), 1)
    k64 = krows.astype(np.float64)
    q = np.einsum("kij,nvj->knvi", w2c[:, :3, :3].astype(np.float64), corners.astype(np.float64)) + w2c[:, None, None, :3, 3].astype(np.float64)
    checked = 0
    for p in range(3):
        for b in range(20):
            for e, (ia, ib) in enumerate(D.EDGES):
                za, zb = q[p, b, ia, 2], q[p, b, ib, 2]
                surv = bool((out["edge_mask"][p, b] >> e) & 1)
                if abs(za - 0.1) > 1e-4 and abs(zb - 0.1) > 1e-4:
                    assert surv == (za >= 0.1 or zb >= 0.1), (p, b, e)
                if za >= 0.11 and zb >= 0.11:
                    for end, i in ((0, ia), (2, ib)):
                        u = k64[0, 0] * q[p, b, i, 0] / q[p, b, i, 2] + k64[0, 2]
                        xo = (u - (3 + 0.5)) / 1 + 0.5
                        if abs(xo - round(xo)) > 1e-3 and abs(xo) < 1e5:
                            assert out["edges"][p, b, e, end] == int(np.floor(xo)), (p, b, e)
                            checked += 1
    assert checked > 300
    m = out["edge_mask"][0, 20:]
    assert m[0] == 0xFFF or bin(int(m[0])).count("1") >= 4          # holds the camera centre: edges cross the near plane and survive clipped
    assert m[1] == 0 and (out["rect"][0, 21] == -1).all()            # wholly behind
    assert 0 < bin(int(m[2])).count("1") <= 12                       # straddles
    assert m[3] == 0xFFF and len({tuple(v) for v in out["edges"][0, 23].reshape(-1, 2).tolist()}) == 1      # zero size: one pixel
    assert np.abs(out["edges"][0, 24]).max() == D.CLAMP             # 10^4 m to the side reaches the clamp
    assert m[5] != 0xFFF and bin(int(m[5])).count("1") == 9          # a NaN corner drops its three edges
    assert np.isfinite(out["zrange"]).all() and (out["zrange"][..., 0] <= out["zrange"][..., 1]).all()


# ---- streams and groups on the CPU ----
class _Det:
    training = False
    render_testing = False


def _metas(n):
    from nerfdet_amd.synth import ring_scene_meta
    return [ring_scene_meta(6, (64, 96), origin=(0.1 * i, 0.0, 0.5)) for i in range(n)]


def _streams(training=False):
    """A SceneStream and a SceneGroup of two scenes on a meta-only detector, as tests/test_frames_out_cpu.py builds them: no device touched,
    no views kept -- the detections-out methods need neither."""
    from nerfdet_amd.streaming import SceneGroup, SceneStream
    det = _Det()
    det.training = training
    s = SceneStream.__new__(SceneStream)
    s.det, s.meta, s.device = det, _metas(1)[0], None
    g = SceneGroup.__new__(SceneGroup)
    g.det, g.metas, g.device = det, _metas(2), None
    return s, g


def _result(n=5):
    from nerfdet_amd.boxes import DepthInstance3DBoxes
    rs = np.random.RandomState(9)
    return dict(boxes_3d=DepthInstance3DBoxes(torch.from_numpy(D.random_boxes(n, 2))), scores_3d=torch.from_numpy(rs.rand(n).astype(F)),
                labels_3d=torch.from_numpy(rs.randint(0, 18, n)))


def test_streams_refuse_bad_arguments_before_any_launch():
    s, g = _streams()
    ext = s.meta["lidar2img"]["extrinsic"]
    c2w = [np.linalg.inv(e) for e in ext[:2]]
    res = _result()
    frames = torch.zeros((2, 64, 96, 3), dtype=torch.uint8)
    depth = torch.zeros((2, 64, 96), dtype=torch.uint16)
    cap = torch.zeros((2, 128, 192, 3), dtype=torch.uint8)
    assert tuple(s.meta["ori_shape"][:2]) == (128, 192) and tuple(s.meta["img_shape"][:2]) == (64, 96)
    bad_res = dict(res, scores_3d=res["scores_3d"][:3])
    for fr, kw in ((frames, dict()), (frames, dict(c2w=c2w, extrinsic=ext[:2])), (frames, dict(c2w=c2w, stride=0)), (frames, dict(c2w=c2w, stride=4)),
                   (frames, dict(c2w=c2w, window=(0, 0, 10, 10))), (frames[:1], dict(c2w=c2w)), (frames.float(), dict(c2w=c2w)),
                   (frames[..., :2], dict(c2w=c2w)), (frames.numpy(), dict(c2w=c2w)), (frames, dict(c2w=c2w, thickness=2)),
                   (frames, dict(c2w=c2w, thickness=7)), (frames, dict(c2w=c2w, capture=True)), (cap, dict(c2w=c2w, capture=True, window=(0, 0, 128, 192))),
                   (cap, dict(c2w=c2w, capture=True, stride=2)), (cap, dict(c2w=c2w)), (frames, dict(c2w=c2w, capture=1)),
                   (frames, dict(c2w=c2w, score_thr="high")), (frames, dict(c2w=c2w, palette=np.zeros((18, 4), dtype=np.uint8))),
                   (frames, dict(c2w=c2w, palette=np.zeros((2, 3), dtype=np.uint8))), (frames, dict(c2w=[np.eye(3)] * 2)), (frames, dict(c2w=[]))):
        with pytest.raises(ValueError):
            s.draw_detections(fr, res, **kw)
        gkw = {k: ([v, v] if k in ("c2w", "extrinsic") else v) for k, v in kw.items()}
        with pytest.raises(ValueError):
            g.draw_detections([fr, fr], [res, res], **gkw)
    for r in (bad_res, [res], dict(boxes_3d=res["boxes_3d"]), dict(res, labels_3d=res["scores_3d"])):
        with pytest.raises(ValueError):
            s.draw_detections(frames, r, c2w=c2w)
        with pytest.raises(ValueError):
            s.label_detections(depth, r, c2w=c2w)
        with pytest.raises(ValueError):
            g.draw_detections([frames, frames], [res, r], c2w=[c2w, c2w])
    for d, kw in ((depth, dict()), (depth, dict(c2w=c2w, extrinsic=ext[:2])), (depth.to(torch.int32), dict(c2w=c2w)), (depth[:, :60], dict(c2w=c2w)),
                  (depth, dict(c2w=c2w, capture=True)), (torch.zeros((2, 128, 192), dtype=torch.uint16), dict(c2w=c2w, capture=True, window=(0, 0, 4, 4))),
                  (depth, dict(c2w=c2w, stride=2)), (depth, dict(c2w=c2w[:1]))):
        with pytest.raises(ValueError):
            s.label_detections(d, res, **kw)
        gkw = {k: ([v, v] if k in ("c2w", "extrinsic") else v) for k, v in kw.items()}
        with pytest.raises(ValueError):
            g.label_detections([d, d], [res, res], **gkw)
    # the group's lists
    for args, kw in ((([frames], [res, res]), dict(c2w=[c2w, c2w])), (([frames, frames], [res]), dict(c2w=[c2w, c2w])),
                     (([frames, frames], [res, res]), dict(c2w=[c2w])), (([frames, frames], [res, res]), dict(c2w=[c2w, c2w], scenes=[1])),
                     (([frames, frames], [res, res]), dict(c2w=[c2w, c2w], scenes=[0, 0])), ((frames, res), dict(c2w=[c2w], scenes=[0])),
                     (([frames, frames], [res, res]), dict(c2w=np.stack(c2w)))):
        with pytest.raises(ValueError):
            g.draw_detections(*args, **kw)
    # a CPU tensor is what is left once the arguments are good: no CPU fallback (and no launch: these tensors have no device)
    with pytest.raises(RuntimeError, match="GPU"):
        s.draw_detections(frames, res, c2w=c2w)
    with pytest.raises(RuntimeError, match="GPU"):
        s.draw_detections(cap, res, extrinsic=ext[:2], capture=True, thickness=5, score_thr=0.3)
    with pytest.raises(RuntimeError, match="GPU"):
        s.label_detections(depth, res, extrinsic=ext[:2])
    with pytest.raises(RuntimeError, match="GPU"):
        g.draw_detections([frames, frames[:1]], [res, res], c2w=[c2w, c2w[:1]])
    with pytest.raises(RuntimeError, match="GPU"):
        g.label_detections([depth], [res], extrinsic=[ext[:2]], scenes=[1])
    # a training detector
    s, g = _streams(training=True)
    with pytest.raises(RuntimeError, match="eval"):
        s.draw_detections(frames, res, c2w=c2w)
    with pytest.raises(RuntimeError, match="eval"):
        s.label_detections(depth, res, c2w=c2w)
    with pytest.raises(RuntimeError, match="eval"):
        g.draw_detections([frames, frames], [res, res], c2w=[c2w, c2w])
    with pytest.raises(RuntimeError, match="eval"):
        g.label_detections([depth, depth], [res, res], c2w=[c2w, c2w])


def test_kept_detections_order_and_colours():
    from nerfdet_amd.pipeline import class_palette
    from nerfdet_amd.streaming import _kept_detections
    res = _result(6)
    res["scores_3d"] = torch.tensor([0.5, 0.9, 0.1, 0.5, 0.3, 0.9])
    res["labels_3d"] = torch.tensor([3, 0, 17, 20, 1, 3])
    kept, boxes, col = _kept_detections(res, 0.3, None, "x")
    assert kept.tolist() == [4, 0, 3, 1, 5] and kept.dtype == np.int64
    assert np.array_equal(boxes, res["boxes_3d"].tensor.numpy()[kept]) and boxes.dtype == F
    assert np.array_equal(col, class_palette(21)[[1, 3, 20, 0, 3]]) and col.dtype == np.uint8 and col[2].tolist() == class_palette(3)[2].tolist()
    own = np.arange(63, dtype=np.uint8).reshape(21, 3)
    assert np.array_equal(_kept_detections(res, 0.0, own, "x")[2], own[[17, 1, 3, 20, 0, 3]])
    kept, boxes, col = _kept_detections(res, 0.95, None, "x")
    assert kept.shape == (0,) and boxes.shape == (0, 7) and col.shape == (0, 3)


def test_pipeline_wrappers_refuse_wrong_shapes_and_cpu_tensors():
    from nerfdet_amd import pipeline as P
    from nerfdet_amd.boxes import box_corners, box_frames
    krows, rot, lpos = R.cameras(2)
    k = np.eye(3, dtype=F)
    k[:2] = krows
    c2w = R.c2w_of(rot, lpos)
    boxes = D.random_boxes(4, 2)
    corners, bf = box_corners(boxes), box_frames(boxes)
    good = dict(intrinsic=k, corners=corners, window=(0, 0, 4, 5), stride=1, c2w=c2w)
    for bad in (dict(intrinsic=np.eye(2)), dict(corners=corners[0]), dict(corners=corners[:, :7]), dict(corners=corners[:0]),
                dict(corners=corners.astype(np.int32)), dict(window=(0, 0, 0, 5)), dict(stride=0), dict(c2w=None), dict(extrinsic=c2w),
                dict(c2w=c2w[0]), dict(c2w=np.zeros((2, 3, 4))), dict(near=0.0), dict(near=-1.0), dict(near=float("nan")), dict(near="x")):
        with pytest.raises(ValueError):
            P.project_boxes(**dict(good, **bad))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):
            P.project_boxes(**good)
        with pytest.raises(RuntimeError, match="GPU"):
            P.project_boxes(k, corners, (0, 0, 4, 5), extrinsic=torch.from_numpy(c2w), device="cpu")
    frames = torch.zeros((2, 4, 5, 3), dtype=torch.uint8)
    proj = dict(edges=torch.zeros((2, 4, 12, 4), dtype=torch.int32), edge_mask=torch.zeros((2, 4), dtype=torch.int32), window=(0, 0, 4, 5), stride=1)
    col = P.class_palette(4)
    for args in ((frames.float(), proj, col), (frames[0], proj, col), (frames[..., :2], proj, col), (frames[:1], proj, col),
                 (frames, dict(proj, edges=proj["edges"].long()), col), (frames, dict(proj, edge_mask=proj["edge_mask"][:, :3]), col),
                 (frames, dict(proj, edges=proj["edges"][:, :, :11]), col), (frames, dict(proj, window=(0, 0, 5, 4)), col), (frames, {}, col),
                 (frames, proj, col[:3]), (frames, proj, col.astype(np.int32)), (frames, proj, torch.zeros((4, 3))), (frames, proj, col, 2),
                 (frames, proj, col, 0), (frames, proj, col, True)):
        with pytest.raises(ValueError):
            P.draw_boxes(*args)
    with pytest.raises(RuntimeError, match="GPU"):
        P.draw_boxes(frames, proj, col)
    with pytest.raises(RuntimeError, match="GPU"):
        P.draw_boxes(frames, proj, torch.from_numpy(col), 5)
    depth = torch.zeros((2, 4, 5), dtype=torch.uint16)
    for args in ((depth.to(torch.int16), k, c2w, bf, (0, 0, 4, 5)), (depth[0], k, c2w, bf, (0, 0, 4, 5)), (depth, k, c2w, bf, (0, 0, 5, 4)),
                 (depth, np.eye(2), c2w, bf, (0, 0, 4, 5)), (depth, k, c2w[:1], bf, (0, 0, 4, 5)), (depth, k, c2w, bf[:, :7], (0, 0, 4, 5)),
                 (depth, k, c2w, bf[:0], (0, 0, 4, 5)), (depth, k, c2w, np.zeros((32768, 8), dtype=F), (0, 0, 4, 5)), (depth, k, c2w, bf, (0, 0, 4, 5), 0)):
        with pytest.raises(ValueError):
            P.label_frames(*args)
    with pytest.raises(RuntimeError, match="GPU"):
        P.label_frames(depth, k, c2w, bf, (0, 0, 4, 5))
