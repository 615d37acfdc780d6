"""CPU side of the depth-tested, labelled overlay (k_project_boxes_w and k_draw_overlay of csrc/detections_out_kernels.hip,
pipeline.FONT_5X7 / encode_texts / draw_overlay / project_boxes(depths=True), the new keywords of SceneStream / SceneGroup.draw_detections):
the font table and the text encoding are what they say, the closed form of a plate is the picture a cell-by-cell painter makes, the
reference of tests/overlay_ref.py without its two optional groups is detections_out_ref.draw_boxes_ref, both entry points refuse bad
arguments before any device work, the streams refuse what they must without touching a device -- and the inputs of
tests/test_overlay_gpu.py reach every case of the rule, which is checked here so that it holds wherever the suite runs."""
import ctypes
import math

import numpy as np
import pytest
import torch

import detections_out_ref as D
import overlay_ref as O
from test_detections_out_cpu import _result, _streams

F = np.float32


def test_entry_points_exist():
    from nerfdet_amd import _lib, pipeline, streaming
    import inspect
    lib = _lib.load()
    for name in ("ndet_project_boxes_w", "ndet_draw_overlay"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    for fn in ("draw_overlay", "encode_texts"):
        assert callable(getattr(pipeline, fn))
    assert inspect.signature(pipeline.project_boxes).parameters["depths"].default is False
    for cls in (streaming.SceneStream, streaming.SceneGroup):
        par = inspect.signature(cls.draw_detections).parameters
        assert [par[key].default for key in ("depth_frames", "occluded", "depth_bias", "text", "text_scale")] == [None, "hide", 0.05, None, 1]
    par = inspect.signature(pipeline.draw_overlay).parameters
    assert [par[key].default for key in ("thickness", "depth_frames", "occluded", "depth_bias", "texts", "text_scale")] == [1, None, "hide", 0.05, None, 1]


# ---- the font and the texts ----
def test_font_table():
    from nerfdet_amd.pipeline import FONT_5X7
    assert FONT_5X7.shape == (96, 7) and FONT_5X7.dtype == np.uint8
    assert not (FONT_5X7 & 0xE0).any(), "only the low five bits of a row are used"
    assert not FONT_5X7[0].any(), "space is blank"
    assert (FONT_5X7[95] == 0x1F).all(), "index 95 is the full block"
    glyphs = [tuple(FONT_5X7[code - 32].tolist()) for code in range(33, 127)]
    assert all(any(g) for g in glyphs), "codes 33..126 are not blank"
    assert len(set(glyphs)) == len(glyphs) == 94 and tuple(FONT_5X7[95].tolist()) not in glyphs, "and pairwise distinct"
    # bit 4 is the leftmost pixel, the first row the top one: L is a left column and a bottom row, T a top row and a middle column
    assert FONT_5X7[ord("L") - 32].tolist() == [0x10] * 6 + [0x1F] and FONT_5X7[ord("T") - 32].tolist() == [0x1F] + [0x04] * 6


def test_encode_texts():
    from nerfdet_amd.pipeline import encode_texts
    long = "abcdefghijklmnopqrstuvwxyz0123456789"
    codes, lens = encode_texts(["chair 0.87", "", long, "café 猫\t~", " "])
    assert codes.shape == (5, 32) and codes.dtype == np.uint8 and lens.dtype == np.int32 and lens.tolist() == [10, 0, 32, 8, 1]
    assert bytes(codes[0, :10]) == b"chair 0.87" and not codes[0, 10:].any() and not codes[1].any()
    assert bytes(codes[2]) == long[:32].encode(), "cut at 32 characters"
    assert codes[3, :8].tolist() == [99, 97, 102, 127, 32, 127, 127, 126], "a character outside 32..126 becomes 127"
    assert encode_texts(["\x7f\x1f"])[0][0, :2].tolist() == [127, 127]
    codes, lens = encode_texts([])
    assert codes.shape == (0, 32) and lens.shape == (0,)
    for bad in ("abc", [b"abc"], [1, 2], ["a", None]):
        with pytest.raises(ValueError):
            encode_texts(bad)


# ---- plates ----
def test_the_closed_form_of_a_plate_equals_the_cell_painter():
    """Scales 1-3, lengths 0, 1, 32 (and 5, and the clamped 40 and -2): a plate wider than the frame, one pushed in from the right border,
    one whose box lies less than a plate's height under the top border, a box without a rectangle."""
    from nerfdet_amd.pipeline import FONT_5X7, encode_texts
    h, w = 37, 53
    codes = encode_texts(["W", "Mg{|}~ 0.50 chair/sofa_[x]^`@#$%&", "i1l|!"])[0]
    raw = codes[1].copy()
    raw[2:6] = (200, 127, 3, 31)                            # codes outside the table in the raw buffer: the block
    seen = set()
    for scale in (1, 2, 3):
        for length, row in ((0, codes[0]), (1, codes[0]), (32, codes[1]), (32, raw), (5, codes[2]), (40, codes[1]), (-2, codes[0])):
            for rect in ((20, 30, 25, 33), (w - 3, 20, w - 1, 22), (0, 2, 4, 5), (4, 0, 9, 9), (w - 1, h - 1, w - 1, h - 1), (-1, -1, -1, -1), (7, 10, 7, 10)):
                got = O.plate_closed_form(rect, length, row, FONT_5X7, scale, h, w)
                want = O.plate_brute(rect, length, row, FONT_5X7, scale, h, w)
                assert np.array_equal(got, want), (scale, length, rect)
                o = O.plate_origin(rect, length, scale, w)
                if o is None:
                    assert not got.any() and (rect[0] < 0 or length <= 0)
                    continue
                px0, py0, pw, ph = o
                assert (got > 0).sum() == (min(px0 + pw, w) - px0) * (min(py0 + ph, h) - py0) and (got == 2).any()
                seen.add(("wider", pw > w))
                seen.add(("pushed", px0 < rect[0] and pw <= w))
                seen.add(("top", rect[1] < ph))
                seen.add(("clamped", length > 32))
    assert {("wider", True), ("wider", False), ("pushed", True), ("pushed", False), ("top", True), ("top", False), ("clamped", True)} <= seen
    # one glyph by hand at scale 2: "L" with its left column one cell in, its bottom row in the plate's row 7
    pic = O.plate_closed_form((10, 30, 12, 32), 1, encode_texts(["L"])[0][0], FONT_5X7, 2, h, w)
    assert pic[12:30, 10:24].all() and not pic[:12].any() and not pic[30:].any() and not pic[:, :10].any() and not pic[:, 24:].any()
    ink = np.zeros((18, 14), dtype=bool)
    ink[2:16, 2:4] = True
    ink[14:16, 2:12] = True
    assert np.array_equal(pic[12:30, 10:24] == 2, ink)
    assert O.ink_colour((255, 255, 255)) == 0 and O.ink_colour((0, 0, 0)) == 255 and O.ink_colour((0, 218, 0)) == 0 and O.ink_colour((0, 217, 0)) == 255


# ---- the reference ----
def test_the_ref_without_its_groups_is_the_draw_ref():
    rs = np.random.RandomState(4)
    frames = rs.randint(0, 256, (2, 37, 53, 3)).astype(np.uint8)
    edges, mask = D.hand_edge_table(2, 37, 53)
    col = rs.randint(0, 256, (30, 3)).astype(np.uint8)
    for t in (1, 3, 5):
        got = O.overlay_ref(frames, edges, mask, col, t)
        assert got.dtype == np.uint8 and np.array_equal(got, D.draw_boxes_ref(frames, edges, mask, col, t)), t
    # and a depth frame of holes, or one far behind everything, changes nothing: nothing is hidden
    w = rs.rand(2, 30, 12, 2).astype(F) + F(0.1)
    for depth in (np.zeros((2, 37, 53), dtype=np.uint16), np.full((2, 37, 53), 65535, dtype=np.uint16)):
        assert np.array_equal(O.overlay_ref(frames, edges, mask, col, 3, depth, w, 0.0, 1), D.draw_boxes_ref(frames, edges, mask, col, 3))


def test_the_ref_on_pixels_one_can_check_by_hand():
    """One x-major edge from 1 m to 4 m, drawn from its far end: 1/z is linear, so the middle pixel lies at 1.6 m, not 2.5 m."""
    frames = np.full((1, 5, 9, 3), 100, dtype=np.uint8)
    edges = np.zeros((1, 2, 12, 4), dtype=np.int32)
    edges[0, 0, 0], edges[0, 1, 3] = (8, 2, 0, 2), (4, 0, 4, 4)
    mask = np.array([[1, 8]], dtype=np.int32)
    w = np.zeros((1, 2, 12, 2), dtype=F)
    w[0, 0, 0], w[0, 1, 3] = (0.25, 1.0), (0.5, 0.5)
    col = np.array([[200, 0, 0], [0, 200, 0]], dtype=np.uint8)
    recs = O.edge_records(edges, mask, w, 1, 5, 9)
    assert recs[0]["swapped"] and recs[0]["xs"].tolist() == list(range(9))
    assert np.allclose(recs[0]["e_mm"], [1000.0 / (1 - 0.09375 * i) for i in range(9)], rtol=1e-6, atol=0) and recs[0]["e_mm"][0] == 1000.0
    assert recs[0]["e_mm"][4] == 1600.0 and recs[0]["e_mm"][8] == 4000.0 and (recs[1]["e_mm"] == 2000.0).all() and not recs[1]["swapped"]
    depth = np.full((1, 5, 9), 1800, dtype=np.uint16)          # a wall at 1.8 m: box 0 is hidden from x = 5 on, box 1 (2 m) everywhere
    depth[0, 2, 7], depth[0, 4, 4], depth[0, 2, 4] = 0, 2000, 1599
    hide, info = O.overlay_ref(frames, edges, mask, col, 1, depth, w, 0.0, 0, info=True)
    assert [hide[0, 2, x].tolist() for x in range(9)] == [[200, 0, 0]] * 4 + [[100] * 3] * 3 + [[200, 0, 0]] + [[100] * 3]
    assert hide[0, 4, 4].tolist() == [0, 200, 0] and hide[0, 0, 4].tolist() == [100] * 3 and info["bh"][0, 2, 4] == 1 and info["bv"][0, 2, 4] == -1
    dim = O.overlay_ref(frames, edges, mask, col, 1, depth, w, 0.0, 1)
    assert dim[0, 2, 5].tolist() == [125, 75, 75] and dim[0, 0, 4].tolist() == [75, 125, 75] and dim[0, 2, 4].tolist() == [75, 125, 75]
    biased = O.overlay_ref(frames, edges, mask, col, 1, depth, w, 200.0, 1)       # 0.2 m of bias: the wall no longer hides box 1 at 2 m
    assert np.array_equal(biased[0, [0, 1, 3, 4], 4], np.broadcast_to(col[1], (4, 3))) and biased[0, 2, 4].tolist() == [200, 0, 0]
    depth[0, 2, 4] = 1600                                      # box 0 visible there again: it beats the hidden edge of the higher box 1
    assert O.overlay_ref(frames, edges, mask, col, 1, depth, w, 0.0, 1)[0, 2, 4].tolist() == [200, 0, 0]


# ---- the entry points ----
def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from nerfdet_amd import _lib
    lib = _lib.load()
    f, g, odd, err = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x100000), ctypes.c_void_p(0x1001), lib.ndet_last_error

    def proj(kn=f, e=f, c=f, k=3, n=20, x0=2, y0=3, s=1, h=37, w=53, near=0.1, ed=f, m=f, r=f, z=f, ew=f):
        return lib.ndet_project_boxes_w(kn, e, c, k, n, x0, y0, s, h, w, near, ed, m, r, z, ew, None)
    for null in ("kn", "e", "c", "ed", "m", "r", "z", "ew"):
        assert proj(**{null: None}) == -1 and b"null" in err(), null
    for bad in (dict(k=0), dict(n=0), dict(n=-3), dict(h=0), dict(w=-1), dict(s=0), dict(s=-2), dict(x0=-1), dict(y0=-1), dict(near=0.0),
                dict(near=-0.1), dict(near=float("nan"))):
        assert proj(**bad) == -1, bad
    for name in ("kn", "e", "c", "ed", "m", "r", "z", "ew"):
        assert proj(**{name: odd}) == -2 and b"aligned" in err(), name
    assert proj(ed=ctypes.c_void_p(0x1004)) == -2 and proj(r=ctypes.c_void_p(0x1008)) == -2
    assert proj(ew=ctypes.c_void_p(0x1004)) == -2 and b"edge_w" in err()                                 # edge_w: 8 bytes
    assert proj(k=1 << 13, n=1 << 13) == -2 and b"2^31" in err()

    def draw(fi=f, ed=f, m=f, col=f, d=None, ew=None, bias=0.0, occ=0, r=None, tx=None, tl=None, ft=None, sc=1, k=3, h=37, w=53, n=30, t=1, fo=g):
        return lib.ndet_draw_overlay(fi, ed, m, col, d, ew, bias, occ, r, tx, tl, ft, sc, k, h, w, n, t, fo, None)
    depth, plates = dict(d=f, ew=f), dict(r=f, tx=f, tl=f, ft=f)
    for group in ({}, depth, plates, dict(depth, **plates)):
        for null in ("fi", "ed", "m", "col", "fo"):
            assert draw(**dict(group, **{null: None})) == -1 and b"null" in err(), null
        for bad in (dict(k=0), dict(h=0), dict(w=-5), dict(n=0), dict(t=0), dict(t=2), dict(t=4), dict(t=7), dict(t=-1), dict(occ=2), dict(occ=-1),
                    dict(bias=-1.0), dict(bias=float("nan")), dict(bias=float("inf")), dict(bias=-float("inf"))):
            assert draw(**dict(group, **bad)) == -1, (group, bad)
        assert draw(**dict(group, fo=f)) == -1 and b"overlaps" in err()
        assert draw(**dict(group, fo=ctypes.c_void_p(0x1000 + 37 * 53 * 3))) == -1
        assert draw(**dict(group, k=1, h=1 << 15, w=1 << 15)) == -2 and b"2^31" in err()
        assert draw(**dict(group, k=1 << 13, n=1 << 13, h=1, w=1)) == -2
        assert draw(**dict(group, k=1 << 24, h=1, w=1, n=1, fo=ctypes.c_void_p(1 << 30))) == -2 and b"2^24" in err()     # a tile a frame
        assert draw(**dict(group, ed=ctypes.c_void_p(0x1004))) == -2 and b"aligned" in err() and draw(**dict(group, m=odd)) == -2
    # an incomplete group
    for part in (dict(d=f), dict(ew=f), dict(r=f), dict(tx=f), dict(tl=f), dict(ft=f), dict(r=f, tx=f, tl=f), dict(r=f, tx=f, ft=f), dict(r=f, tl=f, ft=f),
                 dict(tx=f, tl=f, ft=f), dict(depth, r=f), dict(plates, d=f)):
        assert draw(**part) == -1 and b"together" in err(), part
    # the text scale counts with plates only
    for sc in (0, 4, -1):
        assert draw(**dict(plates, sc=sc)) == -1 and b"text_scale" in err()
        assert draw(**dict(depth, sc=sc, fo=f)) == -1 and b"overlaps" in err(), "without plates the scale is not looked at: the next refusal"
    # alignment of the optional pointers
    assert draw(**dict(depth, ew=ctypes.c_void_p(0x1004))) == -2 and b"aligned" in err() and draw(**dict(depth, ew=odd)) == -2
    assert draw(**dict(depth, d=odd)) == -2 and draw(**dict(plates, r=ctypes.c_void_p(0x1008))) == -2 and draw(**dict(plates, tl=ctypes.c_void_p(0x1002))) == -2
    with pytest.raises(AssertionError):
        _lib.check(draw(occ=3), "x")
    with pytest.raises(ValueError):
        _lib.check(draw(**dict(depth, d=odd)), "x")


def test_pipeline_wrappers_refuse_wrong_shapes_and_cpu_tensors():
    from nerfdet_amd import pipeline as P
    frames = torch.zeros((2, 4, 5, 3), dtype=torch.uint8)
    proj = dict(edges=torch.zeros((2, 4, 12, 4), dtype=torch.int32), edge_mask=torch.zeros((2, 4), dtype=torch.int32), window=(0, 0, 4, 5), stride=1,
                rect=torch.zeros((2, 4, 4), dtype=torch.int32), edge_w=torch.zeros((2, 4, 12, 2)))
    col = P.class_palette(4)
    depth = torch.zeros((2, 4, 5), dtype=torch.uint16)
    texts = ["a", "", "chair 0.50", "x" * 40]
    no_w = {key: v for key, v in proj.items() if key != "edge_w"}
    no_rect = {key: v for key, v in proj.items() if key != "rect"}
    for args, kw in (((frames.float(), proj, col), {}), ((frames[:1], proj, col), {}), ((frames, {}, col), {}), ((frames, proj, col[:3]), {}),
                     ((frames, proj, col, 2), {}), ((frames, proj, col, True), {}), ((frames, dict(proj, window=(0, 0, 5, 4)), col), {}),
                     ((frames, proj, col), dict(depth_frames=depth[:1])), ((frames, proj, col), dict(depth_frames=depth.to(torch.int16))),
                     ((frames, proj, col), dict(depth_frames=depth.numpy())), ((frames, proj, col), dict(depth_frames=depth[:, :, :4])),
                     ((frames, no_w, col), dict(depth_frames=depth)), ((frames, dict(proj, edge_w=proj["edge_w"].double()), col), dict(depth_frames=depth)),
                     ((frames, dict(proj, edge_w=proj["edge_w"][:, :3]), col), dict(depth_frames=depth)),
                     ((frames, proj, col), dict(occluded="blend")), ((frames, proj, col), dict(occluded=1)), ((frames, proj, col), dict(depth_bias=-0.1)),
                     ((frames, proj, col), dict(depth_bias=float("nan"))), ((frames, proj, col), dict(depth_bias=float("inf"))),
                     ((frames, proj, col), dict(depth_bias="5cm")), ((frames, proj, col), dict(depth_bias=1e40)), ((frames, proj, col), dict(text_scale=0)),
                     ((frames, proj, col), dict(text_scale=4)), ((frames, proj, col), dict(text_scale=True)), ((frames, proj, col), dict(text_scale=1.5)),
                     ((frames, proj, col), dict(texts=texts[:3])), ((frames, proj, col), dict(texts="abcd")), ((frames, proj, col), dict(texts=[1, 2, 3, 4])),
                     ((frames, no_rect, col), dict(texts=texts)), ((frames, dict(proj, rect=proj["rect"].long()), col), dict(texts=texts))):
        with pytest.raises(ValueError):
            P.draw_overlay(*args, **kw)
    for kw in (dict(), dict(depth_frames=depth), dict(texts=texts), dict(depth_frames=depth, occluded="dim", depth_bias=0, texts=texts, text_scale=3)):
        with pytest.raises(RuntimeError, match="GPU"):
            P.draw_overlay(frames, proj, col, 3, **kw)
    with pytest.raises(ValueError):
        P.project_boxes(np.eye(3, dtype=F), np.zeros((2, 8, 3), dtype=F), (0, 0, 4, 5), c2w=np.eye(4)[None], depths=1)
    opts = P.check_overlay_options("dim", 0.05, 2, "x")
    assert opts[0] == 1 and opts[1] == F(50.0) and opts[1].dtype == F and opts[2] == 2 and P.check_overlay_options("hide", 0, 1, "x")[:2] == (0, F(0))


# ---- streams and groups on the CPU ----
def test_streams_refuse_bad_arguments_before_any_launch():
    s, g = _streams()
    ext = s.meta["lidar2img"]["extrinsic"]
    c2w = [np.linalg.inv(e) for e in ext[:2]]
    res = _result()
    frames = torch.zeros((2, 64, 96, 3), dtype=torch.uint8)
    depth = torch.zeros((2, 64, 96), dtype=torch.uint16)
    cap = torch.zeros((2, 128, 192, 3), dtype=torch.uint8)
    cap_depth = torch.zeros((2, 128, 192), dtype=torch.uint16)
    names = [f"class{i}" for i in range(18)]
    assert int(res["labels_3d"].max()) >= 5
    for fr, kw in ((frames, dict(depth_frames=depth[:1])), (frames, dict(depth_frames=depth.to(torch.int32))), (frames, dict(depth_frames=depth.numpy())),
                   (frames, dict(depth_frames=cap_depth)), (cap, dict(capture=True, depth_frames=depth)), (frames, dict(depth_frames=depth[:, :, :90])),
                   (frames, dict(depth_frames=depth, occluded="ghost")), (frames, dict(occluded=None)), (frames, dict(depth_frames=depth, depth_bias=-1)),
                   (frames, dict(depth_frames=depth, depth_bias=float("nan"))), (frames, dict(depth_bias="x")), (frames, dict(text=True, text_scale=4)),
                   (frames, dict(text_scale=0)), (frames, dict(text=False)), (frames, dict(text="chair")), (frames, dict(text=names[:5])),
                   (frames, dict(text=[1, 2, 3])), (frames, dict(text=np.arange(18))), (frames, dict(text=True, thickness=2)),
                   (frames[:1], dict(text=True, depth_frames=depth))):
        with pytest.raises(ValueError):
            s.draw_detections(fr, res, c2w=c2w, **kw)
        gkw = {k: ([v, v] if k == "depth_frames" else v) for k, v in kw.items()}
        with pytest.raises(ValueError):
            g.draw_detections([fr, fr], [res, res], c2w=[c2w, c2w], **gkw)
    # the group's list of depth frames
    for d in (depth, [depth], [depth, depth, depth], [depth, None, depth]):
        with pytest.raises(ValueError):
            g.draw_detections([frames, frames], [res, res], c2w=[c2w, c2w], depth_frames=d)
    with pytest.raises(ValueError):                            # the second scene's names are checked before the first one draws
        g.draw_detections([frames, frames], [res, dict(res, labels_3d=res["labels_3d"] + 20)], c2w=[c2w, c2w], text=names)
    # what is left once the arguments are good: CPU tensors, no fallback and no launch
    for kw in (dict(depth_frames=depth), dict(text=True), dict(text=names, text_scale=3, depth_frames=depth, occluded="dim", depth_bias=0.0)):
        with pytest.raises(RuntimeError, match="GPU"):
            s.draw_detections(frames, res, c2w=c2w, **kw)
        gkw = {k: ([v, v] if k == "depth_frames" else v) for k, v in kw.items()}
        with pytest.raises(RuntimeError, match="GPU"):
            g.draw_detections([frames, frames], [res, res], c2w=[c2w, c2w], **gkw)
    with pytest.raises(RuntimeError, match="GPU"):
        s.draw_detections(cap, res, extrinsic=ext[:2], capture=True, depth_frames=cap_depth, text=True)
    with pytest.raises(RuntimeError, match="GPU"):
        g.draw_detections([frames, frames], [res, res], c2w=[c2w, c2w], depth_frames=[depth, None])     # one scene without a depth frame
    s, g = _streams(training=True)
    with pytest.raises(RuntimeError, match="eval"):
        s.draw_detections(frames, res, c2w=c2w, depth_frames=depth, text=True)
    with pytest.raises(RuntimeError, match="eval"):
        g.draw_detections([frames, frames], [res, res], c2w=[c2w, c2w], text=True)


def test_the_texts_of_a_result():
    from nerfdet_amd.streaming import _kept_detections, _plan_overlay
    res = _result(6)
    res["scores_3d"] = torch.tensor([0.5, 0.899, 0.1, 0.5, 0.304, 1.0])
    res["labels_3d"] = torch.tensor([3, 0, 17, 2, 1, 3])
    frames = torch.zeros((1, 4, 4, 3), dtype=torch.uint8)
    plan = dict(frames=frames, kept=_kept_detections(res, 0.3, None, "x")[0])
    assert plan["kept"].tolist() == [4, 0, 3, 1, 5]
    _plan_overlay(plan, res, None, "hide", 0.05, True, 1, "x")
    assert plan["overlay"]["texts"] == ["1 0.30", "3 0.50", "2 0.50", "0 0.90", "3 1.00"] and plan["overlay"]["depth_frames"] is None
    _plan_overlay(plan, res, None, "dim", 0.0, ["bed", "chair", "sofa", "table"], 2, "x")
    assert plan["overlay"]["texts"] == ["chair 0.30", "table 0.50", "sofa 0.50", "bed 0.90", "table 1.00"]
    assert plan["overlay"]["occluded"] == "dim" and plan["overlay"]["text_scale"] == 2
    _plan_overlay(plan, res, None, "hide", 0.05, None, 1, "x")
    assert plan["overlay"] is None, "both absent: the old path"
    with pytest.raises(ValueError):                            # label 17 is kept now
        _plan_overlay(dict(frames=frames, kept=_kept_detections(res, 0.0, None, "x")[0]), res, None, "hide", 0.05, ["a", "b", "c", "d"], 1, "x")


# ---- the inputs of the GPU tests reach every case ----
def _edge_cases(info, depth, bias, edge_w):
    """Counts of the pixels of one reference run by case."""
    bv, bh, recs = info["bv"], info["bh"], info["records"]
    covered = np.zeros(depth.shape, dtype=bool)
    just_visible = just_hidden = point = swapped = clipped = 0
    for r in recs:
        covered[r["frame"], r["ys"], r["xs"]] = True
        mm = depth[r["frame"], r["ys"], r["xs"]].astype(np.int64)
        e = r["e_mm"].astype(np.float64)
        hid = O.hidden_of(r, depth, bias)
        for m, v, hd in zip(mm, e, hid):
            if math.isfinite(v) and m != 0:
                turn = math.ceil(v - bias)                   # exact: a float32, an integer-valued bias, in float64
                just_visible += m == turn and not hd
                just_hidden += m == turn - 1 and hd
                assert hd == (m < turn), "the threshold lies where the depth frames were built to straddle it"
        point += len(r["xs"]) * r["point"]
        swapped += len(r["xs"]) * r["swapped"]
        clipped += len(r["xs"]) * bool((edge_w[r["frame"], r["box"], r["edge"]] == F(1.0) / F(0.1)).any())
    return dict(visible=int((bv >= 0).sum()), hidden=int(((bv < 0) & (bh >= 0)).sum()), higher_hidden_under_visible=int(((bv >= 0) & (bh > bv)).sum()),
                hole_under_edge=int((covered & (depth == 0)).sum()), saturated_under_edge=int((covered & (depth == 65535)).sum()),
                just_visible=int(just_visible), just_hidden=int(just_hidden), point=int(point), swapped=int(swapped), near_clipped=int(clipped))


def test_the_gpu_fixtures_are_exercised():
    """What tests/test_overlay_gpu.py hands to the kernels, run through the reference: every case of the rule holds at least one pixel."""
    from nerfdet_amd.pipeline import FONT_5X7
    proj = O.projected_ref()
    frames, col = O.case_frames(), O.case_colours(36)
    assert (proj["edge_mask"][0, 30:] != 0xFFF).any() and proj["edge_mask"][0, 31] == 0 and proj["edge_mask"][0, 33] == 0xFFF
    for t in (1, 5):
        for bias in (0.0, 50.0):
            depth, _ = O.depth_case(t, bias)
            outs = {}
            for mode in (0, 1):
                outs[mode], info = O.overlay_ref(frames, proj["edges"], proj["edge_mask"], col, t, depth, proj["edge_w"], bias, mode, info=True)
                counts = _edge_cases(info, depth, bias, proj["edge_w"])
                assert all(v > 0 for v in counts.values()), (t, bias, mode, counts)
            hidden = (info["bv"] < 0) & (info["bh"] >= 0)
            assert np.array_equal(outs[0][hidden], frames[hidden]), "hide: a hidden pixel keeps its bytes"
            assert (outs[1][hidden] != frames[hidden]).any() and np.array_equal(outs[1][~hidden], outs[0][~hidden]), "dim: it is blended"
            plain = D.draw_boxes_ref(frames, proj["edges"], proj["edge_mask"], col, t)
            assert (outs[0] != plain).any() and (outs[1] != plain).any(), "the depth test changes the picture"
    # plates alone: 300 boxes, both batches hold plates
    edges, mask, rect, codes, lens = O.plate_case()
    assert rect.shape == (2, 300, 4) and (rect[:, 257:, 0] >= 0).any() and (rect[:, :256, 0] >= 0).any() and codes.max() >= 128
    assert {0, 1, 32} <= set(lens.tolist()) and lens.max() > 32 and lens.min() < 0
    col300 = O.case_colours(300)
    for scale in (1, 2, 3):
        out, info = O.overlay_ref(frames, edges, mask, col300, 1, rect=rect, text=codes, text_len=lens, font=FONT_5X7, text_scale=scale, info=True)
        _plate_cases(info, rect, lens, scale)
        assert (info["plate"] >= 257).any() and ((info["plate"] < 0) & (info["bv"] >= 0)).any(), "plates of the second batch; edges beside the plates"
        pens = {O.ink_colour(col300[b]) for b in np.unique(info["plate"][info["ink"]])}
        assert pens == {0, 255}, "both inks"
    # plates together with the depth test
    codes36, lens36 = O.case_texts(36)
    depth, _ = O.depth_case(1, 50.0)
    out, info = O.overlay_ref(frames, proj["edges"], proj["edge_mask"], col, 1, depth, proj["edge_w"], 50.0, 1, rect=proj["rect"], text=codes36,
                              text_len=lens36, font=FONT_5X7, text_scale=1, info=True)
    _plate_cases(info, proj["rect"], lens36, 1)
    free = info["plate"] < 0
    assert (free & (info["bv"] >= 0)).any() and (free & (info["bv"] < 0) & (info["bh"] >= 0)).any()


def _plate_cases(info, rect, lens, scale):
    plate, ink = info["plate"], info["ink"]
    h, w = plate.shape[1:]
    assert ink.sum() > 0 and ((plate >= 0) & ~ink).sum() > 0, "plate ink and plate background"
    assert ((plate >= 0) & ((info["bv"] >= 0) | (info["bh"] >= 0))).sum() > 0, "a plate over an edge"
    assert (info["n_plates"] > 1).sum() > 0, "two overlapping plates"
    clipped = 0
    for f in range(rect.shape[0]):
        for b in range(rect.shape[1]):
            o = O.plate_origin(rect[f, b], lens[b], scale, w)
            clipped += o is not None and (o[0] + o[2] > w or o[1] + o[3] > h)
    assert clipped > 0, "a clipped plate"
