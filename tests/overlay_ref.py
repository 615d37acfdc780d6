"""numpy / Python references of the overlay kernels (k_project_boxes_w, k_draw_overlay of csrc/detections_out_kernels.hip) and the inputs
of their tests, on top of tests/detections_out_ref.py (imported, not edited): the reciprocal depths of the projected edges, the per-pixel
rule of ndet_draw_overlay painted naively -- every box in ascending order, every edge, every pixel it covers -- the plates by their closed
form and, against that, a painter that loops over glyph cells.  Float steps are float32 numpy operations and ``detections_out_ref.fmaf_v``;
everything else is integers.  include/nerfdet_hip.h holds the definitions."""
import math

import numpy as np

import detections_out_ref as D
import frames_out_ref as R
from detections_out_ref import EDGES, F, fmaf_v

GRID = (37, 53)
WINDOW = (3, 5) + GRID


# ---- the projection's reciprocal depths -----------------------------------------------------------------------------------------------
def edge_w_ref(krows, w2c, corners, window, stride=1, near=0.1):
    """``(k, n, 12, 2)`` float32: for an edge ``project_boxes_ref`` keeps, ``1.0f / z`` of its two ends in corner order after the near
    clip (a clipped end has z = near); zeros for a dropped edge."""
    mask = D.project_boxes_ref(krows, w2c, corners, window, stride, near)["edge_mask"]
    q = D.camera_points_ref(w2c, corners)
    near = F(near)
    k, n = mask.shape
    out = np.zeros((k, n, 12, 2), dtype=F)
    for p in range(k):
        for b in range(n):
            for e, (ia, ib) in enumerate(EDGES):
                if (int(mask[p, b]) >> e) & 1:
                    za, zb = q[p, b, ia, 2], q[p, b, ib, 2]
                    out[p, b, e] = (F(1.0) / (za if za >= near else near), F(1.0) / (zb if zb >= near else near))
    return out


# ---- an edge's pixels with their depths -------------------------------------------------------------------------------------------------
def edge_records(edges, edge_mask, edge_w, thickness, h, w):
    """One record per surviving edge that covers a pixel of the h x w frame: ``dict(frame, box, edge, xs, ys, e_mm, swapped, point)``, the
    covered pixels by the integer line rule (``detections_out_ref.edge_pixels``) and at each of them the edge's depth in millimetres:
    with the ends ordered along the major axis (their w with them), ``s = (float)(P - p0) / (float)a``, ``w_p = fmaf(s, w_1 - w_0, w_0)``
    (``a = 0``: ``w_0``), ``e_mm = (1.0f / w_p) * 1000.0f``.  ``edge_w=None``: ``e_mm`` is None."""
    r = (thickness - 1) // 2
    out = []
    for f in range(edges.shape[0]):
        for b in range(edges.shape[1]):
            for e in range(12):
                if not (int(edge_mask[f, b]) >> e) & 1:
                    continue
                xa, ya, xb, yb = (int(v) for v in edges[f, b, e])
                px = sorted(D.edge_pixels(xa, ya, xb, yb, r, 0, w - 1, 0, h - 1))
                if not px:
                    continue
                xs, ys = np.array([p[0] for p in px]), np.array([p[1] for p in px])
                y_major = abs(xb - xa) < abs(yb - ya)
                p0, p1 = (ya, yb) if y_major else (xa, xb)
                swapped = p0 > p1
                e_mm = None
                if edge_w is not None:
                    w0, w1 = (F(v) for v in edge_w[f, b, e])
                    if swapped:
                        p0, p1, w0, w1 = p1, p0, w1, w0
                    if p1 == p0:
                        wp = np.full(len(px), w0, dtype=F)
                    else:
                        s = ((ys if y_major else xs) - p0).astype(F) / F(p1 - p0)
                        wp = fmaf_v(s, np.full(len(px), w1 - w0, dtype=F), np.full(len(px), w0, dtype=F))
                    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
                        e_mm = (F(1.0) / wp) * F(1000.0)
                    assert e_mm.dtype == F
                out.append(dict(frame=f, box=b, edge=e, xs=xs, ys=ys, e_mm=e_mm, swapped=swapped, point=(xa, ya) == (xb, yb)))
    return out


def hidden_of(rec, depth_mm, bias_mm):
    """Which of a record's pixels are hidden: ``mm != 0 && (float)mm + bias_mm < e_mm``."""
    mm = depth_mm[rec["frame"], rec["ys"], rec["xs"]]
    with np.errstate(invalid="ignore"):
        return (mm != 0) & (mm.astype(F) + F(bias_mm) < rec["e_mm"])


# ---- plates -----------------------------------------------------------------------------------------------------------------------------
def plate_origin(rect, length, scale, w):
    """``(px0, py0, pw, ph)`` of a plate, or None when the box has none: ``rect = (xmin, ymin, xmax, ymax)``, ``length`` as given."""
    ln = min(max(int(length), 0), 32)
    if int(rect[0]) < 0 or ln == 0:
        return None
    pw, ph = scale * (6 * ln + 1), scale * 9
    return min(int(rect[0]), max(w - pw, 0)), max(int(rect[1]) - ph, 0), pw, ph


def glyph_of(code):
    return int(code) - 32 if 32 <= int(code) <= 127 else 95


def plate_ink(x, y, px0, py0, scale, length, codes, font):
    """The closed form: is pixel (x, y) of a plate at (px0, py0) ink."""
    ln = min(max(int(length), 0), 32)
    u, v = (x - px0) // scale, (y - py0) // scale
    c, r = u - 1, v - 1
    if c < 0 or r < 0 or r > 6:
        return False
    g = c // 6
    gc = c - 6 * g
    return gc < 5 and g < ln and bool((int(font[glyph_of(codes[g])][r]) >> (4 - gc)) & 1)


def plate_closed_form(rect, length, codes, font, scale, h, w):
    """``(h, w)`` int8 by the per-pixel rule: 0 outside the plate, 1 background, 2 ink."""
    out = np.zeros((h, w), dtype=np.int8)
    o = plate_origin(rect, length, scale, w)
    if o is None:
        return out
    px0, py0, pw, ph = o
    for y in range(max(py0, 0), min(py0 + ph, h)):
        for x in range(max(px0, 0), min(px0 + pw, w)):
            out[y, x] = 2 if plate_ink(x, y, px0, py0, scale, length, codes, font) else 1
    return out


def plate_brute(rect, length, codes, font, scale, h, w):
    """The same picture from the glyph cells: the background as ``6 len + 1`` by 9 cells of scale x scale pixels, then every set bit of
    every glyph's seven rows as one cell, one column in from the left and one row down; clipped to the frame at the very end."""
    ln = min(max(int(length), 0), 32)
    if int(rect[0]) < 0 or ln == 0:
        return np.zeros((h, w), dtype=np.int8)
    cells = np.ones((9, 6 * ln + 1), dtype=np.int8)
    for g in range(ln):
        code = int(codes[g])
        rows = font[code - 32] if 32 <= code <= 127 else font[95]
        for r in range(7):
            for col in range(5):
                if (int(rows[r]) >> (4 - col)) & 1:
                    cells[1 + r, 1 + 6 * g + col] = 2
    big = np.kron(cells, np.ones((scale, scale), dtype=np.int8))
    ph, pw = big.shape
    px0 = int(rect[0]) if int(rect[0]) + pw <= w else max(w - pw, 0)          # pushed in from the right border, never past the left one
    py0 = max(int(rect[1]) - ph, 0)
    out = np.zeros((max(h, py0 + ph), max(w, px0 + pw)), dtype=np.int8)
    out[py0:py0 + ph, px0:px0 + pw] = big
    return out[:h, :w]


def ink_colour(col):
    """Black on a light plate, white on a dark one; ``col`` is BGR."""
    return 0 if (29 * int(col[0]) + 150 * int(col[1]) + 77 * int(col[2]) + 128) >> 8 >= 128 else 255


# ---- the whole rule -----------------------------------------------------------------------------------------------------------------------
def overlay_ref(frames, edges, edge_mask, colours, thickness=1, depth_mm=None, edge_w=None, bias_mm=0.0, occluded=0, rect=None, text=None,
                text_len=None, font=None, text_scale=1, info=False):
    """New frames by ndet_draw_overlay's rule; ``info=True`` adds ``dict(bv, bh, plate (k,h,w) int`` -- the winning boxes, -1 for none --
    ``, ink (k,h,w) bool, n_plates (k,h,w) int`` -- how many plates cover the pixel -- ``, records)``.  ``bv`` and ``bh`` are also taken
    under a plate, where the kernel does not look."""
    frames = np.asarray(frames)
    k, h, w = frames.shape[:3]
    n = edges.shape[1]
    assert (depth_mm is None) == (edge_w is None) and (rect is None) == (text is None) == (text_len is None) == (font is None)
    bv, bh = np.full((k, h, w), -1, dtype=np.int64), np.full((k, h, w), -1, dtype=np.int64)
    records = edge_records(edges, edge_mask, edge_w, thickness, h, w)
    for rec in records:                                     # ascending boxes: the last word is the highest index's
        f, xs, ys = rec["frame"], rec["xs"], rec["ys"]
        hid = hidden_of(rec, depth_mm, bias_mm) if depth_mm is not None else np.zeros(len(xs), dtype=bool)
        bv[f, ys[~hid], xs[~hid]] = rec["box"]
        bh[f, ys[hid], xs[hid]] = rec["box"]
    plate, ink, n_plates = np.full((k, h, w), -1, dtype=np.int64), np.zeros((k, h, w), dtype=bool), np.zeros((k, h, w), dtype=np.int64)
    if rect is not None:
        for f in range(k):
            for b in range(n):
                pic = plate_closed_form(rect[f, b], text_len[b], text[b], font, text_scale, h, w)
                n_plates[f] += pic > 0
                plate[f][pic > 0] = b
                ink[f][pic > 0] = (pic == 2)[pic > 0]
    out = frames.copy()
    col = np.asarray(colours)
    dim = (bv < 0) & (bh >= 0) & (occluded == 1)
    out[dim] = ((3 * frames[dim].astype(np.int64) + col[bh[dim]].astype(np.int64) + 2) >> 2).astype(np.uint8)
    out[bv >= 0] = col[bv[bv >= 0]]
    out[plate >= 0] = col[plate[plate >= 0]]
    pens = np.array([ink_colour(c) for c in col], dtype=np.uint8)
    out[ink] = pens[plate[ink]][:, None]
    return (out, dict(bv=bv, bh=bh, plate=plate, ink=ink, n_plates=n_plates, records=records)) if info else out


# ---- the inputs of the GPU tests (tests/test_overlay_cpu.py checks on the CPU that they reach every case) --------------------------------
_CACHE = {}


def projection_case():
    """``frames_out_ref.cameras(2)``, 30 random boxes in front of camera 0 (15 yawed) and the six constructed ones: ``(krows, w2c, corners)``."""
    if "proj" not in _CACHE:
        from nerfdet_amd.boxes import box_corners
        krows, rot, lpos = R.cameras(2)
        corners = np.concatenate([box_corners(D.random_boxes(30, 15, centre=lpos[0] + 4 * rot[0][:, 2])), D.constructed_corners(rot, lpos)])
        _CACHE["proj"] = (krows, D.w2c_of(rot, lpos), corners)
    return _CACHE["proj"]


def projected_ref(stride=1):
    """``project_boxes_ref``'s dict of :func:`projection_case` on the window (3, 5, 37, 53) with ``edge_w`` added; made once per stride."""
    key = ("projected", stride)
    if key not in _CACHE:
        krows, w2c, corners = projection_case()
        out = D.project_boxes_ref(krows, w2c[:, :3], corners, WINDOW, stride)
        out["edge_w"] = edge_w_ref(krows, w2c[:, :3], corners, WINDOW, stride)
        _CACHE[key] = out
    return _CACHE[key]


def case_frames(k=2, seed=0):
    return np.random.RandomState(500 + seed).randint(0, 256, (k,) + GRID + (3,)).astype(np.uint8)


def case_colours(n, seed=0):
    """(n, 3) uint8 BGR, light and dark ones, so that both inks appear."""
    rs = np.random.RandomState(600 + seed)
    light = (np.arange(n) // 2 % 2 == 0)[:, None]
    return np.where(light, rs.randint(150, 256, (n, 3)), rs.randint(0, 100, (n, 3))).astype(np.uint8)


def depth_case(thickness, bias_mm, seed=0):
    """``(depth_mm (2, 37, 53) uint16, records)`` for :func:`projected_ref`'s edges: a random field of 300 .. 7000 mm -- the range of the
    boxes -- with a fifth holes and some 65535, and, on every third covered pixel in turn, the two values one millimetre apart between
    which an edge there turns from hidden to visible: ``ceil(e_mm - bias)`` (visible) and one less (hidden)."""
    key = ("depth", thickness, float(bias_mm), seed)
    if key not in _CACHE:
        proj = projected_ref()
        h, w = GRID
        records = edge_records(proj["edges"], proj["edge_mask"], proj["edge_w"], thickness, h, w)
        rs = np.random.RandomState(700 + seed + thickness)
        depth = rs.randint(300, 7000, (2, h, w))
        depth[rs.rand(2, h, w) < 0.2] = 0
        depth[rs.rand(2, h, w) < 0.05] = 65535
        turn = 0
        for rec in records:
            for x, y, e in zip(rec["xs"], rec["ys"], rec["e_mm"]):
                turn += 1
                if turn % 3 and np.isfinite(e):
                    edge = math.ceil(float(e) - float(bias_mm)) - (turn % 3 == 2)
                    if 1 <= edge <= 65535:
                        depth[rec["frame"], y, x] = edge
        _CACHE[key] = (depth.astype(np.uint16), records)
    return _CACHE[key]


def case_texts(n, seed=0):
    """``(codes (n, 32) uint8, lens (n,) int32)`` as raw buffers: lengths 0, 1 and 32 among random ones, lengths past 32 and below 0 (the
    kernel clamps them), codes at and above 127 and below 32 (the block glyph)."""
    rs = np.random.RandomState(800 + seed)
    codes = rs.randint(32, 127, (n, 32)).astype(np.uint8)
    lens = rs.randint(0, 9, n).astype(np.int32)
    lens[:6] = (0, 1, 32, 40, -3, 2)
    lens[n - 1] = 3
    codes[1, 0], codes[2, 5], codes[2, 6], codes[5, 1], codes[n - 1, :3] = 200, 127, 7, 255, (65, 128, 66)
    return codes, lens


def plate_case(n=300, seed=0):
    """``(edges, edge_mask, rect (2, n, 4) int32, codes, lens)``: ``hand_edge_table`` for n boxes with tiny rectangles all over the frame
    -- more plates than one batch of 256 -- some boxes without one (rect = -1), some at the borders."""
    key = ("plates", n, seed)
    if key not in _CACHE:
        h, w = GRID
        rs = np.random.RandomState(900 + seed)
        edges, mask = D.hand_edge_table(2, h, w, n=n)
        x, y = rs.randint(0, w, (2, n)), rs.randint(0, h, (2, n))
        rect = np.stack([x, y, np.minimum(x + 2, w - 1), np.minimum(y + 2, h - 1)], axis=-1).astype(np.int32)
        rect[:, np.arange(n) % 4 != 1] = -1                 # a plate on every fourth box, in both batches: the edges stay in sight
        rect[0, 2], rect[0, 3], rect[1, 5] = (w - 1, h - 1, w - 1, h - 1), (0, 0, 1, 1), (w - 2, 3, w - 1, 4)
        rect[1, 0], rect[1, 4], rect[:, n - 1] = (20, 20, 22, 22), (10, 20, 12, 22), (30, 30, 33, 33)     # lengths 0 and -3: no plate; the last box
        codes, lens = case_texts(n, seed)
        _CACHE[key] = (edges, mask, rect, codes, lens)
    return _CACHE[key]
