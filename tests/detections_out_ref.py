"""numpy / Python references of the detections-out kernels (csrc/detections_out_kernels.hip) and the inputs that tell their arithmetic from
its near misses, in the manner of tests/frames_out_ref.py.

``project_boxes_ref`` and ``label_frames_ref`` follow the kernels' float32 statement order (include/nerfdet_hip.h); every fused step is
rounded ONCE from the exact value: :func:`fmaf_v` is ``frames_out_ref.fmaf`` (exact rationals, ``rn32``) over arrays -- the product of two
float32 is exact in float64, the float64 sum's error is recovered exactly (TwoSum), and the one case where rounding twice differs from
rounding once (the float64 sum lies exactly between two float32) is decided by that error's sign; tests/test_detections_out_cpu.py holds
the two against each other.  The line rule (``edge_pixels``, ``draw_boxes_ref``) and the label choice work in Python integers."""
import math
from fractions import Fraction

import numpy as np

from frames_out_ref import F, fmaf, rn32  # noqa: F401  (re-exported: the scalar fmaf the vector one is checked against)

EDGES = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7))
CLAMP = 2 ** 20


def fmaf_v(a, b, c):
    """fmaf on float32 arrays: a * b + c rounded once (NaN and inf pass through as IEEE has them)."""
    a, b, c = (np.asarray(v, dtype=F).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b                                           # exact: 24 + 24 significant bits
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)                       # TwoSum: p + c == s + e exactly
        t = s.astype(F).astype(np.float64)
        r = s - t                                           # exact
        other = t + 2.0 * r
        tie = np.isfinite(s) & (r != 0) & (e != 0) & (other.astype(F).astype(np.float64) == other)
        s = np.where(tie, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(F)


# ---- projection -----------------------------------------------------------------------------------------------------------------------
def camera_points_ref(w2c, corners):
    """(k, n, 8, 3) float32: q_r = fmaf(E[r][2], Z, fmaf(E[r][1], Y, E[r][0] * X)) + E[r][3]."""
    E = np.asarray(w2c, dtype=F)[:, None, None, :3, :]                        # (k,1,1,3,4)
    P = np.asarray(corners, dtype=F)[None, :, :, None, :]                     # (1,n,8,1,3)
    with np.errstate(invalid="ignore", over="ignore"):
        q = fmaf_v(E[..., 2], P[..., 2], fmaf_v(E[..., 1], P[..., 1], E[..., 0] * P[..., 0])) + E[..., 3]
    assert q.dtype == F
    return q


def _pixel(f, centre, c, z, off, stride):
    u = fmaf_v(f, c / z, centre)
    return (u - (F(off) + F(0.5))) / F(stride) + F(0.5)


def _cell(v):
    return int(np.floor(np.minimum(np.maximum(v, F(-CLAMP)), F(CLAMP))))


def project_boxes_ref(krows, w2c, corners, window, stride=1, near=0.1):
    """``dict(edges (k,n,12,4) int32, edge_mask (k,n) int32, rect (k,n,4) int32, zrange (k,n,2) float32)`` by the kernel's steps."""
    k6 = np.asarray(krows, dtype=F).reshape(6)
    y0, x0, h, w = window
    near = F(near)
    q = camera_points_ref(w2c, corners)
    k, n = q.shape[:2]
    edges = np.zeros((k, n, 12, 4), dtype=np.int32)
    mask = np.zeros((k, n), dtype=np.int32)
    rect = np.full((k, n, 4), -1, dtype=np.int32)
    zrange = np.empty((k, n, 2), dtype=F)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for p in range(k):
            for b in range(n):
                z = q[p, b, :, 2]
                lo = hi = z[0]
                for c in range(1, 8):
                    if z[c] < lo or lo != lo:
                        lo = z[c]
                    if z[c] > hi or hi != hi:
                        hi = z[c]
                zrange[p, b] = lo, hi
                xs, ys = [], []
                for e, (ia, ib) in enumerate(EDGES):
                    A, B = q[p, b, ia].copy(), q[p, b, ib].copy()
                    oka, okb = bool(A[2] >= near), bool(B[2] >= near)
                    if not (oka or okb):
                        continue
                    if not okb:
                        t = (near - A[2]) / (B[2] - A[2])
                        B = np.array([fmaf_v(t, B[0] - A[0], A[0]), fmaf_v(t, B[1] - A[1], A[1]), near], dtype=F)
                    elif not oka:
                        t = (near - B[2]) / (A[2] - B[2])
                        A = np.array([fmaf_v(t, A[0] - B[0], B[0]), fmaf_v(t, A[1] - B[1], B[1]), near], dtype=F)
                    px = [_pixel(k6[0], k6[2], A[0], A[2], x0, stride), _pixel(k6[4], k6[5], A[1], A[2], y0, stride),
                          _pixel(k6[0], k6[2], B[0], B[2], x0, stride), _pixel(k6[4], k6[5], B[1], B[2], y0, stride)]
                    assert all(v.dtype == F for v in px)
                    if any(v != v for v in px):
                        continue
                    cells = [_cell(v) for v in px]
                    edges[p, b, e] = cells
                    mask[p, b] |= 1 << e
                    xs += [cells[0], cells[2]]
                    ys += [cells[1], cells[3]]
                if xs:
                    r = (max(min(xs), 0), max(min(ys), 0), min(max(xs), w - 1), min(max(ys), h - 1))
                    if r[0] <= r[2] and r[1] <= r[3]:
                        rect[p, b] = r
    return dict(edges=edges, edge_mask=mask, rect=rect, zrange=zrange)


# ---- the line rule, in Python integers --------------------------------------------------------------------------------------------------
def edge_pixels(xa, ya, xb, yb, r, x_lo, x_hi, y_lo, y_hi):
    """The set of pixels (x, y) of [x_lo, x_hi] x [y_lo, y_hi] an edge covers at radius ``r`` (include/nerfdet_hip.h, ndet_draw_boxes)."""
    xa, ya, xb, yb = int(xa), int(ya), int(xb), int(yb)
    a, b = xb - xa, yb - ya
    out = set()
    if abs(a) >= abs(b):                                    # x-major, and the point a = b = 0
        if a < 0:
            xa, ya, xb, yb, a, b = xb, yb, xa, ya, -a, -b
        for x in range(max(xa, x_lo), min(xb, x_hi) + 1):
            yl = ya if a == 0 else ya + (2 * b * (x - xa) + a) // (2 * a)
            out.update((x, y) for y in range(max(yl - r, y_lo), min(yl + r, y_hi) + 1))
    else:
        if b < 0:
            xa, ya, xb, yb, a, b = xb, yb, xa, ya, -a, -b
        for y in range(max(ya, y_lo), min(yb, y_hi) + 1):
            xl = xa + (2 * a * (y - ya) + b) // (2 * b)
            out.update((x, y) for x in range(max(xl - r, x_lo), min(xl + r, x_hi) + 1))
    return out


def edge_pixels_brute(xa, ya, xb, yb, r, x_lo, x_hi, y_lo, y_hi):
    """The same set from the exact rational line: at every column (x-major) or row (y-major) of the window the line's other coordinate
    rounded half up, every pixel of the window tested."""
    xa, ya, xb, yb = int(xa), int(ya), int(xb), int(yb)
    a, b = xb - xa, yb - ya
    half = Fraction(1, 2)
    out = set()
    for x in range(x_lo, x_hi + 1):
        for y in range(y_lo, y_hi + 1):
            if abs(a) >= abs(b):
                if not min(xa, xb) <= x <= max(xa, xb):
                    continue
                line = Fraction(ya) if a == 0 else ya + Fraction(b * (x - xa), a)
                if abs(y - math.floor(line + half)) <= r:
                    out.add((x, y))
            else:
                if not min(ya, yb) <= y <= max(ya, yb):
                    continue
                line = xa + Fraction(a * (y - ya), b)
                if abs(x - math.floor(line + half)) <= r:
                    out.add((x, y))
    return out


def draw_boxes_ref(frames, edges, edge_mask, colours, thickness=1):
    """New frames: boxes painted in ascending index, so the highest index with a covering edge has the last word."""
    frames = np.asarray(frames)
    out = frames.copy()
    k, h, w = frames.shape[:3]
    r = (thickness - 1) // 2
    for f in range(k):
        for b in range(edges.shape[1]):
            for e in range(12):
                if (int(edge_mask[f, b]) >> e) & 1:
                    for x, y in edge_pixels(*edges[f, b, e].tolist(), r, 0, w - 1, 0, h - 1):
                        out[f, y, x] = colours[b]
    return out


# ---- labels -----------------------------------------------------------------------------------------------------------------------------
def frame_points_ref(depth_mm, krows, rot, lpos, window, stride=1):
    """(k, h, w, 3) float32: p_j = fmaf(z, d_j, lpos_j) with z = (float)mm / 1000.0f and d k_camera_rays' direction, statement for statement."""
    k6 = np.asarray(krows, dtype=F).reshape(6)
    rot, lpos = np.asarray(rot, dtype=F), np.asarray(lpos, dtype=F)
    y0, x0, h, w = window
    xs = ((np.arange(w, dtype=np.int64) * stride + x0).astype(F) + F(0.5) - k6[2]) / k6[0]
    ys = ((np.arange(h, dtype=np.int64) * stride + y0).astype(F) + F(0.5) - k6[5]) / k6[4]
    z = np.asarray(depth_mm).astype(F) / F(1000.0)
    assert xs.dtype == F and z.dtype == F
    n = rot.shape[0]
    pts = np.empty((n, h, w, 3), dtype=F)
    for c in range(n):
        for j in range(3):
            d = fmaf_v(ys[:, None], rot[c, j, 1], (xs * rot[c, j, 0])[None, :]) + rot[c, j, 2]
            pts[c, ..., j] = fmaf_v(z[c], d, lpos[c, j])
    return pts


def label_frames_ref(depth_mm, krows, rot, lpos, box_frames, window, stride=1):
    """(k, h, w) int16: the highest index among the boxes that hold the pixel's point, -1 for none and for 0 millimetres."""
    depth_mm = np.asarray(depth_mm)
    pts = frame_points_ref(depth_mm, krows, rot, lpos, window, stride)
    bf = np.asarray(box_frames, dtype=F)
    best = np.full(depth_mm.shape, -1, dtype=np.int64)
    for i in range(bf.shape[0]):
        cx, cy, cz, hx, hy, hz, cos, sin = bf[i]
        dx, dy, dz = pts[..., 0] - cx, pts[..., 1] - cy, pts[..., 2] - cz
        lx = fmaf_v(dx, cos, -(dy * sin))
        ly = fmaf_v(dx, sin, dy * cos)
        inside = (np.abs(lx) <= hx) & (np.abs(ly) <= hy) & (np.abs(dz) <= hz)
        best = np.where(inside, i, best)                    # ascending: the last hit is the highest index
    return np.where(depth_mm != 0, best, -1).astype(np.int16)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def w2c_of(rot, lpos):
    """(n,4,4) float32 world-to-camera of camera-to-world rotations and centres: inverted in float64, rounded once."""
    from frames_out_ref import c2w_of
    return np.linalg.inv(c2w_of(rot, lpos).astype(np.float64)).astype(F)


def random_boxes(n, n_yawed, seed=0, centre=(0.0, 0.0, 0.0), spread=4.0):
    """(n, 7) float32 boxes around ``centre``, the last ``n_yawed`` with a yaw."""
    rs = np.random.RandomState(200 + seed)
    b = np.zeros((n, 7), dtype=F)
    b[:, :3] = np.asarray(centre, dtype=F) + rs.uniform(-spread, spread, (n, 3))
    b[:, 3:6] = rs.uniform(0.3, 2.0, (n, 3))
    b[n - n_yawed:, 6] = rs.uniform(-np.pi, np.pi, n_yawed)
    return b


def constructed_corners(rot, lpos):
    """(6, 8, 3) float32 corners about camera 0: a box that holds the camera centre, one wholly behind the camera, one straddling the near
    plane, one of zero size in front of it, one 10^4 m away to the side (its pixels reach the clamp), one with a NaN corner."""
    from nerfdet_amd.boxes import box_corners
    c, fwd, side = lpos[0].astype(np.float64), rot[0][:, 2].astype(np.float64), rot[0][:, 0].astype(np.float64)

    def box(at, size):
        return [at[0], at[1], at[2] - size / 2, size, size, size, 0.3]
    rows = np.array([box(c, 1.0), box(c - 3.0 * fwd, 1.0), box(c + 0.3 * fwd, 0.8), box(c + 2.0 * fwd, 0.0), box(c + 1.0 * fwd + 1e4 * side, 2.0),
                     box(c + 2.5 * fwd, 0.7)], dtype=F)
    out = box_corners(rows)
    out[5, 3, 1] = np.nan
    return out


def octant_edges():
    """Edges ``(x_a, y_a, x_b, y_b)`` about (20, 14): all eight octants with both slopes' roundings, the axes, |a| = |b|, a = b = 0."""
    cx, cy = 20, 14
    ends = [(9, 4), (4, 9), (-4, 9), (-9, 4), (-9, -4), (-4, -9), (4, -9), (9, -4),          # the eight octants
            (11, 0), (0, 7), (-11, 0), (0, -7), (6, 6), (-6, 6), (6, -6), (-6, -6),          # the axes and the diagonals
            (7, 2), (2, 7), (-7, 3), (3, -7), (10, 5), (5, 10), (0, 0)]                      # ties at half a pixel; a point
    return [(cx, cy, cx + dx, cy + dy) for dx, dy in ends]


def hand_edge_table(k, h, w, n=30, seed=0):
    """``(edges (k,n,12,4) int32, edge_mask (k,n) int32)``: the octant cases in both endpoint orders, edges wholly outside the frame, edges
    that cross it with both ends outside (one from the clamp's corner), masked-off edges that would paint, two boxes that overlap, and
    short random edges up to ``n`` boxes -- 12 n edges, more than one batch of 256 for n = 30."""
    rs = np.random.RandomState(300 + seed + 7 * k + h * w)
    flat = []
    for e in octant_edges():
        flat += [e, (e[2], e[3], e[0], e[1])]
    flat += [(-50, -9, -3, -2), (w + 2, 3, w + 40, 11), (2, h + 1, 30, h + 9), (3, -20, 25, -1)]             # wholly outside
    flat += [(-30, -11, w + 25, h + 17), (-CLAMP, -CLAMP, CLAMP, CLAMP), (w // 2, -40, w // 2 - 3, h + 40), (-7, h // 2, w + 9, h // 2 + 2),
             (CLAMP, 5, -CLAMP, 9)]                                                                              # crossing, both ends outside
    while len(flat) < 12 * n:                               # short random edges in and about the frame
        x, y = int(rs.randint(-6, w + 6)), int(rs.randint(-6, h + 6))
        flat.append((x, y, x + int(rs.randint(-7, 8)), y + int(rs.randint(-7, 8))))
    one = np.asarray(flat[:12 * n], dtype=np.int32).reshape(n, 12, 4)
    one[n - 1] = one[n - 2]                                 # two boxes on the same edges: the higher index wins them all
    edges = np.stack([np.roll(one, f, axis=0) + np.int32(f) for f in range(k)])
    edges = np.clip(edges, -CLAMP, CLAMP).astype(np.int32)
    mask = np.full((k, n), 0xFFF, dtype=np.int32)
    mask[:, 3] = 0x0A5                                      # masked-off edges must not paint
    mask[:, 5] = 0
    return edges, mask
