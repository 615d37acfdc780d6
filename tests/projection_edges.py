"""Exact scenes for the projecting kernels: every decision a kernel takes about a (point, view) pair is put ON its edge, not near it.

Both projection rules of the project -- nearest pixel (ndet_project_z: round-half-even, 0 <= x < w, d > 0, strict depth band) and bilinear
(ndet_ray_project: denominator clamped at 1e-8, pixel clamped to +-1e6, 0 <= px <= w-1 inclusive, q2 > 0, zero
padded align_corners=True taps) -- are fed cameras whose matrices hold small dyadic numbers only (focal length 16, integer principal
point, axis-aligned rotations, dyadic translations) and points with dyadic coordinates.  u, v, d and the quotients are then exactly
representable: the float32 chain of the kernels and a float64 evaluation agree bit for bit on every decision, so masks and counts can be
held to equality with no sample excused (test_projection_edges_cpu.py proves that from the references alone).

Nothing here needs a GPU.  The geometry is built without a random number generator; only the feature values are drawn (seeded).

Layout of a scene's points: the edge set three times, each copy in another fixed order --
  "first": from index 0, categories dealt round-robin (the first 16 rows, one 16-voxel tile, hold a row of every category),
  "mid":   behind a filler whose length puts the copy at an offset that is 37 modulo 64 (inside a wave, a tile and a sample group),
  "last":  the final rows of the array, whose length is no multiple of 16, 64, 84 or 124 (ragged last tile / wave / block),
with filler points (integer pixels two units in front of an edge camera, seen by two views) in between.
View layout: edge cameras at indices 0, 63, 64 and last (n_v = 5: 0, 1, 3, 4), blind cameras -- camera depth -1 for every point -- elsewhere."""
import functools
import math

import numpy as np
import torch

from oracle import nerfdet_oracle as O
from projection_ref import _k4_ref

F1 = 16.0                          # stride-1 focal length; stride 4: 4.0
CX1, CY1 = 20.0, 16.0              # stride-1 principal point; stride 4: (5, 4)
SIZES = {"even_w": (9, 12), "odd_w": (8, 11)}      # feature map h x w; images are 4 x
BAND, GATE_DEPTH = 0.25, 2.0       # depth gate: voxel_size[2] and the constant depth map
VOXEL_SIZE = (1.0, 1.0, BAND)
X0, Y0 = 3.0, 2.0                  # the in-range stride-4 pixel the other axis of an edge row sits on (stride 1: 12, 8)
NAN, INF = float("nan"), float("inf")

# edge cameras: (name, R (signed permutation), t (dyadic)), camera = R world + t
EDGE_CAMERAS = (
    ("ident", ((1, 0, 0), (0, 1, 0), (0, 0, 1)), (0.0, 0.0, 0.0)),
    ("back", ((-1, 0, 0), (0, 1, 0), (0, 0, -1)), (0.0, 0.0, 0.0)),         # looks the opposite way
    ("turn", ((0, 0, -1), (0, 1, 0), (1, 0, 0)), (0.0, 0.0, 0.0)),          # a quarter turn about y: camera z = world x
    ("shift", ((1, 0, 0), (0, 1, 0), (0, 0, 1)), (0.5, -0.25, 1.0)),
)
UNTRANSLATED = (0, 1, 2)
# a blind camera: third row (0 0 0 -1), so d = q2 = -1 for every finite point (NaN for the others) and q0 = 16 - 20 = -4, far outside
BLIND_E = ((0, 0, 0, 1.0), (0, 0, 0, 1.0), (0, 0, 0, -1.0), (0, 0, 0, 1.0))
PLACEMENTS = ("first", "mid", "last")


def edge_view_indices(n_v):
    return (0, 1, 3, 4) if n_v == 5 else (0, 63, 64, n_v - 1)


def _extrinsic(r, t):
    e = np.eye(4, dtype=np.float32)
    e[:3, :3] = np.asarray(r, dtype=np.float32)
    e[:3, 3] = np.asarray(t, dtype=np.float32)
    return e


@functools.lru_cache(maxsize=None)
def cameras(n_v, size):
    """meta of the n_v cameras for the feature-map size ``size``; returns (meta, P4 (n_v,3,4), P1 (n_v,3,4), rows (1,n_v,34))."""
    h, w = SIZES[size]
    ext = [np.asarray(BLIND_E, dtype=np.float32) for _ in range(n_v)]
    for slot, v in enumerate(edge_view_indices(n_v)):
        ext[v] = _extrinsic(EDGE_CAMERAS[slot][1], EDGE_CAMERAS[slot][2])
    k = np.array([[F1, 0, CX1, 0], [0, F1, CY1, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)
    meta = dict(lidar2img=dict(intrinsic=k, extrinsic=ext, origin=np.zeros(3, dtype=np.float32)), ori_shape=(4 * h, 4 * w, 3),
                img_shape=(4 * h, 4 * w, 3))
    return meta, O.compute_projection(meta, 4), O.compute_projection(meta, 1), O.compute_ray_cameras(meta)


def _world(slot, pc):
    """camera-frame point -> world point of edge camera ``slot``: R^T (pc - t), exact for a signed permutation and dyadic numbers."""
    _, r, t = EDGE_CAMERAS[slot]
    q = [float(a) - float(b) for a, b in zip(pc, t)]
    # column j of R has one nonzero entry: picked out by hand, a matrix product would form 0 * inf
    world = [next(r[i][j] * q[i] for i in range(3) if r[i][j]) for j in range(3)]
    # a coordinate of 2^31 and more absorbs the translation when it becomes a float32 number; every other coordinate is one already
    # (asserted where the scenes are built)
    return tuple(c if abs(c) < 2.0 ** 30 else float(np.float32(c)) for c in world)


def _at(px, py, d, f, cx, cy):
    """camera-frame point that projects to pixel (px, py) at depth d."""
    return ((px - cx) * d / f, (py - cy) * d / f, d)


# ----------------------------------------------------------------------------------------------------------------------------------
# nearest-pixel family
# ----------------------------------------------------------------------------------------------------------------------------------
def nearest_edge_rows(size, slot):
    """[(category, camera-frame point, expected stride-4 validity, expected stride-1 validity, expected gate or None)] of one edge camera.
    The expectations are written down by hand from the rule (round half to even, 0 <= x < w, d > 0), never computed by it; None = not
    pinned.  Gate: the expected outcome of the strict band D - band < z < D + band for a pixel that is valid."""
    h, w = SIZES[size]
    H, W = 4 * h, 4 * w
    rows = []
    at4 = lambda px, py, d: _at(px, py, d, F1 / 4, CX1 / 4, CY1 / 4)
    # (coordinate, valid at stride 4?, valid at stride 1?): stride-1 coordinate = 4 x
    lo = [(-1.0, False, False), (-0.75, False, False), (-0.5, True, False),          # -0.5 -> -0 (valid); -2 at stride 1
          (-0.25, True, False), (-0.125, True, True),                                # stride 1: -0.5 -> -0, the same tie one level down
          (0.0, True, True), (0.5, True, True),                                      # 0.5 -> 0 (tie to even)
          (1.5, True, True), (2.5, True, True)]                                      # 1.5 -> 2, 2.5 -> 2
    for axis, n, big in (("x", w, W), ("y", h, H)):
        hi = [(n - 1.5, True, True),                                                  # tie: n-2 or n-1, both inside; stride 1: 4n-6
              (n - 1.0, True, True), (n - 0.75, True, True),                          # stride 1: 4n-4, 4n-3
              (n - 0.5, n % 2 == 1, True),                                            # tie: up to n (even n, invalid), down to n-1 (odd n); 4n-2
              (n - 0.25, False, True),                                                # -> n; stride 1: 4n-1, the last pixel
              (float(n), False, False)]
        for name, coords in (("lo", lo), ("hi", hi)):
            for c, ok4, ok1 in coords:
                for d in (1.0, 2.0, 0.5):
                    pc = at4(c, Y0, d) if axis == "x" else at4(X0, c, d)
                    rows.append((f"{name}_{axis}", pc, ok4, ok1, d == GATE_DEPTH))
        # stride 4 sees it, stride 1 does not: stride-1 coordinate in [-2, -0.5)
        for s1 in (-2.0, -1.5, -1.0, -0.75):
            pc = at4(s1 / 4, Y0, 1.0) if axis == "x" else at4(X0, s1 / 4, 1.0)
            rows.append((f"s4_only_{axis}", pc, True, False, False))
        # the converse: stride 1 at N - 1.5 (tie to the even N - 2: valid), stride 4 at n - 0.375 -> n
        pc = at4((big - 1.5) / 4, Y0, 1.0) if axis == "x" else at4(X0, (big - 1.5) / 4, 1.0)
        rows.append((f"s1_only_{axis}", pc, False, True, False))
        for val in (2.0 ** 31, 2.0 ** 40, 2.0 ** 64, INF, -INF, NAN):
            pc = (val, -0.5, 1.0) if axis == "x" else (-0.5, val, 1.0)
            rows.append((f"huge_{axis}", pc, False, False, None))
    rows.append(("d_zero", (0.0, 0.0, 0.0), False, False, None))                      # 0 / 0
    rows.append(("d_zero", (0.25, 0.25, 0.0), False, False, None))                    # x / 0 = inf
    rows.append(("d_neg", at4(X0, Y0, -1.0), False, False, None))                     # the quotient is in range, d < 0
    rows.append(("d_neg", at4(X0, Y0, -0.5), False, False, None))
    if slot in UNTRANSLATED:                                                          # (2^-30 - 1) + 1 is not exact under a translation
        rows.append(("d_tiny", at4(X0, Y0, 2.0 ** -30), True, True, False))
    # depth band around the constant 2.0: out, in, in, in, out (both inequalities strict)
    for z, inside in ((1.75, False), (1.75 + 2.0 ** -20, True), (2.0, True), (2.25 - 2.0 ** -20, True), (2.25, False)):
        rows.append(("gate", at4(X0, Y0, z), True, True, inside))
    return rows


def _layout(sets, fillers):
    """sets: per edge camera slot a list of row tuples (first entry: category).  Returns the rows in scene order as (row, slot, placement)
    (placement None: filler)."""
    edge = [(row, slot) for slot, rows in enumerate(sets) for row in rows]
    n = len(edge)
    # first: round-robin over the categories
    by_cat = {}
    for item in edge:
        by_cat.setdefault(item[0][0], []).append(item)
    first, queues = [], [list(v) for v in by_cat.values()]
    while any(queues):
        for q in queues:
            if q:
                first.append(q.pop(0))
    mid = edge[::-1]
    step = next(s for s in range(7, n) if math.gcd(s, n) == 1)
    last = [edge[(i * step + 3) % n] for i in range(n)]
    fill = lambda k, at: [(fillers[(at + i) % len(fillers)], None) for i in range(k)]
    k1 = (37 - n) % 64 or 64
    out = [(r, s, "first") for r, s in first] + [(r, None, None) for r, _ in fill(k1, 0)] + [(r, s, "mid") for r, s in mid]
    k2 = 5
    while any((len(out) + k2 + n) % m == 0 for m in (16, 64, 84, 124)):
        k2 += 1
    out += [(r, None, None) for r, _ in fill(k2, k1)] + [(r, s, "last") for r, s in last]
    assert (n + k1) % 64 == 37 and all(len(out) % m for m in (16, 64, 84, 124))
    return out


def _signed_values(gen, n_v, c, h, w):
    """|value| in [0.25, 2], one random sign per (view, channel): a bilinear blend of one map's pixels never cancels, so a sample no image
    contains has a variance exponent of 0 (no tap) or far above 100 (test_projection_edges_cpu.py asserts it)."""
    mag = 0.25 + 1.75 * torch.rand(n_v, c, h, w, generator=gen)
    sign = torch.where(torch.rand(n_v, c, 1, 1, generator=gen) < 0.5, -1.0, 1.0)
    return mag * sign


class NearestScene:
    """points (3,N,1,1), projections, features (n_v,C,h,w), mapped (n_v,cm,h,w), bias, rgb (n_v,3,H,W), per-point bookkeeping."""


@functools.lru_cache(maxsize=None)
def nearest_scene(n_v, size, c=8, cm=8, reverse=False):
    h, w = SIZES[size]
    meta, p4, p1, _ = cameras(n_v, size)
    sets = [nearest_edge_rows(size, slot) for slot in range(4)]
    at4 = lambda px, py, d: _at(px, py, d, F1 / 4, CX1 / 4, CY1 / 4)
    fillers = [("filler", _world(slot, at4(float(x), float(y), 2.0)), None, None, None) for slot in range(4) for x, y in ((1, 1), (4, 3), (6, 5))]
    sets = [[(cat, _world(slot, pc), ok4, ok1, gate) for cat, pc, ok4, ok1, gate in rows] for slot, rows in enumerate(sets)]
    rows = _layout(sets, fillers)
    if reverse:
        rows = rows[::-1]
    s = NearestScene()
    s.n_v, s.size, s.h, s.w, s.H, s.W, s.c, s.cm = n_v, size, h, w, 4 * h, 4 * w, c, cm
    s.meta, s.proj, s.rgb_proj = meta, p4, p1
    s.points = torch.tensor([r[0][1] for r in rows], dtype=torch.float64).t().contiguous().to(torch.float32).reshape(3, -1, 1, 1)
    assert torch.equal(s.points.double().nan_to_num(0.5, INF, -INF).reshape(3, -1).t(),
                       torch.tensor([r[0][1] for r in rows], dtype=torch.float64).nan_to_num(0.5, INF, -INF)), "a coordinate is not a float32 number"
    s.n = len(rows)
    s.grid = (s.n, 1, 1)
    s.category = [r[0][0] for r in rows]
    s.slot = [r[1] for r in rows]
    s.placement = [r[2] for r in rows]
    s.expect4 = [r[0][2] for r in rows]
    s.expect1 = [r[0][3] for r in rows]
    s.expect_gate = [r[0][4] for r in rows]
    s.edge_views = edge_view_indices(n_v)
    gen = torch.Generator().manual_seed(1000 * n_v + h + (500 if reverse else 0))
    s.feat = _signed_values(gen, n_v, c, h, w)
    s.mapped = _signed_values(gen, n_v, cm, h, w)
    s.bias = _signed_values(torch.Generator().manual_seed(n_v + h), 1, cm, 1, 1).reshape(cm)       # shared by a scene and its reversed twin
    s.rgb = 0.25 + 0.75 * torch.rand(n_v, 3, 4 * h, 4 * w, generator=gen)
    s.depth = {torch.float32: torch.full((n_v, h, w), GATE_DEPTH), torch.float64: torch.full((n_v, h, w), GATE_DEPTH, dtype=torch.float64)}
    s.depth_r = {k: torch.full((n_v, 4 * h, 4 * w), GATE_DEPTH, dtype=k) for k in s.depth}
    return s


def nearest_valid64(points, projection, h, w):
    """The rule of O.backproject evaluated in float64 throughout (points, matrices, quotient): (valid (n_v,N), z (n_v,N))."""
    p = torch.cat([points.reshape(3, -1).double(), torch.ones(1, points[0].numel(), dtype=torch.float64)])
    # k-ordered like the float32 chain, so that 0 * inf and inf - inf come out NaN in the same places
    pj = projection.double()
    uvw = pj[:, :, 0:1] * p[0]
    for k in (1, 2, 3):
        uvw = uvw + pj[:, :, k:k + 1] * p[k]
    x, y, z = (uvw[:, 0] / uvw[:, 2]).round(), (uvw[:, 1] / uvw[:, 2]).round(), uvw[:, 2]
    return (x >= 0) & (y >= 0) & (x < w) & (y < h) & (z > 0), z


# ----------------------------------------------------------------------------------------------------------------------------------
# bilinear family
# ----------------------------------------------------------------------------------------------------------------------------------
IMAGE_KINDS = ("same", "padded", "tiny")     # image tensor: the cameras' h x w; taller and wider (padded); smaller than the feature map


def image_hw(size, kind):
    h, w = SIZES[size]
    return {"same": (4 * h, 4 * w), "padded": (4 * h + 4, 4 * w + 8), "tiny": (5, 7)}[kind]


def bilinear_edge_rows(size, slot):
    """[(category, camera-frame point, expected mask of this camera or None)]: px, py are stride-1 pixels of the cameras' h x w image."""
    h, w = SIZES[size]
    H, W = 4.0 * h, 4.0 * w
    at1 = lambda px, py, q2: _at(px, py, q2, F1, CX1, CY1)
    bx, by = 12.0, 8.0
    rows = []
    for axis, n in (("x", W), ("y", H)):
        coords = [(-1.25, False, "out_near"), (-1.0, False, "out_near"), (-0.5, False, "out_near"), (0.0, True, "border"), (0.25, True, "inside"),
                  (n - 1.25, True, "inside"), (n - 1.0, True, "border"),               # px == w - 1: inside (inclusive)
                  (n - 0.75, False, "out_near"), (n - 0.5, False, "out_near"), (n, False, "out_near"), (n + 0.5, False, "out_near"),
                  (-5.0, False, "out_feat")]                                            # feature taps all outside; a tiny image's may be inside
        for c, ok, kind in coords:
            # -1 and n: the only tap inside an image of the cameras' size has a weight that is float32's rounding residue of the normalised
            # coordinate (1e-6).  Seen by no view such a sample would have a variance exponent of 1e-6: neither 0 nor large.  The rows of
            # "ident" and "turn" are seen by another camera (count >= 1, an ordinary variance); those of "back" and "shift" by none, and
            # these two coordinates are left out there
            if c in (-1.0, n) and EDGE_CAMERAS[slot][0] in ("back", "shift"):
                continue
            rows.append((f"{kind}_{axis}", at1(c, by, 1.0) if axis == "x" else at1(bx, c, 1.0), ok))
    for cx in (0.0, W - 1.0):
        for cy in (0.0, H - 1.0):
            rows.append(("corner", at1(cx, cy, 1.0), True))
    for q2 in (1.0, 2.0, 0.5):
        rows.append(("q2_pos", at1(bx, by, q2), True))
    rows.append(("q2_zero", (0.0, 0.0, 0.0), False))                                  # q0 = q1 = 0: px = py = 0 in range, only q2 > 0 fails
    rows.append(("q2_zero", (0.5 / F1, 0.25 / F1, 0.0), False))
    rows.append(("q2_neg", (CX1 / F1, CY1 / F1, -1.0), False))                        # q0 = q1 = 0 again, q2 = -1
    rows.append(("q2_neg", ((CX1 + 0.5) / F1, (CY1 + 0.5) / F1, -1.0), False))       # q0 = q1 = 0.5: px = 5e7 clamped, out
    if slot in UNTRANSLATED:
        t = 2.0 ** -27                                                                # below the 1e-8 clamp: px = q0 / 1e-8 = 3.7, 1.5
        rows.append(("q2_tiny", ((5.0 - CX1) * t / F1, (2.0 - CY1) * t / F1, t), True))
    for sgn in (1.0, -1.0):                                                           # |px| = 2^21 > 1e6 through q2 = 2^-10
        q2 = 2.0 ** -10
        rows.append(("clamped", ((sgn * 2.0 ** 11 - CX1 * q2) / F1, (by - CY1) * q2 / F1, q2), False))
    for val in (NAN, INF, -INF):
        rows.append(("nonfinite", (val, 0.0, 1.0), None))
        rows.append(("nonfinite", (0.0, 0.0, val), None))
    return rows


class BilinearScene:
    """samples (n,3), camera rows (1,n_v,34), KE (n_v,3,4), features (n_v,d,hf,wf), images (n_v,3,H,W), per-sample bookkeeping."""


@functools.lru_cache(maxsize=None)
def bilinear_scene(n_v, size, d, kind="same", reverse=False):
    from nerfdet_amd import rays
    hf, wf = SIZES[size]
    meta, _, p1, cams = cameras(n_v, size)
    at1 = lambda px, py, q2: _at(px, py, q2, F1, CX1, CY1)
    sets = [[(cat, _world(slot, pc), ok) for cat, pc, ok in bilinear_edge_rows(size, slot)] for slot in range(4)]
    fillers = [("filler", _world(slot, at1(float(x), float(y), 2.0)), None) for slot in range(4) for x, y in ((4, 4), (16, 12), (24, 20))]
    rows = _layout(sets, fillers)
    if reverse:
        rows = rows[::-1]
    s = BilinearScene()
    s.n_v, s.size, s.d, s.kind, s.hf, s.wf = n_v, size, d, kind, hf, wf
    s.h, s.w = 4 * hf, 4 * wf
    s.H, s.W = image_hw(size, kind)
    s.meta, s.cams = meta, cams
    s.ke, ch, cw = rays._camera_matrices(cams.squeeze(0))
    assert (ch, cw) == (s.h, s.w) and torch.equal(s.ke, p1), "the camera rows do not reproduce the dyadic K E"
    s.points = torch.tensor([r[0][1] for r in rows], dtype=torch.float64).to(torch.float32)
    assert torch.equal(s.points.double().nan_to_num(0.5, INF, -INF), torch.tensor([r[0][1] for r in rows], dtype=torch.float64).nan_to_num(0.5, INF, -INF))
    s.n = len(rows)
    s.category = [r[0][0] for r in rows]
    s.slot = [r[1] for r in rows]
    s.placement = [r[2] for r in rows]
    s.expect = [r[0][2] for r in rows]
    s.edge_views = edge_view_indices(n_v)
    gen = torch.Generator().manual_seed(77 * n_v + hf + d + (500 if reverse else 0))
    s.feat = _signed_values(gen, n_v, d, hf, wf)
    s.img = 0.25 + 0.75 * torch.rand(n_v, 3, s.H, s.W, generator=gen)
    return s


def bilinear_mask64(points, ke, h, w):
    """projection.py:42-64 + the mask of projection.py:127-136 in float64 throughout: (n, n_v) bool."""
    p = torch.cat([points.double().t(), torch.ones(1, points.shape[0], dtype=torch.float64)])
    k = ke.double()
    q = k[:, :, 0:1] * p[0]
    for i in (1, 2, 3):
        q = q + k[:, :, i:i + 1] * p[i]
    den = q[:, 2].clamp(min=1e-8)
    px, py = (q[:, 0] / den).clamp(-1e6, 1e6), (q[:, 1] / den).clamp(-1e6, 1e6)
    return ((px <= w - 1.0) & (px >= 0) & (py <= h - 1.0) & (py >= 0) & (q[:, 2] > 0)).t()


@functools.lru_cache(maxsize=None)
def bilinear_reference(n_v, size, d, kind="same", reverse=False):
    """Float64 statistics of a scene through _k4_ref, once for the feature maps and once for the images (the sampler treats an image as a
    3-channel map of its own size).  Returns dict(glob (n, 2 (3 + d)), mask (n, n_v), count (n,), var_feat, var_img (n, c) exponents,
    taps_feat, taps_img)."""
    s = bilinear_scene(n_v, size, d, kind, reverse)
    out = {}
    parts = []
    for name, maps in (("img", s.img), ("feat", s.feat)):
        mean, ev, mask, taps = _k4_ref(s.points, s.ke, (s.h, s.w), maps.double())
        parts.append((mean, ev))
        out["taps_" + name] = taps
        out["var_" + name] = -torch.log(ev)
        out["near_" + name] = sum((wt != 0) for _, wt in taps).t() > 0          # (n, n_v): some tap of the view reaches the map
    out["mask"], out["count"] = mask, mask.sum(1)
    out["glob"] = torch.cat([parts[0][0], parts[1][0], parts[0][1], parts[1][1]], dim=1)
    return out


# the scenes both test modules run on
NEAREST_SCENES = [(5, "even_w"), (5, "odd_w"), (70, "odd_w"), (130, "even_w")]
BILINEAR_SCENES = [(5, "even_w", 8, "same"), (5, "odd_w", 32, "tiny"), (70, "odd_w", 32, "same"), (70, "even_w", 32, "padded"),
                   (130, "even_w", 8, "padded")]


# ----------------------------------------------------------------------------------------------------------------------------------
# the two rules with one slip each: what a kernel with that slip would decide (float32 chain, so bit for bit what it would compute).
# test_projection_edges_cpu.py shows that every slip changes decisions on every scene, i.e. that the equalities the GPU tests assert
# would not hold for such a kernel
# ----------------------------------------------------------------------------------------------------------------------------------
NEAREST_SLIPS = ("roundf", "fx_le_w", "fy_le_h", "band_lo_closed", "band_hi_closed")
BILINEAR_SLIPS = ("px_lt_w1", "py_lt_h1", "q2_ge_0", "xb_from_0", "yb_from_0")


def nearest_rule(points, projection, h, w, slip=None, depth=None):
    """ndet_project_z (+ ndet_depth_band against a constant float32 ``depth``) with ``slip``: (valid (n_v,N), x, y)."""
    fu, fv, z = O.project_voxels(points, projection)
    if slip == "roundf":                                     # half away from zero
        x, y = torch.sign(fu) * torch.floor(fu.abs() + 0.5), torch.sign(fv) * torch.floor(fv.abs() + 0.5)
    else:
        x, y = fu.round(), fv.round()
    in_x = (x <= w) if slip == "fx_le_w" else (x < w)
    in_y = (y <= h) if slip == "fy_le_h" else (y < h)
    valid = (x >= 0) & (y >= 0) & in_x & in_y & ((z >= 0) if slip == "d_ge_0" else (z > 0))
    if depth is not None:
        lo, hi = torch.tensor(depth - BAND, dtype=torch.float32), torch.tensor(depth + BAND, dtype=torch.float32)
        valid = valid & ((z >= lo) if slip == "band_lo_closed" else (z > lo)) & ((z <= hi) if slip == "band_hi_closed" else (z < hi))
    return valid, x, y


def bilinear_rule(points, ke, h, w, hf, wf, slip=None):
    """ndet_ray_project and the tap rule of rs_taps with ``slip``: (mask (n, n_v), tap (n, n_v): some tap of the
    view lies inside the hf x wf map with a nonzero weight)."""
    hom = torch.cat([points.t(), torch.ones(1, points.shape[0])]).numpy()[None]
    q = torch.from_numpy(O.fma_chain_matmul(ke.numpy(), hom))
    den = q[:, 2].clamp(min=1e-8)
    px, py = (q[:, 0] / den).clamp(-1e6, 1e6), (q[:, 1] / den).clamp(-1e6, 1e6)
    in_x = (px < w - 1.0) if slip == "px_lt_w1" else (px <= w - 1.0)
    in_y = (py < h - 1.0) if slip == "py_lt_h1" else (py <= h - 1.0)
    mask = in_x & (px >= 0) & in_y & (py >= 0) & ((q[:, 2] >= 0) if slip == "q2_ge_0" else (q[:, 2] > 0))
    ix = ((2.0 * px / (w - 1.0) - 1.0 + 1) / 2) * (wf - 1)
    iy = ((2.0 * py / (h - 1.0) - 1.0 + 1) / 2) * (hf - 1)
    fx, fy = ix.floor(), iy.floor()
    xa, xb = (fx >= 0) & (fx <= wf - 1), (fx >= (0 if slip == "xb_from_0" else -1)) & (fx <= wf - 2)
    ya, yb = (fy >= 0) & (fy <= hf - 1), (fy >= (0 if slip == "yb_from_0" else -1)) & (fy <= hf - 2)
    wx0, wx1, wy0, wy1 = fx + 1 - ix, ix - fx, fy + 1 - iy, iy - fy
    tap = (ya & xa & (wx0 * wy0 != 0)) | (ya & xb & (wx1 * wy0 != 0)) | (yb & xa & (wx0 * wy1 != 0)) | (yb & xb & (wx1 * wy1 != 0))
    return mask.t(), tap.t()
