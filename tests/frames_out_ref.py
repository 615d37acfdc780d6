"""numpy references of the frames-out kernels (csrc/frames_out_kernels.hip) and the inputs that tell their arithmetic from its near misses.

``camera_rays_ref`` follows k_camera_rays' float32 operation order; its one fused step is rounded once from exact rationals (the ``rn32`` of
tests/test_fullsize_reference_cpu.py).  ``pack_frames_ref`` works in float32, ``frame_errors_ref`` in Python / numpy integers."""
from fractions import Fraction

import numpy as np

F = np.float32


def rn32(fr):
    """Correctly rounded float32 of a rational: the nearest of a first guess and its neighbours, ties to even."""
    y = F(float(fr))
    cands = [y, np.nextafter(y, F(np.inf)), np.nextafter(y, F(-np.inf))]
    return F(min(cands, key=lambda c: (abs(Fraction(float(c)) - fr), int(F(c).view(np.int32)) & 1)))


def fmaf(a, b, c):
    """fmaf on float32 scalars: a * b + c rounded once."""
    return rn32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def camera_rays_ref(krows, rot, lpos, window, stride=1):
    """``(ray_o, ray_d)``, each (n, h * w, 3) float32: output pixel (i, j) looks through image pixel (y0 + i * stride, x0 + j * stride);
    x = ((float)px + 0.5f - k[2]) / k[0], y likewise, d_r = fmaf(y, R[r][1], x * R[r][0]) + R[r][2]; the camera centre repeated."""
    k = np.asarray(krows, dtype=F).reshape(6)
    rot, lpos = np.asarray(rot, dtype=F), np.asarray(lpos, dtype=F)
    y0, x0, h, w = window
    n = rot.shape[0]
    xs = ((np.arange(w, dtype=np.int64) * stride + x0).astype(F) + F(0.5) - k[2]) / k[0]
    ys = ((np.arange(h, dtype=np.int64) * stride + y0).astype(F) + F(0.5) - k[5]) / k[4]
    assert xs.dtype == F and ys.dtype == F
    ray_d = np.empty((n, h, w, 3), dtype=F)
    for c in range(n):
        for r in range(3):
            xr = xs * rot[c, r, 0]                                   # float32 products, one per column
            for i in range(h):
                for j in range(w):
                    ray_d[c, i, j, r] = fmaf(ys[i], rot[c, r, 1], xr[j]) + rot[c, r, 2]
    ray_o = np.broadcast_to(lpos[:, None, :], (n, h * w, 3)).copy()
    return ray_o, ray_d.reshape(n, h * w, 3)


def _quantise(v, hi):
    """NaN and v < 0 give 0, v > hi gives hi, else trunc(v + 0.5f), all on float32 ``v``."""
    assert v.dtype == F
    with np.errstate(invalid="ignore", over="ignore"):
        inside = (v >= 0) & (v <= F(hi))
        q = np.where(inside, v + F(0.5), F(0)).astype(F).astype(np.int64)
        return np.where(v > F(hi), int(hi), q)


def pack_frames_ref(rgb, depth, mask=None):
    """``(bytes like rgb, uint16 like depth)``: v = x * 255.0f / d = depth * 1000.0f in float32, quantised as above; depth 0 where mask is false."""
    rgb, depth = np.asarray(rgb, dtype=F), np.asarray(depth, dtype=F)
    with np.errstate(invalid="ignore", over="ignore"):
        b = _quantise(rgb * F(255.0), 255.0).astype(np.uint8)
        d = _quantise(depth * F(1000.0), 65535.0)
    if mask is not None:
        d = np.where(np.asarray(mask, dtype=bool), d, 0)
    return b, d.astype(np.uint16)


def frame_errors_ref(a, b, da, db=None):
    """(n, 4) int64: sse over the bytes of the pixels with da != 0, their number, sum |da - db| over da != 0 and db != 0, their number."""
    a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    da = np.asarray(da).astype(np.int64)
    n = a.shape[0]
    a, b, da = a.reshape(n, -1, 3), b.reshape(n, -1, 3), da.reshape(n, -1)
    seen = da != 0
    out = np.zeros((n, 4), dtype=np.int64)
    out[:, 0] = (((a - b) ** 2).sum(-1) * seen).sum(-1)
    out[:, 1] = seen.sum(-1)
    if db is not None:
        db = np.asarray(db).astype(np.int64).reshape(n, -1)
        both = seen & (db != 0)
        out[:, 2] = (np.abs(da - db) * both).sum(-1)
        out[:, 3] = both.sum(-1)
    return out


def psnr_ref(sse, n_px):
    """10 log10(255^2 * 3 * n_px / sse) in float64: inf where sse == 0, nan where n_px == 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(255.0 ** 2 * 3.0 * np.asarray(n_px, dtype=np.float64) / np.asarray(sse, dtype=np.float64))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
SPECIAL_RGB = [0.0, 1.0, -0.0, -1e-3, -5.0, 1.0 + 1e-6, 1.002, 7.0, np.inf, -np.inf, np.nan, 0.5 / 255, 254.5 / 255, 255.49 / 255, 255.5 / 255,
               1e-30, -1e-30, 0.999999]
SPECIAL_DEPTH = [0.0, 0.0004, 0.0005, 0.00049999, 65.5349, 65.535, 65.5354, 65.536, 100.0, -0.0, -1.0, np.inf, -np.inf, np.nan, 1e-30, 3.2765, 0.0015,
                 0.0025]


def edge_rgb():
    """The specials, then k / 255 and the ties (k + 0.5) / 255 for every byte k, as float32."""
    k = np.arange(256, dtype=np.float64)
    return np.concatenate([np.asarray(SPECIAL_RGB, dtype=np.float64), k / 255.0, (k + 0.5) / 255.0]).astype(F)


def edge_depth():
    return np.asarray(SPECIAL_DEPTH, dtype=np.float64).astype(F)


def pack_inputs(seed=0, n_random=1000):
    """``(rgb (L,3), depth (L,), mask (L,) bool)`` float32: the edge vectors plus ``n_random`` seeded values each -- colours in [-0.1, 1.1),
    depths in [0, 70) metres, the first 18 rows holding the specials of both; the mask drops every third row and keeps the specials twice
    (rows 0-17 kept, rows 18-35 the depth specials again, dropped)."""
    rs = np.random.RandomState(seed)
    c = np.concatenate([edge_rgb(), rs.uniform(-0.1, 1.1, n_random).astype(F)])
    c = np.concatenate([c, np.zeros((-len(c)) % 3, dtype=F)]).reshape(-1, 3)
    rows = c.shape[0]
    ed = edge_depth()
    d = np.concatenate([ed, ed, rs.uniform(0.0, 70.0, rows - 2 * len(ed)).astype(F)])
    m = np.arange(rows) % 3 != 2
    m[:len(ed)] = True
    m[len(ed):2 * len(ed)] = False
    return c, d, m


def errors_inputs(n, h, w, seed=0):
    """Random frames and depth frames (about a third of either depth's pixels are holes): ``a, b (n,h,w,3) uint8, da, db (n,h,w) uint16``."""
    rs = np.random.RandomState(seed + 31 * n + h * w)
    a = rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    b = rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    da = (rs.randint(1, 65536, (n, h, w)) * (rs.rand(n, h, w) > 0.3)).astype(np.uint16)
    db = (rs.randint(1, 65536, (n, h, w)) * (rs.rand(n, h, w) > 0.3)).astype(np.uint16)
    return a, b, da, db


def cameras(n, seed=0):
    """Intrinsic rows (2,3) with fractional entries, n rotations (proper, from a QR) and n centres, float32."""
    rs = np.random.RandomState(100 + seed)
    krows = np.array([[28.893501, 0.0, 13.75], [0.0, 29.1337, 9.25]], dtype=F)
    rot = np.stack([np.linalg.qr(rs.randn(3, 3))[0] for _ in range(n)]).astype(F)
    lpos = (rs.randn(n, 3) * 2.0).astype(F)
    return krows, rot, lpos


def c2w_of(rot, lpos):
    m = np.tile(np.eye(4, dtype=F), (rot.shape[0], 1, 1))
    m[:, :3, :3], m[:, :3, 3] = rot, lpos
    return m
