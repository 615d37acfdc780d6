"""Numpy restatement of ndet_frame_ssim (include/nerfdet_hip.h) and the inputs the frame-SSIM tests share.  Byte form: cumulative-sum box
sums in int64, the five float64 lines of the definition, ``np.rint`` -- the kernel's ``ssim_sum`` and ``n_windows`` to the bit.  Float form:
the same lines on float64 box sums (a tolerance reference, not a bit reference)."""
import numpy as np

WIN = 7
NP = WIN * WIN
# float64, left to right -- what csrc/frame_ssim_kernels.hip carries as hexadecimal literals
C1_U8 = (0.01 * 2 * 255) * (0.01 * 2 * 255) * (49 * 49)
C2_U8 = (0.03 * 2 * 255) * (0.03 * 2 * 255) * (49 * 48)
C1_F32 = (0.01 * 2) * (0.01 * 2) * (49 * 49)
C2_F32 = (0.03 * 2) * (0.03 * 2) * (49 * 48)
SCALE = float(2 ** 40)


def box(t):
    """Sums over the valid 7 x 7 windows of the two axes after the first: (n, h, w, ...) -> (n, h - 6, w - 6, ...), in t's dtype."""
    c = np.cumsum(np.cumsum(t, axis=1), axis=2)
    c = np.pad(c, [(0, 0), (1, 0), (1, 0)] + [(0, 0)] * (t.ndim - 3))
    return c[:, WIN:, WIN:] - c[:, :-WIN, WIN:] - c[:, WIN:, :-WIN] + c[:, :-WIN, :-WIN]


def counting(shape, depth_a):
    """(n, h - 6, w - 6) bool: the windows all of whose 49 pixels have depth_a != 0; every window without depth_a."""
    n, h, w = shape
    if depth_a is None:
        return np.ones((n, h - WIN + 1, w - WIN + 1), dtype=bool)
    return box((np.asarray(depth_a) != 0).astype(np.int64)) == NP


def frame_ssim_ref(a, b, depth_a=None):
    """(n, 4) int64: Q_0, Q_1, Q_2, n_w of uint8 frames a, b (n, h, w, 3)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.uint8 and b.dtype == np.uint8 and a.shape == b.shape and a.ndim == 4 and a.shape[3] == 3
    x, y = a.astype(np.int64), b.astype(np.int64)
    sx, sy, sxx, syy, sxy = box(x), box(y), box(x * x), box(y * y), box(x * y)
    a1 = (2 * sx * sy).astype(np.float64) + C1_U8
    a2 = (2 * (NP * sxy - sx * sy)).astype(np.float64) + C2_U8
    b1 = (sx * sx + sy * sy).astype(np.float64) + C1_U8
    b2 = (NP * sxx - sx * sx + NP * syy - sy * sy).astype(np.float64) + C2_U8
    s = (a1 * a2) / (b1 * b2)
    q = np.rint(s * SCALE).astype(np.int64)
    cnt = counting(a.shape[:3], depth_a)
    out = np.zeros((a.shape[0], 4), dtype=np.int64)
    out[:, :3] = (q * cnt[..., None]).sum(axis=(1, 2))
    out[:, 3] = cnt.sum(axis=(1, 2))
    return out


def frame_ssim_f32_ref(a, b, depth_a=None):
    """The float form's definition in float64 numpy: (n, 4) int64.  Its box sums add in another order than the kernel's."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape
    x, y = a.astype(np.float64), b.astype(np.float64)
    win = lambda t: np.lib.stride_tricks.sliding_window_view(t, (WIN, WIN), axis=(1, 2)).sum(axis=(-2, -1))
    sx, sy, sxx, syy, sxy = win(x), win(y), win(x * x), win(y * y), win(x * y)
    a1 = 2.0 * (sx * sy) + C1_F32
    a2 = 2.0 * (NP * sxy - sx * sy) + C2_F32
    b1 = (sx * sx + sy * sy) + C1_F32
    b2 = ((NP * sxx - sx * sx) + (NP * syy - sy * sy)) + C2_F32
    q = np.rint((a1 * a2) / (b1 * b2) * SCALE).astype(np.int64)
    cnt = counting(a.shape[:3], depth_a)
    out = np.zeros((a.shape[0], 4), dtype=np.int64)
    out[:, :3] = (q * cnt[..., None]).sum(axis=(1, 2))
    out[:, 3] = cnt.sum(axis=(1, 2))
    return out


def ssim_of(out):
    """``(ssim_channels (n,3), ssim (n,))`` float64 of an (n, 4) result, as pipeline.frame_ssim forms them: nan where n_w == 0."""
    out = np.asarray(out)
    with np.errstate(divide="ignore", invalid="ignore"):
        ch = out[:, :3].astype(np.float64) / (SCALE * out[:, 3].astype(np.float64))[:, None]
    return ch, (ch[:, 0] + ch[:, 1] + ch[:, 2]) / 3.0


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
TILE = (16, 32)          # pipeline.SSIM_TILE; tests/test_frame_ssim_cpu.py checks that the two agree


def shapes(tile=TILE):
    """(h, w): one window, one row and one column of windows, two small odd sizes, one window past a tile seam in each direction, and exactly
    whole tiles."""
    th, tw = tile
    return [(7, 7), (7, 40), (40, 7), (8, 13), (39, 70), (th + 7, 2 * tw + 7), (2 * th + 6, tw + 6)]


CONTENTS = ("random", "smooth", "equal", "extremes", "inverted", "channels")


def frames(content, n, h, w, seed=0):
    """``a, b (n, h, w, 3) uint8`` with different content in every frame."""
    rs = np.random.RandomState(1000 * seed + 7 * h + w + 131 * n + CONTENTS.index(content))
    a = rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    if content == "random":
        b = rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    elif content == "smooth":        # a smooth pattern, and the same pattern plus noise: SSIM about 0.97
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        base = np.stack([127.5 + 100.0 * np.sin(xx / (5.0 + f) + c) * np.cos(yy / (7.0 + c) + f) for f in range(n) for c in range(3)])
        base = base.reshape(n, 3, h, w).transpose(0, 2, 3, 1)
        a = np.clip(np.rint(base), 0, 255).astype(np.uint8)
        b = np.clip(np.rint(base + rs.normal(0.0, 4.0, base.shape)), 0, 255).astype(np.uint8)
    elif content == "equal":
        b = a.copy()
    elif content == "extremes":      # the largest integer terms, a tiny positive s
        a = np.full((n, h, w, 3), 255, dtype=np.uint8)
        b = np.zeros((n, h, w, 3), dtype=np.uint8)
    elif content == "inverted":      # s about -0.94: negative q
        b = (255 - a.astype(np.int64)).astype(np.uint8)
    elif content == "channels":      # channel 0 equal, channel 1 inverted, channel 2 unrelated
        b = rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
        b[..., 0] = a[..., 0]
        b[..., 1] = 255 - a[..., 1]
    else:
        raise KeyError(content)
    return a, b


HOLES = ("corner", "seam", "row", "frame")


def holes(kind, n, h, w, tile=TILE):
    """``depth_a (n, h, w) uint16``, non-zero but for: one corner pixel of every frame; one interior pixel next to the tile seams (pixel
    (th + 2, tw + 2) lies in the 49 windows (th - 4 .. th + 2, tw - 4 .. tw + 2): both sides of both seams, when the frame is large enough);
    one whole row; the whole of frame 1."""
    rs = np.random.RandomState(17 + h * w)
    d = rs.randint(1, 65536, (n, h, w)).astype(np.uint16)
    if kind == "corner":
        d[:, 0, 0] = 0
    elif kind == "seam":
        d[:, min(h - 1, tile[0] + 2), min(w - 1, tile[1] + 2)] = 0
    elif kind == "row":
        d[:, h // 2, :] = 0
    elif kind == "frame":
        d[1 % n] = 0
    else:
        raise KeyError(kind)
    return d


def float_frames(n, h, w, seed=0):
    """``pred, target (n, h, w, 3) float32`` in [0, 1]: a smooth target and a noisy render of it, as render_testing produces."""
    rs = np.random.RandomState(500 + seed + h * w + n)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    t = np.stack([0.5 + 0.4 * np.sin(xx / (4.0 + f) + c) * np.cos(yy / (6.0 + c) - f) for f in range(n) for c in range(3)])
    t = t.reshape(n, 3, h, w).transpose(0, 2, 3, 1)
    p = np.clip(t + rs.normal(0.0, 0.05, t.shape), 0.0, 1.0)
    return np.ascontiguousarray(p, dtype=np.float32), np.ascontiguousarray(t, dtype=np.float32)
