"""The numpy side of the NV12 tests (ndet_resize_normalize_views_nv12, ndet_nv12_to_bgr, ndet_bgr_to_nv12 and what stands on them): NV12
surfaces packed with a pitch and a uv_row of the caller's choice and unpacked again, the two data sets every size is tested on, a
FLOATING-point conversion that the host definition must differ from (the blindness check), and the oracle --

    raw_frames_ref.prepare(stack(datasets.nv12_to_bgr(surface)), ...)

the datasets chain of tests/raw_frames_ref.py on the host-converted frames.

Test infrastructure only."""
import numpy as np

import raw_frames_ref as R

# capture size (even), img_scale (w, h), resized size, pad size: the even counterparts of raw_frames_ref.SIZES
SIZES = {
    "38x54-down-bottom-pad": ((38, 54), (32, 24), (23, 32), (24, 32)),
    "100x130-right-pad": ((100, 130), (32, 24), (24, 31), (24, 32)),
    "20x24-upscale": ((20, 24), (32, 24), (24, 29), (24, 32)),
    "24x32-copy": ((24, 32), (32, 24), (24, 32), (24, 32)),
    "98x132-no-pad": ((98, 132), (32, 24), (24, 32), (24, 32)),
}
DATA = ("full-range", "video-range")
SLACK = 0xA5    # what fills the bytes of a padded layout that belong to no plane


def planes(size_hw, data: str, n: int = 14, seed: int = 0):
    """``(y (n, Hs, Ws), uv (n, Hs/2, Ws/2, 2))`` uint8.  'full-range': random bytes, which reach the Y < 16 clamp and both saturations of
    every channel (about 40 % of the converted bytes are saturated); 'video-range': Y in [16, 235], U and V in [96, 160], where about 10 %
    are, so a wrong coefficient or rounding shows in the rest."""
    hs, ws = size_hw
    assert hs % 2 == 0 and ws % 2 == 0 and data in DATA
    rng = np.random.RandomState(hs * 1000 + ws + 7 * seed + (0 if data == "full-range" else 1))
    if data == "full-range":
        return rng.randint(0, 256, (n, hs, ws)).astype(np.uint8), rng.randint(0, 256, (n, hs // 2, ws // 2, 2)).astype(np.uint8)
    return rng.randint(16, 236, (n, hs, ws)).astype(np.uint8), rng.randint(96, 161, (n, hs // 2, ws // 2, 2)).astype(np.uint8)


def padded_layout(size_hw):
    """``(pitch, uv_row, rows)`` of the tests' padded layout: pitch = Ws + 10 rounded up to even, two slack rows between the planes and one
    after them."""
    hs, ws = size_hw
    pitch = ws + 10 + (ws + 10) % 2
    return pitch, hs + 2, hs + 2 + hs // 2 + 1


def tight_layout(size_hw):
    hs, ws = size_hw
    return ws, hs, hs * 3 // 2


def pack(y, uv, pitch=None, uv_row=None, rows=None):
    """Surfaces (n, rows, pitch) uint8 from planes; the defaults are tight.  Every byte outside the planes is SLACK."""
    n, hs, ws = y.shape
    pitch, uv_row = ws if pitch is None else pitch, hs if uv_row is None else uv_row
    rows = uv_row + hs // 2 if rows is None else rows
    assert pitch >= ws and uv_row >= hs and rows >= uv_row + hs // 2 and uv.shape == (n, hs // 2, ws // 2, 2)
    s = np.full((n, rows, pitch), SLACK, np.uint8)
    s[:, :hs, :ws] = y
    s[:, uv_row:uv_row + hs // 2, :ws] = uv.reshape(n, hs // 2, ws)
    return s


def unpack(surfaces, size_hw, uv_row=None):
    """``(y, uv)`` of surfaces (n, rows, pitch)."""
    hs, ws = size_hw
    uv_row = hs if uv_row is None else uv_row
    return surfaces[:, :hs, :ws].copy(), surfaces[:, uv_row:uv_row + hs // 2, :ws].reshape(len(surfaces), hs // 2, ws // 2, 2).copy()


def to_bgr(y, uv):
    """The host definition on a batch: (n, Hs, Ws, 3) uint8."""
    from nerfdet_amd.datasets import nv12_to_bgr
    return np.stack([nv12_to_bgr(a, b) for a, b in zip(y, uv)])


def to_nv12(frames):
    """The host definition of the other direction on a batch, as tight surfaces (n, He * 3 / 2, We)."""
    from nerfdet_amd.datasets import bgr_to_nv12
    out = [bgr_to_nv12(f) for f in frames]
    return pack(np.stack([o[0] for o in out]), np.stack([o[1] for o in out]))


def float_nv12_to_bgr(y, uv):
    """BT.601 limited range in floating point with the textbook coefficients and round-to-nearest: what a kernel that converted in
    floats would give.  One surface."""
    yy = 1.164 * (y.astype(np.float64) - 16.0)
    c = uv.astype(np.float64).repeat(2, axis=0).repeat(2, axis=1) - 128.0
    u, v = c[..., 0], c[..., 1]
    bgr = np.stack((yy + 2.018 * u, yy - 0.813 * v - 0.391 * u, yy + 1.596 * v), axis=-1)
    return np.clip(np.rint(bgr), 0, 255).astype(np.uint8)


def prepare(y, uv, img_scale, pad_size, mean, std, ids=None):
    """The oracle: raw_frames_ref.prepare on the host-converted frames."""
    return R.prepare(to_bgr(y, uv), img_scale, pad_size, mean, std, ids=ids)
