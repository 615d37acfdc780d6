"""The numpy oracle of the depth-frame path (ndet_depth_frames, ndet_positive_indices, pipeline.prepare_depth_frames,
MultiViewPipeline(depth_frames=), add_frames(depth_frames=)): nothing but

  1. frame / 1000                                   the sensor's uint16 millimetres -> float64 metres (multi_view.py:102-104)
  2. datasets.imresize_linear(., (w, h))            the project's definition of mmcv.imresize, float64 branch
  3. the margin crop [m, h - m) x [m, w - m)         the target views' pixel grid (multi_view.py:124-132, 156-166)
  4. np.flatnonzero(. > 0)                          the rays with depth (render_ray.py:386-404, datasets.py:293)

Depth frames are random uint16 in [400, 6000) with 4 x 4 patches of zeros (a sensor's holes), so that some resized pixels are exactly 0.
Test infrastructure only."""
import numpy as np

# depth size -> output size: what each exercises is in tests/test_depth_frames_gpu.py
CASES = {
    "30x41-noninteger": ((30, 41), (22, 32)),
    "48x64-ratio2": ((48, 64), (24, 32)),
    "13x17-upscale": ((13, 17), (24, 32)),
    "24x32-copy": ((24, 32), (24, 32)),
    "61x83-reduce2.7": ((61, 83), (22, 32)),
}
NONINTEGER = ("30x41-noninteger", "13x17-upscale", "61x83-reduce2.7")
N_FRAMES = 14
SEED = 5
MARGINS = (0, 2)
IDS = {"descending-with-repeats": [13, 13, 9, 9, 4, 2, 2, 0], "null": None}
CAPTURE = ((480, 640), ((239, 320, 0), (240, 320, 10)))      # one pair of real frames -> (h, w, margin)
_frames_cache = {}


def frames(size_hw, n=N_FRAMES, seed=SEED):
    """(n, Hd, Wd) uint16 in [400, 6000) with about a tenth of the area in 4 x 4 zero patches; computed once per size, read-only."""
    key = (tuple(size_hw), n, seed)
    if key not in _frames_cache:
        h, w = size_hw
        rs = np.random.RandomState(seed + 1000 * h + w)
        d = rs.randint(400, 6000, (n, h, w)).astype(np.uint16)
        for f in range(n):
            for _ in range(max(1, h * w // 160)):
                y, x = rs.randint(0, h - 3), rs.randint(0, w - 3)
                d[f, y:y + 4, x:x + 4] = 0
        d.setflags(write=False)
        _frames_cache[key] = d
    return _frames_cache[key]


def resize(frames_u16, size_hw, ids=None, margin=0):
    """Links 1-3: (n_sel, h - 2m, w - 2m) float64.  Each distinct frame is resized once."""
    from nerfdet_amd.datasets import imresize_linear
    h, w = size_hw
    ids = list(range(len(frames_u16))) if ids is None else [int(i) for i in ids]
    one = {i: imresize_linear(frames_u16[i] / 1000, (w, h))[margin:h - margin, margin:w - margin] for i in set(ids)}
    return np.ascontiguousarray(np.stack([one[i] for i in ids]))


def batch(frames_u16, ids, target_ids, view_hw, pad_hw, margin):
    """The depth keys of a collated batch: ``depth`` (1, n_v, Hr, Wr), and with targets ``gt_depths`` (1, T, H - 2m, W - 2m) and
    ``depth_rays`` (1, K) int64."""
    out = dict(depth=resize(frames_u16, view_hw, ids)[None])
    if len(target_ids):
        gd = resize(frames_u16, pad_hw, target_ids, margin)
        out.update(gt_depths=gd[None], depth_rays=np.flatnonzero(gd.reshape(-1) > 0)[None])
    return out


# ---- variants that must differ from the oracle (tests/test_depth_frames_cpu.py) ----
def _taps(n_dst, n_src):
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * (n_src / n_dst) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    lo = s < 0
    f[lo], s[lo] = 0.0, 0
    hi = s >= n_src - 1
    f[hi], s[hi] = 0.0, n_src - 1
    return s, np.minimum(s + 1, n_src - 1), f


def variant_multiply(frame_u16, size_hw):
    """frame * 0.001 in place of frame / 1000."""
    from nerfdet_amd.datasets import imresize_linear
    return imresize_linear(frame_u16 * 0.001, (size_hw[1], size_hw[0]))


def variant_float32(frame_u16, size_hw):
    """The interpolation in float32 (imresize_linear's branch for a float32 image), widened afterwards."""
    from nerfdet_amd.datasets import imresize_linear
    return imresize_linear((frame_u16 / 1000).astype(np.float32), (size_hw[1], size_hw[0])).astype(np.float64)


def variant_contracted(frame_u16, size_hw):
    """Each pass as fma(a, 1 - f, b * f): the product b * f rounded, a * (1 - f) + that rounded ONCE -- what a compiler that contracts
    the first product into the sum would give.  Emulated exactly with rationals."""
    from fractions import Fraction
    h, w = size_hw
    src = frame_u16 / 1000
    hs, ws = src.shape
    if (hs, ws) == (h, w):
        return src.copy()
    x0, x1, fx = _taps(w, ws)
    y0, y1, fy = _taps(h, hs)
    fx, fy = fx.astype(np.float64), fy.astype(np.float64)

    def fma(a, g, bf):
        return float(Fraction(a) * Fraction(g) + Fraction(bf))      # float(Fraction) rounds to nearest even
    hor = np.empty((hs, w))
    for y in range(hs):
        for x in range(w):
            hor[y, x] = fma(src[y, x0[x]], 1 - fx[x], src[y, x1[x]] * fx[x])
    out = np.empty((h, w))
    for y in range(h):
        for x in range(w):
            out[y, x] = fma(hor[y0[y], x], 1 - fy[y], hor[y1[y], x] * fy[y])
    return out
