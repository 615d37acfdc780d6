"""numpy restatement of the keep rule of the early-stop kernels (csrc/early_stop_kernels.hip, include/nerfdet_hip.h): which samples of one
depth segment ndet_front_count / ndet_front_write keep.  Written from the definition, not from the kernel; the lattice test is
tests/skip_empty_ref.py's."""
import numpy as np

import skip_empty_ref as SE


def live(T, eps):
    """(R,) bool: ray r is live iff ``!(T[r] < eps)`` in float32 -- a NaN transmittance and ``T == eps`` keep the ray."""
    T = np.asarray(T, dtype=np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        return ~(T < np.float32(eps))


def keep_mask(pts, T, s0, s1, eps, grid=None):
    """(R, w) bool over the virtual points (r, c) of the segment ``[s0, s1)`` of ``pts`` (R, S, 3): the ray is live and, with
    ``grid = (bits, n_voxels, p0, vs, outside)``, the lattice keeps ``pts[r, s0 + c]``."""
    pts = np.asarray(pts, dtype=np.float32)
    r, s = pts.shape[:2]
    assert 0 <= s0 < s1 <= s and s1 - s0 <= 32
    w = s1 - s0
    keep = np.repeat(live(T, eps)[:, None], w, axis=1)
    if grid is not None:
        bits, nv, p0, vs, outside = grid
        keep &= SE.keep_mask(pts[:, s0:s1].reshape(-1, 3), bits, nv, p0, vs, outside).reshape(r, w)
    return keep


def front(pts, T, s0, s1, eps, grid=None):
    """``(idx (M,) int32, pts_kept (M, 3) float32)``: the flat indices ``f = r S + s0 + c`` of the kept virtual points, ascending."""
    pts = np.asarray(pts, dtype=np.float32)
    s = pts.shape[1]
    rr, cc = np.nonzero(keep_mask(pts, T, s0, s1, eps, grid))          # row-major: (r, c) ascending is f ascending
    idx = (rr * s + s0 + cc).astype(np.int32)
    return idx, pts.reshape(-1, 3)[idx]


def front_blocks(n_rays, w):
    """ndet_front_blocks: a block is 512 / nominal rays, nominal the least of 4, 8, 16, 32 that holds w."""
    if n_rays <= 0 or not 1 <= w <= 32:
        return 0
    nominal = next(n for n in (4, 8, 16, 32) if w <= n)
    per = 512 // nominal
    return (n_rays + per - 1) // per
