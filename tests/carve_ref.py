"""numpy restatement of space carving from depth frames (csrc/carve_kernels.hip, include/nerfdet_hip.h): a view's evidence
for a fine voxel, the packed saturating counters and the carved bit grid.  Written from the definitions, on
``oracle.nerfdet_oracle.project_voxels`` for the projection; plus the inputs the tests share."""
from __future__ import annotations

import numpy as np
import torch

from oracle import nerfdet_oracle as O
from skip_empty_ref import pack_bits

SAT = 65535


def project(points, projection):
    """``(fu, fv, z)`` float32 arrays (k, N): oracle.nerfdet_oracle.project_voxels' pixel coordinates before rounding and camera depths."""
    with np.errstate(all="ignore"):
        return tuple(t.numpy() for t in O.project_voxels(points, projection))


def evidence(points, projection, depth, band, hw, projected=None):
    """``(free (k, N) bool, hit (k, N) bool)`` of k views for the N lattice points ``points`` (3, X, Y, Z) float32 tensor: ``projection``
    (k, 3, 4) float32 tensor, ``depth`` (k, H, W) float32 / float64 array at the image's size ``hw``.  The pixel is the rounded
    (half-even) projection, accepted iff in the image with z > 0; d = the map there; ``not d > 0`` says nothing; in the map's dtype
    (band rounded to it, z widened exactly) free iff ``not (z > d - band)``, hit iff ``d - band < z < d + band``.  ``projected``:
    :func:`project` of the same points and projections, when the caller has it already."""
    h, w = hw
    depth = np.asarray(depth)
    assert depth.dtype in (np.float32, np.float64) and depth.shape[1:] == (h, w)
    with np.errstate(all="ignore"):
        fu, fv, z = projected if projected is not None else project(points, projection)
        x, y = np.rint(fu), np.rint(fv)
        ok = (x >= 0) & (y >= 0) & (x < np.float32(w)) & (y < np.float32(h)) & (z > 0)
        xi, yi = np.where(ok, x, 0).astype(np.int64), np.where(ok, y, 0).astype(np.int64)
        d = depth[np.arange(depth.shape[0])[:, None], yi, xi]
        b = depth.dtype.type(band)
        zz = z.astype(depth.dtype)
        lo, hi = (d - b).astype(depth.dtype), (d + b).astype(depth.dtype)
        seen = ok & (d > 0)
        free = seen & ~(zz > lo)
        hit = seen & (zz > lo) & (zz < hi)
    return free, hit


def unpack(words):
    """int32 / uint32 words -> ``(free, hit)`` int64."""
    w = np.asarray(words).view(np.uint32).astype(np.int64)
    return w & 0xffff, w >> 16


def pack(free, hit):
    return ((np.minimum(free, SAT) | (np.minimum(hit, SAT) << 16)).astype(np.uint32)).view(np.int32)


def accumulate(words, points, projection, depth, band, hw, projected=None):
    """The counter words after a chunk: each count plus the chunk's, saturating at 65535."""
    free, hit = evidence(points, projection, depth, band, hw, projected)
    f0, h0 = unpack(words)
    return pack(f0 + free.sum(0), h0 + hit.sum(0))


def dilate_mask(m, dilate):
    """Any voxel within Chebyshev distance ``dilate``, inside the grid, is set: a running OR over shifted copies, axis by axis."""
    for axis in range(3):
        out = m.copy()
        for s in range(1, int(dilate) + 1):
            lo, hi = [slice(None)] * 3, [slice(None)] * 3
            lo[axis], hi[axis] = slice(0, m.shape[axis] - s), slice(s, None)
            if m.shape[axis] > s:
                out[tuple(lo)] |= m[tuple(hi)]
                out[tuple(hi)] |= m[tuple(lo)]
        m = out
    return m


def solid_mask(segments, n_voxels, min_free, coarse_bits=None, refine=1):
    """(X, Y, Z) bool: not (free >= min_free and hit == 0) over the segments' sums; with ``coarse_bits`` ANDed with the parent voxel's bit."""
    nx, ny, nz = (int(v) for v in n_voxels)
    free = sum(unpack(s)[0] for s in segments)
    hit = sum(unpack(s)[1] for s in segments)
    solid = ~((free >= min_free) & (hit == 0)).reshape(nx, ny, nz)
    if coarse_bits is not None:
        r = int(refine)
        cw = np.asarray(coarse_bits).view(np.uint32)
        n_par = (nx // r) * (ny // r) * (nz // r)
        par = ((cw[np.arange(n_par) >> 5] >> (np.arange(n_par) & 31).astype(np.uint32)) & 1).astype(bool).reshape(nx // r, ny // r, nz // r)
        solid &= np.repeat(np.repeat(np.repeat(par, r, 0), r, 1), r, 2)
    return solid


def bits(segments, n_voxels, min_free, dilate, coarse_bits=None, refine=1):
    return pack_bits(dilate_mask(solid_mask(segments, n_voxels, min_free, coarse_bits, refine), dilate))


# ---- shared inputs ----
HW = (24, 32)
VS = (0.25, 0.25, 0.25)           # dyadic: the lattice points, the dyadic cameras' z and d +- band are exact in float32
ORIGIN = (0.5, -0.25, 0.125)
BAND = 0.25


def fine_points(n_voxels, refine):
    """The fine lattice (3, rX, rY, rZ) float32 tensor of the detection lattice ``n_voxels`` at VS around ORIGIN."""
    return O.get_points([refine * v for v in n_voxels], [v / refine for v in VS], ORIGIN)


def _look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """world -> camera (3, 4), camera z towards ``target``."""
    eye, target = np.float64(eye), np.float64(target)
    f = target - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, np.float64(up))
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    rot = np.stack([r, d, f])
    return np.concatenate([rot, (-rot @ eye)[:, None]], axis=1)


def views_case(n_voxels, k, dtype, seed=0):
    """``(projection (k, 3, 4) float32 tensor, depth (k, H, W) array of ``dtype``)`` for the lattice: view 0 is DYADIC -- it looks along
    +x from x = ORIGIN_x - 3 with focal 32, so z = x + const exactly, over depths of 3 and 2.875 m: lattice layers lie exactly on
    d - band (free) and d + band (behind) -- the others look at the lattice from a ring of radius 1.2 to 3 m, every third from
    INSIDE the box (points behind the camera), with a focal length that leaves part of the lattice outside the image, over a wavy
    depth around the distance to the centre, so that free, hit and behind all occur.  Every view but the first has 8 % holes; view
    1 % k holds a negative and a NaN patch."""
    rng = np.random.RandomState(1000 * seed + 17 * k + n_voxels[2])
    h, w = HW
    centre = np.float64(ORIGIN)
    kk = np.float64([[32.0, 0, 16.0], [0, 32.0, 12.0], [0, 0, 1.0]])
    proj, depth = [], []
    ext0 = np.float64([[0, 1, 0, 0.25], [0, 0, 1, -0.125], [1, 0, 0, 3.0 - ORIGIN[0]]])       # z = x - ORIGIN_x + 3
    proj.append(kk @ ext0)
    depth.append(np.where(np.arange(w)[None] < 16, 3.0, 2.875) * np.ones((h, 1)))        # two constants: every lattice of the tests meets both edges
    vv, uu = np.mgrid[0:h, 0:w]
    for v in range(1, k):
        ang, rad = rng.rand() * 2 * np.pi, (0.2 if v % 3 == 2 else 1.2 + 1.8 * rng.rand())
        eye = centre + rad * np.float64([np.cos(ang), np.sin(ang), 0.6 * rng.rand() - 0.2])
        ext = _look_at(eye, centre + 0.3 * (rng.rand(3) - 0.5))
        f = 20.0 + 20.0 * rng.rand()
        proj.append(np.float64([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1.0]]) @ ext)
        d = rad + 0.5 * np.sin(uu / 3.0 + v) * np.cos(vv / 4.0) + 0.2 * rng.rand(h, w)
        d[rng.rand(h, w) < 0.08] = 0.0
        depth.append(d)
    depth = np.stack(depth)
    if k > 1:
        depth[1, 8:12, 10:16] = -1.5
        depth[1, 12:16, 16:22] = np.nan
    else:
        depth[0, 4:7, 13:16] = 0.0
        depth[0, 16:19, 13:16] = -2.0
        depth[0, 10:12, 17:20] = np.nan
    return torch.from_numpy(np.stack(proj).astype(np.float32)), depth.astype(dtype)


def segments_case(n, n_segs, seed):
    """``n_segs`` counter segments (n,) int32: per voxel a total free count from {0, 1, 2, 3, 5} and a total hit count (0 for three
    voxels in four, else 1 or 2) dealt over the segments at random; voxel 1 is free 65535 times in every segment, voxel 2 hit so."""
    rng = np.random.RandomState(seed)
    free = np.zeros((n_segs, n), dtype=np.int64)
    hit = np.zeros((n_segs, n), dtype=np.int64)
    tot_f = rng.choice([0, 1, 2, 3, 5], n)
    tot_h = np.where(rng.rand(n) < 0.75, 0, rng.randint(1, 3, n))
    for tot, out in ((tot_f, free), (tot_h, hit)):
        for _ in range(int(tot.max())):
            live = tot > 0
            np.add.at(out, (rng.randint(0, n_segs, n)[live], np.nonzero(live)[0]), 1)
            tot = tot - live
    if n > 2:
        free[:, 1], hit[:, 1] = SAT, 0
        free[:, 2], hit[:, 2] = 3, SAT
    return [pack(free[j], hit[j]) for j in range(n_segs)]


# ---- the wall scene of the geometry check (float64 throughout, apart from the restatement itself) ----
WALL_X = 1.5


def wall_scene(n_views=6, hw=(48, 64), focal=64.0):
    """Cameras within about 20 degrees of the normal of the wall plane x = WALL_X, looking at it from x around -2.6, and their ANALYTIC
    float64 depth maps (camera depth of the wall along each pixel's ray).  Returns ``(projection (k, 3, 4) float32 tensor, depth
    (k, H, W) float64, extrinsics (k, 3, 4) float64, intrinsic (3, 3) float64)``."""
    h, w = hw
    kk = np.float64([[focal, 0, w / 2 - 0.5], [0, focal, h / 2 - 0.5], [0, 0, 1.0]])
    kinv = np.linalg.inv(kk)
    vv, uu = np.mgrid[0:h, 0:w].astype(np.float64)
    pix = np.stack([uu.ravel(), vv.ravel(), np.ones(uu.size)])
    exts, depth = [], []
    for v in range(n_views):
        yaw, pitch = np.deg2rad(-12.0 + 24.0 * v / max(n_views - 1, 1)), np.deg2rad(6.0 * ((v % 3) - 1))
        fwd = np.float64([np.cos(yaw) * np.cos(pitch), np.sin(yaw) * np.cos(pitch), np.sin(pitch)])
        target = np.float64([WALL_X, 0.1 * (v - 2.5), 0.05 * v])
        eye = target - 4.1 * fwd
        ext = _look_at(eye, target)
        rot, t = ext[:, :3], ext[:, 3]
        dw = rot.T @ (kinv @ pix)                           # world directions of the pixels' rays, camera z = 1
        s = (WALL_X - eye[0]) / dw[0]                       # = camera depth of the wall along the ray
        assert (s > 0).all()
        exts.append(ext)
        depth.append(s.reshape(h, w))
    exts = np.stack(exts)
    return torch.from_numpy((kk @ exts).astype(np.float32)), np.stack(depth), exts, kk
