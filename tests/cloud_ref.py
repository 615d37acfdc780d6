"""numpy restatement of the point cloud of a streamed RGB-D scene (csrc/cloud_kernels.hip, include/nerfdet_hip.h): a
pixel's point, its voxel and sub-voxel offset, the seven integer sums of a voxel, the emitted points and their labels.  Written from the
definitions; every fused step is ``detections_out_ref.fmaf_v`` (rounded once).  Plus the inputs the tests share."""
from __future__ import annotations

import numpy as np
import torch

from carve_ref import _look_at
from detections_out_ref import fmaf_v
from oracle import nerfdet_oracle as O

F = np.float32
FIELDS = ("n", "qx", "qy", "qz", "b", "g", "r")
PIXELS_MAX = 2 ** 24


# ---- definitions ----
def lattice(n_voxels, voxel_size, origin, refine):
    """``(n_voxels_fine, p0 (3,) float32, vs (3,) float32)``: the carve's fine lattice -- ``get_points(r n, voxel_size / r, origin)`` --
    its first point and its voxel size (a float32 division by a power of two is exact)."""
    nv = tuple(int(refine) * int(v) for v in n_voxels)
    vs = np.asarray(voxel_size, dtype=F) / F(refine)
    p0 = O.get_points(nv, [float(v) for v in vs], origin)[:, 0, 0, 0].numpy().astype(F)
    return nv, p0, vs


def krows_of(intrinsic):
    return np.ascontiguousarray(np.asarray(intrinsic)[:2, :3], dtype=F).reshape(6)


def c2w_of_extrinsics(extrinsics):
    """(k,4,4) float32 camera-to-world: the world-to-camera matrices inverted in float64, then rounded (pipeline.project_boxes' way)."""
    return np.linalg.inv(np.stack([np.asarray(e, dtype=np.float64) for e in extrinsics])).astype(F)


def pixel_points(depth, krows, c2w, max_depth=None):
    """``(ok (k,H,W) bool, pts (k,H,W,3) float32, d (k,H,W) float32)``: d = (float) the map's value; a pixel contributes iff d > 0, d is
    finite and d <= max_depth; its point is p_j = fmaf(d, dir_j, centre_j) with k_camera_rays' direction, statement for statement."""
    depth = np.asarray(depth)
    assert depth.dtype in (np.float32, np.float64) and depth.ndim == 3
    k, h, w = depth.shape
    k6 = np.asarray(krows, dtype=F).reshape(6)
    c2w = np.asarray(c2w, dtype=F)
    rot, lpos = c2w[:, :3, :3], c2w[:, :3, 3]
    with np.errstate(all="ignore"):
        d = depth.astype(F)
        ok = (d > 0) & np.isfinite(d)
        if max_depth is not None:
            ok &= d <= F(max_depth)
        xs = (np.arange(w, dtype=np.int64).astype(F) + F(0.5) - k6[2]) / k6[0]
        ys = (np.arange(h, dtype=np.int64).astype(F) + F(0.5) - k6[5]) / k6[4]
        pts = np.empty((k, h, w, 3), dtype=F)
        for v in range(k):
            for j in range(3):
                dj = fmaf_v(ys[:, None], rot[v, j, 1], (xs * rot[v, j, 0])[None, :]) + rot[v, j, 2]
                pts[v, ..., j] = fmaf_v(d[v], dj, lpos[v, j])
    return ok, pts, d


def voxel_of(pts, nv, p0, vs):
    """``(inside (...,) bool, flat (...,) int64, q (..., 3) int64)`` of float32 points (..., 3): per axis, in float32, t = (x - p0) / vs +
    0.5, i = floor(t), frac = t - i, q = min(int(frac * 256), 255); inside iff every coordinate is finite and every index in range."""
    pts = np.asarray(pts, dtype=F)
    with np.errstate(all="ignore"):
        t = (pts - np.asarray(p0, dtype=F)) / np.asarray(vs, dtype=F) + F(0.5)
        assert t.dtype == F
        i = np.floor(t)
        frac = t - i
        n = np.asarray(nv, dtype=F)
        inside = (np.isfinite(pts) & (i >= 0) & (i < n)).all(-1)
        ii = np.where(inside[..., None], i, 0).astype(np.int64)
        q = np.minimum(np.where(inside[..., None], frac * F(256.0), 0).astype(np.int64), 255)
    flat = (ii[..., 0] * int(nv[1]) + ii[..., 1]) * int(nv[2]) + ii[..., 2]
    return inside, flat, q


def colour_bytes(x):
    """pack_frames' byte of a float32 plane value: x * 255 rounded half up and saturated, NaN -> 0."""
    with np.errstate(all="ignore"):
        v = np.asarray(x, dtype=F) * F(255.0)
        out = np.where(v > F(255.0), F(255.0), v + F(0.5))
        out = np.where(v >= 0, out, F(0.0))
    return out.astype(np.int64)


def accumulate(sums, nv, p0, vs, depth, rgb, krows, c2w, max_depth=None):
    """``sums`` (N, 7) int64 -- n, qx, qy, qz, b, g, r per fine voxel -- plus a chunk: ``depth`` (k,H,W) float32 / float64, ``rgb``
    (k,3,H,W) float32 B, G, R planes.  Returns a new array."""
    ok, pts, _ = pixel_points(depth, krows, c2w, max_depth)
    inside, flat, q = voxel_of(pts, nv, p0, vs)
    use = ok & inside
    col = colour_bytes(np.moveaxis(np.asarray(rgb), 1, -1))
    vals = np.concatenate([np.ones(use.shape + (1,), dtype=np.int64), q, col], axis=-1)[use]
    out = np.array(sums, dtype=np.int64, copy=True)
    np.add.at(out, flat[use], vals)
    return out


def zero_sums(nv):
    return np.zeros((int(nv[0]) * int(nv[1]) * int(nv[2]), 7), dtype=np.int64)


def emit(sums, nv, p0, vs, min_points=1):
    """``dict(xyz (M,3) float32, bgr (M,3) uint8, count (M,) int32, voxel (M,) int32)`` of the summed records ``sums`` (N, 7) int64: the
    voxels with n >= min_points in ascending flat index."""
    sums = np.asarray(sums, dtype=np.int64)
    voxel = np.nonzero(sums[:, 0] >= int(min_points))[0]
    s = sums[voxel]
    n = s[:, 0]
    idx = np.stack([voxel // (int(nv[1]) * int(nv[2])), (voxel // int(nv[2])) % int(nv[1]), voxel % int(nv[2])], axis=1)
    nd = n.astype(np.float64)[:, None]
    off = (s[:, 1:4].astype(np.float64) + 0.5 * nd) / (256.0 * nd)
    cell = idx.astype(np.float64) - 0.5 + off
    xyz = (np.asarray(p0, dtype=F).astype(np.float64) + np.asarray(vs, dtype=F).astype(np.float64) * cell).astype(F)
    bgr = ((2 * s[:, 4:7] + n[:, None]) // (2 * n[:, None])).astype(np.uint8)
    return dict(xyz=xyz, bgr=bgr, count=np.minimum(n, 2 ** 31 - 1).astype(np.int32), voxel=voxel.astype(np.int32))


def label_points(xyz, box_frames):
    """(M,) int16: the highest index among the ``box_frames`` rows (centre, half extents, cos yaw, sin yaw) that hold the point, -1 for
    none: k_label_frames' test."""
    pts = np.asarray(xyz, dtype=F)
    bf = np.asarray(box_frames, dtype=F).reshape(-1, 8)
    best = np.full(pts.shape[0], -1, dtype=np.int64)
    for i in range(bf.shape[0]):
        cx, cy, cz, hx, hy, hz, cos, sin = bf[i]
        dx, dy, dz = pts[:, 0] - cx, pts[:, 1] - cy, pts[:, 2] - cz
        lx = fmaf_v(dx, cos, -(dy * sin))
        ly = fmaf_v(dx, sin, dy * cos)
        best = np.where((np.abs(lx) <= hx) & (np.abs(ly) <= hy) & (np.abs(dz) <= hz), i, best)
    return best.astype(np.int16)


def stack_sums(d):
    """ops.cloud_sums' dict of (X,Y,Z) tensors -> (N, 7) int64."""
    return np.stack([d[f].cpu().numpy().reshape(-1) for f in FIELDS], axis=1)


# ---- shared inputs: the standard small case ----
NV = (8, 8, 4)                      # the detection lattice: 16 x 16 x 8 at refine 2
VS = (0.25, 0.25, 0.25)
ORIGIN = (0.5, -0.25, 0.125)
HW = (24, 40)                       # 960 pixels a view: waves straddle rows; a view is 15 whole waves
ODD_HW = (23, 40)                   # 920 pixels a view: waves straddle rows and views, 3 views end in a partial wave
FLOOR_Z = -0.125
BOX = (0.375, -0.5, 0.875, -0.0625, FLOOR_Z, 0.1875)          # x0, y0, x1, y1, z0, z1 of the box that stands on the floor
INTRINSIC = np.array([[30.0, 0.0, 20.0], [0.0, 30.0, 12.0], [0.0, 0.0, 1.0]])


def ring_extrinsics(k, radius=1.7, height=0.95, target=(0.5, -0.25, 0.0), phase=0.4):
    """k world-to-camera 4 x 4 float64 on a ring around ``target``, looking at it from above."""
    out = []
    for v in range(k):
        a = phase + 2 * np.pi * v / k
        eye = np.float64(target) + np.float64([radius * np.cos(a), radius * np.sin(a), height])
        out.append(np.concatenate([_look_at(eye, np.float64(target)), [[0.0, 0.0, 0.0, 1.0]]]))
    return np.stack(out)


def cast_depth(extrinsics, intrinsic, hw, floor_z=FLOOR_Z, box=BOX):
    """(k,H,W) float64 camera depths of the floor plane z = floor_z with an axis-aligned box on it, through the centres of the pixels
    (camera_rays' convention: pixel (x, y) looks through (x + 0.5, y + 0.5)); 0 where a ray hits nothing."""
    h, w = hw
    kk = np.asarray(intrinsic, dtype=np.float64)
    vv, uu = np.mgrid[0:h, 0:w].astype(np.float64)
    cam = np.stack([(uu + 0.5 - kk[0, 2]) / kk[0, 0], (vv + 0.5 - kk[1, 2]) / kk[1, 1], np.ones_like(uu)], axis=-1)
    out = []
    for e in np.asarray(extrinsics, dtype=np.float64):
        rot, eye = e[:3, :3].T, -e[:3, :3].T @ e[:3, 3]
        dirs = cam @ rot.T                                  # world directions with camera z = 1: the ray parameter is the camera depth
        with np.errstate(all="ignore"):
            t = (floor_z - eye[2]) / dirs[..., 2]
            t = np.where(t > 0, t, np.inf)
            if box is not None:
                lo, hi = np.float64([box[0], box[1], box[4]]), np.float64([box[2], box[3], box[5]])
                t0, t1 = (lo - eye) / dirs, (hi - eye) / dirs
                near, far = np.minimum(t0, t1).max(-1), np.maximum(t0, t1).min(-1)
                t = np.where((near <= far) & (near > 0), np.minimum(t, near), t)
        out.append(np.where(np.isfinite(t), t, 0.0))
    return np.stack(out)


def planes(k, hw, seed=0, pad=(0, 0)):
    """(k,3,H+pad,W+pad) float32 B, G, R planes: mostly in [0, 1], with values below 0, above 1, a NaN and exact .5 / 255 steps."""
    rng = np.random.RandomState(40 + seed)
    h, w = hw[0] + pad[0], hw[1] + pad[1]
    p = (rng.rand(k, 3, h, w) * 1.1 - 0.05).astype(F)
    p[:, :, 1, 1::7] = (rng.randint(0, 255, p[:, :, 1, 1::7].shape) + 0.5).astype(F) / F(255.0)
    p[0, 1, 2, 3] = np.nan
    return p


def standard_case(dtype=np.float64, k=3, hw=HW):
    """The standard small case: ``dict(depth (k,H,W) dtype, rgb (k,3,H,W) float32, extrinsics (k,4,4) float64, c2w (k,4,4) float32, krows,
    intrinsic)``: k poses around the floor with the box on it; view 0 holds a patch of holes, a NaN, an Inf and a negative value; the far
    floor of every view leaves the lattice."""
    ext = ring_extrinsics(k)
    depth = cast_depth(ext, INTRINSIC, hw)
    depth[0, 3:6, 5:9] = 0.0
    depth[0, 10, 11] = np.nan
    depth[0, 10, 12] = np.inf
    depth[0, 11, 11:14] = -1.25
    return dict(depth=depth.astype(dtype), rgb=planes(k, hw), extrinsics=ext, c2w=c2w_of_extrinsics(ext), krows=krows_of(INTRINSIC),
                intrinsic=INTRINSIC)


def meta_of(case, hw=HW):
    """An img_meta of a case at the image's own scale (ori_shape == img_shape)."""
    return dict(lidar2img=dict(intrinsic=np.asarray(case["intrinsic"], dtype=np.float32), extrinsic=[e.astype(np.float32) for e in case["extrinsics"]],
                               origin=ORIGIN), ori_shape=(hw[0], hw[1], 3), img_shape=(hw[0], hw[1], 3))


def wall_case(distance, hw, k=1, grazing=False):
    """A camera ``distance`` metres from the wall x = 1.0 of the lattice, looking at it head on -- or, ``grazing``, along it from one end at
    a few degrees; ``dict`` as :func:`standard_case`, constant colour ramps."""
    h, w = hw
    ext = []
    for v in range(k):
        if grazing:
            eye, target = np.float64([0.9, -1.2 + 0.01 * v, 0.125]), np.float64([1.9, 0.5, 0.125])
        else:
            eye, target = np.float64([1.0 - distance, -0.25 + 0.05 * v, 0.125]), np.float64([1.0, -0.25 + 0.05 * v, 0.125])
        ext.append(np.concatenate([_look_at(eye, target), [[0.0, 0.0, 0.0, 1.0]]]))
    ext = np.stack(ext)
    kk = np.array([[float(w), 0.0, w / 2.0], [0.0, float(w), h / 2.0], [0.0, 0.0, 1.0]])
    vv, uu = np.mgrid[0:h, 0:w].astype(np.float64)
    cam = np.stack([(uu + 0.5 - kk[0, 2]) / kk[0, 0], (vv + 0.5 - kk[1, 2]) / kk[1, 1], np.ones_like(uu)], axis=-1)
    depth = []
    for e in ext:
        rot, eye = e[:3, :3].T, -e[:3, :3].T @ e[:3, 3]
        dirs = cam @ rot.T
        with np.errstate(all="ignore"):
            t = (1.0 - eye[0]) / dirs[..., 0]
        depth.append(np.where(np.isfinite(t) & (t > 0), t, 0.0))
    return dict(depth=np.stack(depth), rgb=planes(k, hw, seed=7), extrinsics=ext, c2w=c2w_of_extrinsics(ext), krows=krows_of(kk), intrinsic=kk)


def oblique_case(hw=(16, 16), focal=8.0):
    """A wide view of the bare floor from low above it: at refine 4 neighbouring pixels' points lie more than a voxel apart, so most lanes
    of a wave hold voxels of their own (tests/test_cloud_cpu.py counts them).  ``dict`` as :func:`standard_case`."""
    h, w = hw
    ext = np.stack([np.concatenate([_look_at(np.float64([0.5, -0.3, 0.45]), np.float64([0.6, -0.2, FLOOR_Z])), [[0.0, 0.0, 0.0, 1.0]]])])
    kk = np.array([[focal, 0.0, w / 2.0], [0.0, focal, h / 2.0], [0.0, 0.0, 1.0]])
    return dict(depth=cast_depth(ext, kk, hw, box=None), rgb=planes(1, hw, seed=9), extrinsics=ext, c2w=c2w_of_extrinsics(ext),
                krows=krows_of(kk), intrinsic=kk)


def keys_per_wave(case, nv, p0, vs, max_depth=None):
    """Per wave of 64 consecutive pixels (x fastest, then rows, then views) the number of distinct voxels its contributing pixels fall
    into, and the largest number of pixels one voxel takes."""
    ok, pts, _ = pixel_points(case["depth"], case["krows"], case["c2w"], max_depth)
    inside, flat, _ = voxel_of(pts, nv, p0, vs)
    f = np.where(ok & inside, flat, -1).reshape(-1)
    return [len(set(f[i:i + 64].tolist()) - {-1}) for i in range(0, f.size, 64)], int(np.bincount(f[f >= 0]).max()) if (f >= 0).any() else 0


def boxes7():
    """Three boxes (x, y, z_bottom, dx, dy, dz, yaw): a far one that holds nothing, then two that overlap -- one around the scene's box, a
    yawed one over its corner."""
    return np.array([[2.5, 2.5, 0.0, 0.5, 0.5, 0.5, 0.0],
                     [0.625, -0.28125, -0.15, 0.55, 0.5, 0.4, 0.0],
                     [0.8, -0.1, -0.15, 0.4, 0.3, 0.35, 0.6]], dtype=np.float32)


def to_torch(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)
