"""numpy restatement of the empty-space skipping kernels (csrc/skip_empty_kernels.hip, include/nerfdet_hip.h): the occupancy bit grid
and the ordered cull of sample points against it.  Written from the definitions, not from the kernels."""
import numpy as np


def solid(alpha, count, thr):
    """Voxel n is solid iff ``!(alpha[n] <= thr) || count[n] == 0`` (a NaN alpha is solid)."""
    alpha = np.asarray(alpha, dtype=np.float32).reshape(-1)
    count = np.asarray(count).reshape(-1)
    with np.errstate(invalid="ignore"):
        return ~(alpha <= np.float32(thr)) | (count == 0)


def occupancy_mask(alpha, count, n_voxels, thr, dilate):
    """(nx, ny, nz) bool: any voxel within Chebyshev distance ``dilate``, inside the grid, is solid.  The cube is separable: a running
    OR over shifted copies, axis by axis."""
    nx, ny, nz = (int(v) for v in n_voxels)
    m = solid(alpha, count, thr).reshape(nx, ny, nz)
    for axis in range(3):
        out = m.copy()
        for s in range(1, int(dilate) + 1):
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[axis], hi[axis] = slice(0, m.shape[axis] - s), slice(s, None)
            if m.shape[axis] > s:
                out[tuple(lo)] |= m[tuple(hi)]
                out[tuple(hi)] |= m[tuple(lo)]
        m = out
    return m


def grid_case(n_voxels, seed, thr=0.25):
    """Inputs for a grid test: ``(alpha (N,) float32, count (N,) int64, thr)``.  Random alpha below ``thr`` (not solid), some exactly
    ``thr`` (not solid either), and solid voxels of three kinds in turn -- alpha above thr, NaN alpha, count 0 -- on all eight corners,
    on every face, and at N // 400 random places.  Every placed solid but the random ones has z = 0 or nz - 1, so that with nz >= 7 the
    middle z layers of a small grid stay clear at dilate 2 and no case can come out all set."""
    nx, ny, nz = (int(v) for v in n_voxels)
    n = nx * ny * nz
    rng = np.random.RandomState(seed)
    thr = np.float32(thr)
    alpha = (rng.rand(n).astype(np.float32) * thr * np.float32(0.99)).astype(np.float32)
    count = rng.randint(1, 5, n).astype(np.int64)
    flat = lambda x, y, z: (x * ny + y) * nz + z
    placed = [flat(x, y, z) for x in (0, nx - 1) for y in (0, ny - 1) for z in (0, nz - 1)]
    placed += [flat(0, ny // 2, nz - 1), flat(nx - 1, ny // 2, 0), flat(nx // 2, 0, 0), flat(nx // 2, ny - 1, nz - 1),
               flat(nx // 2, ny // 2, 0), flat(nx // 2, ny // 2, nz - 1)]
    placed += list(rng.choice(n, n // 400, replace=False))
    free = np.setdiff1d(np.arange(n), placed)
    alpha[rng.choice(free, max(len(free) // 16, 1), replace=False)] = thr
    for j, i in enumerate(placed):
        if j % 3 == 0:
            alpha[i] = thr * np.float32(1.5) if j % 2 else np.nextafter(thr, np.float32(1))
        elif j % 3 == 1:
            alpha[i] = np.nan
        else:
            count[i] = 0
    return alpha, count, thr


def pack_bits(mask):
    """Flat bool mask (N,) -> int32 words ((N + 31) // 32,): bit n is bit ``n & 31`` of word ``n >> 5``, spare bits 0."""
    flat = np.asarray(mask, dtype=bool).reshape(-1)
    n = flat.size
    padded = np.zeros(((n + 31) // 32) * 32, dtype=np.uint32)
    padded[:n] = flat
    words = (padded.reshape(-1, 32) << np.arange(32, dtype=np.uint32)).sum(axis=1, dtype=np.uint64).astype(np.uint32)
    return words.view(np.int32)


def occupancy_bits(alpha, count, n_voxels, thr, dilate):
    return pack_bits(occupancy_mask(alpha, count, n_voxels, thr, dilate))


def bit(bits, n):
    w = np.asarray(bits).view(np.uint32)
    return ((w[n >> 5] >> np.uint32(n & 31)) & np.uint32(1)).astype(bool)


def keep_mask(points_f32, bits, n_voxels, p0, vs, outside):
    """(n,) bool over ``points_f32`` (n, 3): per axis in float32 ``q = (x - p0) / vs``, ``i = (int)floorf(q + 0.5f)``; inside iff all three
    i lie in [0, n_axis) and the coordinates are finite; an inside point is kept iff its bit is set, another iff ``outside == 'keep'``."""
    assert outside in ("keep", "cull")
    p = np.asarray(points_f32, dtype=np.float32).reshape(-1, 3)
    p0 = np.asarray(p0, dtype=np.float32)
    vs = np.asarray(vs, dtype=np.float32)
    nv = np.asarray([int(v) for v in n_voxels], dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        q = ((p - p0) / vs).astype(np.float32)
        f = np.floor((q + np.float32(0.5)).astype(np.float32))
        inside = np.isfinite(p).all(axis=1) & (f >= 0).all(axis=1) & (f < nv.astype(np.float32)).all(axis=1)
    i = np.where(inside[:, None], f, 0).astype(np.int64)
    n = (i[:, 0] * nv[1] + i[:, 1]) * nv[2] + i[:, 2]
    return np.where(inside, bit(bits, n), outside == "keep")


def cull(points_f32, bits, n_voxels, p0, vs, outside):
    """``(idx (M,) int32 ascending, pts_kept (M, 3) float32)``."""
    p = np.asarray(points_f32, dtype=np.float32).reshape(-1, 3)
    idx = np.nonzero(keep_mask(p, bits, n_voxels, p0, vs, outside))[0].astype(np.int32)
    return idx, p[idx]
