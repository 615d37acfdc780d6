"""Test helper: the depth gate of the reference's backproject() (mmdet3d/models/detectors/nerfdet.py:404-411) restated on the CPU, and
analytic RGB-D depth maps for the synthetic camera rig.  The oracle keeps refusing depth; tests that need the gated statement substitute
:func:`gated_backproject` for ``oracle.nerfdet_oracle.backproject``."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle import nerfdet_oracle as O


def resize_depth(depth: torch.Tensor, hw) -> torch.Tensor:
    """nerfdet.py:405: (n_v, Hd, Wd) -> (n_v, h, w), bilinear, align_corners=False, in depth's dtype."""
    return F.interpolate(depth.unsqueeze(1), size=tuple(hw), mode="bilinear").squeeze(1)


def gate_terms(points, projection, h, w, depth, voxel_size):
    """(valid (n_v, N) after the gate, ungated valid, z (n_v, N) float32, D' at each voxel's pixel (n_v, N))."""
    fu, fv, z = O.project_voxels(points, projection)
    x = fu.round().long()
    y = fv.round().long()
    valid = (x >= 0) & (y >= 0) & (x < w) & (y < h) & (z > 0)
    d = resize_depth(depth, (h, w))
    dv = torch.zeros(z.shape, dtype=d.dtype)
    gated = valid.clone()
    for i in range(z.shape[0]):
        m = valid[i]
        dv[i, m] = d[i, y[i, m], x[i, m]]
        # both strict, in PyTorch's promotion of `z > depth - voxel_size[-1]` (float32 z against a float32 / float64 map)
        gated[i, m] = (z[i, m] > d[i, y[i, m], x[i, m]] - voxel_size[-1]) & (z[i, m] < d[i, y[i, m], x[i, m]] + voxel_size[-1])
    return gated, valid, z, dv


def gated_backproject(features, points, projection, depth, voxel_size):
    """backproject(features, points, projection, depth, voxel_size) of nerfdet.py:393-420 with the depth branch."""
    n_v, c, h, w = features.shape
    gx, gy, gz = points.shape[-3:]
    fu, fv, _ = O.project_voxels(points, projection)
    x = fu.round().long()
    y = fv.round().long()
    valid, _, _, _ = gate_terms(points, projection, h, w, depth, voxel_size)
    volume = torch.zeros((n_v, c, gx * gy * gz), dtype=features.dtype)
    for i in range(n_v):
        m = valid[i]
        volume[i, :, m] = features[i, :, y[i, m], x[i, m]]
    return volume.view(n_v, c, gx, gy, gz), valid.view(n_v, 1, gx, gy, gz)


def oracle_extract_volume(monkeypatch, depth, voxel_size, *args, **kwargs):
    """O.extract_volume with the gated backproject substituted (both of its backproject calls)."""
    monkeypatch.setattr(O, "backproject", lambda f, p, pr: gated_backproject(f, p, pr, depth, voxel_size))
    try:
        return O.extract_volume(*args, **kwargs)
    finally:
        monkeypatch.undo()


def plane_depth(meta, hw, plane_z, noise=0.0, seed=0, dtype=np.float64, missing=0.0):
    """Camera-frame depth (metres) of the horizontal plane z = plane_z seen by every camera of ``meta`` at resolution ``hw``, + Gaussian
    noise; 0 where the ray misses the plane (and, with ``missing`` > 0, at that fraction of random pixels: ScanNet's holes)."""
    rs = np.random.RandomState(seed)
    hd, wd = hw
    k = np.asarray(meta["lidar2img"]["intrinsic"], dtype=np.float64)[:3, :3].copy()
    k[:2] *= hd / meta["ori_shape"][0]
    kinv = np.linalg.inv(k)
    u, v = np.meshgrid(np.arange(wd, dtype=np.float64), np.arange(hd, dtype=np.float64))
    rays_c = kinv @ np.stack([u.ravel(), v.ravel(), np.ones(u.size)])          # camera frame, z = 1
    out = []
    for e in meta["lidar2img"]["extrinsic"]:
        e = np.asarray(e, dtype=np.float64)
        r, t = e[:3, :3], e[:3, 3]
        centre = -r.T @ t
        dw = r.T @ rays_c
        with np.errstate(divide="ignore", invalid="ignore"):
            s = (plane_z - centre[2]) / dw[2]                                      # = camera depth, the rays' z being 1
        s = np.where(np.isfinite(s) & (s > 0), s, 0.0)
        d = s + noise * rs.randn(s.size) * (s > 0)
        if missing > 0:
            d[rs.rand(d.size) < missing] = 0.0
        out.append(d.reshape(hd, wd))
    return torch.from_numpy(np.stack(out).astype(dtype))
