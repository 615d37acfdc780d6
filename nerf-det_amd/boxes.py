"""Minimal depth-coordinate 3D box container -- only what the nerfdet path touches
(result wrapper of imvoxel_head_v2.py:544, ``gravity_center`` / ``tensor`` / ``volume`` used by
get_targets :457-470).  Semantics of mmdet3d/core/bbox/structures/base_box3d.py:37-64: stored as
(x, y, z_bottom, dx, dy, dz, yaw); a (N,6) input gets a zero yaw; ``origin`` re-bases the centre."""
from __future__ import annotations

import numpy as np
import torch


class DepthInstance3DBoxes:
    def __init__(self, tensor, box_dim: int = 7, with_yaw: bool = True, origin=(0.5, 0.5, 0)):
        device = tensor.device if isinstance(tensor, torch.Tensor) else torch.device("cpu")
        t = torch.as_tensor(tensor, dtype=torch.float32, device=device)
        if t.numel() == 0:
            t = t.reshape((0, box_dim))
        assert t.dim() == 2 and t.size(-1) == box_dim, t.size()
        if t.shape[-1] == 6:
            t = torch.cat((t, t.new_zeros(t.shape[0], 1)), dim=-1)
            self.box_dim, self.with_yaw = box_dim + 1, False
        else:
            self.box_dim, self.with_yaw = box_dim, with_yaw
        self.tensor = t.clone()
        if tuple(origin) != (0.5, 0.5, 0):
            self.tensor[:, :3] += self.tensor[:, 3:6] * (self.tensor.new_tensor((0.5, 0.5, 0)) - self.tensor.new_tensor(origin))

    @property
    def device(self):
        return self.tensor.device

    @property
    def volume(self):
        return self.tensor[:, 3] * self.tensor[:, 4] * self.tensor[:, 5]

    @property
    def gravity_center(self):
        c = self.tensor[:, :3].clone()
        c[:, 2] = self.tensor[:, 2] + self.tensor[:, 5] * 0.5
        return c

    def to(self, device):
        out = object.__new__(DepthInstance3DBoxes)
        out.tensor, out.box_dim, out.with_yaw = self.tensor.to(device), self.box_dim, self.with_yaw
        return out

    def __len__(self):
        return self.tensor.shape[0]


def bbox3d2result(bboxes, scores, labels):
    """mmdet3d/core/bbox/transforms.py:49-67: results live on the CPU.  From the GPU they travel as ONE device-to-host copy (three
    separate copies are three stream synchronisations at the end of every scene); class ids are exact in fp32."""
    t = bboxes.tensor
    if t.is_cuda and scores.is_cuda and labels.is_cuda and t.dtype == torch.float32 and scores.dtype == torch.float32 and t.dim() == 2:
        k, c = t.shape
        packed = torch.cat([t, scores.reshape(k, 1), labels.reshape(k, 1).to(torch.float32)], dim=1).cpu()
        out = object.__new__(type(bboxes))
        out.tensor, out.box_dim, out.with_yaw = packed[:, :c].contiguous(), bboxes.box_dim, bboxes.with_yaw
        return dict(boxes_3d=out, scores_3d=packed[:, c].contiguous(), labels_3d=packed[:, c + 1].to(torch.int64))
    return dict(boxes_3d=bboxes.to("cpu"), scores_3d=scores.cpu(), labels_3d=labels.cpu())


# DepthInstance3DBoxes.corners' order (mmdet3d/core/bbox/structures/depth_box3d.py:72-78): unit offsets about the origin (0.5, 0.5, 0)
CORNER_OFFSETS = ((0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0), (1, 0, 0), (1, 0, 1), (1, 1, 1), (1, 1, 0))
# the 12 edges as corner pairs: the x = 0 face loop, the x = 1 face loop, the four connectors (csrc/detections_out_kernels.hip)
BOX_EDGES = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7))


def _boxes_f64(tensor) -> np.ndarray:
    """(n, 7) boxes, numpy or a CPU tensor, as float64; ValueError for another shape."""
    t = tensor.detach().numpy() if isinstance(tensor, torch.Tensor) else np.asarray(tensor)
    if t.ndim != 2 or t.shape[1] != 7:
        raise ValueError(f"boxes must be (n, 7) = (x, y, z_bottom, dx, dy, dz, yaw), got {t.shape}")
    return t.astype(np.float64)


def box_corners(tensor) -> np.ndarray:
    """The corners of (n, 7) boxes ``(x, y, z_bottom, dx, dy, dz, yaw)``, numpy or a CPU tensor, as (n, 8, 3) float32: what
    ``DepthInstance3DBoxes.corners`` returns (depth_box3d.py:46-84), in its order, with the yaw sign of ``rotation_3d_in_axis(axis=2)``
    (structures/utils.py:21-61: x' = x cos + y sin, y' = -x sin + y cos) -- computed in float64 and rounded once to float32."""
    t = _boxes_f64(tensor)
    norm = np.asarray(CORNER_OFFSETS, dtype=np.float64) - np.array([0.5, 0.5, 0.0])
    c = t[:, None, 3:6] * norm[None]
    cos, sin = np.cos(t[:, 6])[:, None], np.sin(t[:, 6])[:, None]
    out = np.empty_like(c)
    out[..., 0] = c[..., 0] * cos + c[..., 1] * sin
    out[..., 1] = c[..., 0] * -sin + c[..., 1] * cos
    out[..., 2] = c[..., 2]
    return (out + t[:, None, :3]).astype(np.float32)


def box_frames(tensor) -> np.ndarray:
    """(n, 8) float32 for ndet_label_frames: the gravity centre (3), the half extents (3), cos yaw, sin yaw of (n, 7) boxes -- computed in
    float64 and rounded once.  A point p lies in the box's frame at lx = dx cos - dy sin, ly = dx sin + dy cos, (dx, dy) = p - centre: the
    inverse of :func:`box_corners`' rotation."""
    t = _boxes_f64(tensor)
    out = np.empty((t.shape[0], 8), dtype=np.float64)
    out[:, :2] = t[:, :2]
    out[:, 2] = t[:, 2] + t[:, 5] * 0.5
    out[:, 3:6] = t[:, 3:6] * 0.5
    out[:, 6], out[:, 7] = np.cos(t[:, 6]), np.sin(t[:, 6])
    return out.astype(np.float32)


def drawing_order(scores, score_thr: float = 0.0) -> np.ndarray:
    """The indices of the detections with ``score >= score_thr`` in drawing order, int64: by ascending score, the sort stable -- of equal
    scores the one later in the result comes last.  The best detection gets the highest position and wins every pixel it shares."""
    s = scores.detach().cpu().numpy() if isinstance(scores, torch.Tensor) else np.asarray(scores)
    if s.ndim != 1:
        raise ValueError(f"scores must be (n,), got {s.shape}")
    keep = np.flatnonzero(s >= score_thr)
    return keep[np.argsort(s[keep], kind="stable")].astype(np.int64)
