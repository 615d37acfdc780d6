#!/usr/bin/env python3
"""Generate tests/golden/box_corners.npz from the REAL reference box class.

Run in the build container only (``/root/reference`` does not exist on the GPU box):

    python tests/golden/make_golden_boxes.py

In the style of make_golden.py: ``DepthInstance3DBoxes`` (mmdet3d/core/bbox/structures/depth_box3d.py) and the modules it stands on
(base_box3d.py, utils.py) are imported *from where they lie*, by file path, with ``sys.modules`` stand-ins for what they import at module
level and never touch on the ``corners`` path (the compiled iou3d / rotated-iou extensions, BasePoints, points_in_boxes_batch).

The class stores its boxes in float32 and ``corners`` computes in the stored dtype.  The fixture holds two runs of the reference's own code
on the same float32 boxes: ``corners_f32``, as the class computes them, and ``corners`` -- the same property with the stored tensor widened
to float64 first (``boxes.tensor = boxes.tensor.double()``; ``corners_norm`` and the rotation follow ``dims.dtype``), rounded once to float32:
what ``nerfdet_amd.boxes.box_corners`` promises bit for bit.

Outputs are data only: a dozen boxes and the reference's corners for them.
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
STRUCT = "mmdet3d/core/bbox/structures/"


def _pkg(name):
    m = types.ModuleType(name)
    m.__path__ = []
    sys.modules[name] = m
    return m


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def load_reference():
    for p in ["mmdet3d", "mmdet3d.core", "mmdet3d.core.points", "mmdet3d.core.bbox", "mmdet3d.core.bbox.structures", "mmdet3d.ops",
              "mmdet3d.ops.iou3d", "mmdet3d.ops.rotated_iou", "mmdet3d.ops.rotated_iou.oriented_iou_loss"]:
        _pkg(p)
    sm = sys.modules
    sm["mmdet3d.core.points"].BasePoints = object
    sm["mmdet3d.ops"].points_in_boxes_batch = None
    sm["mmdet3d.ops.iou3d"].iou3d_cuda = None
    sm["mmdet3d.ops.rotated_iou.oriented_iou_loss"].cal_giou_3d = None
    _load("mmdet3d.core.bbox.structures.utils", STRUCT + "utils.py")
    _load("mmdet3d.core.bbox.structures.base_box3d", STRUCT + "base_box3d.py")
    return _load("mmdet3d.core.bbox.structures.depth_box3d", STRUCT + "depth_box3d.py").DepthInstance3DBoxes


def main():
    cls = load_reference()
    rs = np.random.RandomState(12)
    boxes = np.zeros((12, 7), dtype=np.float32)
    boxes[:, :3] = rs.uniform(-3.0, 3.0, (12, 3))
    boxes[:, 3:6] = rs.uniform(0.2, 2.5, (12, 3))
    boxes[6:, 6] = rs.uniform(-np.pi, np.pi, 6)                       # rows 0-5: yaw 0; rows 6-11: yawed
    boxes[0] = [0.5, -1.25, 0.0, 1.0, 2.0, 0.5, 0.0]                  # dyadic: exact in either precision
    boxes[6, 6], boxes[7, 6] = np.float32(np.pi / 2), np.float32(-0.3)
    b = cls(torch.from_numpy(boxes))
    assert b.tensor.dtype == torch.float32 and torch.equal(b.tensor, torch.from_numpy(boxes))
    corners_f32 = b.corners.numpy()
    b.tensor = b.tensor.double()
    wide = b.corners
    assert wide.dtype == torch.float64
    corners = wide.numpy().astype(np.float32)
    assert corners.shape == corners_f32.shape == (12, 8, 3) and np.abs(corners - corners_f32).max() < 1e-5
    path = os.path.join(OUT, "box_corners.npz")
    np.savez_compressed(path, boxes=boxes, corners=corners, corners_f32=corners_f32)
    print(f"box_corners.npz  {os.path.getsize(path)} bytes; float32 run differs from the float64 run in "
          f"{int((corners != corners_f32).sum())} of {corners.size} elements")


if __name__ == "__main__":
    main()
