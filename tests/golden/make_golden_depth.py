#!/usr/bin/env python3
"""Golden vectors of the depth-gated backprojection (mmdet3d/models/detectors/nerfdet.py:404-411) from the REAL reference code.
Run in the build container only, like make_golden.py:
    python tests/golden/make_golden_depth.py
Two small scenes, the depth map an analytic plane seen by the ring rig + noise, so that many voxels sit on both sides of both band
edges: s0 float64 depth at img_shape (what the loader produces), s1 float32 depth at a non-integer ratio with missing (zero) pixels.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import make_golden as G  # noqa: E402
from depth_gate_ref import plane_depth  # noqa: E402
from oracle import nerfdet_oracle as O  # noqa: E402


def make_depth_fixture(ref, name, seed, n_v, c, img_hw, depth_hw, depth_dtype, n_voxels, voxel_size, plane_z, noise, missing, mlp_width=32):
    torch.manual_seed(seed)
    np.random.seed(seed)
    h, w = img_hw
    meta = O.ring_scene_meta(n_v, img_hw)
    meta["box_type_3d"] = None
    det = ref.nerfdet.nerfdet(
        backbone=dict(type="backbone"), neck=dict(type="fpn", out_channels=c), neck_3d=dict(type="id"),
        bbox_head=dict(), n_voxels=n_voxels, voxel_size=voxel_size, aabb=None, near_far_range=[0.2, 8.0],
        N_samples=8, N_rand=16, nerf_mode="image", squeeze_scale=4, nerf_density=True)
    det.nerf_mlp = ref.nerf_mlp.VanillaNeRFRadianceField(net_depth=4, net_width=mlp_width, skip_layer=3, feature_dim=c // 4 + 6,
                                                         net_depth_condition=1, net_width_condition=mlp_width // 2)
    with torch.no_grad():
        det.mapping[0].bias.normal_(0, 0.5)
        for p in det.nerf_mlp.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)
    det.eval()
    feats = torch.randn(n_v, c, h // 4, w // 4)
    img = torch.randn(1, n_v, 3, h, w)
    denorm = torch.rand(1, n_v, 3, h, w)
    depth = plane_depth(meta, depth_hw, plane_z, noise, seed, depth_dtype, missing)
    det.backbone.payload = feats
    ray_batch = dict(ray_o=torch.zeros(1, 1, 4, 3), ray_d=torch.ones(1, 1, 4, 3), gt_rgb=torch.zeros(1, 1, 4, 3),
                     gt_depth=[], nerf_sizes=[torch.tensor([[2, 2, 3]])], denorm_images=denorm)
    with torch.no_grad():
        x, valids, _, rgb_preds, _ = det.extract_feat(img, [meta], "test", depth.unsqueeze(0), ray_batch)
        proj = det._compute_projection(meta, 4, None)
        rgb_proj = det._compute_projection(meta, 1, None)
        pts = ref.nerfdet.get_points(torch.tensor(n_voxels), torch.tensor(voxel_size), torch.tensor(meta["lidar2img"]["origin"]))
        vol, valid = ref.nerfdet.backproject(feats, pts, proj, depth, voxel_size)
        rgb_vol, rgb_valid = ref.nerfdet.backproject(denorm[0], pts, rgb_proj, depth, voxel_size)
        _, valid_ungated = ref.nerfdet.backproject(feats, pts, proj, None, voxel_size)
    assert rgb_preds == [None]
    print(f"{name}: {int(valid.sum())} of {int(valid_ungated.sum())} (voxel, view) pairs pass the gate; "
          f"{int((valids[0] > 0).sum())} of {valids[0].numel()} voxels seen")
    arrays = dict(features=feats, denorm_images=denorm[0], depth=depth, n_voxels=np.array(n_voxels),
                  voxel_size=np.array(voxel_size, dtype=np.float64),
                  out_volume=x[0], out_valid=valids[0], projection=proj, rgb_projection=rgb_proj, points=pts,
                  bp_valid=valid, rgb_bp_valid=rgb_valid, bp_volume_v0=vol[0], bp_volume_sum=vol.sum(0), rgb_bp_volume_sum=rgb_vol.sum(0),
                  **G.meta_arrays(meta))
    arrays.update(G.sd_arrays("mapping.", det.mapping))
    arrays.update(G.sd_arrays("nerf_mlp.", det.nerf_mlp))
    G.npz(name, **arrays)


def main():
    ref = G.load_reference()
    make_depth_fixture(ref, "volume_depth_s0", 0, n_v=6, c=16, img_hw=(60, 80), depth_hw=(60, 80), depth_dtype=np.float64,
                       n_voxels=(10, 10, 6), voxel_size=(0.4, 0.4, 0.3), plane_z=0.3, noise=0.05, missing=0.0)
    make_depth_fixture(ref, "volume_depth_s1", 1, n_v=7, c=32, img_hw=(60, 80), depth_hw=(47, 61), depth_dtype=np.float32,
                       n_voxels=(10, 8, 6), voxel_size=(0.4, 0.5, 0.25), plane_z=0.4, noise=0.05, missing=0.1)


if __name__ == "__main__":
    main()
