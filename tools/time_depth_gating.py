#!/usr/bin/env python3
"""Cost of the depth gate (nerfdet.py:404-411) at the cfg2 shapes (50 views 240x320, C = 256, 40x40x16 voxels), float64 depth of a plane
seen by the ring rig: the resize launch, K1 and K2 gated and ungated, and the whole volumetric step (extract_volume) with and without
depth.  Median of --reps event-timed launches after --warmup, one line per figure, then one JSON line.
    python tools/time_depth_gating.py [--reps 50 --warmup 10]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    import nerfdet_amd  # noqa: F401
    from nerfdet_amd import ops
    from nerfdet_amd.radiance_field import VanillaNeRFRadianceField
    from nerfdet_amd.volume import extract_volume, map_features_2d_hip, scene_geometry
    from depth_gate_ref import plane_depth
    from oracle import nerfdet_oracle as O
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    n_v, c, hw, grid, vs = 50, 256, (240, 320), (40, 40, 16), (0.16, 0.16, 0.2)
    meta = O.ring_scene_meta(n_v, hw)
    feats = torch.randn(n_v, c, hw[0] // 4, hw[1] // 4, device=dev).contiguous(memory_format=torch.channels_last)
    rgb = torch.rand(n_v, 3, *hw, device=dev)
    depth = plane_depth(meta, hw, 0.45, noise=0.03, seed=5).to(dev)
    mapping = torch.nn.Sequential(torch.nn.Linear(c, c // 8)).to(dev)
    mlp = VanillaNeRFRadianceField(4, 256, 3, 2 * (c // 8 + 3), 1, 128).to(dev).eval()
    geo = scene_geometry(meta, grid, vs, 4, dev)
    h, w = hw[0] // 4, hw[1] // 4
    res = {}
    with torch.no_grad():
        gate = ops.depth_gate(depth, vs, (h, w), hw)
        mapped = map_features_2d_hip(feats, mapping[0])
        alpha = torch.rand(grid[0] * grid[1] * grid[2], device=dev)
        res["resize_ms"] = timed(lambda: ops.depth_resize(depth, (h, w), hw), args.reps, args.warmup)
        for name, gt in (("ungated", None), ("gated", gate)):
            res[f"k1_{name}_ms"] = timed(lambda: ops.backproject_aggregate(feats, geo["points"], geo["proj"], alpha, True, depth_gate=gt),
                                         args.reps, args.warmup)
            res[f"k2_{name}_ms"] = timed(lambda: ops.density_features(mapped, mapping[0].bias, rgb, geo["points"], geo["proj"], geo["rgb_proj"],
                                                                      depth_gate=gt), args.reps, args.warmup)
        res["step_ungated_ms"] = timed(lambda: extract_volume(feats, rgb, meta, grid, vs, mapping, mlp, geometry=geo), args.reps, args.warmup)
        res["step_gated_ms"] = timed(lambda: extract_volume(feats, rgb, meta, grid, vs, mapping, mlp, geometry=geo, depth=depth), args.reps,
                                     args.warmup)
        _, cnt0 = ops.backproject_aggregate(feats, geo["points"], geo["proj"])
        _, cnt1 = ops.backproject_aggregate(feats, geo["points"], geo["proj"], depth_gate=gate)
        res["pairs_ungated"], res["pairs_gated"] = int(cnt0.sum()), int(cnt1.sum())
    for k, v in res.items():
        print(f"{k:>16}: {v:.4f}" if isinstance(v, float) else f"{k:>16}: {v}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
