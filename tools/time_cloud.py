#!/usr/bin/env python3
"""What the point cloud of a streamed RGB-D scene costs at cfg2's shapes (50 views 240 x 320, 40 x 40 x 16 voxels of 0.16 / 0.16 / 0.2 m),
on tools/time_carve.py's plane scene: a float64 depth map of a plane seen by the ring rig, random colour planes.
  accumulate_r<r>_k<k>_<form>_ms  k_cloud_accumulate over one chunk of k = 5 / 50 views at refine r = 1, 2, 4, merged (a wave sums the lanes
                                  that share a voxel first) and unmerged, through the C entry point on operands that are on the device
                                  already, --inner launches per timed window; beside floor_us: the bytes of the pixel reads,
                                  k H W (map bytes + 12), over the HBM rate of MI355X_PEAK_HBM; keys_r<r>: the distinct voxels a wave's
                                  pixels fall into, mean over the 50 views' waves
  points_r<r>_s<s>_ms             ops.cloud_points (k_cloud_count, the prefix sum, the read of M, k_cloud_write) over s = 1 / 64 segments
  label_points_ms                 pipeline.label_points of the r = 2 cloud against 32 boxes
  add_frames_*_ms                 SceneStream.add_frames of 5 capture frames (480 x 640 BGR + uint16 depth frames) into a window of 10
                                  chunks, with cloud=None and cloud=dict(refine=r); --parent-tree DIR times the same call, without the
                                  keyword, in ANOTHER checkout's build (a tree of the parent commit with its library built) and nothing
                                  else: run the two commands in turns in one session
Every figure: the median of --reps event-timed windows after --warmup, with the least and the greatest; compared calls take turns inside
one loop.  One line per figure, then one JSON line.  A record, not a gate: the weights are random and the scene is a plane.
    python tools/time_cloud.py [--reps 30 --warmup 5 --inner 10 --skip-model | --skip-kernels] [--parent-tree DIR]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MI355X_PEAK_HBM = 8.0e12      # bytes / s


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def turns(calls, reps, warmup, inner=1):
    """``{name: [median, least, greatest]}`` of the calls, which take turns inside one loop; a window holds ``inner`` calls and is
    divided by it."""
    def window(fn):
        for _ in range(inner):
            fn()

    for _ in range(warmup):
        for _, fn in calls:
            window(fn)
    ts = {name: [] for name, _ in calls}
    for _ in range(reps):
        for name, fn in calls:
            ts[name].append(event_ms(lambda: window(fn)) / inner)
    return {name: [statistics.median(t), min(t), max(t)] for name, t in ts.items()}


def chunk_meta(meta, v0, v1):
    m = dict(meta)
    m["lidar2img"] = dict(meta["lidar2img"], extrinsic=list(meta["lidar2img"]["extrinsic"][v0:v1]))
    return m


def kernels(res, args, dev):
    import cloud_ref as C
    from nerfdet_amd import _lib, ops, pipeline
    from nerfdet_amd._lib import _ptr, _stream, check, float3
    from depth_gate_ref import plane_depth
    from oracle import nerfdet_oracle as O
    n_v, hw, grid, vs = 50, (240, 320), (40, 40, 16), (0.16, 0.16, 0.2)
    h, w = hw
    meta = O.ring_scene_meta(n_v, hw)
    depth = plane_depth(meta, hw, 0.45, noise=0.03, seed=5).to(dev)
    rgb = torch.rand((n_v, 3, h, w), generator=torch.Generator().manual_seed(1)).to(dev)
    kk = np.array(meta["lidar2img"]["intrinsic"], dtype=np.float32)
    kk[:2] = kk[:2] / (meta["ori_shape"][0] / meta["img_shape"][0])
    c2w = C.c2w_of_extrinsics(meta["lidar2img"]["extrinsic"])
    buf = torch.from_numpy(np.concatenate([C.krows_of(kk), c2w[:, :3, :3].reshape(-1), c2w[:, :3, 3].reshape(-1)])).to(dev)
    lib = _lib.load()
    clouds = {}
    for r in ops.CARVE_REFINES:
        fine, fvs = ops.carve_lattice(grid, vs, r)
        p0 = [float(v) for v in ops.get_points(fine, fvs, meta["lidar2img"]["origin"], dev)[:, 0, 0, 0].cpu()]
        n = fine[0] * fine[1] * fine[2]
        sums = torch.zeros((n, ops.CLOUD_WORDS), dtype=torch.int32, device=dev)
        calls = []
        for k in (5, 50):
            for form, merge in (("merged", 1), ("unmerged", 0)):
                def launch(k=k, merge=merge):
                    check(lib.ndet_cloud_accumulate(_ptr(depth), 1, h * w, w, _ptr(rgb), 3 * h * w, h * w, w, _ptr(buf), _ptr(buf[6:]),
                                                    _ptr(buf[6 + 9 * n_v:]), k, h, w, float3(p0), float3(fvs), fine[0], fine[1], fine[2], 0.0, merge,
                                                    _ptr(sums), _stream(sums)), "cloud_accumulate")
                calls.append((f"accumulate_r{r}_k{k}_{form}", launch))
            res[f"accumulate_k{k}_floor_us"] = k * h * w * (8 + 12) / MI355X_PEAK_HBM * 1e6
        for name, t in turns(calls, args.reps, args.warmup, args.inner).items():
            res[name + "_ms"] = t
        res[f"segment_r{r}_bytes"] = 4 * ops.CLOUD_WORDS * n
        # the scene's own segments: ten chunks of five views, and what a wave has to merge
        segs = []
        for v0 in range(0, n_v, 5):
            seg = torch.zeros_like(sums)
            ops.cloud_accumulate(seg, fine, p0, fvs, depth[v0:v0 + 5], rgb[v0:v0 + 5], kk, c2w[v0:v0 + 5])
            segs.append(seg)
        both = [torch.zeros_like(sums), torch.zeros_like(sums)]
        for seg, merge in zip(both, (True, False)):
            ops.cloud_accumulate(seg, fine, p0, fvs, depth, rgb, kk, c2w, merge=merge)
        assert torch.equal(both[0], both[1]) and torch.equal(ops.cloud_sums(both[:1], fine)["n"], ops.cloud_sums(segs, fine)["n"])
        tot = ops.cloud_sums(both[:1], fine)["n"]
        res[f"pixels_in_r{r}"] = int(tot.sum()) / (n_v * h * w)
        res[f"voxels_hit_r{r}"] = int((tot > 0).sum())
        keys, _ = C.keys_per_wave(dict(depth=depth[:2].cpu().numpy(), krows=C.krows_of(kk), c2w=c2w[:2]), fine, np.float32(p0), np.float32(fvs))
        res[f"keys_r{r}"] = float(np.mean(keys))
        clouds[r] = (fine, p0, fvs, segs)
    calls = []
    for r in (2, 4):
        fine, p0, fvs, segs = clouds[r]
        many = [segs[i % len(segs)] for i in range(64)]
        for s, which in ((1, segs[:1]), (64, many)):
            calls.append((f"points_r{r}_s{s}", (lambda which, fine, p0, fvs: lambda: ops.cloud_points(which, fine, p0, fvs, 1))(which, fine, p0, fvs)))
            res[f"points_r{r}_s{s}_m"] = int(ops.cloud_points(which, fine, p0, fvs, 1)["xyz"].shape[0])
            res[f"points_r{r}_s{s}_floor_us"] = 2 * 32 * s * segs[0].shape[0] / MI355X_PEAK_HBM * 1e6
    fine, p0, fvs, segs = clouds[2]
    xyz = ops.cloud_points(segs, fine, p0, fvs, 1)["xyz"]
    rs = np.random.RandomState(3)
    boxes = np.concatenate([rs.rand(32, 2) * 6 - 3, np.full((32, 1), 0.2), rs.rand(32, 3) + 0.3, rs.rand(32, 1) * 3], 1).astype(np.float32)
    from nerfdet_amd.boxes import box_frames
    bf = box_frames(boxes)
    calls.append(("label_points", lambda: pipeline.label_points(xyz, bf)))
    res["label_points_m"] = int(xyz.shape[0])
    for name, t in turns(calls, args.reps, args.warmup).items():
        res[name + "_ms"] = t


def model(res, args, dev, root=ROOT, parent=False):
    from nerfdet_amd import pipeline as P
    from depth_gate_ref import plane_depth
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    w = bench.WORKLOADS["cfg2"]
    det = bench.build_model(w).to(dev).eval()
    meta0 = bench.synth_batch(w, 0)["img_metas"][0]
    size = (480, 640)
    meta = P.frame_meta(meta0["lidar2img"], size, (320, 240), (240, 320))
    rs = np.random.RandomState(0)
    n_v = len(meta["lidar2img"]["extrinsic"])
    frames = torch.from_numpy(rs.randint(0, 256, (1, n_v) + size + (3,)).astype(np.uint8)).to(dev)
    metres = plane_depth(meta, size, 0.45, noise=0.03, seed=5).numpy()
    depth_frames = torch.from_numpy(np.clip(np.rint(metres * 1000), 0, 65535).astype(np.uint16)[None]).to(dev)
    scenes = {}
    with torch.no_grad():
        for tag, cloud in ((("parent", None),) if parent else (("plain", None), ("r1", dict(refine=1)), ("r2", dict(refine=2)), ("r4", dict(refine=4)))):
            sc = det.begin_scene(dict(meta), window=10, **({} if parent else dict(cloud=cloud)))
            for v0 in range(0, n_v, 5):
                sc.add_frames(frames[:, v0:v0 + 5], chunk_meta(meta, v0, v0 + 5), depth_frames=depth_frames[:, v0:v0 + 5])
            scenes[tag] = sc
        # every call feeds the same five frames again: the window slides, the states and stores are reused
        calls = [(f"add_frames_{tag}", (lambda sc: lambda: sc.add_frames(frames[:, :5], chunk_meta(meta, 0, 5), depth_frames=depth_frames[:, :5]))(sc))
                 for tag, sc in scenes.items()]
        for name, t in turns(calls, args.reps, args.warmup).items():
            res[name + "_ms"] = t
        if not parent:
            for tag in ("r1", "r2", "r4"):
                res[f"scene_points_{tag}_m"] = int(scenes[tag].points()["xyz"].shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10, help="kernel launches per timed window")
    ap.add_argument("--skip-model", action="store_true", help="the kernels only")
    ap.add_argument("--skip-kernels", action="store_true", help="add_frames only (for taking turns with --parent-tree runs)")
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built: time its add_frames only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/time_cloud.py measures on the GPU: none found")
    if args.parent_tree:
        sys.path.insert(0, os.path.abspath(args.parent_tree))
    import nerfdet_amd  # noqa: F401
    dev = torch.device("cuda:0")
    res = dict(reps=args.reps, warmup=args.warmup, inner=args.inner)
    with torch.no_grad():
        if args.parent_tree:
            assert os.path.abspath(nerfdet_amd.__file__).startswith(os.path.abspath(args.parent_tree)), nerfdet_amd.__file__
            model(res, args, dev, os.path.abspath(args.parent_tree), parent=True)
        else:
            if not args.skip_kernels:
                kernels(res, args, dev)
            if not args.skip_model:
                model(res, args, dev)
    for key, v in res.items():
        if isinstance(v, list):
            print(f"{key:>36}: median {v[0]:.4f}  least {v[1]:.4f}  greatest {v[2]:.4f}")
        else:
            print(f"{key:>36}: {v:.4f}" if isinstance(v, float) else f"{key:>36}: {v}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
