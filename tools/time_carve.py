#!/usr/bin/env python3
"""What carving free space from depth frames costs and saves at cfg2's shapes (50 views 240 x 320, 40 x 40 x 16 voxels of 0.16 / 0.16 /
0.2 m), on tools/time_depth_gating.py's plane scene: a float64 depth map of a plane seen by the ring rig.
  accumulate_r<r>_k<k>_ms    k_carve_accumulate over one chunk of k = 5 / 50 views at refine r = 1, 2, 4, beside floor_us: the bytes the
                             kernel must move (20 B a fine voxel: three floats of the point, the word read and written; 48 B a view;
                             the depth map once) over the HBM rate of MI355X_PEAK_HBM
  bits_s<s>_d<d>_<form>_ms   k_carve_bits at refine 2 over s = 1 / 64 segments, dilate d, in its one-pass and its two-pass form
  add_frames_*_ms            SceneStream.add_frames of 5 capture frames (480 x 640 BGR + uint16 depth frames) into a window of 10 chunks,
                             with carve=None and carve=dict(refine=r); --parent-tree DIR times the same call, without the keyword, in
                             ANOTHER checkout's build (a tree of the parent commit with its library built) and nothing else: run the
                             two commands in turns in one session
  render_<source>_ms         SceneStream.render_frames of one 239 x 320 frame, plain and with skip_empty at source alpha / depth / both
                             (dilate 1, outside='cull'), with n_kept / n_samples of each
Every figure: the median of --reps event-timed calls after --warmup, with the least and the greatest; compared calls take turns inside
one loop.  One line per figure, then one JSON line.  A record, not a gate: the weights are random and the scene is a plane.
    python tools/time_carve.py [--reps 30 --warmup 5 --skip-model] [--parent-tree DIR]
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
WIN = (0, 0, 239, 320)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def turns(calls, reps, warmup):
    """``{name: [median, least, greatest]}`` of the calls, which take turns inside one loop."""
    for _ in range(warmup):
        for _, fn in calls:
            fn()
    ts = {name: [] for name, _ in calls}
    for _ in range(reps):
        for name, fn in calls:
            ts[name].append(event_ms(fn))
    return {name: [statistics.median(t), min(t), max(t)] for name, t in ts.items()}


def chunk_meta(meta, v0, v1):
    m = dict(meta)
    m["lidar2img"] = dict(meta["lidar2img"], extrinsic=list(meta["lidar2img"]["extrinsic"][v0:v1]))
    return m


def kernels(res, args, dev):
    from nerfdet_amd import ops
    from depth_gate_ref import plane_depth
    from oracle import nerfdet_oracle as O
    n_v, hw, grid, vs = 50, (240, 320), (40, 40, 16), (0.16, 0.16, 0.2)
    meta = O.ring_scene_meta(n_v, hw)
    depth = plane_depth(meta, hw, 0.45, noise=0.03, seed=5).to(dev)
    gate = ops.depth_gate(depth, vs, (hw[0] // 4, hw[1] // 4), hw)
    proj = ops.compute_projection(meta, 1, dev)
    segments = {}
    for r in ops.CARVE_REFINES:
        fine, fvs = ops.carve_lattice(grid, vs, r)
        pts = ops.get_points(fine, fvs, meta["lidar2img"]["origin"], dev)
        n = pts[0].numel()
        counts = torch.zeros((n,), dtype=torch.int32, device=dev)
        calls = []
        for k in (5, 50):
            g = ops.DepthGate(gate.depth_f[:k], gate.depth_r[:k], gate.band)
            calls.append((f"accumulate_r{r}_k{k}", (lambda g, k: lambda: ops.carve_accumulate(counts, pts, proj[:k], g))(g, k)))
            res[f"accumulate_r{r}_k{k}_floor_us"] = (20 * n + 48 * k + 8 * k * hw[0] * hw[1]) / MI355X_PEAK_HBM * 1e6
        for name, t in turns(calls, args.reps, args.warmup).items():
            res[name + "_ms"] = t
        res[f"segment_r{r}_bytes"] = 4 * n
        if r == 2:
            counts.zero_()
            for v0 in range(0, n_v, 5):         # ten chunks of five views: the segments of a window
                seg = torch.zeros_like(counts)
                ops.carve_accumulate(seg, pts, proj[v0:v0 + 5], ops.DepthGate(gate.depth_f[v0:v0 + 5], gate.depth_r[v0:v0 + 5], gate.band))
                segments[v0] = seg
            fine2 = fine
    segs = list(segments.values())
    many = [segs[i % len(segs)] for i in range(64)]
    calls = []
    for s, which in ((1, segs[:1]), (64, many)):
        for d in (0, 1, 2):
            for form, two in (("one", False), ("two", True)):
                if d == 0 and two:
                    continue
                calls.append((f"bits_s{s}_d{d}_{form}", (lambda w, d, two: lambda: ops.carve_bits(w, fine2, 2, d, two_pass=two))(which, d, two)))
        res[f"bits_s{s}_floor_us"] = (4 * s + 0.125) * segs[0].numel() / MI355X_PEAK_HBM * 1e6
    for name, t in turns(calls, args.reps, args.warmup).items():
        res[name + "_ms"] = t
    bits = ops.carve_bits(segs, fine2, 2, 1)
    res["bits_set_r2_window_d1"] = float(sum(bin(v & 0xFFFFFFFF).count("1") for v in bits.cpu().tolist()) / segs[0].numel())


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
        for tag, carve in ((("parent", None),) if parent else (("plain", None), ("r1", dict(refine=1)), ("r2", dict(refine=2)), ("r4", dict(refine=4)))):
            sc = det.begin_scene(dict(meta), window=10, keep_views=True, **({} if parent else dict(carve=carve)))
            for v0 in range(0, n_v, 5):
                sc.add_frames(frames[:, v0:v0 + 5], chunk_meta(meta, v0, v0 + 5), depth_frames=depth_frames[:, v0:v0 + 5])
            scenes[tag] = sc
        # every call feeds the same five frames again: the window slides, the states and stores are reused
        calls = [(f"add_frames_{tag}", (lambda sc: lambda: sc.add_frames(frames[:, :5], chunk_meta(meta, 0, 5), depth_frames=depth_frames[:, :5]))(sc))
                 for tag, sc in scenes.items()]
        for name, t in turns(calls, args.reps, args.warmup).items():
            res[name + "_ms"] = t
        if parent:
            return
        sc = det.begin_scene(dict(meta), keep_views=True, carve=dict(refine=2))
        for v0 in range(0, n_v, 5):
            sc.add_frames(frames[:, v0:v0 + 5], chunk_meta(meta, v0, v0 + 5), depth_frames=depth_frames[:, v0:v0 + 5])
        ext = meta["lidar2img"]["extrinsic"][7:8]
        alpha = sc._finish()[0]
        thr = float(torch.quantile(alpha, 0.5))         # random weights: the median alpha, as tools/time_skip_empty.py's 50 % case
        cases = [("plain", None), ("alpha", dict(threshold=thr, dilate=1, outside="cull")),
                 ("depth", dict(dilate=1, outside="cull", source="depth")),
                 ("both", dict(threshold=thr, dilate=1, outside="cull", source="both"))]
        calls = []
        for tag, knobs in cases:
            fn = (lambda k: lambda: sc.render_frames(extrinsic=ext, window=WIN, stride=1, skip_empty=k))(knobs)
            out = fn()
            if knobs is not None:
                res[f"render_{tag}_kept"] = out["n_kept"] / out["n_samples"]
            calls.append((f"render_{tag}", fn))
        for name, t in turns(calls, max(3, args.reps // 3), 2).items():
            res[name + "_ms"] = t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-model", action="store_true", help="the two kernels only")
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built: time its add_frames only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/time_carve.py measures on the GPU: none found")
    if args.parent_tree:
        sys.path.insert(0, os.path.abspath(args.parent_tree))
    import nerfdet_amd  # noqa: F401
    dev = torch.device("cuda:0")
    res = dict(reps=args.reps, warmup=args.warmup)
    with torch.no_grad():
        if args.parent_tree:
            assert os.path.abspath(nerfdet_amd.__file__).startswith(os.path.abspath(args.parent_tree)), nerfdet_amd.__file__
            model(res, args, dev, os.path.abspath(args.parent_tree), parent=True)
        else:
            kernels(res, args, dev)
            if not args.skip_model:
                model(res, args, dev)
    for key, v in res.items():
        if isinstance(v, list):
            print(f"{key:>32}: median {v[0]:.4f}  least {v[1]:.4f}  greatest {v[2]:.4f}")
        else:
            print(f"{key:>32}: {v:.4f}" if isinstance(v, float) else f"{key:>32}: {v}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
