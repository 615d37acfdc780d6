#!/usr/bin/env python3
"""What skipping empty space costs and saves at cfg2's shapes: one camera's 239 x 320 frame (76 480 rays x 64 samples, ten passes of 8192
rays) against a bank of 50 views fed in chunks of 5, as tools/time_frames_out.py sets it up.
  plain_ms               SceneStream.render_frames of the frame, no skip_empty
  parent_ms              the same call in ANOTHER checkout's build (--parent DIR: a tree of the parent commit with its library built), served
                         by a second process that holds its own scene; the two take turns, block by block, in one session
  kept_<p>_ms            render_frames(skip_empty=grid) with the threshold at the alpha quantile that keeps about p % of the samples
                         (100: a threshold below every alpha, outside='keep' -- nothing is culled, the whole overhead is paid; the others:
                         dilate 0, outside='cull', the quantile found by bisection on the frame's own kept fraction), with the fraction reached
  overhead_ms            kept_100_ms - plain_ms: the count pass, the cull with its read, the gathers and the scatter, over ten passes
  spans_100_ms           the new kernels' own event-timed spans of one such call, summed per kernel
  break_even             the kept fraction at which a least-squares line through the kept_<p> points meets plain_ms (and parent_ms)
Medians of --reps event-timed calls after --warmup, every compared call taking turns inside one loop.  One line per figure, then one JSON
line.  A record, not a gate: the weights are random, a trained model's scenes will keep other fractions.
    python tools/time_skip_empty.py [--reps 20 --warmup 3 --rounds 4 --parent DIR]
"""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIN = (0, 0, 239, 320)


def chunk_meta(meta, v0, v1):
    m = dict(meta)
    m["lidar2img"] = dict(meta["lidar2img"], extrinsic=list(meta["lidar2img"]["extrinsic"][v0:v1]))
    return m


def setup(root):
    """cfg2's model and a stream holding bench.py's 50 synthetic views, from the tree at ``root``: ``(scene, one camera's extrinsic)``."""
    sys.path.insert(0, root)
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    dev = torch.device("cuda:0")
    w = bench.WORKLOADS["cfg2"]
    det = bench.build_model(w).to(dev).eval()
    batch = bench.to_device(bench.synth_batch(w, 0), dev)
    img, dn, meta = batch["img"], batch["denorm_images"], batch["img_metas"][0]
    with torch.no_grad():
        scene = det.begin_scene(dict(meta), keep_views=True)
        for v0 in range(0, img.shape[1], 5):
            scene.add_views(img[:, v0:v0 + 5], dn[:, v0:v0 + 5], chunk_meta(meta, v0, v0 + 5))
    return scene, meta["lidar2img"]["extrinsic"][7:8]


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def serve(root):
    """The second process: ``go N`` on stdin -> one JSON list of N event-timed plain render_frames calls on stdout; anything else ends it."""
    scene, ext = setup(root)
    call = lambda: scene.render_frames(extrinsic=ext, window=WIN, stride=1)
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    print("ready", flush=True)
    for line in sys.stdin:
        parts = line.split()
        if len(parts) != 2 or parts[0] != "go":
            break
        print(json.dumps([event_ms(call) for _ in range(int(parts[1]))]), flush=True)


def threshold_for(scene, ext, alpha, target):
    """Bisect the alpha quantile (dilate 0, outside='cull') until the frame keeps about ``target`` of its samples: ``(knobs, fraction)``."""
    lo, hi, best = 0.0, 1.0, None
    for _ in range(10):
        q = 0.5 * (lo + hi)
        knobs = dict(threshold=float(torch.quantile(alpha, q)), dilate=0, outside="cull")
        out = scene.render_frames(extrinsic=ext, window=WIN, stride=1, skip_empty=knobs)
        frac = out["n_kept"] / out["n_samples"]
        if best is None or abs(frac - target) < abs(best[1] - target):
            best = (knobs, frac)
        if frac > target:        # a higher threshold leaves fewer voxels solid
            lo = q
        else:
            hi = q
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=4, help="blocks the reps are split into; the parent's process takes its turn after each")
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--serve", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.serve:
        return serve(args.serve)
    child = None
    if args.parent:      # started before this process touches the GPU; it builds its scene while this one builds its own
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--serve", os.path.abspath(args.parent)], stdin=subprocess.PIPE,
                                 stdout=subprocess.PIPE, text=True, cwd=os.path.abspath(args.parent))
    scene, ext = setup(HERE)
    from nerfdet_amd import trace
    if child:
        assert child.stdout.readline().strip() == "ready", "the parent's process did not come up"
    res = dict(views=scene.n_views, frame=list(WIN[2:]), reps=args.reps, warmup=args.warmup, rounds=args.rounds, parent=bool(child))
    try:
        with torch.no_grad():
            alpha = scene._finish()[0]
            res["alpha_min_median_max"] = [float(alpha.min()), float(alpha.median()), float(alpha.max())]
            cases = [("100", dict(threshold=-1.0, dilate=0, outside="keep"))]
            for target in (0.5, 0.25, 0.1):
                knobs, frac = threshold_for(scene, ext, alpha, target)
                cases.append((f"{round(100 * target)}", knobs))
            grids = [(tag, scene.occupancy(**knobs)) for tag, knobs in cases]
            plain = lambda: scene.render_frames(extrinsic=ext, window=WIN, stride=1)
            calls = [("plain", plain)] + [(f"kept_{tag}", (lambda g: lambda: scene.render_frames(extrinsic=ext, window=WIN, stride=1, skip_empty=g))(g))
                                          for tag, g in grids]
            for tag, g in grids:
                out = scene.render_frames(extrinsic=ext, window=WIN, stride=1, skip_empty=g)
                res[f"kept_{tag}_fraction"] = out["n_kept"] / out["n_samples"]
                res[f"kept_{tag}_threshold"] = g.threshold
                res[f"kept_{tag}_bits_set"] = float(sum(bin(v & 0xFFFFFFFF).count("1") for v in g.bits.cpu().tolist()) / alpha.numel())
            want = plain()
            full = scene.render_frames(extrinsic=ext, window=WIN, stride=1, skip_empty=grids[0][1])
            res["kept_100_equals_plain"] = bool(torch.equal(full["rgb"], want["rgb"]) and torch.equal(full["depth"], want["depth"])
                                                and torch.equal(full["mask"], want["mask"]))
            for _ in range(args.warmup):
                for _, fn in calls:
                    fn()
            ts = {name: [] for name, _ in calls}
            parent_ts = []
            per = max(1, args.reps // args.rounds)
            for _ in range(args.rounds):
                for _ in range(per):
                    for name, fn in calls:
                        ts[name].append(event_ms(fn))
                if child:
                    torch.cuda.synchronize()
                    child.stdin.write(f"go {per}\n")
                    child.stdin.flush()
                    parent_ts += json.loads(child.stdout.readline())
            for name, t in ts.items():
                res[f"{name}_ms"] = statistics.median(t)
            if parent_ts:
                res["parent_ms"] = statistics.median(parent_ts)
            res["overhead_ms"] = res["kept_100_ms"] - res["plain_ms"]
            trace.recorder = trace.Recorder(sample=lambda name: name in ("k_ray_count_bank", "k_cull_count", "k_cull_write", "k_ray_stats_bank"))
            try:
                calls[1][1]()
                torch.cuda.synchronize()
                res["spans_100_ms"] = {k: sum(ms for ms, _ in v) for k, v in trace.recorder.span_ms().items()}
            finally:
                trace.recorder = None
            f = np.array([res[f"kept_{tag}_fraction"] for tag, _ in grids])
            t = np.array([res[f"kept_{tag}_ms"] for tag, _ in grids])
            slope, icpt = np.polyfit(f, t, 1)
            res["fit_ms_at_0_and_per_unit_kept"] = [float(icpt), float(slope)]
            res["break_even"] = float((res["plain_ms"] - icpt) / slope)
            if parent_ts:
                res["break_even_parent"] = float((res["parent_ms"] - icpt) / slope)
    finally:
        if child:
            child.stdin.write("quit\n")
            child.stdin.flush()
            child.wait(timeout=60)
    for key, v in res.items():
        print(f"{key:>32}: {v:.4f}" if isinstance(v, float) else f"{key:>32}: {v}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
