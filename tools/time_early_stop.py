#!/usr/bin/env python3
"""What stopping rays early costs and saves at cfg2's shapes: one camera's 239 x 320 frame (76 480 rays x 64 samples, ten passes of 8192
rays) against a bank of 50 views fed in chunks of 5, as tools/time_skip_empty.py sets it up.
  plain_ms               SceneStream.render_frames of the frame, no early_stop, no skip_empty
  parent_ms              the same call in ANOTHER checkout's build (--parent DIR: a tree of the parent commit with its library built), served
                         by a second process that holds its own scene; the two take turns, block by block, in one session
  eps0_ms                render_frames(early_stop=dict(eps=0, segment=default)): nothing stops, the whole overhead is paid
  stop_<w>_ms            render_frames(early_stop=dict(eps=1e-3, segment=w)) for w = 8, 16, 32
  skip_ms                render_frames(skip_empty=True) alone
  both_ms                render_frames(skip_empty=True, early_stop=True)
  <row>_fraction         the row's kept fraction, n_kept / n_samples
  reads_per_pass         device-to-host reads a pass of the default early_stop makes (one per front segment that counts)
  spans_ms               the new kernels' own event-timed spans of one early_stop=True call, summed per kernel, beside the sampler's
Medians of --reps event-timed calls after --warmup, every compared call taking turns inside one loop.  One line per figure, then one JSON
line.  A record, not a gate: the weights are random, so rays stop sooner or later than a trained model's would; the kept fractions are
this scene's, and nobody has measured a trained checkpoint.
    python tools/time_early_stop.py [--reps 20 --warmup 3 --rounds 4 --parent DIR]
"""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIN = (0, 0, 239, 320)
NEW = ("k_ray_advance", "k_front_count", "k_front_write")


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
    from nerfdet_amd import streaming, trace
    if child:
        assert child.stdout.readline().strip() == "ready", "the parent's process did not come up"
    default = streaming.EARLY_STOP_DEFAULTS["segment"]
    res = dict(views=scene.n_views, frame=list(WIN[2:]), reps=args.reps, warmup=args.warmup, rounds=args.rounds, parent=bool(child),
               default_segment=default)
    try:
        with torch.no_grad():
            alpha = scene._finish()[0]
            res["alpha_min_median_max"] = [float(alpha.min()), float(alpha.median()), float(alpha.max())]
            frame = lambda **kw: (lambda: scene.render_frames(extrinsic=ext, window=WIN, stride=1, **kw))
            calls = [("plain", frame()), ("eps0", frame(early_stop=dict(eps=0, segment=default)))]
            calls += [(f"stop_{w}", frame(early_stop=dict(eps=1e-3, segment=w))) for w in (8, 16, 32)]
            calls += [("skip", frame(skip_empty=True)), ("both", frame(skip_empty=True, early_stop=True))]
            want = calls[0][1]()
            for name, fn in calls[1:]:
                out = fn()
                res[f"{name}_fraction"] = out["n_kept"] / out["n_samples"]
                if name != "plain":
                    res[f"{name}_max_rgb_diff"] = float((out["rgb"] - want["rgb"]).abs().max())
            full = calls[1][1]()
            res["eps0_equals_plain"] = bool(torch.equal(full["rgb"], want["rgb"]) and torch.equal(full["depth"], want["depth"])
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
            res["overhead_ms"] = res["eps0_ms"] - res["plain_ms"]
            trace.recorder = trace.Recorder(sample=lambda name: name in NEW + ("k_ray_count_bank", "k_ray_stats_bank"))
            try:
                frame(early_stop=True)()
                torch.cuda.synchronize()
                spans = trace.recorder.span_ms()
                res["spans_ms"] = {k: sum(ms for ms, _ in v) for k, v in spans.items()}
                res["span_launches"] = {k: len(v) for k, v in spans.items()}
            finally:
                trace.recorder = None
            passes = -(-WIN[2] * WIN[3] // 8192)
            res["reads_per_pass"] = res["span_launches"].get("k_front_count", 0) / passes
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
