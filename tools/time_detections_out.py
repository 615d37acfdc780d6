#!/usr/bin/env python3
"""Cost of putting a detection result into the camera's image, at two sizes: cfg2's render grid (one 239 x 320 frame) and capture size
(four 968 x 1296 frames), 50 boxes about the scene's origin seen from the scene's own cameras.
  project_boxes_<S>_ms     ndet_project_boxes, k poses x 50 boxes
  draw_boxes_t<T>_<S>_ms   ndet_draw_boxes over the projected edges, thickness 1 and 5
  label_frames_<S>_ms      ndet_label_frames, k depth frames x 50 boxes
  draw_detections_<S>_ms   SceneStream.draw_detections, event-timed: the host's corner maths, one upload, the two launches
  draw_detections_<S>_call_ms   the same call, wall clock, synchronised before and after
  pack_frames_<S>_ms, frame_errors_<S>_ms   the frames-out launches at the same sizes, for scale
The launches: median of --reps event-timed runs after --warmup.  One line per figure, then one JSON line.  A record, not a gate.
    python tools/time_detections_out.py [--reps 50 --warmup 10]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time
from ctypes import c_float, c_void_p

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def wall(fn, reps, warmup):
    ts = []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from nerfdet_amd import _lib, pipeline as P
    from nerfdet_amd.boxes import DepthInstance3DBoxes, box_corners, box_frames, drawing_order
    from nerfdet_amd.streaming import _scene_intrinsic
    lib, ptr = _lib.load(), _lib._ptr
    dev = torch.device("cuda:0")
    w = bench.WORKLOADS["cfg2"]
    det = bench.build_model(w).to(dev).eval()
    meta = bench.synth_batch(w, 0)["img_metas"][0]
    n_boxes = 50
    rs = np.random.RandomState(0)
    boxes = np.zeros((n_boxes, 7), dtype=np.float32)
    boxes[:, :3] = np.asarray(meta["lidar2img"]["origin"], dtype=np.float32) + rs.uniform(-2.0, 2.0, (n_boxes, 3)) * np.float32([1, 1, 0.4])
    boxes[:, 3:6] = rs.uniform(0.3, 1.5, (n_boxes, 3))
    boxes[:, 6] = rs.uniform(-np.pi, np.pi, n_boxes)
    result = dict(boxes_3d=DepthInstance3DBoxes(torch.from_numpy(boxes)), scores_3d=torch.from_numpy(rs.rand(n_boxes).astype(np.float32)),
                  labels_3d=torch.from_numpy(rs.randint(0, 18, n_boxes)))
    kept = drawing_order(result["scores_3d"])
    corners, frames8 = box_corners(boxes[kept]), box_frames(boxes[kept])
    colours = torch.from_numpy(P.class_palette(18)[result["labels_3d"].numpy()[kept]]).to(dev)
    res = dict(boxes=n_boxes, reps=args.reps, warmup=args.warmup)
    st = c_void_p(_lib.raw_stream(dev))
    sizes = (("cfg2", 1, (239, 320), False, dict(meta)), ("capture", 4, (968, 1296), True, dict(meta, ori_shape=(968, 1296, 3))))
    with torch.no_grad():
        for tag, k, (h, wd), capture, m in sizes:
            scene = det.begin_scene(m)
            ext = m["lidar2img"]["extrinsic"][7:7 + k]
            intrinsic = np.array(m["lidar2img"]["intrinsic"], dtype=np.float32) if capture else _scene_intrinsic(m)
            w2c = np.stack(ext).astype(np.float32)
            c2w = np.linalg.inv(np.stack(ext).astype(np.float64)).astype(np.float32)
            res[f"frames_{tag}"] = [k, h, wd]
            frames = torch.from_numpy(rs.randint(0, 256, (k, h, wd, 3)).astype(np.uint8)).to(dev)
            depth = torch.from_numpy((rs.randint(400, 6000, (k, h, wd)) * (rs.rand(k, h, wd) > 0.1)).astype(np.uint16)).to(dev)
            proj = P.project_boxes(intrinsic, corners, (0, 0, h, wd), 1, extrinsic=w2c, device=dev)
            res[f"boxes_in_frame_{tag}"] = int((proj["rect"][..., 0] >= 0).sum())
            cam = torch.from_numpy(np.concatenate([intrinsic[:2, :3].reshape(-1), w2c[:, :3, :].reshape(-1), corners.reshape(-1)])).to(dev)
            lab_in = torch.from_numpy(np.concatenate([intrinsic[:2, :3].reshape(-1), c2w[:, :3, :3].reshape(-1), c2w[:, :3, 3].reshape(-1),
                                                      frames8.reshape(-1)])).to(dev)
            edges, mask, rect, zr = (torch.empty_like(proj[key]) for key in ("edges", "edge_mask", "rect", "zrange"))
            out, labels = torch.empty_like(frames), torch.empty((k, h, wd), dtype=torch.int16, device=dev)

            def project():
                _lib.check(lib.ndet_project_boxes(ptr(cam), ptr(cam[6:]), ptr(cam[6 + 12 * k:]), k, n_boxes, 0, 0, 1, h, wd, c_float(0.1), ptr(edges),
                                                  ptr(mask), ptr(rect), ptr(zr), st), "project_boxes")

            def draw(t):
                _lib.check(lib.ndet_draw_boxes(ptr(frames), ptr(edges), ptr(mask), ptr(colours), k, h, wd, n_boxes, t, ptr(out), st), "draw_boxes")

            def label():
                _lib.check(lib.ndet_label_frames(ptr(depth), ptr(lab_in), ptr(lab_in[6:]), ptr(lab_in[6 + 9 * k:]), ptr(lab_in[6 + 12 * k:]), k, h, wd,
                                                 n_boxes, 0, 0, 1, ptr(labels), st), "label_frames")

            res[f"project_boxes_{tag}_ms"] = timed(project, args.reps, args.warmup)
            assert torch.equal(edges, proj["edges"]) and torch.equal(rect, proj["rect"])
            for t in (1, 5):
                res[f"draw_boxes_t{t}_{tag}_ms"] = timed(lambda: draw(t), args.reps, args.warmup)
            res[f"label_frames_{tag}_ms"] = timed(label, args.reps, args.warmup)
            res[f"pixels_drawn_t5_{tag}"] = int((out != frames).any(-1).sum())
            res[f"pixels_labelled_{tag}"] = int((labels >= 0).sum())
            grid = dict(capture=True) if capture else dict(window=(0, 0, h, wd))
            call = lambda: scene.draw_detections(frames, result, extrinsic=ext, thickness=5, **grid)
            assert torch.equal(call()["frames"], out)
            assert torch.equal(scene.label_detections(depth, result, extrinsic=ext, **grid), labels)
            res[f"draw_detections_{tag}_ms"] = timed(call, args.reps, args.warmup)
            res[f"draw_detections_{tag}_call_ms"] = wall(call, args.reps, args.warmup)
            # the frames-out launches at the same sizes, for scale
            rays = k * h * wd
            rgb, dep = torch.rand((rays, 3), device=dev), torch.rand(rays, device=dev) * 6.0
            mk = torch.rand(rays, device=dev) > 0.1
            b8, mm = torch.empty_like(frames), torch.empty_like(depth)
            sums = torch.empty((k, 4), dtype=torch.int64, device=dev)
            res[f"pack_frames_{tag}_ms"] = timed(lambda: _lib.check(lib.ndet_pack_frames(ptr(rgb), ptr(dep), ptr(mk), rays, ptr(b8), ptr(mm), st), "pack"),
                                                 args.reps, args.warmup)
            res[f"frame_errors_{tag}_ms"] = timed(lambda: _lib.check(lib.ndet_frame_errors(ptr(b8), ptr(frames), ptr(mm), ptr(depth), k, h * wd, ptr(sums), st),
                                                                     "errors"), args.reps, args.warmup)
    for key, v in res.items():
        print(f"{key:>32}: {v:.4f}" if isinstance(v, float) else f"{key:>32}: {v}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
