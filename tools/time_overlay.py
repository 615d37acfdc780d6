#!/usr/bin/env python3
"""Cost of the depth-tested, labelled overlay against the plain wireframes, at the two sizes of tools/time_detections_out.py: cfg2's render
grid (one 239 x 320 frame) and capture size (four 968 x 1296 frames), the same 50 boxes seen from the scene's own cameras, thickness 5.
  project_boxes_<S>_ms, project_boxes_w_<S>_ms   ndet_project_boxes and ndet_project_boxes_w, k poses x 50 boxes
  draw_boxes_<S>_ms                ndet_draw_boxes over the projected edges
  draw_overlay_plain_<S>_ms        ndet_draw_overlay with both groups null (the same bytes)
  draw_overlay_depth_<S>_ms        with a depth frame: a wall at 3 m with a tenth holes, hidden edges dimmed
  draw_overlay_plates_<S>_ms       with text plates ("<label> <score>", scale 1 at cfg2's size, 2 at capture size)
  draw_overlay_both_<S>_ms         with both
  draw_detections_<S>_ms, draw_detections_both_<S>_ms   SceneStream.draw_detections, event-timed: today's path and depth frames + text
The launches: median of --reps event-timed runs after --warmup.  One line per figure, then one JSON line.  A record, not a gate.
    python tools/time_overlay.py [--reps 50 --warmup 10]
"""
import argparse
import importlib.util
import json
import os
import sys
from ctypes import c_float, c_void_p

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from time_detections_out import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from nerfdet_amd import _lib, pipeline as P
    from nerfdet_amd.boxes import DepthInstance3DBoxes, box_corners, drawing_order
    from nerfdet_amd.streaming import _scene_intrinsic
    lib, ptr = _lib.load(), _lib._ptr
    dev = torch.device("cuda:0")
    w = bench.WORKLOADS["cfg2"]
    det = bench.build_model(w).to(dev).eval()
    meta = bench.synth_batch(w, 0)["img_metas"][0]
    n_boxes = 50
    rs = np.random.RandomState(0)                           # the boxes of tools/time_detections_out.py
    boxes = np.zeros((n_boxes, 7), dtype=np.float32)
    boxes[:, :3] = np.asarray(meta["lidar2img"]["origin"], dtype=np.float32) + rs.uniform(-2.0, 2.0, (n_boxes, 3)) * np.float32([1, 1, 0.4])
    boxes[:, 3:6] = rs.uniform(0.3, 1.5, (n_boxes, 3))
    boxes[:, 6] = rs.uniform(-np.pi, np.pi, n_boxes)
    result = dict(boxes_3d=DepthInstance3DBoxes(torch.from_numpy(boxes)), scores_3d=torch.from_numpy(rs.rand(n_boxes).astype(np.float32)),
                  labels_3d=torch.from_numpy(rs.randint(0, 18, n_boxes)))
    kept = drawing_order(result["scores_3d"])
    corners = box_corners(boxes[kept])
    colours = torch.from_numpy(P.class_palette(18)[result["labels_3d"].numpy()[kept]]).to(dev)
    texts = [f"{int(lab)} {float(s):.2f}" for lab, s in zip(result["labels_3d"].numpy()[kept], result["scores_3d"].numpy()[kept])]
    codes, lens = P.encode_texts(texts)
    text_buf = torch.from_numpy(np.concatenate([lens.view(np.uint8), codes.reshape(-1), P.FONT_5X7.reshape(-1)])).to(dev)
    res = dict(boxes=n_boxes, reps=args.reps, warmup=args.warmup, thickness=5)
    st = c_void_p(_lib.raw_stream(dev))
    sizes = (("cfg2", 1, (239, 320), False, dict(meta), 1), ("capture", 4, (968, 1296), True, dict(meta, ori_shape=(968, 1296, 3)), 2))
    with torch.no_grad():
        for tag, k, (h, wd), capture, m, scale in sizes:
            scene = det.begin_scene(m)
            ext = m["lidar2img"]["extrinsic"][7:7 + k]
            intrinsic = np.array(m["lidar2img"]["intrinsic"], dtype=np.float32) if capture else _scene_intrinsic(m)
            w2c = np.stack(ext).astype(np.float32)
            res[f"frames_{tag}"] = [k, h, wd]
            frames = torch.from_numpy(rs.randint(0, 256, (k, h, wd, 3)).astype(np.uint8)).to(dev)
            depth = torch.from_numpy((np.full((k, h, wd), 3000) * (rs.rand(k, h, wd) > 0.1)).astype(np.uint16)).to(dev)
            proj = P.project_boxes(intrinsic, corners, (0, 0, h, wd), 1, extrinsic=w2c, device=dev, depths=True)
            cam = torch.from_numpy(np.concatenate([intrinsic[:2, :3].reshape(-1), w2c[:, :3, :].reshape(-1), corners.reshape(-1)])).to(dev)
            edges, mask, rect, zr, ew = (torch.empty_like(proj[key]) for key in ("edges", "edge_mask", "rect", "zrange", "edge_w"))
            out = torch.empty_like(frames)
            head = (ptr(cam), ptr(cam[6:]), ptr(cam[6 + 12 * k:]), k, n_boxes, 0, 0, 1, h, wd, c_float(0.1), ptr(edges), ptr(mask), ptr(rect), ptr(zr))
            res[f"project_boxes_{tag}_ms"] = timed(lambda: _lib.check(lib.ndet_project_boxes(*head, st), "project_boxes"), args.reps, args.warmup)
            res[f"project_boxes_w_{tag}_ms"] = timed(lambda: _lib.check(lib.ndet_project_boxes_w(*head, ptr(ew), st), "project_boxes_w"), args.reps, args.warmup)
            assert torch.equal(edges, proj["edges"]) and torch.equal(ew, proj["edge_w"])

            def overlay(with_depth, with_plates):
                d = (ptr(depth), ptr(ew)) if with_depth else (None, None)
                t = (ptr(rect), ptr(text_buf[4 * n_boxes:]), ptr(text_buf), ptr(text_buf[36 * n_boxes:])) if with_plates else (None,) * 4
                _lib.check(lib.ndet_draw_overlay(ptr(frames), ptr(edges), ptr(mask), ptr(colours), *d, c_float(50.0), 1, *t, scale, k, h, wd, n_boxes, 5,
                                                 ptr(out), st), "draw_overlay")

            res[f"draw_boxes_{tag}_ms"] = timed(lambda: _lib.check(lib.ndet_draw_boxes(ptr(frames), ptr(edges), ptr(mask), ptr(colours), k, h, wd, n_boxes, 5,
                                                                                       ptr(out), st), "draw_boxes"), args.reps, args.warmup)
            plain = out.clone()
            for name, flags in (("plain", (False, False)), ("depth", (True, False)), ("plates", (False, True)), ("both", (True, True))):
                res[f"draw_overlay_{name}_{tag}_ms"] = timed(lambda: overlay(*flags), args.reps, args.warmup)
                res[f"pixels_changed_{name}_{tag}"] = int((out != frames).any(-1).sum())
                assert (name == "plain") == bool(torch.equal(out, plain))
            grid = dict(capture=True) if capture else dict(window=(0, 0, h, wd))
            old = lambda: scene.draw_detections(frames, result, extrinsic=ext, thickness=5, **grid)
            new = lambda: scene.draw_detections(frames, result, extrinsic=ext, thickness=5, depth_frames=depth, occluded="dim", text=True, text_scale=scale,
                                                **grid)
            assert torch.equal(old()["frames"], plain) and torch.equal(new()["frames"], out)
            res[f"draw_detections_{tag}_ms"] = timed(old, args.reps, args.warmup)
            res[f"draw_detections_both_{tag}_ms"] = timed(new, args.reps, args.warmup)
    for key, v in res.items():
        print(f"{key:>36}: {v:.4f}" if isinstance(v, float) else f"{key:>36}: {v}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
