#!/usr/bin/env python3
"""Cost of the output side of a camera server at cfg2's shapes: one camera's 239 x 320 frame against a bank of 50 views (fed in chunks of 5),
at stride 1 (76 480 rays) and stride 4 (a 60 x 80 thumbnail, 4 800 rays).
  camera_rays_s<S>_ms     ndet_camera_rays, one camera
  pack_frames_s<S>_ms     ndet_pack_frames over the render's rgb / depth / mask
  frame_errors_s<S>_ms    ndet_frame_errors, the frame against a held-out one with depth (its memset node and its one kernel)
  render_frames_s<S>_ms   SceneStream.render_frames of one camera, event-timed: the rays, the passes of 8192 rays, the pack
  render_frames_s<S>_call_ms   the same call, wall clock, synchronised before and after
  render_rays_s<S>_ms     SceneStream.render_rays on the same rays made beforehand: what render_frames adds is the difference
  frame_ssim_<n>x<h>x<w>_ms   ndet_frame_ssim on byte frames (its memset node and its one kernel), frame_errors_<n>x<h>x<w>_ms beside it
  ssim_views_10x220x300_ms    rays.ssim_views on 10 float views, compute_ssim_loop_10x220x300_ms rays.compute_ssim looped over them
                              (these rows: medians of 20 runs, the compared calls taking turns in one loop; --ssim-only runs them alone)
The launches: median of --reps event-timed runs after --warmup.  One line per figure, then one JSON line.  A record, not a gate.
    python tools/time_frames_out.py [--reps 50 --warmup 10]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time
from ctypes import c_void_p

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


def timed_in_turns(fns, reps, warmup):
    """The medians of ``reps`` event-timed runs of every call in ``fns``, the calls taking turns inside one loop."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for fn, t in zip(fns, ts):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            t.append(a.elapsed_time(b))
    return [statistics.median(t) for t in ts]


def ssim_rows(bench, dev, res, reps=20, warmup=5):
    """ndet_frame_ssim (its memset node and its one kernel) beside ndet_frame_errors on the same byte frames -- one 239 x 320 frame, 8 of them,
    one 968 x 1296 capture frame -- and rays.ssim_views on 10 float views of 220 x 300 beside rays.compute_ssim looped over them; medians of
    ``reps`` event-timed calls, the compared calls taking turns in one loop, next to the box's live copy ceiling."""
    from nerfdet_amd import _lib, rays
    lib, ptr, st = _lib.load(), _lib._ptr, c_void_p(_lib.raw_stream(dev))
    res["hbm_copy_ceiling_gbs"] = bench.hbm_copy_ceiling(dev)["best"]
    rs = np.random.RandomState(1)
    for n, h, w in ((1, 239, 320), (8, 239, 320), (1, 968, 1296)):
        a = torch.from_numpy(rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)).to(dev)
        b = torch.from_numpy(rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)).to(dev)
        da = torch.from_numpy((rs.randint(400, 6000, (n, h, w)) * (rs.rand(n, h, w) > 0.001)).astype(np.uint16)).to(dev)
        sums, errs = torch.empty((n, 4), dtype=torch.int64, device=dev), torch.empty((n, 4), dtype=torch.int64, device=dev)

        def ssim():
            _lib.check(lib.ndet_frame_ssim(ptr(a), ptr(b), ptr(da), 0, n, h, w, ptr(sums), st), "frame_ssim")

        def errors():
            _lib.check(lib.ndet_frame_errors(ptr(a), ptr(b), ptr(da), None, n, h * w, ptr(errs), st), "frame_errors")

        tag = f"{n}x{h}x{w}"
        t_ssim, t_err = timed_in_turns([ssim, errors], reps, warmup)
        res[f"frame_ssim_{tag}_ms"], res[f"frame_errors_{tag}_ms"] = t_ssim, t_err
        res[f"frame_ssim_{tag}_gbs"] = n * h * w * 8 / (t_ssim * 1e-3) / 1e9       # 3 + 3 + 2 bytes a pixel, halos not counted
        res[f"frame_ssim_{tag}_windows"] = sums[:, 3].tolist()
    pred = torch.from_numpy(rs.rand(10, 220, 300, 3).astype(np.float32)).to(dev)
    target = torch.from_numpy(rs.rand(10, 220, 300, 3).astype(np.float32)).to(dev)
    fused = lambda: rays.ssim_views(pred, target)
    loop = lambda: torch.stack([rays.compute_ssim(pred[v], target[v]) for v in range(10)])
    res["ssim_views_10x220x300_ms"], res["compute_ssim_loop_10x220x300_ms"] = timed_in_turns([fused, loop], reps, warmup)
    res["ssim_views_max_abs_diff"] = float((fused() - loop()).abs().max())


def chunk_meta(meta, v0, v1):
    m = dict(meta)
    m["lidar2img"] = dict(meta["lidar2img"], extrinsic=list(meta["lidar2img"]["extrinsic"][v0:v1]))
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--ssim-only", action="store_true", help="only the frame-SSIM rows (no model is built)")
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from nerfdet_amd import _lib, pipeline as P
    from nerfdet_amd.streaming import _scene_intrinsic
    lib, ptr = _lib.load(), _lib._ptr
    dev = torch.device("cuda:0")
    if args.ssim_only:
        res = {}
        ssim_rows(bench, dev, res)
        for key, v in res.items():
            print(f"{key:>36}: {v:.4f}" if isinstance(v, float) else f"{key:>36}: {v}")
        print(json.dumps(res))
        return
    w = bench.WORKLOADS["cfg2"]
    det = bench.build_model(w).to(dev).eval()
    batch = bench.to_device(bench.synth_batch(w, 0), dev)
    img, dn, meta = batch["img"], batch["denorm_images"], batch["img_metas"][0]
    n_v = img.shape[1]
    res = dict(views=n_v, frame=[239, 320], reps=args.reps, warmup=args.warmup)
    with torch.no_grad():
        scene = det.begin_scene(dict(meta), keep_views=True)
        for v0 in range(0, n_v, 5):
            scene.add_views(img[:, v0:v0 + 5], dn[:, v0:v0 + 5], chunk_meta(meta, v0, v0 + 5))
        ext = meta["lidar2img"]["extrinsic"][7:8]
        c2w = np.linalg.inv(np.stack(ext).astype(np.float64)).astype(np.float32)
        k = _scene_intrinsic(meta)
        st = c_void_p(_lib.raw_stream(dev))
        rs = np.random.RandomState(0)
        for stride, win in ((1, (0, 0, 239, 320)), (4, (2, 2, 60, 80))):
            h, wd = win[2], win[3]
            rays = h * wd
            tag = f"s{stride}"
            res[f"rays_{tag}"] = rays
            out = scene.render_frames(extrinsic=ext, window=win, stride=stride)
            ray_o, ray_d = P.camera_rays(k, c2w, win, stride, device=dev)
            want = scene.render_rays(ray_o.view(-1, 3), ray_d.view(-1, 3))
            assert torch.equal(out["rgb"].view(-1, 3), want["rgb"]) and torch.equal(out["depth"].view(-1), want["depth"])
            res[f"mask_mean_{tag}"] = float(out["mask"].float().mean())
            cam = torch.from_numpy(np.concatenate([k[:2, :3].reshape(-1), c2w[:, :3, :3].reshape(-1), c2w[:, :3, 3].reshape(-1)])).to(dev)
            rgb, depth, mask = out["rgb"].view(-1, 3), out["depth"].view(-1), out["mask"].view(-1)
            frames, mm = torch.empty_like(out["frames"]), torch.empty_like(out["depth_frames"])
            held = torch.from_numpy(rs.randint(0, 256, (1, h, wd, 3)).astype(np.uint8)).to(dev)
            held_mm = torch.from_numpy((rs.randint(400, 6000, (1, h, wd)) * (rs.rand(1, h, wd) > 0.1)).astype(np.uint16)).to(dev)
            sums = torch.empty((1, 4), dtype=torch.int64, device=dev)

            def make_rays():
                _lib.check(lib.ndet_camera_rays(ptr(cam), ptr(cam[6:]), ptr(cam[15:]), 1, win[1], win[0], stride, h, wd, ptr(ray_o), ptr(ray_d), st),
                           "camera_rays")

            def pack():
                _lib.check(lib.ndet_pack_frames(ptr(rgb), ptr(depth), ptr(mask), rays, ptr(frames), ptr(mm), st), "pack_frames")

            def errors():
                _lib.check(lib.ndet_frame_errors(ptr(frames), ptr(held), ptr(mm), ptr(held_mm), 1, rays, ptr(sums), st), "frame_errors")

            res[f"camera_rays_{tag}_ms"] = timed(make_rays, args.reps, args.warmup)
            res[f"pack_frames_{tag}_ms"] = timed(pack, args.reps, args.warmup)
            res[f"frame_errors_{tag}_ms"] = timed(errors, args.reps, args.warmup)
            assert torch.equal(frames, out["frames"]) and torch.equal(mm, out["depth_frames"])
            call = lambda: scene.render_frames(extrinsic=ext, window=win, stride=stride)
            res[f"render_frames_{tag}_ms"] = timed(call, args.reps, args.warmup)
            res[f"render_frames_{tag}_call_ms"] = wall(call, args.reps, args.warmup)
            res[f"render_rays_{tag}_ms"] = timed(lambda: scene.render_rays(ray_o.view(-1, 3), ray_d.view(-1, 3)), args.reps, args.warmup)
            res[f"sums_{tag}"] = sums[0].tolist()
    ssim_rows(bench, dev, res)
    for key, v in res.items():
        print(f"{key:>28}: {v:.4f}" if isinstance(v, float) else f"{key:>28}: {v}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
