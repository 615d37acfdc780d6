#!/usr/bin/env python3
"""Cost of the depth part of one cfg3-shaped pipeline call: 50 selected + 10 target depth frames of 480 x 640 uint16, margin 10.
  depth_views_ms        ndet_depth_frames, the 50 selected views -> 239 x 320 (the meta's img_shape)
  gt_depths_ms          ndet_depth_frames, the 10 target views -> the margin crop 220 x 300 of the padded 240 x 320
  positive_indices_ms   ndet_positive_indices over the 660 000 rays (its memset node and its one kernel)
  depth_part_ms         the three in a row, as pipeline.MultiViewPipeline queues them, without the 8-byte read of the count
  depth_part_call_ms    MultiViewPipeline._depth: the same with the ids' uploads and the read of the count (wall clock, synchronised)
  host_chain_ms         / 1000, datasets.imresize_linear and flatnonzero on the same frames in host memory, one frame per task on --threads
                        threads (at most 16), wall clock; host_upload_ms adds the copy of depth, gt_depths and depth_rays to the device
The launches: median of --reps event-timed runs after --warmup; the host chain: median of --host-reps runs.  One line per figure, then one
JSON line.  A record, not a gate.
    python tools/time_depth_frames.py [--reps 50 --warmup 10 --threads 16 --host-reps 3]
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-reps", type=int, default=3)
    args = ap.parse_args()
    threads = max(1, min(16, args.threads))
    from nerfdet_amd import _lib, pipeline as P
    from nerfdet_amd.datasets import imresize_linear
    lib = _lib.load()
    dev = torch.device("cuda:0")
    n_v, t, (hd, wd), (hr, wr), (h, w), m = 50, 10, (480, 640), (239, 320), (240, 320), 10
    rs = np.random.RandomState(0)
    raw = rs.randint(400, 6000, (n_v + t, hd, wd)).astype(np.uint16)
    raw[rs.rand(n_v + t, hd // 4, wd // 4).repeat(4, 1).repeat(4, 2) < 0.1] = 0       # a sensor's holes, in 4 x 4 patches
    frames = torch.from_numpy(raw).to(dev)
    ids, tids = list(range(n_v)), list(range(n_v, n_v + t))
    ids_d, tids_d = (torch.tensor(x, dtype=torch.int32, device=dev) for x in (ids, tids))
    depth = torch.empty((n_v, hr, wr), dtype=torch.float64, device=dev)
    gt = torch.empty((t, h - 2 * m, w - 2 * m), dtype=torch.float64, device=dev)
    rays = gt.numel()
    idx = torch.empty(rays, dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    ws = torch.empty(lib.ndet_positive_indices_workspace_bytes(rays), dtype=torch.uint8, device=dev)
    st = c_void_p(_lib.raw_stream(dev))
    ptr = _lib._ptr

    def views():
        _lib.check(lib.ndet_depth_frames(ptr(frames), ptr(ids_d), n_v, hd, wd, hr, wr, 0, ptr(depth), st), "depth_frames")

    def targets():
        _lib.check(lib.ndet_depth_frames(ptr(frames), ptr(tids_d), t, hd, wd, h, w, m, ptr(gt), st), "depth_frames")

    def compaction():
        _lib.check(lib.ndet_positive_indices(ptr(gt), rays, ptr(idx), ptr(count), ptr(ws), st), "positive_indices")

    def part():
        views()
        targets()
        compaction()

    res = dict(views=n_v, targets=t, depth_frame=[hd, wd], img_shape=[hr, wr], pad=[h, w], margin=m, rays=rays, threads=threads)
    res["depth_views_ms"] = timed(views, args.reps, args.warmup)
    res["gt_depths_ms"] = timed(targets, args.reps, args.warmup)
    res["positive_indices_ms"] = timed(compaction, args.reps, args.warmup)
    res["depth_part_ms"] = timed(part, args.reps, args.warmup)
    res["rays_with_depth"] = int(count.item())

    pipe = P.MultiViewPipeline(n_v, margin=m, nerf_target_views=t)
    ts = []
    for i in range(args.warmup + args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pipe._depth(frames, ids, tids, (hr, wr), (h, w))
        torch.cuda.synchronize()
        if i >= args.warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    res["depth_part_call_ms"] = statistics.median(ts)

    def one(job):
        frame, size_hw, margin = job
        hh, ww = size_hw
        return imresize_linear(frame / 1000, (ww, hh))[margin:hh - margin, margin:ww - margin]

    def host(frames_np):
        jobs = [(frames_np[i], (hr, wr), 0) for i in ids] + [(frames_np[i], (h, w), m) for i in tids]
        with ThreadPoolExecutor(threads) as pool:
            maps = list(pool.map(one, jobs))
        d, g = np.stack(maps[:n_v]), np.ascontiguousarray(np.stack(maps[n_v:]))
        return d, g, np.flatnonzero(g.reshape(-1) > 0)

    ts, up = [], []
    for _ in range(args.host_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d, g, k = host(raw)
        t1 = time.perf_counter()
        on_dev = [torch.from_numpy(x).to(dev) for x in (d, g, k)]
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        ts.append((t1 - t0) * 1e3)
        up.append((t2 - t0) * 1e3)
    res["host_chain_ms"], res["host_upload_ms"] = statistics.median(ts), statistics.median(up)
    res["bit_equal_to_host_chain"] = bool(torch.equal(out["depth"][0], on_dev[0]) and torch.equal(out["gt_depths"][0], on_dev[1])
                                          and torch.equal(out["depth_rays"][0], on_dev[2]))
    for key, v in res.items():
        print(f"{key:>24}: {v:.4f}" if isinstance(v, float) else f"{key:>24}: {v}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
