#!/usr/bin/env python3
"""Cost of taking frames at capture resolution at the cfg2 shapes: 50 uint8 BGR frames of 968 x 1296 -> 239 x 320 in a 240 x 320 pad.
  resize_normalize_ms   ndet_resize_normalize_views on the raw frames (img, denorm; with --u8 also the resized bytes)
  resize_normalize_rotating_ms   the same launch over --rotate copies of the frames in turn, so that its source comes from HBM
  normalize_ms          ndet_normalize_views on frames already resized and padded to 240 x 320 (what the launch above replaces on the device)
  host_chain_ms         datasets Resize(keep_ratio) -> Normalize -> Pad on the same frames in host memory, one frame per task on --threads
                        threads (at most 16), wall clock; host_round_trip_ms adds the copy of the raw frames to the host and of img back
The two launches: median of --reps event-timed launches after --warmup; the host chain: median of --host-reps runs.  One line per figure,
then one JSON line.
    python tools/time_raw_frames.py [--reps 50 --warmup 10 --threads 16 --host-reps 3]
    python tools/time_raw_frames.py --format nv12       # the NV12 ingest instead: fused launch, two-launch chain, BGR launch (nv12_figures)
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


def nv12_figures(args):
    """--format nv12: 50 tight NV12 surfaces of 968 x 1296 -> 239 x 320 in 240 x 320.
      nv12_fused_ms      ndet_resize_normalize_views_nv12 on the surfaces
      nv12_chain_ms      ndet_nv12_to_bgr to capture-size BGR frames, then ndet_resize_normalize_views on those: the two launches the fused
                         one replaces
      bgr_ms             ndet_resize_normalize_views on BGR frames of the same size, for the same session's comparison
    each on one source buffer and (``*_rotating_ms``) over --rotate copies in turn, so that the source comes from HBM."""
    from nerfdet_amd import _lib, pipeline as P
    lib = _lib.load()
    dev = torch.device("cuda:0")
    n, (hs, ws), scale, (h, w) = 50, (968, 1296), (320, 240), (240, 320)
    hr, wr = P.rescale_size((hs, ws), scale)
    rows = hs * 3 // 2
    rng = np.random.RandomState(0)
    surfaces = torch.from_numpy(rng.randint(0, 256, (n, rows, ws)).astype(np.uint8)).to(dev)
    frames = torch.from_numpy(rng.randint(0, 256, (n, hs, ws, 3)).astype(np.uint8)).to(dev)
    bgr = torch.empty((n, hs, ws, 3), dtype=torch.uint8, device=dev)
    img = torch.empty((n, 3, h, w), device=dev)
    dn = torch.empty_like(img)
    u8 = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev) if args.u8 else None
    mean, std = np.asarray(P.IMG_MEAN, np.float64), np.asarray(P.IMG_STD, np.float64)
    mp, sp = mean.ctypes.data_as(c_void_p), std.ctypes.data_as(c_void_p)
    st = c_void_p(_lib.raw_stream(dev))
    ptr = _lib._ptr

    def fused(s):
        _lib.check(lib.ndet_resize_normalize_views_nv12(ptr(s), None, n, hs, ws, ws, hs, rows, hr, wr, h, w, mp, sp, ptr(img), ptr(dn), ptr(u8), st),
                   "resize_normalize_views_nv12")

    def from_bgr(f):
        _lib.check(lib.ndet_resize_normalize_views(ptr(f), None, n, hs, ws, hr, wr, h, w, mp, sp, ptr(img), ptr(dn), ptr(u8), st), "resize_normalize_views")

    def chain(s):
        _lib.check(lib.ndet_nv12_to_bgr(ptr(s), None, n, hs, ws, ws, hs, rows, ptr(bgr), st), "nv12_to_bgr")
        from_bgr(bgr)

    res = dict(format="nv12", frames=n, capture=[hs, ws], resized=[hr, wr], pad=[h, w])
    for name, fn, src in (("nv12_fused", fused, surfaces), ("nv12_chain", chain, surfaces), ("bgr", from_bgr, frames)):
        res[f"{name}_ms"] = timed(lambda: fn(src), args.reps, args.warmup)
        copies = [src] + [src.clone() for _ in range(max(0, args.rotate - 1))]
        turn = [0]

        def rotating():
            turn[0] = (turn[0] + 1) % len(copies)
            fn(copies[turn[0]])

        res[f"{name}_rotating_ms"] = timed(rotating, args.reps, args.warmup)
        del copies
    # the fused launch writes what the chain writes
    fused(surfaces)
    a = (img.clone(), dn.clone())
    chain(surfaces)
    torch.cuda.synchronize()
    res["fused_equals_chain"] = bool(torch.equal(a[0], img) and torch.equal(a[1], dn))
    for k, v in res.items():
        print(f"{k:>24}: {v:.4f}" if isinstance(v, float) else f"{k:>24}: {v}")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--u8", action="store_true", help="also write the resized bytes")
    ap.add_argument("--rotate", type=int, default=4, help="copies of the raw frames the rotating figure walks")
    ap.add_argument("--format", choices=("bgr", "nv12"), default="bgr", help="nv12: the NV12 ingest figures instead (see nv12_figures)")
    args = ap.parse_args()
    if args.format == "nv12":
        return nv12_figures(args)
    threads = max(1, min(16, args.threads))
    from nerfdet_amd import _lib, pipeline as P
    from nerfdet_amd.datasets import Normalize, Pad, Resize
    lib = _lib.load()
    dev = torch.device("cuda:0")
    n, (hs, ws), scale, (h, w) = 50, (968, 1296), (320, 240), (240, 320)
    hr, wr = P.rescale_size((hs, ws), scale)
    raw = torch.from_numpy(np.random.RandomState(0).randint(0, 256, (n, hs, ws, 3)).astype(np.uint8))
    frames = raw.to(dev)
    small = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device=dev)
    ids = torch.arange(n, dtype=torch.int32, device=dev)
    img = torch.empty((n, 3, h, w), device=dev)
    dn = torch.empty_like(img)
    u8 = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev) if args.u8 else None
    mean, std = np.asarray(P.IMG_MEAN, np.float64), np.asarray(P.IMG_STD, np.float64)
    mp, sp = mean.ctypes.data_as(c_void_p), std.ctypes.data_as(c_void_p)
    st = c_void_p(_lib.raw_stream(dev))
    ptr = _lib._ptr

    def resize_normalize():
        _lib.check(lib.ndet_resize_normalize_views(ptr(frames), None, n, hs, ws, hr, wr, h, w, mp, sp, ptr(img), ptr(dn), ptr(u8), st), "resize_normalize_views")

    def normalize():
        _lib.check(lib.ndet_normalize_views(ptr(small), ptr(ids), n, h, w, mp, sp, ptr(img), ptr(dn), st), "normalize_views")

    res = dict(frames=n, capture=[hs, ws], resized=[hr, wr], pad=[h, w], threads=threads)
    res["resize_normalize_ms"] = timed(resize_normalize, args.reps, args.warmup)
    res["normalize_ms"] = timed(normalize, args.reps, args.warmup)
    # the 188 MB of raw frames fit the 256 MiB last-level cache, which repeated launches on one buffer then read from: the same launch
    # walking --rotate copies of the frames (4: 752 MB) finds its source in HBM
    copies = [frames] + [frames.clone() for _ in range(max(0, args.rotate - 1))]
    turn = [0]

    def rotating():
        turn[0] = (turn[0] + 1) % len(copies)
        f = copies[turn[0]]
        _lib.check(lib.ndet_resize_normalize_views(ptr(f), None, n, hs, ws, hr, wr, h, w, mp, sp, ptr(img), ptr(dn), ptr(u8), st), "resize_normalize_views")

    res["resize_normalize_rotating_ms"] = timed(rotating, args.reps, args.warmup)
    del copies
    # bytes the launch must move: the source rows its taps touch (two per output row, whole rows), img + denorm (+ the resized bytes)
    moved = n * (2 * hr * ws * 3 + 2 * 3 * h * w * 4 + (h * w * 3 if args.u8 else 0))
    res["resize_normalize_gb_s"] = moved / res["resize_normalize_ms"] / 1e6
    res["resize_normalize_rotating_gb_s"] = moved / res["resize_normalize_rotating_ms"] / 1e6

    chain = [Resize(img_scale=scale, keep_ratio=True), Normalize(P.IMG_MEAN, P.IMG_STD, to_rgb=True), Pad(size=(h, w))]

    def one(frame):
        r = dict(img=frame)
        for t in chain:
            r = t(r)
        return r["img"]

    def host(frames_np):
        with ThreadPoolExecutor(threads) as pool:
            return np.stack(list(pool.map(one, frames_np)))

    ts, trip = [], []
    for _ in range(args.host_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        on_host = frames.cpu().numpy()
        t1 = time.perf_counter()
        out = host(on_host)
        t2 = time.perf_counter()
        torch.from_numpy(out).to(dev)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        ts.append((t2 - t1) * 1e3)
        trip.append((t3 - t0) * 1e3)
    res["host_chain_ms"], res["host_round_trip_ms"] = statistics.median(ts), statistics.median(trip)
    resize_normalize()
    torch.cuda.synchronize()
    # same resized bytes; datasets.Normalize subtracts and scales with float64 scalars (cv2's way) and rounds once, the kernels keep
    # mmcv's float32 image arithmetic as oracle/pipeline_oracle.py pins it: the last float bit may differ
    res["host_chain_max_abs_diff"] = float((img.cpu().permute(0, 2, 3, 1) - torch.from_numpy(out)).abs().max())
    for k, v in res.items():
        print(f"{k:>24}: {v:.4f}" if isinstance(v, float) else f"{k:>24}: {v}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
