#!/usr/bin/env python3
"""Cost of streaming scene inference (nerf-det_amd/streaming.py) at the cfg2 shapes (bench.py's workload: 50 views 240x320, ResNet-50,
40x40x16 voxels): SceneStream.add_views for chunks of k = 1, 5, 10, 50 views, detect(), and a whole 50-view scene streamed in chunks of 5
against one simple_test on the same views, with the peak of torch.cuda.max_memory_allocated for both.  Medians of --reps event-timed
calls after --warmup, one line per figure, then one JSON line.
    python tools/time_streaming.py [--reps 20 --warmup 3]
With --window 1,4,8 it times sliding windows instead: for every S a window of S full chunks of 5 views -- detect() and the two ring
finishes (ops.density_finish_ring / volume_finish_ring, with their achieved bytes/s next to the live copy ceiling of bench.py) -- next to
detect() of an unwindowed stream holding the same views, the calls alternating inside one loop; and the peak allocation of filling the
window and detecting once.
    python tools/time_streaming.py --window 1,4,8 [--reps 20 --warmup 3]
With --render it times rendering from a streamed scene (begin_scene(keep_views=True)): the view-bank sampler against the packed sampler on
the scene's 50 views and 8192 x 64 sample points, for the bank held as 1, 10 and 50 segments; the bank sampler at 150 and 300 views against
the generic sampler over a concatenated copy; scene.render of one target view next to rays.render_rays(render_testing=True) over the same
maps; and the bank's bytes per view.  The calls of a comparison alternate inside one loop.
    python tools/time_streaming.py --render [--reps 20 --warmup 3]
Both --render modes end with the hierarchical-sampling table: the target view (scene.render) and the groups' previews (group.render_rays, per
scene and batched) with n_importance = 0 / 64 / 128 fine samples a ray, each against n_importance=0 in the same alternating loop;
--importance-only times nothing else.
With --group 1,4,8,16 it times scene groups (det.begin_scenes): for every S, group.add_views of S x 1 and S x 5 views against S separate
SceneStream.add_views calls of the same chunks, and group.detect() against group.detect(batched=True) and S separate detect() calls (one after the other, and all queued
with defer=True before the first is collected) with every scene holding the workload's 50 views -- the compared calls alternating inside
one loop -- plus the group's state size and the peak allocation of building a group, adding 5 views per scene and detecting once.
    python tools/time_streaming.py --group 1,4,8,16 [--reps 20 --warmup 3]
With --group-window S:W[,S:W...] it times windowed groups (det.begin_scenes(metas, window=W)): for every configuration S scenes with full
windows of W single-view chunks -- group.add_views of S x 1 views against S windowed SceneStream.add_views calls and against the
unwindowed group's; group.detect() against group.detect(batched=True), the S windowed streams' detect(defer=True) calls, all queued before the first is collected, and
against the unwindowed group's; the two grouped ring finishes alone against S calls of each single-scene ring finish -- the compared calls
alternating inside one loop -- plus the finish and sigma-MLP spans of one detect(), the pool's size and the peak allocations of
sliding a window once and detecting.
    python tools/time_streaming.py --group-window 8:4,8:8 [--reps 20 --warmup 3]
With --group S[,S...] --render it times rendering for scene groups (det.begin_scenes(metas, keep_views=True)), every scene holding the
workload's 50 views in chunks of 5: the grouped bank sampler (one launch for S banks) against S single-bank sampler calls at 2048 and 8192
rays x 64 samples per scene, checked torch.equal first; group.render_rays of 2048 rays per scene with batched=False and batched=True
against S SceneStream.render_rays calls; and the banks' bytes per view.  The compared calls alternate inside one loop.
    python tools/time_streaming.py --group 4,8 --render [--reps 20 --warmup 3]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys

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


def timed_alternating(fns, reps, warmup):
    """Medians (and [min, max]) of ``reps`` event-timed calls of every function in ``fns``, the functions taking turns inside one loop."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b))
    return {k: statistics.median(v) for k, v in ts.items()}, {k: [min(v), max(v)] for k, v in ts.items()}


def window_mode(bench, det, img, dn, meta, sizes, reps, warmup, dev):
    from nerfdet_amd import ops
    res = {"hbm_copy_ceiling_gbs": bench.hbm_copy_ceiling(dev)["best"]}
    chunk = 5
    for S in sizes:
        assert 1 <= S and S * chunk <= img.shape[1], f"--window {S}: the workload has {img.shape[1]} views, chunks are of {chunk}"

        def fill(stream):
            for v0 in range(0, S * chunk, chunk):
                stream.add_views(img[:, v0:v0 + chunk], dn[:, v0:v0 + chunk], chunk_meta(meta, v0, v0 + chunk))
            return stream

        def windowed_once():
            return fill(det.begin_scene(dict(meta), window=S)).detect()

        windowed_once()     # the first chunk of a shape allocates the convolutions' cached workspaces: not the window's memory
        res[f"window_S{S}_peak_mb"] = peak_mb(windowed_once)
        win, flat = fill(det.begin_scene(dict(meta), window=S)), fill(det.begin_scene(dict(meta)))
        assert win.n_chunks == S and win.n_views == flat.n_views == S * chunk
        bias = win._lin.bias
        alpha = torch.rand(win._segs[0].n_voxels, device=dev)
        fns = {"detect_ms": win.detect, "unwindowed_detect_ms": flat.detect,
               "density_finish_ring_ms": lambda: ops.density_finish_ring(win._segs, bias),
               "volume_finish_ring_ms": lambda: ops.volume_finish_ring(win._segs, alpha)}
        med, span = timed_alternating(fns, reps, warmup)
        n, c, cm = win._segs[0].n_voxels, win._segs[0].c, win._segs[0].cm
        # bytes the kernels move: every segment's counts, the rows of the voxels a segment sees (the others are skipped), the outputs;
        # "_full" counts every row instead, what ops reports to the trace
        seen1 = sum(int((st.k1_count != 0).sum()) for st in win._segs)
        seen_f = sum(int((st.k2_count[:, 0] != 0).sum()) for st in win._segs)
        seen_r = sum(int((st.k2_count[:, 1] != 0).sum()) for st in win._segs)
        out_d, out_v = n * 2 * (3 + cm) * 4, n * c * 4 + n * 12
        nbytes = {"density_finish_ring": S * n * 8 + seen_f * 3 * cm * 4 + seen_r * 3 * 16 + out_d,
                  "volume_finish_ring": S * n * 4 + seen1 * c * 4 + out_v,
                  "density_finish_ring_full": S * (win._segs[0].k2_sum.numel() + 2 * n) * 4 + out_d,
                  "volume_finish_ring_full": S * (n * c + n) * 4 + out_v}
        res[f"window_S{S}_rows_read_fraction"] = seen1 / (S * n)
        for k in fns:
            res[f"window_S{S}_{k}"] = med[k]
            res[f"window_S{S}_{k}_min_max"] = span[k]
        for k, b in nbytes.items():
            res[f"window_S{S}_{k}_gbs"] = b / (med[k.replace("_full", "") + "_ms"] * 1e-3) / 1e9
        res[f"window_S{S}_state_mb"] = S * sum(t.numel() * t.element_size() for t in (
            win._segs[0].k1_sum, win._segs[0].k1_count, win._segs[0].k2_sum, win._segs[0].k2_count)) / 2 ** 20
    return res


def group_mode(det, img, dn, meta, sizes, reps, warmup, dev):
    import numpy as np
    res = {}
    n_v = img.shape[1]
    for S in sizes:
        # S scenes on the workload's rig: scene i has its own origin (its own points) and starts its chunks at another view
        metas = []
        for i in range(S):
            m = dict(meta)
            m["lidar2img"] = dict(meta["lidar2img"], origin=np.asarray(meta["lidar2img"]["origin"], dtype=np.float32) + np.float32([0.05 * i, -0.03 * i, 0.0]))
            metas.append(m)
        group = det.begin_scenes([dict(m) for m in metas])
        streams = [det.begin_scene(dict(m)) for m in metas]
        for k in (1, 5):
            starts = [(i * k) % (n_v - k + 1) for i in range(S)]
            gimg = torch.cat([img[:, v:v + k] for v in starts]).contiguous()
            gdn = torch.cat([dn[:, v:v + k] for v in starts]).contiguous()
            cmetas = [chunk_meta(m, v, v + k) for m, v in zip(metas, starts)]

            def separate():
                for i, st in enumerate(streams):
                    st.add_views(gimg[i:i + 1], gdn[i:i + 1], cmetas[i])

            fns = {f"group_add_views_{S}x{k}_ms": lambda: group.add_views(gimg, gdn, cmetas), f"separate_add_views_{S}x{k}_ms": separate}
            med, span = timed_alternating(fns, reps, warmup)
            for name in fns:
                res[name], res[name + "_min_max"] = med[name], span[name]
            res[f"add_views_{S}x{k}_separate_over_group"] = med[f"separate_add_views_{S}x{k}_ms"] / med[f"group_add_views_{S}x{k}_ms"]
        group.reset()
        for st in streams:
            st.reset()
        for v0 in range(0, n_v, 5):     # every scene takes the workload's views, 5 per call: S x 5 views share a backbone pass
            group.add_views(img[:, v0:v0 + 5].expand(S, -1, -1, -1, -1).contiguous(), dn[:, v0:v0 + 5].expand(S, -1, -1, -1, -1).contiguous(),
                            [chunk_meta(m, v0, v0 + 5) for m in metas])
            for st, m in zip(streams, metas):
                st.add_views(img[:, v0:v0 + 5], dn[:, v0:v0 + 5], chunk_meta(m, v0, v0 + 5))
        assert group.n_views == [n_v] * S

        def deferred():
            pending = [st.detect(defer=True) for st in streams]
            return [f() for f in pending]

        fns = {f"group_detect_S{S}_ms": group.detect, f"group_detect_batched_S{S}_ms": lambda: group.detect(batched=True),
               f"separate_detect_S{S}_ms": lambda: [st.detect() for st in streams], f"separate_deferred_detect_S{S}_ms": deferred}
        med, span = timed_alternating(fns, reps, warmup)
        for name in fns:
            res[name], res[name + "_min_max"] = med[name], span[name]
        res[f"detect_S{S}_group_over_batched"] = med[f"group_detect_S{S}_ms"] / med[f"group_detect_batched_S{S}_ms"]
        res[f"detect_S{S}_separate_over_group"] = med[f"separate_detect_S{S}_ms"] / med[f"group_detect_S{S}_ms"]
        res[f"detect_S{S}_deferred_over_group"] = med[f"separate_deferred_detect_S{S}_ms"] / med[f"group_detect_S{S}_ms"]
        res[f"group_S{S}_state_mb"] = sum(t.numel() * t.element_size() for st in group.group.states
                                          for t in (st.k1_sum, st.k1_count, st.k2_sum, st.k2_count)) / 2 ** 20
        del group, streams
        gimg, gdn = torch.cat([img[:, :5]] * S).contiguous(), torch.cat([dn[:, :5]] * S).contiguous()

        def once():
            g = det.begin_scenes([dict(m) for m in metas])
            g.add_views(gimg, gdn, [chunk_meta(m, 0, 5) for m in metas])
            return g.detect()

        res[f"group_S{S}_peak_mb"] = peak_mb(once)
        del gimg, gdn
    return res


def group_window_mode(det, img, dn, meta, configs, reps, warmup, dev):
    import numpy as np
    from nerfdet_amd import ops, trace
    res = {}
    n_v = img.shape[1]
    for S, W in configs:
        tag = f"S{S}_W{W}"
        metas = []
        for i in range(S):
            m = dict(meta)
            m["lidar2img"] = dict(meta["lidar2img"], origin=np.asarray(meta["lidar2img"]["origin"], dtype=np.float32) + np.float32([0.05 * i, -0.03 * i, 0.0]))
            metas.append(m)

        def frames(r):
            """Round r's call: one view per scene, scene i on view (r + 3 i) of the workload's rig."""
            starts = [(r + 3 * i) % n_v for i in range(S)]
            return (torch.cat([img[:, v:v + 1] for v in starts]).contiguous(), torch.cat([dn[:, v:v + 1] for v in starts]).contiguous(),
                    [chunk_meta(m, v, v + 1) for m, v in zip(metas, starts)])

        wgroup = det.begin_scenes([dict(m) for m in metas], window=W)
        ugroup = det.begin_scenes([dict(m) for m in metas])
        streams = [det.begin_scene(dict(m), window=W) for m in metas]

        def stream_add(call):
            for i, st in enumerate(streams):
                st.add_views(call[0][i:i + 1], call[1][i:i + 1], call[2][i])

        for r in range(W + 1):        # full windows that have slid once: from here on nothing is allocated
            call = frames(r)
            wgroup.add_views(*call)
            ugroup.add_views(*call)
            stream_add(call)
        assert wgroup.n_chunks == [W] * S and all(st.n_chunks == W for st in streams)
        call = frames(W + 1)
        fns = {"window_group_add_views_ms": lambda: wgroup.add_views(*call), "window_streams_add_views_ms": lambda: stream_add(call),
               "unwindowed_group_add_views_ms": lambda: ugroup.add_views(*call)}
        med, span = timed_alternating(fns, reps, warmup)

        def deferred():
            pending = [st.detect(defer=True) for st in streams]
            return [f() for f in pending]

        bias = wgroup._lin.bias
        alpha = torch.rand(S * wgroup.pool.n_voxels, device=dev)
        a1 = alpha[:wgroup.pool.n_voxels]
        fns2 = {"window_group_detect_ms": wgroup.detect, "window_group_detect_batched_ms": lambda: wgroup.detect(batched=True),
                "window_streams_deferred_detect_ms": deferred, "unwindowed_group_detect_ms": ugroup.detect,
                "density_finish_group_ring_ms": lambda: ops.density_finish_group_ring(wgroup.pool, bias),
                "density_finish_ring_x_S_ms": lambda: [ops.density_finish_ring(st._segs, bias) for st in streams],
                "volume_finish_group_ring_ms": lambda: ops.volume_finish_group_ring(wgroup.pool, alpha),
                "volume_finish_ring_x_S_ms": lambda: [ops.volume_finish_ring(st._segs, a1) for st in streams]}
        med2, span2 = timed_alternating(fns2, reps, warmup)
        med.update(med2)
        span.update(span2)
        for k in med:
            res[f"{tag}_{k}"], res[f"{tag}_{k}_min_max"] = med[k], span[k]
        res[f"{tag}_add_views_streams_over_window_group"] = med["window_streams_add_views_ms"] / med["window_group_add_views_ms"]
        res[f"{tag}_detect_streams_over_window_group"] = med["window_streams_deferred_detect_ms"] / med["window_group_detect_ms"]
        res[f"{tag}_detect_window_group_over_batched"] = med["window_group_detect_ms"] / med["window_group_detect_batched_ms"]
        res[f"{tag}_density_finish_separate_over_group"] = med["density_finish_ring_x_S_ms"] / med["density_finish_group_ring_ms"]
        res[f"{tag}_volume_finish_separate_over_group"] = med["volume_finish_ring_x_S_ms"] / med["volume_finish_group_ring_ms"]
        # the launches of one windowed-group detect(): spans of the finishes and of the sigma-MLP
        prev, trace.recorder = trace.recorder, trace.Recorder()
        try:
            wgroup.detect()
            names = [sp[0] for sp in trace.recorder.spans]
        finally:
            trace.recorder = prev
        res[f"{tag}_detect_spans"] = {n: names.count(n) for n in sorted(set(names)) if "finish" in n or "point_mlp" in n or "sigma" in n}
        pool = wgroup.pool
        res[f"{tag}_pool_states"] = len(pool.states)
        res[f"{tag}_pool_mb"] = sum(t.numel() * t.element_size() for st in pool.states for t in (st.k1_sum, st.k1_count, st.k2_sum, st.k2_count)) / 2 ** 20
        del wgroup, ugroup, streams, pool
        calls = [frames(r) for r in range(W + 1)]

        def slide_group(window):
            g = det.begin_scenes([dict(m) for m in metas], window=window)
            for c in calls:
                g.add_views(*c)
            return g.detect()

        def slide_streams():
            sts = [det.begin_scene(dict(m), window=W) for m in metas]
            for c in calls:
                for i, st in enumerate(sts):
                    st.add_views(c[0][i:i + 1], c[1][i:i + 1], c[2][i])
            pending = [st.detect(defer=True) for st in sts]
            return [f() for f in pending]

        res[f"{tag}_window_group_peak_mb"] = peak_mb(lambda: slide_group(W))
        res[f"{tag}_window_streams_peak_mb"] = peak_mb(slide_streams)
        res[f"{tag}_unwindowed_group_peak_mb"] = peak_mb(lambda: slide_group(None))
        del calls
    return res


N_IMPORTANCE = (0, 64, 128)     # fine samples per ray of the hierarchical-sampling table (0 = the coarse render it is measured against)


def importance_table(res, prefix, call, reps, warmup):
    """``call(k)`` with k fine samples per ray for every k of N_IMPORTANCE, alternating inside one loop; each figure also as a multiple of
    the k = 0 render of the same loop, next to the (2S + k) / S that compositing S + k samples after S would cost at equal cost a sample."""
    fns = {f"n_importance_{k}_ms": (lambda k=k: call(k)) for k in N_IMPORTANCE}
    med, span = timed_alternating(fns, reps, warmup)
    for k in N_IMPORTANCE:
        key = f"n_importance_{k}_ms"
        res[f"{prefix}_{key}"], res[f"{prefix}_{key}_min_max"] = med[key], span[key]
        res[f"{prefix}_n_importance_{k}_over_0"] = med[key] / med["n_importance_0_ms"]
        res[f"{prefix}_n_importance_{k}_samples_ratio"] = (2 * 64 + k) / 64 if k else 1.0


def render_mode(det, img, dn, meta, rb, reps, warmup, dev, importance_only=False):
    from nerfdet_amd import rays, synth
    res = {}
    n_v = img.shape[1]
    # the workload's ray batch is a dummy of 4 rays: one target view of real rays (tools/bench_render_testing.py's, 220 x 300 at cfg2)
    target = synth.batch_to(synth.train_scene(1, tuple(img.shape[-2:]), t_views=1, n_boxes=1, seed=1), dev)
    rb = det._ray_batch({k: v for k, v in target.items() if k not in ("img", "img_metas")})
    scene = det.begin_scene(dict(meta), keep_views=True)
    for v0 in range(0, n_v, 5):
        scene.add_views(img[:, v0:v0 + 5], dn[:, v0:v0 + 5], chunk_meta(meta, v0, v0 + 5))
    bank = scene.bank
    res["bank_bytes_per_view"] = bank.nbytes() / bank.n_views
    res["bank_mb"] = bank.nbytes() / 2 ** 20
    feat = torch.cat([s.feat for s in bank.segments])                      # (n_v, hf, wf, cm)
    rgb4 = torch.cat([s.rgb4 for s in bank.segments])
    rgb = rgb4[..., :3].permute(0, 3, 1, 2).contiguous()
    cams = rays._compute_projection(meta)
    ray_o, ray_d = rb["ray_o"].reshape(-1, 3)[:8192], rb["ray_d"].reshape(-1, 3)[:8192]
    pts, _ = rays.sample_along_camera_ray(ray_o, ray_d, det.near_far_range, 64, det=True)
    if importance_only:
        assert det.N_samples == 64
        fine = scene.render(rb, n_importance=64)
        assert torch.equal(fine["outputs_coarse"]["rgb"], scene.render(rb)["outputs_coarse"]["rgb"]) and bool(torch.isfinite(fine["outputs_fine"]["rgb"]).all())
        importance_table(res, "render_1view", lambda k: scene.render(rb, n_importance=k), max(3, reps // 4), 1)
        res["render_1view_rays"] = int(rb["ray_o"].reshape(-1, 3).shape[0])
        return res

    def regroup(sizes):
        b, v = rays.ViewBank(), 0
        for k in sizes:
            b.append(feat[v:v + k].permute(0, 3, 1, 2), rgb[v:v + k], chunk_meta(meta, v, v + k))
            v += k
        return b

    # 1. the bank sampler against the packed one: same 50 views, same points; 1, 10 and 50 segments
    banks = {1: regroup([n_v]), 10: regroup([n_v // 10] * 10), n_v: regroup([1] * n_v)}
    f_cl = feat.permute(0, 3, 1, 2)
    assert rays.packed_ok(n_v, f_cl.shape[1])
    fns = {"packed_ms": lambda: rays.ray_view_stats(pts, rgb, cams, f_cl)}
    for k, b in banks.items():
        fns[f"bank_{k}seg_ms"] = (lambda b=b: rays.ray_view_stats_bank(pts, b))
    want = fns["packed_ms"]()
    for k in banks:
        got = fns[f"bank_{k}seg_ms"]()
        assert all(torch.equal(a, c) for a, c in zip(got, want)), f"{k} segments: not the packed sampler's bits"
    med, span = timed_alternating(fns, reps, warmup)
    for k in fns:
        res[f"stats_50v_{k}"], res[f"stats_50v_{k}_min_max"] = med[k], span[k]
    for k in banks:
        res[f"stats_50v_bank_{k}seg_over_packed"] = med[f"bank_{k}seg_ms"] / med["packed_ms"]

    # 2. beyond the packed sampler's 128 views: against the generic sampler over one concatenated copy
    hw = (rgb.shape[2], rgb.shape[3])
    for n_big in (150, 300):
        g = torch.Generator().manual_seed(n_big)
        big_meta = synth.ring_scene_meta(n_big, hw)
        big_meta["img_shape"], big_meta["ori_shape"] = meta["img_shape"], meta["ori_shape"]
        big_meta["lidar2img"] = dict(big_meta["lidar2img"], intrinsic=meta["lidar2img"]["intrinsic"])
        bf = torch.randn(n_big, feat.shape[3], feat.shape[1], feat.shape[2], generator=g).to(dev).contiguous(memory_format=torch.channels_last)
        bi = torch.rand(n_big, 3, *hw, generator=g).to(dev)
        big, v = rays.ViewBank(), 0
        while v < n_big:
            k = min(5, n_big - v)
            big.append(bf[v:v + k], bi[v:v + k], chunk_meta(big_meta, v, v + k))
            v += k
        big_cams = rays._compute_projection(big_meta)
        assert not rays.packed_ok(n_big, bf.shape[1])
        fns = {"generic_ms": lambda: rays.ray_view_stats(pts, bi, big_cams, bf), "bank_ms": lambda: rays.ray_view_stats_bank(pts, big)}
        a, b = fns["generic_ms"](), fns["bank_ms"]()
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
        res[f"stats_{n_big}v_max_abs_diff"] = float((a[0] - b[0]).abs().max())
        med, span = timed_alternating(fns, reps, warmup)
        for k in fns:
            res[f"stats_{n_big}v_{k}"], res[f"stats_{n_big}v_{k}_min_max"] = med[k], span[k]
        res[f"stats_{n_big}v_bank_over_generic"] = med["bank_ms"] / med["generic_ms"]
        del big, bf, bi

    # 3. one target view: scene.render against the one-shot render_testing walk over the same maps
    one = rb
    fns = {"scene_render_ms": lambda: scene.render(one),
           "one_shot_render_ms": lambda: rays.render_rays(one, None, None, f_cl, rgb, det.aabb, det.near_far_range, det.N_samples, det.N_rand,
                                                           det.nerf_mlp, meta, None, "image", is_train=False, render_testing=True)}
    a, b = fns["scene_render_ms"](), fns["one_shot_render_ms"]()
    assert torch.equal(a["outputs_coarse"]["rgb"], b["outputs_coarse"]["rgb"])
    med, span = timed_alternating(fns, max(3, reps // 4), 1)
    for k in fns:
        res[f"render_1view_{k}"], res[f"render_1view_{k}_min_max"] = med[k], span[k]
    res["render_1view_rays"] = int(one["ray_o"].reshape(-1, 3).shape[0])
    # 4. hierarchical sampling: the same target view with 0 / 64 / 128 fine samples a ray
    importance_table(res, "render_1view", lambda k: scene.render(one, n_importance=k), max(3, reps // 4), 1)
    return res


def group_render_mode(det, img, dn, meta, sizes, reps, warmup, dev, importance_only=False):
    import numpy as np
    from nerfdet_amd import rays, synth
    res = {}
    n_v = img.shape[1]
    target = synth.batch_to(synth.train_scene(1, tuple(img.shape[-2:]), t_views=1, n_boxes=1, seed=1), dev)
    rb = det._ray_batch({k: v for k, v in target.items() if k not in ("img", "img_metas")})
    all_o, all_d = rb["ray_o"].reshape(-1, 3), rb["ray_d"].reshape(-1, 3)
    for S in sizes:
        metas = []
        for i in range(S):
            m = dict(meta)
            m["lidar2img"] = dict(meta["lidar2img"], origin=np.asarray(meta["lidar2img"]["origin"], dtype=np.float32) + np.float32([0.05 * i, -0.03 * i, 0.0]))
            metas.append(m)
        group = det.begin_scenes([dict(m) for m in metas], keep_views=True)
        streams = [det.begin_scene(dict(m), keep_views=True) for m in metas]
        for v0 in range(0, n_v, 5):
            group.add_views(img[:, v0:v0 + 5].expand(S, -1, -1, -1, -1).contiguous(), dn[:, v0:v0 + 5].expand(S, -1, -1, -1, -1).contiguous(),
                            [chunk_meta(m, v0, v0 + 5) for m in metas])
            for st, m in zip(streams, metas) if not importance_only else ():
                st.add_views(img[:, v0:v0 + 5], dn[:, v0:v0 + 5], chunk_meta(m, v0, v0 + 5))
        banks = group.banks
        assert [b.n_views for b in banks] == [n_v] * S and all(len(b.segments) == n_v // 5 for b in banks)
        res[f"S{S}_bank_bytes_per_view"] = banks[0].nbytes() / banks[0].n_views
        res[f"S{S}_banks_mb"] = sum(b.nbytes() for b in banks) / 2 ** 20
        # 1. the sampler alone: one grouped launch against S single-bank launches, every scene with rays of its own
        for n_rays in (2048, 8192) if not importance_only else ():
            pts = []
            for i in range(S):
                o, d = all_o.roll(-977 * i, 0)[:n_rays], all_d.roll(-977 * i, 0)[:n_rays]
                pts.append(rays.sample_along_camera_ray(o, d, det.near_far_range, 64, det=True)[0])
            fns = {"group_ms": lambda: rays.ray_view_stats_bank_group(pts, banks),
                   "singles_ms": lambda: [rays.ray_view_stats_bank(p, b) for p, b in zip(pts, banks)]}
            for got, want in zip(fns["group_ms"](), fns["singles_ms"]()):
                assert all(torch.equal(a, c) for a, c in zip(got, want)), "the grouped sampler differs from the single-bank sampler"
            med, span = timed_alternating(fns, reps, warmup)
            for k in fns:
                res[f"S{S}_stats_{n_rays}r_{k}"], res[f"S{S}_stats_{n_rays}r_{k}_min_max"] = med[k], span[k]
            res[f"S{S}_stats_{n_rays}r_singles_over_group"] = med["singles_ms"] / med["group_ms"]
            del pts
        # 2. a preview per scene: 2048 rays each
        os_ = [all_o.roll(-977 * i, 0)[:2048].contiguous() for i in range(S)]
        ds_ = [all_d.roll(-977 * i, 0)[:2048].contiguous() for i in range(S)]
        # 3. hierarchical sampling: the same previews with 0 / 64 / 128 fine samples a ray
        for batched in (False, True):
            importance_table(res, f"S{S}_render_rays" + ("_batched" if batched else ""),
                             lambda k: group.render_rays(os_, ds_, batched=batched, n_importance=k), max(5, reps // 2), warmup)
        if importance_only:
            del group, streams, banks
            continue
        fns = {"group_render_rays_ms": lambda: group.render_rays(os_, ds_), "group_render_rays_batched_ms": lambda: group.render_rays(os_, ds_, batched=True),
               "streams_render_rays_ms": lambda: [st.render_rays(o, d) for st, o, d in zip(streams, os_, ds_)]}
        plain, bat = fns["group_render_rays_ms"](), fns["group_render_rays_batched_ms"]()
        for i in range(S):
            alone = group.render_rays(os_[i:i + 1], ds_[i:i + 1], scenes=[i])[0]
            assert all(torch.equal(plain[i][k], alone[k]) for k in ("rgb", "depth", "mask")), "a scene's render depends on its neighbours"
            assert torch.equal(plain[i]["mask"], bat[i]["mask"])
        res[f"S{S}_batched_max_abs_rgb"] = max(float((a["rgb"] - b["rgb"]).abs().max()) for a, b in zip(plain, bat))
        res[f"S{S}_batched_max_abs_depth"] = max(float((a["depth"] - b["depth"]).abs().max()) for a, b in zip(plain, bat))
        med, span = timed_alternating(fns, max(5, reps // 2), warmup)
        for k in fns:
            res[f"S{S}_{k}"], res[f"S{S}_{k}_min_max"] = med[k], span[k]
        res[f"S{S}_render_rays_streams_over_group"] = med["streams_render_rays_ms"] / med["group_render_rays_ms"]
        res[f"S{S}_render_rays_streams_over_batched"] = med["streams_render_rays_ms"] / med["group_render_rays_batched_ms"]
        del group, streams, banks
    return res


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def chunk_meta(meta, v0, v1):
    m = dict(meta)
    m["lidar2img"] = dict(meta["lidar2img"], extrinsic=list(meta["lidar2img"]["extrinsic"][v0:v1]))
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window", type=str, default=None, help="comma-separated window sizes in chunks of 5 views, e.g. 1,4,8")
    ap.add_argument("--render", action="store_true", help="time rendering from a streamed scene (the view-bank sampler)")
    ap.add_argument("--group", type=str, default=None, help="comma-separated scene-group sizes, e.g. 1,4,8,16")
    ap.add_argument("--importance-only", action="store_true", help="with --render: only the n_importance 0 / 64 / 128 table")
    ap.add_argument("--group-window", type=str, default=None, help="comma-separated scenes:window configurations of windowed groups, e.g. 8:4,8:8")
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    dev = torch.device("cuda:0")
    w = bench.WORKLOADS["cfg2"]
    det = bench.build_model(w).to(dev).eval()
    batch = bench.to_device(bench.synth_batch(w, 0), dev)
    img, dn, meta = batch["img"], batch["denorm_images"], batch["img_metas"][0]
    rb = det._ray_batch({k: v for k, v in batch.items() if k not in ("img", "img_metas")})
    n_v = img.shape[1]
    res = {}
    if args.render and args.group:
        with torch.no_grad():
            res = group_render_mode(det, img, dn, meta, [int(v) for v in args.group.split(",")], args.reps, args.warmup, dev, args.importance_only)
        for k, v in res.items():
            print(f"{k:>52}: " + (f"{v:.3e}" if isinstance(v, float) and "max_abs" in k else f"{v:.3f}" if isinstance(v, float) else str(v)))
        print(json.dumps(res))
        return
    if args.render:
        with torch.no_grad():
            res = render_mode(det, img, dn, meta, rb, args.reps, args.warmup, dev, args.importance_only)
        for k, v in res.items():
            print(f"{k:>44}: " + (f"{v:.3f}" if isinstance(v, float) else str(v)))
        print(json.dumps(res))
        return
    if args.group_window:
        configs = [tuple(int(x) for x in c.split(":")) for c in args.group_window.split(",")]
        with torch.no_grad():
            res = group_window_mode(det, img, dn, meta, configs, args.reps, args.warmup, dev)
        for k, v in res.items():
            print(f"{k:>52}: " + (f"{v:.3f}" if isinstance(v, float) else str(v)))
        print(json.dumps(res))
        return
    if args.group:
        with torch.no_grad():
            res = group_mode(det, img, dn, meta, [int(v) for v in args.group.split(",")], args.reps, args.warmup, dev)
        for k, v in res.items():
            print(f"{k:>44}: " + (f"{v:.3f}" if isinstance(v, float) else str(v)))
        print(json.dumps(res))
        return
    if args.window:
        with torch.no_grad():
            res = window_mode(bench, det, img, dn, meta, [int(v) for v in args.window.split(",")], args.reps, args.warmup, dev)
        for k, v in res.items():
            print(f"{k:>44}: " + (f"{v:.3f}" if isinstance(v, float) else str(v)))
        print(json.dumps(res))
        return
    with torch.no_grad():
        s = det.begin_scene(dict(meta))
        for k in (1, 5, 10, 50):
            def add(k=k):
                s.reset()
                s.add_views(img[:, :k], dn[:, :k], chunk_meta(meta, 0, k))
            res[f"add_views_k{k}_ms"] = timed(add, args.reps, args.warmup)
            res[f"add_views_k{k}_ms_per_view"] = res[f"add_views_k{k}_ms"] / k
        s.reset()
        s.add_views(img, dn, chunk_meta(meta, 0, n_v))
        res["detect_ms"] = timed(lambda: s.detect(), args.reps, args.warmup)

        def streamed():
            st = det.begin_scene(dict(meta))
            for v0 in range(0, n_v, 5):
                st.add_views(img[:, v0:v0 + 5], dn[:, v0:v0 + 5], chunk_meta(meta, v0, v0 + 5))
            return st.detect()

        def one_shot():
            return det.simple_test(img, [dict(meta)], ray_batch=rb)

        res["stream_50_in_5s_total_ms"] = timed(streamed, args.reps, args.warmup)
        res["simple_test_50_ms"] = timed(one_shot, args.reps, args.warmup)
        res["stream_50_in_5s_peak_mb"] = peak_mb(streamed)
        res["simple_test_50_peak_mb"] = peak_mb(one_shot)
        st = det.begin_scene(dict(meta))
        res["scene_state_mb"] = sum(t.numel() * t.element_size() for t in (st.state.k1_sum, st.state.k1_count, st.state.k2_sum,
                                                                             st.state.k2_count)) / 2 ** 20
    for k, v in res.items():
        print(f"{k:>28}: {v:.3f}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
