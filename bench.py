#!/usr/bin/env python3
"""Headline benchmark: scenes/s of NeRF-Det inference on BASELINE.json configs[1]
(nerfdet_res50_2x_low_res, 50 views 240x320, 40x40x16 voxels, fp32, 1 scene per step per GPU).

    python bench.py --gpus N --steps K --warmup W          # N > 1: spawns its N ranks itself (one process per GPU)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W             # or under an external launcher (RANK / WORLD_SIZE in the env)

A step is one full ``nerfdet.forward_test`` -- literally ``det(return_loss=False, **batch)`` -- on one synthetic scene:
ResNet-50 + FPN, the hand-written HIP hot path (projection, gather, multi-view aggregation, density MLP gating), the 3D neck +
head, box decoding and HIP NMS, results copied to the host as the reference does.  Nothing is skipped or cached between
steps.  Inputs are resident in HBM when the timed region starts.

One process per GPU.  Scenes are independent units, so N ranks run N scene streams with no data-path collective (weak
scaling); the only collectives are the timing barrier and the max-over-ranks of the elapsed time.  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the K steps and prints the headline (scenes/s, ms_per_step, per-step percentiles).
``--dump-outputs DIR`` writes the detections of the last timed step as DIR/<name>.npy (float32); inputs and weights are seeded, so two
builds given the same arguments can be compared output for output.  ``--full`` adds everything else the benchmark measures:
the per-kernel event spans and stage times of the timed steps, the HBM copy ceiling, the rooflines, the two-scenes-in-flight loop, the
interleaved bf16x3 comparison, the CPU baseline and the training-step probe.
Per-kernel figures (``--full``) come from event pairs the product path records on its launch stream while the timed steps run
(nerfdet_amd/trace.py): `roofline` = the dominant hand-written kernel of the step (the convolution instantiation with the largest
share) against the matrix-core peak of its arithmetic; `roofline_all_convolutions` aggregates every convolution launch;
`roofline_memory_bound_convolutions` prices the launches whose arithmetic intensity lies below the machine's ridge point (the
ResNet 1x1 layers) against HBM instead; `roofline_projection` / `roofline_density_features` are the gather kernels K1 / K2
of the volumetric path against HBM.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec; the ceiling a float4 copy reaches on the box is measured live (hbm_copy_ceiling)
MFMA_F32_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: dense fp32-input MFMA peak (v_mfma_f32_16x16x4_f32), = fp32 vector peak
MFMA_BF16_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 MFMA peak (no sparsity)

# BASELINE.json configs; cfg5's voxel size is halved so that the 80x80x32 grid keeps the room's extent ("state which")
# The ~80 convolution launches of a step are bracketed by event pairs on every SPAN_EVERY-th timed step only: the pairs are commands in the stream
# like any other (~2 us each on the command processor), and a step that carries all of them runs ~0.45 ms longer (p90 vs median of the per-step
# times).  Five instrumented steps of thirty give every launch five samples; the other spans (K1, K2, post-processing) and the stage marks are
# recorded on every step.
SPAN_EVERY = 6

WORKLOADS = {
    "cfg2": dict(n_views=50, img_hw=(240, 320), channels=256, n_voxels=(40, 40, 16), voxel_size=(0.16, 0.16, 0.2), depth=50),
    "cfg1": dict(n_views=10, img_hw=(240, 320), channels=256, n_voxels=(40, 40, 16), voxel_size=(0.16, 0.16, 0.2), depth=50),
    "cfg5": dict(n_views=101, img_hw=(320, 480), channels=256, n_voxels=(80, 80, 32), voxel_size=(0.08, 0.08, 0.1), depth=101),
    "tiny": dict(n_views=6, img_hw=(64, 96), channels=256, n_voxels=(16, 16, 8), voxel_size=(0.4, 0.4, 0.4), depth=50),
}


def k1_algorithmic_bytes(w):
    """every FPN feature row read once + (C fp32 + int64 count) written per voxel."""
    n = w["n_voxels"][0] * w["n_voxels"][1] * w["n_voxels"][2]
    hf, wf = w["img_hw"][0] // 4, w["img_hw"][1] // 4
    return w["n_views"] * w["channels"] * hf * wf * 4 + (w["channels"] * 4 + 8) * n


def k2_algorithmic_bytes(w, cm=32):
    """de-normalised images + mapped map read once + 2*(3+cm) floats written per voxel."""
    n = w["n_voxels"][0] * w["n_voxels"][1] * w["n_voxels"][2]
    h, wd = w["img_hw"]
    return 4 * (w["n_views"] * 3 * h * wd + w["n_views"] * cm * (h // 4) * (wd // 4) + 2 * (3 + cm) * n)


def profile_kernel_name(name, arithmetic):
    """bench's span name ("k_conv_split_halo<4,4>/f16x2") -> the instantiation's name in a rocprofv3 profile ("k_conv_split_halo<4,4,1>"): the
    last template argument of the split-family kernels is their arithmetic scheme (0 = bf16x3, 1 = fp16 pair, 2 = one bf16 product)."""
    base = name[:-len("/f16x2")] if name.endswith("/f16x2") else name
    sch = 1 if name.endswith("/f16x2") else (2 if arithmetic == "bf16" else 0)
    if base == "k_conv_split_ws":
        return f"k_conv_split_ws<{sch}>"
    if base.startswith("k_conv_split_wsp<"):
        args = base[len("k_conv_split_wsp<"):-1].split(",")
        return f"k_conv_split_wsp<{sch},{args[0]},{args[1] if len(args) > 1 else 4}>"
    if base.endswith(",p8>"):
        return base[:-len(",p8>")] + f",{sch},8>"
    if base.startswith("k_conv_split_halo<"):
        return base[:-1] + f",{sch},4>"
    if base.startswith(("k_conv_split<", "k_conv_split_chain<")):
        return base[:-1] + f",{sch}>"
    return base


def traffic_of(traffic, name, arithmetic="bf16x3"):
    """Per-launch bytes of kernel ``name`` in a {profile kernel name: bytes} table (rocprofv3 --pmc passes under profiles/)."""
    want = profile_kernel_name(name, arithmetic)
    if want in traffic:
        return traffic[want]
    if want.startswith("k_conv_split_halo<") and want.endswith(",4>") and want[:-len(",4>")] + ">" in traffic:
        return traffic[want[:-len(",4>")] + ">"]          # profiles older than the producer-count template argument
    stem = name[:-1] if name.endswith(">") else name
    return next((v for k, v in traffic.items() if k == name or k.startswith(stem + "<") or k.startswith(stem + ">")
                 or (not name.endswith(">") and k.startswith(stem + "_packed"))), None)    # K1 / K2 / K4 run as "<name><...>" / "<name>_packed<...>"


def measured_traffic(workload):
    """HBM-side bytes per launch from the rocprofv3 PMC passes committed under profiles/ (FETCH_SIZE / WRITE_SIZE in separate
    passes, FETCH_SIZE doubled as the gfx950 note in MI355X_MICROARCH.md prescribes): {kernel-name prefix: bytes}, source file."""
    import glob
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_hbm_traffic.json")), reverse=True):  # newest round first
        try:
            with open(path) as f:
                d = json.load(f)
            if d.get("workload") != workload:
                continue
            out = {"k_backproject_aggregate": int(d["k1"]["traffic_bytes"])}
            for name, v in d.get("kernels", {}).items():
                out[name] = int(v["traffic_bytes"])
            return out, os.path.relpath(path, ROOT)
        except (OSError, KeyError, ValueError):
            pass
    return {}, None


def synth_batch(w, seed):
    """ring cameras, img ~ N(0,1), denorm_images ~ U[0,1), one dummy NeRF target view
    (rays are unused at inference unless render_testing)."""
    from nerfdet_amd.synth import ring_scene_meta
    g = torch.Generator().manual_seed(seed)
    h, wd = w["img_hw"]
    meta = ring_scene_meta(w["n_views"], w["img_hw"])
    return dict(img=torch.randn(1, w["n_views"], 3, h, wd, generator=g), img_metas=[meta],
                denorm_images=torch.rand(1, w["n_views"], 3, h, wd, generator=g),
                lightpos=torch.zeros(1, 1, 4, 3), raydirs=torch.ones(1, 1, 4, 3), gt_images=torch.zeros(1, 1, 4, 3),
                gt_depths=[], nerf_sizes=[torch.tensor([[2, 2, 3]])])


def build_model(w):
    """Seeded random-init nerfdet (no checkpoints offline).  A raw random init is a degenerate workload (density 0
    everywhere, every score below score_thr -> NMS sees nothing), so the weights are nudged into a trained-like
    regime: O(1) FPN features, positive densities, a few hundred NMS candidates.  Costs are data independent
    except for NMS."""
    from nerfdet_amd.presets import build_nerfdet
    torch.manual_seed(0)
    det = build_nerfdet(w["depth"], n_voxels=w["n_voxels"], voxel_size=w["voxel_size"])
    with torch.no_grad():
        det.neck.fpn_convs[0].conv.weight.mul_(1 / 30.0)
        if w["depth"] != 50:
            # a deeper random-init ResNet without calibrated BatchNorm statistics grows its activations with depth (x1000 at 101
            # layers): bring FPN level 0 to the scale the ResNet-50 workload has (std ~2), measured on two small random views
            g = torch.Generator().manual_seed(1)
            det.eval()
            std = float(det.neck(det.backbone(torch.randn(2, 3, 120, 160, generator=g)))[0].std())
            det.neck.fpn_convs[0].conv.weight.mul_(2.0 / std)
            det.neck.fpn_convs[0].conv.bias.mul_(2.0 / std)
        det.nerf_mlp.mlp.sigma_layer.output_layer.bias.fill_(2.0)
        det.bbox_head.cls_conv.weight.normal_(0, 0.3)
        det.bbox_head.cls_conv.bias.fill_(-2.0)
        det.bbox_head.centerness_conv.weight.normal_(0, 0.1)
        det.bbox_head.reg_conv.weight.normal_(0, 0.05)
        det.mapping[0].bias.normal_(0, 0.3)
    return det.eval()


def to_device(batch, device):
    out = {}
    for k, v in batch.items():
        out[k] = v.to(device) if isinstance(v, torch.Tensor) else v
    return out


def dump_outputs(directory, res, rank):
    """What a caller of ``forward_test`` receives for the step's one scene -- boxes (K, 7), scores (K,), labels (K,) -- as
    DIR/{boxes_3d,scores_3d,labels_3d}.npy in float32 (class ids are exact in fp32); ranks r > 0 add ``_rank<r>`` to the names."""
    import numpy as np
    (scene,) = res
    os.makedirs(directory, exist_ok=True)
    suffix = f"_rank{rank}" if rank else ""
    for name, t in (("boxes_3d", scene["boxes_3d"].tensor), ("scores_3d", scene["scores_3d"]), ("labels_3d", scene["labels_3d"])):
        np.save(os.path.join(directory, f"{name}{suffix}.npy"), t.detach().to("cpu", torch.float32).numpy())


def cpu_baseline(w, det_cpu, batch, scenes=5, warmups=2):
    """The reference's algorithm on the host cores (median of >= 5 runs after 2 warm-ups, per stage):
    the oracle (PyTorch-CPU restatement: materialised per-view volume, Python per-view loops, sequential NMS) for the
    volumetric path, 3D neck, head and NMS, plus the same ResNet+FPN modules run by PyTorch-CPU."""
    from oracle import nerfdet_oracle as O
    O.PINNED_ARITHMETIC = False   # time the reference's own library calls (torch.bmm), not the oracle's host-independent emulation of them
    cores = min(os.cpu_count() or 1, 32)  # measured on the GPU box: 16-32 threads is the knee (256 is 50x slower)
    torch.set_num_threads(cores)
    meta = batch["img_metas"][0]
    tc = det_cpu.bbox_head.test_cfg
    sd_mlp = det_cpu.nerf_mlp.state_dict()
    sd_n3 = dict(det_cpu.neck_3d.state_dict())
    sd_head = det_cpu.bbox_head.state_dict()
    rows = []
    with torch.no_grad():
        for _ in range(scenes + warmups):
            t = [time.perf_counter()]
            feats = det_cpu.neck(det_cpu.backbone(batch["img"][0]))[0]
            t.append(time.perf_counter())
            ov = O.extract_volume(feats, batch["denorm_images"][0], meta, w["n_voxels"], w["voxel_size"],
                                  det_cpu.mapping[0].weight, det_cpu.mapping[0].bias, sd_mlp)
            t.append(time.perf_counter())
            n3 = O.neck3d_forward(sd_n3, ov["volume"].unsqueeze(0))
            t.append(time.perf_counter())
            ctr, reg, cls = O.head_forward(sd_head, n3)
            O.head_get_bboxes(ctr, reg, cls, ov["valid"].unsqueeze(0).float(), meta["lidar2img"]["origin"], w["voxel_size"],
                              tc.nms_pre, tc.score_thr, tc.iou_thr)
            t.append(time.perf_counter())
            rows.append([b - a for a, b in zip(t, t[1:])] + [t[-1] - t[0]])
    rows = rows[warmups:]
    med = [sorted(r[i] for r in rows)[len(rows) // 2] for i in range(5)]
    return dict(value=1.0 / med[4], unit="scenes/s", cores=cores, kind="port",
                sample=f"median of {scenes} full scenes after {warmups} warm-ups ({med[4]:.2f} s/scene): ResNet-{w['depth']}+FPN (PyTorch-CPU) + "
                       f"oracle volumetric path + 3D neck + head + sequential NMS, same shapes and weights, fp32",
                stages_s=dict(backbone_fpn=med[0], volumetric_hot_path=med[1], neck3d=med[2], head_nms=med[3]))


def launch_ranks(args) -> int:
    """``python bench.py --gpus N`` without a launcher: start the N ranks as fresh child processes (this parent never touches the
    GPU), rank 0 inherits stdout and prints the JSON line; a rank that dies takes the others down (nerfdet_amd.dist.launch_local_ranks)."""
    from nerfdet_amd.dist import launch_local_ranks
    return launch_local_ranks(__file__, sys.argv[1:], args.gpus)


def dry_run(args, rank, world):
    """Launcher / rendezvous / timing plumbing without a GPU (tests/test_dist_cpu.py): gloo, a sleep as the step."""
    import torch.distributed as dist
    if world > 1:
        dist.init_process_group("gloo")
        from nerfdet_amd.dist import apply_rank_affinity
        share = apply_rank_affinity(int(os.environ.get("LOCAL_RANK", rank)), int(os.environ.get("LOCAL_WORLD_SIZE", world)))
        assert share["threads"] >= 1 and torch.get_num_threads() == share["threads"]
    for _ in range(args.warmup):
        time.sleep(0.001)
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        time.sleep(0.002 * (rank + 1))   # ranks differ: the job's time must be the slowest rank's
    if os.environ.get("NDET_DRYRUN_DIE_RANK") == str(rank):      # test hook of the dry run only: this rank dies while the others sit in the barrier
        os._exit(3)
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    from nerfdet_amd.dist import max_over_ranks
    dt = max_over_ranks(dt)
    if rank == 0:
        print(json.dumps({"metric": "dry-run", "value": world * args.steps / dt, "unit": "steps/s", "n_gpus": world, "steps": args.steps,
                          "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "dry_run": True}))
    if world > 1:
        dist.destroy_process_group()


def hbm_copy_ceiling(device, mib=1024, reps=20):
    """Empirical HBM ceiling: the library's float4 copy kernel (ndet_hbm_copy) on two ``mib``-MiB buffers -- far beyond the
    256 MB Infinity Cache --, HIP events on the launch stream, best and median of ``reps`` launches.  GB/s counts read + write."""
    from ctypes import c_void_p
    from nerfdet_amd import _lib
    lib = _lib.load()
    n = mib * (1 << 20) // 4
    src = torch.empty(n, dtype=torch.float32, device=device).normal_()
    dst = torch.empty_like(src)
    stream = torch.cuda.current_stream(device)
    sp = c_void_p(stream.cuda_stream)

    def launch():
        _lib.check(lib.ndet_hbm_copy(c_void_p(src.data_ptr()), c_void_p(dst.data_ptr()), n, sp), "hbm_copy")
    for _ in range(3):
        launch()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(stream)
        launch()
        b.record(stream)
    torch.cuda.synchronize(device)
    assert torch.equal(dst[:4096], src[:4096]) and torch.equal(dst[-4096:], src[-4096:])
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    gbs = [2 * 4 * n / (m * 1e-3) / 1e9 for m in ms]
    return {"best": gbs[0], "median": gbs[len(gbs) // 2], "mib_per_buffer": mib, "launches": reps}


def serve_in_flight(det, batch, steps, n_streams=2):
    """The same K scenes with ``n_streams`` of them in flight (nerfdet.forward_test_async: every launch of a scene queued on its own
    stream, the host collecting the previous scene's detections meanwhile).  Not the headline: `value` is the one-scene-at-a-time loop the
    reference's test loop runs; this is what a server gets out of the same kernels.  Returns scenes/s."""
    kw = {k: v for k, v in batch.items() if k not in ("img", "img_metas")}
    streams = [torch.cuda.Stream() for _ in range(n_streams)]
    with torch.no_grad():
        for s_ in streams:                      # per-stream buffers and allocator pools
            with torch.cuda.stream(s_):
                det.forward_test_async(batch["img"], batch["img_metas"], **kw)()
        torch.cuda.synchronize()
        pend, last = [], None
        t0 = time.perf_counter()
        for i in range(steps):
            with torch.cuda.stream(streams[i % n_streams]):
                pend.append(det.forward_test_async(batch["img"], batch["img_metas"], **kw))
            if len(pend) == n_streams:
                last = pend.pop(0)()
        while pend:
            last = pend.pop(0)()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    assert last is not None and "boxes_3d" in last[0]
    return steps / dt


def train_probe(det_gpu, batch):
    """BASELINE configs[2]'s per-rank training step (40 source + 10 NeRF target views 240x320, 40x40x16 voxels, 2048 rays x 64 samples, five
    losses, backward, clip, AdamW) timed by tools/bench_train.py in a CHILD process after everything else has been measured (this process
    first drops its model and cache: the child gets the card to itself).  Not the headline -- the step the reference trains with, in the
    driver's record.  Returns {ms, median_ms, dtype, roofline_all_convolutions, ...} or {error}."""
    import gc
    import subprocess
    det_gpu.to("cpu")
    batch.clear()
    gc.collect()
    torch.cuda.empty_cache()
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_train.py"), "--steps", "8", "--warmup", "3"], capture_output=True, text=True,
                           timeout=420, env={k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")})
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode != 0 or not lines:
            return {"error": f"tools/bench_train.py rc={r.returncode}: {r.stderr[-300:]}"}
        d = json.loads(lines[-1])
        keep = {"ms": d["ms_per_step"], "median_ms": d["median_ms"], "p10_ms": d["p10_ms"], "p90_ms": d["p90_ms"], "steps": d["steps"], "warmup": d["warmup"],
                "dtype": d["dtype"], "scenes_per_s": d["value"], "workload": d["config"]["workload"], "log_vars": d["log_vars"], "peak_mem_GB": d["peak_mem_GB"],
                "host_sync": d.get("host_sync"), "ms_host_read_every_step": d.get("ms_per_step_host_read_every_step"),
                "note": "tools/bench_train.py --steps 8 --warmup 3 in a child process after the timed region; one rank, no DDP"}
        for k in ("roofline", "roofline_all_convolutions", "roofline_k4_forward", "roofline_k4_backward"):
            if k in d:
                keep[k] = {kk: vv for kk, vv in d[k].items() if kk != "per_kernel"}
        return keep
    except Exception as e:      # the extra figure must never cost the headline line
        return {"error": f"{type(e).__name__}: {e}"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="cfg2", choices=sorted(WORKLOADS))
    ap.add_argument("--full", action="store_true", help="besides the headline: per-kernel spans and stage times of the timed steps, HBM copy ceiling, "
                    "rooflines, two-scenes-in-flight loop, bf16x3 comparison, CPU baseline, training-step probe")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the detections of the last timed step to DIR/<name>.npy (float32)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-train-probe", action="store_true", help="with --full: skip the cfg3 training-step figure (tools/bench_train.py in a child "
                    "process after the timed region; BENCH records then carry a driver-run training number: key train_cfg3_step)")
    ap.add_argument("--no-serving", action="store_true", help="with --full: skip the extra two-scenes-in-flight loop after the timed region (profiling "
                    "runs: its overlapped launches would enter the per-kernel averages)")
    ap.add_argument("--graph", action="store_true",
                    help="replay the static part of the step from hipGraphs (nerfdet_amd/graphed.py); measured equal to eager "
                         "launches within 1 %% on MI355X: the step is GPU-bound, launch-ahead already hides the gaps")
    ap.add_argument("--conv-arithmetic", default=None, choices=["f32", "bf16x3", "bf16", "f16x2"],
                    help="convolution kernel family (default: the package default, nerfdet_amd.conv3d.ARITHMETIC)")
    ap.add_argument("--dry-run", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-gc-freeze", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-chain-mapping", action="store_true", help=argparse.SUPPRESS)     # measurement: the feature mapping as a launch of its own
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    if args.dry_run:
        return dry_run(args, rank, world)
    assert torch.cuda.is_available(), "bench.py needs a GPU"
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    from nerfdet_amd import dist as D
    if world > 1 or D.launched():      # under a launcher also a single rank joins a process group: the 1-GPU run exercises the RCCL path
        D.init_dist("nccl")
        # N ranks share the host: each keeps to its own block of CPUs and caps its thread pools (nerfdet_amd.dist.rank_affinity)
        D.apply_rank_affinity(local, int(os.environ.get("LOCAL_WORLD_SIZE", world)))
    grouped = torch.distributed.is_available() and torch.distributed.is_initialized()

    import nerfdet_amd.conv3d as C3
    from nerfdet_amd import trace
    w = WORKLOADS[args.workload]
    det = build_model(w)
    batch_cpu = synth_batch(w, rank)
    det_gpu = det.to(device)
    if args.no_chain_mapping and "chain_linear" in det_gpu.neck.__dict__:
        det_gpu.neck.__dict__["chain_linear"] = None
    batch = to_device(batch_cpu, device)
    if args.conv_arithmetic:
        C3.set_arithmetic(args.conv_arithmetic)

    state = {"step": 0}
    # ~150 conv launches per step: their event pairs cost ~2 % of the step, so they are sampled on every SPAN_EVERY-th timed step (see the constant); the two
    # gather kernels and the five stage marks are recorded on every step.  A plain run records none of them (trace.recorder stays None).
    rec = None
    if args.full:
        rec = trace.Recorder(sample=lambda name: (not name.startswith(("k_conv", "k_bottleneck", "k_point_mlp", "f32:", "bf16x3:", "f16x2:", "bf16:"))) or state["step"] % SPAN_EVERY == 0)

    if args.graph:
        from nerfdet_amd.graphed import GraphedForwardTest
        graphed = GraphedForwardTest(det_gpu)
        graphed.k1_hook = lambda fn: trace.span("k_backproject_aggregate", fn, bytes=k1_algorithmic_bytes(w), kind="hbm")

        def step():
            return graphed(return_loss=False, **batch)
    else:
        def step():
            with torch.no_grad():
                return det_gpu(return_loss=False, **batch)

    def barrier():
        if grouped:
            torch.distributed.barrier()

    for _ in range(args.warmup):
        res = step()
    # the model's ~10^5 long-lived Python objects out of the cyclic collector's reach (what a serving process does after start-up): a full collection
    # in the middle of the timed steps walks all of them
    import gc
    gc.collect()
    if not args.no_gc_freeze:
        gc.freeze()
    trace.recorder = rec
    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ticks = [t0]
    for i in range(args.steps):
        state["step"] = i
        res = step()
        ticks.append(time.perf_counter())     # a step hands back host-side detections: it has ended when it returns
    torch.cuda.synchronize()
    barrier()
    dt = time.perf_counter() - t0
    from nerfdet_amd.dist import max_over_ranks
    dt = max_over_ranks(dt, device)
    per_step = sorted((b - a) * 1e3 for a, b in zip(ticks, ticks[1:]))
    pct = lambda q: per_step[min(len(per_step) - 1, int(round(q * (len(per_step) - 1))))]
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, res, rank)

    def headline():
        return {
            "metric": f"scenes/sec ({w['n_views']}-view {w['img_hw'][0]}x{w['img_hw'][1]}, {'x'.join(map(str, w['n_voxels']))} voxels)",
            "value": world * args.steps / dt,
            "unit": "scenes/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3,
            "median_ms": pct(0.5), "p10_ms": pct(0.1), "p90_ms": pct(0.9),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": {"f32": "f32", "f16x2": "f32 (convolutions: fp32 operands as hi + lo fp16 pairs of the power-of-two pre-scaled tensors, three products per "
                               "multiply on the fp16 MFMA, fp32 accumulate; error against fp64 at or below the six-product bf16x3 form's; a device-side range "
                               "guard repeats a scene on bf16x3 when part of a tensor falls outside the pair's window: range_guard_trips)",
                      "bf16x3": "f32 (convolutions: fp32 operands as exact 3-term bf16 sums on the bf16 MFMA, fp32 accumulate)",
                      "bf16": "bf16 (convolution operands rounded to bf16 on the MFMA, fp32 accumulate; activations, projection, aggregation, "
                              "NMS fp32 -- SURVEY.md 0.1)"}[C3.ARITHMETIC],
            "data": "synthetic",
            "config": {"workload": f"{args.workload}: nerfdet_res{w['depth']}_2x_low_res forward_test, {w['n_views']} views "
                                   f"{w['img_hw'][0]}x{w['img_hw'][1]}, {'x'.join(map(str, w['n_voxels']))} voxels, "
                                   f"{'bf16 convolutions' if C3.ARITHMETIC == 'bf16' else 'fp32'}, 1 scene/step/GPU, random-init weights",
                       "scenes_per_step": world, "parallelism": f"scene replicas x{world} (no data-path collective)"},
            "collectives": (f"{torch.distributed.get_backend()} (timing barrier + max-over-ranks only)" if grouped else "none (bare single process)"),
            "execution": "hipGraph replay (2 graphs) + eager K1 + eager post-processing" if args.graph else "eager launches",
            "detections_last_step": int(len(res[0]["scores_3d"])),
            "range_guard_trips": C3.guard_trips,      # scenes repeated on bf16x3 because a fp16-pair launch reported a visible absolute error floor (expected: 0)
        }

    if not args.full:
        if rank == 0:
            print(json.dumps(headline()))
        if grouped:
            torch.distributed.destroy_process_group()
        return

    n_conv_steps = len([i for i in range(args.steps) if i % SPAN_EVERY == 0])
    if args.graph:  # per-kernel breakdown from a few eager steps outside the timed region (events cannot sit inside a graph)
        keep = [s for s in rec.spans if s[0] == "k_backproject_aggregate"]
        rec.spans, rec.marks = [], []
        state["step"] = 0
        n_conv_steps = 5
        with torch.no_grad():
            for _ in range(n_conv_steps):
                det_gpu(return_loss=False, **batch)
        rec.spans = [s for s in rec.spans if s[0] != "k_backproject_aggregate"] + keep
    trace.recorder = None
    torch.cuda.synchronize()
    serving = None
    if not (args.graph or args.no_serving):
        try:
            serving = serve_in_flight(det_gpu, batch, args.steps)
        except Exception as e:     # the extra figure must never cost the headline line
            print(f"serve_in_flight skipped: {type(e).__name__}: {e}", file=sys.stderr)

    six = None
    if C3.ARITHMETIC == "f16x2" and not (args.graph or args.no_serving):
        # the same scenes in the six-product bf16x3 arithmetic (operands represented exactly), INTERLEAVED with the fp16-pair arithmetic step by step
        # in one loop after the timed region: a step hands back host-side detections, so every step is timed on its own, and the two series share
        # the clock state, the box and the allocator -- what the fp16-pair arithmetic is measured against
        try:
            n_ab = max(6, min(args.steps, 24))
            for a in ("bf16x3", "f16x2", "bf16x3"):          # both packs and tile tables warm
                C3.set_arithmetic(a)
                step()
            per = {"f16x2": [], "bf16x3": []}
            torch.cuda.synchronize()
            for i in range(2 * n_ab):
                a = ("f16x2", "bf16x3")[i & 1]
                C3.set_arithmetic(a)
                t_a = time.perf_counter()
                step()
                per[a].append((time.perf_counter() - t_a) * 1e3)
            torch.cuda.synchronize()
            med = {a: sorted(v)[len(v) // 2] for a, v in per.items()}
            six = {"value": world * 1e3 / med["bf16x3"], "unit": "scenes/s", "median_ms": med["bf16x3"],
                   "interleaved_f16x2": {"value": world * 1e3 / med["f16x2"], "median_ms": med["f16x2"]},
                   "speedup_f16x2_over_bf16x3": med["bf16x3"] / med["f16x2"], "steps_each": n_ab,
                   "note": "conv3d.set_arithmetic('bf16x3'): fp32 operands as exact 3-term bf16 sums, six MFMA products per multiply; same scenes, "
                           "alternating step by step with the fp16-pair arithmetic after the timed region (medians of per-step host times); not the headline"}
        except Exception as e:
            print(f"bf16x3 comparison skipped: {type(e).__name__}: {e}", file=sys.stderr)
        finally:
            C3.set_arithmetic("f16x2")

    copy = hbm_copy_ceiling(device) if rank == 0 else None
    if rank == 0:
        spans = rec.span_ms()
        stages = rec.stage_ms()
        traffic, traffic_src = measured_traffic(args.workload)
        conv_traffic = lambda name: traffic_of(traffic, name, C3.ARITHMETIC)
        bf16x3 = C3.ARITHMETIC == "bf16x3"
        # MFMA products issued per algorithmic multiply-add by a launch of the split family: 3 in the fp16-pair arithmetic, 6 in bf16x3
        # (in f16x2 mode the layers below conv3d.F16_MIN_KSTEPS K steps run on bf16x3: their names carry no "/f16x2")
        products = (lambda name: 3.0 if name.endswith("/f16x2") else 6.0) if C3.ARITHMETIC == "f16x2" else None
        if C3.ARITHMETIC == "f16x2":
            conv_kernel = ("k_conv_split in its fp16-pair mode (implicit-GEMM convolution on the fp16 matrix cores, fp32 operands as hi + lo fp16 pairs of "
                           "the power-of-two pre-scaled tensors, 3 MFMA products per multiply, fp32 accumulate; layers with fewer than "
                           f"{C3.F16_MIN_KSTEPS} K steps in the 6-product bf16x3 mode): 3D neck + head, ResNet/FPN; all tile instantiations, split-K reduce "
                           "launches included in the event spans")
            conv_peak = MFMA_BF16_PEAK_TFLOPS / 3.0
            conv_peak_note = ("achieved = algorithmic fp32 convolution FLOPs / time; peak = dense fp16 MFMA peak 2500 TFLOP/s / issued products per "
                              "algorithmic multiply-add (3 for the fp16-pair launches, 6 for the bf16x3 ones; for a mix of launches: the FLOP-weighted "
                              "harmonic mean)")
        elif C3.ARITHMETIC == "bf16":
            conv_kernel = ("k_conv_split in its one-product mode (implicit-GEMM convolution, both operands rounded to bf16, one bf16 MFMA product per "
                           "multiply, fp32 accumulate, fp32 activations in HBM): 3D neck + head, ResNet/FPN; all tile instantiations")
            conv_peak = MFMA_BF16_PEAK_TFLOPS
            conv_peak_note = "achieved = algorithmic convolution FLOPs / time; peak = dense bf16 MFMA peak 2500 TFLOP/s"
        elif bf16x3:
            conv_kernel = ("k_conv_split (implicit-GEMM convolution on the bf16 matrix cores, fp32 operands split exactly into 3 bf16 terms, "
                           "6 MFMA products per multiply, fp32 accumulate: 3D neck + head, ResNet/FPN; all tile instantiations, split-K "
                           "reduce launches included in the event spans)")
            conv_peak = MFMA_BF16_PEAK_TFLOPS / 6.0
            conv_peak_note = ("achieved = algorithmic fp32 convolution FLOPs / time; peak = dense bf16 MFMA peak 2500 TFLOP/s / 6 issued "
                              "products per algorithmic multiply-add")
        else:
            conv_kernel = ("k_conv3d_igemm (fp32-MFMA implicit-GEMM convolution: 3D neck + head, ResNet/FPN bottlenecks; both tile "
                           "instantiations, split-K reduce launches included in the event spans)")
            conv_peak = MFMA_F32_PEAK_TFLOPS
            conv_peak_note = "dense fp32-input MFMA peak"
        ridge = conv_peak * 1e12 / (HBM_PEAK_GBS * 1e9)     # FLOP per byte where the two roofs meet
        conv = {k: v for k, v in spans.items() if v and v[0][1].get("kind") == "conv"}
        by_kernel = {k: [sum(i["flops"] for _, i in v), sum(ms for ms, _ in v), len(v), sum(i["bytes"] for _, i in v)] for k, v in conv.items()}
        conv_flops = sum(v[0] for v in by_kernel.values())
        conv_ms = sum(v[1] for v in by_kernel.values())
        conv_n = sum(v[2] for v in by_kernel.values())
        # the dominant kernel: the kernel TEMPLATE (k_conv_split_halo, k_conv_split_ws, ...) with the largest share of the step in one arithmetic, its
        # tile instantiations (<4,2>, <4,4>, <8,2>, <4,4,p8>: the same source, chosen per layer shape) taken together; they are listed one by one
        # under roofline_all_convolutions.per_kernel
        family = lambda name: name.split("<")[0] + ("/f16x2" if name.endswith("/f16x2") else "")
        by_family = {}
        for k, v in by_kernel.items():
            f = by_family.setdefault(family(k), [0.0, 0.0, 0, 0.0, []])
            for i in range(4):
                f[i] += v[i]
            f[4].append(k)
        dom_name, (dom_flops, dom_ms, dom_n, dom_bytes, dom_members) = max(by_family.items(), key=lambda kv: kv[1][1])
        dom_tflops = dom_flops / (dom_ms * 1e-3) / 1e12
        dom_peak = all_peak = conv_peak
        if products is not None:      # per-launch product counts: the time the matrix cores need at their peak sets the roof
            dom_peak = MFMA_BF16_PEAK_TFLOPS / products(dom_name)
            all_peak = conv_flops / sum(v[0] * products(k) / MFMA_BF16_PEAK_TFLOPS for k, v in by_kernel.items())
        dom_big = max(dom_members, key=lambda k: by_kernel[k][1])      # the instantiation the PMC traffic figure is quoted for
        mem = [(ms, i) for v in conv.values() for ms, i in v if i["flops"] / max(i["bytes"], 1) < ridge]
        mem_bytes, mem_ms = sum(i["bytes"] for _, i in mem), sum(ms for ms, _ in mem)

        def hbm_line(name, label, abytes):
            ms = sorted(m for m, _ in spans.get(name, []))
            if not ms:
                return None
            avg = sum(ms) / len(ms)
            ach = abytes / (avg * 1e-3) / 1e9
            tr = traffic_of(traffic, name)   # profile names carry template arguments
            return {"kernel": label, "bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                    "frac_of_copy_ceiling": ach / copy["best"], "traffic": tr, "traffic_source": None if tr is None else
                    f"{traffic_src} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes)",
                    "algorithmic_bytes": abytes, "avg_launch_ms": avg, "median_launch_ms": ms[len(ms) // 2], "launches": len(ms)}

        out = {
            **headline(),
            "hbm_copy_ceiling_gbs": copy["best"], "hbm_copy_ceiling": copy,
            "roofline": {"kernel": f"{dom_name} (the convolution kernel with the largest share of the step, tile instantiations {sorted(dom_members)} "
                                   f"together; event spans include the split-K reduce launch where a layer splits K; traffic: {dom_big})",
                         "bound": "mfma", "achieved": dom_tflops, "peak": dom_peak, "unit": "TFLOP/s",
                         "frac": dom_tflops / dom_peak, "traffic": conv_traffic(dom_big),
                         "achieved_over_six_product_roof": dom_tflops / (MFMA_BF16_PEAK_TFLOPS / 6.0),   # the roof of the bf16x3 arithmetic (rounds 1 - 3a)
                         "traffic_source": None if conv_traffic(dom_big) is None else traffic_src, "peak_note": conv_peak_note,
                         "traffic_launches_algorithmic_bytes": by_kernel[dom_big][3] / by_kernel[dom_big][2],
                         "algorithmic_flops_per_launch": dom_flops / dom_n, "algorithmic_bytes_per_launch": dom_bytes / dom_n,
                         "launches_per_step": dom_n / n_conv_steps,
                         "avg_launch_ms": dom_ms / dom_n, "total_ms_per_step": dom_ms / n_conv_steps, "sampled_steps": n_conv_steps},
            "roofline_all_convolutions": {"kernel": conv_kernel,
                         "bound": "mfma", "achieved": conv_flops / (conv_ms * 1e-3) / 1e12, "peak": all_peak, "unit": "TFLOP/s",
                         "frac": conv_flops / (conv_ms * 1e-3) / 1e12 / all_peak, "traffic": None, "peak_note": conv_peak_note,
                         "algorithmic_flops_per_step": conv_flops / n_conv_steps, "launches_per_step": conv_n / n_conv_steps,
                         "avg_launch_ms": conv_ms / conv_n, "total_ms_per_step": conv_ms / n_conv_steps,
                         "sampled_steps": n_conv_steps,
                         "per_kernel": {k: {"launches_per_step": v[2] / n_conv_steps, "avg_launch_ms": v[1] / v[2],
                                            "tflops": v[0] / (v[1] * 1e-3) / 1e12, "gbytes_per_s": v[3] / (v[1] * 1e-3) / 1e9}
                                        for k, v in sorted(by_kernel.items())}},
            "roofline_memory_bound_convolutions": None if not mem else {
                         "kernel": f"convolution launches whose algorithmic intensity is below the ridge point ({ridge:.0f} FLOP/B): the ResNet "
                                   f"1x1 layers and the stride-2 / small-K layers -- HBM is the roof that binds them",
                         "bound": "hbm", "achieved": mem_bytes / (mem_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": mem_bytes / (mem_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                         "frac_of_copy_ceiling": mem_bytes / (mem_ms * 1e-3) / 1e9 / copy["best"], "traffic": None,
                         "algorithmic_bytes_per_step": mem_bytes / n_conv_steps, "launches_per_step": len(mem) / n_conv_steps,
                         "total_ms_per_step": mem_ms / n_conv_steps},
            "roofline_projection": hbm_line("k_backproject_aggregate", "k_backproject_aggregate (K1: fused backproject + view mean/count + alpha gating)",
                                            k1_algorithmic_bytes(w)),
            "roofline_density_features": hbm_line("k_density_features", "k_density_features (K2: mapped features + RGB -> per-voxel mean / exp(-var) rows)",
                                                  k2_algorithmic_bytes(w)),
            "stages_ms": stages,
        }
        if serving is not None:
            out["serving_two_scenes_in_flight"] = {
                "value": serving * world, "unit": "scenes/s",
                "note": "the same K scenes per GPU through nerfdet.forward_test_async with two scenes in flight on two streams (results collected "
                        "on the host one scene behind); not the headline -- `value` is the reference's one-scene-at-a-time test loop"}
        if six is not None:
            out["six_product_bf16x3_arithmetic"] = six
        if not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(w, build_model(w), batch_cpu)
        if not (args.no_train_probe or args.graph or args.no_serving) and world == 1 and args.workload == "cfg2":
            out["train_cfg3_step"] = train_probe(det_gpu, batch)
        print(json.dumps(out))
    if grouped:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
