"""Streaming scene inference: a scene's views arrive in chunks, detections are available after any of them.

``nerfdet.begin_scene(img_meta)`` returns a :class:`SceneStream`.  ``add_views`` runs the backbone and FPN on a chunk of views (the FPN's
output convolution producing the mapped map on the way, as ``extract_feat`` does) and folds the chunk into the scene's running sums
(ops.scene_accumulate); the chunk's feature maps are dropped right after.  ``detect`` finishes the sums into the reference's conditioning
rows and gated volume (nerfdet.py:164-176, 234-261) and runs neck_3d and the head, exactly as ``simple_test``'s tail does.  The backbone
runs once per view, when the view arrives, and memory is the state's (ops.SceneState), whatever the number of views.

K1's sums and every count are the same bits whatever the chunking; K2's sums add per chunk, so its rows differ from the one-shot kernel's by
rounding only.  A single chunk reproduces ``simple_test`` bit for bit.

``begin_scene(img_meta, window=S)`` keeps the last S chunks only: every ``add_views`` call fills a state of its own, the oldest state is
dropped when an (S+1)-th chunk arrives (or by ``drop_oldest``), and ``detect`` finishes over the states held, oldest first
(ops.density_finish_ring / volume_finish_ring).  Nothing is subtracted, so a dropped chunk leaves no trace: the window's answer is the
bits a fresh windowed stream gives when fed the same chunks.

``begin_scene(img_meta, keep_views=True)`` also keeps what the NeRF ray branch needs of every view, chunk by chunk, in a view bank
(rays.ViewBank): the mapped map as it is accumulated, the packed image and 12 camera floats -- 4 (hf wf cm + 4 H W) + 64 bytes a view.
``render_rays(ray_o, ray_d)`` then renders any rays at any time, ``render(ray_batch)`` the target views of a ray batch as
``render_rays(render_testing=True)`` returns them (rays.rendering_metrics applies).  The sampler (rays.ray_view_stats_bank) reads the
views through a device table of pointers, oldest first, so the summation order is the one-shot path's: for at most 128 views held a
render is the one-shot packed sampler's bits over the same maps; beyond, the one-pass variance differs from the generic kernel's two-pass
one by rounding.  In a window a chunk's bank segment leaves with its state.  Renders and evictions go out on one stream (rays.ViewBank).

``nerfdet.begin_scenes([img_meta_0, ...])`` returns a :class:`SceneGroup`: up to 64 scenes with a state each, fed and finished together -- one
backbone pass, one guard read and one grouped accumulate per ``add_views`` call over one chunk per listed scene (ops.scene_accumulate_group),
one grouped density finish, one sigma-MLP call and one grouped volume finish per ``detect`` (ops.density_finish_group / volume_finish_group), then
neck_3d and the tails scene by scene, all queued before the host waits.  Each scene's state holds the bits
``ops.scene_accumulate`` leaves for that scene alone; a group of one scene is a ``SceneStream`` bit for bit.

``nerfdet.begin_scenes(metas, keep_views=True)`` (windowed or not) gives every scene of the group a view bank that follows its states
(``group.banks``): ``group.render_rays(ray_o, ray_d, scenes=None, batched=False)`` and ``group.render(ray_batches, ...)`` render the listed
scenes with ONE sampler launch per pass over all their banks (rays.ray_view_stats_bank_group), every scene bit for bit what a
``SceneStream`` holding the same maps renders; ``batched=True`` also runs the NeRF MLP and the compositing once per pass (shared fp16-pair
scales: masks bit-equal, rgb to 1e-4, depth to 1e-4 x far).  4 (hf wf cm + 4 H W) + 64 bytes a view held and scene; one stream for
renders and evictions (rays.ViewBank).

``nerfdet.begin_scenes(metas, window=S)`` gives every scene of the group a sliding window of S chunks: each listed scene's chunk fills a
state of its own through the same grouped accumulate (ops.scene_accumulate_group_ring), scenes evict independently, and ``detect`` finishes
the listed scenes' windows with one grouped density ring finish, one sigma-MLP call and one grouped volume ring finish
(ops.density_finish_group_ring / volume_finish_group_ring), whose outputs are the single-scene ring finishes' bit for bit.

``scene.add_frames(frames, img_meta)`` / ``group.add_frames(frames, metas, scenes=None)`` take frames at CAPTURE resolution, uint8 BGR
(1 or len(scenes), k, Hs, Ws, 3) on the device, instead of prepared tensors: the frames are checked against the scene's meta (``ori_shape``,
``img_shape``, ``pad_shape``: pipeline.frame_meta), resized, normalised and padded in ONE launch for the whole call (pipeline.prepare_frames,
ndet_resize_normalize_views; ``mean`` / ``std`` are ``begin_scene(s)`` keywords) and handed to ``add_views``, which does the rest.
``format="nv12"`` (an explicit keyword, never inferred from the rank) on ``add_frames`` and ``score_frames`` takes a hardware video
decoder's NV12 surfaces (1 or len(scenes), k, rows, pitch) instead, with ``uv_row=`` the row where the U,V plane starts: the same one
launch converts inside the resize taps (ndet_resize_normalize_views_nv12), bit-equal to ``datasets.nv12_to_bgr`` followed by the BGR road.

``scene.render_frames(c2w= | extrinsic=)`` / ``group.render_frames(...)`` are the output side in the same formats: the rays of k camera poses
come from one launch (pipeline.camera_rays, ndet_camera_rays -- a pose needs no frame), go through ``render_rays``' passes, and one launch
packs the result into (k, h, w, 3) uint8 BGR and (k, h, w) uint16 millimetre frames beside the float outputs (pipeline.pack_frames; depth 0
is a hole); ``window`` crops, ``stride`` makes a thumbnail.  ``score_frames(frames, meta, depth_frames=)`` compares such a render with
held-out capture-resolution frames on the device (pipeline.frame_errors: integer sums per frame and their PSNR; with ``ssim=True`` also
pipeline.frame_ssim: the SSIM per frame from one fused window kernel) and adds nothing to the scene.

``scene.draw_detections(frames, result, c2w= | extrinsic=)`` / ``label_detections(depth_frames, result, ...)`` (and the group's, with one
list per listed scene) put a detection result into the camera's image: the kept boxes' corners go up in one upload, one launch projects
them (pipeline.project_boxes, ndet_project_boxes), one draws their wireframes onto frames that lie in device memory (pipeline.draw_boxes,
ndet_draw_boxes: new frames, the best detection on top) or says which detection each pixel of a depth frame belongs to
(pipeline.label_frames, ndet_label_frames).  They use the scene's meta only and need no ``keep_views``.  ``draw_detections(...,
depth_frames=, occluded=, depth_bias=, text=, text_scale=)`` depth-tests the edges against millimetre depth frames and writes class and
score on a plate above each box: one ndet_project_boxes_w and one ndet_draw_overlay (pipeline.draw_overlay) in place of the two launches.

``scene.occupancy(threshold, dilate, outside)`` / ``group.occupancy(..., scenes=)`` make an occupancy grid (rays.OccupancyGrid) from the
finishes ``volume()`` runs -- the sigma-MLP's alpha at the lattice is the expression compositing applies to a sample -- and
``skip_empty=`` on ``render_rays``, ``render``, ``render_frames`` and ``score_frames`` leaves out the samples the grid calls empty: per pass
one count launch over all samples for the ray mask (rays.ray_view_count_bank), one ordered cull (rays.cull_points, one read), sampler and
MLP over the kept rows only, and the compositing over the same ray ranges with the culled samples at sigma = 0, an exact no-op.  The
default ``skip_empty=None`` makes the launches and the bits it made without the keyword.

``early_stop=`` on the same four calls, alone or with ``skip_empty``, walks every pass front to back in segments of a few samples and
stops a ray once its transmittance is below ``eps``: a transmittance per ray advanced over each finished segment
(rays.advance_transmittance), the live rays' samples of the next one compacted in order (rays.front_segment, through the grid in the same
launch; one read), sampler and MLP over those rows only.  What lies behind the first opaque surface composites as sigma = 0; the result
is the plain pieces' with those rows zeroed, within ``eps`` of the plain render.  The default ``early_stop=None`` changes nothing.

Inference only: no training / autograd, no hipGraph replay, one scene per stream; whole chunks are dropped, not single views out of one.
Without ``keep_views`` there is no ray branch (rendering needs every view's map).
"""
from __future__ import annotations

import functools
from collections import OrderedDict
from typing import List, Optional

import numpy as np
import torch

from . import conv3d, ops, pipeline
from .pipeline import (FRAME_FORMATS, IMG_MEAN, IMG_STD, _host_matrices, camera_rays, check_window, class_palette, depth_to_mm, draw_boxes, frame_errors,
                       SSIM_WINDOW, frame_ssim, label_frames, pack_frames, prepare_depth_frames, prepare_frames, project_boxes, rescale_size,
                       surface_layout)
from .volume import map_features_2d, map_features_2d_hip

Tensor = torch.Tensor


def _norm_cfg(mean, std):
    """``begin_scene(s)``'s img-norm ``mean`` / ``std`` (RGB) as tuples of three floats, ``std`` positive; else ValueError."""
    mean, std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
    if len(mean) != 3 or len(std) != 3 or min(std) <= 0.0:
        raise ValueError(f"mean and std must hold three values each, std positive; got {mean} and {std}")
    return mean, std


def check_chunk_meta(scene_meta: dict, img_meta: dict, k: int) -> None:
    """A chunk's meta against its scene's: same intrinsic, origin, img_shape and ori_shape, and k extrinsics (else ValueError)."""
    a, b = scene_meta, img_meta
    for key in ("intrinsic", "origin"):
        if not np.array_equal(np.asarray(a["lidar2img"][key], dtype=np.float64), np.asarray(b["lidar2img"][key], dtype=np.float64)):
            raise ValueError(f"add_views: the chunk's lidar2img.{key} differs from the scene's")
    for key in ("img_shape", "ori_shape"):
        if tuple(a[key]) != tuple(b[key]):
            raise ValueError(f"add_views: the chunk's {key} {tuple(b[key])} differs from the scene's {tuple(a[key])}")
    if len(b["lidar2img"]["extrinsic"]) != k:
        raise ValueError(f"add_views: {len(b['lidar2img']['extrinsic'])} extrinsics for {k} views")


def check_frames_meta(scene_meta: dict, frames: Tensor, n: int, format: str = "bgr", uv_row=None):
    """``add_frames``'s own checks, before any device work: ``frames`` is (n, k, Hs, Ws, 3) uint8 with ``(Hs, Ws)`` the scene's
    ``ori_shape``, and the scene's ``img_shape`` is what ``Resize(keep_ratio=True)`` into the ``pad_shape`` box makes of such a frame
    (pipeline.rescale_size; a meta without ``pad_shape`` is unpadded: ``pad_shape = img_shape``).  ``format="nv12"``: ``frames`` is
    (n, k, rows, pitch) uint8, a video decoder's surfaces whose Y plane is the scene's ``ori_shape`` -- which must be even -- and whose
    U,V plane starts at row ``uv_row`` (None: Hs); rows and pitch must hold both planes (pipeline.surface_layout).  Returns
    ``(img_scale, pad_size)`` as pipeline.prepare_frames takes them, else ValueError."""
    if format not in FRAME_FORMATS:
        raise ValueError(f"add_frames: format={format!r} must be one of {FRAME_FORMATS}")
    if format == "nv12":
        if frames.dim() != 4 or frames.shape[0] != n or 0 in frames.shape or frames.dtype != torch.uint8:
            raise ValueError(f"add_frames takes NV12 surfaces as uint8 ({n}, k, rows, pitch); got {tuple(frames.shape)} {frames.dtype}")
        hs, ws = (int(v) for v in scene_meta["ori_shape"][:2])
        if hs % 2 or ws % 2:
            raise ValueError(f"add_frames: NV12 surfaces have even sizes, the scene's ori_shape is {tuple(scene_meta['ori_shape'])}")
        surface_layout(int(frames.shape[2]), int(frames.shape[3]), (hs, ws), uv_row, "add_frames")
    else:
        if uv_row is not None:
            raise ValueError("add_frames: uv_row= describes NV12 surfaces (format='nv12')")
        if frames.dim() != 5 or frames.shape[0] != n or frames.shape[1] < 1 or frames.shape[-1] != 3 or frames.dtype != torch.uint8:
            raise ValueError(f"add_frames takes raw uint8 BGR frames ({n}, k, Hs, Ws, 3); got {tuple(frames.shape)} {frames.dtype}")
        hs, ws = int(frames.shape[2]), int(frames.shape[3])
        if (hs, ws) != tuple(scene_meta["ori_shape"][:2]):
            raise ValueError(f"add_frames: frames of {(hs, ws)} differ from the scene's ori_shape {tuple(scene_meta['ori_shape'])}")
    img_shape = tuple(scene_meta["img_shape"][:2])
    h, w = tuple(scene_meta.get("pad_shape", scene_meta["img_shape"])[:2])
    if rescale_size((hs, ws), (w, h)) != img_shape:
        raise ValueError(f"add_frames: a {(hs, ws)} frame rescales to {rescale_size((hs, ws), (w, h))} inside pad_shape {(h, w)}, "
                         f"not to the scene's img_shape {img_shape}")
    return (w, h), (h, w)


def _surface_kwargs(scene_meta: dict, format: str, uv_row) -> dict:
    """What pipeline.prepare_frames needs beyond the frames of a checked call: nothing for BGR frames, the surfaces' description for NV12."""
    return {} if format == "bgr" else dict(format=format, size=tuple(scene_meta["ori_shape"][:2]), uv_row=uv_row)


def check_depth_frames(depth_frames, depth, n: int, k: int) -> None:
    """``add_frames(depth_frames=)``'s own checks, on the descriptor only: None, or contiguous (n, k, Hd, Wd) uint16 on the GPU and no
    ``depth`` beside it, else ValueError."""
    if depth_frames is None:
        return
    if depth is not None:
        raise ValueError("add_frames: depth_frames and depth exclude each other (depth_frames is resized into the call's depth)")
    if (depth_frames.dim() != 4 or depth_frames.dtype != torch.uint16 or tuple(depth_frames.shape[:2]) != (n, k) or 0 in depth_frames.shape
            or not depth_frames.is_contiguous() or not depth_frames.is_cuda):
        raise ValueError(f"add_frames takes depth_frames as contiguous uint16 millimetres ({n}, {k}, Hd, Wd) on the GPU; got "
                         f"{tuple(depth_frames.shape)} {depth_frames.dtype} on {depth_frames.device}")


def _check_pad_shape(scene_meta: dict, img_meta: dict) -> None:
    if "pad_shape" in img_meta and tuple(img_meta["pad_shape"]) != tuple(scene_meta.get("pad_shape", scene_meta["img_shape"])):
        raise ValueError(f"add_frames: the chunk's pad_shape {tuple(img_meta['pad_shape'])} differs from the scene's")


def _check_n_importance(n_importance) -> int:
    """The fine samples per ray of a render call: an int in 0 .. 256 (k_importance_merge's limit), else ValueError."""
    if isinstance(n_importance, bool) or not isinstance(n_importance, int) or not 0 <= n_importance <= 256:
        raise ValueError(f"n_importance={n_importance!r} must be an int in 0 .. 256")
    return n_importance


def _render_dict(coarse, fine):
    """``render_rays``'s result of one scene: ``(rgb, depth, mask)`` of the coarse pass and of the fine pass (None without one)."""
    keys = ("rgb", "depth", "mask")
    if fine is None:
        return OrderedDict(zip(keys, coarse))
    out = OrderedDict(zip(keys, fine))
    out["coarse"] = OrderedDict(zip(keys, coarse))
    return out


def _camera_poses(c2w, extrinsic, what: str) -> np.ndarray:
    """The k >= 1 poses of a ``render_frames`` call as (k,4,4) float32 camera-to-world matrices: exactly one of ``c2w`` (taken as given) and
    ``extrinsic`` (world-to-camera, as a chunk meta carries them: inverted on the host in float64, then rounded to float32); else ValueError."""
    if (c2w is None) == (extrinsic is None):
        raise ValueError(f"{what} takes exactly one of c2w (camera-to-world) and extrinsic (world-to-camera)")
    if c2w is not None:
        return _host_matrices(c2w, f"{what}: c2w").astype(np.float32)
    return np.linalg.inv(_host_matrices(extrinsic, f"{what}: extrinsic").astype(np.float64)).astype(np.float32)


def _scene_intrinsic(meta: dict) -> np.ndarray:
    """The scene meta's intrinsics at the scale of its ``img_shape``: rows 0 and 1 divided by ``ori_shape[0] / img_shape[0]`` in float32, as
    pipeline.MultiViewPipeline forms the target views' ``krows`` (multi_view.py:113-114)."""
    k = np.array(meta["lidar2img"]["intrinsic"], dtype=np.float32)
    k[:2] = k[:2] / (meta["ori_shape"][0] / meta["img_shape"][0])
    return k


def _frame_grid(meta: dict, window, stride):
    """``((y0, x0, h, w), stride)`` of a ``render_frames`` call.  ``window=None``: the content region of the meta's ``img_shape`` -- with
    ``stride=s`` the pixels ``s // 2, s // 2 + s, ...`` inside it on both axes (a thumbnail).  ValueError for anything that leaves no pixel."""
    if window is None:
        _, stride = check_window((0, 0, 1, 1), stride)
        hr, wr = int(meta["img_shape"][0]), int(meta["img_shape"][1])
        o = stride // 2
        if o >= hr or o >= wr:
            raise ValueError(f"stride={stride} leaves no pixel of the {(hr, wr)} content region")
        window = (o, o, (hr - o + stride - 1) // stride, (wr - o + stride - 1) // stride)
    return check_window(window, stride)


def _frames_dict(coarse, fine, shape):
    """``render_frames``'s result of one scene: per pass ``frames``, ``depth_frames`` (pipeline.pack_frames) and the float ``rgb`` (k,h,w,3),
    ``depth``, ``mask`` (k,h,w) they were packed from -- of the fine pass, with the coarse pass's under ``'coarse'``, when there was one."""
    k, h, w = shape

    def one(rgb, depth, mask):
        frames, depth_frames = pack_frames(rgb, depth, mask, shape)
        return OrderedDict(frames=frames, depth_frames=depth_frames, rgb=rgb.view(k, h, w, 3), depth=depth.view(k, h, w), mask=mask.view(k, h, w))

    if fine is None:
        return one(*coarse)
    out = one(*fine)
    out["coarse"] = one(*coarse)
    return out


def _held_out(frames: Tensor, depth_frames, meta: dict, img_scale, pad_size, mean, std, grid, surf: dict = {}):
    """The held-out side of ``score_frames``: ``frames`` (n, Hs, Ws, 3) -- or NV12 surfaces (n, rows, pitch) described by ``surf``
    (:func:`_surface_kwargs`) -- through pipeline.prepare_frames' resized bytes, cropped to the content
    region and strided like the render -- (n, h, w, 3) uint8 -- and ``depth_frames`` (n, Hd, Wd) or None through
    pipeline.prepare_depth_frames at the content size, strided the same way and quantised by pipeline.depth_to_mm -- (n, h, w) uint16."""
    (y0, x0, h, w), s = grid
    hr, wr = int(meta["img_shape"][0]), int(meta["img_shape"][1])
    u8 = prepare_frames(frames, img_scale, pad_size, mean, std, want_u8=True, **surf)[2]
    held = u8[:, y0:hr:s, x0:wr:s].contiguous()
    assert tuple(held.shape[1:3]) == (h, w)
    if depth_frames is None:
        return held, None
    return held, depth_to_mm(prepare_depth_frames(depth_frames, (hr, wr))[:, y0::s, x0::s].contiguous())


def _kept_detections(result, score_thr, palette, what: str):
    """What of one scene's detection result (``detect()[0]``: ``boxes_3d``, ``scores_3d``, ``labels_3d`` on the host) goes to the device:
    ``(kept (m,) int64 indices in boxes.drawing_order, their boxes (m,7) float32, their colours (m,3) uint8)`` -- the colour of a box is its
    label's row of ``palette`` ((c,3) uint8; None: pipeline.class_palette).  ValueError for anything else."""
    from .boxes import drawing_order
    if not isinstance(result, dict) or not all(key in result for key in ("boxes_3d", "scores_3d", "labels_3d")):
        raise ValueError(f"{what} takes one scene's result as detect() returns it: dict(boxes_3d, scores_3d, labels_3d)")
    boxes = getattr(result["boxes_3d"], "tensor", result["boxes_3d"])
    boxes = boxes.detach().cpu().numpy() if isinstance(boxes, Tensor) else np.asarray(boxes)
    scores, labels = (t.detach().cpu().numpy() if isinstance(t, Tensor) else np.asarray(t) for t in (result["scores_3d"], result["labels_3d"]))
    if boxes.ndim != 2 or boxes.shape[1] != 7 or scores.shape != (boxes.shape[0],) or labels.shape != scores.shape or labels.dtype.kind not in "iu":
        raise ValueError(f"{what}: a result holds (n,7) boxes, (n,) scores and (n,) integer labels, got {boxes.shape}, {scores.shape}, "
                         f"{labels.shape} {labels.dtype}")
    if not isinstance(score_thr, (int, float, np.floating, np.integer)) or isinstance(score_thr, bool) or score_thr != score_thr:
        raise ValueError(f"{what}: score_thr={score_thr!r} must be a number")
    if palette is not None:
        palette = palette.detach().cpu().numpy() if isinstance(palette, Tensor) else np.asarray(palette)
        if palette.ndim != 2 or palette.shape[0] < 1 or palette.shape[1] != 3 or palette.dtype != np.uint8:
            raise ValueError(f"{what}: palette must be (c, 3) uint8 BGR, got {palette.shape} {palette.dtype}")
    kept = drawing_order(scores, score_thr)
    lab = labels[kept].astype(np.int64)
    if len(lab) and (lab.min() < 0 or (palette is not None and lab.max() >= palette.shape[0])):
        raise ValueError(f"{what}: labels {int(lab.min())} .. {int(lab.max())} do not index the palette")
    if palette is None:
        palette = class_palette(int(lab.max()) + 1 if len(lab) else 1)
    return kept, np.ascontiguousarray(boxes[kept], dtype=np.float32), np.ascontiguousarray(palette[lab])


def _detection_grid(meta: dict, window, stride, capture, what: str):
    """``(intrinsic, (y0, x0, h, w), stride)`` of a ``draw_detections`` / ``label_detections`` call: the render grid of ``render_frames``
    (:func:`_frame_grid`, :func:`_scene_intrinsic`), or with ``capture=True`` the whole frame at ``ori_shape`` with the meta's intrinsics
    unscaled -- a window or a stride is refused there."""
    if not isinstance(capture, bool):
        raise ValueError(f"{what}: capture must be a bool, got {capture!r}")
    if not capture:
        return (_scene_intrinsic(meta),) + _frame_grid(meta, window, stride)
    if window is not None or isinstance(stride, bool) or stride != 1:
        raise ValueError(f"{what}: capture=True takes whole frames at ori_shape {tuple(meta['ori_shape'][:2])}: no window, stride 1")
    return np.array(meta["lidar2img"]["intrinsic"], dtype=np.float32), (0, 0, int(meta["ori_shape"][0]), int(meta["ori_shape"][1])), 1


def _plan_detections(det, meta: dict, frames, trailing: tuple, dtype, result, c2w, extrinsic, window, stride, capture, score_thr, palette, what: str):
    """Every check of one scene's ``draw_detections`` / ``label_detections`` call, before any launch: the frames' shape and dtype against
    the grid and the poses, the result, the grid.  Returns what the launches need."""
    if det.training:
        raise RuntimeError(f"{what} is inference only: call det.eval() first")
    intrinsic, win, stride = _detection_grid(meta, window, stride, capture, what)
    poses = _camera_poses(c2w, extrinsic, what)                # validates the pair; camera-to-world
    shape = (poses.shape[0], win[2], win[3]) + trailing
    if not isinstance(frames, Tensor) or frames.dtype != dtype or tuple(frames.shape) != shape or not frames.is_contiguous():
        got = f"{tuple(frames.shape)} {frames.dtype}" if isinstance(frames, Tensor) else type(frames).__name__
        raise ValueError(f"{what} takes {poses.shape[0]} frames as a contiguous {shape} {dtype} tensor for this grid, got {got}")
    kept, boxes, colours = _kept_detections(result, score_thr, palette, what)
    if len(kept) > 32767:
        raise ValueError(f"{what}: {len(kept)} detections kept; an int16 label holds 32767")
    return dict(frames=frames, intrinsic=intrinsic, window=win, stride=stride, poses=poses, c2w=c2w, extrinsic=extrinsic, kept=kept, boxes=boxes,
                colours=colours)


def _need_device_frames(plans, what: str) -> None:
    if any(not p["frames"].is_cuda for p in plans):
        raise RuntimeError(f"{what}: the frames must live on the GPU (no CPU fallback)")


def _plan_overlay(p: dict, result, depth_frames, occluded, depth_bias, text, text_scale, what: str) -> None:
    """The checks of ``draw_detections``' depth test and text plates for one scene's checked plan, before any launch; ``p["overlay"]``
    becomes None (both absent: the two launches of old) or ``pipeline.draw_overlay``'s keywords, the texts in drawing order."""
    pipeline.check_overlay_options(occluded, depth_bias, text_scale, what)
    shape = tuple(p["frames"].shape[:3])
    d = depth_frames
    if d is not None and (not isinstance(d, Tensor) or d.dtype != torch.uint16 or tuple(d.shape) != shape or not d.is_contiguous()):
        got = f"{tuple(d.shape)} {d.dtype}" if isinstance(d, Tensor) else type(d).__name__
        raise ValueError(f"{what} takes depth_frames on the frames' own grid, a contiguous {shape} uint16 tensor (millimetres), got {got}")
    texts = None
    if text is not None:
        names = None if text is True else text
        if text is False or (names is not None and (isinstance(names, str) or not isinstance(names, (list, tuple))
                                                    or not all(isinstance(s, str) for s in names))):
            raise ValueError(f"{what}: text must be None, True (the label's number) or a list of class names, got {text!r}")
        kept = p["kept"]
        scores, labels = (np.asarray(t.detach().cpu() if isinstance(t, Tensor) else t)[kept] for t in (result["scores_3d"], result["labels_3d"]))
        if names is not None and len(labels) and int(labels.max()) >= len(names):
            raise ValueError(f"{what}: label {int(labels.max())} has no name among the {len(names)} given")
        texts = [f"{int(lab) if names is None else names[int(lab)]} {float(s):.2f}" for lab, s in zip(labels, scores)]
    p["overlay"] = None if d is None and text is None else dict(depth_frames=d, occluded=occluded, depth_bias=depth_bias, texts=texts,
                                                                  text_scale=text_scale)


def _need_device_depth(plans, what: str) -> None:
    for p in plans:
        d = p["overlay"]["depth_frames"] if p["overlay"] else None
        if d is not None and (not d.is_cuda or d.device != p["frames"].device):
            raise RuntimeError(f"{what}: the depth frames must live on the frames' GPU (no CPU fallback)")


def _draw_plan(p: dict, thickness: int) -> dict:
    """One scene's ``draw_detections`` from its checked plan: one ndet_project_boxes and one ndet_draw_boxes launch -- with a depth test or
    text plates one ndet_project_boxes_w (ndet_project_boxes without depth frames) and one ndet_draw_overlay -- or none when no detection
    is kept."""
    from .boxes import box_corners
    frames, k = p["frames"], p["poses"].shape[0]
    kept = torch.from_numpy(p["kept"])
    if len(p["kept"]) == 0:
        return OrderedDict(frames=frames.clone(), rect=torch.empty((k, 0, 4), dtype=torch.int32, device=frames.device),
                           zrange=torch.empty((k, 0, 2), dtype=torch.float32, device=frames.device), kept=kept)
    over = p.get("overlay")
    proj = project_boxes(p["intrinsic"], box_corners(p["boxes"]), p["window"], p["stride"], c2w=p["c2w"], extrinsic=p["extrinsic"],
                         device=frames.device, depths=over is not None and over["depth_frames"] is not None)
    drawn = draw_boxes(frames, proj, p["colours"], thickness) if over is None else pipeline.draw_overlay(frames, proj, p["colours"], thickness, **over)
    return OrderedDict(frames=drawn, rect=proj["rect"], zrange=proj["zrange"], kept=kept)


def _label_plan(p: dict) -> Tensor:
    """One scene's ``label_detections`` from its checked plan: one ndet_label_frames launch, or a frame of -1 when no detection is kept."""
    from .boxes import box_frames
    if len(p["kept"]) == 0:
        return torch.full(p["frames"].shape, -1, dtype=torch.int16, device=p["frames"].device)
    return label_frames(p["frames"], p["intrinsic"], p["poses"], box_frames(p["boxes"]), p["window"], p["stride"])


def _check_thickness(thickness, what: str) -> int:
    if isinstance(thickness, bool) or thickness not in (1, 3, 5):
        raise ValueError(f"{what}: thickness={thickness!r} must be 1, 3 or 5")
    return int(thickness)


def _render_views(coarse, fine, shape, gt_rgb, gt_depth):
    """``render``'s result of one scene (render_ray.py:452-517), ``outputs_fine`` beside ``outputs_coarse`` when there was a fine pass."""
    t, hh, ww = shape
    out = {"outputs_coarse": {"rgb": coarse[0].view(t, hh, ww, 3), "depth": coarse[1].view(t, hh, ww, 1)},
           "gt_rgb": gt_rgb.view(t, hh, ww, 3),
           "gt_depth": gt_depth.view(t, hh, ww, 1) if gt_depth is not None else None}
    if fine is not None:
        out["outputs_fine"] = {"rgb": fine[0].view(t, hh, ww, 3), "depth": fine[1].view(t, hh, ww, 1)}
    return out


# ---- what SceneStream and SceneGroup share: a stream is a group of one scene bit for bit because both run these bodies ----
def _chunk_features(det, lin, img: Tensor, img_shape):
    """The backbone and FPN on a call's views under the range guard of the fp16-pair arithmetic: the guard word is cleared, read back once
    after the backbone (a synchronisation), and a tripped call is redone on bf16x3 (``conv3d.guard_trips`` counts it).  Returns ``(feat,
    mapped, stride)``: the feature map and its ``lin`` image (the FPN's own when it made one), channels-last, cropped to ``img_shape // stride``."""
    def features():
        x, _, stride = det.extract_2d(img)
        return x, getattr(x, "_ndet_feature_2d", None), stride

    guarded = conv3d.ARITHMETIC == "f16x2" and img.is_cuda
    if guarded:
        conv3d.guard_begin(img.device)
    x, f2d, stride = features()
    if guarded and conv3d.guard_tripped(img.device):
        conv3d.guard_trips += 1
        prev = conv3d.set_arithmetic("bf16x3")
        try:
            x, f2d, stride = features()
        finally:
            conv3d.set_arithmetic(prev)
    h, w = img_shape[0] // stride, img_shape[1] // stride
    feat = ops.to_channels_last(x)[:, :, :h, :w]
    if f2d is not None:
        mapped = f2d[:, :, :h, :w]
    elif lin.in_features % 32 == 0:
        mapped = map_features_2d_hip(feat, lin)
    else:
        mapped = map_features_2d(feat, lin.weight, lin.bias)
    return feat, mapped, stride


def _prepared_frames(frames: Tensor, depth_frames, depth, img_shape, img_scale, pad_size, mean, std, surf: dict = {}):
    """``add_frames``' device work for the (n, k) frames of a call: ONE ndet_resize_normalize_views launch over all of them (NV12
    surfaces described by ``surf``, :func:`_surface_kwargs`: ONE ndet_resize_normalize_views_nv12 launch) and, with
    ``depth_frames`` (n, k, Hd, Wd), ONE ndet_depth_frames launch.  Returns ``(img, denorm_images, depth)`` shaped (n, k, ...) as
    ``add_views`` takes them; without ``depth_frames`` the call's ``depth`` passes through."""
    rows = lambda t: t.reshape((-1,) + tuple(t.shape[2:]))
    chunks = lambda t: t.view(tuple(frames.shape[:2]) + tuple(t.shape[1:]))
    img, denorm = prepare_frames(rows(frames), img_scale, pad_size, mean, std, **surf)
    if depth_frames is not None:
        depth = chunks(prepare_depth_frames(rows(depth_frames), img_shape[:2]))
    return chunks(img), chunks(denorm), depth


def _score_held_out(first: dict, scene_metas, frames: Tensor, chunk_metas, depth_frames, stride, n_importance, mean, std, ssim=False,
                    format: str = "bgr", uv_row=None):
    """Everything ``score_frames`` checks of its own arguments, before any launch, and then its held-out side (:func:`_held_out`) for the
    n listed scenes' rows of k frames at once: ``(held (n k, h, w, 3), held depth (n k, h, w) or None, k, n_importance)``.  ``first``: the
    meta that says what becomes of a frame (a group's scenes share it).  ``ssim``: the call also wants pipeline.frame_ssim, which needs a
    strided content region of at least 7 x 7 pixels."""
    n = len(scene_metas)
    img_scale, pad_size = check_frames_meta(first, frames, n, format, uv_row)
    if len(chunk_metas) != n:
        raise ValueError(f"score_frames: {len(chunk_metas)} chunk metas for {n} listed scenes")
    k = frames.shape[1]
    for scene_meta, m in zip(scene_metas, chunk_metas):
        check_chunk_meta(scene_meta, m, k)
    check_depth_frames(depth_frames, None, n, k)
    n_importance = _check_n_importance(n_importance)
    grid = _frame_grid(first, None, stride)
    if not isinstance(ssim, bool):
        raise ValueError(f"score_frames: ssim must be a bool, got {ssim!r}")
    if ssim and min(grid[0][2], grid[0][3]) < SSIM_WINDOW:
        raise ValueError(f"score_frames: ssim=True needs frames of at least {SSIM_WINDOW} x {SSIM_WINDOW} pixels, stride {grid[1]} leaves "
                         f"{grid[0][2]} x {grid[0][3]}")
    rows = lambda t: t.reshape((n * k,) + tuple(t.shape[2:]))
    held, held_depth = _held_out(rows(frames), None if depth_frames is None else rows(depth_frames), first, img_scale, pad_size, mean, std, grid,
                                 _surface_kwargs(first, format, uv_row))
    return held, held_depth, k, n_importance


def _frame_scores(out: dict, held: Tensor, held_depth, ssim: bool) -> dict:
    """What ``score_frames`` returns for one scene: pipeline.frame_errors of the render ``out`` against the held-out frames and, with
    ``ssim``, pipeline.frame_ssim's ``ssim``, ``ssim_channels`` and ``n_windows`` beside it."""
    scores = frame_errors(out["frames"], held, out["depth_frames"], held_depth)
    if ssim:
        s = frame_ssim(out["frames"], held, out["depth_frames"])
        scores.update(ssim=s["ssim"], ssim_channels=s["ssim_channels"], n_windows=s["n_windows"])
    return scores


def _camera_lists(c2w, extrinsic, what: str) -> list:
    """The cameras of a grouped call: exactly one of ``c2w`` and ``extrinsic``, one list of 4 x 4 matrices per listed scene (else ValueError);
    returns the one given, as a list."""
    if (c2w is None) == (extrinsic is None):
        raise ValueError(f"{what} takes exactly one of c2w (camera-to-world) and extrinsic (world-to-camera)")
    given = c2w if c2w is not None else extrinsic
    if isinstance(given, (Tensor, np.ndarray)) and given.ndim != 4:
        raise ValueError(f"{what} takes one LIST of 4 x 4 matrices per listed scene")
    return list(given)


def _unpack_ray_batch(ray_batch: dict):
    """A ray batch's target views as flat rays (render_ray.py:452-468): ``(ray_o (R,3), ray_d (R,3), (T, h, w), gt_rgb (R,3), gt_depth (R,1)
    or None)``."""
    ray_o, ray_d, gt_rgb, gt_depth = ray_batch["ray_o"], ray_batch["ray_d"], ray_batch["gt_rgb"], ray_batch["gt_depth"]
    nerf_size = ray_batch["nerf_sizes"][0]
    view_num = ray_o.shape[1]
    hh, ww = int(nerf_size[0][0]), int(nerf_size[0][1])
    ray_o, ray_d, gt_rgb = ray_o.view(-1, 3), ray_d.view(-1, 3), gt_rgb.view(-1, 3)
    gt_depth = gt_depth.view(-1, 1) if len(gt_depth) != 0 else None
    assert view_num * hh * ww == ray_o.shape[0]  # render_ray.py:468
    return ray_o, ray_d, (view_num, hh, ww), gt_rgb, gt_depth


def _render_step(det) -> int:
    """The rays per pass of ``render``: the passes of rays.render_rays."""
    from . import rays
    return det.N_rand * max(1, rays.RENDER_TESTING_RAYS // det.N_rand)


def _one_bank_stats(xyz_list, banks):
    """rays.bank_group_stats for ONE bank through the single-bank sampler (k_ray_stats_bank): the same flat ``(globalfeat, pixel_mask,
    view_count, points)``, all views of its outputs and of the points -- nothing is copied."""
    from . import rays
    (xyz,), (bank,) = xyz_list, banks
    glob, pm, vc = rays.ray_view_stats_bank(xyz, bank)
    return glob.view(-1, glob.shape[-1]), pm.view(-1), vc.view(-1), xyz.reshape(-1, 3)


def _render_passes(det, banks, ray_os, ray_ds, step: int, batched: bool, n_importance: int, sampler):
    """render_ray.py:250-327 (``det=True``, mode 'image') over one bank per scene, at most ``step`` rays per scene and pass: per scene
    ``((rgb, depth, mask) of the coarse pass, the same of the fine pass or None)``.  A pass samples every scene that still has rays, runs
    ONE ``sampler`` launch over their banks (rays.bank_group_stats, or :func:`_one_bank_stats` for a stream's one bank) and then the MLP
    and the compositing per scene, or with ``batched`` once over all the pass's samples.  With ``n_importance > 0`` ONE k_importance_merge
    launch over all the pass's rays then gives the fine samples (the kernel is per ray), and the same three steps run over them."""
    from . import rays
    n = len(banks)
    batched = bool(batched) and n > 1 and conv3d.ARITHMETIC != "f32"
    outs = [([], [], []) for _ in range(n)]
    fines = [([], [], []) for _ in range(n)]

    def shade(live, accs, dirs, pts, zs, ss, want_weights):
        """Sampler, MLP and compositing of one pass over ``ss`` samples a ray; appends to ``accs``, returns the rays' weights (R, ss)."""
        mlp = det.nerf_mlp if ss == det.N_samples else (lambda p, d, g: rays.fine_mlp(det.nerf_mlp, p, d, g))
        glob, pm, _, all_pts = sampler(pts, [banks[i] for i in live])
        counts = [p.shape[0] for p in pts]
        if batched and len(live) > 1:
            # one MLP call and one compositing call over the pass: the scenes share linear_rows' per-tensor fp16-pair scales
            rr = sum(counts)
            rgb_pts, density_pts = mlp(all_pts.view(rr, ss, 3), torch.cat(dirs, dim=0), glob.view(rr, ss, -1))
            out = rays.raw2outputs(torch.cat([rgb_pts, density_pts], dim=-1), torch.cat(zs, dim=0), pm.view(rr, ss))
            at = 0
            for i, c in zip(live, counts):
                for acc, key in zip(accs[i], ("rgb", "depth", "mask")):
                    acc.append(out[key][at:at + c])
                at += c
            return out["weights"]
        at, wts = 0, []
        for i, c, d, p, z in zip(live, counts, dirs, pts, zs):
            rows = slice(at * ss, (at + c) * ss)
            rgb_pts, density_pts = mlp(p, d, glob[rows].view(c, ss, -1))
            out = rays.raw2outputs(torch.cat([rgb_pts, density_pts], dim=-1), z, pm[rows].view(c, ss))
            for acc, key in zip(accs[i], ("rgb", "depth", "mask")):
                acc.append(out[key])
            wts.append(out["weights"])
            at += c
        return (wts[0] if len(wts) == 1 else torch.cat(wts, dim=0)) if want_weights else None

    with torch.no_grad():
        for i0 in range(0, max(o.shape[0] for o in ray_os), step):
            live = [i for i in range(n) if ray_os[i].shape[0] > i0]
            origins, dirs, pts, zs = [], [], [], []
            for i in live:
                o, d = ray_os[i][i0:i0 + step], ray_ds[i][i0:i0 + step]
                p, z = rays.sample_along_camera_ray(o, d, det.near_far_range, det.N_samples, det=True)
                origins.append(o)
                dirs.append(d)
                pts.append(p)
                zs.append(z)
            weights = shade(live, outs, dirs, pts, zs, det.N_samples, n_importance > 0)
            if n_importance > 0:
                one = len(live) == 1
                pts_f, z_f, _ = rays.importance_merge(zs[0] if one else torch.cat(zs, dim=0), weights,
                                                      origins[0] if one else torch.cat(origins, dim=0),
                                                      dirs[0] if one else torch.cat(dirs, dim=0), n_importance, True)
                counts = [p.shape[0] for p in pts]
                shade(live, fines, dirs, list(torch.split(pts_f, counts, dim=0)), list(torch.split(z_f, counts, dim=0)),
                      det.N_samples + n_importance, False)
    cat = lambda acc: tuple(a[0] if len(a) == 1 else torch.cat(a, dim=0) for a in acc)
    return [(cat(c), cat(f) if n_importance > 0 else None) for c, f in zip(outs, fines)]


# ---- skip_empty=: renders that leave out the samples an occupancy grid calls empty ----
SKIP_EMPTY_DEFAULTS = dict(threshold=1e-3, dilate=1, outside="keep")


def _check_occupancy_knobs(threshold, dilate, outside):
    """``occupancy``'s three knobs as ``(float threshold, int dilate, outside)``: a finite number, 0 .. 2, 'keep' or 'cull'; else ValueError."""
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.floating, np.integer)) or not np.isfinite(threshold):
        raise ValueError(f"occupancy: threshold={threshold!r} must be a finite number")
    if isinstance(dilate, bool) or not isinstance(dilate, (int, np.integer)) or not 0 <= dilate <= 2:
        raise ValueError(f"occupancy: dilate={dilate!r} must be 0, 1 or 2")
    if outside not in ("keep", "cull"):
        raise ValueError(f"occupancy: outside={outside!r} must be 'keep' or 'cull'")
    return float(threshold), int(dilate), outside


OCCUPANCY_SOURCES = ("alpha", "depth", "both")
CARVE_DEFAULTS = dict(refine=2, band=None)


def _check_source_knobs(source, min_free):
    """``occupancy``'s ``source`` and ``min_free`` as ``(source, int min_free)``: 'alpha', 'depth' or 'both', an int from 1 to 65535; else
    ValueError."""
    if source not in OCCUPANCY_SOURCES:
        raise ValueError(f"occupancy: source={source!r} must be 'alpha', 'depth' or 'both'")
    if isinstance(min_free, bool) or not isinstance(min_free, (int, np.integer)) or not 1 <= min_free <= 65535:
        raise ValueError(f"occupancy: min_free={min_free!r} must be an int from 1 to 65535")
    return source, int(min_free)


def _carve_knobs(carve, det):
    """What a ``carve=`` argument of ``begin_scene`` / ``begin_scenes`` asks for, checked before any device work: None (None or False: no
    carving), or ``(refine, band)`` -- True: ``refine=2`` and the reference gate's band ``voxel_size[2]``; a dict of ``refine`` (1, 2, 4)
    and ``band`` (None, or a finite positive number of metres).  Else ValueError.  ``det.voxel_size`` is read only when a carve is asked for."""
    if carve is None or carve is False:
        return None
    if carve is True:
        carve = {}
    if not isinstance(carve, dict) or not set(carve) <= set(CARVE_DEFAULTS):
        raise ValueError(f"carve={carve!r} must be None, True or a dict with the keys {sorted(CARVE_DEFAULTS)}")
    knobs = dict(CARVE_DEFAULTS, **carve)
    refine, band = knobs["refine"], knobs["band"]
    if isinstance(refine, bool) or not isinstance(refine, (int, np.integer)) or int(refine) not in ops.CARVE_REFINES:
        raise ValueError(f"carve: refine={refine!r} must be 1, 2 or 4")
    if band is None:
        band = float(det.voxel_size[2])
    if isinstance(band, bool) or not isinstance(band, (int, float, np.floating, np.integer)) or not np.isfinite(band) or not band > 0:
        raise ValueError(f"carve: band={band!r} must be None or a finite positive number")
    return int(refine), float(band)


class SceneCarve:
    """One scene's carve (``begin_scene(carve=)``): the fine lattice -- ``ops.get_points(r n_voxels, voxel_size / r, origin)`` -- the band, fixed
    for the scene's life because the counters depend on it, and the rays.CarveStore that follows the scene's states."""

    def __init__(self, det, origin, device, knobs, windowed: bool):
        from .rays import CarveStore
        self.refine, self.band = knobs
        self.n_voxels, self.voxel_size = ops.carve_lattice(det.n_voxels, det.voxel_size, self.refine)
        self.points = ops.get_points(self.n_voxels, self.voxel_size, origin, device)
        self.store = CarveStore(self.n_voxels[0] * self.n_voxels[1] * self.n_voxels[2], device, windowed)

    def chunk(self, gate, rgb_proj: Tensor) -> Tensor:
        """The store's target with a chunk's evidence added: one k_carve_accumulate launch over the chunk's depth gate (its ``depth_r``)
        and stride-1 projections; without a gate nothing is launched (no evidence).  The store itself is not changed."""
        seg = self.store.target()
        if gate is not None:
            try:
                ops.carve_accumulate(seg, self.points, rgb_proj, ops.DepthGate(gate.depth_f, gate.depth_r, self.band))
            except BaseException:
                if not any(seg is s for s in self.store.segments):
                    self.store.give_back(seg)
                raise
        return seg

    def grid(self, min_free: int, dilate: int, outside: str, coarse_bits=None):
        """The rays.OccupancyGrid over the fine lattice of the segments held now: one k_carve_bits call."""
        from .rays import OccupancyGrid
        bits = ops.carve_bits(self.store.segments, self.n_voxels, min_free, dilate, coarse_bits, self.refine)
        return OccupancyGrid(bits, self.n_voxels, self.points[:, 0, 0, 0].cpu(), np.float32(self.voxel_size), outside, None, dilate)


CLOUD_DEFAULTS = dict(refine=2, max_depth=None)


def _cloud_knobs(cloud):
    """What a ``cloud=`` argument of ``begin_scene`` / ``begin_scenes`` asks for, checked before any device work: None (None or False: no
    cloud), or ``(refine, max_depth)`` -- True: ``refine=2`` and no depth limit; a dict of ``refine`` (1, 2, 4) and ``max_depth`` (None, or
    a finite positive number of metres).  Else ValueError."""
    if cloud is None or cloud is False:
        return None
    if cloud is True:
        cloud = {}
    if not isinstance(cloud, dict) or not set(cloud) <= set(CLOUD_DEFAULTS):
        raise ValueError(f"cloud={cloud!r} must be None, True or a dict with the keys {sorted(CLOUD_DEFAULTS)}")
    knobs = dict(CLOUD_DEFAULTS, **cloud)
    refine, max_depth = knobs["refine"], knobs["max_depth"]
    if isinstance(refine, bool) or not isinstance(refine, (int, np.integer)) or int(refine) not in ops.CARVE_REFINES:
        raise ValueError(f"cloud: refine={refine!r} must be 1, 2 or 4")
    ops.check_cloud_max_depth(max_depth)
    return int(refine), (None if max_depth is None else float(max_depth))


def _check_min_points(min_points) -> int:
    if isinstance(min_points, bool) or not isinstance(min_points, (int, np.integer)) or not 1 <= min_points < 2 ** 31:
        raise ValueError(f"points: min_points={min_points!r} must be an int of at least 1")
    return int(min_points)


class SceneCloud:
    """One scene's point cloud (``begin_scene(cloud=)``): the carve's fine lattice -- ``ops.get_points(r n_voxels, voxel_size / r,
    origin)``, of which the first point ``p0`` and the voxel size ``vs`` are kept on the host -- the depth limit, the intrinsics at the scale
    of ``img_shape`` (what ``render_frames`` hands to ``camera_rays``) and the rays.CloudStore that follows the scene's states."""

    def __init__(self, det, meta: dict, device, knobs, windowed: bool):
        from .rays import CloudStore
        self.refine, self.max_depth = knobs
        self.n_voxels, self.voxel_size = ops.carve_lattice(det.n_voxels, det.voxel_size, self.refine)
        self.p0 = tuple(float(v) for v in ops.get_points(self.n_voxels, self.voxel_size, meta["lidar2img"]["origin"], device)[:, 0, 0, 0].cpu())
        self.vs = tuple(float(np.float32(v)) for v in self.voxel_size)
        self.intrinsic = _scene_intrinsic(meta)
        self.pixels = int(meta["img_shape"][0]) * int(meta["img_shape"][1])      # of one view
        self.device = device
        self.store = CloudStore(self.n_voxels[0] * self.n_voxels[1] * self.n_voxels[2], device, windowed)

    def check(self, k: int, with_depth: bool) -> None:
        """What the store refuses for a next chunk of k views (ValueError: 2^24 pixels or more, 64 full segments); no device work."""
        self.store.check(k * self.pixels if with_depth else 0)

    def chunk(self, gate, rgb: Tensor, c2w: np.ndarray) -> tuple:
        """``(segment, pixels)``: the store's target with a chunk's pixels added -- one k_cloud_accumulate launch over the chunk's depth gate
        (its ``depth_r``), its B, G, R planes and its camera-to-world matrices; without a gate nothing is launched.  The store itself is
        not changed."""
        pixels = 0 if gate is None else rgb.shape[0] * self.pixels
        seg = self.store.target(pixels)
        if gate is not None:
            try:
                ops.cloud_accumulate(seg, self.n_voxels, self.p0, self.vs, gate.depth_r, rgb, self.intrinsic, c2w, self.max_depth)
            except BaseException:
                if not any(seg is s for s in self.store.segments):
                    self.store.give_back(seg)
                raise
        return seg, pixels

    def sums(self) -> dict:
        segs = self.store.segments or [torch.zeros((self.store.n, ops.CLOUD_WORDS), dtype=torch.int32, device=self.device)]
        return ops.cloud_sums(segs, self.n_voxels)

    def points(self, min_points, result, score_thr) -> dict:
        """``scene.points``: every check before any launch; ops.cloud_points over the segments held (none held: M = 0 and no launch), and
        with a result one ndet_label_points launch."""
        min_points = _check_min_points(min_points)
        kept = None
        if result is not None:
            kept, boxes, _ = _kept_detections(result, score_thr, None, "points")
            if len(kept) > 32767:
                raise ValueError(f"points: {len(kept)} detections kept; an int16 label holds 32767")
        if self.store.segments:
            out = ops.cloud_points(self.store.segments, self.n_voxels, self.p0, self.vs, min_points)
        else:
            out = dict(xyz=torch.empty((0, 3), dtype=torch.float32, device=self.device), bgr=torch.empty((0, 3), dtype=torch.uint8, device=self.device),
                       count=torch.empty((0,), dtype=torch.int32, device=self.device), voxel=torch.empty((0,), dtype=torch.int32, device=self.device))
        if kept is not None:
            from .boxes import box_frames
            out["ids"] = pipeline.label_points(out["xyz"], box_frames(boxes) if len(kept) else np.zeros((0, 8), dtype=np.float32))
            out["kept"] = torch.from_numpy(kept)
        return out


def _chunk_c2w(img_meta: dict) -> np.ndarray:
    """A chunk meta's extrinsics as (k,4,4) float32 camera-to-world matrices: inverted on the host in float64, then rounded, as
    pipeline.project_boxes does."""
    return _camera_poses(None, img_meta["lidar2img"]["extrinsic"], "cloud")


def _need_cloud(cloud, what: str, call: str = "begin_scene(img_meta, cloud=True)"):
    if cloud is None:
        raise ValueError(f"{what} needs a scene with a point cloud: {call}")


def _need_carve(carve, source: str, what: str):
    if source != "alpha" and carve is None:
        raise ValueError(f"{what}: source={source!r} needs a carved scene: begin_scene(img_meta, carve=True)")


def _grid_refine(grid_n_voxels, n_voxels):
    """r in (1, 2, 4) with ``grid_n_voxels == r * n_voxels`` on all three axes, or None."""
    for r in ops.CARVE_REFINES:
        if tuple(grid_n_voxels) == tuple(r * v for v in n_voxels):
            return r
    return None


def _skip_knobs(skip_empty, det, device, what: str):
    """What a ``skip_empty=`` argument asks for, checked before any launch: None (no culling: None or False), a dict of ``occupancy``'s
    keywords (True: the defaults; ``source`` and ``min_free`` are carried only when given), or the caller's rays.OccupancyGrid, whose
    lattice must be the detector's or refine it by 2 or 4 on all three axes.  Else ValueError."""
    if skip_empty is None or skip_empty is False:
        return None
    from .rays import OccupancyGrid
    if skip_empty is True:
        return dict(SKIP_EMPTY_DEFAULTS)
    if isinstance(skip_empty, OccupancyGrid):
        n_voxels = tuple(int(v) for v in det.n_voxels)
        if _grid_refine(skip_empty.n_voxels, n_voxels) is None:
            raise ValueError(f"{what}: the grid's n_voxels {tuple(skip_empty.n_voxels)} are not 1, 2 or 4 times the scene's {n_voxels}")
        if not skip_empty.bits.is_cuda or skip_empty.bits.device != device:
            raise RuntimeError(f"{what}: the grid's bits must live on the scene's GPU (no CPU fallback)")
        return skip_empty
    if isinstance(skip_empty, dict):
        if not set(skip_empty) <= set(SKIP_EMPTY_DEFAULTS) | {"source", "min_free"}:
            raise ValueError(f"{what}: skip_empty takes the keys {sorted(SKIP_EMPTY_DEFAULTS) + ['min_free', 'source']}, got {sorted(skip_empty)}")
        knobs = dict(SKIP_EMPTY_DEFAULTS, **skip_empty)
        knobs["threshold"], knobs["dilate"], knobs["outside"] = _check_occupancy_knobs(knobs["threshold"], knobs["dilate"], knobs["outside"])
        if "source" in knobs or "min_free" in knobs:
            source, min_free = _check_source_knobs(knobs.get("source", "alpha"), knobs.get("min_free", 2))
            knobs.update({k: v for k, v in (("source", source), ("min_free", min_free)) if k in knobs})
        return knobs
    raise ValueError(f"{what}: skip_empty={skip_empty!r} must be None, True, a dict of occupancy()'s keywords or a rays.OccupancyGrid")


def _check_culled_call(det, what: str, *tensors, keyword: str = "skip_empty") -> None:
    """What a culled (or, ``keyword='early_stop'``, a stopped) render refuses beyond its plain twin: a training detector and CPU tensors
    (RuntimeError), before any launch."""
    if det.training:
        raise RuntimeError(f"{what}({keyword}=) is inference only: call det.eval() first")
    if any(not t.is_cuda for t in tensors):
        raise RuntimeError(f"{what}({keyword}=): the rays must live on the GPU (no CPU fallback)")


def _make_occupancy(alpha: Tensor, valid: Tensor, points: Tensor, n_voxels, voxel_size, threshold: float, dilate: int, outside: str):
    """A scene's rays.OccupancyGrid from its finished alpha (N,), its ``valid`` (1,X,Y,Z) and its lattice ``points`` (3,X,Y,Z): one
    k_occupancy_bits launch and one 12-byte read of the lattice's first point."""
    from .rays import OccupancyGrid
    bits = ops.occupancy_bits(alpha, valid, n_voxels, threshold, dilate)
    return OccupancyGrid(bits, n_voxels, points[:, 0, 0, 0].cpu(), np.float32([float(v) for v in voxel_size]), outside, threshold, dilate)


def _culled_shade(det, bank, occ, dirs: Tensor, pts: Tensor, z: Tensor):
    """Sampler, MLP and compositing of one pass of one scene over the samples ``occ`` keeps: ``pts`` (c, ss, 3), ``z`` (c, ss), ``dirs``
    (c, 3) -> ``(rays.raw2outputs' dict, kept rows)``.  The ray mask comes from the sampler's count pass over ALL the samples
    (rays.ray_view_count_bank: ``seen > 8`` counts them all); the kept rows alone go through the sampler (at most
    ``RENDER_TESTING_RAYS * N_samples`` rows a launch) and ``nerf_mlp`` (at most ``rays.FINE_MLP_ROWS`` rows a call) and are scattered
    into a zero-filled raw -- a zero row is an exact no-op in k_composite -- which is composited over the pass's rays as ever (the depth
    clamp's ``zminmax`` is per pass).  One device-to-host read (rays.cull_points); no kept row: neither sampler nor MLP is launched."""
    from . import rays
    c, ss = pts.shape[:2]
    flat = pts.view(-1, 3)
    pm, _ = rays.ray_view_count_bank(flat, bank)
    idx, kept = rays.cull_points(flat, occ)
    m = idx.shape[0]
    raw = torch.zeros((c * ss, 4), dtype=torch.float32, device=pts.device)
    _shade_rows(det, bank, dirs, ss, idx, kept, raw)
    return rays.raw2outputs(raw.view(c, ss, 4), z, pm.view(c, ss)), m


def _shade_rows(det, bank, dirs: Tensor, ss: int, idx: Tensor, kept: Tensor, raw: Tensor, floor: int = 0) -> None:
    """The kept sample rows ``idx`` (M,) with their points ``kept`` (M, 3) through the bank sampler (at most ``RENDER_TESTING_RAYS *
    N_samples`` rows a launch) and ``nerf_mlp`` (at most ``rays.FINE_MLP_ROWS`` rows a call), with the direction of row f's ray
    ``f // ss``, into the rows ``idx`` of ``raw`` (c ss, 4).  No kept row: nothing is launched.  ``floor``: an MLP call of fewer rows is
    padded up to it (rays.mlp_rows_padded), for callers whose calls can be small."""
    from . import rays
    m = idx.shape[0]
    if not m:
        return
    idx = idx.to(torch.int64)
    kdirs = dirs.to(torch.float32)[idx // ss]
    rows = rays.RENDER_TESTING_RAYS * det.N_samples
    for a in range(0, m, rows):
        glob = rays.ray_view_stats_bank(kept[a:a + rows], bank)[0]
        for b in range(0, glob.shape[0], rays.FINE_MLP_ROWS):
            sl = slice(a + b, a + min(b + rays.FINE_MLP_ROWS, glob.shape[0]))
            rgb, sigma = rays.mlp_rows_padded(det.nerf_mlp, kept[sl], kdirs[sl], glob[b:b + rays.FINE_MLP_ROWS], floor)
            raw.index_copy_(0, idx[sl], torch.cat([rgb, sigma], dim=-1))


def _render_passes_culled(det, bank, occ, ray_o: Tensor, ray_d: Tensor, step: int, n_importance: int, shade=None):
    """:func:`_render_passes` for ONE scene with the samples ``occ`` calls empty left out (:func:`_culled_shade`), over the same ray ranges
    pass by pass: ``((rgb, depth, mask) of the coarse pass, the same of the fine pass or None, kept rows, sample rows)``, the last two
    host ints over every cull of the call.  With ``n_importance > 0`` the coarse weights are the culled coarse pass's (dense, zero where
    culled), rays.importance_merge runs over them and the merged samples are culled, sampled, shaded and composited the same way.
    ``shade(dirs, pts, z)`` replaces :func:`_culled_shade` (:func:`_render_passes_stopped`)."""
    from . import rays
    if shade is None:
        shade = lambda d, pts, z: _culled_shade(det, bank, occ, d, pts, z)
    out, fine = ([], [], []), ([], [], [])
    n_kept = n_samples = 0
    with torch.no_grad():
        for i0 in range(0, ray_o.shape[0], step):
            o, d = ray_o[i0:i0 + step], ray_d[i0:i0 + step]
            pts, z = rays.sample_along_camera_ray(o, d, det.near_far_range, det.N_samples, det=True)
            res, m = shade(d, pts, z)
            n_kept, n_samples = n_kept + m, n_samples + z.numel()
            for acc, key in zip(out, ("rgb", "depth", "mask")):
                acc.append(res[key])
            if n_importance > 0:
                pts_f, z_f, _ = rays.importance_merge(z, res["weights"], o, d, n_importance, True)
                res, m = shade(d, pts_f, z_f)
                n_kept, n_samples = n_kept + m, n_samples + z_f.numel()
                for acc, key in zip(fine, ("rgb", "depth", "mask")):
                    acc.append(res[key])
    cat = lambda acc: tuple(a[0] if len(a) == 1 else torch.cat(a, dim=0) for a in acc)
    return cat(out), cat(fine) if n_importance > 0 else None, n_kept, n_samples


# ---- early_stop=: renders that walk every ray front to back and leave out what lies behind an opaque surface ----
EARLY_STOP_SEGMENTS = (4, 8, 16, 32)
EARLY_STOP_DEFAULTS = dict(eps=1e-3, segment=8)      # segment: the fastest of 8, 16, 32 at the cfg2 frame


def _stop_knobs(early_stop, what: str):
    """What an ``early_stop=`` argument asks for, checked before any launch: None (no stopping: None or False) or ``dict(eps, segment)``
    (True: the defaults; a dict: those of its two keys it names).  ``eps``: a number in [0, 1); ``segment``: 4, 8, 16 or 32.  Else
    ValueError."""
    if early_stop is None or early_stop is False:
        return None
    if early_stop is True:
        return dict(EARLY_STOP_DEFAULTS)
    if not isinstance(early_stop, dict):
        raise ValueError(f"{what}: early_stop={early_stop!r} must be None, True or a dict of the keys {sorted(EARLY_STOP_DEFAULTS)}")
    if not set(early_stop) <= set(EARLY_STOP_DEFAULTS):
        raise ValueError(f"{what}: early_stop takes the keys {sorted(EARLY_STOP_DEFAULTS)}, got {sorted(early_stop)}")
    knobs = dict(EARLY_STOP_DEFAULTS, **early_stop)
    eps, segment = knobs["eps"], knobs["segment"]
    if isinstance(eps, bool) or not isinstance(eps, (int, float, np.floating, np.integer)) or not 0.0 <= float(np.float32(eps)) < 1.0:
        raise ValueError(f"{what}: early_stop's eps={eps!r} must be a number in [0, 1) as a float32")
    if isinstance(segment, bool) or not isinstance(segment, (int, np.integer)) or segment not in EARLY_STOP_SEGMENTS:
        raise ValueError(f"{what}: early_stop's segment={segment!r} must be one of {EARLY_STOP_SEGMENTS}")
    return dict(eps=float(eps), segment=int(segment))


def _stop_checked(det, early_stop, what: str, *tensors, batched: bool = False):
    """The ``dict(eps, segment)`` of an ``early_stop=`` render (None: no stopping) once everything the call refuses has been checked, before
    any launch: bad knobs and ``batched=True`` are a ValueError, a training detector and CPU tensors a RuntimeError."""
    stop = _stop_knobs(early_stop, what)
    if stop is not None:
        if batched:
            raise ValueError(f"{what}: batched=True and early_stop exclude each other for now")
        _check_culled_call(det, what, *tensors, keyword="early_stop")
    return stop


def _front_shade(det, bank, occ, stop: dict, dirs: Tensor, pts: Tensor, z: Tensor):
    """:func:`_culled_shade` walked front to back: ``pts`` (c, ss, 3), ``z`` (c, ss), ``dirs`` (c, 3) -> ``(rays.raw2outputs' dict, kept
    rows)``.  The samples of a ray go in segments of ``stop['segment']`` columns (the last may be shorter).  ``T`` (c,) starts at 1 and is
    advanced over each finished segment (rays.advance_transmittance: k_composite's own exclusive product of the raw built so far); at a
    segment's first column b > 0 a ray with ``T < stop['eps']`` is stopped: its rows from b on are never computed and stay zero, which
    leaves ``T`` where it is, so the ray stays stopped.  rays.front_segment picks the live rays' samples of the segment -- through ``occ``
    as well when there is a grid (None: no culling) -- and they alone go through sampler and MLP (:func:`_shade_rows`).  The ray mask
    comes from the count pass over ALL samples, and the compositing runs over the pass's rays as ever.  One device-to-host read per
    segment; without a grid none for the first (every ray is live), and no live ray ends the walk.  A late segment has few live rows,
    and a ``nerf_mlp`` call of few rows makes other launches than the pass-sized call of the plain render, whose ``rgb`` differs in the
    last bit: such a call is padded to ``min(rays.MLP_STABLE_ROWS, c ss)`` rows (rays.mlp_rows_padded), which keeps the result the
    plain pieces' bit for bit at the price of an MLP call of that size per late segment."""
    from . import rays
    c, ss = pts.shape[:2]
    seg, eps = stop["segment"], stop["eps"]
    pts = pts.to(torch.float32).contiguous()
    pm, _ = rays.ray_view_count_bank(pts.view(-1, 3), bank)
    raw = torch.zeros((c * ss, 4), dtype=torch.float32, device=pts.device)
    T = torch.ones((c,), dtype=torch.float32, device=pts.device)
    kept_rows, floor = 0, min(rays.MLP_STABLE_ROWS, c * ss)
    for s0 in range(0, ss, seg):
        if s0:
            rays.advance_transmittance(raw.view(c, ss, 4), T, s0 - seg, s0)
        idx, kept = rays.front_segment(pts, T, s0, min(s0 + seg, ss), eps, occ, all_live=occ is None and s0 == 0)
        if occ is None and not idx.shape[0]:
            break                                              # every ray has stopped
        _shade_rows(det, bank, dirs, ss, idx, kept, raw, floor)
        kept_rows += idx.shape[0]
    return rays.raw2outputs(raw.view(c, ss, 4), z, pm.view(c, ss)), kept_rows


def _render_passes_stopped(det, bank, occ, stop: dict, ray_o: Tensor, ray_d: Tensor, step: int, n_importance: int):
    """:func:`_render_passes_culled` with every pass shaded front to back (:func:`_front_shade`; ``occ`` None: no grid).  With
    ``n_importance > 0`` the coarse weights are dense, zero where stopped or culled; rays.importance_merge runs over them and the merged
    ``N_samples + k`` samples are segmented again from ``T = 1``."""
    return _render_passes_culled(det, bank, occ, ray_o, ray_d, step, n_importance,
                                 shade=lambda d, pts, z: _front_shade(det, bank, occ, stop, d, pts, z))


def _with_counts(out: dict, counts) -> dict:
    """A render's result with what its culls counted: the unculled call's dict as it is (``counts`` None), else with the host ints
    ``n_kept`` and ``n_samples`` -- sample rows that went through sampler and MLP, and all sample rows, over every cull of the call (the
    fine pass's included)."""
    if counts is not None:
        out["n_kept"], out["n_samples"] = int(counts[0]), int(counts[1])
    return out


def _finished_alpha(mlp, points: Tensor, glob: Tensor) -> Tensor:
    """The sigma-MLP over the density finish's rows and their alpha: the fused trunk where the MLP has one."""
    if hasattr(mlp, "hip_trunk_ok") and mlp.hip_trunk_ok():
        return mlp.alpha_from_points(points, glob)
    return ops.sigma_to_alpha(mlp.raw_sigma_from_rows(ops.posenc_concat(points, glob)))


def _repeat_tails(det, vol: Tensor, valid: Tensor, metas):
    """neck_3d and the tails of a call's scenes once more on bf16x3, from the finished volumes (n,C,X,Y,Z): the scenes of a call share the
    stream's guard word, so a set word says that some launch of the call tripped, not which scene's."""
    conv3d.guard_trips += 1
    prev = conv3d.set_arithmetic("bf16x3")
    try:
        with torch.no_grad():
            n = vol.shape[0]
            x = det.neck_3d(vol)
            return [det._detect_tail(x if n == 1 else [lvl[i:i + 1] for lvl in x], valid[i:i + 1], metas[i], False, False, vol.device, None)
                    for i in range(n)]
    finally:
        conv3d.set_arithmetic(prev)


class _LatticePoints(Tensor):
    """``SceneStream.points`` of one scene: the lattice tensor (3,X,Y,Z) that the attribute has always been -- indexing, ``.cpu()`` and
    every torch function see that tensor and return plain tensors -- which, called, is :meth:`SceneStream.points`, the scene's point
    cloud.  The stream itself works on ``lattice``, the plain tensor that shares its memory."""

    __torch_function__ = torch._C._disabled_torch_function_impl

    def __call__(self, *args, **kwargs):
        return self._cloud_call(*args, **kwargs)


class SceneStream:
    """One scene of a :class:`~nerfdet_amd.detector.nerfdet` detector, filled chunk by chunk (:meth:`add_views`) and detected at any time
    (:meth:`detect`).  ``img_meta`` fixes the scene: ``lidar2img.intrinsic``, ``lidar2img.origin``, ``img_shape`` and ``ori_shape``; its
    extrinsics are not used (each chunk brings its own).  ``window``: None, or the number of chunks kept (1 .. ops.RING_MAX): the
    stream then holds one state per ``add_views`` call and forgets the oldest when a chunk arrives at a full window.  ``keep_views``: also
    keep the views' mapped maps, images and cameras (``bank``, a rays.ViewBank) so that :meth:`render_rays` / :meth:`render` work."""

    bank = None     # rays.ViewBank with keep_views, else None
    _occ = None     # (threshold, dilate, outside[, source, min_free]) -> rays.OccupancyGrid of the views held now, made by occupancy(); dropped by _drop_grids()
    carve = None    # SceneCarve with begin_scene(carve=), else None
    cloud = None    # SceneCloud with begin_scene(cloud=), else None
    mean, std = IMG_MEAN, IMG_STD     # img_norm_cfg of add_frames (RGB)

    def __init__(self, det, img_meta: dict, window: Optional[int] = None, keep_views: bool = False, mean=IMG_MEAN, std=IMG_STD, carve=None,
                 cloud=None):
        self.mean, self.std = _norm_cfg(mean, std)
        if not isinstance(keep_views, bool):
            raise ValueError(f"keep_views must be a bool, got {keep_views!r}")
        if window is not None:
            ops.check_window(window)
        carve = _carve_knobs(carve, det)
        cloud = _cloud_knobs(cloud)
        if det.training:
            raise RuntimeError("SceneStream is inference only: call det.eval() first")
        if det.render_testing and not keep_views:
            raise NotImplementedError("SceneStream does not render rays (render_testing needs every view's feature map): "
                                      "begin_scene(img_meta, keep_views=True) keeps them")
        self.det = det
        self.meta = img_meta
        self.device = next(det.parameters()).device
        lin = det.mapping[0]
        self._lin = lin
        self.window = window
        # unwindowed: one state for the scene.  Windowed: one state per chunk held, oldest first, allocated when first needed; a
        # dropped state is zeroed and kept for a chunk to come, so a sliding window allocates nothing once it has slid once.
        self.state = ops.SceneState(det.n_voxels, lin.in_features, lin.out_features, self.device) if window is None else None
        self._segs: List[ops.SceneState] = []
        self._spare: List[ops.SceneState] = []
        self.lattice = ops.get_points(det.n_voxels, det.voxel_size, img_meta["lidar2img"]["origin"], self.device)
        self.points = self.lattice.as_subclass(_LatticePoints)      # the tensor it has always been; called, the method below
        self.points._cloud_call = functools.partial(SceneStream.points, self)
        if keep_views:
            from .rays import ViewBank
            self.bank = ViewBank()
        if carve is not None:
            self.carve = SceneCarve(det, img_meta["lidar2img"]["origin"], self.device, carve, window is not None)
        if cloud is not None:
            self.cloud = SceneCloud(det, self.meta, self.device, cloud, window is not None)

    @property
    def chunk_views(self) -> List[int]:
        """View counts of the chunks held, oldest first (an unwindowed stream holds its views as one)."""
        if self.window is None:
            return [self.state.n_views] if self.state.n_views else []
        return [st.n_views for st in self._segs]

    @property
    def n_chunks(self) -> int:
        return len(self.chunk_views)

    @property
    def n_views(self) -> int:
        return sum(self.chunk_views)

    def _drop_grids(self) -> None:
        """Whatever changes the views held drops the cached occupancy grids."""
        self._occ = None

    def reset(self) -> None:
        """Forget every view: the scene starts empty again."""
        self._drop_grids()
        if self.window is None:
            self.state.reset()
            if self.bank is not None:
                self.bank.clear()
            if self.carve is not None:
                self.carve.store.clear()
            if self.cloud is not None:
                self.cloud.store.clear()
        else:
            self.drop_oldest(len(self._segs))

    def drop_oldest(self, k: int = 1) -> None:
        """Forget the k oldest chunks of a windowed stream (their states are zeroed and kept for the chunks to come)."""
        if self.window is None:
            raise ValueError("drop_oldest needs a windowed stream: begin_scene(img_meta, window=S)")
        if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k <= len(self._segs):
            raise ValueError(f"drop_oldest: k={k!r} for {len(self._segs)} chunks held")
        self._drop_grids()
        for st in self._segs[:k]:
            st.reset()
            self._spare.append(st)
        del self._segs[:k]
        if self.bank is not None:
            self.bank.drop_oldest(k)
        if self.carve is not None:
            self.carve.store.drop_oldest(k)
        if self.cloud is not None:
            self.cloud.store.drop_oldest(k)

    def _accumulate(self, *chunk, depth_gate=None, banked=None, cloud_c2w=None) -> None:
        """Fold a chunk into the scene's state, or in a window into an empty state that joins the window once it is filled; only then does
        the oldest chunk leave a full window.  A chunk that fails leaves the window as it was (its state goes back, zeroed).  ``banked``:
        the chunk's view-bank segment, made by the caller (rays.ViewBank.make_segment changes nothing); it joins the bank once the
        states have taken the chunk, so states and bank hold the same chunks.  A carved scene's counters (SceneCarve.chunk: the chunk's
        depth gate and stride-1 projection, the last of ``chunk``) follow the same rule: a windowed scene's are made in a spare segment
        beside the state and join the store with it; an unwindowed scene's are added to its one segment once the state has taken the
        chunk.  So do a cloud scene's records (SceneCloud.chunk: the gate's ``depth_r``, the chunk's B, G, R planes -- ``chunk[3]`` -- and
        ``cloud_c2w``, its camera-to-world matrices)."""
        self._drop_grids()
        carve, cloud = self.carve, self.cloud
        if self.window is None:
            ops.scene_accumulate(self.state, *chunk, depth_gate=depth_gate)
            if banked is not None:
                self.bank.push(banked)
            if carve is not None:
                carve.store.push(carve.chunk(depth_gate, chunk[-1]))
            if cloud is not None:
                cloud.store.push(*cloud.chunk(depth_gate, chunk[3], cloud_c2w))
            return
        lin = self._lin
        # a sliding window therefore owns S + 1 states: the chunk that leaves hands its (zeroed) state to the chunk after the next
        st = self._spare.pop() if self._spare else ops.SceneState(self.det.n_voxels, lin.in_features, lin.out_features, self.device)
        cseg = pseg = None
        try:
            ops.scene_accumulate(st, *chunk, depth_gate=depth_gate)
            if carve is not None:
                cseg = carve.chunk(depth_gate, chunk[-1])
            if cloud is not None:
                pseg = cloud.chunk(depth_gate, chunk[3], cloud_c2w)
        except BaseException:
            st.reset()
            self._spare.append(st)
            if cseg is not None:
                carve.store.give_back(cseg)
            raise
        if len(self._segs) == self.window:
            self.drop_oldest(1)
        self._segs.append(st)
        if banked is not None:
            self.bank.push(banked)
        if cseg is not None:
            carve.store.push(cseg)
        if pseg is not None:
            cloud.store.push(*pseg)

    def _check_meta(self, img_meta: dict, k: int) -> None:
        check_chunk_meta(self.meta, img_meta, k)

    def _check_chunk(self, img: Tensor, denorm_images: Tensor, img_meta: dict, depth) -> None:
        """Everything add_views refuses, before anything is launched (only shapes are read)."""
        if img.dim() != 5 or img.shape[0] != 1:
            raise ValueError(f"add_views takes one scene's chunk, (1, k, 3, H, W); got {tuple(img.shape)}")
        k = img.shape[1]
        if k < 1 or denorm_images.shape[:2] != img.shape[:2]:
            raise ValueError(f"add_views: img {tuple(img.shape)} and denorm_images {tuple(denorm_images.shape)} must hold the same k >= 1 views")
        if depth is not None and (depth.dim() != 4 or depth.shape[:2] != img.shape[:2]):
            raise ValueError(f"add_views: depth must be (1, k, Hd, Wd), got {tuple(depth.shape)}")
        self._check_meta(img_meta, k)
        if self.det.training:
            raise RuntimeError("SceneStream is inference only: call det.eval() first")

    def add_frames(self, frames: Tensor, img_meta: dict, depth: Optional[Tensor] = None, depth_frames: Optional[Tensor] = None,
                   format: str = "bgr", uv_row=None) -> None:
        """:meth:`add_views` for k >= 1 frames at CAPTURE resolution: ``frames`` (1, k, Hs, Ws, 3) uint8 BGR on the device -- or, with
        ``format="nv12"``, the NV12 surfaces (1, k, rows, pitch) uint8 a hardware video decoder leaves there: their Y plane is the
        scene's ``ori_shape``, which must be even, their U,V plane starts at row ``uv_row`` (None: Hs, the tight layout), and ONE
        ndet_resize_normalize_views_nv12 launch converts inside the resize taps, which leaves the scene what ``datasets.nv12_to_bgr`` of
        the surfaces would, bit for bit.  The format is never inferred from the rank.  The scene's meta says what becomes of them (pipeline.frame_meta makes such a meta): ``(Hs, Ws)`` must be its
        ``ori_shape``, its ``img_shape`` what ``Resize(keep_ratio=True)`` into the ``pad_shape`` box gives (pipeline.rescale_size;
        ``pad_shape`` absent: ``img_shape``), else ValueError -- raised, like everything :meth:`add_views` refuses, before any device
        work.  One ndet_resize_normalize_views launch then makes the chunk's ``img`` and ``denorm_images`` (1, k, 3, H, W) at the padded
        size -- ``datasets.imresize_linear``'s bytes, normalised with ``mean`` / ``std`` of ``begin_scene`` as ndet_normalize_views does, then
        padded, as the configs' Resize -> Normalize -> Pad -- and :meth:`add_views` takes them: guard, window, bank and the promise that a call that raises changes nothing are its own.  ``depth`` passes through
        (ops.depth_gate resizes it to ``img_shape``).  ``depth_frames`` instead of ``depth``: the sensor's frames (1, k, Hd, Wd) uint16
        millimetres on the device, of any size of their own; one ndet_depth_frames launch makes the float64 metres at the scene's
        ``img_shape`` (pipeline.prepare_depth_frames: ``datasets.imresize_linear(frame / 1000, ...)`` bit for bit), which go to
        :meth:`add_views` as its ``depth``.  Both given, a wrong dtype or another k: ValueError, before any device work."""
        img_scale, pad_size = check_frames_meta(self.meta, frames, 1, format, uv_row)
        _check_pad_shape(self.meta, img_meta)
        k = frames.shape[1]
        check_depth_frames(depth_frames, depth, 1, k)
        shape = torch.empty((1, k, 3) + pad_size, device="meta")
        self._check_chunk(shape, shape, img_meta, depth)
        if self.cloud is not None:
            self.cloud.check(k, depth is not None or depth_frames is not None)
        img, denorm, depth = _prepared_frames(frames, depth_frames, depth, self.meta["img_shape"], img_scale, pad_size, self.mean, self.std,
                                              _surface_kwargs(self.meta, format, uv_row))
        self.add_views(img, denorm, img_meta, depth=depth)

    def add_views(self, img: Tensor, denorm_images: Tensor, img_meta: dict, depth: Optional[Tensor] = None) -> None:
        """Fold k >= 1 views into the scene.  ``img``, ``denorm_images`` (1, k, 3, H, W); ``img_meta`` the chunk's (its ``extrinsic`` list has
        k entries; the rest must equal the scene's, else ValueError); ``depth`` None or (1, k, Hd, Wd) float32 / float64: the chunk's views are
        depth-gated as by ``simple_test(depth=)`` (nerfdet.py:404-411).

        Range guard of the fp16-pair arithmetic: the guard word is cleared before the chunk's backbone and read back before the chunk enters
        the state -- one 4-byte device-to-host read (a synchronisation) per chunk.  A tripped chunk is redone on bf16x3 first
        (``conv3d.guard_trips`` counts it), so no tripped chunk reaches the state."""
        self._check_chunk(img, denorm_images, img_meta, depth)
        cloud_c2w = None
        if self.cloud is not None:
            self.cloud.check(img.shape[1], depth is not None)
            cloud_c2w = _chunk_c2w(img_meta)
        with torch.no_grad():
            lin = self._lin
            hh, ww = self.meta["img_shape"][0], self.meta["img_shape"][1]
            feat, mapped, stride = _chunk_features(self.det, lin, img, (hh, ww))
            rgb = denorm_images[0][:, :, :hh, :ww]
            gate = None
            if depth is not None:
                gate = ops.depth_gate(depth[0].to(self.device, non_blocking=True), self.det.voxel_size, (hh // stride, ww // stride), (hh, ww))
            proj = ops.compute_projection(img_meta, stride, self.device)
            rgb_proj = ops.compute_projection(img_meta, 1, self.device)
            # the bank takes the mapped map as it is accumulated and the images as extract_feat hands them to render_rays (uncropped)
            banked = None if self.bank is None else self.bank.make_segment(mapped, denorm_images[0], img_meta)
            self._accumulate(feat, mapped, lin.bias, rgb, self.lattice, proj, rgb_proj, depth_gate=gate, banked=banked, cloud_c2w=cloud_c2w)

    def _need_bank(self, what: str):
        bank = self.bank
        if bank is None:
            raise RuntimeError(f"{what} needs the scene's views: begin_scene(img_meta, keep_views=True)")
        if bank.n_views == 0:
            raise RuntimeError("the scene has no views yet: call add_views first")
        return bank

    def _render(self, ray_o: Tensor, ray_d: Tensor, step: int, n_importance: int = 0):
        """render_ray.py:250-327 (``det=True``, mode 'image') over the bank, ``step`` rays per pass: ``(rgb, depth, mask)`` of the coarse
        pass and, with ``n_importance > 0``, of the fine pass of ``rays.render_rays_func`` (else None)."""
        bank = self._need_bank("rendering")
        return _render_passes(self.det, [bank], [ray_o], [ray_d], step, False, n_importance, _one_bank_stats)[0]

    def _render_counted(self, ray_o: Tensor, ray_d: Tensor, step: int, n_importance: int, occ, stop=None):
        """``((coarse, fine), counts)``: :meth:`_render` and None without a grid and without ``stop``, else the culled passes
        (:func:`_render_passes_culled`) or, with ``stop``, the front-to-back ones (:func:`_render_passes_stopped`) and their ``(n_kept,
        n_samples)``."""
        if occ is None and stop is None:
            return self._render(ray_o, ray_d, step, n_importance), None
        bank = self._need_bank("rendering")
        if stop is None:
            coarse, fine, n_kept, n_samples = _render_passes_culled(self.det, bank, occ, ray_o, ray_d, step, n_importance)
        else:
            coarse, fine, n_kept, n_samples = _render_passes_stopped(self.det, bank, occ, stop, ray_o, ray_d, step, n_importance)
        return (coarse, fine), (n_kept, n_samples)

    def render_rays(self, ray_o: Tensor, ray_d: Tensor, n_importance: int = 0, skip_empty=None, early_stop=None):
        """Render rays ``ray_o``, ``ray_d`` (R,3) against the views held: ``dict(rgb (R,3), depth (R,), mask (R,) bool)``, what
        ``rays.render_rays_func(det=True)`` composites (render_ray.py:250-327) with the detector's ``near_far_range`` and ``N_samples``,
        ``rays.RENDER_TESTING_RAYS`` rays per pass.  Needs ``keep_views=True`` and at least one view (else RuntimeError).

        ``n_importance=k > 0`` adds the fine pass of ``rays.render_rays_func(N_importance=k)``: k further depths per ray drawn from the
        coarse weights (one k_importance_merge launch a pass), then the sampler, the MLP and the compositing again over the
        ``N_samples + k`` depths.  ``rgb``, ``depth`` and ``mask`` are then the fine pass's, and the dict gains ``'coarse'``:
        ``dict(rgb, depth, mask)`` of the coarse pass, which is what ``n_importance=0`` returns.

        ``skip_empty``: None (the default: every launch and every bit as without the keyword), True (:meth:`occupancy`'s defaults), a
        dict of :meth:`occupancy`'s keywords, or a rays.OccupancyGrid over the scene's lattice.  The samples the grid calls empty are
        then left out: per pass one count launch over all samples keeps the ray mask exact (rays.ray_view_count_bank), one cull
        (rays.cull_points: its read of the kept count is the one synchronisation a pass adds) picks the kept rows, which alone go
        through the sampler and ``nerf_mlp``; the others composite as ``sigma = 0``, an exact no-op in k_composite, over the same ray
        ranges as the unculled passes.  ``mask`` is the unculled call's bit for bit; ``rgb`` and ``depth`` are those of the unculled
        samples with the culled ones' sigma set to 0 -- bit for bit as measured (the MLP's launches scale per row or not at all, so
        regrouping its rows across calls changes nothing).  With ``n_importance > 0`` the fine samples are drawn from the culled coarse weights and culled the
        same way.  The dict gains the host ints ``n_kept`` and ``n_samples``.  Many culled samples each just under the threshold can
        add up along a ray: compare with the plain render (or :meth:`score_frames`) on your own data.  Inference only, not graphed:
        a training detector or CPU rays are a RuntimeError, bad knobs or another lattice's grid a ValueError, before any launch.

        ``early_stop``: None or False (the default: every launch and every bit as without the keyword), True (``eps=1e-3`` and the
        default ``segment``) or ``dict(eps=, segment=)`` with ``0 <= eps < 1`` and ``segment`` 4, 8, 16 or 32; alone or with
        ``skip_empty``.  Every pass is then walked front to back in segments of ``segment`` samples (:func:`_front_shade`): a ray whose
        transmittance -- k_composite's own exclusive product -- is below ``eps`` at a segment's first sample is stopped, and its
        samples from there on are never computed: they composite as ``sigma = 0``.  The result is bit for bit that of the plain
        pieces with those rows (and the grid's) zeroed; ``mask`` is the plain render's.  Against the plain render a stopped ray's
        ``rgb`` moves by less than ``eps`` per channel and its ``depth`` by at most ``eps far / (1 - eps)``; ``eps=0`` stops
        nothing.  The default ``eps`` rests on that bound (a frame byte moves by at most one level), not on a measurement on trained
        weights.  Each segment costs one device-to-host read.  The dict gains ``n_kept`` and ``n_samples``.  Refusals as for
        ``skip_empty``."""
        from . import rays
        self._need_bank("render_rays")
        n_importance = _check_n_importance(n_importance)
        if ray_o.dim() != 2 or ray_o.shape[1] != 3 or ray_d.shape != ray_o.shape:
            raise ValueError(f"render_rays takes (R,3) origins and directions, got {tuple(ray_o.shape)} and {tuple(ray_d.shape)}")
        stop = _stop_checked(self.det, early_stop, "render_rays", ray_o, ray_d)
        occ = self._skip_grid(skip_empty, "render_rays", ray_o, ray_d)
        (coarse, fine), counts = self._render_counted(ray_o, ray_d, rays.RENDER_TESTING_RAYS, n_importance, occ, stop)
        return _with_counts(_render_dict(coarse, fine), counts)

    def render(self, ray_batch: dict, n_importance: int = 0, skip_empty=None, early_stop=None):
        """Every ray of the ray batch's target views, as ``rays.render_rays(render_testing=True)`` returns them (render_ray.py:452-517):
        ``outputs_coarse.rgb`` (T,h,w,3), ``outputs_coarse.depth`` (T,h,w,1), ``gt_rgb``, ``gt_depth`` -- ``rays.rendering_metrics`` applies.
        ``n_importance=k > 0`` adds ``outputs_fine`` (same shapes), as ``rays.render_rays(render_testing=True, N_importance=k)`` does.
        ``skip_empty`` and ``early_stop`` as in :meth:`render_rays` (the dict gains ``n_kept`` and ``n_samples``)."""
        self._need_bank("render")
        n_importance = _check_n_importance(n_importance)
        ray_o, ray_d, shape, gt_rgb, gt_depth = _unpack_ray_batch(ray_batch)
        stop = _stop_checked(self.det, early_stop, "render", ray_o, ray_d)
        occ = self._skip_grid(skip_empty, "render", ray_o, ray_d)
        (coarse, fine), counts = self._render_counted(ray_o, ray_d, _render_step(self.det), n_importance, occ, stop)
        return _with_counts(_render_views(coarse, fine, shape, gt_rgb, gt_depth), counts)

    def render_frames(self, c2w=None, extrinsic=None, window=None, stride: int = 1, n_importance: int = 0, skip_empty=None, early_stop=None):
        """Camera frames of k >= 1 poses against the views held -- pose in, BGR and depth out, in the formats :meth:`add_frames` takes.
        Exactly one of ``c2w`` (k camera-to-world 4 x 4, as ``pipeline.scene_cameras(info)["c2w"]``) and ``extrinsic`` (k world-to-camera
        4 x 4, as a chunk meta carries them: inverted on the host in float64, rounded to float32).  The intrinsics are the scene meta's,
        scaled by ``ori_shape[0] / img_shape[0]`` as pipeline.MultiViewPipeline scales the target views'.  ``window = (y0, x0, h, w)``: the
        h x w output looks through image pixels ``(y0 + i * stride, x0 + j * stride)``; None: the content region of ``img_shape``, with
        ``stride=s`` its pixels ``s // 2, s // 2 + s, ...`` (a thumbnail).  One ndet_camera_rays launch makes all the rays
        (pipeline.camera_rays), which go through :meth:`render_rays`' passes of ``rays.RENDER_TESTING_RAYS``; one ndet_pack_frames launch
        per pass kind makes the frames (pipeline.pack_frames).

        Returns ``dict(frames (k,h,w,3) uint8 BGR, depth_frames (k,h,w) uint16 millimetres, rgb (k,h,w,3), depth (k,h,w), mask (k,h,w))``;
        with ``n_importance > 0`` these are the fine pass's and ``'coarse'`` holds the same five keys for the coarse pass.  The float
        outputs are bit for bit ``self.render_rays(*camera_rays(...))`` on the concatenated rays, reshaped; the frames are
        ``pack_frames`` of them: depth 0 is a hole (``mask`` false), as in the sensor's frames.  Needs ``keep_views=True`` and at least one
        view (else RuntimeError); bad arguments are a ValueError before any launch.  No state and no bank is changed.
        ``skip_empty`` and ``early_stop`` as in :meth:`render_rays`: the frames are ``pack_frames`` of the culled or stopped float
        outputs, and the dict gains ``n_kept`` and ``n_samples``."""
        from . import rays
        self._need_bank("render_frames")
        n_importance = _check_n_importance(n_importance)
        poses = _camera_poses(c2w, extrinsic, "render_frames")
        win, stride = _frame_grid(self.meta, window, stride)
        knobs = _skip_knobs(skip_empty, self.det, self.device, "render_frames")        # refused before the ray launch
        if knobs is not None:
            _check_culled_call(self.det, "render_frames")
        stop = _stop_checked(self.det, early_stop, "render_frames")
        ray_o, ray_d = camera_rays(_scene_intrinsic(self.meta), poses, win, stride, device=self.device)
        occ = self._skip_grid(knobs, "render_frames")
        (coarse, fine), counts = self._render_counted(ray_o.view(-1, 3), ray_d.view(-1, 3), rays.RENDER_TESTING_RAYS, n_importance, occ, stop)
        return _with_counts(_frames_dict(coarse, fine, (poses.shape[0], win[2], win[3])), counts)

    def score_frames(self, frames: Tensor, meta: dict, depth_frames: Optional[Tensor] = None, stride: int = 1, n_importance: int = 0,
                     ssim: bool = False, skip_empty=None, early_stop=None, format: str = "bgr", uv_row=None) -> dict:
        """Held-out camera frames against the scene's render of their poses, on the device: ``frames`` (1, k, Hs, Ws, 3) uint8 BGR at capture
        resolution -- ``format="nv12"``: NV12 surfaces (1, k, rows, pitch) with ``uv_row``, scored as ``datasets.nv12_to_bgr`` of them would
        be, exactly -- checked against the scene as :meth:`add_frames` checks them; ``meta`` a chunk meta with the k extrinsics; ``depth_frames``
        optionally the sensor's (1, k, Hd, Wd) uint16 millimetres.  The held-out bytes are pipeline.prepare_frames' resized bytes cropped to
        the content region and strided like the render (``stride=s``: pixels ``s // 2, s // 2 + s, ...``), the held-out depth
        pipeline.prepare_depth_frames at the content size, strided the same way and quantised by pack_frames' rule (pipeline.depth_to_mm);
        the render is :meth:`render_frames` of the extrinsics.  Returns ``pipeline.frame_errors(render, held_out, render_depth,
        held_out_depth)``: per frame ``sse``, ``n_px``, ``depth_sad_mm``, ``n_depth`` (int64) and ``psnr`` (float64) over the pixels the
        render has a depth for.  With ``ssim=True`` one more launch (``pipeline.frame_ssim(render, held_out, render_depth)``) adds the
        reference's second metric over the 7 x 7 windows the render has a depth for throughout: ``ssim``, ``ssim_channels`` (float64) and
        ``n_windows`` (int64) per frame, on the strided frames as they are; a strided content region below 7 x 7 pixels is then a
        ValueError before any launch.  Nothing is added to the scene.  ``skip_empty`` as in :meth:`render_rays`: the culled render is
        scored, and the dict gains ``n_kept`` and ``n_samples`` -- scoring with and without it says what a threshold costs.
        ``early_stop`` as in :meth:`render_rays`, in the same way."""
        self._need_bank("score_frames")
        knobs = _skip_knobs(skip_empty, self.det, self.device, "score_frames")
        if knobs is not None:
            _check_culled_call(self.det, "score_frames", frames)
        stop = _stop_checked(self.det, early_stop, "score_frames", frames)
        held, held_depth, _, n_importance = _score_held_out(self.meta, [self.meta], frames, [meta], depth_frames, stride, n_importance, self.mean, self.std,
                                                            ssim, format, uv_row)
        out = self.render_frames(extrinsic=meta["lidar2img"]["extrinsic"], stride=stride, n_importance=n_importance, skip_empty=knobs,
                                 early_stop=stop)
        return _with_counts(_frame_scores(out, held, held_depth, ssim), (out["n_kept"], out["n_samples"]) if "n_kept" in out else None)

    def draw_detections(self, frames: Tensor, result: dict, c2w=None, extrinsic=None, window=None, stride: int = 1, capture: bool = False,
                        score_thr: float = 0.0, thickness: int = 1, palette=None, depth_frames=None, occluded: str = "hide",
                        depth_bias: float = 0.05, text=None, text_scale: int = 1) -> dict:
        """The wireframes of one detection result on k camera frames that lie in device memory.  ``result``: what ``detect()[0]`` returns;
        the detections with ``score >= score_thr`` are kept, handed over by ascending score (boxes.drawing_order: the best one wins every
        pixel it shares) and coloured by label (``palette`` (c,3) uint8 BGR; None: pipeline.class_palette).  Exactly one of ``c2w`` and
        ``extrinsic``, the k poses as :meth:`render_frames` takes them.  ``capture=False``: ``frames`` (k,h,w,3) uint8 on the grid
        ``window`` / ``stride`` of :meth:`render_frames` -- its ``frames`` output fits -- with the scene meta's scaled intrinsics;
        ``capture=True``: ``frames`` (k,Hs,Ws,3) at ``ori_shape`` with the meta's intrinsics unscaled (no window, no stride).  One
        ndet_project_boxes and one ndet_draw_boxes launch (pipeline.project_boxes, pipeline.draw_boxes), none when nothing is kept.
        Returns ``dict(frames`` -- new frames, the input is only read -- ``, rect (k,m,4) int32, zrange (k,m,2) float32, kept (m,) int64``:
        the result's indices in drawing order, which is the numbering of ``rect`` and ``zrange``).  Uses the scene's meta only: no
        ``keep_views``, no state and no bank is changed.  Bad arguments are a ValueError before any launch, CPU frames a RuntimeError.

        ``depth_frames`` (k,h,w) uint16 millimetres on the frames' own grid (``capture=True`` included; :meth:`render_frames`'
        ``depth_frames`` fits, a sensor frame of another size is the caller's to bring there:
        ``depth_to_mm(prepare_depth_frames(...))``) depth-tests the edges: a covered pixel is hidden where the depth frame lies more than
        ``depth_bias`` metres in front of the edge (a hole hides nothing); ``occluded="hide"`` leaves hidden pixels as they were,
        ``"dim"`` blends a quarter of the colour in.  The default ``depth_bias`` of 0.05 m is a choice, not a measurement: it covers the
        one-pixel error of the edge's interpolated depth and sensor noise at indoor range.  ``text=True`` writes ``f"{label} {score:.2f}"``
        on a plate in the box's colour above its rectangle, a sequence of class names ``f"{names[label]} {score:.2f}"`` (a label outside
        it is a ValueError), at ``text_scale`` 1, 2 or 3 (pipeline.FONT_5X7).  With ``depth_frames`` and ``text`` both None the call is
        the two launches above; otherwise one ndet_project_boxes_w (ndet_project_boxes without depth frames) and one ndet_draw_overlay
        (pipeline.draw_overlay).  The returned dict is the same."""
        thickness = _check_thickness(thickness, "draw_detections")
        plan = _plan_detections(self.det, self.meta, frames, (3,), torch.uint8, result, c2w, extrinsic, window, stride, capture, score_thr, palette,
                                "draw_detections")
        _plan_overlay(plan, result, depth_frames, occluded, depth_bias, text, text_scale, "draw_detections")
        _need_device_frames([plan], "draw_detections")
        _need_device_depth([plan], "draw_detections")
        return _draw_plan(plan, thickness)

    def label_detections(self, depth_frames: Tensor, result: dict, c2w=None, extrinsic=None, window=None, stride: int = 1, capture: bool = False,
                         score_thr: float = 0.0) -> Tensor:
        """Which kept detection each pixel of k depth frames belongs to: ``(k,h,w)`` int16 in the numbering of :meth:`draw_detections`'
        ``kept`` (the best detection that holds the pixel's point wins), -1 for none and for a hole.  ``depth_frames`` (k,h,w) uint16
        millimetres at the grid's size -- :meth:`render_frames`' ``depth_frames``, or with ``capture=True`` a sensor frame whose size is
        ``ori_shape``'s; the other arguments as in :meth:`draw_detections`.  One ndet_label_frames launch (pipeline.label_frames)."""
        plan = _plan_detections(self.det, self.meta, depth_frames, (), torch.uint16, result, c2w, extrinsic, window, stride, capture, score_thr, None,
                                "label_detections")
        _need_device_frames([plan], "label_detections")
        return _label_plan(plan)

    def volume(self):
        """``(volume (C,X,Y,Z), valid (1,X,Y,Z) int64)`` of the views so far: K2-finish -> sigma-MLP -> K1-finish, what ``extract_volume``
        returns for them (channels-last memory)."""
        return self._finish()[1:]

    def _finish(self):
        """The finishes :meth:`volume` and :meth:`occupancy` share, ring or not: ``(alpha (N,), volume, valid)``."""
        if self.n_views == 0:
            raise RuntimeError("the scene has no views yet: call add_views first")
        ring = self.window is not None
        with torch.no_grad():
            glob = ops.density_finish_ring(self._segs, self._lin.bias) if ring else ops.density_finish(self.state, self._lin.bias)
            alpha = _finished_alpha(self.det.nerf_mlp, self.lattice, glob)
            return (alpha,) + (ops.volume_finish_ring(self._segs, alpha) if ring else ops.volume_finish(self.state, alpha))

    def carve_counts(self):
        """``(free, hit)`` int32 (X,Y,Z) tensors over the carve's fine lattice: the counts of the chunks held now, for inspection.  Needs
        ``begin_scene(carve=)`` (else ValueError); no chunk held: zeros."""
        if self.carve is None:
            raise ValueError("carve_counts needs a carved scene: begin_scene(img_meta, carve=True)")
        segs = self.carve.store.segments or [torch.zeros((self.carve.store.n,), dtype=torch.int32, device=self.device)]
        return ops.carve_counts(segs, self.carve.n_voxels)

    def points(self, min_points: int = 1, result=None, score_thr: float = 0.0):
        """The scene's point cloud from the depth frames of the chunks held now: ``dict(xyz (M,3) float32, bgr (M,3) uint8,
        count (M,) int32, voxel (M,) int32)`` on the device -- one point per voxel of the cloud's fine lattice that ``min_points`` (an int of
        at least 1) or more depth pixels fell into, in ascending flat index: their mean position, their mean colour, their number and the
        voxel's index (ops.cloud_points: two launches, one device-to-host read).  ``result``: one scene's ``detect()[0]``; the dict then
        also holds ``ids (M,)`` int16, for every point the index INTO ``kept`` of the box that holds it (the last such in drawing
        order; -1: none), and ``kept``, the result's indices with ``scores_3d >= score_thr`` by ascending score, as
        :meth:`label_detections` defines them.  ``pipeline.write_ply`` writes such a cloud to a file.  ``detect()`` does not use the
        cloud.  Needs ``begin_scene(cloud=)`` (else ValueError); no chunk held: M = 0."""
        _need_cloud(self.cloud, "points")
        return self.cloud.points(min_points, result, score_thr)

    def cloud_sums(self):
        """``dict(n, qx, qy, qz, b, g, r)`` of int64 (X,Y,Z) tensors over the cloud's fine lattice: the sums of the chunks held now, for
        inspection.  Needs ``begin_scene(cloud=)`` (else ValueError); no chunk held: zeros."""
        _need_cloud(self.cloud, "cloud_sums")
        return self.cloud.sums()

    def occupancy(self, threshold: float = 1e-3, dilate: int = 1, outside: str = "keep", *, source: str = "alpha", min_free: int = 2):
        """The scene's occupancy grid (rays.OccupancyGrid) over the views held now, from the stream's own finishes -- density finish, the
        sigma-MLP's alpha, ``volume_finish``'s ``valid``: exactly what :meth:`volume` runs -- and one k_occupancy_bits launch.  A voxel is
        solid iff ``not (alpha <= threshold)`` or no view saw it; a bit is set iff a voxel within Chebyshev distance ``dilate`` (0, 1, 2)
        is solid; ``outside``: 'keep' or 'cull', what a culled render does with a sample outside the lattice.  The alpha is the same
        ``1 - exp(-relu(sigma))`` of the same ``nerf_mlp`` that compositing applies to a sample, so the two compare directly.  The
        default threshold is a GUESS: nobody has judged it on a trained checkpoint.  The grid is as coarse as the detection lattice.

        ``source``: 'alpha' (the above), 'depth' or 'both'; the last two need ``begin_scene(carve=)`` (else ValueError).  'depth': the grid
        carved from the depth frames of the chunks held, over the carve's FINE lattice -- a fine voxel is empty iff at least
        ``min_free`` views saw it in front of their surface by the band or more and none saw it on a surface, and solid otherwise (unseen,
        behind a surface, on one); ``dilate`` counts fine voxels; one k_carve_bits call, no MLP, ``threshold`` is not used.  'both': solid
        iff carve-solid AND the parent detection voxel is solid in the undilated alpha grid; dilation follows on the fine lattice.  Whether
        a carved grid helps on a real scene is yours to judge: :meth:`score_frames` with and without it.

        Cached per ``(threshold, dilate, outside)`` and, for the other sources, ``source`` and ``min_free``; dropped by whatever changes
        the views held (``add_views``, ``add_frames``, an eviction, ``drop_oldest``, ``reset``).  No views held: RuntimeError; bad knobs:
        ValueError, before any launch."""
        key = _check_occupancy_knobs(threshold, dilate, outside)
        source, min_free = _check_source_knobs(source, min_free)
        _need_carve(self.carve, source, "occupancy")
        if self.n_views == 0:
            raise RuntimeError("the scene has no views yet: call add_views first")
        if self._occ is None:
            self._occ = {}
        if source != "alpha":
            key = key + (source, min_free)
        if key not in self._occ:
            if source == "depth":
                self._occ[key] = self.carve.grid(min_free, key[1], key[2])
            else:
                alpha, _, valid = self._finish()
                if source == "alpha":
                    self._occ[key] = _make_occupancy(alpha, valid, self.lattice, self.det.n_voxels, self.det.voxel_size, *key)
                else:
                    self._occ[key] = self.carve.grid(min_free, key[1], key[2], ops.occupancy_bits(alpha, valid, self.det.n_voxels, key[0], 0))
        return self._occ[key]

    def _skip_grid(self, skip_empty, what: str, *tensors):
        """The grid of a ``skip_empty=`` render (None: no culling) once everything the call refuses has been checked."""
        knobs = _skip_knobs(skip_empty, self.det, self.device, what)
        if knobs is None:
            return None
        _check_culled_call(self.det, what, *tensors)
        return self.occupancy(**knobs) if isinstance(knobs, dict) else knobs

    def detect(self, defer: bool = False):
        """Detections over the views so far: what ``simple_test`` returns, ``[dict(boxes_3d, scores_3d, labels_3d)]``; with ``defer`` a
        ``finish()`` callable that returns it (one device-to-host copy).  The state is not changed: more views may follow.  When a fp16-pair
        launch of neck_3d or the head trips the range guard, those two are repeated on bf16x3 from the finished volume."""
        vol, valid = self.volume()
        metas = [dict(self.meta)]
        with torch.no_grad():
            guarded = conv3d.ARITHMETIC == "f16x2" and vol.is_cuda
            if guarded:
                conv3d.guard_begin(vol.device)
            x = self.det.neck_3d(vol.unsqueeze(0))
            return self.det._detect_tail(x, valid.unsqueeze(0), metas, defer, guarded, vol.device, lambda: self._repeat_tail(vol, valid, metas))

    def _repeat_tail(self, vol: Tensor, valid: Tensor, metas):
        return _repeat_tails(self.det, vol.unsqueeze(0), valid.unsqueeze(0), [metas])[0]


_TRIPPED = object()     # a deferred tail's answer when the range-guard word came back set (SceneGroup.detect)


class SceneGroup:
    """S scenes (1 .. ops.GROUP_MAX) of one detector streamed together: ``det.begin_scenes([img_meta_0, ..., img_meta_{S-1}])``.  Every scene
    has its own ``lidar2img.intrinsic``, ``lidar2img.origin`` and extrinsics and its own state; ``img_shape``, ``ori_shape``, the voxel grid and
    the detector are the group's.  One :meth:`add_views` call runs the backbone once over one chunk of k views (1 .. ops.GROUP_VIEWS_MAX) per
    listed scene and folds every chunk into its scene's state with one grouped accumulate (ops.scene_accumulate_group); one :meth:`detect`
    finishes the listed scenes with one grouped density finish, one sigma-MLP call, one grouped volume finish and one neck_3d call over the
    batch (which neck_3d walks scene by scene; ``detect(batched=True)``: one launch per neck layer and head level for all the listed scenes, which
    then share the 3D part's fp16-pair scales), queues every scene's tail and then waits once.  ``scenes``: None (all scenes, in order) or a list of distinct scene indices -- cameras do not
    tick together, so a call may serve a subset.

    What is exact: a scene's state after a grouped accumulate is bit-equal to ops.scene_accumulate on that scene alone (sums and counts),
    whatever the other scenes, the subset or its order, and the grouped finishes give the single-state finishes' rows, volume and counts bit
    for bit.  A group of one scene gives :class:`SceneStream`'s detections bit for bit (hence a single chunk gives ``simple_test``'s).  With
    more than one scene the backbone's per-tensor fp16-pair scales are shared by the scenes of a call (neck_3d and the head still run scene by
    scene, on scales of their own): detections agree with separate streams within the chunking contract -- same labels in the same order,
    scores and boxes to 1e-4.

    ``window``: None, or the number of chunks every scene keeps (1 .. ops.RING_MAX).  A windowed group holds one state per chunk and scene
    (ops.SceneGroupRingState: at most ``window + 1`` states per scene, allocated when first needed).  Every listed scene's chunk of an
    :meth:`add_views` call fills a state of its own through the same grouped accumulate; only when it has succeeded do the states join
    their scenes' windows and the oldest chunk leaves each listed scene whose window was full -- scenes evict independently, and a call
    that raises leaves every window as it was.  :meth:`detect` finishes the listed windows with one grouped density ring finish, one
    sigma-MLP call and one grouped volume ring finish, whose outputs are ops.density_finish_ring / volume_finish_ring's per scene bit
    for bit: a windowed group of one scene is a windowed :class:`SceneStream` bit for bit, and a dropped chunk leaves no trace.

    ``keep_views``: also keep every scene's views in a view bank of its own (``banks[s]``, a rays.ViewBank; None without it) so that
    :meth:`render_rays` / :meth:`render` work; a detector with ``render_testing=True`` is accepted only then.  :meth:`add_views` makes
    every listed scene's segment from its rows of the mapped map and of ``denorm_images`` before the grouped accumulate
    (``make_segment`` changes nothing) and pushes them only once it has succeeded; in a windowed group a scene's oldest segment leaves
    with its oldest state (a full window, :meth:`drop_oldest`), :meth:`reset` clears the listed banks, and a call that raises anywhere
    leaves every state, window and bank as it was.  After every call a scene's bank holds exactly the chunks its states hold
    (windowed: ``[seg.n_views for seg in banks[s].segments] == chunk_views[s]``; an unwindowed scene reports its views as one chunk,
    its bank keeps a segment per call, the totals agree).  4 (hf wf cm + 4 H W) + 64 bytes a view held.  As with one bank, renders and
    evictions must be issued on ONE stream (rays.ViewBank).

    Out of scope: scenes of different image sizes or grids in one group, training or autograd through the banks, and the graphed path."""

    window = None       # None, or the chunks every scene keeps
    pool = None         # ops.SceneGroupRingState of a windowed group
    group = None        # ops.SceneGroupState of an unwindowed one
    banks = None        # with keep_views one rays.ViewBank per scene, else None
    _occ = None         # per scene (threshold, dilate, outside[, source, min_free]) -> rays.OccupancyGrid of the views it holds now, made by occupancy()
    carves = None       # with begin_scenes(carve=) one SceneCarve per scene (one refine and band for the group), else None
    clouds = None       # with begin_scenes(cloud=) one SceneCloud per scene (one refine and max_depth for the group), else None
    mean, std = IMG_MEAN, IMG_STD     # img_norm_cfg of add_frames (RGB)

    def __init__(self, det, img_metas, window: Optional[int] = None, keep_views: bool = False, mean=IMG_MEAN, std=IMG_STD, carve=None,
                 cloud=None):
        self.mean, self.std = _norm_cfg(mean, std)
        if not isinstance(keep_views, bool):
            raise ValueError(f"keep_views must be a bool, got {keep_views!r}")
        if window is not None:
            ops.check_window(window)
        carve = _carve_knobs(carve, det)
        cloud = _cloud_knobs(cloud)
        metas = list(img_metas)
        if not 1 <= len(metas) <= ops.GROUP_MAX:
            raise ValueError(f"begin_scenes takes 1 to {ops.GROUP_MAX} scenes, got {len(metas)}")
        self._check_shapes(metas[0], metas)
        if det.training:
            raise RuntimeError("SceneGroup is inference only: call det.eval() first")
        if det.render_testing and not keep_views:
            raise NotImplementedError("SceneGroup does not render rays (render_testing needs every view's feature map): "
                                      "begin_scenes(img_metas, keep_views=True) keeps them")
        self.det = det
        self.metas = metas
        self.device = next(det.parameters()).device
        lin = det.mapping[0]
        self._lin = lin
        points = [ops.get_points(det.n_voxels, det.voxel_size, m["lidar2img"]["origin"], self.device) for m in metas]
        self.window = window
        if window is None:
            self.group = ops.SceneGroupState(det.n_voxels, lin.in_features, lin.out_features, points, self.device)
        else:
            self.pool = ops.SceneGroupRingState(det.n_voxels, lin.in_features, lin.out_features, points, window, self.device)
        if keep_views:
            from .rays import ViewBank
            self.banks = [ViewBank() for _ in metas]
        if carve is not None:
            self.carves = [SceneCarve(det, m["lidar2img"]["origin"], self.device, carve, window is not None) for m in metas]
        if cloud is not None:
            self.clouds = [SceneCloud(det, m, self.device, cloud, window is not None) for m in metas]

    @staticmethod
    def _check_shapes(first: dict, metas) -> None:
        for i, m in enumerate(metas):
            for key in ("img_shape", "ori_shape"):
                if tuple(m[key]) != tuple(first[key]):
                    raise ValueError(f"scene {i}'s {key} {tuple(m[key])} differs from the group's {tuple(first[key])}")

    @property
    def n_scenes(self) -> int:
        return len(self.metas)

    @property
    def n_views(self) -> List[int]:
        """View counts of the S scenes (of a windowed group: over the chunks held)."""
        return self.group.n_views if self.window is None else self.pool.n_views

    @property
    def chunk_views(self) -> List[List[int]]:
        """Per scene the view counts of the chunks held, oldest first (an unwindowed scene holds its views as one)."""
        if self.window is None:
            return [[v] if v else [] for v in self.group.n_views]
        return self.pool.chunk_views

    @property
    def n_chunks(self) -> List[int]:
        return [len(c) for c in self.chunk_views]

    def _drop_grids(self, scenes) -> None:
        """Whatever changes the views a scene holds drops that scene's cached occupancy grids."""
        if self._occ is not None:
            for s in scenes:
                self._occ[s].clear()

    def reset(self, scenes=None) -> None:
        """Forget every view of the listed scenes: they start empty again; the others keep theirs."""
        scenes = ops.listed_scenes(self.n_scenes, scenes)
        self._drop_grids(scenes)
        for s in scenes:
            if self.window is None:
                self.group.states[s].reset()
            else:
                self.pool.drop_oldest(len(self.pool.segs[s]), [s])
            if self.banks is not None:
                self.banks[s].clear()
            if self.carves is not None:
                self.carves[s].store.clear()
            if self.clouds is not None:
                self.clouds[s].store.clear()

    def drop_oldest(self, k: int = 1, scenes=None) -> None:
        """Forget the k oldest chunks of every listed scene of a windowed group (their states are zeroed and kept for the chunks to come).
        The call is refused whole (ValueError) when any listed scene holds fewer than k chunks; ``k = 0`` is allowed."""
        if self.window is None:
            raise ValueError("drop_oldest needs a windowed group: begin_scenes(img_metas, window=S)")
        scenes = ops.listed_scenes(self.n_scenes, scenes)
        self.pool.drop_oldest(k, scenes)            # refused whole before any window or bank changes
        self._drop_grids(scenes)
        if self.banks is not None:
            for s in scenes:
                self.banks[s].drop_oldest(k)
        if self.carves is not None:
            for s in scenes:
                self.carves[s].store.drop_oldest(k)
        if self.clouds is not None:
            for s in scenes:
                self.clouds[s].store.drop_oldest(k)

    def _carve_chunks(self, scenes, depth_gate, rgb_proj: Tensor) -> list:
        """Every listed scene's carve target with its chunk's evidence added (SceneCarve.chunk over the scene's k views of the call's gate
        and stride-1 projections: one k_carve_accumulate launch a scene); no store is changed.  When a scene's launch is refused, the
        targets made so far go back."""
        k = rgb_proj.shape[0] // len(scenes)
        segs = []
        try:
            for i, s in enumerate(scenes):
                sl = slice(i * k, (i + 1) * k)
                g = None if depth_gate is None else ops.DepthGate(depth_gate.depth_f[sl], depth_gate.depth_r[sl], depth_gate.band)
                segs.append(self.carves[s].chunk(g, rgb_proj[sl]))
        except BaseException:
            if self.window is not None:
                for s, seg in zip(scenes, segs):
                    self.carves[s].store.give_back(seg)
            raise
        return segs

    def _cloud_chunks(self, scenes, depth_gate, rgb: Tensor, c2ws) -> list:
        """Every listed scene's cloud target with its chunk's pixels added, and their number (SceneCloud.chunk over the scene's k views of
        the call's gate, B, G, R planes and camera-to-world matrices: one k_cloud_accumulate launch a scene); no store is changed.  When a
        scene's launch is refused, the targets made so far go back."""
        k = rgb.shape[0] // len(scenes)
        segs = []
        try:
            for i, s in enumerate(scenes):
                sl = slice(i * k, (i + 1) * k)
                g = None if depth_gate is None else ops.DepthGate(depth_gate.depth_f[sl], depth_gate.depth_r[sl], depth_gate.band)
                segs.append(self.clouds[s].chunk(g, rgb[sl], c2ws[i]))
        except BaseException:
            if self.window is not None:
                for s, (seg, _) in zip(scenes, segs):
                    self.clouds[s].store.give_back(seg)
            raise
        return segs

    def _accumulate(self, scenes, *chunk, depth_gate=None, banked=None, cloud_c2w=None) -> None:
        """Fold one chunk per listed scene into the scenes' states, or in a windowed group into empty states that join the scenes' windows
        once the grouped accumulate has succeeded (ops.SceneGroupRingState.accumulate): a call that fails leaves every window as it was.
        ``banked``: the listed scenes' view-bank segments, made by the caller (rays.ViewBank.make_segment changes nothing); they join
        their banks only once the states have taken the chunks, and a scene's oldest segment leaves with the oldest state of its full
        window, so states and banks hold the same chunks.  Carved scenes' counter segments (:meth:`_carve_chunks`) follow the same rule:
        in a windowed group they are made inside the grouped accumulate's transaction and join their stores with the states; in an
        unwindowed one they are added to the scenes' segments once the states have taken the chunks."""
        self._drop_grids(scenes)
        carved = clouded = None
        if self.window is None:
            ops.scene_accumulate_group(self.group, scenes, *chunk, depth_gate=depth_gate)
            if self.carves is not None:
                carved = self._carve_chunks(scenes, depth_gate, chunk[-1])
            if self.clouds is not None:
                clouded = self._cloud_chunks(scenes, depth_gate, chunk[3], cloud_c2w)
        else:
            full = [len(self.pool.segs[s]) == self.window for s in scenes]

            def fill(states):
                nonlocal carved, clouded
                ops.scene_accumulate_group_ring(self.pool, scenes, *chunk, depth_gate=depth_gate, states=states)
                if self.carves is not None:
                    carved = self._carve_chunks(scenes, depth_gate, chunk[-1])
                if self.clouds is not None:
                    try:
                        clouded = self._cloud_chunks(scenes, depth_gate, chunk[3], cloud_c2w)
                    except BaseException:
                        if carved is not None:
                            for s, seg in zip(scenes, carved):
                                self.carves[s].store.give_back(seg)
                        raise

            self.pool.accumulate(scenes, fill)
            for s, was_full in zip(scenes, full):
                if was_full:
                    if banked is not None:
                        self.banks[s].drop_oldest(1)
                    if carved is not None:
                        self.carves[s].store.drop_oldest(1)
                    if clouded is not None:
                        self.clouds[s].store.drop_oldest(1)
        if banked is not None:
            for s, seg in zip(scenes, banked):
                self.banks[s].push(seg)
        if carved is not None:
            for s, seg in zip(scenes, carved):
                self.carves[s].store.push(seg)
        if clouded is not None:
            for s, seg in zip(scenes, clouded):
                self.clouds[s].store.push(*seg)

    def _check_call(self, img: Tensor, denorm_images: Tensor, metas, scenes, depth):
        """Everything add_views refuses, before anything is launched: ``(listed scenes, k)``."""
        scenes = ops.listed_scenes(self.n_scenes, scenes)
        n = len(scenes)
        if img.dim() != 5 or img.shape[0] != n:
            raise ValueError(f"add_views takes one chunk per listed scene, ({n}, k, 3, H, W); got {tuple(img.shape)}")
        k = img.shape[1]
        if not 1 <= k <= ops.GROUP_VIEWS_MAX:
            raise ValueError(f"add_views: k={k} views per scene, must be 1 .. {ops.GROUP_VIEWS_MAX}")
        if denorm_images.dim() != 5 or denorm_images.shape[:2] != img.shape[:2]:
            raise ValueError(f"add_views: img {tuple(img.shape)} and denorm_images {tuple(denorm_images.shape)} must hold the same scenes and views")
        if depth is not None and (depth.dim() != 4 or depth.shape[:2] != img.shape[:2]):
            raise ValueError(f"add_views: depth must be ({n}, k, Hd, Wd), got {tuple(depth.shape)}")
        metas = list(metas)
        if len(metas) != n:
            raise ValueError(f"add_views: {len(metas)} chunk metas for {n} listed scenes")
        for s, m in zip(scenes, metas):
            check_chunk_meta(self.metas[s], m, k)
        if self.det.training:
            raise RuntimeError("SceneGroup is inference only: call det.eval() first")
        return scenes, k

    def add_frames(self, frames: Tensor, metas, scenes=None, depth: Optional[Tensor] = None, depth_frames: Optional[Tensor] = None,
                   format: str = "bgr", uv_row=None) -> None:
        """:meth:`add_views` for frames at CAPTURE resolution: ``frames`` (len(scenes), k, Hs, Ws, 3) uint8 BGR on the device, one row of k
        frames per listed scene -- or, with ``format="nv12"``, a video decoder's NV12 surfaces (len(scenes), k, rows, pitch) uint8 with
        ``uv_row`` as in :meth:`SceneStream.add_frames`, still ONE launch (ndet_resize_normalize_views_nv12) for the whole call.  The group's meta says what becomes of them, as in :meth:`SceneStream.add_frames`: ``(Hs, Ws)`` must be
        its ``ori_shape`` and its ``img_shape`` what ``Resize(keep_ratio=True)`` into the ``pad_shape`` box gives, else ValueError --
        raised, like everything :meth:`add_views` refuses, before any device work.  ONE ndet_resize_normalize_views launch over all the
        ``len(scenes) * k`` frames makes ``img`` and ``denorm_images`` (with ``mean`` / ``std`` of ``begin_scenes``), and :meth:`add_views` takes them: guard, windows, banks and the promise that a call that raises changes
        nothing are its own.  ``depth`` passes through.  ``depth_frames`` instead of ``depth``: the sensor's frames (len(scenes), k, Hd, Wd)
        uint16 millimetres on the device; ONE ndet_depth_frames launch over all of them makes the float64 metres at the group's
        ``img_shape``, as in :meth:`SceneStream.add_frames`.  Both given, a wrong dtype or another k: ValueError, before any device work."""
        listed = ops.listed_scenes(self.n_scenes, scenes)
        n = len(listed)
        img_scale, pad_size = check_frames_meta(self.metas[0], frames, n, format, uv_row)
        metas = list(metas)
        for m in metas:
            _check_pad_shape(self.metas[0], m)
        k = frames.shape[1]
        check_depth_frames(depth_frames, depth, n, k)
        shape = torch.empty((n, k, 3) + pad_size, device="meta")
        self._check_call(shape, shape, metas, scenes, depth)
        if self.clouds is not None:
            for s in listed:
                self.clouds[s].check(k, depth is not None or depth_frames is not None)
        img, denorm, depth = _prepared_frames(frames, depth_frames, depth, self.metas[0]["img_shape"], img_scale, pad_size, self.mean, self.std,
                                              _surface_kwargs(self.metas[0], format, uv_row))
        self.add_views(img, denorm, metas, scenes=scenes, depth=depth)

    def add_views(self, img: Tensor, denorm_images: Tensor, metas, scenes=None, depth: Optional[Tensor] = None) -> None:
        """Fold k views into each listed scene.  ``img``, ``denorm_images`` (len(scenes), k, 3, H, W), one row per listed scene; ``metas`` one
        chunk meta per row (its ``extrinsic`` list has k entries; the rest must equal its scene's, else ValueError); ``depth`` None or
        (len(scenes), k, Hd, Wd) float32 / float64: it gates every scene of the call or none (nerfdet.py:404-411).

        One pass for the whole call: the guard word is cleared, the backbone runs on all the chunks, the word is read back once (one
        synchronisation per call, not per scene), and one grouped accumulate folds every scene's rows into its own state (in a windowed
        group: into a state of its own per listed scene, which then joins that scene's window).  A tripped call's backbone is redone on
        bf16x3 before any state or window is touched (``conv3d.guard_trips`` counts it once).  With ``keep_views`` every listed scene's
        bank segment is made before the accumulate and joins its bank after it.  A call that is refused leaves every state, window
        and bank as it was -- also one the backbone refuses: the ``len(scenes) * k`` views share its launches, whose operands address
        at most 2 GB each (200 views of 240 x 320 are too many)."""
        scenes, k = self._check_call(img, denorm_images, metas, scenes, depth)
        n = len(scenes)
        metas = list(metas)
        cloud_c2w = None
        if self.clouds is not None:
            for s in scenes:
                self.clouds[s].check(k, depth is not None)
            cloud_c2w = [_chunk_c2w(m) for m in metas]
        with torch.no_grad():
            lin = self._lin
            hh, ww = self.metas[0]["img_shape"][0], self.metas[0]["img_shape"][1]
            feat, mapped, stride = _chunk_features(self.det, lin, img, (hh, ww))
            rgb = denorm_images.reshape([-1] + list(denorm_images.shape)[2:])[:, :, :hh, :ww]
            gate = None
            if depth is not None:
                d = depth.reshape([-1] + list(depth.shape)[2:]).to(self.device, non_blocking=True)
                gate = ops.depth_gate(d, self.det.voxel_size, (hh // stride, ww // stride), (hh, ww))
            proj = ops.compute_projection_group(metas, (stride, 1), self.device)     # the n k projections at both strides: one upload
            # every bank takes its scene's rows of the mapped map as they are accumulated and of the images as extract_feat hands them to
            # render_rays (uncropped); all the segments are made before any state, window or bank changes
            banked = None
            if self.banks is not None:
                banked = [self.banks[s].make_segment(mapped[i * k:(i + 1) * k], denorm_images[i], metas[i]) for i, s in enumerate(scenes)]
            self._accumulate(scenes, feat, mapped, lin.bias, rgb, proj[0], proj[1], depth_gate=gate, banked=banked, cloud_c2w=cloud_c2w)

    def _need_views(self, scenes) -> List[int]:
        scenes = ops.listed_scenes(self.n_scenes, scenes)
        held = self.n_views
        empty = [s for s in scenes if held[s] == 0]
        if empty:
            raise ValueError(f"scenes {empty} have no views yet: call add_views first")
        return scenes

    def _need_banks(self, what: str, scenes) -> List[int]:
        if self.banks is None:
            raise RuntimeError(f"{what} needs the scenes' views: begin_scenes(img_metas, keep_views=True)")
        scenes = ops.listed_scenes(self.n_scenes, scenes)
        empty = [s for s in scenes if self.banks[s].n_views == 0]
        if empty:
            raise RuntimeError(f"scenes {empty} have no views yet: call add_views first")
        return scenes

    def _render(self, ray_os, ray_ds, scenes: List[int], step: int, batched: bool, n_importance: int = 0):
        """:func:`_render_passes` over the listed scenes' banks with ONE grouped sampler launch per pass (rays.bank_group_stats,
        k_ray_stats_bank_group): per listed scene ``((rgb, depth, mask) of the coarse pass, the same of the fine pass or None)``."""
        from . import rays
        return _render_passes(self.det, [self.banks[s] for s in scenes], ray_os, ray_ds, step, batched, n_importance, rays.bank_group_stats)

    def _render_counted(self, ray_os, ray_ds, scenes: List[int], step: int, batched: bool, n_importance: int, occs, stop=None):
        """``(per listed scene (coarse, fine), per listed scene (n_kept, n_samples))``: :meth:`_render` and Nones without grids, else every
        listed scene's culled passes on their own (:func:`_render_passes_culled`, the body of ``SceneStream``'s culled render): the kept
        counts differ from scene to scene and are known only after each scene's read, so a scene's launches follow its own cull --
        per scene and pass one count launch, one cull, one sampler launch and the MLP's calls, nothing grouped."""
        if occs is None and stop is None:
            return self._render(ray_os, ray_ds, scenes, step, batched, n_importance), [None] * len(scenes)
        occs = [None] * len(scenes) if occs is None else occs
        if stop is None:
            res = [_render_passes_culled(self.det, self.banks[s], occ, o, d, step, n_importance) for s, occ, o, d in zip(scenes, occs, ray_os, ray_ds)]
        else:          # front to back (early_stop=), scene by scene for the same reason
            res = [_render_passes_stopped(self.det, self.banks[s], occ, stop, o, d, step, n_importance)
                   for s, occ, o, d in zip(scenes, occs, ray_os, ray_ds)]
        return [r[:2] for r in res], [r[2:] for r in res]

    def render_rays(self, ray_o, ray_d, scenes=None, batched: bool = False, n_importance: int = 0, skip_empty=None, early_stop=None):
        """Render rays against the views the listed scenes hold: ``ray_o``, ``ray_d`` are lists of (R_s, 3) tensors, one pair per listed
        scene (the counts may differ, each at least 1); returns per listed scene ``dict(rgb (R_s,3), depth (R_s,), mask (R_s,) bool)`` as
        :meth:`SceneStream.render_rays` does.  Passes of at most ``rays.RENDER_TESTING_RAYS`` rays per scene: every scene that still has
        rays is sampled (``rays.sample_along_camera_ray(det=True)``), ONE grouped sampler launch serves all of them
        (rays.ray_view_stats_bank_group, k_ray_stats_bank_group), then ``nerf_mlp`` and ``rays.raw2outputs`` run per scene.  Every
        scene's result is bit for bit what ``rays.render_rays_func(det=True)`` gives, pass by pass, over the concatenation of that
        scene's own bank segments -- what a :class:`SceneStream` holding the same maps renders, whatever the other scenes; a group of
        one scene is ``SceneStream(keep_views=True).render_rays`` bit for bit.

        ``batched=True`` with more than one listed scene: one ``nerf_mlp`` call and one ``raw2outputs`` call over all the scenes'
        samples of a pass.  The ``linear_rows`` layers of the MLP take a per-tensor fp16-pair scale, which the scenes of a call then
        share (the fused trunk's scales are per row and do not change): masks stay bit-equal, ``rgb`` agrees with ``batched=False`` to
        1e-4 absolute and ``depth`` to 1e-4 x ``near_far_range[1]``.  One listed scene, or the "f32" arithmetic: the ``batched=False``
        path bit for bit.

        ``n_importance=k > 0`` adds the fine pass of ``rays.render_rays_func(N_importance=k)`` to every pass: after the coarse
        compositing ONE k_importance_merge launch over all the listed scenes' rays of the pass (rays.importance_merge), a second grouped
        sampler launch over the ``N_samples + k`` depths, then the MLP and the compositing again, per scene or ``batched``.  Each
        dict's ``rgb``, ``depth`` and ``mask`` are then the fine pass's and it gains ``'coarse'``, as :meth:`SceneStream.render_rays`
        returns them -- with ``batched=False`` bit for bit, with ``batched=True`` to the bounds above.

        Needs ``keep_views=True`` and at least one view in every listed scene (else RuntimeError); wrong list lengths or shapes are a
        ValueError; everything is refused before anything is launched.  No bank or state is changed.  Renders and evictions
        (``add_views`` at a full window, ``drop_oldest``, ``reset``) must be issued on ONE stream (rays.ViewBank).

        ``skip_empty`` as in :meth:`SceneStream.render_rays` -- None, True, a dict of :meth:`occupancy`'s keywords (each scene then uses
        its own grid) or one rays.OccupancyGrid for every listed scene: each listed scene's dict, ``n_kept`` and ``n_samples``
        included, is what a :class:`SceneStream` holding the same chunks returns with the same ``skip_empty``.  The culled passes run
        scene by scene (one count launch, one cull, one sampler launch per scene and pass).  With ``batched=True``: ValueError.
        ``early_stop`` as in :meth:`SceneStream.render_rays`, alone or with ``skip_empty``: each listed scene's dict is the stream's with
        the same ``early_stop``; the passes run scene by scene, and ``batched=True`` is a ValueError."""
        from . import rays
        scenes = self._need_banks("render_rays", scenes)
        n_importance = _check_n_importance(n_importance)
        ray_o, ray_d = self._check_rays(ray_o, ray_d, len(scenes))
        stop = _stop_checked(self.det, early_stop, "render_rays", *ray_o, *ray_d, batched=batched)
        occs = self._skip_grids(skip_empty, scenes, batched, "render_rays", *ray_o, *ray_d)
        res, counts = self._render_counted(ray_o, ray_d, scenes, rays.RENDER_TESTING_RAYS, batched, n_importance, occs, stop)
        return [_with_counts(_render_dict(coarse, fine), c) for (coarse, fine), c in zip(res, counts)]

    @staticmethod
    def _check_rays(ray_o, ray_d, n: int):
        if isinstance(ray_o, Tensor) or isinstance(ray_d, Tensor):
            raise ValueError("render_rays takes LISTS of (R,3) origins and directions, one pair per listed scene")
        ray_o, ray_d = list(ray_o), list(ray_d)
        if len(ray_o) != n or len(ray_d) != n:
            raise ValueError(f"render_rays: {len(ray_o)} origin and {len(ray_d)} direction tensors for {n} listed scenes")
        for i, (o, d) in enumerate(zip(ray_o, ray_d)):
            if o.dim() != 2 or o.shape[1] != 3 or o.shape[0] < 1 or d.shape != o.shape:
                raise ValueError(f"render_rays takes (R,3) origins and directions with R >= 1, got {tuple(o.shape)} and {tuple(d.shape)} "
                                 f"for listed scene {i}")
        return ray_o, ray_d

    def render(self, ray_batches, scenes=None, batched: bool = False, n_importance: int = 0, skip_empty=None, early_stop=None):
        """Every ray of the target views of one ray batch per listed scene: per scene what :meth:`SceneStream.render` returns
        (``outputs_coarse.rgb`` (T,h,w,3), ``outputs_coarse.depth`` (T,h,w,1), ``gt_rgb``, ``gt_depth`` -- ``rays.rendering_metrics``
        applies), through the passes of :meth:`render_rays` with SceneStream.render's pass size,
        ``N_rand * max(1, RENDER_TESTING_RAYS // N_rand)``; ``batched`` and ``n_importance`` (which adds ``outputs_fine``) as in
        :meth:`render_rays`.  One stream, as there.  ``skip_empty`` and ``early_stop`` as in :meth:`render_rays`."""
        scenes = self._need_banks("render", scenes)
        n_importance = _check_n_importance(n_importance)
        ray_batches = list(ray_batches)
        if len(ray_batches) != len(scenes):
            raise ValueError(f"render: {len(ray_batches)} ray batches for {len(scenes)} listed scenes")
        unpacked = [_unpack_ray_batch(rb) for rb in ray_batches]
        os_, ds_ = self._check_rays([u[0] for u in unpacked], [u[1] for u in unpacked], len(scenes))
        stop = _stop_checked(self.det, early_stop, "render", *os_, *ds_, batched=batched)
        occs = self._skip_grids(skip_empty, scenes, batched, "render", *os_, *ds_)
        res, counts = self._render_counted(os_, ds_, scenes, _render_step(self.det), batched, n_importance, occs, stop)
        return [_with_counts(_render_views(coarse, fine, shape, gt_rgb, gt_depth), c)
                for (coarse, fine), (_, _, shape, gt_rgb, gt_depth), c in zip(res, unpacked, counts)]

    def render_frames(self, c2w=None, extrinsic=None, scenes=None, batched: bool = False, window=None, stride: int = 1, n_importance: int = 0,
                      skip_empty=None, early_stop=None):
        """:meth:`SceneStream.render_frames` for the listed scenes at once: exactly one of ``c2w`` and ``extrinsic``, a list with one list of
        4 x 4 matrices per listed scene (the counts may differ, each at least 1).  Every scene uses its own intrinsics, scaled as in
        :meth:`SceneStream.render_frames`; ``window`` and ``stride`` are the call's (the group shares ``img_shape``).  ONE
        ndet_camera_rays launch per distinct intrinsics makes the rays of all the scenes that share them (scenes of one camera model: one
        launch for the call), rendering goes through :meth:`render_rays`' grouped passes (``batched`` and ``n_importance`` as there), and
        every scene's frames are packed by one ndet_pack_frames launch per pass kind.  Returns a list of dicts as
        :meth:`SceneStream.render_frames` returns them: per scene bit for bit ``group.render_rays`` on the generated rays (with
        ``batched=True`` to :meth:`render_rays`' documented bounds), and a group of one scene is ``SceneStream.render_frames`` bit for bit.
        RuntimeError without ``keep_views`` or for a listed scene without views; bad arguments are a ValueError before any launch.
        ``skip_empty`` and ``early_stop`` as in :meth:`render_rays`."""
        from . import rays
        scenes = self._need_banks("render_frames", scenes)
        n_importance = _check_n_importance(n_importance)
        given = _camera_lists(c2w, extrinsic, "render_frames")
        if len(given) != len(scenes):
            raise ValueError(f"render_frames: {len(given)} camera lists for {len(scenes)} listed scenes")
        poses = [_camera_poses(g, None, "render_frames") if c2w is not None else _camera_poses(None, g, "render_frames") for g in given]
        win, stride = _frame_grid(self.metas[0], window, stride)
        ks = [_scene_intrinsic(self.metas[s]) for s in scenes]
        knobs = _skip_knobs(skip_empty, self.det, self.device, "render_frames")        # refused before the ray launches
        if knobs is not None:
            if batched:
                raise ValueError("render_frames: batched=True and skip_empty exclude each other for now")
            _check_culled_call(self.det, "render_frames")
        stop = _stop_checked(self.det, early_stop, "render_frames", batched=batched)
        shared = OrderedDict()                      # listed scenes by the bytes of their intrinsic rows: one launch each
        for i, k in enumerate(ks):
            shared.setdefault(k[:2, :3].tobytes(), []).append(i)
        ray_os, ray_ds = [None] * len(scenes), [None] * len(scenes)
        for idx in shared.values():
            o, d = camera_rays(ks[idx[0]], np.concatenate([poses[i] for i in idx]), win, stride, device=self.device)
            at = 0
            for i in idx:
                c = poses[i].shape[0]
                ray_os[i], ray_ds[i] = o[at:at + c].view(-1, 3), d[at:at + c].view(-1, 3)
                at += c
        occs = self._skip_grids(knobs, scenes, batched, "render_frames")
        res, counts = self._render_counted(ray_os, ray_ds, scenes, rays.RENDER_TESTING_RAYS, batched, n_importance, occs, stop)
        return [_with_counts(_frames_dict(coarse, fine, (p.shape[0], win[2], win[3])), c) for (coarse, fine), p, c in zip(res, poses, counts)]

    def score_frames(self, frames: Tensor, metas, scenes=None, depth_frames: Optional[Tensor] = None, batched: bool = False, stride: int = 1,
                     n_importance: int = 0, ssim: bool = False, skip_empty=None, early_stop=None, format: str = "bgr", uv_row=None):
        """:meth:`SceneStream.score_frames` for the listed scenes at once: ``frames`` (len(scenes), k, Hs, Ws, 3) uint8 BGR, one row of k
        held-out frames per listed scene (``format="nv12"``: NV12 surfaces (len(scenes), k, rows, pitch) with ``uv_row``), checked as :meth:`add_frames` checks them; ``metas`` one chunk meta per row with its k extrinsics;
        ``depth_frames`` optionally (len(scenes), k, Hd, Wd) uint16 millimetres.  One ndet_resize_normalize_views launch (and one
        ndet_depth_frames launch) makes all the held-out frames, :meth:`render_frames` all the renders, and one ndet_frame_errors launch
        per scene compares them -- with ``ssim=True`` one ndet_frame_ssim launch per scene beside it, which adds ``ssim``, ``ssim_channels``
        and ``n_windows`` as in :meth:`SceneStream.score_frames`.  Returns a list of ``pipeline.frame_errors`` dicts; nothing is added to
        any scene.  ``skip_empty`` as in :meth:`render_rays`: the culled renders are scored, every dict gains ``n_kept`` and ``n_samples``.
        ``early_stop`` as in :meth:`render_rays`, in the same way."""
        scenes = self._need_banks("score_frames", scenes)
        knobs = _skip_knobs(skip_empty, self.det, self.device, "score_frames")
        if knobs is not None:
            if batched:
                raise ValueError("score_frames: batched=True and skip_empty exclude each other for now")
            _check_culled_call(self.det, "score_frames", frames)
        stop = _stop_checked(self.det, early_stop, "score_frames", frames, batched=batched)
        metas = list(metas)
        held, held_depth, k, n_importance = _score_held_out(self.metas[0], [self.metas[s] for s in scenes], frames, metas, depth_frames, stride, n_importance,
                                                            self.mean, self.std, ssim, format, uv_row)
        outs = self.render_frames(extrinsic=[m["lidar2img"]["extrinsic"] for m in metas], scenes=scenes, batched=batched, stride=stride,
                                  n_importance=n_importance, skip_empty=knobs, early_stop=stop)
        return [_with_counts(_frame_scores(out, held[i * k:(i + 1) * k], None if held_depth is None else held_depth[i * k:(i + 1) * k], ssim),
                             (out["n_kept"], out["n_samples"]) if "n_kept" in out else None) for i, out in enumerate(outs)]

    def _plan_detections(self, frames, results, c2w, extrinsic, scenes, trailing, dtype, window, stride, capture, score_thr, palette, what: str):
        """The checked plans of a grouped ``draw_detections`` / ``label_detections`` call, one per listed scene; nothing is launched, and
        where the tensors live is the caller's to check after its own arguments (``_need_device_frames``)."""
        scenes = ops.listed_scenes(self.n_scenes, scenes)
        given = _camera_lists(c2w, extrinsic, what)
        if isinstance(frames, Tensor) or isinstance(results, dict):
            raise ValueError(f"{what} takes one frames tensor and one result per listed scene, as lists")
        frames, results = list(frames), list(results)
        if not len(frames) == len(results) == len(given) == len(scenes):
            raise ValueError(f"{what}: {len(frames)} frame tensors, {len(results)} results and {len(given)} camera lists for {len(scenes)} listed scenes")
        plans = [_plan_detections(self.det, self.metas[s], f, trailing, dtype, r, g if c2w is not None else None, g if c2w is None else None,
                                  window, stride, capture, score_thr, palette, what) for s, f, r, g in zip(scenes, frames, results, given)]
        return plans

    def draw_detections(self, frames, results, c2w=None, extrinsic=None, scenes=None, window=None, stride: int = 1, capture: bool = False,
                        score_thr: float = 0.0, thickness: int = 1, palette=None, depth_frames=None, occluded: str = "hide",
                        depth_bias: float = 0.05, text=None, text_scale: int = 1):
        """:meth:`SceneStream.draw_detections` for the listed scenes: ``frames``, ``results`` and exactly one of ``c2w`` / ``extrinsic`` are
        lists with one entry per listed scene (a frames tensor, a ``detect()`` entry, a list of poses; the counts may differ), and so is
        ``depth_frames`` when given.  Every scene uses its own meta; the other arguments are the call's.  One ndet_project_boxes and one
        ndet_draw_boxes launch per scene (with depth frames or text the stream's other two), as ``pack_frames`` and ``frame_errors`` are
        per scene.  Returns a list of dicts as the stream's method returns them; a group of one scene is the stream bit for bit.  Bad
        arguments are refused whole, before any launch."""
        what = "draw_detections"
        thickness = _check_thickness(thickness, what)
        if depth_frames is not None and not isinstance(depth_frames, (list, tuple)):
            raise ValueError(f"{what} takes depth_frames as a list, one tensor per listed scene")
        plans = self._plan_detections(frames, results, c2w, extrinsic, scenes, (3,), torch.uint8, window, stride, capture, score_thr, palette, what)
        depths = [None] * len(plans) if depth_frames is None else list(depth_frames)
        if len(depths) != len(plans):
            raise ValueError(f"{what}: {len(depths)} depth frame tensors for {len(plans)} listed scenes")
        for p, r, d in zip(plans, list(results), depths):
            _plan_overlay(p, r, d, occluded, depth_bias, text, text_scale, what)
        _need_device_frames(plans, what)
        _need_device_depth(plans, what)
        return [_draw_plan(p, thickness) for p in plans]

    def label_detections(self, depth_frames, results, c2w=None, extrinsic=None, scenes=None, window=None, stride: int = 1, capture: bool = False,
                         score_thr: float = 0.0):
        """:meth:`SceneStream.label_detections` for the listed scenes, the lists as in :meth:`draw_detections`: a list of (k,h,w) int16
        tensors, one ndet_label_frames launch per scene."""
        plans = self._plan_detections(depth_frames, results, c2w, extrinsic, scenes, (), torch.uint16, window, stride, capture, score_thr, None,
                                      "label_detections")
        _need_device_frames(plans, "label_detections")
        return [_label_plan(p) for p in plans]

    def _volumes(self, scenes: List[int]):
        """``(volume (n,C,X,Y,Z), valid (n,1,X,Y,Z) int64)`` of the listed scenes: grouped K2-finish -> one sigma-MLP call over all their
        rows -> grouped K1-finish (channels-last memory); in a windowed group the two finishes are the grouped ring finishes."""
        return self._finishes(scenes)[1:]

    def _finishes(self, scenes: List[int]):
        """The finishes :meth:`_volumes` and :meth:`occupancy` share: ``(alpha (n N,), volume, valid)``, listed scene i's alpha in rows
        ``[i N, (i + 1) N)``."""
        ring = self.window is not None
        points = self.pool.points if ring else self.group.points
        pts = torch.cat([points[s].reshape(3, -1) for s in scenes], dim=1) if len(scenes) > 1 else points[scenes[0]]
        if ring:
            glob = ops.density_finish_group_ring(self.pool, self._lin.bias, scenes)
        else:
            glob = ops.density_finish_group(self.group, self._lin.bias, scenes)
        alpha = _finished_alpha(self.det.nerf_mlp, pts, glob)
        return (alpha,) + (ops.volume_finish_group_ring(self.pool, alpha, scenes) if ring else ops.volume_finish_group(self.group, alpha, scenes))

    def carve_counts(self, scenes=None):
        """Per listed scene :meth:`SceneStream.carve_counts`' ``(free, hit)``.  Needs ``begin_scenes(carve=)`` (else ValueError)."""
        if self.carves is None:
            raise ValueError("carve_counts needs carved scenes: begin_scenes(img_metas, carve=True)")
        out = []
        for s in ops.listed_scenes(self.n_scenes, scenes):
            c = self.carves[s]
            out.append(ops.carve_counts(c.store.segments or [torch.zeros((c.store.n,), dtype=torch.int32, device=self.device)], c.n_voxels))
        return out

    def points(self, min_points: int = 1, results=None, score_thr: float = 0.0, scenes=None):
        """Per listed scene :meth:`SceneStream.points`: a list of dicts.  ``results``: None, or one ``detect()`` result per listed scene.
        Needs ``begin_scenes(cloud=)`` (else ValueError); every check comes before any launch."""
        _need_cloud(self.clouds, "points", "begin_scenes(img_metas, cloud=True)")
        scenes = ops.listed_scenes(self.n_scenes, scenes)
        results = [None] * len(scenes) if results is None else list(results)
        if len(results) != len(scenes):
            raise ValueError(f"points: {len(results)} results for {len(scenes)} listed scenes")
        _check_min_points(min_points)
        for r in results:
            if r is not None:
                _kept_detections(r, score_thr, None, "points")
        return [self.clouds[s].points(min_points, r, score_thr) for s, r in zip(scenes, results)]

    def cloud_sums(self, scenes=None):
        """Per listed scene :meth:`SceneStream.cloud_sums`' dict.  Needs ``begin_scenes(cloud=)`` (else ValueError)."""
        _need_cloud(self.clouds, "cloud_sums", "begin_scenes(img_metas, cloud=True)")
        return [self.clouds[s].sums() for s in ops.listed_scenes(self.n_scenes, scenes)]

    def occupancy(self, threshold: float = 1e-3, dilate: int = 1, outside: str = "keep", scenes=None, *, source: str = "alpha",
                  min_free: int = 2):
        """:meth:`SceneStream.occupancy` for the listed scenes: a list of rays.OccupancyGrid, each scene's own, from ONE run of the grouped
        finishes :meth:`volume` runs over the listed scenes that have no cached grid for these knobs, and one k_occupancy_bits launch
        each.  ``source='depth'`` runs no finish and no MLP: one k_carve_bits call per listed scene over its own counter segments;
        ``'both'`` runs the finishes and ANDs each scene's carve with its undilated alpha grid.  Both need ``begin_scenes(carve=)``.  A
        scene's grid is cached per ``(threshold, dilate, outside)`` -- and ``source``, ``min_free`` for the carved ones -- until
        ``add_views`` / ``add_frames``, an eviction, ``drop_oldest`` or ``reset`` lists the scene.  ValueError for bad knobs or a listed
        scene without views, before any launch."""
        key = _check_occupancy_knobs(threshold, dilate, outside)
        source, min_free = _check_source_knobs(source, min_free)
        _need_carve(self.carves, source, "occupancy")
        scenes = self._need_views(scenes)
        if self._occ is None:
            self._occ = [{} for _ in self.metas]
        thr, dil, out = key
        if source != "alpha":
            key = key + (source, min_free)
        todo = [s for s in scenes if key not in self._occ[s]]
        if todo and source == "depth":
            for s in todo:
                self._occ[s][key] = self.carves[s].grid(min_free, dil, out)
        elif todo:
            points = self.pool.points if self.window is not None else self.group.points
            with torch.no_grad():
                alpha, _, valid = self._finishes(todo)
            n = alpha.numel() // len(todo)
            for i, s in enumerate(todo):
                if source == "alpha":
                    self._occ[s][key] = _make_occupancy(alpha[i * n:(i + 1) * n], valid[i], points[s].view(3, *[int(v) for v in self.det.n_voxels]),
                                                        self.det.n_voxels, self.det.voxel_size, *key)
                else:
                    coarse = ops.occupancy_bits(alpha[i * n:(i + 1) * n], valid[i], self.det.n_voxels, thr, 0)
                    self._occ[s][key] = self.carves[s].grid(min_free, dil, out, coarse)
        return [self._occ[s][key] for s in scenes]

    def _skip_grids(self, skip_empty, scenes: List[int], batched: bool, what: str, *tensors):
        """The listed scenes' grids of a ``skip_empty=`` render (None: no culling) once everything the call refuses has been checked: a
        rays.OccupancyGrid serves every listed scene (the group shares the lattice's size; each scene's first point is its own)."""
        knobs = _skip_knobs(skip_empty, self.det, self.device, what)
        if knobs is None:
            return None
        if batched:
            raise ValueError(f"{what}: batched=True and skip_empty exclude each other for now")
        _check_culled_call(self.det, what, *tensors)
        return self.occupancy(scenes=scenes, **knobs) if isinstance(knobs, dict) else [knobs] * len(scenes)

    def volume(self, scenes=None):
        """Per listed scene ``(volume (C,X,Y,Z), valid (1,X,Y,Z) int64)`` of its views so far, as :meth:`SceneStream.volume` returns them."""
        scenes = self._need_views(scenes)
        with torch.no_grad():
            vol, valid = self._volumes(scenes)
        return [(vol[i], valid[i]) for i in range(len(scenes))]

    def _can_batch(self, vol: Tensor) -> bool:
        """Would neck_3d and the head take their HIP inference paths on ``vol`` in an arithmetic that has batched launches?"""
        det = self.det
        neck, head = det.neck_3d, det.bbox_head
        return (conv3d.ARITHMETIC in conv3d.SPLIT_FAMILY and hasattr(neck, "forward_batched") and hasattr(head, "raws_batched")
                and vol.is_cuda and not neck.training and not head.training and not torch.is_grad_enabled() and vol.shape[1] % 32 == 0
                and head.centerness_conv.in_channels % 32 == 0)

    def detect(self, scenes=None, batched: bool = False):
        """Detections of the listed scenes over their views so far: a list with, per scene, what ``SceneStream.detect()[0]`` returns
        (``dict(boxes_3d, scores_3d, labels_3d)``).  No state is changed.  neck_3d runs once on the scenes' volumes as one batch; every scene's
        tail is queued before the first result is collected, so the host waits once for the queue, not once per scene.  By default neck_3d and
        the tails are still launches per scene (neck_3d walks its batch scene by scene), so the fp16-pair scales of the 3D part are each
        scene's own.  The listed scenes share the stream's range-guard word: when it comes back set with any scene's picks, the whole
        call is repeated on bf16x3 from the finished volumes (``conv3d.guard_trips`` counts it once), so no f16x2 result of a tripped
        launch gets out.

        ``batched=True`` with more than one listed scene: the finished volumes go through neck_3d and the head's convolutions as ONE batch --
        one launch per layer and level for all the scenes (``neck_3d.forward_batched``, ``bbox_head.raws_batched``: ndet_conv_split_batch), one
        amax pass for the volume batch; every scene's tail (decode, selection, NMS) then takes its scene's slice, queued before the host waits
        as above.  The scenes of such a call SHARE the fp16-pair scales of neck_3d and the head, so a scene's detections depend (within the
        chunking contract: same labels in the same order, scores and boxes to 1e-4) on the scenes it is listed with; the volumes and states
        stay bit-equal.  A set guard word repeats the call exactly as the unbatched call is repeated (per scene, on bf16x3): a tripped
        batched call returns a tripped unbatched call's results.  One listed scene, the "f32" arithmetic, or a neck / head that would not
        take its HIP inference path: the unbatched path, bit for bit."""
        scenes = self._need_views(scenes)
        n = len(scenes)
        det = self.det
        with torch.no_grad():
            vol, valid = self._volumes(scenes)
            dev = vol.device
            guarded = conv3d.ARITHMETIC == "f16x2" and vol.is_cuda
            if guarded:
                conv3d.guard_begin(dev)
            batched = bool(batched) and n > 1 and self._can_batch(vol)
            x = det.neck_3d.forward_batched(vol) if batched else det.neck_3d(vol)
            raws = det.bbox_head.raws_batched(x) if batched else None
            metas = [[dict(self.metas[s])] for s in scenes]
            pending, word_rides = [], True
            for i in range(n):
                xi = x if n == 1 else [lvl[i:i + 1] for lvl in x]
                word_rides = word_rides and hasattr(det.bbox_head, "can_fuse") and det.bbox_head.can_fuse(xi)
                pending.append(det._detect_tail(xi, valid[i:i + 1], metas[i], True, guarded, dev, lambda: _TRIPPED,
                                                raws=[r[i] for r in raws] if batched else None))
            # a tail that is not the fused one does not carry the guard word with its picks: read the word once for all of them
            tripped = guarded and not word_rides and conv3d.guard_tripped(dev)
            results = [finish() for finish in pending]
            if tripped or any(r is _TRIPPED for r in results):
                results = _repeat_tails(det, vol, valid, metas)
        return [r[0] for r in results]
