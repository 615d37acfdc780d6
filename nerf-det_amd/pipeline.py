"""Host side of the input contract: the batch ``nerfdet.forward_*`` expects, assembled on
the GPU from decoded frames -- the counterpart of ``ScanNetMultiViewDataset.get_data_info``
(mmdet3d/datasets/scannet_monocular_dataset.py:16-76), ``MultiViewPipeline`` (datasets/pipelines/multi_view.py:13-196),
``get_dtu_raydir`` (data_augment_utils.py:410-424) and ``DefaultFormatBundle3D`` (formating.py:33-117, 216-290).

JPEG / video decoding stays upstream.  The module takes the scene's frames as one uint8 BGR tensor on the device, either already at
network resolution (resized and padded upstream: per step only the selected views are normalised and only the target views get
rays -- two kernel launches instead of 50-100 per-frame numpy passes on the single data-loader worker the reference configures,
config:134), or at CAPTURE resolution: :func:`prepare_frames` / ``MultiViewPipeline(img_scale=, pad_size=)`` then run the configs'
``Resize(keep_ratio) -> Normalize -> Pad`` in one launch (ndet_resize_normalize_views), the resize being
``datasets.imresize_linear`` bit for bit, and report ``img_shape`` / ``pad_shape`` as that chain leaves them.

What a hardware video decoder hands over is not BGR but NV12 surfaces (a Y plane and a half-size plane of interleaved U,V bytes, with a
row pitch and a chroma-plane row of its own choosing): ``prepare_frames(format="nv12")`` / ``MultiViewPipeline(frame_format="nv12")``
take those at capture resolution and convert inside the resize taps (ndet_resize_normalize_views_nv12) -- the BGR call's outputs on
``datasets.nv12_to_bgr`` of each surface bit for bit; :func:`nv12_to_bgr` and :func:`bgr_to_nv12` are the two conversions alone
(ndet_nv12_to_bgr, ndet_bgr_to_nv12), the second for an encoder.

The sensor's depth frames (uint16 millimetres on the device) go the same way: :func:`prepare_depth_frames` is the loader's
``imresize_linear(frame / 1000, ...)`` in float64 (ndet_depth_frames), :func:`positive_indices` its ``flatnonzero(gt_depths > 0)``
(ndet_positive_indices), and ``MultiViewPipeline(...)(..., depth_frames=)`` adds ``depth``, ``gt_depths`` and ``depth_rays`` to the batch.

The output side speaks the same formats: :func:`camera_rays` makes the rays of any camera pose without a frame (ndet_camera_rays:
ndet_target_rays' arithmetic), :func:`pack_frames` turns a render into uint8 BGR and uint16 millimetre frames (ndet_pack_frames), and
:func:`frame_errors` compares two such frames on the device with exact integer sums (ndet_frame_errors) -- what
``SceneStream / SceneGroup.render_frames`` and ``score_frames`` stand on.  :func:`frame_ssim` is the reference's second metric for the
same frames, and for float renders: one fused 7 x 7 window kernel with integer sums per frame and channel (ndet_frame_ssim).

A detection result goes the same way into the camera's image: :func:`project_boxes` says where boxes fall in the frames of given poses
(ndet_project_boxes), :func:`draw_boxes` puts their wireframes onto frames in device memory (ndet_draw_boxes) and :func:`label_frames` says
which box each pixel of a depth frame belongs to (ndet_label_frames) -- what ``draw_detections`` and ``label_detections`` stand on.
:func:`draw_overlay` is :func:`draw_boxes` with the edges depth-tested against a millimetre depth frame and with the class and the score
written on a plate above each box (ndet_draw_overlay; ``project_boxes(depths=True)``, ndet_project_boxes_w, gives the edges' depths;
:data:`FONT_5X7` and :func:`encode_texts` the glyphs and the codes).
"""
from __future__ import annotations

from ctypes import c_void_p
from typing import Sequence

import numpy as np
import torch

from . import _lib
from ._lib import _ptr, check

IMG_MEAN = (123.675, 116.28, 103.53)   # configs/nerfdet/*.py img_norm_cfg (RGB)
IMG_STD = (58.395, 57.12, 57.375)


def get_dtu_raydir(pixelcoords, intrinsic, rot, dir_norm=None):
    """Same signature and arithmetic as the reference helper (numpy): un-normalised camera rays rotated to the world."""
    x = (pixelcoords[..., 0] + 0.5 - intrinsic[0, 2]) / intrinsic[0, 0]
    y = (pixelcoords[..., 1] + 0.5 - intrinsic[1, 2]) / intrinsic[1, 1]
    dirs = np.stack([x, y, np.ones_like(x)], axis=-1) @ rot[:, :].T
    if dir_norm:
        dirs = dirs / (np.linalg.norm(dirs, axis=-1, keepdims=True) + 1e-5)
    return dirs


def scene_cameras(info: dict) -> dict:
    """The camera part of ``get_data_info``: ``extrinsic = inv(axis_align @ pose)`` (world -> camera), ``c2w``, its rotation
    and translation (``camrotc2w``, ``lightpos``), the fp32 intrinsics and the fixed voxel origin (0, 0, 0.5)."""
    axis_align = np.asarray(info["annos"]["axis_align_matrix"]).astype(np.float32)
    c2w = [(axis_align @ np.asarray(p)).astype(np.float32) for p in info["extrinsics"]]
    return dict(extrinsic=[np.linalg.inv(axis_align @ np.asarray(p)).astype(np.float32) for p in info["extrinsics"]],
                intrinsic=np.asarray(info["intrinsics"]).astype(np.float32), origin=np.array([.0, .0, .5], dtype=np.float32),
                c2w=c2w, camrotc2w=[m[0:3, 0:3] for m in c2w], lightpos=[m[0:3, 3] for m in c2w])


def select_views(n_frames: int, n_images: int, nerf_target_views: int, loading: str = "random", sample_freq: int = 3):
    """View sampling of ``MultiViewPipeline`` (multi_view.py:60-83) on numpy's global RNG stream, like the reference:
    'random' draws ``n_images`` (with replacement only when the scene is shorter), takes ``nerf_target_views`` of them as
    NeRF targets and removes those from the sources with ``setdiff1d`` (which also sorts and de-duplicates); any other
    mode takes every ``sample_freq``-th frame and uses all of them as targets too."""
    if loading == "random":
        ids = np.random.choice(np.arange(n_frames), n_images, replace=n_images > n_frames)
        if nerf_target_views == 0:
            return ids.tolist(), []
        target = np.random.choice(ids, nerf_target_views, replace=False)
        return np.setdiff1d(ids, target).tolist(), target.tolist()
    ids = np.arange(0, n_images * sample_freq, sample_freq).tolist()
    return ids, (list(ids) if nerf_target_views != 0 else [])


def rescale_size(size_hw, img_scale):
    """``(Hr, Wr)`` of ``datasets.Resize(img_scale, keep_ratio=True)`` on an ``(Hs, Ws)`` frame (mmcv.imrescale): the largest rescale that
    fits the long edge into ``max(img_scale)`` and the short edge into ``min(img_scale)``, each new edge rounded half up."""
    h, w = int(size_hw[0]), int(size_hw[1])
    if h < 1 or w < 1 or len(img_scale) != 2 or min(img_scale) <= 0:
        raise ValueError(f"rescale_size: frame {tuple(size_hw)} and img_scale {tuple(img_scale)} must be positive")
    s = min(max(img_scale) / max(h, w), min(img_scale) / min(h, w))
    return int(h * s + 0.5), int(w * s + 0.5)


def _frame_sizes(size_hw, img_scale, pad_size):
    """``(Hr, Wr), (H, W)`` of a capture-size frame through Resize(keep_ratio) and Pad(size=pad_size); ValueError when it does not fit."""
    hr, wr = rescale_size(size_hw, img_scale)
    h, w = int(pad_size[0]), int(pad_size[1])
    if hr < 1 or wr < 1 or hr > h or wr > w:
        raise ValueError(f"a {tuple(size_hw)} frame rescales to {(hr, wr)} at img_scale {tuple(img_scale)}, which does not fit pad_size {(h, w)}")
    return (hr, wr), (h, w)


FRAME_FORMATS = ("bgr", "nv12")


def _check_format(format, what: str) -> str:
    if format not in FRAME_FORMATS:
        raise ValueError(f"{what}: format={format!r} must be one of {FRAME_FORMATS}")
    return format


def surface_layout(rows: int, pitch: int, size, uv_row, what: str):
    """The checked description ``(Hs, Ws, uv_row)`` of NV12 surfaces of ``rows`` rows of ``pitch`` bytes: the Y plane ``size = (Hs, Ws)``,
    both even, in rows [0, Hs), the interleaved U,V plane in rows [uv_row, uv_row + Hs / 2) (``uv_row=None``: Hs, the tight layout).
    ValueError for a layout the surfaces cannot hold and for an odd pitch (ndet_resize_normalize_views_nv12 loads a UV pair at once);
    only integers are read."""
    if size is None or len(size) < 2:
        raise ValueError(f"{what}: NV12 surfaces need size=(Hs, Ws), the size of their Y plane")
    hs, ws = int(size[0]), int(size[1])
    if hs < 2 or ws < 2 or hs % 2 or ws % 2:
        raise ValueError(f"{what}: an NV12 surface has even sizes, got {(hs, ws)}")
    uv = hs if uv_row is None else int(uv_row)
    if pitch < ws:
        raise ValueError(f"{what}: surfaces of pitch {pitch} do not hold rows of {ws} pixels")
    if uv < hs:
        raise ValueError(f"{what}: uv_row={uv} lies inside the Y plane of {hs} rows")
    if rows < uv + hs // 2:
        raise ValueError(f"{what}: surfaces of {rows} rows do not hold a {hs}-row Y plane and its {hs // 2} UV rows at row {uv}")
    if pitch % 2:
        raise ValueError(f"{what}: an odd pitch ({pitch}) is not supported")
    if rows * pitch >= 1 << 31:
        raise ValueError(f"{what}: a surface of {rows} rows x {pitch} bytes holds 2^31 bytes or more")
    return hs, ws, uv


def _check_surfaces(frames, size, uv_row, what: str):
    """ValueError for anything but contiguous (n, rows, pitch) uint8 surfaces that hold the described planes: ``(n, rows, pitch, Hs, Ws, uv_row)``."""
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 3 or 0 in frames.shape or not frames.is_contiguous():
        got = f"{tuple(frames.shape)} {frames.dtype}" if isinstance(frames, torch.Tensor) else type(frames).__name__
        raise ValueError(f"{what} takes contiguous (n, rows, pitch) uint8 NV12 surfaces, got {got}")
    n, rows, pitch = (int(v) for v in frames.shape)
    return (n, rows, pitch) + surface_layout(rows, pitch, size, uv_row, what)


def _device_ids(ids, n: int, dev, what: str):
    """``(ids on the device or None, n_sel)`` of a call that selects frames."""
    if ids is None:
        return None, n
    ids = [int(i) for i in ids]
    if not ids or min(ids) < 0 or max(ids) >= n:
        raise ValueError(f"{what}: ids must be a non-empty list of frame indices below {n}")
    return torch.tensor(ids, dtype=torch.int32, device=dev), len(ids)


def prepare_frames(frames: torch.Tensor, img_scale, pad_size, mean: Sequence[float] = IMG_MEAN, std: Sequence[float] = IMG_STD, ids=None,
                   want_u8: bool = False, format: str = "bgr", size=None, uv_row=None):
    """The configs' ``Resize(img_scale, keep_ratio=True) -> Normalize(mean, std, to_rgb=True) -> Pad(size=pad_size)`` and the reference's
    de-normalised copy for frames at capture resolution, in one launch: ``frames`` (n, Hs, Ws, 3) uint8 BGR on the device ->
    ``(img, denorm)``, both (n_sel, 3, H, W) float32 (``ids``: a sequence of frame indices, None for every frame in order), and with
    ``want_u8`` also the resized, zero-padded bytes (n_sel, H, W, 3).  The content region holds ``datasets.imresize_linear``'s bytes
    normalised as ``ndet_normalize_views`` does; the pad is 0 in ``img`` and ``trunc(mean) / 255`` in ``denorm``.  ValueError when the
    rescaled frame does not fit ``pad_size`` (a portrait frame into a landscape pad).

    ``format="nv12"``: ``frames`` are a video decoder's surfaces, (n, rows, pitch) uint8 with the Y plane ``size = (Hs, Ws)`` in rows
    [0, Hs) and the interleaved U,V plane from row ``uv_row`` (None: Hs, the tight layout; :func:`surface_layout`).  One
    ndet_resize_normalize_views_nv12 launch converts inside the resize taps: the outputs are the BGR call's on
    ``datasets.nv12_to_bgr`` of each surface, bit for bit, and no BGR frame at capture size is ever written."""
    what = "prepare_frames"
    if _check_format(format, what) == "nv12":
        n, rows, pitch, hs, ws, uv = _check_surfaces(frames, size, uv_row, what)
    else:
        if size is not None or uv_row is not None:
            raise ValueError("prepare_frames: size= and uv_row= describe NV12 surfaces (format='nv12')")
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3 or not frames.is_contiguous():
            raise ValueError(f"prepare_frames takes contiguous (n, Hs, Ws, 3) uint8 frames, got {tuple(frames.shape)} {frames.dtype}")
        n, hs, ws, _ = frames.shape
    (hr, wr), (h, w) = _frame_sizes((hs, ws), img_scale, pad_size)
    if not frames.is_cuda:
        raise RuntimeError("nerfdet_amd.pipeline: frames must live on the GPU (no CPU fallback)")
    dev = frames.device
    ids_d, n_sel = _device_ids(ids, n, dev, what)
    mean, std = np.asarray(mean, dtype=np.float64), np.asarray(std, dtype=np.float64)
    img = torch.empty((n_sel, 3, h, w), dtype=torch.float32, device=dev)
    denorm = torch.empty_like(img)
    u8 = torch.empty((n_sel, h, w, 3), dtype=torch.uint8, device=dev) if want_u8 else None
    tail = (hr, wr, h, w, mean.ctypes.data_as(c_void_p), std.ctypes.data_as(c_void_p), _ptr(img), _ptr(denorm), _ptr(u8), c_void_p(_lib.raw_stream(dev)))
    if format == "nv12":
        check(_lib.load().ndet_resize_normalize_views_nv12(_ptr(frames), _ptr(ids_d), n_sel, hs, ws, pitch, uv, rows, *tail), "resize_normalize_views_nv12")
    else:
        check(_lib.load().ndet_resize_normalize_views(_ptr(frames), _ptr(ids_d), n_sel, hs, ws, *tail), "resize_normalize_views")
    return (img, denorm, u8) if want_u8 else (img, denorm)


def nv12_to_bgr(frames: torch.Tensor, size, uv_row=None, ids=None) -> torch.Tensor:
    """NV12 surfaces as BGR frames at full size, in one launch (ndet_nv12_to_bgr): ``frames`` (n, rows, pitch) uint8 on the device,
    described by ``size = (Hs, Ws)`` and ``uv_row`` as :func:`prepare_frames` takes them -> (n_sel, Hs, Ws, 3) uint8,
    ``datasets.nv12_to_bgr`` of each selected surface bit for bit.  For what needs capture-size BGR, ``draw_detections(capture=True)``
    for one; the ingest road does not (``prepare_frames(format="nv12")`` converts inside the resize)."""
    what = "nv12_to_bgr"
    n, rows, pitch, hs, ws, uv = _check_surfaces(frames, size, uv_row, what)
    if hs * ws * 3 >= 1 << 31:
        raise ValueError(f"{what}: a frame of {hs} x {ws} x 3 holds 2^31 elements or more")
    if not frames.is_cuda:
        raise RuntimeError("nerfdet_amd.pipeline: frames must live on the GPU (no CPU fallback)")
    dev = frames.device
    ids_d, n_sel = _device_ids(ids, n, dev, what)
    out = torch.empty((n_sel, hs, ws, 3), dtype=torch.uint8, device=dev)
    check(_lib.load().ndet_nv12_to_bgr(_ptr(frames), _ptr(ids_d), n_sel, hs, ws, pitch, uv, rows, _ptr(out), c_void_p(_lib.raw_stream(dev))), what)
    return out


def bgr_to_nv12(frames: torch.Tensor):
    """BGR frames as the NV12 surfaces a hardware encoder takes, in one launch (ndet_bgr_to_nv12): ``frames`` (n, H, W, 3) uint8 on the
    device, of ANY size -- ``render_frames``' and ``draw_detections``' outputs fit -- -> ``(surfaces (n, He * 3 / 2, We) uint8, (He, We))``
    in the tight layout, ``He = H + H % 2``, ``We = W + W % 2`` (the last row / column replicated): ``datasets.bgr_to_nv12`` of each
    frame bit for bit, Y in rows [0, He), interleaved U,V from row He."""
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3 or 0 in frames.shape \
            or not frames.is_contiguous():
        got = f"{tuple(frames.shape)} {frames.dtype}" if isinstance(frames, torch.Tensor) else type(frames).__name__
        raise ValueError(f"bgr_to_nv12 takes contiguous (n, H, W, 3) uint8 frames, got {got}")
    n, h, w = (int(v) for v in frames.shape[:3])
    if h * w * 3 >= 1 << 31:
        raise ValueError(f"bgr_to_nv12: a frame of {h} x {w} x 3 holds 2^31 elements or more")
    if not frames.is_cuda:
        raise RuntimeError("nerfdet_amd.pipeline: frames must live on the GPU (no CPU fallback)")
    he, we = h + h % 2, w + w % 2
    out = torch.empty((n, he // 2 * 3, we), dtype=torch.uint8, device=frames.device)
    check(_lib.load().ndet_bgr_to_nv12(_ptr(frames), n, h, w, _ptr(out), c_void_p(_lib.raw_stream(frames.device))), "bgr_to_nv12")
    return out, (he, we)


def _check_depth_frames(depth_frames, what: str, n_frames=None):
    """ValueError for anything but contiguous (n, Hd, Wd) uint16 on the GPU (``n_frames`` given: with that n); only the descriptor is read."""
    if (not isinstance(depth_frames, torch.Tensor) or depth_frames.dtype != torch.uint16 or depth_frames.dim() != 3 or 0 in depth_frames.shape
            or not depth_frames.is_contiguous() or not depth_frames.is_cuda):
        got = f"{tuple(depth_frames.shape)} {depth_frames.dtype} on {depth_frames.device}" if isinstance(depth_frames, torch.Tensor) else type(depth_frames).__name__
        raise ValueError(f"{what} takes contiguous (n, Hd, Wd) torch.uint16 depth frames (millimetres) on the GPU, got {got}")
    if n_frames is not None and depth_frames.shape[0] != n_frames:
        raise ValueError(f"{what}: {depth_frames.shape[0]} depth frames for {n_frames} colour frames")


def prepare_depth_frames(depth_frames: torch.Tensor, size_hw, ids=None, margin: int = 0) -> torch.Tensor:
    """The loader's depth maps from the sensor's frames, in one launch (ndet_depth_frames): ``depth_frames`` (n, Hd, Wd) uint16
    millimetres on the device -> ``datasets.imresize_linear(frame / 1000, (w, h))`` in float64 metres, bit for bit (what
    ``datasets.MultiViewPipeline._depth`` makes of the PNG), cropped to ``[margin, h - margin) x [margin, w - margin)``:
    ``(n_sel, h - 2 * margin, w - 2 * margin)`` float64.  ``size_hw = (h, w)``; ``ids``: a sequence of frame indices, None for every frame in
    order.  ValueError for anything but contiguous (n, Hd, Wd) ``torch.uint16`` on the GPU, for bad ``ids`` and for a margin that leaves
    no pixel."""
    _check_depth_frames(depth_frames, "prepare_depth_frames")
    n, hd, wd = depth_frames.shape
    h, w, m = int(size_hw[0]), int(size_hw[1]), int(margin)
    if h < 1 or w < 1 or m < 0 or 2 * m >= h or 2 * m >= w:
        raise ValueError(f"prepare_depth_frames: margin {m} leaves no pixel of a {(h, w)} map")
    dev = depth_frames.device
    ids_d = None
    if ids is not None:
        ids = [int(i) for i in ids]
        if not ids or min(ids) < 0 or max(ids) >= n:
            raise ValueError(f"prepare_depth_frames: ids must be a non-empty list of frame indices below {n}")
        ids_d = torch.tensor(ids, dtype=torch.int32, device=dev)
    n_sel = n if ids is None else len(ids)
    out = torch.empty((n_sel, h - 2 * m, w - 2 * m), dtype=torch.float64, device=dev)
    check(_lib.load().ndet_depth_frames(_ptr(depth_frames), _ptr(ids_d), n_sel, hd, wd, h, w, m, _ptr(out), c_void_p(_lib.raw_stream(dev))),
          "depth_frames")
    return out


def positive_indices(x: torch.Tensor) -> torch.Tensor:
    """``flatnonzero(x > 0)`` of a float64 tensor on the device, as the loader leaves ``depth_rays`` (datasets.DefaultFormatBundle3D): (K,)
    int64, ascending, from one launch (ndet_positive_indices) and one 8-byte read of the count -- the only synchronisation."""
    if x.dtype != torch.float64 or not x.is_cuda or not x.is_contiguous() or x.numel() == 0:
        raise ValueError(f"positive_indices takes a contiguous, non-empty float64 tensor on the GPU, got {tuple(x.shape)} {x.dtype}")
    lib, dev, n = _lib.load(), x.device, x.numel()
    if n >= 2 ** 31:
        raise ValueError(f"positive_indices: {n} elements, 2^31 or more")
    idx = torch.empty(n, dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    ws = torch.empty(lib.ndet_positive_indices_workspace_bytes(n), dtype=torch.uint8, device=dev)
    check(lib.ndet_positive_indices(_ptr(x), n, _ptr(idx), _ptr(count), _ptr(ws), c_void_p(_lib.raw_stream(dev))), "positive_indices")
    k = int(count.item())
    if k < 0:
        raise _lib.NdetError("positive_indices: a wait inside the scan ran out of polls")
    return idx[:k]


def check_window(window, stride) -> tuple:
    """``(y0, x0, h, w), stride`` of a ray grid as ints: offsets >= 0, an h x w output of at least one pixel, stride >= 1; else ValueError."""
    ok = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)
    if not ok(stride) or stride < 1:
        raise ValueError(f"stride={stride!r} must be an int of at least 1")
    if not isinstance(window, (tuple, list)) or len(window) != 4 or not all(ok(v) for v in window):
        raise ValueError(f"window={window!r} must be (y0, x0, h, w), four ints")
    y0, x0, h, w = (int(v) for v in window)
    if y0 < 0 or x0 < 0 or h < 1 or w < 1:
        raise ValueError(f"window {(y0, x0, h, w)} is empty or starts before pixel 0")
    return (y0, x0, h, w), int(stride)


def _host_matrices(mats, what: str) -> np.ndarray:
    """``n >= 1`` matrices of 4 x 4 (a list of numpy arrays or tensors, or one (n,4,4) array or tensor) as one float64-exact numpy array."""
    if isinstance(mats, torch.Tensor):
        mats = mats.detach().cpu().numpy()
    elif not isinstance(mats, np.ndarray):
        mats = [m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m) for m in mats]
        if not mats or any(m.shape != (4, 4) for m in mats):
            raise ValueError(f"{what} must hold at least one 4 x 4 matrix")
        mats = np.stack(mats)
    if mats.ndim != 3 or mats.shape[0] < 1 or mats.shape[1:] != (4, 4):
        raise ValueError(f"{what} must be n >= 1 matrices of 4 x 4, got {mats.shape}")
    return mats


def camera_rays(intrinsic, c2w, window, stride: int = 1, device=None):
    """The rays of n camera poses that need no frame: ``(ray_o, ray_d)``, each (n, h * w, 3) float32 on the device, from one launch
    (ndet_camera_rays).  ``intrinsic``: the 3 x 3 or 4 x 4 intrinsics already scaled to the image grid; ``c2w``: n camera-to-world matrices
    of 4 x 4, numpy or tensors, as in ``scene_cameras(info)["c2w"]``; ``window = (y0, x0, h, w)``: output pixel (i, j) looks through image
    pixel ``(y0 + i * stride, x0 + j * stride)`` -- the image has no bound here, a pose may look anywhere.  ``ray_d`` is ``get_dtu_raydir``
    in ndet_target_rays' float32 operation order (bit for bit its ``raydirs`` for the same pixels), ``ray_o`` the camera centre repeated.
    ``device``: the GPU to work on (default: the current one).  ValueError for wrong shapes, RuntimeError without a GPU (no CPU fallback)."""
    (y0, x0, h, w), stride = check_window(window, stride)
    k = intrinsic.detach().cpu().numpy() if isinstance(intrinsic, torch.Tensor) else np.asarray(intrinsic)
    if k.shape not in ((3, 3), (4, 4)):
        raise ValueError(f"camera_rays takes 3 x 3 or 4 x 4 intrinsics, got {k.shape}")
    m = _host_matrices(c2w, "camera_rays: c2w").astype(np.float32)
    n = m.shape[0]
    if n * h * w * 3 >= 2 ** 31:
        raise ValueError(f"camera_rays: {n} cameras of {h} x {w} rays hold 2^31 elements or more")
    if device is None and isinstance(c2w, torch.Tensor) and c2w.is_cuda:
        device = c2w.device
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("nerfdet_amd.pipeline: camera rays are made on the GPU (no CPU fallback)")
    # one upload: 6 intrinsic floats, then the n rotations, then the n centres
    host = np.concatenate([np.ascontiguousarray(k[:2, :3], dtype=np.float32).reshape(-1), m[:, :3, :3].reshape(-1), m[:, :3, 3].reshape(-1)])
    buf = torch.from_numpy(host).to(dev)
    ray_o = torch.empty((n, h * w, 3), dtype=torch.float32, device=dev)
    ray_d = torch.empty_like(ray_o)
    check(_lib.load().ndet_camera_rays(_ptr(buf), _ptr(buf[6:]), _ptr(buf[6 + 9 * n:]), n, x0, y0, stride, h, w, _ptr(ray_o), _ptr(ray_d),
                                       c_void_p(_lib.raw_stream(dev))), "camera_rays")
    return ray_o, ray_d


def pack_frames(rgb: torch.Tensor, depth: torch.Tensor, mask, shape):
    """A render as the formats ``add_frames`` takes: ``(frames (n,h,w,3) uint8, depth_frames (n,h,w) uint16 millimetres)`` from one launch
    (ndet_pack_frames).  ``rgb`` float32 with ``n * h * w`` rows of 3, ``depth`` float32 metres and ``mask`` bool (or None: all true) with
    as many elements, ``shape = (n, h, w)``.  Bytes are ``x * 255`` rounded half up and saturated (NaN: 0), in the channel order given --
    a view bank's images are BGR planes, so a render from one is BGR already; millimetres are ``depth * 1000`` rounded half up, saturated at
    65535, and 0 -- the sensor's hole -- where ``mask`` is false.  ValueError for wrong shapes or dtypes, RuntimeError for CPU tensors."""
    if len(tuple(shape)) != 3 or min(int(v) for v in shape) < 1:
        raise ValueError(f"pack_frames: shape {tuple(shape)} must be (n, h, w), all positive")
    n, h, w = (int(v) for v in shape)
    rows = n * h * w
    for t, name, dtype, numel in ((rgb, "rgb", torch.float32, rows * 3), (depth, "depth", torch.float32, rows), (mask, "mask", torch.bool, rows)):
        if t is None and name == "mask":
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.numel() != numel or not t.is_contiguous():
            got = f"{tuple(t.shape)} {t.dtype}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"pack_frames takes {name} as a contiguous {dtype} tensor of {numel} elements for frames {(n, h, w)}, got {got}")
    if rgb.shape[-1] != 3:
        raise ValueError(f"pack_frames takes rgb as rows of 3, got {tuple(rgb.shape)}")
    if rows * 3 >= 2 ** 31:
        raise ValueError(f"pack_frames: {rows} pixels, 2^31 colour elements or more")
    if not rgb.is_cuda or depth.device != rgb.device or (mask is not None and mask.device != rgb.device):
        raise RuntimeError("nerfdet_amd.pipeline: renders must live on the GPU (no CPU fallback)")
    dev = rgb.device
    frames = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    depth_frames = torch.empty((n, h, w), dtype=torch.uint16, device=dev)
    check(_lib.load().ndet_pack_frames(_ptr(rgb), _ptr(depth), _ptr(mask), rows, _ptr(frames), _ptr(depth_frames), c_void_p(_lib.raw_stream(dev))),
          "pack_frames")
    return frames, depth_frames


def frame_errors(frames_a: torch.Tensor, frames_b: torch.Tensor, depth_a: torch.Tensor, depth_b=None) -> dict:
    """Frames a (a render) against frames b (held-out camera frames) on the device: ``frames_*`` (n, h, w, 3) uint8, ``depth_*`` (n, h, w)
    uint16 millimetres, ``depth_b`` optional.  One launch behind a memset node (ndet_frame_errors) gives, per frame and as (n,) int64
    device tensors, ``sse`` = sum (a - b)^2 over the bytes of the pixels where a has depth (``depth_a != 0``), ``n_px`` their number,
    ``depth_sad_mm`` = sum |depth_a - depth_b| over the pixels where both have depth and ``n_depth`` their number (both 0 without
    ``depth_b``) -- integer sums, the same bytes on every call -- and ``psnr`` (n,) float64 = 10 log10(255^2 * 3 * n_px / sse), by torch on
    the device: inf where ``sse == 0``, nan where ``n_px == 0``.  ValueError for wrong shapes or dtypes, RuntimeError for CPU tensors."""
    a, b = frames_a, frames_b
    if (not isinstance(a, torch.Tensor) or not isinstance(b, torch.Tensor) or a.dtype != torch.uint8 or b.dtype != torch.uint8 or a.dim() != 4
            or a.shape[-1] != 3 or 0 in a.shape or b.shape != a.shape or not a.is_contiguous() or not b.is_contiguous()):
        raise ValueError(f"frame_errors takes two contiguous (n, h, w, 3) uint8 tensors of one shape, got "
                         f"{tuple(getattr(a, 'shape', ()))} {getattr(a, 'dtype', None)} and {tuple(getattr(b, 'shape', ()))} {getattr(b, 'dtype', None)}")
    for d, name in ((depth_a, "depth_a"), (depth_b, "depth_b")):
        if d is None and name == "depth_b":
            continue
        if not isinstance(d, torch.Tensor) or d.dtype != torch.uint16 or d.shape != a.shape[:3] or not d.is_contiguous():
            got = f"{tuple(d.shape)} {d.dtype}" if isinstance(d, torch.Tensor) else type(d).__name__
            raise ValueError(f"frame_errors takes {name} as a contiguous {tuple(a.shape[:3])} uint16 tensor (millimetres), got {got}")
    n, px = int(a.shape[0]), int(a.shape[1]) * int(a.shape[2])
    if n * px * 3 >= 2 ** 31:
        raise ValueError(f"frame_errors: {n} frames of {px} pixels hold 2^31 elements or more")
    if not a.is_cuda or any(t is not None and t.device != a.device for t in (b, depth_a, depth_b)):
        raise RuntimeError("nerfdet_amd.pipeline: frames must live on the GPU (no CPU fallback)")
    dev = a.device
    out = torch.empty((n, 4), dtype=torch.int64, device=dev)
    check(_lib.load().ndet_frame_errors(_ptr(a), _ptr(b), _ptr(depth_a), _ptr(depth_b), n, px, _ptr(out), c_void_p(_lib.raw_stream(dev))),
          "frame_errors")
    sse, n_px = out[:, 0], out[:, 1]
    psnr = 10.0 * torch.log10(255.0 ** 2 * 3.0 * n_px.to(torch.float64) / sse.to(torch.float64))
    return dict(sse=sse, n_px=n_px, depth_sad_mm=out[:, 2], n_depth=out[:, 3], psnr=psnr)


SSIM_TILE = (16, 32)     # window rows and columns a workgroup of k_frame_ssim owns (SSIM_TH, SSIM_TW in csrc/frame_ssim_kernels.hip)
SSIM_WINDOW = 7


def frame_ssim(frames_a: torch.Tensor, frames_b: torch.Tensor, depth_a=None) -> dict:
    """The structural similarity of frames a (a render) and frames b (held-out frames) on the device, the reference's second render metric
    (save_rendered_img.py:21-36: scikit-image 0.18.1's ``structural_similarity(multichannel=True)`` -- 7 x 7 uniform window, sample
    covariance, K1 = 0.01, K2 = 0.03, data range 2, the window-valid interior).  ``frames_*`` (n, h, w, 3), both uint8 (bytes, scored as
    x / 255) or both float32; ``depth_a`` optionally (n, h, w) uint16: a window counts only if all its 49 pixels have ``depth_a != 0``.  One
    launch behind a memset node (ndet_frame_ssim, which states the arithmetic) gives ``ssim_sum`` (n, 3) int64 -- per channel the sum over
    the counting windows of ``llrint(s * 2^40)`` -- and ``n_windows`` (n,) int64; for bytes every box sum is an exact integer and the sums
    are the same bytes on every call, whatever the tiling.  By torch on the device, in float64: ``ssim_channels`` (n, 3) =
    ``ssim_sum / (2^40 n_windows)`` and ``ssim`` (n,) their mean, nan where ``n_windows == 0``.  ValueError for wrong shapes or dtypes and
    for h or w below 7, RuntimeError for CPU tensors."""
    a, b = frames_a, frames_b
    if (not isinstance(a, torch.Tensor) or not isinstance(b, torch.Tensor) or a.dtype not in (torch.uint8, torch.float32) or b.dtype != a.dtype
            or a.dim() != 4 or a.shape[-1] != 3 or 0 in a.shape or b.shape != a.shape or not a.is_contiguous() or not b.is_contiguous()):
        raise ValueError(f"frame_ssim takes two contiguous (n, h, w, 3) tensors of one shape, both uint8 or both float32, got "
                         f"{tuple(getattr(a, 'shape', ()))} {getattr(a, 'dtype', None)} and {tuple(getattr(b, 'shape', ()))} {getattr(b, 'dtype', None)}")
    if depth_a is not None and (not isinstance(depth_a, torch.Tensor) or depth_a.dtype != torch.uint16 or depth_a.shape != a.shape[:3]
                                or not depth_a.is_contiguous()):
        got = f"{tuple(depth_a.shape)} {depth_a.dtype}" if isinstance(depth_a, torch.Tensor) else type(depth_a).__name__
        raise ValueError(f"frame_ssim takes depth_a as a contiguous {tuple(a.shape[:3])} uint16 tensor (millimetres), got {got}")
    n, h, w = (int(v) for v in a.shape[:3])
    if h < SSIM_WINDOW or w < SSIM_WINDOW:
        raise ValueError(f"frame_ssim: frames of {h} x {w} pixels hold no {SSIM_WINDOW} x {SSIM_WINDOW} window")
    if (h - SSIM_WINDOW + 1) * (w - SSIM_WINDOW + 1) >= 2 ** 22:
        raise ValueError(f"frame_ssim: frames of {h} x {w} pixels hold 2^22 windows or more")
    if n * h * w * 3 >= 2 ** 31:
        raise ValueError(f"frame_ssim: {n} frames of {h} x {w} pixels hold 2^31 elements or more")
    if not a.is_cuda or b.device != a.device or (depth_a is not None and depth_a.device != a.device):
        raise RuntimeError("nerfdet_amd.pipeline: frames must live on the GPU (no CPU fallback)")
    dev = a.device
    out = torch.empty((n, 4), dtype=torch.int64, device=dev)
    check(_lib.load().ndet_frame_ssim(_ptr(a), _ptr(b), _ptr(depth_a), 0 if a.dtype == torch.uint8 else 1, n, h, w, _ptr(out),
                                      c_void_p(_lib.raw_stream(dev))), "frame_ssim")
    ssim_sum, n_windows = out[:, :3], out[:, 3]
    ssim_channels = ssim_sum.to(torch.float64) / (float(2 ** 40) * n_windows.to(torch.float64)).unsqueeze(1)
    # elementwise, one rounding per operation, in this order; a tensor divisor, for torch multiplies by the reciprocal of a scalar one
    ssim = (ssim_channels[:, 0] + ssim_channels[:, 1] + ssim_channels[:, 2]) / torch.full_like(n_windows, 3, dtype=torch.float64)
    return dict(ssim_sum=ssim_sum, n_windows=n_windows, ssim_channels=ssim_channels, ssim=ssim)


# BGR, one colour a class, repeated beyond the table (the 18 ScanNet classes get 18 distinct colours)
PALETTE_BGR = ((75, 25, 230), (75, 180, 60), (25, 225, 255), (200, 130, 0), (48, 130, 245), (180, 30, 145), (240, 240, 70), (230, 50, 240),
               (60, 245, 210), (212, 190, 250), (128, 128, 0), (255, 190, 220), (40, 110, 170), (200, 250, 255), (0, 0, 128), (195, 255, 170),
               (0, 128, 128), (180, 215, 255))


def class_palette(n: int) -> np.ndarray:
    """``(n, 3)`` uint8 BGR colours, one a class: the fixed table ``PALETTE_BGR`` repeated."""
    if not isinstance(n, (int, np.integer)) or isinstance(n, bool) or n < 1:
        raise ValueError(f"class_palette takes a positive int, got {n!r}")
    table = np.asarray(PALETTE_BGR, dtype=np.uint8)
    return table[np.arange(int(n)) % len(table)]


def _gpu(device, given=None) -> torch.device:
    """The GPU a wrapper works on: ``device``, else ``given``'s when that is a device tensor, else the current one; RuntimeError without one."""
    if device is None and isinstance(given, torch.Tensor) and given.is_cuda:
        device = given.device
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("nerfdet_amd.pipeline: detections are projected, drawn and labelled on the GPU (no CPU fallback)")
    return dev


def _intrinsic_rows(intrinsic, what: str) -> np.ndarray:
    k = intrinsic.detach().cpu().numpy() if isinstance(intrinsic, torch.Tensor) else np.asarray(intrinsic)
    if k.shape not in ((3, 3), (4, 4)):
        raise ValueError(f"{what} takes 3 x 3 or 4 x 4 intrinsics, got {k.shape}")
    return np.ascontiguousarray(k[:2, :3], dtype=np.float32).reshape(-1)


def _host_f32(a, shape_tail: tuple, what: str) -> np.ndarray:
    """``a`` (numpy or tensor) as a float32 numpy array of shape (n >= 1,) + shape_tail; else ValueError."""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    if a.ndim != 1 + len(shape_tail) or a.shape[0] < 1 or tuple(a.shape[1:]) != shape_tail or a.dtype.kind != "f":
        raise ValueError(f"{what} must be a float array of shape (n >= 1,) + {shape_tail}, got {a.shape} {a.dtype}")
    return np.ascontiguousarray(a, dtype=np.float32)


def project_boxes(intrinsic, corners, window, stride: int = 1, c2w=None, extrinsic=None, near: float = 0.1, device=None, depths: bool = False) -> dict:
    """Where n boxes fall in the frames of k camera poses: one launch (ndet_project_boxes), one small upload, nothing read back.
    ``intrinsic``: 3 x 3 or 4 x 4, scaled to the image grid; ``corners`` (n, 8, 3) float, as ``boxes.box_corners`` makes them;
    ``window = (y0, x0, h, w)`` and ``stride`` as in :func:`camera_rays`; exactly one of ``c2w`` (k camera-to-world 4 x 4, inverted on the host
    in float64 and rounded to float32) and ``extrinsic`` (k world-to-camera 4 x 4, taken as given); ``near`` > 0 in metres, the plane edges are
    clipped at.  Returns ``dict(edges (k,n,12,4) int32, edge_mask (k,n) int32, rect (k,n,4) int32, zrange (k,n,2) float32, window, stride)``
    on the device, as include/nerfdet_hip.h defines them.  ``depths=True`` makes the launch ndet_project_boxes_w: the same tables bit for
    bit and ``edge_w (k,n,12,2) float32``, the reciprocal camera z of every surviving edge's ends after the near clip, which
    :func:`draw_overlay`'s depth test needs.  ValueError for wrong shapes, RuntimeError without a GPU (no CPU fallback)."""
    if not isinstance(depths, bool):
        raise ValueError(f"project_boxes: depths must be a bool, got {depths!r}")
    (y0, x0, h, w), stride = check_window(window, stride)
    krows = _intrinsic_rows(intrinsic, "project_boxes")
    pts = _host_f32(corners, (8, 3), "project_boxes: corners")
    if (c2w is None) == (extrinsic is None):
        raise ValueError("project_boxes takes exactly one of c2w (camera-to-world) and extrinsic (world-to-camera)")
    if c2w is not None:
        w2c = np.linalg.inv(_host_matrices(c2w, "project_boxes: c2w").astype(np.float64)).astype(np.float32)
    else:
        w2c = _host_matrices(extrinsic, "project_boxes: extrinsic").astype(np.float32)
    if not isinstance(near, (int, float, np.floating, np.integer)) or isinstance(near, bool) or not near > 0:
        raise ValueError(f"project_boxes: near={near!r} must be a positive number of metres")
    k, n = w2c.shape[0], pts.shape[0]
    if k * n * 48 >= 2 ** 31:
        raise ValueError(f"project_boxes: {k} poses of {n} boxes hold 2^31 edge elements or more")
    dev = _gpu(device, c2w if c2w is not None else extrinsic)
    # one upload: 6 intrinsic floats, then the k matrices' three rows, then the corners
    buf = torch.from_numpy(np.concatenate([krows, w2c[:, :3, :].reshape(-1), pts.reshape(-1)])).to(dev)
    edges = torch.empty((k, n, 12, 4), dtype=torch.int32, device=dev)
    edge_mask = torch.empty((k, n), dtype=torch.int32, device=dev)
    rect = torch.empty((k, n, 4), dtype=torch.int32, device=dev)
    zrange = torch.empty((k, n, 2), dtype=torch.float32, device=dev)
    out = dict(edges=edges, edge_mask=edge_mask, rect=rect, zrange=zrange, window=(y0, x0, h, w), stride=stride)
    args = (_ptr(buf), _ptr(buf[6:]), _ptr(buf[6 + 12 * k:]), k, n, x0, y0, stride, h, w, float(near), _ptr(edges), _ptr(edge_mask), _ptr(rect),
            _ptr(zrange))
    if depths:
        out["edge_w"] = torch.empty((k, n, 12, 2), dtype=torch.float32, device=dev)
        check(_lib.load().ndet_project_boxes_w(*args, _ptr(out["edge_w"]), c_void_p(_lib.raw_stream(dev))), "project_boxes")
    else:
        check(_lib.load().ndet_project_boxes(*args, c_void_p(_lib.raw_stream(dev))), "project_boxes")
    return out


def draw_boxes(frames: torch.Tensor, projected: dict, colours, thickness: int = 1) -> torch.Tensor:
    """The wireframes of :func:`project_boxes`' boxes on frames that lie in device memory: one launch (ndet_draw_boxes) writes NEW frames,
    ``frames`` (k, h, w, 3) uint8 is only read.  ``projected``: project_boxes' dict for the same k and an h x w window; ``colours`` (n, 3)
    uint8, numpy or tensor (a device tensor is used as it is); ``thickness`` 1, 3 or 5 pixels across the line's major axis.  Where the edges
    of several boxes cover a pixel the HIGHEST box index wins, so hand the boxes over by ascending score (``boxes.drawing_order``).
    ValueError for wrong shapes or dtypes before any launch, RuntimeError for CPU tensors."""
    (k, h, w, n), edges, edge_mask, col = _check_drawing(frames, projected, colours, thickness, "draw_boxes")
    _need_gpu_drawing(frames, edges, edge_mask)
    dev = frames.device
    col = _device_colours(col, dev)
    out = torch.empty_like(frames)
    check(_lib.load().ndet_draw_boxes(_ptr(frames), _ptr(edges), _ptr(edge_mask), _ptr(col), k, h, w, n, int(thickness), _ptr(out),
                                      c_void_p(_lib.raw_stream(dev))), "draw_boxes")
    return out


def _check_drawing(frames, projected, colours, thickness, what: str):
    """The shape and dtype checks :func:`draw_boxes` and :func:`draw_overlay` share: ``((k, h, w, n), edges, edge_mask, colours)``, the
    colours a tensor or a numpy array as given; ValueError for anything else."""
    if thickness not in (1, 3, 5) or isinstance(thickness, bool):
        raise ValueError(f"{what}: thickness={thickness!r} must be 1, 3 or 5")
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3 or 0 in frames.shape \
            or not frames.is_contiguous():
        got = f"{tuple(frames.shape)} {frames.dtype}" if isinstance(frames, torch.Tensor) else type(frames).__name__
        raise ValueError(f"{what} takes frames as a contiguous (k, h, w, 3) uint8 tensor, got {got}")
    k, h, w = (int(v) for v in frames.shape[:3])
    if not isinstance(projected, dict):
        raise ValueError(f"{what} takes project_boxes' dict, got {type(projected).__name__}")
    edges, edge_mask = projected.get("edges"), projected.get("edge_mask")
    if (not isinstance(edges, torch.Tensor) or not isinstance(edge_mask, torch.Tensor) or edges.dtype != torch.int32 or edge_mask.dtype != torch.int32
            or edges.dim() != 4 or edges.shape[0] != k or edges.shape[1] < 1 or tuple(edges.shape[2:]) != (12, 4)
            or edge_mask.shape != edges.shape[:2] or not edges.is_contiguous() or not edge_mask.is_contiguous()):
        raise ValueError(f"{what} takes project_boxes' edges ({k}, n, 12, 4) and edge_mask ({k}, n) as contiguous int32 tensors")
    if "window" in projected and tuple(projected["window"][2:]) != (h, w):
        raise ValueError(f"{what}: the boxes were projected onto a {tuple(projected['window'][2:])} grid, the frames are {(h, w)}")
    n = int(edges.shape[1])
    col = colours if isinstance(colours, torch.Tensor) else np.asarray(colours)
    if tuple(col.shape) != (n, 3) or col.dtype != (torch.uint8 if isinstance(col, torch.Tensor) else np.uint8):
        raise ValueError(f"{what} takes colours as ({n}, 3) uint8, got {tuple(col.shape)} {col.dtype}")
    if k * h * w * 3 >= 2 ** 31:
        raise ValueError(f"{what}: {k} frames of {h} x {w} pixels hold 2^31 elements or more")
    return (k, h, w, n), edges, edge_mask, col


def _need_gpu_drawing(frames, *others) -> None:
    if not frames.is_cuda or any(t.device != frames.device for t in others):
        raise RuntimeError("nerfdet_amd.pipeline: frames and projected boxes must live on the GPU (no CPU fallback)")


def _device_colours(col, dev) -> torch.Tensor:
    return col.to(dev).contiguous() if isinstance(col, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(col)).to(dev)


def _glyphs(rows: str) -> list:
    return [int(v, 16) for v in rows.split()]


# 5 x 7 bitmaps of the codes 32..126 in the low five bits of a byte a row, bit 4 leftmost, top row first; index 95 (code 127, and every
# code the table does not hold) is a full block.  Drawn for this project; the one source of the glyphs: draw_overlay uploads it.
FONT_5X7 = np.array([_glyphs(g) for g in (
    "00 00 00 00 00 00 00", "04 04 04 04 04 00 04", "0A 0A 0A 00 00 00 00", "0A 0A 1F 0A 1F 0A 0A",     # space ! " #
    "04 0F 14 0E 05 1E 04", "18 19 02 04 08 13 03", "0C 12 14 08 15 12 0D", "0C 04 08 00 00 00 00",     # $ % & '
    "02 04 08 08 08 04 02", "08 04 02 02 02 04 08", "00 04 15 0E 15 04 00", "00 04 04 1F 04 04 00",     # ( ) * +
    "00 00 00 00 0C 04 08", "00 00 00 1F 00 00 00", "00 00 00 00 00 0C 0C", "00 01 02 04 08 10 00",     # , - . /
    "0E 11 13 15 19 11 0E", "04 0C 04 04 04 04 0E", "0E 11 01 02 04 08 1F", "1F 02 04 02 01 11 0E",     # 0 1 2 3
    "02 06 0A 12 1F 02 02", "1F 10 1E 01 01 11 0E", "06 08 10 1E 11 11 0E", "1F 01 02 04 08 08 08",     # 4 5 6 7
    "0E 11 11 0E 11 11 0E", "0E 11 11 0F 01 02 0C", "00 0C 0C 00 0C 0C 00", "00 0C 0C 00 0C 04 08",     # 8 9 : ;
    "02 04 08 10 08 04 02", "00 00 1F 00 1F 00 00", "08 04 02 01 02 04 08", "0E 11 01 02 04 00 04",     # < = > ?
    "0E 11 01 0D 15 15 0E", "0E 11 11 11 1F 11 11", "1E 11 11 1E 11 11 1E", "0E 11 10 10 10 11 0E",     # @ A B C
    "1C 12 11 11 11 12 1C", "1F 10 10 1E 10 10 1F", "1F 10 10 1E 10 10 10", "0E 11 10 17 11 11 0F",     # D E F G
    "11 11 11 1F 11 11 11", "0E 04 04 04 04 04 0E", "07 02 02 02 02 12 0C", "11 12 14 18 14 12 11",     # H I J K
    "10 10 10 10 10 10 1F", "11 1B 15 15 11 11 11", "11 11 19 15 13 11 11", "0E 11 11 11 11 11 0E",     # L M N O
    "1E 11 11 1E 10 10 10", "0E 11 11 11 15 12 0D", "1E 11 11 1E 14 12 11", "0F 10 10 0E 01 01 1E",     # P Q R S
    "1F 04 04 04 04 04 04", "11 11 11 11 11 11 0E", "11 11 11 11 11 0A 04", "11 11 11 15 15 15 0A",     # T U V W
    "11 11 0A 04 0A 11 11", "11 11 11 0A 04 04 04", "1F 01 02 04 08 10 1F", "0E 08 08 08 08 08 0E",     # X Y Z [
    "00 10 08 04 02 01 00", "0E 02 02 02 02 02 0E", "04 0A 11 00 00 00 00", "00 00 00 00 00 00 1F",     # \ ] ^ _
    "08 04 02 00 00 00 00", "00 00 0E 01 0F 11 0F", "10 10 16 19 11 11 1E", "00 00 0E 10 10 11 0E",     # ` a b c
    "01 01 0D 13 11 11 0F", "00 00 0E 11 1F 10 0E", "06 09 08 1C 08 08 08", "00 0F 11 11 0F 01 0E",     # d e f g
    "10 10 16 19 11 11 11", "04 00 0C 04 04 04 0E", "02 00 06 02 02 12 0C", "10 10 12 14 18 14 12",     # h i j k
    "0C 04 04 04 04 04 0E", "00 00 1A 15 15 11 11", "00 00 16 19 11 11 11", "00 00 0E 11 11 11 0E",     # l m n o
    "00 00 1E 11 1E 10 10", "00 00 0D 13 0F 01 01", "00 00 16 19 10 10 10", "00 00 0E 10 0E 01 1E",     # p q r s
    "08 08 1C 08 08 09 06", "00 00 11 11 11 13 0D", "00 00 11 11 11 0A 04", "00 00 11 11 15 15 0A",     # t u v w
    "00 00 11 0A 04 0A 11", "00 00 11 11 0F 01 0E", "00 00 1F 02 04 08 1F", "02 04 04 08 04 04 02",     # x y z {
    "04 04 04 04 04 04 04", "08 04 04 02 04 04 08", "00 00 08 15 02 00 00", "1F 1F 1F 1F 1F 1F 1F",     # | } ~ block
)], dtype=np.uint8)
TEXT_MAX = 32      # codes a plate holds


def encode_texts(strings) -> tuple:
    """``(codes (n, 32) uint8, lens (n,) int32)`` of n strings for :func:`draw_overlay`: a string is cut at 32 characters, a character
    outside 32..126 becomes code 127 (the block glyph); rows are padded with zeros."""
    if isinstance(strings, (str, bytes)) or not all(isinstance(s, str) for s in strings):
        raise ValueError("encode_texts takes a sequence of str")
    strings = list(strings)
    codes = np.zeros((len(strings), TEXT_MAX), dtype=np.uint8)
    lens = np.zeros(len(strings), dtype=np.int32)
    for i, s in enumerate(strings):
        s = s[:TEXT_MAX]
        lens[i] = len(s)
        codes[i, :len(s)] = [ord(c) if 32 <= ord(c) <= 126 else 127 for c in s]
    return codes, lens


OCCLUDED = {"hide": 0, "dim": 1}


def check_overlay_options(occluded, depth_bias, text_scale, what: str) -> tuple:
    """``(ndet_draw_overlay's occluded, bias_mm as np.float32, text_scale)`` of a call's options; ValueError for anything else."""
    if not isinstance(occluded, str) or occluded not in OCCLUDED:
        raise ValueError(f"{what}: occluded={occluded!r} must be 'hide' or 'dim'")
    if not isinstance(depth_bias, (int, float, np.floating, np.integer)) or isinstance(depth_bias, bool) or not 0 <= depth_bias < float("inf"):
        raise ValueError(f"{what}: depth_bias={depth_bias!r} must be a finite number of metres, not negative")
    with np.errstate(over="ignore"):
        bias_mm = np.float32(depth_bias * 1000.0)
    if not np.isfinite(bias_mm):
        raise ValueError(f"{what}: depth_bias={depth_bias!r} does not fit float32 millimetres")
    if isinstance(text_scale, bool) or text_scale not in (1, 2, 3):
        raise ValueError(f"{what}: text_scale={text_scale!r} must be 1, 2 or 3")
    return OCCLUDED[occluded], bias_mm, int(text_scale)


def draw_overlay(frames: torch.Tensor, projected: dict, colours, thickness: int = 1, depth_frames=None, occluded: str = "hide",
                 depth_bias: float = 0.05, texts=None, text_scale: int = 1) -> torch.Tensor:
    """:func:`draw_boxes` with a depth test of the edges and text plates: one launch (ndet_draw_overlay) writes NEW frames.  ``frames``,
    ``projected``, ``colours`` and ``thickness`` as in :func:`draw_boxes`; with ``depth_frames`` and ``texts`` both None the bytes are its.
    ``depth_frames`` (k, h, w) uint16 millimetres on the frames' device (0: a hole, which hides nothing) needs ``projected["edge_w"]``
    (``project_boxes(..., depths=True)``): a covered pixel of an edge is hidden where the depth frame lies more than ``depth_bias`` metres
    in front of the edge there (``bias_mm = np.float32(depth_bias * 1000.0)``); ``occluded="hide"`` leaves a pixel whose edges are all
    hidden as it was, ``"dim"`` blends a quarter of the colour in; a visible edge beats a hidden one of any index.  The edge's depth is
    interpolated from integer cells, so it is off by up to a pixel's worth: the default ``depth_bias`` of 0.05 m is a choice, not a
    measurement, made to cover that and sensor noise at indoor range.  ``texts``: n strings (:func:`encode_texts`: 32 characters at most);
    box b gets a filled plate in its colour above its ``projected["rect"]`` carrying its string in :data:`FONT_5X7` at ``text_scale``
    1, 2 or 3 -- ahead of every edge, the highest box index on top, never depth-tested; no plate for an empty string or a box outside the
    frame.  One upload for texts, lengths and font.  ValueError for wrong shapes or dtypes before any launch, RuntimeError for CPU tensors."""
    (k, h, w, n), edges, edge_mask, col = _check_drawing(frames, projected, colours, thickness, "draw_overlay")
    mode, bias_mm, text_scale = check_overlay_options(occluded, depth_bias, text_scale, "draw_overlay")
    device_side = [edges, edge_mask]
    edge_w = rect = None
    if depth_frames is not None:
        d, edge_w = depth_frames, projected.get("edge_w")
        if not isinstance(d, torch.Tensor) or d.dtype != torch.uint16 or tuple(d.shape) != (k, h, w) or not d.is_contiguous():
            got = f"{tuple(d.shape)} {d.dtype}" if isinstance(d, torch.Tensor) else type(d).__name__
            raise ValueError(f"draw_overlay takes depth_frames as a contiguous ({k}, {h}, {w}) uint16 tensor (millimetres), got {got}")
        if not isinstance(edge_w, torch.Tensor) or edge_w.dtype != torch.float32 or tuple(edge_w.shape) != (k, n, 12, 2) or not edge_w.is_contiguous():
            raise ValueError(f"draw_overlay: a depth test needs project_boxes(..., depths=True)'s edge_w ({k}, {n}, 12, 2) float32")
        device_side += [d, edge_w]
    if texts is not None:
        rect = projected.get("rect")
        if not isinstance(rect, torch.Tensor) or rect.dtype != torch.int32 or tuple(rect.shape) != (k, n, 4) or not rect.is_contiguous():
            raise ValueError(f"draw_overlay: text plates need project_boxes' rect ({k}, {n}, 4) int32")
        codes, lens = encode_texts(texts)
        if len(lens) != n:
            raise ValueError(f"draw_overlay: {len(lens)} texts for {n} boxes")
        device_side.append(rect)
    _need_gpu_drawing(frames, *device_side)
    dev = frames.device
    col = _device_colours(col, dev)
    text = text_len = font = None
    if texts is not None:
        # one upload: the n lengths (int32), then the n x 32 codes, then the font's 672 bytes
        buf = torch.from_numpy(np.concatenate([lens.view(np.uint8), codes.reshape(-1), FONT_5X7.reshape(-1)])).to(dev)
        text_len, text, font = buf, buf[4 * n:], buf[36 * n:]
    out = torch.empty_like(frames)
    check(_lib.load().ndet_draw_overlay(_ptr(frames), _ptr(edges), _ptr(edge_mask), _ptr(col), _ptr(depth_frames), _ptr(edge_w), float(bias_mm), mode,
                                        _ptr(rect), _ptr(text), _ptr(text_len), _ptr(font), text_scale, k, h, w, n, int(thickness), _ptr(out),
                                        c_void_p(_lib.raw_stream(dev))), "draw_overlay")
    return out


def label_frames(depth_frames: torch.Tensor, intrinsic, c2w, box_frames, window, stride: int = 1) -> torch.Tensor:
    """Which box each pixel of a depth frame belongs to: ``(k, h, w)`` int16 from one launch (ndet_label_frames) -- the highest index among
    the boxes that hold the pixel's point, -1 for none and for a hole (0 millimetres).  ``depth_frames`` (k, h, w) uint16 millimetres on the
    device, on the grid ``window = (y0, x0, h, w)``, ``stride`` of :func:`camera_rays` with its ``intrinsic`` and ``c2w`` (k camera-to-world
    4 x 4); ``box_frames`` (n, 8) float as ``boxes.box_frames`` makes them, n <= 32767.  The point of a pixel is the camera centre plus
    ``mm / 1000`` times :func:`camera_rays`' direction.  ValueError for wrong shapes or dtypes before any launch, RuntimeError for CPU tensors."""
    (y0, x0, h, w), stride = check_window(window, stride)
    krows = _intrinsic_rows(intrinsic, "label_frames")
    d = depth_frames
    if not isinstance(d, torch.Tensor) or d.dtype != torch.uint16 or d.dim() != 3 or d.shape[0] < 1 or tuple(d.shape[1:]) != (h, w) or not d.is_contiguous():
        got = f"{tuple(d.shape)} {d.dtype}" if isinstance(d, torch.Tensor) else type(d).__name__
        raise ValueError(f"label_frames takes depth_frames as a contiguous (k, {h}, {w}) uint16 tensor (millimetres), got {got}")
    k = int(d.shape[0])
    m = _host_matrices(c2w, "label_frames: c2w").astype(np.float32)
    if m.shape[0] != k:
        raise ValueError(f"label_frames: {m.shape[0]} poses for {k} depth frames")
    bf = _host_f32(box_frames, (8,), "label_frames: box_frames")
    n = bf.shape[0]
    if n > 32767:
        raise ValueError(f"label_frames: {n} boxes do not fit an int16 label")
    if k * h * w >= 2 ** 31:
        raise ValueError(f"label_frames: {k} frames of {h} x {w} pixels hold 2^31 elements or more")
    if not d.is_cuda:
        raise RuntimeError("nerfdet_amd.pipeline: depth frames must live on the GPU (no CPU fallback)")
    dev = d.device
    # one upload: 6 intrinsic floats, the k rotations, the k centres, the boxes
    buf = torch.from_numpy(np.concatenate([krows, m[:, :3, :3].reshape(-1), m[:, :3, 3].reshape(-1), bf.reshape(-1)])).to(dev)
    labels = torch.empty((k, h, w), dtype=torch.int16, device=dev)
    check(_lib.load().ndet_label_frames(_ptr(d), _ptr(buf), _ptr(buf[6:]), _ptr(buf[6 + 9 * k:]), _ptr(buf[6 + 12 * k:]), k, h, w, n, x0, y0, stride,
                                        _ptr(labels), c_void_p(_lib.raw_stream(dev))), "label_frames")
    return labels


def label_points(xyz: torch.Tensor, box_frames) -> torch.Tensor:
    """Which box each point belongs to: ``(M,)`` int16 from one launch (ndet_label_points) -- :func:`label_frames`' rule on points the
    caller has already (a scene's ``points()["xyz"]``): the highest index among the boxes that hold the point, -1 for none.  ``xyz`` (M, 3)
    float32 on the device; ``box_frames`` (n, 8) float as ``boxes.box_frames`` makes them, n <= 32767 -- no box at all, (0, 8), or no point
    launches nothing.  ValueError for wrong shapes or dtypes before any launch, RuntimeError for CPU tensors."""
    if not isinstance(xyz, torch.Tensor) or xyz.dtype != torch.float32 or xyz.dim() != 2 or xyz.shape[1] != 3 or not xyz.is_contiguous():
        got = f"{tuple(xyz.shape)} {xyz.dtype}" if isinstance(xyz, torch.Tensor) else type(xyz).__name__
        raise ValueError(f"label_points takes xyz as a contiguous (M, 3) float32 tensor, got {got}")
    bf = box_frames.detach().cpu().numpy() if isinstance(box_frames, torch.Tensor) else np.asarray(box_frames)
    if bf.ndim != 2 or bf.shape[1] != 8 or (bf.shape[0] and bf.dtype.kind != "f"):
        raise ValueError(f"label_points: box_frames must be a float array of shape (n, 8), got {bf.shape} {bf.dtype}")
    n, m = bf.shape[0], xyz.shape[0]
    if n > 32767:
        raise ValueError(f"label_points: {n} boxes do not fit an int16 label")
    if m >= 2 ** 31:
        raise ValueError(f"label_points: {m} points, 2^31 or more")
    if not xyz.is_cuda:
        raise RuntimeError("nerfdet_amd.pipeline: points must live on the GPU (no CPU fallback)")
    dev = xyz.device
    if n == 0 or m == 0:
        return torch.full((m,), -1, dtype=torch.int16, device=dev)
    buf = torch.from_numpy(np.ascontiguousarray(bf, dtype=np.float32).reshape(-1)).to(dev)
    labels = torch.empty((m,), dtype=torch.int16, device=dev)
    check(_lib.load().ndet_label_points(_ptr(xyz), m, _ptr(buf), n, _ptr(labels), c_void_p(_lib.raw_stream(dev))), "label_points")
    return labels


def write_ply(path, xyz, bgr, labels=None) -> None:
    """A point cloud as a binary little-endian PLY file, on the host: per vertex ``x y z`` float32 and ``red green blue`` uchar -- ``bgr``'s
    columns swapped -- and with ``labels`` a ``label`` short.  ``xyz`` (M, 3) float, ``bgr`` (M, 3) uint8, ``labels`` None or (M,) int16;
    tensors (of any device) or arrays.  ValueError for wrong shapes or dtypes, before the file is opened."""
    host = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    xyz, bgr = host(xyz), host(bgr)
    if xyz.ndim != 2 or xyz.shape[1] != 3 or xyz.dtype.kind != "f":
        raise ValueError(f"write_ply: xyz must be a float array of shape (M, 3), got {xyz.shape} {xyz.dtype}")
    m = xyz.shape[0]
    if bgr.shape != (m, 3) or bgr.dtype != np.uint8:
        raise ValueError(f"write_ply: bgr must be a uint8 array of shape ({m}, 3), got {bgr.shape} {bgr.dtype}")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")]
    if labels is not None:
        labels = host(labels)
        if labels.shape != (m,) or labels.dtype != np.int16:
            raise ValueError(f"write_ply: labels must be an int16 array of shape ({m},), got {labels.shape} {labels.dtype}")
        fields.append(("label", "<i2"))
    rows = np.empty((m,), dtype=np.dtype(fields))
    for j, name in enumerate("xyz"):
        rows[name] = xyz[:, j]
    for j, name in enumerate(("blue", "green", "red")):
        rows[name] = bgr[:, j]
    if labels is not None:
        rows["label"] = labels
    names = {"<f4": "float", "u1": "uchar", "<i2": "short"}
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {m}"] + [f"property {names[t]} {f}" for f, t in fields] + ["end_header"]
    with open(path, "wb") as out:
        out.write(("\n".join(header) + "\n").encode("ascii"))
        out.write(rows.tobytes())


def depth_to_mm(depth: torch.Tensor) -> torch.Tensor:
    """Metres -> uint16 millimetres by :func:`pack_frames`' own rule, with torch: in float32 ``d = depth * 1000``; NaN and d < 0 give 0,
    d > 65535 gives 65535, else trunc(d + 0.5).  For the held-out depth maps of ``score_frames``."""
    d = depth.to(torch.float32) * 1000.0
    q = torch.where(d > 65535.0, torch.full_like(d, 65535.0), d + 0.5)
    q = torch.where(d >= 0.0, q, torch.zeros_like(d))          # NaN compares false
    return q.to(torch.int32).to(torch.uint16)


def frame_meta(cams_or_lidar2img: dict, size_hw, img_scale, pad_size) -> dict:
    """The ``img_meta`` of capture-size frames as the ``datasets`` chain leaves it: ``lidar2img{intrinsic, extrinsic[], origin}`` of the
    cameras (``scene_cameras``'s dict or a ``lidar2img``), ``ori_shape = (Hs, Ws, 3)``, ``img_shape = (Hr, Wr, 3)`` -- what
    ``ops.compute_projection`` divides by -- and ``pad_shape = (H, W, 3)``."""
    (hr, wr), (h, w) = _frame_sizes(size_hw, img_scale, pad_size)
    c = cams_or_lidar2img
    return dict(lidar2img=dict(intrinsic=c["intrinsic"], extrinsic=list(c["extrinsic"]), origin=c["origin"]),
                ori_shape=(int(size_hw[0]), int(size_hw[1]), 3), img_shape=(hr, wr, 3), pad_shape=(h, w, 3))


class MultiViewPipeline:
    """``MultiViewPipeline`` + ``DefaultFormatBundle3D`` + batch-1 collate for frames resident on the GPU.

    ``__call__(frames, cams, ori_shape)`` -> the keyword arguments of ``nerfdet.forward_train / forward_test``:
    ``img (1,n_v,3,H,W)``, ``denorm_images (1,n_v,3,H,W)``, ``raydirs / lightpos / gt_images (1,T,R,3)``, ``nerf_sizes``,
    ``depth_range`` and ``img_metas`` with ``lidar2img{intrinsic, extrinsic[], origin}``, ``ori_shape``, ``img_shape``.

    ``img_scale=(w, h)`` and ``pad_size=(H, W)``, both given: ``frames`` are at capture resolution (n, Hs, Ws, 3) and the batch is what
    the ``datasets`` chain ``Resize(img_scale, keep_ratio=True) -> Normalize -> Pad(size=pad_size)`` + ``MultiViewPipeline`` produces:
    ``img`` / ``denorm_images`` from one ndet_resize_normalize_views launch over the selected and the target views, ``img_metas`` as
    :func:`frame_meta` gives (``ori_shape`` is the frames' own; the argument must be None or equal to it), target intrinsics scaled by
    ``Hs / Hr``, the ray grid over the padded H x W (multi_view.py takes ``imgs[0].shape``) and ``gt_images`` the margin crop of the
    target views' de-normalised planes, so a pad pixel is ``trunc(mean) / 255``.  Both None: frames at network resolution, as above.

    ``frame_format="nv12"`` (raw mode only): ``frames`` are a video decoder's NV12 surfaces (n, rows, pitch) uint8, ``ori_shape=(Hs, Ws[, 3])``
    says the size of their Y plane and ``uv_row=`` where the U,V plane starts (None: Hs; :func:`surface_layout`).  The one launch is
    ndet_resize_normalize_views_nv12 and the batch is the BGR raw mode's on ``datasets.nv12_to_bgr`` of the surfaces bit for bit; everything
    after the resize is the same code.

    ``depth_frames=`` (n_frames, Hd, Wd) uint16 millimetres on the device, one per colour frame, of any size of their own: the batch gains
    what the ``*_depth_sp`` configs' loader adds (multi_view.py:98-105, 156-166; formating.py) -- ``depth`` (1, n_v, Hr, Wr) float64 metres,
    the selected views' maps at the meta's ``img_shape``, for ``simple_test(depth=)``; and with target views ``gt_depths``
    (1, T, H - 2m, W - 2m) float64, the margin crop of the targets' maps at the PADDED size (the reference resizes them to ``gt_rgb_shape``:
    240 x 320 where the image content is 239 x 320), and ``depth_rays`` (1, K) int64, ``flatnonzero(gt_depths > 0)`` -- each
    ``datasets.imresize_linear(frame / 1000, ...)`` bit for bit (:func:`prepare_depth_frames`).  Three launches and one 8-byte read (the
    count K) on top of the call's own; without ``depth_frames`` nothing changes and ``gt_depths`` stays ``[]``."""

    def __init__(self, n_images: int, mean: Sequence[float] = IMG_MEAN, std: Sequence[float] = IMG_STD, margin: int = 10,
                 depth_range=(0.5, 5.5), loading: str = "random", nerf_target_views: int = 0, sample_freq: int = 3, img_scale=None,
                 pad_size=None, frame_format: str = "bgr"):
        self.n_images, self.margin, self.depth_range = n_images, margin, list(depth_range)
        self.frame_format = _check_format(frame_format, "MultiViewPipeline")
        if frame_format == "nv12" and img_scale is None:
            raise ValueError("MultiViewPipeline: frame_format='nv12' takes surfaces at capture resolution: give img_scale and pad_size")
        self.loading, self.nerf_target_views, self.sample_freq = loading, nerf_target_views, sample_freq
        self.mean = np.asarray(mean, dtype=np.float64)
        self.std = np.asarray(std, dtype=np.float64)
        if (img_scale is None) != (pad_size is None):
            raise ValueError("MultiViewPipeline: img_scale and pad_size go together (raw frames) or are both None")
        self.img_scale = None if img_scale is None else tuple(img_scale)
        self.pad_size = None if pad_size is None else tuple(pad_size)

    def _depth(self, depth_frames: torch.Tensor, ids, target_ids, view_hw, pad_hw) -> dict:
        """The depth keys of a batch: the selected views at ``view_hw``, the targets' margin crop at ``pad_hw`` and its positive rays."""
        out = dict(depth=prepare_depth_frames(depth_frames, view_hw, ids=ids).unsqueeze(0))
        if target_ids:
            gt = prepare_depth_frames(depth_frames, pad_hw, ids=target_ids, margin=self.margin)
            out.update(gt_depths=gt.unsqueeze(0), depth_rays=positive_indices(gt).reshape(1, -1))
        return out

    def _raw(self, frames: torch.Tensor, cams: dict, ori_shape, ids, target_ids, depth_frames=None, uv_row=None) -> dict:
        """``__call__`` for frames at capture resolution."""
        if self.frame_format == "nv12":
            (hs, ws), surf = (int(ori_shape[0]), int(ori_shape[1])), dict(format="nv12", size=ori_shape[:2], uv_row=uv_row)
        else:
            n_frames, hs, ws, _ = frames.shape
            surf = {}
            if ori_shape is not None and tuple(ori_shape)[:2] != (hs, ws):
                raise ValueError(f"MultiViewPipeline: ori_shape {tuple(ori_shape)} differs from the raw frames' {(hs, ws, 3)}")
        (hr, wr), (h, w) = _frame_sizes((hs, ws), self.img_scale, self.pad_size)
        dev = frames.device
        n, m = len(ids), self.margin
        # one launch over the selected and the target views; only the targets' rays need the resized bytes
        out = prepare_frames(frames, self.img_scale, self.pad_size, self.mean, self.std, ids=list(ids) + target_ids, want_u8=bool(target_ids), **surf)
        img, denorm = out[0], out[1]
        meta = frame_meta(dict(cams, extrinsic=[cams["extrinsic"][i] for i in ids]), (hs, ws), self.img_scale, self.pad_size)
        batch = dict(img=img[:n].unsqueeze(0), img_metas=[meta])
        if target_ids:
            t, u8 = len(target_ids), out[2]
            if not (m >= 0 and 2 * m < h and 2 * m < w):
                raise ValueError(f"MultiViewPipeline: margin {m} leaves no ray in a {h} x {w} image")
            k = cams["intrinsic"].copy()
            k[:2] = k[:2] / (hs / hr)                                 # multi_view.py:113-114 with ratio = ori_shape[0] / img_shape[0]
            krows = torch.from_numpy(np.ascontiguousarray(k[:2, :3])).to(dev)
            rot = torch.from_numpy(np.stack([cams["camrotc2w"][i] for i in target_ids])).to(dev).contiguous()
            lpos = torch.from_numpy(np.stack([cams["lightpos"][i] for i in target_ids])).to(dev).contiguous()
            t_d = torch.arange(t, dtype=torch.int32, device=dev)     # the targets are rows n .. n+t-1 of the launch above
            raydirs = torch.empty((t, (h - 2 * m) * (w - 2 * m), 3), dtype=torch.float32, device=dev)
            lightpos, unused = torch.empty_like(raydirs), torch.empty_like(raydirs)
            mp, sp = self.mean.ctypes.data_as(c_void_p), self.std.ctypes.data_as(c_void_p)
            check(_lib.load().ndet_target_rays(_ptr(u8[n:]), _ptr(t_d), t, h, w, m, _ptr(krows), _ptr(rot), _ptr(lpos), mp, sp, _ptr(raydirs),
                                               _ptr(lightpos), _ptr(unused), c_void_p(_lib.raw_stream(dev))), "target_rays")
            # its colours would be the round trip of the pad's zero BYTE; the chain pads after Normalize: take them from denorm
            gt = denorm[n:, :, m:h - m, m:w - m].permute(0, 2, 3, 1).reshape(t, -1, 3)
            size = torch.tensor([[h - 2 * m, w - 2 * m, 3]])
            batch.update(denorm_images=denorm[:n].unsqueeze(0), raydirs=raydirs.unsqueeze(0), lightpos=lightpos.unsqueeze(0),
                         gt_images=gt.unsqueeze(0), gt_depths=[], nerf_sizes=[size.clone() for _ in target_ids],
                         depth_range=torch.tensor([[self.depth_range]], dtype=torch.float32, device=dev),
                         c2w=[cams["c2w"][i] for i in target_ids])
        if depth_frames is not None:
            batch.update(self._depth(depth_frames, ids, target_ids, (hr, wr), (h, w)))
        return batch

    def __call__(self, frames: torch.Tensor, cams: dict, ori_shape=None, ids=None, target_ids=None, depth_frames=None, uv_row=None) -> dict:
        if self.frame_format == "nv12":
            if ori_shape is None:
                raise ValueError("MultiViewPipeline: NV12 surfaces need ori_shape=(Hs, Ws[, 3]), the size of their Y plane")
            n_frames = _check_surfaces(frames, ori_shape, uv_row, "MultiViewPipeline")[0]
        elif uv_row is not None:
            raise ValueError("MultiViewPipeline: uv_row= describes NV12 surfaces (frame_format='nv12')")
        if not frames.is_cuda:
            raise RuntimeError("nerfdet_amd.pipeline: frames must live on the GPU (no CPU fallback)")
        if self.frame_format == "nv12":
            h = w = None
        else:
            assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[-1] == 3 and frames.is_contiguous()
            n_frames, h, w, _ = frames.shape
        if depth_frames is not None:
            _check_depth_frames(depth_frames, "MultiViewPipeline", n_frames)
        if ids is None:
            ids, target_ids = select_views(n_frames, self.n_images, self.nerf_target_views, self.loading, self.sample_freq)
        target_ids = list(target_ids or [])
        if self.img_scale is not None:
            return self._raw(frames, cams, ori_shape, ids, target_ids, depth_frames, uv_row)
        dev = frames.device
        lib = _lib.load()
        st = c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        mean, std = self.mean, self.std
        mp, sp = mean.ctypes.data_as(c_void_p), std.ctypes.data_as(c_void_p)
        ids_d = torch.tensor(ids, dtype=torch.int32, device=dev)
        img = torch.empty((len(ids), 3, h, w), dtype=torch.float32, device=dev)
        denorm = torch.empty_like(img)
        check(lib.ndet_normalize_views(_ptr(frames), _ptr(ids_d), len(ids), h, w, mp, sp, _ptr(img), _ptr(denorm), st), "normalize_views")
        meta = dict(lidar2img=dict(intrinsic=cams["intrinsic"], extrinsic=[cams["extrinsic"][i] for i in ids], origin=cams["origin"]),
                    ori_shape=tuple(ori_shape), img_shape=(h, w, 3), pad_shape=(h, w, 3))
        batch = dict(img=img.unsqueeze(0), img_metas=[meta])
        if target_ids:
            ratio = ori_shape[0] / h
            k = cams["intrinsic"].copy()
            k[:2] = k[:2] / ratio                                     # multi_view.py:113-114
            krows = torch.from_numpy(np.ascontiguousarray(k[:2, :3])).to(dev)
            rot = torch.from_numpy(np.stack(cams["camrotc2w"])).to(dev).contiguous()
            lpos = torch.from_numpy(np.stack(cams["lightpos"])).to(dev).contiguous()
            t_d = torch.tensor(target_ids, dtype=torch.int32, device=dev)
            rays_per = (h - 2 * self.margin) * (w - 2 * self.margin)
            raydirs = torch.empty((len(target_ids), rays_per, 3), dtype=torch.float32, device=dev)
            lightpos, gt = torch.empty_like(raydirs), torch.empty_like(raydirs)
            check(lib.ndet_target_rays(_ptr(frames), _ptr(t_d), len(target_ids), h, w, self.margin, _ptr(krows), _ptr(rot), _ptr(lpos), mp, sp,
                                       _ptr(raydirs), _ptr(lightpos), _ptr(gt), st), "target_rays")
            size = torch.tensor([[h - 2 * self.margin, w - 2 * self.margin, 3]])
            batch.update(denorm_images=denorm.unsqueeze(0), raydirs=raydirs.unsqueeze(0), lightpos=lightpos.unsqueeze(0),
                         gt_images=gt.unsqueeze(0), gt_depths=[], nerf_sizes=[size.clone() for _ in target_ids],
                         depth_range=torch.tensor([[self.depth_range]], dtype=torch.float32, device=dev),
                         c2w=[cams["c2w"][i] for i in target_ids])
        if depth_frames is not None:
            batch.update(self._depth(depth_frames, ids, target_ids, (h, w), (h, w)))
        return batch
