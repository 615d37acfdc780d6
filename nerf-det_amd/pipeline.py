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

The sensor's depth frames (uint16 millimetres on the device) go the same way: :func:`prepare_depth_frames` is the loader's
``imresize_linear(frame / 1000, ...)`` in float64 (ndet_depth_frames), :func:`positive_indices` its ``flatnonzero(gt_depths > 0)``
(ndet_positive_indices), and ``MultiViewPipeline(...)(..., depth_frames=)`` adds ``depth``, ``gt_depths`` and ``depth_rays`` to the batch.
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


def prepare_frames(frames: torch.Tensor, img_scale, pad_size, mean: Sequence[float] = IMG_MEAN, std: Sequence[float] = IMG_STD, ids=None,
                   want_u8: bool = False):
    """The configs' ``Resize(img_scale, keep_ratio=True) -> Normalize(mean, std, to_rgb=True) -> Pad(size=pad_size)`` and the reference's
    de-normalised copy for frames at capture resolution, in one launch: ``frames`` (n, Hs, Ws, 3) uint8 BGR on the device ->
    ``(img, denorm)``, both (n_sel, 3, H, W) float32 (``ids``: a sequence of frame indices, None for every frame in order), and with
    ``want_u8`` also the resized, zero-padded bytes (n_sel, H, W, 3).  The content region holds ``datasets.imresize_linear``'s bytes
    normalised as ``ndet_normalize_views`` does; the pad is 0 in ``img`` and ``trunc(mean) / 255`` in ``denorm``.  ValueError when the
    rescaled frame does not fit ``pad_size`` (a portrait frame into a landscape pad)."""
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3 or not frames.is_contiguous():
        raise ValueError(f"prepare_frames takes contiguous (n, Hs, Ws, 3) uint8 frames, got {tuple(frames.shape)} {frames.dtype}")
    n, hs, ws, _ = frames.shape
    (hr, wr), (h, w) = _frame_sizes((hs, ws), img_scale, pad_size)
    if not frames.is_cuda:
        raise RuntimeError("nerfdet_amd.pipeline: frames must live on the GPU (no CPU fallback)")
    dev = frames.device
    ids_d = None
    if ids is not None:
        ids = [int(i) for i in ids]
        if not ids or min(ids) < 0 or max(ids) >= n:
            raise ValueError(f"prepare_frames: ids must be a non-empty list of frame indices below {n}")
        ids_d = torch.tensor(ids, dtype=torch.int32, device=dev)
    n_sel = n if ids is None else len(ids)
    mean, std = np.asarray(mean, dtype=np.float64), np.asarray(std, dtype=np.float64)
    img = torch.empty((n_sel, 3, h, w), dtype=torch.float32, device=dev)
    denorm = torch.empty_like(img)
    u8 = torch.empty((n_sel, h, w, 3), dtype=torch.uint8, device=dev) if want_u8 else None
    check(_lib.load().ndet_resize_normalize_views(_ptr(frames), _ptr(ids_d), n_sel, hs, ws, hr, wr, h, w, mean.ctypes.data_as(c_void_p),
                                                  std.ctypes.data_as(c_void_p), _ptr(img), _ptr(denorm), _ptr(u8),
                                                  c_void_p(_lib.raw_stream(dev))), "resize_normalize_views")
    return (img, denorm, u8) if want_u8 else (img, denorm)


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

    ``depth_frames=`` (n_frames, Hd, Wd) uint16 millimetres on the device, one per colour frame, of any size of their own: the batch gains
    what the ``*_depth_sp`` configs' loader adds (multi_view.py:98-105, 156-166; formating.py) -- ``depth`` (1, n_v, Hr, Wr) float64 metres,
    the selected views' maps at the meta's ``img_shape``, for ``simple_test(depth=)``; and with target views ``gt_depths``
    (1, T, H - 2m, W - 2m) float64, the margin crop of the targets' maps at the PADDED size (the reference resizes them to ``gt_rgb_shape``:
    240 x 320 where the image content is 239 x 320), and ``depth_rays`` (1, K) int64, ``flatnonzero(gt_depths > 0)`` -- each
    ``datasets.imresize_linear(frame / 1000, ...)`` bit for bit (:func:`prepare_depth_frames`).  Three launches and one 8-byte read (the
    count K) on top of the call's own; without ``depth_frames`` nothing changes and ``gt_depths`` stays ``[]``."""

    def __init__(self, n_images: int, mean: Sequence[float] = IMG_MEAN, std: Sequence[float] = IMG_STD, margin: int = 10,
                 depth_range=(0.5, 5.5), loading: str = "random", nerf_target_views: int = 0, sample_freq: int = 3, img_scale=None,
                 pad_size=None):
        self.n_images, self.margin, self.depth_range = n_images, margin, list(depth_range)
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

    def _raw(self, frames: torch.Tensor, cams: dict, ori_shape, ids, target_ids, depth_frames=None) -> dict:
        """``__call__`` for frames at capture resolution."""
        n_frames, hs, ws, _ = frames.shape
        if ori_shape is not None and tuple(ori_shape)[:2] != (hs, ws):
            raise ValueError(f"MultiViewPipeline: ori_shape {tuple(ori_shape)} differs from the raw frames' {(hs, ws, 3)}")
        (hr, wr), (h, w) = _frame_sizes((hs, ws), self.img_scale, self.pad_size)
        dev = frames.device
        n, m = len(ids), self.margin
        # one launch over the selected and the target views; only the targets' rays need the resized bytes
        out = prepare_frames(frames, self.img_scale, self.pad_size, self.mean, self.std, ids=list(ids) + target_ids, want_u8=bool(target_ids))
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

    def __call__(self, frames: torch.Tensor, cams: dict, ori_shape=None, ids=None, target_ids=None, depth_frames=None) -> dict:
        if not frames.is_cuda:
            raise RuntimeError("nerfdet_amd.pipeline: frames must live on the GPU (no CPU fallback)")
        assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[-1] == 3 and frames.is_contiguous()
        n_frames, h, w, _ = frames.shape
        if depth_frames is not None:
            _check_depth_frames(depth_frames, "MultiViewPipeline", n_frames)
        if ids is None:
            ids, target_ids = select_views(n_frames, self.n_images, self.nerf_target_views, self.loading, self.sample_freq)
        target_ids = list(target_ids or [])
        if self.img_scale is not None:
            return self._raw(frames, cams, ori_shape, ids, target_ids, depth_frames)
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
