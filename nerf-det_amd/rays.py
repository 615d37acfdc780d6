"""Host mirror of the NeRF ray branch (A7-A12): ``Projector`` (mmdet3d/models/model_utils/projection.py:20-151),
``compute_mask_points`` / ``sample_along_camera_ray`` / ``raw2outputs`` / ``render_rays_func`` / ``render_rays``
(model_utils/render_ray.py:48-93,145-327,371-520), same signatures, bodies on the HIP kernels of
csrc/ray_kernels.hip.  The fused path (:func:`ray_view_stats`) never builds the (R,S,n_views,35) tensor.  Hierarchical sampling
(``sample_pdf``, render_ray.py:96-142, and the fine pass of ``render_rays_func``) runs on csrc/importance_kernels.hip."""
from __future__ import annotations

import ctypes
from collections import OrderedDict
from ctypes import c_void_p
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _lib, ops, trace
from ._lib import _ptr, check
from .hostmath import matmul_mul_add

Tensor = torch.Tensor
rng = np.random.RandomState(234)  # render_ray.py:20 -- module-global stream used for ray selection


def _stream(t):
    return c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


# ------------------------------------------------------------------------------------------------------
# A1 (ray-branch twin)
# ------------------------------------------------------------------------------------------------------
def _compute_projection(img_meta: dict) -> Tensor:
    """(1,n_views,34) rows ``[h, w | K(4x4) | E(4x4)]``, intrinsics rows 0-1 / (ori_h/img_h).  render_ray.py:48-69."""
    ext = img_meta["lidar2img"]["extrinsic"]
    n = len(ext)
    k = torch.tensor(np.asarray(img_meta["lidar2img"]["intrinsic"], dtype=np.float32)[:4, :4])
    k[:2] /= img_meta["ori_shape"][0] / img_meta["img_shape"][0]
    size = torch.tensor([float(img_meta["img_shape"][0]), float(img_meta["img_shape"][1])])
    e = torch.from_numpy(np.stack([np.asarray(x, dtype=np.float32) for x in ext])).reshape(n, 16)
    return torch.cat([size.expand(n, 2), k.reshape(1, 16).expand(n, 16), e], dim=-1).unsqueeze(0)


def _camera_matrices(train_cameras: Tensor) -> Tuple[Tensor, float, float]:
    """cameras (n_views,34) -> KE (n_views,3,4) = rows 0..2 of K @ E (projection.py:52-58), h, w."""
    cams = train_cameras.detach().to("cpu", torch.float32)
    k = cams[:, 2:18].reshape(-1, 4, 4)
    e = cams[:, -16:].reshape(-1, 4, 4)
    ke = torch.from_numpy(matmul_mul_add(k.numpy(), e.numpy())[:, :3, :].copy())     # = k.bmm(e), in a host-independent op order
    return ke, float(cams[0, 0]), float(cams[0, 1])


def _to_device(host: Tensor, device) -> Tensor:
    """Small per-scene constants go up through the pinned staging ring of nerfdet_amd.ops: a pageable copy waits for everything queued."""
    if torch.device(device).type != "cuda" or host.is_cuda:
        return host.to(device)
    from .ops import _upload_async
    return _upload_async(host, device)


def _prep_sources(train_imgs: Tensor, featmaps: Tensor):
    """train_imgs (1,n_v,H,W,3) as the reference passes it (a permuted view of the (n_v,3,H,W) images) or the
    (n_v,3,H,W) tensor itself; featmaps logical (n_v,d,h,w)."""
    if train_imgs.dim() == 5:
        assert train_imgs.shape[0] == 1, "only support batch_size=1 for now"  # projection.py:100-101
        rgb = train_imgs.squeeze(0).permute(0, 3, 1, 2)
    else:
        rgb = train_imgs
    if rgb.dtype != torch.float32:
        rgb = rgb.float()
    if rgb.stride(3) != 1:
        rgb = rgb.contiguous()
    f = ops.to_channels_last(featmaps)
    return rgb, f


_PACKED_RGB = {}  # one entry: the (n_v,H,W,4) copy of the scene's source images, reused by every chunk / backward of that scene


def packed_rgb(rgb: Tensor) -> Tensor:
    """(n_v,3,H,W) -> dense (n_v,H,W,4) fp32, 4th component 0 (one image pixel = one 16-byte load in the packed sampler).  Cached
    for the tensor it was made from (``render_testing`` walks one scene in hundreds of chunks)."""
    key = (rgb.data_ptr(), rgb._version, tuple(rgb.shape), tuple(rgb.stride()), str(rgb.device))
    hit = _PACKED_RGB.get("last")
    if hit is not None and hit[0] == key:
        return hit[1]
    n_v, _, h, w = rgb.shape
    out = torch.empty((n_v, h, w, 4), dtype=torch.float32, device=rgb.device)
    check(_lib.load().ndet_pack_rgb_nhwc4(_ptr(rgb), n_v, h, w, rgb.stride(0), rgb.stride(1), rgb.stride(2), _ptr(out), _stream(rgb)),
          "pack_rgb_nhwc4")
    _PACKED_RGB["last"] = (key, out, rgb)   # keeps the source alive so that its data_ptr stays unique
    return out


def packed_ok(n_views: int, d: int, backward: bool = False) -> bool:
    """Shapes the packed sampler (csrc/ray_stats_kernels.hip) takes; everything else runs on the generic kernel."""
    if d % 4 or d > 128 or n_views > 128:
        return False
    lanes = d // 4 + (0 if backward else 1)
    g, nvp = 64 // lanes, (n_views + 63) // 64 * 64
    if backward:
        return d <= 64 and 4 * g * nvp * 8 + 4 * g * d * 16 + 4 * g * 32 <= 64 * 1024
    return 4 * g * nvp * 8 <= 64 * 1024


def _stats_buffers(n: int, d: int, device):
    """The samplers' outputs for n sample points: ``globalfeat`` (n, 2*(3+d)), ``pixel_mask`` (n,) bool, ``view_count`` (n,) int32."""
    return (torch.empty((n, 2 * (3 + d)), dtype=torch.float32, device=device), torch.empty((n,), dtype=torch.bool, device=device),
            torch.empty((n,), dtype=torch.int32, device=device))


def ray_view_stats(xyz: Tensor, train_imgs: Tensor, train_cameras: Tensor, featmaps: Tensor):
    """Fused A7+A8: sample points (R,S,3) -> ``globalfeat`` (R,S,2*(3+d)), ``pixel_mask`` (R,S) bool,
    ``view_count`` (R,S) int32.  Equals Projector.compute + compute_mask_points + cat + ``mask.sum(2) > 1``
    (render_ray.py:299-303)."""
    if not xyz.is_cuda:
        raise RuntimeError("nerfdet_amd.rays: tensors must live on the GPU (no CPU fallback)")
    cams = train_cameras.squeeze(0) if train_cameras.dim() == 3 else train_cameras
    ke, h, w = _camera_matrices(cams)
    ke = _to_device(ke, xyz.device)
    rgb, f = _prep_sources(train_imgs, featmaps)
    n_v, d, hf, wf = f.shape
    assert rgb.shape[0] == n_v and ke.shape[0] == n_v
    shape = xyz.shape[:-1]
    pts = xyz.to(torch.float32).reshape(-1, 3).contiguous()
    n = pts.shape[0]
    glob, pm, vc = _stats_buffers(n, d, xyz.device)
    nbytes = 4 * (n_v * 3 * rgb.shape[2] * rgb.shape[3] + n_v * d * hf * wf + 2 * (3 + d) * n)
    if packed_ok(n_v, d) and f.stride(0) % 4 == 0 and f.stride(2) % 4 == 0 and f.data_ptr() % 16 == 0:
        rgb4 = packed_rgb(rgb)
        trace.span("k_ray_stats_packed", lambda: check(
            _lib.load().ndet_ray_view_stats_packed(_ptr(pts), n, _ptr(ke), n_v, h, w, _ptr(rgb4), rgb.shape[2], rgb.shape[3], _ptr(f), d, hf, wf,
                                                   f.stride(0), f.stride(2), _ptr(glob), _ptr(pm), _ptr(vc), _stream(xyz)),
            "ray_view_stats_packed"), bytes=nbytes, kind="hbm")
        return glob.view(*shape, -1), pm.view(*shape), vc.view(*shape)
    trace.span("k_ray_view_stats", lambda: check(
        _lib.load().ndet_ray_view_stats(_ptr(pts), n, _ptr(ke), n_v, h, w, _ptr(rgb), rgb.shape[2], rgb.shape[3], rgb.stride(0), rgb.stride(1),
                                        rgb.stride(2), _ptr(f), d, hf, wf, f.stride(0), f.stride(2), _ptr(glob), _ptr(pm), _ptr(vc),
                                        _stream(xyz)), "ray_view_stats"),
        bytes=nbytes, kind="hbm")
    return glob.view(*shape, -1), pm.view(*shape), vc.view(*shape)


class BankSegment:
    """One chunk of a :class:`ViewBank`: ``feat`` (k,hf,wf,d) dense mapped maps, ``rgb4`` (k,H,W,4) packed images (device), ``ke`` (k,3,4)
    rows 0..2 of K @ E (host), ``img_hw`` the cameras' image size (render_ray.py:48-69: cameras[:, :2])."""
    __slots__ = ("feat", "rgb4", "ke", "img_hw")

    def __init__(self, feat: Tensor, rgb4: Tensor, ke: Tensor, img_hw: Tuple[float, float]):
        self.feat, self.rgb4, self.ke, self.img_hw = feat, rgb4, ke, img_hw

    @property
    def n_views(self) -> int:
        return self.feat.shape[0]


class ViewBank:
    """What the ray branch needs of a streamed scene's source views, kept chunk by chunk: ``segments``, oldest first, each with its own
    allocations (mapped map + packed image + 12 camera floats per view).  :func:`ray_view_stats_bank` samples all of them through a device
    table of per-view pointers (``NdetBankView``), built when first needed, uploaded through the pinned staging ring and kept until the
    segment list changes.  The bank owns every tensor the table points to.

    Renders and evictions must be issued on ONE stream: a dropped segment's memory goes back to the caching allocator, whose stream
    order then keeps a later allocation on that stream behind the renders already queued; a render queued on another stream would
    have no such protection."""

    def __init__(self):
        self.segments: List[BankSegment] = []
        self._table = None                                     # (device table, n_views) of the current segment list

    @property
    def n_views(self) -> int:
        return sum(s.n_views for s in self.segments)

    def nbytes(self) -> int:
        """Device bytes held: maps, images and the 64-byte table rows."""
        return sum(4 * (s.feat.numel() + s.rgb4.numel()) + 64 * s.n_views for s in self.segments)

    def append(self, mapped: Tensor, images: Tensor, img_meta: dict) -> None:
        """Bank a chunk (:meth:`make_segment`, then :meth:`push`)."""
        self.push(self.make_segment(mapped, images, img_meta))

    def push(self, seg: BankSegment) -> None:
        """A segment made by :meth:`make_segment` for this bank becomes its newest."""
        self.segments.append(seg)
        self._table = None

    def make_segment(self, mapped: Tensor, images: Tensor, img_meta: dict) -> BankSegment:
        """A chunk's segment, checked against the bank, which is not changed: ``mapped`` logical (k,d,hf,wf) (any crop of a channels-last map), ``images`` (k,3,H,W) as the reference hands them
        to Projector.compute (uncropped: grid_sample normalises by their size), ``img_meta`` with the chunk's k extrinsics."""
        if not mapped.is_cuda:
            raise RuntimeError("nerfdet_amd.rays: tensors must live on the GPU (no CPU fallback)")
        k, d = mapped.shape[0], mapped.shape[1]
        if images.dim() != 4 or images.shape[0] != k or images.shape[1] != 3:
            raise ValueError(f"ViewBank.append: images {tuple(images.shape)} for {k} mapped maps")
        if d % 4 or d > 128:
            raise ValueError(f"ViewBank.append: d={d} must be a multiple of 4, at most 128")
        ke, h, w = _camera_matrices(_compute_projection(img_meta).squeeze(0))
        if ke.shape[0] != k:
            raise ValueError(f"ViewBank.append: {ke.shape[0]} extrinsics for {k} views")
        if self.segments:
            s0 = self.segments[0]
            if tuple(mapped.shape[1:]) != (s0.feat.shape[3], s0.feat.shape[1], s0.feat.shape[2]) or tuple(images.shape[2:]) != tuple(s0.rgb4.shape[1:3]) \
                    or (h, w) != s0.img_hw or mapped.device != s0.feat.device:
                raise ValueError("ViewBank.append: the chunk's map, image or camera size differs from the bank's")
        feat = mapped.detach().to(torch.float32).permute(0, 2, 3, 1).contiguous()
        if feat.data_ptr() == mapped.data_ptr():
            feat = feat.clone()                                # a copy of its own: the producer may reuse the chunk's map
        rgb = images.detach()
        if rgb.dtype != torch.float32:
            rgb = rgb.float()
        if rgb.stride(3) != 1:
            rgb = rgb.contiguous()
        rgb = rgb.to(feat.device)
        rgb4 = torch.empty((k, rgb.shape[2], rgb.shape[3], 4), dtype=torch.float32, device=feat.device)
        check(_lib.load().ndet_pack_rgb_nhwc4(_ptr(rgb), k, rgb.shape[2], rgb.shape[3], rgb.stride(0), rgb.stride(1), rgb.stride(2), _ptr(rgb4),
                                              _stream(feat)), "pack_rgb_nhwc4")
        assert feat.data_ptr() % 16 == 0 and rgb4.data_ptr() % 16 == 0
        return BankSegment(feat, rgb4, ke, (h, w))

    def drop_oldest(self, k_segments: int = 1) -> None:
        if isinstance(k_segments, bool) or not isinstance(k_segments, int) or not 0 <= k_segments <= len(self.segments):
            raise ValueError(f"ViewBank.drop_oldest: k={k_segments!r} for {len(self.segments)} segments held")
        if k_segments:
            del self.segments[:k_segments]
            self._table = None

    def clear(self) -> None:
        self.drop_oldest(len(self.segments))

    def table(self) -> Tuple[Tensor, int]:
        """``(device table (n_views, 64) uint8 of NdetBankView rows, n_views)`` for the segments held now."""
        n = self.n_views
        if n == 0:
            raise RuntimeError("the view bank holds no views")
        if self._table is not None:
            return self._table
        rows = (_lib.NdetBankView * n)()
        i = 0
        for s in self.segments:
            fp, ip = s.feat.stride(0) * 4, s.rgb4.stride(0) * 4
            ke = s.ke.reshape(-1, 12).tolist()
            for j in range(s.n_views):
                rows[i].feat, rows[i].rgb4 = s.feat.data_ptr() + j * fp, s.rgb4.data_ptr() + j * ip
                rows[i].ke[:] = ke[j]
                i += 1
        host = torch.from_numpy(np.frombuffer(rows, dtype=np.uint8).reshape(n, 64).copy())
        self._table = (_to_device(host, self.segments[0].feat.device), n)
        return self._table


def _bank_call(bank: ViewBank, n_views: int, n: int):
    """What a bank sampler's launch over ``n_views`` views and ``n`` sample points takes from the bank's sizes (its oldest segment's, which
    every segment shares): the entry points' ``(img_h, img_w, H, W, d, hf, wf)``, the outputs on the bank's device, the bytes for the trace."""
    s0 = bank.segments[0]
    _, hf, wf, d = s0.feat.shape
    H, W = s0.rgb4.shape[1], s0.rgb4.shape[2]
    nbytes = 4 * (n_views * 4 * H * W + n_views * d * hf * wf + 2 * (3 + d) * n)
    return (*s0.img_hw, H, W, d, hf, wf), _stats_buffers(n, d, s0.feat.device), nbytes


def ray_view_stats_bank(xyz: Tensor, bank: ViewBank):
    """:func:`ray_view_stats` over a :class:`ViewBank`: sample points (R,S,3) -> ``globalfeat`` (R,S,2*(3+d)), ``pixel_mask`` (R,S) bool,
    ``view_count`` (R,S) int32 (projection.py:91-151 + render_ray.py:71-93, 299-303), for any number of views in any number of segments.
    The bank is not changed.  At most 128 views give the packed sampler's bits over the concatenated segments."""
    if not xyz.is_cuda:
        raise RuntimeError("nerfdet_amd.rays: tensors must live on the GPU (no CPU fallback)")
    table, n_v = bank.table()
    s0 = bank.segments[0]
    if xyz.device != s0.feat.device:
        raise ValueError("ray_view_stats_bank: the points and the bank live on different devices")
    shape = xyz.shape[:-1]
    pts = xyz.to(torch.float32).reshape(-1, 3).contiguous()
    n = pts.shape[0]
    geom, (glob, pm, vc), nbytes = _bank_call(bank, n_v, n)
    trace.span("k_ray_stats_bank", lambda: check(
        _lib.load().ndet_ray_view_stats_bank(_ptr(pts), n, _ptr(table), n_v, *geom, _ptr(glob), _ptr(pm), _ptr(vc), _stream(xyz)),
        "ray_view_stats_bank"), bytes=nbytes, kind="hbm")
    return glob.view(*shape, -1), pm.view(*shape), vc.view(*shape)


def ray_view_stats_bank_group(xyz_list, banks):
    """:func:`ray_view_stats_bank` for several banks in ONE launch (k_ray_stats_bank_group): ``xyz_list[i]`` (..., 3) are the sample points
    of ``banks[i]``; returns a list of ``(globalfeat, pixel_mask, view_count)``, one per bank, each shaped as :func:`ray_view_stats_bank`
    shapes it and a view into the call's concatenated buffers.  The banks share map, image and camera sizes and the device (else
    ValueError); 1 .. 64 banks, a single one goes through the same entry point.  Every bank's outputs are :func:`ray_view_stats_bank`'s
    over that bank and its points bit for bit, whatever the other banks or their order.  No bank is changed; as with one bank, the call
    and the banks' evictions belong on one stream (:class:`ViewBank`)."""
    xyz_list = list(xyz_list)
    glob, pm, vc, _ = bank_group_stats(xyz_list, banks)
    out, at = [], 0
    for x in xyz_list:
        shape, c = x.shape[:-1], x.numel() // 3
        out.append((glob[at:at + c].view(*shape, -1), pm[at:at + c].view(*shape), vc[at:at + c].view(*shape)))
        at += c
    return out


def bank_group_stats(xyz_list, banks):
    """The launch of :func:`ray_view_stats_bank_group` with its buffers whole: ``(globalfeat (P, 2*(3+d)), pixel_mask (P,), view_count (P,),
    points (P, 3))`` over the ``P = sum of points`` rows, bank i's rows after bank i-1's."""
    xyz_list, banks = list(xyz_list), list(banks)
    n = len(banks)
    if len(xyz_list) != n or not 1 <= n <= _lib.NDET_GROUP_MAX:
        raise ValueError(f"ray_view_stats_bank_group: {len(xyz_list)} point sets for {n} banks (1 .. {_lib.NDET_GROUP_MAX})")
    for x in xyz_list:
        if not x.is_cuda:
            raise RuntimeError("nerfdet_amd.rays: tensors must live on the GPU (no CPU fallback)")
    tables = [b.table() for b in banks]          # RuntimeError for an empty bank
    s0 = banks[0].segments[0]
    dev = s0.feat.device
    for i, (x, b) in enumerate(zip(xyz_list, banks)):
        s = b.segments[0]
        if s.feat.shape[1:] != s0.feat.shape[1:] or s.rgb4.shape[1:] != s0.rgb4.shape[1:] or s.img_hw != s0.img_hw:
            raise ValueError(f"ray_view_stats_bank_group: bank {i}'s map, image or camera size differs from bank 0's")
        if s.feat.device != dev or x.device != dev:
            raise ValueError(f"ray_view_stats_bank_group: bank {i} or its points live on another device than bank 0")
        if x.shape[-1] != 3 or x.numel() == 0:
            raise ValueError(f"ray_view_stats_bank_group: points {tuple(x.shape)} of bank {i} must be (..., 3) with at least one point")
    flat = [x.to(torch.float32).reshape(-1, 3) for x in xyz_list]
    counts = [f.shape[0] for f in flat]
    pts = flat[0].contiguous() if n == 1 else torch.cat(flat, dim=0)
    sel = _lib.NdetBankGroupSel()
    sel.size, sel.n = ctypes.sizeof(_lib.NdetBankGroupSel), n
    for i, ((table, n_v), c) in enumerate(zip(tables, counts)):
        sel.views[i], sel.n_views[i], sel.n_points[i] = table.data_ptr(), n_v, c
    geom, (glob, pm, vc), nbytes = _bank_call(banks[0], sum(t[1] for t in tables), pts.shape[0])
    trace.span("k_ray_stats_bank_group", lambda: check(
        _lib.load().ndet_ray_view_stats_bank_group(_ptr(pts), ctypes.byref(sel), *geom, _ptr(glob), _ptr(pm), _ptr(vc), _stream(pts)),
        "ray_view_stats_bank_group"), bytes=nbytes, kind="hbm")
    return glob, pm, vc, pts


# ------------------------------------------------------------------------------------------------------
# empty-space skipping (csrc/skip_empty_kernels.hip): the bank sampler's count pass alone, and an ordered cull against an occupancy grid
# ------------------------------------------------------------------------------------------------------
def ray_view_count_bank(xyz: Tensor, bank: ViewBank):
    """The count pass of :func:`ray_view_stats_bank` alone (k_ray_count_bank): sample points (..., 3) -> ``(pixel_mask (...) bool,
    view_count (...) int32)``, that function's second and third output bit for bit, with no gathers.  The bank is not changed."""
    if not xyz.is_cuda:
        raise RuntimeError("nerfdet_amd.rays: tensors must live on the GPU (no CPU fallback)")
    table, n_v = bank.table()
    s0 = bank.segments[0]
    if xyz.device != s0.feat.device:
        raise ValueError("ray_view_count_bank: the points and the bank live on different devices")
    shape = xyz.shape[:-1]
    pts = xyz.to(torch.float32).reshape(-1, 3).contiguous()
    n = pts.shape[0]
    pm = torch.empty((n,), dtype=torch.bool, device=pts.device)
    vc = torch.empty((n,), dtype=torch.int32, device=pts.device)
    trace.span("k_ray_count_bank", lambda: check(
        _lib.load().ndet_ray_view_count_bank(_ptr(pts), n, _ptr(table), n_v, *s0.img_hw, _ptr(pm), _ptr(vc), _stream(xyz)),
        "ray_view_count_bank"), bytes=17 * n + 64 * n_v, kind="hbm")
    return pm.view(*shape), vc.view(*shape)


class OccupancyGrid:
    """Where a streamed scene may hold matter: ``bits`` (ops.occupancy_bits' words, on the device) over the detection lattice of
    ``n_voxels`` voxels whose first point is ``p0`` and whose pitch is ``voxel_size`` (three float32 each, on the host), and ``outside``:
    'keep' or 'cull', what becomes of a sample outside the lattice.  ``threshold`` and ``dilate`` record how it was made (None when
    unknown).  :func:`cull_points` reads it; ``SceneStream.occupancy`` makes it."""
    __slots__ = ("bits", "n_voxels", "p0", "voxel_size", "outside", "threshold", "dilate")

    def __init__(self, bits: Tensor, n_voxels, p0, voxel_size, outside: str = "keep", threshold=None, dilate=None):
        nv = tuple(int(v) for v in (n_voxels.tolist() if isinstance(n_voxels, Tensor) else n_voxels))
        p0 = tuple(float(np.float32(v)) for v in (p0.tolist() if isinstance(p0, (Tensor, np.ndarray)) else p0))
        vs = tuple(float(np.float32(v)) for v in (voxel_size.tolist() if isinstance(voxel_size, (Tensor, np.ndarray)) else voxel_size))
        if len(nv) != 3 or len(p0) != 3 or len(vs) != 3 or min(nv) < 1:
            raise ValueError(f"OccupancyGrid: n_voxels {nv}, p0 {p0} and voxel_size {vs} must hold three values each, n_voxels positive")
        if not all(np.isfinite(p0)) or not all(np.isfinite(vs)) or min(vs) <= 0.0:
            raise ValueError(f"OccupancyGrid: p0 {p0} must be finite and voxel_size {vs} positive and finite")
        if outside not in _lib.NDET_OUTSIDE:
            raise ValueError(f"OccupancyGrid: outside={outside!r} must be 'keep' or 'cull'")
        words = (nv[0] * nv[1] * nv[2] + 31) // 32
        if not isinstance(bits, Tensor) or bits.dtype != torch.int32 or tuple(bits.shape) != (words,) or not bits.is_contiguous():
            raise ValueError(f"OccupancyGrid: bits must be a contiguous ({words},) int32 tensor for {nv} voxels")
        self.bits, self.n_voxels, self.p0, self.voxel_size, self.outside = bits, nv, p0, vs, outside
        self.threshold, self.dilate = threshold, dilate


class CarveStore:
    """A carved scene's counter segments (ops.carve_accumulate's words over one fine lattice of ``n`` voxels), oldest first, following the
    scene's states as a :class:`ViewBank` follows them: :meth:`push`, :meth:`drop_oldest`, :meth:`clear`.  Unwindowed: ONE segment, into
    which every chunk accumulates.  Windowed: one segment per chunk held.  :meth:`target` hands out the buffer the next chunk's counts
    go into -- the held segment of an unwindowed store, else a zeroed spare that belongs to no window until it is pushed; a dropped
    segment is zeroed and kept, so a sliding window allocates nothing once it has slid.  A chunk without depth pushes its target as it
    is: all zero, no evidence.  4 n bytes a segment."""

    def __init__(self, n: int, device, windowed: bool):
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
            raise ValueError(f"CarveStore: n={n!r} voxels")
        self.n, self.device, self.windowed = int(n), device, bool(windowed)
        self.segments: List[Tensor] = []
        self._spare: List[Tensor] = []

    def nbytes(self) -> int:
        """Device bytes owned: the segments held and the spares."""
        return 4 * self.n * (len(self.segments) + len(self._spare))

    def target(self) -> Tensor:
        """The (n,) int32 buffer the next chunk's counts are added into; the store is not changed."""
        if not self.windowed and self.segments:
            return self.segments[0]
        return self._spare.pop() if self._spare else torch.zeros((self.n,), dtype=torch.int32, device=self.device)

    def give_back(self, seg: Tensor) -> None:
        """A target whose chunk failed: zeroed and spare again (an unwindowed store's held segment is never given back)."""
        if any(seg is s for s in self.segments):
            raise ValueError("CarveStore.give_back: the segment is held")
        seg.zero_()
        self._spare.append(seg)

    def push(self, seg: Tensor) -> None:
        """The chunk's target joins the store as its newest segment (unwindowed: it is, or becomes, the one segment)."""
        if seg.dtype != torch.int32 or tuple(seg.shape) != (self.n,):
            raise ValueError(f"CarveStore.push: a segment is an ({self.n},) int32 tensor, got {tuple(seg.shape)} {seg.dtype}")
        if not self.windowed and self.segments:
            if seg is not self.segments[0]:
                raise ValueError("CarveStore.push: an unwindowed store accumulates into its one segment (target())")
            return
        self.segments.append(seg)

    def drop_oldest(self, k_segments: int = 1) -> None:
        if isinstance(k_segments, bool) or not isinstance(k_segments, int) or not 0 <= k_segments <= len(self.segments):
            raise ValueError(f"CarveStore.drop_oldest: k={k_segments!r} for {len(self.segments)} segments held")
        for seg in self.segments[:k_segments]:
            seg.zero_()
            self._spare.append(seg)
        del self.segments[:k_segments]

    def clear(self) -> None:
        self.drop_oldest(len(self.segments))


class CloudStore(CarveStore):
    """A cloud scene's record segments (ops.cloud_accumulate's (n, 8) int32 sums over one fine lattice), oldest first, following the scene's
    states as a :class:`CarveStore` does, with ``pixels[j]``, the pixels of the chunks segment j has taken -- an upper bound of what any of
    its voxels holds.  A sum of 8-bit values is exact below 2^24 contributions, so no segment may pass ``budget`` (default 2^24 - 1)
    pixels: a chunk of more is refused; an unwindowed store, which accumulates into its newest segment, opens a further one when the
    next chunk would take that past the budget, and is refused, whole, once it holds :data:`ops.RING_MAX` segments.  Every refusal is a
    ValueError of :meth:`target`, which changes nothing.  Windowed: one segment per chunk held.  32 n bytes a segment."""

    def __init__(self, n: int, device, windowed: bool, budget: int = 2 ** 24 - 1):
        super().__init__(n, device, windowed)
        if isinstance(budget, bool) or not isinstance(budget, (int, np.integer)) or not 1 <= budget < 2 ** 24:
            raise ValueError(f"CloudStore: budget={budget!r} must be an int from 1 to 2^24 - 1")
        self.budget = int(budget)
        self.pixels: List[int] = []

    def nbytes(self) -> int:
        return 4 * ops.CLOUD_WORDS * self.n * (len(self.segments) + len(self._spare))

    def _joins(self, pixels: int) -> bool:
        return not self.windowed and bool(self.segments) and self.pixels[-1] + pixels <= self.budget

    def check(self, pixels: int = 0) -> None:
        """What :meth:`target` refuses for a next chunk of ``pixels`` pixels (ValueError), with no device work."""
        if isinstance(pixels, bool) or not isinstance(pixels, (int, np.integer)) or pixels < 0:
            raise ValueError(f"CloudStore: pixels={pixels!r}")
        if pixels > self.budget:
            raise ValueError(f"CloudStore: a chunk of {pixels} pixels is more than a segment may hold ({self.budget}); add fewer views at a time")
        if not self.windowed and not self._joins(pixels) and len(self.segments) >= ops.RING_MAX:
            raise ValueError(f"CloudStore: {ops.RING_MAX} segments of {self.budget} pixels are full; reset the scene or stream it through a window")

    def target(self, pixels: int = 0) -> Tensor:
        """The (n, 8) int32 buffer a next chunk of ``pixels`` pixels is added into; the store is not changed."""
        self.check(pixels)
        if self._joins(pixels):
            return self.segments[-1]
        return self._spare.pop() if self._spare else torch.zeros((self.n, ops.CLOUD_WORDS), dtype=torch.int32, device=self.device)

    def push(self, seg: Tensor, pixels: int = 0) -> None:
        """The chunk's target joins the store (unwindowed: it is the newest segment, or becomes it) with its ``pixels``."""
        if seg.dtype != torch.int32 or tuple(seg.shape) != (self.n, ops.CLOUD_WORDS):
            raise ValueError(f"CloudStore.push: a segment is an ({self.n}, {ops.CLOUD_WORDS}) int32 tensor, got {tuple(seg.shape)} {seg.dtype}")
        if self.segments and seg is self.segments[-1]:
            if not self._joins(pixels):
                raise ValueError("CloudStore.push: the newest segment cannot take this chunk (target())")
            self.pixels[-1] += int(pixels)
            return
        if any(seg is s for s in self.segments) or self._joins(pixels) or len(self.segments) >= ops.RING_MAX or pixels > self.budget:
            raise ValueError("CloudStore.push: not the segment target() hands out for this chunk")
        self.segments.append(seg)
        self.pixels.append(int(pixels))

    def drop_oldest(self, k_segments: int = 1) -> None:
        super().drop_oldest(k_segments)
        del self.pixels[:k_segments]


def _kept_points(m: int, device):
    """What a compaction of points returns: ``(idx (M,) int32, pts_kept (M, 3) float32)``, to be written."""
    return torch.empty((m,), dtype=torch.int32, device=device), torch.empty((m, 3), dtype=torch.float32, device=device)


def cull_points(pts: Tensor, occ: OccupancyGrid):
    """Ordered compaction of ``pts`` (..., 3) against ``occ``: ``(idx (M,) int32, pts_kept (M, 3))``, the flat indices of the kept points
    in ascending order and those points.  Per axis, in float32, ``i = int(floor((x - p0) / voxel_size + 0.5))`` is the nearest lattice
    point; a point with all three in range and finite coordinates is kept iff its bit is set, any other iff ``occ.outside == 'keep'``.
    Two launches (k_cull_count, k_cull_write) around one prefix sum; M reaches the host in ONE device-to-host read, the call's only
    synchronisation; ``M = 0`` skips the second launch.  The same bytes on every call."""
    if not (pts.is_cuda and occ.bits.is_cuda):
        raise RuntimeError("nerfdet_amd.rays: tensors must live on the GPU (no CPU fallback)")
    if pts.device != occ.bits.device:
        raise ValueError("cull_points: the points and the grid live on different devices")
    p = pts.to(torch.float32).reshape(-1, 3).contiguous()
    n = p.shape[0]
    if n < 1:
        raise ValueError(f"cull_points: points {tuple(pts.shape)} must be (..., 3) with at least one point")
    lib = _lib.load()
    geom = ((ctypes.c_int * 3)(*occ.n_voxels), _lib.float3(occ.p0), _lib.float3(occ.voxel_size), _lib.NDET_OUTSIDE[occ.outside])
    counts = torch.empty((int(lib.ndet_cull_blocks(n)),), dtype=torch.int32, device=p.device)
    trace.span("k_cull_count", lambda: check(lib.ndet_cull_count(_ptr(p), n, _ptr(occ.bits), *geom, _ptr(counts), _stream(p)), "cull_count"),
               bytes=12 * n + 4 * counts.numel(), kind="hbm")
    first, m = ops.compaction_offsets(counts)
    idx, kept = _kept_points(m, p.device)
    if m:
        trace.span("k_cull_write", lambda: check(lib.ndet_cull_write(_ptr(p), n, _ptr(occ.bits), *geom, _ptr(first), _ptr(idx), _ptr(kept),
                                                                     _stream(p)), "cull_write"),
                   bytes=12 * n + 16 * m, kind="hbm")
    return idx, kept


# ------------------------------------------------------------------------------------------------------
# early ray termination (csrc/early_stop_kernels.hip): a transmittance state per ray, and the live rays' samples of one depth segment
# ------------------------------------------------------------------------------------------------------
def advance_transmittance(raw: Tensor, T: Tensor, s0: int, s1: int) -> Tensor:
    """``T[r] *= prod over columns s0 <= s < s1 of ((1 - a) + 1e-10)``, ``a = 1 - exp(-raw[r, s, 3])``, s ascending, in k_composite's
    float32 statements (k_ray_advance): advanced from 1 over columns ``[0, b)``, ``T`` is ``raw2outputs(raw, ...)['transparency'][:, b]``
    bit for bit.  ``raw`` (R, S, 4) and ``T`` (R,) contiguous float32; ``T`` is updated in place and returned.  ``s0 == s1`` launches
    nothing."""
    if not (raw.is_cuda and T.is_cuda):
        raise RuntimeError("nerfdet_amd.rays: tensors must live on the GPU (no CPU fallback)")
    if raw.dim() != 3 or raw.shape[2] != 4 or tuple(T.shape) != (raw.shape[0],) or raw.dtype != torch.float32 or T.dtype != torch.float32 \
            or not raw.is_contiguous() or not T.is_contiguous() or raw.device != T.device:
        raise ValueError(f"advance_transmittance: raw {tuple(raw.shape)} must be contiguous float32 (R, S, 4) and T {tuple(T.shape)} (R,) beside it")
    r, s = raw.shape[:2]
    call = lambda: check(_lib.load().ndet_ray_advance(_ptr(raw), _ptr(T), r, s, int(s0), int(s1), _stream(raw)), "advance_transmittance")
    if s0 == s1:
        call()                                                 # the host checks alone
    else:
        trace.span("k_ray_advance", call, bytes=16 * r * (s1 - s0) + 8 * r, kind="hbm")
    return T


def front_segment(pts: Tensor, T: Tensor, s0: int, s1: int, eps: float, occ: Optional[OccupancyGrid] = None, all_live: bool = False):
    """Ordered compaction of the live rays' samples of the segment ``[s0, s1)`` (at most 32 columns) of ``pts`` (R, S, 3):
    ``(idx (M,) int32, pts_kept (M, 3))``, the flat indices ``f = r S + s`` of the kept samples in ascending order and those points.  A
    sample is kept iff ``not (T[r] < eps)`` in float32 (a NaN transmittance keeps its ray) and, with ``occ``, :func:`cull_points` would
    keep it -- in the same launch.  Two launches (k_front_count, k_front_write) around one prefix sum; M reaches the host in ONE
    device-to-host read, the call's only synchronisation; ``M = 0`` skips the second launch.  ``all_live=True`` (no ``occ``) is the
    caller's word that no ray has stopped: ``M = R (s1 - s0)`` is then known on the host, and neither the count launch nor the read
    happens.  The same bytes on every call."""
    if not (pts.is_cuda and T.is_cuda and (occ is None or occ.bits.is_cuda)):
        raise RuntimeError("nerfdet_amd.rays: tensors must live on the GPU (no CPU fallback)")
    if pts.dim() != 3 or pts.shape[2] != 3 or tuple(T.shape) != (pts.shape[0],) or T.dtype != torch.float32 or not T.is_contiguous():
        raise ValueError(f"front_segment: pts {tuple(pts.shape)} must be (R, S, 3) and T {tuple(T.shape)} contiguous float32 (R,)")
    if pts.device != T.device or (occ is not None and occ.bits.device != pts.device):
        raise ValueError("front_segment: the points, the transmittance and the grid live on different devices")
    if all_live and occ is not None:
        raise ValueError("front_segment: all_live says nothing about what a grid culls")
    p = pts.to(torch.float32).contiguous()
    r, s = p.shape[:2]
    s0, s1, eps = int(s0), int(s1), float(eps)
    w = s1 - s0
    lib = _lib.load()
    if occ is None:
        geom = (None, None, None, None, 0)
    else:
        geom = (_ptr(occ.bits), (ctypes.c_int * 3)(*occ.n_voxels), _lib.float3(occ.p0), _lib.float3(occ.voxel_size), _lib.NDET_OUTSIDE[occ.outside])
    blocks = int(lib.ndet_front_blocks(r, w))
    if all_live and blocks:
        per = 512 >> max(2, (w - 1).bit_length())              # rays of a block: 512 / the nominal width (include/nerfdet_hip.h)
        first = torch.arange(blocks, dtype=torch.int32, device=p.device) * (per * w)
        m = r * w
    else:
        counts = torch.empty((blocks,), dtype=torch.int32, device=p.device)
        trace.span("k_front_count", lambda: check(lib.ndet_front_count(_ptr(p), r, s, s0, s1, _ptr(T), eps, *geom, _ptr(counts), _stream(p)),
                                                  "front_count"), bytes=4 * r + (12 * r * w if occ is not None else 0) + 4 * blocks, kind="hbm")
        first, m = ops.compaction_offsets(counts)
    idx, kept = _kept_points(m, p.device)
    if m:
        trace.span("k_front_write", lambda: check(lib.ndet_front_write(_ptr(p), r, s, s0, s1, _ptr(T), eps, *geom, _ptr(first), _ptr(idx),
                                                                       _ptr(kept), _stream(p)), "front_write"),
                   bytes=4 * r + 12 * r * w + 16 * m, kind="hbm")
    return idx, kept


class Projector:
    """projection.py:20-151.  ``compute`` keeps the reference's signature and materialised outputs."""

    def __init__(self, device="cuda"):
        self.device = device

    def compute(self, xyz, train_imgs, train_cameras, featmaps=None, grid_sample=True):
        assert (train_imgs.shape[0] == 1) and (train_cameras.shape[0] == 1)  # projection.py:100-101
        assert grid_sample, "grid_sample=False indexes (y, y) in the reference (projection.py:142) and is dead code"
        assert featmaps is not None, "featmaps=None is only reached in nerf_mode='volume' (dead in the configs)"
        if not xyz.is_cuda:
            raise RuntimeError("nerfdet_amd.rays: tensors must live on the GPU (no CPU fallback)")
        ke, h, w = _camera_matrices(train_cameras.squeeze(0))
        ke = _to_device(ke, xyz.device)
        rgb, f = _prep_sources(train_imgs, featmaps)
        n_v, d, hf, wf = f.shape
        r, s = xyz.shape[:2]
        pts = xyz.to(torch.float32).reshape(-1, 3).contiguous()
        out = torch.empty((r, s, n_v, 3 + d), dtype=torch.float32, device=xyz.device)
        mask = torch.empty((r, s, n_v, 1), dtype=torch.float32, device=xyz.device)
        check(_lib.load().ndet_project_sample(_ptr(pts), r * s, _ptr(ke), n_v, h, w, _ptr(rgb), rgb.shape[2], rgb.shape[3],
                                              rgb.stride(0), rgb.stride(1), rgb.stride(2), _ptr(f), d, hf, wf, f.stride(0),
                                              f.stride(2), _ptr(out), _ptr(mask), _stream(xyz)), "Projector.compute")
        return out, mask


def compute_mask_points(feature: Tensor, mask: Tensor) -> Tuple[Tensor, Tensor]:
    """render_ray.py:71-93 on already-materialised samples (API parity; the fused path is ray_view_stats).
    Plain tensor algebra on the GPU."""
    denom = torch.sum(mask, dim=2, keepdim=True) + 1e-8
    mean = torch.sum(feature * (mask / denom), dim=2, keepdim=True)
    var = torch.sum((feature - mean) ** 2, dim=2, keepdim=True) / denom
    return mean, torch.exp(-var)


# ------------------------------------------------------------------------------------------------------
# A9
# ------------------------------------------------------------------------------------------------------
def sample_along_camera_ray(ray_o, ray_d, depth_range, N_samples, inv_uniform=False, det=False, t_rand: Optional[Tensor] = None):
    """render_ray.py:145-189.  ``t_rand`` (R,S) replaces the reference's ``torch.rand_like`` draw when given."""
    assert not inv_uniform, "inv_uniform sampling is never enabled by the nerfdet configs"
    near, far = float(depth_range[0]), float(depth_range[1])
    assert near > 0 and far > 0 and far > near  # render_ray.py:161
    if not ray_d.is_cuda:
        raise RuntimeError("nerfdet_amd.rays: tensors must live on the GPU (no CPU fallback)")
    o = ray_o.to(torch.float32).contiguous()
    d = ray_d.to(torch.float32).contiguous()
    r = d.shape[0]
    if not det and t_rand is None:
        t_rand = torch.rand((r, N_samples), dtype=torch.float32, device=d.device)
    if det:
        t_rand = None
    elif t_rand is not None:
        t_rand = t_rand.to(torch.float32).contiguous()
    pts = torch.empty((r, N_samples, 3), dtype=torch.float32, device=d.device)
    z = torch.empty((r, N_samples), dtype=torch.float32, device=d.device)
    check(_lib.load().ndet_sample_along_rays(_ptr(o), _ptr(d), r, N_samples, near, far, _ptr(t_rand), _ptr(pts), _ptr(z), _stream(d)),
          "sample_along_camera_ray")
    return pts, z


# ------------------------------------------------------------------------------------------------------
# hierarchical sampling (render_ray.py:96-142, 343-356)
# ------------------------------------------------------------------------------------------------------
def _uniforms(u: Optional[Tensor], det: bool, r: int, n: int, device) -> Tuple[Tensor, int]:
    """The ``u`` of sample_pdf (render_ray.py:113-117) as the C ABI takes it: ``(tensor, row stride)``.  ``det``: torch's own
    ``linspace(0, 1, n)`` as ONE row every ray shares (stride 0); else the caller's ``u`` -- (R, n), or (n,) / (1, n) shared -- or a
    ``torch.rand`` draw."""
    if det:
        return torch.linspace(0., 1., n, device=device), 0
    if u is None:
        return torch.rand((r, n), dtype=torch.float32, device=device), n
    if not u.is_cuda:
        raise RuntimeError("nerfdet_amd.rays: tensors must live on the GPU (no CPU fallback)")
    u = u.to(torch.float32).contiguous()
    if tuple(u.shape) in ((n,), (1, n)):
        return u, 0
    if tuple(u.shape) != (r, n):
        raise ValueError(f"u {tuple(u.shape)} must be ({r}, {n}), or ({n},) shared by every ray")
    return u, n


def sample_pdf(bins, weights, N_samples, det=False, u: Optional[Tensor] = None):
    """render_ray.py:96-142: ``bins`` (R, M+1), ``weights`` (R, M) -> (R, N_samples) depths drawn from the piecewise-constant pdf the
    weights give over the bins.  ``u`` (R, N_samples) replaces the reference's ``torch.rand`` draw when given (``det`` wins, as in
    :func:`sample_along_camera_ray`).  ``weights`` is NOT modified: the reference adds 1e-5 to it in place and is only ever handed a
    clone.  The sums run in the kernel's order (csrc/importance_kernels.hip), so the depths agree with torch's to rounding in CDF
    space, not bit for bit.  M <= 254, N_samples <= 256."""
    if not (bins.is_cuda and weights.is_cuda):
        raise RuntimeError("nerfdet_amd.rays: tensors must live on the GPU (no CPU fallback)")
    r, m = weights.shape
    if tuple(bins.shape) != (r, m + 1):
        raise ValueError(f"sample_pdf: bins {tuple(bins.shape)} for weights {tuple(weights.shape)}")
    b = bins.detach().to(torch.float32).contiguous()
    w = weights.detach().to(torch.float32).contiguous()
    n = int(N_samples)
    uu, stride = _uniforms(u, det, r, n, b.device)
    out = torch.empty((r, n), dtype=torch.float32, device=b.device)
    trace.span("k_sample_pdf", lambda: check(
        _lib.load().ndet_sample_pdf(_ptr(b), _ptr(w), r, m, _ptr(uu), stride, n, _ptr(out), _stream(b)), "sample_pdf"))
    return out


def importance_merge(z_vals, weights, ray_o, ray_d, N_importance, det, u: Optional[Tensor] = None):
    """The fine pass's samples (render_ray.py:343-356, ``inv_uniform=False``) in ONE launch (k_importance_merge): ``z_vals``,
    ``weights`` (R, S) of the coarse pass -> ``(pts (R, S+k, 3), z_vals (R, S+k), z_samples (R, k))`` with ``z_samples =
    sample_pdf(.5 * (z[1:] + z[:-1]), weights[:, 1:-1], k, det, u)`` bit for bit, the merged depths ``sort(cat(z_vals, z_samples))``
    and ``pts = z * ray_d + ray_o``.  3 <= S <= 256, 1 <= k <= 256.  Nothing is differentiable here (the reference detaches the
    weights, render_ray.py:332)."""
    if not (z_vals.is_cuda and weights.is_cuda and ray_o.is_cuda and ray_d.is_cuda):
        raise RuntimeError("nerfdet_amd.rays: tensors must live on the GPU (no CPU fallback)")
    r, s = z_vals.shape
    k = int(N_importance)
    if tuple(weights.shape) != (r, s) or tuple(ray_o.shape) != (r, 3) or tuple(ray_d.shape) != (r, 3):
        raise ValueError(f"importance_merge: z_vals {tuple(z_vals.shape)}, weights {tuple(weights.shape)}, ray_o {tuple(ray_o.shape)}, "
                         f"ray_d {tuple(ray_d.shape)}")
    z = z_vals.detach().to(torch.float32).contiguous()
    w = weights.detach().to(torch.float32).contiguous()
    o = ray_o.detach().to(torch.float32).contiguous()
    d = ray_d.detach().to(torch.float32).contiguous()
    uu, stride = _uniforms(u, det, r, k, z.device)
    tot = s + max(k, 0)
    z_out = torch.empty((r, tot), dtype=torch.float32, device=z.device)
    pts = torch.empty((r, tot, 3), dtype=torch.float32, device=z.device)
    z_samples = torch.empty((r, max(k, 0)), dtype=torch.float32, device=z.device)
    trace.span("k_importance_merge", lambda: check(
        _lib.load().ndet_importance_merge(_ptr(z), _ptr(w), _ptr(o), _ptr(d), r, s, _ptr(uu), stride, k, _ptr(z_out), _ptr(pts),
                                          _ptr(z_samples), _stream(z)), "importance_merge"),
        bytes=4 * r * (2 * s + 5 * tot), kind="hbm")
    return pts, z_out, z_samples


FINE_MLP_ROWS = 8192 * 64     # sample rows per nerf_mlp call of a fine pass: what a coarse pass of RENDER_TESTING_RAYS rays x 64 samples hands it


MLP_STABLE_ROWS = 24576       # sample rows from which on a nerf_mlp call's launches no longer depend on its row count (mlp_rows_padded)


def mlp_rows_padded(nerf_mlp, pts, ray_d, globalfeat, floor: int):
    """``nerf_mlp`` over flat sample rows -- ``pts`` (n, 3), ``ray_d`` (n, 3), ``globalfeat`` (n, F) -- as ``(rgb, sigma)``, the call
    padded with copies of its first row up to ``floor`` rows.  No scale is shared across a call's rows (:func:`fine_mlp`), but WHICH
    launches a call makes depends on its row count: below 192 tiles of 128 rows the bottleneck layer leaves the 128 x 256 tile
    (conv3d.choose_tiling_split), and below some 16 384 rows ATen's 128 -> 3 GEMM of the colour head picks another kernel; both sum in
    another order, and ``rgb`` moves in its last bit (2.4e-7 measured; sigma does not move).  From MLP_STABLE_ROWS rows on a row's
    result was the same in every call measured then (24 575 .. 262 143 rows) -- sizes measured, not a guarantee: a later call of exactly
    132 292 rows moved ``rgb``'s last bit (1.8e-7) against calls of 131 072, 147 456 and 262 144 rows over the same rows.  A caller whose row counts fall below that, and who owes the
    bits of a larger call, pads up to ``min(MLP_STABLE_ROWS, rows of the larger call)``: at that size the call makes the larger call's
    launches or is the larger call's size."""
    n = pts.shape[0]
    if n >= floor:
        return nerf_mlp(pts, ray_d, globalfeat)
    pad = lambda t: torch.cat([t, t[:1].expand(floor - n, *t.shape[1:])], dim=0)
    rgb, sigma = nerf_mlp(pad(pts), pad(ray_d), pad(globalfeat))
    return rgb[:n], sigma[:n]


def fine_mlp(nerf_mlp, pts, ray_d, globalfeat):
    """``nerf_mlp(pts, ray_d, globalfeat)`` over the (R, S + k, .) samples of a fine pass, as ``(rgb, sigma)``: in one call up to
    FINE_MLP_ROWS sample rows, beyond that in the fewest calls of whole rays, equal in size to within one ray, that stay under it.  The
    row MLP's 1x1-convolution kernels address at most 2 GB per operand, which 8192 rays x 128 samples of the cfg2 widths exceed.  The
    split is a function of (R, S + k) alone, so every renderer's fine pass makes the same calls over the same rays.  No scale is shared
    across a call's rows: the fused trunk scales per row, and the ``linear_rows`` layers are pinned to bf16x3 (conv3d.packed_linear),
    which splits the operands exactly and has no per-tensor scale
    (tests/test_ray_forward_gpu.py::test_radiance_mlp_at_inference_against_float64 asserts the arithmetic of every launch)."""
    r, s = pts.shape[:2]
    most = max(1, FINE_MLP_ROWS // s)          # rays a call may take
    if r <= most:
        return nerf_mlp(pts, ray_d, globalfeat)
    step = -(-r // -(-r // most))
    outs = [nerf_mlp(pts[i:i + step], ray_d[i:i + step], globalfeat[i:i + step]) for i in range(0, r, step)]
    return torch.cat([o[0] for o in outs], dim=0), torch.cat([o[1] for o in outs], dim=0)


# ------------------------------------------------------------------------------------------------------
# A11
# ------------------------------------------------------------------------------------------------------
def raw2outputs(raw, z_vals, mask, white_bkgd=False):
    """render_ray.py:196-247 -> OrderedDict(rgb, depth, weights, mask, alpha, z_vals, transparency).  Differentiable in
    ``raw`` (through rgb and depth) when it requires grad."""
    if torch.is_grad_enabled() and raw.requires_grad:
        from .autograd import Composite
        rgb, depth, wts, alpha, trans, rmask = Composite.apply(raw, z_vals, mask, white_bkgd)
        return OrderedDict([("rgb", rgb), ("depth", depth), ("weights", wts), ("mask", None if mask is None else rmask),
                            ("alpha", alpha), ("z_vals", z_vals), ("transparency", trans)])
    return _raw2outputs_impl(raw, z_vals, mask, white_bkgd)


def _raw2outputs_impl(raw, z_vals, mask, white_bkgd=False):
    if not raw.is_cuda:
        raise RuntimeError("nerfdet_amd.rays: tensors must live on the GPU (no CPU fallback)")
    r, s = raw.shape[:2]
    raw_c = raw.to(torch.float32).contiguous()
    z = z_vals.to(torch.float32).contiguous()
    dev = raw.device
    zmm = torch.stack([z.min(), z.max()])
    pm = None if mask is None else mask.to(torch.bool).contiguous()
    rgb = torch.empty((r, 3), dtype=torch.float32, device=dev)
    depth = torch.empty((r,), dtype=torch.float32, device=dev)
    wts = torch.empty((r, s), dtype=torch.float32, device=dev)
    alpha = torch.empty((r, s), dtype=torch.float32, device=dev)
    trans = torch.empty((r, s), dtype=torch.float32, device=dev)
    rmask = None if mask is None else torch.empty((r,), dtype=torch.bool, device=dev)
    check(_lib.load().ndet_composite(_ptr(raw_c), _ptr(z), _ptr(pm), r, s, int(bool(white_bkgd)), _ptr(zmm), _ptr(rgb), _ptr(depth),
                                     _ptr(wts), _ptr(rmask), _ptr(alpha), _ptr(trans), _stream(raw)), "raw2outputs")
    return OrderedDict([("rgb", rgb), ("depth", depth), ("weights", wts), ("mask", rmask), ("alpha", alpha),
                        ("z_vals", z_vals), ("transparency", trans)])


# ------------------------------------------------------------------------------------------------------
# A12
# ------------------------------------------------------------------------------------------------------
def render_rays_func(ray_o, ray_d, mean_volume, cov_volume, features_2D, img, aabb, near_far_range, N_samples, N_rand=4096,
                     nerf_mlp=None, img_meta=None, projector=None, mode="volume", nerf_sample_view=3, inv_uniform=False,
                     N_importance=0, det=False, is_train=True, white_bkgd=False, gt_rgb=None, gt_depth=None, t_rand=None):
    """render_ray.py:250-369, ``mode='image'``.  ``N_importance=0`` is the only branch the reference can reach.

    ``N_importance=k > 0`` is THIS PROJECT'S definition of the fine pass: the reference's branch (render_ray.py:329-367) names
    ``model``, ``ray_batch`` and ``featmaps``, which do not exist there, and cannot run.  Here the coarse weights (detached,
    render_ray.py:332) go through :func:`importance_merge` (render_ray.py:343-356), and the merged ``N_samples + k`` samples through the
    same sampler, the same ``nerf_mlp`` -- NeRF-Det has one MLP, there is no separate fine network -- and :func:`raw2outputs`;
    the result is ``ret['outputs_fine']``, ``outputs_coarse`` and ``sigma`` are the coarse pass's, unchanged.  The fine pass is
    inference only: with autograd on and ``features_2D.requires_grad`` it raises ValueError.  ``inv_uniform`` stays refused."""
    assert mode == "image", "nerf_mode='volume' is not used by any nerfdet config"
    assert N_importance >= 0
    training = torch.is_grad_enabled() and features_2D.requires_grad
    if N_importance > 0 and training:
        raise ValueError("render_rays_func: N_importance > 0 has no backward (the fine pass is inference only)")
    ret = {"outputs_coarse": None, "outputs_fine": None, "gt_rgb": gt_rgb, "gt_depth": gt_depth}
    pts, z_vals = sample_along_camera_ray(ray_o, ray_d, near_far_range, N_samples, inv_uniform=inv_uniform, det=det, t_rand=t_rand)
    cams = _compute_projection(img_meta)
    if training:
        from .autograd import RayViewStats
        globalfeat, pixel_mask, _ = RayViewStats.apply(features_2D, pts, img, cams)
    else:
        globalfeat, pixel_mask, _ = ray_view_stats(pts, img, cams, features_2D)
    rgb_pts, density_pts = nerf_mlp(pts, ray_d, globalfeat)
    ret["sigma"] = density_pts
    ret["outputs_coarse"] = raw2outputs(torch.cat([rgb_pts, density_pts], dim=-1), z_vals, pixel_mask, white_bkgd=white_bkgd)
    if N_importance > 0:
        weights = ret["outputs_coarse"]["weights"].detach()                                  # render_ray.py:332
        pts_f, z_f, _ = importance_merge(z_vals, weights, ray_o, ray_d, N_importance, det)   # render_ray.py:343-356
        globalfeat_f, pixel_mask_f, _ = ray_view_stats(pts_f, img, cams, features_2D)
        rgb_f, density_f = fine_mlp(nerf_mlp, pts_f, ray_d, globalfeat_f)
        ret["outputs_fine"] = raw2outputs(torch.cat([rgb_f, density_f], dim=-1), z_f, pixel_mask_f, white_bkgd=white_bkgd)
    return ret


RENDER_TESTING_RAYS = 8192     # rays per pass of the render_testing walk on the GPU (a multiple of N_rand is used)


def begin_selection(ray_batch):
    """First half of the training-time ray draw of render_ray.py:386-404: the rays WITH depth (``gt_depth > 0``; all rays when the scene has
    no depth maps), as indices into the flattened ray list, and their number.  Depends on the inputs only, so the detector takes it
    before it queues the backbone: the one host sync it needs then waits for nothing."""
    gt_depth = ray_batch["gt_depth"]
    rays = ray_batch["ray_d"].view(-1, 3)
    if len(gt_depth) == 0:
        return None, rays.shape[0], rays.device
    given = ray_batch.get("depth_rays")
    if given is not None and (given.dim() == 1 or given.shape[0] == 1):
        # found by the loader on the host, before the upload (datasets.py: DefaultFormatBundle3D; batches of one scene, config:133): the count is a
        # shape.  On the device the same ``nonzero`` reads its count back through a stream synchronisation -- with the step's log read lazily
        # (train.StepLog) the host would wait there for the whole previous step's backward.
        kept = given.reshape(-1)
        return kept, int(kept.numel()), rays.device
    kept = torch.nonzero(gt_depth.view(-1) > 0).view(-1)
    return kept, int(kept.numel()), rays.device


def _draw(n, n_rand):
    return rng.choice(n, size=(n_rand,), replace=False)


_DRAW_WORKER = None
THREADED_DRAW = False     # True: the permutation runs on a worker thread beside the backbone's launches.  Measured (tools/bench_train.py --threaded-draw,
                          # same box, alternating): no difference while the host runs ahead of the device (38.2 vs 38.3 ms per step), and 2 - 4 ms
                          # WORSE when it does not (host read every step: 47.0 - 49.8 vs 45.0 - 45.7 ms) -- the hand-over between the threads costs more
                          # than the 5 ms it hides behind launches that are themselves host-bound there


def submit_draw(begun, n_rand):
    """Start the host half of the ray draw on a worker thread: ``RandomState.choice(n, N_rand, replace=False)`` is a full Fisher-Yates shuffle of
    all n rays with depth (660 000 at the configs' sizes: ~5 ms) whatever N_rand is, and the reference's RNG stream (render_ray.py:20,398) leaves no
    way around it.  With THREADED_DRAW numpy shuffles on a worker (GIL released) while the backbone's launches go out -- ONE worker, submissions in
    call order: the module-global RandomState is consumed in the same order as by direct calls; by default the draw runs right here (see
    THREADED_DRAW for the measurement).  Returns a handle for :func:`collect_draw`."""
    global _DRAW_WORKER
    kept, n, dev = begun
    if not THREADED_DRAW:
        from concurrent.futures import Future
        done = Future()
        done.set_result(_draw(n, n_rand))
        return kept, dev, done
    if _DRAW_WORKER is None:
        from concurrent.futures import ThreadPoolExecutor
        _DRAW_WORKER = ThreadPoolExecutor(max_workers=1, thread_name_prefix="ndet-ray-draw")
    return kept, dev, _DRAW_WORKER.submit(_draw, n, n_rand)


def collect_draw(handle):
    """Second half of :func:`submit_draw`: wait for the draw, upload it (pinned staging), map it through the rays-with-depth indices."""
    kept, dev, fut = handle
    draw = torch.from_numpy(fut.result())
    if torch.device(dev).type == "cuda":
        from .ops import _upload_async
        draw = _upload_async(draw, dev)           # pinned staging: a pageable copy here would wait for the queued backbone to drain
    return draw if kept is None else kept[draw]


def finish_selection(begun, n_rand):
    """Second half: ``N_rand`` of those rays drawn without replacement from the module-global RandomState (the reference's stream and call,
    render_ray.py:20,398 -- a permutation of all kept rays on the host, milliseconds).  Returns indices into the flattened ray list (device
    tensor).  The detector uses :func:`submit_draw` / :func:`collect_draw` instead, which run the permutation beside the backbone's launches."""
    return collect_draw(submit_draw(begun, n_rand))


def render_rays(ray_batch, mean_volume, cov_volume, features_2D, img, aabb, near_far_range, N_samples, N_rand=4096, nerf_mlp=None,
                img_meta=None, projector=None, mode="volume", nerf_sample_view=3, inv_uniform=False, N_importance=0, det=False,
                is_train=True, white_bkgd=False, render_testing=False, selection=None):
    """render_ray.py:371-520: training = drop rays without depth, draw ``N_rand`` rays from the module-global
    RandomState, one ``render_rays_func``; ``render_testing`` = every ray of the target views in chunks of
    ``N_rand``, deterministic sampling; otherwise ``None``."""
    ray_o, ray_d, gt_rgb, gt_depth = ray_batch["ray_o"], ray_batch["ray_d"], ray_batch["gt_rgb"], ray_batch["gt_depth"]
    if is_train:
        ray_o, ray_d, gt_rgb = ray_o.view(-1, 3), ray_d.view(-1, 3), gt_rgb.view(-1, 3)
        gt_depth = gt_depth.view(-1, 1) if len(gt_depth) != 0 else None
        sel = selection if selection is not None else finish_selection(begin_selection(ray_batch), N_rand)
        ray_o, ray_d, gt_rgb = ray_o[sel], ray_d[sel], gt_rgb[sel]
        if gt_depth is not None:
            gt_depth = gt_depth[sel]
        return render_rays_func(ray_o, ray_d, mean_volume, cov_volume, features_2D, img, aabb, near_far_range, N_samples, N_rand,
                                nerf_mlp, img_meta, projector, mode, nerf_sample_view, inv_uniform, N_importance, det, is_train,
                                white_bkgd, gt_rgb, gt_depth)
    if render_testing:
        nerf_size = ray_batch["nerf_sizes"][0]
        view_num = ray_o.shape[1]
        hh, ww = int(nerf_size[0][0]), int(nerf_size[0][1])
        ray_o, ray_d, gt_rgb = ray_o.view(-1, 3), ray_d.view(-1, 3), gt_rgb.view(-1, 3)
        gt_depth = gt_depth.view(-1, 1) if len(gt_depth) != 0 else None
        assert view_num * hh * ww == ray_o.shape[0]  # render_ray.py:468
        rgbs, depths, rgbs_f, depths_f = [], [], [], []
        # the reference walks the rays N_rand at a time (render_ray.py:470); a ray's result does not depend on its chunk mates (deterministic
        # sampling, row-wise MLP), so on the GPU several of its chunks go through one pass: fewer, larger GEMMs
        step = N_rand * max(1, RENDER_TESTING_RAYS // N_rand) if ray_o.is_cuda else N_rand
        for i in range(0, ray_o.shape[0], step):
            ret = render_rays_func(ray_o[i:i + step], ray_d[i:i + step], mean_volume, cov_volume, features_2D, img, aabb,
                                   near_far_range, N_samples, N_rand, nerf_mlp, img_meta, projector, mode, nerf_sample_view,
                                   inv_uniform, N_importance, True, is_train, white_bkgd, gt_rgb, gt_depth)
            rgbs.append(ret["outputs_coarse"]["rgb"])
            depths.append(ret["outputs_coarse"]["depth"])
            if N_importance > 0:
                rgbs_f.append(ret["outputs_fine"]["rgb"])
                depths_f.append(ret["outputs_fine"]["depth"])
        out = {"outputs_coarse": {"rgb": torch.cat(rgbs, dim=0).view(view_num, hh, ww, 3),
                                  "depth": torch.cat(depths, dim=0).view(view_num, hh, ww, 1)},
               "gt_rgb": gt_rgb.view(view_num, hh, ww, 3),
               "gt_depth": gt_depth.view(view_num, hh, ww, 1) if gt_depth is not None else None}
        if N_importance > 0:             # this project's fine pass (render_rays_func), stacked like the coarse one
            out["outputs_fine"] = {"rgb": torch.cat(rgbs_f, dim=0).view(view_num, hh, ww, 3),
                                   "depth": torch.cat(depths_f, dim=0).view(view_num, hh, ww, 1)}
        return out
    return None


def compute_psnr(pred: Tensor, target: Tensor, mask: Optional[Tensor] = None) -> Tensor:
    """PSNR of a rendered view against its ground truth, maximum pixel value 1: ``-10 log10(mean((pred - target)^2))``
    (model_utils/save_rendered_img.py:10-19)."""
    if mask is not None:
        pred, target = pred[mask], target[mask]
    return -10.0 * torch.log(((pred - target) ** 2).mean()) / float(np.log(10.0))


def compute_ssim(pred: Tensor, target: Tensor) -> Tensor:
    """SSIM of a rendered (H,W,3) view as the reference's ``compute_ssim`` obtains it (model_utils/save_rendered_img.py:21-36 ->
    ``skimage.metrics.structural_similarity(..., multichannel=True)`` of the pinned scikit-image 0.18.1): per channel, 7 x 7 uniform
    window, sample covariance, K1 = 0.01, K2 = 0.03, data range 2 (float images), float64, mean over the window-valid interior, then over
    the channels.  The 49-pixel box means are one average pooling each, on the device."""
    assert pred.shape == target.shape and pred.dim() == 3 and pred.shape[-1] == 3 and min(pred.shape[:2]) >= 7
    x, y = pred.permute(2, 0, 1).unsqueeze(0).double(), target.permute(2, 0, 1).unsqueeze(0).double()
    box = lambda t: torch.nn.functional.avg_pool2d(t, 7, stride=1)
    ux, uy, uxx, uyy, uxy = box(x), box(y), box(x * x), box(y * y), box(x * y)
    norm = 49.0 / 48.0
    vx, vy, vxy = norm * (uxx - ux * ux), norm * (uyy - uy * uy), norm * (uxy - ux * uy)
    c1, c2 = (0.01 * 2.0) ** 2, (0.03 * 2.0) ** 2
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
    return s.mean(dim=(2, 3)).mean()


def ssim_views(pred: Tensor, target: Tensor) -> Tensor:
    """:func:`compute_ssim` of n views at once: ``pred``, ``target`` (n,H,W,3) float32 on the device -> (n,) float64, from ONE launch of the
    fused window kernel (pipeline.frame_ssim's float form: float64 box sums in a fixed order, the per-window values summed as integers
    of 2^-40, so the same bytes on every call).  Agrees with :func:`compute_ssim` per view to 1e-10."""
    from .pipeline import frame_ssim
    if not isinstance(pred, Tensor) or not isinstance(target, Tensor) or pred.dtype != torch.float32 or target.dtype != torch.float32:
        raise ValueError("ssim_views takes two float32 (n, H, W, 3) tensors")
    return frame_ssim(pred.contiguous(), target.contiguous())["ssim"]


def rendering_metrics(rendered: dict, which: str = "outputs_coarse", fused: bool = False):
    """What ``save_rendered_img`` returns (model_utils/save_rendered_img.py:38-78) for one ``render_rays(render_testing=True)`` result,
    without its PNG dump: mean PSNR and mean SSIM over the target views (device scalars) and the mean squared depth error MAP
    (H,W,1) the reference calls rmse (None without depth maps).  ``which``: ``'outputs_coarse'`` (the reference's) or
    ``'outputs_fine'`` of a render with ``N_importance > 0``.  ``fused=True``: the SSIM of all the views from one :func:`ssim_views`
    launch in place of :func:`compute_ssim` view by view (within 1e-10 of it); PSNR and the depth error are the same code either way."""
    rgb, gt = rendered[which]["rgb"], rendered["gt_rgb"]
    depth, gt_depth = rendered[which]["depth"], rendered["gt_depth"]
    n = gt.shape[0]
    psnr = torch.stack([compute_psnr(rgb[v], gt[v]) for v in range(n)]).mean()
    if fused:
        ssim = ssim_views(rgb, gt).mean()
    else:
        ssim = torch.stack([compute_ssim(rgb[v], gt[v]) for v in range(n)]).mean()
    err = None if gt_depth is None else ((depth - gt_depth) ** 2).mean(dim=0)
    return psnr, ssim, err

