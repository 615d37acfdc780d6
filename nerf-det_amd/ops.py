"""Host-side mirror of the reference's module-level hot-path callables,
bodies routed to libnerfdet_hip.so through the C ABI.  PyTorch is used for device memory and
streams only; every function here requires CUDA(HIP) tensors and raises otherwise.

Reference signatures kept: ``get_points``, ``backproject`` (mmdet3d/models/detectors/nerfdet.py:380-420, with or without the depth
gate of :405-411).
Fused forms that have no single reference counterpart (``backproject_aggregate``, ``density_features``)
document the reference lines they replace.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, trace
from .hostmath import matmul_fma_chain
from ._lib import NDET_LAYOUT_CN, NDET_LAYOUT_NC, NdetDepthGate, NdetSceneAccum, _ptr, _stream, check, float3

Tensor = torch.Tensor


def _need_gpu(*ts: Tensor):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("nerfdet_amd.ops: tensors must live on the GPU (no CPU fallback in the product path)")


def _f32c(t: Tensor) -> Tensor:
    return t.to(torch.float32).contiguous()


# --------------------------------------------------------------------------------------------
# A1
# --------------------------------------------------------------------------------------------
_STAGING = {}   # (shape, dtype, device) -> [ring of pinned buffers, next slot]


def _upload_async(host: Tensor, device) -> Tensor:
    """H2D copy that does not stall the host: through a small ring of pinned staging buffers allocated once (a pageable
    copy waits for the stream to drain -- ~200 queued backbone launches at this point of the step; pinning per call costs
    more than the stall)."""
    key = (tuple(host.shape), host.dtype, str(device))
    ring = _STAGING.get(key)
    if ring is None:
        ring = _STAGING[key] = [[[torch.empty(host.shape, dtype=host.dtype).pin_memory(), None] for _ in range(8)], 0]
    slot = ring[0][ring[1]]
    ring[1] = (ring[1] + 1) % len(ring[0])
    if slot[1] is not None:
        slot[1].synchronize()   # the copy that last read this slot (8 uploads ago) must have left the host buffer
    slot[0].copy_(host)
    out = slot[0].to(device, non_blocking=True)
    slot[1] = torch.cuda.Event()
    slot[1].record(torch.cuda.current_stream(out.device))
    return out


def compute_projection(img_meta: dict, stride: int, device=None) -> Tensor:
    """(n_views,3,4) pixel projections ``K' @ E[:3]`` (nerfdet.py:363-378, angles=None).

    50 3x4 matrices: built on the host in the fp32 op order the reference's BLAS call has in the build container (hostmath.py: the
    result does not depend on the host's library or thread pool), one asynchronous H2D copy."""
    k = torch.tensor(np.asarray(img_meta["lidar2img"]["intrinsic"], dtype=np.float32)[:3, :3])
    k[:2] /= img_meta["ori_shape"][0] / (img_meta["img_shape"][0] / stride)
    ext = np.stack([np.asarray(e, dtype=np.float32)[:3] for e in img_meta["lidar2img"]["extrinsic"]])
    proj = torch.from_numpy(matmul_fma_chain(k.numpy()[None], ext))
    if device is None:
        return proj
    return _upload_async(proj, device) if torch.device(device).type == "cuda" else proj.to(device)


# --------------------------------------------------------------------------------------------
# A2
# --------------------------------------------------------------------------------------------
def get_points(n_voxels, voxel_size, origin, device=None) -> Tensor:
    """Voxel lower-corner lattice (3,X,Y,Z) fp32 on the GPU.  nerfdet.py:380-390."""
    nv = [int(v) for v in (n_voxels.tolist() if isinstance(n_voxels, Tensor) else n_voxels)]
    vs = [float(v) for v in (voxel_size.tolist() if isinstance(voxel_size, Tensor) else voxel_size)]
    org = origin.tolist() if isinstance(origin, (Tensor, np.ndarray)) else list(origin)
    assert len(nv) == 3 and len(vs) == 3 and len(org) == 3
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise RuntimeError("nerfdet_amd.ops.get_points: device must be a GPU")
    pts = torch.empty((3, nv[0], nv[1], nv[2]), dtype=torch.float32, device=dev)
    check(_lib.load().ndet_get_points(_ptr(pts), nv[0], nv[1], nv[2], float3(np.float32(vs)), float3(np.float32(org)),
                                      _stream(pts)), "get_points")
    return pts


# --------------------------------------------------------------------------------------------
# layout
# --------------------------------------------------------------------------------------------
def to_channels_last(x: Tensor) -> Tensor:
    """(n,C,h,w) logical tensor -> same logical tensor whose memory is (n,h,w,C) (torch channels_last).

    A tensor that already has unit channel stride and x-stride == C is returned as is (also when it is
    an [:h,:w] crop of a larger channels-last map); a contiguous NCHW one goes through the HIP transpose."""
    _need_gpu(x)
    n, c, h, w = x.shape
    if x.dtype == torch.float32 and x.stride(1) == 1 and x.stride(3) == c and x.stride(2) % 4 == 0 and x.stride(0) % 4 == 0 \
            and x.data_ptr() % 16 == 0:
        return x
    if x.dtype == torch.float32 and x.is_contiguous():
        out = torch.empty((n, h, w, c), dtype=torch.float32, device=x.device)
        check(_lib.load().ndet_nchw_to_nhwc(_ptr(x), _ptr(out), n, c, h * w, _stream(x)), "nchw_to_nhwc")
        return out.permute(0, 3, 1, 2)
    return to_channels_last(_f32c(x))


# --------------------------------------------------------------------------------------------
# depth gate (RGB-D scenes): nerfdet.py:404-411
# --------------------------------------------------------------------------------------------
_DEPTH_DTYPES = {torch.float32: 0, torch.float64: 1}


def depth_resize(depth: Tensor, feat_hw, img_hw=None) -> Tuple[Tensor, Optional[Tensor]]:
    """``F.interpolate(depth.unsqueeze(1), size, mode="bilinear")`` (nerfdet.py:405) to the feature map's ``feat_hw`` and, with
    ``img_hw``, to the image's as well -- both in one launch, in the depth map's own dtype (float32 or float64).
    ``depth`` (n_v, Hd, Wd) on the GPU.  Returns ``(D_f (n_v,h,w), D_r (n_v,H,W) or None)``, contiguous."""
    _need_gpu(depth)
    assert depth.dim() == 3, f"depth must be (n_views, H, W), got {tuple(depth.shape)}"
    if depth.dtype not in _DEPTH_DTYPES:
        raise ValueError(f"depth maps are float32 or float64, got {depth.dtype}")
    if depth.stride(2) != 1:
        depth = depth.contiguous()
    n_v, hd, wd = depth.shape
    h, w = int(feat_hw[0]), int(feat_hw[1])
    out_f = torch.empty((n_v, h, w), dtype=depth.dtype, device=depth.device)
    out_r = None
    hh = ww = 0
    if img_hw is not None:
        hh, ww = int(img_hw[0]), int(img_hw[1])
        out_r = torch.empty((n_v, hh, ww), dtype=depth.dtype, device=depth.device)
    trace.span("k_depth_resize", lambda: check(
        _lib.load().ndet_depth_resize(_ptr(depth), _DEPTH_DTYPES[depth.dtype], n_v, hd, wd, depth.stride(0), depth.stride(1), _ptr(out_f), h, w,
                                      _ptr(out_r), hh, ww, _stream(depth)), "depth_resize"),
        bytes=depth.element_size() * (n_v * hd * wd + out_f.numel() + (0 if out_r is None else out_r.numel())), kind="hbm")
    return out_f, out_r


class DepthGate:
    """One scene's depth gate (nerfdet.py:404-411): the depth map resized to the feature map (``depth_f``) and, for the density features'
    stride-1 projection, to the image (``depth_r``), plus ``band`` = voxel_size[2].  A view sees a voxel only where its camera depth z
    satisfies ``D' - band < z < D' + band``.  Built by :func:`depth_gate`; passed to the ``depth_gate=`` argument of the ops."""

    def __init__(self, depth_f: Tensor, depth_r: Optional[Tensor], band: float):
        assert math.isfinite(band) and band > 0, f"the depth band (voxel_size[2]) must be finite and > 0, got {band}"
        self.depth_f, self.depth_r, self.band = depth_f, depth_r, float(band)

    @property
    def n_views(self) -> int:
        return self.depth_f.shape[0]

    def block(self) -> NdetDepthGate:
        """The C ABI's NdetDepthGate for this gate (the tensors stay owned by ``self``)."""
        f, r = self.depth_f, self.depth_r
        g = NdetDepthGate()
        g.size = ctypes.sizeof(NdetDepthGate)
        g.dtype = _DEPTH_DTYPES[f.dtype]
        g.n_views, g.h, g.w = f.shape[0], f.shape[1], f.shape[2]
        g.depth_f, g.f_view_pitch, g.f_row_pitch = f.data_ptr(), f.stride(0), f.stride(1)
        if r is not None:
            g.H, g.W = r.shape[1], r.shape[2]
            g.depth_r, g.r_view_pitch, g.r_row_pitch = r.data_ptr(), r.stride(0), r.stride(1)
        g.band = self.band
        return g


def depth_gate(depth: Tensor, voxel_size, feat_hw, img_hw=None) -> DepthGate:
    """The :class:`DepthGate` of ``depth`` (n_v, Hd, Wd) for a (h, w) feature map [and an (H, W) image]: one resize launch."""
    assert voxel_size is not None, "the depth gate needs voxel_size (its band is voxel_size[2], nerfdet.py:408)"
    vs = voxel_size.tolist() if isinstance(voxel_size, Tensor) else list(voxel_size)
    d_f, d_r = depth_resize(depth, feat_hw, img_hw)
    return DepthGate(d_f, d_r, float(vs[-1]))


def _gate_arg(gate: Optional[DepthGate], n_v: int, hw, img_hw=None):
    if gate is None:
        return None
    assert gate.n_views == n_v and tuple(gate.depth_f.shape[1:]) == tuple(hw), \
        f"depth gate for {tuple(gate.depth_f.shape)}, map is {(n_v,) + tuple(hw)}"
    if img_hw is not None:
        assert gate.depth_r is not None and tuple(gate.depth_r.shape[1:]) == tuple(img_hw), "depth gate has no map at the image's size"
    return ctypes.byref(gate.block())


# --------------------------------------------------------------------------------------------
# A3 exact form
# --------------------------------------------------------------------------------------------
def backproject(features: Tensor, points: Tensor, projection: Tensor, depth=None, voxel_size=None) -> Tuple[Tensor, Tensor]:
    """Reference API: (n_v,C,h,w),(3,X,Y,Z),(n_v,3,4) -> volume (n_v,C,X,Y,Z), valid (n_v,1,X,Y,Z) bool.
    nerfdet.py:393-420.  Materialises the per-view volume exactly like the reference; the inference
    path uses :func:`backproject_aggregate` instead.  With ``depth`` (n_v,Hd,Wd) float32/float64 and ``voxel_size``, a view
    sees a voxel only within voxel_size[2] of the observed surface (nerfdet.py:404-411): the map is resized to (h, w) in its
    own dtype and the band test runs in that dtype, as PyTorch evaluates the reference's expression."""
    if depth is not None:
        assert isinstance(depth, Tensor) and depth.dim() == 3 and depth.shape[0] == features.shape[0], \
            "depth must be (n_views, H, W) (nerfdet.py:405)"
        assert voxel_size is not None, "depth-gated backproject needs voxel_size (nerfdet.py:408)"
    _need_gpu(features, points, projection, depth)
    if features.dtype != torch.float32:
        features = features.float()
    n_v, c, h, w = features.shape
    gx, gy, gz = points.shape[-3:]
    n = gx * gy * gz
    points = _f32c(points)
    projection = _f32c(projection)
    assert projection.shape == (n_v, 3, 4)
    volume = torch.empty((n_v, c, gx, gy, gz), dtype=torch.float32, device=features.device)
    valid = torch.empty((n_v, 1, gx, gy, gz), dtype=torch.bool, device=features.device)
    sv, sc, sy, sx = features.stride()
    if depth is None:
        check(_lib.load().ndet_backproject(_ptr(features), n_v, c, h, w, sv, sc, sy, sx, _ptr(points), n, _ptr(projection),
                                           _ptr(volume), _ptr(valid), _stream(features)), "backproject")
    else:
        gate = depth_gate(depth, voxel_size, (h, w))
        check(_lib.load().ndet_backproject_gated(_ptr(features), n_v, c, h, w, sv, sc, sy, sx, _ptr(points), n, _ptr(projection),
                                                 _ptr(volume), _ptr(valid), _gate_arg(gate, n_v, (h, w)), _stream(features)), "backproject_gated")
    return volume, valid


# --------------------------------------------------------------------------------------------
# K1: A3 + A4 (+ A6 gating)
# --------------------------------------------------------------------------------------------
def backproject_aggregate(features: Tensor, points: Tensor, projection: Tensor, alpha: Optional[Tensor] = None,
                          channels_last_out: bool = True, out: Optional[Tuple[Tensor, Tensor]] = None,
                          depth_gate: Optional[DepthGate] = None) -> Tuple[Tensor, Tensor]:
    """Fused ``backproject`` + view mean/count of nerfdet.py:164-176 (and, with ``alpha``, the gating of
    nerfdet.py:259-261): returns ``(volume (C,X,Y,Z), count (1,X,Y,Z) int64)``.  With ``depth_gate`` (:func:`depth_gate` at the
    features' h x w) only views whose observed depth lies within the band count (nerfdet.py:404-411).

    ``features`` is the logical (n_v,C,h,w) map, ideally channels-last in memory.  With
    ``channels_last_out`` the result's memory is (X,Y,Z,C) -- what a channels-last 3D conv wants -- while
    its logical shape stays the reference's (C,X,Y,Z)."""
    _need_gpu(features, points, projection, alpha)
    f = to_channels_last(features)
    n_v, c, h, w = f.shape
    gx, gy, gz = points.shape[-3:]
    n = gx * gy * gz
    points = _f32c(points)
    projection = _f32c(projection)
    assert projection.shape == (n_v, 3, 4)
    if alpha is not None:
        alpha = _f32c(alpha).reshape(-1)
        assert alpha.numel() == n
    if out is not None:  # caller-owned result buffers (static buffers of a hipGraph pipeline)
        vol, count = out
        buf = vol.permute(1, 2, 3, 0) if channels_last_out else vol
        assert buf.is_contiguous() and buf.dtype == torch.float32 and vol.shape == (c, gx, gy, gz)
        assert count.shape == (1, gx, gy, gz) and count.dtype == torch.int64 and count.is_contiguous()
        out, layout = vol, (NDET_LAYOUT_NC if channels_last_out else NDET_LAYOUT_CN)
        from .conv3d import note_raw_write
        note_raw_write(vol)     # written through its raw pointer: any max |x| slot tagged on a tensor over this storage is stale from here on
    else:
        count = torch.empty((1, gx, gy, gz), dtype=torch.int64, device=f.device)
        if channels_last_out:
            buf = torch.empty((gx, gy, gz, c), dtype=torch.float32, device=f.device)
            out, layout = buf.permute(3, 0, 1, 2), NDET_LAYOUT_NC
        else:
            buf = torch.empty((c, gx, gy, gz), dtype=torch.float32, device=f.device)
            out, layout = buf, NDET_LAYOUT_CN
    # algorithmic bytes: every feature row once + (C fp32 + int64 count) per voxel
    lib = _lib.load()
    if depth_gate is None:
        launch = lambda: check(lib.ndet_backproject_aggregate(_ptr(f), n_v, c, h, w, f.stride(0), f.stride(2), _ptr(points), n, _ptr(projection),
                                                              _ptr(alpha), _ptr(buf), layout, _ptr(count), _stream(f)), "backproject_aggregate")
    else:
        g = _gate_arg(depth_gate, n_v, (h, w))
        launch = lambda: check(lib.ndet_backproject_aggregate_gated(_ptr(f), n_v, c, h, w, f.stride(0), f.stride(2), _ptr(points), n,
                                                                    _ptr(projection), _ptr(alpha), _ptr(buf), layout, _ptr(count), g, _stream(f)),
                               "backproject_aggregate_gated")
    trace.span("k_backproject_aggregate", launch, bytes=4 * n_v * c * h * w + (4 * c + 8) * n, kind="hbm")
    return out, count


# --------------------------------------------------------------------------------------------
# K2: A5
# --------------------------------------------------------------------------------------------
def density_packed_ok(n_views: int, cm: int, mapped: Optional[Tensor] = None, bias: Optional[Tensor] = None) -> bool:
    """Shapes the packed K2 kernel (csrc/density_kernels.hip) takes; everything else runs on the generic kernel."""
    if cm % 4 or cm > 128 or n_views > 128:
        return False
    if mapped is not None and (mapped.stride(0) % 4 or mapped.stride(2) % 4 or mapped.data_ptr() % 16):
        return False
    return bias is None or bias.data_ptr() % 16 == 0


def density_features(mapped: Tensor, bias: Tensor, denorm_images: Tensor, points: Tensor, projection: Tensor,
                     rgb_projection: Tensor, depth_gate: Optional[DepthGate] = None) -> Tensor:
    """(N, 2*(3+cm)) NeRF conditioning rows for the voxel grid; replaces nerfdet.py:234-253.
    With ``depth_gate`` (maps at the features' h x w and the images' H x W) both projections are depth-gated (nerfdet.py:404-411).

    ``mapped``: logical (n_v,cm,h,w) = Linear(C->cm) of the feature map (``feature_2d`` of nerfdet.py:194-197),
    ``bias`` its bias (contributed by views that do not see a voxel), ``denorm_images`` (n_v,3,H,W)."""
    _need_gpu(mapped, bias, denorm_images, points, projection, rgb_projection)
    m = to_channels_last(mapped)
    n_v, cm, h, w = m.shape
    rgb = denorm_images if denorm_images.dtype == torch.float32 else denorm_images.float()
    assert rgb.shape[0] == n_v and rgb.shape[1] == 3
    if rgb.stride(3) != 1:
        rgb = rgb.contiguous()
    hh, ww = rgb.shape[2:]
    n = points.shape[-3] * points.shape[-2] * points.shape[-1]
    points, projection, rgb_projection, bias = _f32c(points), _f32c(projection), _f32c(rgb_projection), _f32c(bias)
    out = torch.empty((n, 2 * (3 + cm)), dtype=torch.float32, device=m.device)
    # algorithmic bytes: images + mapped map read once, 2*(3+cm) floats written per voxel
    lib = _lib.load()
    packed = density_packed_ok(n_v, cm, m, bias)
    args = (_ptr(m), n_v, cm, h, w, m.stride(0), m.stride(2), _ptr(bias), _ptr(rgb), hh, ww, rgb.stride(0), rgb.stride(1), rgb.stride(2),
            _ptr(points), n, _ptr(projection), _ptr(rgb_projection), _ptr(out))
    if depth_gate is None:
        fn = lib.ndet_density_features_packed if packed else lib.ndet_density_features
        launch = lambda: check(fn(*args, _stream(m)), "density_features")
    else:
        fn = lib.ndet_density_features_packed_gated if packed else lib.ndet_density_features_gated
        g = _gate_arg(depth_gate, n_v, (h, w), (hh, ww))
        launch = lambda: check(fn(*args, g, _stream(m)), "density_features_gated")
    trace.span("k_density_features", launch, bytes=4 * (n_v * 3 * hh * ww + n_v * cm * h * w + 2 * (3 + cm) * n), kind="hbm")
    return out


# --------------------------------------------------------------------------------------------
# Streaming scenes: K1 and K2 split into accumulate / finish (include/nerfdet_hip.h, NdetSceneAccum)
# --------------------------------------------------------------------------------------------
class SceneState:
    """One scene's running sums on the device, views added chunk by chunk (:func:`scene_accumulate`) and finished at any time
    (:func:`density_finish`, :func:`volume_finish`).  Per voxel: K1's C-float feature-row sum and view count, K2's three sums of the 3 + cm
    channels (sum v, sum (v - fill)^2, sum (v - fill), quad-padded rows) and its two view counts -- 4 C + 12 (cm + 4) + 12 bytes."""

    def __init__(self, n_voxels, c: int, cm: int, device):
        self.grid = tuple(int(v) for v in n_voxels)
        n = self.grid[0] * self.grid[1] * self.grid[2]
        assert c % 4 == 0 and cm % 4 == 0, f"streaming needs C and cm in multiples of 4 (got {c}, {cm})"
        self.c, self.cm, self.n_views = int(c), int(cm), 0
        self.k1_sum = torch.zeros((n, c), dtype=torch.float32, device=device)
        self.k1_count = torch.zeros((n,), dtype=torch.int32, device=device)
        self.k2_sum = torch.zeros((n, 3 * (cm + 4)), dtype=torch.float32, device=device)
        self.k2_count = torch.zeros((n, 2), dtype=torch.int32, device=device)

    @property
    def n_voxels(self) -> int:
        return self.k1_sum.shape[0]

    def reset(self) -> None:
        for t in (self.k1_sum, self.k1_count, self.k2_sum, self.k2_count):
            t.zero_()
        self.n_views = 0

    def block(self) -> NdetSceneAccum:
        """The C ABI's NdetSceneAccum for this state (the tensors stay owned by ``self``)."""
        b = NdetSceneAccum()
        b.size = ctypes.sizeof(NdetSceneAccum)
        b.N, b.C, b.cm, b.n_views = self.n_voxels, self.c, self.cm, self.n_views
        b.k1_sum, b.k1_pitch, b.k1_count = self.k1_sum.data_ptr(), self.k1_sum.stride(0), self.k1_count.data_ptr()
        b.k2_sum, b.k2_pitch, b.k2_count = self.k2_sum.data_ptr(), self.k2_sum.stride(0), self.k2_count.data_ptr()
        return b


def _chunk_args(features: Tensor, mapped: Tensor, bias: Tensor, denorm_images: Tensor, projection: Tensor, rgb_projection: Tensor,
                depth_gate: Optional[DepthGate], c: int, cm: int):
    """A chunk's arguments as the accumulate entry points take them, for a state of ``c`` and ``cm`` channels: ``(features, mapped`` (both
    channels-last), ``bias, images`` (float32, unit pixel stride), ``projection, rgb_projection`` (float32, contiguous), ``n_v, h, w, H, W,``
    the gate block or None, the bytes the launch reads of the chunk)``."""
    _need_gpu(features, mapped, bias, denorm_images, projection, rgb_projection)
    f = to_channels_last(features)
    m = to_channels_last(mapped)
    n_v, h, w = f.shape[0], f.shape[2], f.shape[3]
    assert m.shape[0] == n_v and m.shape[2:] == f.shape[2:], f"mapped map {tuple(m.shape)} for features {tuple(f.shape)}"
    assert (f.shape[1], m.shape[1]) == (c, cm), f"state for C={c}, cm={cm}; chunk has {f.shape[1]}, {m.shape[1]}"
    if not density_packed_ok(0, cm, m):       # the packed walk's channel quads need 16-byte aligned rows
        m = to_channels_last(m.contiguous())
    rgb = denorm_images if denorm_images.dtype == torch.float32 else denorm_images.float()
    assert rgb.shape[0] == n_v and rgb.shape[1] == 3
    if rgb.stride(3) != 1:
        rgb = rgb.contiguous()
    hh, ww = rgb.shape[2:]
    projection, rgb_projection, bias = _f32c(projection), _f32c(rgb_projection), _f32c(bias)
    assert projection.shape == (n_v, 3, 4) and rgb_projection.shape == (n_v, 3, 4)
    g = _gate_arg(depth_gate, n_v, (h, w), (hh, ww))
    return f, m, bias, rgb, projection, rgb_projection, n_v, h, w, hh, ww, g, 4 * (n_v * (c * h * w + cm * h * w + 3 * hh * ww))


def scene_accumulate(state: SceneState, features: Tensor, mapped: Tensor, bias: Tensor, denorm_images: Tensor, points: Tensor,
                     projection: Tensor, rgb_projection: Tensor, depth_gate: Optional[DepthGate] = None) -> None:
    """Add one chunk of k views to ``state``: K1's view sum and count of nerfdet.py:164-176 and K2's sums of nerfdet.py:234-253, both without
    their finish.  Arguments as :func:`backproject_aggregate` (``features`` (k,C,h,w)) and :func:`density_features` (``mapped`` (k,cm,h,w),
    ``bias``, ``denorm_images`` (k,3,H,W)) for the chunk's views; ``depth_gate`` for the chunk's views (nerfdet.py:404-411).  K1's sums hold
    the same bits whatever the chunking; K2 runs in launches of at most 128 views."""
    _need_gpu(points)
    f, m, bias, rgb, projection, rgb_projection, n_v, h, w, hh, ww, g, read = _chunk_args(
        features, mapped, bias, denorm_images, projection, rgb_projection, depth_gate, state.c, state.cm)
    assert points.shape[-3:] == state.grid, f"points {tuple(points.shape)} for a {state.grid} state"
    points = _f32c(points)
    blk = state.block()
    trace.span("k_scene_accumulate", lambda: check(_lib.load().ndet_scene_accumulate(
        ctypes.byref(blk), _ptr(f), n_v, h, w, f.stride(0), f.stride(2), _ptr(m), m.stride(0), m.stride(2), _ptr(bias), _ptr(rgb), hh, ww,
        rgb.stride(0), rgb.stride(1), rgb.stride(2), _ptr(points), _ptr(projection), _ptr(rgb_projection), g, _stream(f)), "scene_accumulate"),
        bytes=read + 2 * (state.k1_sum.numel() + state.k2_sum.numel()) * 4, kind="hbm")
    state.n_views += n_v


def _density_out(bias: Tensor, cm: int, rows: int, device):
    """What every density finish starts from: the bias checked against ``cm`` and the ``(rows, 2*(3+cm))`` output."""
    bias = _f32c(bias)
    assert bias.numel() == cm
    return bias, torch.empty((rows, 2 * (3 + cm)), dtype=torch.float32, device=device)


def _volume_out(alpha: Optional[Tensor], n: int, grid, c: int, device):
    """What every volume finish starts from, for n scenes: ``alpha`` flattened and checked (or None), the ``(n,X,Y,Z,C)`` volume buffer and
    the ``(n,1,X,Y,Z)`` int64 count.  A single-scene finish returns their row 0."""
    gx, gy, gz = grid
    if alpha is not None:
        alpha = _f32c(alpha).reshape(-1)
        assert alpha.numel() == n * gx * gy * gz
    return (alpha, torch.empty((n, gx, gy, gz, c), dtype=torch.float32, device=device),
            torch.empty((n, 1, gx, gy, gz), dtype=torch.int64, device=device))


def density_finish(state: SceneState, bias: Tensor) -> Tensor:
    """(N, 2*(3+cm)) conditioning rows over every view in ``state`` (nerfdet.py:234-253), the packed K2's finish; ``state`` is not changed.
    A state filled by one chunk of at most 128 views gives :func:`density_features`'s rows bit for bit."""
    _need_gpu(bias)
    assert state.n_views > 0, "the scene has no views yet"
    bias, out = _density_out(bias, state.cm, state.n_voxels, state.k1_sum.device)
    blk = state.block()
    trace.span("k_density_finish", lambda: check(_lib.load().ndet_scene_density_finish(ctypes.byref(blk), _ptr(bias), _ptr(out), _stream(out)),
                                                 "scene_density_finish"), bytes=4 * (state.k2_sum.numel() + out.numel()), kind="hbm")
    return out


def volume_finish(state: SceneState, alpha: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """K1's epilogue over ``state`` (nerfdet.py:175-176 and, with ``alpha``, 259-261): ``(volume (C,X,Y,Z) with (X,Y,Z,C) memory, count
    (1,X,Y,Z) int64)``, bit for bit what :func:`backproject_aggregate` returns over all the state's views; ``state`` is not changed."""
    _need_gpu(alpha)
    alpha, buf, count = _volume_out(alpha, 1, state.grid, state.c, state.k1_sum.device)
    blk = state.block()
    trace.span("k_volume_finish", lambda: check(_lib.load().ndet_scene_volume_finish(ctypes.byref(blk), _ptr(alpha), _ptr(buf), _ptr(count),
                                                                                     _stream(buf)), "scene_volume_finish"),
               bytes=8 * state.k1_sum.numel() + 12 * state.n_voxels, kind="hbm")
    return buf[0].permute(3, 0, 1, 2), count[0]


RING_MAX = 64   # segments one ring finish reads (include/nerfdet_hip.h)


def _ring_blocks(states: Sequence[SceneState]):
    """The host array of NdetSceneAccum blocks the ring finishes take, oldest first."""
    states = list(states)
    assert 1 <= len(states) <= RING_MAX, f"a ring holds 1 to {RING_MAX} states, got {len(states)}"
    s0 = states[0]
    for s in states[1:]:
        assert (s.grid, s.c, s.cm) == (s0.grid, s0.c, s0.cm), "the ring's states must share grid, C and cm"
        assert s.k1_sum.device == s0.k1_sum.device
    assert sum(s.n_views for s in states) > 0, "the scene has no views yet"
    arr = (NdetSceneAccum * len(states))()
    for i, s in enumerate(states):
        arr[i] = s.block()
    return states, arr


def density_finish_ring(states: Sequence[SceneState], bias: Tensor) -> Tensor:
    """:func:`density_finish` over several states at once (oldest first, at most 64): per voxel the states' K2 sums and counts are added in
    that order, then finished over the states' total view count.  One state gives :func:`density_finish`'s rows bit for bit; no state is
    changed.  The span's bytes count every state in full: an upper bound, the kernel skips a state's row where its count is 0 (knowing
    how many would cost a device-to-host read per call; tools/time_streaming.py --window counts them)."""
    _need_gpu(bias)
    states, arr = _ring_blocks(states)
    s0 = states[0]
    bias, out = _density_out(bias, s0.cm, s0.n_voxels, s0.k1_sum.device)
    read = sum(s.k2_sum.numel() + s.k2_count.numel() for s in states)
    trace.span("k_density_finish_ring", lambda: check(_lib.load().ndet_scene_density_finish_ring(arr, len(states), _ptr(bias), _ptr(out),
                                                                                                _stream(out)), "scene_density_finish_ring"),
               bytes=4 * (read + out.numel()), kind="hbm")
    return out


def volume_finish_ring(states: Sequence[SceneState], alpha: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """:func:`volume_finish` over several states at once (oldest first, at most 64): per voxel the states' K1 sums and counts are added in
    that order, then divided and gated.  One state gives :func:`volume_finish`'s outputs bit for bit; no state is changed.  The span's bytes count every
    state in full, an upper bound as in :func:`density_finish_ring`."""
    _need_gpu(alpha)
    states, arr = _ring_blocks(states)
    s0 = states[0]
    alpha, buf, count = _volume_out(alpha, 1, s0.grid, s0.c, s0.k1_sum.device)
    read = sum(s.k1_sum.numel() + s.k1_count.numel() for s in states)
    trace.span("k_volume_finish_ring", lambda: check(_lib.load().ndet_scene_volume_finish_ring(arr, len(states), _ptr(alpha), _ptr(buf),
                                                                                              _ptr(count), _stream(buf)),
                                                    "scene_volume_finish_ring"),
               bytes=4 * (read + buf.numel()) + (12 if alpha is not None else 8) * s0.n_voxels, kind="hbm")
    return buf[0].permute(3, 0, 1, 2), count[0]


# --------------------------------------------------------------------------------------------
# Scene groups: many scenes' states behind one device table, accumulated and finished by grouped launches
# (include/nerfdet_hip.h, NdetSceneSlot / NdetSceneGroup / NdetGroupSel)
# --------------------------------------------------------------------------------------------
GROUP_MAX = 64        # scenes of one group (include/nerfdet_hip.h, NDET_GROUP_MAX)
GROUP_VIEWS_MAX = 128  # views one scene brings to one grouped accumulate (one packed K2 launch)


def listed_scenes(n_scenes: int, scenes) -> list:
    """``scenes`` of a grouped call over ``n_scenes`` scenes -- None: all of them, in order -- as a list of distinct indices (else ValueError)."""
    if scenes is None:
        return list(range(n_scenes))
    scenes = list(scenes)
    if not scenes:
        raise ValueError("a grouped call lists at least one scene")
    for s in scenes:
        if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or not 0 <= s < n_scenes:
            raise ValueError(f"scene index {s!r} outside the group's {n_scenes} scenes")
    if len(set(int(s) for s in scenes)) != len(scenes):
        raise ValueError(f"scenes {scenes} lists a scene twice")
    return [int(s) for s in scenes]


def compute_projection_group(img_metas, strides, device=None) -> Tensor:
    """:func:`compute_projection` for the chunk metas of several scenes and several strides at once: ``(len(strides), sum of views, 3, 4)``, the
    rows in the metas' order -- the same host arithmetic element for element (hostmath.py), one product and one asynchronous upload for all."""
    ks, exts = [], []
    for stride in strides:
        for m in img_metas:
            k = torch.tensor(np.asarray(m["lidar2img"]["intrinsic"], dtype=np.float32)[:3, :3])
            k[:2] /= m["ori_shape"][0] / (m["img_shape"][0] / stride)
            ext = np.stack([np.asarray(e, dtype=np.float32)[:3] for e in m["lidar2img"]["extrinsic"]])
            ks.append(np.broadcast_to(k.numpy()[None], (ext.shape[0], 3, 3)))
            exts.append(ext)
    proj = torch.from_numpy(matmul_fma_chain(np.concatenate(ks), np.concatenate(exts))).reshape(len(strides), -1, 3, 4)
    if device is None:
        return proj
    return _upload_async(proj, device) if torch.device(device).type == "cuda" else proj.to(device)


def _group_points(points: Sequence[Tensor], grid, on_gpu: bool) -> list:
    """The ``(3,X,Y,Z)`` point lattices of a group's 1 .. GROUP_MAX scenes, checked against ``grid``, as contiguous float32."""
    points = list(points)
    if not 1 <= len(points) <= GROUP_MAX:
        raise ValueError(f"a scene group holds 1 to {GROUP_MAX} scenes, got {len(points)}")
    for p in points:
        if on_gpu:
            _need_gpu(p)
        assert tuple(p.shape[-3:]) == grid and p.shape[0] == 3, f"points {tuple(p.shape)} for a {grid} state"
    return [_f32c(p) for p in points]


def _fill_slot(row, st: SceneState, p: Tensor) -> None:
    """One NdetSceneSlot row: the state's four tensors and its scene's points.  The grouped kernels take the pitches from the group's block
    (:func:`_group_block`) and walk the rows in quads."""
    assert (st.k1_sum.stride(0), st.k2_sum.stride(0)) == (st.c, 3 * (st.cm + 4))
    assert (st.k1_sum.data_ptr() | st.k2_sum.data_ptr()) % 16 == 0 and st.k1_count.data_ptr() % 4 == 0 and st.k2_count.data_ptr() % 8 == 0 \
        and p.data_ptr() % 4 == 0, "state rows must be 16-byte aligned"
    row.k1_sum, row.k1_count, row.k2_sum, row.k2_count = st.k1_sum.data_ptr(), st.k1_count.data_ptr(), st.k2_sum.data_ptr(), st.k2_count.data_ptr()
    row.points = p.data_ptr()


def _upload_table(rows, device) -> Tensor:
    """A host array of table rows as bytes on ``device``, uploaded asynchronously on the current stream."""
    host = torch.frombuffer(bytearray(bytes(rows)), dtype=torch.uint8)
    return _upload_async(host, device) if device.type == "cuda" else host.clone()


def _group_block(n_slots: int, n_voxels: int, c: int, cm: int, table: Tensor) -> "_lib.NdetSceneGroup":
    """The C ABI's NdetSceneGroup for a table of ``n_slots`` states of ``c`` and ``cm`` channels."""
    g = _lib.NdetSceneGroup()
    g.size = ctypes.sizeof(_lib.NdetSceneGroup)
    g.n_slots, g.N, g.C, g.cm = n_slots, n_voxels, c, cm
    g.k1_pitch, g.k2_pitch, g.table = c, 3 * (cm + 4), table.data_ptr()
    return g


def _accumulate_group(front, n: int, s0: SceneState, features: Tensor, mapped: Tensor, bias: Tensor, denorm_images: Tensor,
                      projection: Tensor, rgb_projection: Tensor, depth_gate: Optional[DepthGate]) -> int:
    """The launch of ndet_scene_accumulate_group for n listed scenes whose states are like ``s0``: the chunk is checked, then ``front()``
    gives ``(block, selection, table tensor or None)`` -- the table is held until the launches are queued.  Returns k, the views a scene."""
    f, m, bias, rgb, projection, rgb_projection, n_v, h, w, hh, ww, g, read = _chunk_args(
        features, mapped, bias, denorm_images, projection, rgb_projection, depth_gate, s0.c, s0.cm)
    if n_v % n or not 1 <= n_v // n <= GROUP_VIEWS_MAX:
        raise ValueError(f"{n_v} views for {n} scenes: every listed scene brings the same 1 .. {GROUP_VIEWS_MAX} views")
    k = n_v // n
    blk, sel, table = front()
    trace.span("k_scene_accumulate_group", lambda: check(_lib.load().ndet_scene_accumulate_group(
        ctypes.byref(blk), ctypes.byref(sel), k, _ptr(f), h, w, f.stride(0), f.stride(2), _ptr(m), m.stride(0), m.stride(2), _ptr(bias), _ptr(rgb),
        hh, ww, rgb.stride(0), rgb.stride(1), rgb.stride(2), _ptr(projection), _ptr(rgb_projection), g, _stream(f)), "scene_accumulate_group"),
        bytes=read + 2 * n * (s0.k1_sum.numel() + s0.k2_sum.numel()) * 4, kind="hbm")
    return k


class SceneGroupState:
    """The states of S scenes (1 .. 64) that share grid, C and cm, one :class:`SceneState` and one ``(3,X,Y,Z)`` point lattice per scene, and
    the device table the grouped kernels find them through: one 64-byte NdetSceneSlot per scene, built on the host once and uploaded
    asynchronously.  The group owns every tensor the table points to, for its whole life: states are zeroed in place, never replaced.
    The upload is ordered on the stream that is current when the group is built (as a view bank's table is): use the group on that stream, or
    make the other stream wait for it first."""

    def __init__(self, n_voxels, c: int, cm: int, points: Sequence[Tensor], device):
        self.grid = tuple(int(v) for v in n_voxels)
        self.points = _group_points(points, self.grid, True)
        self.states = [SceneState(n_voxels, c, cm, device) for _ in self.points]
        self.c, self.cm, self.device = self.states[0].c, self.states[0].cm, torch.device(device)
        rows = (_lib.NdetSceneSlot * len(self.points))()
        for row, st, p in zip(rows, self.states, self.points):
            _fill_slot(row, st, p)
        self.table = _upload_table(rows, self.device)

    def __len__(self) -> int:
        return len(self.states)

    @property
    def n_voxels(self) -> int:
        return self.states[0].n_voxels

    @property
    def n_views(self):
        return [st.n_views for st in self.states]

    def listed(self, scenes) -> list:
        """``scenes`` (None: every scene, in order) as a checked list of distinct scene indices."""
        return listed_scenes(len(self.states), scenes)

    def block(self) -> "_lib.NdetSceneGroup":
        return _group_block(len(self.states), self.n_voxels, self.c, self.cm, self.table)

    def sel(self, scenes) -> "_lib.NdetGroupSel":
        """The C ABI's selection block for the (checked) scene list, with the scenes' view totals."""
        sel = _lib.NdetGroupSel()
        sel.size = ctypes.sizeof(_lib.NdetGroupSel)
        sel.n = len(scenes)
        for i, s in enumerate(scenes):
            sel.slot[i], sel.n_views[i] = s, self.states[s].n_views
        return sel


def scene_accumulate_group(group: SceneGroupState, scenes, features: Tensor, mapped: Tensor, bias: Tensor, denorm_images: Tensor,
                           projection: Tensor, rgb_projection: Tensor, depth_gate: Optional[DepthGate] = None) -> None:
    """:func:`scene_accumulate` for the listed scenes in two launches: every listed scene brings k views (1 .. 128), the view-indexed arguments
    hold ``len(scenes) * k`` views, scene-major in the listed order (``features`` (n k,C,h,w), ``mapped`` (n k,cm,h,w), ``denorm_images``
    (n k,3,H,W), the projections (n k,3,4), the gate's maps).  ``scenes``: None (all, in order) or distinct scene indices.  ``depth_gate``
    gates every scene of the call.  Each scene's state ends up bit-equal to :func:`scene_accumulate` on that scene alone, whatever the
    other scenes, the subset or its order."""
    _need_gpu(features, mapped, bias, denorm_images, projection, rgb_projection)
    scenes = group.listed(scenes)
    k = _accumulate_group(lambda: (group.block(), group.sel(scenes), None), len(scenes), group.states[0], features, mapped, bias, denorm_images,
                          projection, rgb_projection, depth_gate)
    for s in scenes:
        group.states[s].n_views += k


def _group_finish_args(group: SceneGroupState, scenes):
    scenes = group.listed(scenes)
    empty = [s for s in scenes if group.states[s].n_views == 0]
    if empty:
        raise ValueError(f"scenes {empty} have no views yet")
    return scenes, group.block(), group.sel(scenes)


def density_finish_group(group: SceneGroupState, bias: Tensor, scenes=None) -> Tensor:
    """:func:`density_finish` for the listed scenes in one launch: ``(len(scenes) * N, 2*(3+cm))`` rows, listed scene i's voxel v in row
    ``i N + v``, each scene finished over its own view total; bit for bit :func:`density_finish`'s rows per scene.  No state is changed."""
    _need_gpu(bias)
    scenes, blk, sel = _group_finish_args(group, scenes)
    s0 = group.states[0]
    bias, out = _density_out(bias, group.cm, len(scenes) * s0.n_voxels, s0.k1_sum.device)
    trace.span("k_density_finish_group", lambda: check(_lib.load().ndet_scene_density_finish_group(
        ctypes.byref(blk), ctypes.byref(sel), _ptr(bias), _ptr(out), _stream(out)), "scene_density_finish_group"),
        bytes=4 * (len(scenes) * s0.k2_sum.numel() + out.numel()), kind="hbm")
    return out


def volume_finish_group(group: SceneGroupState, alpha: Optional[Tensor] = None, scenes=None) -> Tuple[Tensor, Tensor]:
    """:func:`volume_finish` for the listed scenes in one launch: ``(volume (n,C,X,Y,Z) with (n,X,Y,Z,C) memory, count (n,1,X,Y,Z) int64)``;
    ``alpha`` None or ``n * N`` values indexed as :func:`density_finish_group`'s rows.  Bit for bit :func:`volume_finish`'s outputs per scene;
    no state is changed."""
    _need_gpu(alpha)
    scenes, blk, sel = _group_finish_args(group, scenes)
    n, s0 = len(scenes), group.states[0]
    alpha, buf, count = _volume_out(alpha, n, group.grid, group.c, s0.k1_sum.device)
    trace.span("k_volume_finish_group", lambda: check(_lib.load().ndet_scene_volume_finish_group(
        ctypes.byref(blk), ctypes.byref(sel), _ptr(alpha), _ptr(buf), _ptr(count), _stream(buf)), "scene_volume_finish_group"),
        bytes=n * (8 * s0.k1_sum.numel() + 12 * s0.n_voxels), kind="hbm")
    return buf.permute(0, 4, 1, 2, 3), count


# --------------------------------------------------------------------------------------------
# Windowed groups: every scene of a group keeps a sliding window of chunks, one state per chunk, all the states behind one pool table
# (include/nerfdet_hip.h, NdetGroupRingSel)
# --------------------------------------------------------------------------------------------
GROUP_POOL_MAX = GROUP_MAX * (RING_MAX + 1)    # states one pool table may hold (include/nerfdet_hip.h, NDET_GROUP_POOL_MAX)


def check_window(window) -> int:
    """``window`` of a windowed stream or group: an int in 1 .. RING_MAX (else ValueError)."""
    if isinstance(window, bool) or not isinstance(window, int) or not 1 <= window <= RING_MAX:
        raise ValueError(f"window must be None or an int in 1 .. {RING_MAX}, got {window!r}")
    return window


class SceneGroupRingState:
    """The windows of S scenes (1 .. 64) that share grid, C and cm: per scene the states of the chunks held, oldest first (``segs[s]``), and
    its zeroed states waiting for chunks to come (``spare[s]``) -- at most ``window + 1`` states per scene, allocated when first needed (a
    sliding window owns S + 1: the chunk that leaves hands its state to the chunk after the next).  Every state is a row of one pool
    table on the device (64-byte NdetSceneSlot rows, each with its scene's points), uploaded again only when a state is first allocated;
    the table has room for every state the pool can come to own, so its address changes with an upload but not its size.  The pool owns
    every tensor the table points to: states are zeroed in place, never replaced.  Uploads are ordered on the stream that is current
    when they are made: use the pool on one stream."""

    def __init__(self, n_voxels, c: int, cm: int, points: Sequence[Tensor], window: int, device):
        self.window = check_window(window)
        self.grid, self.device = tuple(int(v) for v in n_voxels), torch.device(device)
        self.points = _group_points(points, self.grid, self.device.type == "cuda")
        assert c % 4 == 0 and cm % 4 == 0, f"streaming needs C and cm in multiples of 4 (got {c}, {cm})"
        self.c, self.cm = int(c), int(cm)
        self.segs = [[] for _ in self.points]
        self.spare = [[] for _ in self.points]
        self.states = []            # every state of the pool; a state's pool row is its index here (``state.row``)
        self.owner = []             # the scene of every pool row
        self._table = None          # the device table, or None when a state has been allocated since the last upload
        self._version = 0           # bumped whenever a window changes: the finishes' selection is built once per version and scene list
        self._sel = None

    def __len__(self) -> int:
        return len(self.segs)

    @property
    def n_voxels(self) -> int:
        return self.grid[0] * self.grid[1] * self.grid[2]

    @property
    def chunk_views(self):
        """Per scene the view counts of the chunks held, oldest first."""
        return [[st.n_views for st in segs] for segs in self.segs]

    @property
    def n_chunks(self):
        return [len(segs) for segs in self.segs]

    @property
    def n_views(self):
        return [sum(st.n_views for st in segs) for segs in self.segs]

    def listed(self, scenes) -> list:
        return listed_scenes(len(self.segs), scenes)

    def owned(self, s: int) -> int:
        """States scene ``s`` owns, held or spare."""
        return len(self.segs[s]) + len(self.spare[s])

    def _new_state(self, s: int) -> SceneState:
        assert sum(1 for o in self.owner if o == s) <= self.window, f"scene {s} already owns {self.window + 1} states"
        st = SceneState(self.grid, self.c, self.cm, self.device)
        st.row = len(self.states)
        self.states.append(st)
        self.owner.append(s)
        self._table = None
        return st

    def take(self, scenes) -> list:
        """One empty state per listed scene, from its spares or freshly allocated; they belong to no window until :meth:`push`."""
        return [self.spare[s].pop() if self.spare[s] else self._new_state(s) for s in scenes]

    def give_back(self, scenes, states) -> None:
        """States taken for a call that failed go back to their scenes' spares, zeroed."""
        for s, st in zip(scenes, states):
            st.reset()
            self.spare[s].append(st)

    def push(self, scenes, states) -> None:
        """The filled states join their scenes' windows; the oldest chunk leaves each listed scene whose window was full."""
        for s, st in zip(scenes, states):
            if len(self.segs[s]) == self.window:
                self._drop(s, 1)
            self.segs[s].append(st)
        self._version += 1

    def _drop(self, s: int, k: int) -> None:
        for st in self.segs[s][:k]:
            st.reset()
            self.spare[s].append(st)
        del self.segs[s][:k]

    def drop_oldest(self, k: int = 1, scenes=None) -> None:
        """Forget the k oldest chunks of every listed scene; refused whole (ValueError) when a listed scene holds fewer than k."""
        scenes = self.listed(scenes)
        if isinstance(k, bool) or not isinstance(k, int) or k < 0:
            raise ValueError(f"drop_oldest: k={k!r}")
        short = [s for s in scenes if len(self.segs[s]) < k]
        if short:
            raise ValueError(f"drop_oldest: k={k!r} for {[len(self.segs[s]) for s in short]} chunks held by scenes {short}")
        for s in scenes:
            self._drop(s, k)
        self._version += 1

    def accumulate(self, scenes, fill) -> None:
        """One chunk per listed scene: ``fill(states)`` fills one empty state per listed scene; only when it has succeeded do the states
        join the windows and the oldest chunks leave the full ones.  When it raises, every window stays as it was and the states go back
        zeroed."""
        states = self.take(scenes)
        try:
            fill(states)
        except BaseException:
            self.give_back(scenes, states)
            raise
        self.push(scenes, states)

    def table(self) -> Tensor:
        """The pool table on the device, uploaded when a state has been allocated since the last call; rows beyond the states allocated
        are null and beyond ``n_slots``."""
        if self._table is None:
            rows = (_lib.NdetSceneSlot * (len(self.segs) * (self.window + 1)))()
            for st, s in zip(self.states, self.owner):
                _fill_slot(rows[st.row], st, self.points[s])
            self._table = _upload_table(rows, self.device)
        return self._table

    def block(self):
        """``(NdetSceneGroup block of the pool, the table tensor it points to)``."""
        table = self.table()
        return _group_block(len(self.states), self.n_voxels, self.c, self.cm, table), table

    def front(self, scenes, states):
        """A call's front table -- one row per listed scene, pointing at the state it fills and its scene's points -- with the block and the
        selection ndet_scene_accumulate_group takes for it: ``(block, sel, table tensor)``."""
        rows = (_lib.NdetSceneSlot * len(scenes))()
        sel = _lib.NdetGroupSel()
        sel.size, sel.n = ctypes.sizeof(_lib.NdetGroupSel), len(scenes)
        for i, (s, st) in enumerate(zip(scenes, states)):
            assert st.n_views == 0, "a front state must be empty"
            _fill_slot(rows[i], st, self.points[s])
            sel.slot[i], sel.n_views[i] = i, 0
        table = _upload_table(rows, self.device)
        return _group_block(len(scenes), self.n_voxels, self.c, self.cm, table), sel, table

    def ring_sel(self, scenes):
        """The grouped ring finishes' arguments for the (checked) scene list: ``(NdetGroupRingSel, segment lists on the host, on the
        device)``, (n, RING_MAX) int32 pool rows, oldest first; built and uploaded once per scene list and window change."""
        key = (tuple(scenes), self._version)
        if self._sel is None or self._sel[0] != key:
            sel = _lib.NdetGroupRingSel()
            sel.size, sel.n = ctypes.sizeof(_lib.NdetGroupRingSel), len(scenes)
            host = torch.zeros((len(scenes), RING_MAX), dtype=torch.int32)
            for i, s in enumerate(scenes):
                segs = self.segs[s]
                sel.n_segs[i], sel.n_views[i] = len(segs), sum(st.n_views for st in segs)
                host[i, :len(segs)] = torch.tensor([st.row for st in segs], dtype=torch.int32)
            dev = _upload_async(host, self.device) if self.device.type == "cuda" else host.clone()
            self._sel = (key, sel, host, dev)
        return self._sel[1:]


def scene_accumulate_group_ring(pool: SceneGroupRingState, scenes, features: Tensor, mapped: Tensor, bias: Tensor, denorm_images: Tensor,
                                projection: Tensor, rgb_projection: Tensor, depth_gate: Optional[DepthGate] = None, states=None) -> None:
    """:func:`scene_accumulate_group` for a windowed group: one chunk of k views per listed scene, each into an empty state of its own that
    then joins its scene's window (the oldest chunk leaving a full one); arguments as :func:`scene_accumulate_group`'s.  The grouped
    accumulate runs unchanged over a per-call table of the n states it fills, so each holds the bits :func:`scene_accumulate` leaves in an
    empty state for that chunk -- what a windowed SceneStream's segment holds.  A call that raises leaves every window as it was.
    ``states``: None, or the empty states to fill (one per listed scene, from ``pool.take``); the caller then does the pool's bookkeeping
    (``pool.accumulate`` is that bookkeeping, and what this function does with ``states=None``)."""
    scenes = pool.listed(scenes)
    if states is None:
        pool.accumulate(scenes, lambda front: scene_accumulate_group_ring(pool, scenes, features, mapped, bias, denorm_images, projection,
                                                                          rgb_projection, depth_gate=depth_gate, states=front))
        return
    _need_gpu(features, mapped, bias, denorm_images, projection, rgb_projection)
    assert len(states) == len(scenes)
    k = _accumulate_group(lambda: pool.front(scenes, states), len(scenes), states[0], features, mapped, bias, denorm_images, projection,
                          rgb_projection, depth_gate)
    for st in states:
        st.n_views = k


def _group_ring_finish_args(pool: SceneGroupRingState, scenes):
    scenes = pool.listed(scenes)
    empty = [s for s in scenes if sum(st.n_views for st in pool.segs[s]) == 0]
    if empty:
        raise ValueError(f"scenes {empty} have no views yet")
    blk, table = pool.block()
    return (scenes, blk, table) + tuple(pool.ring_sel(scenes))


def density_finish_group_ring(pool: SceneGroupRingState, bias: Tensor, scenes=None) -> Tensor:
    """:func:`density_finish_ring` for the listed scenes' windows in one launch: ``(len(scenes) * N, 2*(3+cm))`` rows as
    :func:`density_finish_group` returns them, listed scene i finished over its own segments and view total; bit for bit
    :func:`density_finish_ring`'s rows over that scene's states.  No state is changed.  The span's bytes count every segment in full, an
    upper bound as in :func:`density_finish_ring`."""
    _need_gpu(bias)
    scenes, blk, table, sel, segs_host, segs_dev = _group_ring_finish_args(pool, scenes)
    bias, out = _density_out(bias, pool.cm, len(scenes) * pool.n_voxels, pool.device)
    read = sum(st.k2_sum.numel() + st.k2_count.numel() for s in scenes for st in pool.segs[s])
    trace.span("k_density_finish_group_ring", lambda: check(_lib.load().ndet_scene_density_finish_group_ring(
        ctypes.byref(blk), ctypes.byref(sel), segs_host.data_ptr(), _ptr(segs_dev), _ptr(bias), _ptr(out), _stream(out)),
        "scene_density_finish_group_ring"), bytes=4 * (read + out.numel()), kind="hbm")
    return out


def volume_finish_group_ring(pool: SceneGroupRingState, alpha: Optional[Tensor] = None, scenes=None) -> Tuple[Tensor, Tensor]:
    """:func:`volume_finish_ring` for the listed scenes' windows in one launch: ``(volume (n,C,X,Y,Z) with (n,X,Y,Z,C) memory, count
    (n,1,X,Y,Z) int64)`` as :func:`volume_finish_group` returns them; ``alpha`` None or ``n * N`` values indexed as
    :func:`density_finish_group_ring`'s rows.  Bit for bit :func:`volume_finish_ring`'s outputs over each scene's states; no state is
    changed.  The span's bytes count every segment in full, an upper bound."""
    _need_gpu(alpha)
    scenes, blk, table, sel, segs_host, segs_dev = _group_ring_finish_args(pool, scenes)
    n, n_vox = len(scenes), pool.n_voxels
    alpha, buf, count = _volume_out(alpha, n, pool.grid, pool.c, pool.device)
    read = sum(st.k1_sum.numel() + st.k1_count.numel() for s in scenes for st in pool.segs[s])
    trace.span("k_volume_finish_group_ring", lambda: check(_lib.load().ndet_scene_volume_finish_group_ring(
        ctypes.byref(blk), ctypes.byref(sel), segs_host.data_ptr(), _ptr(segs_dev), _ptr(alpha), _ptr(buf), _ptr(count), _stream(buf)),
        "scene_volume_finish_group_ring"), bytes=4 * (read + buf.numel()) + (12 if alpha is not None else 8) * n * n_vox, kind="hbm")
    return buf.permute(0, 4, 1, 2, 3), count


# --------------------------------------------------------------------------------------------
# A6 pieces
# --------------------------------------------------------------------------------------------
def sigma_to_alpha(raw_sigma: Tensor) -> Tensor:
    """``1 - exp(-relu(raw_sigma))`` (nerf_mlp.py:227, nerfdet.py:257)."""
    _need_gpu(raw_sigma)
    r = _f32c(raw_sigma).reshape(-1)
    out = torch.empty_like(r)
    check(_lib.load().ndet_sigma_to_alpha(_ptr(r), _ptr(out), r.numel(), _stream(r)), "sigma_to_alpha")
    return out


def occupancy_bits(alpha: Tensor, count: Tensor, n_voxels, threshold: float, dilate: int) -> Tensor:
    """The lattice's alpha (N,) and view count (N,) int64, flat as :func:`get_points` orders the voxels, as a dilated occupancy bit grid:
    ``((N + 31) // 32,)`` int32 words, bit ``n & 31`` of word ``n >> 5`` set iff a voxel within Chebyshev distance ``dilate`` (0, 1, 2) of
    voxel n is solid -- ``not (alpha <= threshold)`` (a NaN is solid) or seen by no view (k_occupancy_bits; the same bytes on every call)."""
    _need_gpu(alpha, count)
    nv = [int(v) for v in (n_voxels.tolist() if isinstance(n_voxels, Tensor) else n_voxels)]
    a = _f32c(alpha).reshape(-1)
    c = count.to(torch.int64).contiguous().reshape(-1)
    n = nv[0] * nv[1] * nv[2]
    assert len(nv) == 3 and a.numel() == n and c.numel() == n, f"alpha {tuple(alpha.shape)} and count {tuple(count.shape)} for a {nv} lattice"
    bits = torch.empty(((n + 31) // 32,), dtype=torch.int32, device=a.device)
    trace.span("k_occupancy_bits", lambda: check(_lib.load().ndet_occupancy_bits(_ptr(a), _ptr(c), nv[0], nv[1], nv[2], float(threshold), int(dilate),
                                                                                _ptr(bits), _stream(a)), "occupancy_bits"),
               bytes=12 * n + 4 * bits.numel(), kind="hbm")
    return bits


# --------------------------------------------------------------------------------------------
# space carving from depth frames (csrc/carve_kernels.hip)
# --------------------------------------------------------------------------------------------
CARVE_REFINES = (1, 2, 4)


def carve_lattice(n_voxels, voxel_size, refine: int):
    """``(n_voxels_fine, voxel_size_fine)`` of the fine lattice that refines the detection lattice by ``refine`` (1, 2, 4) per axis:
    ``get_points(r n_voxels, voxel_size / r, origin)``, the same box and centre; ``voxel_size / r`` is taken in float32, where a division
    by a power of two is exact."""
    if isinstance(refine, bool) or not isinstance(refine, (int, np.integer)) or int(refine) not in CARVE_REFINES:
        raise ValueError(f"carve: refine={refine!r} must be 1, 2 or 4")
    r = int(refine)
    nv = [int(v) for v in (n_voxels.tolist() if isinstance(n_voxels, Tensor) else n_voxels)]
    vs = [float(v) for v in (voxel_size.tolist() if isinstance(voxel_size, Tensor) else voxel_size)]
    return tuple(r * v for v in nv), tuple(float(np.float32(v) / np.float32(r)) for v in vs)


def carve_accumulate(counts: Tensor, points: Tensor, projection: Tensor, gate: DepthGate) -> Tensor:
    """Add the evidence of a chunk's k views to ``counts`` (N,) int32, one word per voxel of the fine lattice ``points`` (3,X,Y,Z): the
    free count in bits 0-15, the hit count in bits 16-31, each saturating at 65535.  ``projection`` (k,3,4) the chunk's stride-1
    projections; ``gate`` the chunk's :class:`DepthGate`, whose image-resolution map ``depth_r`` (k,H,W) and ``band`` are read.  View by
    view, a voxel the projection accepts at a pixel of depth ``d > 0`` is FREE iff ``not (z > d - band)`` and a HIT iff the gate's own
    band test holds (include/nerfdet_hip.h).  In place, one k_carve_accumulate launch; returns ``counts``."""
    _need_gpu(counts, points, projection)
    d = gate.depth_r
    assert d is not None, "carve_accumulate: the depth gate has no map at the image's size (ops.depth_gate(..., img_hw=))"
    assert points.dim() == 4 and points.shape[0] == 3 and points.dtype == torch.float32 and points.is_contiguous(), \
        f"points must be a contiguous float32 (3,X,Y,Z) lattice, got {tuple(points.shape)}"
    nx, ny, nz = points.shape[1:]
    n = nx * ny * nz
    assert counts.dtype == torch.int32 and counts.is_contiguous() and counts.numel() == n, \
        f"counts must be a contiguous int32 tensor of {n} words, got {tuple(counts.shape)} {counts.dtype}"
    proj = _f32c(projection)
    k = proj.shape[0]
    assert tuple(proj.shape) == (k, 3, 4) and k >= 1 and d.shape[0] == k, f"projection {tuple(projection.shape)} for a {tuple(d.shape)} map"
    if d.stride(2) != 1:
        d = d.contiguous()
    h, w = d.shape[1], d.shape[2]
    trace.span("k_carve_accumulate", lambda: check(
        _lib.load().ndet_carve_accumulate(_ptr(points), nx, ny, nz, _ptr(proj), k, _ptr(d), _DEPTH_DTYPES[d.dtype], d.stride(0), d.stride(1), h, w,
                                          float(gate.band), _ptr(counts), _stream(counts)), "carve_accumulate"),
        bytes=20 * n + 48 * k + d.element_size() * k * h * w, kind="hbm")
    return counts


CARVE_TWO_PASS = True   # carve_bits with dilate > 0: undilated bits first, then a dilation from the bits (DESIGN.md 21 has the timings)


def carve_bits(segments: Sequence[Tensor], n_voxels_fine, min_free: int, dilate: int, coarse_bits: Optional[Tensor] = None, refine: int = 1,
               two_pass: Optional[bool] = None) -> Tensor:
    """1 .. 64 counter segments of :func:`carve_accumulate` over one fine lattice -> its dilated occupancy bit grid, ``((N + 31) // 32,)``
    int32 words in :func:`occupancy_bits`' format.  Free and hit are summed over the segments; a voxel is empty iff ``free >= min_free
    and hit == 0`` and solid otherwise; with ``coarse_bits`` (an undilated :func:`occupancy_bits` grid of the parent lattice
    ``n_voxels_fine / refine``) it is solid iff it is carve-solid and its parent's bit is set; a bit is set iff a voxel within Chebyshev
    distance ``dilate`` is solid.  ``two_pass``: None (``CARVE_TWO_PASS``), or which of the kernel's two forms runs; the bytes are the
    same.  The same bytes on every call."""
    segments = list(segments)
    _need_gpu(*segments, coarse_bits)
    nv = [int(v) for v in (n_voxels_fine.tolist() if isinstance(n_voxels_fine, Tensor) else n_voxels_fine)]
    n = nv[0] * nv[1] * nv[2]
    assert 1 <= len(segments) <= RING_MAX, f"carve_bits takes 1 to {RING_MAX} segments, got {len(segments)}"
    for s in segments:
        assert s.dtype == torch.int32 and s.is_contiguous() and s.numel() == n and s.device == segments[0].device, \
            f"every segment must be a contiguous int32 tensor of {n} words on one device"
    words = (n + 31) // 32
    if coarse_bits is not None:
        r = int(refine)
        assert r in CARVE_REFINES and all(v % r == 0 for v in nv), f"refine={refine!r} for a {nv} lattice"
        cw = (n // r ** 3 + 31) // 32
        assert coarse_bits.dtype == torch.int32 and coarse_bits.is_contiguous() and tuple(coarse_bits.shape) == (cw,), \
            f"coarse_bits must be a contiguous ({cw},) int32 tensor"
    dev = segments[0].device
    bits = torch.empty((words,), dtype=torch.int32, device=dev)
    two = (CARVE_TWO_PASS if two_pass is None else bool(two_pass)) and int(dilate) > 0
    scratch = torch.empty((words,), dtype=torch.int32, device=dev) if two else None
    ptrs = (ctypes.c_void_p * len(segments))(*[s.data_ptr() for s in segments])
    reads = len(segments) * (1 if two or not dilate else (2 * int(dilate) + 1) ** 3)
    trace.span("k_carve_bits", lambda: check(
        _lib.load().ndet_carve_bits(ptrs, len(segments), int(min_free), int(dilate), nv[0], nv[1], nv[2], _ptr(coarse_bits), int(refine),
                                    _ptr(scratch), _ptr(bits), _stream(bits)), "carve_bits"),
        bytes=4 * n * reads + 4 * words * (3 if two else 1), kind="hbm")
    return bits


def carve_counts(segments: Sequence[Tensor], n_voxels_fine) -> Tuple[Tensor, Tensor]:
    """``(free, hit)`` int32 (X,Y,Z) tensors: the segments' counts summed (torch arithmetic; for inspection, not on a hot path)."""
    nv = [int(v) for v in n_voxels_fine]
    free = sum((s & 0xffff) for s in segments)
    hit = sum(((s >> 16) & 0xffff) for s in segments)
    return free.view(*nv).to(torch.int32), hit.view(*nv).to(torch.int32)


# --------------------------------------------------------------------------------------------
# points out: a voxel-downsampled point cloud of a streamed RGB-D scene (csrc/cloud_kernels.hip)
# --------------------------------------------------------------------------------------------
CLOUD_WORDS = 8                 # uint32 words of a fine voxel's record: n, sum qx, qy, qz, sum b, g, r, one spare word (32 bytes)
CLOUD_FIELDS = ("n", "qx", "qy", "qz", "b", "g", "r")
CLOUD_PIXELS_MAX = 2 ** 24      # pixels of one launch, and contributions a segment may hold, stay below this: a sum of bytes stays exact
CLOUD_WAVE_MERGE = True         # k_cloud_accumulate sums the lanes of a wave that share a voxel before it touches memory


def _cloud_lattice(n_voxels_fine, p0, vs):
    nv = [int(v) for v in (n_voxels_fine.tolist() if isinstance(n_voxels_fine, Tensor) else n_voxels_fine)]
    p0 = [float(v) for v in (p0.tolist() if isinstance(p0, (Tensor, np.ndarray)) else p0)]
    vs = [float(v) for v in (vs.tolist() if isinstance(vs, (Tensor, np.ndarray)) else vs)]
    if len(nv) != 3 or len(p0) != 3 or len(vs) != 3 or min(nv) < 1:
        raise ValueError(f"cloud: a lattice is three positive voxel counts, a first point and a voxel size, got {nv}, {p0}, {vs}")
    if not all(np.isfinite(v) and v > 0 for v in vs) or not all(np.isfinite(v) for v in p0):
        raise ValueError(f"cloud: the voxel size {vs} must be positive and finite, the first point {p0} finite")
    if nv[0] * nv[1] * nv[2] >= 2 ** 31:
        raise ValueError(f"cloud: {nv} holds 2^31 voxels or more")
    return nv, p0, vs


def _cloud_segments(segments, n: int, what: str) -> list:
    segments = list(segments)
    if not 1 <= len(segments) <= RING_MAX:
        raise ValueError(f"{what} takes 1 to {RING_MAX} segments, got {len(segments)}")
    for s in segments:
        if not isinstance(s, Tensor) or s.dtype != torch.int32 or tuple(s.shape) != (n, CLOUD_WORDS) or not s.is_contiguous() \
                or s.device != segments[0].device:
            raise ValueError(f"{what}: every segment must be a contiguous ({n}, {CLOUD_WORDS}) int32 tensor on one device")
    return segments


def check_cloud_max_depth(max_depth):
    """``max_depth`` of a cloud as the float32 value the kernel compares with (0.0: none): None or a finite positive number; else ValueError."""
    if max_depth is None:
        return 0.0
    if isinstance(max_depth, bool) or not isinstance(max_depth, (int, float, np.floating, np.integer)) or not np.isfinite(max_depth) \
            or not float(np.float32(max_depth)) > 0:
        raise ValueError(f"cloud: max_depth={max_depth!r} must be None or a finite positive number of metres")
    return float(np.float32(max_depth))


def cloud_accumulate(sums: Tensor, n_voxels_fine, p0, vs, depth_r: Tensor, rgb: Tensor, intrinsic, c2w, max_depth=None,
                     merge: Optional[bool] = None) -> Tensor:
    """Add a chunk's k views to ``sums`` (N, 8) int32, the records of the fine lattice ``n_voxels_fine`` with first point ``p0`` and voxel
    size ``vs`` (:func:`carve_lattice` over :func:`get_points`).  ``depth_r`` (k, H, W) float32 / float64 metres at the image's size (a
    :class:`DepthGate`'s ``depth_r``), ``rgb`` (k, 3, H, W) float32 B, G, R planes in [0, 1]; both may be pitched views with a unit last
    stride.  ``intrinsic`` 3 x 3 or 4 x 4 at the image's scale and ``c2w`` k camera-to-world 4 x 4, as pipeline.camera_rays takes them.
    A pixel with ``d > 0``, finite and ``d <= max_depth`` (None: no limit) adds its point -- the camera centre plus d times camera_rays'
    direction -- to the voxel ``floor((x - p0) / vs + 0.5)`` (include/nerfdet_hip.h).  ``merge``: None (``CLOUD_WAVE_MERGE``), or which of
    the kernel's two forms runs; the bytes are the same.  In place, one k_cloud_accumulate launch; returns ``sums``.  ValueError for wrong
    shapes or dtypes before the launch, RuntimeError for CPU tensors."""
    nv, p0, vs = _cloud_lattice(n_voxels_fine, p0, vs)
    n = nv[0] * nv[1] * nv[2]
    md = check_cloud_max_depth(max_depth)
    if not isinstance(sums, Tensor) or sums.dtype != torch.int32 or tuple(sums.shape) != (n, CLOUD_WORDS) or not sums.is_contiguous():
        raise ValueError(f"cloud_accumulate: sums must be a contiguous ({n}, {CLOUD_WORDS}) int32 tensor")
    d = depth_r
    if not isinstance(d, Tensor) or d.dim() != 3 or d.dtype not in _DEPTH_DTYPES or min(d.shape) < 1:
        raise ValueError("cloud_accumulate: depth_r must be a (k, H, W) float32 or float64 tensor")
    k, h, w = (int(v) for v in d.shape)
    if not isinstance(rgb, Tensor) or rgb.dtype != torch.float32 or tuple(rgb.shape) != (k, 3, h, w):
        raise ValueError(f"cloud_accumulate: rgb must be a ({k}, 3, {h}, {w}) float32 tensor beside depth_r {tuple(d.shape)}")
    if k * h * w >= CLOUD_PIXELS_MAX:
        raise ValueError(f"cloud_accumulate: {k} views of {h} x {w} hold 2^24 pixels or more; add them in smaller chunks")
    kk = intrinsic.detach().cpu().numpy() if isinstance(intrinsic, Tensor) else np.asarray(intrinsic)
    if kk.shape not in ((3, 3), (4, 4)):
        raise ValueError(f"cloud_accumulate takes 3 x 3 or 4 x 4 intrinsics, got {kk.shape}")
    m = c2w.detach().cpu().numpy() if isinstance(c2w, Tensor) else np.asarray(c2w)
    if m.shape != (k, 4, 4):
        raise ValueError(f"cloud_accumulate: c2w must be ({k}, 4, 4) camera-to-world matrices, got {m.shape}")
    _need_gpu(sums, d, rgb)
    if d.device != sums.device or rgb.device != sums.device:
        raise ValueError("cloud_accumulate: sums, depth_r and rgb live on different devices")
    if d.stride(2) != 1 or d.stride(1) < w or d.stride(0) < h * d.stride(1):
        d = d.contiguous()
    if rgb.stride(3) != 1 or rgb.stride(2) < w or rgb.stride(1) < h * rgb.stride(2) or rgb.stride(0) < 3 * rgb.stride(1):
        rgb = rgb.contiguous()
    m = m.astype(np.float32)
    # one upload: 6 intrinsic floats, then the k rotations, then the k centres (pipeline.camera_rays' layout)
    host = np.concatenate([np.ascontiguousarray(kk[:2, :3], dtype=np.float32).reshape(-1), m[:, :3, :3].reshape(-1), m[:, :3, 3].reshape(-1)])
    buf = _upload_async(torch.from_numpy(host), sums.device)
    merge = CLOUD_WAVE_MERGE if merge is None else bool(merge)
    trace.span("k_cloud_accumulate", lambda: check(
        _lib.load().ndet_cloud_accumulate(_ptr(d), _DEPTH_DTYPES[d.dtype], d.stride(0), d.stride(1), _ptr(rgb), rgb.stride(0), rgb.stride(1),
                                          rgb.stride(2), _ptr(buf), _ptr(buf[6:]), _ptr(buf[6 + 9 * k:]), k, h, w, float3(p0), float3(vs),
                                          nv[0], nv[1], nv[2], md, int(merge), _ptr(sums), _stream(sums)), "cloud_accumulate"),
        bytes=k * h * w * (d.element_size() + 12), kind="hbm")
    return sums


def compaction_offsets(counts: Tensor):
    """Between the two launches of an ordered compaction (csrc/grid_common.hpp): the count pass' ``counts`` (blocks,) int32 -> ``(first,
    M)``, the exclusive prefix sum that the write pass reads and the number of kept elements.  M reaches the host in ONE device-to-host
    read, the compaction's only synchronisation; the caller skips the write launch when ``M = 0``."""
    last = torch.cumsum(counts, 0, dtype=torch.int32)
    return last - counts, int(last[-1])                        # the one read


def cloud_points(segments: Sequence[Tensor], n_voxels_fine, p0, vs, min_points: int = 1) -> dict:
    """1 .. 64 segments of :func:`cloud_accumulate` records over one fine lattice -> ``dict(xyz (M,3) float32, bgr (M,3) uint8, count (M,)
    int32, voxel (M,) int32)``: one point per fine voxel whose count, summed over the segments, is ``min_points`` or more, in ascending
    flat index -- the mean position, the mean colour (rounded half up), the count and the index (include/nerfdet_hip.h).  Two launches
    (k_cloud_count, k_cloud_write) around one prefix sum; M reaches the host in ONE device-to-host read, the call's only synchronisation;
    ``M = 0`` skips the second launch.  The same bytes on every call."""
    nv, p0, vs = _cloud_lattice(n_voxels_fine, p0, vs)
    n = nv[0] * nv[1] * nv[2]
    if isinstance(min_points, bool) or not isinstance(min_points, (int, np.integer)) or not 1 <= min_points < 2 ** 31:
        raise ValueError(f"cloud_points: min_points={min_points!r} must be an int of at least 1")
    segments = _cloud_segments(segments, n, "cloud_points")
    _need_gpu(*segments)
    lib, dev = _lib.load(), segments[0].device
    ptrs = (ctypes.c_void_p * len(segments))(*[s.data_ptr() for s in segments])
    geom = (nv[0], nv[1], nv[2], float3(p0), float3(vs), int(min_points))
    counts = torch.empty((int(lib.ndet_cloud_blocks(n)),), dtype=torch.int32, device=dev)
    trace.span("k_cloud_count", lambda: check(lib.ndet_cloud_count(ptrs, len(segments), *geom, _ptr(counts), _stream(counts)), "cloud_count"),
               bytes=32 * n * len(segments) + 4 * counts.numel(), kind="hbm")
    first, m = compaction_offsets(counts)
    out = dict(xyz=torch.empty((m, 3), dtype=torch.float32, device=dev), bgr=torch.empty((m, 3), dtype=torch.uint8, device=dev),
               count=torch.empty((m,), dtype=torch.int32, device=dev), voxel=torch.empty((m,), dtype=torch.int32, device=dev))
    if m:
        trace.span("k_cloud_write", lambda: check(
            lib.ndet_cloud_write(ptrs, len(segments), *geom, _ptr(first), _ptr(out["xyz"]), _ptr(out["bgr"]), _ptr(out["count"]),
                                 _ptr(out["voxel"]), _stream(counts)), "cloud_write"),
            bytes=32 * n * len(segments) + 23 * m, kind="hbm")
    return out


def cloud_sums(segments: Sequence[Tensor], n_voxels_fine) -> dict:
    """``dict(n, qx, qy, qz, b, g, r)`` of int64 (X,Y,Z) tensors: the segments' records summed field by field (torch arithmetic; for
    inspection, not on a hot path)."""
    nv = [int(v) for v in n_voxels_fine]
    segments = _cloud_segments(segments, nv[0] * nv[1] * nv[2], "cloud_sums")
    total = sum((s.to(torch.int64) & 0xffffffff) for s in segments)
    return {f: total[:, i].reshape(*nv).contiguous() for i, f in enumerate(CLOUD_FIELDS)}


def alpha_gate(mean: Tensor, density: Tensor, count: Tensor) -> Tensor:
    """Unfused gating of nerfdet.py:257-261: ``(1-exp(-density)) * mean`` zeroed where count == 0.
    ``mean`` (C,X,Y,Z) contiguous or channels-last (as produced by :func:`backproject_aggregate`)."""
    _need_gpu(mean, density, count)
    c = mean.shape[0]
    n = mean[0].numel()
    if mean.is_contiguous():
        layout, out = NDET_LAYOUT_CN, torch.empty_like(mean)
        src = mean
    else:
        src = mean.permute(1, 2, 3, 0)
        if not src.is_contiguous():
            return alpha_gate(mean.contiguous(), density, count)
        layout = NDET_LAYOUT_NC
        out = torch.empty_like(src).permute(3, 0, 1, 2)
    density = _f32c(density).reshape(-1)
    count = count.to(torch.int64).contiguous().reshape(-1)
    assert density.numel() == n and count.numel() == n
    check(_lib.load().ndet_alpha_gate(_ptr(src), _ptr(density), _ptr(count), _ptr(out), c, n, layout, _stream(mean)), "alpha_gate")
    return out


def posenc_concat(points: Tensor, global_feat: Optional[Tensor], pad_to: int = 0) -> Tensor:
    """Input rows of the sigma-MLP: ``[posenc_10(xyz) (63) | global_feat | zeros]`` (nerf_mlp.py:181-197,140).
    ``points`` (3,X,Y,Z) or (3,N); ``pad_to`` widens the rows with zero columns (K-step padding for the MFMA kernel)."""
    _need_gpu(points, global_feat)
    p = _f32c(points).reshape(3, -1)
    n = p.shape[1]
    f = 0
    if global_feat is not None:
        global_feat = _f32c(global_feat)
        assert global_feat.shape[0] == n
        f = global_feat.shape[1]
    width = max(63 + f, pad_to)
    out = torch.empty((n, width), dtype=torch.float32, device=p.device)
    check(_lib.load().ndet_posenc_concat(_ptr(p), _ptr(global_feat), n, f, width, _ptr(out), _stream(p)), "posenc_concat")
    return out


def sigma_head(h: Tensor, rows: Tensor, n_in: int, weight: Tensor, bias: Tensor, want_raw: bool = False):
    """alpha = 1 - exp(-relu(w . [h | rows[:, :n_in]] + b)) per row (nerf_mlp.py:86,143,227; nerfdet.py:257)."""
    _need_gpu(h, rows, weight, bias)
    assert h.is_contiguous() and rows.is_contiguous() and h.shape[0] == rows.shape[0]
    n, ch = h.shape
    w = _f32c(weight).reshape(-1)
    assert w.numel() == ch + n_in
    alpha = torch.empty((n,), dtype=torch.float32, device=h.device)
    raw = torch.empty((n,), dtype=torch.float32, device=h.device) if want_raw else None
    check(_lib.load().ndet_sigma_head(_ptr(h), ch, _ptr(rows), n_in, rows.shape[1], _ptr(w), _ptr(_f32c(bias)), n, _ptr(raw), _ptr(alpha),
                                      _stream(h)), "sigma_head")
    return (alpha, raw) if want_raw else alpha


def point_mlp_alpha(points: Tensor, global_feat: Optional[Tensor], layers, w_sigma: Tensor, b_sigma: Tensor, want_raw: bool = False,
                    want_h: bool = False):
    """The whole density MLP in one launch (csrc/point_mlp_kernels.hip): encoder + concat, four Linear + ReLU layers with the activations
    resident in LDS, sigma layer over [h | input], alpha.  nerf_mlp.py:80-90,138-144,181-197,224-227 + nerfdet.py:254-257.

    ``points`` (3,N) / (3,X,Y,Z); ``global_feat`` (N,F) or None; ``layers`` = 4 x (fp16-pair planes, 1 / scale, bias) of the hidden layers
    (conv3d.split_planes_f16 of conv3d.packed_linear, the first one padded to a multiple of 32 inputs).  Returns alpha (N) [, raw sigma (N)]
    [, trunk output (N, 256)]."""
    import ctypes
    _need_gpu(points, global_feat, w_sigma, b_sigma)
    pts = _f32c(points).reshape(3, -1)
    n = pts.shape[1]
    f = 0
    if global_feat is not None:
        global_feat = _f32c(global_feat)
        assert global_feat.shape[0] == n
        f = global_feat.shape[1]
    k0 = (63 + f + 31) // 32 * 32
    assert len(layers) == 4
    hidden = layers[0][2].numel()
    planes = (ctypes.c_void_p * 4)(*[l[0].data_ptr() for l in layers])
    winv = (ctypes.c_float * 4)(*[float(l[1]) for l in layers])
    biases = (ctypes.c_void_p * 4)(*[l[2].data_ptr() for l in layers])
    for i, (pl, _, b) in enumerate(layers):
        assert pl.numel() == (k0 if i == 0 else hidden) * 2 * hidden and b.numel() == hidden and b.dtype == torch.float32, "layer planes / bias of the wrong size"
    ws = _f32c(w_sigma).reshape(-1)
    assert ws.numel() == hidden + 63 + f
    alpha = torch.empty((n,), dtype=torch.float32, device=pts.device)
    raw = torch.empty((n,), dtype=torch.float32, device=pts.device) if want_raw else None
    h = torch.empty((n, hidden), dtype=torch.float32, device=pts.device) if want_h else None
    flops = 2 * n * (k0 * hidden + 3 * hidden * hidden + hidden + 63 + f)
    nbytes = 4 * (3 * n + f * n + n) + 2 * 2 * hidden * (k0 + 3 * hidden)
    trace.span("k_point_mlp/f16x2", lambda: check(
        _lib.load().ndet_point_mlp_alpha(_ptr(pts), _ptr(global_feat), n, f, k0, hidden, planes, winv, biases, _ptr(ws), _ptr(_f32c(b_sigma)),
                                         _ptr(raw), _ptr(alpha), _ptr(h), _stream(pts)), "point_mlp_alpha"),
        flops=flops, bytes=nbytes, kind="conv")
    out = (alpha,) + ((raw,) if want_raw else ()) + ((h,) if want_h else ())
    return out if len(out) > 1 else alpha
