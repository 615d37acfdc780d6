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

Inference only: no training / autograd, no hipGraph replay, one scene per stream; whole chunks are dropped, not single views out of one.
Without ``keep_views`` there is no ray branch (rendering needs every view's map).
"""
from __future__ import annotations

from collections import OrderedDict
from typing import List, Optional

import numpy as np
import torch

from . import conv3d, ops
from .volume import map_features_2d, map_features_2d_hip

Tensor = torch.Tensor


class SceneStream:
    """One scene of a :class:`~nerfdet_amd.detector.nerfdet` detector, filled chunk by chunk (:meth:`add_views`) and detected at any time
    (:meth:`detect`).  ``img_meta`` fixes the scene: ``lidar2img.intrinsic``, ``lidar2img.origin``, ``img_shape`` and ``ori_shape``; its
    extrinsics are not used (each chunk brings its own).  ``window``: None, or the number of chunks kept (1 .. ops.RING_MAX): the
    stream then holds one state per ``add_views`` call and forgets the oldest when a chunk arrives at a full window.  ``keep_views``: also
    keep the views' mapped maps, images and cameras (``bank``, a rays.ViewBank) so that :meth:`render_rays` / :meth:`render` work."""

    bank = None     # rays.ViewBank with keep_views, else None

    def __init__(self, det, img_meta: dict, window: Optional[int] = None, keep_views: bool = False):
        if not isinstance(keep_views, bool):
            raise ValueError(f"keep_views must be a bool, got {keep_views!r}")
        if window is not None and (isinstance(window, bool) or not isinstance(window, int) or not 1 <= window <= ops.RING_MAX):
            raise ValueError(f"window must be None or an int in 1 .. {ops.RING_MAX}, got {window!r}")
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
        self.points = ops.get_points(det.n_voxels, det.voxel_size, img_meta["lidar2img"]["origin"], self.device)
        if keep_views:
            from .rays import ViewBank
            self.bank = ViewBank()

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

    def reset(self) -> None:
        """Forget every view: the scene starts empty again."""
        if self.window is None:
            self.state.reset()
            if self.bank is not None:
                self.bank.clear()
        else:
            self.drop_oldest(len(self._segs))

    def drop_oldest(self, k: int = 1) -> None:
        """Forget the k oldest chunks of a windowed stream (their states are zeroed and kept for the chunks to come)."""
        if self.window is None:
            raise ValueError("drop_oldest needs a windowed stream: begin_scene(img_meta, window=S)")
        if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k <= len(self._segs):
            raise ValueError(f"drop_oldest: k={k!r} for {len(self._segs)} chunks held")
        for st in self._segs[:k]:
            st.reset()
            self._spare.append(st)
        del self._segs[:k]
        if self.bank is not None:
            self.bank.drop_oldest(k)

    def _accumulate(self, *chunk, depth_gate=None, banked=None) -> None:
        """Fold a chunk into the scene's state, or in a window into an empty state that joins the window once it is filled; only then does
        the oldest chunk leave a full window.  A chunk that fails leaves the window as it was (its state goes back, zeroed).  ``banked``:
        the chunk's view-bank segment, made by the caller (rays.ViewBank.make_segment changes nothing); it joins the bank once the
        states have taken the chunk, so states and bank hold the same chunks."""
        if self.window is None:
            ops.scene_accumulate(self.state, *chunk, depth_gate=depth_gate)
            if banked is not None:
                self.bank.push(banked)
            return
        lin = self._lin
        # a sliding window therefore owns S + 1 states: the chunk that leaves hands its (zeroed) state to the chunk after the next
        st = self._spare.pop() if self._spare else ops.SceneState(self.det.n_voxels, lin.in_features, lin.out_features, self.device)
        try:
            ops.scene_accumulate(st, *chunk, depth_gate=depth_gate)
        except BaseException:
            st.reset()
            self._spare.append(st)
            raise
        if len(self._segs) == self.window:
            self.drop_oldest(1)
        self._segs.append(st)
        if banked is not None:
            self.bank.push(banked)

    def _check_meta(self, img_meta: dict, k: int) -> None:
        a, b = self.meta, img_meta
        for key in ("intrinsic", "origin"):
            if not np.array_equal(np.asarray(a["lidar2img"][key], dtype=np.float64), np.asarray(b["lidar2img"][key], dtype=np.float64)):
                raise ValueError(f"add_views: the chunk's lidar2img.{key} differs from the scene's")
        for key in ("img_shape", "ori_shape"):
            if tuple(a[key]) != tuple(b[key]):
                raise ValueError(f"add_views: the chunk's {key} {tuple(b[key])} differs from the scene's {tuple(a[key])}")
        if len(b["lidar2img"]["extrinsic"]) != k:
            raise ValueError(f"add_views: {len(b['lidar2img']['extrinsic'])} extrinsics for {k} views")

    def _features(self, img: Tensor):
        x, _, stride = self.det.extract_2d(img)
        return x, getattr(x, "_ndet_feature_2d", None), stride

    def add_views(self, img: Tensor, denorm_images: Tensor, img_meta: dict, depth: Optional[Tensor] = None) -> None:
        """Fold k >= 1 views into the scene.  ``img``, ``denorm_images`` (1, k, 3, H, W); ``img_meta`` the chunk's (its ``extrinsic`` list has
        k entries; the rest must equal the scene's, else ValueError); ``depth`` None or (1, k, Hd, Wd) float32 / float64: the chunk's views are
        depth-gated as by ``simple_test(depth=)`` (nerfdet.py:404-411).

        Range guard of the fp16-pair arithmetic: the guard word is cleared before the chunk's backbone and read back before the chunk enters
        the state -- one 4-byte device-to-host read (a synchronisation) per chunk.  A tripped chunk is redone on bf16x3 first
        (``conv3d.guard_trips`` counts it), so no tripped chunk reaches the state."""
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
        with torch.no_grad():
            guarded = conv3d.ARITHMETIC == "f16x2" and img.is_cuda
            if guarded:
                conv3d.guard_begin(img.device)
            x, f2d, stride = self._features(img)
            if guarded and conv3d.guard_tripped(img.device):
                conv3d.guard_trips += 1
                prev = conv3d.set_arithmetic("bf16x3")
                try:
                    x, f2d, stride = self._features(img)
                finally:
                    conv3d.set_arithmetic(prev)
            hh, ww = self.meta["img_shape"][0], self.meta["img_shape"][1]
            h, w = hh // stride, ww // stride
            feat = ops.to_channels_last(x)[:, :, :h, :w]
            lin = self._lin
            if f2d is not None:
                mapped = f2d[:, :, :h, :w]
            elif lin.in_features % 32 == 0:
                mapped = map_features_2d_hip(feat, lin)
            else:
                mapped = map_features_2d(feat, lin.weight, lin.bias)
            rgb = denorm_images[0][:, :, :hh, :ww]
            gate = None
            if depth is not None:
                gate = ops.depth_gate(depth[0].to(self.device, non_blocking=True), self.det.voxel_size, (h, w), (hh, ww))
            proj = ops.compute_projection(img_meta, stride, self.device)
            rgb_proj = ops.compute_projection(img_meta, 1, self.device)
            # the bank takes the mapped map as it is accumulated and the images as extract_feat hands them to render_rays (uncropped)
            banked = None if self.bank is None else self.bank.make_segment(mapped, denorm_images[0], img_meta)
            self._accumulate(feat, mapped, lin.bias, rgb, self.points, proj, rgb_proj, depth_gate=gate, banked=banked)

    def _need_bank(self, what: str):
        bank = self.bank
        if bank is None:
            raise RuntimeError(f"{what} needs the scene's views: begin_scene(img_meta, keep_views=True)")
        if bank.n_views == 0:
            raise RuntimeError("the scene has no views yet: call add_views first")
        return bank

    def _render(self, ray_o: Tensor, ray_d: Tensor, step: int):
        """render_ray.py:250-327 (``det=True``, mode 'image') over the bank, ``step`` rays per pass."""
        from . import rays
        bank = self._need_bank("rendering")
        det = self.det
        rgbs, depths, masks = [], [], []
        with torch.no_grad():
            for i in range(0, ray_o.shape[0], step):
                o, d = ray_o[i:i + step], ray_d[i:i + step]
                pts, z_vals = rays.sample_along_camera_ray(o, d, det.near_far_range, det.N_samples, det=True)
                globalfeat, pixel_mask, _ = rays.ray_view_stats_bank(pts, bank)
                rgb_pts, density_pts = det.nerf_mlp(pts, d, globalfeat)
                out = rays.raw2outputs(torch.cat([rgb_pts, density_pts], dim=-1), z_vals, pixel_mask)
                rgbs.append(out["rgb"])
                depths.append(out["depth"])
                masks.append(out["mask"])
        return torch.cat(rgbs, dim=0), torch.cat(depths, dim=0), torch.cat(masks, dim=0)

    def render_rays(self, ray_o: Tensor, ray_d: Tensor):
        """Render rays ``ray_o``, ``ray_d`` (R,3) against the views held: ``dict(rgb (R,3), depth (R,), mask (R,) bool)``, what
        ``rays.render_rays_func(det=True)`` composites (render_ray.py:250-327) with the detector's ``near_far_range`` and ``N_samples``,
        ``rays.RENDER_TESTING_RAYS`` rays per pass.  Needs ``keep_views=True`` and at least one view (else RuntimeError)."""
        from . import rays
        self._need_bank("render_rays")
        if ray_o.dim() != 2 or ray_o.shape[1] != 3 or ray_d.shape != ray_o.shape:
            raise ValueError(f"render_rays takes (R,3) origins and directions, got {tuple(ray_o.shape)} and {tuple(ray_d.shape)}")
        rgb, depth, mask = self._render(ray_o, ray_d, rays.RENDER_TESTING_RAYS)
        return OrderedDict([("rgb", rgb), ("depth", depth), ("mask", mask)])

    def render(self, ray_batch: dict):
        """Every ray of the ray batch's target views, as ``rays.render_rays(render_testing=True)`` returns them (render_ray.py:452-517):
        ``outputs_coarse.rgb`` (T,h,w,3), ``outputs_coarse.depth`` (T,h,w,1), ``gt_rgb``, ``gt_depth`` -- ``rays.rendering_metrics`` applies."""
        from . import rays
        self._need_bank("render")
        ray_o, ray_d, gt_rgb, gt_depth = ray_batch["ray_o"], ray_batch["ray_d"], ray_batch["gt_rgb"], ray_batch["gt_depth"]
        nerf_size = ray_batch["nerf_sizes"][0]
        view_num = ray_o.shape[1]
        hh, ww = int(nerf_size[0][0]), int(nerf_size[0][1])
        ray_o, ray_d, gt_rgb = ray_o.view(-1, 3), ray_d.view(-1, 3), gt_rgb.view(-1, 3)
        gt_depth = gt_depth.view(-1, 1) if len(gt_depth) != 0 else None
        assert view_num * hh * ww == ray_o.shape[0]  # render_ray.py:468
        n_rand = self.det.N_rand
        step = n_rand * max(1, rays.RENDER_TESTING_RAYS // n_rand)       # the passes of rays.render_rays
        rgb, depth, _ = self._render(ray_o, ray_d, step)
        return {"outputs_coarse": {"rgb": rgb.view(view_num, hh, ww, 3), "depth": depth.view(view_num, hh, ww, 1)},
                "gt_rgb": gt_rgb.view(view_num, hh, ww, 3),
                "gt_depth": gt_depth.view(view_num, hh, ww, 1) if gt_depth is not None else None}

    def volume(self):
        """``(volume (C,X,Y,Z), valid (1,X,Y,Z) int64)`` of the views so far: K2-finish -> sigma-MLP -> K1-finish, what ``extract_volume``
        returns for them (channels-last memory)."""
        if self.n_views == 0:
            raise RuntimeError("the scene has no views yet: call add_views first")
        ring = self.window is not None
        with torch.no_grad():
            glob = ops.density_finish_ring(self._segs, self._lin.bias) if ring else ops.density_finish(self.state, self._lin.bias)
            mlp = self.det.nerf_mlp
            if hasattr(mlp, "hip_trunk_ok") and mlp.hip_trunk_ok():
                alpha = mlp.alpha_from_points(self.points, glob)
            else:
                alpha = ops.sigma_to_alpha(mlp.raw_sigma_from_rows(ops.posenc_concat(self.points, glob)))
            return ops.volume_finish_ring(self._segs, alpha) if ring else ops.volume_finish(self.state, alpha)

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
        conv3d.guard_trips += 1
        prev = conv3d.set_arithmetic("bf16x3")
        try:
            with torch.no_grad():
                x = self.det.neck_3d(vol.unsqueeze(0))
                return self.det._detect_tail(x, valid.unsqueeze(0), metas, False, False, vol.device, None)
        finally:
            conv3d.set_arithmetic(prev)
