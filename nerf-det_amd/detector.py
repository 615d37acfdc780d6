"""``nerfdet`` detector: mirror of mmdet3d/models/detectors/nerfdet.py:13-361 with the volumetric hot
path routed through the HIP kernels.  Same registry name, constructor keys, method names, batch-dict
keys and return structures, so ``configs/nerfdet/*.py`` build it unmodified."""
from __future__ import annotations

import torch
from torch import nn

from . import ops, trace
from .boxes import DepthInstance3DBoxes, bbox3d2result
from .pipeline import IMG_MEAN, IMG_STD
from .radiance_field import VanillaNeRFRadianceField
from .registry import DETECTORS, build_backbone, build_head, build_neck
from .volume import extract_volume, scene_geometry


class BaseDetector(nn.Module):
    """The slice of mmdet's BaseDetector the path uses: ``forward(return_loss=...)`` dispatch and
    ``train_step`` / ``_parse_losses``."""

    def init_weights(self, pretrained=None):
        pass

    def forward(self, img, img_metas, return_loss=True, **kwargs):
        if return_loss:
            return self.forward_train(img, img_metas, **kwargs)
        return self.forward_test(img, img_metas, **kwargs)

    @staticmethod
    def _parse_losses(losses, defer_log=False):
        """mmdet's BaseDetector._parse_losses.  ``defer_log``: the logged values stay device scalars (the caller reads them after it has
        queued backward and the optimizer step -- ``.item()`` here drains the launch queue between forward and backward)."""
        import torch.distributed as dist
        log = {}
        for k, v in losses.items():
            log[k] = v.mean() if isinstance(v, torch.Tensor) else sum(x.mean() for x in v)
        loss = sum(v for k, v in log.items() if "loss" in k)
        log["loss"] = loss
        out = {}
        for k, v in log.items():
            v = v.detach().clone()
            if dist.is_available() and dist.is_initialized():
                dist.all_reduce(v.div_(dist.get_world_size()))
            out[k] = v if defer_log else v.item()
        return loss, out

    def train_step(self, data, optimizer=None, defer_log=False):
        loss, log_vars = self._parse_losses(self(**data), defer_log)
        return dict(loss=loss, log_vars=log_vars, num_samples=len(data["img_metas"]))


@DETECTORS.register_module()
class nerfdet(BaseDetector):
    def __init__(self, backbone, neck, neck_3d, bbox_head, n_voxels, voxel_size, head_2d=None, train_cfg=None,
                 test_cfg=None, pretrained=None, aabb=None, near_far_range=None, N_samples=40, N_rand=4096,
                 depth_supervise=False, use_nerf_mask=True, nerf_sample_view=3, nerf_mode="volume", squeeze_scale=4,
                 rgb_supervision=True, nerf_density=False, render_testing=False):
        super().__init__()
        assert head_2d is None, "head_2d (SUN RGB-D layout head) is not used by any nerfdet config (nerfdet.py:46)"
        self.backbone = build_backbone(backbone)
        self.neck = build_neck(neck)
        self.neck_3d = build_neck(neck_3d)
        bbox_head = dict(bbox_head)
        bbox_head.update(train_cfg=train_cfg, test_cfg=test_cfg)
        self.bbox_head = build_head(bbox_head)
        self.bbox_head.voxel_size = voxel_size
        self.head_2d = None
        self.n_voxels, self.voxel_size = n_voxels, voxel_size
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.aabb, self.near_far_range = aabb, near_far_range
        self.N_samples, self.N_rand = N_samples, N_rand
        self.depth_supervise, self.use_nerf_mask, self.rgb_supervision = depth_supervise, use_nerf_mask, rgb_supervision
        self.squeeze_scale, self.nerf_mode = squeeze_scale, nerf_mode
        self.nerf_density, self.nerf_sample_view, self.render_testing = nerf_density, nerf_sample_view, render_testing
        c = neck["out_channels"]
        fd = c // squeeze_scale
        self.nerf_mlp = VanillaNeRFRadianceField(net_depth=4, net_width=256, skip_layer=3, feature_dim=fd + 6,
                                                 net_depth_condition=1, net_width_condition=128)
        # parameters the reference constructs but never uses in nerf_mode="image" (nerfdet.py:77-111): kept
        # so released checkpoints load key-for-key
        self.cov = nn.Sequential(nn.Conv3d(c, c, 3, padding=1), nn.ReLU(inplace=True), nn.Conv3d(c, c, 3, padding=1),
                                 nn.ReLU(inplace=True), nn.Conv3d(c, 1, 1))
        self.mean_mapping = nn.Sequential(nn.Conv3d(c, fd // 2, 1))
        self.cov_mapping = nn.Sequential(nn.Conv3d(c, fd // 2, 1))
        self.mapping = nn.Sequential(nn.Linear(c, fd // 2))
        self.mapping_2d = nn.Sequential(nn.Conv2d(c, fd // 2, 1))
        if hasattr(self.neck, "forward_hip") and "chain_linear" in self.neck.__dict__:
            # inference: the level-0 output convolution of the FPN projects its rows through self.mapping in the same launch (backbone.FPN.forward_hip);
            # through __dict__: the Linear must not become a submodule of the neck (state-dict keys)
            self.neck.__dict__["chain_linear"] = self.mapping[0]
        self.init_weights(pretrained=pretrained)
        # MI355X: 2D convs run channels-last (MIOpen NHWC), so FPN level 0 arrives in the layout the
        # gather kernels want; only FPN output 0 is consumed (nerfdet.py:142)
        self.backbone.to(memory_format=torch.channels_last)
        self.neck.to(memory_format=torch.channels_last)
        if hasattr(self.neck, "active_outs"):
            self.neck.active_outs = (0,)

    def init_weights(self, pretrained=None):
        super().init_weights(pretrained)
        self.backbone.init_weights(pretrained=pretrained)
        self.neck.init_weights()
        self.neck_3d.init_weights()
        self.bbox_head.init_weights()

    # ---------------------------------------------------------------------------------------
    def extract_2d(self, img):
        """(B,n_v,3,H,W) -> FPN level 0 (B,n_v,C,H/4,W/4), channels-last memory (nerfdet.py:134-147)."""
        b = img.shape[0]
        x = img.reshape([-1] + list(img.shape)[2:])       # the stem kernel reads the images in the layout they arrive in
        x = self.neck(self.backbone(x))[0]
        stride = img.shape[-1] / x.shape[-1]
        assert stride == 4
        return x, b, int(stride)

    def extract_feat(self, img, img_metas, mode, depth=None, ray_batch=None):
        """Same contract as nerfdet.py:133-269: returns (neck_3d outputs, valids, features_2d, rgb_preds, densitys).
        ``depth`` (B, n_v, Hd, Wd) float32 / float64, in metres (the loader's ``depth`` key): every backprojection is depth-gated
        (nerfdet.py:136-139, 164-169, 204-210, 404-411)."""
        if depth is not None:
            assert depth.shape[0] == img.shape[0], "depth and img must hold the same scenes (nerfdet.py:137)"
            depth = depth.reshape([-1] + list(depth.shape)[2:])
        assert ray_batch is not None and self.nerf_density and self.nerf_mode == "image", \
            "effective contract of the reference: use_ray=True, nerf_density=True, nerf_mode='image' (SURVEY.md 0.2)"
        trace.mark("begin")
        draws = begun = None
        if mode == "train":
            from . import rays
            from .rays import begin_selection, collect_draw, submit_draw
            begun = begin_selection(ray_batch)       # (reads one count back unless the loader supplied depth_rays)
            if begun is not None and rays.THREADED_DRAW:      # the permutation on a worker thread beside the backbone's launches
                draws = [submit_draw(begun, self.N_rand) for _ in img_metas]
        x, batch, stride = self.extract_2d(img)
        trace.mark("backbone_fpn")
        if begun is not None and draws is None:
            # the reference's host-side ray draw (a numpy permutation of every ray with depth: ~5 ms) once the backbone is queued: the device works
            # through that queue meanwhile; one draw per scene, in scene order, as render_ray.py:398 consumes its RandomState
            draws = [submit_draw(begun, self.N_rand) for _ in img_metas]
        # per-scene constants: host arithmetic while the GPU works through the backbone queue, asynchronous upload
        geoms = None
        if not torch.is_grad_enabled():
            geoms = [scene_geometry(m, self.n_voxels, self.voxel_size, stride, img.device) for m in img_metas]
        n_v = x.shape[0] // batch
        f2d = getattr(x, "_ndet_feature_2d", None)        # the mapped map, when the FPN's output convolution produced it on the way (inference)
        denorm = ray_batch["denorm_images"]
        volumes, valids, rgb_preds = [], [], []
        for b, img_meta in enumerate(img_metas):
            feat = x[b * n_v:(b + 1) * n_v]
            dn = denorm.reshape([-1] + list(denorm.shape)[2:])
            # channels-last volume straight into the MFMA convolutions of the 3D neck (inference and training alike)
            hf, wf = img_meta["img_shape"][0] // stride, img_meta["img_shape"][1] // stride
            # the keyword only when there is depth: callers that stand in for extract_volume keep the ungated signature
            gated = {} if depth is None else dict(depth=depth[b * n_v:(b + 1) * n_v])
            out = extract_volume(feat, dn, img_meta, self.n_voxels, self.voxel_size, self.mapping, self.nerf_mlp,
                                 stride=stride, channels_last_out=True,
                                 feature_2d=None if (f2d is None or torch.is_grad_enabled()) else f2d[b * n_v:(b + 1) * n_v, :, :hf, :wf],
                                 geometry=None if geoms is None else geoms[b], **gated)
            if mode == "train" or self.render_testing:
                from .rays import render_rays
                rgb_preds.append(render_rays(ray_batch, None, None, out["feature_2d"], dn, self.aabb, self.near_far_range,
                                             self.N_samples, self.N_rand, self.nerf_mlp, img_meta, None, self.nerf_mode,
                                             self.nerf_sample_view, is_train=(mode == "train"),
                                             render_testing=self.render_testing, selection=None if draws is None else collect_draw(draws[b])))
            else:
                rgb_preds.append(None)  # render_ray.py:518-519
            volumes.append(out["volume"])
            valids.append(out["valid"])
        x3 = volumes[0].unsqueeze(0) if len(volumes) == 1 else torch.stack(volumes)
        valids = valids[0].unsqueeze(0) if len(valids) == 1 else torch.stack(valids)
        trace.mark("volumetric_hot_path")
        x3 = self.neck_3d(x3)
        trace.mark("neck3d")
        return x3, valids, None, rgb_preds, []

    @staticmethod
    def _ray_batch(kwargs):
        rb = {}
        if "raydirs" in kwargs:
            rb = dict(ray_o=kwargs["lightpos"], ray_d=kwargs["raydirs"], gt_rgb=kwargs["gt_images"],
                      gt_depth=kwargs["gt_depths"], nerf_sizes=kwargs["nerf_sizes"], denorm_images=kwargs["denorm_images"])
            if kwargs.get("depth_rays") is not None:
                rb["depth_rays"] = kwargs["depth_rays"]          # the loader's nonzero(gt_depths > 0) (datasets.py): no host sync for the ray draw
        return rb

    def forward_train(self, img, img_metas, gt_bboxes_3d, gt_labels_3d, **kwargs):
        rb = self._ray_batch(kwargs)
        x, valids, _, rgb_preds, _ = self.extract_feat(img, img_metas, "train", ray_batch=rb or None)
        losses = self.bbox_head.forward_train(x, valids.float(), img_metas, gt_bboxes_3d, gt_labels_3d)
        if rb and self.rgb_supervision:
            losses.update(self.nvs_loss_func(rgb_preds))
        if self.depth_supervise:
            losses.update(self.depth_loss_func(rgb_preds))
        return losses

    def nvs_loss_func(self, rgb_pred):
        loss = 0
        for ret in rgb_pred:
            rgb, gt, m = ret["outputs_coarse"]["rgb"], ret["gt_rgb"], ret["outputs_coarse"]["mask"]
            loss = loss + (torch.sum(m.unsqueeze(-1) * (rgb - gt) ** 2) / (m.sum() + 1e-6) if self.use_nerf_mask
                           else torch.mean((rgb - gt) ** 2))
        return dict(loss_nvs=loss)

    def depth_loss_func(self, rgb_pred):
        loss = 0
        for ret in rgb_pred:
            d, gt, m = ret["outputs_coarse"]["depth"], ret["gt_depth"].squeeze(-1), ret["outputs_coarse"]["mask"]
            loss = loss + (torch.sum(m * torch.abs(d - gt)) / (m.sum() + 1e-6) if self.use_nerf_mask
                           else torch.mean(torch.abs(d - gt)))
        return dict(loss_depth=loss)

    def forward_test(self, img, img_metas, **kwargs):
        rb = self._ray_batch(kwargs)
        return self.simple_test(img, img_metas, ray_batch=rb or None)

    def _repeat_exact(self, img, img_metas, depth, ray_batch, evaluate_nerf):
        """A scene whose range-guard word came back set (a fp16-pair launch saw max|in| * ||w||_1 * 2^-39 above conv3d.GUARD_TOL: its per-tensor
        scale left part of a tensor with an absolute error that could show): once more on the six-product bf16x3 arithmetic, whose operands are
        exact whatever their range."""
        from . import conv3d
        conv3d.guard_trips += 1
        prev = conv3d.set_arithmetic("bf16x3")
        try:
            return self.simple_test(img, img_metas, depth, ray_batch, evaluate_nerf, defer=False)
        finally:
            conv3d.set_arithmetic(prev)

    def simple_test(self, img, img_metas, depth=None, ray_batch=None, evaluate_nerf=False, defer=False):
        from . import conv3d
        guarded = conv3d.ARITHMETIC == "f16x2" and img.is_cuda
        if guarded:
            conv3d.guard_begin(img.device)
        x, valids, _, rgb_preds, _ = self.extract_feat(img, img_metas, "test", depth, ray_batch)
        if evaluate_nerf:
            # nerfdet.py:342-343 computes (psnr, ssim, rmse) with save_rendered_img and drops them; kept here for the caller, without the PNGs
            from .rays import rendering_metrics
            assert rgb_preds and rgb_preds[-1] is not None, "evaluate_nerf needs render_testing=True (render_ray.py:452-517)"
            self.render_metrics = rendering_metrics(rgb_preds[-1])
        return self._detect_tail(x, valids, img_metas, defer, guarded, img.device,
                                 lambda: self._repeat_exact(img, img_metas, depth, ray_batch, evaluate_nerf))

    def _detect_tail(self, x, valids, img_metas, defer, guarded, device, repeat, raws=None):
        """neck_3d outputs -> detections (nerfdet.py:292-311), shared by simple_test and streaming.SceneStream.detect: the fused head with its
        single device-to-host copy where it applies.  ``guarded``: a set range-guard word calls ``repeat()`` for the answer instead.  ``raws``: the
        scene's head convolutions when a batched launch has computed them already (streaming.SceneGroup.detect(batched=True)); the tail then
        starts behind them."""
        from . import conv3d
        for m in img_metas:
            m.setdefault("box_type_3d", DepthInstance3DBoxes)
        if hasattr(self.bbox_head, "can_fuse") and self.bbox_head.can_fuse(x) and len(img_metas) == 1:
            bbox_list = self.bbox_head.simple_test_fused(x, valids.float(), img_metas, defer=defer, raws=raws)
        else:
            outs = self.bbox_head(x) if raws is None else self.bbox_head.outputs_from_raws(raws)
            bbox_list = self.bbox_head.get_bboxes(*outs, valids.float(), img_metas)
            if defer:
                ready = bbox_list
                bbox_list = lambda: ready
        if defer:
            pending = bbox_list

            def finish():
                got = pending()
                if guarded and getattr(got, "range_guard", False):
                    return repeat()
                return [bbox3d2result(b, s, l) for b, s, l in got]
            return finish
        if guarded and (getattr(bbox_list, "range_guard", False) or (not hasattr(bbox_list, "range_guard") and conv3d.guard_tripped(device))):
            return repeat()
        res = [bbox3d2result(b, s, l) for b, s, l in bbox_list]
        trace.mark("head_nms")
        return res

    def begin_scene(self, img_meta, window=None, keep_views=False, mean=IMG_MEAN, std=IMG_STD, carve=None, cloud=None):
        """A :class:`~nerfdet_amd.streaming.SceneStream` for one scene whose views arrive in chunks: ``add_views`` runs the backbone on a
        chunk and folds it into the scene's running sums, ``detect`` returns what :meth:`simple_test` returns for the views so far.  ``window=S`` keeps
        the last S chunks only (a sliding window; ``drop_oldest`` forgets chunks explicitly).  ``keep_views=True`` also keeps the views' mapped maps,
        images and cameras, so that ``scene.render_rays`` / ``scene.render`` render novel views from the views held.  ``scene.add_frames(frames, img_meta)``
        takes frames at capture resolution instead (uint8 BGR on the device; ``img_meta`` as pipeline.frame_meta makes it) and resizes, normalises
        with the img-norm ``mean`` / ``std`` given here (RGB; default: the configs') and pads them in one launch before ``add_views``.
        ``carve``: None (the default: every launch and every bit as without the keyword), True or ``dict(refine=2, band=None)``: the scene
        also counts, per voxel of a lattice ``refine`` (1, 2, 4) times finer than the detection one, how many of the depth frames it is
        given saw the voxel free and how many saw it on a surface (``band``: None = ``voxel_size[2]``, fixed for the scene's life), so that
        ``scene.occupancy(source="depth")`` and ``skip_empty=dict(source="depth")`` carve free space from the sensor.
        ``cloud``: None (the default: every launch and every bit as without the keyword), True or ``dict(refine=2, max_depth=None)``: the
        scene also keeps, per voxel of such a fine lattice, integer sums of the depth pixels that fell into it (those with
        ``0 < d <= max_depth`` metres), so that ``scene.points()`` returns a coloured, voxel-downsampled point cloud of the chunks held and
        labels it with a ``detect()`` result.  Independent of ``carve`` and of ``keep_views``.  Bad knobs: ValueError,
        before any device work."""
        from .streaming import SceneStream
        return SceneStream(self, img_meta, window=window, keep_views=keep_views, mean=mean, std=std, carve=carve, cloud=cloud)

    def begin_scenes(self, img_metas, window=None, keep_views=False, mean=IMG_MEAN, std=IMG_STD, carve=None, cloud=None):
        """A :class:`~nerfdet_amd.streaming.SceneGroup` for 1 .. 64 scenes streamed together, each with its own intrinsic, origin and extrinsics
        (``img_shape``, ``ori_shape``, the voxel grid and the detector are shared): ``group.add_views(img, denorm, metas, scenes=None)`` runs the
        backbone once over one chunk of k views per listed scene and folds them into the scenes' states with one grouped accumulate;
        ``group.detect(scenes=None)`` returns, per listed scene, what ``begin_scene(...).detect()[0]`` returns.  ``window=S`` (1 .. 64) gives
        every scene a sliding window of its last S chunks, as ``begin_scene(img_meta, window=S)`` gives one scene: each listed scene's chunk
        fills a state of its own, scenes evict independently (``group.drop_oldest(k, scenes)`` forgets chunks explicitly), and ``detect``
        finishes the listed windows with two grouped ring finishes.  ``keep_views=True`` gives every scene a view bank that follows its
        states (``group.banks``): ``group.render_rays(ray_o, ray_d, scenes=None, batched=False)`` / ``group.render(ray_batches, ...)`` then
        render novel views of the listed scenes with one grouped sampler launch per pass, each scene bit for bit what
        ``begin_scene(..., keep_views=True)`` renders from the same maps.  ``group.add_frames(frames, metas, scenes=None)`` takes capture-resolution
        frames (len(scenes), k, Hs, Ws, 3) instead and prepares all of them in one launch with ``mean`` / ``std``, as ``begin_scene`` describes.
        ``carve`` as in :meth:`begin_scene`, one ``refine`` and ``band`` for the group: every scene gets counter segments of its own that follow
        its states (one k_carve_accumulate launch per listed scene and call).  ``cloud`` as in :meth:`begin_scene`, one ``refine`` and
        ``max_depth`` for the group: every scene gets record segments of its own (one k_cloud_accumulate launch per listed scene and call),
        read by ``group.points(scenes=)``.  One image size and grid per group, inference only, not graphed."""
        from .streaming import SceneGroup
        return SceneGroup(self, img_metas, window=window, keep_views=keep_views, mean=mean, std=std, carve=carve, cloud=cloud)

    def forward_test_async(self, img, img_metas, **kwargs):
        """Serving form of :meth:`forward_test`: every launch of the scene is queued on the current stream and a ``finish()`` callable is
        returned; ``finish()`` waits for the scene's single device-to-host copy and returns what ``forward_test`` returns.  Two scenes in
        flight on two streams keep the queue full across the step boundary and let one scene's small late layers share the chip with the
        other's backbone (bench.py reports that throughput next to the sequential one)."""
        rb = self._ray_batch(kwargs)
        return self.simple_test(img, img_metas, ray_batch=rb or None, defer=True)

    def aug_test(self, imgs, img_metas):
        pass

    def show_results(self, *args, **kwargs):
        pass

    @staticmethod
    def _compute_projection(img_meta, stride, angles=None):
        assert angles is None
        return ops.compute_projection(img_meta, stride)
