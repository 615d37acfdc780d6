"""A14 / A16: ``ScanNetImVoxelHeadV2`` mirror (mmdet3d/models/dense_heads/imvoxel_head_v2.py:12-300,
442-566): FCOS-style anchor-free 3D head over the three neck levels.  Same constructor keys, state-dict
keys (``centerness_conv``, ``reg_conv``, ``cls_conv``, ``scales.N.scale``) and outputs.

Inference post-processing runs on the GPU: lattice points from the HIP ``get_points`` kernel, greedy NMS
from csrc/nms_kernels.hip (identical pick order to the reference's Python loop)."""
from __future__ import annotations

import math
from typing import List

import torch
from torch import nn

from . import losses  # noqa: F401  (registers the loss types the head builds)
from . import ops
from .conv3d import carry_amax, conv3d_ndhwc, guard_tripped, guard_word, packed, to_ndhwc
from .nms import aligned_3d_nms
from .registry import HEADS, build_loss
from ._lib import raw_stream


class Scale(nn.Module):
    """mmcv.cnn.Scale: learnable scalar multiply."""

    def __init__(self, scale: float = 1.0):
        super().__init__()
        self.scale = nn.Parameter(torch.tensor(scale, dtype=torch.float))

    def forward(self, x):
        return x * self.scale


class Detections(list):
    """``[(boxes, scores, labels)]`` of one scene plus the scene's range-guard word (conv3d.guard_word): True when a fp16-pair launch of the
    scene reported an absolute error floor above conv3d.GUARD_TOL -- the detector repeats such a scene on the bf16x3 arithmetic."""
    range_guard = False


def compute_centerness(t):
    """imvoxel_head_v2.py:558-566: sqrt of the product of min/max ratios per axis."""
    x, y, z = t[..., 0:2], t[..., 2:4], t[..., 4:6]      # slices: a list index builds its index tensor on the host and copies it over (a blocking pageable copy each)
    c = x.min(dim=-1)[0] / x.max(dim=-1)[0] * y.min(dim=-1)[0] / y.max(dim=-1)[0] * z.min(dim=-1)[0] / z.max(dim=-1)[0]
    return torch.sqrt(c)


def _dist_to_box(points, d):
    """(x-,x+,y-,y+,z-,z+) distances from `points` -> (x1,y1,z1,x2,y2,z2).  imvoxel_head_v2.py:547-555."""
    return torch.stack([points[:, 0] - d[:, 0], points[:, 1] - d[:, 2], points[:, 2] - d[:, 4],
                        points[:, 0] + d[:, 1], points[:, 1] + d[:, 3], points[:, 2] + d[:, 5]], -1)


@HEADS.register_module()
class ScanNetImVoxelHeadV2(nn.Module):
    def __init__(self, n_classes, n_channels, n_reg_outs, n_scales, limit, centerness_topk=-1,
                 loss_centerness=dict(type="CrossEntropyLoss", use_sigmoid=True, loss_weight=1.0),
                 loss_bbox=dict(type="AxisAlignedIoULoss", loss_weight=1.0),
                 loss_cls=dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
                 train_cfg=None, test_cfg=None):
        super().__init__()
        self.n_classes, self.n_scales, self.limit, self.centerness_topk = n_classes, n_scales, limit, centerness_topk
        self.loss_centerness = build_loss(loss_centerness)
        self.loss_bbox = build_loss(loss_bbox)
        self.loss_cls = build_loss(loss_cls)
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.voxel_size = None  # set by the detector (nerfdet.py:45)
        self.centerness_conv = nn.Conv3d(n_channels, 1, 3, padding=1, bias=False)
        self.reg_conv = nn.Conv3d(n_channels, n_reg_outs, 3, padding=1, bias=False)
        self.cls_conv = nn.Conv3d(n_channels, n_classes, 3, padding=1)
        self.scales = nn.ModuleList([Scale(1.0) for _ in range(n_scales)])

    def init_weights(self):
        """N(0, .01) weights, class bias = -log((1-p)/p) at p = .01 (imvoxel_head_v2.py:52-55)."""
        for m in (self.centerness_conv, self.reg_conv, self.cls_conv):
            nn.init.normal_(m.weight, 0.0, 0.01)
        nn.init.constant_(self.cls_conv.bias, float(-math.log((1 - 0.01) / 0.01)))

    # ---- forward ---------------------------------------------------------------------------
    def forward_single(self, x, scale):
        if x.is_cuda and not self.training and not torch.is_grad_enabled() and x.shape[1] % 32 == 0:
            return self.forward_single_hip(x, scale)
        if x.is_cuda and torch.is_grad_enabled():   # training: the three layers as one convolution on the MFMA kernels (conv_train.py)
            from .conv_train import conv_forward_shared
            ctr, reg, cls = conv_forward_shared([self.centerness_conv, self.reg_conv, self.cls_conv], x)
            return ctr, torch.exp(scale(reg)), cls
        return self.centerness_conv(x), torch.exp(scale(self.reg_conv(x))), self.cls_conv(x)

    def forward_single_hip(self, x, scale):
        """The three 3x3x3 convs share their input: one MFMA conv with Cout = 1 + n_reg + n_classes (cls bias in the
        epilogue shift), then channel views.  imvoxel_head_v2.py:444-449."""
        pk = packed([self.centerness_conv, self.reg_conv, self.cls_conv])
        n_reg = self.reg_conv.out_channels
        one = x.shape[0] == 1      # a batch of one: x[0] holds the same elements as x (the fp16-pair arithmetic's maximum carries over)
        outs = [conv3d_ndhwc(to_ndhwc(carry_amax(x, x[b]) if one else x[b].float()), pk, amax=False).permute(3, 0, 1, 2) for b in range(x.shape[0])]
        o = outs[0].unsqueeze(0) if len(outs) == 1 else torch.stack(outs)
        return o[:, :1], torch.exp(scale(o[:, 1:1 + n_reg])), o[:, 1 + n_reg:]

    def raws_batched(self, x):
        """Per level the fused ``centerness | reg | cls`` convolution of :meth:`forward_single_hip` over the WHOLE batch in one launch:
        x[l] (B,C,X,Y,Z), a view of channels-last memory -> (B,X,Y,Z,1 + n_reg + n_classes).  Scene b's contiguous slice ``raw[b]`` is what
        :meth:`simple_test_fused` (``raws=``) and :meth:`outputs_from_raws` take."""
        pk = packed([self.centerness_conv, self.reg_conv, self.cls_conv])
        raws = []
        for f in x:
            t = f.float().permute(0, 2, 3, 4, 1)
            raws.append(conv3d_ndhwc(carry_amax(f, t if t.is_contiguous() else t.contiguous()), pk, amax=False))
        return raws

    def outputs_from_raws(self, raws):
        """What :meth:`forward` returns for one scene, from that scene's precomputed per-level raws (X,Y,Z,1 + n_reg + n_classes)."""
        n_reg = self.reg_conv.out_channels
        outs = []
        for raw, scale in zip(raws, self.scales):
            o = raw.permute(3, 0, 1, 2).unsqueeze(0)
            outs.append((o[:, :1], torch.exp(scale(o[:, 1:1 + n_reg])), o[:, 1 + n_reg:]))
        return tuple(map(list, zip(*outs)))

    def forward(self, x):
        outs = [self.forward_single(f, s) for f, s in zip(x, self.scales)]
        return tuple(map(list, zip(*outs)))

    def forward_train(self, x, valid, img_metas, gt_bboxes, gt_labels):
        return self.loss(*(self(x) + (valid, img_metas, gt_bboxes, gt_labels)))

    @torch.no_grad()
    def get_points(self, featmap_sizes, origin, device):
        """Per-level lattice with voxel_size * 2^i (imvoxel_head_v2.py:205-214), (n_i, 3) each."""
        out = []
        for i, size in enumerate(featmap_sizes):
            vs = torch.tensor(self.voxel_size) * (2 ** i)
            out.append(ops.get_points(list(size), vs, origin, device).reshape(3, -1).transpose(0, 1))
        return out

    def _level_valids(self, centernesses, valid):
        return [nn.functional.interpolate(valid, size=x.shape[-3:], mode="trilinear").round().bool() for x in centernesses]

    # ---- inference -------------------------------------------------------------------------
    def get_bboxes(self, centernesses, bbox_preds, cls_scores, valid, img_metas):
        assert len(centernesses[0]) == len(bbox_preds[0]) == len(cls_scores[0]) == len(img_metas)
        valids = self._level_valids(centernesses, valid)
        res = []
        for b in range(len(img_metas)):
            res.append(self._get_bboxes_single([x[b].detach() for x in centernesses], [x[b].detach() for x in bbox_preds],
                                               [x[b].detach() for x in cls_scores], [x[b].detach() for x in valids],
                                               img_metas[b]))
        return res

    def _candidates(self, centernesses, bbox_preds, cls_scores, valids, img_meta):
        """Per-level sigmoid scores * centerness * valid, top ``nms_pre`` per level, decoded boxes
        (imvoxel_head_v2.py:248-282)."""
        sizes = [f.size()[-3:] for f in centernesses]
        pts_l = self.get_points(sizes, img_meta["lidar2img"]["origin"], centernesses[0].device)
        boxes, scores = [], []
        for ctr, reg, cls, val, pts in zip(centernesses, bbox_preds, cls_scores, valids, pts_l):
            ctr = ctr.permute(1, 2, 3, 0).reshape(-1).sigmoid()
            reg = reg.permute(1, 2, 3, 0).reshape(-1, reg.shape[0])
            sc = cls.permute(1, 2, 3, 0).reshape(-1, self.n_classes).sigmoid()
            sc = sc * ctr[:, None] * val.permute(1, 2, 3, 0).reshape(-1)[:, None]
            if len(sc) > self.test_cfg.nms_pre > 0:
                _, ids = sc.max(dim=1)[0].topk(self.test_cfg.nms_pre)
                reg, sc, pts = reg[ids], sc[ids], pts[ids]
            boxes.append(_dist_to_box(pts, reg))
            scores.append(sc)
        return torch.cat(boxes), torch.cat(scores)

    def _get_bboxes_single(self, centernesses, bbox_preds, cls_scores, valids, img_meta):
        boxes, scores = self._candidates(centernesses, bbox_preds, cls_scores, valids, img_meta)
        return self._nms(boxes, scores, img_meta)

    def _nms(self, bboxes, scores, img_meta):
        """class argmax, score threshold, greedy aligned NMS, corner -> (centre, size) (imvoxel_head_v2.py:528-545)."""
        scores, labels = scores.max(dim=1)
        ids = scores > self.test_cfg.score_thr
        bboxes, scores, labels = bboxes[ids], scores[ids], labels[ids]
        ids = aligned_3d_nms(bboxes, scores, labels, self.test_cfg.iou_thr)
        b = bboxes[ids]
        b = torch.stack(((b[:, 0] + b[:, 3]) / 2.0, (b[:, 1] + b[:, 4]) / 2.0, (b[:, 2] + b[:, 5]) / 2.0,
                         b[:, 3] - b[:, 0], b[:, 4] - b[:, 1], b[:, 5] - b[:, 2]), dim=1)
        b = img_meta["box_type_3d"](b, origin=(0.5, 0.5, 0.5), box_dim=6, with_yaw=False)
        return b, scores[ids], labels[ids]

    # ---- fused inference (HIP decode) ---------------------------------------------------------
    def can_fuse(self, x) -> bool:
        return (x[0].is_cuda and not self.training and not torch.is_grad_enabled() and x[0].shape[1] % 32 == 0
                and x[0].shape[0] == 1 and self.reg_conv.out_channels == 6)

    def simple_test_fused(self, x, valid, img_metas, defer=False, raws=None):
        """``raws``: the scene's per-level fused head convolutions (X,Y,Z,25) when the caller has run them already (:meth:`raws_batched`: one
        launch per level for several scenes); everything from the decode onward is this scene's as usual.

        ``defer=True``: everything is enqueued, the picks travel to a pinned host buffer asynchronously, and a ``finish()`` callable is
        returned that waits for that copy and builds the detections -- a server keeps a second scene's launches queued (on another
        stream) while this one drains.  Default: the detections themselves.

        forward + get_bboxes for one scene in a dozen launches: fused head conv -> level mask -> decode (best score, label,
        box per voxel; csrc/nms_kernels.hip::k_head_decode) -> one order-preserving ``score > thr`` compaction over all
        levels -> greedy NMS -> detections.  Same candidates as :meth:`get_bboxes` (imvoxel_head_v2.py:216-285,528-555):
        a level's top-``nms_pre`` cut only matters when more than ``nms_pre`` of its voxels clear the score threshold, and is
        then taken over the survivors.  More than four levels fall back to the generic library-op path below."""
        import ctypes
        import numpy as np
        from ctypes import c_void_p
        from . import _lib
        from ._lib import check, float3
        lib = _lib.load()
        meta = img_metas[0]
        pk = packed([self.centerness_conv, self.reg_conv, self.cls_conv])
        dev = x[0].device
        st = c_void_p(raw_stream(dev))
        gx0, gy0, gz0 = valid.shape[-3:]
        v0 = valid.reshape(gx0, gy0, gz0).float().contiguous()
        bests, labels, boxes = [], [], []
        if raws is None:
            raws = [conv3d_ndhwc(to_ndhwc(carry_amax(f, f[0]) if f.dtype == torch.float32 else f[0].float()), pk, amax=False) for f in x]  # (X,Y,Z,25) each
        grids = [tuple(r.shape[:3]) for r in raws]
        facs = [gx0 // g[0] for g in grids]
        org = np.float32(np.asarray(meta["lidar2img"]["origin"]))
        if len(raws) <= 4 and all(fc >= 1 and (fc == 1 or fc % 2 == 0) and (g[0] * fc, g[1] * fc, g[2] * fc) == (gx0, gy0, gz0) for fc, g in zip(facs, grids)):
            # every level's validity mask + decode in one launch (csrc/nms_kernels.hip::k_head_decode_levels)
            nlv = len(raws)
            for g in grids:
                n = g[0] * g[1] * g[2]
                bests.append(torch.empty((n,), dtype=torch.float32, device=dev))
                labels.append(torch.empty((n,), dtype=torch.int64, device=dev))
                boxes.append(torch.empty((n, 6), dtype=torch.float32, device=dev))
            vp = lambda ts: (ctypes.c_void_p * nlv)(*[t.data_ptr() for t in ts])
            vsz = np.concatenate([np.float32((torch.tensor(self.voxel_size) * (2 ** i)).tolist()) for i in range(nlv)]).astype(np.float32)
            check(lib.ndet_head_decode_levels(nlv, vp(raws), vp([sc.scale for sc in self.scales][:nlv]), (ctypes.c_int * (3 * nlv))(*[v for g in grids for v in g]),
                                              (ctypes.c_int * nlv)(*facs), vsz.ctypes.data_as(c_void_p), org.ctypes.data_as(c_void_p), self.n_classes,
                                              c_void_p(v0.data_ptr()), gx0, gy0, gz0, vp(bests), vp(labels), vp(boxes), st), "head_decode_levels")
        else:
            for i, (raw, sc) in enumerate(zip(raws, self.scales)):
                gx, gy, gz = raw.shape[:3]
                n = gx * gy * gz
                fac = facs[i]
                if fac >= 1 and (fac == 1 or fac % 2 == 0) and (gx * fac, gy * fac, gz * fac) == (gx0, gy0, gz0):
                    v = torch.empty((n,), dtype=torch.uint8, device=dev)
                    check(lib.ndet_level_valid(c_void_p(v0.data_ptr()), gx0, gy0, gz0, fac, c_void_p(v.data_ptr()), st), "level_valid")
                else:
                    v = nn.functional.interpolate(valid, size=(gx, gy, gz), mode="trilinear").round().bool().reshape(-1).contiguous()
                best = torch.empty((n,), dtype=torch.float32, device=dev)
                lab = torch.empty((n,), dtype=torch.int64, device=dev)
                box = torch.empty((n, 6), dtype=torch.float32, device=dev)
                vs = (torch.tensor(self.voxel_size) * (2 ** i)).tolist()
                check(lib.ndet_head_decode(c_void_p(raw.data_ptr()), self.n_classes, c_void_p(v.data_ptr()), c_void_p(sc.scale.data_ptr()),
                                           gx, gy, gz, float3(np.float32(vs)), float3(org),
                                           c_void_p(best.data_ptr()), c_void_p(lab.data_ptr()), c_void_p(box.data_ptr()), st), "head_decode")
                bests.append(best)
                labels.append(lab)
                boxes.append(box)
        nl = len(bests)
        if nl <= 4:
            sizes = [int(b.shape[0]) for b in bests]
            tot = sum(sizes)
            c_best = torch.empty((tot,), dtype=torch.float32, device=dev)
            c_lab = torch.empty((tot,), dtype=torch.int64, device=dev)
            c_box = torch.empty((tot, 6), dtype=torch.float32, device=dev)
            pa = lambda ts: (ctypes.c_void_p * nl)(*[t.data_ptr() for t in ts])
            counts = torch.empty((nl + 2,), dtype=torch.int32, device=dev)
            from .boxes import DepthInstance3DBoxes

            def general():
                # ---- general tail (more than 4096 candidates or 1024 picks, another box container): host-driven ----
                nonlocal c_best, c_lab, c_box
                check(lib.ndet_select_candidates(nl, pa(bests), pa(labels), pa(boxes), (ctypes.c_int * nl)(*sizes), float(self.test_cfg.score_thr),
                                                 c_void_p(c_best.data_ptr()), c_void_p(c_lab.data_ptr()), c_void_p(c_box.data_ptr()),
                                                 c_void_p(counts.data_ptr()), st), "select_candidates")
                cnt = counts.cpu().tolist()   # host sync 1 of 2
                pre = self.test_cfg.nms_pre
                n = cnt[nl]
                if pre > 0 and any(c > pre for c in cnt[:nl]):
                    # a level has more survivors than nms_pre: its top-nms_pre by score (all of them above the threshold, so the
                    # same set the reference's "top-k, then threshold" keeps); the other levels stay as compacted
                    pb, plab, pbox, off = [], [], [], 0
                    for c in cnt[:nl]:
                        sb, sl, sx = c_best[off:off + c], c_lab[off:off + c], c_box[off:off + c]
                        if c > pre:
                            sb, ids = sb.topk(pre)
                            sl, sx = sl[ids], sx[ids]
                        pb.append(sb); plab.append(sl); pbox.append(sx)
                        off += c
                    c_best, c_lab, c_box = torch.cat(pb), torch.cat(plab), torch.cat(pbox).contiguous()
                    n = int(c_best.shape[0])
                if n == 0:
                    b = meta["box_type_3d"](c_box[:0], origin=(0.5, 0.5, 0.5), box_dim=6, with_yaw=False)
                    return [(b, c_best[:0], c_lab[:0])]
                ids = aligned_3d_nms(c_box[:n], c_best[:n], c_lab[:n], self.test_cfg.iou_thr)   # host sync 2
                k = int(ids.shape[0])
                o_box = torch.empty((k, 6), dtype=torch.float32, device=dev)
                o_sc = torch.empty((k,), dtype=torch.float32, device=dev)
                o_lab = torch.empty((k,), dtype=torch.int64, device=dev)
                if k:
                    check(lib.ndet_gather_detections(c_void_p(ids.data_ptr()), k, c_void_p(c_box.data_ptr()), c_void_p(c_best.data_ptr()),
                                                     c_void_p(c_lab.data_ptr()), c_void_p(o_box.data_ptr()), c_void_p(o_sc.data_ptr()),
                                                     c_void_p(o_lab.data_ptr()), st), "gather_detections")
                return [(meta["box_type_3d"](o_box, origin=(0.5, 0.5, 0.5), box_dim=6, with_yaw=False), o_sc, o_lab)]

            def fast(host):
                """The packed picks on the host -> detections; None when the device-side tail flagged an overflow (status != 0).  Header word 3
                is the scene's range-guard word (conv3d.guard_word): it rides on the returned list as ``range_guard``."""
                k, status = int(host[0]), int(host[2])
                if status != 0:
                    return None
                rows = host[4:4 + k * 9].view(k, 9)
                b = object.__new__(DepthInstance3DBoxes)
                b.tensor, b.box_dim, b.with_yaw = rows[:, :7].contiguous(), 7, False
                dets = Detections([(b, rows[:, 7].contiguous(), rows[:, 8].to(torch.int64))])
                dets.range_guard = bool(int(host[3]) & 1)
                return dets

            # ---- fast tail: the per-level top-nms_pre cut, the NMS (candidate count read on the device) and the packing of the picks for
            # ONE device-to-host copy, all enqueued behind the neck's kernels: no host round trip inside the post-processing ----
            if meta["box_type_3d"] is DepthInstance3DBoxes and float(self.test_cfg.score_thr) >= 0:
                check(lib.ndet_select_candidates_topk(nl, pa(bests), pa(labels), pa(boxes), (ctypes.c_int * nl)(*sizes), float(self.test_cfg.score_thr),
                                                      int(self.test_cfg.nms_pre), c_void_p(c_best.data_ptr()), c_void_p(c_lab.data_ptr()),
                                                      c_void_p(c_box.data_ptr()), c_void_p(counts.data_ptr()), st), "select_candidates_topk")
                n_cap, k_cap = min(tot, 4096), 1024
                bufs = self.__dict__.setdefault("_ndet_post", {})
                stream = torch.cuda.current_stream(dev)
                key = (str(dev), n_cap, int(stream.cuda_stream))     # one set per stream: scenes in flight do not share it
                if key not in bufs:
                    bufs[key] = (torch.empty((n_cap,), dtype=torch.int64, device=dev), torch.empty((1,), dtype=torch.int64, device=dev),
                                 torch.empty((max(int(lib.ndet_nms_workspace_bytes(n_cap)), 8),), dtype=torch.uint8, device=dev))
                keep, n_keep, ws = bufs[key]
                packed_out = torch.empty((4 + k_cap * 9,), dtype=torch.float32, device=dev)
                gw = guard_word(dev)
                check(lib.ndet_nms_pack_detections(c_void_p(c_box.data_ptr()), c_void_p(c_best.data_ptr()), c_void_p(c_lab.data_ptr()),
                                                   c_void_p(counts.data_ptr()), nl, int(self.test_cfg.nms_pre), n_cap, float(self.test_cfg.iou_thr),
                                                   c_void_p(keep.data_ptr()), c_void_p(n_keep.data_ptr()), c_void_p(ws.data_ptr()),
                                                   c_void_p(packed_out.data_ptr()), k_cap, c_void_p(0 if gw is None else gw.data_ptr()), st),
                      "nms_pack_detections")
                if defer:
                    # every handle owns its pinned landing buffer + event until it is collected: a scene queued on the same stream before
                    # the previous handle's finish() ran must not overwrite that scene's picks.  Collected pairs return to a free list.
                    free = bufs.setdefault(("pinned-free", k_cap), [])
                    pin = free.pop() if free else [torch.empty((4 + k_cap * 9,), dtype=torch.float32).pin_memory(), torch.cuda.Event()]
                    pin[0].copy_(packed_out, non_blocking=True)
                    pin[1].record(stream)
                    state = {"res": None}

                    def finish():
                        if state["res"] is None:                                  # a handle may be collected more than once
                            pin[1].synchronize()                                  # the scene's one host sync, whenever the caller gets to it
                            got = fast(pin[0].clone())
                            free.append(pin)
                            if got is None:
                                with torch.cuda.stream(stream):
                                    got = Detections(general())
                                    got.range_guard = guard_tripped(dev)
                            state["res"] = got
                        return state["res"]
                    return finish
                # (a pinned landing buffer + event wait, as the deferred form uses, measured 0.4 % SLOWER here in same-box alternating runs: kept pageable)
                got = fast(packed_out.cpu())                                  # the one host sync of the scene
                if got is not None:
                    return got
            res = Detections(general())
            res.range_guard = guard_tripped(dev)           # (the host-driven tail has synchronised already)
            return (lambda: res) if defer else res
        # generic path: per-level top-k, then threshold, NMS, box conversion with library ops
        for i in range(nl):
            if bests[i].shape[0] > self.test_cfg.nms_pre > 0:
                bests[i], ids = bests[i].topk(self.test_cfg.nms_pre)
                labels[i], boxes[i] = labels[i][ids], boxes[i][ids]
        best, lab, box = torch.cat(bests), torch.cat(labels), torch.cat(boxes)
        keep = best > self.test_cfg.score_thr
        best, lab, box = best[keep], lab[keep], box[keep]
        ids = aligned_3d_nms(box, best, lab, self.test_cfg.iou_thr)
        b = box[ids]
        b = torch.stack(((b[:, 0] + b[:, 3]) / 2.0, (b[:, 1] + b[:, 4]) / 2.0, (b[:, 2] + b[:, 5]) / 2.0,
                         b[:, 3] - b[:, 0], b[:, 4] - b[:, 1], b[:, 5] - b[:, 2]), dim=1)
        b = meta["box_type_3d"](b, origin=(0.5, 0.5, 0.5), box_dim=6, with_yaw=False)
        res = [(b, best[ids], lab[ids])]
        return (lambda: res) if defer else res

    # ---- training (A16) --------------------------------------------------------------------
    def loss(self, centernesses, bbox_preds, cls_scores, valid, img_metas, gt_bboxes, gt_labels):
        assert len(centernesses[0]) == len(valid) == len(img_metas) == len(gt_bboxes) == len(gt_labels)
        valids = self._level_valids(centernesses, valid)
        acc: List[List[torch.Tensor]] = [[], [], []]
        for b in range(len(img_metas)):
            ls = self._loss_single([x[b] for x in centernesses], [x[b] for x in bbox_preds], [x[b] for x in cls_scores],
                                   [x[b] for x in valids], img_metas[b], gt_bboxes[b], gt_labels[b])
            for a, l in zip(acc, ls):
                a.append(l)
        return dict(loss_centerness=torch.mean(torch.stack(acc[0])), loss_bbox=torch.mean(torch.stack(acc[1])),
                    loss_cls=torch.mean(torch.stack(acc[2])))

    def _loss_single(self, centernesses, bbox_preds, cls_scores, valids, img_meta, gt_bboxes, gt_labels):
        """imvoxel_head_v2.py:116-203."""
        dev = centernesses[0].device
        pts_l = self.get_points([f.size()[-3:] for f in centernesses], img_meta["lidar2img"]["origin"], dev)
        ctr_t, box_t, labels = self.get_targets(pts_l, gt_bboxes, gt_labels)
        ctr = torch.cat([c.permute(1, 2, 3, 0).reshape(-1) for c in centernesses])
        reg = torch.cat([r.permute(1, 2, 3, 0).reshape(-1, r.shape[0]) for r in bbox_preds])
        cls = torch.cat([c.permute(1, 2, 3, 0).reshape(-1, self.n_classes) for c in cls_scores])
        val = torch.cat([v.permute(1, 2, 3, 0).reshape(-1) for v in valids])
        ctr_t, box_t, labels = ctr_t.to(dev), box_t.to(dev), labels.to(dev)
        pts = torch.cat(pts_l)
        from .losses import AxisAlignedIoULoss
        if ctr.is_cuda and type(self.loss_bbox) is AxisAlignedIoULoss and self.loss_bbox.reduction == "mean":
            return self._losses_masked(ctr, reg, cls, val, pts, ctr_t, box_t, labels)     # (another loss_bbox: the gathered form below)
        pos = torch.nonzero(torch.logical_and(labels >= 0, val)).reshape(-1)
        n_pos = torch.tensor(len(pos), dtype=torch.float, device=dev)
        n_pos = max(_reduce_mean(n_pos), 1.0)
        if torch.any(val):
            loss_cls = self.loss_cls(cls[val], labels[val], avg_factor=n_pos)
        else:
            loss_cls = cls[val].sum()
        if len(pos) > 0:
            loss_ctr = self.loss_centerness(ctr[pos], ctr_t[pos], avg_factor=n_pos)
            loss_box = self.loss_bbox(_dist_to_box(pts[pos], reg[pos]), box_t[pos], weight=ctr_t[pos],
                                      avg_factor=ctr_t[pos].sum())
        else:
            loss_ctr, loss_box = ctr[pos].sum(), reg[pos].sum()
        return loss_ctr, loss_box, loss_cls

    def _losses_masked(self, ctr, reg, cls, val, pts, ctr_t, box_t, labels):
        """The three losses of imvoxel_head_v2.py:170-203 without reading anything back to the host: instead of gathering the positive /
        valid locations (``nonzero``, ``len(pos)``, ``if torch.any``: each one a host sync in the middle of the step, after which the launch
        queue is empty while the host builds the rest of the loss graph) every location is evaluated and weighted by its mask.  Row by row
        the arithmetic is the reference's; only the order of the final sums differs.  Rows outside the mask get benign operands first (unit
        boxes, target 0), so neither their values nor their gradients can turn into NaN x 0."""
        from .losses import _reduce, aligned_iou_3d
        posm = torch.logical_and(labels >= 0, val)
        n_pos = torch.clamp(_reduce_mean(posm.sum().float()), min=1.0)
        loss_cls = self.loss_cls(cls, labels, weight=val.to(cls.dtype), avg_factor=n_pos)
        w_pos = posm.to(ctr.dtype)
        loss_ctr = self.loss_centerness(ctr, torch.where(posm, ctr_t, torch.zeros_like(ctr_t)), weight=w_pos, avg_factor=n_pos)
        pm = posm.unsqueeze(1)
        unit = torch.ones_like(reg)
        pred = _dist_to_box(pts, torch.where(pm, reg, unit))
        target = torch.where(pm, box_t, _dist_to_box(pts, unit))
        w_box = torch.where(posm, ctr_t, torch.zeros_like(ctr_t))
        denom = w_box.sum()
        denom = torch.where(denom > 0, denom, torch.ones_like(denom))           # no positives: the reference returns reg[pos].sum() = 0
        loss_box = _reduce(1 - aligned_iou_3d(pred, target), w_box, "mean", denom) * self.loss_bbox.loss_weight
        return loss_ctr, loss_box, loss_cls

    @torch.no_grad()
    def get_targets(self, points, gt_bboxes, gt_labels):
        """FCOS-3D assignment of imvoxel_head_v2.py:457-526: a location is positive for a box when it is
        inside it, sits on the box's best scale (first level with fewer than ``limit`` inside points,
        minus one; last level if none), and is among the box's ``centerness_topk`` most central
        locations; ties between boxes go to the smallest volume."""
        big = 1e8
        dev = gt_labels.device
        lvl = torch.cat([torch.full((len(p),), float(i), dtype=p.dtype, device=p.device) for i, p in enumerate(points)]).to(dev)
        pts = torch.cat(points, dim=0).to(dev)
        n_pts, n_box = len(pts), len(gt_bboxes)
        vol = gt_bboxes.volume.to(dev).expand(n_pts, n_box).contiguous()
        gt = torch.cat((gt_bboxes.gravity_center, gt_bboxes.tensor[:, 3:6]), dim=1).to(dev).expand(n_pts, n_box, 6)
        p = pts.unsqueeze(1).expand(n_pts, n_box, 3)
        t = torch.stack((p[..., 0] - gt[..., 0] + gt[..., 3] / 2, gt[..., 0] + gt[..., 3] / 2 - p[..., 0],
                         p[..., 1] - gt[..., 1] + gt[..., 4] / 2, gt[..., 1] + gt[..., 4] / 2 - p[..., 1],
                         p[..., 2] - gt[..., 2] + gt[..., 5] / 2, gt[..., 2] + gt[..., 5] / 2 - p[..., 2]), dim=-1)
        inside = t.min(-1)[0] > 0
        per_scale = torch.stack([torch.sum(torch.logical_and(inside, (lvl == i).unsqueeze(1)), dim=0) for i in range(self.n_scales)], dim=0)
        low = per_scale < self.limit
        rank = torch.arange(self.n_scales, 0, -1, device=dev).unsqueeze(1).expand(self.n_scales, n_box)
        first_low = torch.argmax(low.int() * rank, dim=0) - 1
        first_low = torch.where(first_low < 0, torch.zeros_like(first_low), first_low)
        none_low = torch.all(torch.logical_not(low), dim=0)
        best = torch.where(none_low, torch.ones_like(none_low) * self.n_scales - 1, first_low)
        on_best = best.unsqueeze(0).expand(n_pts, n_box) == lvl.unsqueeze(1).expand(n_pts, n_box)
        ctr = compute_centerness(t)
        ctr = torch.where(inside, ctr, torch.ones_like(ctr) * -1)
        ctr = torch.where(on_best, ctr, torch.ones_like(ctr) * -1)
        kth = torch.topk(ctr, self.centerness_topk + 1, dim=0).values[-1]
        central = ctr > kth.unsqueeze(0)
        for m in (inside, on_best, central):
            vol = torch.where(m, vol, torch.ones_like(vol) * big)
        min_vol, arg = vol.min(dim=1)
        labels = gt_labels[arg]
        labels = torch.where(min_vol == big, torch.ones_like(labels) * -1, labels)
        t = t[torch.arange(n_pts, device=dev), arg]
        return compute_centerness(t), _dist_to_box(pts, t), labels


def _reduce_mean(t):
    """mmdet.core.reduce_mean: identity unless distributed, else all-reduce(SUM) / world."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return t
    t = t.clone()
    dist.all_reduce(t.div_(dist.get_world_size()), op=dist.ReduceOp.SUM)
    return t
