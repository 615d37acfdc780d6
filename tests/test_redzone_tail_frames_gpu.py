"""The detection tail and the frame kernels inside tests/redzone.py.  Every row twice, fill 0x00 then 0xFF, inputs placed flush against guards, every
buffer the Python layer takes carved: no guard byte and no input changed, the documented results equal bit for bit.

Detection tail: ScanNetImVoxelHeadV2.simple_test_fused with hand-made per-level head outputs (``raws=``), so that the number of candidates a level
hands on is chosen here: decode of every level, the ``score > thr`` compaction with the per-level cut, the NMS and the packing (fast tail), and the
host-driven tail (select, aligned_3d_nms, gather) when the picks overflow the packed tail's 1024 rows.  Don't-care regions, compared by nobody here:
  * the compacted candidates beyond the device-side count: ``c_best`` / ``c_lab`` / ``c_box`` are allocated at the total voxel count and
    include/nerfdet_hip.h says of ndet_select_candidates "survivors go to out_* in level-then-voxel order, counts ... = per level, then the
    total" -- nothing is said of, and head.py reads nothing of, the elements after the total (``c_box[:n]``);
  * the packed picks beyond row n_keep: include/nerfdet_hip.h, ndet_nms_pack_detections: "out_packed = {n_keep, n_candidates, status, range
    guard} followed by up to k_cap rows", and head.py's ``fast`` reads ``host[4:4 + k * 9]`` only.
The results of a row are the detections the call returns -- boxes, scores, labels -- which are cut from the defined part by the library itself.

Frames: prepare_frames (BGR and NV12), prepare_depth_frames, positive_indices, nv12_to_bgr / bgr_to_nv12, camera_rays, pack_frames, frame_errors,
frame_ssim, project_boxes, draw_boxes, draw_overlay, label_frames.  All integer or one fixed-order sum per element (frame_errors and frame_ssim sum
integers: "the same bytes on every call").  Numbers are held to the references by tests/test_detection_tail_gpu.py, test_raw_frames_gpu.py,
test_depth_frames_gpu.py, test_nv12_frames_gpu.py, test_frames_out_gpu.py, test_frame_ssim_gpu.py, test_detections_out_gpu.py and
test_overlay_gpu.py."""
import numpy as np
import pytest
import torch

import detections_out_ref as D
import overlay_ref as OV
from redzone import both_fills
from test_detections_out_gpu import _k33

pytestmark = pytest.mark.gpu


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ---- detection tail ----
SMALL, LARGE = [(12, 12, 4), (6, 6, 2), (3, 3, 1)], [(24, 24, 4), (12, 12, 2), (6, 6, 1)]


def _raws(grids, counts, seed, reg):
    """Per level an (X, Y, Z, 25) head output with exactly ``counts[l]`` voxels whose best score clears any sensible threshold (class logit 0 .. 3,
    centerness 2) and every other voxel far below it (logits -20); box half-extents exp(scale * (reg .. reg + 1))."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for (x, y, z), k in zip(grids, counts):
        n = x * y * z
        raw = torch.empty(n, 25)
        raw[:, 0] = 2.0
        raw[:, 1:7] = torch.rand(n, 6, generator=g) + reg
        raw[:, 7:] = -20.0
        hot = torch.randperm(n, generator=g)[:k]
        raw[hot, 7 + torch.randint(0, 18, (k,), generator=g)] = torch.rand(k, generator=g) * 3
        out.append(raw.view(x, y, z, 25))
    return out


# (level grids, candidates per level, nms_pre, reg): 257 = one past a 256-thread workgroup's sweep; a level without a detection; a scene without
# any; 257 > nms_pre = 100: the per-level cut; 1100 boxes narrower than a voxel: more than the 1024 picks the packed tail holds, so its status
# word sends the scene through the host-driven tail (select, aligned_3d_nms, gather)
@pytest.mark.parametrize("grids,counts,nms_pre,reg", [(SMALL, (257, 0, 3), 1000, -2.5), (SMALL, (1, 0, 0), 1000, -2.5), (SMALL, (0, 0, 0), 1000, -2.5),
                                                      (SMALL, (257, 0, 3), 100, -2.5), (SMALL, (64, 65, 9), 1000, -2.5), (LARGE, (1100, 0, 3), 2000, -4.0)],
                         ids=["257-0-3", "1-0-0", "none", "257-0-3-pre100", "64-65-9", "1100-host-tail"])
def test_redzone_detection_tail(device, grids, counts, nms_pre, reg):
    from nerfdet_amd.boxes import DepthInstance3DBoxes
    from nerfdet_amd.config import ConfigDict
    from nerfdet_amd.head import ScanNetImVoxelHeadV2
    torch.manual_seed(1)
    head = ScanNetImVoxelHeadV2(n_classes=18, n_channels=32, n_reg_outs=6, n_scales=3, limit=27, centerness_topk=18,
                                test_cfg=ConfigDict(nms_pre=nms_pre, iou_thr=0.25, score_thr=0.01))
    head.voxel_size = (0.16, 0.16, 0.2)
    with torch.no_grad():
        for i, sc in enumerate(head.scales):
            sc.scale.fill_(1.0 + 0.3 * i)
    head.eval()
    raws = _raws(grids, counts, sum(counts) + nms_pre, reg)
    valid = torch.ones(1, 1, *grids[0])
    valid[0, 0, 0, 0, 0] = 0.0
    meta = dict(lidar2img=dict(origin=np.array([0.0, 0.0, 0.5], dtype=np.float32)), box_type_3d=DepthInstance3DBoxes)

    def body(rz):
        with torch.no_grad():
            h = rz.place_module(head)
            feats = [torch.zeros(1, 32, *g, device=device) for g in grids]           # only their device and shapes are read when ``raws`` is given
            (boxes, scores, labels), = h.simple_test_fused(feats, rz.place(valid, "valid"), [meta], raws=[rz.place(r, f"raw{i}") for i, r in enumerate(raws)])
            return {"boxes": boxes.tensor, "scores": scores, "labels": labels}
    host_tail = sum(counts) > 1024
    got = both_fills(device, body, results_on_host=not host_tail)      # the fast tail hands its picks over in one packed host copy
    assert got["scores"].shape[0] <= sum(counts) and (sum(counts) == 0) == (got["scores"].shape[0] == 0)
    assert (got["scores"].shape[0] > 1024) == host_tail, "the row does not reach the tail it is named for"
    assert got["boxes"].shape[0] == got["labels"].shape[0] == got["scores"].shape[0]


# ---- frames in ----
def _bgr_frames(n, h, w, seed):
    return torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("want_u8", [False, True])
def test_redzone_prepare_frames_bgr(device, want_u8):
    """An odd source size, 37 x 53 -> 28 x 40 inside a 32 x 48 pad; a selection of frames in another order."""
    from nerfdet_amd import pipeline as P
    frames = _bgr_frames(3, 37, 53, 1)
    assert P.rescale_size((37, 53), (40, 30)) == (28, 40)

    def body(rz):
        out = P.prepare_frames(rz.place(frames, "frames"), (40, 30), (32, 48), ids=[2, 0], want_u8=want_u8)
        return dict(zip(("img", "denorm", "u8"), out))
    both_fills(device, body)


@pytest.mark.parametrize("margin", [0, 3])
def test_redzone_prepare_depth_frames(device, margin):
    from nerfdet_amd import pipeline as P
    g = torch.Generator().manual_seed(2)
    mm = torch.randint(0, 6000, (3, 37, 53), generator=g).to(torch.uint16)

    def body(rz):
        d = P.prepare_depth_frames(rz.place(mm, "depth_frames"), (28, 40), ids=[1, 2], margin=margin)
        return {"depth": d, "positive": P.positive_indices(d.contiguous())}
    got = both_fills(device, body)
    assert got["depth"].shape == (2, 28 - 2 * margin, 40 - 2 * margin)


@pytest.mark.parametrize("hs,ws", [(2, 2), (6, 10), (8, 18)], ids=["2x2", "6x10", "8x18"])
def test_redzone_nv12_in_and_out(device, hs, ws):
    """The smallest even surface, and widths (10, 18) that are no multiple of 4, 8 or 16 pixels; tight layout."""
    from nerfdet_amd import pipeline as P
    g = torch.Generator().manual_seed(hs * ws)
    surf = torch.randint(0, 256, (2, hs * 3 // 2, ws), dtype=torch.uint8, generator=g)
    odd = _bgr_frames(2, hs + 1, ws + 1, 3)                                    # bgr_to_nv12 replicates the last row / column of an odd frame

    def body(rz):
        s = rz.place(surf, "surfaces")
        img, denorm = P.prepare_frames(s, (max(hs, ws), min(hs, ws)), (hs, ws), format="nv12", size=(hs, ws))
        bgr = P.nv12_to_bgr(s, (hs, ws), ids=[1, 0])
        back, size = P.bgr_to_nv12(bgr)
        from_odd, size_odd = P.bgr_to_nv12(rz.place(odd, "odd_frames"))
        assert size == (hs, ws) and size_odd == (hs + 2, ws + 2)
        return {"img": img, "denorm": denorm, "bgr": bgr, "surfaces": back, "surfaces_from_odd": from_odd}
    both_fills(device, body)


# ---- frames out ----
def test_redzone_frames_out(device):
    """camera_rays over an odd window, pack_frames and frame_errors over 2 frames of 37 x 53 (no multiple of any tile)."""
    from nerfdet_amd import pipeline as P
    n, h, w = 2, 37, 53
    g = torch.Generator().manual_seed(4)
    rgb = torch.rand(n * h * w, 3, generator=g) * 1.2 - 0.1
    depth = torch.rand(n * h * w, generator=g) * 8
    mask = torch.rand(n * h * w, generator=g) < 0.8
    other, other_mm = _bgr_frames(n, h, w, 5), torch.randint(0, 6000, (n, h, w), generator=g).to(torch.uint16)
    krows, w2c, _ = OV.projection_case()
    c2w = np.linalg.inv(np.asarray(w2c, dtype=np.float64))

    def body(rz):
        ray_o, ray_d = P.camera_rays(_k33(krows), c2w, (1, 2, h, w), device=device)
        frames, mm = P.pack_frames(rz.place(rgb, "rgb"), rz.place(depth, "depth"), rz.place(mask, "mask"), (n, h, w))
        err = P.frame_errors(frames, rz.place(other, "frames_b"), mm, rz.place(other_mm, "depth_b"))
        return {"ray_o": ray_o, "ray_d": ray_d, "frames": frames, "mm": mm, **{f"err_{k}": v for k, v in err.items()}}
    both_fills(device, body)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
@pytest.mark.parametrize("h,w", [(7, 7), (9, 13)], ids=["7x7", "9x13"])
def test_redzone_frame_ssim(device, h, w, dtype):
    """Frames smaller than two 7 x 7 windows: one window, and 3 x 7 of them."""
    from nerfdet_amd import pipeline as P
    a, b = _bgr_frames(2, h, w, 6), _bgr_frames(2, h, w, 7)
    if dtype == torch.float32:
        a, b = a.float() / 255, b.float() / 255
    mm = torch.randint(0, 3, (2, h, w), generator=torch.Generator().manual_seed(8)).to(torch.uint16)

    def body(rz):
        ad, bd = rz.place(a, "frames_a"), rz.place(b, "frames_b")
        plain, gated = P.frame_ssim(ad, bd), P.frame_ssim(ad, bd, rz.place(mm, "depth_a"))
        return {**{f"plain_{k}": v for k, v in plain.items()}, **{f"gated_{k}": v for k, v in gated.items()}}
    both_fills(device, body)


@pytest.mark.parametrize("thickness,scale", [(1, 1), (5, 3)])
def test_redzone_overlay(device, thickness, scale):
    """tests/overlay_ref.py's projection case (36 boxes over two 37 x 53 frames, several partly or wholly off-frame, some cut by the near plane): the
    projection with depths, the plain wireframes, the depth-tested overlay with text plates, and the per-pixel labels."""
    from nerfdet_amd import pipeline as P
    from nerfdet_amd.boxes import box_frames
    krows, w2c, corners = OV.projection_case()
    frames, col = _t(OV.case_frames()), OV.case_colours(36)
    depth = _t(OV.depth_case(thickness, 50.0)[0])
    texts = ["chair 0.87", "", "x", "a much longer name than any class has, cut"] + [f"box {i}" for i in range(4, 36)]
    ref = OV.projected_ref()
    assert (ref["edge_mask"] == 0).any() and ((ref["edge_mask"] != 0) & (ref["edge_mask"] != 0xFFF)).any(), "no box leaves the frame or the near plane"
    c2w = np.linalg.inv(np.asarray(w2c, dtype=np.float64))
    bf = box_frames(D.random_boxes(5, 2, centre=np.zeros(3, dtype=np.float32)))

    def body(rz):
        proj = P.project_boxes(_k33(krows), corners, OV.WINDOW, 1, extrinsic=w2c, device=device, depths=True)
        fd, dd = rz.place(frames, "frames"), rz.place(depth, "depth_frames")
        cd = rz.place(_t(col), "colours")
        out = {key: proj[key] for key in ("edges", "edge_mask", "rect", "zrange", "edge_w")}
        out["wire"] = P.draw_boxes(fd, proj, cd, thickness)
        out["overlay"] = P.draw_overlay(fd, proj, cd, thickness, depth_frames=dd, occluded="dim", texts=texts, text_scale=scale)
        out["labels"] = P.label_frames(dd, _k33(krows), c2w, bf, OV.WINDOW)
        return out
    both_fills(device, body)
