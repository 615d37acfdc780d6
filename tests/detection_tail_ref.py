"""Test helper: the detection tail (imvoxel_head_v2.py:262-285,528-555 and box3d_nms.py:91-138) restated on the CPU with plain torch
and plain loops -- the per-voxel decode, the ``score > thr`` compaction with the per-level top-``nms_pre`` cut, the greedy aligned NMS
and the packing of the picks.  Nothing here imports the package under test; test_detection_tail_ref_cpu.py checks these functions
against the oracle, the golden picks and the library-op chains."""
from __future__ import annotations

import numpy as np
import torch


# --------------------------------------------------------------------------- decode
def decode_ref(raw, valid_u8, scale, grid, voxel_size, origin):
    """raw (N, 7 + n_cls) = [centerness | 6 reg | class logits] of an (nx, ny, nz) level, z fastest; valid_u8 (N).
    -> best (N) fp64, label (N) int64, boxes (N, 6) fp64, margin (N) fp64 (best minus second-best class score).

    score_k = sigmoid(cls_k) * sigmoid(ctr) * valid; best starts at -1 with label 0 and a class replaces it only when strictly larger
    (so the first of equal classes wins and a NaN row stays at -1 / 0).  The voxel corner p is fp32, rounded as get_points rounds it
    (nerfdet.py:380-390: idx * voxel_size + (origin - n / 2 * voxel_size), every step its own rounding)."""
    nx, ny, nz = (int(v) for v in grid)
    n = nx * ny * nz
    raw = raw.reshape(n, -1).to(torch.float64)
    n_cls = raw.shape[1] - 7
    v = (valid_u8.reshape(n) != 0).to(torch.float64)
    ctr = 1.0 / (1.0 + torch.exp(-raw[:, 0]))
    sc = (1.0 / (1.0 + torch.exp(-raw[:, 7:]))) * ctr[:, None] * v[:, None]
    best = torch.full((n,), -1.0, dtype=torch.float64)
    label = torch.zeros((n,), dtype=torch.int64)
    for k in range(n_cls):
        m = sc[:, k] > best
        best[m] = sc[m, k]
        label[m] = k
    if n_cls > 1:
        top2 = torch.sort(torch.nan_to_num(sc, nan=-np.inf), dim=1, descending=True)[0][:, :2]
        margin = top2[:, 0] - top2[:, 1]
        margin[torch.isnan(margin)] = 0.0
    else:
        margin = torch.full((n,), np.inf, dtype=torch.float64)
    vs = np.asarray(voxel_size, dtype=np.float32)
    org = np.asarray(origin, dtype=np.float32)
    dims = np.asarray([nx, ny, nz], dtype=np.float32)
    shifted = (org - ((dims / np.float32(2.0)) * vs).astype(np.float32)).astype(np.float32)
    p = np.empty((n, 3), dtype=np.float32)
    i = 0
    for ix in range(nx):
        for iy in range(ny):
            for iz in range(nz):
                for a, idx in enumerate((ix, iy, iz)):
                    p[i, a] = np.float32(np.float32(idx) * vs[a]) + shifted[a]
                i += 1
    p = torch.from_numpy(p).to(torch.float64)
    d = torch.exp(float(scale) * raw[:, 1:7])
    boxes = torch.stack([p[:, 0] - d[:, 0], p[:, 1] - d[:, 2], p[:, 2] - d[:, 4],
                         p[:, 0] + d[:, 1], p[:, 1] + d[:, 3], p[:, 2] + d[:, 5]], dim=1)
    return best, label, boxes, margin


# --------------------------------------------------------------------------- compaction
def select_ref(bests, labels, boxes, thr, nms_pre):
    """Per level: the voxels with ``score > thr`` (fp32 compare); when more than ``nms_pre > 0`` of them survive, the nms_pre largest,
    ties at the cut going to the first in voxel order.  Output in voxel order, levels concatenated.
    -> scores (n) fp32, labels (n) int64, boxes (n, 6) fp32, counts = [kept of level 0, ..., kept in all, survivors before any cut]."""
    thr = float(np.float32(thr))
    o_s, o_l, o_b, counts, raw_total = [], [], [], [], 0
    for s, lab, box in zip(bests, labels, boxes):
        vals = s.to(torch.float32).tolist()
        surv = [i for i, v in enumerate(vals) if v > thr]
        raw_total += len(surv)
        if nms_pre > 0 and len(surv) > nms_pre:
            surv = sorted(sorted(surv, key=lambda i: (-vals[i], i))[:nms_pre])
        idx = torch.tensor(surv, dtype=torch.int64)
        o_s.append(s[idx])
        o_l.append(lab[idx])
        o_b.append(box[idx])
        counts.append(len(surv))
    counts = counts + [sum(counts), raw_total]
    return torch.cat(o_s), torch.cat(o_l), torch.cat(o_b), counts


# --------------------------------------------------------------------------- NMS
def nms_order(scores):
    """Candidate indices in descending (score, index) order: among equal scores the higher index comes first.  No NaN scores."""
    vals = scores.to(torch.float32).tolist()
    assert not any(v != v for v in vals)
    return sorted(range(len(vals)), key=lambda i: (vals[i], i), reverse=True)


def nms_ref(boxes, scores, classes, thr, details=False):
    """The sequential greedy loop of box3d_nms.py:91-138 in fp32, one pick at a time, candidates visited in :func:`nms_order`.
    A later candidate j is removed by pick i unless ``iou_ij * [class_i == class_j] <= thr``; a NaN IoU fails that and removes.
    -> picks (k) int64 in pick order; with ``details`` also (order, suppressor): the visiting order and, per candidate, the pick that
    removed it (-1 for the picks themselves)."""
    n = boxes.shape[0]
    order = torch.tensor(nms_order(scores), dtype=torch.int64)
    b = boxes.to(torch.float32)[order]
    c = classes.to(torch.int64)[order]
    lo, hi = b[:, :3], b[:, 3:6]
    ext = hi - lo
    vol = ext[:, 0] * ext[:, 1] * ext[:, 2]
    t = torch.tensor(float(thr), dtype=torch.float32)
    zero = torch.tensor(0.0, dtype=torch.float32)
    alive = torch.ones(n, dtype=torch.bool)
    by = torch.full((n,), -1, dtype=torch.int64)      # in sorted positions
    picks = []
    pos = 0
    while pos < n:
        nz = torch.nonzero(alive[pos:])
        if nz.numel() == 0:
            break
        p = pos + int(nz[0])
        picks.append(p)
        pos = p + 1
        if pos >= n:
            break
        e = torch.maximum(torch.minimum(hi[p], hi[pos:]) - torch.maximum(lo[p], lo[pos:]), zero)
        inter = e[:, 0] * e[:, 1] * e[:, 2]
        iou = inter / (vol[p] + vol[pos:] - inter)
        iou = iou * (c[p] == c[pos:]).to(torch.float32)
        gone = ~(iou <= t) & alive[pos:]
        by[pos:][gone] = p
        alive[pos:] &= ~gone
    picks = torch.tensor(picks, dtype=torch.int64)
    out = order[picks] if n else picks
    if not details:
        return out
    suppressor = torch.full((n,), -1, dtype=torch.int64)
    hit = by >= 0
    suppressor[order[hit]] = order[by[hit]]
    return out, order, suppressor


# --------------------------------------------------------------------------- picks -> detections
def pack_ref(keep, boxes, scores, labels):
    """(k, 9) fp32 rows [cx, cy, z_bottom, dx, dy, dz, 0, score, label] of the picks, every operation rounded to fp32 on its own."""
    b = boxes.to(torch.float32)[keep]
    half = torch.tensor(-0.5, dtype=torch.float32)
    dz = b[:, 5] - b[:, 2]
    return torch.stack([(b[:, 0] + b[:, 3]) / 2.0, (b[:, 1] + b[:, 4]) / 2.0, (b[:, 2] + b[:, 5]) / 2.0 + dz * half,
                        b[:, 3] - b[:, 0], b[:, 4] - b[:, 1], dz, torch.zeros_like(dz),
                        scores.to(torch.float32)[keep], labels[keep].to(torch.float32)], dim=1)


def gather_ref(keep, boxes, scores, labels):
    """(k, 6) fp32 [centre, size] boxes, scores and labels of the picks (imvoxel_head_v2.py:546-555)."""
    b = boxes.to(torch.float32)[keep]
    out = torch.stack([(b[:, 0] + b[:, 3]) / 2.0, (b[:, 1] + b[:, 4]) / 2.0, (b[:, 2] + b[:, 5]) / 2.0,
                       b[:, 3] - b[:, 0], b[:, 4] - b[:, 1], b[:, 5] - b[:, 2]], dim=1)
    return out, scores.to(torch.float32)[keep], labels[keep]


# --------------------------------------------------------------------------- inputs shared by the CPU and the GPU tests
def clustered_boxes(n, n_cls, seed, quantised=False):
    """n boxes in tight clusters (about seven per cluster and class), so that greedy NMS removes most of them: boxes (n, 6) fp32,
    scores (n) fp32 (``quantised``: 16 levels, massive ties), classes (n) int64."""
    g = torch.Generator().manual_seed(seed)
    m = max(1, n // (7 * n_cls))
    side = 2.0 * m ** (1.0 / 3.0)
    centres = torch.rand(m, 3, generator=g) * side
    which = torch.randint(0, m, (n,), generator=g)
    ctr = centres[which] + 0.12 * torch.randn(n, 3, generator=g)
    size = 0.8 + 0.4 * torch.rand(n, 3, generator=g)
    boxes = torch.cat([ctr - size / 2, ctr + size / 2], 1)
    # distinct by construction (torch.rand draws 24 bits: 4096 of them already hold an exact tie)
    scores = (torch.randperm(n, generator=g).to(torch.float32) + 0.5) / n
    if quantised:
        scores = torch.floor(scores * 16.0) / 16.0
    classes = torch.randint(0, n_cls, (n,), generator=g)
    return boxes, scores, classes


def plant_first_to_last(boxes, scores, classes):
    """Make the last candidate of the visiting order a near copy of the first, so that the first pick removes a candidate of the
    last 64-block.  Boxes and classes only: the visiting order does not change."""
    order = nms_order(scores)
    first, last = order[0], order[-1]
    boxes, classes = boxes.clone(), classes.clone()
    boxes[last] = boxes[first] + torch.tensor([0.0, 0.0, 0.0, 0.015625, 0.0, 0.0])
    classes[last] = classes[first]
    return boxes, classes
