"""The plain CPU reference of the detection tail (tests/detection_tail_ref.py) against what it restates: the oracle's NMS, the golden picks
of the reference's own NMS, the library-op "topk, then threshold" chain and the oracle's get_bboxes in fp64.  No GPU."""
import numpy as np
import pytest
import torch

import detection_tail_ref as R
from conftest import load_golden
from oracle import nerfdet_oracle as O


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 4095])
def test_nms_ref_equals_the_oracle_on_tie_free_inputs(n):
    boxes, scores, classes = R.clustered_boxes(n, 3, 100 + n)
    assert scores.unique().numel() == n, "the inputs must be tie-free: the oracle's argsort leaves ties undefined"
    for thr in (0.25, 0.5):
        ref = O.aligned_3d_nms(boxes, scores, classes, thr)
        got, order, suppressor = R.nms_ref(boxes, scores, classes, thr, details=True)
        assert torch.equal(got, ref), (n, thr)
        assert torch.equal(order, torch.argsort(scores, descending=True))
        # every candidate is either a pick or removed by a pick of higher score
        assert torch.equal((suppressor < 0).nonzero().flatten().sort()[0], got.sort()[0])
        gone = (suppressor >= 0).nonzero().flatten()
        assert bool((scores[suppressor[gone]] > scores[gone]).all())
        if n >= 63:
            assert 0.1 * n <= len(ref) <= 0.6 * n, f"kept {len(ref) / n:.2f}"


def test_nms_ref_reproduces_the_golden_picks_of_the_reference():
    g = load_golden("nms_random")
    for thr in (0.25, 0.5):
        assert torch.equal(R.nms_ref(g["boxes"], g["scores"], g["classes"], thr), g[f"pick_{int(thr * 100)}"])
    # zero-volume boxes: 0/0 = NaN IoU removes
    assert torch.equal(R.nms_ref(g["deg_boxes"], g["scores"][:40], torch.zeros(40, dtype=torch.long), 0.25), g["deg_pick"])


def test_nms_ref_visits_ties_from_the_higher_index_down():
    b = torch.tensor([[0.0, 0, 0, 1, 1, 1]]).repeat(4, 1)
    b[2:] += 10.0
    s = torch.tensor([0.5, 0.5, 0.5, 0.5])
    pick, order, suppressor = R.nms_ref(b, s, torch.zeros(4, dtype=torch.long), 0.25, details=True)
    assert order.tolist() == [3, 2, 1, 0] and pick.tolist() == [3, 1] and suppressor.tolist() == [1, -1, 3, -1]
    assert R.nms_ref(b[:0], s[:0], torch.zeros(0, dtype=torch.long), 0.25).tolist() == []


def test_select_ref_equals_topk_then_threshold_on_tie_free_inputs():
    g = torch.Generator().manual_seed(11)
    sizes = [1, 1023, 1024, 2049]
    bests = [torch.rand(n, generator=g) for n in sizes]
    labels = [torch.randint(0, 18, (n,), generator=g) for n in sizes]
    boxes = [torch.rand(n, 6, generator=g) for n in sizes]
    assert all(b.unique().numel() == b.numel() for b in bests), "tie-free"
    for thr, nms_pre in ((0.05, 300), (0.7, 300), (0.05, 1), (0.05, 0), (0.0, 5000)):
        s, l, x, counts = R.select_ref(bests, labels, boxes, thr, nms_pre)
        off = 0
        for lv, n in enumerate(sizes):
            bb, ll, xx = bests[lv], labels[lv], boxes[lv]
            if n > nms_pre > 0:
                bb, ids = bb.topk(nms_pre)
                ll, xx = ll[ids], xx[ids]
            keep = bb > thr
            bb, ll, xx = bb[keep], ll[keep], xx[keep]
            c = counts[lv]
            assert c == len(bb), (thr, nms_pre, lv)
            # the chain orders a cut level by score, select_ref by voxel: compare as sets, through the (unique) scores
            o1, o2 = torch.argsort(bb), torch.argsort(s[off:off + c])
            assert torch.equal(bb[o1], s[off:off + c][o2]) and torch.equal(ll[o1], l[off:off + c][o2]) and torch.equal(xx[o1], x[off:off + c][o2])
            off += c
        assert counts[len(sizes)] == off == len(s) and counts[len(sizes) + 1] == sum(int((b > thr).sum()) for b in bests)
    # voxel order inside a level, and the cut did apply somewhere
    s, _, _, counts = R.select_ref(bests, labels, boxes, 0.05, 300)
    assert counts[:4] == [int(bests[0][0] > 0.05), 300, 300, 300] and counts[5] > 3000
    lv1 = s[counts[0]:counts[0] + 300]
    pos = torch.tensor([int((bests[1] == v).nonzero()) for v in lv1])
    assert bool((pos[1:] > pos[:-1]).all())


def test_select_ref_resolves_ties_at_the_cut_in_voxel_order():
    b = torch.tensor([0.9, 0.5, 0.1, 0.5, 0.7, 0.5, 0.5])
    lab = torch.arange(7)
    box = torch.arange(42, dtype=torch.float32).view(7, 6)
    s, l, x, counts = R.select_ref([b], [lab], [box], 0.2, 4)
    assert l.tolist() == [0, 1, 3, 4] and counts == [4, 4, 6] and torch.equal(x, box[l]) and torch.equal(s, b[l])


def test_decode_ref_agrees_with_get_bboxes_in_fp64():
    g = torch.Generator().manual_seed(5)
    grid, n_cls, scale = (6, 5, 4), 18, 1.3
    vs, origin = (0.16, 0.16, 0.2), (0.3, -0.2, 1.1)
    n = grid[0] * grid[1] * grid[2]
    raw = torch.randn(n, 7 + n_cls, generator=g, dtype=torch.float64)
    raw[:, 1:7] *= 0.5
    valid = (torch.rand(n, generator=g) < 0.7)
    best, label, boxes, margin = R.decode_ref(raw, valid.to(torch.uint8), scale, grid, vs, origin)
    vol = lambda t: t.reshape(*grid, -1).permute(3, 0, 1, 2)[None]
    ctr, cls = vol(raw[:, :1]), vol(raw[:, 7:])
    reg = torch.exp(vol(raw[:, 1:7]) * scale)
    # a view count whose trilinear resize to its own size is the identity; score_thr high: the oracle's own NMS stays small
    out = O.head_get_bboxes([ctr], [reg], [cls], vol(valid.to(torch.float64)[:, None]) * 3.0, origin, vs, 0, 0.6, 0.25, n_cls)
    ref_best, ref_label = out["all_scores"].max(dim=1)
    assert out["all_scores"].dtype == torch.float64 and out["all_boxes"].dtype == torch.float64
    torch.testing.assert_close(best, ref_best, rtol=1e-14, atol=0)
    torch.testing.assert_close(boxes, out["all_boxes"], rtol=1e-14, atol=1e-14)
    assert torch.equal(label, ref_label)
    second = out["all_scores"].sort(dim=1, descending=True)[0][:, 1]
    torch.testing.assert_close(margin, ref_best - second, rtol=0, atol=1e-15)
    assert 0.5 < float(valid.float().mean()) < 0.9 and bool((best[~valid] == 0).all()) and bool((label[~valid] == 0).all())
    # a NaN row never wins a class: best -1, label 0
    raw[3, 7:] = float("nan")
    best, label, _, _ = R.decode_ref(raw, torch.ones(n, dtype=torch.uint8), scale, grid, vs, origin)
    assert float(best[3]) == -1.0 and int(label[3]) == 0


def test_pack_ref_rows():
    boxes = torch.tensor([[0.0, 1, 2, 4, 7, 3], [1.0, 1, 1, 2, 2, 2]])
    rows = R.pack_ref(torch.tensor([1, 0]), boxes, torch.tensor([0.25, 0.75]), torch.tensor([7, 2 ** 40]))
    assert rows.dtype == torch.float32 and rows.tolist() == [[1.5, 1.5, 1.0, 1, 1, 1, 0, 0.75, float(2 ** 40)], [2.0, 4.0, 2.0, 4, 6, 1, 0, 0.25, 7.0]]
    c, s, l = R.gather_ref(torch.tensor([0]), boxes, torch.tensor([0.25, 0.75]), torch.tensor([7, 9]))
    assert c.tolist() == [[2.0, 4.0, 2.5, 4, 6, 1]] and s.tolist() == [0.25] and l.tolist() == [7]


def test_decode_inputs_of_the_gpu_tests_exclude_few_labels():
    """The share of voxels whose label the GPU decode tests cannot compare (valid, and the best two fp64 class scores inside the score
    tolerance rtol 1e-5 / atol 1e-7) stays under 1 %, from the reference alone."""
    import test_detection_tail_gpu as G
    _, raws, _, valids, refs = G._decode_inputs()
    total = sum(len(r[0]) for r in refs)
    excl = sum(int((valids[l].bool() & ~torch.isnan(raws[l][:, 7:]).any(1) & ~(m > 1e-7 + 1e-5 * b.abs())).sum()) for l, (b, _, _, m) in enumerate(refs))
    assert total == 512 + 64 + 8 and excl / total <= 0.01, (excl, total)


def test_compaction_inputs_of_the_gpu_tests_have_their_properties():
    import test_detection_tail_gpu as G
    for name, (levels, thr, nms_pre, cond) in G.SELECT_CASES.items():
        assert cond([G._cut(b, thr, nms_pre) for b in levels]), name
