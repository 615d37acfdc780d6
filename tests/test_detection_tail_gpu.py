"""The kernels of csrc/nms_kernels.hip -- decode, ``score > thr`` compaction, device-side top-nms_pre radix select, NMS (count from the
host and count on the device), packing of the picks -- each called through the C ABI and compared with the plain CPU reference of
tests/detection_tail_ref.py.  Every input comes from a seeded CPU generator; every condition on an input (kept fraction, winners per
block, ties at a cut ...) is asserted from the reference, never from a kernel's output."""
import ctypes
import functools
from ctypes import c_void_p

import numpy as np
import pytest
import torch

import detection_tail_ref as R

pytestmark = pytest.mark.gpu

SIZES = [2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4095, 4096]
SENT = -12345.0      # poison of the float outputs
KSENT = -7           # poison of keep / counts / labels


def _lib():
    from nerfdet_amd import _lib as L
    return L.load(), L.check


def _p(t):
    return c_void_p(t.data_ptr())


def _stream(device):
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int32)


# --------------------------------------------------------------------------- NMS inputs and their reference picks (computed once)
@functools.lru_cache(maxsize=None)
def _case(n, n_cls, quantised):
    b, s, c = R.clustered_boxes(n, n_cls, 1000 + n, quantised)
    if n >= 1024:
        b, c = R.plant_first_to_last(b, s, c)
    assert quantised or s.unique().numel() == n
    assert not quantised or s.unique().numel() <= 16
    return b, s, c


@functools.lru_cache(maxsize=None)
def _expected(n, n_cls, quantised, thr):
    """nms_ref's picks, with the conditions on the inputs asserted from the reference itself."""
    b, s, c = _case(n, n_cls, quantised)
    picks, order, suppressor = R.nms_ref(b, s, c, thr, details=True)
    frac = len(picks) / n
    if n >= 63:
        assert 0.1 <= frac <= 0.6, f"n={n} classes={n_cls} ties={quantised} thr={thr}: the reference keeps {frac:.3f} of the candidates"
    if n >= 1024:
        pos = torch.empty(n, dtype=torch.int64)
        pos[order] = torch.arange(n)
        per_block = torch.bincount(pos[picks] // 64)
        assert int(per_block.max()) > 16, f"n={n}: at most {int(per_block.max())} winners in a 64-block (kept {frac:.3f})"
        last = order[(n - 1) // 64 * 64:]
        by = suppressor[last]
        assert bool((pos[by[by >= 0]] < 64).any()), f"n={n}: no winner of block 0 removes a candidate of the last block"
    return picks, frac


def _nms_host(device, b, s, c, thr):
    """ndet_aligned_3d_nms on poisoned outputs and workspace -> picks (CPU)."""
    lib, check = _lib()
    n = len(s)
    db, ds, dc = b.to(device).contiguous(), s.to(device).contiguous(), c.to(device).contiguous()
    keep = torch.full((max(n, 1),), KSENT, dtype=torch.int64, device=device)
    n_keep = torch.full((1,), KSENT, dtype=torch.int64, device=device)
    ws = torch.full((max(int(lib.ndet_nms_workspace_bytes(n)), 8),), 0xFF, dtype=torch.uint8, device=device)
    check(lib.ndet_aligned_3d_nms(_p(db), _p(ds), _p(dc), n, float(thr), _p(keep), _p(n_keep), _p(ws), _stream(device)), "aligned_3d_nms")
    k = int(n_keep.item())
    assert 0 <= k <= n
    out = keep.cpu()
    assert bool((out[k:] == KSENT).all()), "keep[] written past n_keep"
    return out[:k]


@pytest.mark.parametrize("quantised", [False, True], ids=["distinct", "ties16"])
@pytest.mark.parametrize("n", SIZES)
def test_nms_count_from_the_host_equals_the_reference(device, n, quantised):
    """ndet_aligned_3d_nms at the word (64), shuffle/LDS (256) and NMS_MAX (4096) boundaries, 1 and 3 classes, thresholds 0.25 / 0.5,
    distinct scores and 16 score levels (ties are visited from the higher index down)."""
    for n_cls in (1, 3):
        b, s, c = _case(n, n_cls, quantised)
        for thr in (0.25, 0.5):
            ref, frac = _expected(n, n_cls, quantised, thr)
            got = _nms_host(device, b, s, c, thr)
            assert torch.equal(got, ref), f"n={n} classes={n_cls} thr={thr} kept fraction {frac:.3f}: {len(got)} picks against {len(ref)}"


def _edge_cases():
    g = torch.Generator().manual_seed(9)
    out = {}
    b, s, c = R.clustered_boxes(300, 3, 41)
    out["all_scores_equal"] = (b, torch.full((300,), 0.5), c, 0.25)
    # IoU == thr exactly in fp32: unit cube against 1 x 1 x 4 (1 / 4) and 1 x 1 x 2 (1 / 2) towers; kept, because `<=`
    for thr, h in ((0.25, 4.0), (0.5, 2.0)):
        eb = torch.tensor([[0.0, 0, 0, 1, 1, 1], [0.0, 0, 0, 1, 1, h], [0.0, 0, 0, 1, 1, h * 0.875]])
        out[f"iou_equals_thr_{thr}"] = (eb, torch.tensor([0.9, 0.8, 0.7]), torch.zeros(3, dtype=torch.int64), thr)
    b, s, c = R.clustered_boxes(300, 1, 42)
    flip = torch.rand(300, 3, generator=g) < 0.2          # some axes of some boxes inverted: negative extents, negative volumes
    lo, hi = b[:, :3].clone(), b[:, 3:].clone()
    b = torch.cat([torch.where(flip, hi, lo), torch.where(flip, lo, hi)], 1)
    out["inverted_boxes"] = (b, s, c, 0.25)
    b, s, c = R.clustered_boxes(300, 3, 43)
    out["class_ids_above_2_31"] = (b, s, 7 + c * 2 ** 32, 0.25)     # equal in their low 32 bits
    b, s, c = R.clustered_boxes(300, 3, 44)
    s = s.clone()
    s[torch.rand(300, generator=g) < 0.3] = float("-inf")
    out["minus_inf_scores"] = (b, s, c, 0.25)
    return out


EDGES = _edge_cases()


@pytest.mark.parametrize("name", sorted(EDGES))
def test_nms_edge_cases_equal_the_reference(device, name):
    b, s, c, thr = EDGES[name]
    ref, order, suppressor = R.nms_ref(b, s, c, thr, details=True)
    if name.startswith("iou_equals_thr"):
        e = (torch.minimum(b[0, 3:], b[1, 3:]) - torch.maximum(b[0, :3], b[1, :3])).clamp(min=0)
        inter = e[0] * e[1] * e[2]
        vol = lambda x: (x[3] - x[0]) * (x[4] - x[1]) * (x[5] - x[2])
        assert float(inter / (vol(b[0]) + vol(b[1]) - inter)) == thr and ref.tolist() == [0, 1] and int(suppressor[2]) == 0
    if name == "inverted_boxes":
        ext = b[:, 3:] - b[:, :3]
        assert int((ext.prod(1) < 0).sum()) > 30 and 30 < len(ref) < 300
    if name == "class_ids_above_2_31":
        assert int(c.max()) > 2 ** 31 and c.unique().numel() == 3
        assert len(ref) > len(R.nms_ref(b, s, torch.zeros_like(c), thr))      # the classes matter
    if name == "minus_inf_scores":
        assert 50 < int(torch.isinf(s).sum()) < 150 and bool(torch.isinf(s[ref]).any())
    got = _nms_host(device, b, s, c, thr)
    assert torch.equal(got, ref), (name, got.tolist()[:20], ref.tolist()[:20])


# --------------------------------------------------------------------------- NMS with the count on the device + packing
def _nms_pack(device, b, s, c, thr, n_cap, k_cap, level_counts=None, nms_pre=0, guard=None, ws=None):
    """ndet_nms_pack_detections with counts[] written on the device; keep, out_packed and (unless handed in) the workspace poisoned.
    -> (keep (n_cap) CPU, n_keep, out_packed CPU, workspace)."""
    lib, check = _lib()
    n = len(s)
    level_counts = [n] if level_counts is None else list(level_counts)
    nl = len(level_counts)
    counts = torch.tensor(level_counts + [n, n], dtype=torch.int32).to(device)
    db, ds, dc = b.to(device).contiguous(), s.to(device).contiguous(), c.to(device).contiguous()
    keep = torch.full((n_cap,), KSENT, dtype=torch.int64, device=device)
    n_keep = torch.full((1,), KSENT, dtype=torch.int64, device=device)
    if ws is None:
        ws = torch.full((int(lib.ndet_nms_workspace_bytes(n_cap)),), 0xFF, dtype=torch.uint8, device=device)
    assert ws.numel() >= int(lib.ndet_nms_workspace_bytes(n_cap))
    out = torch.full((4 + 9 * k_cap,), SENT, dtype=torch.float32, device=device)
    gw = None if guard is None else torch.tensor([guard], dtype=torch.int32).to(device)
    check(lib.ndet_nms_pack_detections(_p(db), _p(ds), _p(dc), _p(counts), nl, int(nms_pre), int(n_cap), float(thr), _p(keep), _p(n_keep), _p(ws),
                                       _p(out), int(k_cap), c_void_p(0) if gw is None else _p(gw), _stream(device)), "nms_pack_detections")
    torch.cuda.synchronize(device)
    return keep.cpu(), int(n_keep.item()), out.cpu(), ws


def _check_pack(res, ref, b, s, c, k_cap, status=0, guard=0.0, what=""):
    keep, n_keep, out, _ = res
    k, n = len(ref), len(s)
    assert n_keep == k, (what, n_keep, k)
    assert torch.equal(keep[:k], ref), what
    assert bool((keep[k:] == KSENT).all()), f"{what}: keep[] written past n_keep"
    assert out[:4].tolist() == [float(k), float(n), float(status), float(guard)], (what, out[:4].tolist())
    rows = out[4:].view(k_cap, 9)
    w = min(k, k_cap)
    assert torch.equal(_bits(rows[:w]), _bits(R.pack_ref(ref[:w], b, s, c))), f"{what}: packed rows differ from pack_ref"
    assert bool((rows[w:] == SENT).all()), f"{what}: a row past min(k, k_cap) was written"


@pytest.mark.parametrize("quantised", [False, True], ids=["distinct", "ties16"])
@pytest.mark.parametrize("n", SIZES)
def test_nms_count_on_the_device_and_packing_equal_the_reference(device, n, quantised):
    """ndet_nms_pack_detections: the grid is sized for n_cap, the row pitch of the bit matrix comes from the count on the device."""
    for n_cls in (1, 3):
        b, s, c = _case(n, n_cls, quantised)
        for thr in (0.25, 0.5):
            ref, frac = _expected(n, n_cls, quantised, thr)
            for n_cap in sorted({n, 4096}):
                res = _nms_pack(device, b, s, c, thr, n_cap, k_cap=n)
                _check_pack(res, ref, b, s, c, n, what=f"n={n} n_cap={n_cap} classes={n_cls} thr={thr} kept fraction {frac:.3f}")


def test_nms_workspace_reused_from_a_larger_launch(device):
    """A large launch, then small ones in the same workspace, not cleared in between: no stale word of the bit matrix is read."""
    big = _case(4096, 1, True)
    res = _nms_pack(device, *big, 0.25, 4096, k_cap=4096)
    _check_pack(res, _expected(4096, 1, True, 0.25)[0], *big, 4096, what="n=4096")
    ws = res[3]
    for n in (65, 2, 1025):
        b, s, c = _case(n, 1, True)
        res = _nms_pack(device, b, s, c, 0.25, 4096, k_cap=n, ws=ws)
        _check_pack(res, _expected(n, 1, True, 0.25)[0], b, s, c, n, what=f"n={n} after n=4096 in the same workspace")


def test_nms_pack_status_bits_and_guard_word(device):
    b, s, c = _case(129, 3, False)
    ref, _ = _expected(129, 3, False, 0.25)
    # bit 0: one candidate more than n_cap -> nothing picked, no row written, the count still reported
    keep, n_keep, out, _ = _nms_pack(device, b, s, c, 0.25, n_cap=128, k_cap=128)
    assert n_keep == 0 and bool((keep == KSENT).all())
    assert out[:4].tolist() == [0.0, 129.0, 1.0, 0.0] and bool((out[4:] == SENT).all())
    # bit 2: more picks than rows -> k in the header, the first k_cap rows as the reference's
    assert len(ref) > 8
    _check_pack(_nms_pack(device, b, s, c, 0.25, n_cap=129, k_cap=8), ref, b, s, c, 8, status=4, what="k_cap=8")
    # bit 1: an uncut level count above nms_pre; the picks are what they are
    _check_pack(_nms_pack(device, b, s, c, 0.25, 4096, 129, level_counts=[5, 124], nms_pre=4), ref, b, s, c, 129, status=2, what="counts[0] > nms_pre")
    _check_pack(_nms_pack(device, b, s, c, 0.25, 4096, 129, level_counts=[4, 100, 20, 5], nms_pre=100), ref, b, s, c, 129, status=0, what="no level above nms_pre")
    _check_pack(_nms_pack(device, b, s, c, 0.25, 128, 8, level_counts=[100, 29], nms_pre=50), ref[:0], b, s, c, 8, status=3, what="bits 0 and 1")
    # header word 3: the range-guard word
    for guard, word in ((None, 0.0), (0, 0.0), (1, 1.0)):
        _check_pack(_nms_pack(device, b, s, c, 0.25, 129, 129, guard=guard), ref, b, s, c, 129, guard=word, what=f"guard={guard}")
    # class ids above 2^31 survive the packing as floats
    b, s, c, thr = EDGES["class_ids_above_2_31"]
    _check_pack(_nms_pack(device, b, s, c, thr, 300, 300), R.nms_ref(b, s, c, thr), b, s, c, 300, what="large class ids")


# --------------------------------------------------------------------------- more than one launch takes
def test_nms_in_windows_with_ties_across_the_window_boundary(device):
    """n = 6000 > NMS_MAX through nms.aligned_3d_nms: 16 score levels, so a level spans the boundary of the first window, and one
    explicit pair of equal score: the earlier member (in visiting order) is kept in the first window, its overlapping partner
    arrives in the second and has to be removed by it."""
    from nerfdet_amd.nms import NMS_MAX, aligned_3d_nms
    n = 6000
    b, s, c = R.clustered_boxes(n, 1, 77, quantised=True)
    order = R.nms_order(s)
    first, partner = order[4000], order[4100]
    assert n > NMS_MAX == 4096 and float(s[order[4095]]) == float(s[order[4096]]) and float(s[first]) == float(s[partner])
    b = b.clone()
    b[first] = torch.tensor([100.0, 100, 100, 101, 101, 101])          # away from every cluster: certainly a pick
    b[partner] = torch.tensor([100.0, 100, 100, 101.015625, 101, 101])
    ref, order_t, suppressor = R.nms_ref(b, s, c, 0.25, details=True)
    assert order_t.tolist() == order and first in ref.tolist() and int(suppressor[partner]) == first
    assert 0.1 * n < len(ref) < NMS_MAX
    got = aligned_3d_nms(b.to(device), s.to(device), c.to(device), 0.25).cpu()
    assert (partner in got.tolist()) is False and first in got.tolist(), "the tied partner of the next window displaced a kept box"
    assert torch.equal(got, ref), f"{len(got)} picks against {len(ref)}"


# --------------------------------------------------------------------------- compaction
def _select(device, d_best, d_label, d_box, thr, nms_pre, topk):
    """ndet_select_candidates[_topk] on device tensors (as handed in: views keep their pointers) -> scores, labels, boxes, counts (CPU)."""
    lib, check = _lib()
    nl = len(d_best)
    sizes = [int(t.shape[0]) for t in d_best]
    tot = sum(sizes)
    o_b = torch.full((tot,), SENT, dtype=torch.float32, device=device)
    o_l = torch.full((tot,), KSENT, dtype=torch.int64, device=device)
    o_x = torch.full((tot, 6), SENT, dtype=torch.float32, device=device)
    counts = torch.full((nl + 2,), KSENT, dtype=torch.int32, device=device)
    pa = lambda ts: (ctypes.c_void_p * nl)(*[t.data_ptr() for t in ts])
    if topk:
        check(lib.ndet_select_candidates_topk(nl, pa(d_best), pa(d_label), pa(d_box), (ctypes.c_int * nl)(*sizes), float(thr), int(nms_pre), _p(o_b), _p(o_l),
                                              _p(o_x), _p(counts), _stream(device)), "select_candidates_topk")
    else:
        check(lib.ndet_select_candidates(nl, pa(d_best), pa(d_label), pa(d_box), (ctypes.c_int * nl)(*sizes), float(thr), _p(o_b), _p(o_l), _p(o_x),
                                         _p(counts), _stream(device)), "select_candidates")
    torch.cuda.synchronize(device)
    return o_b.cpu(), o_l.cpu(), o_x.cpu(), counts.cpu().tolist()


def _check_select(got, ref, nl, topk, what):
    o_b, o_l, o_x, cnt = got
    r_b, r_l, r_x, r_cnt = ref
    assert cnt[:nl + 1] == r_cnt[:nl + 1], (what, cnt, r_cnt)
    assert cnt[nl + 1] == (r_cnt[nl + 1] if topk else KSENT), (what, cnt, r_cnt)
    t = r_cnt[nl]
    assert torch.equal(_bits(o_b[:t]), _bits(r_b)), f"{what}: scores"
    assert torch.equal(o_l[:t], r_l), f"{what}: labels"
    assert torch.equal(_bits(o_x[:t]), _bits(r_x)), f"{what}: boxes"
    assert bool((o_b[t:] == SENT).all()) and bool((o_l[t:] == KSENT).all()) and bool((o_x[t:] == SENT).all()), f"{what}: written past the total"


def _cut(best, thr, nms_pre):
    """(survivors, of them above the cut value, equal to it, quota of the equal ones that are kept) of one level, on the CPU."""
    v = best[best > np.float32(thr)]
    if nms_pre <= 0 or len(v) <= nms_pre:
        return len(v), None, None, None
    cut = torch.sort(v, descending=True)[0][nms_pre - 1]
    n_gt = int((v > cut).sum())
    return len(v), n_gt, int((v == cut).sum()), nms_pre - n_gt


def _with_payload(bests, seed):
    g = torch.Generator().manual_seed(seed)
    return (bests, [torch.randint(0, 18, (len(b),), generator=g) for b in bests], [torch.rand(len(b), 6, generator=g) for b in bests])


def _select_cases():
    """name -> (levels' scores, thr, nms_pre, check(list of _cut per level)).  The checks state, from the CPU alone, what the case is about."""
    g = torch.Generator().manual_seed(21)
    rnd = lambda n: torch.rand(n, generator=g)
    cases = {}
    some_cut = lambda cuts: any(c[1] is not None for c in cuts)
    no_cut = lambda cuts: all(c[1] is None for c in cuts)
    ties_at_cut = lambda l: (lambda cuts: cuts[l][1] is not None and cuts[l][2] > cuts[l][3] >= 1)

    a = rnd(1025)
    a[100:140] = 0.625
    cases["one_level"] = ([a], 0.05, 300, some_cut)
    cases["three_levels"] = ([torch.tensor([0.5]), rnd(1023), rnd(1024)], 0.05, 300, lambda cuts: cuts[0][0] == 1 and cuts[1][1] is not None and cuts[2][1] is not None)
    cases["four_levels"] = ([rnd(1024), rnd(1025) * 0.04, rnd(2049), torch.tensor([0.01])], 0.05, 300,
                            lambda cuts: cuts[1][0] == 0 and cuts[3][0] == 0 and cuts[0][1] is not None and cuts[2][1] is not None)
    a = rnd(36001)
    a[20000:20040] = float(torch.sort(a, descending=True)[0][990])        # ties at the cut of the level that does not fit the LDS
    cases["level_of_36001"] = ([a, rnd(1025)], 0.05, 1000, lambda cuts: cuts[0][0] > 30000 and ties_at_cut(0)(cuts) and cuts[1][1] is None)
    a = rnd(1025) * 0.05
    a[torch.randperm(1025, generator=g)[:301]] = 0.1 + 0.9 * rnd(301)
    cases["survivors_equal_nms_pre"] = ([a], 0.05, 301, lambda cuts: cuts[0][0] == 301 and no_cut(cuts))
    cases["survivors_nms_pre_plus_one"] = ([a], 0.05, 300, lambda cuts: cuts[0][0] == 301 and cuts[0][1] is not None)
    cases["nms_pre_one"] = ([rnd(1025), rnd(2049)], 0.05, 1, lambda cuts: cuts[0][1] == 0 and cuts[1][1] == 0)
    cases["nms_pre_zero"] = ([rnd(1025), rnd(2049)], 0.05, 0, lambda cuts: no_cut(cuts) and cuts[1][0] > 1500)
    a = rnd(2049)
    a[a < 0.5] = 0.0
    a[::7] = 1.0
    a[3::11] = float(np.float32(2.0 ** -140))
    cases["thr_zero_zeros_ones_subnormals"] = ([a], 0.0, 400, lambda cuts, a=a: int((a == 0).sum()) > 500 and cuts[0][0] < 2049 - 500 and cuts[0][1] is not None)
    a = rnd(1025) * 0.9
    a[torch.randperm(1025, generator=g)[:500]] = 1.0
    cases["ties_at_one"] = ([a], 0.05, 300, lambda cuts: cuts[0][1] == 0 and cuts[0][2] == 500 and cuts[0][3] == 300)
    sub = torch.randint(1, 4000, (1025,), generator=g).to(torch.int32).view(torch.float32)      # k * 2^-149
    cases["subnormal_scores"] = ([sub.clone()], 0.0, 300, lambda cuts: float(sub.max()) < 1.2e-38 and cuts[0][0] == 1025 and cuts[0][1] is not None)
    k22 = torch.randint(0, 1024, (2049,), generator=g)
    a = (0x3F000000 + k22).to(torch.int32).view(torch.float32)
    v = torch.sort(a, descending=True)[0][299]
    assert int((a == v).sum()) >= 2          # 2049 draws of 1024 values: the cut is placed one into a block of equal scores
    cases["survivors_share_top_22_bits"] = ([a], 0.05, int((a > v).sum()) + 1, ties_at_cut(0))
    k11 = torch.randint(0, 2 ** 21, (2049,), generator=g)
    cases["survivors_share_top_11_bits"] = ([(0x3F000000 + k11).to(torch.int32).view(torch.float32)], 0.05, 300, lambda cuts: cuts[0][1] is not None)
    # a tie block at the cut longer than a thread's run (ceil(4000 / 1024) = 4 voxels), starting and ending inside runs: voxels 401..410
    a = rnd(4000) * 0.4
    a[torch.randperm(4000, generator=g)[:200]] += 0.5
    a[401:411] = 0.45
    n_gt = int((a > 0.45).sum())
    for name, quota in (("tie_quota_one", 1), ("tie_quota_all_but_one", 9)):
        cases[name] = ([a], 0.05, n_gt + quota, (lambda q: lambda cuts: cuts[0][2] == 10 > 4 and cuts[0][3] == q and (401 + q) % 4 != 0)(quota))
    return cases


SELECT_CASES = _select_cases()


@pytest.mark.parametrize("name", sorted(SELECT_CASES))
def test_compaction_with_the_device_side_cut_equals_the_reference(device, name):
    """ndet_select_candidates_topk against select_ref: scores, labels, boxes and counts exactly.
    (Ties at the cut go to the first in voxel order here.  The host-driven tail cuts with ``topk`` over the compacted survivors, which may
    choose other members of a tie block; the reference leaves ties undefined, and that difference is not checked anywhere.)"""
    levels, thr, nms_pre, cond = SELECT_CASES[name]
    bests, labels, boxes = _with_payload(levels, 5)
    assert cond([_cut(b, thr, nms_pre) for b in bests]), f"{name}: the inputs do not have the property the case is about"
    ref = R.select_ref(bests, labels, boxes, thr, nms_pre)
    for l, b in enumerate(bests):      # the cut really applies where _cut says so
        surv, n_gt, _, _ = _cut(b, thr, nms_pre)
        assert ref[3][l] == (surv if n_gt is None else nms_pre)
    dev = lambda ts: [t.to(device) for t in ts]
    _check_select(_select(device, dev(bests), dev(labels), dev(boxes), thr, nms_pre, True), ref, len(bests), True, name)


def test_compaction_from_a_misaligned_level_equals_the_aligned_one(device):
    """A 4000-voxel level whose scores start 4 bytes into their allocation (read from global memory, not through the LDS copy), and the
    same scores aligned: identical results, both the reference's."""
    g = torch.Generator().manual_seed(31)
    a = torch.rand(4000, generator=g)
    a[1000:1030] = float(torch.sort(a, descending=True)[0][495])
    bests, labels, boxes = _with_payload([a, torch.rand(1023, generator=g)], 6)
    surv, n_gt, n_eq, quota = _cut(a, 0.05, 500)
    assert surv > 500 and n_eq > quota >= 1
    ref = R.select_ref(bests, labels, boxes, 0.05, 500)
    dl, dx = [t.to(device) for t in labels], [t.to(device) for t in boxes]
    aligned = [t.to(device) for t in bests]
    store = torch.empty(4001, dtype=torch.float32, device=device)
    store[1:] = aligned[0]
    shifted = [store[1:], aligned[1]]
    assert aligned[0].data_ptr() % 16 == 0 and shifted[0].data_ptr() % 16 == 4
    got_a = _select(device, aligned, dl, dx, 0.05, 500, True)
    got_s = _select(device, shifted, dl, dx, 0.05, 500, True)
    _check_select(got_a, ref, 2, True, "aligned")
    _check_select(got_s, ref, 2, True, "misaligned")
    assert all(torch.equal(x, y) for x, y in zip(got_a[:3], got_s[:3])) and got_a[3] == got_s[3]


@pytest.mark.parametrize("name", ["one_level", "three_levels", "four_levels", "thr_zero_zeros_ones_subnormals", "subnormal_scores"])
def test_plain_compaction_equals_the_reference(device, name):
    """ndet_select_candidates (no cut; counts[n_levels + 1] is not its to write) against select_ref."""
    levels, thr, _, _ = SELECT_CASES[name]
    bests, labels, boxes = _with_payload(levels, 7)
    ref = R.select_ref(bests, labels, boxes, thr, 0)
    assert ref[3][len(bests)] > 0 and (ref[3][len(bests)] == sum(len(b) for b in bests)) == (name == "subnormal_scores")   # there, thr = 0 drops nothing
    dev = lambda ts: [t.to(device) for t in ts]
    _check_select(_select(device, dev(bests), dev(labels), dev(boxes), thr, 0, False), ref, len(bests), False, name)


# --------------------------------------------------------------------------- decode
DEC_GRID, DEC_CLS = (16, 8, 4), 18
DEC_SCALES = (1.0, 0.5, 1.25)
DEC_VS0, DEC_ORIGIN = np.float32([0.16, 0.16, 0.2]), np.float32([0.3, -0.2, 1.1])
# level-0 voxels with planted rows
V_EQUAL, V_SAT, V_NEG, V_NAN, V_BIG, V_SMALL, V_INF, V_ZERO, V_INVALID = 10, 50, 90, 130, 170, 210, 250, 290, 330


@functools.lru_cache(maxsize=None)
def _decode_inputs():
    g = torch.Generator().manual_seed(13)
    X, Y, Z = DEC_GRID
    valid = (torch.rand(X, Y, Z, generator=g) < 0.7).float() * torch.randint(1, 6, (X, Y, Z), generator=g).float()
    flat = valid.view(-1)
    for v in (V_EQUAL, V_SAT, V_NEG, V_NAN, V_BIG, V_SMALL, V_INF, V_ZERO):
        flat[v] = 2.0
    flat[V_INVALID] = 0.0
    raws, grids, valids = [], [], []
    for l in range(3):
        f = 2 ** l
        grid = (X // f, Y // f, Z // f)
        n = grid[0] * grid[1] * grid[2]
        raw = torch.randn(n, 7 + DEC_CLS, generator=g)
        raw[:, 1:7] *= 0.5
        raw[:, 7:] = raw[:, 7:] * 2.0 - 2.0
        if l == 0:
            raw[V_EQUAL, 7:] = -1.0
            raw[V_EQUAL, 7 + 4] = raw[V_EQUAL, 7 + 9] = raw[V_EQUAL, 7 + 15] = 3.0
            raw[V_SAT, 7:] = -100.0
            raw[V_SAT, 7 + 2] = raw[V_SAT, 7 + 5] = raw[V_SAT, 7 + 11] = 100.0
            raw[V_NEG, 7:] = -100.0
            raw[V_NAN, 7:] = float("nan")
            raw[V_BIG, 1:7], raw[V_SMALL, 1:7] = 80.0, -80.0            # level 0's scale is 1: reg * scale is exact
            raw[V_INF, 1:7], raw[V_ZERO, 1:7] = 100.0, -100.0
        raws.append(raw)
        grids.append(grid)
        valids.append(torch.nn.functional.interpolate(valid[None, None], size=grid, mode="trilinear").round().bool().reshape(-1).to(torch.uint8))
    refs = [R.decode_ref(raws[l], valids[l], DEC_SCALES[l], grids[l], DEC_VS0 * np.float32(2 ** l), DEC_ORIGIN) for l in range(3)]
    return valid, raws, grids, valids, refs


def _check_decode(outs, what):
    _, raws, grids, valids, refs = _decode_inputs()
    total = excluded = 0
    for l, ((best, label, box), (r_best, r_label, r_box, margin)) in enumerate(zip(outs, refs)):
        best, label, box = best.cpu(), label.cpu(), box.cpu()
        ok = valids[l].bool()
        torch.testing.assert_close(best, r_best.float(), rtol=1e-5, atol=1e-7, msg=lambda m: f"{what} level {l} scores: {m}")
        torch.testing.assert_close(box, r_box.float(), rtol=1e-5, atol=1e-5, msg=lambda m: f"{what} level {l} boxes: {m}")
        assert bool((best[~ok] == 0.0).all()) and bool((label[~ok] == 0).all()), f"{what} level {l}: invalid voxels"
        nan_row = torch.isnan(raws[l][:, 7:]).any(1)
        skip = ok & ~nan_row & ~(margin > 1e-7 + 1e-5 * r_best.abs())
        assert torch.equal(label[~skip], r_label[~skip]), f"{what} level {l}: labels"
        total += len(best)
        excluded += int(skip.sum())
        assert bool(ok.any()) and (l > 0 or 0.2 < float(ok.float().mean()) < 0.95)      # the coarse levels see nearly every voxel
        if l == 0:
            ctr = lambda v: float(torch.sigmoid(raws[0][v, 0].double()))
            assert int(label[V_EQUAL]) == 4 and int(label[V_SAT]) == 2 and int(label[V_NEG]) == 0
            assert abs(float(best[V_SAT]) - ctr(V_SAT)) <= 1e-7 + 1e-5 * ctr(V_SAT) and float(best[V_NEG]) == 0.0
            assert float(best[V_NAN]) == -1.0 and int(label[V_NAN]) == 0 and not (float(best[V_NAN]) > 0.0)
            assert float(best[V_INVALID]) == 0.0 and int(label[V_INVALID]) == 0 and int(valids[0][V_INVALID]) == 0
            big = float(np.exp(np.float64(80.0)))
            assert bool(torch.isfinite(box[V_BIG]).all()) and abs(float(box[V_BIG, 3]) / big - 1.0) < 1e-5
            assert bool(torch.isinf(box[V_INF]).all()) and bool((box[V_INF, :3] < 0).all()) and bool((box[V_INF, 3:] > 0).all())
            assert torch.equal(box[V_ZERO, :3], box[V_ZERO, 3:]) and torch.equal(box[V_SMALL, :3], box[V_SMALL, 3:])
            assert bool(torch.isfinite(box[[V_INF - 1, V_INF + 1, V_BIG - 1, V_BIG + 1]]).all())
    share = excluded / total
    print(f"{what}: labels not compared at {excluded} of {total} voxels ({100 * share:.2f} %)")
    assert share <= 0.01, f"{what}: {100 * share:.2f} % of the voxels have an fp64 margin inside the score tolerance"
    return share


def test_head_decode_per_level_equals_the_reference(device):
    lib, check = _lib()
    from nerfdet_amd._lib import float3
    _, raws, grids, valids, _ = _decode_inputs()
    outs = []
    for l in range(3):
        n = grids[l][0] * grids[l][1] * grids[l][2]
        raw, v = raws[l].to(device).contiguous(), valids[l].to(device)
        sc = torch.tensor([DEC_SCALES[l]], dtype=torch.float32, device=device)
        best = torch.full((n,), SENT, dtype=torch.float32, device=device)
        label = torch.full((n,), KSENT, dtype=torch.int64, device=device)
        box = torch.full((n, 6), SENT, dtype=torch.float32, device=device)
        check(lib.ndet_head_decode(_p(raw), DEC_CLS, _p(v), _p(sc), *grids[l], float3(DEC_VS0 * np.float32(2 ** l)), float3(DEC_ORIGIN), _p(best), _p(label),
                                   _p(box), _stream(device)), "head_decode")
        outs.append((best, label, box))
    torch.cuda.synchronize(device)
    _check_decode(outs, "ndet_head_decode")


def test_head_decode_levels_equals_the_reference(device):
    lib, check = _lib()
    valid, raws, grids, _, _ = _decode_inputs()
    d_valid = valid.to(device).contiguous()
    d_raws = [r.to(device).contiguous() for r in raws]
    scales = [torch.tensor([s], dtype=torch.float32, device=device) for s in DEC_SCALES]
    outs = []
    for g in grids:
        n = g[0] * g[1] * g[2]
        outs.append((torch.full((n,), SENT, dtype=torch.float32, device=device), torch.full((n,), KSENT, dtype=torch.int64, device=device),
                     torch.full((n, 6), SENT, dtype=torch.float32, device=device)))
    vp = lambda ts: (ctypes.c_void_p * 3)(*[t.data_ptr() for t in ts])
    vsz = np.concatenate([DEC_VS0 * np.float32(2 ** l) for l in range(3)]).astype(np.float32)
    check(lib.ndet_head_decode_levels(3, vp(d_raws), vp(scales), (ctypes.c_int * 9)(*[v for g in grids for v in g]), (ctypes.c_int * 3)(1, 2, 4),
                                      vsz.ctypes.data_as(c_void_p), DEC_ORIGIN.ctypes.data_as(c_void_p), DEC_CLS, _p(d_valid), *DEC_GRID,
                                      vp([o[0] for o in outs]), vp([o[1] for o in outs]), vp([o[2] for o in outs]), _stream(device)), "head_decode_levels")
    torch.cuda.synchronize(device)
    _check_decode(outs, "ndet_head_decode_levels")


# --------------------------------------------------------------------------- gather
def test_gather_detections_equals_the_reference(device):
    lib, check = _lib()
    b, s, c = _case(257, 3, False)
    c = c + 2 ** 33
    keep = R.nms_ref(b, s, c, 0.25)
    k = len(keep)
    db, ds, dc, dk = b.to(device).contiguous(), s.to(device), c.to(device), keep.to(device)
    o_x = torch.full((k + 3, 6), SENT, dtype=torch.float32, device=device)
    o_s = torch.full((k + 3,), SENT, dtype=torch.float32, device=device)
    o_l = torch.full((k + 3,), KSENT, dtype=torch.int64, device=device)
    check(lib.ndet_gather_detections(_p(dk), k, _p(db), _p(ds), _p(dc), _p(o_x), _p(o_s), _p(o_l), _stream(device)), "gather_detections")
    torch.cuda.synchronize(device)
    r_x, r_s, r_l = R.gather_ref(keep, b, s, c)
    assert k > 30 and torch.equal(_bits(o_x[:k].cpu()), _bits(r_x)) and torch.equal(_bits(o_s[:k].cpu()), _bits(r_s)) and torch.equal(o_l[:k].cpu(), r_l)
    assert bool((o_x[k:] == SENT).all()) and bool((o_s[k:] == SENT).all()) and bool((o_l[k:] == KSENT).all())
