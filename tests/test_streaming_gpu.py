"""GPU checks of streaming scene inference (nerf-det_amd/streaming.py, ops.scene_accumulate / density_finish / volume_finish): chunked
accumulation against the one-shot K1 / K2 kernels and an fp64 statement of nerfdet.py:234-253, SceneStream against simple_test, the range
guard on a chunk."""
import copy

import pytest
import torch

from oracle import nerfdet_oracle as O

pytestmark = pytest.mark.gpu


def _chunk_meta(meta, v0, v1):
    m = dict(meta)
    m["lidar2img"] = dict(meta["lidar2img"], extrinsic=list(meta["lidar2img"]["extrinsic"][v0:v1]))
    return m


def _splits(n, sizes):
    out, v = [], 0
    for k in sizes:
        out.append((v, v + k))
        v += k
    assert v == n
    return out


def _inputs(device, n_v, hw=(64, 96), grid=(12, 12, 6), c=64, cm=8, seed=0):
    from nerfdet_amd import ops
    g = torch.Generator().manual_seed(seed)
    meta = O.ring_scene_meta(n_v, hw)
    h, w = hw[0] // 4, hw[1] // 4
    feats = torch.randn(n_v, c, h, w, generator=g).to(device).contiguous(memory_format=torch.channels_last)
    weight, bias = torch.randn(cm, c, generator=g) / c ** 0.5, torch.randn(cm, generator=g) * 0.5
    mapped = torch.nn.functional.linear(feats.permute(0, 2, 3, 1), weight.to(device), bias.to(device)).permute(0, 3, 1, 2)
    rgb = torch.rand(n_v, 3, *hw, generator=g).to(device)
    depth = (torch.rand(n_v, *hw, generator=g, dtype=torch.float64) * 5.0 + 0.5).to(device)
    return dict(meta=meta, feats=feats, mapped=mapped, bias=bias.to(device), rgb=rgb, depth=depth, vs=(0.5, 0.5, 0.5), grid=grid,
                points=ops.get_points(grid, (0.5, 0.5, 0.5), meta["lidar2img"]["origin"], device),
                proj=ops.compute_projection(meta, 4, device), rgb_proj=ops.compute_projection(meta, 1, device), hw=hw, h=h, w=w)


def _gate(d, v0, v1, gated):
    from nerfdet_amd import ops
    return ops.depth_gate(d["depth"][v0:v1], d["vs"], (d["h"], d["w"]), d["hw"]) if gated else None


def _accumulate(d, splits, gated):
    from nerfdet_amd import ops
    st = ops.SceneState(d["grid"], d["feats"].shape[1], d["mapped"].shape[1], d["feats"].device)
    for v0, v1 in splits:
        ops.scene_accumulate(st, d["feats"][v0:v1], d["mapped"][v0:v1], d["bias"], d["rgb"][v0:v1], d["points"], d["proj"][v0:v1],
                             d["rgb_proj"][v0:v1], depth_gate=_gate(d, v0, v1, gated))
    return st


def _rows_fp64(d, gated):
    """nerfdet.py:234-253 in float64 over the exact-API backprojection's gathers (the reference's own statement of the rows)."""
    from nerfdet_amd import ops
    dep = dict(depth=d["depth"], voxel_size=d["vs"]) if gated else {}
    fv, fvalid = ops.backproject(d["mapped"].contiguous(), d["points"], d["proj"], **dep)
    rv, rvalid = ops.backproject(d["rgb"], d["points"], d["rgb_proj"], **dep)
    n_v = fv.shape[0]
    fv, rv = fv.reshape(n_v, fv.shape[1], -1).double().cpu(), rv.reshape(n_v, 3, -1).double().cpu()
    fm, rm = fvalid.reshape(n_v, 1, -1).cpu(), rvalid.reshape(n_v, 1, -1).cpu()
    fv = torch.where(fm, fv, d["bias"].double().cpu().view(1, -1, 1))     # the "0 bias issue": unseen views contribute the bias
    rv = torch.where(rm, rv, torch.zeros_like(rv))
    vals = torch.cat([rv, fv], 1)                                          # (n_v, 3 + cm, N)
    cnt = fm.sum(0).double()                                               # (1, N)
    mean = vals.sum(0) / (cnt + 1e-8)
    var = ((vals - mean) ** 2).sum(0) / (cnt + 1e-8)
    var = torch.where(cnt == 0, torch.full_like(var, 1e6), var)
    rows = torch.stack([mean, torch.exp(-var)], -1)                       # (3 + cm, N, 2)
    return rows.permute(1, 0, 2).reshape(mean.shape[1], -1), fm.sum(0)[0], rm.sum(0)[0]


def _rows_bar(got, one_shot, ref):
    err_one = float((one_shot.double().cpu() - ref).abs().max())
    bar = torch.maximum(torch.full_like(ref, 2 * err_one), 1e-6 * ref.abs().clamp(min=1.0))
    over = ((got.double().cpu() - ref).abs() / bar).max()
    assert float(over) <= 1.0, f"chunked rows {float(over):.2f}x outside the bar (one-shot error {err_one:.2e})"


@pytest.mark.parametrize("gated", [False, True])
def test_ops_chunks_match_one_shot(device, gated):
    from nerfdet_amd import ops
    n_v = 12
    d = _inputs(device, n_v)
    gate = _gate(d, 0, n_v, gated)
    ref_mean, ref_cnt = ops.backproject_aggregate(d["feats"], d["points"], d["proj"], alpha=None, depth_gate=gate)
    alpha = torch.rand(d["points"][0].numel(), generator=torch.Generator().manual_seed(3)).to(device)
    ref_gated, _ = ops.backproject_aggregate(d["feats"], d["points"], d["proj"], alpha=alpha, depth_gate=gate)
    ref_rows = ops.density_features(d["mapped"], d["bias"], d["rgb"], d["points"], d["proj"], d["rgb_proj"], depth_gate=gate)
    rows64, cnt_f, cnt_r = _rows_fp64(d, gated)
    assert int(ref_cnt.sum()) > 0
    for sizes in ([12], [1] * 12, [3] * 4, [4, 1, 7]):
        st = _accumulate(d, _splits(n_v, sizes), gated)
        assert st.n_views == n_v
        mean, cnt = ops.volume_finish(st, torch.ones_like(alpha))
        assert torch.equal(cnt, ref_cnt), sizes
        assert torch.equal(mean, ref_mean), f"K1 sums differ from one launch for chunks {sizes}"
        vol, _ = ops.volume_finish(st, alpha)
        assert torch.equal(vol, ref_gated), sizes
        assert torch.equal(st.k2_count[:, 0].cpu(), cnt_f.to(torch.int32)) and torch.equal(st.k2_count[:, 1].cpu(), cnt_r.to(torch.int32))
        assert torch.equal(st.k1_count.cpu(), cnt_f.to(torch.int32))
        rows = ops.density_finish(st, d["bias"])
        if len(sizes) == 1:
            assert torch.equal(rows, ref_rows), "a single chunk must give the packed kernel's rows bit for bit"
        _rows_bar(rows, ref_rows, rows64)
        # finishing leaves the state as it was
        assert torch.equal(ops.density_finish(st, d["bias"]), rows) and torch.equal(ops.volume_finish(st, alpha)[0], vol)
    if gated:
        _, ungated = ops.backproject_aggregate(d["feats"], d["points"], d["proj"])
        assert int(ref_cnt.sum()) < int(ungated.sum())


def test_more_than_128_views(device):
    """150 views in chunks of 50 (K2 launches of <= 128 views) against one shot, which takes the unpacked K2 kernel there."""
    from nerfdet_amd import ops
    n_v = 150
    d = _inputs(device, n_v, hw=(32, 48), grid=(8, 8, 4), seed=5)
    assert not ops.density_packed_ok(n_v, d["mapped"].shape[1])
    ref_mean, ref_cnt = ops.backproject_aggregate(d["feats"], d["points"], d["proj"])
    ref_rows = ops.density_features(d["mapped"], d["bias"], d["rgb"], d["points"], d["proj"], d["rgb_proj"])
    rows64, cnt_f, cnt_r = _rows_fp64(d, False)
    for sizes in ([50] * 3, [150]):
        st = _accumulate(d, _splits(n_v, sizes), False)
        mean, cnt = ops.volume_finish(st)
        assert torch.equal(cnt, ref_cnt) and torch.equal(mean, ref_mean)
        assert torch.equal(st.k2_count[:, 0].cpu(), cnt_f.to(torch.int32)) and torch.equal(st.k2_count[:, 1].cpu(), cnt_r.to(torch.int32))
        _rows_bar(ops.density_finish(st, d["bias"]), ref_rows, rows64)


# ---- detector level ----
def _det_and_scene(device, n_v=10, seed=4):
    from test_detector_gpu import _scene, _small_detector
    det = _small_detector(device)
    img, dn, meta, rays = _scene(device, seed, n_v=n_v)
    return det, img, dn, meta, rays


def _one_shot(det, img, dn, meta, rays, depth=None):
    with torch.no_grad():
        rb = det._ray_batch(dict(denorm_images=dn, **rays))
        return det.simple_test(img, [dict(meta)], depth=depth, ray_batch=rb)[0]


def _stream(det, img, dn, meta, sizes, depth=None, stream=None):
    s = stream or det.begin_scene(dict(meta))
    for v0, v1 in _splits(img.shape[1], sizes):
        s.add_views(img[:, v0:v1], dn[:, v0:v1], _chunk_meta(meta, v0, v1), depth=None if depth is None else depth[:, v0:v1])
    return s


def _one(r):
    if isinstance(r, list):     # detect() returns simple_test's list of one result dict
        assert len(r) == 1
        return r[0]
    return r


def _same(a, b):
    a, b = _one(a), _one(b)
    assert torch.equal(a["labels_3d"], b["labels_3d"]) and torch.equal(a["scores_3d"], b["scores_3d"])
    assert torch.equal(a["boxes_3d"].tensor, b["boxes_3d"].tensor)


def _close(a, b):
    a, b = _one(a), _one(b)
    assert torch.equal(a["labels_3d"], b["labels_3d"]), "labels or their order differ"
    torch.testing.assert_close(a["scores_3d"], b["scores_3d"], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(a["boxes_3d"].tensor, b["boxes_3d"].tensor, rtol=1e-4, atol=1e-4, equal_nan=True)


def test_single_chunk_equals_simple_test(device):
    det, img, dn, meta, rays = _det_and_scene(device)
    want = _one_shot(det, img, dn, meta, rays)
    assert len(want["scores_3d"]) > 5
    s = _stream(det, img, dn, meta, [10])
    assert s.n_views == 10
    _same(s.detect(), want)
    # with depth (float64 maps at the image size)
    depth = (torch.rand(1, 10, 64, 96, generator=torch.Generator().manual_seed(9), dtype=torch.float64) * 1.5 + 2.0).to(device)
    want_d = _one_shot(det, img, dn, meta, rays, depth=depth)
    _same(_stream(det, img, dn, meta, [10], depth=depth).detect(), want_d)
    _close(_stream(det, img, dn, meta, [3, 7], depth=depth).detect(), want_d)


@pytest.mark.parametrize("sizes", [[1] * 10, [5, 5], [3, 6, 1]])
def test_many_chunks_match_simple_test(device, sizes):
    det, img, dn, meta, rays = _det_and_scene(device)
    want = _one_shot(det, img, dn, meta, rays)
    _close(_stream(det, img, dn, meta, sizes).detect(), want)


def test_repeated_detect(device):
    det, img, dn, meta, rays = _det_and_scene(device)
    want = _one_shot(det, img, dn, meta, rays)
    s = det.begin_scene(dict(meta))
    s.add_views(img[:, :4], dn[:, :4], _chunk_meta(meta, 0, 4))
    early = s.detect()
    _close(early, _one_shot(det, img[:, :4], dn[:, :4], _chunk_meta(meta, 0, 4), rays))
    s.add_views(img[:, 4:], dn[:, 4:], _chunk_meta(meta, 4, 10))
    a, b = s.detect(), s.detect()
    _close(a, want)
    _same(a, b)
    _same(s.detect(defer=True)(), a)
    vol, valid = s.volume()
    assert valid.shape == (1,) + tuple(det.n_voxels) and vol.shape[0] == det.mapping[0].in_features
    s.reset()
    assert s.n_views == 0
    with pytest.raises(RuntimeError):
        s.detect()


def _blind(meta, views):
    """The same rig with the cameras of ``views`` moved 1000 m back: they see no voxel."""
    m = copy.deepcopy(meta)
    for v in views:
        e = m["lidar2img"]["extrinsic"][v].copy()
        e[2, 3] -= 1000.0
        m["lidar2img"]["extrinsic"][v] = e
    return m


def test_blind_chunk_and_blind_scene(device):
    det, img, dn, meta, rays = _det_and_scene(device)
    m = _blind(meta, [6, 7, 8])
    want = _one_shot(det, img, dn, m, rays)
    s = _stream(det, img, dn, m, [6, 3, 1])     # the middle chunk sees nothing
    _close(s.detect(), want)
    # a scene no view sees: K2's unseen-voxel rows, an all-zero volume, simple_test's (empty) answer
    m = _blind(meta, range(10))
    want = _one_shot(det, img, dn, m, rays)
    s = _stream(det, img, dn, m, [4, 6])
    vol, valid = s.volume()
    assert int(valid.sum()) == 0 and not vol.any()
    _close(s.detect(), want)


def test_two_streams_alternately(device):
    det, img, dn, meta, rays = _det_and_scene(device)
    img2, dn2 = img.flip(0).roll(1, dims=1), dn.roll(1, dims=1)
    meta2 = _chunk_meta(meta, 0, 10)
    meta2["lidar2img"]["extrinsic"] = meta2["lidar2img"]["extrinsic"][-1:] + meta2["lidar2img"]["extrinsic"][:-1]
    want1, want2 = _one_shot(det, img, dn, meta, rays), _one_shot(det, img2, dn2, meta2, rays)
    s1, s2 = det.begin_scene(dict(meta)), det.begin_scene(dict(meta2))
    for v0, v1 in _splits(10, [2, 5, 3]):
        s1.add_views(img[:, v0:v1], dn[:, v0:v1], _chunk_meta(meta, v0, v1))
        s2.add_views(img2[:, v0:v1], dn2[:, v0:v1], _chunk_meta(meta2, v0, v1))
    _close(s1.detect(), want1)
    _close(s2.detect(), want2)


def test_guard_trip_in_one_chunk(device):
    """cfg2 (50 views) with the bright region of test_adversarial_gpu in the first chunk: that chunk's backbone is redone on bf16x3 before it
    enters the state, and the answer meets the chunked bars against simple_test (which repeats the whole scene).  A plain scene trips nothing."""
    from nerfdet_amd import conv3d as C
    from test_adversarial_gpu import _adversarial_detector, _bench
    bench = _bench()
    w = bench.WORKLOADS["cfg2"]
    det = _adversarial_detector(bench, w).to(device)
    batch = bench.to_device(bench.synth_batch(w, 0), device)
    plain = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
    batch["img"][:, :4, :, 60:140, 100:220] *= 1.0e6
    meta = batch["img_metas"][0]
    rays = {k: batch[k] for k in ("lightpos", "raydirs", "gt_images", "gt_depths", "nerf_sizes")}
    assert C.ARITHMETIC == "f16x2"
    with torch.no_grad():
        before = C.guard_trips
        want = _one_shot(det, batch["img"], batch["denorm_images"], meta, rays)
        assert C.guard_trips == before + 1
        s = det.begin_scene(dict(meta))
        s.add_views(batch["img"][:, :10], batch["denorm_images"][:, :10], _chunk_meta(meta, 0, 10))
        assert C.guard_trips == before + 2, "the bright chunk was not redone"
        for v0 in range(10, 50, 10):
            v1 = v0 + 10
            s.add_views(batch["img"][:, v0:v1], batch["denorm_images"][:, v0:v1], _chunk_meta(meta, v0, v1))
        assert C.guard_trips == before + 2, "a plain chunk tripped the guard"
        _close(s.detect(), want)
        before = C.guard_trips
        s = _stream(det, plain["img"], plain["denorm_images"], meta, [25, 25])
        s.detect()
        assert C.guard_trips == before, "an ordinary scene must stay on the fp16-pair arithmetic"
