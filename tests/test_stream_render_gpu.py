"""GPU checks of rendering from a streamed scene: the view-bank sampler (csrc/ray_stats_kernels.hip: k_ray_stats_bank, rays.ViewBank /
ray_view_stats_bank) against the packed and the generic samplers on the same inputs, and SceneStream.render / render_rays
(nerf-det_amd/streaming.py, keep_views=True) against the one-shot ray branch."""
import numpy as np
import pytest
import torch

from oracle import nerfdet_oracle as O

pytestmark = pytest.mark.gpu

ATOL = 2e-5      # tests/test_rays_gpu.py: the packed (one-pass) against the generic (two-pass) statistics on identical fp32 coordinates
R, S = 257, 19   # 4883 samples: not a multiple of any samples-per-block

_CACHE = {}


def _inputs(device, n_v, d, hw):
    """The inputs of test_packed_sampler_equals_generic_kernel (tests/test_rays_gpu.py), made once per shape and never changed."""
    key = (str(device), n_v, d, hw)
    if key not in _CACHE:
        from nerfdet_amd import rays
        gen = torch.Generator().manual_seed(n_v * 100 + d)
        meta = O.ring_scene_meta(n_v, hw)
        feat = torch.randn(n_v, d, hw[0] // 4, hw[1] // 4, generator=gen).to(device).contiguous(memory_format=torch.channels_last)
        img = torch.rand(n_v, 3, *hw, generator=gen).to(device)
        ang = torch.rand(R, generator=gen) * 2 * np.pi
        ray_o = torch.stack([2.0 * torch.cos(ang), 2.0 * torch.sin(ang), 1.0 + 0.3 * torch.rand(R, generator=gen)], -1)
        ray_d = -ray_o / ray_o.norm(dim=-1, keepdim=True) + 0.35 * torch.randn(R, 3, generator=gen)
        pts, _ = rays.sample_along_camera_ray(ray_o.to(device), ray_d.to(device), [0.2, 8.0], S, det=True)
        _CACHE[key] = dict(meta=meta, feat=feat, img=img, pts=pts, cams=rays._compute_projection(meta))
    return _CACHE[key]


def _chunk_meta(meta, v0, v1):
    m = dict(meta)
    m["lidar2img"] = dict(meta["lidar2img"], extrinsic=list(meta["lidar2img"]["extrinsic"][v0:v1]))
    return m


def _bank(d, sizes):
    from nerfdet_amd import rays
    bank, v = rays.ViewBank(), 0
    for k in sizes:
        bank.append(d["feat"][v:v + k], d["img"][v:v + k], _chunk_meta(d["meta"], v, v + k))
        v += k
    assert v == d["feat"].shape[0] and bank.n_views == v and len(bank.segments) == len(sizes)
    return bank


def _generic(d):
    from nerfdet_amd import rays
    key = "generic"
    if key not in d:
        saved = rays.packed_ok
        rays.packed_ok = lambda *a, **k: False           # force the generic kernel
        try:
            d[key] = rays.ray_view_stats(d["pts"], d["img"], d["cams"], d["feat"])
        finally:
            rays.packed_ok = saved
    return d[key]


def _packed(d):
    from nerfdet_amd import rays
    if "packed" not in d:
        n_v, c = d["feat"].shape[:2]
        assert rays.packed_ok(n_v, c)
        d["packed"] = rays.ray_view_stats(d["pts"], d["img"], d["cams"], d["feat"])
    return d["packed"]


def _equal(got, want, what):
    for a, b, name in zip(got, want, ("globalfeat", "pixel_mask", "view_count")):
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {name} {tuple(a.shape)} {a.dtype} vs {tuple(b.shape)} {b.dtype}"
        assert torch.equal(a, b), f"{what}: {name} differs, max |diff| {float((a.float() - b.float()).abs().max()):.3e}"


# ---- K-a: one segment, one or two rounds of views: the packed kernel's bits ----
@pytest.mark.parametrize("n_v,d,hw", [(9, 8, (60, 80)), (40, 32, (64, 96)), (5, 48, (48, 64))])
def test_one_segment_equals_packed_kernel(device, n_v, d, hw):
    from nerfdet_amd import rays
    inp = _inputs(device, n_v, d, hw)
    want = _packed(inp)
    got = rays.ray_view_stats_bank(inp["pts"], _bank(inp, [n_v]))
    assert 0.02 < want[1].float().mean() < 0.98
    _equal(got, want, f"{n_v} views, d={d}")


# ---- K-b: several segments (separate allocations) ----
@pytest.mark.parametrize("n_v,sizes", [(12, [12]), (12, [1] * 12), (12, [4, 1, 7]), (100, [63, 2, 35])])
def test_segments_equal_packed_kernel_over_the_concatenation(device, n_v, sizes):
    """[63, 2, 35]: a segment straddles the 64-view ballot word; 100 views take the count pass and two rounds."""
    from nerfdet_amd import rays
    inp = _inputs(device, n_v, 32, (64, 96))
    want = _packed(inp)
    bank = _bank(inp, sizes)
    assert len({s.feat.data_ptr() for s in bank.segments}) == len(sizes)
    _equal(rays.ray_view_stats_bank(inp["pts"], bank), want, f"segments {sizes}")


# ---- K-c: more than 128 views: the generic kernel ----
@pytest.mark.parametrize("d", [8, 32])
def test_more_than_128_views_match_generic_kernel(device, d):
    from nerfdet_amd import rays
    n_v = 150
    inp = _inputs(device, n_v, d, (32, 48))
    assert not rays.packed_ok(n_v, d)
    glob_g, pm_g, vc_g = _generic(inp)
    one = rays.ray_view_stats_bank(inp["pts"], _bank(inp, [150]))
    four = rays.ray_view_stats_bank(inp["pts"], _bank(inp, [63, 2, 64, 21]))
    print(f"d={d}: max |bank - generic| = {float((one[0] - glob_g).abs().max()):.3e}, pixel_mask mean {float(pm_g.float().mean()):.3f}, "
          f"max view_count {int(vc_g.max())}")
    assert 0.02 < pm_g.float().mean() < 0.98
    assert torch.equal(one[1], pm_g) and torch.equal(one[2], vc_g)
    torch.testing.assert_close(one[0], glob_g, rtol=0, atol=ATOL)
    _equal(four, one, "segments [63, 2, 64, 21] against [150]")


# ---- K-d: samples no view sees ----
@pytest.mark.parametrize("n_v,d,hw", [(9, 8, (60, 80)), (150, 32, (32, 48))])
def test_unseen_samples_are_zero(device, n_v, d, hw):
    from nerfdet_amd import rays
    inp = _inputs(device, n_v, d, hw)
    glob, pm, vc = rays.ray_view_stats_bank(inp["pts"], _bank(inp, [n_v]))
    unseen = vc == 0
    assert unseen.any() and (vc > 0).any()
    assert int(vc.max()) <= n_v and int(vc.min()) >= 0
    assert not pm[unseen].any()
    assert torch.equal(pm, vc > 1)
    means = glob[..., :3 + d][unseen]
    assert torch.equal(means, torch.zeros_like(means))


# ---- K-e: repeated calls ----
def test_repeated_calls_leave_the_bank_unchanged(device):
    from nerfdet_amd import rays
    inp = _inputs(device, 12, 32, (64, 96))
    bank = _bank(inp, [4, 1, 7])
    before = [(s.feat.clone(), s.rgb4.clone(), s.ke.clone()) for s in bank.segments]
    table = bank.table()[0]
    a = rays.ray_view_stats_bank(inp["pts"], bank)
    b = rays.ray_view_stats_bank(inp["pts"], bank)
    _equal(b, a, "second call")
    assert bank.table()[0] is table, "the device table is cached until the segment list changes"
    for s, (f, i, k) in zip(bank.segments, before):
        assert torch.equal(s.feat, f) and torch.equal(s.rgb4, i) and torch.equal(s.ke, k)
    bank.drop_oldest(1)
    assert bank.n_views == 8 and bank.table()[1] == 8 and bank.table()[0] is not table
    bank.clear()
    assert bank.n_views == 0
    with pytest.raises(RuntimeError):
        rays.ray_view_stats_bank(inp["pts"], bank)


# ---- detector level ----
def _det_and_scene(device):
    from nerfdet_amd import synth
    from test_detector_gpu import _small_detector
    det = _small_detector(device)
    batch = synth.batch_to(synth.train_scene(6, (64, 96), t_views=2, n_boxes=2, seed=4), device)
    meta = batch["img_metas"][0]
    rb = det._ray_batch(batch)
    return det, batch["img"], batch["denorm_images"], meta, rb


def _feed(scene, img, dn, meta, splits):
    for v0, v1 in splits:
        scene.add_views(img[:, v0:v1], dn[:, v0:v1], _chunk_meta(meta, v0, v1))
    return scene


def _same_detections(a, b):
    a, b = a[0], b[0]
    assert torch.equal(a["labels_3d"], b["labels_3d"]) and torch.equal(a["scores_3d"], b["scores_3d"])
    assert torch.equal(a["boxes_3d"].tensor, b["boxes_3d"].tensor)


def test_single_chunk_render_equals_render_testing(device):
    """D-a: one chunk with all 6 views: ``scene.render`` is ``extract_feat``'s render_testing result bit for bit; keeping the views does not
    change the detections."""
    from nerfdet_amd import rays
    det, img, dn, meta, rb = _det_and_scene(device)
    det.render_testing = True
    try:
        with pytest.raises(NotImplementedError):
            det.begin_scene(dict(meta))
        with torch.no_grad():
            want = det.extract_feat(img, [dict(meta)], "test", ray_batch=rb)[3][0]
        scene = _feed(det.begin_scene(dict(meta), keep_views=True), img, dn, meta, [(0, 6)])
    finally:
        det.render_testing = False
    got = scene.render(rb)
    t, hh, ww = 2, 44, 76
    assert got["outputs_coarse"]["rgb"].shape == (t, hh, ww, 3) and got["outputs_coarse"]["depth"].shape == (t, hh, ww, 1)
    assert torch.equal(got["outputs_coarse"]["rgb"], want["outputs_coarse"]["rgb"])
    assert torch.equal(got["outputs_coarse"]["depth"], want["outputs_coarse"]["depth"])
    assert float(want["outputs_coarse"]["rgb"].abs().max()) > 0
    assert torch.equal(got["gt_rgb"], want["gt_rgb"]) and torch.equal(got["gt_depth"], want["gt_depth"])
    psnr, ssim, err = rays.rendering_metrics(got)
    assert torch.isfinite(psnr) and torch.isfinite(ssim) and err.shape == (hh, ww, 1)
    plain = _feed(det.begin_scene(dict(meta)), img, dn, meta, [(0, 6)])
    assert plain.bank is None
    _same_detections(scene.detect(), plain.detect())


def test_three_chunks_render_equals_one_shot_over_the_bank(device):
    """D-b: chunks [2, 1, 3]: ``render_rays`` against ``render_rays_func`` over the concatenation of the bank's own segments (the maps the
    stream accumulated), so the chunking-dependent scale of the fp16-pair FPN does not enter and no tolerance is needed."""
    from nerfdet_amd import rays
    det, img, dn, meta, rb = _det_and_scene(device)
    scene = _feed(det.begin_scene(dict(meta), keep_views=True), img, dn, meta, [(0, 2), (2, 3), (3, 6)])
    bank = scene.bank
    assert [s.n_views for s in bank.segments] == [2, 1, 3] and bank.n_views == scene.n_views == 6
    assert tuple(bank.segments[0].rgb4.shape[1:]) == (64, 96, 4)
    ray_o, ray_d = rb["ray_o"].view(-1, 3), rb["ray_d"].view(-1, 3)
    assert ray_o.shape[0] <= rays.RENDER_TESTING_RAYS          # one pass on either side
    got = scene.render_rays(ray_o, ray_d)
    feat = torch.cat([s.feat for s in bank.segments]).permute(0, 3, 1, 2)
    rgb = torch.cat([s.rgb4 for s in bank.segments])[..., :3].permute(0, 3, 1, 2)
    assert rays.packed_ok(6, feat.shape[1])
    with torch.no_grad():
        want = rays.render_rays_func(ray_o, ray_d, None, None, feat, rgb, det.aabb, det.near_far_range, det.N_samples, det.N_rand, det.nerf_mlp,
                                     dict(meta), None, "image", det=True)["outputs_coarse"]
    assert got["rgb"].shape == (ray_o.shape[0], 3) and got["depth"].shape == (ray_o.shape[0],) and got["mask"].shape == (ray_o.shape[0],)
    assert torch.equal(got["rgb"], want["rgb"]) and torch.equal(got["depth"], want["depth"]) and torch.equal(got["mask"], want["mask"])
    assert got["mask"].any()
    with pytest.raises(RuntimeError):
        _feed(det.begin_scene(dict(meta)), img, dn, meta, [(0, 6)]).render_rays(ray_o, ray_d)


def test_sliding_window_render(device):
    """D-c: window of 2 chunks fed a, b, c renders what a fresh windowed stream fed b, c renders; the bank follows the states."""
    det, img, dn, meta, rb = _det_and_scene(device)
    ray_o, ray_d = rb["ray_o"].view(-1, 3)[:2048], rb["ray_d"].view(-1, 3)[:2048]
    scene = _feed(det.begin_scene(dict(meta), window=2, keep_views=True), img, dn, meta, [(0, 2), (2, 3), (3, 6)])
    fresh = _feed(det.begin_scene(dict(meta), window=2, keep_views=True), img, dn, meta, [(2, 3), (3, 6)])
    assert scene.bank.n_views == scene.n_views == 4 and [s.n_views for s in scene.bank.segments] == scene.chunk_views == [1, 3]
    got, want = scene.render_rays(ray_o, ray_d), fresh.render_rays(ray_o, ray_d)
    for key in ("rgb", "depth", "mask"):
        assert torch.equal(got[key], want[key]), key
    assert got["mask"].any()
    scene.drop_oldest(1)
    assert scene.bank.n_views == scene.n_views == 3 and len(scene.bank.segments) == 1
    scene.reset()
    assert scene.bank.n_views == scene.n_views == 0 and scene.bank.segments == []
    with pytest.raises(RuntimeError):
        scene.render_rays(ray_o, ray_d)
    with pytest.raises(RuntimeError):
        scene.render(rb)
