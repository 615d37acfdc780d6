"""``n_importance=`` on SceneStream and SceneGroup renders (nerfdet_amd/streaming.py) with the small detector of
tests/test_stream_render_gpu.py and tests/test_group_render_gpu.py: a stream's fine pass is rays.render_rays_func(N_importance=k) over the
bank's own maps bit for bit, a group's is each scene's stream bit for bit (``batched=True``: within the project's bound for scenes that
share a launch's scales) in one k_importance_merge launch and two grouped sampler launches a pass, and ``n_importance=0`` is untouched."""
import pytest
import torch

from test_group_render_gpu import CALLS, _chunk_meta, _det_scenes, _fed_meta, _feed, _rays_of, _same_render

pytestmark = pytest.mark.gpu
K = 16


def _bank_maps(bank):
    feat = torch.cat([s.feat for s in bank.segments]).permute(0, 3, 1, 2)
    rgb = torch.cat([s.rgb4 for s in bank.segments])[..., :3].permute(0, 3, 1, 2)
    return feat, rgb


def _func_passes(det, bank, meta, ray_o, ray_d, k):
    """rays.render_rays_func(det=True, N_importance=k) over the concatenation of the bank's segments, RENDER_TESTING_RAYS rays a pass."""
    from nerfdet_amd import rays
    feat, rgb = _bank_maps(bank)
    assert rays.packed_ok(feat.shape[0], feat.shape[1])
    coarse, fine = [], []
    with torch.no_grad():
        for i in range(0, ray_o.shape[0], rays.RENDER_TESTING_RAYS):
            o, d = ray_o[i:i + rays.RENDER_TESTING_RAYS], ray_d[i:i + rays.RENDER_TESTING_RAYS]
            ret = rays.render_rays_func(o, d, None, None, feat, rgb, det.aabb, det.near_far_range, det.N_samples, det.N_rand, det.nerf_mlp,
                                        meta, None, "image", N_importance=k, det=True)
            coarse.append(ret["outputs_coarse"])
            fine.append(ret["outputs_fine"])
    cat = lambda outs: {key: torch.cat([o[key] for o in outs]) for key in ("rgb", "depth", "mask")}
    return cat(coarse), cat(fine)


def _stream(det, sc, splits):
    scene = det.begin_scene(dict(sc["meta"]), keep_views=True)
    for a, b in splits:
        scene.add_views(sc["img"][:, a:b], sc["dn"][:, a:b], _chunk_meta(sc["meta"], a, b))
    return scene


def _stream_over(det, sc, bank):
    """A SceneStream holding the SAME maps as a group's bank (its segments, shared): the maps a group accumulates depend on the scenes that
    shared its backbone calls (per-tensor fp16-pair scales), so "its stream" is the stream over these maps, as in
    tests/test_group_render_gpu.py."""
    scene = det.begin_scene(dict(sc["meta"]), keep_views=True)
    for seg in bank.segments:
        scene.bank.push(seg)
    return scene


@pytest.mark.parametrize("splits", [[(0, 6)], [(0, 2), (2, 3), (3, 6)]])
def test_stream_render_rays_is_render_rays_func(device, splits):
    det, scenes = _det_scenes(device)
    sc = scenes[0]
    scene = _stream(det, sc, splits)
    o, d = sc["rb"]["ray_o"].view(-1, 3), sc["rb"]["ray_d"].view(-1, 3)
    plain = scene.render_rays(o, d)
    got = scene.render_rays(o, d, n_importance=K)
    assert list(plain) == ["rgb", "depth", "mask"] and list(got) == ["rgb", "depth", "mask", "coarse"] and list(got["coarse"]) == ["rgb", "depth", "mask"]
    coarse, fine = _func_passes(det, scene.bank, _fed_meta(sc, splits), o, d, K)
    _same_render(got, fine, "the fine pass")
    _same_render(got["coarse"], coarse, "the coarse pass of a fine render")
    _same_render(plain, coarse, "n_importance=0")
    assert got["mask"].any() and not torch.equal(got["depth"], plain["depth"])
    for bad in (-1, 257, 1.5, True):
        with pytest.raises(ValueError, match="n_importance"):
            scene.render_rays(o, d, n_importance=bad)


def test_stream_render_returns_outputs_fine_like_render_testing(device):
    from nerfdet_amd import rays
    det, scenes = _det_scenes(device)
    sc = scenes[1]
    scene = _stream(det, sc, [(0, 6)])
    plain, got = scene.render(sc["rb"]), scene.render(sc["rb"], n_importance=K)
    assert set(got) == set(plain) | {"outputs_fine"} and "outputs_fine" not in plain
    feat, rgb = _bank_maps(scene.bank)
    with torch.no_grad():
        want = rays.render_rays(sc["rb"], None, None, feat, rgb, det.aabb, det.near_far_range, det.N_samples, det.N_rand, det.nerf_mlp,
                                dict(sc["meta"]), None, "image", N_importance=K, is_train=False, render_testing=True)
        base = rays.render_rays(sc["rb"], None, None, feat, rgb, det.aabb, det.near_far_range, det.N_samples, det.N_rand, det.nerf_mlp,
                                dict(sc["meta"]), None, "image", is_train=False, render_testing=True)
    assert "outputs_fine" not in base and set(want) == set(got)
    for which in ("outputs_coarse", "outputs_fine"):
        for key in ("rgb", "depth"):
            assert got[which][key].shape == want[which][key].shape and torch.equal(got[which][key], want[which][key]), (which, key)
    for key in ("rgb", "depth"):
        assert torch.equal(plain["outputs_coarse"][key], base["outputs_coarse"][key]) and torch.equal(plain["outputs_coarse"][key], got["outputs_coarse"][key])
    psnr_c, ssim_c, _ = rays.rendering_metrics(got)
    psnr_f, ssim_f, err_f = rays.rendering_metrics(got, which="outputs_fine")
    assert torch.isfinite(psnr_f) and torch.isfinite(ssim_f) and err_f.shape == got["outputs_fine"]["depth"].shape[1:]
    assert torch.equal(psnr_c, rays.rendering_metrics(plain)[0])


def test_group_fine_pass_is_each_scenes_stream(device):
    """Ray counts 3000, 2048 and RENDER_TESTING_RAYS + 5 (two passes, two scenes running out early): every listed scene equals its
    stream bit for bit, for a subset listed out of order too; per pass exactly one k_importance_merge launch and two grouped sampler
    launches; batched=True within the project's bound for scenes sharing a launch's scales; n_importance=0 is today's result."""
    from nerfdet_amd import rays, trace
    det, scenes = _det_scenes(device)
    group = _feed(det.begin_scenes([dict(sc["meta"]) for sc in scenes], keep_views=True), scenes, CALLS)
    streams = [_stream_over(det, scenes[s], group.banks[s]) for s in range(3)]
    counts = [3000, 2048, rays.RENDER_TESTING_RAYS + 5]
    assert counts[2] == 8197
    rr = [_rays_of(sc, n) for sc, n in zip(scenes, counts)]
    o, d = [r[0] for r in rr], [r[1] for r in rr]
    want = [st.render_rays(a, b, n_importance=K) for st, a, b in zip(streams, o, d)]
    want0 = [st.render_rays(a, b) for st, a, b in zip(streams, o, d)]

    rec = trace.Recorder()
    trace.recorder = rec
    try:
        got = group.render_rays(o, d, n_importance=K)
    finally:
        trace.recorder = None
    names = [name for name, *_ in rec.spans]
    passes = 2
    assert names.count("k_importance_merge") == passes, names
    assert names.count("k_ray_stats_bank_group") == 2 * passes, names
    assert names.count("k_ray_stats_bank") == 0 and names.count("k_sample_pdf") == 0
    for s in range(3):
        assert list(got[s]) == ["rgb", "depth", "mask", "coarse"]
        _same_render(got[s], want[s], f"scene {s}, fine")
        _same_render(got[s]["coarse"], want[s]["coarse"], f"scene {s}, coarse")
        _same_render(got[s]["coarse"], want0[s], f"scene {s}, coarse against n_importance=0")
        assert got[s]["rgb"].shape == (counts[s], 3) and got[s]["mask"].any()

    rec = trace.Recorder()
    trace.recorder = rec
    try:
        got0 = group.render_rays(o, d)
    finally:
        trace.recorder = None
    names = [name for name, *_ in rec.spans]
    assert names.count("k_importance_merge") == 0 and names.count("k_ray_stats_bank_group") == passes
    for s in range(3):
        assert list(got0[s]) == ["rgb", "depth", "mask"]
        _same_render(got0[s], want0[s], f"scene {s}, n_importance=0")

    sub = group.render_rays([o[2], o[0]], [d[2], d[0]], scenes=[2, 0], n_importance=K)
    _same_render(sub[0], want[2], "scenes=[2, 0]: scene 2")
    _same_render(sub[1], want[0], "scenes=[2, 0]: scene 0")

    bat = group.render_rays(o, d, batched=True, n_importance=K)
    far = float(det.near_far_range[1])
    for s in range(3):
        e_rgb = float((bat[s]["rgb"] - want[s]["rgb"]).abs().max())
        e_depth = float((bat[s]["depth"] - want[s]["depth"]).abs().max())
        print(f"scene {s}: batched fine pass against the stream: max |rgb| {e_rgb:.3e} (bound 1e-4), max |depth| {e_depth:.3e} (bound {1e-4 * far:.3e})")
        assert torch.equal(bat[s]["mask"], want[s]["mask"]) and torch.equal(bat[s]["coarse"]["mask"], want[s]["coarse"]["mask"])
        assert e_rgb <= 1e-4 and e_depth <= 1e-4 * far


def test_group_render_outputs_fine(device):
    det, scenes = _det_scenes(device)
    group = _feed(det.begin_scenes([dict(sc["meta"]) for sc in scenes], keep_views=True), scenes, CALLS)
    listed = [1, 2]
    plain = group.render([scenes[s]["rb"] for s in listed], scenes=listed)
    got = group.render([scenes[s]["rb"] for s in listed], scenes=listed, n_importance=K)
    for s, p, g in zip(listed, plain, got):
        assert set(g) == set(p) | {"outputs_fine"} and "outputs_fine" not in p
        want = _stream_over(det, scenes[s], group.banks[s]).render(scenes[s]["rb"], n_importance=K)
        for which in ("outputs_coarse", "outputs_fine"):
            for key in ("rgb", "depth"):
                assert torch.equal(g[which][key], want[which][key]), (s, which, key)
        for key in ("rgb", "depth"):
            assert torch.equal(p["outputs_coarse"][key], g["outputs_coarse"][key])


def test_a_split_fine_mlp_is_split_alike_everywhere(device, monkeypatch):
    """With the row cap lowered so that the fine pass's MLP runs in three calls (rays.fine_mlp), stream, group and render_rays_func still
    agree bit for bit: the split depends on (rays, samples) alone."""
    from nerfdet_amd import rays
    det, scenes = _det_scenes(device)
    sc = scenes[2]
    splits = [(0, 3), (3, 6)]
    scene = _stream(det, sc, splits)
    o, d = _rays_of(sc, 1000)
    whole = scene.render_rays(o, d, n_importance=K)
    monkeypatch.setattr(rays, "FINE_MLP_ROWS", 400 * (det.N_samples + K))
    seen = []
    mlp = det.nerf_mlp.forward
    monkeypatch.setattr(det.nerf_mlp, "forward", lambda x, *a, **k: (seen.append(x.shape[0]), mlp(x, *a, **k))[1])
    got = scene.render_rays(o, d, n_importance=K)
    assert seen == [1000, 334, 334, 332], seen          # the coarse pass whole, then ceil(1000 / 400) = 3 calls of at most 334 rays
    coarse, fine = _func_passes(det, scene.bank, _fed_meta(sc, splits), o, d, K)
    _same_render(got, fine, "the split fine pass")
    _same_render(got["coarse"], whole["coarse"], "the coarse pass")
    group = det.begin_scenes([dict(sc["meta"])], keep_views=True)
    for seg in scene.bank.segments:
        group.banks[0].push(seg)
    _same_render(group.render_rays([o], [d], n_importance=K)[0], got, "a group over the same maps")
