"""GPU checks of empty-space skipping (csrc/skip_empty_kernels.hip, rays.OccupancyGrid / cull_points / ray_view_count_bank,
SceneStream / SceneGroup ``skip_empty=``): the bit grid and the ordered cull against the numpy restatement (tests/skip_empty_ref.py) byte
for byte, the count kernel against the bank sampler's own masks, and culled renders against the public pieces run over every sample
with the culled samples' rows zeroed."""
import numpy as np
import pytest
import torch

import skip_empty_ref as R

pytestmark = pytest.mark.gpu

RGB_ATOL = 1e-4      # README: MLP rows regrouped across calls (batched=True): rgb to 1e-4, depth to 1e-4 x far
NEW_KERNELS = {"k_occupancy_bits", "k_cull_count", "k_cull_write", "k_ray_count_bank"}
QUANTILE = 0.5       # the alpha quantile the end-to-end threshold is taken at (the median)

_CACHE = {}


def _i32(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ---- the grid ----
def _grid(nv, seed=11):
    key = ("grid", nv, seed)
    if key not in _CACHE:
        _CACHE[key] = R.grid_case(nv, seed)
    return _CACHE[key]


@pytest.mark.parametrize("nv", [(5, 3, 7), (8, 8, 40), (40, 40, 16), (128, 128, 64)])
def test_occupancy_bits_equal_the_restatement(device, nv):
    """105 bits (a ragged last word); Z crossing a word boundary; cfg5-like; and bits beyond 64 KiB."""
    from nerfdet_amd import ops
    alpha, count, thr = _grid(nv)
    assert np.isnan(alpha).any() and (count == 0).any() and (alpha == thr).any()
    a, c = torch.from_numpy(alpha).to(device), torch.from_numpy(count).to(device)
    n = nv[0] * nv[1] * nv[2]
    for dilate in (0, 1, 2):
        got = ops.occupancy_bits(a, c, nv, float(thr), dilate)
        want = R.occupancy_bits(alpha, count, nv, thr, dilate)
        assert got.dtype == torch.int32 and tuple(got.shape) == ((n + 31) // 32,)
        assert np.array_equal(got.cpu().numpy(), want), f"{nv} dilate {dilate}"
        frac = np.unpackbits(want.view(np.uint8)).sum() / n
        print(f"{nv} dilate {dilate}: {frac:.4f} of the bits set")
        assert 0 < frac < 1, frac
        assert torch.equal(ops.occupancy_bits(a, c, nv, float(thr), dilate), got)


# ---- the cull ----
N_POINTS = [1, 63, 64, 65, 1023, 1024, 1025, 3 * 1024 + 17]
LATTICES = {   # path -> (n_voxels, p0, voxel_size): dyadic sizes make (i - 0.5) vs + p0 and q + 0.5 exact
    "lds": ((5, 3, 7), np.float32([-1.0, 0.5, 2.0]), np.float32([0.25, 0.5, 0.125])),
    "lds_odd": ((40, 40, 16), np.float32([-3.17, -3.23, -0.07]), np.float32([0.16, 0.16, 0.2])),
    "global": ((128, 128, 64), np.float32([-3.0, 1.0, -0.5]), np.float32([0.0625, 0.03125, 0.125])),
}


def _points(nv, p0, vs, n, seed):
    """n points: first the special ones -- per axis the lattice's two outer cell boundaries (where q + 0.5 is an integer on a dyadic
    lattice), their float32 neighbours just outside and just inside each of the six faces, and an inner cell boundary; then NaN and
    +-inf coordinates -- then random ones from a cell and a half outside the lattice on either side; shuffled.  n >= 63 holds them all."""
    rng = np.random.RandomState(seed)
    nvf = np.float32(nv)
    mid = ((nvf // 2) * vs + p0).astype(np.float32)
    special = []
    for k in range(3):
        lo, hi = np.float32(p0[k] + np.float32(-0.5) * vs[k]), np.float32(p0[k] + (nvf[k] - np.float32(0.5)) * vs[k])
        for x in (lo, np.nextafter(lo, np.float32(-np.inf)), np.nextafter(lo, np.float32(np.inf)), hi, np.nextafter(hi, np.float32(np.inf)),
                  np.nextafter(hi, np.float32(-np.inf)), np.float32(p0[k] + np.float32(1.5) * vs[k])):
            c = mid.copy()
            c[k] = x
            special.append(c)
    bad = np.repeat(mid[None], 4, 0)
    bad[0, 0], bad[1, 1], bad[2, 2], bad[3, 0] = np.nan, np.inf, -np.inf, -np.inf
    rand = ((rng.rand(n, 3).astype(np.float32) * (nvf + 2) - np.float32(1.5)) * vs + p0).astype(np.float32)
    pts = np.concatenate([np.float32(special), bad, rand])[:n].copy()
    rng.shuffle(pts)
    return np.ascontiguousarray(pts, dtype=np.float32)


@pytest.mark.parametrize("outside", ["keep", "cull"])
@pytest.mark.parametrize("path", ["lds", "lds_odd", "global"])
def test_cull_equals_the_restatement(device, path, outside):
    from nerfdet_amd import rays
    nv, p0, vs = LATTICES[path]
    n_words = (nv[0] * nv[1] * nv[2] + 31) // 32
    assert (4 * n_words > 64 * 1024) == (path == "global")
    alpha, count, thr = _grid(nv)
    bits = R.occupancy_bits(alpha, count, nv, thr, 1)
    occ = rays.OccupancyGrid(_i32(bits, device), nv, p0, vs, outside)
    some_in = some_out = False
    for n in N_POINTS:
        pts = _points(nv, p0, vs, n, seed=n)
        want_idx, want_pts = R.cull(pts, bits, nv, p0, vs, outside)
        dev_pts = torch.from_numpy(pts).to(device)
        idx, kept = rays.cull_points(dev_pts, occ)
        assert idx.dtype == torch.int32 and kept.dtype == torch.float32 and tuple(kept.shape) == (idx.shape[0], 3)
        assert idx.shape[0] == len(want_idx), f"{path} {outside} n={n}: M {idx.shape[0]} vs {len(want_idx)}"
        assert torch.equal(idx.cpu(), torch.from_numpy(want_idx)), f"{path} {outside} n={n}: idx"
        assert np.array_equal(kept.cpu().numpy().view(np.int32), want_pts.view(np.int32)), f"{path} {outside} n={n}: pts_kept"
        idx2, kept2 = rays.cull_points(dev_pts, occ)
        assert torch.equal(idx2, idx) and torch.equal(kept2.view(torch.int32), kept.view(torch.int32)), "a second call gives other bytes"
        some_in, some_out = some_in or 0 < len(want_idx), some_out or len(want_idx) < n
    assert some_in and some_out


@pytest.mark.parametrize("path", ["lds", "global"])
def test_cull_all_kept_and_none_kept(device, path):
    from nerfdet_amd import rays
    nv, p0, vs = LATTICES[path]
    n_words = (nv[0] * nv[1] * nv[2] + 31) // 32
    ones = torch.full((n_words,), -1, dtype=torch.int32, device=device)
    zeros = torch.zeros((n_words,), dtype=torch.int32, device=device)
    for n in N_POINTS:
        pts = torch.from_numpy(_points(nv, p0, vs, n, seed=n + 1)).to(device)
        idx, kept = rays.cull_points(pts, rays.OccupancyGrid(ones, nv, p0, vs, "keep"))
        assert torch.equal(idx, torch.arange(n, dtype=torch.int32, device=device)) and torch.equal(kept.view(torch.int32), pts.view(torch.int32))
        idx, kept = rays.cull_points(pts, rays.OccupancyGrid(zeros, nv, p0, vs, "cull"))
        assert tuple(idx.shape) == (0,) and tuple(kept.shape) == (0, 3)


# ---- the count kernel ----
@pytest.mark.parametrize("n_v,sizes,hw", [(1, [1], (64, 96)), (2, [2], (64, 96)), (64, [64], (32, 48)), (65, [65], (32, 48)),
                                          (130, [63, 2, 65], (32, 48))])
def test_count_kernel_equals_the_bank_sampler(device, n_v, sizes, hw):
    from nerfdet_amd import rays
    from test_stream_render_gpu import R as RAYS, S, _bank, _inputs
    inp = _inputs(device, n_v, 32, hw)
    bank = _bank(inp, sizes)
    _, pm, vc = rays.ray_view_stats_bank(inp["pts"], bank)
    got_pm, got_vc = rays.ray_view_count_bank(inp["pts"], bank)
    assert tuple(got_pm.shape) == (RAYS, S) and got_pm.dtype == torch.bool and got_vc.dtype == torch.int32
    assert torch.equal(got_pm, pm) and torch.equal(got_vc, vc)
    assert int(vc.max()) > 0 and int(vc.min()) < n_v
    flat_pm, flat_vc = rays.ray_view_count_bank(inp["pts"].view(-1, 3), bank)
    assert torch.equal(flat_pm, pm.view(-1)) and torch.equal(flat_vc, vc.view(-1))


# ---- end to end ----
def _scene(device):
    """_small_detector, synth.train_scene(6, (64, 96), t_views=2), a stream fed [2, 1, 3] with keep_views, its alpha and its rays; made
    once, never changed."""
    key = ("scene", str(device))
    if key not in _CACHE:
        from test_stream_render_gpu import _det_and_scene, _feed
        det, img, dn, meta, rb = _det_and_scene(device)
        scene = _feed(det.begin_scene(dict(meta), keep_views=True), img, dn, meta, [(0, 2), (2, 3), (3, 6)])
        alpha, _, valid = scene._finish()
        thr = float(torch.quantile(alpha, QUANTILE, interpolation="lower"))
        _CACHE[key] = dict(det=det, img=img, dn=dn, meta=meta, rb=rb, scene=scene, alpha=alpha, valid=valid, thr=thr,
                           ray_o=rb["ray_o"].view(-1, 3).contiguous(), ray_d=rb["ray_d"].view(-1, 3).contiguous(),
                           knobs=dict(threshold=thr, dilate=0, outside="cull"))
    return _CACHE[key]


def _keep(occ, pts):
    """The restatement's keep mask of sample points (..., 3), on the points' device, flat."""
    keep = R.keep_mask(pts.detach().cpu().numpy().reshape(-1, 3), occ.bits.cpu().numpy(), occ.n_voxels, np.float32(occ.p0),
                       np.float32(occ.voxel_size), occ.outside)
    return torch.from_numpy(keep).to(pts.device)


def _expected_pass(det, bank, occ, d, pts, z):
    """One pass from the public pieces: the bank sampler and nerf_mlp over ALL points, sigma and rgb zeroed where the restatement culls,
    raw2outputs.  Returns ``(outputs, keep (c, ss))``."""
    from nerfdet_amd import rays
    glob, pm, _ = rays.ray_view_stats_bank(pts, bank)
    mlp = det.nerf_mlp if pts.shape[1] == det.N_samples else (lambda p, dd, g: rays.fine_mlp(det.nerf_mlp, p, dd, g))
    rgb, sigma = mlp(pts, d, glob)
    keep = _keep(occ, pts).view(pts.shape[:2])
    raw = torch.cat([rgb, sigma], dim=-1)
    raw[~keep] = 0.0
    return rays.raw2outputs(raw, z, pm), keep


def _expected(det, bank, occ, ray_o, ray_d):
    from nerfdet_amd import rays
    outs, kept = [], 0
    with torch.no_grad():
        for i in range(0, ray_o.shape[0], rays.RENDER_TESTING_RAYS):
            o, d = ray_o[i:i + rays.RENDER_TESTING_RAYS], ray_d[i:i + rays.RENDER_TESTING_RAYS]
            pts, z = rays.sample_along_camera_ray(o, d, det.near_far_range, det.N_samples, det=True)
            out, keep = _expected_pass(det, bank, occ, d, pts, z)
            outs.append(out)
            kept += int(keep.sum())
    return {k: torch.cat([o[k] for o in outs]) for k in ("rgb", "depth", "mask")}, kept


def _close(got, want, far, what):
    """README's bound for MLP rows regrouped across calls is 1e-4 on rgb and 1e-4 x far on depth.  Measured on an MI355X every
    difference is 0 -- the radiance MLP's launches scale per row (the fused trunk) or not at all (the bf16x3 ``linear_rows`` layers), so a
    row's result does not depend on the rows it shares a call with -- and the comparison is therefore ``torch.equal``."""
    assert torch.equal(got["mask"], want["mask"]), f"{what}: mask differs"
    e_rgb, e_depth = float((got["rgb"] - want["rgb"]).abs().max()), float((got["depth"] - want["depth"]).abs().max())
    print(f"{what}: max |rgb diff| {e_rgb:.3e}, max |depth diff| {e_depth:.3e} (far {far})")
    assert e_rgb <= RGB_ATOL and e_depth <= RGB_ATOL * far, f"{what}: rgb {e_rgb:.3e}, depth {e_depth:.3e}"
    assert torch.equal(got["rgb"], want["rgb"]) and torch.equal(got["depth"], want["depth"]), f"{what}: rgb {e_rgb:.3e}, depth {e_depth:.3e}"


def test_culled_render_equals_the_public_pieces(device, monkeypatch):
    """Two passes (4096 rays a pass over 6688 rays) at the median alpha, dilate 0, outside culled."""
    from nerfdet_amd import rays, streaming
    c = _scene(device)
    det, scene = c["det"], c["scene"]
    monkeypatch.setattr(rays, "RENDER_TESTING_RAYS", 4096)
    occ = scene.occupancy(**c["knobs"])
    assert scene.occupancy(**c["knobs"]) is occ
    want_bits = R.occupancy_bits(c["alpha"].cpu().numpy(), c["valid"].cpu().numpy(), occ.n_voxels, np.float32(c["thr"]), 0)
    assert np.array_equal(occ.bits.cpu().numpy(), want_bits)
    assert occ.n_voxels == tuple(int(v) for v in det.n_voxels) and occ.outside == "cull"
    assert occ.p0 == tuple(float(v) for v in scene.points[:, 0, 0, 0].cpu())
    got = scene.render_rays(c["ray_o"], c["ray_d"], skip_empty=c["knobs"])
    want, kept = _expected(det, scene.bank, occ, c["ray_o"], c["ray_d"])
    assert got["n_samples"] == c["ray_o"].shape[0] * det.N_samples and got["n_kept"] == kept
    frac = got["n_kept"] / got["n_samples"]
    print(f"kept {got['n_kept']} of {got['n_samples']} samples ({frac:.4f}) at the {QUANTILE} quantile of alpha = {c['thr']:.6f}")
    assert 0.05 < frac < 0.95
    _close(got, want, float(det.near_far_range[1]), "culled render")
    assert got["mask"].any() and float(got["rgb"].abs().max()) > 0
    # the same grid handed over, and the same result on a second call
    again = scene.render_rays(c["ray_o"], c["ray_d"], skip_empty=occ)
    for key in ("rgb", "depth", "mask"):
        assert torch.equal(again[key], got[key]), key
    # the weights of culled samples are exactly 0 (one pass, from the shading step itself)
    o, d = c["ray_o"][:4096], c["ray_d"][:4096]
    with torch.no_grad():
        pts, z = rays.sample_along_camera_ray(o, d, det.near_far_range, det.N_samples, det=True)
        out, m = streaming._culled_shade(det, scene.bank, occ, d, pts, z)
    keep = _keep(occ, pts)
    assert m == int(keep.sum()) and 0 < m < keep.numel()
    w = out["weights"].reshape(-1)
    assert torch.equal(w[~keep], torch.zeros_like(w[~keep])) and float(w[keep].max()) > 0


def test_mlp_calls_of_a_culled_pass_are_split_by_rows(device, monkeypatch):
    """FINE_MLP_ROWS below the kept count: several nerf_mlp calls per pass, the same bounds."""
    from nerfdet_amd import rays
    c = _scene(device)
    det, scene = c["det"], c["scene"]
    occ = scene.occupancy(**c["knobs"])
    want, kept = _expected(det, scene.bank, occ, c["ray_o"], c["ray_d"])
    monkeypatch.setattr(rays, "FINE_MLP_ROWS", kept // 3 + 1)
    got = scene.render_rays(c["ray_o"], c["ray_d"], skip_empty=occ)
    assert got["n_kept"] == kept
    _close(got, want, float(det.near_far_range[1]), "three MLP calls")


def test_a_threshold_below_every_alpha_keeps_everything(device):
    c = _scene(device)
    det, scene = c["det"], c["scene"]
    assert float(c["alpha"].min()) >= 0.0
    got = scene.render_rays(c["ray_o"], c["ray_d"], skip_empty=dict(threshold=-1.0, dilate=0, outside="keep"))
    assert got["n_kept"] == got["n_samples"] == c["ray_o"].shape[0] * det.N_samples
    _close(got, scene.render_rays(c["ray_o"], c["ray_d"]), float(det.near_far_range[1]), "everything kept against the plain render")


def test_no_sample_kept(device):
    from nerfdet_amd import rays, trace
    c = _scene(device)
    det, scene = c["det"], c["scene"]
    real = scene.occupancy(**c["knobs"])
    empty = rays.OccupancyGrid(torch.zeros_like(real.bits), real.n_voxels, real.p0, real.voxel_size, "cull")
    o, d = c["ray_o"][:2000], c["ray_d"][:2000]
    trace.recorder = trace.Recorder()
    try:
        got = scene.render_rays(o, d, skip_empty=empty)
        names = {s[0] for s in trace.recorder.spans}
    finally:
        trace.recorder = None
    assert got["n_kept"] == 0 and got["n_samples"] == 2000 * det.N_samples
    assert "k_ray_count_bank" in names and "k_cull_count" in names and not names & {"k_cull_write", "k_ray_stats_bank"}
    with torch.no_grad():
        pts, z = rays.sample_along_camera_ray(o, d, det.near_far_range, det.N_samples, det=True)
        pm = rays.ray_view_stats_bank(pts, scene.bank)[1]
        want = rays.raw2outputs(torch.zeros(pts.shape[:2] + (4,), device=device), z, pm)
    for key in ("rgb", "depth", "mask"):
        assert torch.equal(got[key], want[key]), key
    assert torch.equal(got["mask"], scene.render_rays(o, d)["mask"]) and got["mask"].any()
    assert torch.equal(got["rgb"], torch.zeros_like(got["rgb"]))


def test_importance_pass_over_the_culled_weights(device):
    from nerfdet_amd import rays, streaming
    c = _scene(device)
    det, scene = c["det"], c["scene"]
    occ = scene.occupancy(**c["knobs"])
    o, d = c["ray_o"][:3000], c["ray_d"][:3000]
    got = scene.render_rays(o, d, n_importance=8, skip_empty=occ)
    coarse = scene.render_rays(o, d, skip_empty=occ)
    for key in ("rgb", "depth", "mask"):
        assert torch.equal(got["coarse"][key], coarse[key]), key
    with torch.no_grad():
        pts, z = rays.sample_along_camera_ray(o, d, det.near_far_range, det.N_samples, det=True)
        out_c, m_c = streaming._culled_shade(det, scene.bank, occ, d, pts, z)      # the culled coarse pass: dense weights, 0 where culled
        pts_f, z_f, _ = rays.importance_merge(z, out_c["weights"], o, d, 8, True)
        want, keep_f = _expected_pass(det, scene.bank, occ, d, pts_f, z_f)
    assert tuple(pts_f.shape) == (3000, det.N_samples + 8, 3)
    assert got["n_samples"] == 3000 * (2 * det.N_samples + 8) and got["n_kept"] == m_c + int(keep_f.sum())
    _close(got, want, float(det.near_far_range[1]), "fine pass")


def test_render_frames_packs_its_own_culled_outputs(device):
    from nerfdet_amd import pipeline
    c = _scene(device)
    scene = c["scene"]
    ext = c["meta"]["lidar2img"]["extrinsic"][:2]
    out = scene.render_frames(extrinsic=ext, stride=2, skip_empty=c["knobs"])
    k, h, w = out["rgb"].shape[:3]
    frames, depth_frames = pipeline.pack_frames(out["rgb"].reshape(-1, 3), out["depth"].reshape(-1), out["mask"].reshape(-1), (k, h, w))
    assert torch.equal(out["frames"], frames) and torch.equal(out["depth_frames"], depth_frames)
    assert 0 < out["n_kept"] < out["n_samples"] == k * h * w * c["det"].N_samples
    plain = scene.render_frames(extrinsic=ext, stride=2)
    assert "n_kept" not in plain and torch.equal(plain["mask"], out["mask"])


def test_the_grid_is_dropped_when_the_views_change(device):
    from test_stream_render_gpu import _chunk_meta, _feed
    c = _scene(device)
    det, img, dn, meta = c["det"], c["img"], c["dn"], c["meta"]
    scene = _feed(det.begin_scene(dict(meta), keep_views=True), img, dn, meta, [(0, 2), (2, 3)])
    first = scene.occupancy(**c["knobs"])
    assert scene.occupancy(**c["knobs"]) is first and scene.occupancy(c["thr"], 1, "cull") is not first
    scene.add_views(img[:, 3:6], dn[:, 3:6], _chunk_meta(meta, 3, 6))
    second = scene.occupancy(**c["knobs"])
    assert second is not first and not torch.equal(second.bits, first.bits)
    assert torch.equal(second.bits, c["scene"].occupancy(**c["knobs"]).bits)       # the same chunks: the same grid
    scene.reset()
    with pytest.raises(RuntimeError, match="no views"):
        scene.occupancy(**c["knobs"])


def test_a_window_after_an_eviction_equals_a_fresh_window(device):
    from test_stream_render_gpu import _feed
    c = _scene(device)
    det, img, dn, meta = c["det"], c["img"], c["dn"], c["meta"]
    o, d = c["ray_o"][:2048], c["ray_d"][:2048]
    scene = _feed(det.begin_scene(dict(meta), window=2, keep_views=True), img, dn, meta, [(0, 2), (2, 3)])
    before = scene.occupancy(**c["knobs"])
    _feed(scene, img, dn, meta, [(3, 6)])                     # evicts the first chunk
    fresh = _feed(det.begin_scene(dict(meta), window=2, keep_views=True), img, dn, meta, [(2, 3), (3, 6)])
    a, b = scene.occupancy(**c["knobs"]), fresh.occupancy(**c["knobs"])
    assert a is not before and torch.equal(a.bits, b.bits) and a.p0 == b.p0
    got, want = scene.render_rays(o, d, skip_empty=c["knobs"]), fresh.render_rays(o, d, skip_empty=c["knobs"])
    for key in ("rgb", "depth", "mask"):
        assert torch.equal(got[key], want[key]), key
    assert got["n_kept"] == want["n_kept"] and 0 < got["n_kept"] < got["n_samples"]
    scene.drop_oldest(1)
    assert scene.occupancy(**c["knobs"]) is not a


def test_a_group_of_two_scenes_equals_two_streams(device):
    """Every add_views call lists one scene, so the group's states and banks are the streams' bit for bit (scenes listed together share
    the backbone's fp16-pair scales); each scene's culled render is then the stream's, and each scene has its own grid."""
    from test_group_render_gpu import _chunk_meta, _det_scenes, _feed, _rays_of
    det, scenes = _det_scenes(device)
    calls = [[(0, 0, 3)], [(1, 0, 3)], [(0, 3, 6)], [(1, 3, 6)]]
    group = _feed(det.begin_scenes([dict(scenes[s]["meta"]) for s in (0, 1)], keep_views=True), scenes, calls)
    streams = []
    for s in (0, 1):
        st = det.begin_scene(dict(scenes[s]["meta"]), keep_views=True)
        for a, b in ((0, 3), (3, 6)):
            st.add_views(scenes[s]["img"][:, a:b], scenes[s]["dn"][:, a:b], _chunk_meta(scenes[s]["meta"], a, b))
        streams.append(st)
    thr = float(torch.quantile(streams[0]._finish()[0], QUANTILE, interpolation="lower"))
    knobs = dict(threshold=thr, dilate=0, outside="cull")
    grids = group.occupancy(**knobs)
    assert group.occupancy(**knobs)[1] is grids[1] and group.occupancy(scenes=[1], **knobs)[0] is grids[1]
    for s in (0, 1):
        want = streams[s].occupancy(**knobs)
        assert torch.equal(grids[s].bits, want.bits) and grids[s].p0 == want.p0
    assert grids[0].p0 != grids[1].p0 and not torch.equal(grids[0].bits, grids[1].bits)
    ray_o, ray_d = zip(*[_rays_of(scenes[s], 1500 + 300 * s) for s in (0, 1)])
    got = group.render_rays(list(ray_o), list(ray_d), skip_empty=knobs)
    for s in (0, 1):
        want = streams[s].render_rays(ray_o[s], ray_d[s], skip_empty=knobs)
        for key in ("rgb", "depth", "mask"):
            assert torch.equal(got[s][key], want[key]), (s, key)
        assert got[s]["n_kept"] == want["n_kept"] and got[s]["n_samples"] == want["n_samples"] and 0 < want["n_kept"] < want["n_samples"]
    one = group.render_rays([ray_o[1]], [ray_d[1]], scenes=[1], n_importance=4, skip_empty=knobs)[0]
    want = streams[1].render_rays(ray_o[1], ray_d[1], n_importance=4, skip_empty=knobs)
    assert torch.equal(one["rgb"], want["rgb"]) and torch.equal(one["coarse"]["depth"], want["coarse"]["depth"]) and one["n_kept"] == want["n_kept"]
    frames = group.render_frames(extrinsic=[scenes[s]["meta"]["lidar2img"]["extrinsic"][:1] for s in (0, 1)], stride=4, skip_empty=knobs)
    for s in (0, 1):
        want = streams[s].render_frames(extrinsic=scenes[s]["meta"]["lidar2img"]["extrinsic"][:1], stride=4, skip_empty=knobs)
        assert torch.equal(frames[s]["frames"], want["frames"]) and torch.equal(frames[s]["depth_frames"], want["depth_frames"])
        assert frames[s]["n_kept"] == want["n_kept"]
    with pytest.raises(ValueError, match="batched"):
        group.render_rays(list(ray_o), list(ray_d), batched=True, skip_empty=knobs)
    group.add_views(scenes[1]["img"][:, 0:1], scenes[1]["dn"][:, 0:1], [_chunk_meta(scenes[1]["meta"], 0, 1)], scenes=[1])
    after = group.occupancy(**knobs)
    assert after[0] is grids[0] and after[1] is not grids[1]       # only the listed scene's grid is dropped


def test_the_default_makes_todays_launches(device):
    from nerfdet_amd import trace
    c = _scene(device)
    scene = c["scene"]
    o, d = c["ray_o"][:2048], c["ray_d"][:2048]
    want = scene.render_rays(o, d)
    trace.recorder = trace.Recorder()
    try:
        got = scene.render_rays(o, d, skip_empty=None)
        plain = [s[0] for s in trace.recorder.spans]
        trace.recorder = trace.Recorder()
        culled = scene.render_rays(o, d, skip_empty=c["knobs"])
        with_grid = {s[0] for s in trace.recorder.spans}
    finally:
        trace.recorder = None
    assert list(got) == ["rgb", "depth", "mask"]
    for key in got:
        assert torch.equal(got[key], want[key]), key
    assert "k_ray_stats_bank" in plain and not set(plain) & NEW_KERNELS
    assert {"k_ray_count_bank", "k_cull_count", "k_cull_write", "k_ray_stats_bank"} <= with_grid and culled["n_kept"] > 0


def test_culled_calls_refuse_before_any_launch(device):
    from nerfdet_amd import rays, trace
    c = _scene(device)
    det, scene = c["det"], c["scene"]
    o, d = c["ray_o"][:64], c["ray_d"][:64]
    real = scene.occupancy(**c["knobs"])
    other = rays.OccupancyGrid(torch.zeros(((4 * 4 * 4 + 31) // 32,), dtype=torch.int32, device=device), (4, 4, 4), real.p0, real.voxel_size)
    trace.recorder = trace.Recorder()
    try:
        for bad in (dict(dilate=3), dict(threshold=float("inf")), dict(outside="drop"), dict(quantile=0.5), 7):
            with pytest.raises(ValueError):
                scene.render_rays(o, d, skip_empty=bad)
        with pytest.raises(ValueError, match="n_voxels"):
            scene.render_rays(o, d, skip_empty=other)
        with pytest.raises(ValueError):
            scene.render_frames(extrinsic=c["meta"]["lidar2img"]["extrinsic"][:1], skip_empty=dict(dilate=-1))
        with pytest.raises(RuntimeError, match="GPU"):
            scene.render_rays(o.cpu(), d.cpu(), skip_empty=True)
        det.train()
        try:
            with pytest.raises(RuntimeError, match="inference only"):
                scene.render_rays(o, d, skip_empty=True)
        finally:
            det.eval()
        plain = det.begin_scene(dict(c["meta"]))
        with pytest.raises(RuntimeError, match="keep_views"):
            plain.render_rays(o, d, skip_empty=True)
        assert trace.recorder.spans == []
    finally:
        trace.recorder = None
