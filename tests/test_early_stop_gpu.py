"""GPU checks of early ray termination (csrc/early_stop_kernels.hip, rays.advance_transmittance / front_segment, SceneStream / SceneGroup
``early_stop=``): the transmittance state against the compositor's own ``transparency`` bit for bit, the ordered compaction of the live
rays' samples against the numpy restatement (tests/early_stop_ref.py) byte for byte, and stopped renders against their definition: the
public pieces run over every sample with the raw rows of stopped (ray, segment) pairs zeroed."""
import numpy as np
import pytest
import torch

import early_stop_ref as E
import skip_empty_ref as SE
from test_skip_empty_gpu import LATTICES, _close, _grid, _i32, _keep, _points, _scene

pytestmark = pytest.mark.gpu

NEW_KERNELS = {"k_ray_advance", "k_front_count", "k_front_write"}
N_RAYS = [1, 63, 64, 65, 1000]
N_COLS = [5, 64, 69]
WIDTHS = [4, 8, 16, 32]
SIGMAS = np.float32([0.0, 1e-3, 0.5, 3.0, 20.0, 200.0])
EPS = 1e-3
# The end-to-end eps values.  Along the fixture's 6688 rays the sample alphas have the median 0.89, so the plain transparency falls fast:
# at column 4 it spans 4.5e-5 .. 7.2e-2 (median 1.4e-3), at column 60 its 99th percentile is 3.8e-37 and its maximum 2.4e-27 (measured on
# an MI355X).  At eps = 1e-3 every ray has therefore stopped by column 12 (2267 at 4, 4415 at 8, 6 at 12, none never): the default is
# covered, but it cannot show a ray that never stops.  The two PATTERN values lie below the largest final transparency, so that rays stop
# at many different boundaries (at 1e-30: 28 .. 60, 164 .. 13 rays each) and a few never do (5 at 1e-30); the pattern is asserted on the
# expected result, not assumed.
PATTERN_EPS = [1e-30, 1e-36]
EPS_E2E = [EPS] + PATTERN_EPS

_CACHE = {}


def _raw_case(device, r, s):
    """(raw (r, s, 4), z (r, s), the compositor's transparency (r, s)): sigma drawn from SIGMAS, random rgb; made once, never changed."""
    key = ("raw", str(device), r, s)
    if key not in _CACHE:
        from nerfdet_amd import rays
        rng = np.random.RandomState(1000 * r + s)
        raw = np.concatenate([rng.rand(r, s, 3).astype(np.float32), SIGMAS[rng.randint(0, len(SIGMAS), (r, s, 1))]], axis=-1)
        raw = torch.from_numpy(np.ascontiguousarray(raw)).to(device)
        z = torch.linspace(0.2, 5.0, s, device=device).repeat(r, 1).contiguous()
        _CACHE[key] = (raw, z, rays.raw2outputs(raw, z, None)["transparency"])
    return _CACHE[key]


# ---- 1. the transmittance state ----
@pytest.mark.parametrize("s", N_COLS)
@pytest.mark.parametrize("r", N_RAYS)
def test_advance_equals_the_compositor(device, r, s):
    from nerfdet_amd import rays
    raw, z, trans = _raw_case(device, r, s)
    assert torch.equal(trans[:, 0], torch.ones(r, device=device))
    for w in WIDTHS:
        T = torch.ones(r, device=device)
        for b in range(w, s, w):
            assert rays.advance_transmittance(raw, T, b - w, b) is T
            assert torch.equal(T, trans[:, b]), f"R {r} S {s} w {w}: T at boundary {b}"
        before = T.clone()
        rays.advance_transmittance(raw, T, s, s)                # a no-op
        assert torch.equal(T, before)
    if r >= 63:
        assert float(trans[:, -1].min()) < EPS < float(trans[:, 1].max())      # both sides of a stop occur


def test_a_nan_sigma_gives_a_nan_transmittance_and_the_ray_is_kept(device):
    from nerfdet_amd import rays
    raw, z, _ = _raw_case(device, 65, 69)
    raw = raw.clone()
    raw[7, 2, 3] = float("nan")
    trans = rays.raw2outputs(raw, z, None)["transparency"]
    T = torch.ones(65, device=device)
    rays.advance_transmittance(raw, T, 0, 4)
    assert torch.isnan(T[7]) and int(torch.isnan(T).sum()) == 1 and torch.isnan(trans[7, 4])
    assert torch.equal(torch.nan_to_num(T, nan=-1.0), torch.nan_to_num(trans[:, 4], nan=-1.0))
    pts = torch.rand(65, 69, 3, device=device)
    idx, _ = rays.front_segment(pts, T, 4, 8, EPS)
    assert (idx // 69 == 7).sum() == 4                          # the NaN ray's four samples are kept


# ---- 2. the front segment ----
def _t_case(r, seed):
    """Transmittances with values below eps, above eps, exactly eps (kept) and NaN (kept), and the condition the comparison rests on: no
    value lies within 1e-4 eps of eps unless it is eps exactly (asserted in float64)."""
    rng = np.random.RandomState(seed)
    eps = np.float32(EPS)
    vals = np.float32([1.0, 0.5, 2e-3, eps, 5e-4, 1e-6, 0.0, np.nan])
    T = vals[rng.randint(0, len(vals), r)]
    if r >= 8:
        T[:8] = vals
        T[8:] = T[8:][rng.permutation(r - 8)]
    t64 = T.astype(np.float64)
    near = np.abs(t64 - np.float64(eps)) <= 1e-4 * np.float64(eps)
    assert np.array_equal(near & ~np.isnan(t64), T == eps), "a transmittance close to eps that was not put there exactly"
    return np.ascontiguousarray(T)


def _segments(s, w):
    """The first, a middle and the last (possibly short) segment of s columns at width w."""
    firsts = list(range(0, s, w))
    return [(a, min(a + w, s)) for a in sorted({firsts[0], firsts[len(firsts) // 2], firsts[-1]})]


@pytest.mark.parametrize("grid", ["none", "lds-keep", "lds-cull", "global-keep", "global-cull"])
def test_front_segment_equals_the_restatement(device, grid):
    from nerfdet_amd import rays
    occ = ref_grid = None
    if grid != "none":
        path, outside = grid.split("-")
        nv, p0, vs = LATTICES[path]
        assert (4 * ((nv[0] * nv[1] * nv[2] + 31) // 32) > 64 * 1024) == (path == "global")
        alpha, count, thr = _grid(nv)
        bits = SE.occupancy_bits(alpha, count, nv, thr, 1)
        occ = rays.OccupancyGrid(_i32(bits, device), nv, p0, vs, outside)
        ref_grid = (bits, nv, p0, vs, outside)
    stopped_some = kept_some = short = False
    for r in N_RAYS:
        T = _t_case(r, seed=r)
        dev_T = torch.from_numpy(T).to(device)
        for s in N_COLS:
            if grid == "none":
                pts = np.random.RandomState(r + s).rand(r, s, 3).astype(np.float32)
            else:
                pts = _points(nv, p0, vs, r * s, seed=r + s).reshape(r, s, 3)
            dev_pts = torch.from_numpy(pts).to(device)
            for w in WIDTHS:
                for s0, s1 in _segments(s, w):
                    want_idx, want_pts = E.front(pts, T, s0, s1, EPS, ref_grid)
                    idx, kept = rays.front_segment(dev_pts, dev_T, s0, s1, EPS, occ)
                    what = f"{grid} R {r} S {s} [{s0}, {s1})"
                    assert idx.dtype == torch.int32 and kept.dtype == torch.float32 and tuple(kept.shape) == (idx.shape[0], 3)
                    assert idx.shape[0] == len(want_idx), f"{what}: M {idx.shape[0]} vs {len(want_idx)}"
                    assert torch.equal(idx.cpu(), torch.from_numpy(want_idx)), f"{what}: idx"
                    assert np.array_equal(kept.cpu().numpy().view(np.int32), want_pts.view(np.int32)), f"{what}: pts_kept"
                    stopped_some, kept_some = stopped_some or len(want_idx) < r * (s1 - s0), kept_some or len(want_idx) > 0
                    short = short or s1 - s0 not in WIDTHS
    assert stopped_some and kept_some and short


# ---- 3. all rays live, all rays stopped, nothing left out ----
@pytest.mark.parametrize("path", ["lds", "global"])
def test_live_rays_through_a_grid_equal_the_cull(device, path):
    from nerfdet_amd import rays
    nv, p0, vs = LATTICES[path]
    alpha, count, thr = _grid(nv)
    occ = rays.OccupancyGrid(_i32(SE.occupancy_bits(alpha, count, nv, thr, 1), device), nv, p0, vs, "cull")
    for r, s in ((65, 69), (1000, 64), (1, 5)):
        pts = torch.from_numpy(_points(nv, p0, vs, r * s, seed=3 * r + s).reshape(r, s, 3)).to(device)
        T = torch.ones(r, device=device)
        for w in WIDTHS:
            for s0, s1 in _segments(s, w):
                idx, kept = rays.front_segment(pts, T, s0, s1, EPS, occ)
                c_idx, c_kept = rays.cull_points(pts[:, s0:s1], occ)
                c_idx = c_idx.to(torch.int64)
                f = (c_idx // (s1 - s0)) * s + s0 + c_idx % (s1 - s0)
                assert torch.equal(idx.to(torch.int64), f) and torch.equal(kept.view(torch.int32), c_kept.view(torch.int32)), (r, s, s0, s1)
                again = rays.front_segment(pts, T, s0, s1, EPS, occ)
                assert torch.equal(again[0], idx) and torch.equal(again[1].view(torch.int32), kept.view(torch.int32)), "other bytes on a second call"
        assert 0 < idx.shape[0] < r * (s1 - s0) or r == 1


def test_all_stopped_and_nothing_left_out(device):
    from nerfdet_amd import rays, trace
    nv, p0, vs = LATTICES["lds"]
    ones = rays.OccupancyGrid(torch.full(((nv[0] * nv[1] * nv[2] + 31) // 32,), -1, dtype=torch.int32, device=device), nv, p0, vs, "keep")
    for r, s in ((65, 69), (1000, 64)):
        pts = torch.from_numpy(_points(nv, p0, vs, r * s, seed=r).reshape(r, s, 3)).to(device)
        for w in WIDTHS:
            for s0, s1 in _segments(s, w):
                every = (torch.arange(r, device=device)[:, None] * s + torch.arange(s0, s1, device=device)[None]).reshape(-1).to(torch.int32)
                for occ in (None, ones):
                    trace.recorder = trace.Recorder()
                    try:
                        idx, kept = rays.front_segment(pts, torch.zeros(r, device=device), s0, s1, EPS, occ)
                        names = [sp[0] for sp in trace.recorder.spans]
                    finally:
                        trace.recorder = None
                    assert tuple(idx.shape) == (0,) and tuple(kept.shape) == (0, 3) and names == ["k_front_count"]      # M = 0: no write launch
                    idx, kept = rays.front_segment(pts, torch.ones(r, device=device), s0, s1, EPS, occ)
                    assert torch.equal(idx, every) and torch.equal(kept.view(torch.int32), pts[:, s0:s1].reshape(-1, 3).view(torch.int32))
                # the caller's word that every ray is live: the same bytes with no count launch and no read
                trace.recorder = trace.Recorder()
                try:
                    idx, kept = rays.front_segment(pts, torch.ones(r, device=device), s0, s1, EPS, all_live=True)
                    names = [sp[0] for sp in trace.recorder.spans]
                finally:
                    trace.recorder = None
                assert names == ["k_front_write"] and torch.equal(idx, every)
                assert torch.equal(kept.view(torch.int32), pts[:, s0:s1].reshape(-1, 3).view(torch.int32))


# ---- end to end: the definition from the public pieces ----
def _expected_pass(det, bank, stop, occ, d, pts, z):
    """One pass by the definition: the bank sampler and nerf_mlp over ALL points give raw_full (the grid's rows zeroed first); for each
    boundary b ascending the rays whose transparency at b is below eps lose their rows from b on; raw2outputs.  Returns ``(outputs,
    rows not zeroed (c, ss) bool, first stopped boundary per ray (ss where never stopped))``."""
    from nerfdet_amd import rays
    c, ss = pts.shape[:2]
    glob, pm, _ = rays.ray_view_stats_bank(pts, bank)
    mlp = det.nerf_mlp if ss == det.N_samples else (lambda p, dd, g: rays.fine_mlp(det.nerf_mlp, p, dd, g))
    rgb, sigma = mlp(pts, d, glob)
    raw_m = torch.cat([rgb, sigma], dim=-1)
    computed = torch.ones((c, ss), dtype=torch.bool, device=pts.device)
    if occ is not None:
        computed = _keep(occ, pts).view(c, ss).clone()
        raw_m[~computed] = 0.0
    eps = torch.tensor(stop["eps"], dtype=torch.float32, device=pts.device)
    at = torch.full((c,), ss, dtype=torch.int64, device=pts.device)
    for b in range(stop["segment"], ss, stop["segment"]):
        stopped = rays.raw2outputs(raw_m, z, pm)["transparency"][:, b] < eps
        raw_m[stopped, b:] = 0.0
        computed[stopped, b:] = False
        at = torch.where(stopped & (at == ss), torch.full_like(at, b), at)
    return rays.raw2outputs(raw_m, z, pm), computed, at


def _expected(det, bank, stop, occ, ray_o, ray_d, n_importance=0):
    from nerfdet_amd import rays
    outs, fines, ats, kept = [], [], [], 0
    with torch.no_grad():
        for i in range(0, ray_o.shape[0], rays.RENDER_TESTING_RAYS):
            o, d = ray_o[i:i + rays.RENDER_TESTING_RAYS], ray_d[i:i + rays.RENDER_TESTING_RAYS]
            pts, z = rays.sample_along_camera_ray(o, d, det.near_far_range, det.N_samples, det=True)
            out, computed, at = _expected_pass(det, bank, stop, occ, d, pts, z)
            outs.append(out)
            ats.append(at)
            kept += int(computed.sum())
            if n_importance:
                pts_f, z_f, _ = rays.importance_merge(z, out["weights"], o, d, n_importance, True)
                out_f, computed_f, _ = _expected_pass(det, bank, stop, occ, d, pts_f, z_f)
                fines.append(out_f)
                kept += int(computed_f.sum())
    cat = lambda res: {k: torch.cat([o[k] for o in res]) for k in ("rgb", "depth", "mask", "weights")}
    return cat(outs), cat(fines) if n_importance else None, torch.cat(ats), kept


def _two_passes(monkeypatch):
    from nerfdet_amd import rays
    monkeypatch.setattr(rays, "RENDER_TESTING_RAYS", 4096)


@pytest.mark.parametrize("eps", EPS_E2E)
def test_stopped_render_equals_the_definition(device, monkeypatch, eps):
    """Two passes (4096 rays a pass over 6688 rays) at segment 4."""
    from nerfdet_amd import rays, streaming
    c = _scene(device)
    det, scene = c["det"], c["scene"]
    _two_passes(monkeypatch)
    stop = dict(eps=eps, segment=4)
    got = scene.render_rays(c["ray_o"], c["ray_d"], early_stop=stop)
    want, _, at, kept = _expected(det, scene.bank, stop, None, c["ray_o"], c["ray_d"])
    ss = det.N_samples
    bounds, counts = torch.unique(at, return_counts=True)
    print(f"eps {eps:g}: rays first stopped at boundary (S = never) " + ", ".join(f"{int(b) if b < ss else 'S'}: {int(n)}" for b, n in zip(bounds, counts)))
    assert int((bounds < ss).sum()) >= 2, "the expected pattern has rays stopped at fewer than two different boundaries"
    if eps in PATTERN_EPS:
        assert int((at == ss).sum()) >= 1, "the expected pattern has no ray that never stopped"
    _close(got, want, float(det.near_far_range[1]), f"stopped render, eps {eps:g}")
    assert got["n_samples"] == c["ray_o"].shape[0] * ss and got["n_kept"] == kept
    print(f"eps {eps:g}: kept {kept} of {got['n_samples']} rows ({kept / got['n_samples']:.4f})")
    assert 0 < kept < got["n_samples"]
    # the weights of stopped samples are exactly 0 (one pass, from the shading step itself)
    o, d = c["ray_o"][:4096], c["ray_d"][:4096]
    with torch.no_grad():
        pts, z = rays.sample_along_camera_ray(o, d, det.near_far_range, ss, det=True)
        out, m = streaming._front_shade(det, scene.bank, None, stop, d, pts, z)
    live = torch.arange(ss, device=device)[None, :] < at[:4096, None]
    assert m == int(live.sum())
    assert torch.equal(out["weights"][~live], torch.zeros_like(out["weights"][~live])) and float(out["weights"][live].max()) > 0
    assert torch.equal(out["weights"], want["weights"][:4096])


def test_eps_zero_equals_the_plain_render(device, monkeypatch):
    c = _scene(device)
    scene = c["scene"]
    _two_passes(monkeypatch)
    plain = scene.render_rays(c["ray_o"], c["ray_d"])
    for segment in (4, 32):
        got = scene.render_rays(c["ray_o"], c["ray_d"], early_stop=dict(eps=0, segment=segment))
        for key in ("rgb", "depth", "mask"):
            assert torch.equal(got[key], plain[key]), (segment, key)
        assert got["n_kept"] == got["n_samples"] == c["ray_o"].shape[0] * c["det"].N_samples


@pytest.mark.parametrize("eps", EPS_E2E)
def test_stopped_render_against_the_plain_render(device, monkeypatch, eps):
    c = _scene(device)
    det, scene = c["det"], c["scene"]
    _two_passes(monkeypatch)
    far = float(det.near_far_range[1])
    stop = dict(eps=eps, segment=4)
    plain = scene.render_rays(c["ray_o"], c["ray_d"])
    got = scene.render_rays(c["ray_o"], c["ray_d"], early_stop=stop)
    at = _expected(det, scene.bank, stop, None, c["ray_o"], c["ray_d"])[2]
    never = at == det.N_samples
    assert (never.any() or eps not in PATTERN_EPS) and (~never).any()
    assert torch.equal(got["mask"], plain["mask"])
    assert torch.equal(got["rgb"][never], plain["rgb"][never]) and torch.equal(got["depth"][never], plain["depth"][never])
    e_rgb =float((got["rgb"][~never] - plain["rgb"][~never]).abs().max())
    e_depth = float((got["depth"][~never] - plain["depth"][~never]).abs().max())
    print(f"eps {eps:g}: on {int((~never).sum())} stopped rays max |rgb diff| {e_rgb:.3e} (bound {eps + 1e-5:.3e}), "
          f"max |depth diff| {e_depth:.3e} (bound {eps * far / (1 - eps) + 1e-5 * far:.3e})")
    assert e_rgb <= eps + 1e-5 and e_depth <= eps * far / (1 - eps) + 1e-5 * far


def test_with_skip_empty_as_well(device, monkeypatch):
    c = _scene(device)
    det, scene = c["det"], c["scene"]
    _two_passes(monkeypatch)
    stop = dict(eps=EPS, segment=4)
    occ = scene.occupancy(**c["knobs"])
    got = scene.render_rays(c["ray_o"], c["ray_d"], skip_empty=c["knobs"], early_stop=stop)
    want, _, at, kept = _expected(det, scene.bank, stop, occ, c["ray_o"], c["ray_d"])
    _close(got, want, float(det.near_far_range[1]), "stopped and culled render")
    assert got["n_kept"] == kept and got["n_samples"] == c["ray_o"].shape[0] * det.N_samples
    only_grid = scene.render_rays(c["ray_o"], c["ray_d"], skip_empty=occ)["n_kept"]
    only_stop = scene.render_rays(c["ray_o"], c["ray_d"], early_stop=stop)["n_kept"]
    print(f"kept rows: both {kept}, the grid alone {only_grid}, stopping alone {only_stop}, of {got['n_samples']}")
    assert 0 < kept <= min(only_grid, only_stop)
    assert torch.equal(got["mask"], scene.render_rays(c["ray_o"], c["ray_d"])["mask"])


def test_fine_pass_over_the_stopped_weights(device):
    c = _scene(device)
    det, scene = c["det"], c["scene"]
    o, d = c["ray_o"][:3000], c["ray_d"][:3000]
    stop = dict(eps=EPS, segment=4)
    got = scene.render_rays(o, d, n_importance=8, early_stop=stop)
    want_c, want_f, _, kept = _expected(det, scene.bank, stop, None, o, d, n_importance=8)
    far = float(det.near_far_range[1])
    _close(got, want_f, far, "fine pass")
    _close(got["coarse"], want_c, far, "coarse pass")
    assert got["n_samples"] == 3000 * (2 * det.N_samples + 8) and got["n_kept"] == kept


def test_mlp_calls_of_a_segment_are_split_by_rows(device, monkeypatch):
    """FINE_MLP_ROWS below the first segment's kept count (4 x 4096 rows): several nerf_mlp calls per segment, the same equalities."""
    from nerfdet_amd import rays
    c = _scene(device)
    det, scene = c["det"], c["scene"]
    _two_passes(monkeypatch)
    stop = dict(eps=EPS, segment=4)
    want, _, _, kept = _expected(det, scene.bank, stop, None, c["ray_o"], c["ray_d"])
    monkeypatch.setattr(rays, "FINE_MLP_ROWS", 4 * 4096 // 3 + 1)
    got = scene.render_rays(c["ray_o"], c["ray_d"], early_stop=stop)
    assert got["n_kept"] == kept
    _close(got, want, float(det.near_far_range[1]), "three MLP calls a segment")


def test_frames_and_scores(device):
    from nerfdet_amd import pipeline
    from test_stream_render_gpu import _chunk_meta
    c = _scene(device)
    scene = c["scene"]
    chunk = _chunk_meta(c["meta"], 4, 6)
    ext = chunk["lidar2img"]["extrinsic"]
    out = scene.render_frames(extrinsic=ext, stride=2, early_stop=True)
    k, h, w = out["rgb"].shape[:3]
    frames, depth_frames = pipeline.pack_frames(out["rgb"].reshape(-1, 3), out["depth"].reshape(-1), out["mask"].reshape(-1), (k, h, w))
    assert torch.equal(out["frames"], frames) and torch.equal(out["depth_frames"], depth_frames)
    assert 0 < out["n_kept"] < out["n_samples"] == k * h * w * c["det"].N_samples
    plain = scene.render_frames(extrinsic=ext, stride=2)
    assert "n_kept" not in plain and torch.equal(plain["mask"], out["mask"])
    moved = (out["frames"].to(torch.int16) - plain["frames"].to(torch.int16)).abs()
    print(f"eps 1e-3: {int((moved > 0).sum())} of {moved.numel()} frame bytes moved, by at most {int(moved.max())}")
    assert int(moved.max()) <= 1
    # score_frames scores that render
    rs = np.random.RandomState(5)
    held = torch.from_numpy(rs.randint(0, 256, (1, 2, 128, 192, 3)).astype(np.uint8)).to(device)
    got = scene.score_frames(held, chunk, stride=2, early_stop=True)
    u8 = pipeline.prepare_frames(held[0], (96, 64), (64, 96), want_u8=True)[2][:, 1:64:2, 1:96:2].contiguous()
    want = pipeline.frame_errors(out["frames"], u8, out["depth_frames"], None)
    for key in ("sse", "n_px", "psnr"):
        assert torch.equal(got[key], want[key]), key
    assert got["n_kept"] == out["n_kept"] and got["n_samples"] == out["n_samples"]
    assert "n_kept" not in scene.score_frames(held, chunk, stride=2)


def test_a_group_of_two_scenes_equals_two_streams(device):
    """Every add_views call lists one scene, so the group's states and banks are the streams' bit for bit; each scene's stopped render is
    then the stream's."""
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
    stop = dict(eps=EPS, segment=8)
    ray_o, ray_d = zip(*[_rays_of(scenes[s], 1500 + 300 * s) for s in (0, 1)])
    got = group.render_rays(list(ray_o), list(ray_d), early_stop=stop)
    for s in (0, 1):
        want = streams[s].render_rays(ray_o[s], ray_d[s], early_stop=stop)
        for key in ("rgb", "depth", "mask"):
            assert torch.equal(got[s][key], want[key]), (s, key)
        assert got[s]["n_kept"] == want["n_kept"] and got[s]["n_samples"] == want["n_samples"] and 0 < want["n_kept"] < want["n_samples"]
    one = group.render_rays([ray_o[1]], [ray_d[1]], scenes=[1], n_importance=4, skip_empty=True, early_stop=stop)[0]
    want = streams[1].render_rays(ray_o[1], ray_d[1], n_importance=4, skip_empty=True, early_stop=stop)
    assert torch.equal(one["rgb"], want["rgb"]) and torch.equal(one["coarse"]["depth"], want["coarse"]["depth"]) and one["n_kept"] == want["n_kept"]
    frames = group.render_frames(extrinsic=[scenes[s]["meta"]["lidar2img"]["extrinsic"][:1] for s in (0, 1)], stride=4, early_stop=stop)
    for s in (0, 1):
        want = streams[s].render_frames(extrinsic=scenes[s]["meta"]["lidar2img"]["extrinsic"][:1], stride=4, early_stop=stop)
        assert torch.equal(frames[s]["frames"], want["frames"]) and torch.equal(frames[s]["depth_frames"], want["depth_frames"])
        assert frames[s]["n_kept"] == want["n_kept"]
    with pytest.raises(ValueError, match="batched"):
        group.render_rays(list(ray_o), list(ray_d), batched=True, early_stop=stop)
    with pytest.raises(ValueError, match="batched"):
        group.render_frames(extrinsic=[scenes[s]["meta"]["lidar2img"]["extrinsic"][:1] for s in (0, 1)], batched=True, early_stop=True)


def test_the_default_makes_todays_launches(device):
    from nerfdet_amd import trace
    c = _scene(device)
    det, scene = c["det"], c["scene"]
    o, d = c["ray_o"][:2048], c["ray_d"][:2048]
    trace.recorder = trace.Recorder()
    try:
        want = scene.render_rays(o, d)
        without = [s[0] for s in trace.recorder.spans]
        trace.recorder = trace.Recorder()
        got = scene.render_rays(o, d, early_stop=None)
        plain = [s[0] for s in trace.recorder.spans]
        trace.recorder = trace.Recorder()
        stopped = scene.render_rays(o, d, early_stop=True)
        with_stop = {s[0] for s in trace.recorder.spans}
    finally:
        trace.recorder = None
    assert list(got) == ["rgb", "depth", "mask"]
    for key in got:
        assert torch.equal(got[key], want[key]), key
    assert plain == without and "k_ray_stats_bank" in plain and not set(plain) & NEW_KERNELS
    assert NEW_KERNELS | {"k_ray_count_bank", "k_ray_stats_bank"} <= with_stop and 0 < stopped["n_kept"] < stopped["n_samples"]


def test_stopped_calls_refuse_before_any_launch(device):
    from nerfdet_amd import trace
    c = _scene(device)
    det, scene = c["det"], c["scene"]
    o, d = c["ray_o"][:64], c["ray_d"][:64]
    ext = c["meta"]["lidar2img"]["extrinsic"][:1]
    trace.recorder = trace.Recorder()
    try:
        for bad in (dict(eps=-1e-3), dict(eps=1), dict(eps=float("nan")), dict(eps="x"), dict(segment=3), dict(segment=64), dict(width=8), 7):
            with pytest.raises(ValueError):
                scene.render_rays(o, d, early_stop=bad)
            with pytest.raises(ValueError):
                scene.render_frames(extrinsic=ext, early_stop=bad)
        with pytest.raises(ValueError):
            scene.render_rays(o, d, skip_empty=True, early_stop=dict(segment=5))      # refused before the grid is made
        with pytest.raises(RuntimeError, match="GPU"):
            scene.render_rays(o.cpu(), d.cpu(), early_stop=True)
        det.train()
        try:
            with pytest.raises(RuntimeError, match=r"early_stop=\) is inference only"):
                scene.render_rays(o, d, early_stop=True)
            with pytest.raises(RuntimeError, match="inference only"):
                scene.render_frames(extrinsic=ext, early_stop=True)
        finally:
            det.eval()
        plain = det.begin_scene(dict(c["meta"]))
        with pytest.raises(RuntimeError, match="keep_views"):
            plain.render_rays(o, d, early_stop=True)
        assert trace.recorder.spans == []
    finally:
        trace.recorder = None
