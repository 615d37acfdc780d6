"""Every projecting kernel at exact image-border and depth edges, against plain-torch CPU references.

The scenes of projection_edges.py put points ON the edges of both projection rules (rounding ties, the first and last pixel, d = 0, the
1e-8 and 1e6 clamps, the strict depth band, zero-padded taps) with dyadic cameras and coordinates, at the first tile, inside a wave and in
the ragged last block, with the edge cameras at view 0, 63, 64 and last.  test_projection_edges_cpu.py shows that every decision is the
same in float32 and float64, so here masks, validity and counts are held to EQUALITY with no sample excused; values are held to the
tolerances of the existing tests of the same kernels (test_volume_gpu.py, test_rays_gpu.py, test_backward_shapes_gpu.py)."""
import copy
import functools

import pytest
import torch

import projection_edges as E
from oracle import nerfdet_oracle as O
from projection_ref import _backproject64, _check, _hits, _k4_ref, _k4_val, EPS32

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]

ATOL = 2e-5                                        # test_volume_gpu.py / test_rays_gpu.py
GATES = [None, torch.float32, torch.float64]
GATE_IDS = ["ungated", "gate32", "gate64"]
MODES = [("float", 1.0), ("det", 1.0)]
MODE_IDS = ["float", "det"]
CHUNKS = {5: (2, 3), 70: (63, 7), 130: (63, 67)}
SEGMENTS = {5: (2, 1, 2), 70: (63, 2, 5), 130: (63, 2, 65)}    # an edge view ends one segment and starts the next


@pytest.fixture
def scatter_mode(request, device):
    from nerfdet_amd import autograd as A
    mode, gscale = request.param
    prev = A.set_deterministic(mode == "det")
    try:
        yield mode == "det", gscale
    finally:
        A.set_deterministic(prev)


# ------------------------------------------------------------------------------------------------------------------------------
# nearest-pixel family
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _nearest_ref(n_v, size, gate_dt, reverse=False):
    """Float64 values over the oracle's float32 decisions (gated: its restatement _backproject64 against the constant map)."""
    s = E.nearest_scene(n_v, size, reverse=reverse)
    dm_f, dm_r = (None, None) if gate_dt is None else (s.depth[gate_dt], s.depth_r[gate_dt])
    vol, valid = _backproject64(s.feat.double(), s.points, s.proj, dm_f, E.BAND)
    mean, cnt, _ = O.aggregate_views(vol, valid)
    mvol, _ = _backproject64(s.mapped.double(), s.points, s.proj, dm_f, E.BAND)
    mvol = mvol + (~valid) * s.bias.double().view(1, -1, 1, 1, 1)            # nerfdet.py:234-243: a view that misses contributes the bias
    rvol, _ = _backproject64(s.rgb.double(), s.points, s.rgb_proj, dm_r, E.BAND)
    glob = O.density_features(mvol, rvol, cnt, torch.eye(s.cm, dtype=torch.float64), torch.zeros(s.cm, dtype=torch.float64))
    return dict(valid=valid, mean=mean, cnt=cnt, glob=glob)


def _gate(s, device, dt, views=slice(None), rgb=True):
    from nerfdet_amd import ops
    if dt is None:
        return None
    return ops.DepthGate(s.depth[dt][views].to(device), s.depth_r[dt][views].to(device) if rgb else None, E.BAND)


def _on(device, s):
    cl = lambda t: t.to(device).contiguous(memory_format=torch.channels_last)
    return cl(s.feat), cl(s.mapped), s.bias.to(device), s.rgb.to(device), s.points.to(device), s.proj.to(device), s.rgb_proj.to(device)


def _check_glob(got, ref, cnt, what):
    """test_volume_gpu.py:123 (values) and :392 (a voxel no view sees: cov exactly 0, mean = n_v fill / 1e-8 to float32 rounding)."""
    got = got.cpu().double()
    seen = cnt.reshape(-1) > 0
    assert seen.any() and (~seen).any()
    torch.testing.assert_close(got[seen], ref[seen], rtol=1e-5, atol=ATOL, msg=lambda m: f"{what}, seen voxels: {m}")
    assert float(got[~seen][:, 1::2].abs().max()) == 0, f"{what}: cov of an unseen voxel"
    torch.testing.assert_close(got[~seen], ref[~seen], rtol=1e-5, atol=ATOL, msg=lambda m: f"{what}, unseen voxels: {m}")


@pytest.mark.parametrize("gate_dt", GATES, ids=GATE_IDS)
@pytest.mark.parametrize("n_v,size", E.NEAREST_SCENES)
def test_backproject_is_the_oracles_gather(device, n_v, size, gate_dt):
    from nerfdet_amd import ops
    s = E.nearest_scene(n_v, size)
    if gate_dt is None:
        vol, valid = O.backproject(s.feat, s.points, s.proj)
        kw = {}
    else:
        vol, valid = _backproject64(s.feat, s.points, s.proj, s.depth[gate_dt], E.BAND)
        kw = dict(depth=s.depth[gate_dt].to(device), voxel_size=E.VOXEL_SIZE)      # already h x w: the resize is the identity
    assert torch.equal(valid, _nearest_ref(n_v, size, gate_dt)["valid"])
    for f in (s.feat.to(device), s.feat.to(device).contiguous(memory_format=torch.channels_last)):
        got, gvalid = ops.backproject(f, s.points.to(device), s.proj.to(device), **kw)
        bad = gvalid.cpu() != valid
        assert not bad.any(), f"validity differs in {int(bad.sum())} pairs, first (view, point) {bad.reshape(n_v, -1).nonzero()[0].tolist()}"
        assert torch.equal(got.cpu(), vol)


@pytest.mark.parametrize("gate_dt", GATES, ids=GATE_IDS)
@pytest.mark.parametrize("n_v,size", E.NEAREST_SCENES)
def test_backproject_aggregate_counts_and_mean(device, n_v, size, gate_dt):
    from nerfdet_amd import ops
    s = E.nearest_scene(n_v, size)
    ref = _nearest_ref(n_v, size, gate_dt)
    f, _, _, _, pts, proj, _ = _on(device, s)
    alpha = 0.25 + 0.5 * torch.rand(s.n, generator=torch.Generator().manual_seed(n_v))
    unseen = ref["cnt"][0] == 0
    assert unseen.any() and (~unseen).any()
    for cl_out in (True, False):
        for a in (None, alpha):
            got, cnt = ops.backproject_aggregate(f, pts, proj, None if a is None else a.to(device), cl_out, depth_gate=_gate(s, device, gate_dt, rgb=False))
            bad = cnt.cpu() != ref["cnt"]
            assert not bad.any(), f"view count differs in {int(bad.sum())} voxels, first {bad.reshape(-1).nonzero()[0].tolist()}"
            exp = ref["mean"] if a is None else a.view(1, *ref["mean"].shape[1:]) * ref["mean"]
            torch.testing.assert_close(got.cpu().double(), exp, rtol=0, atol=ATOL)
            assert (got.cpu()[:, unseen] == 0).all()


@pytest.mark.parametrize("gate_dt", GATES, ids=GATE_IDS)
@pytest.mark.parametrize("n_v,size", E.NEAREST_SCENES)
def test_density_features_packed_and_generic(device, monkeypatch, n_v, size, gate_dt):
    from nerfdet_amd import ops
    s = E.nearest_scene(n_v, size)
    ref = _nearest_ref(n_v, size, gate_dt)
    _, m, bias, rgb, pts, proj, rgb_proj = _on(device, s)
    assert ops.density_packed_ok(n_v, s.cm, m, bias) == (n_v <= 128)
    gate = _gate(s, device, gate_dt)
    _check_glob(ops.density_features(m, bias, rgb, pts, proj, rgb_proj, depth_gate=gate), ref["glob"], ref["cnt"], "as dispatched")
    if n_v <= 128:
        monkeypatch.setattr(ops, "density_packed_ok", lambda *a, **k: False)
        _check_glob(ops.density_features(m, bias, rgb, pts, proj, rgb_proj, depth_gate=gate), ref["glob"], ref["cnt"], "generic kernel")


@pytest.mark.parametrize("gate_dt", GATES, ids=GATE_IDS)
@pytest.mark.parametrize("n_v,size", E.NEAREST_SCENES)
def test_scene_accumulate_in_two_uneven_chunks(device, n_v, size, gate_dt):
    from nerfdet_amd import ops
    s = E.nearest_scene(n_v, size)
    ref = _nearest_ref(n_v, size, gate_dt)
    f, m, bias, rgb, pts, proj, rgb_proj = _on(device, s)
    state = ops.SceneState(s.grid, s.c, s.cm, device)
    at = 0
    for k in CHUNKS[n_v]:
        v = slice(at, at + k)
        ops.scene_accumulate(state, f[v], m[v], bias, rgb[v], pts, proj[v], rgb_proj[v], depth_gate=_gate(s, device, gate_dt, v))
        at += k
    assert at == n_v == state.n_views
    _check_glob(ops.density_finish(state, bias), ref["glob"], ref["cnt"], "density_finish")
    vol, cnt = ops.volume_finish(state)
    assert torch.equal(cnt.cpu(), ref["cnt"])
    torch.testing.assert_close(vol.cpu().double(), ref["mean"], rtol=0, atol=ATOL)
    assert (vol.cpu()[:, ref["cnt"][0] == 0] == 0).all()


@pytest.mark.parametrize("gate_dt", GATES, ids=GATE_IDS)
@pytest.mark.parametrize("n_v,size", [c for c in E.NEAREST_SCENES if c[0] <= 128])
def test_scene_accumulate_group_two_scenes_one_launch(device, n_v, size, gate_dt):
    """The second scene holds the same points in the opposite order (first tile <-> last block) and features of its own."""
    from nerfdet_amd import ops
    scenes = [E.nearest_scene(n_v, size), E.nearest_scene(n_v, size, reverse=True)]
    assert not torch.equal(scenes[0].feat, scenes[1].feat) and torch.equal(scenes[0].bias, scenes[1].bias)
    refs = [_nearest_ref(n_v, size, gate_dt), _nearest_ref(n_v, size, gate_dt, True)]
    dev = [_on(device, s) for s in scenes]
    group = ops.SceneGroupState(scenes[0].grid, scenes[0].c, scenes[0].cm, [d[4] for d in dev], device)
    cat = lambda i: torch.cat([d[i] for d in dev])
    gate = None
    if gate_dt is not None:
        s0 = scenes[0]
        gate = ops.DepthGate(torch.cat([s0.depth[gate_dt]] * 2).to(device), torch.cat([s0.depth_r[gate_dt]] * 2).to(device), E.BAND)
    feats = cat(0).contiguous(memory_format=torch.channels_last)
    mapped = cat(1).contiguous(memory_format=torch.channels_last)
    ops.scene_accumulate_group(group, None, feats, mapped, dev[0][2], cat(3), cat(5), cat(6), depth_gate=gate)
    rows = ops.density_finish_group(group, dev[0][2])
    vol, cnt = ops.volume_finish_group(group)
    n = scenes[0].n
    for i, ref in enumerate(refs):
        assert torch.equal(cnt[i].cpu(), ref["cnt"]), f"scene {i}"
        torch.testing.assert_close(vol[i].cpu().double(), ref["mean"], rtol=0, atol=ATOL)
        _check_glob(rows[i * n:(i + 1) * n], ref["glob"], ref["cnt"], f"scene {i}")


# ---- K1 / K2 backward ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _k1_grad(n_v, size, gate_dt):
    s = E.nearest_scene(n_v, size)
    g = torch.randn(s.c, *s.grid, generator=torch.Generator().manual_seed(n_v + 1))
    f64 = s.feat.double().requires_grad_(True)
    vol, valid = _backproject64(f64, s.points, s.proj, None if gate_dt is None else s.depth[gate_dt], E.BAND)
    mean, cnt, _ = O.aggregate_views(vol, valid)
    (grad,) = torch.autograd.grad(mean, f64, g.double())
    return g, grad, cnt, _hits(valid, s.points, s.proj, s.h, s.w)


@pytest.mark.parametrize("scatter_mode", MODES, ids=MODE_IDS, indirect=True)
@pytest.mark.parametrize("gate_dt", GATES, ids=GATE_IDS)
@pytest.mark.parametrize("n_v,size", E.NEAREST_SCENES)
def test_k1_backward_at_the_edges(device, scatter_mode, n_v, size, gate_dt):
    from nerfdet_amd.autograd import BackprojectMean
    det, gscale = scatter_mode
    s = E.nearest_scene(n_v, size)
    g, ref, cnt, hits = _k1_grad(n_v, size, gate_dt)
    assert (cnt == 0).any() and int(hits[s.edge_views[-1]].sum()) > 0
    for cl_out in (True, False):
        fd = s.feat.to(device).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        out, count = BackprojectMean.apply(fd, s.points.to(device), s.proj.to(device), cl_out, _gate(s, device, gate_dt, rgb=False))
        assert torch.equal(count.cpu(), cnt)
        gu = (g * gscale).to(device)
        if cl_out:
            gu = gu.permute(1, 2, 3, 0).contiguous().permute(3, 0, 1, 2)
        torch.autograd.backward(out, gu)
        slack = hits.unsqueeze(1).expand(-1, s.c, -1, -1) if det else None
        _check(fd.grad, ref * gscale, f"K1 d features n_v={n_v} {size} cl_out={cl_out}", slack)


@functools.lru_cache(maxsize=None)
def _k2_grad(n_v, size, gate_dt):
    s = E.nearest_scene(n_v, size)
    gen = torch.Generator().manual_seed(n_v + 2)
    m64, b64 = s.mapped.double().requires_grad_(True), s.bias.double().requires_grad_(True)
    dm_f, dm_r = (None, None) if gate_dt is None else (s.depth[gate_dt], s.depth_r[gate_dt])
    vol, valid = _backproject64(m64, s.points, s.proj, dm_f, E.BAND)
    vol = vol + (~valid) * b64.view(1, s.cm, 1, 1, 1)
    rvol, _ = _backproject64(s.rgb.double(), s.points, s.rgb_proj, dm_r, E.BAND)
    cnt = valid.sum(dim=0)
    glob = O.density_features(vol, rvol, cnt, torch.eye(s.cm, dtype=torch.float64), torch.zeros(s.cm, dtype=torch.float64))
    g = torch.randn(glob.shape, generator=gen)
    g[cnt.flatten() == 0] = 0.0                       # as the dense cases of test_backward_shapes_gpu.py
    dm, db = torch.autograd.grad(glob, (m64, b64), g.double())
    return g, glob.detach(), dm, db, cnt, _hits(valid, s.points, s.proj, s.h, s.w)


@pytest.mark.parametrize("scatter_mode", MODES, ids=MODE_IDS, indirect=True)
@pytest.mark.parametrize("gate_dt", GATES, ids=GATE_IDS)
@pytest.mark.parametrize("n_v,size", E.NEAREST_SCENES)
def test_k2_backward_at_the_edges(device, scatter_mode, n_v, size, gate_dt):
    from nerfdet_amd.autograd import DensityFeatures
    det, gscale = scatter_mode
    s = E.nearest_scene(n_v, size)
    g, glob_ref, ref_dm, ref_db, cnt, hits = _k2_grad(n_v, size, gate_dt)
    assert torch.equal(cnt, _nearest_ref(n_v, size, gate_dt)["cnt"])
    md = s.mapped.to(device).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    bd = s.bias.to(device).requires_grad_(True)
    glob = DensityFeatures.apply(md, bd, s.rgb.to(device), s.points.to(device), s.proj.to(device), s.rgb_proj.to(device), _gate(s, device, gate_dt))
    _check_glob(glob.detach(), glob_ref, cnt, "K2 forward")
    torch.autograd.backward(glob, (g * gscale).to(device))
    slack = hits.unsqueeze(1).expand(-1, s.cm, -1, -1) if det else None
    _check(md.grad, ref_dm * gscale, f"K2 d mapped n_v={n_v} {size}", slack)
    n_waves = 4 * ((cnt.numel() + 15) // 16)
    _check(bd.grad, ref_db * gscale, f"K2 d bias n_v={n_v} {size}", torch.full((s.cm,), n_waves) if det else None)


# ------------------------------------------------------------------------------------------------------------------------------
# bilinear family
# ------------------------------------------------------------------------------------------------------------------------------
def _check_stats(got, s, ref, what):
    glob, pm, vc = (t.cpu() for t in got)
    glob, pm, vc = glob.reshape(s.n, -1).double(), pm.reshape(-1), vc.reshape(-1)
    bad = vc.long() != ref["count"]
    assert not bad.any(), f"{what}: view count differs in {int(bad.sum())} samples, first {bad.nonzero()[0].tolist()} ({s.category[int(bad.nonzero()[0])]})"
    assert torch.equal(pm, ref["count"] > 1), f"{what}: pixel_mask"
    torch.testing.assert_close(glob, ref["glob"], rtol=0, atol=ATOL, msg=lambda m: f"{what}: {m}")
    # a sample no image contains: mean exactly 0, exp(-var) exactly 1 (no tap reaches a map) or 0, as the reference says
    unseen = ref["count"] == 0
    assert unseen.any() and torch.equal(glob[unseen], ref["glob"][unseen]), f"{what}: rows of samples no view sees"


def _cams_args(s, device):
    return s.points.view(-1, 1, 3).to(device), s.img.to(device), s.cams, s.feat.to(device).contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("n_v,size,d,kind", E.BILINEAR_SCENES)
def test_ray_view_stats_packed_and_generic(device, monkeypatch, n_v, size, d, kind):
    from nerfdet_amd import rays
    s = E.bilinear_scene(n_v, size, d, kind)
    ref = E.bilinear_reference(n_v, size, d, kind)
    xyz, img, cams, f = _cams_args(s, device)
    assert rays.packed_ok(n_v, d) == (n_v <= 128)
    _check_stats(rays.ray_view_stats(xyz, img, cams, f), s, ref, "as dispatched")
    if n_v <= 128:
        monkeypatch.setattr(rays, "packed_ok", lambda *a, **k: False)
        _check_stats(rays.ray_view_stats(xyz, img, cams, f), s, ref, "generic kernel")


def _bank(s, device):
    from nerfdet_amd import rays
    bank = rays.ViewBank()
    at = 0
    for k in SEGMENTS[s.n_v]:
        meta = copy.copy(s.meta)
        meta["lidar2img"] = dict(s.meta["lidar2img"], extrinsic=s.meta["lidar2img"]["extrinsic"][at:at + k])
        bank.append(s.feat[at:at + k].to(device), s.img[at:at + k].to(device), meta)
        at += k
    assert at == s.n_v == bank.n_views
    return bank


@pytest.mark.parametrize("n_v,size,d,kind", E.BILINEAR_SCENES)
def test_ray_view_stats_bank_with_an_edge_view_at_a_segment_border(device, n_v, size, d, kind):
    from nerfdet_amd import rays
    s = E.bilinear_scene(n_v, size, d, kind)
    got = rays.ray_view_stats_bank(s.points.view(-1, 1, 3).to(device), _bank(s, device))
    _check_stats(got, s, E.bilinear_reference(n_v, size, d, kind), "bank")


@pytest.mark.parametrize("n_v,size,d,kind", [E.BILINEAR_SCENES[2], E.BILINEAR_SCENES[4]])
def test_ray_view_stats_bank_group_two_banks(device, n_v, size, d, kind):
    """Two banks in one launch: the scene and its twin with the samples in the opposite order and maps of its own."""
    from nerfdet_amd import rays
    scenes = [E.bilinear_scene(n_v, size, d, kind), E.bilinear_scene(n_v, size, d, kind, reverse=True)]
    assert not torch.equal(scenes[0].feat, scenes[1].feat)
    outs = rays.ray_view_stats_bank_group([s.points.to(device) for s in scenes], [_bank(s, device) for s in scenes])
    for i, (s, got) in enumerate(zip(scenes, outs)):
        _check_stats(got, s, E.bilinear_reference(n_v, size, d, kind, reverse=bool(i)), f"bank {i}")


@pytest.mark.parametrize("n_v,size,d,kind", E.BILINEAR_SCENES)
def test_projector_compute_masks_and_zero_padding(device, n_v, size, d, kind):
    from nerfdet_amd import rays
    assert {c[2] for c in E.BILINEAR_SCENES} == {8, 32}
    s = E.bilinear_scene(n_v, size, d, kind)
    ref = E.bilinear_reference(n_v, size, d, kind)
    xyz, img, cams, f = _cams_args(s, device)
    out, mask = rays.Projector(device).compute(xyz, img.permute(0, 2, 3, 1).unsqueeze(0), cams.to(device), f)
    assert torch.equal(mask.cpu().reshape(s.n, n_v) > 0, ref["mask"]) and set(mask.unique().tolist()) <= {0.0, 1.0}
    want = torch.cat([_k4_val(s.img.double(), ref["taps_img"]), _k4_val(s.feat.double(), ref["taps_feat"])], dim=-1)     # (n, n_v, 3 + d)
    got = out.cpu().reshape(s.n, n_v, 3 + d).double()
    torch.testing.assert_close(got, want, rtol=0, atol=ATOL)
    assert (got[want == 0] == 0).all(), "a zero-padded sample is not exactly zero"
    # the reference's own float32 path (bmm + grid_sample) where its coordinates are finite
    rf, _ = O.projector_compute(s.points.view(-1, 1, 3), s.img.permute(0, 2, 3, 1).unsqueeze(0), s.cams, s.feat)
    finite = torch.isfinite(rf.reshape(s.n, -1)).all(1) & torch.isfinite(s.points).all(1)
    torch.testing.assert_close(out.cpu().reshape(s.n, n_v, 3 + d)[finite], rf.reshape(s.n, n_v, 3 + d)[finite], rtol=0, atol=1e-4)


# ---- K4 backward ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _k4_grad(n_v, size, d, kind):
    s = E.bilinear_scene(n_v, size, d, kind)
    nch = 3 + d
    g = torch.randn(s.n, 2 * nch, generator=torch.Generator().manual_seed(n_v + d))
    f64 = s.feat.double().requires_grad_(True)
    mean, ev, mask, taps = _k4_ref(s.points, s.ke, (s.h, s.w), f64)
    un = (mask.sum(1) == 0).double().unsqueeze(-1)
    out = {}
    for part, sel in (("seen", 1 - un), ("unseen", un)):
        (ref,) = torch.autograd.grad((mean, ev), f64, (g[:, 3:nch].double() * sel, g[:, nch + 3:].double() * sel), retain_graph=True)
        cnt = torch.zeros(n_v * s.hf * s.wf, dtype=torch.int64)           # (sample, view, tap) contributions per feature pixel
        for idx, wt in taps:
            cnt.scatter_add_(0, idx.reshape(-1), ((wt != 0) & (sel.t() > 0)).long().reshape(-1))
        out[part] = (ref, cnt.view(n_v, 1, s.hf, s.wf).expand(-1, d, -1, -1))
    return g, un, out


@pytest.mark.parametrize("scatter_mode", MODES, ids=MODE_IDS, indirect=True)
@pytest.mark.parametrize("kernel", ["generic", "packed"])
@pytest.mark.parametrize("n_v,size,d,kind", E.BILINEAR_SCENES)
def test_k4_backward_at_the_edges(device, monkeypatch, scatter_mode, kernel, n_v, size, d, kind):
    """_check's "nonzero exactly where the reference is" clause at the edges: no gradient lands on a pixel whose tap the reference
    zero-pads, and a view that is masked out but near receives exactly the variance term (the reference's gradient of it)."""
    from nerfdet_amd import rays
    from nerfdet_amd.autograd import RayViewStats
    det, gscale = scatter_mode
    if kernel == "packed":
        if not rays.packed_ok(n_v, d, backward=True):
            assert n_v > 128 or d == 8                # 128-view limit; LDS of the packed backward too small at d = 8
            return
    else:
        monkeypatch.setattr(rays, "packed_ok", lambda *a, **k: False)
    s = E.bilinear_scene(n_v, size, d, kind)
    g, un, refs = _k4_grad(n_v, size, d, kind)
    xyz, img, cams, _ = _cams_args(s, device)
    fd = s.feat.to(device).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    glob, pm, vc = RayViewStats.apply(fd, xyz, img, cams)
    _check_stats((glob.detach(), pm, vc), s, E.bilinear_reference(n_v, size, d, kind), f"forward ({kernel})")
    assert torch.equal((vc.cpu().reshape(-1) == 0).double().unsqueeze(-1), un)
    seen_scale = None
    for part, sel in (("seen", 1 - un), ("unseen", un)):
        (got,) = torch.autograd.grad(glob, fd, (g * gscale * sel).float().view(s.n, 1, -1).to(device), retain_graph=True)
        ref, cnt = refs[part]
        slack = cnt if det else None
        if part == "seen":
            _check(got, ref * gscale, f"K4 d features n_v={n_v} d={d} {kernel}", slack)
            seen_scale = float(ref.abs().max()) * gscale
        else:
            # the looser arguments test_backward_shapes_gpu.py documents for samples no image contains
            _check(got, ref * gscale, f"K4 d features n_v={n_v} d={d} {kernel}, unseen samples", slack, tol=1e-3, etol=1e-3, atol=1e-5,
                   floor=EPS32 * seen_scale)
