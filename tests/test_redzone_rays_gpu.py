"""The ray branch's forward kernels inside tests/redzone.py: the sampler, the compositor, sample_pdf and the fused importance merge, the early-stop
``advance`` and front-segment kernels, the packed / bank / bank-group view statistics and the bank's count kernel.  Every row twice, fill 0x00 then
0xFF, inputs placed flush against guards, outputs and block counts carved: no guard byte and no input changed, the results equal bit for bit.
advance_transmittance updates ``T`` in place, as its docstring says; that placed tensor is named as written and is the row's result.  The
compaction outputs are allocated at the kept count M, so they have no don't-care tail.  Numbers are held to fp64 / the restatements by
tests/test_ray_forward_gpu.py, test_importance_gpu.py, test_early_stop_gpu.py, test_stream_render_gpu.py and test_skip_empty_gpu.py, whose inputs are
imported here; every kernel here is one fixed-order sum per output element ("the same bytes on every call")."""
import numpy as np
import pytest
import torch

import early_stop_ref as ES
import importance_ref as I
import ray_forward_ref as Rf
import skip_empty_ref as SE
import test_early_stop_gpu as TE
import test_skip_empty_gpu as TS
import test_stream_render_gpu as TR
from oracle import nerfdet_oracle as O
from redzone import both_fills

pytestmark = pytest.mark.gpu

RAYS = [65, 257]          # 64 k + 1 and 256 k + 1: one ray past a wave, one past a 256-thread workgroup


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize("jitter", ["det", "random"])
@pytest.mark.parametrize("r,s", [(65, 2), (257, 19)])
def test_redzone_sampler(device, r, s, jitter):
    from nerfdet_amd import rays
    ray_o, ray_d, t = Rf.sampler_inputs(r, s, jitter)

    def body(rz):
        pts, z = rays.sample_along_camera_ray(rz.place(ray_o, "ray_o"), rz.place(ray_d, "ray_d"), [0.2, 8.0], s, det=t is None,
                                              t_rand=None if t is None else rz.place(t, "t_rand"))
        return {"pts": pts, "z": z}
    both_fills(device, body)


@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("r,s", [(65, 1), (65, 69), (257, 19)])
def test_redzone_compositor(device, r, s, white):
    from nerfdet_amd import rays
    torch.manual_seed(r + s)
    raw = torch.cat([torch.rand(r, s, 3), torch.randn(r, s, 1) * 3], -1)
    z = torch.sort(torch.rand(r, s) * 5 + 0.2, dim=-1).values
    pmask = torch.rand(r, s) < 0.7

    def body(rz):
        with torch.no_grad():
            out = rays.raw2outputs(rz.place(raw, "raw"), rz.place(z, "z_vals"), rz.place(pmask, "mask"), white_bkgd=white)
        return {k: out[k] for k in Rf.COMPOSITE_KEYS + ("mask",)}
    both_fills(device, body)


@pytest.mark.parametrize("s,n", I.SHAPES)
@pytest.mark.parametrize("r", RAYS)
def test_redzone_sample_pdf_and_importance_merge(device, r, s, n):
    from nerfdet_amd import rays
    z = I.coarse_depths(r, s, seed=31 + r)
    w = I.weights_of("uniform", r, s, seed=32 + r)
    g = torch.Generator().manual_seed(r)
    o = torch.rand(r, 3, generator=g) - 0.5
    d = torch.nn.functional.normalize(torch.randn(r, 3, generator=g), dim=-1)
    u = torch.rand(r, n, generator=g)

    def body(rz):
        zd, wd = rz.place(z, "z_vals"), rz.place(w, "weights")
        ud = rz.place(u, "u")
        pts, z_out, zs = rays.importance_merge(zd, wd, rz.place(o, "ray_o"), rz.place(d, "ray_d"), n, False, u=ud)
        alone = rays.sample_pdf(rz.place(I.mid_bins(z), "bins"), rz.place(w[:, 1:-1].contiguous(), "inner_weights"), n, det=False, u=ud)
        det = rays.sample_pdf(rz.place(I.mid_bins(z), "bins_det"), rz.place(w[:, 1:-1].contiguous(), "inner_weights_det"), n, det=True)
        return {"pts": pts, "z_out": z_out, "z_samples": zs, "alone": alone, "det": det}
    got = both_fills(device, body)
    assert torch.equal(got["z_samples"], got["alone"])


@pytest.mark.parametrize("s", [5, 69])
@pytest.mark.parametrize("r", RAYS)
def test_redzone_advance(device, r, s):
    from nerfdet_amd import rays
    rng = np.random.RandomState(1000 * r + s)
    raw = np.concatenate([rng.rand(r, s, 3).astype(np.float32), TE.SIGMAS[rng.randint(0, len(TE.SIGMAS), (r, s, 1))]], axis=-1)

    def body(rz):
        T = rz.place(torch.ones(r), "T")
        rd = rz.place(_t(raw), "raw")
        for a in range(0, s - 4, 4):
            assert rays.advance_transmittance(rd, T, a, a + 4) is T
        return {"T": T}
    both_fills(device, body, written=("T",))                     # advance_transmittance: "``T`` is updated in place and returned"


@pytest.mark.parametrize("grid", ["none", "lds-cull", "global-keep"])
@pytest.mark.parametrize("r", RAYS)
def test_redzone_front_segment(device, r, grid):
    from nerfdet_amd import rays
    s = 69
    T = TE._t_case(r, seed=r)
    bits = None
    if grid == "none":
        pts = np.random.RandomState(r + s).rand(r, s, 3).astype(np.float32)
    else:
        path, outside = grid.split("-")
        nv, p0, vs = TS.LATTICES[path]
        alpha, count, thr = TS._grid(nv)
        bits = SE.occupancy_bits(alpha, count, nv, thr, 1)
        pts = TS._points(nv, p0, vs, r * s, seed=r + s).reshape(r, s, 3)

    def body(rz):
        occ = None if bits is None else rays.OccupancyGrid(rz.place(_t(bits), "bits"), nv, p0, vs, outside)
        dp, dT = rz.place(_t(pts), "pts"), rz.place(_t(T), "T")
        out = {}
        for w in (4, 32):
            for s0, s1 in TE._segments(s, w):
                out[f"idx{w}_{s0}"], out[f"kept{w}_{s0}"] = rays.front_segment(dp, dT, s0, s1, TE.EPS, occ)
        if occ is None:
            out["idx_live"], out["kept_live"] = rays.front_segment(dp, rz.place(torch.ones(r), "T_live"), 64, 69, TE.EPS, all_live=True)
        return out
    got = both_fills(device, body)
    want_idx, _ = ES.front(pts, T, 0, 4, TE.EPS, None if bits is None else (bits, nv, p0, vs, outside))
    assert got["idx4_0"].shape[0] == len(want_idx)


# ---- view statistics: (n_v, d, hw, sizes) = (9, 8, (60, 80), [3, 1, 5]) ----
N_V, D, HW, SIZES = 9, 8, (60, 80), [3, 1, 5]


def _stats_case():
    gen = torch.Generator().manual_seed(N_V * 100 + D)
    meta = O.ring_scene_meta(N_V, HW)
    feat = torch.randn(N_V, D, HW[0] // 4, HW[1] // 4, generator=gen).contiguous(memory_format=torch.channels_last)
    img = torch.rand(N_V, 3, *HW, generator=gen)
    r, s = 65, 19
    ang = torch.rand(r, generator=gen) * 2 * np.pi
    ray_o = torch.stack([2.0 * torch.cos(ang), 2.0 * torch.sin(ang), 1.0 + 0.3 * torch.rand(r, generator=gen)], -1)
    ray_d = -ray_o / ray_o.norm(dim=-1, keepdim=True) + 0.35 * torch.randn(r, 3, generator=gen)
    z = torch.linspace(0.2, 8.0, s)
    pts = (z[None, :, None] * ray_d[:, None] + ray_o[:, None]).contiguous()
    return meta, feat, img, pts


def _placed_bank(rz, meta, feat, img, sizes, device):
    """A ViewBank whose segments' maps are placed inputs (make_segment copies the chunk's map with .contiguous() / .clone(), which the harness does
    not redirect; the packed image it makes is carved by itself)."""
    from nerfdet_amd import rays
    bank, v = rays.ViewBank(), 0
    for i, k in enumerate(sizes):
        seg = bank.make_segment(feat[v:v + k].to(device), rz.place(img[v:v + k].contiguous(), f"images{i}"), TR._chunk_meta(meta, v, v + k))
        seg.feat = rz.place(seg.feat.cpu(), f"mapped{i}")
        bank.push(seg)
        v += k
    return bank


@pytest.mark.parametrize("kind", ["packed", "generic"])
def test_redzone_view_stats(device, kind):
    from nerfdet_amd import rays
    meta, feat, img, pts = _stats_case()
    cams = rays._compute_projection(meta)

    def body(rz):
        saved = rays.packed_ok
        if kind == "generic":
            rays.packed_ok = lambda *a, **k: False
        rays._PACKED_RGB.clear()                                 # the packed copy of the images is made, carved, in this run
        try:
            assert kind == "generic" or rays.packed_ok(N_V, D)
            glob, pm, vc = rays.ray_view_stats(rz.place(pts, "pts"), rz.place(img, "images"), cams, rz.place(feat, "featmaps"))
        finally:
            rays.packed_ok = saved
            rays._PACKED_RGB.clear()
        return {"globalfeat": glob, "pixel_mask": pm, "view_count": vc}
    got = both_fills(device, body)
    assert 0 < int(got["view_count"].max()) and int(got["view_count"].min()) < N_V


def test_redzone_view_stats_bank_and_count(device):
    from nerfdet_amd import rays
    meta, feat, img, pts = _stats_case()

    def body(rz):
        bank = _placed_bank(rz, meta, feat, img, SIZES, device)
        p = rz.place(pts, "pts")
        glob, pm, vc = rays.ray_view_stats_bank(p, bank)
        pm2, vc2 = rays.ray_view_count_bank(p, bank)
        return {"globalfeat": glob, "pixel_mask": pm, "view_count": vc, "count_mask": pm2, "count": vc2}
    got = both_fills(device, body)
    assert torch.equal(got["count"], got["view_count"]) and torch.equal(got["count_mask"], got["pixel_mask"])


def test_redzone_view_stats_bank_group(device):
    """Two banks of unequal view counts (the 9 views as [3, 1, 5] and their first 4 as [3, 1]) and unequal point counts in one launch."""
    from nerfdet_amd import rays
    meta, feat, img, pts = _stats_case()

    def body(rz):
        banks = [_placed_bank(rz, meta, feat, img, SIZES, device), _placed_bank(rz, TR._chunk_meta(meta, 0, 4), feat[:4], img[:4], [3, 1], device)]
        glob, pm, vc, flat = rays.bank_group_stats([rz.place(pts, "pts0"), rz.place(pts[:33].contiguous(), "pts1")], banks)
        return {"globalfeat": glob, "pixel_mask": pm, "view_count": vc, "points": flat}
    both_fills(device, body)


def test_redzone_count_kernel_65_views(device):
    """n_v = 65: one view past the 64 a wave's ballot holds."""
    from nerfdet_amd import rays
    n_v, hw = 65, (32, 48)
    gen = torch.Generator().manual_seed(n_v)
    meta = O.ring_scene_meta(n_v, hw)
    feat = torch.randn(n_v, 32, hw[0] // 4, hw[1] // 4, generator=gen).contiguous(memory_format=torch.channels_last)
    img = torch.rand(n_v, 3, *hw, generator=gen)
    pts = _stats_case()[3]

    def body(rz):
        bank = _placed_bank(rz, meta, feat, img, [65], device)
        pm, vc = rays.ray_view_count_bank(rz.place(pts, "pts"), bank)
        return {"pixel_mask": pm, "view_count": vc}
    both_fills(device, body)
