"""Hierarchical sampling on the GPU (csrc/importance_kernels.hip through nerfdet_amd.rays): the draw against the float64 restatement
in CDF space and, where well conditioned, in depth; its structure; the fused merge bit for bit against torch on the kernel's own
samples; and rays.render_rays_func(N_importance=k).

Bounds (tests/importance_ref.py, checked on the float32 reference by tests/test_importance_cpu.py):
  CDF space  |cdf64(sample) - u| <= 1e-5 + (M + 4) * 2^-24 on every weight and u pattern;
  depth      that bound times the sample's slope (bins[above] - bins[below]) / denom from the float64 restatement, on weights in [0.2, 1]."""
import math

import pytest
import torch

import importance_ref as I
from conftest import golden_meta, load_golden

pytestmark = pytest.mark.gpu


def _draw(device, bins, w, n, up, u):
    from nerfdet_amd import rays
    keep = w.clone()
    z = rays.sample_pdf(bins, w, n, det=(up == "det"), u=None if up == "det" else u.to(device))
    assert torch.equal(w, keep), "sample_pdf changed the weights"
    assert z.shape == (w.shape[0], n) and z.dtype == torch.float32
    return z


@pytest.mark.parametrize("s,n", I.SHAPES)
def test_draw_in_cdf_space_and_structure(device, s, n):
    m = s - 2
    bound = I.cdf_bound(m)
    worst = 0.0
    for r in I.RAY_COUNTS:
        bins = I.mid_bins(I.coarse_depths(r, s, seed=11 + r)).to(device)
        for wp in I.WEIGHT_PATTERNS:
            w = I.weights_of(wp, r, m, seed=12 + r).to(device)
            for up in I.U_PATTERNS:
                u = I.uniforms_of(up, r, n, seed=13 + r)
                z = _draw(device, bins, w, n, up, u)
                what = f"S={s} n_imp={n} R={r} weights={wp} u={up}"
                uu = I._rows(u.to(device), r)
                err = float((I.cdf64(bins, w, z) - uu.double()).abs().max())
                worst = max(worst, err)
                assert err <= bound, f"{what}: CDF-space error {err:.3e} over the bound {bound:.3e}"
                assert bool((z >= bins[:, :1]).all()) and bool((z <= bins[:, -1:]).all()), f"{what}: a sample leaves [bins[0], bins[M]]"
                if up == "det":
                    assert bool((z[:, 1:] >= z[:, :-1]).all()), f"{what}: a det row decreases"
                if up in ("det", "ends"):
                    assert torch.equal(z[:, 0], bins[:, 0]), f"{what}: u = 0 does not give bins[0]"
                if up == "det" and wp.startswith("onehot"):
                    b = I.onehot_bin(wp, m)
                    outside = ((z < bins[:, b:b + 1]) | (z > bins[:, b + 1:b + 2])).sum(dim=1)
                    allowed = math.ceil(n * m * 1e-5) + 2
                    assert int(outside.max()) <= allowed, f"{what}: {int(outside.max())} samples outside the one-hot bin (allowed {allowed})"
    print(f"(S={s}, n_imp={n}): worst CDF-space error {worst:.3e}, bound {bound:.3e}")


@pytest.mark.parametrize("s,n", I.SHAPES)
def test_draw_in_depth_on_well_conditioned_weights(device, s, n):
    """Weights in [0.2, 1]: against the float64 restatement for every ray count and u pattern, and against the reference's own det
    draw (the fixture's 'plateau' ray); all the fixture's rays in CDF space."""
    m = s - 2
    bound = I.cdf_bound(m)
    for r in I.RAY_COUNTS:
        bins = I.mid_bins(I.coarse_depths(r, s, seed=21 + r)).to(device)
        w = I.weights_of("plateau", r, m, seed=22 + r).to(device)
        for up in I.U_PATTERNS:
            u = I.uniforms_of(up, r, n, seed=23 + r)
            z = _draw(device, bins, w, n, up, u)
            z64, slope = I.sample_pdf64(bins, w, u.to(device))
            gap = (z.double() - z64).abs()
            ratio = float((gap / (bound * slope)).max())
            assert ratio <= 1.0, f"S={s} n_imp={n} R={r} u={up}: depth error reaches {ratio:.3f} of bound x slope"
    g = load_golden("sample_pdf_det")
    ci = I.SHAPES.index((s, n))
    bins, w, ref = (g[f"c{ci}_{k}"].to(device) for k in ("bins", "weights", "samples"))
    z = _draw(device, bins, w, n, "det", None)
    u = torch.linspace(0., 1., n, device=device)
    assert float((I.cdf64(bins, w, z) - u.double()).abs().max()) <= bound
    row = I.WEIGHT_PATTERNS.index("plateau")
    _, slope = I.sample_pdf64(bins, w, u)
    gap = (z[row] - ref[row]).abs().double()
    print(f"(S={s}, n_imp={n}): against the reference's det draw, max depth gap {float(gap.max()):.3e}, allowed >= {float((bound * slope[row]).min()):.3e}")
    assert bool((gap <= bound * slope[row]).all())


def _merge_case(device, r, s, seed, wp="uniform"):
    g = torch.Generator().manual_seed(seed)
    z = I.coarse_depths(r, s, seed=seed).to(device)
    w = I.weights_of(wp, r, s, seed=seed + 1).to(device)
    o = (torch.rand(r, 3, generator=g) - 0.5).to(device)
    d = torch.nn.functional.normalize(torch.randn(r, 3, generator=g), dim=-1).to(device)
    return z, w, o, d


@pytest.mark.parametrize("s,n", I.SHAPES)
def test_merge_is_sort_of_cat_and_the_points_bit_for_bit(device, s, n):
    from nerfdet_amd import rays
    for r in I.RAY_COUNTS:
        for wp, up in (("uniform", "det"), ("uniform", "random"), ("onehot_mid", "ends"), ("zero", "random")):
            z, w, o, d = _merge_case(device, r, s, seed=31 + r, wp=wp)
            u = I.uniforms_of(up, r, n, seed=33 + r)
            keep = (z.clone(), w.clone())
            pts, z_out, zs = rays.importance_merge(z, w, o, d, n, up == "det", u=None if up == "det" else u.to(device))
            what = f"S={s} n_imp={n} R={r} weights={wp} u={up}"
            assert torch.equal(z, keep[0]) and torch.equal(w, keep[1]), f"{what}: an input changed"
            assert z_out.shape == (r, s + n) and pts.shape == (r, s + n, 3) and zs.shape == (r, n)
            want = torch.sort(torch.cat([z, zs], dim=-1), dim=-1).values
            assert torch.equal(z_out, want), f"{what}: z_out is not sort(cat(z_vals, z_samples))"
            assert torch.equal(pts, z_out[..., None] * d[:, None] + o[:, None]), f"{what}: pts is not z * ray_d + ray_o"
            alone = rays.sample_pdf(I.mid_bins(z), w[:, 1:-1], n, det=(up == "det"), u=None if up == "det" else u.to(device))
            assert torch.equal(zs, alone), f"{what}: the fused draw is not ndet_sample_pdf's"


def test_merge_without_z_samples_out_and_with_unsorted_coarse_depths(device):
    """z_samples_out may be null; the merge sorts whatever order the coarse depths come in (the bitonic network sorts all S + n_imp slots)."""
    from nerfdet_amd import _lib, rays
    r, s, n = 5, 40, 64
    z, w, o, d = _merge_case(device, r, s, seed=41)
    u = torch.linspace(0., 1., n, device=device)
    pts, z_out, _ = rays.importance_merge(z, w, o, d, n, True)
    z2, p2 = torch.full_like(z_out, -1.0), torch.full_like(pts, -1.0)
    _lib.check(_lib.load().ndet_importance_merge(_lib._ptr(z), _lib._ptr(w), _lib._ptr(o), _lib._ptr(d), r, s, _lib._ptr(u), 0, n, _lib._ptr(z2),
                                                 _lib._ptr(p2), None, _lib._stream(z)), "importance_merge")
    assert torch.equal(z2, z_out) and torch.equal(p2, pts)
    perm = torch.randperm(s, generator=torch.Generator().manual_seed(5)).to(device)
    zp = z[:, perm].contiguous()
    _, z3, zs3 = rays.importance_merge(zp, w, o, d, n, True)
    assert torch.equal(z3, torch.sort(torch.cat([zp, zs3], dim=-1), dim=-1).values)


# ---- rays.render_rays_func(N_importance=k) on the small rig of tests/test_rays_gpu.py ----
def _rig(device):
    from test_rays_gpu import _mlp
    g = load_golden("rays_small_s0")
    return dict(o=g["ray_o"].to(device), d=g["ray_d"].to(device), feat=g["features_2d"].to(device), img=g["img"].to(device),
                s=int(g["n_samples"]), mlp=_mlp(g, device), meta=golden_meta(g))


def _func(rig, k, feat=None, **kw):
    from nerfdet_amd import rays
    return rays.render_rays_func(rig["o"], rig["d"], None, None, rig["feat"] if feat is None else feat, rig["img"], None, [0.2, 8.0], rig["s"],
                                 4096, rig["mlp"], rig["meta"], None, "image", N_importance=k, det=True, **kw)


def test_render_rays_func_fine_pass(device):
    from nerfdet_amd import rays
    rig = _rig(device)
    k = 16
    with torch.no_grad():
        plain, fine = _func(rig, 0), _func(rig, k)
        assert plain["outputs_fine"] is None and set(plain) == set(fine)
        for key, v in plain["outputs_coarse"].items():
            assert (v is None and fine["outputs_coarse"][key] is None) or torch.equal(v, fine["outputs_coarse"][key]), f"outputs_coarse.{key} moved"
        assert torch.equal(plain["sigma"], fine["sigma"])
        # the chain spelled out from the public pieces
        cams = rays._compute_projection(rig["meta"])
        pts, z = rays.sample_along_camera_ray(rig["o"], rig["d"], [0.2, 8.0], rig["s"], det=True)
        glob, pm, _ = rays.ray_view_stats(pts, rig["img"], cams, rig["feat"])
        rgb, sigma = rig["mlp"](pts, rig["d"], glob)
        coarse = rays.raw2outputs(torch.cat([rgb, sigma], dim=-1), z, pm)
        pts_f, z_f, _ = rays.importance_merge(z, coarse["weights"], rig["o"], rig["d"], k, True)
        glob_f, pm_f, _ = rays.ray_view_stats(pts_f, rig["img"], cams, rig["feat"])
        rgb_f, sigma_f = rig["mlp"](pts_f, rig["d"], glob_f)
        want = rays.raw2outputs(torch.cat([rgb_f, sigma_f], dim=-1), z_f, pm_f)
    got = fine["outputs_fine"]
    assert list(got) == list(want) and got["weights"].shape == (rig["o"].shape[0], rig["s"] + k)
    for key in want:
        assert torch.equal(got[key], want[key]), f"outputs_fine.{key} differs from the chain"
    assert bool(torch.isfinite(got["rgb"]).all()) and bool(torch.isfinite(got["depth"]).all())
    with pytest.raises(AssertionError):
        _func(rig, k, inv_uniform=True)


def test_render_rays_func_fine_pass_has_no_backward(device):
    rig = _rig(device)
    feat = rig["feat"].clone().requires_grad_(True)
    with pytest.raises(ValueError, match="no backward"):
        _func(rig, 4, feat=feat)
    with torch.no_grad():
        assert _func(rig, 4, feat=feat)["outputs_fine"] is not None
