"""The forward kernels of the NeRF ray branch against float64 at edge shapes: k_sample_rays, k_composite, the radiance MLP at inference
(forward_rows_hip: k_point_mlp, or k_posenc_concat + linear_rows + k_sigma_head) and the small A6 kernels k_posenc_concat, k_sigma_head,
k_sigma_to_alpha, k_alpha_gate.  References, inputs and bars are tests/ray_forward_ref.py's (its docstring has the table; the CPU test
asserts it).  Every test prints its worst errors before it asserts (``pytest -s``)."""
import functools
from ctypes import c_void_p

import numpy as np
import pytest
import torch

import ray_forward_ref as Rf

pytestmark = pytest.mark.gpu


def _worst(got, ref):
    return float((got.detach().cpu().double() - ref).abs().max())


# ------------------------------------------------------------------------------------------------------
# sampler
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("near_far", Rf.SAMPLER_RANGES)
@pytest.mark.parametrize("r,s", Rf.SAMPLER_SHAPES)
def test_sampler_against_float64_and_its_structure(device, r, s, near_far):
    """S = 2, grids of 255 / 256 / 771 threads against the 256-thread workgroup, the largest S the merge accepts; a wide and a very
    narrow depth range; deterministic, and jitter at both ends of a stratum, in its middle and random."""
    from nerfdet_amd import rays
    near, far = (np.float32(v) for v in near_far)
    bar = Rf.bar(("sampler_z", near_far))
    zs = {}
    for jitter in ["det"] + Rf.JITTERS:
        ray_o, ray_d, t = Rf.sampler_inputs(r, s, jitter)
        o, d = ray_o.to(device), ray_d.to(device)
        pts, z = rays.sample_along_camera_ray(o, d, list(near_far), s, det=t is None, t_rand=None if t is None else t.to(device))
        _, z64 = Rf.sample64(ray_o, ray_d, near_far, s, t)
        err = _worst(z, z64)
        print(f"RAYFWD sampler {near_far} ({r}, {s}) {jitter}: z err {err:.2e} (bar {bar:.2e})")
        assert z.shape == (r, s) and pts.shape == (r, s, 3) and z.dtype == pts.dtype == torch.float32
        assert err <= bar, (jitter, err, bar)
        assert torch.equal(pts, z[..., None] * d[:, None] + o[:, None]), jitter         # a multiply, then an add
        assert bool((z[:, 1:] >= z[:, :-1]).all()), jitter
        zs[jitter] = z.cpu()
    assert bool((zs["det"] == zs["det"][:1]).all())                 # the same depths on every ray
    assert bool((zs["det"][:, 0] == near).all()) and bool((zs["zero"][:, 0] == near).all())
    assert bool((zs["below_one"][:, -1] <= far).all())
    # adjacent strata share their bound as the same float32 expression: the upper end of one is the lower end of the next
    assert bool((zs["below_one"][:, :-1] <= zs["zero"][:, 1:]).all())
    assert bool((zs["zero"] <= zs["half"]).all() and (zs["half"] <= zs["below_one"]).all())


def test_sampler_refuses_before_any_launch(device):
    """S = 1, near <= 0, far <= near: the library's error return, with the outputs untouched."""
    from nerfdet_amd import _lib, rays
    o, d = torch.zeros(4, 3, device=device), torch.ones(4, 3, device=device)
    lib = _lib.load()
    st = c_void_p(torch.cuda.current_stream(device).cuda_stream)
    for s, near, far in [(1, 0.2, 8.0), (4, 0.0, 8.0), (4, -1.0, 8.0), (4, 0.2, 0.2), (4, 0.2, 0.1)]:
        pts = torch.full((4, s, 3), 7.0, device=device)
        z = torch.full((4, s), 7.0, device=device)
        rc = lib.ndet_sample_along_rays(c_void_p(o.data_ptr()), c_void_p(d.data_ptr()), 4, s, near, far, c_void_p(0), c_void_p(pts.data_ptr()),
                                        c_void_p(z.data_ptr()), st)
        torch.cuda.synchronize()
        assert rc != 0 and lib.ndet_last_error(), (s, near, far)
        assert bool((pts == 7.0).all()) and bool((z == 7.0).all()), (s, near, far)
        with pytest.raises(AssertionError):
            rays.sample_along_camera_ray(o, d, [near, far], s, det=True)


# ------------------------------------------------------------------------------------------------------
# compositor
# ------------------------------------------------------------------------------------------------------
def _same_bits(a, b, keys=Rf.COMPOSITE_KEYS, rows=slice(None)):
    return [k for k in keys if not torch.equal(a[k], b[k][rows])]


@pytest.mark.parametrize("negate", [False, True])
@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("r,s", Rf.COMPOSITE_SHAPES)
def test_compositor_against_float64(device, r, s, white, negate):
    """1 .. 512 samples (the fine pass composites S + k), ray counts around the 64-thread workgroup, equal depths, both signs of z;
    transparent rays clamped to the call's own z range, opaque samples first, last, single and in threes."""
    from nerfdet_amd import rays
    raw, z, pmask = Rf.composite_inputs(r, s, negate)
    ref = Rf.composite64(raw, z, pmask, white)
    rd, zd, pd = raw.to(device), z.to(device), pmask.to(device)
    with torch.no_grad():
        out = rays.raw2outputs(rd, zd, pd, white_bkgd=white)
        again = rays.raw2outputs(rd, zd, pd, white_bkgd=white)
        nomask = rays.raw2outputs(rd, zd, None, white_bkgd=white)
    bars = {"rgb": Rf.ATOL, "depth": Rf.ATOL, **{k: Rf.bar(("composite_" + k, (r, s))) for k in ("weights", "alpha", "transparency")}}
    errs = {k: _worst(out[k], ref[k]) for k in Rf.COMPOSITE_KEYS}
    print(f"RAYFWD composite ({r}, {s}) white={white} negate={negate}: " + ", ".join(f"{k} {errs[k]:.2e}/{bars[k]:.2e}" for k in errs))
    for k in Rf.COMPOSITE_KEYS:
        assert out[k].shape == ref[k].shape and out[k].dtype == torch.float32
        assert errs[k] <= bars[k], (k, errs[k], bars[k])
    assert bool((out["transparency"][:, 0] == 1).all())
    # fully transparent rays: the depth is the call's z minimum (maximum for negative z), exactly
    t = Rf.row_kind(r) == Rf.ROW_KINDS.index("transparent")
    assert bool((out["depth"].cpu()[t] == (z.max() if negate else z.min())).all())
    # ray mask: more than 8 seen samples
    counts = Rf.planted_counts(r, s)
    assert out["mask"].dtype == torch.bool and out["mask"].cpu()[:len(counts)].tolist() == [c > 8 for c in counts]
    if s > 9:
        assert counts == [0, 8, 9, s][:r] and out["mask"].cpu()[:4].tolist()[:len(counts)] == [False, False, True, True][:len(counts)]
    assert torch.equal(out["mask"].cpu(), ref["mask"])
    assert nomask["mask"] is None and _same_bits(nomask, out) == []
    assert _same_bits(again, out) == [] and torch.equal(again["mask"], out["mask"])
    # rays [a:b] alone: the same bits, but for the depth, whose clamp range is the call's own ...
    a, b = r // 3, r - r // 4
    with torch.no_grad():
        part = rays.raw2outputs(rd[a:b], zd[a:b], pd[a:b], white_bkgd=white)
    assert _same_bits(part, out, ("rgb", "weights", "alpha", "transparency", "mask"), slice(a, b)) == []
    # ... and the depth too once the slice's z holds the full call's minimum and maximum
    ends = torch.nonzero((z == z.min()).any(1) | (z == z.max()).any(1)).squeeze(1)
    a, b = int(ends.min()), int(ends.max()) + 1
    with torch.no_grad():
        part = rays.raw2outputs(rd[a:b], zd[a:b], pd[a:b], white_bkgd=white)
    assert _same_bits(part, out, Rf.COMPOSITE_KEYS + ("mask",), slice(a, b)) == []


# ------------------------------------------------------------------------------------------------------
# radiance MLP at inference
# ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mlp_reference(arch, r, s):
    mlp = Rf.build_mlp(arch)
    pts, dirs, glob = Rf.mlp_inputs(arch, r, s)
    rgb64, sig64, _ = Rf.nerf_forward64(mlp.state_dict(), pts, dirs, glob)
    return mlp, (pts, dirs, glob), rgb64, sig64


def _traced(fn):
    """fn()'s result and the names of the kernel spans it launched."""
    from nerfdet_amd import trace
    assert trace.recorder is None
    trace.recorder = trace.Recorder()
    try:
        out = fn()
        names = [sp[0] for sp in trace.recorder.spans]
    finally:
        trace.recorder = None
    return out, names


MLP_RUNS = [(arch, mode) for arch in ("w256_f22", "w256_f70", "w256_f102") for mode in ("f16x2", "bf16x3", "layers")] + [("w128_f70", "f16x2")]


@pytest.mark.parametrize("r,s", Rf.MLP_SHAPES)
@pytest.mark.parametrize("arch,mode", MLP_RUNS)
def test_radiance_mlp_at_inference_against_float64(device, arch, mode, r, s):
    """``VanillaNeRFRadianceField.forward`` under no_grad (forward_rows_hip): 1, 65, 511 and 3840 rows against the 64-row tile, padded input
    widths 96 / 160 / 192, the fused trunk under both arithmetics, the layer-by-layer path (FUSED_MLP off; width 128 can never fuse), with
    zero, ordinary, bright and x 1e-4 conditioning rows in every tile.  Which path ran is asserted from the launch spans."""
    import copy
    from nerfdet_amd import conv3d
    cpu_mlp, (pts, dirs, glob), rgb64, sig64 = _mlp_reference(arch, r, s)
    width, fdim = Rf.MLP_ARCHS[arch]
    mlp = copy.deepcopy(cpu_mlp).to(device)
    fused = mode != "layers" and width == 256
    prev = conv3d.set_arithmetic("bf16x3" if mode == "bf16x3" else "f16x2")
    mlp.FUSED_MLP = mode != "layers"
    try:
        assert mlp.hip_trunk_ok() and mlp.fused_ok((63 + fdim + 31) // 32 * 32) == fused
        p, d, g = pts.to(device), dirs.to(device), glob.to(device)
        with torch.no_grad():
            (rgb, sig), names = _traced(lambda: mlp(p, d, g))
            rgb_b, sig_b = mlp(p, d[:, None, :].expand(r, s, 3).contiguous(), g)       # one direction per sample, the same values
    finally:
        conv3d.set_arithmetic(prev)
    # the path: the fused trunk is one k_point_mlp launch + bottleneck + colour layer; layer by layer it is six linear_rows launches
    n_fused = names.count("k_point_mlp/f16x2")
    assert n_fused == (1 if fused else 0) and len(names) == (3 if fused else 6), names
    # ... none of them in the fp16-pair arithmetic with its per-tensor scale (conv3d.packed_linear pins them to bf16x3, which has none)
    assert not any(nm.endswith("/f16x2") for nm in names if nm != "k_point_mlp/f16x2"), names
    assert rgb.shape == (r, s, 3) and sig.shape == (r, s, 1)
    assert torch.equal(rgb, rgb_b) and torch.equal(sig, sig_b)
    assert bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(sig).all())
    cls = Rf.row_class(r * s)
    e_sig = ((sig.cpu().double() - sig64).abs() / (1 + sig64.abs())).view(-1)
    e_rgb = (rgb.cpu().double() - rgb64).abs().amax(-1).view(-1)
    bar = Rf.bar(("mlp_rgb", arch))
    worst = {name: (float(e_sig[cls == i].max()), float(e_rgb[cls == i].max())) for i, name in enumerate(Rf.ROW_CLASSES) if bool((cls == i).any())}
    msg = ", ".join(f"{k} sigma {v[0]:.2e} rgb {v[1]:.2e}" for k, v in worst.items())
    print(f"RAYFWD mlp {arch} {mode} ({r}, {s}) path={'fused' if fused else 'layers'}: {msg} (bars {Rf.SIGMA_REL:.0e}, {bar:.2e})")
    assert all(v[0] <= Rf.SIGMA_REL for v in worst.values()), msg
    assert all(v[1] <= bar for v in worst.values()), msg
    if r * s >= 64:
        assert float(sig64.max()) > 0 and 0.05 < float(rgb64.std())


# ------------------------------------------------------------------------------------------------------
# the small A6 kernels
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257])
def test_posenc_concat_columns(device, n):
    """k_posenc_concat: points and conditioning columns copied, padding exactly 0, the 60 sines in the reference's order."""
    from nerfdet_amd import ops
    pts = Rf.encoder_points(n)
    ref = Rf.encode_f32args(pts.t(), Rf.POS_DEG)
    bar = Rf.bar(("encoder_pos", Rf.POS_DEG))
    gen = torch.Generator().manual_seed(n)
    worst = 0.0
    for f in (0, 22, 70):
        glob = None if f == 0 else torch.randn(n, f, generator=gen)
        for pad_to in (0, 96, 160):
            out = ops.posenc_concat(pts.to(device), None if glob is None else glob.to(device), pad_to=pad_to).cpu()
            width = max(63 + f, pad_to)
            assert out.shape == (n, width) and out.dtype == torch.float32
            assert torch.equal(out[:, :3], pts.t())
            if f:
                assert torch.equal(out[:, 63:63 + f], glob)
            assert float(out[:, 63 + f:].abs().sum()) == 0 and not bool(torch.signbit(out[:, 63 + f:]).any())
            err = float((out[:, 3:63].double() - ref[:, 3:]).abs().max())
            worst = max(worst, err)
            assert err <= bar, (f, pad_to, err, bar)
    print(f"RAYFWD posenc_concat n={n}: sines err {worst:.2e} (bar {bar:.2e})")


@pytest.mark.parametrize("n", [1, 3, 4, 5, 259])
def test_sigma_head_against_float64(device, n):
    """k_sigma_head, four rows per workgroup: the dot product over [h | rows[:, :n_in]] with ``rows`` wider than n_in (the columns
    behind n_in hold 1e6: reading one shows)."""
    from nerfdet_amd import ops
    gen = torch.Generator().manual_seed(n)
    worst_raw = worst_alpha = 0.0
    for ch in (32, 256):
        for n_in in (63, 85, 133):
            h = torch.relu(torch.randn(n, ch, generator=gen))
            rows = torch.randn(n, n_in + 11, generator=gen)
            rows[:, n_in:] = 1.0e6
            w = torch.randn(1, ch + n_in, generator=gen) / (ch + n_in) ** 0.5
            b = torch.randn(1, generator=gen) * 0.1
            raw64 = torch.cat([h, rows[:, :n_in]], 1).double() @ w.double().view(-1) + b.double()
            alpha64 = 1 - torch.exp(-torch.relu(raw64))
            hd, rd, wd, bd = h.to(device), rows.to(device), w.to(device), b.to(device)
            alpha, raw = ops.sigma_head(hd, rd, n_in, wd, bd, want_raw=True)
            alone = ops.sigma_head(hd, rd, n_in, wd, bd)
            assert alpha.shape == raw.shape == alone.shape == (n,) and torch.equal(alpha, alone)
            e_raw = float(((raw.cpu().double() - raw64).abs() / (1 + raw64.abs())).max())
            e_alpha = _worst(alpha, alpha64)
            worst_raw, worst_alpha = max(worst_raw, e_raw), max(worst_alpha, e_alpha)
            assert e_raw <= Rf.SIGMA_REL and e_alpha <= Rf.ALPHA_ATOL, (ch, n_in, e_raw, e_alpha)
    print(f"RAYFWD sigma_head n={n}: raw err {worst_raw:.2e} (bar {Rf.SIGMA_REL:.0e} (1 + |raw|)), alpha err {worst_alpha:.2e} (bar {Rf.ALPHA_ATOL:.0e})")


SIGMAS = [-3.5, -1e-12, -0.0, 0.0, 1e-12, 1e-3, 0.7, 16.0, 40.0, 1e4]


@pytest.mark.parametrize("n", [1, 256, 257])
def test_sigma_to_alpha_against_float64(device, n):
    """k_sigma_to_alpha: 1 - exp(-relu(x)); exactly 0 for x <= 0, exactly 1 for x >= 40."""
    from nerfdet_amd import ops
    gen = torch.Generator().manual_seed(n)
    if n == 1:
        cases = [torch.tensor([v]) for v in SIGMAS]
    else:
        x = torch.randn(n, generator=gen) * 5
        x[:len(SIGMAS)] = torch.tensor(SIGMAS)
        x[-1] = 40.0                                      # the last thread of the grid
        cases = [x]
    worst = 0.0
    for x in cases:
        out = ops.sigma_to_alpha(x.to(device)).cpu()
        ref = 1 - torch.exp(-torch.relu(x.double()))
        assert out.shape == (n,) and out.dtype == torch.float32
        worst = max(worst, _worst(out, ref))
        assert worst <= Rf.ALPHA_ATOL
        assert bool((out[x <= 0] == 0).all()) and bool((out[x >= 40] == 1).all())
    print(f"RAYFWD sigma_to_alpha n={n}: err {worst:.2e} (bar {Rf.ALPHA_ATOL:.0e})")


@pytest.mark.parametrize("grid", [(3, 5, 7), (4, 4, 16), (5, 4, 13)])
def test_alpha_gate_layouts_and_unseen_voxels(device, grid):
    """k_alpha_gate on a contiguous ``mean``, a channels-last one and a slice that is neither (the copying branch): exactly 0 where
    count == 0 whatever ``mean`` holds there, elsewhere ``fl(alpha * mean)``.  The bar: one float32 rounding of the product, 2^-24 of
    the float64 product, on top of alpha's own float32 evaluation -- expf to an ulp and a subtraction from 1, each within 2^-24
    absolute whatever the density -- which the product carries as 2^-23 |mean|."""
    from nerfdet_amd import ops
    x, y, z = grid
    nvox = x * y * z
    gen = torch.Generator().manual_seed(nvox)
    worst = 0.0
    for c in (1, 3, 64):
        density = torch.rand(nvox, generator=gen) * 5
        density[0::7] = 0.0
        density[1::7] = 40.0
        density[2::7] = 1e-3
        count = torch.randint(0, 4, (1, x, y, z), generator=gen)
        count.view(-1)[-1] = 0
        count.view(-1)[0] = 2
        unseen = (count.view(-1) == 0)
        base = torch.randn(c, nvox, generator=gen) * 3
        poison = torch.tensor([float("nan"), float("inf"), -float("inf"), 1e9])[torch.arange(nvox) % 4]
        base[:, unseen] = poison[unseen]
        base = base.view(c, x, y, z)
        wide = torch.zeros(c, x, y, z + 3)
        wide[..., 1:z + 1] = base
        layouts = {"contiguous": base.to(device),
                   "channels_last": base.permute(1, 2, 3, 0).contiguous().to(device).permute(3, 0, 1, 2),
                   "slice": wide.to(device)[..., 1:z + 1]}
        assert not layouts["slice"].is_contiguous() and not layouts["slice"].permute(1, 2, 3, 0).is_contiguous()
        seen = ~unseen
        ref = (1 - torch.exp(-density.double())).view(1, -1) * base.view(c, -1).double()
        tol = 2.0 ** -24 * ref.abs() + 2.0 ** -23 * base.view(c, -1).double().abs()
        for name, mean in layouts.items():
            out = ops.alpha_gate(mean, density.view(x, y, z).to(device), count.to(device))
            assert out.shape == mean.shape and out.dtype == torch.float32
            if name == "channels_last":
                assert out.permute(1, 2, 3, 0).is_contiguous()
            else:
                assert out.is_contiguous()            # the slice is copied: its result is contiguous
            o = out.cpu().reshape(c, -1)
            assert float(o[:, unseen].abs().sum()) == 0, (c, name)
            err = (o[:, seen].double() - ref[:, seen]).abs()
            assert bool((err <= tol[:, seen]).all()), (c, name, float((err / tol[:, seen]).max()))
            worst = max(worst, float((err / base.view(c, -1)[:, seen].double().abs()).max()))
    print(f"RAYFWD alpha_gate {grid}: worst err {worst:.2e} of |mean| (bar 2^-23 = {2.0 ** -23:.2e} of |mean| + 2^-24 of the product)")
