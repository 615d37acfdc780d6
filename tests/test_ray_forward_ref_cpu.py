"""tests/ray_forward_ref.py checked without a GPU: its float64 restatements reproduce what the real reference recorded
(tests/golden/rays_small_s*.npz) at the tolerances tests/test_rays_gpu.py uses for the same arrays; on every case of
tests/test_ray_forward_gpu.py the float32 restatement alone stays within the bar (the inputs were chosen so that the reference passes);
the inputs hold what their builders promise; and the table of floors and bars in the module's docstring is what is measured now."""
import numpy as np
import pytest
import torch

import ray_forward_ref as Rf
from conftest import load_golden, sub_state
from oracle import nerfdet_oracle as O

GOLDENS = ["rays_small_s0", "rays_small_s1"]


@pytest.fixture(scope="module")
def floors():
    return Rf.measure_floors()


# ------------------------------------------------------------------------------------------------------
# the restatements against the reference's recorded outputs
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS)
def test_float64_sampler_reproduces_the_golden(name):
    g = load_golden(name)
    s = int(g["n_samples"])
    pts, z = Rf.sample64(g["ray_o"], g["ray_d"], (0.2, 8.0), s, None)
    torch.testing.assert_close(z.float(), g["z_det"], rtol=0, atol=1e-6)
    torch.testing.assert_close(pts.float(), g["pts_det"], rtol=0, atol=2e-6)
    pts, z = Rf.sample64(g["ray_o"], g["ray_d"], (0.2, 8.0), s, g["t_rand"])
    torch.testing.assert_close(z.float(), g["z_rnd"], rtol=0, atol=1e-6)
    torch.testing.assert_close(pts.float(), g["pts_rnd"], rtol=0, atol=2e-6)


@pytest.mark.parametrize("name", GOLDENS)
def test_float64_compositor_reproduces_the_golden(name):
    g = load_golden(name)
    raw = torch.cat([g["rgb_pts"], g["sigma_pts"]], -1)
    comp = Rf.composite64(raw, g["z_rnd"], g["mask"][..., 0].sum(dim=2) > 1, False)
    for k, gk in [("rgb", "comp_rgb"), ("depth", "comp_depth"), ("weights", "comp_weights"), ("alpha", "comp_alpha"), ("transparency", "comp_T")]:
        torch.testing.assert_close(comp[k].float(), g[gk], rtol=1e-5, atol=2e-6)
    assert torch.equal(comp["mask"], g["comp_mask"])
    comp2 = Rf.composite64(g["raw_rand"], g["z_rnd"], None, True)
    torch.testing.assert_close(comp2["rgb"].float(), g["comp2_rgb"], rtol=1e-5, atol=2e-6)
    torch.testing.assert_close(comp2["depth"].float(), g["comp2_depth"], rtol=1e-5, atol=2e-6)
    assert comp2["mask"] is None


@pytest.mark.parametrize("name", GOLDENS)
def test_float64_mlp_reproduces_the_golden(name):
    g = load_golden(name)
    glob = torch.cat([g["mean"], g["var"]], dim=-1).squeeze(2)
    rgb, sigma, _ = Rf.nerf_forward64(sub_state(g, "nerf_mlp."), g["pts_rnd"], g["ray_d"], glob)
    torch.testing.assert_close(rgb.float(), g["rgb_pts"], rtol=1e-5, atol=Rf.ATOL)
    torch.testing.assert_close(sigma.float(), g["sigma_pts"], rtol=1e-5, atol=Rf.ATOL)


def test_single_sample_compositing_is_defined_as_the_first_sample_of_two():
    """The reference returns empty weights for S = 1 (the ones it prepends take their shape from an empty slice); the restatement
    composites the sample with an empty one behind it."""
    raw, z, pmask = Rf.composite_inputs(1, 1)
    out = Rf.composite64(raw, z, pmask, False)
    alpha = 1 - torch.exp(-raw[:, :, 3].double())
    assert out["weights"].shape == out["alpha"].shape == out["transparency"].shape == (1, 1)
    assert torch.equal(out["transparency"], torch.ones(1, 1, dtype=torch.float64))
    torch.testing.assert_close(out["weights"], alpha, rtol=0, atol=0)
    torch.testing.assert_close(out["rgb"], alpha * raw[:, 0, :3].double(), rtol=0, atol=1e-15)


# ------------------------------------------------------------------------------------------------------
# the encoder helper
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deg", [Rf.POS_DEG, Rf.VIEW_DEG])
def test_encoder_with_float32_arguments(deg):
    x = Rf.encoder_points(257).t()
    got = Rf.encode_f32args(x, deg)
    ref32 = O.sinusoidal_encode(x.float(), deg)
    assert got.dtype == torch.float64 and got.shape == ref32.shape == (257, 3 + 6 * deg)
    assert float((got - ref32.double()).abs().max()) <= 2 * Rf.EPS32
    assert torch.equal(got[:, :3], x.double())
    # column order: degree-major, xyz-minor, the + pi/2 half last
    k, d = 2, 1
    col = 3 + 3 * k + d
    torch.testing.assert_close(got[:, col], torch.sin(x[:, d].double() * 4), rtol=0, atol=1e-12)
    arg = (x[:, d] * 4 + torch.tensor(0.5 * np.pi, dtype=torch.float32)).double()
    assert torch.equal(got[:, col + 3 * deg], torch.sin(arg))


def test_pure_float64_encoder_is_another_function_at_the_far_end():
    """Why the helper exists: the float32 sum ``x 2^k + float32(pi / 2)`` is rounded, the float64 one is not.  The difference is NOT the
    half ulp of 4096 (2.4e-4) one would expect at |x| = 8, k = 9, and never above 1e-5: pi / 2 lies 4.45e-6 below a multiple of
    2^-12, so on every float32 grid from 2^-17 up the sum moves by exactly that.  4.45e-6 is still 30 times the encoder's bar."""
    x = Rf.encoder_points(257).t()
    diff = (Rf.encode_f32args(x, Rf.POS_DEG) - Rf.encode_f64(x, Rf.POS_DEG)).abs()
    c = 0.5 * np.pi
    gap = round(c * 4096) / 4096 - c
    assert 4.4e-6 < gap < 4.5e-6
    assert 0.99 * gap < float(diff.max()) <= gap + 1e-12
    assert float(diff.max()) > 30 * Rf.bar(("encoder_pos", Rf.POS_DEG))
    assert float(diff[x.abs().amax(1) > 4].max()) == float(diff.max())       # ... at the far end
    assert float(diff[:, :33].max()) == 0       # x and the sin(x 2^k) half have exact arguments


# ------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,s", Rf.COMPOSITE_SHAPES)
@pytest.mark.parametrize("negate", [False, True])
def test_compositing_inputs_hold_what_the_builder_promises(r, s, negate):
    raw, z, pmask = Rf.composite_inputs(r, s, negate)
    assert raw.shape == (r, s, 4) and z.shape == (r, s) and pmask.shape == (r, s) and pmask.dtype == torch.bool     # nothing filtered
    assert raw.dtype == z.dtype == torch.float32
    sigma = raw[..., 3]
    assert bool(Rf.sigma_allowed(sigma).all())
    assert not bool(((sigma > 0) & (sigma < 1e-3) & (sigma != np.float32(Rf.TINY))).any()) and not bool(((sigma > 16) & (sigma < 40)).any())
    if r >= len(Rf.ROW_KINDS):
        assert set(sigma.unique().tolist()) >= {0.0, float(np.float32(Rf.TINY)), Rf.OPAQUE}
    dz = z[:, 1:] - z[:, :-1]
    assert bool((dz <= 0).all() if negate else (dz >= 0).all())
    assert float(z.abs().min()) == float(np.float32(0.2)) and (float(z.abs().max()) == 8.0 or r * s == 1)
    if (r, s) == (130, 80):
        assert int((dz[:, 3::5] != 0).sum()) <= 1                                   # all but the planted maximum
    rows = torch.nonzero((z.abs() == z.abs().min()).any(1) | (z.abs() == z.abs().max()).any(1)).squeeze(1)
    assert int(rows.max()) - int(rows.min()) <= 1                                   # a slice of two rays holds both ends
    counts = Rf.planted_counts(r, s)
    assert pmask[:len(counts)].sum(1).tolist() == counts
    kind = Rf.row_kind(r)
    for name in ("transparent",):
        rows = sigma[kind == Rf.ROW_KINDS.index(name)]
        assert bool((rows <= np.float32(Rf.TINY)).all())
    assert bool((sigma[kind == Rf.ROW_KINDS.index("opaque_first"), 0] == Rf.OPAQUE).all())
    assert bool((sigma[kind == Rf.ROW_KINDS.index("opaque_last"), -1] == Rf.OPAQUE).all())
    if s >= 3:
        assert bool(((sigma[kind == Rf.ROW_KINDS.index("three_opaque")] == Rf.OPAQUE).sum(1) >= 3).all())
    # the fully transparent rays are clamped in float64 as in float32, at the end the sign of z names
    out = Rf.composite64(raw, z, pmask, False)
    t = kind == Rf.ROW_KINDS.index("transparent")
    assert bool((out["depth"][t] == (z.max() if negate else z.min()).double()).all())
    # ... and the planted mask rows give False, False, True, True for 0, 8, 9, S seen samples (S > 8)
    assert out["mask"][:len(counts)].tolist() == [c > 8 for c in counts]


@pytest.mark.parametrize("arch", list(Rf.MLP_ARCHS))
@pytest.mark.parametrize("r,s", Rf.MLP_SHAPES)
def test_mlp_inputs_hold_what_the_builder_promises(arch, r, s):
    pts, dirs, glob = Rf.mlp_inputs(arch, r, s)
    fdim = Rf.MLP_ARCHS[arch][1]
    assert pts.shape == (r, s, 3) and dirs.shape == (r, 3) and glob.shape == (r, s, fdim)
    assert float(pts.abs().max()) <= 8 and (r * s < 64 or float(pts.abs().max()) > 7)
    g, cls = glob.view(-1, fdim), Rf.row_class(r * s)
    for tile in range(0, r * s - 63, 64):
        assert set(cls[tile:tile + 64].tolist()) == {0, 1, 2, 3}
    assert float(g[cls == 0].abs().max()) == 0
    if r * s >= 4:
        assert float(g[cls == 2].abs().max()) > 0.5 * Rf.BRIGHT and 0 < float(g[cls == 3].abs().max()) < 1e-3
        half = fdim // 2
        assert float(g[cls == 1][:, half:].min()) > 0 and float(g[cls == 1][:, half:].max()) <= 1      # exp(-var)
        assert float(g[cls == 1][:, :3].min()) >= 0 and float(g[cls == 1][:, :3].max()) < 1           # mean colours


# ------------------------------------------------------------------------------------------------------
# the float32 restatement alone passes every case
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("near_far", Rf.SAMPLER_RANGES)
@pytest.mark.parametrize("r,s", Rf.SAMPLER_SHAPES)
def test_float32_sampler_within_the_bar_and_structured(near_far, r, s):
    near, far = Rf.f32_range(near_far)
    for jitter in ["det"] + Rf.JITTERS:
        ray_o, ray_d, t = Rf.sampler_inputs(r, s, jitter)
        pts, z = Rf.sample32(ray_o, ray_d, near_far, s, t)
        _, z64 = Rf.sample64(ray_o, ray_d, near_far, s, t)
        assert float((z.double() - z64).abs().max()) <= Rf.bar(("sampler_z", near_far)), jitter
        assert bool((z[:, 1:] >= z[:, :-1]).all()), jitter
        assert bool((z64 >= near).all() and (z64 <= far).all())
        if jitter in ("det", "zero"):
            assert bool((z[:, 0] == np.float32(near)).all())
        if jitter == "below_one":
            assert bool((z[:, -1] <= np.float32(far)).all())


@pytest.mark.parametrize("r,s", Rf.COMPOSITE_SHAPES)
def test_float32_compositor_within_the_bars(r, s):
    for white in (False, True):
        for negate in (False, True):
            f = Rf.composite_case_floor(r, s, white, negate)
            assert f["rgb"] <= Rf.ATOL / 4 and f["depth"] <= Rf.ATOL / 4, f
            for k in ("weights", "alpha", "transparency"):
                assert f[k] <= Rf.bar(("composite_" + k, (r, s))), (k, f)


@pytest.mark.parametrize("arch", list(Rf.MLP_ARCHS))
def test_float32_mlp_within_the_bars(arch):
    """sigma: within HALF of 2e-5 (1 + |sigma|) -- the rule that set BRIGHT asks a quarter, measured 3.4e-6 on the machine the table
    was written on; another CPU's GEMM sums in another order -- and rgb within its bar."""
    for r, s in Rf.MLP_SHAPES:
        rgb, sig = Rf.mlp_case_floor(arch, r, s)
        assert sig <= Rf.SIGMA_REL / 2, (r, s, sig)
        assert rgb <= Rf.bar(("mlp_rgb", arch)) <= Rf.RGB_CAP, (r, s, rgb)


# ------------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------------
def test_table_of_floors_and_bars_is_what_is_measured(floors):
    assert list(floors) == list(Rf.FLOORS)
    for key, floor in Rf.FLOORS.items():
        assert floor / 4 <= floors[key] <= Rf.bar(key), (key, floors[key], floor)
        mag = float(np.float32(key[1][1])) if key[0] == "sampler_z" else 1.0
        want = max(4 * floor, 2.0 ** -23 * mag)
        assert Rf.bar(key) == (min(want, 1e-4) if key[0] == "mlp_rgb" else want)
        assert Rf.bar(key) < 1e-3 * mag          # a missing term or a shifted index shows at 1e-3 or more
    assert Rf.render_table() in Rf.__doc__ and len(Rf.render_table().splitlines()) == 2 + len(Rf.FLOORS)
