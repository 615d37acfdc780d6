"""Hierarchical sampling without a GPU: the tests' own restatements (tests/importance_ref.py) against the fixture the real reference
produced (tests/golden/sample_pdf_det.npz, sample_pdf(det=True) of render_ray.py:96-142 on the CPU), the bound the GPU tests use
checked on the reference first, the new symbols, and every documented refusal of the two entry points -- none of which touches a device."""
import ctypes

import pytest
import torch

import importance_ref as I
from conftest import load_golden


def _fixture_cases():
    g = load_golden("sample_pdf_det")
    assert [str(p) for p in g["patterns"]] == I.WEIGHT_PATTERNS
    for ci, (s, n) in enumerate(I.SHAPES):
        assert tuple(int(v) for v in g[f"c{ci}_shape"]) == (s, n)
        yield s, n, g[f"c{ci}_bins"], g[f"c{ci}_weights"], g[f"c{ci}_samples"]


def test_restatements_meet_the_reference_fixture():
    """The float32 restatement IS the reference's det draw bit for bit (same operations, same order, on the CPU); the float64 one and
    the fixture agree in CDF space under the bound of importance_ref.cdf_bound for every weight pattern, and in depth under that bound
    times the sample's slope."""
    for s, n, bins, weights, samples in _fixture_cases():
        m = s - 2
        assert bins.shape == (len(I.WEIGHT_PATTERNS), m + 1) and weights.shape[1] == m and samples.shape[1] == n
        u = torch.linspace(0., 1., n)
        assert torch.equal(I.sample_pdf32(bins, weights, u), samples), (s, n)
        err = (I.cdf64(bins, weights, samples) - u.double()).abs().max(dim=1).values
        print(f"(S={s}, n_imp={n}): reference fp32 in CDF space, worst row {float(err.max()):.3e} (bound {I.cdf_bound(m):.3e})")
        assert float(err.max()) <= I.cdf_bound(m), (s, n, err)
        z64, slope = I.sample_pdf64(bins, weights, u)
        row = I.WEIGHT_PATTERNS.index("plateau")
        assert float(weights[row].min()) >= 0.2
        gap = (samples[row].double() - z64[row]).abs()
        assert bool((gap <= I.cdf_bound(m) * slope[row] + 1e-12).all()), (s, n, float(gap.max()))


@pytest.mark.parametrize("s,n", I.SHAPES)
def test_the_cdf_bound_holds_for_the_float32_reference_on_every_pattern(s, n):
    """What the GPU draw is held to, asked of the float32 torch restatement first (64 rays, every weight and u pattern): no pattern had
    to be dropped."""
    m, r = s - 2, 64
    bins = I.mid_bins(I.coarse_depths(r, s, seed=7))
    for wp in I.WEIGHT_PATTERNS:
        w = I.weights_of(wp, r, m, seed=8)
        keep = w.clone()
        for up in I.U_PATTERNS:
            u = I.uniforms_of(up, r, n, seed=9)
            z = I.sample_pdf32(bins, w, u)
            err = float((I.cdf64(bins, w, z) - I._rows(u, r).double()).abs().max())
            assert err <= I.cdf_bound(m), (wp, up, err, I.cdf_bound(m))
        assert torch.equal(w, keep)


def test_cdf64_inverts_the_float64_draw():
    bins = I.mid_bins(I.coarse_depths(5, 40, seed=1))
    w = I.weights_of("plateau", 5, 38, seed=2)
    u = I.uniforms_of("random", 5, 64, seed=3)
    z, slope = I.sample_pdf64(bins, w, u)
    assert float((I.cdf64(bins, w, z) - u.double()).abs().max()) <= 1e-12 and bool((slope > 0).all())


def test_the_library_exports_the_new_entry_points():
    from nerfdet_amd import _lib
    lib = _lib.load()
    for name in ("ndet_sample_pdf", "ndet_importance_merge"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.ndet_version() == 110


def test_cpu_tensors_raise():
    from nerfdet_amd import rays
    z = I.coarse_depths(2, 8, seed=0)
    w = torch.rand(2, 8)
    o, d = torch.zeros(2, 3), torch.ones(2, 3)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        rays.sample_pdf(I.mid_bins(z), w[:, 1:-1], 4, det=True)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        rays.importance_merge(z, w, o, d, 4, True)


def test_sample_pdf_refuses_bad_arguments_without_a_gpu():
    from nerfdet_amd import _lib
    lib = _lib.load()
    f = ctypes.c_void_p(0x1000)
    err = lib.ndet_last_error

    def call(bins=f, weights=f, R=8, M=62, u=f, stride=0, n=128, samples=f):
        return lib.ndet_sample_pdf(bins, weights, R, M, u, stride, n, samples, None)

    for null in ("bins", "weights", "u", "samples"):
        assert call(**{null: None}) == -1 and b"null pointer" in err(), null
    for bad in (dict(R=0), dict(R=-3), dict(M=0), dict(n=0), dict(n=-1)):
        assert call(**bad) == -1 and b"need R >= 1" in err(), bad
    for bad in (dict(stride=1), dict(stride=127), dict(stride=-128), dict(stride=256)):
        assert call(**bad) == -1 and b"u_row_stride" in err(), bad
    assert call(M=255) == -2 and b"bins" in err()
    assert call(n=257) == -2 and b"samples a ray" in err()
    assert call(R=(1 << 31) // (63 + 128) + 1) == -2 and b"2^31" in err()
    # the largest sizes are inside the limits: only the stride is refused
    assert call(M=254, n=256, stride=3) == -1 and b"u_row_stride" in err()


def test_importance_merge_refuses_bad_arguments_without_a_gpu():
    from nerfdet_amd import _lib
    lib = _lib.load()
    f = ctypes.c_void_p(0x1000)
    err = lib.ndet_last_error

    def call(z=f, w=f, o=f, d=f, R=8, S=64, u=f, stride=0, n=128, z_out=f, pts=f, zs=f):
        return lib.ndet_importance_merge(z, w, o, d, R, S, u, stride, n, z_out, pts, zs, None)

    for null in ("z", "w", "o", "d", "u", "z_out", "pts"):
        assert call(**{null: None}) == -1 and b"null pointer" in err(), null
    for bad in (dict(R=0), dict(S=2), dict(S=0), dict(n=0), dict(n=-5)):
        assert call(**bad) == -1 and b"need R >= 1" in err(), bad
    for bad in (dict(stride=64), dict(stride=1), dict(stride=-128)):
        assert call(**bad) == -1 and b"u_row_stride" in err(), bad
    assert call(S=257) == -2 and b"coarse samples" in err()
    assert call(n=257) == -2 and b"fine samples" in err()
    assert call(R=(1 << 31) // (64 + 128) + 1) == -2 and b"2^31" in err()
    assert call(R=(1 << 31) // 512, S=256, n=256) == -2 and b"2^31" in err()      # R * S_tot == 2^31 exactly
    assert call(S=256, n=256, stride=5) == -1 and b"u_row_stride" in err()


def test_the_codes_become_the_usual_exceptions():
    """NDET_E_INVALID -> AssertionError, NDET_E_UNSUPPORTED -> ValueError (nerfdet_amd._lib.check), without a device."""
    from nerfdet_amd import _lib
    with pytest.raises(AssertionError, match="need R >= 1"):
        _lib.check(_lib.load().ndet_importance_merge(*([ctypes.c_void_p(0x1000)] * 4), 4, 2, ctypes.c_void_p(0x1000), 0, 8,
                                                     *([ctypes.c_void_p(0x1000)] * 3), None), "importance_merge")
    with pytest.raises(ValueError, match="fine samples"):
        _lib.check(_lib.load().ndet_importance_merge(*([ctypes.c_void_p(0x1000)] * 4), 4, 8, ctypes.c_void_p(0x1000), 0, 300,
                                                     *([ctypes.c_void_p(0x1000)] * 3), None), "importance_merge")


def test_fine_mlp_splits_whole_rays_under_the_row_cap():
    """rays.fine_mlp is plumbing: one call up to FINE_MLP_ROWS sample rows, else the fewest calls of whole rays, equal to within one ray."""
    from nerfdet_amd import rays
    calls = []

    def mlp(p, d, g):
        assert p.shape[0] == d.shape[0] == g.shape[0]
        calls.append(p.shape[0])
        return p[..., :3] * 2.0, g[..., :1] + 1.0

    assert rays.FINE_MLP_ROWS == 8192 * 64
    for r, s, want in ((8192, 64, [8192]), (8192, 128, [4096, 4096]), (8192, 192, [2048] * 4), (5, 320, [5]), (8197, 80, [4099, 4098])):
        pts, d, g = torch.zeros(r, s, 3), torch.arange(r * 3, dtype=torch.float32).view(r, 3), torch.ones(r, s, 2)
        del calls[:]
        rgb, sigma = rays.fine_mlp(mlp, pts, d, g)
        assert calls == want and rgb.shape == (r, s, 3) and sigma.shape == (r, s, 1), (r, s, calls)
        assert all(c * s <= rays.FINE_MLP_ROWS for c in calls)
