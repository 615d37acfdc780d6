"""The depth gate of the reference's backproject() (nerfdet.py:404-411), restated in tests/depth_gate_ref.py, against the fixtures the real
reference produced (tests/golden/make_golden_depth.py); and the host-side checks of the gated C entry points."""
import ctypes

import pytest
import torch

from conftest import golden_meta, load_golden
from depth_gate_ref import gate_terms, gated_backproject, resize_depth


@pytest.mark.parametrize("name", ["volume_depth_s0", "volume_depth_s1"])
def test_restated_gate_equals_the_reference(name):
    g = load_golden(name)
    meta = golden_meta(g)
    vs = [float(v) for v in g["voxel_size"]]
    h, w = meta["img_shape"][0] // 4, meta["img_shape"][1] // 4
    vol, valid = gated_backproject(g["features"][:, :, :h, :w], g["points"], g["projection"], g["depth"], vs)
    assert torch.equal(valid, g["bp_valid"])
    assert torch.equal(vol[0], g["bp_volume_v0"])
    _, rgb_valid = gated_backproject(g["denorm_images"], g["points"], g["rgb_projection"], g["depth"], vs)
    assert torch.equal(rgb_valid, g["rgb_bp_valid"])
    # the scene is not vacuous: the gate removes most views and keeps some, from both band edges
    gated, ungated, z, dv = gate_terms(g["points"], g["projection"], h, w, g["depth"], vs)
    assert 0 < int(gated.sum()) < int(ungated.sum()) // 2
    assert int((ungated & (z <= dv - vs[-1])).sum()) > 50 and int((ungated & (z >= dv + vs[-1])).sum()) > 50


def test_fixture_dtypes_are_the_loaders_and_a_float32_map():
    s0, s1 = load_golden("volume_depth_s0"), load_golden("volume_depth_s1")
    assert s0["depth"].dtype == torch.float64 and tuple(s0["depth"].shape[1:]) == tuple(int(v) for v in s0["img_shape"][:2])
    assert s1["depth"].dtype == torch.float32 and bool((s1["depth"] == 0).any())
    # float32 band arithmetic is float32 subtraction with the band rounded to float32 (PyTorch's scalar promotion)
    d = s1["depth"][s1["depth"] > 0][:1000]
    assert torch.equal(d - 0.25, d - torch.tensor(0.25, dtype=torch.float32))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("src,dst", [((60, 80), (15, 20)), ((60, 80), (60, 80)), ((120, 160), (30, 40)), ((240, 320), (60, 80)),
                                     ((240, 320), (240, 320)), ((480, 640), (120, 160))])
def test_resize_form_matches_interpolate_at_integer_ratios(dtype, src, dst):
    """The form the resize kernel implements (include/nerfdet_hip.h, ndet_depth_resize) equals F.interpolate bit for bit at the ratios
    the loader's maps meet (1 and 4), on both sides of PyTorch's output-size switch."""
    torch.manual_seed(0)
    d = torch.rand(3, *src, dtype=dtype) * 5
    assert torch.equal(resize_form(d, dst), resize_depth(d, dst))


def resize_form(d, hw):
    """The kernel's arithmetic, vectorised: src = max((dst + 0.5) * (in / out) - 0.5, 0), i1 = i0 + (i0 < in - 1), and the tap sum in the
    order of PyTorch's CPU path for the output's size."""
    n, hi, wi = d.shape
    dt = d.dtype

    def axis(out, inn):
        s = torch.tensor(inn, dtype=dt) / torch.tensor(out, dtype=dt)
        src = ((torch.arange(out, dtype=dt) + 0.5) * s - 0.5).clamp(min=0)
        i0 = src.long()
        i1 = i0 + (i0 < inn - 1).long()
        l1 = src - i0.to(dt)
        return i0, i1, 1 - l1, l1
    y0, y1, ly0, ly1 = axis(hw[0], hi)
    x0, x1, lx0, lx1 = axis(hw[1], wi)
    v00, v01 = d[:, y0][:, :, x0], d[:, y0][:, :, x1]
    v10, v11 = d[:, y1][:, :, x0], d[:, y1][:, :, x1]
    ly0, ly1, lx0, lx1 = ly0[:, None], ly1[:, None], lx0[None], lx1[None]
    if hw[0] + hw[1] <= 128:     # the small-output path of PyTorch's CPU kernel
        return (((ly0 * lx0) * v00 + (ly0 * lx1) * v01) + (ly1 * lx0) * v10) + (ly1 * lx1) * v11
    return ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11)


def test_gated_entry_points_reject_bad_gates_without_a_gpu():
    from nerfdet_amd import _lib
    lib = _lib.load()
    assert lib.ndet_version() >= 109
    fake = ctypes.c_void_p(0x1000)

    def gate(**kw):
        g = _lib.NdetDepthGate(size=ctypes.sizeof(_lib.NdetDepthGate), dtype=1, n_views=2, h=4, w=4, H=16, W=16, depth_f=0x1000, f_view_pitch=16,
                               f_row_pitch=4, depth_r=0x2000, r_view_pitch=256, r_row_pitch=16, band=0.16)
        for k, v in kw.items():
            setattr(g, k, v)
        return ctypes.byref(g)

    def k1(g):
        return lib.ndet_backproject_aggregate_gated(fake, 2, 8, 4, 4, 128, 32, fake, 16, fake, None, fake, 1, fake, g, None)

    assert k1(None) == -1
    assert k1(gate(size=8)) == -1 and b"size" in lib.ndet_last_error()
    assert k1(gate(dtype=2)) == -1 and b"dtype" in lib.ndet_last_error()
    assert k1(gate(band=0.0)) == -1 and b"band" in lib.ndet_last_error()
    assert k1(gate(band=float("inf"))) == -1
    assert k1(gate(band=float("nan"))) == -1
    assert k1(gate(n_views=3)) == -1 and b"views" in lib.ndet_last_error()
    assert k1(gate(h=5)) == -1 and b"depth_f" in lib.ndet_last_error()
    assert k1(gate(f_row_pitch=3)) == -1 and b"pitch" in lib.ndet_last_error()
    # the density features need the image-sized map too
    args = (fake, 2, 8, 4, 4, 128, 32, fake, fake, 16, 16, 768, 256, 16, fake, 16, fake, fake, fake)
    assert lib.ndet_density_features_gated(*args, gate(depth_r=None), None) == -1 and b"depth_r" in lib.ndet_last_error()
    assert lib.ndet_density_features_packed_gated(*args, gate(H=15), None) == -1 and b"depth_r" in lib.ndet_last_error()
    assert lib.ndet_backproject_gated(fake, 2, 8, 4, 4, 128, 16, 4, 1, fake, 16, fake, fake, fake, gate(w=5), None) == -1
    assert lib.ndet_backproject_aggregate_bwd_gated(fake, 1, 2, 8, 4, 4, 128, 32, fake, 16, fake, fake, gate(dtype=-1), None) == -1
    assert lib.ndet_density_features_bwd_gated(fake, fake, 2, 8, 4, 4, 32, 8, fake, fake, 16, fake, fake, fake, gate(band=-1.0), None) == -1
    # the resize
    assert lib.ndet_depth_resize(fake, 3, 2, 8, 8, 64, 8, fake, 4, 4, None, 0, 0, None) == -1
    assert lib.ndet_depth_resize(fake, 0, 2, 8, 8, 64, 7, fake, 4, 4, None, 0, 0, None) == -1
    assert lib.ndet_depth_resize(fake, 0, 2, 8, 8, 64, 8, fake, 4, 4, fake, 0, 4, None) == -1


def test_backproject_keeps_refusing_malformed_depth_without_a_gpu():
    from nerfdet_amd import ops
    f = torch.zeros(2, 4, 3, 3)
    with pytest.raises(AssertionError):
        ops.backproject(f, torch.zeros(3, 2, 2, 2), torch.zeros(2, 3, 4), depth=torch.zeros(1))
    with pytest.raises(AssertionError):
        ops.backproject(f, torch.zeros(3, 2, 2, 2), torch.zeros(2, 3, 4), depth=torch.zeros(2, 3, 3), voxel_size=None)
