"""The point MLPs inside tests/redzone.py: ops.point_mlp_alpha (csrc/point_mlp_kernels.hip: 8-byte plane writes, a float4 trunk output) with
``want_raw`` and ``want_h``, and the layer-by-layer pieces it replaces -- posenc_concat, linear_rows, sigma_head -- plus sigma_to_alpha and alpha_gate.
Every row twice, fill 0x00 then 0xFF, points / conditioning / weights placed flush against guards, planes and outputs carved: no guard byte and no
input changed, alpha / raw sigma / trunk output equal bit for bit.  Numbers are held to fp64 by tests/test_volume_gpu.py
(test_fused_point_mlp_against_fp64) and tests/test_ray_forward_gpu.py; all of these kernels are one fixed-order sum per element."""
import pytest
import torch

from redzone import both_fills

pytestmark = pytest.mark.gpu


def _mlp(f):
    from nerfdet_amd.radiance_field import VanillaNeRFRadianceField
    mlp = VanillaNeRFRadianceField(4, 256, 3, f, 1, 128)
    with torch.no_grad():
        for p in mlp.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)
    return mlp


# (n, F): K0 = 160, 64, 96 and the 256 limit; tiles of 1, 64 + 1 and 2 x 64 + 2 rows, and one exact tile
@pytest.mark.parametrize("n,f", [(1, 70), (65, 0), (130, 33), (64, 193)])
def test_redzone_point_mlp_alpha(device, n, f):
    from nerfdet_amd import conv3d as C, ops
    torch.manual_seed(n + f)
    mlp = _mlp(f)
    pts = torch.rand(3, n) * 6 - 3
    glob = torch.randn(n, f) * torch.exp(torch.randn(n, 1)) if f else None
    width = (63 + f + 31) // 32 * 32
    assert width == {70: 160, 0: 64, 33: 96, 193: 256}[f]

    def body(rz):
        prev = C.set_arithmetic("f16x2")
        try:
            with torch.no_grad():
                m = rz.place_module(mlp)
                assert m.fused_ok(width)
                out = m.mlp.sigma_layer.output_layer
                alpha, raw, h = ops.point_mlp_alpha(rz.place(pts, "points"), None if glob is None else rz.place(glob, "global_feat"),
                                                    m._fused_layers(width), out.weight, out.bias, want_raw=True, want_h=True)
        finally:
            C.set_arithmetic(prev)
        return {"alpha": alpha, "raw": raw, "h": h}
    got = both_fills(device, body)
    assert got["alpha"].shape == (n,) and got["raw"].shape == (n,) and got["h"].shape == (n, 256)
    assert all(bool(torch.isfinite(v).all()) for v in got.values())


@pytest.mark.parametrize("arith", ["f16x2", "bf16x3"])
def test_redzone_layer_by_layer_mlp(device, arith):
    """n = 130: k_posenc_concat, four linear_rows launches (the MFMA kernel on (130, K) rows: three row tiles of 64, the last of two rows) and
    k_sigma_head over [h | rows[:, :n_in]] with rows wider than n_in -- the steps of VanillaNeRFRadianceField.alpha_from_points with FUSED_MLP off."""
    from nerfdet_amd import conv3d as C, ops
    n, f = 130, 33
    torch.manual_seed(n)
    mlp = _mlp(f)
    pts, glob = torch.rand(3, n) * 6 - 3, torch.randn(n, f)
    n_in, width = 63 + f, 96

    def body(rz):
        prev = C.set_arithmetic(arith)
        C.AMAX.fresh(device)
        try:
            with torch.no_grad():
                m = rz.place_module(mlp)
                rows = ops.posenc_concat(rz.place(pts, "points"), rz.place(glob, "global_feat"), pad_to=width)
                res = {"rows": rows}
                h = rows
                for i, lin in enumerate(m.mlp.base.hidden_layers):
                    h = C.linear_rows(h, C.packed_linear(lin, pad_in_to=width if i == 0 else 0), relu=1)
                    res[f"h{i}"] = h
                out = m.mlp.sigma_layer.output_layer
                res["alpha"], res["raw"] = ops.sigma_head(h, rows, n_in, out.weight, out.bias, want_raw=True)
                res["alpha_again"] = ops.sigma_to_alpha(res["raw"])
        finally:
            C.set_arithmetic(prev)
            C.AMAX.fresh(device)
        return res
    got = both_fills(device, body)
    assert got["rows"].shape == (n, width) and got["h3"].shape == (n, 256) and bool(torch.isfinite(got["alpha"]).all())


@pytest.mark.parametrize("n", [1, 130])
def test_redzone_sigma_to_alpha(device, n):
    from nerfdet_amd import ops
    torch.manual_seed(n)
    x = torch.randn(n) * 5

    def body(rz):
        return {"alpha": ops.sigma_to_alpha(rz.place(x, "raw_sigma"))}
    both_fills(device, body)


@pytest.mark.parametrize("c", [1, 3, 64])
@pytest.mark.parametrize("layout", ["contiguous", "channels_last"])
def test_redzone_alpha_gate(device, layout, c):
    """130 voxels as a (2, 5, 13) lattice, both layouts k_alpha_gate takes without a copy."""
    from nerfdet_amd import ops
    grid = (2, 5, 13)
    torch.manual_seed(c)
    mean = torch.randn(c, *grid)
    density = torch.rand(130) * 5
    count = torch.randint(0, 3, (1, *grid))
    if layout == "channels_last":
        mean = mean.permute(1, 2, 3, 0).contiguous().permute(3, 0, 1, 2)

    def body(rz):
        m = rz.place(mean, "mean")
        assert m.stride() == mean.stride()
        return {"gated": ops.alpha_gate(m, rz.place(density, "density"), rz.place(count, "count"))}
    got = both_fills(device, body)
    assert got["gated"].shape == (c, *grid)
