"""The training kernels inside tests/redzone.py: the convolutions' data and weight gradients (ConvS1, ConvT2: adjoint launches, the implicit and
staged weight-gradient forms with the split counts the plan picks), BatchNormRows forward and backward, the fused ReLU-affine backward, and the
K1 / K2 / K4 / compositing backward kernels.  Every row twice, fill 0x00 then 0xFF, inputs and upstream gradients placed flush against guards,
planes, padded gradients, split-K workspaces, statistics and results carved: no guard byte and no input changed, the results equal bit for bit.

Deterministic modes only: autograd.set_deterministic(True) (the fixed-point scatter of K1 / K2 / K4 backward, the MFMA form of the stride-2 data
gradient), and split-K sums that are added in index order (tests/test_wgrad_shapes_gpu.py::test_partial_sums_are_added_in_index_order).
BatchNormRows updates ``running_mean`` / ``running_var`` in place as torch's batch_norm does ("written through raw pointers", conv_train.py): those
placed tensors are named as written and are results of the row.  Numbers are held to fp64 by tests/test_dgrad_shapes_gpu.py,
test_wgrad_shapes_gpu.py, test_conv_train_gpu.py and test_backward_shapes_gpu.py."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import nerfdet_oracle as O
from redzone import both_fills

pytestmark = pytest.mark.gpu

ARITHS = ("f16x2", "bf16x3")


@contextlib.contextmanager
def _training(device, arith):
    """fp16-pair mode with the training arithmetic ``arith``, the deterministic scatter / data-gradient mode, a fresh (so: carved) amax pool."""
    from nerfdet_amd import autograd as A, conv3d as C
    prev = (C.set_arithmetic("f16x2"), C.TRAIN_F16X2, A.set_deterministic(True))
    C.TRAIN_F16X2 = arith == "f16x2"
    C.AMAX.fresh(device)
    try:
        assert C.train_arithmetic() == arith
        yield
    finally:
        C.set_arithmetic(prev[0])
        C.TRAIN_F16X2 = prev[1]
        A.set_deterministic(prev[2])
        C.AMAX.fresh(device)


# ---- data and weight gradients: (input grid, Cin, Cout, k, stride) ----
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("grid,cin,cout,k,stride", [((8, 8, 4), 128, 25, 3, 1), ((9, 8, 6), 64, 64, 3, 2), ((7, 6, 5), 64, 40, 1, 1)],
                         ids=["8x8x4-128to25-k3s1", "9x8x6-64to64-k3s2", "7x6x5-64to40-k1s1"])
def test_redzone_conv_gradients(device, grid, cin, cout, k, stride, arith):
    """ConvS1 forward and backward: Cout 25 (dy zero-padded to 32 channels for the adjoint launch, a ragged Cout in k_wgrad_to_torch), stride 2 on odd
    extents (dy scattered into a zero tensor of the input's extent), a 1x1 layer (the staged weight gradient)."""
    from nerfdet_amd.conv_train import ConvS1
    torch.manual_seed(sum(grid) + cin + cout)
    x, w = torch.randn(*grid, cin), torch.randn(cout, cin, k, k, k) / (cin * k ** 3) ** 0.5
    out = tuple((n + 2 * (k // 2) - k) // stride + 1 for n in grid)
    dy = torch.randn(*out, cout)

    def body(rz):
        with _training(device, arith):
            xd, wd = rz.place(x, "x").requires_grad_(True), rz.place(w, "weight").requires_grad_(True)
            y = ConvS1.apply(xd, wd, stride)
            y.backward(rz.place(dy, "dy"))
            return {"y": y.detach(), "dx": xd.grad, "dw": wd.grad}
    got = both_fills(device, body)
    assert got["dx"].shape == x.shape and got["dw"].shape == w.shape and got["y"].shape == dy.shape


@pytest.mark.parametrize("arith", ARITHS)
def test_redzone_transposed_conv_gradients(device, arith):
    """ConvT2 ((5, 4, 3), 64 -> 32): eight tap launches forward; the data gradient is the unpadded k2 s2 convolution, the weight gradient the staged
    form with the roles of x and dy swapped."""
    from nerfdet_amd.conv_train import ConvT2
    torch.manual_seed(12)
    x, w, dy = torch.randn(5, 4, 3, 64), torch.randn(64, 32, 2, 2, 2) / 8, torch.randn(10, 8, 6, 32)

    def body(rz):
        with _training(device, arith):
            xd, wd = rz.place(x, "x").requires_grad_(True), rz.place(w, "weight").requires_grad_(True)
            y = ConvT2.apply(xd, wd)
            y.backward(rz.place(dy, "dy"))
            return {"y": y.detach(), "dx": xd.grad, "dw": wd.grad}
    both_fills(device, body)


@pytest.mark.parametrize("arith", ARITHS)
def test_redzone_implicit_weight_gradient(device, arith):
    """weight_grad(implicit=True) at ((8, 8, 4), 128, 25, 3, 1): k_wgrad_split reads x in place with the split count implicit_plan picks (256 voxels: 8 K
    steps), then ndet_wgrad_to_torch."""
    from nerfdet_amd import conv_train
    torch.manual_seed(3)
    x, dy = torch.randn(8, 8, 4, 128), torch.randn(8, 8, 4, 25)

    def body(rz):
        with _training(device, arith):
            return {"dw": conv_train.weight_grad(rz.place(x, "x"), rz.place(dy, "dy"), (3, 3, 3), 1, implicit=True)}
    got = both_fills(device, body)
    assert got["dw"].shape == (25, 128, 3, 3, 3)


# ---- BatchNormRows ----
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("relu,with_res", [(False, False), (True, True)], ids=["plain", "relu-res"])
@pytest.mark.parametrize("n,c", [(777, 128), (50, 64), (5, 4)])
def test_redzone_batch_norm_rows(device, n, c, relu, with_res, arith):
    from nerfdet_amd.conv_train import BatchNormRows
    torch.manual_seed(n + c)
    x, res, g = torch.randn(n, c) * 2 + 0.5, torch.randn(n, c), torch.randn(n, c)
    gamma, beta = torch.rand(c) + 0.5, torch.randn(c) * 0.2
    rmean, rvar = torch.randn(c) * 0.1, torch.rand(c) + 0.5

    def body(rz):
        with _training(device, arith):
            xd = rz.place(x, "x").requires_grad_(True)
            wd, bd = rz.place(gamma, "weight").requires_grad_(True), rz.place(beta, "bias").requires_grad_(True)
            rd = rz.place(res, "residual").requires_grad_(True) if with_res else None
            rm, rv = rz.place(rmean, "running_mean"), rz.place(rvar, "running_var")
            y = BatchNormRows.apply(xd, wd, bd, rm, rv, 0.1, 1e-5, relu, rd)
            y.backward(rz.place(g, "dy"))
            out = {"y": y.detach(), "dx": xd.grad, "dgamma": wd.grad, "dbeta": bd.grad, "running_mean": rm, "running_var": rv}
            if with_res:
                out["dres"] = rd.grad
            slot = getattr(y, "_ndet_amax", None)
            if slot is not None:
                out["amax"] = slot.view(-1, 32)[:, 0].max().reshape(1)
            return out
    both_fills(device, body, written=("running_mean", "running_var"))


# ---- the fused ReLU-affine backward at (50, 64): 50 rows of 64 channels ----
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("relu,with_res", [(True, True), (False, False)], ids=["relu-res", "plain"])
def test_redzone_relu_affine_backward(device, relu, with_res, arith):
    from nerfdet_amd.conv_train import ConvAffineAct
    torch.manual_seed(50 + 64)
    x, w = torch.randn(1, 5, 10, 64), torch.randn(64, 64, 3, 3) / 24
    scale, shift = torch.rand(64) + 0.5, torch.randn(64) * 0.2
    res, g = torch.randn(1, 5, 10, 64), torch.randn(1, 5, 10, 64)

    def body(rz):
        with _training(device, arith):
            xd, wd = rz.place(x, "x").requires_grad_(True), rz.place(w, "weight").requires_grad_(True)
            rd = rz.place(res, "residual").requires_grad_(True) if with_res else None
            y = ConvAffineAct.apply(xd, wd, rz.place(scale, "scale"), rz.place(shift, "shift"), rd, relu, 1)
            y.backward(rz.place(g, "dy"))
            out = {"y": y.detach(), "dx": xd.grad, "dw": wd.grad}
            if with_res:
                out["dres"] = rd.grad
            return out
    both_fills(device, body)


# ---- K1 / K2 / K4 / compositing backward: the smallest row of each table of tests/test_backward_shapes_gpu.py, deterministic scatter ----
HW, GRID, VOXEL = (240, 320), (15, 11, 7), (0.36, 0.36, 0.36)
FHW = (HW[0] // 4, HW[1] // 4)


def _scene(n_v, hw=HW):
    meta = O.ring_scene_meta(n_v, hw)
    return meta, O.compute_projection(meta, 4), O.compute_projection(meta, 1), O.get_points(GRID, VOXEL, meta["lidar2img"]["origin"])


@pytest.mark.parametrize("cl_out", [True, False], ids=["channels_last", "contiguous"])
def test_redzone_k1_backward(device, cl_out):
    """K1_CASES[0]: C = 256, 40 views."""
    from nerfdet_amd.autograd import BackprojectMean
    c, n_v = 256, 40
    _, proj, _, pts = _scene(n_v)
    gen = torch.Generator().manual_seed(1000 * n_v + c)
    feat = torch.randn(n_v, c, *FHW, generator=gen).contiguous(memory_format=torch.channels_last)
    g = torch.randn(c, *GRID, generator=gen)
    if cl_out:
        g = g.permute(1, 2, 3, 0).contiguous().permute(3, 0, 1, 2)

    def body(rz):
        with _training(device, "f16x2"):
            fd = rz.place(feat, "features").requires_grad_(True)
            out, count = BackprojectMean.apply(fd, rz.place(pts, "points"), rz.place(proj, "projection"), cl_out, None)
            torch.autograd.backward(out, rz.place(g, "g"))
            return {"volume": out.detach(), "count": count, "dfeatures": fd.grad}
    both_fills(device, body)


def test_redzone_k2_backward(device):
    """K2_CASES: cm = 5, 65 views (the smallest map of the table; an odd channel count, one view past a round of 64)."""
    from nerfdet_amd.autograd import DensityFeatures
    cm, n_v = 5, 65
    _, proj, rgb_proj, pts = _scene(n_v)
    gen = torch.Generator().manual_seed(7 * n_v + cm)
    mapped = torch.randn(n_v, cm, *FHW, generator=gen).contiguous(memory_format=torch.channels_last)
    bias = 0.5 * torch.randn(cm, generator=gen)
    rgb = torch.rand(n_v, 3, *HW, generator=gen)
    g = torch.randn(GRID[0] * GRID[1] * GRID[2], 2 * (3 + cm), generator=gen)

    def body(rz):
        with _training(device, "f16x2"):
            md, bd = rz.place(mapped, "mapped").requires_grad_(True), rz.place(bias, "bias").requires_grad_(True)
            glob = DensityFeatures.apply(md, bd, rz.place(rgb, "images"), rz.place(pts, "points"), rz.place(proj, "projection"),
                                         rz.place(rgb_proj, "rgb_projection"), None)
            torch.autograd.backward(glob, rz.place(g, "g"))
            return {"rows": glob.detach(), "dmapped": md.grad, "dbias": bd.grad}
    both_fills(device, body)


@pytest.mark.parametrize("n_v,d,img_hw,packed", [(20, 64, (240, 320), True), (40, 8, (240, 320), False)], ids=["packed", "generic"])
def test_redzone_k4_backward(device, n_v, d, img_hw, packed):
    """K4_CASES: the smallest packed and the smallest generic row, over 65 rays of 19 samples."""
    from nerfdet_amd import rays
    from nerfdet_amd.autograd import RayViewStats
    assert rays.packed_ok(n_v, d, backward=True) == packed
    gen = torch.Generator().manual_seed(n_v * 100 + d)
    meta = O.ring_scene_meta(n_v, img_hw)
    feat = torch.randn(n_v, d, img_hw[0] // 4, img_hw[1] // 4, generator=gen).contiguous(memory_format=torch.channels_last)
    img = torch.rand(n_v, 3, *img_hw, generator=gen)
    r, s = 65, 19
    ang = torch.rand(r, generator=gen) * 2 * np.pi
    ray_o = torch.stack([2.0 * torch.cos(ang), 2.0 * torch.sin(ang), 1.0 + 0.3 * torch.rand(r, generator=gen)], -1)
    ray_d = -ray_o / ray_o.norm(dim=-1, keepdim=True) + 0.35 * torch.randn(r, 3, generator=gen)
    pts = (torch.linspace(0.2, 8.0, s)[None, :, None] * ray_d[:, None] + ray_o[:, None]).contiguous()
    g = torch.randn(r, s, 2 * (3 + d), generator=gen)
    cams = rays._compute_projection(meta)

    def body(rz):
        with _training(device, "f16x2"):
            rays._PACKED_RGB.clear()
            try:
                fd = rz.place(feat, "features").requires_grad_(True)
                glob, pm, vc = RayViewStats.apply(fd, rz.place(pts, "pts"), rz.place(img, "images"), cams)
                torch.autograd.backward(glob, rz.place(g, "g"))
            finally:
                rays._PACKED_RGB.clear()
            return {"globalfeat": glob.detach(), "pixel_mask": pm, "view_count": vc, "dfeatures": fd.grad}
    both_fills(device, body)


@pytest.mark.parametrize("white", [False, True])
def test_redzone_composite_backward(device, white):
    """The compositor under autograd at 65 rays of 64 samples (the table's sample count, one ray past a wave)."""
    from nerfdet_amd import rays
    gen = torch.Generator().manual_seed(11 + int(white))
    r, s = 65, 64
    raw = torch.cat([torch.rand(r, s, 3, generator=gen), 3 * torch.rand(r, s, 1, generator=gen) ** 3], -1)
    raw[:8, :, 3] = 0.0
    raw[8:16, 20, 3] = 40.0
    z = torch.sort(torch.rand(r, s, generator=gen) * 7.8 + 0.2, dim=1)[0]
    pmask = torch.rand(r, s, generator=gen) < 0.2
    w_rgb, w_dep = torch.randn(r, 3, generator=gen), torch.randn(r, generator=gen)

    def body(rz):
        with _training(device, "f16x2"):
            b = rz.place(raw, "raw").requires_grad_(True)
            p = rays.raw2outputs(b, rz.place(z, "z_vals"), rz.place(pmask, "mask"), white_bkgd=white)
            torch.autograd.backward((p["rgb"], p["depth"]), (rz.place(w_rgb, "w_rgb"), rz.place(w_dep, "w_dep")))
            return {"rgb": p["rgb"].detach(), "depth": p["depth"].detach(), "weights": p["weights"].detach(), "draw": b.grad}
    both_fills(device, body)
