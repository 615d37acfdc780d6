"""The forward convolutions and the fused ResNet blocks inside tests/redzone.py: every row runs under fill 0x00 and then 0xFF with its input,
residual, weights and BatchNorm statistics placed flush against guards and its packs, output, split-K workspace and amax slots carved.  Asserted per
row: no guard byte changed, no input changed, and the documented results -- the output tensor and, in the fp16-pair arithmetic, the max |out| and
tile-minimum words read the way conv3d.amax_value / conv3d.tilemin_value read them (the per-XCD sub-slots of a slot are not a documented result:
which sub-slot a workgroup commits to depends on where it ran) -- are equal bit for bit between the two fills.  Numerical correctness stays with
tests/test_f16x2_edges_gpu.py, test_conv3d_gpu.py, test_conv_batch_gpu.py, test_fused_blocks_gpu.py and test_stem_gpu.py, whose builders and rows
are imported here.  Every op here is a fixed-order sum (split-K included: test_f16x2_edges_gpu.py asserts a second launch gives the same bits)."""
import math
import types

import pytest
import torch
from torch import nn

import test_conv3d_gpu as T3
import test_conv_batch_gpu as TB
import test_f16x2_edges_gpu as E
import test_fused_blocks_gpu as FB
from redzone import both_fills

pytestmark = pytest.mark.gpu


def _results(y):
    """The documented results of a convolution launch: the tensor and, when the launch left a slot, its two words as their readers take them."""
    out = {"out": y}
    slot = getattr(y, "_ndet_amax", None)
    if slot is not None:
        out["amax"] = slot.view(-1, 32)[:, 0].max().reshape(1)
        out["tilemin"] = slot.view(torch.int32).view(-1, 32)[:, 1].max().reshape(1)
    return out


class _Arith:
    """conv3d in ``arith`` (and DIRECT_EPILOGUE as asked) with a fresh amax pool, so the slots of the run are carved too; restored on exit."""

    def __init__(self, device, arith, direct=True):
        self.device, self.arith, self.direct = device, arith, direct

    def __enter__(self):
        from nerfdet_amd import conv3d as C
        self.prev = (C.set_arithmetic(self.arith), C.DIRECT_EPILOGUE)
        C.DIRECT_EPILOGUE = self.direct
        C.AMAX.fresh(self.device)
        self.grad = torch.no_grad()
        self.grad.__enter__()

    def __exit__(self, *exc):
        from nerfdet_amd import conv3d as C
        self.grad.__exit__(*exc)
        C.set_arithmetic(self.prev[0])
        C.DIRECT_EPILOGUE = self.prev[1]
        C.AMAX.fresh(self.device)            # the pool carved in this run is not handed to whoever comes next
        return False


def _conv_row(device, case, arith, tile, splits, direct=False, batch_res=None):
    """One _Case (or _Batch) through conv2d_nhwc / conv3d_ndhwc on ``tile`` in ``arith``, twice."""
    from nerfdet_amd import conv3d as C

    def body(rz):
        with _Arith(device, arith, direct):
            x = rz.place(case.x, "x")
            up2 = isinstance(case.res, tuple)
            res = case.res[1] if up2 else case.res
            res = None if res is None else rz.place(res, "residual")
            pk = C.packed([rz.place_module(case.conv)], rz.place_module(case.bn))
            if getattr(case, "dim", 3) == 2:
                y = C.conv2d_nhwc(x, pk, residual=res, relu=case.relu, splits=splits, tile=tile, residual_up2=up2)
            else:
                y = C.conv3d_ndhwc(x, pk, residual=res, relu=case.relu, splits=splits, tile=tile)
            return _results(y)
    got = both_fills(device, body)
    assert got["out"].shape == case.ref.shape and torch.isfinite(got["out"]).all()


# ---- the table of tests/test_f16x2_edges_gpu.py, on each tile it names, plus a row that reaches the direct form of tile 12864 ----
EDGE_ROWS = list(E.ROWS) + [E._row(12864, 64, 64, (9, 8, 6), 3, 2, 1, 0, 1)]        # Cout % 32 == 0, unsplit: 112864 under direct=True


def _edge_params():
    out = []
    for p in EDGE_ROWS:
        tile = p.values[0]
        for arith in (("f16x2",) if tile == 3258 else ("bf16x3", "f16x2")):
            out.append(pytest.param(*p.values, arith, id=f"{p.id}-{arith}"))
    return out


def test_edge_table_still_holds_what_the_rows_must_include():
    from nerfdet_amd import conv_tiles
    rows = [p.values for p in EDGE_ROWS]
    assert {25, 40, 300, 304} <= {r[3] for r in rows}
    assert any(r[6] == 2 and r[7] == "conv" and any(g % 2 for g in r[4]) for r in rows), "stride 2 on odd extents"
    assert any(r[7] == "tr" for r in rows), "the k2 s2 transposed form"
    assert {2, 3, 8} <= {r[10] for r in rows} and any(r[8] == 2 and r[10] > 1 for r in rows), "split-K 2, 3, 8; ReLU before the residual with split-K"
    assert any(r[9] == 2 for r in rows), "the nearest-x2 upsampled residual"
    direct = {conv_tiles.TILES[r[0]].partner for r in rows if E._direct_ok(r[0], types.SimpleNamespace(mode=r[7]), r[3], r[10])}
    assert direct == {100064, 100128, 112864}, direct


@pytest.mark.parametrize("tile,dim,cin,cout,grid,k,stride,mode,relu,res,splits,bias,arith", _edge_params())
def test_redzone_conv_edge_row(device, tile, dim, cin, cout, grid, k, stride, mode, relu, res, splits, bias, arith):
    from nerfdet_amd import conv_tiles
    case = E._case(dim, cin, cout, grid, k, stride, mode, relu, res, bias)
    _conv_row(device, case, arith, tile, splits, direct=False)
    if E._direct_ok(tile, case, cout, splits):          # the same tile storing straight from the accumulators (100064 / 100128 / 112864)
        _conv_row(device, case, arith, conv_tiles.TILES[tile].partner, 1, direct=True)


# ---- halo tile 3128: the smallest HALO_CASES row of tests/test_conv3d_gpu.py, through _conv_split as that test calls it ----
HALO_3128 = min((r for r in T3.HALO_CASES if r[7] == 3128), key=lambda r: math.prod(r[2]))


@pytest.mark.parametrize("arith", ["bf16x3", "f16x2"])
def test_redzone_halo_3128(device, arith):
    from nerfdet_amd import conv3d as C
    cin, cout, grid, kern, relu, use_res, splits, tile = HALO_3128
    torch.manual_seed(cin + cout + sum(kern))
    conv = nn.Conv3d(cin, cout, kern, 1, tuple(k // 2 for k in kern), bias=False)
    bn = nn.BatchNorm3d(cout).eval()
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.3); bn.running_var.uniform_(0.5, 2.0); bn.weight.uniform_(0.5, 1.5); bn.bias.normal_(0, 0.3)
    x = torch.randn(*grid, cin)
    res = torch.randn(*grid, cout) if use_res else None

    def body(rz):
        with _Arith(device, arith):
            pk = C.packed([rz.place_module(conv)], rz.place_module(bn))
            out = torch.empty((*grid, cout), device=device)
            y = C._conv_split(rz.place(x, "x"), pk, out, grid, kern, (1, 1, 1), tuple(k // 2 for k in kern), False,
                              None if res is None else rz.place(res, "residual"), False, relu, splits, tile, math.prod(grid),
                              math.prod(kern) * (cin // 32), 0)
            return _results(y)
    both_fills(device, body)


# ---- the fp32-MFMA kernel (k_conv3d_igemm, with and without its split-K reduce) and the one-product bf16 arithmetic ----
@pytest.mark.parametrize("arith,tile,splits", [("f32", 64, 1), ("f32", 64, 3), ("bf16", 64, 3)])
def test_redzone_f32_and_bf16(device, arith, tile, splits):
    case = E._case(3, 128, 25, (10, 10, 4), 3, 1, "conv", 0, 0, True)          # the first row of BF16_ROWS: scalar columns, M = 400 ragged
    _conv_row(device, case, arith, tile, splits)


# ---- the batched form (_conv3d_batch) at the smallest rows of tests/test_conv_batch_gpu.py: the transposed one (60 rows) and the smallest split-K one ----
@pytest.mark.parametrize("tile,n,grid,cin,cout,k,stride,mode,relu,res,splits", [
    (64, 2, (2, 3, 5), 64, 32, 2, 2, "tr", 1, 0, 1),
    (64, 3, (3, 5, 6), 64, 40, 3, 1, "conv", 1, 1, 2),
])
@pytest.mark.parametrize("arith", ["bf16x3", "f16x2"])
def test_redzone_conv_batch(device, arith, tile, n, grid, cin, cout, k, stride, mode, relu, res, splits):
    case = TB._batch(n, grid, cin, cout, k, stride, mode, relu, res)
    _conv_row(device, case, arith, tile, splits)


# ---- fused blocks ----
CHAIN_UNSTRIDED = min((r for r in FB.CHAIN_ROWS if r[5] == 1), key=lambda r: math.prod(r[3]))
CHAIN_STRIDED = min((r for r in FB.CHAIN_ROWS if r[5] == 2), key=lambda r: math.prod(r[3]))


@pytest.mark.parametrize("arith", ["bf16x3", "f16x2"])
@pytest.mark.parametrize("row", [CHAIN_UNSTRIDED, CHAIN_STRIDED, (64, 64, 256, (1, 9, 15), 3, 1, False, 0)], ids=FB._row_id)
def test_redzone_conv_chain(device, row, arith):
    from nerfdet_amd import conv3d as C
    case = FB._chain_case(*row)

    def body(rz):
        with _Arith(device, arith):
            pk2 = C.packed([rz.place_module(case.c2)], rz.place_module(case.b2))
            pk3 = C.packed([rz.place_module(case.c3)], rz.place_module(case.b3))
            assert C.chain_ok(pk2, pk3)
            y = C.conv2d_chain_nhwc(rz.place(case.x, "x"), pk2, pk3, residual=None if case.res is None else rz.place(case.res, "residual"),
                                    relu=case.relu3)
            return _results(y)
    both_fills(device, body)


@pytest.mark.parametrize("inplanes,nhw", [(256, (1, 4, 16)), (64, (5, 3, 5))], ids=["identity-1x4x16", "downsample-5x3x5"])
def test_redzone_bottleneck(device, inplanes, nhw):
    from nerfdet_amd import conv3d as C
    ds = inplanes == 64
    blk = FB._bottleneck(int(ds), 23 + int(ds))
    torch.manual_seed(sum(nhw))
    x = FB._features(*nhw, inplanes)

    def body(rz):
        with _Arith(device, "f16x2"):
            b = rz.place_module(blk)
            pk1, pk2, pk3 = C.packed([b.conv1], b.bn1), C.packed([b.conv2], b.bn2), C.packed([b.conv3], b.bn3)
            pkd = C.packed([b.downsample[0]], b.downsample[1]) if ds else None
            return _results(C.conv2d_bottleneck_nhwc(rz.place(x, "x"), pk1, pk2, pk3, pkd))
    both_fills(device, body)


@pytest.mark.parametrize("arith", ["bf16x3", "f16x2"])
@pytest.mark.parametrize("nhw,layout", [((2, 17, 23), "view"), ((2, 61, 83), "nchw")])
def test_redzone_stem(device, nhw, layout, arith):
    from nerfdet_amd import conv3d as C
    torch.manual_seed(sum(nhw))
    n, h, w = nhw
    conv = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
    bn = nn.BatchNorm2d(64).eval()
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.3); bn.running_var.uniform_(0.5, 2.0); bn.weight.uniform_(0.5, 1.5); bn.bias.normal_(0, 0.3)
    x = torch.randn(n, 3, h, w)
    if layout == "view":                      # the image is a window of a larger buffer, as in test_fused_stem_matches_torch_fp32
        big = torch.zeros(n, 3, h + 5, w + 9)
        big[:, :, 2:2 + h, 4:4 + w] = x

    def body(rz):
        with _Arith(device, arith):
            xd = rz.place(big, "x")[:, :, 2:2 + h, 4:4 + w] if layout == "view" else rz.place(x, "x")
            c, b = rz.place_module(conv), rz.place_module(bn)
            assert C.stem_ok(c, b, xd)
            return _results(C.stem_conv_bn_relu_maxpool(xd, c, b))
    both_fills(device, body)


@pytest.mark.parametrize("nhwc", [(2, 7, 9, 64), (1, 5, 3, 68)], ids=lambda s: "x".join(map(str, s)))
def test_redzone_bn_relu_maxpool(device, nhwc):
    from nerfdet_amd import conv3d as C
    torch.manual_seed(sum(nhwc))
    bn = nn.BatchNorm2d(nhwc[3]).eval()
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.3); bn.running_var.uniform_(0.5, 2.0); bn.weight.uniform_(0.5, 1.5); bn.bias.normal_(0, 0.3)
    x = torch.randn(*nhwc)

    def body(rz):
        with torch.no_grad():
            return {"out": C.bn_relu_maxpool_nhwc(rz.place(x, "x"), rz.place_module(bn))}
    both_fills(device, body)
