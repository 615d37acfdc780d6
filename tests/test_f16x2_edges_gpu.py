"""The fp16-pair convolutions (conv3d.set_arithmetic("f16x2"), csrc/conv_split_kernels.hip SCH 1: the arithmetic that ships) at the edge shapes the
bf16x3 instantiations are held to in tests/test_conv3d_gpu.py, on every tile family and with the tile that ran checked through conv3d.launch_hook:
ragged row tiles, Cout of 25 / 40 / 300 / 304, stride 2 on odd extents, the k2 s2 transposed form, ReLU before the residual with split-K, the
scalar-column epilogue, the nearest-x2 upsampled residual, and the eight-producer halo tile 3258 that exists in this arithmetic only.  Replaces the
same reference modules as tests/test_f16x2_gpu.py (mmdet3d/models/necks/imvoxelnet.py:22-67,233-260, dense_heads/imvoxel_head_v2.py:45-49, the
ResNet/FPN behind detectors/nerfdet.py:140).  Every row against an fp64 convolution of the same modules on the CPU:

* elementwise |got - ref| <= 2e-5 max(1, max|ref|) (the bar of tests/test_conv3d_gpu.py) and rel-rms < 2e-6 (test_f16x2_error_not_above_bf16x3);
  an emulation of the operand scheme alone (hi/lo fp16 of the scaled operands, three products, one fp32 rounding; K = 128 ... 6912) leaves 8e-8
  rel-rms / 9e-8 elementwise, so both bars keep more than 7x before the kernel's fp32 accumulation;
* the max |out| slot the launch leaves for the next layer is exact (split-K: committed by the reduce pass; transposed: by eight tap launches);
* a second launch gives the same bits (split-K is a fixed-order sum); the direct epilogue equals the staged one bit for bit; the persistent
  tiles equal the one-shot tile 128256 bit for bit;
* the kernel that ran is the named tile's "/f16x2" instantiation and conv_tiles.resolve left tile and splits alone.

Also: the mixed mode (fewer than F16_MIN_KSTEPS K steps run the bf16x3 kernel and still leave an exact slot), degenerate tensors (all zero, all
negative, a slot that is a loose upper bound), and the one-product bf16 arithmetic (SCH 2) on one edge row per family.

Measured on an MI355X (elementwise error / max(1, max|ref|), rel-rms, and the PRINTED, not asserted, ratio rel-rms(f16x2) / rel-rms(bf16x3) on the
same tile; rows that share a shape gave the same figures on every tile named).  No row is replaced by a rejection: the library took all of them.

    tile(s)                  cin->cout  grid      kernel        relu res splits     elem    rel-rms  f16x2/bf16x3
    64                       128->25    10x10x4   3x3x3          0   -    3      5.19e-07  3.48e-07   0.75
    12864                    128->25    10x10x4   3x3x3          0   -    2      5.53e-07  4.16e-07   0.80
    128                      64->40     7x6x5     3x3x3          0   -    1      6.77e-07  4.01e-07   0.71
    64, 128 (+ direct)       64->128    9x8x6     3x3x3 s2       1   -    1      5.79e-07  4.18e-07   0.76
    64, 128 (+ direct)       128->64    8x8x4     1x1x1 s2       0   -    1      1.95e-07  1.48e-07   0.90
    64, 128                  64->128    6x6x4     3x3x3          2   y    3      3.32e-07  1.47e-07   0.89
    64, 128                  128->32    5x4x3     transposed     1   -    1      1.56e-07  1.37e-07   0.87
    128256, 129256/257/064   64->256    9x8x6     3x3x3          1   y    1      6.28e-07  2.90e-07   0.80
    128256                   96->300    7x6x5     3x3x3 s2       0   -    1      8.72e-07  4.31e-07   0.83
    129256/257/064           96->304    7x6x5     3x3x3 s2       0   -    1      6.64e-07  4.14e-07   0.79
    128256, 129256/257/064   128->256   6x6x4     3x3x3          2   y    3      4.66e-07  1.81e-07   0.80
    128256                   256->25    10x10x4   3x3x3          0   -    2      7.54e-07  5.53e-07   0.79
    128256                   128->512   5x4x3     transposed     1   -    1      1.61e-07  7.86e-08   0.90
    129256/257/064           256->512   1x40x52   1x1x1          1   y    1      3.25e-07  1.47e-07   0.83
    129256/257/064           128->256   1x21x30   1x1 2D         0  up2   1      2.38e-07  1.16e-07   0.97
    129256/257/064           128->96    2x21x30   1x1 2D         1  up2   1      1.87e-07  1.11e-07   0.95
    129064                   1024->128  1x16x16   1x1x1          0   -    8      7.89e-08  1.43e-07   0.85
    3258                     128->300   2x15x20   3x3 2D         1   y    2      4.31e-07  2.00e-07   0.83
    3258                     96->288    5x7x9     3x3x3          0   -    3      3.33e-07  2.64e-07   0.85
    3258                     256->256   1x50x60   3x3 2D         1   y    8      3.35e-07  1.58e-07   0.87
    3258                     64->25     10x10x4   3x3x3          0   -    1      4.54e-07  3.80e-07   0.77
    3258                     64->256    6x8x16    3x3x3          2   y    1      4.40e-07  2.70e-07   0.85

The ratio stays between 0.71 and 0.97 down to K = 128 (four K steps): the 1.15 that test_f16x2_error_not_above_bf16x3 asserts at K >= 1728 would hold
on every row here as well; whether to assert it at small K is left to a later change.  Degenerate tensors (all tiles): all-negative input 7.05e-07 /
2.86e-07, loose slot 5.05e-07 / 2.64e-07.
"""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu

ELEM_BAR, RMS_BAR = 2e-5, 2e-6


def _rel_rms(a, ref):
    a, ref = a.double().cpu(), ref.double()
    return ((a - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


def _forward(conv, bn, x, dim, relu, res):
    """relu-mode(bn(conv(x)) + residual) of channels-last ``x`` ((D,H,W,C), or (N,H,W,C) for ``dim`` 2) in the dtype of the arguments.  ``res``: None,
    a tensor of the output's shape, or ("up2", coarse) = a half-resolution map added nearest-x2 upsampled."""
    y = conv(x.permute(0, 3, 1, 2) if dim == 2 else x.permute(3, 0, 1, 2).unsqueeze(0))
    if bn is not None:
        y = bn(y)
    y = y.permute(0, 2, 3, 1) if dim == 2 else y[0].permute(1, 2, 3, 0)
    if relu == 2:
        y = F.relu(y)
    if isinstance(res, tuple):
        y = y + res[1].to(y.dtype)[:, torch.arange(y.shape[1]) // 2][:, :, torch.arange(y.shape[2]) // 2]
    elif res is not None:
        y = y + res.to(y.dtype)
    if relu == 1:
        y = F.relu(y)
    return y.contiguous()


class _Case:
    """One layer on the CPU (modules, input, residual) with its fp64 result: built once per shape and shared, unchanged, by every test and tile."""

    def __init__(self, dim, cin, cout, grid, k, stride, mode, relu, res, bias, xkind):
        torch.manual_seed(1000 * dim + cin + 3 * cout + 7 * k + stride + sum(grid) + relu + 5 * res)
        self.dim, self.relu, self.mode = dim, relu, mode
        if mode == "tr":
            self.conv = nn.ConvTranspose3d(cin, cout, 2, 2, bias=False)
        else:
            self.conv = (nn.Conv2d if dim == 2 else nn.Conv3d)(cin, cout, k, stride, k // 2, bias=bias)
        self.bn = None
        if not bias:
            self.bn = (nn.BatchNorm2d if dim == 2 else nn.BatchNorm3d)(cout).eval()
            with torch.no_grad():
                self.bn.weight.uniform_(0.5, 1.5); self.bn.bias.normal_(0, 0.2); self.bn.running_mean.normal_(0, 0.2); self.bn.running_var.uniform_(0.5, 1.5)
        if xkind == "zero":
            self.x = torch.zeros(*grid, cin)
        elif xkind == "randn" or (xkind == "auto" and bias):
            self.x = torch.randn(*grid, cin)                                            # bias-only layers (heads, FPN laterals) read signed features
        else:                                                                           # post-ReLU-like, per-voxel magnitudes spread over e^+-3
            self.x = (torch.relu(torch.randn(*grid, cin)) + (0.1 if xkind == "neg" else 0.0)) * torch.exp(torch.randn(*grid, 1))
            if xkind == "neg":
                self.x = -self.x
        with torch.no_grad():
            probe = _forward(self.conv, self.bn, self.x, dim, 0, None)
            self.res = None
            if res == 1:
                self.res = torch.randn_like(probe)
            elif res == 2:
                self.res = ("up2", torch.randn(probe.shape[0], (probe.shape[1] + 1) // 2, (probe.shape[2] + 1) // 2, cout))
            self.ref = self.forward(torch.float64)

    def forward(self, dtype, conv=None, x=None):
        conv = copy.deepcopy(self.conv if conv is None else conv).to(dtype)
        bn = None if self.bn is None else copy.deepcopy(self.bn).to(dtype)
        with torch.no_grad():
            return _forward(conv, bn, (self.x if x is None else x).to(dtype), self.dim, self.relu, self.res)

    def on(self, device):
        """(x, pack, residual) on the GPU; the modules' device copies (and the weight planes cached on their pack) are made once."""
        from nerfdet_amd import conv3d as C
        if not hasattr(self, "_dev"):
            conv_d = copy.deepcopy(self.conv).to(device)
            bn_d = None if self.bn is None else copy.deepcopy(self.bn).to(device)
            res = self.res[1] if isinstance(self.res, tuple) else self.res
            self._dev = (conv_d, bn_d, C.packed([conv_d], bn_d), None if res is None else res.to(device))
        return self.x.to(device), self._dev[2], self._dev[3]


@functools.lru_cache(maxsize=None)
def _case(dim, cin, cout, grid, k, stride, mode, relu, res, bias, xkind="auto"):
    return _Case(dim, cin, cout, grid, k, stride, mode, relu, res, bias, xkind)


def _launch(device, case, arith, tile, splits, direct=True, prepare=None):
    """One launch of ``case`` in ``arith`` on ``tile``; returns (out, kernel names the launch hook saw, (tile, splits) conv_tiles.resolve handed to the
    library).  ``prepare(x)`` may tag the device input before the launch."""
    from nerfdet_amd import conv3d as C, conv_tiles
    x, pk, res = case.on(device)
    if prepare is not None:
        prepare(x)
    names, resolved = [], []
    real_resolve = conv_tiles.resolve

    def hook(flops, thunk, name):
        names.append(name)
        return thunk()

    def resolve(*a, **kw):
        resolved.append(real_resolve(*a, **kw))
        return resolved[-1]
    prev, prev_direct, prev_hook = C.set_arithmetic(arith), C.DIRECT_EPILOGUE, C.launch_hook
    try:
        C.DIRECT_EPILOGUE, C.launch_hook, conv_tiles.resolve = direct, hook, resolve
        with torch.no_grad():
            if case.dim == 2:
                y = C.conv2d_nhwc(x, pk, residual=res, relu=case.relu, splits=splits, tile=tile, residual_up2=isinstance(case.res, tuple))
            else:
                y = C.conv3d_ndhwc(x, pk, residual=res, relu=case.relu, splits=splits, tile=tile)
        torch.cuda.synchronize()
    finally:
        C.set_arithmetic(prev)
        C.DIRECT_EPILOGUE, C.launch_hook, conv_tiles.resolve = prev_direct, prev_hook, real_resolve
    return y, names, resolved[-1]


def _errors(got, ref):
    """(max |got - ref| / max(1, max|ref|), rel-rms) against the fp64 result."""
    assert tuple(got.shape) == tuple(ref.shape)
    return float((got.double().cpu() - ref).abs().max()) / max(1.0, float(ref.abs().max())), _rel_rms(got, ref)


def _slot_is_exact(got):
    from nerfdet_amd import conv3d as C
    assert C.amax_value(got._ndet_amax) == float(got.abs().max()), "the launch's max |out| slot is not the tensor's maximum"


def _ran(names, resolved, tile, splits, suffix):
    """The launch was the asked tile's kernel in the asked arithmetic, with the asked split: nothing re-routed on the way."""
    from nerfdet_amd import conv_tiles
    assert names == [conv_tiles.TILES[tile].name + suffix], (names, tile)
    assert resolved == (tile, splits), (resolved, tile, splits)


def _direct_ok(tile, case, cout, splits):
    from nerfdet_amd import conv_tiles
    return conv_tiles.TILES[tile].family == "unified" and splits == 1 and case.mode != "tr" and cout % 32 == 0


def _row(tile, cin, cout, grid, k, stride, relu, res, splits, dim=3, mode="conv", bias=False):
    name = f"{tile}-{cin}to{cout}-{'x'.join(map(str, grid))}-{'tr' if mode == 'tr' else f'k{k}s{stride}'}{'-2d' if dim == 2 else ''}-relu{relu}-res{res}-sp{splits}"
    return pytest.param(tile, dim, cin, cout, grid, k, stride, mode, relu, res, splits, bias, id=name)


def _family_rows(tiles, *rows, **kw):
    return [_row(t, *r, **kw) for r in rows for t in tiles]


WSP = (129256, 129257, 129064)
ROWS = (
    # tile, cin, cout, grid, k, stride, relu (0 none / 1 after / 2 before the residual), residual (0 none / 1 plain / 2 nearest-x2 upsampled), splits
    # ---- unified tiles ----
    [_row(64, 128, 25, (10, 10, 4), 3, 1, 0, 0, 3, bias=True),          # scalar columns, M = 400 ragged; the non-vector reduce commits the slot
     _row(12864, 128, 25, (10, 10, 4), 3, 1, 0, 0, 2),                  # the production head row
     _row(128, 64, 40, (7, 6, 5), 3, 1, 0, 0, 1, bias=True)]            # Cout % 32 != 0: staged; M = 210
    + _family_rows((64, 128),
                   (64, 128, (9, 8, 6), 3, 2, 1, 0, 1),                 # stride 2 on odd extents; direct + staged
                   (128, 64, (8, 8, 4), 1, 2, 0, 0, 1),                 # 1x1x1 stride 2, exactly F16_MIN_KSTEPS K steps
                   (64, 128, (6, 6, 4), 3, 1, 2, 1, 3))                 # ReLU before the residual in the reduce pass
    + _family_rows((64, 128), (128, 32, (5, 4, 3), 2, 2, 1, 0, 1), mode="tr")      # k2 s2 transposed: eight tap launches
    # ---- wave-specialised 128 x 256 ----
    + _family_rows((128256,),
                   (64, 256, (9, 8, 6), 3, 1, 1, 1, 1),                 # M = 432 ragged
                   (96, 300, (7, 6, 5), 3, 2, 0, 0, 1),                 # ragged Cout past one tile, stride 2
                   (128, 256, (6, 6, 4), 3, 1, 2, 1, 3),                # split-K, ReLU before the residual
                   (256, 25, (10, 10, 4), 3, 1, 0, 0, 2))               # scalar columns with split-K
    + _family_rows((128256,), (128, 512, (5, 4, 3), 2, 2, 1, 0, 1), mode="tr")
    # ---- its persistent forms ----
    + _family_rows(WSP,
                   (64, 256, (9, 8, 6), 3, 1, 1, 1, 1),                 # M = 432 ragged
                   (96, 304, (7, 6, 5), 3, 2, 0, 0, 1),                 # Cout past one tile, stride 2
                   (128, 256, (6, 6, 4), 3, 1, 2, 1, 3),                # split-K, ReLU before the residual
                   (256, 512, (1, 40, 52), 1, 1, 1, 1, 1))              # two column tiles over the persistent grid
    + _family_rows(WSP,
                   (128, 256, (1, 21, 30), 1, 1, 0, 2, 1),              # FPN lateral: upsampled residual, odd map height
                   (128, 96, (2, 21, 30), 1, 1, 1, 2, 1), dim=2)        # ... with Cout * 4 not a power of two
    + [_row(129064, 1024, 128, (1, 16, 16), 1, 1, 0, 0, 8)]             # Cout = half a tile, many splits (the weight-gradient shape class)
    # ---- halo-stationary, eight producer waves ----
    + [_row(3258, 128, 300, (2, 15, 20), 3, 1, 1, 1, 2, dim=2),         # ragged Cout, split-K
       _row(3258, 96, 288, (5, 7, 9), 3, 1, 0, 0, 3),                   # 3x3x3, splits = Cin / 32
       _row(3258, 256, 256, (1, 50, 60), 3, 1, 1, 1, 8, dim=2),         # the production row (3000, 256, 72) -> (3258, 8)
       _row(3258, 64, 25, (10, 10, 4), 3, 1, 0, 0, 1),                  # scalar columns
       _row(3258, 64, 256, (6, 8, 16), 3, 1, 2, 1, 1)]                  # ReLU before the residual
)


@pytest.mark.parametrize("tile,dim,cin,cout,grid,k,stride,mode,relu,res,splits,bias", ROWS)
def test_f16x2_edge_row(device, request, tile, dim, cin, cout, grid, k, stride, mode, relu, res, splits, bias):
    from nerfdet_amd import conv3d as C, conv_tiles
    row = conv_tiles.TILES[tile]
    assert (1 if mode == "tr" else k ** dim) * cin // 32 >= C.F16_MIN_KSTEPS, "too few K steps: the row would run the bf16x3 kernel"
    case = _case(dim, cin, cout, grid, k, stride, mode, relu, res, bias)
    got, names, resolved = _launch(device, case, "f16x2", tile, splits, direct=False)
    _ran(names, resolved, tile, splits, "/f16x2")
    _slot_is_exact(got)
    elem, rms = _errors(got, case.ref)
    again, _, _ = _launch(device, case, "f16x2", tile, splits, direct=False)
    assert torch.equal(got, again), "the same launch twice: split-K is a fixed-order sum"
    if _direct_ok(tile, case, cout, splits):         # the same tile storing straight from the accumulators: the same bits
        direct, names, resolved = _launch(device, case, "f16x2", row.partner, 1, direct=True)
        _ran(names, resolved, row.partner, 1, "/f16x2")
        _slot_is_exact(direct)
        assert torch.equal(direct, got), "direct and staged epilogue differ"
    if row.family == "wsp":                          # same K walk, same epilogue arithmetic as the one-shot tile
        one_shot, names, resolved = _launch(device, case, "f16x2", 128256, splits, direct=False)
        _ran(names, resolved, 128256, splits, "/f16x2")
        assert torch.equal(got, one_shot), "the persistent tile must reproduce the one-shot tile bit for bit"
    ref3, names, _ = _launch(device, case, "bf16x3", tile, splits, direct=False)
    assert names == [row.name]
    elem3, rms3 = _errors(ref3, case.ref)
    print(f"EDGE {request.node.callspec.id}: elem {elem:.2e} rel-rms {rms:.2e} | bf16x3 elem {elem3:.2e} rel-rms {rms3:.2e} | f16x2/bf16x3 {rms / rms3:.2f}")
    assert elem <= ELEM_BAR and rms < RMS_BAR, (elem, rms)


@pytest.mark.parametrize("tile", [64, 128256])
def test_f16x2_mode_keeps_short_k_walks_on_bf16x3(device, tile):
    """Fewer than F16_MIN_KSTEPS K steps under ARITHMETIC == "f16x2": the launch is the six-product kernel (HBM-bound, nothing to gain), and it
    still leaves the exact max |out| slot the next fp16-pair layer scales by."""
    from nerfdet_amd import conv3d as C, conv_tiles
    case = _case(3, 32, 256, (3, 12, 16), 1, 1, "conv", 1, 0, False)
    assert 32 // 32 < C.F16_MIN_KSTEPS
    got, names, resolved = _launch(device, case, "f16x2", tile, 1)
    assert names == [conv_tiles.TILES[tile].name], names
    assert resolved == ((conv_tiles.TILES[tile].partner or tile), 1), resolved        # (the unified tile in its direct form: Cout % 32 == 0)
    _slot_is_exact(got)
    elem, rms = _errors(got, case.ref)
    assert elem <= ELEM_BAR and rms < RMS_BAR, (elem, rms)


DEGENERATE_TILES = [64, 128256, 129064, 3258]      # one tile per family
DEGENERATE = dict(dim=3, cin=64, cout=96, grid=(5, 6, 7), k=3, stride=1, mode="conv", relu=1, res=1, bias=False)     # M = 210 ragged, BatchNorm, residual, ReLU


@pytest.mark.parametrize("tile", DEGENERATE_TILES)
def test_f16x2_all_zero_input_with_a_zero_slot(device, tile):
    """max |x| = 0 (an empty scene's volume): the scale derived from a zero slot is finite, the accumulators are zero, and the output is exactly
    relu(shift + residual)."""
    from nerfdet_amd import conv3d as C
    case = _case(**DEGENERATE, xkind="zero")
    got, names, _ = _launch(device, case, "f16x2", tile, 1, prepare=lambda x: C._tag_amax(x, C.AMAX.take(device), produced=False))
    assert names[0].endswith("/f16x2")
    _, pk, res = case.on(device)
    assert torch.isfinite(got).all()
    assert torch.equal(got, torch.relu(pk.shift.view(1, 1, 1, -1) + res))
    _slot_is_exact(got)


@pytest.mark.parametrize("tile", DEGENERATE_TILES)
@pytest.mark.parametrize("kind", ["negative", "loose_slot"])
def test_f16x2_negative_input_and_loose_upper_bound(device, tile, kind):
    """An all-negative tensor (the maximum is of |x|), and an input whose slot holds a LOOSE upper bound (8 max|x|: conv_train._per_scene and _rows
    hand a scene / a tap copy the slot of the larger tensor it came from -- "an upper bound is all the scale needs"): the bars of the matrix."""
    from nerfdet_amd import conv3d as C
    case = _case(**DEGENERATE, xkind="neg" if kind == "negative" else "auto")
    prepare = None
    if kind == "loose_slot":
        prepare = lambda x: C._tag_amax(x, C.amax_of(x * 8.0), produced=False)
    got, names, _ = _launch(device, case, "f16x2", tile, 1, prepare=prepare)
    assert names[0].endswith("/f16x2")
    _slot_is_exact(got)
    elem, rms = _errors(got, case.ref)
    print(f"DEGENERATE {tile} {kind}: elem {elem:.2e} rel-rms {rms:.2e}")
    assert elem <= ELEM_BAR and rms < RMS_BAR, (elem, rms)


@pytest.mark.parametrize("tile", DEGENERATE_TILES)
def test_f16x2_rows_past_m_stay_out_of_the_slot(device, tile):
    """The rows of the last tile past M hold zero accumulators: through the epilogue they are ``shift``, values that are not the layer's.  Here one channel
    has non-negative weights, a bias of 1000 and a strictly negative input, so every output of it lies BELOW 1000 and a slot that let a row past M in
    reads exactly 1000 (the ordinary rows cannot tell: there |shift| is below the tensor's maximum).  Staged and direct epilogue of the unified tile."""
    from nerfdet_amd import conv_tiles
    case = _Case(3, 64, 96, (5, 6, 7), 3, 1, "conv", 0, 0, True, "neg")             # M = 210: ragged on 64- and 128-row tiles
    with torch.no_grad():
        case.conv.weight[7].abs_()
        case.conv.bias[7] = 1000.0
    case.ref = case.forward(torch.float64)
    top = float(case.ref.abs().max())
    assert float(case.ref[..., 7].max()) < 1000.0 and 900.0 < top < 1000.0, "the row does not separate the two maxima"
    forms = [(tile, False)] + ([(conv_tiles.TILES[tile].partner, True)] if _direct_ok(tile, case, 96, 1) else [])
    for t, direct in forms:
        got, names, resolved = _launch(device, case, "f16x2", t, 1, direct=direct)
        _ran(names, resolved, t, 1, "/f16x2")
        _slot_is_exact(got)
        elem, rms = _errors(got, case.ref)
        assert elem <= ELEM_BAR and rms < RMS_BAR, (elem, rms)


BF16_ROWS = [
    # one edge row per family from the matrix above
    _row(64, 128, 25, (10, 10, 4), 3, 1, 0, 0, 3, bias=True),           # unified: scalar columns, ragged rows, split-K
    _row(128, 128, 32, (5, 4, 3), 2, 2, 1, 0, 1, mode="tr"),            # unified: transposed
    _row(128256, 96, 300, (7, 6, 5), 3, 2, 0, 0, 1),                    # ws: ragged Cout, stride 2
    _row(129064, 128, 256, (6, 6, 4), 3, 1, 2, 1, 3),                   # wsp: split-K, ReLU before the residual
    _row(3258, 96, 288, (5, 7, 9), 3, 1, 0, 0, 3),                      # halo (eight producers in this arithmetic too): 3x3x3, ragged, split-K
]


@pytest.mark.parametrize("tile,dim,cin,cout,grid,k,stride,mode,relu,res,splits,bias", BF16_ROWS)
def test_bf16_edge_row(device, tile, dim, cin, cout, grid, k, stride, mode, relu, res, splits, bias):
    """set_arithmetic("bf16") (SCH 2: one operand plane, its own LDS sizing): the convolution of the bf16-ROUNDED operands accumulated in fp32, as
    test_bf16_arithmetic_is_a_bf16_rounded_convolution states it -- within 2e-5 max|ref| of PyTorch-CPU fp32 on operands rounded the same way, and at
    least 1e-4 max|ref| away from the unrounded result."""
    from nerfdet_amd import conv_tiles
    case = _case(dim, cin, cout, grid, k, stride, mode, relu, res, bias)
    rounded = copy.deepcopy(case.conv)
    with torch.no_grad():
        rounded.weight.copy_(rounded.weight.bfloat16().float())
    ref = case.forward(torch.float32, conv=rounded, x=case.x.bfloat16().float())
    full = case.forward(torch.float32)
    got, names, resolved = _launch(device, case, "bf16", tile, splits, direct=False)
    assert names == [conv_tiles.TILES[tile].name] and resolved == (tile, splits), (names, resolved)
    scale = float(ref.abs().max())
    assert float((got.cpu() - ref).abs().max()) <= 2e-5 * scale
    assert float((got.cpu() - full).abs().max()) >= 1e-4 * scale
