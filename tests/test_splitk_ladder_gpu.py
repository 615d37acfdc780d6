"""The split-K factor of the forward split-family convolutions (csrc/conv_split_kernels.hip: the unified tiles' conv_split_mainloop, k_conv_split_ws,
k_conv_split_wsp, k_conv_split_halo, and k_conv3d_splitk_reduce behind them) at EVERY split count the tables and conv3d.choose_tiling_split can
dispatch, on every tile id of conv_tiles.ids("unified", "ws", "wsp", "halo"), in the arithmetic that ships (f16x2) and in bf16x3.  The layers are those
of tests/test_f16x2_edges_gpu.py (mmdet3d/models/necks/imvoxelnet.py:22-67,233-260, dense_heads/imvoxel_head_v2.py:45-49, the ResNet/FPN behind
detectors/nerfdet.py:140), whose rows launch with splits in {1, 2, 3, 8} only.

Why the split count is an edge of its own: split s of S walks the K steps [n s / S, n (s + 1) / S) -- neighbouring walks differ by one step and start
in the middle of a tap sequence or a channel chunk; the wave-specialised kernels round each walk up to a multiple of WS_DEPTH = 2 (an odd walk runs a
dead pipeline step, an odd start swaps the LDS stage parity against the global step); the halo kernels split over the Cin / 32 channel chunks only.

1. THE EXACT LADDER (test_ladder, test_ladder_batched).  Integer data: x in [-3, 3] (with a +3 and a -3: the per-tensor fp16-pair scale is 2^13 and
   every low half is empty), weights in [-2, 2] (scale 2^13, bf16-exact too), an integer conv bias, no BatchNorm (epilogue scale 1), some rows an
   integer residual under relu 0 / 1 / 2.  Every product and every partial sum is then an integer below

       27 taps x 1024 channels x 3 x 2 = 165 888 < 2^24                                    (asserted per case, with the bias and the residual)

   so fp32 holds every intermediate exactly WHATEVER the order of the sum, and the output must equal the fp64 convolution bit for bit at every
   split count from 1 to min(32, K steps) (halo: min(32, Cin / 32)).  A K step dropped, run twice, or taken from the wrong tap or chunk changes
   integers.  (tests/test_splitk_ladder_cpu.py proves the premise on the CPU and pins the walks this file relies on.)  Per launch: torch.equal with
   the reference, the named tile's kernel in the asked arithmetic with (tile, splits) left alone by conv_tiles.resolve, in f16x2 an exact max |out|
   slot; the persistent tiles equal 128256's bits at the same split count; a halo launch asked for one split more than it has chunks runs the
   clamped count.  Batched (conv3d_ndhwc on (2, D, H, W, C): one ndet_conv_split_batch launch) once per family that takes a batch -- the
   persistent tiles do not: conv_tiles.resolve sends them to 128256 -- at splits 2, 5 and the cap.

2. THE PRODUCTION PAIRS ON REAL-VALUED DATA (test_production_pair_*).  The ladder says nothing about the low halves of the fp16 pairs or the reduce
   pass's rounding.  One row per (tile, splits > 1) pair that TUNED_F16, TUNED_SPLIT or TUNED_BF16 of conv_tuning.py name (PRODUCTION below; the
   CPU file holds it against the tables), on the edges file's data (post-ReLU-like inputs, per-voxel magnitudes over e^+-3, eval BatchNorm), at the
   smallest ragged shape whose K-step (halo: chunk) count is NOT a multiple of the split count; ReLU before the residual on the rows with
   splits >= 12.  The edges file's bars, imported: |got - ref| <= ELEM_BAR max(1, max|ref|) elementwise and rel-rms < RMS_BAR against the fp64
   convolution, an exact slot, the same bits from a second launch, the named kernel.  One bf16x3 row per family and the one-product bf16 (SCH 2)
   arithmetic on pairs TUNED_BF16 names (that file's bf16 bar: 2e-5 max|ref| against the convolution of the bf16-rounded operands).

Measured on an MI355X (elementwise error / max(1, max|ref|), rel-rms, the PRINTED ratio rel-rms(f16x2) / rel-rms(bf16x3) on the same tile and split):

    tile    splits  cin->cout   grid    kernel  relu res  walks     elem      rel-rms   f16x2/bf16x3      (walks: K steps; halo tiles: chunks)
    64         3    320->40     5x7x9   1x1x1   0    -   3 / 4     1.34e-07  1.53e-07  0.89
    64         4    64->40      3x4x5   3x3x3   1    y   13 / 14   1.84e-07  1.40e-07  0.82
    64         8    64->40      3x4x5   3x3x3   1    y   6 / 7     1.26e-07  1.15e-07  0.88
    64        12    64->40      3x4x5   3x3x3   2    y   4 / 5     1.75e-07  1.11e-07  1.01
    64        16    64->40      3x4x5   3x3x3   2    y   3 / 4     1.61e-07  9.91e-08  1.03
    64        32    64->40      3x4x5   3x3x3   2    y   1 / 2     1.48e-07  9.00e-08  1.02
    128        4    64->136     3x4x5   3x3x3   1    y   13 / 14   3.24e-07  1.64e-07  0.87
    128        6    96->136     3x4x5   3x3x3   0    -   13 / 14   2.62e-07  1.97e-07  0.84
    128       12    64->136     3x4x5   3x3x3   2    y   4 / 5     1.50e-07  8.31e-08  0.88
    128       16    64->136     3x4x5   3x3x3   2    y   3 / 4     1.45e-07  7.94e-08  0.97
    128       24    64->136     3x4x5   3x3x3   2    y   2 / 3     1.25e-07  7.59e-08  0.99
    12864      2    96->25      3x4x5   3x3x3   0    -   40 / 41   4.44e-07  3.25e-07  0.80
    12864      3    320->25     5x7x9   1x1x1   0    -   3 / 4     1.45e-07  1.41e-07  1.06
    12864      4    64->25      3x4x5   3x3x3   1    y   13 / 14   1.88e-07  1.34e-07  0.93
    12864      6    96->25      3x4x5   3x3x3   0    -   13 / 14   2.22e-07  2.17e-07  0.82
    128256     2    96->300     3x4x5   3x3x3   0    -   40 / 41   9.41e-07  3.11e-07  0.81
    128256     3    320->300    5x7x9   1x1x1   0    -   3 / 4     2.15e-07  1.37e-07  0.99
    128256     4    64->300     3x4x5   3x3x3   1    y   13 / 14   3.08e-07  1.47e-07  0.89
    128256     6    96->300     3x4x5   3x3x3   0    -   13 / 14   2.90e-07  2.16e-07  0.86
    128256     8    64->300     3x4x5   3x3x3   1    y   6 / 7     1.82e-07  1.23e-07  0.97
    128256    12    64->300     3x4x5   3x3x3   2    y   4 / 5     2.09e-07  7.80e-08  1.00
    128256    16    64->300     3x4x5   3x3x3   2    y   3 / 4     1.78e-07  7.54e-08  1.01
    128256    24    64->300     3x4x5   3x3x3   2    y   2 / 3     1.84e-07  7.40e-08  1.08
    129256    12    64->304     3x4x5   3x3x3   2    y   4 / 5     2.03e-07  9.51e-08  0.92
    129064     2    96->304     3x4x5   3x3x3   0    -   40 / 41   7.34e-07  3.16e-07  0.81
    129064     4    64->304     3x4x5   3x3x3   1    y   13 / 14   2.59e-07  1.07e-07  0.84
    129064     8    64->304     3x4x5   3x3x3   1    y   6 / 7     1.94e-07  8.69e-08  0.92
    129064    16    64->304     3x4x5   3x3x3   2    y   3 / 4     1.50e-07  8.83e-08  1.02
    129064    32    64->304     3x4x5   3x3x3   2    y   1 / 2     2.03e-07  8.76e-08  1.08
    3128       2    96->136     3x4x5   3x3x3   0    -   1 / 2     4.19e-07  3.04e-07  0.79
    3128       4    192->136    3x4x5   3x3x3   1    y   1 / 2     3.56e-07  2.23e-07  0.82
    3128       8    320->136    3x4x5   3x3x3   1    y   1 / 2     4.82e-07  1.82e-07  0.80
    3128      12    448->136    3x4x5   3x3x3   2    y   1 / 2     2.75e-07  1.65e-07  0.80
    3128      32    1056->136   2x5x6   3x3x3   2    y   1 / 2     2.20e-07  1.27e-07  0.88
    3256       2    96->300     3x4x5   3x3x3   0    -   1 / 2     7.65e-07  3.23e-07  0.79
    3256       3    160->300    3x4x5   3x3x3   0    -   1 / 2     4.78e-07  3.41e-07  0.83
    3256       4    192->300    3x4x5   3x3x3   1    y   1 / 2     3.86e-07  2.11e-07  0.81
    3256       8    320->300    3x4x5   3x3x3   1    y   1 / 2     3.39e-07  1.82e-07  0.83
    3257       2    96->300     3x4x5   3x3x3   0    -   1 / 2     7.65e-07  3.23e-07  0.79
    3257       4    192->300    3x4x5   3x3x3   1    y   1 / 2     3.86e-07  2.11e-07  0.81
    3258       2    96->300     3x4x5   3x3x3   0    -   1 / 2     7.65e-07  3.23e-07  0.79
    3258       8    320->300    3x4x5   3x3x3   1    y   1 / 2     3.39e-07  1.82e-07  0.83

bf16x3 rows: 128 x 24 1.33e-07 / 7.63e-08, 128256 x 16 2.05e-07 / 7.48e-08, 129064 x 32 2.19e-07 / 8.12e-08, 3128 x 32 2.12e-07 / 1.45e-07.  bf16 rows
(|got - ref(bf16 operands)| / max|ref|): 128 x 24 1.35e-07, 128256 x 4 1.89e-07, 3257 x 4 2.56e-07, 3128 x 32 3.17e-07.  The ratio passes 1 (up to 1.08) on
the rows with 12 and more splits, where the fp32 sum of the partials in the reduce pass, the same in both arithmetics, is most of the error; it is
printed, not asserted, as in the edges file.  The ladder: all 44 (tile, case, arithmetic) rows and the six batched ones equal the fp64 result at every
split count.  The library took every pair: no row is replaced by a rejection.
"""
import copy
import functools

import pytest
import torch
from torch import nn

from nerfdet_amd import conv_tiles
from test_conv_batch_gpu import _run
from test_f16x2_edges_gpu import ELEM_BAR, RMS_BAR, _Case, _case, _errors, _launch, _ran, _slot_is_exact

pytestmark = pytest.mark.gpu

MAX_SPLITS = 32                     # conv3d.choose_tiling_split hands out nothing above
EXACT_BELOW = 1 << 24               # integers of smaller magnitude are exact in fp32
TILE_IDS = conv_tiles.ids("unified", "ws", "wsp", "halo")


def walks(n, splits):
    """Per-split walk lengths of ``n`` K steps (halo: channel chunks) over ``splits``: it_end - it_begin of the kernels."""
    return [n * (s + 1) // splits - n * s // splits for s in range(splits)]


def starts(n, splits):
    return [n * s // splits for s in range(splits)]


# ---- 1. the exact ladder ----
LADDER = {
    # name: Cin, Cout, grid (M = 60 or 315 rows, 120 voxels for the long halo walk: never a tile multiple), kernel, relu, residual
    "k27c96-cout40": (96, 40, (3, 4, 5), 3, 2, 1),          # 81 K steps: 32 splits walk 2 / 3 steps, 24 walk 3 / 4; ragged Cout on the unified tiles
    "k1c1024-cout64": (1024, 64, (5, 7, 9), 1, 1, 1),       # 32 K steps: 32 splits of ONE step; five / three row tiles
    "k27c96-cout300": (96, 300, (3, 4, 5), 3, 2, 1),        # ragged Cout past one 256-column tile
    "k27c96-cout304": (96, 304, (3, 4, 5), 3, 2, 1),        # ... in the form the persistent tiles take (Cout % 16 == 0)
    "k1c1024-cout256": (1024, 256, (5, 7, 9), 1, 0, 0),
    "k27c1024-cout72": (1024, 72, (4, 5, 6), 3, 1, 1),      # halo: 32 chunks, 32 splits of ONE chunk; the largest K of the file
    "k27c320-cout300": (320, 300, (3, 4, 5), 3, 2, 1),      # halo: 10 chunks, 4 splits walk 2 / 3 chunks, 8 walk 1 / 2; ragged Cout
}
FAMILY_CASES = {
    "unified": ("k27c96-cout40", "k1c1024-cout64"),
    "ws": ("k27c96-cout300", "k1c1024-cout256"),
    "wsp": ("k27c96-cout304", "k1c1024-cout256"),
    "halo": ("k27c1024-cout72", "k27c320-cout300"),
}
LADDER_ROWS = [(t, name) for t in TILE_IDS for name in FAMILY_CASES[conv_tiles.TILES[t].family]]
BATCHED = {"unified": (64, "k27c96-cout40"), "ws": (128256, "k27c96-cout300"), "halo": (3256, "k27c320-cout300")}


def ladder_ksteps(name):
    cin, _, _, k, _, _ = LADDER[name]
    return k ** 3 * cin // 32


def ladder_units(tile, name):
    """What the tile splits: the channel chunks on the halo tiles, the K steps (chunk outermost, taps innermost) on the others."""
    return LADDER[name][0] // 32 if conv_tiles.TILES[tile].family == "halo" else ladder_ksteps(name)


def ladder_cap(tile, name):
    return min(MAX_SPLITS, ladder_units(tile, name))


class _IntCase(_Case):
    """One bias-only 3D layer on integer data (see 1. above) with its fp64 result.  ``volume`` > 0: the same layer on other data (the further
    volumes of a batch)."""

    def __init__(self, name, volume=0):
        cin, cout, grid, k, relu, res = LADDER[name]
        seed = 7919 * sorted(LADDER).index(name)
        gw, gx = torch.Generator().manual_seed(seed), torch.Generator().manual_seed(seed + 1 + volume)
        self.dim, self.relu, self.mode, self.bn = 3, relu, "conv", None
        self.conv = nn.Conv3d(cin, cout, k, 1, k // 2, bias=True)
        with torch.no_grad():
            self.conv.weight.copy_(torch.randint(-2, 3, tuple(self.conv.weight.shape), generator=gw).float())
            self.conv.bias.copy_(torch.randint(-5, 6, (cout,), generator=gw).float())
        self.x = torch.randint(-3, 4, (*grid, cin), generator=gx).float()
        self.x[0, 0, 0, 0], self.x[-1, -1, -1, -1] = 3.0, -3.0
        self.res = torch.randint(-4, 5, (*grid, cout), generator=gx).float() if res else None
        # the largest magnitude any partial sum, and the output through bias and residual, can reach
        self.bound = k ** 3 * cin * 3 * 2 + 5 + (4 if res else 0)
        self.ref = self.forward(torch.float64)


@functools.lru_cache(maxsize=None)
def _int_case(name, volume=0):
    return _IntCase(name, volume)


def _exact_ref(case, device):
    ref = case.ref.float()
    assert case.bound < EXACT_BELOW and float(case.ref.abs().max()) <= case.bound and torch.equal(ref.double(), case.ref)
    return ref.to(device)


def _differs(got, ref):
    return int((got != ref).sum()), float((got - ref).abs().max())


@pytest.mark.parametrize("arith", ["f16x2", "bf16x3"])
@pytest.mark.parametrize("tile,name", LADDER_ROWS, ids=[f"{t}-{n}" for t, n in LADDER_ROWS])
def test_ladder(device, tile, name, arith):
    from nerfdet_amd import conv3d as C
    family = conv_tiles.TILES[tile].family
    case = _int_case(name)
    ref = _exact_ref(case, device)
    assert ladder_ksteps(name) >= C.F16_MIN_KSTEPS, "too few K steps: the f16x2 row would run the bf16x3 kernel"
    suffix = "/f16x2" if arith == "f16x2" else ""
    cap = ladder_cap(tile, name)
    wrong = []            # (splits, differing elements, max |difference|): every split count is run before the verdict
    for splits in range(1, cap + 1):
        got, names, resolved = _launch(device, case, arith, tile, splits, direct=False)
        _ran(names, resolved, tile, splits, suffix)
        if not torch.equal(got, ref):
            wrong.append((splits,) + _differs(got, ref))
        if arith == "f16x2":
            _slot_is_exact(got)
        if family == "wsp":
            one_shot, names, resolved = _launch(device, case, arith, 128256, splits, direct=False)
            _ran(names, resolved, 128256, splits, suffix)
            assert torch.equal(got, one_shot), f"splits {splits}: the persistent tile must reproduce the one-shot tile bit for bit"
    if family == "halo" and cap < MAX_SPLITS:         # one split more than there are chunks: the clamped count runs
        got, names, resolved = _launch(device, case, arith, tile, cap + 1, direct=False)
        _ran(names, resolved, tile, cap, suffix)
        if not torch.equal(got, ref):
            wrong.append((cap + 1,) + _differs(got, ref))
    print(f"LADDER {tile} {name} {arith}: splits 1..{cap} over {ladder_units(tile, name)} {'chunks' if family == 'halo' else 'K steps'}, wrong at {wrong}")
    assert not wrong, f"(splits, differing elements, max |got - ref|) on exact integer data: {wrong}"


@pytest.mark.parametrize("arith", ["f16x2", "bf16x3"])
@pytest.mark.parametrize("family", sorted(BATCHED))
def test_ladder_batched(device, family, arith):
    """The same rows through the batched entry: two volumes of different data, one launch, the 64- and 128-row tiles straddling the volume boundary
    at row 60."""
    from nerfdet_amd import conv3d as C
    tile, name = BATCHED[family]
    vols = [_int_case(name, v) for v in range(2)]
    ref = torch.stack([_exact_ref(c, device) for c in vols])
    _, pk, _ = vols[0].on(device)
    x = torch.stack([c.x for c in vols]).to(device)
    res = None if vols[0].res is None else torch.stack([c.res for c in vols]).to(device)
    want = conv_tiles.TILES[tile].name + ("/f16x2" if arith == "f16x2" else "") + "/batch"
    cap = ladder_cap(tile, name)
    for splits in (2, 5, cap):
        got, names, resolved = _run(device, arith, tile, splits, lambda: C.conv3d_ndhwc(x, pk, residual=res, relu=vols[0].relu, splits=splits, tile=tile))
        assert names == [want] and resolved == [(tile, splits)], (names, resolved)
        assert torch.equal(got, ref), (splits,) + _differs(got, ref)
        if arith == "f16x2":
            _slot_is_exact(got)


# ---- 2. the production pairs on real-valued data ----
PRODUCTION = {
    # tile: the split counts > 1 that TUNED_F16, TUNED_SPLIT and TUNED_BF16 choose for it (tests/test_splitk_ladder_cpu.py reads the tables)
    64: (3, 4, 8, 12, 16, 32),
    128: (4, 6, 12, 16, 24),
    12864: (2, 3, 4, 6),
    128256: (2, 3, 4, 6, 8, 12, 16, 24),
    129256: (12,),
    129064: (2, 4, 8, 16, 32),
    3128: (2, 4, 8, 12, 32),
    3256: (2, 3, 4, 8),
    3257: (2, 4),
    3258: (2, 8),
}
PRODUCTION_ROWS = [(t, s) for t, ss in PRODUCTION.items() for s in ss]
BF16X3_ROWS = [(128, 24), (128256, 16), (129064, 32), (3128, 32)]       # one per family, the longest sum of partials it has
BF16_ROWS = [(128, 24), (128256, 4), (3257, 4), (3128, 32)]             # pairs TUNED_BF16 names (it has none on a persistent tile)
PRODUCTION_COUT = {64: 40, 128: 136, 12864: 25, 128256: 300, 129256: 304, 129257: 304, 129064: 304, 3128: 136, 3256: 300, 3257: 300, 3258: 300}


def production_shape(tile, splits):
    """(Cin, Cout, grid, kernel, relu, residual) of the row of one pair: the smallest ragged shape whose K-step count (halo: chunk count) is no multiple
    of ``splits``.  3x3x3 on 60 voxels with 54 or 81 K steps; 27 c is always a multiple of 3, so three splits take a 1x1x1 layer of 10 steps on 315."""
    if conv_tiles.TILES[tile].family == "halo":
        cin = 32 * {2: 3, 3: 5, 4: 6, 8: 10, 12: 14, 32: 33}[splits]
        k, grid = 3, (2, 5, 6) if splits == 32 else (3, 4, 5)
    elif splits == 3:
        cin, k, grid = 320, 1, (5, 7, 9)
    else:
        cin, k, grid = (96 if splits in (2, 6) else 64), 3, (3, 4, 5)
    relu, res = (2, 1) if splits >= 12 else ((1, 1) if splits in (4, 8) else (0, 0))
    return cin, PRODUCTION_COUT[tile], grid, k, relu, res


def production_units(tile, splits):
    cin, _, _, k, _, _ = production_shape(tile, splits)
    return cin // 32 if conv_tiles.TILES[tile].family == "halo" else k ** 3 * cin // 32


# what this file covers, for the CPU file's check against the tables: the ladder (every count up to its cap) and the rows
LADDER_PAIRS = frozenset((t, s) for t, name in LADDER_ROWS for s in range(1, ladder_cap(t, name) + 1))
ROW_PAIRS = frozenset(PRODUCTION_ROWS)
COVERED = LADDER_PAIRS | ROW_PAIRS


def _production_case(tile, splits):
    from nerfdet_amd import conv3d as C
    cin, cout, grid, k, relu, res = production_shape(tile, splits)
    units = production_units(tile, splits)
    assert units >= splits and units % splits, "the row must cut its K walk unevenly"
    assert k ** 3 * cin // 32 >= C.F16_MIN_KSTEPS, "too few K steps: the row would run the bf16x3 kernel"
    return _case(3, cin, cout, grid, k, 1, "conv", relu, res, False), f"{cin}->{cout} {'x'.join(map(str, grid))} k{k} relu{relu} res{res}"


@pytest.mark.parametrize("tile,splits", PRODUCTION_ROWS)
def test_production_pair_row(device, tile, splits):
    case, what = _production_case(tile, splits)
    got, names, resolved = _launch(device, case, "f16x2", tile, splits, direct=False)
    _ran(names, resolved, tile, splits, "/f16x2")
    _slot_is_exact(got)
    elem, rms = _errors(got, case.ref)
    again, _, _ = _launch(device, case, "f16x2", tile, splits, direct=False)
    assert torch.equal(got, again), "the same launch twice: split-K is a fixed-order sum"
    ref3, names, _ = _launch(device, case, "bf16x3", tile, splits, direct=False)
    assert names == [conv_tiles.TILES[tile].name]
    elem3, rms3 = _errors(ref3, case.ref)
    print(f"PAIR {tile} x {splits} ({what}, walks {sorted(set(walks(production_units(tile, splits), splits)))}): elem {elem:.2e} rel-rms {rms:.2e} | "
          f"bf16x3 elem {elem3:.2e} rel-rms {rms3:.2e} | f16x2/bf16x3 {rms / rms3:.2f}")
    assert elem <= ELEM_BAR and rms < RMS_BAR, (elem, rms)


@pytest.mark.parametrize("tile,splits", BF16X3_ROWS)
def test_production_pair_row_bf16x3(device, tile, splits):
    case, what = _production_case(tile, splits)
    got, names, resolved = _launch(device, case, "bf16x3", tile, splits, direct=False)
    _ran(names, resolved, tile, splits, "")
    elem, rms = _errors(got, case.ref)
    again, _, _ = _launch(device, case, "bf16x3", tile, splits, direct=False)
    assert torch.equal(got, again), "the same launch twice: split-K is a fixed-order sum"
    print(f"PAIR-BF16X3 {tile} x {splits} ({what}): elem {elem:.2e} rel-rms {rms:.2e}")
    assert elem <= ELEM_BAR and rms < RMS_BAR, (elem, rms)


@pytest.mark.parametrize("tile,splits", BF16_ROWS)
def test_production_pair_row_bf16(device, tile, splits):
    """set_arithmetic("bf16") (SCH 2), as tests/test_f16x2_edges_gpu.py::test_bf16_edge_row states it: the convolution of the bf16-ROUNDED operands
    accumulated in fp32 -- within 2e-5 max|ref| of PyTorch-CPU fp32 on operands rounded the same way, at least 1e-4 max|ref| from the unrounded one."""
    case, what = _production_case(tile, splits)
    rounded = copy.deepcopy(case.conv)
    with torch.no_grad():
        rounded.weight.copy_(rounded.weight.bfloat16().float())
    ref = case.forward(torch.float32, conv=rounded, x=case.x.bfloat16().float())
    full = case.forward(torch.float32)
    got, names, resolved = _launch(device, case, "bf16", tile, splits, direct=False)
    _ran(names, resolved, tile, splits, "")
    again, _, _ = _launch(device, case, "bf16", tile, splits, direct=False)
    assert torch.equal(got, again)
    scale = float(ref.abs().max())
    err = float((got.cpu() - ref).abs().max())
    print(f"PAIR-BF16 {tile} x {splits} ({what}): |got - ref(bf16 operands)| {err / scale:.2e} max|ref|")
    assert err <= 2e-5 * scale
    assert float((got.cpu() - full).abs().max()) >= 1e-4 * scale
