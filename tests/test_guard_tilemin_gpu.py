"""Word 1 of the amax slot -- the smallest non-zero TILE maximum, the range guard's second condition (csrc/conv_common.hpp::conv_guard_check,
conv_amax_commit; DESIGN.md "range guard") -- read back with conv3d.tilemin_value on every kernel that commits it, and the guard of every kernel
family that reads it.  A producer that records the wrong minimum leaves its own output correct and disarms the guard of the layer AFTER it, so the
rows here look at the word itself and at the hand-off.

Every row runs in the fp16-pair arithmetic with a zero BatchNorm shift and ReLU (positive-homogeneous: an input region scaled by 2^-30 gives outputs
scaled by 2^-30), against an fp64 evaluation of the same modules on the CPU at the bars of tests/test_f16x2_edges_gpu.py.  An input has a bright part
(standard normal / U[0,1)) and a dim region (the same values x 2^-30) that holds at least one whole tile for any tile alignment; the fp64 result says
that the region's outputs lie below 2^-16 of the tensor's maximum.

Producer rows (unified 64 / 128 / 12864 staged and direct, wave-specialised 128256, halo 3128 / 3256 in 2D and 3D, the k2 s2 transposed form, the
split-K reduce, the batched form, the chained kernel, the BatchNorm apply, the ReLU-affine backward, the stem at three persistent iterations, and the
persistent tiles 129064 / 129256 / 129257 at more tiles than compute units):
 (a) kernels whose tile is a stated block (conv_tiles.TILES rows x columns; 3 x 8 pooled pixels x 64 channels of one image for the stem):
     tilemin_value == min over tiles of max |got|, non-zero tiles only -- both sides from the GPU output: bit equality;
 (b) elsewhere: smallest non-zero maximum of the aligned 16-row x 16-channel blocks of got <= tilemin_value <= max |got[dim region]|;
 (c) the same input without its dim region, x 3e7: tilemin_value >= 2^-16 amax_value (a launch that recorded nothing, or element minima, fails);
 (d) a consumer convolution on the producer's output, reading the producer's slot (amax_fallbacks unchanged): guard_tripped with the input scaled so
     that the consumer's floor is 4 GUARD_TOL, clear for the uniform twin and clear at GUARD_TOL / 4.
Consumer rows: the slot comes from ndet_amax_f32 and (d) is repeated with the guarded launch on every family that calls conv_guard_check.
Structure smaller than a tile (VERDICT.md "What's weak" item 2): a dark pixel / a dark 5 x 5 block inside a bright tensor whose maximum is 1e9 --
bf16x3 inside 1e-4 max(1, |ref|), f16x2 inside the bound of conv_common.hpp:62-66 and more than 10x further out than bf16x3; the guard's word is
printed, not asserted; the same dark region grown to whole tiles must trip.

The persistent rows take M = BM (2 n_cu + 37) - 43 / BM (n_cu + 19) - 43 rows: the stated number of row tiles with a ragged last one.

Measured on an MI355X (n_cu 256):
    producer                      elem      rel-rms    amax       word 1     expected (a) / bounds (b)     twin word 1 / amax
    unified64 staged              4.71e-07  3.48e-07   2.926e+00  2.288e-09  = 2.288e-09                   0.677
    unified64 direct              8.19e-07  3.47e-07   3.010e+00  2.408e-09  = 2.408e-09                   0.609
    unified128 staged             8.19e-07  3.47e-07   3.010e+00  2.775e-09  = 2.775e-09                   0.769
    unified128 direct             6.58e-07  3.46e-07   2.799e+00  2.499e-09  = 2.499e-09                   0.710
    unified12864 staged, direct   8.19e-07  3.47e-07   3.010e+00  2.608e-09  = 2.608e-09                   0.748
    ws128256                      5.73e-07  3.43e-07   2.799e+00  3.010e-09  = 3.010e-09                   0.748
    halo3128 3D                   1.06e-06  3.46e-07   3.010e+00  2.775e-09  [1.121e-09, 3.033e-09]        0.868
    halo3256 3D                   5.73e-07  3.43e-07   2.799e+00  3.010e-09  [9.127e-10, 3.524e-09]        0.748
    halo3128 2D                   4.63e-07  2.65e-07   3.869e+00  2.634e-09  [7.415e-10, 3.879e-09]        0.681
    halo3256 2D                   4.68e-07  2.68e-07   4.694e+00  3.190e-09  [9.099e-10, 3.805e-09]        0.684
    transposed 64                 3.74e-07  1.52e-07   1.911e+00  1.098e-09  [5.801e-10, 2.026e-09]        0.543
    transposed 128256             2.42e-07  1.49e-07   1.100e+00  7.380e-10  [2.736e-10, 9.874e-10]        0.560
    splits 2, 64                  3.50e-07  2.52e-07   3.010e+00  1.490e-09  [1.121e-09, 3.033e-09]        0.453
    splits 2, 128256              3.82e-07  2.52e-07   2.799e+00  1.555e-09  [9.127e-10, 3.524e-09]        0.321
    batch unified128 / halo3128   9.26e-07  4.26e-07   3.333e+00  2.346e-09  [1.054e-09, 3.338e-09]        0.702
    chain <64>                    3.94e-07  3.11e-07   1.280e+00  1.001e-09  [2.484e-10, 1.421e-09]        0.657
    bn_rows apply                 1.33e-07  5.90e-08   4.796e+00  1.806e-08  [6.834e-09, 1.911e-08]        0.795
    relu_affine_bwd               4.02e-08  2.54e-08   5.871e+00  3.540e-09  [2.021e-09, 4.851e-09]        0.613
    stem, images 7 and 30 dim     3.26e-07  1.43e-07   4.647e+00  1.809e-09  = 1.809e-09                   0.367
    stem, image 19 dim            3.26e-07  1.43e-07   4.647e+00  1.723e-09  = 1.723e-09                   0.367
    stem bf16x3 + slot, image 19  4.79e-07  1.73e-07   4.647e+00  1.723e-09  = 1.723e-09                   0.367
    129064 cout 32, M 35093       3.25e-07  1.50e-07   1.637e+00  1.008e-09  = 1.008e-09                   0.595
    129064 cout 512, M 17557      2.97e-07  1.45e-07   2.319e+00  1.526e-09  = 1.526e-09                   0.649
    129256 / 129257 cout 32, M 70229   2.67e-07  1.37e-07   2.142e+00  1.352e-09  = 1.352e-09              0.595
    129256 / 129257 cout 512, M 35157  2.72e-07  1.42e-07   2.532e+00  1.557e-09  = 1.557e-09              0.653

Before the persistent kernels kept a minimum per tile (one value per workgroup for all the tiles of its walk) the stem rows read word 1 = 1.969 / 1.973
and the six persistent rows 1.058 ... 1.734 -- a bright tile's maximum -- and the consumer behind them stayed clear at a floor of 4 GUARD_TOL.
Every hand-off (d) and every consumer row: tripped at 4 GUARD_TOL, clear at GUARD_TOL / 4, clear for the uniform twin.

    structure smaller than a tile   max|ref| dark   bf16x3 err   f16x2 err   f16x2 err / bound   f16x2 / bf16x3   guard
    1x1, dark pixel                 6.679e-01       9.98e-08     8.50e-04    0.087               8516             clear
    1x1, dark 5x5 block             9.238e-01       3.07e-07     1.45e-03    0.113               4733             clear
    3x3, dark 5x5 block             1.050e+00       7.82e-07     1.17e-03    0.028               1498             clear
"""
import copy
import ctypes
import functools
from ctypes import c_void_p

import pytest
import torch
from torch import nn

from test_conv_batch_gpu import _run
from test_f16x2_edges_gpu import ELEM_BAR, RMS_BAR, _errors, _forward
from test_stem_gpu import LOOP3, TPX, TPY, _ref64, _Stem, _tiles

pytestmark = pytest.mark.gpu

DIM = 2.0 ** -30            # the dim region's factor
WINDOW = 2.0 ** -16         # the fp16-pair window below the tensor's maximum (conv_guard_check's condition 2)
TWIN = 3.0e7                # the uniformly bright twin's factor


# ---------------------------------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _zero_shift_bn(dim, c):
    bn = (nn.BatchNorm2d if dim == 2 else nn.BatchNorm3d)(c).eval()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5); bn.running_var.uniform_(0.5, 1.5); bn.running_mean.zero_(); bn.bias.zero_()
    return bn


def _block_max(got2d, rows, cols):
    """max |got| of the aligned rows x cols blocks of an (M, C) tensor (ragged edges: what is there), as an (M / rows, C / cols) tensor."""
    m, c = got2d.shape
    mt, ct = -(-m // rows), -(-c // cols)
    pad = torch.zeros(mt * rows, ct * cols, dtype=got2d.dtype)
    pad[:m, :c] = got2d.abs()
    return pad.view(mt, rows, ct, cols).amax((1, 3))


def _min_nonzero(t):
    return float(t[t > 0].min())


def _band_max(t2d, bands):
    return max(float(t2d[a:b].abs().max()) for a, b in bands)


class _Layer:
    """relu(bn0(conv(x))) with a zero BatchNorm shift on the CPU: the bright input, the input with its dim rows, the fp64 result, and the bands of
    flattened OUTPUT rows that see dim inputs only.  ``in_bands`` / ``out_bands``: [a, b) over the rows of x.view(-1, Cin) / out.view(-1, Cout)."""

    def __init__(self, dim, cin, cout, grid, k, mode, in_bands, out_bands, xkind="randn", batch=False):
        torch.manual_seed(7 * cin + cout + 13 * k + sum(grid) + dim)
        self.dim, self.mode, self.batch, self.cout = dim, mode, batch, cout
        if mode == "tr":
            self.conv = nn.ConvTranspose3d(cin, cout, 2, 2, bias=False)
        else:
            self.conv = (nn.Conv2d if dim == 2 else nn.Conv3d)(cin, cout, k, 1, k // 2, bias=False)
        self.bn = _zero_shift_bn(dim, cout)
        self.bright = torch.randn(*grid, cin) if xkind == "randn" else torch.rand(*grid, cin)
        self.x = self.bright.clone()
        for a, b in in_bands:
            self.x.view(-1, cin)[a:b] *= DIM
        self.out_bands = out_bands
        self.ref = self.fp64(self.x)
        ref2d = self.ref.view(-1, cout)
        assert _band_max(ref2d, out_bands) < WINDOW * float(self.ref.abs().max()), "the dim region's outputs are not below the window"
        assert _band_max(ref2d, out_bands) > 0.0

    def fp64(self, x):
        conv, bn = copy.deepcopy(self.conv).double(), copy.deepcopy(self.bn).double()
        with torch.no_grad():
            if self.batch:
                return torch.stack([_forward(conv, bn, v.double(), 3, 1, None) for v in x])
            return _forward(conv, bn, x.double(), self.dim, 1, None)

    def pack(self, device):
        from nerfdet_amd import conv3d as C
        if not hasattr(self, "_pk"):
            conv_d, bn_d = copy.deepcopy(self.conv).to(device), copy.deepcopy(self.bn).to(device)
            self._pk = (conv_d, bn_d, C.packed([conv_d], bn_d))
            assert float(self._pk[2].shift.abs().max()) == 0.0, "the folded shift must be exactly 0"
        return self._pk[2]


@functools.lru_cache(maxsize=None)
def _conv_case(kind):
    """The shared layers of the producer and consumer rows, built (with their fp64 results) once."""
    if kind == "3d":            # 16 x 8 x 8 voxels, 3x3x3: dim input planes 2..14, outputs of planes 3..13 see dim inputs only (640 rows: five 128-row tiles)
        return _Layer(3, 64, 128, (16, 8, 8), 3, "conv", [(2 * 64, 14 * 64)], [(3 * 64, 13 * 64)])
    if kind == "3d-64":         # the same grid into 64 channels (12864 and the staged 64)
        return _Layer(3, 64, 64, (16, 8, 8), 3, "conv", [(2 * 64, 14 * 64)], [(3 * 64, 13 * 64)])
    if kind == "3d-256":        # ... and into 256 (wave-specialised, halo 3256): two column tiles of the 128-column kernels
        return _Layer(3, 64, 256, (16, 8, 8), 3, "conv", [(2 * 64, 14 * 64)], [(3 * 64, 13 * 64)])
    if kind == "2d-256":        # 8 images of 16 x 16, 3x3: images 2..6 dim (1024 rows)
        return _Layer(2, 64, 256, (8, 16, 16), 3, "conv", [(2 * 256, 6 * 256)], [(2 * 256, 6 * 256)])
    if kind == "2d-128":
        return _Layer(2, 64, 128, (8, 16, 16), 3, "conv", [(2 * 256, 6 * 256)], [(2 * 256, 6 * 256)])
    if kind == "tr-64":         # k2 s2 transposed, 12 x 6 x 6 -> 24 x 12 x 12: input planes 2..10 dim (288 GEMM rows: a whole 128-row tile) = output planes 4..20
        return _Layer(3, 128, 64, (12, 6, 6), 2, "tr", [(2 * 36, 10 * 36)], [(4 * 144, 20 * 144)])
    if kind == "tr-256":
        return _Layer(3, 128, 256, (12, 6, 6), 2, "tr", [(2 * 36, 10 * 36)], [(4 * 144, 20 * 144)])
    if kind == "batch":         # three volumes of 6 x 8 x 8 (384 rows each, three 128-row tiles), the middle one dim
        return _Layer(3, 64, 128, (3, 6, 8, 8), 3, "conv", [(384, 768)], [(384, 768)], batch=True)
    raise KeyError(kind)


def _expect_name(tile, batch=False):
    from nerfdet_amd import conv_tiles
    return conv_tiles.TILES[tile].name + "/f16x2" + ("/batch" if batch else "")


def _conv_runner(device, layer, tile, splits, direct):
    """run(x_cpu) -> the launch's output, after asserting that the named tile's fp16-pair kernel ran."""
    from nerfdet_amd import conv3d as C, conv_tiles
    pk = layer.pack(device)
    want_tile = conv_tiles.TILES[tile].partner if direct else tile

    def run(x):
        xd = x.to(device)
        prev = C.DIRECT_EPILOGUE
        try:
            C.DIRECT_EPILOGUE = direct
            fn = (lambda: C.conv2d_nhwc(xd, pk, relu=1, splits=splits, tile=tile)) if layer.dim == 2 else \
                (lambda: C.conv3d_ndhwc(xd, pk, relu=1, splits=splits, tile=tile))
            y, names, resolved = _run(device, "f16x2", tile, splits, fn)
        finally:
            C.DIRECT_EPILOGUE = prev
        assert names == [_expect_name(tile, layer.batch)] and resolved == [(want_tile, splits)], (names, resolved)
        return y
    return run


@functools.lru_cache(maxsize=None)
def _consumer(cin):
    """The guarded consumer of the hand-off: a 3x3 convolution (9 cin / 32 K steps) over the producer's rows as one 1 x M map."""
    torch.manual_seed(100 + cin)
    conv = nn.Conv2d(cin, 32, 3, 1, 1, bias=False)
    return conv, _zero_shift_bn(2, 32)


def _consume(device, y, pkc):
    """The consumer on ``y`` under a fresh guard word: (tripped, did it read y's own slot)."""
    from nerfdet_amd import conv3d as C
    rows = C.carry_amax(y, y.view(1, 1, -1, y.shape[-1]))
    before = C.amax_fallbacks
    prev = C.set_arithmetic("f16x2")
    try:
        C.guard_begin(device)
        with torch.no_grad():
            C.conv2d_nhwc(rows, pkc, relu=1)
        tripped = C.guard_tripped(device)
    finally:
        C.set_arithmetic(prev)
    return tripped, C.amax_fallbacks == before


def _check_producer(device, tag, run, x, bright, ref, out_bands, cout, exact=None, scaled=None):
    """(a)-(d) of the module docstring for one producer.  ``run(x_cpu)`` launches it; ``exact(got)``: the tile maxima of a kernel whose tile is a stated
    block, else None (bounds).  ``scaled(x, s)``: the input that scales the OUTPUT by s (default x * s)."""
    from nerfdet_amd import conv3d as C
    scaled = scaled or (lambda v, s: v * s)
    y = run(x)
    elem, rms = _errors(y, ref)
    got2d = y.detach().cpu().reshape(-1, cout)
    slot = y._ndet_amax
    amax, tmin = C.amax_value(slot), C.tilemin_value(slot)
    assert amax == float(got2d.abs().max()), "the launch's max |out| slot is not the tensor's maximum"
    dim_max = _band_max(got2d, out_bands)
    fine = _min_nonzero(_block_max(got2d, 16, 16))
    want = _min_nonzero(exact(y.detach().cpu())) if exact is not None else None
    yu = run(scaled(bright, TWIN))
    amax_u, tmin_u = C.amax_value(yu._ndet_amax), C.tilemin_value(yu._ndet_amax)
    print(f"TILEMIN {tag}: elem {elem:.2e} rel-rms {rms:.2e} | amax {amax:.3e} tilemin {tmin:.3e} "
          f"{'exact ' + format(want, '.3e') if want is not None else 'bounds [' + format(fine, '.3e') + ', ' + format(dim_max, '.3e') + ']'} "
          f"| twin tilemin/amax {tmin_u / amax_u:.3e}")
    assert elem <= ELEM_BAR and rms < RMS_BAR, (elem, rms)
    wrong = []              # every statement about word 1 is looked at before the row fails: a wrong minimum shows in (a) / (b) AND in the hand-off
    if exact is not None and tmin != want:
        wrong.append(f"(a) word 1 is {tmin!r}, the smallest non-zero tile maximum of the output is {want!r}")
    if not fine <= tmin <= dim_max:
        wrong.append(f"(b) word 1 {tmin!r} outside [{fine!r}, {dim_max!r}]")
    if not tmin_u >= WINDOW * amax_u:
        wrong.append(f"(c) uniform twin: word 1 {tmin_u!r} below 2^-16 of {amax_u!r}")
    # (d) the hand-off
    conv_c, bn_c = _consumer(cout)
    with torch.no_grad():
        pkc = C.packed([copy.deepcopy(conv_c).to(device)], copy.deepcopy(bn_c).to(device))
    l1 = C.guard_l1(pkc)
    assert amax_u * l1 * 2.0 ** -39 > C.GUARD_TOL, "the twin's floor must be above the tolerance: only condition 2 may hold the guard back"
    tripped, own = _consume(device, yu, pkc)
    if not own or tripped:
        wrong.append(f"(d) uniform twin: tripped {tripped}, read the producer's slot {own}")
    for factor, want_trip in ((4.0, True), (0.25, False)):
        s = factor * C.GUARD_TOL * 2.0 ** 39 / (l1 * amax)
        tripped, own = _consume(device, run(scaled(x, s)), pkc)
        if not own:
            wrong.append("(d) the consumer took a pass of its own over the producer's output")
        if tripped != want_trip:
            wrong.append(f"(d) floor {factor} x GUARD_TOL: guard_tripped is {tripped}")
    assert not wrong, "; ".join(wrong)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1. producers: the convolution families
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _exact_blocks(tile):
    from nerfdet_amd import conv_tiles
    row = conv_tiles.TILES[tile]
    return lambda got: _block_max(got.reshape(-1, got.shape[-1]), row.rows, row.cols)


CONV_PRODUCERS = [
    # id, case, tile, splits, direct epilogue, (a) exact
    ("unified64-staged", "3d-64", 64, 1, False, True),            # 16 row tiles x 1 column tile
    ("unified64-direct", "3d", 64, 1, True, True),                # 16 x 2
    ("unified128-staged", "3d", 128, 1, False, True),             # 8 x 1
    ("unified128-direct", "3d-256", 128, 1, True, True),          # 8 x 2
    ("unified12864-staged", "3d", 12864, 1, False, True),         # 8 x 2
    ("unified12864-direct", "3d", 12864, 1, True, True),
    ("ws128256", "3d-256", 128256, 1, False, True),
    ("halo3128-3d", "3d", 3128, 1, False, False),
    ("halo3256-3d", "3d-256", 3256, 1, False, False),
    ("halo3128-2d", "2d-128", 3128, 1, False, False),
    ("halo3256-2d", "2d-256", 3256, 1, False, False),
    ("tr-64", "tr-64", 64, 1, False, False),
    ("tr-128256", "tr-256", 128256, 1, False, False),
    ("splitk2-64", "3d", 64, 2, False, False),                    # the reduce pass commits
    ("splitk2-128256", "3d-256", 128256, 2, False, False),
    ("batch-unified128", "batch", 128, 1, False, False),
    ("batch-halo3128", "batch", 3128, 1, False, False),
]


@pytest.mark.parametrize("tag,kind,tile,splits,direct,exact", CONV_PRODUCERS, ids=[r[0] for r in CONV_PRODUCERS])
def test_producer_records_its_smallest_tile_maximum(device, tag, kind, tile, splits, direct, exact):
    from nerfdet_amd import _lib, conv_tiles
    layer = _conv_case(kind)
    if conv_tiles.TILES[tile].family == "halo":       # the dim region must hold a whole patch wherever the patches start
        g = layer.x.shape[1:4] if layer.batch else layer.x.shape[:3]
        patch, looped = (ctypes.c_int * 3)(), ctypes.c_int()
        k3 = (ctypes.c_int * 3)(*((1, 3, 3) if layer.dim == 2 else (3, 3, 3)))
        _lib.check(_lib.load().ndet_conv_halo_patch(tile, g[0], g[1], g[2], k3, patch, ctypes.byref(looped)), "conv_halo_patch")
        plane = g[1] * g[2]
        a, b = layer.out_bands[0]
        planes = (b - a) // plane
        assert planes == g[0] or planes >= 2 * patch[0] - 1, (tuple(patch), planes)
    run = _conv_runner(device, layer, tile, splits, direct)
    _check_producer(device, tag, run, layer.x, layer.bright, layer.ref, layer.out_bands, layer.cout, exact=_exact_blocks(tile) if exact else None)


@functools.lru_cache(maxsize=None)
def _chain_case():
    """conv2 (3x3, 64 -> 64) -> conv3 (1x1, 64 -> 256) of a bottleneck, zero shifts: 8 images of 16 x 16, images 2..6 dim."""
    torch.manual_seed(21)
    c2, b2 = nn.Conv2d(64, 64, 3, 1, 1, bias=False), _zero_shift_bn(2, 64)
    c3, b3 = nn.Conv2d(64, 256, 1, bias=False), _zero_shift_bn(2, 256)
    bright = torch.relu(torch.randn(8, 16, 16, 64))
    x = bright.clone()
    x[2:6] *= DIM
    with torch.no_grad():
        mid = _forward(copy.deepcopy(c2).double(), copy.deepcopy(b2).double(), x.double(), 2, 1, None)
        ref = _forward(copy.deepcopy(c3).double(), copy.deepcopy(b3).double(), mid, 2, 1, None)
    bands = [(2 * 256, 6 * 256)]
    assert _band_max(ref.view(-1, 256), bands) < WINDOW * float(ref.abs().max())
    return (c2, b2, c3, b3), bright, x, ref, bands


def test_chained_kernel_records_its_smallest_tile_maximum(device):
    from nerfdet_amd import conv3d as C
    (c2, b2, c3, b3), bright, x, ref, bands = _chain_case()
    with torch.no_grad():
        pk2 = C.packed([copy.deepcopy(c2).to(device)], copy.deepcopy(b2).to(device))
        pk3 = C.packed([copy.deepcopy(c3).to(device)], copy.deepcopy(b3).to(device))

    def run(v):
        xd = v.to(device)
        y, names, _ = _run(device, "f16x2", 0, 1, lambda: C.conv2d_chain_nhwc(xd, pk2, pk3, relu=1))
        assert names == ["k_conv_split_chain<64>/f16x2"], names
        return y
    _check_producer(device, "chain64", run, x, bright, ref, bands, 256)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2. producers: the elementwise passes that commit a slot
# ---------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bn_case():
    """4096 rows x 64 channels for the batch-statistics BatchNorm: the rows come in +- pairs, so every channel's mean is zero and (beta = 0) the
    output of a row is gamma invstd x: rows 1024..2048 dim.  gamma is one number g: scaling it scales the output."""
    torch.manual_seed(31)
    half = torch.randn(2048, 64)
    bright = torch.stack([half, -half], 1).reshape(4096, 64).contiguous()
    x = bright.clone()
    x[1024:2048] *= DIM
    bands = [(1024, 2048)]

    def fp64(v, g):
        v = v.double()
        return torch.relu((v - v.mean(0)) / (v.var(0, unbiased=False) + 1e-5).sqrt() * g)
    ref = fp64(x, 1.0)
    assert _band_max(ref, bands) < WINDOW * float(ref.abs().max())
    return bright, x, ref, bands


def test_bn_rows_apply_records_its_smallest_tile_maximum(device):
    from nerfdet_amd import conv3d as C, conv_train
    bright, x, ref, bands = _bn_case()
    assert C.train_arithmetic() == "f16x2"

    def run(vg):
        v, g = vg
        xd = v.to(device)
        w, b = torch.full((64,), float(g), device=device), torch.zeros(64, device=device)
        with torch.no_grad():
            return conv_train.BatchNormRows.apply(xd, w, b, None, None, 0.1, 1e-5, True, None)
    # the output scales with gamma, not with the input
    _check_producer(device, "bn_rows", lambda vg: run(vg if isinstance(vg, tuple) else (vg, 1.0)), x, bright, ref, bands, 64,
                    scaled=lambda v, s: (v, s))


def test_relu_affine_bwd_records_its_smallest_tile_maximum(device):
    """gs = dy [y > 0] scale of conv_train.ConvAffineAct's backward (ndet_relu_affine_bwd_amax): 4096 rows x 64 channels, rows 1024..2048 of dy dim."""
    from nerfdet_amd import _lib, conv3d as C
    from nerfdet_amd._lib import _ptr, raw_stream
    torch.manual_seed(32)
    bright = torch.randn(4096, 64)
    dy = bright.clone()
    dy[1024:2048] *= DIM
    yfwd = torch.randn(4096, 64)
    scale = torch.empty(64).uniform_(0.5, 1.5)
    bands = [(1024, 2048)]
    ref = torch.where(yfwd > 0, dy.double(), torch.zeros((), dtype=torch.float64)) * scale.double()
    assert _band_max(ref, bands) < WINDOW * float(ref.abs().max())
    yd, sd = yfwd.to(device), scale.to(device)

    def run(g):
        gd = g.to(device)
        gs = torch.empty_like(gd)
        slot = C.AMAX.take(device)
        _lib.check(_lib.load().ndet_relu_affine_bwd_amax(_ptr(gd), _ptr(yd), _ptr(sd), 4096, 64, 1, _ptr(None), _ptr(gs), _ptr(slot),
                                                         c_void_p(raw_stream(device))), "relu_affine_bwd_amax")
        torch.cuda.synchronize()
        C._tag_amax(gs, slot)
        return gs
    _check_producer(device, "relu_affine_bwd", run, dy, bright, ref, bands, 64)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3. producers: the persistent kernels (a workgroup takes a second and a third tile)
# ---------------------------------------------------------------------------------------------------------------------------------------------
STEM_DIM = {"images7and30": (7, 30), "image19": (19,)}


@functools.lru_cache(maxsize=None)
def _stem_case(which):
    n, h, w = LOOP3
    stem = _Stem(5, zero_shift=True)
    bright = torch.randn(n, 3, h, w, generator=torch.Generator().manual_seed(41))
    x = bright.clone()
    for i in STEM_DIM[which]:
        x[i] *= DIM
    ref = _ref64(stem.conv, stem.bn, x)
    _, ph, pw = _tiles(n, h, w)
    bands = [(i * ph * pw, (i + 1) * ph * pw) for i in STEM_DIM[which]]
    assert _band_max(ref.view(-1, 64), bands) < WINDOW * float(ref.abs().max())
    return stem, bright, x, ref, bands


def _stem_tile_max(got):
    """max |got| of the stem's tiles: TPY x TPX pooled pixels x 64 channels of one image."""
    n, ph, pw, c = got.shape
    ty, tx = -(-ph // TPY), -(-pw // TPX)
    pad = torch.zeros(n, ty * TPY, tx * TPX, c)
    pad[:, :ph, :pw] = got.abs()
    return pad.view(n, ty, TPY, tx, TPX, c).amax((2, 4, 5))


@pytest.mark.parametrize("which", list(STEM_DIM))
def test_stem_records_its_smallest_tile_maximum(device, which):
    tiles, ph, pw = _tiles(*LOOP3)
    assert tiles == 1080 and tiles // LOOP3[0] == 24, "1080 tiles at 24 per image: workgroups take a second and a third tile"
    stem, bright, x, ref, bands = _stem_case(which)
    assert float(stem.affine(device)[1].abs().max()) == 0.0
    _check_producer(device, f"stem-{which}", lambda v: stem.run(device, v.to(device), "f16x2"), x, bright, ref, bands, 64, exact=_stem_tile_max)


def test_stem_six_product_form_records_its_smallest_tile_maximum(device):
    """The bf16x3 instantiation of the stem kernel handed a slot through the C ABI (conv3d never does: only the fp16-pair mode keeps slots): it has
    no patch maximum for the tile maximum to ride on and reduces it in a chain of its own."""
    from nerfdet_amd import _lib, conv3d as C
    from nerfdet_amd._lib import _ptr, raw_stream
    stem, bright, x, ref, bands = _stem_case("image19")
    conv_d, bn_d = stem.on(device)
    lib = _lib.load()
    n, h, w = LOOP3
    _, ph, pw = _tiles(n, h, w)
    planes = torch.empty((3, 64, 176), dtype=torch.int16, device=device)
    _lib.check(lib.ndet_stem_pack_weights(_ptr(conv_d.weight.detach().float().contiguous()), _ptr(planes), c_void_p(raw_stream(device))), "stem_pack_weights")
    scale, shift = C.bn_affine(bn_d)

    def run(v):
        xd = v.to(device)
        out = torch.empty((n, ph, pw, 64), dtype=torch.float32, device=device)
        slot = C.AMAX.take(device)
        sn, sc, sy, sx = xd.stride()
        _lib.check(lib.ndet_stem_conv_bn_relu_maxpool(_ptr(xd), n, h, w, sn, sc, sy, sx, _ptr(planes), 0.0, _ptr(scale), _ptr(shift), _ptr(out), _ptr(slot),
                                                      c_void_p(raw_stream(device))), "stem_conv_bn_relu_maxpool")
        torch.cuda.synchronize()
        C._tag_amax(out, slot)
        return out
    _check_producer(device, "stem-image19-bf16x3", run, x, bright, ref, bands, 64, exact=_stem_tile_max)


WSP_TILES = (129064, 129256, 129257)
WSP_CASES = {"cout32": (32, lambda bm, n_cu: bm * (2 * n_cu + 37) - 43), "cout512": (512, lambda bm, n_cu: bm * (n_cu + 19) - 43)}


@functools.lru_cache(maxsize=1)      # (36 MB inputs: 129256 and 129257 share a case, nothing else does)
def _wsp_case(bm, cout, m):
    """A 1x1 convolution 128 -> cout over m rows (four K steps: stays on f16x2).  Dim rows [5 bm + 17, 9 bm + 3): tiles 6..8 wholly dim, 5 and 9
    mixed; and [m - 2 bm - 11, m): the last two row tiles (the last one ragged) wholly dim, the one before them mixed."""
    bands = [(5 * bm + 17, 9 * bm + 3), (m - 2 * bm - 11, m)]
    return _Layer(2, 128, cout, (1, 1, m), 1, "conv", bands, bands, xkind="rand")


@pytest.mark.parametrize("case", list(WSP_CASES))
@pytest.mark.parametrize("tile", WSP_TILES)
def test_persistent_tile_records_its_smallest_tile_maximum(device, tile, case):
    from nerfdet_amd import conv_tiles
    n_cu = torch.cuda.get_device_properties(device).multi_processor_count
    row = conv_tiles.TILES[tile]
    cout, rows_of = WSP_CASES[case]
    m = rows_of(row.rows, n_cu)
    n_tiles = -(-m // row.rows) * -(-cout // row.cols)
    assert n_tiles > (2 * n_cu if case == "cout32" else n_cu) and m % row.rows, (n_tiles, n_cu)
    layer = _wsp_case(row.rows, cout, m)
    run = _conv_runner(device, layer, tile, 1, False)
    _check_producer(device, f"wsp{tile}-{case}-m{m}", run, layer.x, layer.bright, layer.ref, layer.out_bands, cout, exact=_exact_blocks(tile))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 4. consumers: every family that calls conv_guard_check, the slot from ndet_amax_f32
# ---------------------------------------------------------------------------------------------------------------------------------------------
CONSUMERS = [
    # id, case, tile, direct
    ("unified64-staged", "3d-64", 64, False),
    ("unified128-direct", "3d", 128, True),
    ("ws128256", "3d-256", 128256, False),
    ("wsp129256", "3d-256", 129256, False),
    ("halo3128", "3d", 3128, False),
    ("halo3256", "3d-256", 3256, False),
    ("batch-unified128", "batch", 128, False),
    ("batch-halo3128", "batch", 3128, False),
]


@pytest.mark.parametrize("tag,kind,tile,direct", CONSUMERS, ids=[r[0] for r in CONSUMERS])
def test_consumer_guard_reads_the_tile_minimum(device, tag, kind, tile, direct):
    from nerfdet_amd import conv3d as C
    layer = _conv_case(kind)
    run = _conv_runner(device, layer, tile, 1, direct)
    l1 = C.guard_l1(layer.pack(device))
    amax = float(layer.x.abs().max())

    def tripped(x):
        C.guard_begin(device)
        before = C.amax_fallbacks
        run(x)
        assert C.amax_fallbacks == before + 1, "the input's slot must come from ndet_amax_f32"
        return C.guard_tripped(device)
    assert TWIN * float(layer.bright.abs().max()) * l1 * 2.0 ** -39 > C.GUARD_TOL
    got = {f: tripped(layer.x * (f * C.GUARD_TOL * 2.0 ** 39 / (l1 * amax))) for f in (4.0, 0.25)}
    twin = tripped(layer.bright * TWIN)
    print(f"CONSUMER {tag}: floor 4x {got[4.0]}, floor 1/4 {got[0.25]}, uniform twin {twin}")
    assert got[4.0] and not got[0.25] and not twin, (got, twin)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 5. structure smaller than a tile
# ---------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _small_case(k, dark):
    """4 images of 32 x 32 x 128 channels, U[0,1) x 1e9 (the maximum pinned at 1e9), into 64 channels; the dark inputs are x 2^-30.
    ``dark``: "pixel" = image 1, pixel (16, 16); "block" = image 1, rows / columns 14..19 (its 3x3 centre sees only dark inputs through a 3x3 kernel);
    "tiles" = images 1 and 2 whole (2048 rows: whole tiles of every kernel on both axes)."""
    torch.manual_seed(50 + k)
    conv, bn = nn.Conv2d(128, 64, k, 1, k // 2, bias=False), _zero_shift_bn(2, 64)
    x = torch.rand(4, 32, 32, 128) * 1.0e9
    x[0, 0, 0, 0] = 1.0e9
    mask = torch.zeros(4, 32, 32, dtype=torch.bool)        # outputs that see dark inputs only
    r = k // 2
    if dark == "pixel":
        x[1, 16, 16] *= DIM
        if k == 1:
            mask[1, 16, 16] = True
    elif dark == "block":
        x[1, 14:19, 14:19] *= DIM
        mask[1, 14 + r:19 - r, 14 + r:19 - r] = True
    else:
        x[1:3] *= DIM
        mask[1:3, r:32 - r, r:32 - r] = True
    with torch.no_grad():
        conv64, bn64 = copy.deepcopy(conv).double(), copy.deepcopy(bn).double()
        ref = _forward(conv64, bn64, x.double(), 2, 1, None)
        # per output: the bound of conv_common.hpp:62-66 -- 2^-39 amax |scale_j| sum_k |w_jk| + 2^-22 |scale_j| sum_k |w_jk| |a_k|
        scale = (bn64.weight / (bn64.running_var + bn64.eps).sqrt()).abs()
        wabs = copy.deepcopy(conv64)
        wabs.weight.abs_()
        l1 = conv64.weight.abs().sum((1, 2, 3)) * scale
        bound = 2.0 ** -39 * 1.0e9 * l1.view(1, 1, 1, -1) + 2.0 ** -22 * scale.view(1, 1, 1, -1) * _forward(wabs, None, x.double().abs(), 2, 0, None)
    return conv, bn, x, ref, mask, bound


@pytest.mark.parametrize("k,dark", [(1, "pixel"), (1, "block"), (3, "block")], ids=["1x1-pixel", "1x1-block", "3x3-block"])
def test_dark_structure_smaller_than_a_tile(device, k, dark):
    from nerfdet_amd import conv3d as C
    conv, bn, x, ref, mask, bound = _small_case(k, dark)
    assert int(mask.sum()) == (1 if dark == "pixel" else (25 if k == 1 else 9))
    with torch.no_grad():
        pk = C.packed([copy.deepcopy(conv).to(device)], copy.deepcopy(bn).to(device))
    xd = x.to(device)
    out, trip = {}, {}
    for arith in ("bf16x3", "f16x2"):
        C.guard_begin(device)
        out[arith] = _run(device, arith, 0, 0, lambda: C.conv2d_nhwc(xd, pk, relu=1))[0].cpu().double()
        trip[arith] = C.guard_tripped(device)
    err3 = (out["bf16x3"] - ref)[mask].abs()
    err2 = (out["f16x2"] - ref)[mask].abs()
    ratio = float((err2 / bound[mask]).max())
    print(f"SUBTILE {k}x{k} {dark}: dark outputs max|ref| {float(ref[mask].abs().max()):.3e} | bf16x3 err {float(err3.max()):.3e} | f16x2 err {float(err2.max()):.3e} "
          f"measured/bound {ratio:.3f} | f16x2/bf16x3 {float(err2.max()) / max(float(err3.max()), 1e-300):.1f} | guard tripped: {trip['f16x2']}")
    assert bool((err3 <= 1e-4 * ref[mask].abs().clamp_min(1.0)).all()), "bf16x3 on the dark outputs"
    assert not trip["bf16x3"]
    assert ratio <= 1.0, f"f16x2 error is {ratio} x the bound of conv_common.hpp:62-66"
    assert float(err2.max()) > 10.0 * float(err3.max()), (float(err2.max()), float(err3.max()))      # the loss is real


@pytest.mark.parametrize("k", [1, 3])
def test_dark_region_of_whole_tiles_trips(device, k):
    from nerfdet_amd import conv3d as C
    conv, bn, x, ref, mask, bound = _small_case(k, "tiles")
    with torch.no_grad():
        pk = C.packed([copy.deepcopy(conv).to(device)], copy.deepcopy(bn).to(device))
    xd = x.to(device)
    C.guard_begin(device)
    y = _run(device, "f16x2", 0, 0, lambda: C.conv2d_nhwc(xd, pk, relu=1))[0].cpu().double()
    assert C.guard_tripped(device), "a dark region of whole tiles under a 1e9 maximum must raise the guard"
    err = (y - ref)[mask].abs()
    assert float((err / bound[mask]).max()) <= 1.0
