"""The convolution data gradients of the training step (nerfdet_amd/conv_train.py: _conv_grads -> _adjoint_pack -> conv3d.conv3d_ndhwc / conv2d_nhwc, the
training form of ndet_conv_split: NdetConvArgs.w_amax != NULL) against tests/dgrad_ref.py in fp64, on every tile family and in both training
arithmetics (fp16 pairs, the default, and bf16x3: conv3d.TRAIN_F16X2).  The reference is proved against fp64 CPU autograd, and PRODUCTION below
against a walk over the cfg3 training workload, in tests/test_dgrad_ref_cpu.py.

(a) THE EXACT LADDER on the adjoint launch, tile pinned (test_adjoint_ladder*, test_convT2_dx_ladder).  The pack is conv_train._train_pack(w, kernel,
    adjoint=True)[0], the input dy zero-padded to a multiple of 32 channels -- what _conv_grads launches, with the tile named.  On integer data
    (dy in -3 .. 3, weights in -2 .. 2, every partial sum below taps x padded Cout x 6 < 2^24) dx must equal dx_conv in fp64 BIT FOR BIT on every id
    of conv_tiles.ids("unified", "ws", "wsp", "halo") at 1, 2, 3 and min(32, K steps) splits (halo: min(32, padded Cout / 32)); the unsplit unified
    launch also in its direct form (the one production always takes: the adjoint's Cout is a multiple of 32); the persistent tiles give 128256's
    bits.  The 1x1 rows walk 1, 2 and 3 K steps in fp16 pairs (a pinned pack does not fall back to bf16x3 below F16_MIN_KSTEPS) on tiles 64 / 100064 /
    128 / 100128 / 12864 / 112864 and on 128256 (one step under WS_DEPTH = 2).  The ConvT2 dx launch (_train_pack(w, (2, 2, 2), False, 2, (0, 0, 0)))
    at 128 -> 32 and 128 -> 64 on tiles 64 / 128 / 128256.  In f16x2 every launch leaves the exact max |dx| slot and is the named kernel's "/f16x2" form.
(b) REAL-VALUED ROWS (test_real_row), one per (tile, splits) pair the cfg3 step dispatches a data gradient to (PRODUCTION) plus one per family at splits
    1: gradient_like dy (80 % of the voxels zero, magnitudes over e^+-4.5), Kaiming weights, the smallest ragged shape whose K-step count (halo: chunk
    count) is no multiple of the split count, always with 7 zero padding channels.  |dx - ref| <= ELEM_BAR max|ref| elementwise, rel-rms < RMS_BAR
    (tests/test_f16x2_edges_gpu.py's bars: they hold for the same kernels at K = 128 ... 6912, the operand scheme alone leaves 8e-8; here relative to
    max|ref| itself, the stricter form: a gradient has no natural unit), an exact slot, the same bits from a second launch; the ratio
    rel-rms(f16x2) / rel-rms(bf16x3) is printed, not asserted.
(c) THROUGH AUTOGRAD (test_autograd_*), tile not pinned: the launch hook must see the kernel that conv3d.choose_tiling_split + conv_tiles.resolve
    give for the adjoint key (predicted(); the CPU file walks the same rule).  ConvS1 stride 1 and stride 2 (deterministic mode: the bars of (b) and
    two backward passes bitwise equal; vendor-library mode: max(2e-5, 2 e32) max|ref|, e32 the error of dx_conv evaluated in fp32 -- the rule of
    tests/test_wgrad_shapes_gpu.py), ConvAffineAct (d_residual == dy [y > 0] bitwise, the slot on g' exact), the head's shared convolution
    (dx against the sum of the three layers' data gradients), ConvT2; and dy 2^-20 gives dx and dW times 2^-20 bit for bit.
(d) DEGENERATE GRADIENTS (test_all_zero_dy, test_impulses): all-zero dy gives exactly zero, finite, with a zero slot; a single 1.0 in channel 24 of 25
    at each corner and the centre of the output grid gives EXACTLY the weight slab w[24, :, t] at i = s o + t - p (grid_weights: one product per
    output, every operand representable), zero elsewhere, the other image of a 2D batch untouched.  Before each launch NaN blocks of the size of the
    padded dy, the upsample buffer, the workspace and the result are allocated and freed (_poison): an unwritten padding channel shows as NaN.

Measured on an MI355X (elem = max |dx - ref| / max|ref|, rel-rms, the PRINTED ratio rel-rms(f16x2) / rel-rms(bf16x3) on the same tile and split;
K steps = taps x padded Cout / 32, on the halo tiles the channel chunks that they split).  The ladder: all 110 (tile, layer, arithmetic) rows, the six
1x1 rows on seven tile ids and the four ConvT2 rows equal the fp64 result at every split count; THE LIBRARY REFUSED NO PAIR (the 1x1 test asserts it), 128256
took the walks of one, two and three steps.

    (b)  tile(s)                      splits  layer     grid    kernel  K steps    elem      rel-rms   f16x2/bf16x3
         64, 100064, 12864              1     96->25    3x4x5   3x3x3   27         3.19e-07  1.78e-07  0.99
         64                             4     96->25    3x4x5   3x3x3   27         1.84e-07  1.18e-07  1.21
         64                             5     96->25    3x4x5   3x3x3   27         2.38e-07  1.22e-07  1.22
         128, 100128                    1     160->25   3x4x5   3x3x3   27         2.13e-07  1.71e-07  0.91
         128256, 129256/257/064         1     288->25   3x4x5   3x3x3   27         1.94e-07  1.17e-07  1.09
         128256                         2     288->25   3x4x5   3x3x3   27         1.92e-07  1.06e-07  1.17
         128256                         4     288->25   3x4x5   3x3x3   27         1.77e-07  9.82e-08  1.30
         128256                        15     288->25   3x4x5   3x3x3   27         1.46e-07  8.96e-08  1.74
         128256                        16     288->25   3x4x5   3x3x3   27         1.46e-07  8.98e-08  1.74
         3128                           1     160->25   3x4x5   3x3x3   1 chunk    1.99e-07  1.61e-07  0.91
         3256, 3257, 3258               1     288->25   3x4x5   3x3x3   1 chunk    1.94e-07  1.17e-07  1.09
         3258                           2     288->89   3x4x5   3x3x3   3 chunks   3.50e-07  1.85e-07  0.86
         3256                           3     288->121  3x4x5   3x3x3   4 chunks   3.79e-07  1.73e-07  0.96
         3256, 3257                     4     288->153  3x4x5   3x3x3   5 chunks   2.53e-07  1.78e-07  0.87
    (c)  kernel that ran (as predicted)       layer     grid    kernel  K steps    elem      rel-rms   bf16x3 elem / rel-rms   e32, vendor library
         100064 x 1                           96->25    7x9x5   3x3x3   27         3.58e-07  1.81e-07  4.84e-07 / 1.94e-07     1.79e-07
         100064 x 1                           64->96    2x11x13 3x3     27         2.46e-07  1.53e-07  4.07e-07 / 1.85e-07     4.08e-07
         64 x 4 (stride 2, deterministic)     64->128   7x9x5   3x3x3   108        1.49e-07  1.00e-07  8.95e-08 / 8.16e-08     3.27e-07, library 1.23e-07
         100064 x 1 (stride 2, deterministic) 64->64    2x11x13 3x3     18         1.68e-07  1.16e-07  1.67e-07 / 1.17e-07     1.95e-07, library 2.73e-07
         100064 x 1 (ConvAffineAct)           128->64   2x11x13 3x3     18         2.05e-07  1.43e-07  1.94e-07 / 1.56e-07
         100064 x 1 (ConvAffineAct)           256->64   2x11x13 1x1     2          1.92e-07  1.08e-07  2.04e-07 / 1.06e-07
         100064 x 1 (head, 1 + 6 + 18)        128->25   6x5x4   3x3x3   27         4.60e-07  1.83e-07  4.30e-07 / 1.91e-07
         100064 x 1 (ConvT2)                  128->32   3x4x5   2x2x2   8          1.31e-07  1.02e-07  1.31e-07 / 9.07e-08     1.54e-07

Every bar kept a factor 40 or more (2e-5 elementwise, 2e-6 rel-rms; the vendor-library rows' bar was 2e-5: 2 e32 stayed below 1e-6).  The ratio passes 1
where ONE chunk of 27 K steps is split (up to 1.74 at 15 and 16 splits: walks of one and two steps, the fp32 sum of the partials is most of what is
left, and bf16x3's exact operands show); it is printed, not asserted, as in tests/test_f16x2_edges_gpu.py.  The power-of-two scaling, the all-zero
gradients and the impulses held bit for bit in both arithmetics.

With three host-side mutations applied by monkeypatch (a scratch run, nothing of it is kept) this file / tests/test_conv_train_gpu.py failed
151 / 26 tests (adjoint planes without the flip on the last axis: random weights show it there too), 1 / 0 (dy padding channels 1.0: the scaling row
with 25 channels, where the padding takes the fp16-pair scale over from a gradient-sized dy) and 10 / 0 (half the maximum in the slot on dx: every
autograd row in f16x2).
"""
import contextlib
import functools
import math
import types

import pytest
import torch
import torch.nn.functional as F

import dgrad_ref as R
from nerfdet_amd import conv_tiles
from test_f16x2_edges_gpu import ELEM_BAR, RMS_BAR, _slot_is_exact

pytestmark = pytest.mark.gpu

ARITHS = ("f16x2", "bf16x3")
LADDER_TILES = conv_tiles.ids("unified", "ws", "wsp", "halo")
LADDER_ROWS = [(t, n) for t in LADDER_TILES for n in R.LADDER]

# the distinct (tile, splits) pairs the data-gradient launches of one cfg3 training step resolve to (tests/test_dgrad_ref_cpu.py walks the modules)
PRODUCTION = [
    (64, 4), (64, 5),                                                       # the coarsest level's 1024-channel output block and ConvT2 dx
    (100064, 1), (100128, 1),                                               # the unsplit unified launches: always the direct form
    (128256, 1), (128256, 2), (128256, 4), (128256, 15), (128256, 16),      # layer4, the stride-2 detours, the coarse 3D levels
    (129064, 1),                                                            # layer3's 1x1 expansions
    (3256, 1), (3256, 3), (3256, 4), (3257, 1), (3257, 4), (3258, 1), (3258, 2),      # the 3x3 / 3x3x3 layers of 256 and 512 channels
]
REAL_ROWS = PRODUCTION + [(64, 1), (128, 1), (12864, 1), (129256, 1), (129257, 1), (3128, 1)]       # ... and the other tiles, staged and unsplit
# the layer Cin of a row (the adjoint's Cout): ragged on the tile's columns
REAL_CIN = {64: 96, 128: 160, 12864: 96, 128256: 288, 129256: 288, 129257: 288, 129064: 288, 3128: 160, 3256: 288, 3257: 288, 3258: 288}


@contextlib.contextmanager
def train_arithmetic(arith):
    """The training arithmetic for the block: fp16 pairs (the default) or the six-product bf16x3 kernels (conv3d.TRAIN_F16X2 = False)."""
    import nerfdet_amd.conv3d as C
    prev, C.TRAIN_F16X2 = C.TRAIN_F16X2, arith == "f16x2"
    try:
        assert C.train_arithmetic() == arith
        yield
    finally:
        C.TRAIN_F16X2 = prev


@pytest.fixture
def arith(request):
    """The TRAIN_F16X2 fixture of tests/test_conv_train_gpu.py, parametrised indirectly."""
    with train_arithmetic(request.param):
        yield request.param


@contextlib.contextmanager
def watched(direct=True):
    """The launch hook and conv_tiles.resolve watched for the block: (kernel names, resolved (tile, splits)) of every MFMA-convolution launch."""
    from nerfdet_amd import conv3d as C
    names, resolved = [], []
    real_resolve = conv_tiles.resolve

    def hook(flops, thunk, name):
        names.append(name)
        return thunk()

    def resolve(*a, **kw):
        resolved.append(real_resolve(*a, **kw))
        return resolved[-1]
    prev_direct, prev_hook = C.DIRECT_EPILOGUE, C.launch_hook
    try:
        C.DIRECT_EPILOGUE, C.launch_hook, conv_tiles.resolve = direct, hook, resolve
        yield names, resolved
        torch.cuda.synchronize()
    finally:
        C.DIRECT_EPILOGUE, C.launch_hook, conv_tiles.resolve = prev_direct, prev_hook, real_resolve


@contextlib.contextmanager
def conv_outputs():
    """Every tensor conv_train._conv returns inside the block (in a backward pass: the data gradients, as _conv_grads / ConvT2.backward hand them on)."""
    from nerfdet_amd import conv_train
    outs, real = [], conv_train._conv

    def conv(x, pk, **kw):
        outs.append(real(x, pk, **kw))
        return outs[-1]
    conv_train._conv = conv
    try:
        yield outs
    finally:
        conv_train._conv = real


def _dx_slots_are_exact(outs, arith, n=1):
    """The slot the launch left on dx, read where the next layer's data and weight gradients read it: the tensor's maximum in f16x2, none in bf16x3."""
    assert len(outs) == n
    for dx in outs:
        if arith == "f16x2":
            _slot_is_exact(dx)
        else:
            assert getattr(dx, "_ndet_amax", None) is None


def _poison(device, *sizes):
    """NaN into what the launch is about to take with torch.empty / new_zeros -- the padded dy, the upsample buffer, the split-K workspace, the result:
    the caching allocator hands a freed block to the next request of its size (tests/test_wgrad_shapes_gpu.py::_poison).
    That is the allocator's habit, not a guarantee: tests/redzone.py carves every such allocation and fills it itself (tests/test_redzone_train_gpu.py)."""
    blocks = [torch.full((int(n),), float("nan"), device=device) for n in sizes if n]
    del blocks


def kernel_name(tile, arith):
    return conv_tiles.TILES[tile].name + ("/f16x2" if arith == "f16x2" else "")


def _conv(x, pk, **kw):
    from nerfdet_amd import conv3d as C
    return (C.conv3d_ndhwc if pk.ndim == 3 else C.conv2d_nhwc)(x, pk, **kw)


def _pad32(dy):
    return dy if dy.shape[-1] % 32 == 0 else F.pad(dy, (0, 32 - dy.shape[-1] % 32))


def _launch(device, dyp, pk, tile, splits, arith, direct=False):
    """One pinned adjoint launch with its checks: the kernel that ran, (tile, splits) left alone, in f16x2 an exact slot."""
    m = dyp.numel() // dyp.shape[-1]
    _poison(device, dyp.numel(), m * pk.cout * splits, m * pk.cout)
    with watched(direct) as (names, resolved):
        got = _conv(dyp, pk, tile=tile, splits=splits)
    assert names == [kernel_name(tile, arith)] and resolved == [(tile, splits)], (names, resolved, tile, splits)
    if arith == "f16x2":
        _slot_is_exact(got)
    else:
        assert getattr(got, "_ndet_amax", None) is None
    return got


def _differs(got, ref):
    return int((got != ref).sum()), float((got - ref).abs().max())


# ---- (a) the exact ladder ----
@functools.lru_cache(maxsize=None)
def integer_data(name):
    """(dy, w) of a ladder row on the CPU, shared and never written to."""
    if name in R.LADDER_T2:
        cin, cout, grid = R.LADDER_T2[name]
        return R.integer_case(cin, cout, (2, 2, 2), tuple(2 * v for v in grid), seed=sorted(R.LADDER_T2).index(name) + 100, transposed=True)
    cin, cout, kernel, grid = {**R.LADDER, **R.LADDER_1X1}[name]
    return R.integer_case(cin, cout, kernel, grid, seed=sorted({**R.LADDER, **R.LADDER_1X1}).index(name))


@functools.lru_cache(maxsize=None)
def _exact(name, device):
    """(dy zero-padded to 32 channels, w, fp32 copy of the fp64 result) on the device."""
    dy, w = integer_data(name)
    dy, w = dy.to(device), w.to(device)
    if name in R.LADDER_T2:
        ref, bound = R.dx_convT2(dy, w), R.integer_bound(w.shape[1], (2, 2, 2))
    else:
        ref, bound = R.dx_conv(dy, w, 1, tuple(dy.shape[:3])), R.integer_bound(w.shape[0], w.shape[2:])
    assert bound < R.EXACT_BELOW and float(ref.abs().max()) <= bound and torch.equal(ref.float().double(), ref)
    return _pad32(dy).contiguous(), w, ref.float()


@pytest.mark.parametrize("arith", ARITHS, indirect=True)
@pytest.mark.parametrize("tile,name", LADDER_ROWS, ids=[f"{t}-{n}" for t, n in LADDER_ROWS])
def test_adjoint_ladder(device, tile, name, arith):
    from nerfdet_amd import conv_train
    row = conv_tiles.TILES[tile]
    cin, cout, kernel, grid = R.LADDER[name]
    dyp, w, ref = _exact(name, device)
    pk = conv_train._train_pack(w, kernel, adjoint=True)[0]
    assert (pk.cout, pk.cin, pk.arith) == (cin, R.padded(cout), arith) and dyp.shape[-1] == pk.cin
    wrong = []            # (splits, differing elements, max |difference|): every split count is run before the verdict
    for splits in R.ladder_splits(cout, kernel, row.family == "halo"):
        got = _launch(device, dyp, pk, tile, splits, arith)
        if not torch.equal(got, ref):
            wrong.append((splits,) + _differs(got, ref))
        if row.family == "unified" and splits == 1:          # the form production takes: stored straight from the accumulators
            direct = _launch(device, dyp, pk, row.partner, 1, arith, direct=True)
            assert torch.equal(direct, got), "direct and staged epilogue differ"
        if row.family == "wsp":
            one_shot = _launch(device, dyp, pk, 128256, splits, arith)
            assert torch.equal(got, one_shot), f"splits {splits}: the persistent tile must reproduce the one-shot tile bit for bit"
    print(f"DGRAD-LADDER {tile} {name} {arith}: splits {R.ladder_splits(cout, kernel, row.family == 'halo')}, wrong at {wrong}")
    assert not wrong, f"(splits, differing elements, max |got - ref|) on exact integer data: {wrong}"


@pytest.mark.parametrize("arith", ARITHS, indirect=True)
@pytest.mark.parametrize("name", list(R.LADDER_1X1))
def test_adjoint_ladder_of_one_two_and_three_k_steps(device, name, arith):
    """1x1 layers of 32 / 64 / 96 output channels: the pinned fp16-pair pack walks 1, 2, 3 K steps, below conv3d.F16_MIN_KSTEPS."""
    from nerfdet_amd import conv3d as C, conv_train
    cin, cout, kernel, grid = R.LADDER_1X1[name]
    dyp, w, ref = _exact(name, device)
    pk = conv_train._train_pack(w, kernel, adjoint=True)[0]
    assert R.adjoint_ksteps(cout, kernel) < C.F16_MIN_KSTEPS and pk.arith == arith
    wrong, refused = [], []
    for tile in R.TILES_1X1:
        direct = conv_tiles.is_direct(tile)
        for splits in ([1] if direct else R.ladder_splits(cout, kernel, False)):
            try:
                got = _launch(device, dyp, pk, tile, splits, arith, direct=direct)
            except (ValueError, AssertionError) as e:
                if not str(e).startswith("conv_split:"):       # (_lib.check's message; anything else is a failed check of this file)
                    raise
                refused.append((tile, splits))
                continue
            if not torch.equal(got, ref):
                wrong.append((tile, splits) + _differs(got, ref))
    print(f"DGRAD-LADDER-1X1 {name} {arith}: wrong at {wrong}, refused {refused}")
    assert not refused, f"the library refused (tile, splits) {refused} although conv_tiles.resolve let them through: the two must agree"
    assert not wrong, f"(tile, splits, differing elements, max |got - ref|) on exact integer data: {wrong}"


@pytest.mark.parametrize("arith", ARITHS, indirect=True)
@pytest.mark.parametrize("name", list(R.LADDER_T2))
def test_convT2_dx_ladder(device, name, arith):
    """What ConvT2.backward launches for dx: the unpadded k2 s2 convolution of dy with the transposed layer's weight read as a Conv3d weight."""
    from nerfdet_amd import conv_train
    cin, cout, grid = R.LADDER_T2[name]
    dy, w, ref = _exact(name, device)
    pk = conv_train._train_pack(w, (2, 2, 2), False, 2, (0, 0, 0))[0]
    assert (pk.cout, pk.cin, pk.strides, pk.pads) == (cin, cout, (2, 2, 2), (0, 0, 0)) and tuple(ref.shape) == tuple(grid) + (cin,)
    wrong = []
    for tile in R.TILES_T2:
        for splits in sorted({1, 2, 3, 8 * cout // 32}):
            got = _launch(device, dy, pk, tile, splits, arith)
            if not torch.equal(got, ref):
                wrong.append((tile, splits) + _differs(got, ref))
    assert not wrong, f"(tile, splits, differing elements, max |got - ref|) on exact integer data: {wrong}"


# ---- (b) real-valued rows ----
def real_shape(tile, splits):
    """(layer Cin, layer Cout, kernel, grid) of the row of one pair: the smallest ragged shape whose K-step count (halo: chunk count) is NOT a multiple
    of ``splits``; Cout = 32 chunks - 7, so the last chunk always ends in 7 zero padding channels.  3x3x3 on 60 voxels; 27 K steps a chunk are a
    multiple of 3, 9 and 27, so those split counts take a 1x1x1 layer on 315 voxels."""
    row = conv_tiles.TILES[tile]
    cin = REAL_CIN[row.partner if row.flags & conv_tiles.DIRECT else tile]
    if row.family == "halo":
        chunks, kernel, grid = (1 if splits == 1 else splits + 1), (3, 3, 3), (3, 4, 5)
    elif splits > 1 and 27 % splits == 0:
        chunks, kernel, grid = splits + 1, (1, 1, 1), (5, 7, 9)
    else:
        chunks = next(c for c in range(1, 34) if 27 * c >= splits and (splits == 1 or (27 * c) % splits))
        kernel, grid = (3, 3, 3), (3, 4, 5)
    return cin, 32 * chunks - 7, kernel, grid


def real_units(tile, splits):
    cin, cout, kernel, grid = real_shape(tile, splits)
    return R.padded(cout) // 32 if conv_tiles.TILES[tile].family == "halo" else R.adjoint_ksteps(cout, kernel)


@functools.lru_cache(maxsize=None)
def _real(cin, cout, kernel, grid, device):
    """(padded dy, w, fp64 dx) of a real-valued row on the device, shared by every row of that shape."""
    dy = R.gradient_like(grid, cout, seed=cin + 3 * cout + sum(grid)).to(device)
    w = R.kaiming(cout, cin, kernel, seed=cin + cout).to(device)
    return _pad32(dy).contiguous(), w, R.dx_conv(dy, w, 1, grid)


def _check_bars(what, got, ref, elem_bar=ELEM_BAR, rms_bar=RMS_BAR):
    elem, rms = R.rel_max(got, ref), R.rel_rms(got, ref)
    assert bool(torch.isfinite(got).all()), what
    assert elem <= elem_bar and rms < rms_bar, f"{what}: elem {elem:.3e} (bar {elem_bar:.1e}) rel-rms {rms:.3e} (bar {rms_bar:.1e})"
    return elem, rms


@pytest.mark.parametrize("tile,splits", REAL_ROWS)
def test_real_row(device, tile, splits):
    from nerfdet_amd import conv_train
    cin, cout, kernel, grid = real_shape(tile, splits)
    units = real_units(tile, splits)
    assert units >= splits and (splits == 1 or units % splits), "the row must cut its K walk unevenly"
    dyp, w, ref = _real(cin, cout, kernel, grid, device)
    direct = conv_tiles.is_direct(tile)
    out = {}
    for arith in ARITHS:
        with train_arithmetic(arith):
            pk = conv_train._train_pack(w, kernel, adjoint=True)[0]
            out[arith] = _launch(device, dyp, pk, tile, splits, arith, direct=direct)
            again = _launch(device, dyp, pk, tile, splits, arith, direct=direct)
        assert torch.equal(out[arith], again), "the same launch twice: split-K is a fixed-order sum"
    elem3, rms3 = R.rel_max(out["bf16x3"], ref), R.rel_rms(out["bf16x3"], ref)
    elem, rms = R.rel_max(out["f16x2"], ref), R.rel_rms(out["f16x2"], ref)
    print(f"DGRAD-ROW {tile} x {splits} ({cin}->{cout} {'x'.join(map(str, grid))} k{kernel[0]}, {units} {'chunks' if conv_tiles.TILES[tile].family == 'halo' else 'K steps'}): "
          f"elem {elem:.2e} rel-rms {rms:.2e} | bf16x3 elem {elem3:.2e} rel-rms {rms3:.2e} | f16x2/bf16x3 {rms / rms3:.2f}")
    _check_bars(f"{tile} x {splits} f16x2", out["f16x2"], ref)
    _check_bars(f"{tile} x {splits} bf16x3", out["bf16x3"], ref)


# ---- (c) through autograd ----
def predicted(m, cout, cin, taps, halo_ok):
    """(tile, splits) conv3d._conv_split gives a launch of ``m`` rows, ``cout`` output and ``cin`` (padded) input channels over ``taps`` taps when
    nobody names a tile, under ARITHMETIC = "f16x2": the tables and the fallback rule, then conv_tiles.resolve.  Pure Python."""
    from nerfdet_amd import conv3d as C
    prev = C.set_arithmetic("f16x2")
    try:
        tile, splits = C.choose_tiling_split(m, cout, taps * (cin // 32), 0, 0, False, halo_ok)
        return conv_tiles.resolve(tile, splits, m=m, cout=cout, cin=cin, taps=taps, transposed=False, halo_ok=halo_ok, direct_epilogue=C.DIRECT_EPILOGUE)
    finally:
        C.set_arithmetic(prev)


def autograd_key(name):
    """(m, Cout, Cin, taps, halo_ok) of the data-gradient launch of an AUTOGRAD case: the adjoint convolution over the layer's input grid (stride 2:
    the deterministic detour), or, ConvT2, the k2 s2 convolution of dy."""
    module, cin, cout, kernel, stride, grid = R.AUTOGRAD[name]
    if module == "ConvT2":
        return math.prod(grid), cin, cout, 8, False
    return math.prod(grid), cin, R.padded(cout), math.prod(kernel), math.prod(kernel) > 1


def _dx_launch_is_predicted(name, arith, names, resolved):
    tile, splits = predicted(*autograd_key(name))
    assert names == [kernel_name(tile, arith)] and resolved == [(tile, splits)], (name, names, resolved, (tile, splits))


@functools.lru_cache(maxsize=None)
def _auto(name, device):
    """(x, w, dy, fp64 dx, e32) of a ConvS1 / ConvT2 case on the device: shared, never written to."""
    module, cin, cout, kernel, stride, grid = R.AUTOGRAD[name]
    seed = sorted(R.AUTOGRAD).index(name)
    torch.manual_seed(seed)
    x = torch.randn(*grid, cin).to(device)
    if module == "ConvT2":
        w = R.kaiming(cout, cin, kernel, seed, transposed=True).to(device)
        dy = R.gradient_like(tuple(2 * v for v in grid), cout, seed).to(device)
        ref, r32 = R.dx_convT2(dy, w), R.dx_convT2(dy, w, torch.float32)
    else:
        w = R.kaiming(cout, cin, kernel, seed).to(device)
        dy = R.gradient_like(R.out_grid(grid, kernel, stride), cout, seed).to(device)
        ref, r32 = R.dx_conv(dy, w, stride, grid), R.dx_conv(dy, w, stride, grid, torch.float32)
    return x, w, dy, ref, R.rel_max(r32, ref)


def _backward(name, device, dy, want_dw=False):
    """One forward + backward of a ConvS1 / ConvT2 case: (dx, dW or None, kernel names and resolved pairs of the BACKWARD's launches)."""
    from nerfdet_amd.conv_train import ConvS1, ConvT2
    module, cin, cout, kernel, stride, grid = R.AUTOGRAD[name]
    x, w, _, _, _ = _auto(name, device)
    xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(want_dw)
    out = ConvT2.apply(xg, wg) if module == "ConvT2" else ConvS1.apply(xg, wg, stride)
    assert out.shape == dy.shape
    _poison(device, math.prod(grid) * R.padded(cout), math.prod(grid) * cin, dy.numel() // cout * R.padded(cout))
    with watched() as (names, resolved), conv_outputs() as outs:
        out.backward(dy)
    from nerfdet_amd import conv3d as C
    if names:          # (the vendor library's stride-2 data gradient launches nothing of ours and leaves no slot)
        _dx_slots_are_exact(outs[:1], C.train_arithmetic())
    return xg.grad, wg.grad, names, resolved


@pytest.mark.parametrize("arith", ARITHS, indirect=True)
@pytest.mark.parametrize("name", ["s1-3d-96to25", "s1-2d-64to96", "t2-128to32"])
def test_autograd_stride_1_and_transposed(device, name, arith):
    x, w, dy, ref, e32 = _auto(name, device)
    dx, _, names, resolved = _backward(name, device, dy)
    _dx_launch_is_predicted(name, arith, names, resolved)
    elem, rms = _check_bars(f"{name} {arith}", dx, ref)
    print(f"DGRAD-AUTO {name} {arith} ran {names[0]} x {resolved[0][1]}: elem {elem:.2e} rel-rms {rms:.2e} (fp32 statement {e32:.2e})")


@pytest.mark.parametrize("arith", ARITHS, indirect=True)
@pytest.mark.parametrize("name", ["s2-3d-64to128", "s2-2d-64to64"])
def test_autograd_stride_2_in_both_modes(device, name, arith):
    from nerfdet_amd import autograd as A
    x, w, dy, ref, e32 = _auto(name, device)
    prev = A.set_deterministic(True)
    try:
        dx, _, names, resolved = _backward(name, device, dy)
        again, _, _, _ = _backward(name, device, dy)
    finally:
        A.set_deterministic(prev)
    _dx_launch_is_predicted(name, arith, names, resolved)
    assert torch.equal(dx, again), "the deterministic mode's data gradient must reproduce bit for bit"
    elem, rms = _check_bars(f"{name} {arith} deterministic", dx, ref)
    prev = A.set_deterministic(False)
    try:
        lib, _, names, _ = _backward(name, device, dy)
    finally:
        A.set_deterministic(prev)
    assert names == [], "the vendor library's data gradient: no MFMA launch"
    err, bar = R.rel_max(lib, ref), max(2e-5, 2.0 * e32)
    print(f"DGRAD-AUTO {name} {arith} ran {kernel_name(*resolved[0][:1], arith)} x {resolved[0][1]}: elem {elem:.2e} rel-rms {rms:.2e} | vendor library {err:.2e} e32 {e32:.2e} bar {bar:.2e}")
    assert bool(torch.isfinite(lib).all()) and err <= bar, f"{name} vendor library: {err:.3e} > {bar:.3e} (fp32 statement: {e32:.3e})"


@functools.lru_cache(maxsize=None)
def _affine(name, device):
    module, cin, cout, kernel, stride, grid = R.AUTOGRAD[name]
    g = torch.Generator().manual_seed(sorted(R.AUTOGRAD).index(name))
    x = torch.relu(torch.randn(*grid, cin, generator=g)).to(device)
    w = R.kaiming(cout, cin, kernel, 11).to(device)
    scale = ((torch.rand(cout, generator=g) + 0.5) * (1 - 2 * (torch.arange(cout) % 3 == 0).float())).to(device)      # both signs
    shift = (torch.randn(cout, generator=g) * 0.2).to(device)
    res = torch.randn(*grid, cout, generator=g).to(device)
    dy = R.gradient_like(grid, cout, 12).to(device)
    return x, w, scale, shift, res, dy


def _affine_backward(name, device, dy, want_dw=False):
    """ConvAffineAct forward + backward (ReLU, residual): (y, dx, dW, d_residual, g' as _conv_grads received it, names, resolved)."""
    from nerfdet_amd import conv_train
    x, w, scale, shift, res, _ = _affine(name, device)
    xg, wg, rg = x.clone().requires_grad_(True), w.clone().requires_grad_(want_dw), res.clone().requires_grad_(True)
    y = conv_train.ConvAffineAct.apply(xg, wg, scale, shift, rg, True, 1)
    seen, real = [], conv_train._conv_grads

    def grads(ctx, xs, ws, gs):
        seen.append(gs)
        return real(ctx, xs, ws, gs)
    _poison(device, dy.numel(), dy.numel(), x.numel())
    conv_train._conv_grads = grads
    try:
        with watched() as (names, resolved), conv_outputs() as outs:
            y.backward(dy)
    finally:
        conv_train._conv_grads = real
    assert len(seen) == 1
    from nerfdet_amd import conv3d as C
    _dx_slots_are_exact(outs[:1], C.train_arithmetic())
    return y.detach(), xg.grad, wg.grad, rg.grad, seen[0], names, resolved


@pytest.mark.parametrize("arith", ARITHS, indirect=True)
@pytest.mark.parametrize("name", ["affine-2d-128to64", "affine-2d-256to64-1x1"])
def test_autograd_conv_affine_act(device, name, arith):
    from nerfdet_amd import conv3d as C
    module, cin, cout, kernel, stride, grid = R.AUTOGRAD[name]
    x, w, scale, shift, res, dy = _affine(name, device)
    y, dx, _, d_res, gs, names, resolved = _affine_backward(name, device, dy)
    _dx_launch_is_predicted(name, arith, names, resolved)
    dead = y <= 0
    assert bool(dead.any()) and not bool(dead.all())
    assert torch.equal(d_res, dy * (y > 0)), "the identity's gradient is dy [y > 0], bit for bit"
    g64, d64 = R.affine_act_bwd(dy, y, scale, True)
    assert torch.equal(d64.float(), d_res) and R.rel_max(gs, g64) <= 2.0 ** -23
    if arith == "f16x2":
        assert C.amax_value(gs._ndet_amax) == float(gs.abs().max()), "the slot on g' is not its maximum"
    ref = R.dx_conv(g64, w, 1, grid)
    elem, rms = _check_bars(f"{name} {arith}", dx, ref)
    print(f"DGRAD-AUTO {name} {arith} ran {names[0]} x {resolved[0][1]}: elem {elem:.2e} rel-rms {rms:.2e}")


@pytest.mark.parametrize("arith", ARITHS, indirect=True)
def test_autograd_head_shared_convolution(device, arith):
    """conv_train.conv_forward_shared: three layers 128 -> 1 + 6 + 18 as one convolution; dx is the sum of the three layers' data gradients."""
    from torch import nn
    from nerfdet_amd import conv_train
    name = "head-128to25"
    module, cin, cout, kernel, stride, grid = R.AUTOGRAD[name]
    torch.manual_seed(21)
    convs = [nn.Conv3d(cin, c, 3, padding=1, bias=(c == 18)).to(device) for c in R.HEAD_SPLIT]
    for c in convs:
        c.weight.requires_grad_(False)
    x = torch.randn(*grid, cin, device=device)
    dys = [R.gradient_like(grid, c, 30 + c).to(device) for c in R.HEAD_SPLIT]
    xg = x.permute(3, 0, 1, 2).unsqueeze(0).requires_grad_(True)           # logical (1, C, X, Y, Z) on channels-last memory
    outs = conv_train.conv_forward_shared(convs, xg)
    assert [tuple(o.shape) for o in outs] == [(1, c) + tuple(grid) for c in R.HEAD_SPLIT]
    loss = sum((o[0].permute(1, 2, 3, 0) * d).sum() for o, d in zip(outs, dys))
    _poison(device, math.prod(grid) * 32, math.prod(grid) * cin)
    with watched() as (names, resolved), conv_outputs() as outs:
        loss.backward()
    _dx_launch_is_predicted(name, arith, names, resolved)
    _dx_slots_are_exact(outs, arith)
    ref = sum(R.dx_conv(d, c.weight.detach(), 1, grid) for d, c in zip(dys, convs))
    elem, rms = _check_bars(f"{name} {arith}", xg.grad[0].permute(1, 2, 3, 0), ref)
    print(f"DGRAD-AUTO {name} {arith} ran {names[0]} x {resolved[0][1]}: elem {elem:.2e} rel-rms {rms:.2e}")


SCALE_EXP = -20


def _scaled_reference_is_normal(ref):
    """Nothing of the scaled result leaves the normal fp32 range (checked on the reference, with 2^20 to spare for the partial products)."""
    nz = ref[ref != 0].abs()
    assert float(nz.min()) * 2.0 ** (2 * SCALE_EXP) > torch.finfo(torch.float32).tiny and float(nz.max()) < 1e30


@pytest.mark.parametrize("arith", ARITHS, indirect=True)
@pytest.mark.parametrize("name", ["s1-3d-96to25", "s2-3d-64to128", "t2-128to32", "affine-2d-128to64"])
def test_power_of_two_scaling_commutes_bit_for_bit(device, name, arith):
    """dy 2^-20 gives dx and dW times 2^-20, bit for bit: every scale of both schemes is a power of two read from a slot, so the slot of a
    gradient-sized tensor (max ~ 1e-6) is read, tagged and carried as that of an O(1) tensor is (tests/test_stem_gpu.py makes the statement for the stem)."""
    from nerfdet_amd import autograd as A
    s = 2.0 ** SCALE_EXP
    prev = A.set_deterministic(name.startswith("s2"))
    try:
        if name.startswith("affine"):
            dy = _affine(name, device)[5]
            _, dx, dw, d_res, _, _, _ = _affine_backward(name, device, dy, want_dw=True)
            _, dx_s, dw_s, d_res_s, gs, _, _ = _affine_backward(name, device, dy * s, want_dw=True)
            assert torch.equal(d_res_s, d_res * s)
            small = float(gs.abs().max())
            x, w, scale, _, _, _ = _affine(name, device)
            ref = R.dx_conv(R.affine_act_bwd(dy, _affine_backward(name, device, dy)[0], scale, True)[0], w, 1, tuple(x.shape[:3]))
        else:
            dy, ref = _auto(name, device)[2:4]
            dx, dw, _, _ = _backward(name, device, dy, want_dw=True)
            dx_s, dw_s, _, _ = _backward(name, device, dy * s, want_dw=True)
            small = float((dy * s).abs().max())
    finally:
        A.set_deterministic(prev)
    assert small < 2.0 ** -10, "the scaled gradient is gradient-sized"
    _scaled_reference_is_normal(ref)
    _scaled_reference_is_normal(dx.double())
    _scaled_reference_is_normal(dw.double())
    assert torch.equal(dx_s, dx * s), f"dx: {_differs(dx_s, dx * s)}"
    assert torch.equal(dw_s, dw * s), f"dW: {_differs(dw_s, dw * s)}"


# ---- (d) degenerate gradients ----
def _ctx(kernel, stride):
    return types.SimpleNamespace(needs_input_grad=(True, False), kernel=tuple(kernel), stride=stride, adjoint=None)


@pytest.mark.parametrize("arith", ARITHS, indirect=True)
@pytest.mark.parametrize("cout", [25, 64])
def test_all_zero_dy(device, cout, arith):
    """Every ReLU dead: dx is exactly zero and finite through _conv_grads (stride 1) and _dgrad_strided (the deterministic detour), in f16x2 with a zero
    slot going in (Cout 64: tagged on dy; Cout 25: F.pad drops the tag and amax_of finds 0) and the exact, zero, slot coming out."""
    from nerfdet_amd import autograd as A, conv3d as C, conv_train
    cin, kernel, grid = 64, (3, 3, 3), (7, 9, 5)
    w = R.kaiming(cout, cin, kernel, 3).to(device)
    x = torch.randn(*grid, cin, device=device)
    for stride in (1, 2):
        og = R.out_grid(grid, kernel, stride)
        g = torch.zeros(*og, cout, device=device)
        if arith == "f16x2" and cout % 32 == 0:
            C._tag_amax(g, C.AMAX.take(device), produced=False)
        _poison(device, math.prod(grid) * R.padded(cout), math.prod(grid) * cin, math.prod(og) * R.padded(cout))
        prev = A.set_deterministic(True)
        try:
            with watched() as (names, resolved):
                dx, dw = conv_train._conv_grads(_ctx(kernel, stride), x, w, g)
        finally:
            A.set_deterministic(prev)
        assert dw is None and len(names) == 1 and names[0].endswith("/f16x2") == (arith == "f16x2")
        assert tuple(dx.shape) == tuple(grid) + (cin,) and bool(torch.isfinite(dx).all())
        assert not bool((dx != 0).any()), f"stride {stride}: {int((dx != 0).sum())} non-zero elements of a zero gradient"
        if arith == "f16x2":
            _slot_is_exact(dx)
            assert C.amax_value(dx._ndet_amax) == 0.0


IMPULSE_CASES = {
    # name: (layer Cin, layer Cout, kernel, stride, input grid)
    "3d": (64, 25, (3, 3, 3), 1, (4, 5, 6)),
    "2d": (64, 25, (3, 3), 1, (2, 5, 6)),               # N = 2: the other image stays zero
    "3d-stride2": (64, 25, (3, 3, 3), 2, (7, 9, 5)),    # the deterministic detour; output grid 4 x 5 x 3
}


def impulse_points(og, two_d=False):
    """The 8 corners of the output grid and its centre (2D: the corners of both images)."""
    ends = [(0, n - 1) for n in og]
    return [(a, b, c) for a in ends[0] for b in ends[1] for c in ends[2]] + [tuple(n // 2 for n in og)]


def impulse_slab(w, pt, stride, grid):
    """dx of a unit impulse in channel 24 at output position ``pt``: the weight slab w[24, :, t] at input position s o + t - p, clipped at the border
    (2D: within the impulse's image only)."""
    kernel = tuple(w.shape[2:])
    k3 = (1,) + kernel if len(kernel) == 2 else kernel
    s3 = (1, stride, stride) if len(kernel) == 2 else (stride,) * 3
    wt = w[24].reshape(w.shape[1], *k3)
    out = torch.zeros(*grid, w.shape[1], dtype=w.dtype, device=w.device)
    for a in range(k3[0]):
        for b in range(k3[1]):
            for c in range(k3[2]):
                i = tuple(s * o + t - k // 2 for s, o, t, k in zip(s3, pt, (a, b, c), k3))
                if all(0 <= v < n for v, n in zip(i, grid)):
                    out[i] = wt[:, a, b, c]
    return out


@pytest.mark.parametrize("arith", ARITHS, indirect=True)
@pytest.mark.parametrize("name", list(IMPULSE_CASES))
def test_impulses(device, name, arith):
    from nerfdet_amd import autograd as A, conv_train
    cin, cout, kernel, stride, grid = IMPULSE_CASES[name]
    w = R.grid_weights(cout, cin, kernel, seed=5).to(device)
    x = torch.zeros(*grid, cin, device=device)
    og = R.out_grid(grid, kernel, stride)
    wrong = []
    prev = A.set_deterministic(True)
    try:
        for pt in impulse_points(og, len(kernel) == 2):
            g = torch.zeros(*og, cout, device=device)
            g[pt + (24,)] = 1.0
            _poison(device, math.prod(grid) * 32, math.prod(grid) * cin, math.prod(og) * 32)
            with watched() as (names, resolved):
                dx, _ = conv_train._conv_grads(_ctx(kernel, stride), x, w, g)
            assert len(names) == 1 and names[0].endswith("/f16x2") == (arith == "f16x2")
            want = impulse_slab(w, pt, stride, grid)
            assert 0 < int((want != 0).any(dim=-1).sum()) <= math.prod(kernel)
            if not torch.equal(dx, want):
                wrong.append((pt,) + _differs(dx, want))
    finally:
        A.set_deterministic(prev)
    assert not wrong, f"(impulse position, differing elements, max |dx - weight slab|): {wrong}"


# ---- what the CPU file checks the reference at ----
def conv_shapes():
    """{(layer Cin, layer Cout, kernel, stride, input grid)} of every convolution case of this file."""
    shapes = {(cin, cout, k, 1, g) for cin, cout, k, g in {**R.LADDER, **R.LADDER_1X1}.values()}
    shapes |= {real_shape(t, s)[:3] + (1,) + real_shape(t, s)[3:] for t, s in REAL_ROWS}
    for module, cin, cout, k, stride, g in R.AUTOGRAD.values():
        if module == "shared":
            shapes |= {(cin, c, k, stride, g) for c in R.HEAD_SPLIT}
        elif module != "ConvT2":
            shapes.add((cin, cout, k, stride, g))
    shapes |= {(cin, cout, k, s, g) for cin, cout, k, s, g in IMPULSE_CASES.values()}
    shapes |= {(64, c, (3, 3, 3), s, (7, 9, 5)) for c in (25, 64) for s in (1, 2)}
    return shapes


def t2_shapes():
    return set(R.LADDER_T2.values()) | {(cin, cout, g) for module, cin, cout, k, s, g in R.AUTOGRAD.values() if module == "ConvT2"}
