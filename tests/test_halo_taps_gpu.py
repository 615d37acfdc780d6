"""Tile 3128 (csrc/conv_split_kernels.hip: k_conv_split_halo<4,2>) with THREE taps per barrier interval -- the fp16-pair (SCH 1) and one-plane
bf16 (SCH 2) instantiations with SPL_TPS3, taken when the staged image's taps come in threes -- against the one-tap walk of the SAME build
(ndet_conv_halo_taps(1, ...), test support).  The layers are those of mmdet3d/models/necks/imvoxelnet.py:36-67,233-260, dense_heads/
imvoxel_head_v2.py:45-49 and the ResNet/FPN 3x3 behind detectors/nerfdet.py:140, at the smallest shapes that reach a distinct branch of the walk.

Every accumulator sees the same MFMA sequence in both walks (tap-major, the planes, products and tiles of the one-tap loop in its order), so the
claim is bit equality, not a tolerance.  Per case and arithmetic:

* the output's BITS are equal (int32 view: NaN positions and payloads included), and so are the launch's max |out|, its smallest tile maximum
  (amax slot words 0 and 1) and the guard word where the launch commits them (f16x2);
* f16x2 is held to the fp64 bound of tests/test_f16x2_gpu.py: rel-rms error against the fp64 convolution on the CPU no more than 2 x that of the
  exact fp32-MFMA kernel (ndet_conv_ndhwc) on the same layer.  Not asserted on the row with Inf / NaN inputs: the reference is not finite there;
* bf16x3 has no three-tap instantiation and must be bit-identical because it still runs the one-tap loop; the launcher's own rule
  (ndet_conv_halo_taps query) says which walk a row takes: 3 for f16x2 / bf16 on every row but the 1x5x1 one (Tin = 5), 1 for bf16x3.

Cases (what each reaches):
  a  32->128, 1x5x7, 3x3                one chunk, three intervals: less than would fill a pipeline; ragged patch
  b  96->160, 3x4x5, 3x3x3              depth taps inside the image (Tin = 27, nine intervals per chunk); three chunks: the stage parity flips at every
                                        P2 (nine is odd); second column tile 32 wide
  c  64->128, 1x8x16, 3x3x3             the looped-depth form (KDL = 3, Tin = 9; asserted through ndet_conv_halo_patch); depth masks at both faces
  d  192->136, 3x4x5, 3x3x3, splits 2, 4   uneven chunk ranges per split (6 chunks over 4), partial slabs + the reduce launch
  e  3 volumes of 3x6x10, 64->128, splits 1, 2   the batch form: volume index in the offsets and output rows
  f  64->128, 4x9x5, kernel 3x1x3, residual then ReLU (mixed extents, Tin = 9); 64->25, 10x10x4, 3x3x3 (the scalar-column epilogue; the looped-depth form on a real depth);
     64->128, 3x7x5, kernel 1x5x1 (Tin = 5: the one-tap fallback inside the same launch function)
  g  case b with one all-zero chunk; and with one +Inf and one NaN input voxel on top of it

Measured on an MI355X: all 36 rows bit-identical; rel-rms f16x2 / fp32-MFMA kernel (ratio, bound 2): a 1.65e-07 / 1.82e-07 (0.91), b 4.06e-07 /
4.58e-07 (0.89), c 2.36e-07 / 2.55e-07 (0.93), d 4.83e-07 and 3.65e-07 / 8.36e-07 (0.58, 0.44), e 3.77e-07 and 2.72e-07 / 4.20e-07 (0.90, 0.65),
f 1.91e-07 / 2.22e-07 (0.86), 4.18e-07 / 4.46e-07 (0.94), 1.89e-07 / 2.12e-07 (0.89), g (zero chunk) 3.26e-07 / 3.95e-07 (0.82).
"""
import copy
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu

TILE = 3128
CASES = {
    # name: (cin, cout, volumes (0: the plain form), grid, kernel, relu, residual, input kind)
    "a-one-chunk-2d": (32, 128, 0, (1, 5, 7), (1, 3, 3), 0, 0, "relu"),
    "b-depth-inside": (96, 160, 0, (3, 4, 5), (3, 3, 3), 0, 0, "relu"),
    "c-depth-looped": (64, 128, 0, (1, 8, 16), (3, 3, 3), 0, 0, "relu"),
    "d-split-k": (192, 136, 0, (3, 4, 5), (3, 3, 3), 0, 0, "relu"),
    "e-batch": (64, 128, 3, (3, 6, 10), (3, 3, 3), 0, 0, "relu"),
    "f-3x1x3-res-relu": (64, 128, 0, (4, 9, 5), (3, 1, 3), 1, 1, "relu"),
    "f-scalar-columns": (64, 25, 0, (10, 10, 4), (3, 3, 3), 0, 0, "relu"),
    "f-1x5x1-fallback": (64, 128, 0, (3, 7, 5), (1, 5, 1), 0, 0, "relu"),
    "g-zero-chunk": (96, 160, 0, (3, 4, 5), (3, 3, 3), 0, 0, "zero-chunk"),
    "g-inf-nan-zero-chunk": (96, 160, 0, (3, 4, 5), (3, 3, 3), 0, 0, "nonfinite"),
}
SPLITS = {"d-split-k": (2, 4), "e-batch": (1, 2)}
LOOPED = {"c-depth-looped", "f-scalar-columns"}      # the rows whose depth taps are looped outside the image (a 2 x 16 x 4 patch on 10x10x4)
ROWS = [(name, s) for name in CASES for s in SPLITS.get(name, (1,))]
ARITH_ID = {"bf16x3": 0, "f16x2": 1, "bf16": 2}


def _rel_rms(a, ref):
    a, ref = a.double().cpu(), ref.double()
    return ((a - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


class _Layer:
    """One layer on the CPU with its fp64 result: built once per case, shared, never changed."""

    def __init__(self, name):
        cin, cout, n, grid, kernel, relu, res, kind = CASES[name]
        torch.manual_seed(4242 + sorted(CASES).index(name))
        self.cin, self.cout, self.n, self.grid, self.kernel, self.relu = cin, cout, n, grid, kernel, relu
        self.conv = nn.Conv3d(cin, cout, kernel, 1, tuple(k // 2 for k in kernel), bias=False)
        self.bn = nn.BatchNorm3d(cout).eval()
        with torch.no_grad():
            self.bn.weight.uniform_(0.5, 1.5); self.bn.bias.normal_(0, 0.2); self.bn.running_mean.normal_(0, 0.2); self.bn.running_var.uniform_(0.5, 1.5)
        vols = max(n, 1)
        self.x = torch.relu(torch.randn(vols, *grid, cin)) * torch.exp(torch.randn(vols, *grid, 1))     # post-ReLU-like, magnitudes over e^+-3
        if kind in ("zero-chunk", "nonfinite"):
            self.x[..., 32:64] = 0.0
        if kind == "nonfinite":
            self.x[0, 1, 2, 3, 5] = float("inf")
            self.x[0, 2, 0, 1, 70] = float("nan")
        self.finite = kind != "nonfinite"
        self.res = torch.randn(vols, *grid, cout) if res else None
        with torch.no_grad():
            y = self.bn.double()(self.conv.double()(self.x.permute(0, 4, 1, 2, 3).double())).permute(0, 2, 3, 4, 1)
            self.conv.float(); self.bn.float()
            if self.res is not None:
                y = y + self.res.double()
            self.ref = (F.relu(y) if relu else y).contiguous()

    def on(self, device):
        from nerfdet_amd import conv3d as C
        if not hasattr(self, "_dev"):
            conv_d, bn_d = copy.deepcopy(self.conv).to(device), copy.deepcopy(self.bn).to(device)
            x = self.x.to(device) if self.n else self.x[0].to(device)
            res = None if self.res is None else (self.res.to(device) if self.n else self.res[0].to(device))
            self._dev = (conv_d, bn_d, C.packed([conv_d], bn_d), x.contiguous(), None if res is None else res.contiguous())
        return self._dev[3], self._dev[2], self._dev[4]


@functools.lru_cache(maxsize=None)
def _layer(name):
    return _Layer(name)


def _switch(mode):
    from nerfdet_amd import _lib
    _lib.check(_lib.load().ndet_conv_halo_taps(mode, 0, 0, 0, None, None), "conv_halo_taps")


def _launch(device, lay, arith, splits, one_tap):
    """One launch of ``lay`` on tile 3128 in ``arith`` under the switch; (out, (amax, tile minimum) of its slot or None, guard word or None)."""
    from nerfdet_amd import conv3d as C, conv_tiles
    x, pk, res = lay.on(device)
    vols, taps = max(lay.n, 1), lay.kernel[0] * lay.kernel[1] * lay.kernel[2]
    m = vols * lay.grid[0] * lay.grid[1] * lay.grid[2]
    out = torch.empty(tuple(x.shape[:-1]) + (lay.cout,), dtype=torch.float32, device=device)
    names, resolved = [], []
    real_resolve = conv_tiles.resolve

    def hook(flops, thunk, name):
        names.append(name)
        return thunk()

    def resolve(*a, **kw):
        resolved.append(real_resolve(*a, **kw))
        return resolved[-1]
    prev, prev_hook = C.set_arithmetic(arith), C.launch_hook
    try:
        C.launch_hook, conv_tiles.resolve = hook, resolve
        _switch(1 if one_tap else 0)
        C.guard_begin(device)
        with torch.no_grad():
            y = C._conv_split(x, pk, out, lay.grid, lay.kernel, (1, 1, 1), tuple(k // 2 for k in lay.kernel), False, res, False, lay.relu, splits, TILE,
                              m, taps * (lay.cin // 32), 2 * m * lay.cout * lay.cin * taps, batch=vols)
        torch.cuda.synchronize()
        slot = (C.amax_value(y._ndet_amax), C.tilemin_value(y._ndet_amax)) if arith == "f16x2" else None
        gw = C.guard_word(device)
        word = int(gw.item()) if (arith == "f16x2" and gw is not None) else None
    finally:
        _switch(0)
        C.set_arithmetic(prev)
        C.launch_hook, conv_tiles.resolve = prev_hook, real_resolve
    assert len(names) == 1 and names[0].startswith(conv_tiles.TILES[TILE].name + ("/f16x2" if arith == "f16x2" else "")), names
    assert resolved == [(TILE, splits)], resolved
    return y, slot, word


def _f32_kernel(device, lay):
    """The exact fp32-MFMA kernel (ndet_conv_ndhwc) on the same layer, volume by volume."""
    from ctypes import c_void_p
    from nerfdet_amd import _lib
    from nerfdet_amd._lib import _ptr, i3, raw_stream
    x, pk, res = lay.on(device)
    lib, st = _lib.load(), c_void_p(raw_stream(device))
    xs = x if lay.n else x.unsqueeze(0)
    rs = None if res is None else (res if lay.n else res.unsqueeze(0))
    out = torch.empty(tuple(xs.shape[:-1]) + (lay.cout,), dtype=torch.float32, device=device)
    for v in range(xs.shape[0]):
        _lib.check(lib.ndet_conv_ndhwc(_ptr(xs[v]), _ptr(pk.w), _ptr(out[v]), *lay.grid, lay.cin, lay.cout, i3(*lay.kernel), i3(1, 1, 1),
                                       i3(*(k // 2 for k in lay.kernel)), _ptr(pk.scale), _ptr(pk.shift), _ptr(None if rs is None else rs[v]), 0, lay.relu,
                                       1, 64, None, st), "conv_ndhwc")
    torch.cuda.synchronize()
    return out if lay.n else out[0]


def _taps_rule(lay, arith):
    """(taps per interval the launcher's rule gives this row, LDS bytes of its walk, looped-depth form?)"""
    from nerfdet_amd import _lib
    lib = _lib.load()
    patch, looped = (ctypes.c_int * 3)(), ctypes.c_int()
    _lib.check(lib.ndet_conv_halo_patch(TILE, *lay.grid, (ctypes.c_int * 3)(*lay.kernel), patch, ctypes.byref(looped)), "conv_halo_patch")
    tin = lay.kernel[0] * lay.kernel[1] * lay.kernel[2] // (lay.kernel[0] if looped.value else 1)
    taps, lds = ctypes.c_int(), ctypes.c_int()
    _lib.check(lib.ndet_conv_halo_taps(-1, TILE, ARITH_ID[arith], tin, ctypes.byref(taps), ctypes.byref(lds)), "conv_halo_taps")
    return taps.value, lds.value, bool(looped.value)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("arith", ["f16x2", "bf16", "bf16x3"])
@pytest.mark.parametrize("name,splits", ROWS, ids=[f"{n}-sp{s}" for n, s in ROWS])
def test_three_taps_per_interval_equal_the_one_tap_walk(device, name, splits, arith):
    lay = _layer(name)
    taps, lds, looped = _taps_rule(lay, arith)
    assert looped == (name in LOOPED)
    assert taps == (3 if arith != "bf16x3" and name != "f-1x5x1-fallback" else 1) and lds <= 160 * 1024
    want, want_slot, want_word = _launch(device, lay, arith, splits, one_tap=True)
    got, slot, word = _launch(device, lay, arith, splits, one_tap=False)
    assert tuple(got.shape) == tuple(lay.ref.shape[0 if lay.n else 1:])
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert _same_bits(got, want), f"{int((got.view(torch.int32) != want.view(torch.int32)).sum())} elements differ from the one-tap walk"
    assert slot == want_slot or (slot != slot and want_slot != want_slot), (slot, want_slot)
    assert word == want_word, (word, want_word)
    if lay.finite:
        assert bool(torch.isfinite(got).all())
        if arith == "f16x2":
            assert slot[0] == float(got.abs().max()), "the launch's max |out| slot is not the tensor's maximum"
    else:
        assert bool(torch.isnan(got).any()), "the NaN voxel did not reach the output"
    if arith == "f16x2" and lay.finite:
        ref = lay.ref if lay.n else lay.ref[0]
        err16, err32 = _rel_rms(got, ref), _rel_rms(_f32_kernel(device, lay), ref)
        print(f"{name} splits {splits}: rel-rms f16x2 {err16:.3e}  fp32-MFMA {err32:.3e}  ratio {err16 / err32:.2f}")
        assert err16 <= 2.0 * err32, (err16, err32)
