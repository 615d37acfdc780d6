"""The two kernels that compute operand scales INSIDE the launch, from a workgroup's own maximum, and do their own border handling: the whole stage-1
bottleneck in one launch (csrc/bottleneck_kernels.hip, k_bottleneck_f16x2<DS, NCH>: 4 x 16 patches with a one-pixel halo, the halo pixels outside the
image masked by the kernel itself) and conv -> BN -> ReLU -> 1x1 conv -> BN -> residual -> ReLU in one launch (csrc/conv_split_kernels.hip,
k_conv_split_chain<64|128, SCH>: 128-row tiles, rows past M left to the buffer descriptors' bounds).  Replaces mmdet's Bottleneck.forward behind
mmdet3d/models/detectors/nerfdet.py:140.  The single-layer tile families are held by tests/test_f16x2_edges_gpu.py; this file holds these two.

The reference is always the same Bottleneck (nerfdet_amd/backbone.py) or Conv2d / BatchNorm2d pair, deep-copied to fp64 and run on the CPU, built once
per shape (functools.lru_cache) and shared unchanged.  What is held to what:

* every fp16-pair result: elementwise |got - ref| <= 2e-5 max(1, max|ref|), rel-rms < 1e-6, rel-rms <= 1.15 x the rel-rms of the launches the kernel
  replaces (the bottleneck: conv3d.FUSE_BOTTLENECKS = False; the chain: two conv2d_nhwc launches), the max |out| slot exact, a second launch the same
  bits, and conv3d.launch_hook saw exactly one launch of the named kernel;
* A  borders: H in {1, 4, 5} x W in {1, 15, 16, 17, 33} x N in {1, 3}, identity and downsample form, BN1's shift at +5 so that relu(bn1(0)) is far from 0
     and a halo pixel that is not forced to zero moves the border outputs by O(1);
* B  bit for bit (torch.equal): a stacked launch == its single-image launches (N = 3 and N = 11: 66 patches, no multiple of 8), a patch of a
     patch-aligned crop == the same patch of the full map, a patch unchanged by rows 2^20 times larger outside its halo window, and
     block(x 2^k) == block(x) 2^k for k = -40, +40 with every BN shift at zero;
* C  zero intermediates (the eb < 30 clamp of conv_xscale_of on ymax1 / ymax2): an all-zero x, one dead patch (proved dead on the fp64 reference), and
     all-zero x with every shift <= 0 (the output and its slot are exactly 0);
* D  three images 1, 2^-6, 2^-12 in one tensor: EACH image's own rel-rms < 1e-6, fused and two-launch.  The spread is a condition: an emulation of
     the operand scheme alone (hi / lo fp16 of x and w under the tensor's power of two, the three products exact in fp64) keeps the dimmest image's
     conv1 output below 1e-7 rel-rms (measured on the CPU: 5.6e-8 / 5.6e-8 / 5.8e-8 for the three images), so 2^-6 per image did not have to be narrowed;
* E  the identity form at (2, 128, 128): the output is exactly 32 << 20 bytes, the kernel's own non-temporal store threshold (it does not follow the
     nt_bytes knob), 2048 patches;
* F  the range guard on forward_nhwc (clear on ordinary and on uniformly 3e7 x brighter x, set with one image of two 3e7 x brighter), a whole
     stage of three blocks (three launches, ONE amax fallback pass: blocks 2 and 3 read the slot the previous launch left), and the guard across a
     hand-off (the tile minimum block 1's patches committed is what block 2's guard reads: set for a dim image, clear for a uniformly bright tensor --
     "none recorded" would set it);
* G  the chained kernel's tile and column edges (M = 1, 128, 135, 64, 65, 129, 189; Cout 64, 192, 320; one K chunk; stride 2 on odd extents) in three
     arithmetics: f16x2 as above; bf16x3 elementwise only (rel-rms printed); bf16 within 4e-6 max(1, max|ref|) of the two bf16 launches;
* H  the chained kernel bit for bit: homogeneity (k = -40, +40; f16x2 and bf16x3), stacked == single images, nt_bytes = 0 == the default threshold;
     and a first tile whose intermediate is exactly zero (proved on the fp64 reference), and an all-zero x;
* I  ndet_bottleneck_f16x2 / ndet_conv_chain reject one bad argument at a time before any launch: documented code, a message naming the entry
     point, the sentinel-filled output untouched.

Homogeneity at |k| = 40 stays clear of fp32 subnormals; checked on the CPU per stage: (smallest non-zero |input|) 2^-40 (smallest non-zero |w|)
(smallest |BN scale|) >= 2^-126, and the smallest non-zero |output| 2^-40 likewise.  |k| did not have to be reduced.

Measured on an MI355X (elementwise error / max(1, max|ref|), rel-rms; "two": the rel-rms of the launches the kernel replaces; worst row of a sweep):

    fused bottleneck                                     elem      rel-rms   two       fused/two
    A  identity, 30 shapes (worst of each column)        2.31e-07  2.14e-07  2.44e-07  0.80 .. 1.00
    A  downsample, 30 shapes                             2.91e-07  1.83e-07  2.27e-07  0.76 .. 1.05
    C.1 zero image, identity / downsample                1.00e-07  7.88e-08  8.98e-08  0.88 / 0.97
    C.2 dead patch, identity / downsample                1.22e-07  1.03e-07  1.09e-07  0.97 / 0.94
    D  rel-rms of image 0 / 1 / 2 (1, 2^-6, 2^-12)       fused 4.18e-08 / 4.19e-08 / 4.14e-08, two launches 4.68e-08 / 4.73e-08 / 4.67e-08
    E  (2, 128, 128), non-temporal                       3.67e-08  4.35e-08  4.72e-08  0.92
    F.2 stage of three blocks (2, 13, 37)                2.42e-07  1.08e-07  1.15e-07  0.93

    chained kernel (cin-mid-cout-nhw)                    elem      rel-rms   two       f16x2/two  bf16x3 elem  bf16x3 rel-rms (printed)
    64-64-64-1x1x1-k3s1-res1-relu1                       1.02e-07  6.56e-08  6.38e-08  1.03       1.02e-07     6.55e-08
    64-64-192-1x8x16-k3s1-res1-relu1                     1.00e-07  6.15e-08  6.20e-08  0.99       1.30e-07     7.07e-08
    64-64-256-1x9x15-k3s1-res0-relu0                     2.38e-07  1.23e-07  1.25e-07  0.99       2.40e-07     1.45e-07
    32-64-128-2x9x11-k1s1-res1-relu2                     1.47e-07  4.53e-08  4.47e-08  1.01       1.40e-07     4.47e-08
    128-128-320-1x8x8-k3s1-res1-relu1                    1.12e-07  8.03e-08  8.03e-08  1.00       1.75e-07     9.80e-08
    128-128-512-1x5x13-k3s1-res1-relu1                   1.56e-07  9.01e-08  9.01e-08  1.00       1.71e-07     1.03e-07
    128-128-64-1x3x43-k3s1-res0-relu1                    3.75e-07  1.51e-07  1.51e-07  1.00       3.83e-07     1.84e-07
    128-128-512-3x13x17-k3s2-res1-relu1                  1.91e-07  8.16e-08  8.16e-08  1.00       2.58e-07     9.80e-08
    H.3 zero first tile, mid 64 / 128                    1.57e-07  6.98e-08  6.98e-08  1.00
    H.3 zero x, mid 64 / 128                             6.74e-08  3.38e-08  3.38e-08  1.00

bf16: the chained launch gave the bits of the two bf16 launches on every row (difference 0).  Every exact property held: no row needed a narrower
input, and no defect was found in either kernel.
"""
import copy
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu

ELEM_BAR, RMS_BAR, RATIO_BAR, BF16_BAR = 2e-5, 1e-6, 1.15, 4e-6
FUSED, TINY = "k_bottleneck/f16x2", 2.0 ** -126


# ------------------------------------------------------------------ shared helpers ------------------------------------------------------------------
def _errors(got, ref):
    """(max |got - ref| / max(1, max|ref|), rel-rms) against the fp64 result."""
    assert tuple(got.shape) == tuple(ref.shape)
    d = got.double().cpu() - ref
    return float(d.abs().max()) / max(1.0, float(ref.abs().max())), (d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


def _slot_is_exact(got):
    from nerfdet_amd import conv3d as C
    assert C.amax_value(got._ndet_amax) == float(got.abs().max()), "the launch's max |out| slot is not the tensor's maximum"


def _ulps(a, b):
    """Largest distance between two fp32 tensors in units in the last place (ordered-integer view)."""
    def key(t):
        i = t.detach().cpu().contiguous().view(torch.int32).long()
        return torch.where(i < 0, -(i & 0x7fffffff), i)
    return int((key(a) - key(b)).abs().max())


def _features(*shape):
    """Post-ReLU-like rows, one magnitude per pixel: relu(randn) * exp(0.5 randn)."""
    return torch.relu(torch.randn(*shape)) * torch.exp(0.5 * torch.randn(*shape[:-1], 1))


def _randomise(bn, shifts="random", spread=0.2, var=(0.5, 1.5)):
    """BatchNorm statistics as the existing tests draw them.  ``shifts``: "zero" (running_mean = bias = 0: the folded shift is exactly 0) or "nonpos"
    (running_mean = 0, bias <= 0: the folded shift is exactly the bias)."""
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5); bn.bias.normal_(0, spread); bn.running_mean.normal_(0, spread); bn.running_var.uniform_(*var)
        if shifts in ("zero", "nonpos"):
            bn.running_mean.zero_()
            bn.bias.zero_() if shifts == "zero" else bn.bias.copy_(-bn.bias.abs())


class _Hooked:
    """conv3d in ``arith`` with the launch hook recording kernel names (and FUSE_BOTTLENECKS as asked); everything restored on exit."""

    def __init__(self, arith, fuse=True):
        self.arith, self.fuse, self.names = arith, fuse, []

    def __enter__(self):
        from nerfdet_amd import conv3d as C
        self.prev = (C.set_arithmetic(self.arith), C.launch_hook, C.FUSE_BOTTLENECKS)

        def hook(flops, thunk, name):
            self.names.append(name)
            return thunk()
        C.launch_hook, C.FUSE_BOTTLENECKS = hook, self.fuse
        self.grad = torch.no_grad()
        self.grad.__enter__()
        return self.names

    def __exit__(self, *exc):
        from nerfdet_amd import conv3d as C
        self.grad.__exit__(*exc)
        try:
            if exc[0] is None:
                torch.cuda.synchronize()
        finally:
            C.set_arithmetic(self.prev[0])
            C.launch_hook, C.FUSE_BOTTLENECKS = self.prev[1], self.prev[2]
        return False


# ------------------------------------------------------------------ the fused bottleneck ------------------------------------------------------------------
def _bottleneck(ds, seed, shifts="random"):
    """A stage-1 Bottleneck in eval mode on the CPU: identity form (Cin 256) or downsample form (Cin 64).  ``shifts``: "random", "zero", "nonpos" (all
    four BatchNorms), "halo" (BN1's shift ~ +5), "dead" (BN1, BN2 <= 0, the others of mixed sign)."""
    from nerfdet_amd.backbone import Bottleneck
    torch.manual_seed(seed)
    down = nn.Sequential(nn.Conv2d(64, 256, 1, 1, bias=False), nn.BatchNorm2d(256)) if ds else None
    blk = Bottleneck(64 if ds else 256, 64, 1, down).eval()
    for m in blk.modules():
        if isinstance(m, nn.BatchNorm2d):
            _randomise(m, shifts if shifts in ("zero", "nonpos") else "random")
    with torch.no_grad():
        if shifts == "halo":
            blk.bn1.bias.normal_(5.0, 0.2)
        if shifts == "dead":
            _randomise(blk.bn1, "nonpos"); _randomise(blk.bn2, "nonpos")
    return blk


def _fp64(module, x):
    with torch.no_grad():
        return copy.deepcopy(module).double()(x.permute(0, 3, 1, 2).double()).permute(0, 2, 3, 1).contiguous()


class _BlockCase:
    """One block and one input on the CPU with the fp64 result; the device copy of the block (and the packs cached on it) is made once."""

    def __init__(self, blk, x):
        self.blk, self.x, self.ref = blk, x, _fp64(blk, x)

    def on(self, device):
        if not hasattr(self, "_dev"):
            self._dev = copy.deepcopy(self.blk).to(device)
        return self._dev


def _run_block(device, blk, x, fuse=True):
    """blk.forward_nhwc(x) in the fp16-pair arithmetic -> (out, kernel names the launch hook saw).  ``x`` on the CPU is copied (an untagged tensor)."""
    with _Hooked("f16x2", fuse) as names:
        y = blk.forward_nhwc(x if x.is_cuda else x.to(device))
    return y, names


def _fused_holds(tag, device, case):
    """The standard bars on one fused launch of ``case``; returns (out, elem, rms, two-launch rms)."""
    blk = case.on(device)
    got, names = _run_block(device, blk, case.x)
    assert names == [FUSED], names
    _slot_is_exact(got)
    again, _ = _run_block(device, blk, case.x)
    assert torch.equal(got, again), "the same launch twice gave different bits"
    two, names2 = _run_block(device, blk, case.x, fuse=False)
    assert FUSED not in names2 and len(names2) >= 2, names2
    (elem, rms), (elem2, rms2) = _errors(got, case.ref), _errors(two, case.ref)
    print(f"FUSED {tag}: elem {elem:.2e} rel-rms {rms:.2e} | two launches elem {elem2:.2e} rel-rms {rms2:.2e} | ratio {rms / rms2:.2f}")
    assert torch.isfinite(got).all()
    assert elem <= ELEM_BAR and rms < RMS_BAR and rms <= RATIO_BAR * rms2, (elem, rms, rms2)
    return got, elem, rms, rms2


@functools.lru_cache(maxsize=None)
def _border_block(ds):
    return _bottleneck(ds, 11 + ds, "halo")


@functools.lru_cache(maxsize=None)
def _border_case(ds, n, h, w):
    blk = _border_block(ds)
    with torch.no_grad():
        assert float(F.relu(blk.bn1(torch.zeros(1, 64, 1, 1))).min()) > 3.0, "relu(bn1(0)) must be far from 0"
    torch.manual_seed(1000 * n + 37 * h + w + ds)
    return _BlockCase(blk, _features(n, h, w, 64 if ds else 256))


@pytest.mark.parametrize("w", [1, 15, 16, 17, 33])
@pytest.mark.parametrize("h", [1, 4, 5])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("ds", [0, 1], ids=["identity", "downsample"])
def test_fused_bottleneck_borders(device, ds, n, h, w):
    """A: maps of one row / one column, one pixel short of a patch, exactly one, one past it, and three patches with a one-pixel tail, with
    relu(bn1(0)) ~ 5: conv2 pads ITS input with zeros, so a halo pixel outside the image that kept relu(bn1(0)) moves the border outputs by O(1)."""
    _fused_holds(f"A {'ds' if ds else 'id'} {n}x{h}x{w}", device, _border_case(ds, n, h, w))


@functools.lru_cache(maxsize=None)
def _plain_block(ds, shifts="random"):
    return _bottleneck(ds, 23 + ds, shifts)


@pytest.mark.parametrize("n", [3, 11])
@pytest.mark.parametrize("ds", [0, 1], ids=["identity", "downsample"])
def test_fused_bottleneck_images_are_independent(device, ds, n):
    """B.1: N images of 9 x 21 (3 x 2 patches each; N = 11: 66 patches, no multiple of the 8 XCDs), the same largest element planted in each so that
    the scale of x is the same in every run: the stacked launch equals the single-image launches image by image, bit for bit (the n, ty, tx
    decomposition of the patch index and the XCD remap)."""
    torch.manual_seed(31 + n + ds)
    x = _features(n, 9, 21, 64 if ds else 256)
    assert float(x.max()) < 64.0
    x[:, 4, 10, 7] = 64.0
    blk = copy.deepcopy(_plain_block(ds)).to(device)
    stacked, names = _run_block(device, blk, x)
    assert names == [FUSED]
    _slot_is_exact(stacked)
    for i in range(n):
        one, names = _run_block(device, blk, x[i:i + 1].contiguous())
        assert names == [FUSED]
        assert torch.equal(stacked[i:i + 1], one), f"image {i} of {n} differs from its own launch by {_ulps(stacked[i:i + 1], one)} ulp"


@pytest.mark.parametrize("ds", [0, 1], ids=["identity", "downsample"])
def test_fused_bottleneck_patches_are_local(device, ds):
    """B.2: a 20 x 80 map and its patch-aligned crop [4:16, 16:64] (3 x 3 patches), the tensor's maximum planted inside the crop's centre patch: that
    patch reads the same 6 x 18 halo window in both launches and scales its intermediates by its own maxima, so its outputs are the same bits."""
    torch.manual_seed(41 + ds)
    x = _features(1, 20, 80, 64 if ds else 256)
    assert float(x.max()) < 64.0
    x[0, 9, 40, 3] = 64.0
    blk = copy.deepcopy(_plain_block(ds)).to(device)
    full, names = _run_block(device, blk, x)
    crop, names_c = _run_block(device, blk, x[:, 4:16, 16:64].contiguous())
    assert names == [FUSED] and names_c == [FUSED]
    a, b = crop[:, 4:8, 16:32], full[:, 8:12, 32:48]
    assert torch.equal(a, b), f"the centre patch differs by {_ulps(a, b)} ulp"


@pytest.mark.parametrize("ds", [0, 1], ids=["identity", "downsample"])
def test_fused_bottleneck_patch_reads_only_its_halo_window(device, ds):
    """B.2, the other way round: everything OUTSIDE the 6 x 18 halo window of patch (ty 1, tx 1) of a 12 x 48 map replaced by rows 2^20 times larger,
    the tensor's maximum (2^26, planted in another patch) the same in both runs.  The patch's outputs are the same bits: its scales ys1 / ys2 come
    from its own 108 halo pixels and not from the rows 108 .. 127 that pad the halo image to four MFMA tiles (pixels below the window, were they
    read and left unmasked: a maximum 2^20 too large pushes the patch's low halves out of fp16)."""
    torch.manual_seed(43 + ds)
    c = 64 if ds else 256
    x, far = _features(1, 12, 48, c), 2.0 ** 20 * _features(1, 12, 48, c)
    far[:, 3:9, 15:33] = x[:, 3:9, 15:33]
    x[0, 0, 47, 3] = far[0, 0, 47, 3] = 2.0 ** 26
    assert float(x.max()) == 2.0 ** 26 and float(far.max()) == 2.0 ** 26
    blk = copy.deepcopy(_plain_block(ds)).to(device)
    (a, names_a), (b, names_b) = _run_block(device, blk, x), _run_block(device, blk, far)
    assert names_a == [FUSED] and names_b == [FUSED]
    a, b = a[:, 4:8, 16:32], b[:, 4:8, 16:32]
    assert torch.equal(a, b), f"the patch differs by {_ulps(a, b)} ulp"


def _block_stays_normal(blk, x, k):
    """No fp32 value the block forms from x 2^k is subnormal: per stage, (smallest non-zero |input|) 2^k (smallest non-zero |w|) (smallest |BN scale|),
    the smallest single term a sum can consist of, and the smallest non-zero |output| 2^k, on the fp64 reference."""
    b = copy.deepcopy(blk).double()
    with torch.no_grad():
        t = x.permute(0, 3, 1, 2).double()
        y1 = F.relu(b.bn1(b.conv1(t)))
        y2 = F.relu(b.bn2(b.conv2(y1)))
        out = _fp64(blk, x)
        stages = [(t, b.conv1, b.bn1), (y1, b.conv2, b.bn2), (y2, b.conv3, b.bn3)] + ([(t, b.downsample[0], b.downsample[1])] if b.downsample is not None else [])
        smallest = [float(out[out != 0].abs().min())]
        for inp, conv, bn in stages:
            w, s = conv.weight.abs(), (bn.weight / torch.sqrt(bn.running_var + bn.eps)).abs()
            smallest.append(float(inp[inp != 0].abs().min()) * float(w[w != 0].min()) * float(s.min()))
    return min(smallest) * 2.0 ** min(k, 0) >= TINY


@pytest.mark.parametrize("ds", [0, 1], ids=["identity", "downsample"])
def test_fused_bottleneck_is_homogeneous(device, ds):
    """B.3: every BN shift zero -> block(x 2^k) == block(x) 2^k bit for bit, k = -40 and +40: every scale the kernel derives (xs, ys1, ys2 and their
    inverses) is a power of two taken from a maximum that moves by exactly 2^k, so the fp16 pairs and the accumulators are the same numbers."""
    blk_c = _plain_block(ds, "zero")
    torch.manual_seed(53 + ds)
    x = _features(2, 9, 21, 64 if ds else 256)
    blk = copy.deepcopy(blk_c).to(device)
    base, names = _run_block(device, blk, x)
    assert names == [FUSED] and float(base.abs().max()) > 0
    bad = []
    for k in (-40, 40):
        assert _block_stays_normal(blk_c, x, k), f"2^{k} reaches fp32 subnormals: reduce |k|"
        got, names = _run_block(device, blk, x * 2.0 ** k)
        assert names == [FUSED]
        _slot_is_exact(got)
        want = base * 2.0 ** k
        if not torch.equal(got, want):
            bad.append(f"k = {k}: largest distance {_ulps(got, want)} ulp")
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("ds", [0, 1], ids=["identity", "downsample"])
def test_fused_bottleneck_of_a_zero_image(device, ds):
    """C.1: x all zeros (max |x| = 0: the scale derived from a zero slot is the eb < 30 clamp), random BN shifts: the block of a zero image."""
    case = _BlockCase(_plain_block(ds), torch.zeros(2, 5, 17, 64 if ds else 256))
    assert float(case.ref.abs().max()) > 0
    _fused_holds(f"C.1 zero image {'ds' if ds else 'id'}", device, case)


@pytest.mark.parametrize("ds", [0, 1], ids=["identity", "downsample"])
def test_fused_bottleneck_with_one_dead_patch(device, ds):
    """C.2: x zero on the 6 x 18 window of patch (ty 1, tx 1) of a 12 x 48 map, BN1 and BN2 shifts <= 0: that workgroup's halo image and its
    conv2 output are exactly zero (ymax1 == 0 and ymax2 == 0: both clamps taken, proved on the fp64 reference), its output is relu(shift3 + identity)."""
    blk = _bottleneck(ds, 61 + ds, "dead")
    torch.manual_seed(67 + ds)
    x = _features(1, 12, 48, 64 if ds else 256) + 0.01
    x[:, 3:9, 15:33] = 0.0
    b = copy.deepcopy(blk).double()
    with torch.no_grad():
        y1 = F.relu(b.bn1(b.conv1(x.permute(0, 3, 1, 2).double())))
        y2 = F.relu(b.bn2(b.conv2(y1)))
        assert float(y1[:, :, 3:9, 15:33].abs().max()) == 0.0 and float(y2[:, :, 4:8, 16:32].abs().max()) == 0.0, "the patch is not dead"
        assert float(y1.abs().max()) > 0 and float(y2.abs().max()) > 0
        zero = torch.zeros(1, 64, 1, 1, dtype=torch.float64)
        want = b.bn3(b.conv3(zero)) + (b.downsample(torch.zeros(1, 64, 1, 1, dtype=torch.float64)) if ds else 0.0)
        want = F.relu(want).permute(0, 2, 3, 1)                                      # relu(shift3 + identity): x is zero on the patch
        assert float(want.max()) > 0 and float(want.min()) == 0.0, "BN3's shifts must be of mixed sign"
    got, elem, rms, _ = _fused_holds(f"C.2 dead patch {'ds' if ds else 'id'}", device, _BlockCase(blk, x))
    dead = (got[:, 4:8, 16:32].double().cpu() - want).abs().max()
    assert float(dead) <= ELEM_BAR * max(1.0, float(want.abs().max())), float(dead)


@pytest.mark.parametrize("ds", [0, 1], ids=["identity", "downsample"])
def test_fused_bottleneck_all_zero_with_nonpositive_shifts(device, ds):
    """C.3: x all zeros and every shift <= 0: every intermediate and the output are exactly zero, and the slot reads 0."""
    from nerfdet_amd import conv3d as C
    blk = copy.deepcopy(_plain_block(ds, "nonpos")).to(device)
    got, names = _run_block(device, blk, torch.zeros(2, 5, 17, 64 if ds else 256))
    assert names == [FUSED]
    assert torch.equal(got, torch.zeros_like(got))
    assert C.amax_value(got._ndet_amax) == 0.0


def _pair_emulation(x, w):
    """The operand scheme alone: hi / lo fp16 of the rows ``x`` and the weight ``w`` under their tensor's power of two (max in [2^14, 2^15)), the three
    products hi hi + hi lo + lo hi exact in fp64."""
    def pair(t):
        s = math.ldexp(1.0, 15 - math.frexp(float(t.abs().max()))[1])
        v = t.float() * s
        hi = v.half()
        return hi.double(), (v - hi.float()).half().double(), s
    (xh, xl, sx), (wh, wl, sw) = pair(x), pair(w)
    return (xh @ wh.T + xh @ wl.T + xl @ wh.T) / (sx * sw)


SPREAD = 6      # image n is multiplied by 2^(-SPREAD n)


@functools.lru_cache(maxsize=None)
def _magnitude_case():
    torch.manual_seed(71)
    blk = _bottleneck(0, 73, "zero")
    x = _features(3, 12, 48, 256)
    for n in range(3):
        x[n] *= 2.0 ** (-SPREAD * n)
    return _BlockCase(blk, x)


def test_fused_bottleneck_magnitude_per_image(device):
    """D: images at 1, 2^-6 and 2^-12 in one tensor, every BN shift zero (each image's output scales with its input): EACH image's rel-rms against
    its own reference rms.  The fused kernel scales stages 2 and 3 per patch, the two-launch path scales conv1's output per tensor."""
    case = _magnitude_case()
    w1 = case.blk.conv1.weight.detach().view(64, 256)
    emu = _pair_emulation(case.x.view(-1, 256), w1).view(3, -1, 64)
    exact = (case.x.view(-1, 256).double() @ w1.double().T).view(3, -1, 64)
    for n in range(3):        # the condition on the spread, on the CPU: the operand scheme alone keeps conv1 of every image below 1e-7
        e = float((emu[n] - exact[n]).pow(2).mean().sqrt() / exact[n].pow(2).mean().sqrt())
        print(f"FUSED D emulation image {n}: conv1 rel-rms {e:.2e}")
        assert e < 1e-7, (n, e)
    blk = case.on(device)
    fused, names = _run_block(device, blk, case.x)
    assert names == [FUSED]
    _slot_is_exact(fused)
    two, _ = _run_block(device, blk, case.x, fuse=False)
    per = lambda got: [_errors(got[n], case.ref[n])[1] for n in range(3)]
    e_fused, e_two = per(fused), per(two)
    print("FUSED D per image rel-rms: fused " + " ".join(f"{e:.2e}" for e in e_fused) + " | two launches " + " ".join(f"{e:.2e}" for e in e_two))
    assert max(e_fused) < RMS_BAR and max(e_two) < RMS_BAR, (e_fused, e_two)


@functools.lru_cache(maxsize=None)
def _nt_case():
    torch.manual_seed(79)
    return _BlockCase(_plain_block(0), _features(2, 128, 128, 256))


def test_fused_bottleneck_non_temporal_stores(device):
    """E: the output of (2, 128, 128) x 256 channels is exactly 32 << 20 bytes, the threshold from which the kernel stores non-temporally; 2048
    patches: several times what is resident at once."""
    case = _nt_case()
    assert case.ref.numel() * 4 == 32 << 20
    _fused_holds("E non-temporal 2x128x128", device, case)


@pytest.mark.parametrize("ds", [0, 1], ids=["identity", "downsample"])
def test_range_guard_of_the_fused_bottleneck(device, ds):
    """F.1: the fused launch checks conv1 (and the downsample branch) against x as every fp16-pair launch does: floor and tile minimum."""
    from nerfdet_amd import conv3d as C
    torch.manual_seed(83 + ds)
    blk = copy.deepcopy(_plain_block(ds)).to(device)
    x = torch.relu(torch.randn(2, 24, 32, 64 if ds else 256))
    xb = x.clone()
    xb[0] *= 3.0e7                                      # one of the two maps 3e7 times brighter than the other
    for what, inp, want in (("ordinary", x, False), ("uniformly bright", x * 3.0e7, False), ("one bright image", xb, True)):
        C.guard_begin(device)
        _, names = _run_block(device, blk, inp)
        assert names == [FUSED]
        assert C.guard_tripped(device) == want, what


@functools.lru_cache(maxsize=None)
def _stage_case():
    from nerfdet_amd.backbone import Bottleneck
    torch.manual_seed(89)
    down = nn.Sequential(nn.Conv2d(64, 256, 1, 1, bias=False), nn.BatchNorm2d(256))
    stage = nn.Sequential(Bottleneck(64, 64, 1, down), Bottleneck(256, 64), Bottleneck(256, 64)).eval()
    for m in stage.modules():
        if isinstance(m, nn.BatchNorm2d):
            _randomise(m)
    return _BlockCase(stage, _features(2, 13, 37, 64))


def _run_stage(device, stage, x, fuse=True):
    with _Hooked("f16x2", fuse) as names:
        y = x.to(device)
        for blk in stage:
            y = blk.forward_nhwc(y)
    return y, names


def test_fused_stage_hands_the_slot_from_launch_to_launch(device):
    """F.2: three blocks in a row at (2, 13, 37): three launches; the untagged input takes the one ndet_amax_f32 pass, blocks 2 and 3 read the slot the
    previous launch's patches committed."""
    from nerfdet_amd import conv3d as C
    case = _stage_case()
    stage = case.on(device)
    before = C.amax_fallbacks
    got, names = _run_stage(device, stage, case.x)
    assert names == [FUSED] * 3, names
    assert C.amax_fallbacks == before + 1, (C.amax_fallbacks, before)
    _slot_is_exact(got)
    again, _ = _run_stage(device, stage, case.x)
    assert torch.equal(got, again)
    two, names2 = _run_stage(device, stage, case.x, fuse=False)
    assert FUSED not in names2
    (elem, rms), (_, rms2) = _errors(got, case.ref), _errors(two, case.ref)
    print(f"FUSED F.2 stage: elem {elem:.2e} rel-rms {rms:.2e} | two launches rel-rms {rms2:.2e} | ratio {rms / rms2:.2f}")
    assert elem <= ELEM_BAR and rms < RMS_BAR and rms <= RATIO_BAR * rms2, (elem, rms, rms2)


def test_range_guard_across_a_fused_hand_off(device):
    """F.3: block 2's guard reads the tile minimum block 1's patches committed with the maximum.  One image of two 3e7 times dimmer: set.  The same
    tensor uniformly bright: clear -- every patch recorded a maximum within 2^-16 of the tensor's (a launch that recorded none would read as set)."""
    from nerfdet_amd import conv3d as C
    case = _stage_case()
    stage = case.on(device)
    torch.manual_seed(97)
    x = torch.relu(torch.randn(2, 24, 32, 64))
    xb = x.clone()
    xb[0] *= 3.0e7
    ref1 = _fp64(case.blk[0], xb)
    assert float(ref1[1].abs().max()) < 2.0 ** -16 * float(ref1.abs().max()), "block 1's output of the dim image is not below the window"
    for inp, want in ((xb, True), (x * 3.0e7, False)):
        with _Hooked("f16x2") as names:
            C.guard_begin(device)
            y1 = stage[0].forward_nhwc(inp.to(device))
            C.guard_begin(device)
            before = C.amax_fallbacks
            stage[1].forward_nhwc(y1)
            assert C.amax_fallbacks == before, "block 2 did not read the slot block 1 left"
        assert names == [FUSED] * 2
        assert C.guard_tripped(device) == want, "one dim image" if want else "uniformly bright"


# ------------------------------------------------------------------ the chained kernel ------------------------------------------------------------------
class _ChainCase:
    """conv -> BN -> ReLU -> 1x1 conv -> BN -> (+ residual) -> ReLU on the CPU with its fp64 result."""

    def __init__(self, cin, mid, cout, nhw, k, stride, use_res, relu3, shifts="random"):
        torch.manual_seed(cin + 3 * mid + 5 * cout + 7 * k + stride + sum(nhw) + relu3)
        self.mid, self.relu3 = mid, relu3
        self.c2, self.c3 = nn.Conv2d(cin, mid, k, stride, k // 2, bias=False), nn.Conv2d(mid, cout, 1, bias=False)
        self.b2, self.b3 = nn.BatchNorm2d(mid).eval(), nn.BatchNorm2d(cout).eval()
        _randomise(self.b2, shifts, 0.3, (0.5, 2.0))
        _randomise(self.b3, "zero" if shifts == "zero" else "random", 0.3, (0.5, 2.0))
        self.x = _features(*nhw, cin)
        self.res = None
        if use_res:
            n, h, w = nhw
            self.res = torch.randn(n, (h + 2 * (k // 2) - k) // stride + 1, (w + 2 * (k // 2) - k) // stride + 1, cout)
        self.ref = self.forward(self.x)

    def middle(self, x):
        """relu(bn(conv(x))) in fp64, (N, mid, OH, OW)."""
        with torch.no_grad():
            return F.relu(copy.deepcopy(self.b2).double()(copy.deepcopy(self.c2).double()(x.permute(0, 3, 1, 2).double())))

    def forward(self, x):
        with torch.no_grad():
            y = copy.deepcopy(self.b3).double()(copy.deepcopy(self.c3).double()(self.middle(x))).permute(0, 2, 3, 1)
            if self.relu3 == 2:
                y = F.relu(y)
            if self.res is not None:
                y = y + self.res.double()
            if self.relu3 == 1:
                y = F.relu(y)
            return y.contiguous()

    def packs(self, device):
        from nerfdet_amd import conv3d as C
        if not hasattr(self, "_dev"):
            self._dev = [copy.deepcopy(m).to(device) for m in (self.c2, self.b2, self.c3, self.b3)]
        c2, b2, c3, b3 = self._dev
        return C.packed([c2], b2), C.packed([c3], b3)


@functools.lru_cache(maxsize=None)
def _chain_case(cin, mid, cout, nhw, k, stride, use_res, relu3, shifts="random"):
    return _ChainCase(cin, mid, cout, nhw, k, stride, use_res, relu3, shifts)


def _run_chain(device, case, arith, x=None, res=None):
    """One chained launch -> (out, kernel names).  ``x`` / ``res`` replace the case's own (CPU tensors)."""
    from nerfdet_amd import conv3d as C
    x = case.x if x is None else x
    res = case.res if res is None else res
    with _Hooked(arith) as names:
        pk2, pk3 = case.packs(device)
        assert C.chain_ok(pk2, pk3)
        y = C.conv2d_chain_nhwc(x.to(device), pk2, pk3, residual=None if res is None else res.to(device), relu=case.relu3)
    assert names == [f"k_conv_split_chain<{case.mid}>" + ("/f16x2" if arith == "f16x2" else "")], names
    return y


def _run_two(device, case, arith):
    """The two separate launches the chained kernel replaces."""
    from nerfdet_amd import conv3d as C
    with _Hooked(arith) as names:
        pk2, pk3 = case.packs(device)
        y = C.conv2d_nhwc(C.conv2d_nhwc(case.x.to(device), pk2, relu=1), pk3, residual=None if case.res is None else case.res.to(device), relu=case.relu3)
    assert len(names) == 2 and not any("chain" in n for n in names), names
    return y


def _chain_holds(tag, device, case):
    """The standard fp16-pair bars on one chained launch of ``case``."""
    got = _run_chain(device, case, "f16x2")
    _slot_is_exact(got)
    assert torch.equal(got, _run_chain(device, case, "f16x2")), "the same launch twice gave different bits"
    (elem, rms), (elem2, rms2) = _errors(got, case.ref), _errors(_run_two(device, case, "f16x2"), case.ref)
    print(f"CHAIN {tag} f16x2: elem {elem:.2e} rel-rms {rms:.2e} | two launches elem {elem2:.2e} rel-rms {rms2:.2e} | ratio {rms / rms2:.2f}")
    assert torch.isfinite(got).all()
    assert elem <= ELEM_BAR and rms < RMS_BAR and rms <= RATIO_BAR * rms2, (elem, rms, rms2)
    return got


CHAIN_ROWS = [
    # cin, mid, cout3, nhw, k, stride, residual, relu3
    (64, 64, 64, (1, 1, 1), 3, 1, True, 1),           # M = 1; waves 2 and 3 have no column pass
    (64, 64, 192, (1, 8, 16), 3, 1, True, 1),         # M = 128 exactly; Cout no multiple of 128
    (64, 64, 256, (1, 9, 15), 3, 1, False, 0),        # M = 135: the second tile has 7 rows
    (32, 64, 128, (2, 9, 11), 1, 1, True, 2),         # one K chunk in the first convolution
    (128, 128, 320, (1, 8, 8), 3, 1, True, 1),        # MID 128, M = 64: the second half is empty
    (128, 128, 512, (1, 5, 13), 3, 1, True, 1),       # M = 65: the second half holds one row
    (128, 128, 64, (1, 3, 43), 3, 1, False, 1),       # M = 129; Cout 64
    (128, 128, 512, (3, 13, 17), 3, 2, True, 1),      # stride 2 on odd extents; M = 189
]
ROW_64, ROW_128S2 = (64, 64, 256, (3, 13, 17), 3, 1, True, 1), (128, 128, 512, (3, 13, 17), 3, 2, True, 1)


def _row_id(r):
    return f"{r[0]}-{r[1]}-{r[2]}-{'x'.join(map(str, r[3]))}-k{r[4]}s{r[5]}-res{int(r[6])}-relu{r[7]}"


@pytest.mark.parametrize("arith", ["f16x2", "bf16x3", "bf16"])
@pytest.mark.parametrize("row", CHAIN_ROWS, ids=_row_id)
def test_chain_edge_row(device, row, arith):
    """G: tile and column edges of k_conv_split_chain in its three arithmetics."""
    case = _chain_case(*row)
    scale = max(1.0, float(case.ref.abs().max()))
    if arith == "f16x2":
        _chain_holds(_row_id(row), device, case)
    elif arith == "bf16x3":
        elem, rms = _errors(_run_chain(device, case, "bf16x3"), case.ref)
        print(f"CHAIN {_row_id(row)} bf16x3: elem {elem:.2e} rel-rms {rms:.2e}")
        assert elem <= ELEM_BAR, elem
    else:
        got, two = _run_chain(device, case, "bf16"), _run_two(device, case, "bf16")
        d = float((got - two).abs().max()) / scale
        print(f"CHAIN {_row_id(row)} bf16: chained - two launches {d:.2e}")
        assert d <= BF16_BAR, d


def _chain_stays_normal(case, k):
    mid = case.middle(case.x)
    smallest = [float(case.ref[case.ref != 0].abs().min())]
    for inp, conv, bn in ((case.x, case.c2, case.b2), (mid, case.c3, case.b3)):
        w, s = conv.weight.detach().abs(), (bn.weight / torch.sqrt(bn.running_var + bn.eps)).detach().abs()
        smallest.append(float(inp[inp != 0].abs().min()) * float(w[w != 0].min()) * float(s.min()))
    return min(smallest) * 2.0 ** min(k, 0) >= TINY


@pytest.mark.parametrize("arith", ["f16x2", "bf16x3"])
@pytest.mark.parametrize("row", [ROW_64, ROW_128S2], ids=_row_id)
def test_chain_is_homogeneous(device, row, arith):
    """H.1: zero BN shifts, x and the residual times 2^k -> the output times 2^k, bit for bit (k = -40, +40)."""
    case = _chain_case(*row, shifts="zero")
    base = _run_chain(device, case, arith)
    assert float(base.abs().max()) > 0
    bad = []
    for k in (-40, 40):
        assert _chain_stays_normal(case, k), f"2^{k} reaches fp32 subnormals: reduce |k|"
        got, want = _run_chain(device, case, arith, x=case.x * 2.0 ** k, res=case.res * 2.0 ** k), base * 2.0 ** k
        if arith == "f16x2":
            _slot_is_exact(got)
        if not torch.equal(got, want):
            bad.append(f"k = {k}: largest distance {_ulps(got, want)} ulp")
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("arith,nhw", [("bf16x3", (3, 9, 15)), ("f16x2", (3, 8, 16))])
def test_chain_images_are_independent(device, arith, nhw):
    """H.2: the stacked launch == the single-image launches.  bf16x3 has no data-dependent scale (any shape: here tiles straddle images); in f16x2 an
    8 x 16 image is exactly one 128-row tile, so a tile's own ymax sees one image, and the tensor's maximum is planted in every image."""
    case = _chain_case(64, 64, 256, nhw, 3, 1, True, 1)
    x = case.x.clone()
    if arith == "f16x2":
        assert float(x.max()) < 64.0
        x[:, 3, 7, 5] = 64.0
    stacked = _run_chain(device, case, arith, x=x)
    for i in range(nhw[0]):
        one = _run_chain(device, case, arith, x=x[i:i + 1].contiguous(), res=case.res[i:i + 1].contiguous())
        assert torch.equal(stacked[i:i + 1], one), f"image {i} differs from its own launch by {_ulps(stacked[i:i + 1], one)} ulp"


@pytest.mark.parametrize("mid", [64, 128])
@pytest.mark.parametrize("kind", ["first_tile", "all"])
def test_chain_with_a_zero_tile(device, mid, kind):
    """H.3: the first convolution's BN shifts <= 0 and x zero on the first 128 rows plus the rows their 3 x 3 taps reach (or everywhere): the first
    tile's intermediate is exactly zero (ymax == 0: the eb < 30 clamp), its output relu(shift3 + residual)."""
    case = copy.copy(_chain_case(mid, mid, 4 * mid, (3, 13, 17), 3, 1, True, 1, shifts="nonpos"))
    case.x = case.x.clone() + 0.01
    if kind == "all":
        case.x.zero_()
    else:
        case.x[0, :9] = 0.0           # rows 0 .. 127 are the image rows 0 .. 6 and nine pixels of row 7; their taps reach row 8
    case.ref = case.forward(case.x)
    inter = case.middle(case.x).permute(0, 2, 3, 1).reshape(-1, mid)
    assert float(inter[:128].abs().max()) == 0.0, "the first tile's intermediate is not zero"
    assert kind == "all" or float(inter[128:256].abs().max()) > 0
    assert float(case.ref.abs().max()) > 0
    _chain_holds(f"H.3 zero {kind} mid {mid}", device, case)


@pytest.mark.parametrize("arith", ["f16x2", "bf16x3"])
@pytest.mark.parametrize("row", [ROW_64, (128, 128, 512, (1, 5, 13), 3, 1, True, 1)], ids=_row_id)
def test_chain_non_temporal_stores(device, row, arith):
    """H.4: nt_bytes = 0 sends every store down the non-temporal branch: the same bits as with the default threshold (the knob is process wide)."""
    from nerfdet_amd import _lib
    case = _chain_case(*row)
    plain = _run_chain(device, case, arith)
    try:
        _lib.check(_lib.load().ndet_measurement_knob(b"nt_bytes", 0), "measurement_knob")
        streamed = _run_chain(device, case, arith)
    finally:
        _lib.check(_lib.load().ndet_measurement_knob(b"nt_bytes", 32 << 20), "measurement_knob")
    assert torch.equal(plain, streamed), f"non-temporal stores differ by {_ulps(plain, streamed)} ulp"
    if arith == "f16x2":
        _slot_is_exact(streamed)


# ------------------------------------------------------------------ rejections before any launch ------------------------------------------------------------------
SENTINEL = -7.0


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _rejected(lib, code, want, entry, out):
    torch.cuda.synchronize()
    msg = lib.ndet_last_error().decode()
    assert code == want, (code, want, msg)
    assert entry in msg, msg
    assert bool((out == SENTINEL).all()), "a rejected call wrote the output"


def test_bottleneck_entry_rejects_before_any_launch(device):
    """I: ndet_bottleneck_f16x2 with valid device buffers and one bad argument at a time: NDET_E_UNSUPPORTED (-2) / NDET_E_INVALID (-1)."""
    from nerfdet_amd import _lib, conv3d as C
    lib = _lib.load()
    blk = {ds: copy.deepcopy(_plain_block(ds)).to(device) for ds in (0, 1)}
    x = torch.rand(1, 4, 16, 256, device=device)
    out = torch.full((1, 4, 16, 256), SENTINEL, device=device)
    slot = C.amax_of(x)

    def call(ds, cin, w1inv=None, with_wd=None):
        b = blk[ds]
        pks = [C.packed([b.conv1], b.bn1), C.packed([b.conv2], b.bn2), C.packed([b.conv3], b.bn3)]
        (p1, i1), (p2, i2), (p3, i3) = [C.split_planes_f16(pk) for pk in pks]
        pkd = C.packed([blk[1].downsample[0]], blk[1].downsample[1])
        pd, idd = C.split_planes_f16(pkd)
        wd = (ds == 1) if with_wd is None else with_wd
        return lib.ndet_bottleneck_f16x2(_p(x), 1, 4, 16, cin, 256, _p(p1), i1 if w1inv is None else w1inv, _p(pks[0].scale), _p(pks[0].shift), _p(p2), i2,
                                         _p(pks[1].scale), _p(pks[1].shift), _p(p3), i3, _p(pks[2].scale), _p(pks[2].shift), _p(pd if wd else None), idd,
                                         _p(pkd.scale if wd else None), _p(pkd.shift if wd else None), _p(slot), None, _p(out), None, C.GUARD_TOL, None,
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    fn = "ndet_bottleneck_f16x2"
    _rejected(lib, call(0, 128), -2, fn, out)                              # Cin = 128
    _rejected(lib, call(0, 256, with_wd=True), -2, fn, out)                # the downsample form with Cin = 256
    _rejected(lib, call(1, 64, with_wd=False), -1, fn, out)                # the identity form with Cin = 64
    _rejected(lib, call(0, 256, w1inv=0.0), -1, fn, out)                   # w1_inv_scale = 0
    assert call(0, 256) == 0 and call(1, 64) == 0, lib.ndet_last_error()   # the same arguments without the bad one launch
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any())


def test_chain_entry_rejects_before_any_launch(device):
    """I: ndet_conv_chain with valid device buffers and one bad argument at a time."""
    from nerfdet_amd import _lib, conv3d as C
    lib = _lib.load()
    case = _chain_case(64, 64, 256, (1, 8, 16), 3, 1, True, 1)
    with torch.no_grad():
        pk2, pk3 = case.packs(device)
        p1, p3 = C.split_planes(pk2), C.split_planes(pk3)
    x, res = case.x.to(device), case.res.to(device)
    out = torch.full((1, 8, 16, 256), SENTINEL, device=device)
    slot = C.amax_of(x)
    good = dict(cin=64, cmid=64, cout=256, relu3=1, arith=0, in_amax=None)

    def call(**bad):
        a = dict(good, **bad)
        return lib.ndet_conv_chain(_p(x), _p(p1), 1, 8, 16, a["cin"], a["cmid"], _lib.i3(1, 3, 3), _lib.i3(1, 1, 1), _lib.i3(0, 1, 1), _p(pk2.scale), _p(pk2.shift),
                                   _p(p3), a["cout"], _p(pk3.scale), _p(pk3.shift), _p(res), a["relu3"], _p(out), a["arith"], _p(a["in_amax"]), 1.0, 1.0, None,
                                   0.0, 0.0, 0.0, None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    fn = "ndet_conv_chain"
    _rejected(lib, call(cmid=96), -2, fn, out)
    _rejected(lib, call(cin=48), -2, fn, out)
    _rejected(lib, call(cout=96), -2, fn, out)
    _rejected(lib, call(arith=1), -1, fn, out)                             # the fp16-pair arithmetic without in_amax
    _rejected(lib, call(arith=0, in_amax=slot), -1, fn, out)               # ... and in_amax without it
    _rejected(lib, call(relu3=3), -1, fn, out)
    assert call() == 0, lib.ndet_last_error()                              # the same arguments without the bad one launch
    torch.cuda.synchronize()
    assert _errors(out, case.ref)[0] <= ELEM_BAR
