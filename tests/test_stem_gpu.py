"""The ResNet stem's kernels (the first four modules of the mmdet ResNet behind mmdet3d/models/detectors/nerfdet.py:140) against plain references, at
the sizes where the persistent loop of k_stem_conv_pool (csrc/stem_kernels.hip) takes its second and third iteration:

* k_stem_conv_pool<0> (bf16x3, also what the "bf16" mode runs) and <1> (f16x2) against an fp64 evaluation of the same Conv2d + eval BatchNorm2d +
  ReLU + MaxPool2d on the CPU, elementwise within ELEM_BAR and rel-rms below RMS_BAR (tests/test_f16x2_edges_gpu.py), whole tensor AND per image:
  the launcher caps the grid at GRID_CAP = 512 workgroups, so (45, 70, 100) = 1080 tiles gives workgroups 0..55 three iterations and the rest two,
  (23, 70, 100) = 552 tiles gives workgroups 0..39 two and the rest one.  A tile that read its predecessor's patch, scale or staged tile is an O(1)
  error on standard normal images;
* exact homogeneity: out(x 2^k) == out(x) 2^k bit for bit with a zero BatchNorm shift, k changing from image to image and between the halves of
  some images (so the fp16-pair form's per-patch scale changes from one iteration of a workgroup to the next).  The check that runs: bit equality
  on every pooled pixel whose 11 x 11 input window lies in one half, in bf16x3; in f16x2 on those whose tile's whole 19 x 39 PATCH lies in one half
  -- a patch holding both halves is scaled by the larger one's maximum, which moves the smaller half's fp16 low terms into the subnormals, so there
  (tile column 1 of the mixed images) the result is legitimately not a power-of-two multiple and is held to the fp64 bars relative to that image's
  own max |ref| instead, as is every image of the scaled batch;
* patches of exact zeros (what Pad after Normalize leaves): relu(shift) bit for bit wherever the window is all zero, zero and non-zero patches
  following each other inside one workgroup;
* sizes from the entry point's minimum to one pooled column past a tile, in four memory layouts;
* both weight packs against their definition;
* k_bn_relu_maxpool (csrc/conv3d_kernels.hip) bit for bit against the two-rounding fp32 expression and within its derived bound of fp64;
* the route ResNet._stem takes under each arithmetic.

Measured on an MI355X (elementwise error / max(1, max|ref|) and rel-rms; "worst image" = the largest per-image value and its index):

    STEM loop (45, 70, 100) f16x2 : elem 2.96e-07 rel-rms 1.35e-07 | worst image elem 3.85e-07 (#44) rel-rms 1.39e-07 (#7)
    STEM loop (45, 70, 100) bf16x3: elem 3.99e-07 rel-rms 1.64e-07 | worst image elem 4.79e-07 (#1) rel-rms 1.69e-07 (#11)
    STEM loop (23, 70, 100) f16x2 : elem 3.07e-07 rel-rms 1.35e-07 | worst image elem 3.88e-07 (#15) rel-rms 1.38e-07 (#7)
    STEM loop (23, 70, 100) bf16x3: elem 3.86e-07 rel-rms 1.61e-07 | worst image elem 4.48e-07 (#19) rel-rms 1.64e-07 (#22)
    STEM homogeneity f16x2: 1005 of 1125 pooled columns held to bit equality, 0 differ; window in one half but patch in both: 90 columns, 17 differ
    STEM homogeneity f16x2: scaled batch vs fp64 per image: worst elem / max|ref_i| 5.33e-07 (#21) rel-rms 1.48e-07 (#8)
    STEM homogeneity bf16x3: 1095 of 1125 pooled columns held to bit equality, 0 differ; window in one half but patch in both: 90 columns, 0 differ
    STEM homogeneity bf16x3: scaled batch vs fp64 per image: worst elem / max|ref_i| 5.06e-07 (#13) rel-rms 1.81e-07 (#4)
    STEM zeros f16x2 / bf16x3: elem 2.96e-07 / 3.77e-07, rel-rms 1.13e-07 / 1.33e-07
    STEM small (all six sizes, the four layouts give the same figures): elem <= 3.01e-07, rel-rms <= 1.48e-07 in both arithmetics
    STEM route f32 (library convolution + k_bn_relu_maxpool): elem 4.02e-07 rel-rms 1.76e-07; f16x2 2.28e-07 / 1.29e-07; bf16x3 = bf16 2.96e-07 / 1.58e-07

No row comes near RMS_BAR (2e-6) or ELEM_BAR (2e-5).
"""
import copy
import functools
import types
from ctypes import c_void_p

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from test_f16x2_edges_gpu import ELEM_BAR, RMS_BAR, _errors

pytestmark = pytest.mark.gpu

GRID_CAP = 512                    # ndet_stem_conv_bn_relu_maxpool: two persistent workgroups per CU
TPY, TPX = 3, 8                   # pooled pixels of a tile
LOOP3, LOOP2 = (45, 70, 100), (23, 70, 100)


def _tiles(n, h, w):
    """(tiles, PH, PW) as the launcher computes them."""
    ch, cw = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    ph, pw = (ch - 1) // 2 + 1, (cw - 1) // 2 + 1
    return n * ((ph + TPY - 1) // TPY) * ((pw + TPX - 1) // TPX), ph, pw


def _modules(seed, zero_shift=False):
    torch.manual_seed(seed)
    conv = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
    bn = nn.BatchNorm2d(64).eval()
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.3); bn.running_var.uniform_(0.5, 2.0); bn.weight.uniform_(0.5, 1.5); bn.bias.normal_(0, 0.3)
        if zero_shift:
            bn.running_mean.zero_(); bn.bias.zero_()
    return conv, bn


def _ref64(conv, bn, x):
    """max_pool2d(relu(bn(conv(x))), 3, 2, 1) in fp64 on the CPU, channels-last."""
    conv, bn = copy.deepcopy(conv).double(), copy.deepcopy(bn).double()
    with torch.no_grad():
        return F.max_pool2d(F.relu(bn(conv(x.double()))), 3, 2, 1).permute(0, 2, 3, 1).contiguous()


class _Stem:
    """The stem's modules on the CPU and (one copy, made once) on the GPU."""

    def __init__(self, seed, zero_shift=False):
        self.conv, self.bn = _modules(seed, zero_shift)

    def on(self, device):
        if not hasattr(self, "_dev"):
            self._dev = (copy.deepcopy(self.conv).to(device), copy.deepcopy(self.bn).to(device))
        return self._dev

    def run(self, device, xd, arith):
        from nerfdet_amd import conv3d as C
        conv_d, bn_d = self.on(device)
        prev = C.set_arithmetic(arith)
        try:
            assert C.stem_ok(conv_d, bn_d, xd)
            with torch.no_grad():
                out = C.stem_conv_bn_relu_maxpool(xd, conv_d, bn_d)
            torch.cuda.synchronize()
        finally:
            C.set_arithmetic(prev)
        return out

    def affine(self, device):
        from nerfdet_amd import conv3d as C
        scale, shift = C.bn_affine(self.on(device)[1])
        return scale.cpu(), shift.cpu()


@functools.lru_cache(maxsize=None)
def _loop_case(nhw):
    """(stem, x, fp64 result) of a persistent-loop shape: built once, shared unchanged."""
    stem = _Stem(sum(nhw))
    x = torch.randn(nhw[0], 3, nhw[1], nhw[2])
    return stem, x, _ref64(stem.conv, stem.bn, x)


def _per_image(got, ref, floor=1.0):
    """Per image: (max |got - ref| / max(floor, max|ref_i|), rel-rms), as two (N,) tensors."""
    d = (got.double().cpu() - ref).flatten(1)
    r = ref.flatten(1)
    return d.abs().amax(1) / r.abs().amax(1).clamp_min(floor), d.pow(2).mean(1).sqrt() / r.pow(2).mean(1).sqrt()


def _check_bars(tag, got, ref):
    elem, rms = _errors(got, ref)
    print(f"STEM {tag}: elem {elem:.2e} rel-rms {rms:.2e}")
    assert elem <= ELEM_BAR and rms < RMS_BAR, (tag, elem, rms)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1. the persistent loop
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nhw", [LOOP3, LOOP2], ids=lambda s: "x".join(map(str, s)))
def test_persistent_loop_matches_fp64(device, nhw):
    from nerfdet_amd import conv3d as C
    assert _tiles(*LOOP3)[0] > 2 * GRID_CAP, "the first shape must give some workgroups a third iteration"
    assert GRID_CAP < _tiles(*LOOP2)[0] < 2 * GRID_CAP, "the second shape: one or two iterations"
    stem, x, ref = _loop_case(nhw)
    xd = x.to(device)
    outs = {}
    for arith in ("f16x2", "bf16x3", "bf16"):
        got = outs[arith] = stem.run(device, xd, arith)
        assert tuple(got.shape) == (nhw[0],) + _tiles(*nhw)[1:] + (64,)
        if arith == "f16x2":
            assert C.amax_value(got._ndet_amax) == float(got.abs().max()), "the max |out| slot is not the tensor's maximum"
        else:
            assert not hasattr(got, "_ndet_amax")
    assert torch.equal(outs["bf16"], outs["bf16x3"]), "the bf16 mode runs the stem in bf16x3"
    worst = []
    for arith in ("f16x2", "bf16x3"):
        elem, rms = _errors(outs[arith], ref)
        ie, ir = _per_image(outs[arith], ref)
        print(f"STEM loop {nhw} {arith:6s}: elem {elem:.2e} rel-rms {rms:.2e} | worst image elem {float(ie.max()):.2e} (#{int(ie.argmax())}) "
              f"rel-rms {float(ir.max()):.2e} (#{int(ir.argmax())})")
        worst.append((arith, elem, rms, float(ie.max()), float(ir.max())))
    for arith, elem, rms, ie, ir in worst:
        assert elem <= ELEM_BAR and rms < RMS_BAR and ie <= ELEM_BAR and ir < RMS_BAR, (arith, elem, rms, ie, ir)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2. the scale of a patch belongs to that patch
# ---------------------------------------------------------------------------------------------------------------------------------------------
SPLIT = 47           # first column of the right half of the mixed images (inside tile column 1's patch, columns 27..65)


@pytest.mark.parametrize("arith", ["f16x2", "bf16x3"])
def test_power_of_two_scaling_commutes_bit_for_bit(device, arith):
    n, h, w = LOOP3
    _, ph, pw = _tiles(n, h, w)
    stem = _Stem(5, zero_shift=True)
    assert float(stem.affine(device)[1].abs().max()) == 0.0, "the folded shift must be exactly 0"
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(n, 3, h, w, generator=gen)
    kl = torch.randint(-12, 13, (n,), generator=gen)
    mixed = torch.arange(n) % 3 == 1                                                          # these images get another exponent in their right half
    kr = torch.where(mixed, (kl + 12 + torch.randint(1, 25, (n,), generator=gen)) % 25 - 12, kl)
    assert bool((kr[mixed] != kl[mixed]).all()) and bool((kr[~mixed] == kl[~mixed]).all()) and int(kl.abs().max()) <= 12 and int(kr.abs().max()) <= 12
    col = torch.arange(w)
    kmap = torch.where(col[None, :] < SPLIT, kl[:, None], kr[:, None])                        # (n, w)
    xs = x * torch.exp2(kmap.float())[:, None, None, :]
    assert torch.equal(xs.double(), x.double() * torch.exp2(kmap.double())[:, None, None, :]), "the scaling itself must be exact"
    base = stem.run(device, x.to(device), arith).cpu()
    got = stem.run(device, xs.to(device), arith).cpu()

    px = torch.arange(pw)
    lo, hi = (4 * px - 5).clamp_min(0), (4 * px + 5).clamp_max(w - 1)                         # the pooled pixel's input columns
    left, right = hi < SPLIT, lo >= SPLIT
    plo, phi = (32 * (px // TPX) - 5).clamp_min(0), (32 * (px // TPX) + 33).clamp_max(w - 1)  # ... and its tile's patch columns
    patch_one_half = (phi < SPLIT) | (plo >= SPLIT)
    assert int((left | right).sum()) >= pw - 3 and int(((left | right) & ~patch_one_half).sum()) >= 4
    window_ok = torch.where(mixed[:, None], (left | right)[None, :], torch.ones(n, pw, dtype=torch.bool))
    patch_ok = torch.where(mixed[:, None], ((left | right) & patch_one_half)[None, :], torch.ones(n, pw, dtype=torch.bool))
    kout = torch.where(left[None, :], kl[:, None], kr[:, None])                               # (n, pw); anything where neither holds (masked out)
    want = base * torch.exp2(kout.float())[:, None, :, None]
    same = (got == want).all(3).all(1)                                                        # (n, pw): all rows and channels of that pooled column
    exact = patch_ok if arith == "f16x2" else window_ok
    n_window_only = int((window_ok & ~patch_ok).sum())
    print(f"STEM homogeneity {arith}: {int(exact.sum())} of {n * pw} pooled columns held to bit equality, {int((exact & ~same).sum())} differ; "
          f"window in one half but patch in both: {n_window_only} columns, {int((window_ok & ~patch_ok & ~same).sum())} differ")
    assert bool(same[exact].all()), f"out(x 2^k) != out(x) 2^k at (image, pooled column) {torch.nonzero(exact & ~same)[:8].tolist()}"
    assert bool(base.abs().amax((1, 2, 3)).gt(0).all())
    # every image of the scaled batch against fp64, relative to ITS OWN max |ref| (the images span 2^-12 ... 2^12); this is also what holds the f16x2
    # columns whose patch contains both halves
    ref = _ref64(stem.conv, stem.bn, xs)
    ie, ir = _per_image(got, ref, floor=0.0)
    print(f"STEM homogeneity {arith}: scaled batch vs fp64 per image: worst elem / max|ref_i| {float(ie.max()):.2e} (#{int(ie.argmax())}) "
          f"rel-rms {float(ir.max()):.2e} (#{int(ir.argmax())})")
    assert float(ie.max()) <= ELEM_BAR and float(ir.max()) < RMS_BAR, (float(ie.max()), float(ir.max()))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3. exact-zero patches
# ---------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _zero_case():
    """20 images of 64 x 160 (600 tiles: workgroups 0..87 run two iterations): columns from 40 on are zero, every third image is zero altogether, so
    zero and non-zero patches follow each other inside one workgroup in both orders."""
    stem = _Stem(11)
    x = torch.randn(20, 3, 64, 160)
    x[:, :, :, 40:] = 0
    x[1::3] = 0
    return stem, x, _ref64(stem.conv, stem.bn, x)


@pytest.mark.parametrize("arith", ["f16x2", "bf16x3"])
def test_zero_patches_give_relu_of_the_shift(device, arith):
    stem, x, ref = _zero_case()
    n, _, h, w = x.shape
    tiles, ph, pw = _tiles(n, h, w)
    assert GRID_CAP < tiles
    got = stem.run(device, x.to(device), arith).cpu()
    # pooled pixel (py, px) reads input rows 4 py - 5 .. 4 py + 5 and the same columns: a max-pool of the "non-zero" indicator over that window
    nonzero = (x != 0).any(1, keepdim=True).float()
    all_zero = F.max_pool2d(nonzero, 11, 4, 5)[:, 0] == 0                                     # (n, ph, pw)
    assert tuple(all_zero.shape) == (n, ph, pw)
    assert int(all_zero.sum()) >= 7 * ph * pw + 13 * ph * (pw - 12), "whole zero images and whole zero tiles must be among the windows"
    shift = stem.affine(device)[1]
    assert bool((shift > 0).any()) and bool((shift < 0).any())
    want = F.relu(shift).expand(int(all_zero.sum()), 64)
    assert torch.equal(got[all_zero], want), "an all-zero window must give relu(shift) exactly"
    _check_bars(f"zeros {arith}", got, ref)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 4. around one tile and the minimum
# ---------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _small_case(nhw):
    stem = _Stem(100 + sum(nhw))
    x = torch.randn(nhw[0], 3, nhw[1], nhw[2])
    return stem, x, _ref64(stem.conv, stem.bn, x)


def _layout(x, layout, device):
    """The logical (N, 3, H, W) images ``x`` on the GPU in the asked memory layout."""
    n, _, h, w = x.shape
    xd = x.to(device)
    if layout == "nhwc":
        xd = xd.contiguous(memory_format=torch.channels_last)
    elif layout == "view":                                          # a window of a larger NCHW buffer filled with something that must not be read
        big = torch.full((n, 3, h + 5, w + 9), 1e6, device=device)
        big[:, :, 2:2 + h, 4:4 + w] = xd
        xd = big[:, :, 2:2 + h, 4:4 + w]
    elif layout == "rgb4":                                          # three channels of a four-channel channels-last buffer: x stride 4
        big = torch.full((n, h, w, 4), 1e6, device=device)
        big[..., :3] = xd.permute(0, 2, 3, 1)
        xd = big[..., :3].permute(0, 3, 1, 2)
        assert xd.stride() == (h * w * 4, 1, w * 4, 4)
    else:
        assert layout == "nchw"
    assert torch.equal(xd.cpu(), x)
    return xd


@pytest.mark.parametrize("layout", ["nchw", "nhwc", "view", "rgb4"])
@pytest.mark.parametrize("nhw,phw", [((2, 7, 7), (2, 2)), ((1, 7, 34), (2, 9)), ((2, 13, 29), (4, 8)), ((1, 12, 32), (3, 8)), ((3, 9, 33), (3, 9)),
                                     ((2, 8, 130), (2, 33))], ids=lambda v: "x".join(map(str, v)))
def test_small_sizes_and_layouts_match_fp64(device, nhw, phw, layout):
    assert _tiles(*nhw)[1:] == phw
    stem, x, ref = _small_case(nhw)
    xd = _layout(x, layout, device)
    for arith in ("f16x2", "bf16x3"):
        got = stem.run(device, xd, arith)
        assert tuple(got.shape) == tuple(ref.shape) == (nhw[0],) + phw + (64,)
        _check_bars(f"small {nhw} {layout} {arith}", got, ref)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 5. the weight packs
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _packed_layout(w):
    """(64, 3, 7, 7) -> (64, 176) with k = (ky * 3 + c) * 8 + kx, zero at kx = 7 and k >= 168; and the mask of those zero positions."""
    e = torch.zeros(64, 7, 3, 8, dtype=w.dtype)
    e[..., :7] = w.permute(0, 2, 1, 3)
    out = torch.zeros(64, 176, dtype=w.dtype)
    out[:, :168] = e.reshape(64, 168)
    k = torch.arange(176)
    return out, ((k % 8 == 7) | (k >= 168))[None, :].expand(64, 176)


@functools.lru_cache(maxsize=None)
def _wide_weight():
    torch.manual_seed(3)
    w = torch.randn(64, 3, 7, 7) * torch.exp(3 * torch.randn(64, 3, 7, 7))              # many binades
    assert float(w.abs().max()) / float(w.abs().min()) > 2.0 ** 20 and bool((w != 0).all())
    return w


def test_bf16x3_weight_pack_is_an_exact_split(device):
    from nerfdet_amd import _lib
    w = _wide_weight()
    wd = w.to(device)
    planes = torch.full((3, 64, 176), 0x7fc0, dtype=torch.int16, device=device)            # NaN patterns: every element must be written
    _lib.check(_lib.load().ndet_stem_pack_weights(c_void_p(wd.data_ptr()), c_void_p(planes.data_ptr()), c_void_p(torch.cuda.current_stream().cuda_stream)),
               "stem_pack_weights")
    torch.cuda.synchronize()
    p = planes.view(torch.bfloat16).float().cpu()
    want, zero = _packed_layout(w)
    assert torch.equal(p[0], want.bfloat16().float()), "the leading plane is the weight rounded to bf16"
    assert torch.equal(p[0] + p[1] + p[2], want) and torch.equal(p.double().sum(0), want.double()), "the three planes must sum to the weight exactly"
    assert bool((p[:, zero] == 0).all()) and bool((p[0][~zero] != 0).all())


def test_f16x2_weight_pack_matches_its_definition(device):
    from nerfdet_amd import _lib, conv3d as C
    w = _wide_weight()
    wd = w.to(device)
    s = C.f16_weight_scale(float(w.abs().max()))
    assert 2.0 ** 14 <= float(w.abs().max()) * s < 2.0 ** 15
    planes = torch.full((2, 64, 176), 0x7e00, dtype=torch.int16, device=device)
    _lib.check(_lib.load().ndet_stem_pack_weights_f16x2(c_void_p(wd.data_ptr()), s, c_void_p(planes.data_ptr()),
                                                        c_void_p(torch.cuda.current_stream().cuda_stream)), "stem_pack_weights_f16x2")
    torch.cuda.synchronize()
    got = planes.view(torch.float16).cpu()
    want, zero = _packed_layout(w)
    ws = want * s
    hi = ws.half()
    lo = (ws - hi.float()).half()
    assert torch.equal(got.view(torch.int16), torch.stack([hi, lo]).view(torch.int16)), "hi = fp16(w s), lo = fp16(w s - hi)"
    assert bool((got[:, zero] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 6. bn_relu_maxpool_nhwc
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nhwc,bias", [((2, 7, 9, 64), 0.0), ((1, 1, 1, 4), 0.0), ((3, 8, 8, 8), 0.0), ((1, 2, 5, 68), 0.0), ((2, 33, 18, 64), 0.0),
                                       ((2, 33, 18, 64), -2.5)], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"bias{v}")
def test_bn_relu_maxpool_is_the_two_rounding_expression(device, nhwc, bias):
    from nerfdet_amd import conv3d as C
    n, h, w, c = nhwc
    torch.manual_seed(sum(nhwc))
    bn = nn.BatchNorm2d(c).eval()
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.3); bn.running_var.uniform_(0.5, 2.0); bn.weight.uniform_(0.5, 1.5); bn.bias.normal_(bias, 0.3)
    x = torch.randn(n, h, w, c)
    bn_d = copy.deepcopy(bn).to(device)
    got = C.bn_relu_maxpool_nhwc(x.to(device), bn_d)
    torch.cuda.synchronize()
    got = got.cpu()
    scale, shift = (t.cpu() for t in C.bn_affine(bn_d))

    def pooled(xx, sc, sh):                                          # max over fl(fl(x scale) + shift), ReLU'd, in the dtype of the arguments
        return F.max_pool2d(F.relu(xx * sc + sh).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()
    want = pooled(x, scale, shift)
    assert tuple(got.shape) == tuple(want.shape) == (n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c)
    assert torch.equal(got, want), f"differs from the fp32 expression by {float((got - want).abs().max()):.3e}"
    ref = pooled(x.double(), scale.double(), shift.double())
    bound = 2.0 ** -22 * (float((x.double() * scale.double()).abs().max()) + float(shift.abs().max()))      # two fp32 roundings
    assert float((got.double() - ref).abs().max()) <= bound
    if bias < 0:                                                     # windows that are non-positive altogether: the output there is the ReLU's 0
        dead = F.max_pool2d((x.double() * scale.double() + shift.double()).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1) <= 0
        assert int(dead.sum()) > dead.numel() // 4 and int((~dead).sum()) > 0
        assert bool((got[dead] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 7. the route
# ---------------------------------------------------------------------------------------------------------------------------------------------
class _Recording:
    """Stands in for the loaded library: records the name of every entry point that is looked up, and hands back the real one."""

    def __init__(self, lib):
        self.lib, self.names = lib, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self.lib, name)


@pytest.mark.parametrize("arith,fused", [("f32", False), ("f16x2", True), ("bf16x3", True), ("bf16", True)])
def test_stem_route_per_arithmetic(device, arith, fused):
    from nerfdet_amd import _lib, conv3d as C
    from nerfdet_amd.backbone import ResNet
    stem, x, ref = _small_case((2, 61, 83))
    conv_d, bn_d = stem.on(device)
    net = types.SimpleNamespace(conv1=conv_d, bn1=bn_d)             # all that ResNet._stem reads
    real = _lib.load()
    rec = _Recording(real)
    prev = C.set_arithmetic(arith)
    try:
        _lib._lib = rec
        with torch.no_grad():
            got = ResNet._stem(net, x.to(device))
        torch.cuda.synchronize()
    finally:
        _lib._lib = real
        C.set_arithmetic(prev)
    assert ("ndet_stem_conv_bn_relu_maxpool" in rec.names) == fused, rec.names
    assert ("ndet_bn_relu_maxpool_nhwc" in rec.names) == (not fused), rec.names
    _check_bars(f"route {arith}", got, ref)
