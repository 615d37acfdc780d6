"""NaN and +-Inf through the kernels that take a maximum (ReLU, max-pool, clamp, the backward's mask, the variance clamps): planted inputs,
float64 references and the check of DESIGN.md "Non-finite values".  No GPU in here: tests/test_nonfinite_cpu.py shows that PyTorch-CPU fp32
itself meets the contract on every case, tests/test_nonfinite_gpu.py holds the kernels to it.

Values are planted in activations, residuals, features and raw sigma only -- never in points, poses, intrinsics or anything an index is
computed from.  One case gives three float64 CPU results of the same torch modules:

    ref        the planted kind (NaN, +Inf or -Inf) in place
    ref_nan    NaN at the same places
    ref_clean  0 at the same places

``field = isnan(ref_nan)`` is the planted elements' receptive field.  :func:`check` then asserts

1. outside the field ``got`` is finite and within the bars of the case's home test file (max |ref| and the rms taken outside the field);
2. planted NaN: ``isnan(got) == isnan(ref)`` on every element;
3. planted +-Inf: inside the field ``got`` is non-finite wherever ``ref`` is.  Where ``ref`` is finite inside the field (a -Inf that a ReLU
   turned into 0) ``got`` may be anything: the hi / lo operand split of the MFMA kernels makes Inf - Inf = NaN, a wider poison than the
   reference's, which is accepted.

The cases plant three voxels (the first, an interior one, the last voxel's last channel) and one residual element outside their fields, and
every case keeps at least MIN_OUTSIDE of its output outside the field, so that 1. stays a real test (asserted by the CPU test)."""
import copy
import functools
from typing import NamedTuple

import torch
import torch.nn.functional as F

KINDS = ("nan", "+inf", "-inf")
VALUES = {"nan": float("nan"), "+inf": float("inf"), "-inf": -float("inf"), "clean": 0.0}
MIN_OUTSIDE = 0.6


def plant(x, kind, places):
    """A copy of ``x`` with the value of ``kind`` ("nan", "+inf", "-inf", or "clean" = 0) at every index tuple of ``places``."""
    out = x.clone()
    for p in places:
        out[tuple(p)] = VALUES[kind]
    return out


class Refs(NamedTuple):
    ref: torch.Tensor
    ref_nan: torch.Tensor
    ref_clean: torch.Tensor


def three(compute, kind):
    """``compute(k)`` -> a tensor or a dict of tensors for k in (kind, "nan", "clean") -> Refs, or a dict of Refs by output name."""
    got = {k: compute(k) for k in dict.fromkeys((kind, "nan", "clean"))}
    if isinstance(got["nan"], dict):
        return {name: Refs(got[kind][name].double(), got["nan"][name].double(), got["clean"][name].double()) for name in got["nan"]}
    return Refs(got[kind].double(), got["nan"].double(), got["clean"].double())


def field(refs):
    return torch.isnan(refs.ref_nan)


def outside_fraction(refs):
    return float((~field(refs)).double().mean())


def check(got, refs, bars, kind, tag=""):
    """Contracts 1-3 of the module docstring on one output; returns the measured figures.  ``bars``: any of
    "elem" (max error / max(1, max|ref|)), "rms" (rel-rms, strict), "rel" (max error / max|ref|), "abs" (max error), "tol" (a tensor of
    elementwise absolute tolerances), every one over the elements outside the field."""
    ref, f = refs.ref, field(refs)
    g = got.detach().double().cpu()
    assert tuple(g.shape) == tuple(ref.shape), (tag, g.shape, ref.shape)
    out = ~f
    fig = {"outside": float(out.double().mean())}
    assert bool(torch.isfinite(ref[out]).all()), f"{tag}: the reference itself is not finite outside the field"
    assert bool(torch.isfinite(g[out]).all()), f"{tag}: {int((~torch.isfinite(g[out])).sum())} non-finite values outside the planted elements' field"
    if bool(out.any()):
        d, r = (g[out] - ref[out]).abs(), ref[out]
        peak = float(r.abs().max())
        fig["err"] = float(d.max())
        if "elem" in bars:
            fig["elem"] = float(d.max()) / max(1.0, peak)
            assert fig["elem"] <= bars["elem"], (tag, "elem", fig)
        if "rms" in bars and float(r.pow(2).mean()) > 0:
            fig["rms"] = float(d.pow(2).mean().sqrt() / r.pow(2).mean().sqrt())
            assert fig["rms"] < bars["rms"], (tag, "rms", fig)
        if "rel" in bars:
            fig["rel"] = float(d.max()) / max(peak, 1e-12)
            assert fig["rel"] <= bars["rel"], (tag, "rel", fig)
        if "abs" in bars:
            assert fig["err"] <= bars["abs"], (tag, "abs", fig)
        if "tol" in bars:
            tol = bars["tol"].double().expand_as(ref)[out]
            fig["of_tol"] = float((d / tol).max())
            assert bool((d <= tol).all()), (tag, "tol", fig)
    if kind == "nan":
        wrong = torch.isnan(g) != torch.isnan(ref)
        assert not bool(wrong.any()), f"{tag}: isnan differs from the reference's on {int(wrong.sum())} elements ({int((wrong & torch.isnan(ref)).sum())} NaN lost)"
    else:
        need = f & ~torch.isfinite(ref)
        assert not bool(torch.isfinite(g[need]).any()), f"{tag}: {int(torch.isfinite(g[need]).sum())} finite values where the reference is not finite"
    return fig


def same_bits_outside(got, clean, refs, tag=""):
    """Elements outside the field carry the bits of the run on the clean input (kernels whose rows / rays / voxels do not share a scale)."""
    out = ~field(refs)
    a, b = got.detach().cpu(), clean.detach().cpu()
    assert torch.equal(a[out], b[out]), f"{tag}: {int((a[out] != b[out]).sum())} elements outside the field differ from the clean run"


# ------------------------------------------------------------------------------------------------------------------------------------------
# A. convolution epilogues: rows of tests/test_f16x2_edges_gpu.py's table (and one of tests/test_conv_batch_gpu.py's)
# ------------------------------------------------------------------------------------------------------------------------------------------
def _three_voxels(shape):
    """The first voxel, an interior one (channel 1) and the last voxel's last channel of a channels-last tensor."""
    return [tuple(0 for _ in shape), tuple(s // 2 for s in shape[:-1]) + (1,), tuple(s - 1 for s in shape)]


def _middle_outside(covered):
    """Index tuple of the middle element (flattened order) of ``~covered``."""
    free = torch.nonzero(~covered.flatten()).squeeze(1)
    assert free.numel() > 0
    flat = int(free[free.numel() // 2])
    idx = []
    for s in reversed(covered.shape):
        idx.append(flat % s)
        flat //= s
    return tuple(reversed(idx))


class ConvCase:
    """One row of the fp16-pair edge table with planted inputs.  ``variant(kind)`` is the home file's _Case with x (and the residual) planted."""

    def __init__(self, dim, cin, cout, grid, k, stride, mode, relu, res, bias):
        from test_f16x2_edges_gpu import _Case
        self.base = _Case(dim, cin, cout, grid, k, stride, mode, relu, res, bias, "auto")
        self.x_places = _three_voxels(self.base.x.shape)
        self.res_place = None
        if self.base.res is not None:
            fx = torch.isnan(self._planted("nan", with_res=False).forward(torch.float64))
            if isinstance(self.base.res, tuple):          # nearest-x2 upsampled: element (n, i, j, c) of the coarse map covers a 2 x 2 block
                coarse = self.base.res[1]
                covered = torch.zeros(coarse.shape, dtype=torch.bool)
                for a in (0, 1):
                    for b in (0, 1):
                        part = fx[:, a::2, b::2]
                        covered[:, :part.shape[1], :part.shape[2]] |= part
                self.res_place = _middle_outside(covered)
            else:
                self.res_place = _middle_outside(fx)
        self._cache = {}

    def _planted(self, kind, with_res=True):
        v = copy.copy(self.base)
        v.__dict__.pop("_dev", None)
        v.x = plant(self.base.x, kind, self.x_places)
        if with_res and self.res_place is not None:
            if isinstance(self.base.res, tuple):
                v.res = ("up2", plant(self.base.res[1], kind, [self.res_place]))
            else:
                v.res = plant(self.base.res, kind, [self.res_place])
        v.ref = None
        return v

    def variant(self, kind):
        if kind not in self._cache:
            self._cache[kind] = self._planted(kind)
        return self._cache[kind]

    def compute(self, kind, dtype, bf16_operands=False):
        """The torch modules in ``dtype``; ``bf16_operands``: on weights and activations rounded to bf16 (the one-product arithmetic's definition)."""
        key = (kind, dtype, bf16_operands)
        if key not in self._cache:
            v = self.variant(kind)
            if bf16_operands:
                rounded = copy.deepcopy(v.conv)
                with torch.no_grad():
                    rounded.weight.copy_(rounded.weight.bfloat16().float())
                self._cache[key] = v.forward(dtype, conv=rounded, x=v.x.bfloat16().float())
            else:
                self._cache[key] = v.forward(dtype)
        return self._cache[key]

    def refs(self, kind, bf16_operands=False):
        return three(lambda k: self.compute(k, torch.float64, bf16_operands), kind)


@functools.lru_cache(maxsize=None)
def conv_case(dim, cin, cout, grid, k, stride, mode, relu, res, bias):
    return ConvCase(dim, cin, cout, grid, k, stride, mode, relu, res, bias)


# tile, dim, cin, cout, grid, k, stride, mode, relu, res, splits, bias -- as tests/test_f16x2_edges_gpu.py::ROWS lists them
CONV_ROWS = [
    (64, 3, 64, 128, (9, 8, 6), 3, 2, "conv", 1, 0, 1, False),            # staged, and promoted to the direct epilogue
    (128, 3, 64, 128, (9, 8, 6), 3, 2, "conv", 1, 0, 1, False),
    (64, 3, 128, 25, (10, 10, 4), 3, 1, "conv", 0, 0, 3, True),           # scalar columns; the non-vector reduce
    (12864, 3, 128, 25, (10, 10, 4), 3, 1, "conv", 0, 0, 2, False),
    (128, 3, 64, 128, (6, 6, 4), 3, 1, "conv", 2, 1, 3, False),           # split-K: the reduce pass applies the ReLU, before the residual
    (64, 3, 128, 32, (5, 4, 3), 2, 2, "tr", 1, 0, 1, False),              # k2 s2 transposed
    (128256, 3, 64, 256, (9, 8, 6), 3, 1, "conv", 1, 1, 1, False),
    (128256, 3, 128, 256, (6, 6, 4), 3, 1, "conv", 2, 1, 3, False),       # split-K
    (129256, 3, 64, 256, (9, 8, 6), 3, 1, "conv", 1, 1, 1, False),
    (129257, 3, 64, 256, (9, 8, 6), 3, 1, "conv", 1, 1, 1, False),
    (129064, 3, 128, 256, (6, 6, 4), 3, 1, "conv", 2, 1, 3, False),       # split-K
    (129256, 2, 128, 256, (1, 21, 30), 1, 1, "conv", 0, 2, 1, False),     # the nearest-x2 upsampled residual
    (3258, 3, 64, 256, (6, 8, 16), 3, 1, "conv", 2, 1, 1, False),
    (3258, 2, 128, 300, (2, 15, 20), 3, 1, "conv", 1, 1, 2, False),       # split-K, ragged Cout
    (3128, 3, 64, 128, (6, 6, 4), 3, 1, "conv", 2, 1, 1, False),          # the 128- and 256-column halo tiles on shapes of the table
    (3256, 3, 64, 256, (6, 8, 16), 3, 1, "conv", 2, 1, 1, False),
    (3257, 3, 64, 256, (6, 8, 16), 3, 1, "conv", 2, 1, 1, False),
]
# The table's rows carry the ReLU mode of their home row, which leaves some epilogue branches without a ReLU (both Cout-25 rows have none: a
# head has none).  The same shapes with the mode switched, a residual added so that "before" and "after" differ: every ReLU line of every
# epilogue code path is reached with its mode on.
_HEAD = (3, 128, 25, (10, 10, 4), 3, 1, "conv")
RELU_ROWS = [
    (64,) + _HEAD + (1, 1, 1, True),                                      # scalar columns, staged epilogue: ReLU after / before the residual
    (64,) + _HEAD + (2, 1, 1, True),
    (64,) + _HEAD + (1, 1, 3, True),                                      # ... and in the non-vector split-K reduce
    (64,) + _HEAD + (2, 1, 3, True),
    (64, 3, 64, 128, (9, 8, 6), 3, 2, "conv", 2, 1, 1, False),            # staged and direct epilogue, ReLU before the residual
    (128, 3, 64, 128, (9, 8, 6), 3, 2, "conv", 2, 1, 1, False),
    (128256, 3, 64, 256, (9, 8, 6), 3, 1, "conv", 2, 1, 1, False),        # wave-specialised and persistent tiles, unsplit, ReLU before the residual
    (129256, 3, 64, 256, (9, 8, 6), 3, 1, "conv", 2, 1, 1, False),
    (129064, 3, 64, 256, (9, 8, 6), 3, 1, "conv", 2, 1, 1, False),
    (3258, 3, 64, 256, (6, 8, 16), 3, 1, "conv", 1, 1, 1, False),         # halo epilogue, unsplit, ReLU after the residual
]
CONV_ROWS = CONV_ROWS + RELU_ROWS
BF16_CONV_ROWS = [CONV_ROWS[2], CONV_ROWS[5], CONV_ROWS[10], CONV_ROWS[13], RELU_ROWS[1], RELU_ROWS[2], RELU_ROWS[4]]   # one per family, as the home file's BF16_ROWS
F32_CONV_ROWS = [CONV_ROWS[0], CONV_ROWS[2], CONV_ROWS[4]] + RELU_ROWS[:5]     # the fp32-MFMA family has the tiles 64 and 128, 3D


def conv_row_id(r):
    return f"{r[0]}-{r[2]}to{r[3]}-{'x'.join(map(str, r[4]))}-{'tr' if r[7] == 'tr' else f'k{r[5]}s{r[6]}'}-relu{r[8]}-res{r[9]}-sp{r[10]}"


class BatchCase:
    """A tests/test_conv_batch_gpu.py row: NaN (or Inf) in the FIRST volume's last slice; every other volume must stay clean."""

    def __init__(self, n, grid, cin, cout, k, stride, mode, relu, res):
        from test_conv_batch_gpu import _Batch
        self.base = _Batch(n, grid, cin, cout, k, stride, mode, relu, res)
        self.x_places = [(0, grid[0] - 1, grid[1] // 2, grid[2] // 2, 1)]
        self._cache = {}

    def variant(self, kind):
        if kind not in self._cache:
            v = copy.copy(self.base)
            v.__dict__.pop("_dev", None)
            v.x = plant(self.base.x, kind, self.x_places)
            v.ref = None
            self._cache[kind] = v
        return self._cache[kind]

    def compute(self, kind, dtype):
        if (kind, dtype) not in self._cache:
            self._cache[(kind, dtype)] = self.variant(kind).forward(dtype)
        return self._cache[(kind, dtype)]

    def refs(self, kind):
        return three(lambda k: self.compute(k, torch.float64), kind)


BATCH_ROW = (64, 3, (3, 5, 6), 64, 40, 3, 1, "conv", 1, 1, 1)      # tile, n, grid, cin, cout, k, stride, mode, relu, res, splits: 90 rows a volume


@functools.lru_cache(maxsize=None)
def batch_case():
    return BatchCase(*BATCH_ROW[1:10])


# ------------------------------------------------------------------------------------------------------------------------------------------
# B. fused blocks
# ------------------------------------------------------------------------------------------------------------------------------------------
class ChainCase:
    """tests/test_fused_blocks_gpu.py's chained conv -> BN -> ReLU -> 1x1 conv -> BN -> (+ residual) -> ReLU."""

    def __init__(self, row):
        from test_fused_blocks_gpu import _ChainCase
        self.base = _ChainCase(*row)
        self.x_places = _three_voxels(self.base.x.shape)
        fx = torch.isnan(self._fwd(plant(self.base.x, "nan", self.x_places), self.base.res))
        self.res_place = _middle_outside(fx)
        self._cache = {}

    def _fwd(self, x, res, dtype=torch.float64):
        v = copy.copy(self.base)
        v.res = res
        if dtype == torch.float64:
            return v.forward(x)
        with torch.no_grad():          # the same modules in fp32
            y = F.relu(v.b2(v.c2(x.permute(0, 3, 1, 2))))
            y = v.b3(v.c3(y)).permute(0, 2, 3, 1)
            y = F.relu(y) if v.relu3 == 2 else y
            y = y + res if res is not None else y
            return (F.relu(y) if v.relu3 == 1 else y).contiguous()

    def inputs(self, kind):
        return plant(self.base.x, kind, self.x_places), plant(self.base.res, kind, [self.res_place])

    def compute(self, kind, dtype):
        if (kind, dtype) not in self._cache:
            self._cache[(kind, dtype)] = self._fwd(*self.inputs(kind), dtype)
        return self._cache[(kind, dtype)]

    def refs(self, kind):
        return three(lambda k: self.compute(k, torch.float64), kind)


CHAIN_ROW = (64, 64, 256, (3, 13, 17), 3, 1, True, 1)       # ROW_64 of the home file
CHAIN_RELU3 = (1, 2)                                        # ... with the last ReLU after and before the residual


@functools.lru_cache(maxsize=None)
def chain_case(relu3=1):
    return ChainCase(CHAIN_ROW[:7] + (relu3,))


class BlockCase:
    """The one-launch bottleneck of tests/test_fused_blocks_gpu.py (its border block, relu(bn1(0)) ~ 5) on an (n, h, w) map."""

    def __init__(self, ds, nhw):
        from test_fused_blocks_gpu import _border_block, _features
        self.blk = _border_block(ds)
        torch.manual_seed(1000 * nhw[0] + 37 * nhw[1] + nhw[2] + ds)
        self.x = _features(*nhw, 64 if ds else 256)
        self.x_places = _three_voxels(self.x.shape)
        self._cache = {}

    def inputs(self, kind):
        return plant(self.x, kind, self.x_places)

    def compute(self, kind, dtype):
        if (kind, dtype) not in self._cache:
            with torch.no_grad():
                blk = copy.deepcopy(self.blk).to(dtype)
                self._cache[(kind, dtype)] = blk(self.inputs(kind).permute(0, 3, 1, 2).to(dtype)).permute(0, 2, 3, 1).contiguous()
        return self._cache[(kind, dtype)]

    def refs(self, kind):
        return three(lambda k: self.compute(k, torch.float64), kind)


BLOCK_SHAPES = [(0, (1, 4, 16)), (1, (5, 3, 5))]       # (downsample form?, (n, h, w)): Cin 256 and Cin 64


@functools.lru_cache(maxsize=None)
def block_case(ds, nhw):
    return BlockCase(ds, nhw)


class ProjectionCase:
    """tests/test_conv3d_gpu.py::test_chained_projection_in_the_halo_epilogue: 3x3 conv 256 -> 256 with the 256 -> 32 mapping in its epilogue."""

    def __init__(self, nhw):
        from torch import nn
        torch.manual_seed(3256 + nhw[1])
        self.conv, self.lin = nn.Conv2d(256, 256, 3, 1, 1), nn.Linear(256, 32)
        with torch.no_grad():
            self.conv.bias.normal_(0, 0.5)
            self.lin.bias.normal_(0, 0.3)
        self.x = torch.randn(*nhw, 256)
        self.x_places = _three_voxels(self.x.shape)
        self._cache = {}

    def inputs(self, kind):
        return plant(self.x, kind, self.x_places)

    def compute(self, kind, dtype):
        if (kind, dtype) not in self._cache:
            with torch.no_grad():
                o = copy.deepcopy(self.conv).to(dtype)(self.inputs(kind).to(dtype).permute(0, 3, 1, 2)).permute(0, 2, 3, 1).contiguous()
                self._cache[(kind, dtype)] = {"out": o, "mapped": copy.deepcopy(self.lin).to(dtype)(o).reshape(-1, 32)}
        return self._cache[(kind, dtype)]

    def refs(self, kind):
        return three(lambda k: self.compute(k, torch.float64), kind)


PROJECTION_NHW = (3, 13, 21)


@functools.lru_cache(maxsize=None)
def projection_case():
    return ProjectionCase(PROJECTION_NHW)


class StemCase:
    """tests/test_stem_gpu.py's stem (7x7 s2 conv, BN, ReLU, 3x3 s2 max-pool) on (N, 3, H, W) images with three planted pixels."""

    def __init__(self, nhw):
        from test_stem_gpu import _Stem
        self.stem = _Stem(100 + sum(nhw))
        self.x = torch.randn(nhw[0], 3, nhw[1], nhw[2])
        n, h, w = nhw
        self.x_places = [(0, 0, 0, 0), (n // 2, 1, h // 2, w // 2), (n - 1, 2, h - 1, w - 1)]
        self._cache = {}

    def inputs(self, kind):
        return plant(self.x, kind, self.x_places)

    def compute(self, kind, dtype):
        if (kind, dtype) not in self._cache:
            conv, bn = copy.deepcopy(self.stem.conv).to(dtype), copy.deepcopy(self.stem.bn).to(dtype)
            with torch.no_grad():
                self._cache[(kind, dtype)] = F.max_pool2d(F.relu(bn(conv(self.inputs(kind).to(dtype)))), 3, 2, 1).permute(0, 2, 3, 1).contiguous()
        return self._cache[(kind, dtype)]

    def refs(self, kind):
        return three(lambda k: self.compute(k, torch.float64), kind)


STEM_SHAPES = [((2, 17, 23), "view"), ((2, 61, 83), "nchw")]


@functools.lru_cache(maxsize=None)
def stem_case(nhw):
    return StemCase(nhw)


class PoolCase:
    """bn_relu_maxpool_nhwc on (2, 7, 9, 64): the planted values lie (a) in a window whose other entries are larger -- pixel (0, 3, 3) is made the
    smallest of its neighbourhood in channel 5 -- and (b) in the window hanging over the lower right border, pixel (1, 6, 8), channel 63."""
    NHWC = (2, 7, 9, 64)

    def __init__(self):
        from torch import nn
        torch.manual_seed(sum(self.NHWC))
        self.bn = nn.BatchNorm2d(64).eval()
        with torch.no_grad():
            self.bn.running_mean.normal_(0, 0.3); self.bn.running_var.uniform_(0.5, 2.0); self.bn.weight.uniform_(0.5, 1.5); self.bn.bias.normal_(0, 0.3)
        self.x = torch.randn(*self.NHWC)
        self.x[0, 2:5, 2:5, 5] += 4.0                      # every neighbour of (0, 3, 3) in channel 5 is larger than what is planted over
        self.x[0, 3, 3, 5] -= 8.0
        self.x_places = [(0, 3, 3, 5), (1, 6, 8, 63)]

    def inputs(self, kind):
        return plant(self.x, kind, self.x_places)

    def compute(self, kind, dtype):
        with torch.no_grad():
            bn = copy.deepcopy(self.bn).to(dtype)
            return F.max_pool2d(F.relu(bn(self.inputs(kind).to(dtype).permute(0, 3, 1, 2))), 3, 2, 1).permute(0, 2, 3, 1).contiguous()

    def refs(self, kind):
        return three(lambda k: self.compute(k, torch.float64), kind)


    def bars(self):
        """tests/test_stem_gpu.py::test_bn_relu_maxpool_is_the_two_rounding_expression: two fp32 roundings of x scale + shift."""
        bn = self.bn
        scale = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).detach().double()
        shift = (bn.bias.detach().double() - bn.running_mean.double() * scale)
        return {"abs": 2.0 ** -22 * (float((self.inputs("clean").double() * scale).abs().max()) + float(shift.abs().max()))}


@functools.lru_cache(maxsize=None)
def pool_case():
    return PoolCase()


# ------------------------------------------------------------------------------------------------------------------------------------------
# C. BatchNorm rows
# ------------------------------------------------------------------------------------------------------------------------------------------
BN_NAMES = ["y", "dx", "dgamma", "dbeta", "running_mean", "running_var", "dres"]
BN_BAR = 3e-6          # tests/test_conv_train_gpu.py::test_batch_norm_rows_forward_backward_vs_fp64: max(3e-6, 2 x the library's own error)
BN_SHAPES = [(777, 128, True, True), (50, 64, False, True), (777, 128, True, False), (50, 64, False, False), (50, 64, True, True)]


class BnCase:
    """relu?(F.batch_norm(x) (+ residual)) on batch statistics with its gradients, as the home test's ``run`` evaluates it.  ``where``: "x" plants
    three elements of x (channels 0, 1 and C - 1: each poisons exactly its channel) and, with a residual, one residual element of another
    channel; "res" plants one residual element only."""
    MOM, EPS = 0.1, 1e-5

    def __init__(self, n, c, relu, with_res, where):
        torch.manual_seed(n + c)
        self.n, self.c, self.relu, self.where = n, c, relu, where
        self.x = torch.randn(n, c) * 1.7 + torch.linspace(-3, 3, c)
        self.res = torch.randn(n, c) if with_res else None
        self.w, self.b = torch.rand(c) + 0.5, torch.randn(c) * 0.1
        self.gy = torch.randn(n, c)
        self.x_places = [(0, 0), (n // 2, 1), (n - 1, c - 1)] if where == "x" else []
        self.res_places = [(n // 3, c // 2)] if with_res else []
        assert where == "x" or with_res
        self._cache = {}

    def inputs(self, kind):
        return plant(self.x, kind, self.x_places), None if self.res is None else plant(self.res, kind, self.res_places)

    def run(self, kind, dtype, dev="cpu", apply=None):
        """[y, dx, dgamma, dbeta, running_mean, running_var (, dres)] in ``dtype`` on ``dev``; ``apply``: BatchNormRows.apply in place of torch's."""
        x, res = self.inputs(kind)
        xs, ws, bs = (t.detach().to(dev, dtype).clone().requires_grad_(True) for t in (x, self.w, self.b))
        rs = None if res is None else res.detach().to(dev, dtype).clone().requires_grad_(True)
        rm, rv = torch.zeros(self.c, device=dev, dtype=dtype), torch.ones(self.c, device=dev, dtype=dtype)
        if apply is not None:
            y = apply(xs, ws, bs, rm, rv, self.MOM, self.EPS, self.relu, rs)
        else:
            y = F.batch_norm(xs, rm, rv, ws, bs, True, self.MOM, self.EPS)
            y = y if rs is None else y + rs
            y = torch.relu(y) if self.relu else y
        (y * self.gy.to(dev, dtype)).sum().backward()
        out = [y.detach(), xs.grad, ws.grad, bs.grad, rm, rv] + ([rs.grad] if rs is not None else [])
        return dict(zip(BN_NAMES, [t.double().cpu() for t in out]))

    def compute(self, kind, dtype):
        if (kind, dtype) not in self._cache:
            self._cache[(kind, dtype)] = self.run(kind, dtype)
        return self._cache[(kind, dtype)]

    def refs(self, kind):
        return three(lambda k: self.compute(k, torch.float64), kind)


@functools.lru_cache(maxsize=None)
def bn_case(n, c, relu, with_res, where):
    return BnCase(n, c, relu, with_res, where)


def bn_cases():
    out = [(n, c, relu, with_res, "x") for n, c, relu, with_res in BN_SHAPES]
    return out + [(n, c, relu, True, "res") for n, c, relu, with_res in BN_SHAPES if with_res]


def relu_affine_bwd_reference(g, y, scale):
    """(d_conv, d_identity) of y = relu(t * scale + ...) at a y that may hold a NaN, from autograd in float64: threshold_backward lets the
    gradient through wherever ``y <= 0`` is false."""
    t = y.double().clone().requires_grad_(True)
    torch.relu(t).backward(g.double())
    return t.grad * scale.double(), t.grad


# ------------------------------------------------------------------------------------------------------------------------------------------
# D. A6: the density MLP
# ------------------------------------------------------------------------------------------------------------------------------------------
class MlpCase:
    """tests/ray_forward_ref.py's w256_f70 module on n = 130 rows (the last 64-row workgroup is ragged): NaN / +-Inf in conditioning column 5 of
    rows 0, 64 and 129.  Outputs: trunk output h (N, 256), raw sigma (N), alpha (N)."""
    N, ARCH, COLUMN = 130, "w256_f70", 5

    def __init__(self):
        import ray_forward_ref as Rf
        self.mlp = Rf.build_mlp(self.ARCH)
        gen = torch.Generator().manual_seed(self.N)
        self.pts = torch.rand(3, self.N, generator=gen) * 6 - 3
        self.glob = torch.randn(self.N, Rf.MLP_ARCHS[self.ARCH][1], generator=gen)
        self.rows = [0, 64, self.N - 1]
        self.places = [(r, self.COLUMN) for r in self.rows]
        self._cache = {}

    def inputs(self, kind):
        return self.pts, plant(self.glob, kind, self.places)

    def compute(self, kind, dtype):
        import ray_forward_ref as Rf
        from oracle import nerfdet_oracle as O
        if (kind, dtype) not in self._cache:
            sd = {k: v.to(dtype) for k, v in self.mlp.state_dict().items() if v.is_floating_point()}
            pts, glob = self.inputs(kind)
            enc = Rf.encode_f32args(pts.t(), Rf.POS_DEG) if dtype == torch.float64 else O.sinusoidal_encode(pts.t().to(dtype), Rf.POS_DEG)
            with torch.no_grad():
                h = O._mlp_trunk(sd, torch.cat([enc, glob.to(dtype)], dim=-1))
                raw = F.linear(h, sd["mlp.sigma_layer.output_layer.weight"], sd["mlp.sigma_layer.output_layer.bias"]).reshape(-1)
            self._cache[(kind, dtype)] = {"h": h[:, :256].contiguous(), "raw": raw, "alpha": 1 - torch.exp(-torch.relu(raw))}
        return self._cache[(kind, dtype)]

    def refs(self, kind):
        return three(lambda k: self.compute(k, torch.float64), kind)

    def bars(self):
        """The bars of tests/test_volume_gpu.py::test_fused_point_mlp_* / ray_forward_ref: h within 1e-5 of its row maximum, raw sigma within
        2e-5 (1 + |sigma|), alpha within 1e-5."""
        import ray_forward_ref as Rf
        clean = self.compute("clean", torch.float64)
        return {"h": {"tol": 1e-5 * clean["h"].abs().amax(1, keepdim=True).clamp_min(1.0)},
                "raw": {"tol": Rf.SIGMA_REL * (1 + clean["raw"].abs())}, "alpha": {"abs": Rf.ALPHA_ATOL}}


@functools.lru_cache(maxsize=None)
def mlp_case():
    return MlpCase()


SIGMA_TO_ALPHA = ([float("nan"), float("inf"), -float("inf"), -1.0, 2.0], [float("nan"), 1.0, 0.0, 0.0, 1.0 - 0.1353352832366127])


# ------------------------------------------------------------------------------------------------------------------------------------------
# E. the compositor
# ------------------------------------------------------------------------------------------------------------------------------------------
class CompositeCase:
    """raw2outputs with R = 5, S = 8 and one planted sigma, ray 2, sample 3."""
    R, S, PLACE = 5, 8, (2, 3, 3)

    def __init__(self):
        import ray_forward_ref as Rf
        self.raw, self.z, self.pmask = Rf.composite_inputs(self.R, self.S)
        self._cache = {}

    def inputs(self, kind):
        return plant(self.raw, kind, [self.PLACE]), self.z, self.pmask

    def compute(self, kind, dtype):
        import ray_forward_ref as Rf
        if (kind, dtype) not in self._cache:
            raw, z, pmask = self.inputs(kind)
            out = (Rf.composite64 if dtype == torch.float64 else Rf.composite32)(raw, z, pmask, False)
            self._cache[(kind, dtype)] = {k: out[k] for k in Rf.COMPOSITE_KEYS}
        return self._cache[(kind, dtype)]

    def refs(self, kind):
        return three(lambda k: self.compute(k, torch.float64), kind)

    def bars(self):
        """ray_forward_ref's rule on this case's own clean inputs: 2e-5 on colours and depths; for weights, alpha and transparency
        max(4 x the float32 restatement's error against float64, 2^-23)."""
        import ray_forward_ref as Rf
        a, b = self.compute("clean", torch.float32), self.compute("clean", torch.float64)
        floor = {k: float((a[k].double() - b[k]).abs().max()) for k in ("weights", "alpha", "transparency")}
        return {"rgb": {"abs": Rf.ATOL}, "depth": {"abs": Rf.ATOL}, **{k: {"abs": max(4 * v, Rf.EPS32)} for k, v in floor.items()}}


@functools.lru_cache(maxsize=None)
def composite_case():
    return CompositeCase()


# ------------------------------------------------------------------------------------------------------------------------------------------
# F. the variance clamps: density_features (K2) and ray_view_stats (K4) on the recorded goldens, one NaN / Inf in one feature pixel of one view
# ------------------------------------------------------------------------------------------------------------------------------------------
STATS_TOL = (2e-5, 1e-5)      # atol, rtol of tests/test_volume_gpu.py::test_density_features_vs_oracle; tests/test_rays_gpu.py has the atol alone


class DensityCase:
    """golden volume_small_s0: the 16-channel feature maps themselves as the mapped maps (cm = 16: the packed kernel takes them, the generic
    one when forced) with a seeded bias.  The planted pixel of view 0, channel 1, is the one most voxels project to."""
    VIEW, CHANNEL = 0, 1

    def __init__(self):
        from conftest import golden_meta, load_golden
        from oracle import nerfdet_oracle as O
        g = load_golden("volume_small_s0")
        meta = golden_meta(g)
        self.h, self.w = meta["img_shape"][0] // 4, meta["img_shape"][1] // 4
        self.H, self.W = meta["img_shape"][:2]
        self.g = g
        self.mapped = g["features"][:, :, :self.h, :self.w].contiguous()
        self.bias = torch.randn(self.mapped.shape[1], generator=torch.Generator().manual_seed(16)) * 0.1
        fu, fv, fw = O.project_voxels(g["points"], g["projection"])
        x, y = fu.round().long()[self.VIEW], fv.round().long()[self.VIEW]
        ok = (x >= 0) & (y >= 0) & (x < self.w) & (y < self.h) & (fw[self.VIEW] > 0)
        pix, cnt = torch.unique((y * self.w + x)[ok], return_counts=True)
        p = int(pix[cnt.argmax()])
        self.place = (self.VIEW, self.CHANNEL, p // self.w, p % self.w)
        self._cache = {}

    def inputs(self, kind):
        return plant(self.mapped, kind, [self.place])

    def compute(self, kind, dtype):
        """nerfdet.py:234-253 as oracle.density_features states it, on maps that are mapped already: a view that does not see a voxel contributes
        the bias (the kernel's ``fill``), the mean is not zeroed at cnt == 0, the variance is unmasked, [mean_c, exp(-var_c)] interleaved.  The
        oracle's own Linear is left out: its 0 x NaN products would carry one channel's NaN into all of them, which no kernel input can.  The
        projections stay float32 (the pixel indices are the kernel's)."""
        from oracle import nerfdet_oracle as O
        if (kind, dtype) not in self._cache:
            g, b = self.g, self.bias.to(dtype)
            m = self.inputs(kind).to(dtype)
            vol, valid = O.backproject(m, g["points"], g["projection"])
            rvol, _ = O.backproject(g["denorm_images"][:, :, :self.H, :self.W].to(dtype), g["points"], g["rgb_projection"])
            both = torch.cat([rvol, torch.where(valid, vol, b.view(1, -1, 1, 1, 1))], dim=1)
            cnt = valid.sum(0)
            mean = both.sum(dim=0) / (cnt + 1e-8)
            var = torch.sum((both - mean.unsqueeze(0)) ** 2, dim=0) / (cnt + 1e-8)
            var[:, cnt[0] == 0] = 1e6
            self._cache[(kind, dtype)] = torch.stack([mean, torch.exp(-var)], dim=1).reshape(2 * mean.shape[0], -1).permute(1, 0).contiguous()
        return self._cache[(kind, dtype)]

    def refs(self, kind):
        return three(lambda k: self.compute(k, torch.float64), kind)

    def bars(self):
        return {"tol": STATS_TOL[0] + STATS_TOL[1] * self.compute("clean", torch.float64).abs()}


@functools.lru_cache(maxsize=None)
def density_case():
    return DensityCase()


class RayStatsCase:
    """golden rays_small_s0: the sampler's [mean | exp(-var)] rows; the planted feature pixel of view 0, channel 1, is an interior one under the
    first sample that view 0 sees."""
    VIEW, CHANNEL = 0, 1

    def __init__(self):
        from conftest import golden_meta, load_golden
        from oracle import nerfdet_oracle as O
        g = load_golden("rays_small_s0")
        self.g, self.meta = g, golden_meta(g)
        self.pts, self.img, self.cams, self.feat = g["pts_rnd"], g["img"], g["cameras"], g["features_2d"]
        hf, wf = self.feat.shape[2:]
        h, w = (float(v) for v in self.cams[0, 0, :2])
        pix, front = O.project_samples(self.pts, self.cams[0])
        fx, fy = pix[self.VIEW, ..., 0] / (w - 1) * (wf - 1), pix[self.VIEW, ..., 1] / (h - 1) * (hf - 1)
        ok = front[self.VIEW] & (fx > 2) & (fx < wf - 3) & (fy > 2) & (fy < hf - 3)
        r, s = (int(v) for v in torch.nonzero(ok)[0])
        self.place = (self.VIEW, self.CHANNEL, int(fy[r, s]), int(fx[r, s]))
        self._cache = {}

    def inputs(self, kind):
        return plant(self.feat, kind, [self.place])

    def compute(self, kind, dtype):
        from oracle import nerfdet_oracle as O
        if (kind, dtype) not in self._cache:
            # projection.py:91-151 with the pixel coordinates formed in float32, as the golden's inputs define them (a float64 projection moves
            # samples across the image border and across pixel boundaries of these white-noise maps: 4e-3 in the statistics, nothing to do
            # with what is tested); the bilinear samples and the statistics in ``dtype``
            cams = self.cams.squeeze(0)
            h, w = cams[0][:2]
            pix, in_front = O.project_samples(self.pts, cams)
            norm = (2 * pix / torch.tensor([w - 1.0, h - 1.0])[None, None, :] - 1.0).to(dtype)
            rgb = F.grid_sample(self.img.to(dtype), norm, align_corners=True).permute(2, 3, 0, 1)
            ft = F.grid_sample(self.inputs(kind).to(dtype), norm, align_corners=True).permute(2, 3, 0, 1)
            inb = (pix[..., 0] <= w - 1.0) & (pix[..., 0] >= 0) & (pix[..., 1] <= h - 1.0) & (pix[..., 1] >= 0)
            mask = (inb * in_front).to(dtype).permute(1, 2, 0)[..., None]
            mean, var = O.compute_mask_points(torch.cat([rgb, ft], dim=-1), mask)
            self._cache[(kind, dtype)] = torch.cat([mean, var], dim=-1).squeeze(2)
        return self._cache[(kind, dtype)]

    def refs(self, kind):
        return three(lambda k: self.compute(k, torch.float64), kind)

    def bars(self):
        """2e-5 absolute (tests/test_rays_gpu.py), but for the rows of samples NO view sees: there the statistics are divided by the reference's
        1e-8 instead of a view count, which magnifies the float32 rounding of a bilinear sample 1e8 times (one such row of this golden has
        a tap weight of 1e-6 on a map's edge: the float32 CPU restatement itself is 2.5e-3 from float64 in its exp(-var)).  A property of
        float32.  Only the rows of :meth:`widened_rows` -- unseen AND missed by float32 itself -- get 4 x the float32 restatement's own error on
        the row (ray_forward_ref's rule for such bars); every other row, unseen ones included, keeps the flat 2e-5."""
        tol = torch.full_like(self.compute("clean", torch.float64), STATS_TOL[0])
        rows, own = self.widened_rows()
        tol[rows] = 4 * own[rows]
        return {"tol": tol}

    def widened_rows(self):
        """((R, S) mask of the rows whose bar is not the flat 2e-5, (R, S, 1) the float32 restatement's own error per row): exactly the rows that no
        view sees AND on which the float32 restatement itself misses 2e-5 (one row of this golden; the CPU test asserts the count)."""
        a, b = self.compute("clean", torch.float32).double(), self.compute("clean", torch.float64)
        own = (a - b).abs().amax(-1, keepdim=True)
        unseen = self.g["mask"][..., 0].sum(dim=2) == 0
        return unseen & (own.squeeze(-1) > STATS_TOL[0]), own


@functools.lru_cache(maxsize=None)
def ray_stats_case():
    return RayStatsCase()
