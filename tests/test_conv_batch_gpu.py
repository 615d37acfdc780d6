"""The batched split-family 3D convolution (conv3d.conv3d_ndhwc on (N,D,H,W,Cin) -> one ndet_conv_split_batch launch; csrc/conv_split_kernels.hip,
the kernels' SCH + SPL_BATCH instantiations) on every tile family that takes a batch, at the smallest shapes that put a tile across a volume
boundary.  The layers are those of mmdet3d/models/necks/imvoxelnet.py:22-67,233-260 and dense_heads/imvoxel_head_v2.py:45-49, which the
reference runs on nn.Conv3d's batch axis.  Inputs are standard normal everywhere, first and last slices of every volume included, so a tap that
leaks into the neighbouring volume is an O(1) error.  Every row asserts

1. agreement with an fp64 CPU convolution of each volume on its own: the bars of tests/test_f16x2_edges_gpu.py (2e-5 max(1, max|ref|)
   elementwise, 2e-6 rel-rms) for f16x2 and bf16x3, that file's bf16 bar (2e-5 max|ref| against the bf16-rounded operands' convolution) for bf16;
2. bit equality with N single-volume launches at the same tile and splits (f16x2: every volume holds one element of 6.0, above anything a
   standard normal gives here, so each volume's own maximum lies in the batch's binade [4, 8) and the power-of-two scale is the same);
3. the output's amax slot == max|out| over the batch, exactly;
4. through conv3d.launch_hook: exactly one launch, of the named tile's kernel ("/batch" form), tile and splits as asked;
5. batch = 1 through ndet_conv_split_batch gives ndet_conv_split's bits.

Which form of halo_geometry the halo rows run (pinned through the launcher's own rule in tests/test_conv_batch_cpu.py; both are taken): 3128 at 3x6x10 stages the depth taps
INSIDE the halo image (patch 4x8x4, 1x1x3 patches a volume); 3256 / 3257 / 3258 at 3x6x10 LOOP the depth taps outside it (patch 1x8x16, 3x1x1
patches a volume, so the volume index is divided out of a depth patch index), and so does 3128 at 1x8x16 (one patch a volume, both depth
neighbours of every voxel outside the volume)."""
import copy
import functools

import pytest
import torch
from torch import nn

from test_f16x2_edges_gpu import ELEM_BAR, RMS_BAR, _errors, _forward, _slot_is_exact

pytestmark = pytest.mark.gpu

PIN = 6.0       # see 2. above


class _Batch:
    """One layer and a batch of volumes on the CPU, with the fp64 result of every volume convolved on its own: built once per shape, shared."""

    def __init__(self, n, grid, cin, cout, k, stride, mode, relu, res):
        torch.manual_seed(17 * n + 1000 * cin + 3 * cout + 7 * k + stride + sum(grid) + relu + 5 * res)
        self.relu = relu
        if mode == "tr":
            self.conv = nn.ConvTranspose3d(cin, cout, 2, 2, bias=False)
        else:
            self.conv = nn.Conv3d(cin, cout, k, stride, k // 2 if k > 1 else 0, bias=False)
        self.bn = nn.BatchNorm3d(cout).eval()
        with torch.no_grad():
            self.bn.weight.uniform_(0.5, 1.5); self.bn.bias.normal_(0, 0.2); self.bn.running_mean.normal_(0, 0.2); self.bn.running_var.uniform_(0.5, 1.5)
        self.x = torch.randn(n, *grid, cin)
        assert float(self.x.abs().max()) < PIN
        self.x[:, grid[0] // 2, grid[1] // 2, grid[2] // 2, 0] = PIN
        with torch.no_grad():
            probe = _forward(self.conv, self.bn, self.x[0], 3, 0, None)
            self.res = torch.randn(n, *probe.shape) if res else None
            self.ref = self.forward(torch.float64)

    def forward(self, dtype, conv=None, x=None):
        conv = copy.deepcopy(self.conv if conv is None else conv).to(dtype)
        bn = copy.deepcopy(self.bn).to(dtype)
        x = self.x if x is None else x
        with torch.no_grad():
            return torch.stack([_forward(conv, bn, x[i].to(dtype), 3, self.relu, None if self.res is None else self.res[i]) for i in range(x.shape[0])])

    def on(self, device):
        from nerfdet_amd import conv3d as C
        if not hasattr(self, "_dev"):
            conv_d, bn_d = copy.deepcopy(self.conv).to(device), copy.deepcopy(self.bn).to(device)
            self._dev = (conv_d, bn_d, C.packed([conv_d], bn_d), None if self.res is None else self.res.to(device))
        return self.x.to(device), self._dev[2], self._dev[3]


@functools.lru_cache(maxsize=None)
def _batch(n, grid, cin, cout, k, stride, mode, relu, res):
    return _Batch(n, grid, cin, cout, k, stride, mode, relu, res)


def _run(device, arith, tile, splits, fn):
    """``fn()`` under ``arith`` with the launch hook and conv_tiles.resolve watched: (result, kernel names, resolved (tile, splits) per launch)."""
    from nerfdet_amd import conv3d as C, conv_tiles
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
        with torch.no_grad():
            y = fn()
        torch.cuda.synchronize()
    finally:
        C.set_arithmetic(prev)
        C.launch_hook, conv_tiles.resolve = prev_hook, real_resolve
    return y, names, resolved


def _row(tile, n, grid, cin, cout, k, stride, relu, res, splits, ariths=("f16x2",), mode="conv"):
    name = f"{tile}-n{n}-{'x'.join(map(str, grid))}-{cin}to{cout}-{'tr' if mode == 'tr' else f'k{k}s{stride}'}-relu{relu}-res{res}-sp{splits}"
    return [pytest.param(tile, n, grid, cin, cout, k, stride, mode, relu, res, splits, a, id=f"{name}-{a}") for a in ariths]


BOTH = ("f16x2", "bf16x3")
ROWS = (
    # tile, N, one volume's D x H x W, Cin, Cout, k, stride, relu (1 after / 2 before the residual), residual, splits, arithmetics
    # ---- unified 64: 90 rows a volume, so the 64-row tiles straddle; Cout 40 stays staged, Cout 64 with splits 1 is promoted to the direct form ----
    _row(64, 3, (3, 5, 6), 64, 40, 3, 1, 1, 1, 1, BOTH) + _row(64, 3, (3, 5, 6), 64, 40, 3, 1, 1, 1, 2)
    + _row(64, 3, (3, 5, 6), 64, 64, 3, 1, 1, 1, 1, BOTH) + _row(64, 3, (3, 5, 6), 64, 64, 3, 1, 1, 1, 2)
    + _row(64, 3, (3, 5, 6), 64, 64, 3, 1, 2, 1, 1)                                  # the up block's form: ReLU, then the skip add
    # ---- unified 128 (direct) and 12864 (staged): stride 2 on an ODD depth, 5x6x7 -> 3x3x4: stacking the volumes along depth would be wrong ----
    + _row(128, 2, (5, 6, 7), 64, 96, 3, 2, 1, 0, 1, BOTH) + _row(12864, 2, (5, 6, 7), 64, 40, 3, 2, 1, 0, 1)
    # ---- the downsample: 1x1x1 stride 2 (one K step: the mixed mode keeps it on the bf16x3 kernel, as in production) ----
    + _row(64, 3, (3, 4, 6), 32, 64, 1, 2, 0, 0, 1, BOTH)
    # ---- k2 s2 transposed, with ReLU ----
    + _row(64, 2, (2, 3, 5), 64, 32, 2, 2, 1, 0, 1, BOTH, mode="tr")
    # ---- wave-specialised 128 x 256: 120 rows a volume ----
    + _row(128256, 2, (4, 6, 5), 64, 256, 3, 1, 1, 1, 1, ("f16x2", "bf16x3", "bf16")) + _row(128256, 2, (4, 6, 5), 64, 256, 3, 1, 1, 1, 2)
    + _row(128256, 2, (2, 3, 5), 128, 256, 2, 2, 1, 0, 1, BOTH, mode="tr")         # its k2 s2 transposed form (an up block wider than 128 channels)
    # ---- halo-stationary ----
    + _row(3128, 3, (3, 6, 10), 64, 128, 3, 1, 1, 1, 1, BOTH) + _row(3128, 3, (3, 6, 10), 64, 128, 3, 1, 1, 1, 2)
    + _row(3256, 3, (3, 6, 10), 64, 256, 3, 1, 1, 1, 1) + _row(3257, 3, (3, 6, 10), 64, 256, 3, 1, 1, 1, 1) + _row(3258, 3, (3, 6, 10), 64, 256, 3, 1, 1, 1, 1)
    + _row(3256, 3, (3, 6, 10), 64, 256, 3, 1, 1, 1, 2)
    # depth 1 with kd = 3: both depth neighbours of every voxel lie outside its volume -- any leak reads the next volume's values
    + _row(3128, 4, (1, 8, 16), 64, 128, 3, 1, 1, 0, 1, BOTH)
)


@pytest.mark.parametrize("tile,n,grid,cin,cout,k,stride,mode,relu,res,splits,arith", ROWS)
def test_batched_conv_row(device, request, tile, n, grid, cin, cout, k, stride, mode, relu, res, splits, arith):
    from nerfdet_amd import _lib, conv3d as C, conv_tiles
    case = _batch(n, grid, cin, cout, k, stride, mode, relu, res)
    x, pk, r = case.on(device)
    k_iters = (1 if mode == "tr" else k ** 3) * cin // 32
    ran = arith if arith != "f16x2" or k_iters >= C.F16_MIN_KSTEPS else "bf16x3"          # (conv3d.layer_arithmetic)
    direct_ok = conv_tiles.TILES[tile].family == "unified" and splits == 1 and mode != "tr" and cout % 32 == 0
    want_tile = conv_tiles.TILES[tile].partner if direct_ok else tile
    want_name = conv_tiles.TILES[tile].name + ("/f16x2" if ran == "f16x2" else "")

    got, names, resolved = _run(device, arith, tile, splits, lambda: C.conv3d_ndhwc(x, pk, residual=r, relu=relu, splits=splits, tile=tile))
    # 4. one launch, the named tile's batched kernel, nothing re-routed
    assert names == [want_name + "/batch"] and resolved == [(want_tile, splits)], (names, resolved)
    assert tuple(got.shape) == tuple(case.ref.shape) and got.is_contiguous()
    # 3. the slot the launch leaves behind
    if arith == "f16x2":
        _slot_is_exact(got)
    else:
        assert not hasattr(got, "_ndet_amax")
    # 1. every volume against its own fp64 convolution
    if arith == "bf16":
        rounded = copy.deepcopy(case.conv)
        with torch.no_grad():
            rounded.weight.copy_(rounded.weight.bfloat16().float())
        ref = case.forward(torch.float64, conv=rounded, x=case.x.bfloat16().float())
        scale = float(ref.abs().max())
        err = float((got.double().cpu() - ref).abs().max())
        print(f"BATCH {request.node.callspec.id}: bf16 |got - ref(bf16 operands)| {err / scale:.2e} max|ref|")
        assert err <= 2e-5 * scale
        assert float((got.double().cpu() - case.ref).abs().max()) >= 1e-4 * scale
    else:
        elem, rms = _errors(got, case.ref)
        per_vol = [_errors(got[i], case.ref[i])[0] for i in range(n)]
        print(f"BATCH {request.node.callspec.id}: elem {elem:.2e} rel-rms {rms:.2e} per volume {['%.1e' % e for e in per_vol]}")
        assert elem <= ELEM_BAR and rms < RMS_BAR, (elem, rms)
    # 2. N single-volume launches at the same tile and splits: the same bits
    singles, names, resolved = _run(device, arith, tile, splits, lambda: [C.conv3d_ndhwc(x[i], pk, residual=None if r is None else r[i], relu=relu,
                                                                                        splits=splits, tile=tile) for i in range(n)])
    assert names == [want_name] * n and resolved == [(want_tile, splits)] * n, (names, resolved)
    for i in range(n):
        assert torch.equal(got[i], singles[i]), f"volume {i} of the batch differs from its own launch"
    # 5. batch = 1 through the new entry point: ndet_conv_split's launch
    lib = _lib.load()
    real = lib.ndet_conv_split
    try:
        lib.ndet_conv_split = lambda a, st: lib.ndet_conv_split_batch(a, 1, st)
        one, names, _ = _run(device, arith, tile, splits, lambda: C.conv3d_ndhwc(x[0], pk, residual=None if r is None else r[0], relu=relu,
                                                                                 splits=splits, tile=tile))
    finally:
        lib.ndet_conv_split = real
    assert names == [want_name] and torch.equal(one, singles[0])


def test_five_d_input_in_other_settings(device):
    """A batch of one is the 4-D launch (no batched kernel); the fp32-MFMA family refuses a 5-D input with a clear error; the persistent tiles are
    sent to 128256 by conv_tiles.resolve, and the library refuses them when asked directly."""
    from nerfdet_amd import conv3d as C
    case = _batch(2, (4, 6, 5), 64, 256, 3, 1, "conv", 1, 1)
    x, pk, r = case.on(device)
    one, names, _ = _run(device, "f16x2", 128256, 1, lambda: C.conv3d_ndhwc(x[:1], pk, residual=r[:1], relu=1, splits=1, tile=128256))
    single, _, _ = _run(device, "f16x2", 128256, 1, lambda: C.conv3d_ndhwc(x[0], pk, residual=r[0], relu=1, splits=1, tile=128256))
    assert names == ["k_conv_split_ws/f16x2"] and one.shape[0] == 1 and torch.equal(one[0], single)
    with pytest.raises(ValueError, match="5-D"):
        _run(device, "f32", 0, 0, lambda: C.conv3d_ndhwc(x, pk, residual=r, relu=1))
    got, names, resolved = _run(device, "f16x2", 129256, 1, lambda: C.conv3d_ndhwc(x, pk, residual=r, relu=1, splits=1, tile=129256))
    assert names == ["k_conv_split_ws/f16x2/batch"] and resolved == [(128256, 1)]
    ws, _, _ = _run(device, "f16x2", 128256, 1, lambda: C.conv3d_ndhwc(x, pk, residual=r, relu=1, splits=1, tile=128256))
    assert torch.equal(got, ws)
