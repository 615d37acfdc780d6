"""The weight-gradient kernels (csrc/conv_split_kernels.hip: k_wgrad_split, k_wgrad_to_torch; nerfdet_amd/conv_train.py::weight_grad) on the branches a
training step runs: 8, 16, 24 and 32 K splits with the XCD workgroup remap on and off, every tile up to 128 x 256 with one and two column tiles,
output grids one voxel and more than 32 voxels wide, strides 1 and 2, 2D and 3D, and the partial sum of more than nine splits in k_wgrad_to_torch.

Reference: dW[co][ci][t] = sum_j x[s o(j) + t - p][ci] dy[j][co], stated here as one fp64 matmul per tap over zero-padded strided slices of x (on
the device; nothing of conv_train / conv3d is called).  Bar: max |got - ref| <= max(2e-5, 2 e32) max |ref|, e32 the error of the SAME statement
evaluated in plain fp32 -- 2e-5 is the project's bar for this quantity (test_conv_train_gpu.py), the factor 2 the margin
test_neck_training_step_matches_library_path grants over the library path; the sums here run over up to 16 900 voxels.

Every case states the launch it exists for -- tile, split count, keep flag -- as conv_train.implicit_plan gives it (pinned without a GPU in
test_wgrad_plan_cpu.py) and checks what weight_grad handed to ndet_wgrad_split / _to_torch_layout against it.  The TILE is the library's own choice
from (taps, Cin, Cout, arithmetic, knob wgrad_wide); `_library_tile` restates that rule, it cannot be read back from a launch.

Measured on an MI355X, relative to max |ref| (fp16 pairs / bf16x3 / the fp32 statement; the bar was 2e-5 in every case, 2 e32 never above 3.4e-6):
  ladder-8   2.4e-7 / 2.7e-7 / 4.3e-7     ladder-16  2.6e-7 / 2.8e-7 / 5.0e-7     ladder-24  2.7e-7 / 2.8e-7 / 8.6e-7     ladder-32  2.5e-7 / 3.0e-7 / 1.0e-6
  auto-32 dW 3.1e-7 / 3.7e-7 / 1.6e-6     auto-32 dx 5.9e-7 / 8.9e-7 / 2.2e-7
  tile-128x256 2.3e-7 / 3.0e-7 / 5.4e-7 (wgrad_wide = 0: 2.3e-7)   tile-128x256-2col 2.2e-7 / 3.5e-7 / 5.4e-7      tile-128x64 2.1e-7 / 2.7e-7 / 4.9e-7
  tile-64x128-ragged 2.1e-7 / 2.4e-7 / 4.5e-7                      tile-64x64-ragged 2.0e-7 / 2.5e-7 / 3.9e-7
  ow-1 2.0e-7 / 2.9e-7 / 5.5e-7    ow-33 3.1e-7 / 3.2e-7 / 5.6e-7    stride2-3d 2.2e-7 / 3.1e-7 / 4.5e-7    k2s2 2.3e-7 / 2.6e-7 / 5.6e-7
  2d 2.0e-7 / 2.9e-7 / 4.8e-7      2d-stride2 2.5e-7 / 2.8e-7 / 6.2e-7
  impulses (exact products, nothing to sum) 1.0e-7 / 4.4e-8
  staged-1x1-6498 3.4e-7 / 4.2e-7 / 7.4e-7     staged-1x1-16900 4.0e-7 / 5.2e-7 / 1.7e-6     staged-k2s2 5.6e-7 / 8.7e-7 / 5.6e-7
The tiling tables split the staged GEMMs 8, 22 and 2 ways (STAGED below): the keep path into ndet_wgrad_to_torch ran with splits > 1 in all three.
"""
import contextlib
import functools
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ARITHS = ("f16x2", "bf16x3")
BAR = 2e-5

# name -> (input grid, Cin, Cout, kernel, stride, pads (None: same-padded), {arithmetic: (bm, bn, splits)})
_S = lambda s: {"f16x2": (64, 64, s), "bf16x3": (64, 64, s)}      # noqa: E731
LADDER = {
    "ladder-8": ((12, 12, 11), 64, 64, (3, 3, 3), 1, None, _S(8)),          # 1584 voxels, 50 K steps (8 does not divide them)
    "ladder-16": ((13, 13, 14), 64, 64, (3, 3, 3), 1, None, _S(16)),        # 2366 voxels, 74 K steps
    "ladder-24": ((17, 17, 15), 64, 64, (3, 3, 3), 1, None, _S(24)),        # 4335 voxels, 136 K steps
    "ladder-32": ((19, 19, 18), 64, 64, (3, 3, 3), 1, None, _S(32)),        # 6498 voxels, 204 K steps
}
AUTO = {"auto-32": ((26, 26, 25), 64, 64, (3, 3, 3), 1, None, _S(32))}      # 16 900 voxels >= 16 384: weight_grad takes the kernel by itself
TILES = {
    "tile-128x256": ((12, 12, 11), 256, 256, (3, 3, 3), 1, None, {"f16x2": (128, 256, 8), "bf16x3": (128, 128, 8)}),     # 54 row tiles
    # two column tiles: the remap sees gridDim.y = 2 (the six-product arithmetic has no 256-column tile: 216 tiles of 128 x 128, 5 splits, no remap)
    "tile-128x256-2col": ((12, 12, 11), 256, 512, (3, 3, 3), 1, None, {"f16x2": (128, 256, 8), "bf16x3": (128, 128, 5)}),
    "tile-128x64": ((12, 12, 11), 128, 64, (3, 3, 3), 1, None, {"f16x2": (128, 64, 8), "bf16x3": (128, 64, 8)}),
    "tile-64x128-ragged": ((12, 12, 11), 64, 96, (3, 3, 3), 1, None, {"f16x2": (64, 128, 8), "bf16x3": (64, 128, 8)}),   # rows 96 .. 127 of the B tile masked
    "tile-64x64-ragged": ((12, 12, 11), 64, 25, (3, 3, 3), 1, None, _S(8)),           # ... and a ragged Cout in k_wgrad_to_torch
}
GEOMETRY = {
    "ow-1": ((44, 36, 1), 64, 64, (3, 3, 3), 1, None, _S(8)),                 # the voxel walk wraps 32 times a step
    "ow-33": ((6, 8, 33), 64, 64, (3, 3, 3), 1, None, _S(8)),                 # ... at most once
    "stride2-3d": ((23, 23, 22), 64, 64, (3, 3, 3), 2, None, _S(8)),          # -> (12, 12, 11)
    "k2s2": ((24, 24, 22), 64, 64, (2, 2, 2), 2, (0, 0, 0), _S(8)),           # what ConvT2.backward calls with the roles of x and dy swapped
    "2d": ((3, 24, 22), 64, 64, (3, 3), 1, None, _S(8)),
    "2d-stride2": ((3, 47, 43), 64, 64, (3, 3), 2, None, _S(8)),              # -> (3, 24, 22)
}
CASES = {**LADDER, **AUTO, **TILES, **GEOMETRY}
# 1x1 layers and the unpadded 2x2x2 take the staged form (tap copies + one GEMM of the convolution kernel, its split-K partials kept for
# ndet_wgrad_to_torch): name -> (grid, Cin, Cout, kernel, stride, pads, K splits the tiling tables choose for the (taps Cin) x Cout x L GEMM)
STAGED = {
    "staged-1x1-6498": ((19, 19, 18), 64, 256, (1, 1, 1), 1, None, 8),
    "staged-1x1-16900": ((26, 26, 25), 64, 256, (1, 1, 1), 1, None, 22),
    "staged-k2s2": ((24, 24, 22), 64, 64, (2, 2, 2), 2, (0, 0, 0), 2),
}


def geometry(dims, kernel, stride, pads):
    """(k3, s3, p3, output grid) of a case: 2D kernels take the batch as a depth axis of extent-1 taps, as weight_grad does."""
    two_d = len(kernel) == 2
    k3 = ((1,) + tuple(kernel)) if two_d else tuple(kernel)
    s3 = (1, stride, stride) if two_d else (stride,) * 3
    p3 = tuple(v // 2 for v in k3) if pads is None else (((0,) + tuple(pads)) if two_d else tuple(pads))
    return k3, s3, p3, tuple((n + 2 * p - k) // s + 1 for n, p, k, s in zip(dims, p3, k3, s3))


def _library_tile(taps, cin, cout, f16, wide=True):
    """The tile ndet_wgrad_split launches (csrc/conv_split_kernels.hip), restated."""
    if cin % 128 == 0 and f16 and cout % 256 == 0 and taps * (cin // 128) >= 32 and wide:
        return 128, 256
    return (128 if cin % 128 == 0 else 64), (128 if cout > 64 else 64)


def _dw_statement(x, dy, k3, s3, p3, dtype):
    """The weight gradient as the module docstring states it, in ``dtype``: (Cout, Cin, taps)."""
    od, oh, ow, cout = dy.shape
    cin = x.shape[3]
    xp = F.pad(x.to(dtype), (0, 0, p3[2], p3[2], p3[1], p3[1], p3[0], p3[0]))
    g = dy.to(dtype).reshape(-1, cout).t().contiguous()                    # (Cout, L)
    out = torch.empty((cout, cin, k3[0] * k3[1] * k3[2]), dtype=dtype, device=x.device)
    for t, (a, b, c) in enumerate(itertools.product(range(k3[0]), range(k3[1]), range(k3[2]))):
        xs = xp[a:a + s3[0] * (od - 1) + 1:s3[0], b:b + s3[1] * (oh - 1) + 1:s3[1], c:c + s3[2] * (ow - 1) + 1:s3[2]]
        out[:, :, t] = g @ xs.reshape(-1, cin)
    return out


def _dx_statement(dy, w, dtype):
    """Data gradient of a same-padded stride-1 3D convolution: dx[i][ci] = sum_t sum_co dy[i - t + p][co] w[co][ci][t], (D, H, W, Cin) in ``dtype``."""
    d, h, wd, cout = dy.shape
    k = w.shape[2:]
    p = [v // 2 for v in k]
    gp = F.pad(dy.to(dtype), (0, 0, p[2], p[2], p[1], p[1], p[0], p[0]))
    wt = w.to(dtype)
    out = torch.zeros((d * h * wd, w.shape[1]), dtype=dtype, device=dy.device)
    for a, b, c in itertools.product(range(k[0]), range(k[1]), range(k[2])):
        gs = gp[k[0] - 1 - a:k[0] - 1 - a + d, k[1] - 1 - b:k[1] - 1 - b + h, k[2] - 1 - c:k[2] - 1 - c + wd]
        out += gs.reshape(-1, cout) @ wt[:, :, a, b, c]
    return out.view(d, h, wd, -1)


def _rel(got, ref):
    return float((got.double() - ref).abs().max()) / float(ref.abs().max())


@functools.lru_cache(maxsize=None)
def _case(name):
    """(x, dy, fp64 reference, error of the fp32 statement) of a case, on the device; shared by every test that runs the case, never written to."""
    dims, cin, cout, kernel, stride, pads = {**CASES, **STAGED}[name][:6]
    k3, s3, p3, out_dims = geometry(dims, kernel, stride, pads)
    dev = torch.device("cuda:0")
    torch.manual_seed(sum(dims) + cin + cout)
    x = torch.randn(*dims, cin, device=dev)
    dy = torch.randn(*out_dims, cout, device=dev)
    ref = _dw_statement(x, dy, k3, s3, p3, torch.float64)
    e32 = _rel(_dw_statement(x, dy, k3, s3, p3, torch.float32), ref)
    return x, dy, ref, e32


@pytest.fixture
def arith(request):
    """The training arithmetic of the case (parametrised indirectly): fp16 pairs (the default) or the six-product bf16x3 kernels."""
    import nerfdet_amd.conv3d as C
    prev, C.TRAIN_F16X2 = C.TRAIN_F16X2, request.param == "f16x2"
    yield request.param
    C.TRAIN_F16X2 = prev


@pytest.fixture
def launches(monkeypatch, device):
    """Records what weight_grad hands to the library: ``split`` -- (splits, keep) of every ndet_wgrad_split call, ``layout`` -- the split count of
    every _to_torch_layout call (the partials ndet_wgrad_to_torch adds)."""
    from nerfdet_amd import _lib, conv_train
    lib = _lib.load()
    rec = {"split": [], "layout": []}
    split, layout = lib.ndet_wgrad_split, conv_train._to_torch_layout

    def rec_split(*a):           # (x, D, H, W, Cin, kernel, stride, pad, planes, Cout, lrow, splits, arith, x_amax, dy_amax, ws, dw, keep, stream)
        rec["split"].append((int(a[11]), bool(a[17])))
        return split(*a)

    def rec_layout(rows, taps, cin, cout, kernel, splits=1):
        rec["layout"].append(int(splits))
        return layout(rows, taps, cin, cout, kernel, splits)
    monkeypatch.setattr(lib, "ndet_wgrad_split", rec_split)
    monkeypatch.setattr(conv_train, "_to_torch_layout", rec_layout)
    return rec


@contextlib.contextmanager
def _knobs(**values):
    """The library's measurement knobs wgrad_xcd / wgrad_wide for the block; both back to 1 afterwards."""
    from nerfdet_amd import _lib
    lib = _lib.load()
    try:
        for k, v in values.items():
            _lib.check(lib.ndet_measurement_knob(k.encode(), v), "knob")
        yield
    finally:
        for k in ("wgrad_xcd", "wgrad_wide"):
            _lib.check(lib.ndet_measurement_knob(k.encode(), 1), "knob")


def _expect_plan(name, arith, wide=True):
    """Asserts that the case still reaches the branch it is named for and returns (splits, keep)."""
    from nerfdet_amd.conv_train import implicit_plan
    dims, cin, cout, kernel, stride, pads, plans = CASES[name]
    lo = math.prod(geometry(dims, kernel, stride, pads)[3])
    bm, bn, splits = plans[arith]
    f16 = arith == "f16x2"
    keep = f16 and splits > 1
    assert implicit_plan(math.prod(kernel), cin, cout, lo, f16) == (bm, bn, splits, keep), name
    assert _library_tile(math.prod(kernel), cin, cout, f16) == (bm, bn), name
    if not wide:
        assert (bm, bn) == (128, 256) and _library_tile(math.prod(kernel), cin, cout, f16, False) == (128, 128), name
    return splits, keep


def _poison(device, taps, cin, cout, splits):
    """NaN into what weight_grad is about to take with torch.empty -- the split-K workspace, the GEMM rows, the result: the caching allocator hands a
    freed block to the next request of its size, and a tile or a split the kernel never writes would otherwise read what an earlier case of the same
    shape left there (seen with a broken remap: the stale partials of the previous case were the right answer).
    That is the allocator's habit, not a guarantee: tests/redzone.py carves every such allocation and fills it itself (tests/test_redzone_train_gpu.py)."""
    blocks = [torch.full((n,), float("nan"), device=device) for n in (splits * taps * cin * cout, taps * cin * cout, cout * cin * taps)]
    del blocks


def _run(name, arith, launches, implicit=True):
    """weight_grad of a case with the launch check; the gradient as (Cout, Cin, taps)."""
    from nerfdet_amd import conv_train
    dims, cin, cout, kernel, stride, pads = CASES[name][:6]
    x, dy, _, _ = _case(name)
    launches["split"].clear(), launches["layout"].clear()
    _poison(x.device, math.prod(kernel), cin, cout, CASES[name][6][arith][2])
    got = conv_train.weight_grad(x, dy, kernel, stride, pads, implicit=implicit)
    assert got.shape == (cout, cin) + tuple(kernel)
    return got.reshape(cout, cin, -1)


def _check(name, arith, got, ref, e32, what="dW"):
    err = _rel(got, ref)
    bar = max(BAR, 2.0 * e32)
    print(f"{name} {arith} {what}: kernel {err:.2e}  fp32 statement {e32:.2e}  bar {bar:.2e}")
    assert bool(torch.isfinite(got).all()), name
    assert err <= bar, f"{name} {arith} {what}: {err:.3e} > {bar:.3e} (fp32 statement: {e32:.3e})"


def _params(names, ariths=ARITHS, skip=()):
    return [pytest.param(n, a, id=f"{n}-{a}") for n in names for a in ariths if (n, a) not in skip]


@pytest.mark.parametrize("name,arith", _params(list(LADDER) + list(TILES) + list(GEOMETRY)), indirect=["arith"])
def test_implicit_weight_gradient_at_production_splits_and_tiles(device, launches, name, arith):
    """(a), (c), (d) of the module's cases: the split ladder 8 / 16 / 24 / 32, every tile at >= 8 splits, the geometries of the voxel walk."""
    splits, keep = _expect_plan(name, arith)
    got = _run(name, arith, launches)
    assert launches["split"] == [(splits, keep)] and launches["layout"] == [splits if keep else 1], launches
    _, _, ref, e32 = _case(name)
    _check(name, arith, got, ref, e32)


def test_narrow_tile_knob_at_8_splits(device, launches):
    """256 -> 256, 3x3x3 with wgrad_wide = 0: the 128 x 128 tile at the split count planned for the 128 x 256 tile (fp16 pairs)."""
    import nerfdet_amd.conv3d as C
    name = "tile-128x256"
    assert C.train_arithmetic() == "f16x2"
    splits, keep = _expect_plan(name, "f16x2", wide=False)
    with _knobs(wgrad_wide=0):
        got = _run(name, "f16x2", launches)
    assert launches["split"] == [(splits, keep)] and launches["layout"] == [splits]
    _, _, ref, e32 = _case(name)
    _check(name + "/wide=0", "f16x2", got, ref, e32)


@pytest.mark.parametrize("arith", ARITHS, indirect=True)
def test_autograd_takes_the_implicit_kernel_by_itself(device, launches, arith):
    """(b): ConvS1 forward + backward on 16 900 voxels -- the production call site, ``implicit=None``: 32 splits; dW and dx against fp64."""
    from nerfdet_amd.conv_train import ConvS1
    name = "auto-32"
    splits, keep = _expect_plan(name, arith)
    x, dy, ref, e32 = _case(name)
    torch.manual_seed(7)
    w = torch.randn(64, 64, 3, 3, 3, device=device) / (64 * 27) ** 0.5
    xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    out = ConvS1.apply(xg, wg, 1)
    _poison(device, 27, 64, 64, splits)
    (out * dy).sum().backward()
    assert launches["split"] == [(splits, keep)] and launches["layout"] == [splits if keep else 1], launches
    _check(name, arith, wg.grad.reshape(64, 64, 27), ref, e32)
    dx_ref = _dx_statement(dy, w, torch.float64)
    _check(name, arith, xg.grad, dx_ref, _rel(_dx_statement(dy, w, torch.float32), dx_ref), "dx")


def impulse_voxels(lo, splits):
    """[(channel, voxel)] of the impulses: the first voxel of every split and the voxel before it, one channel each (channel 2z: first voxel of split z,
    2z - 1: the voxel before it), and in the last channel both the last voxel of the last full K step and voxel L - 1."""
    ksteps = (lo + 31) // 32
    first = [32 * (ksteps * z // splits) for z in range(splits)]
    imp = [(2 * z, j) for z, j in enumerate(first)] + [(2 * z - 1, j - 1) for z, j in enumerate(first) if z > 0]
    return sorted(imp) + [(2 * splits - 1, 32 * (lo // 32) - 1), (2 * splits - 1, lo - 1)]


@pytest.mark.parametrize("arith", ARITHS, indirect=True)
def test_impulses_at_every_split_boundary(device, launches, arith):
    """(e): dy = 0 but for dy[j][k] = 1 at the first voxel of each of the 32 splits and the voxel before it (channels 0 .. 62, one impulse each) and, in
    channel 63, at the last voxel of the last full K step and at voxel L - 1 (65 voxels for 64 channels).  dW[k] is then x at the tap positions of
    channel k's voxels: within the bar where a tap is inside the grid, EXACTLY 0.0 where it falls in the padding; a channel without an impulse is
    exactly 0.0 (none is left in this shape).  A split that loses or repeats a K step shows in the channels of its boundary."""
    from nerfdet_amd import conv_train
    name = "ladder-32"
    dims, cin, cout, kernel, stride, pads = CASES[name][:6]
    splits, keep = _expect_plan(name, arith)
    k3, s3, p3, out_dims = geometry(dims, kernel, stride, pads)
    lo = math.prod(out_dims)
    imp = impulse_voxels(lo, splits)
    assert len(imp) == 65 and len({j for _, j in imp}) == 65 and {k for k, _ in imp} == set(range(64)) and max(j for _, j in imp) == lo - 1
    x = _case(name)[0]
    dy = torch.zeros(lo, cout, device=device)
    for k, j in imp:
        dy[j, k] = 1.0
    dy = dy.view(*out_dims, cout)
    _poison(device, math.prod(kernel), cin, cout, splits)
    got = conv_train.weight_grad(x, dy, kernel, stride, pads, implicit=True).reshape(cout, cin, -1)
    assert launches["split"] == [(splits, keep)]
    ref = _dw_statement(x, dy, k3, s3, p3, torch.float64)        # one or two terms an element: exact
    pad = ref == 0
    assert bool(pad.any()) and not bool(pad.all())
    err = (got.double() - ref).abs()
    scale = float(ref.abs().max())
    worst = err.amax(dim=(1, 2))
    print(f"{name} {arith} impulses: kernel {float(worst.max()) / scale:.2e}  bar {BAR:.2e}")
    ksteps = (lo + 31) // 32
    split_of = lambda j: max(z for z in range(splits) if ksteps * z // splits <= j // 32)      # noqa: E731
    bad = [(k, [(j, split_of(j)) for kk, j in imp if kk == k], f"{float(worst[k]) / scale:.2e}") for k in range(cout) if not float(worst[k]) <= BAR * scale]
    assert not bad, f"(channel, [(voxel, its split)], error) off the bar: {bad}"
    leaked = sorted({int(k) for k in torch.nonzero(pad & (got != 0))[:, 0]})
    assert not leaked, f"channels with a value where every tap is padding or no impulse sits: {leaked}"
    for k in set(range(cout)) - {k for k, _ in imp}:
        assert not bool((got[k] != 0).any()), k


@pytest.mark.parametrize("name,arith", _params(["ladder-16", "tile-128x256", "tile-128x256-2col"], skip=[("tile-128x256-2col", "bf16x3")]), indirect=["arith"])
def test_workgroup_remap_changes_the_order_only(device, launches, name, arith):
    """(f): wgrad_xcd = 1 (the tiles of a K split on one XCD) against 0 (grid order): "same sums, same partial layout" -- the same bits.
    Two column tiles (gridDim.y = 2): 256 -> 512 on fp16 pairs, 256 -> 256 on bf16x3 (128 x 128 tiles)."""
    splits, keep = _expect_plan(name, arith)
    assert splits >= 8 and splits % 8 == 0          # else the library leaves the remap off whatever the knob says
    with _knobs(wgrad_xcd=1):
        on = _run(name, arith, launches)
    with _knobs(wgrad_xcd=0):
        off = _run(name, arith, launches)
    assert launches["split"] == [(splits, keep)]
    assert torch.equal(on, off)
    _, _, ref, e32 = _case(name)
    _check(name + "/xcd=0", arith, off, ref, e32)


@pytest.mark.parametrize("name", ["tile-128x256", "tile-128x256-2col"])
def test_wide_tile_changes_the_tiling_only(device, launches, name):
    """(f): the 128 x 256 tile against the 128 x 128 tile (wgrad_wide = 0) at the same splits: each element is the same sum in the same order."""
    import nerfdet_amd.conv3d as C
    assert C.train_arithmetic() == "f16x2"
    _expect_plan(name, "f16x2", wide=False)
    with _knobs(wgrad_wide=1):
        wide = _run(name, "f16x2", launches)
    with _knobs(wgrad_wide=0):
        narrow = _run(name, "f16x2", launches)
    assert torch.equal(wide, narrow)


@pytest.mark.parametrize("splits", [1, 2, 8, 9, 10, 17, 32])
def test_partial_sums_are_added_in_index_order(device, splits):
    """(g): ndet_wgrad_to_torch alone on random partials: v = p[0]; v = v + p[s] for s = 1 .. in fp32, moved to torch's layout -- bit for bit (the
    kernel loads eight partials at a time: rounds of 1 + 8 n; ragged Cout; 27 taps take the raised LDS limit)."""
    from nerfdet_amd import conv_train
    torch.manual_seed(splits)
    for taps, cout, cin in itertools.product((1, 8, 9, 27), (25, 64, 96), (32, 64)):
        p = torch.randn(splits, taps * cin, cout, device=device) * torch.exp(torch.randn(splits, 1, 1, device=device))
        got = conv_train._to_torch_layout(p.reshape(-1), taps, cin, cout, (taps,), splits)
        v = p[0]
        for s in range(1, splits):
            v = v + p[s]
        want = v.view(taps, cin, cout).permute(2, 1, 0).contiguous()
        assert got.shape == want.shape and torch.equal(got, want), (splits, taps, cout, cin)


def staged_tiling(name):
    """(tile, splits) the tiling tables give the staged form's GEMM of a STAGED case: rows = (tap, input channel), K = the output voxels."""
    from nerfdet_amd import conv3d as C, conv_tiles
    dims, cin, cout, kernel, stride, pads = STAGED[name][:6]
    lo = math.prod(geometry(dims, kernel, stride, pads)[3])
    m, k_iters = math.prod(kernel) * cin, (lo + 31) // 32
    tile, splits = C.choose_tiling_split(m, cout, k_iters)
    return conv_tiles.resolve(tile, splits, m=m, cout=cout, cin=k_iters * 32, taps=1, transposed=False, halo_ok=False)


@pytest.mark.parametrize("name,arith", _params(list(STAGED)), indirect=["arith"])
def test_staged_weight_gradient_at_long_k(device, launches, name, arith):
    """(h): the staged form (``implicit=False``: the 1x1 layers' route) over 6 498 and 16 900 voxels and on the unpadded 2x2x2 stride-2 shape.  The
    tiling tables split these GEMMs 8, 22 and 2 ways; on fp16 pairs the partials must reach ndet_wgrad_to_torch unreduced (the keep path)."""
    from nerfdet_amd import conv_train
    dims, cin, cout, kernel, stride, pads, want_splits = STAGED[name]
    assert staged_tiling(name)[1] == want_splits and want_splits > 1
    x, dy, ref, e32 = _case(name)
    _poison(device, math.prod(kernel), cin, cout, want_splits)
    got = conv_train.weight_grad(x, dy, kernel, stride, pads, implicit=False)
    assert launches["split"] == [] and launches["layout"] == [want_splits if arith == "f16x2" else 1], launches
    assert got.shape == (cout, cin) + tuple(kernel)
    _check(name, arith, got.reshape(cout, cin, -1), ref, e32)
