"""What tests/test_dgrad_shapes_gpu.py stands on, checked without a GPU: its reference (tests/dgrad_ref.py) against fp64 CPU autograd at every
shape it runs, the premise of its exact ladder, the (tile, splits) pairs the training step's data-gradient launches are dispatched to (its PRODUCTION
list must equal what the walk over the cfg3 workload finds), and the two host rules its rows rely on: a pinned training pack stays on fp16 pairs below
F16_MIN_KSTEPS K steps, and an unsplit unified adjoint launch runs the direct-epilogue partner."""
import inspect
import math

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import dgrad_ref as R
import test_dgrad_shapes_gpu as G
from nerfdet_amd import conv3d as C, conv_tiles, conv_train

VIEWS, IMAGE = 40, (240, 320)       # the cfg3 training workload (tools/bench_train.py: 50 sampled views, 10 of them NeRF targets, 240 x 320)


# ---- the reference against autograd ----
def _autograd_dx(dy, w, stride, dims_in, transposed=False):
    """fp64 CPU autograd of F.conv2d / F.conv3d / F.conv_transpose3d: d (y . dy) / dx, channels-last."""
    wd = w.double()
    if transposed:
        x = torch.zeros(1, w.shape[0], *dims_in, dtype=torch.float64, requires_grad=True)
        y = F.conv_transpose3d(x, wd, stride=2)
        (y * dy.double().permute(3, 0, 1, 2).unsqueeze(0)).sum().backward()
        return x.grad[0].permute(1, 2, 3, 0)
    pad = tuple(int(v) // 2 for v in w.shape[2:])
    if w.dim() == 4:
        x = torch.zeros(dims_in[0], w.shape[1], *dims_in[1:], dtype=torch.float64, requires_grad=True)
        y = F.conv2d(x, wd, stride=stride, padding=pad)
        (y * dy.double().permute(0, 3, 1, 2)).sum().backward()
        return x.grad.permute(0, 2, 3, 1)
    x = torch.zeros(1, w.shape[1], *dims_in, dtype=torch.float64, requires_grad=True)
    y = F.conv3d(x, wd, stride=stride, padding=pad)
    (y * dy.double().permute(3, 0, 1, 2).unsqueeze(0)).sum().backward()
    return x.grad[0].permute(1, 2, 3, 0)


CONV_SHAPES = sorted(G.conv_shapes())         # (layer Cin, layer Cout, kernel, stride, input grid) of every convolution case of the GPU file
T2_SHAPES = sorted(G.t2_shapes())             # (ConvTranspose3d Cin, Cout, input grid)


@pytest.mark.parametrize("cin,cout,kernel,stride,grid", CONV_SHAPES, ids=[f"{a}to{b}-k{'x'.join(map(str, k))}-s{s}-{'x'.join(map(str, g))}" for a, b, k, s, g in CONV_SHAPES])
def test_dx_conv_is_autograd_of_the_convolution(cin, cout, kernel, stride, grid):
    dy = R.gradient_like(R.out_grid(grid, kernel, stride), cout, seed=cin + cout)
    w = R.kaiming(cout, cin, kernel, seed=cin)
    ref = _autograd_dx(dy, w, stride, grid)
    got = R.dx_conv(dy, w, stride, grid, torch.float64)
    assert got.dtype == torch.float64 and tuple(got.shape) == tuple(grid) + (cin,)
    assert R.rel_max(got, ref) <= 1e-12
    # the fp32 evaluation (the e32 figure of the bars) is the same statement: fp32-close, and not the fp64 tensor under another name
    e32 = R.rel_max(R.dx_conv(dy, w, stride, grid, torch.float32), ref)
    assert 0.0 < e32 < 1e-5, e32


@pytest.mark.parametrize("cin,cout,grid", T2_SHAPES)
def test_dx_convT2_is_autograd_of_the_transposed_convolution(cin, cout, grid):
    dy = R.gradient_like(tuple(2 * v for v in grid), cout, seed=cin + cout)
    w = R.kaiming(cout, cin, (2, 2, 2), seed=cin, transposed=True)
    ref = _autograd_dx(dy, w, 2, grid, transposed=True)
    got = R.dx_convT2(dy, w, torch.float64)
    assert tuple(got.shape) == tuple(grid) + (cin,) and R.rel_max(got, ref) <= 1e-12


@pytest.mark.parametrize("relu,with_res", [(True, True), (True, False), (False, True)])
def test_affine_act_bwd_is_autograd_of_the_fused_epilogue(relu, with_res):
    """y = relu(conv(x) scale + shift + res): d/d conv = dy [y > 0] scale, d/d res = dy [y > 0]."""
    g = torch.Generator().manual_seed(3)
    conv = torch.randn(2, 5, 7, 12, generator=g, dtype=torch.float64).requires_grad_(True)
    res = torch.randn(2, 5, 7, 12, generator=g, dtype=torch.float64).requires_grad_(True) if with_res else None
    scale = (torch.rand(12, generator=g, dtype=torch.float64) + 0.5) * (1 - 2 * (torch.arange(12) % 3 == 0).double())      # both signs
    shift = torch.randn(12, generator=g, dtype=torch.float64)
    y = conv * scale + shift
    if with_res:
        y = y + res
    y = torch.relu(y) if relu else y
    dy = torch.randn(2, 5, 7, 12, generator=g, dtype=torch.float64)
    (y * dy).sum().backward()
    gs, d_id = R.affine_act_bwd(dy.float(), y.detach().float(), scale.float(), relu, torch.float64)
    assert bool((y.detach() > 0).any()) and (not relu or bool((y.detach() == 0).any()))
    assert torch.allclose(gs, dy.float().double() * (y.detach() > 0 if relu else 1.0) * scale.float().double(), rtol=0, atol=0)
    assert R.rel_max(gs, conv.grad) <= 1e-7 and (not with_res or R.rel_max(d_id, res.grad) <= 1e-7)        # (dy and scale went through fp32 once)


def test_dx_conv_generalises_the_weight_gradient_files_statement():
    """tests/test_wgrad_shapes_gpu.py states the stride-1 3D data gradient as gathers from padded dy; dx_conv scatters tap by tap: the same sums."""
    import test_wgrad_shapes_gpu as W
    dy, w = R.gradient_like((5, 4, 6), 40, seed=1), R.kaiming(40, 32, (3, 3, 3), seed=2)
    assert R.rel_max(R.dx_conv(dy, w, 1, (5, 4, 6)), W._dx_statement(dy, w, torch.float64)) <= 1e-12


# ---- the premise of the exact ladder ----
INTEGER_CASES = ([(n, cin, cout, k, g, False) for n, (cin, cout, k, g) in {**R.LADDER, **R.LADDER_1X1}.items()]
                 + [(n, cin, cout, (2, 2, 2), tuple(2 * v for v in g), True) for n, (cin, cout, g) in R.LADDER_T2.items()])


@pytest.mark.parametrize("name,cin,cout,kernel,grid,transposed", INTEGER_CASES, ids=[c[0] for c in INTEGER_CASES])
def test_the_integer_cases_are_exact_in_fp32_and_in_both_operand_schemes(name, cin, cout, kernel, grid, transposed):
    dy, w = G.integer_data(name)
    taps = math.prod(kernel)
    assert taps * R.padded(cout) * 3 * 2 == R.integer_bound(cout, kernel) < R.EXACT_BELOW == 2 ** 24
    assert float(dy.abs().max()) == 3.0 and float(w.abs().max()) == 2.0 and torch.equal(dy, dy.round()) and torch.equal(w, w.round())
    assert tuple(dy.shape) == tuple(grid) + (cout,) and tuple(w.shape[:2]) == ((cin, cout) if transposed else (cout, cin))
    ref = R.dx_convT2(dy, w) if transposed else R.dx_conv(dy, w, 1, grid)
    ref32 = R.dx_convT2(dy, w, torch.float32) if transposed else R.dx_conv(dy, w, 1, grid, torch.float32)
    assert float(ref.abs().max()) <= R.integer_bound(cout, kernel) and torch.equal(ref, ref.round())
    assert torch.equal(ref32.double(), ref) and float(ref.abs().max()) > 0
    # the fp16-pair scheme: operand times a power of two, rounded to fp16, nothing left for the low half; the bf16 planes: the leading one holds it
    for t in (dy, w):
        s = C.f16_weight_scale(float(t.abs().max()))
        assert s == 2.0 ** 13 and torch.equal((t * s).half().float(), t * s)
        assert torch.equal(t.bfloat16().float(), t)


def test_grid_weights_and_impulses_are_exact_operands():
    w = R.grid_weights(25, 64, (3, 3, 3), seed=5)
    assert float(w.abs().max()) == 1.0 and torch.equal(w * 1024, (w * 1024).round()) and w.unique().numel() > 1000
    s = C.f16_weight_scale(1.0)
    assert torch.equal((w * s).half().float(), w * s), "exact as the high half of the fp16 pair"
    p0 = w.bfloat16().float()
    p1 = (w - p0).bfloat16().float()
    p2 = (w - p0 - p1).bfloat16().float()
    assert torch.equal(p0 + p1 + p2, w), "exact as three bf16 terms"
    for name in G.IMPULSE_CASES:
        cin, cout, kernel, stride, grid = G.IMPULSE_CASES[name]
        og = R.out_grid(grid, kernel, stride)
        pts = G.impulse_points(og, two_d=len(kernel) == 2)
        assert len(pts) == 9 and len(set(pts)) == 9 and cout == 25
        for pt in pts:
            dy = torch.zeros(*og, cout)
            dy[pt + (24,)] = 1.0
            want = G.impulse_slab(R.grid_weights(cout, cin, kernel, seed=5), pt, stride, grid)
            assert torch.equal(R.dx_conv(dy, R.grid_weights(cout, cin, kernel, seed=5), stride, grid), want.double()), (name, pt)
            assert int((want != 0).any(dim=-1).sum()) <= math.prod(kernel)


# ---- dispatch: where the training step's data-gradient launches go ----
def _static_eligible(conv):
    """conv_train.eligible without the tensor: the convolutions the training step runs on the MFMA kernels."""
    k = conv.kernel_size
    return (isinstance(conv, (nn.Conv2d, nn.Conv3d)) and len(set(conv.stride)) == 1 and conv.stride[0] in (1, 2) and all(d == 1 for d in conv.dilation)
            and conv.groups == 1 and all(v % 2 == 1 and p == v // 2 for v, p in zip(k, conv.padding)) and conv.in_channels % 32 == 0
            and (isinstance(conv, nn.Conv2d) or len(set(k)) == 1))


def _input_shapes(run, root):
    """[(name, convolution, input shape)] of the convolutions under ``root`` whose INPUT needs a gradient when ``run()`` evaluates the model on meta
    tensors (shapes and the autograd graph only: nothing is computed)."""
    seen, hooks = [], []
    names = {m: n for n, m in root.named_modules()}
    for m in root.modules():
        if isinstance(m, (nn.Conv2d, nn.Conv3d, nn.ConvTranspose3d)):
            hooks.append(m.register_forward_pre_hook(lambda mod, args: seen.append((names[mod], mod, tuple(args[0].shape))) if args[0].requires_grad else None))
    try:
        run()
    finally:
        for h in hooks:
            h.remove()
    return seen


def training_dgrad_launches():
    """[(layer, mode, m, adjoint Cout, K steps, tile, splits)] of every data-gradient launch of one cfg3 training step on the split-family kernels,
    as conv3d._conv_split dispatches it under ARITHMETIC = "f16x2": the modules of presets.nerfdet_cfg(50) on VIEWS images of IMAGE and the
    config's voxel grid.  mode "s1": the stride-1 adjoint convolution; "det": the stride-2 detour of the deterministic mode (_dgrad_strided: the
    stride-1 adjoint over the INPUT grid); "t2": the ConvT2 up-blocks' dx (the k2 s2 unpadded convolution of dy)."""
    from nerfdet_amd.backbone import FPN, ResNet
    from nerfdet_amd.head import ScanNetImVoxelHeadV2
    from nerfdet_amd.neck3d import FastIndoorImVoxelNeck
    from nerfdet_amd.presets import nerfdet_cfg
    cfg = nerfdet_cfg(50)["model"]
    args = lambda d: {k: v for k, v in d.items() if k != "type"}      # noqa: E731
    with torch.device("meta"):
        backbone, fpn = ResNet(**args(cfg["backbone"])).train(), FPN(**args(cfg["neck"])).train()
        neck, head = FastIndoorImVoxelNeck(**args(cfg["neck_3d"])).train(), ScanNetImVoxelHeadV2(**args(cfg["bbox_head"])).train()
        images = torch.empty(VIEWS, 3, *IMAGE)
        volume = torch.empty(1, cfg["neck_3d"]["in_channels"], *cfg["n_voxels"]).requires_grad_(True)
    fpn.active_outs = (0,)                          # detector.py: level 0 is the one it keeps
    both = nn.ModuleList([backbone, fpn])
    levels = []
    found = _input_shapes(lambda: fpn(backbone(images)), both) + _input_shapes(lambda: levels.extend(neck(volume)), neck)
    assert backbone.frozen_stages == 1 and not any(n.startswith("0.layer1") or n == "0.conv1" for n, _, _ in found)
    assert len(levels) == 3 and [tuple(v.shape[2:]) for v in levels] == [tuple(n // 2 ** i for n in cfg["n_voxels"]) for i in range(3)]
    shared = [head.centerness_conv, head.reg_conv, head.cls_conv]
    head_cout = sum(c.out_channels for c in shared)
    assert head_cout == sum(R.HEAD_SPLIT) and all(_static_eligible(c) and c.stride[0] == 1 for c in shared)
    rows = []
    prev = C.set_arithmetic("f16x2")
    try:
        def add(layer, mode, m, cout, cin, taps, halo_ok):
            k_iters = taps * (cin // 32)
            tile, splits = C.choose_tiling_split(m, cout, k_iters, 0, 0, False, halo_ok)
            tile, splits = conv_tiles.resolve(tile, splits, m=m, cout=cout, cin=cin, taps=taps, transposed=False, halo_ok=halo_ok,
                                              direct_epilogue=C.DIRECT_EPILOGUE)
            rows.append((layer, mode, m, cout, k_iters, tile, splits))
        for name, conv, shape in found:
            if isinstance(conv, nn.ConvTranspose3d):
                assert tuple(conv.kernel_size) == (2, 2, 2) and tuple(conv.stride) == (2, 2, 2) and conv.out_channels % 32 == 0
                add(name, "t2", math.prod(shape[2:]), conv.in_channels, conv.out_channels, 8, False)
                continue
            assert _static_eligible(conv), name
            taps = math.prod(conv.kernel_size)
            m = math.prod(shape[2:]) * (shape[0] if isinstance(conv, nn.Conv2d) else 1)      # the adjoint runs over the layer's INPUT grid
            add(name, "s1" if conv.stride[0] == 1 else "det", m, conv.in_channels, R.padded(conv.out_channels), taps, taps > 1)
        for i, v in enumerate(levels):
            add(f"head.level{i}", "s1", math.prod(v.shape[2:]), v.shape[1], R.padded(head_cout), 27, True)
    finally:
        C.set_arithmetic(prev)
    return rows


def test_the_walk_sees_the_training_steps_layers():
    rows = training_dgrad_launches()
    layers = {r[0] for r in rows}
    # ResNet-50 stages 2 - 4 (13 blocks x 3 convolutions + 3 downsamples, less the two layers that read the frozen prefix), the FPN's kept output
    # convolution and its laterals but the first (it reads the frozen stage 1), the 3D neck (3 x 2 block convolutions, 2 downsamples, 2 transposed +
    # 2 plain up-block convolutions, 3 output blocks) and the head's shared convolution at three levels
    assert len(rows) == (13 * 3 + 3 - 2) + 4 + (6 + 2 + 4 + 3) + 3, len(rows)
    assert "0.layer2.0.conv1" not in layers and "0.layer2.0.downsample.0" not in layers and "0.layer2.0.conv2" in layers
    assert "1.lateral_convs.0.conv" not in layers and "1.fpn_convs.0.conv" in layers and "1.fpn_convs.1.conv" not in layers
    # stride 2: conv2 of the first block of stages 2 - 4 and the downsamples of stages 3 and 4; conv1 and the downsample of the neck's two coarser levels
    assert sum(r[1] == "t2" for r in rows) == 2 and sum(r[1] == "det" for r in rows) == 5 + 4
    assert all(cout % 32 == 0 for _, _, _, cout, _, _, _ in rows), "the adjoint's Cout is the layer's Cin: always a multiple of 32"
    head = [r for r in rows if r[0].startswith("head.")]
    assert [(m, cout, k) for _, _, m, cout, k, _, _ in head] == [(25600, 128, 27), (3200, 128, 27), (400, 128, 27)]      # 25 channels: ONE chunk of 32


def test_production_is_what_the_training_step_dispatches():
    pairs = {(tile, splits) for *_, tile, splits in training_dgrad_launches()}
    assert pairs, "the walk found launches"
    assert set(G.PRODUCTION) == pairs and len(G.PRODUCTION) == len(set(G.PRODUCTION)), \
        f"PRODUCTION of tests/test_dgrad_shapes_gpu.py misses {sorted(pairs - set(G.PRODUCTION))}, names without a launch {sorted(set(G.PRODUCTION) - pairs)}"
    # every pair has its real-valued row, every family one at splits 1, and each row cuts its K walk unevenly where it splits
    assert set(G.PRODUCTION) <= set(G.REAL_ROWS)
    for family in ("unified", "ws", "wsp", "halo"):
        assert any(conv_tiles.TILES[t].family == family and s == 1 for t, s in G.REAL_ROWS), family
    for tile, splits in G.REAL_ROWS:
        cin, cout, kernel, grid = G.real_shape(tile, splits)
        units = G.real_units(tile, splits)
        assert units >= splits and (splits == 1 or units % splits), (tile, splits, units)
        m = math.prod(grid)
        assert m % 64 and cin % 32 == 0 and 2 * m * cin * R.padded(cout) * math.prod(kernel) <= 0.6e9
        got = conv_tiles.resolve(tile, splits, m=m, cout=cin, cin=R.padded(cout), taps=math.prod(kernel), transposed=False, halo_ok=math.prod(kernel) > 1,
                                 direct_epilogue=conv_tiles.is_direct(tile))          # (as the row launches: a staged id with the direct epilogue off)
        assert got == (tile, splits), (tile, splits, got)


def test_the_autograd_cases_run_where_the_walk_rule_sends_them():
    """G.predicted is the rule of the walk above (choose_tiling_split then resolve under f16x2); the GPU file holds each autograd case's launch to it."""
    for name, (module, cin, cout, kernel, stride, grid) in R.AUTOGRAD.items():
        key = G.autograd_key(name)
        tile, splits = G.predicted(*key)
        assert tile in conv_tiles.TILES and 1 <= splits <= R.MAX_SPLITS, (name, tile, splits)
        if module != "ConvT2":
            assert key[1] == cin and key[2] == R.padded(cout)


# ---- the two rules the GPU rows rely on ----
def _launch_arithmetic(mode, pinned, k_iters):
    """The arithmetic of one split-family launch, restated from conv3d._conv_split: the layer rule, overridden by a pinned pack in the f16x2 mode."""
    arith = "bf16x3" if (mode == "f16x2" and k_iters < C.F16_MIN_KSTEPS) else mode
    if mode == "f16x2" and pinned:
        arith = pinned
    return arith


def test_a_pinned_training_pack_keeps_fp16_pairs_below_the_step_floor():
    src = inspect.getsource(C._conv_split)
    assert "arith = layer_arithmetic(k_iters)" in src and 'if ARITHMETIC == "f16x2" and pk.arith:' in src and "arith = pk.arith" in src, \
        "conv3d._conv_split no longer states the rule _launch_arithmetic restates"
    prev = C.set_arithmetic("f16x2")
    try:
        for k in range(1, 8):
            assert C.layer_arithmetic(k) == _launch_arithmetic("f16x2", None, k) == ("bf16x3" if k < C.F16_MIN_KSTEPS else "f16x2")
            assert _launch_arithmetic("f16x2", "f16x2", k) == "f16x2"
    finally:
        C.set_arithmetic(prev)
    assert C.F16_MIN_KSTEPS == 4 and [R.adjoint_ksteps(c, k) for _, c, k, _ in R.LADDER_1X1.values()] == [1, 2, 3]
    # the pack conv_train builds for a data gradient in the fp16-pair arithmetic IS pinned, keeps its output's maximum and reads its scale on the device
    w, planes, slot = torch.zeros(25, 64, 3, 3, 3), torch.zeros(1, dtype=torch.int16), torch.zeros(C._AmaxSlots.WIDTH)
    pk = conv_train._plane_pack(w, planes, slot, "f16x2", (3, 3, 3), True)
    assert (pk.arith, pk.keep_amax, pk.w_amax is slot, pk.cout, pk.cin, pk.strides, pk.pads) == ("f16x2", True, True, 64, 32, (1, 1, 1), (1, 1, 1))
    pk = conv_train._plane_pack(w, planes, None, "bf16x3", (3, 3, 3), True)
    assert (pk.arith, pk.keep_amax, pk.w_amax) == ("bf16x3", False, None)


def test_an_unsplit_unified_adjoint_launch_resolves_to_the_direct_partner():
    for tile in conv_tiles.ids("unified"):
        partner = conv_tiles.TILES[tile].partner
        assert conv_tiles.is_direct(partner) and conv_tiles.TILES[partner].partner == tile
        for cin, cout, kernel, grid in {**R.LADDER, **R.LADDER_1X1}.values():
            kw = dict(m=math.prod(grid), cout=cin, cin=R.padded(cout), taps=math.prod(kernel), transposed=False, halo_ok=math.prod(kernel) > 1)
            assert cin % 32 == 0
            assert conv_tiles.resolve(tile, 1, **kw) == (partner, 1) == conv_tiles.resolve(partner, 1, **kw)
            assert conv_tiles.resolve(tile, 1, direct_epilogue=False, **kw) == (tile, 1)
            assert conv_tiles.resolve(tile, 2, **kw) == (tile, 2) == conv_tiles.resolve(partner, 2, **kw)
    # ... and so does every unsplit unified launch of the training step
    for layer, mode, m, cout, k_iters, tile, splits in training_dgrad_launches():
        if conv_tiles.TILES[tile].family == "unified" and splits == 1:
            assert conv_tiles.is_direct(tile), (layer, tile)


def test_resolve_leaves_every_ladder_launch_alone():
    for name, (cin, cout, kernel, grid) in R.LADDER.items():
        for tile in G.LADDER_TILES:
            halo = conv_tiles.TILES[tile].family == "halo"
            for splits in R.ladder_splits(cout, kernel, halo):
                got = conv_tiles.resolve(tile, splits, m=math.prod(grid), cout=cin, cin=R.padded(cout), taps=math.prod(kernel), transposed=False,
                                         halo_ok=True, direct_epilogue=False)
                assert got == (tile, splits), (name, tile, splits, got)
    assert G.LADDER_TILES == conv_tiles.ids("unified", "ws", "wsp", "halo")
    assert [R.ladder_splits(c, k, False) for _, c, k, _ in R.LADDER_1X1.values()] == [[1], [1, 2], [1, 2, 3]]
    assert R.ladder_splits(25, (3, 3, 3), True) == [1] and R.ladder_splits(96, (3, 3, 3), True) == [1, 2, 3] and R.ladder_splits(96, (3, 3, 3), False) == [1, 2, 3, 32]
