"""NaN and +-Inf planted in activations, residuals, features and raw sigma ahead of every kernel that takes a maximum -- the convolution epilogues'
ReLU, the fused blocks, the max-pools, BatchNorm's ReLU / backward mask / variance, the density MLP, the compositor's depth clamp and the variance
clamps of the statistics kernels -- against float64 PyTorch-CPU of the same modules.  The contract, the cases and ``check`` are
tests/nonfinite_ref.py's (DESIGN.md "Non-finite values"); tests/test_nonfinite_cpu.py shows that PyTorch-CPU fp32 meets it on the same cases.
Shapes are existing edge rows of the kernels' home test files.  Nothing is planted in points, poses, intrinsics or anything an address is
computed from.

fp16 pairs with an Inf planted (contract 4): the launch runs under conv3d.guard_begin; either the result meets the contract, or the guard word is
set -- and the same call on bf16x3, asserted unconditionally, meets it.  Every test prints what the guard did (``pytest -s``)."""
import copy

import pytest
import torch

import nonfinite_ref as Nf
from test_f16x2_edges_gpu import ELEM_BAR, RMS_BAR

pytestmark = pytest.mark.gpu

CONV_BARS = {"elem": ELEM_BAR, "rms": RMS_BAR}
BF16_BARS = {"rel": 2e-5}          # tests/test_f16x2_edges_gpu.py::test_bf16_edge_row, against the bf16-rounded operands' convolution


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _slot_holds(got, tag):
    """Contract 5: the slot a launch leaves is max |out| over the elements that are not NaN (Inf if an Inf is among them), never a NaN."""
    from nerfdet_amd import conv3d as C
    vals = got[~torch.isnan(got)]
    want = float(vals.abs().max()) if vals.numel() else 0.0
    slot = C.amax_value(got._ndet_amax)
    assert slot == want, f"{tag}: the slot holds {slot}, max |out| over the elements that are not NaN is {want}"


def _slot_if_any(got, tag):
    """bf16x3, bf16 and f32 launches leave no slot under their own arithmetic (tests/test_conv_batch_gpu.py asserts that); one that does holds."""
    if hasattr(got, "_ndet_amax"):
        _slot_holds(got, tag)


def _guarded(device, run, refs, bars, kind, tag, slot=True):
    """One fp16-pair launch under the range guard -> (out, "met" or "tripped").  Planted NaN: contracts 1-3 outright (fmaxf keeps a NaN out of the
    scale).  Planted Inf: 1-3, or the guard word is set (contract 4): missing the contract with the word clear fails."""
    from nerfdet_amd import conv3d as C
    C.guard_begin(device)
    got = run()
    tripped = C.guard_tripped(device)
    if slot is True or (slot == "if any" and hasattr(got, "_ndet_amax")):
        _slot_holds(got, tag)
    if kind == "nan":
        _check_all(got, refs, bars, kind, tag)
        return got, "tripped" if tripped else "met"
    try:
        _check_all(got, refs, bars, kind, tag)
    except AssertionError as e:
        assert tripped, f"{tag}: missed the contract with the guard word clear: {e}"
        return got, "tripped"
    return got, "met (word set)" if tripped else "met"


def _check_all(got, refs, bars, kind, tag):
    if isinstance(refs, dict):
        return {name: Nf.check(got[name], refs[name], bars[name], kind, f"{tag} {name}") for name in refs}
    return Nf.check(got, refs, bars, kind, tag)


# ------------------------------------------------------------------------------------------------------------------------------------------
# A. convolution epilogues
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", Nf.KINDS)
@pytest.mark.parametrize("row", Nf.CONV_ROWS, ids=Nf.conv_row_id)
def test_conv_epilogue_row(device, row, kind):
    """One row per tile family in its home row's ReLU mode (staged and direct epilogue, scalar columns, transposed, split-K reduce, upsampled
    residual), and nonfinite_ref.RELU_ROWS: the same shapes with the ReLU after (1) and before (2) a residual on every epilogue code path -- scalar
    columns unsplit and in the non-vector reduce, staged + direct, wave-specialised / persistent unsplit, halo unsplit.  On bf16x3 and fp16 pairs."""
    from nerfdet_amd import conv_tiles
    from test_f16x2_edges_gpu import _direct_ok, _launch
    tile, dim, cin, cout, grid, k, stride, mode, relu, res, splits, bias = row
    case = Nf.conv_case(dim, cin, cout, grid, k, stride, mode, relu, res, bias)
    v, refs, tag = case.variant(kind), case.refs(kind), f"{Nf.conv_row_id(row)} {kind}"
    forms = [(tile, splits, False)] + ([(conv_tiles.TILES[tile].partner, 1, True)] if _direct_ok(tile, v, cout, splits) else [])
    said = []
    for t, sp, direct in forms:
        got3, names, _ = _launch(device, v, "bf16x3", t, sp, direct=direct)
        assert names == [conv_tiles.TILES[t].name], names
        Nf.check(got3, refs, CONV_BARS, kind, tag + " bf16x3" + (" direct" if direct else ""))
        _slot_if_any(got3, tag + " bf16x3")
        got, word = _guarded(device, lambda: _launch(device, v, "f16x2", t, sp, direct=direct)[0], refs, CONV_BARS, kind,
                             tag + " f16x2" + (" direct" if direct else ""))
        said.append(word)
        if direct:
            assert _bits_equal(got, staged), "direct and staged epilogue differ"
        staged = got
    print(f"NONFINITE conv {tag}: {Nf.outside_fraction(refs):.2f} outside the field; fp16-pair guard: {', '.join(said)}")


@pytest.mark.parametrize("kind", Nf.KINDS)
@pytest.mark.parametrize("row", Nf.BF16_CONV_ROWS, ids=Nf.conv_row_id)
def test_conv_epilogue_row_bf16(device, row, kind):
    """The one-product bf16 arithmetic on one row per family, against the convolution of the bf16-rounded operands."""
    from test_f16x2_edges_gpu import _launch
    tile, dim, cin, cout, grid, k, stride, mode, relu, res, splits, bias = row
    case = Nf.conv_case(dim, cin, cout, grid, k, stride, mode, relu, res, bias)
    got, _, _ = _launch(device, case.variant(kind), "bf16", tile, splits, direct=False)
    Nf.check(got, case.refs(kind, bf16_operands=True), BF16_BARS, kind, f"{Nf.conv_row_id(row)} {kind} bf16")
    _slot_if_any(got, f"{Nf.conv_row_id(row)} {kind} bf16")


@pytest.mark.parametrize("kind", Nf.KINDS)
@pytest.mark.parametrize("row", Nf.F32_CONV_ROWS, ids=Nf.conv_row_id)
def test_conv_epilogue_row_f32(device, row, kind):
    """The fp32-MFMA family (csrc/conv3d_kernels.hip) and its split-K reduce."""
    from nerfdet_amd import conv3d as C
    tile, dim, cin, cout, grid, k, stride, mode, relu, res, splits, bias = row
    case = Nf.conv_case(dim, cin, cout, grid, k, stride, mode, relu, res, bias)
    x, pk, r = case.variant(kind).on(device)
    prev = C.set_arithmetic("f32")
    try:
        with torch.no_grad():
            got = C.conv3d_ndhwc(x, pk, residual=r, relu=relu, splits=splits, tile=tile)
        torch.cuda.synchronize()
    finally:
        C.set_arithmetic(prev)
    Nf.check(got, case.refs(kind), CONV_BARS, kind, f"{Nf.conv_row_id(row)} {kind} f32")
    _slot_if_any(got, f"{Nf.conv_row_id(row)} {kind} f32")


@pytest.mark.parametrize("n", [1, 3, 4, 1027, 300001])
def test_amax_pass_drops_a_nan_and_keeps_an_inf(device, n):
    """ndet_amax_f32 (conv3d.amax_of on a tensor no kernel of the library wrote): the slot is max |x| over the elements that are not NaN -- a NaN in
    the bit-pattern atomicMax would collapse the next layer's scale with the guard silent -- and Inf once an Inf of either sign is among them.
    Sizes: one element, the scalar tail alone, one float4, a tail behind float4s, more than one workgroup."""
    from nerfdet_amd import conv3d as C
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=gen) * 3
    spots = sorted({0, n // 2, n - 1})
    for value, want in ((float("nan"), None), (float("inf"), float("inf")), (-float("inf"), float("inf"))):
        for spot in spots:
            y = x.clone()
            y[spot] = value
            if want is None and n > 1:
                y[(spot + 1) % n] = -77.0                      # the largest magnitude sits next to the NaN
            keep = y[~torch.isnan(y)]
            expect = want if want is not None else (float(keep.abs().max()) if keep.numel() else 0.0)
            got = C.amax_value(C.amax_of(y.to(device)))
            assert got == expect, (n, value, spot, got, expect)
    both = x.clone()
    both[0], both[-1] = float("nan"), float("inf")
    if n > 1:
        assert C.amax_value(C.amax_of(both.to(device))) == float("inf")


@pytest.mark.parametrize("kind", Nf.KINDS)
def test_batched_row_keeps_the_second_volume_clean(device, kind):
    """A 64-row tile straddling two volumes of 90 rows, the planted value in the first volume's last slice: the other volumes stay finite and
    within the bars (the field, from the per-volume float64 convolutions, lies in volume 0 alone)."""
    from nerfdet_amd import conv3d as C
    from test_conv_batch_gpu import _run
    tile, n, grid, cin, cout, k, stride, mode, relu, res, splits = Nf.BATCH_ROW
    case = Nf.batch_case()
    refs = case.refs(kind)
    assert not bool(Nf.field(refs)[1:].any())
    x, pk, r = case.variant(kind).on(device)
    launch = lambda arith: _run(device, arith, tile, splits, lambda: C.conv3d_ndhwc(x, pk, residual=r, relu=relu, splits=splits, tile=tile))[0]
    Nf.check(launch("bf16x3"), refs, CONV_BARS, kind, f"batch {kind} bf16x3")
    got, word = _guarded(device, lambda: launch("f16x2"), refs, CONV_BARS, kind, f"batch {kind} f16x2")
    print(f"NONFINITE batch {kind}: fp16-pair guard: {word}")


# ------------------------------------------------------------------------------------------------------------------------------------------
# B. fused blocks
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", Nf.KINDS)
@pytest.mark.parametrize("relu3", Nf.CHAIN_RELU3)
def test_chained_convolutions(device, relu3, kind):
    """conv2d_chain_nhwc, (64, 64, 256, (3, 13, 17)): the ReLU of the intermediate and the last one, after (1) and before (2) the residual, inside
    one launch."""
    from test_fused_blocks_gpu import _run_chain
    case = Nf.chain_case(relu3)
    x, res = case.inputs(kind)
    refs = case.refs(kind)
    Nf.check(_run_chain(device, case.base, "bf16x3", x=x, res=res), refs, CONV_BARS, kind, f"chain {kind} bf16x3")
    _, word = _guarded(device, lambda: _run_chain(device, case.base, "f16x2", x=x, res=res), refs, CONV_BARS, kind, f"chain {kind} f16x2")
    print(f"NONFINITE chain relu{relu3} {kind}: fp16-pair guard: {word}")


@pytest.mark.parametrize("kind", Nf.KINDS)
@pytest.mark.parametrize("ds,nhw", Nf.BLOCK_SHAPES, ids=["identity-1x4x16", "downsample-5x3x5"])
def test_one_launch_bottleneck(device, ds, nhw, kind):
    from test_fused_blocks_gpu import FUSED, _Hooked, _run_block
    case = Nf.block_case(ds, nhw)
    refs, x = case.refs(kind), case.inputs(kind)
    if not hasattr(case, "_dev"):
        case._dev = copy.deepcopy(case.blk).to(device)
    blk = case._dev
    with _Hooked("bf16x3") as names:
        got3 = blk.forward_nhwc(x.to(device))
    assert FUSED not in names
    Nf.check(got3, refs, CONV_BARS, kind, f"bottleneck {kind} bf16x3")

    def fused():
        y, names = _run_block(device, blk, x)
        assert names == [FUSED], names
        return y
    _, word = _guarded(device, fused, refs, CONV_BARS, kind, f"bottleneck {kind} f16x2")
    print(f"NONFINITE bottleneck ds={ds} {nhw} {kind}: fp16-pair guard: {word}")


@pytest.mark.parametrize("kind", Nf.KINDS)
def test_chained_projection_on_the_halo_tile(device, kind):
    """The 256 -> 32 feature mapping in the epilogue of the 3x3 convolution on tile 3256, (3, 13, 21)."""
    import nerfdet_amd.conv3d as C
    from nerfdet_amd.backbone import _chain_pack
    case = Nf.projection_case()
    refs, x = case.refs(kind), case.inputs(kind).to(device)
    if not hasattr(case, "_dev"):
        case._dev = (copy.deepcopy(case.conv).to(device), copy.deepcopy(case.lin).to(device))
    conv, lin = case._dev
    pk = C.packed([conv])
    bars = {"out": CONV_BARS, "mapped": {"rel": 2e-5}}
    prev = C.set_arithmetic("bf16x3")
    try:
        with torch.no_grad():
            out3 = C.conv2d_nhwc(x, pk, amax=False, tile=3256, splits=1)
    finally:
        C.set_arithmetic(prev)
    Nf.check(out3, refs["out"], CONV_BARS, kind, f"projection {kind} bf16x3")
    prev = C.set_arithmetic("f16x2")
    try:
        assert C.projection_ok()

        def run():
            with torch.no_grad():
                out, mapped = C.conv2d_nhwc(x, pk, amax=False, tile=3256, splits=1, chain=_chain_pack(pk, lin))
            assert mapped is not None
            return {"out": out, "mapped": mapped}
        _, word = _guarded(device, run, refs, bars, kind, f"projection {kind} f16x2", slot=False)
    finally:
        C.set_arithmetic(prev)
    print(f"NONFINITE projection {kind}: fp16-pair guard: {word}")


def _stem_layout(x, layout, device):
    """tests/test_stem_gpu.py::_layout's "view": a window of a larger NCHW buffer filled with something that must not be read."""
    xd = x.to(device)
    if layout == "view":
        n, _, h, w = x.shape
        big = torch.full((n, 3, h + 5, w + 9), 1e6, device=device)
        big[:, :, 2:2 + h, 4:4 + w] = xd
        xd = big[:, :, 2:2 + h, 4:4 + w]
    return xd


@pytest.mark.parametrize("kind", Nf.KINDS)
@pytest.mark.parametrize("nhw,layout", Nf.STEM_SHAPES, ids=["2x17x23-view", "2x61x83"])
def test_stem_relu_and_pool(device, nhw, layout, kind):
    """stem_conv_bn_relu_maxpool with three planted image pixels: the ReLU in front of the pool and the pool's running maximum."""
    case = Nf.stem_case(nhw)
    refs = case.refs(kind)
    xd = _stem_layout(case.inputs(kind), layout, device)
    Nf.check(case.stem.run(device, xd, "bf16x3"), refs, CONV_BARS, kind, f"stem {nhw} {kind} bf16x3")
    _, word = _guarded(device, lambda: case.stem.run(device, xd, "f16x2"), refs, CONV_BARS, kind, f"stem {nhw} {kind} f16x2", slot="if any")
    print(f"NONFINITE stem {nhw} {kind}: fp16-pair guard: {word}")


@pytest.mark.parametrize("kind", Nf.KINDS)
def test_bn_relu_maxpool_window(device, kind):
    """bn_relu_maxpool_nhwc: one planted value in a window whose other entries are larger, one in the window hanging over the border."""
    from nerfdet_amd import conv3d as C
    case = Nf.pool_case()
    refs = case.refs(kind)
    bn_d = copy.deepcopy(case.bn).to(device)
    got = C.bn_relu_maxpool_nhwc(case.inputs(kind).to(device), bn_d)
    clean = C.bn_relu_maxpool_nhwc(case.inputs("clean").to(device), bn_d)
    torch.cuda.synchronize()
    Nf.check(got, refs, case.bars(), kind, f"pool {kind}")
    Nf.same_bits_outside(got, clean, refs, f"pool {kind}")


# ------------------------------------------------------------------------------------------------------------------------------------------
# C. BatchNorm rows
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", Nf.KINDS)
@pytest.mark.parametrize("n,c,relu,with_res,where", Nf.bn_cases())
def test_batch_norm_rows(device, n, c, relu, with_res, where, kind):
    """BatchNormRows forward and backward: a planted x poisons exactly its channel in y, dx, dgamma, running_mean AND running_var, as F.batch_norm in
    float64 does; a planted residual gives one y, and threshold_backward lets the gradient through it.  Bars: the home test's max(3e-6, 2 x the
    library's fp32 error on the same tensors), outside the field."""
    from nerfdet_amd.conv_train import BatchNormRows
    case = Nf.bn_case(n, c, relu, with_res, where)
    refs = case.refs(kind)
    lib = case.run(kind, torch.float32, device)
    ours = case.run(kind, torch.float32, device, apply=BatchNormRows.apply)
    worst = {}
    for name, r in refs.items():
        out = ~Nf.field(r)
        scale = max(float(r.ref[out].abs().max()), 1e-12) if bool(out.any()) else 1.0
        err_l = float((lib[name][out] - r.ref[out]).abs().max()) / scale if bool(out.any()) else 0.0
        fig = Nf.check(ours[name], r, {"rel": max(Nf.BN_BAR, 2.0 * err_l)}, kind, f"bn {name} {kind}")
        worst[name] = (fig.get("rel", 0.0), err_l)
    print(f"NONFINITE bn ({n}, {c}) relu={relu} res={with_res} {where} {kind}: " + ", ".join(f"{k} {v[0]:.1e}/{v[1]:.1e}" for k, v in worst.items()))


@pytest.mark.parametrize("kind", Nf.KINDS)
def test_batch_norm_slots(device, kind):
    """Contract 5 on the slots k_bn_apply and k_bn_bwd_apply leave: max over the elements that are not NaN."""
    from nerfdet_amd import _lib, conv3d as C
    case = Nf.bn_case(777, 128, True, True, "x")
    n, c = case.n, case.c
    lib, P = _lib.load(), _lib._ptr
    x, res = case.inputs(kind)
    xd, rd, wd, bd, gd = (t.to(device) for t in (x, res, case.w, case.b, case.gy))
    rm, rv = torch.zeros(c, device=device), torch.ones(c, device=device)
    y, mean, invstd = torch.empty_like(xd), torch.empty(c, device=device), torch.empty(c, device=device)
    ws = torch.empty(int(lib.ndet_bn_workspace_floats(n, c)), dtype=torch.float32, device=device)
    st = _lib._stream(xd)
    y_slot, dx_slot = C.AMAX.take(device), C.AMAX.take(device)
    _lib.check(lib.ndet_bn_train_forward(P(xd), n, c, P(wd), P(bd), P(rm), P(rv), case.MOM, case.EPS, P(rd), 1, P(y), P(mean), P(invstd), P(y_slot), P(ws), st),
               "bn_train_forward")
    dx, dres = torch.empty_like(xd), torch.empty_like(xd)
    dgamma, dbeta = torch.empty(c, device=device), torch.empty(c, device=device)
    _lib.check(lib.ndet_bn_train_backward(P(gd), P(xd), P(y), n, c, P(wd), P(mean), P(invstd), 1, P(dx), P(dres), P(dgamma), P(dbeta), P(dx_slot), P(ws), st),
               "bn_train_backward")
    for t, slot, name in ((y, y_slot, "y"), (dx, dx_slot, "dx")):
        vals = t[~torch.isnan(t)]
        assert C.amax_value(slot) == float(vals.abs().max()), (name, kind)
    assert bool(torch.isnan(y).any()) or kind != "nan"


@pytest.mark.parametrize("rows,c", [(777, 128), (50, 64)])
def test_relu_affine_bwd_opens_the_mask_at_a_nan(device, rows, c):
    """ndet_relu_affine_bwd / _amax with one NaN in y: the gradient passes there, as autograd's threshold_backward has it; the slot is max |g'|."""
    from nerfdet_amd import _lib, conv3d as C
    torch.manual_seed(rows + c)
    lib, P = _lib.load(), _lib._ptr
    g = torch.randn(rows, c) * torch.exp(torch.randn(rows, 1))
    y = torch.relu(torch.randn(rows, c))
    place = (rows // 2, c // 2 + 1)
    y[place] = float("nan")
    scale = (torch.rand(c) + 0.5) * (1 - 2 * (torch.arange(c) % 3 == 0).float())
    want_conv, want_id = Nf.relu_affine_bwd_reference(g, y, scale)
    assert float(want_id[place]) == float(g[place])
    gd, yd, sd = g.to(device), y.to(device), scale.to(device)
    st = _lib._stream(gd)
    out = {}
    for name in ("plain", "amax"):
        d_conv, d_id = torch.full_like(gd, float("nan")), torch.full_like(gd, float("nan"))
        if name == "plain":
            _lib.check(lib.ndet_relu_affine_bwd(P(gd), P(yd), P(sd), rows, c, 1, P(d_id), P(d_conv), st), "relu_affine_bwd")
        else:
            slot = C.AMAX.take(device)
            _lib.check(lib.ndet_relu_affine_bwd_amax(P(gd), P(yd), P(sd), rows, c, 1, P(d_id), P(d_conv), P(slot), st), "relu_affine_bwd_amax")
        assert torch.equal(d_id.cpu().double(), want_id), name
        torch.testing.assert_close(d_conv.cpu().double(), want_conv, rtol=1e-6, atol=0)
        out[name] = d_conv
    assert torch.equal(out["plain"], out["amax"]) and C.amax_value(slot) == float(out["amax"].abs().max())


# ------------------------------------------------------------------------------------------------------------------------------------------
# D. A6: the density MLP
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", Nf.KINDS)
def test_density_mlp_rows(device, kind):
    """ops.point_mlp_alpha (one launch, a scale per row) and the layer-by-layer path (posenc_concat, linear_rows, sigma_head) on n = 130 rows with
    conditioning column 5 of rows 0, 64 and 129 planted: those rows are NaN / non-finite as the reference's, every other row carries the bits of the
    clean run."""
    from nerfdet_amd import ops
    case = Nf.mlp_case()
    refs, bars = case.refs(kind), case.bars()
    if not hasattr(case, "_dev"):
        case._dev = copy.deepcopy(case.mlp).to(device)
    mlp = case._dev
    out = mlp.mlp.sigma_layer.output_layer
    width = (63 + case.glob.shape[1] + 31) // 32 * 32
    assert mlp.fused_ok(width)

    def fused(k):
        pts, glob = case.inputs(k)
        with torch.no_grad():
            alpha, raw, h = ops.point_mlp_alpha(pts.to(device), glob.to(device), mlp._fused_layers(width), out.weight, out.bias, want_raw=True, want_h=True)
        return {"h": h, "raw": raw, "alpha": alpha}

    def layers(k):
        pts, glob = case.inputs(k)
        mlp.FUSED_MLP = False
        try:
            with torch.no_grad():
                return mlp.alpha_from_points(pts.to(device), glob.to(device))
        finally:
            mlp.FUSED_MLP = True
    got, clean = fused(kind), fused("clean")
    for name in refs:
        fig = Nf.check(got[name], refs[name], bars[name], kind, f"point_mlp {name} {kind}")
        Nf.same_bits_outside(got[name], clean[name], refs[name], f"point_mlp {name} {kind}")
    got_l, clean_l = layers(kind), layers("clean")
    Nf.check(got_l, refs["alpha"], bars["alpha"], kind, f"layer-wise alpha {kind}")
    Nf.same_bits_outside(got_l, clean_l, refs["alpha"], f"layer-wise alpha {kind}")


def test_sigma_to_alpha_on_non_finite_sigma(device):
    from nerfdet_amd import ops
    x, want = (torch.tensor(v) for v in Nf.SIGMA_TO_ALPHA)
    got = ops.sigma_to_alpha(x.to(device)).cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and got[1:4].tolist() == [1.0, 0.0, 0.0]
    assert abs(float(got[4]) - float(want[4])) <= 1e-5


def test_sigma_head_passes_a_nan_row(device):
    """k_sigma_head alone: a NaN in one row's trunk output gives that row's alpha NaN and no other."""
    from nerfdet_amd import ops
    gen = torch.Generator().manual_seed(5)
    h, rows = torch.relu(torch.randn(5, 32, generator=gen)), torch.randn(5, 63, generator=gen)
    w, b = torch.randn(1, 95, generator=gen) / 95 ** 0.5, torch.randn(1, generator=gen) * 0.1
    clean = ops.sigma_head(h.to(device), rows.to(device), 63, w.to(device), b.to(device)).cpu()
    h[3, 7] = float("nan")
    got = ops.sigma_head(h.to(device), rows.to(device), 63, w.to(device), b.to(device)).cpu()
    assert torch.isnan(got).tolist() == [False, False, False, True, False] and torch.equal(got[[0, 1, 2, 4]], clean[[0, 1, 2, 4]])


# ------------------------------------------------------------------------------------------------------------------------------------------
# E. the compositor
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", Nf.KINDS)
def test_compositor_ray(device, kind):
    """raw2outputs, R = 5, S = 8, one planted sigma in ray 2: its rgb, depth (torch.clamp keeps a NaN), weights and transmittance from the next sample
    on follow float64 torch; the other rays carry the bits of the clean run."""
    from nerfdet_amd import rays
    case = Nf.composite_case()
    refs, bars = case.refs(kind), case.bars()

    def run(k):
        raw, z, pmask = case.inputs(k)
        with torch.no_grad():
            return rays.raw2outputs(raw.to(device), z.to(device), pmask.to(device), white_bkgd=False)
    got, clean = run(kind), run("clean")
    for name in refs:
        Nf.check(got[name], refs[name], bars[name], kind, f"composite {name} {kind}")
        Nf.same_bits_outside(got[name], clean[name], refs[name], f"composite {name} {kind}")
    assert torch.equal(got["mask"], clean["mask"])
    if kind == "nan":
        assert bool(torch.isnan(got["depth"][case.PLACE[0]])) and int(torch.isnan(got["depth"]).sum()) == 1


# ------------------------------------------------------------------------------------------------------------------------------------------
# F. the variance clamps
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", Nf.KINDS)
def test_density_features_variance(device, kind):
    """density_features, packed and generic kernel, golden volume_small_s0 with one feature pixel of view 0 planted: the voxels that project to it
    have a NaN mean AND a NaN exp(-var) in that channel (the clamp of the shifted one-pass variance must not turn it into exp(0)); every other
    value carries the bits of the run on the recorded maps."""
    from nerfdet_amd import ops
    case = Nf.density_case()
    g, refs, bars = case.g, case.refs(kind), case.bars()
    bias, rgb = case.bias.to(device), g["denorm_images"].to(device)[:, :, :case.H, :case.W]
    pts, proj, rgb_proj = g["points"].to(device), g["projection"].to(device), g["rgb_projection"].to(device)

    def run(m):
        md = m.to(device).contiguous(memory_format=torch.channels_last)
        return ops.density_features(md, bias, rgb, pts, proj, rgb_proj)
    assert ops.density_packed_ok(case.mapped.shape[0], case.mapped.shape[1], case.mapped.to(device).contiguous(memory_format=torch.channels_last), bias)
    saved = ops.density_packed_ok
    for form in ("packed", "generic"):
        if form == "generic":
            ops.density_packed_ok = lambda *a, **k: False
        try:
            got, recorded = run(case.inputs(kind)), run(case.mapped)
        finally:
            ops.density_packed_ok = saved
        fig = Nf.check(got, refs, bars, kind, f"density {form} {kind}")
        Nf.same_bits_outside(got, recorded, refs, f"density {form} {kind}")
        print(f"NONFINITE density {form} {kind}: {int(Nf.field(refs).sum())} elements in the field, worst error {fig['of_tol']:.2f} of the bar")


@pytest.mark.parametrize("kind", Nf.KINDS)
def test_ray_view_stats_variance(device, kind):
    """ray_view_stats (packed and generic kernel) and ray_view_stats_bank on golden rays_small_s0 with one feature pixel of view 0 planted: the
    samples whose bilinear taps touch it have a NaN mean and a NaN exp(-var) in that channel; all others, the masks and the view counts carry the
    bits of the run on the recorded maps."""
    from nerfdet_amd import rays
    case = Nf.ray_stats_case()
    refs, bars = case.refs(kind), case.bars()
    pts, img, cams = case.pts.to(device), case.img.to(device), case.cams
    n_v, d = case.feat.shape[:2]
    assert rays.packed_ok(n_v, d)

    def cl(f):
        return f.to(device).contiguous(memory_format=torch.channels_last)

    def bank(f):
        b = rays.ViewBank()
        b.append(cl(f), img, case.meta)
        return rays.ray_view_stats_bank(pts, b)
    saved = rays.packed_ok
    for form in ("packed", "generic", "bank"):
        if form == "generic":
            rays.packed_ok = lambda *a, **k: False
        try:
            run = bank if form == "bank" else (lambda f: rays.ray_view_stats(pts, img, cams, cl(f)))
            (got, pm, vc), (rec, pm_r, vc_r) = run(case.inputs(kind)), run(case.feat)
        finally:
            rays.packed_ok = saved
        fig = Nf.check(got, refs, bars, kind, f"ray stats {form} {kind}")
        Nf.same_bits_outside(got, rec, refs, f"ray stats {form} {kind}")
        assert torch.equal(pm, pm_r) and torch.equal(vc, vc_r), form
        print(f"NONFINITE ray stats {form} {kind}: {int(Nf.field(refs).sum())} elements in the field, worst error {fig['of_tol']:.2f} of the bar")
