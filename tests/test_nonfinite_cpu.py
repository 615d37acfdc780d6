"""The non-finite contract (tests/nonfinite_ref.py, DESIGN.md "Non-finite values") is one the reference itself meets: PyTorch-CPU fp32 of every
case, checked against the three float64 references, passes ``check`` for NaN, +Inf and -Inf; every case keeps at least 60 % of its output outside
the planted elements' field; and ``check`` fails on hand-made violations.  No GPU."""
import pytest
import torch

import nonfinite_ref as Nf
from test_f16x2_edges_gpu import ELEM_BAR, RMS_BAR

CONV_BARS = {"elem": ELEM_BAR, "rms": RMS_BAR}


def _holds(case, kind, bars, tag):
    """fp32 CPU against the float64 references on every output of ``case``; returns the smallest outside-the-field share."""
    refs, got = case.refs(kind), case.compute(kind, torch.float32)
    if not isinstance(refs, dict):
        refs, got, bars = {"out": refs}, {"out": got}, {"out": bars}
    share = 1.0
    for name, r in refs.items():
        fig = Nf.check(got[name], r, bars[name], kind, f"{tag} {name} {kind}")
        share = min(share, fig["outside"])
        assert fig["outside"] >= Nf.MIN_OUTSIDE, (tag, name, fig)
        if kind != "nan":          # the Inf kinds' non-finite elements lie inside the NaN field: the field is the receptive field
            assert not bool((~torch.isfinite(r.ref) & ~Nf.field(r)).any()), (tag, name)
    return share


@pytest.mark.parametrize("kind", Nf.KINDS)
@pytest.mark.parametrize("row", Nf.CONV_ROWS, ids=Nf.conv_row_id)
def test_convolution_rows(row, kind):
    case = Nf.conv_case(*row[1:10], row[11])
    share = _holds(case, kind, CONV_BARS, Nf.conv_row_id(row))
    if case.res_place is not None:           # the residual element really lies outside the three voxels' fields: it adds exactly its own footprint
        v = case._planted("nan", with_res=False)
        assert int(torch.isnan(v.forward(torch.float64)).sum()) < int(Nf.field(case.refs(kind)).sum())
    print(f"NONFINITE conv {Nf.conv_row_id(row)} {kind}: {share:.2f} outside the field")


@pytest.mark.parametrize("kind", Nf.KINDS)
def test_bf16_operand_references(kind):
    """The one-product arithmetic is defined on bf16-rounded operands: the same contract on those references."""
    for row in Nf.BF16_CONV_ROWS:
        case = Nf.conv_case(*row[1:10], row[11])
        refs = case.refs(kind, bf16_operands=True)
        Nf.check(case.compute(kind, torch.float32, bf16_operands=True), refs, {"rel": 2e-5}, kind, Nf.conv_row_id(row))
        assert Nf.outside_fraction(refs) >= Nf.MIN_OUTSIDE


@pytest.mark.parametrize("kind", Nf.KINDS)
def test_batched_row_keeps_the_other_volumes_clean(kind):
    case = Nf.batch_case()
    _holds(case, kind, CONV_BARS, "batch")
    f = Nf.field(case.refs(kind))
    assert bool(f[0].any()) and not bool(f[1:].any())


@pytest.mark.parametrize("kind", Nf.KINDS)
def test_fused_block_cases(kind):
    for relu3 in Nf.CHAIN_RELU3:
        _holds(Nf.chain_case(relu3), kind, CONV_BARS, f"chain relu{relu3}")
    for ds, nhw in Nf.BLOCK_SHAPES:
        _holds(Nf.block_case(ds, nhw), kind, CONV_BARS, f"bottleneck {ds} {nhw}")
    _holds(Nf.projection_case(), kind, {"out": CONV_BARS, "mapped": {"rel": 2e-5}}, "projection")
    for nhw, _ in Nf.STEM_SHAPES:
        _holds(Nf.stem_case(nhw), kind, CONV_BARS, f"stem {nhw}")


@pytest.mark.parametrize("kind", Nf.KINDS)
def test_pool_case_plants_under_larger_neighbours_and_over_the_border(kind):
    case = Nf.pool_case()
    _holds(case, kind, case.bars(), "pool")
    clean = case.compute("clean", torch.float64)
    ref = case.refs(kind).ref
    # (a): the window's maximum on clean data is NOT the planted pixel -- a maximum that drops the NaN returns that finite neighbour
    with torch.no_grad():
        act = torch.relu(case.bn.double()(case.inputs("clean").double().permute(0, 3, 1, 2))).permute(0, 2, 3, 1)
    assert float(act[0, 3, 3, 5]) < float(act[0, 2:5, 2:5, 5].max()) and float(clean[0, 1, 1, 5]) > 0
    # (b): the last pooled pixel's window hangs over the border
    if kind == "nan":
        assert bool(torch.isnan(ref[0, 1, 1, 5])) and bool(torch.isnan(ref[1, -1, -1, 63]))


@pytest.mark.parametrize("kind", Nf.KINDS)
@pytest.mark.parametrize("n,c,relu,with_res,where", Nf.bn_cases())
def test_batch_norm_rows(n, c, relu, with_res, where, kind):
    case = Nf.bn_case(n, c, relu, with_res, where)
    refs, got = case.refs(kind), case.compute(kind, torch.float32)
    for name, r in refs.items():
        # the home test's bar is max(3e-6, 2 x torch's own fp32 error); torch's fp32 IS the candidate here
        fig = Nf.check(got[name], r, {}, kind, f"bn {name}")
        Nf.check(got[name], r, {"rel": max(Nf.BN_BAR, 2 * fig.get("err", 0.0) / max(float(r.ref[~Nf.field(r)].abs().max()), 1e-12))}, kind, f"bn {name}")
        assert fig["outside"] >= Nf.MIN_OUTSIDE
    f = Nf.field(refs["y"])
    if where == "x" and kind == "nan":       # a NaN in x poisons exactly its channel, running_var included
        cols = sorted({p[1] for p in case.x_places})
        assert torch.nonzero(f.all(0)).squeeze(1).tolist() == cols
        for name in ("dx", "dgamma", "running_mean", "running_var"):
            fn = Nf.field(refs[name])
            assert torch.nonzero(fn if fn.dim() == 1 else fn.all(0)).squeeze(1).tolist() == cols, name
        # dbeta = sum over rows of dy [not (y <= 0)]: no x in it, and a NaN y opens the mask -- autograd's dbeta stays finite
        assert not bool(Nf.field(refs["dbeta"]).any())
        assert int(f.sum()) == len(cols) * n + (1 if with_res else 0)
    if where == "res":                       # one NaN y; threshold_backward lets its gradient through
        assert int(f.sum()) == 1 and not bool(Nf.field(refs["dx"]).any())
        i, j = case.res_places[0]
        assert float(refs["dres"].ref_nan[i, j]) == float(case.gy[i, j])


def test_relu_affine_bwd_reference_opens_the_mask_at_a_nan():
    g, y, scale = torch.tensor([[1.0, 2.0, 3.0, 4.0]]), torch.tensor([[float("nan"), 0.0, -1.0, 2.0]]), torch.tensor([2.0, 2.0, 2.0, -2.0])
    d_conv, d_id = Nf.relu_affine_bwd_reference(g, y, scale)
    assert d_id.tolist() == [[1.0, 0.0, 0.0, 4.0]] and d_conv.tolist() == [[2.0, 0.0, 0.0, -8.0]]


@pytest.mark.parametrize("kind", Nf.KINDS)
def test_density_mlp_rows(kind):
    case = Nf.mlp_case()
    _holds(case, kind, case.bars(), "mlp")
    refs = case.refs(kind)
    rows = torch.nonzero(Nf.field(refs["raw"])).squeeze(1).tolist()
    assert rows == case.rows and torch.equal(Nf.field(refs["h"]).all(1), Nf.field(refs["raw"]))


def test_sigma_to_alpha_values():
    x, want = (torch.tensor(v, dtype=torch.float64) for v in Nf.SIGMA_TO_ALPHA)
    got = 1 - torch.exp(-torch.relu(x))
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and float((got - want)[1:].abs().max()) < 1e-15


@pytest.mark.parametrize("kind", Nf.KINDS)
def test_compositor_ray(kind):
    case = Nf.composite_case()
    _holds(case, kind, case.bars(), "composite")
    refs = case.refs(kind)
    r, s, _ = case.PLACE
    for name in ("rgb", "depth"):
        assert torch.nonzero(Nf.field(refs[name]).reshape(case.R, -1).any(1)).squeeze(1).tolist() == [r], name
    f = Nf.field(refs["transparency"])
    assert int(f.sum()) == case.S - 1 - s and bool(f[r, s + 1:].all())     # T from the sample after the planted one on
    assert bool(Nf.field(refs["weights"])[r, s:].all()) and int(Nf.field(refs["weights"]).sum()) == case.S - s


@pytest.mark.parametrize("kind", Nf.KINDS)
def test_statistics_on_the_goldens(kind):
    for name, case in (("density", Nf.density_case()), ("ray stats", Nf.ray_stats_case())):
        refs = case.refs(kind)
        fig = Nf.check(case.compute(kind, torch.float32), refs, case.bars(), kind, name)
        f = Nf.field(refs)
        assert fig["outside"] >= Nf.MIN_OUTSIDE and bool(f.any())
        if kind == "nan":
            # mean AND exp(-var) of the planted channel, nothing else
            ch = 3 + case.CHANNEL
            cols = torch.nonzero(f.reshape(-1, f.shape[-1]).any(0)).squeeze(1).tolist()
            d = case.mapped.shape[1] if name == "density" else case.feat.shape[1]
            assert cols == ([2 * ch, 2 * ch + 1] if name == "density" else [ch, 3 + d + ch]), (name, cols)
        print(f"NONFINITE {name} {kind}: {int(f.reshape(-1, f.shape[-1]).any(1).sum())} rows in the field, {fig}")


# ------------------------------------------------------------------------------------------------------------------------------------------
# check() itself
# ------------------------------------------------------------------------------------------------------------------------------------------
def _toy():
    ref_clean = torch.arange(12, dtype=torch.float64).reshape(3, 4) + 1
    ref_nan = ref_clean.clone()
    ref_nan[1, :2] = float("nan")
    return ref_clean, ref_nan


def test_check_accepts_the_reference_and_rejects_violations():
    ref_clean, ref_nan = _toy()
    refs = Nf.Refs(ref_nan, ref_nan, ref_clean)
    bars = {"elem": 1e-6, "rms": 1e-6}
    Nf.check(ref_nan.float(), refs, bars, "nan")
    scrubbed = ref_nan.clone()
    scrubbed[1, 0] = 0.0                                   # a NaN scrubbed to 0
    with pytest.raises(AssertionError, match="NaN lost"):
        Nf.check(scrubbed, refs, bars, "nan")
    leaked = ref_nan.clone()
    leaked[2, 3] = float("nan")                            # a finite element turned NaN outside the field
    with pytest.raises(AssertionError, match="outside the planted"):
        Nf.check(leaked, refs, bars, "nan")
    off = ref_nan.clone()
    off[0, 0] += 1e-3                                      # a miss of the bar outside the field
    with pytest.raises(AssertionError, match="elem"):
        Nf.check(off, refs, bars, "nan")
    # Inf kinds: inside the field a finite reference frees the element, a non-finite one does not
    ref_inf = ref_clean.clone()
    ref_inf[1, 0], ref_inf[1, 1] = float("inf"), 0.0
    refs = Nf.Refs(ref_inf, ref_nan, ref_clean)
    wider = ref_inf.clone()
    wider[1, :2] = float("nan")                            # Inf - Inf = NaN: the wider poison
    Nf.check(wider, refs, bars, "+inf")
    lost = ref_inf.clone()
    lost[1, 0] = 0.0
    with pytest.raises(AssertionError, match="finite values where"):
        Nf.check(lost, refs, bars, "+inf")


def test_plant_and_three():
    x = torch.ones(2, 3)
    assert torch.isnan(Nf.plant(x, "nan", [(0, 1)])[0, 1]) and float(Nf.plant(x, "clean", [(1, 2)])[1, 2]) == 0 and float(x.sum()) == 6
    refs = Nf.three(lambda k: {"a": Nf.plant(x, k, [(0, 0)]) * 2}, "-inf")
    assert float(refs["a"].ref[0, 0]) == -float("inf") and bool(Nf.field(refs["a"])[0, 0]) and int(Nf.field(refs["a"]).sum()) == 1
    assert float(refs["a"].ref_clean[0, 0]) == 0


def test_ray_statistics_bar_is_widened_on_one_unseen_row_only():
    """The flat 2e-5 of tests/test_rays_gpu.py everywhere but on the one row that no view sees and on which float32 itself misses it."""
    case = Nf.ray_stats_case()
    rows, own = case.widened_rows()
    tol = case.bars()["tol"]
    assert int(rows.sum()) == 1 and bool((case.g["mask"][..., 0].sum(dim=2)[rows] == 0).all())
    assert bool((tol[~rows] == Nf.STATS_TOL[0]).all()) and float(tol[rows].max()) == 4 * float(own[rows].max())
    assert not bool((Nf.field(case.refs("nan")).any(-1) & rows).any())          # ... which lies outside the planted pixel's field


def test_every_relu_branch_has_a_row():
    """Each epilogue code path meets a ReLU after (1) and before (2) the residual: staged vector and scalar columns, direct, the vector and the
    non-vector split-K reduce, wave-specialised / persistent unsplit, halo unsplit."""
    rows = Nf.CONV_ROWS
    def has(pred):
        return {r[8] for r in rows if pred(r)} >= {1, 2}
    assert has(lambda r: r[3] == 25 and r[10] == 1) and has(lambda r: r[3] == 25 and r[10] > 1)                 # scalar columns: epilogue, reduce
    assert has(lambda r: r[0] in (64, 128) and r[10] == 1 and r[7] == "conv" and r[3] % 32 == 0)             # staged + direct
    assert has(lambda r: r[3] % 4 == 0 and r[10] > 1)                                                        # vector reduce
    assert has(lambda r: r[0] in (128256, 129256, 129257, 129064) and r[10] == 1 and r[9] == 1)              # ws / wsp unsplit
    assert has(lambda r: r[0] in (3128, 3256, 3257, 3258) and r[10] == 1)                                    # halo unsplit
    assert set(Nf.CHAIN_RELU3) == {1, 2}
