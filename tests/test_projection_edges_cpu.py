"""Conditions on the inputs of test_projection_edges_gpu.py, asserted from the CPU references alone (no kernel runs here).

The GPU tests hold every mask and count to equality and excuse nothing.  That is only fair if each decision is unambiguous: the float32
chain of the oracle and a float64 evaluation must agree on every (point, view) pair, samples no view sees must have exp(-var) of exactly
0 or 1, and every edge category must really be present where the kernels change tiles, waves and ballot rounds."""
import pytest
import torch

import projection_edges as E
from oracle import nerfdet_oracle as O
from projection_ref import _backproject64

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")     # the oracle's float32 FMA chain on inf / NaN points

NEAREST_CATEGORIES = {f"{a}_{b}" for a in ("lo", "hi", "s4_only", "s1_only", "huge") for b in "xy"} | {"d_zero", "d_neg", "gate"}
BILINEAR_CATEGORIES = {f"{a}_{b}" for a in ("out_near", "border", "inside", "out_feat") for b in "xy"} | \
    {"corner", "q2_pos", "q2_zero", "q2_neg", "clamped", "nonfinite"}


def _populated(scene, categories, untranslated_only):
    have = {(c, s, p) for c, s, p in zip(scene.category, scene.slot, scene.placement) if s is not None}
    assert set(scene.category[:16]) == set(categories) | set(untranslated_only), "the first 16-row tile holds a row of every category"
    for p in E.PLACEMENTS:
        for slot in range(4):
            for c in categories:
                assert (c, slot, p) in have, f"category {c} missing at {p}, edge view {scene.edge_views[slot]}"
            for c in untranslated_only:
                assert ((c, slot, p) in have) == (slot in E.UNTRANSLATED), f"{c} belongs to the untranslated cameras only"


@pytest.mark.parametrize("n_v,size", E.NEAREST_SCENES)
def test_nearest_scene_is_exact_and_complete(n_v, size):
    s = E.nearest_scene(n_v, size)
    assert torch.equal(s.rgb_proj[:, :2], 4 * s.proj[:, :2]) and torch.equal(s.rgb_proj[:, 2], s.proj[:, 2])
    assert all(s.n % m for m in (16, 64, 84, 124))
    assert s.edge_views == ((0, 1, 3, 4) if n_v == 5 else (0, 63, 64, n_v - 1))
    masks = {}
    for name, proj, (h, w), maps in (("s4", s.proj, (s.h, s.w), s.feat), ("s1", s.rgb_proj, (s.H, s.W), s.rgb)):
        _, valid = O.backproject(maps, s.points, proj)                      # the float32 chain
        valid = valid.reshape(n_v, -1)
        valid64, z64 = E.nearest_valid64(s.points, proj, h, w)
        assert torch.equal(valid, valid64), f"{name}: {int((valid != valid64).sum())} pairs decided differently in float32 and float64"
        blind = [v for v in range(n_v) if v not in s.edge_views]
        assert not valid[blind].any(), "a blind camera sees a point"
        # the gate, float32 and float64 map, against the band evaluated in float64 on the float64 depth
        for dt in (torch.float32, torch.float64):
            dmap = s.depth[dt] if name == "s4" else s.depth_r[dt]
            _, gated = _backproject64(maps.double(), s.points, proj, dmap, E.BAND)
            want = valid64 & (z64 > E.GATE_DEPTH - E.BAND) & (z64 < E.GATE_DEPTH + E.BAND)
            assert torch.equal(gated.reshape(n_v, -1), want), f"{name} gate, {dt} map"
            masks[name + "_gate"] = gated.reshape(n_v, -1)
        masks[name] = valid
    _populated(s, NEAREST_CATEGORIES, {"d_tiny"})
    # the hand-written expectation of every edge row, at its own camera
    for i in range(s.n):
        if s.slot[i] is None:
            continue
        v = s.edge_views[s.slot[i]]
        what = f"row {i} ({s.category[i]}, view {v}, point {s.points.reshape(3, -1)[:, i].tolist()})"
        assert bool(masks["s4"][v, i]) == s.expect4[i], what + " at stride 4"
        assert bool(masks["s1"][v, i]) == s.expect1[i], what + " at stride 1"
        if s.expect_gate[i] is not None:
            assert bool(masks["s4_gate"][v, i]) == (s.expect4[i] and s.expect_gate[i]), what + " gated, stride 4"
            assert bool(masks["s1_gate"][v, i]) == (s.expect1[i] and s.expect_gate[i]), what + " gated, stride 1"
    # what a scene must contain
    for name in ("s4", "s1", "s4_gate", "s1_gate"):
        m = masks[name]
        assert m.any() and not m.all()
        for slot, v in enumerate(s.edge_views):
            assert m[v].any(), f"{name}: edge view {v} sees nothing"
    cnt = masks["s4"].sum(0)
    assert (cnt == 0).any() and (cnt == 1).any() and (cnt >= 2).any()
    seen4, seen1 = masks["s4"].any(0), masks["s1"].any(0)
    assert (seen4 & ~seen1).any() and (seen1 & ~seen4).any(), "voxels seen in one map but not the other"
    gcnt = masks["s4_gate"].sum(0)
    assert (gcnt < cnt).any() and (gcnt == 0).any() and (gcnt >= 2).any()
    # density features: a voxel no view sees has its variance replaced by 1e6 (exp(-1e6) = 0 in every precision); the reference says so
    vol, valid = O.backproject(s.mapped.double(), s.points, s.proj)
    vol = vol + (~valid) * s.bias.double().view(1, -1, 1, 1, 1)
    rvol, _ = O.backproject(s.rgb.double(), s.points, s.rgb_proj)
    glob = O.density_features(vol, rvol, valid.sum(0), torch.eye(s.cm, dtype=torch.float64), torch.zeros(s.cm, dtype=torch.float64))
    unseen = cnt == 0
    assert (glob[unseen][:, 1::2] == 0).all() and torch.isfinite(glob[~unseen]).all()


def test_nearest_pins():
    """-0.5 is valid (rounds to -0); w - 0.5 is valid iff w is odd; d == 0 is not valid."""
    for size, (h, w) in E.SIZES.items():
        s = E.nearest_scene(5, size)
        _, valid = O.backproject(s.feat, s.points, s.proj)
        valid = valid.reshape(5, -1)
        at4 = lambda px, py, d: E._at(px, py, d, E.F1 / 4, E.CX1 / 4, E.CY1 / 4)
        pts = s.points.reshape(3, -1).t()
        for slot, v in enumerate(s.edge_views):
            def decided(pc):
                world = torch.tensor(E._world(slot, pc), dtype=torch.float32)
                rows = ((pts == world) | (torch.isnan(pts) & torch.isnan(world))).all(1).nonzero().flatten()
                assert len(rows) >= 3, f"point {pc} of camera {slot} is not in the scene three times"
                got = {bool(valid[v, i]) for i in rows.tolist()}
                assert len(got) == 1
                return got.pop()
            for d in (1.0, 2.0, 0.5):
                assert decided(at4(-0.5, E.Y0, d)) and decided(at4(E.X0, -0.5, d))
                assert not decided(at4(-0.75, E.Y0, d))
                assert decided(at4(w - 0.5, E.Y0, d)) == (w % 2 == 1)
                assert decided(at4(E.X0, h - 0.5, d)) == (h % 2 == 1)
                assert decided(at4(w - 1.5, E.Y0, d)) and not decided(at4(float(w), E.Y0, d))
            assert not decided((0.0, 0.0, 0.0)) and not decided(at4(E.X0, E.Y0, -1.0))
    assert {w % 2 for _, w in E.SIZES.values()} == {0, 1} and {h % 2 for h, _ in E.SIZES.values()} == {0, 1}


@pytest.mark.parametrize("n_v,size,d,kind", E.BILINEAR_SCENES)
def test_bilinear_scene_is_exact_and_complete(n_v, size, d, kind):
    s = E.bilinear_scene(n_v, size, d, kind)
    ref = E.bilinear_reference(n_v, size, d, kind)
    assert all(s.n % m for m in (16, 64, 84, 124))
    mask, count = ref["mask"], ref["count"]
    assert torch.equal(mask, E.bilinear_mask64(s.points, s.ke, s.h, s.w)), "pairs decided differently in float32 and float64"
    # ... and the oracle's own float32 path (bmm, grid_sample) takes the same decisions
    _, omask = O.projector_compute(s.points.view(-1, 1, 3), s.img.permute(0, 2, 3, 1).unsqueeze(0), s.cams, s.feat)
    assert torch.equal(omask.reshape(-1, n_v) > 0, mask)
    blind = [v for v in range(n_v) if v not in s.edge_views]
    assert not mask[:, blind].any() and not ref["near_feat"][:, blind].any() and not ref["near_img"][:, blind].any()
    _populated(s, BILINEAR_CATEGORIES, {"q2_tiny"})
    near_f, near_i = ref["near_feat"], ref["near_img"]
    tally = {"out_near": 0, "img_only": 0}
    for i in range(s.n):
        if s.slot[i] is None:
            continue
        v = s.edge_views[s.slot[i]]
        what = f"row {i} ({s.category[i]}, view {v}, point {s.points[i].tolist()})"
        if s.expect[i] is not None:
            assert bool(mask[i, v]) == s.expect[i], what
        if s.category[i].startswith("out_near"):
            assert near_f[i, v] and not mask[i, v], what + ": masked out, but a tap reaches the feature map"
            tally["out_near"] += 1
        if s.category[i].startswith("out_feat"):
            assert not near_f[i, v] and not mask[i, v], what
            tally["img_only"] += int(near_i[i, v])
    # taps inside the image but outside the feature map need an image smaller than the feature map: with W > wf the image's interval of
    # normalised coordinates with a tap, (-1/(W-1), W/(W-1)), lies inside the feature map's
    assert tally["out_near"] > 0 and (tally["img_only"] > 0) == (kind == "tiny")
    assert (count == 0).any() and (count == 1).any() and (count >= 2).any()
    for slot, v in enumerate(s.edge_views):
        assert mask[:, v].any() and not mask[:, v].all()
        assert (near_f[:, v] & ~mask[:, v]).any(), f"edge view {v}: no masked-out sample with a tap in its map"
    # samples no view contains: exp(-var) must be exactly 1 (no tap reaches a map) or exactly 0 (var far above 100) in both precisions
    unseen = count == 0
    for key in ("var_img", "var_feat"):
        var = ref[key][unseen]
        assert ((var == 0) | (var > 100)).all(), f"{key}: {int(((var != 0) & ~(var > 100)).sum())} exponents in between"
        assert (var == 0).any() and (var > 100).any()
    nch = 3 + d
    ev = ref["glob"][unseen][:, nch:]
    assert ((ev == 0) | (ev == 1)).all() and (ref["glob"][unseen][:, :nch] == 0).all()


def test_bilinear_pins():
    """px == w - 1 is inside the mask and px == w - 1 + 0.25 is not; q2 == 0 is invalid."""
    for size, (hf, wf) in E.SIZES.items():
        s = E.bilinear_scene(5, size, 8)
        mask = E.bilinear_reference(5, size, 8)["mask"]
        h, w = 4.0 * hf, 4.0 * wf
        at1 = lambda px, py, q2: E._at(px, py, q2, E.F1, E.CX1, E.CY1)
        for slot, v in enumerate(s.edge_views):
            def decided(pc):
                world = torch.tensor(E._world(slot, pc), dtype=torch.float32)
                rows = (s.points == world).all(1).nonzero().flatten()
                assert len(rows) >= 3, f"point {pc} of camera {slot} is not in the scene three times"
                got = {bool(mask[i, v]) for i in rows.tolist()}
                assert len(got) == 1
                return got.pop()
            assert decided(at1(w - 1.0, 8.0, 1.0)) and not decided(at1(w - 0.75, 8.0, 1.0))
            assert decided(at1(12.0, h - 1.0, 1.0)) and not decided(at1(12.0, h - 0.75, 1.0))
            assert decided(at1(0.0, 8.0, 1.0)) and not decided(at1(-0.5, 8.0, 1.0))
            assert decided(at1(w - 1.0, h - 1.0, 1.0)) and decided(at1(0.0, 0.0, 1.0))
            assert not decided((0.0, 0.0, 0.0)), "q2 == 0 with px = py = 0"
            assert not decided((E.CX1 / E.F1, E.CY1 / E.F1, -1.0)), "q2 < 0 with px = py = 0"


# ----------------------------------------------------------------------------------------------------------------------------------
# the scenes tell a slipped rule from the right one: each slip of projection_edges.NEAREST_SLIPS / BILINEAR_SLIPS, applied to the
# reference rule, changes decisions at every edge camera of every scene -- so a kernel with that slip cannot meet the equalities of
# test_projection_edges_gpu.py
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_v,size", E.NEAREST_SCENES)
def test_nearest_scenes_tell_slipped_rules_apart(n_v, size):
    s = E.nearest_scene(n_v, size)
    for proj, h, w, maps in ((s.proj, s.h, s.w, s.feat), (s.rgb_proj, s.H, s.W, s.rgb)):
        right, x0, y0 = E.nearest_rule(s.points, proj, h, w)
        assert torch.equal(right, O.backproject(maps, s.points, proj)[1].reshape(n_v, -1)), "the restated rule is not the oracle's"
        gated, _, _ = E.nearest_rule(s.points, proj, h, w, depth=E.GATE_DEPTH)
        _, want = _backproject64(maps.double(), s.points, proj, torch.full((n_v, h, w), E.GATE_DEPTH), E.BAND)
        assert torch.equal(gated, want.reshape(n_v, -1))
        for slip in E.NEAREST_SLIPS:
            depth = E.GATE_DEPTH if slip.startswith("band") else None
            base = gated if depth is not None else right
            got, x, y = E.nearest_rule(s.points, proj, h, w, slip, depth)
            for v in s.edge_views:
                assert (got[v] != base[v]).any(), f"{slip}: no decision of view {v} changes"
            assert (got.sum(0) != base.sum(0)).any(), f"{slip}: no view count changes"
            if slip == "roundf":          # ... and ties that stay valid read another pixel
                both = got & base
                assert ((x != x0) & both).any() and ((y != y0) & both).any()
        # d >= 0 in place of d > 0 is no slip of THIS rule: a point with d == 0 has the quotients u / 0, v / 0, never a number in [0, w)
        assert torch.equal(E.nearest_rule(s.points, proj, h, w, "d_ge_0")[0], right)
        assert (O.project_voxels(s.points, proj)[2] == 0).any()


@pytest.mark.parametrize("n_v,size,d,kind", E.BILINEAR_SCENES)
def test_bilinear_scenes_tell_slipped_rules_apart(n_v, size, d, kind):
    s = E.bilinear_scene(n_v, size, d, kind)
    ref = E.bilinear_reference(n_v, size, d, kind)
    mask, tap = E.bilinear_rule(s.points, s.ke, s.h, s.w, s.hf, s.wf)
    assert torch.equal(mask, ref["mask"]) and torch.equal(tap, ref["near_feat"]), "the restated rule is not the reference's"
    for slip in E.BILINEAR_SLIPS:
        got_mask, got_tap = E.bilinear_rule(s.points, s.ke, s.h, s.w, s.hf, s.wf, slip)
        got, base = (got_tap, tap) if slip.endswith("from_0") else (got_mask, mask)
        for v in s.edge_views:
            assert (got[:, v] != base[:, v]).any(), f"{slip}: no decision of view {v} changes"
        if not slip.endswith("from_0"):
            assert (got.sum(1) != base.sum(1)).any(), f"{slip}: no view count changes"
        else:   # a dropped tap changes a value that is compared: the sample's variance term of a masked-out view, or its mean
            assert ((got != base) & ~mask).any() and ((got != base).any(1) & (ref["count"] > 0)).any()
