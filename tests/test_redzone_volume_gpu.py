"""The volume path inside tests/redzone.py: backproject, backproject_aggregate, density_features (packed and generic, plain and depth-gated),
depth_resize, and scene_accumulate followed by every finish -- stream, ring, group and group-ring, density and volume.  Every row twice, fill 0x00
then 0xFF, feature maps / mapped maps / images / depth / points / projections placed flush against guards, outputs and the scene states (SceneState
allocates its sums with torch.zeros) carved: no guard byte and no input changed, the results equal bit for bit.  Numbers are held to the oracle
and to fp64 by tests/test_volume_gpu.py, test_depth_gate_gpu.py, test_streaming_gpu.py, test_streaming_window_gpu.py, test_scene_group_gpu.py and
test_group_window_gpu.py.  Every kernel here sums a voxel's views in view order in one thread ("K1's sums hold the same bits whatever the
chunking"): there is no atomic and no mode to select."""
import pytest
import torch

from oracle import nerfdet_oracle as O
from redzone import both_fills

pytestmark = pytest.mark.gpu

SHAPES = [(7, 8, (60, 80), (10, 6, 5)), (3, 48, (48, 64), (9, 7, 3))]        # (n_v, cm, hw, grid)
VS = (0.5, 0.5, 0.5)
_CACHE = {}


def _case(device, n_v, cm, hw, grid, c=32):
    """CPU inputs of one shape, made once: tests/test_streaming_gpu.py::_inputs with every tensor left on the host."""
    from nerfdet_amd import ops
    key = (n_v, cm, hw, grid)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(n_v * 10 + cm)
        meta = O.ring_scene_meta(n_v, hw)
        h, w = hw[0] // 4, hw[1] // 4
        feats = torch.randn(n_v, c, h, w, generator=g).contiguous(memory_format=torch.channels_last)
        weight, bias = torch.randn(cm, c, generator=g) / c ** 0.5, torch.randn(cm, generator=g) * 0.5
        mapped = torch.nn.functional.linear(feats.permute(0, 2, 3, 1), weight, bias).permute(0, 3, 1, 2)
        assert mapped.stride(1) == 1
        _CACHE[key] = dict(
            meta=meta, feats=feats, mapped=mapped, bias=bias, rgb=torch.rand(n_v, 3, *hw, generator=g),
            depth=torch.rand(n_v, hw[0] // 2 + 1, hw[1] // 2 + 1, generator=g, dtype=torch.float64) * 5.0 + 0.5,
            points=ops.get_points(grid, VS, meta["lidar2img"]["origin"], device).cpu(),
            proj=ops.compute_projection(meta, 4, device).cpu(), rgb_proj=ops.compute_projection(meta, 1, device).cpu(),
            alpha=torch.rand(grid[0] * grid[1] * grid[2], generator=g), hw=hw, fhw=(h, w), grid=grid, c=c, cm=cm, n_v=n_v)
    return _CACHE[key]


def _placed(rz, d, v0=0, v1=None):
    """The views [v0, v1) of a case as placed device tensors (+ the placed depth map, not yet resized)."""
    sl = slice(v0, v1)
    return dict(feats=rz.place(d["feats"][sl], "features"), mapped=rz.place(d["mapped"][sl], "mapped"), bias=rz.place(d["bias"], "bias"),
                rgb=rz.place(d["rgb"][sl].contiguous(), "images"), points=rz.place(d["points"], "points"), proj=rz.place(d["proj"][sl].contiguous(), "projection"),
                rgb_proj=rz.place(d["rgb_proj"][sl].contiguous(), "rgb_projection"), depth=rz.place(d["depth"][sl].contiguous(), "depth"))


def _gate(d, p, gated):
    from nerfdet_amd import ops
    return ops.depth_gate(p["depth"], VS, d["fhw"], d["hw"]) if gated else None


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("n_v,cm,hw,grid", SHAPES)
def test_redzone_depth_resize(device, n_v, cm, hw, grid, dtype):
    """An odd-sized (hw / 2 + 1) map resized to the feature map and to the image in one launch, in the map's own dtype; a pitched view too."""
    from nerfdet_amd import ops
    d = _case(device, n_v, cm, hw, grid)
    depth = d["depth"].to(dtype)

    def body(rz):
        whole = rz.place(depth, "depth")
        f, r = ops.depth_resize(whole, d["fhw"], d["hw"])
        f2, none = ops.depth_resize(whole[:, 1:, 2:], d["fhw"])
        assert none is None
        return {"depth_f": f, "depth_r": r, "crop_f": f2}
    both_fills(device, body)


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
@pytest.mark.parametrize("n_v,cm,hw,grid", SHAPES)
def test_redzone_backproject(device, n_v, cm, hw, grid, gated):
    from nerfdet_amd import ops
    d = _case(device, n_v, cm, hw, grid)

    def body(rz):
        p = _placed(rz, d)
        vol, valid = ops.backproject(p["feats"], p["points"], p["proj"], depth=p["depth"] if gated else None, voxel_size=VS)
        return {"volume": vol, "valid": valid}
    both_fills(device, body)


@pytest.mark.parametrize("layout", ["channels_last", "contiguous"])
@pytest.mark.parametrize("with_alpha", [False, True], ids=["mean", "alpha"])
@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
@pytest.mark.parametrize("n_v,cm,hw,grid", SHAPES)
def test_redzone_backproject_aggregate(device, n_v, cm, hw, grid, gated, with_alpha, layout):
    from nerfdet_amd import ops
    d = _case(device, n_v, cm, hw, grid)

    def body(rz):
        p = _placed(rz, d)
        vol, count = ops.backproject_aggregate(p["feats"], p["points"], p["proj"], alpha=rz.place(d["alpha"], "alpha") if with_alpha else None,
                                               channels_last_out=layout == "channels_last", depth_gate=_gate(d, p, gated))
        return {"volume": vol, "count": count}
    both_fills(device, body)


@pytest.mark.parametrize("kernel", ["packed", "generic"])
@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
@pytest.mark.parametrize("n_v,cm,hw,grid", SHAPES)
def test_redzone_density_features(device, n_v, cm, hw, grid, gated, kernel):
    from nerfdet_amd import ops

    d = _case(device, n_v, cm, hw, grid)

    def body(rz):
        p = _placed(rz, d)
        saved = ops.density_packed_ok
        if kernel == "generic":
            ops.density_packed_ok = lambda *a, **k: False
        try:
            assert kernel == "generic" or ops.density_packed_ok(n_v, cm, ops.to_channels_last(p["mapped"]), p["bias"])
            rows = ops.density_features(p["mapped"], p["bias"], p["rgb"], p["points"], p["proj"], p["rgb_proj"], depth_gate=_gate(d, p, gated))
        finally:
            ops.density_packed_ok = saved
        return {"rows": rows}
    got = both_fills(device, body)
    assert got["rows"].shape == (grid[0] * grid[1] * grid[2], 2 * (3 + cm))


def _finishes(ops, kind, bias, alpha, states=None, group=None, scenes=None):
    if kind == "stream":
        rows, (vol, count) = ops.density_finish(states[0], bias), ops.volume_finish(states[0], alpha)
    elif kind == "ring":
        rows, (vol, count) = ops.density_finish_ring(states, bias), ops.volume_finish_ring(states, alpha)
    elif kind == "group":
        rows, (vol, count) = ops.density_finish_group(group, bias, scenes), ops.volume_finish_group(group, alpha, scenes)
    else:
        rows, (vol, count) = ops.density_finish_group_ring(group, bias, scenes), ops.volume_finish_group_ring(group, alpha, scenes)
    return {"rows": rows, "volume": vol, "count": count}


@pytest.mark.parametrize("with_alpha", [False, True], ids=["mean", "alpha"])
@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
@pytest.mark.parametrize("kind", ["stream", "ring"])
@pytest.mark.parametrize("n_v,cm,hw,grid", SHAPES)
def test_redzone_scene_accumulate_and_finish(device, n_v, cm, hw, grid, kind, gated, with_alpha):
    """stream: one state fed in two chunks; ring: one state per chunk (1 view, then the rest), finished together."""
    from nerfdet_amd import ops
    d = _case(device, n_v, cm, hw, grid)

    def body(rz):
        states = [ops.SceneState(grid, d["c"], cm, device) for _ in range(1 if kind == "stream" else 2)]
        for i, (v0, v1) in enumerate([(0, 1), (1, n_v)]):
            p = _placed(rz, d, v0, v1)
            ops.scene_accumulate(states[i % len(states)], p["feats"], p["mapped"], p["bias"], p["rgb"], p["points"], p["proj"], p["rgb_proj"],
                                 depth_gate=_gate(d, p, gated))
        out = _finishes(ops, kind, rz.place(d["bias"], "bias"), rz.place(d["alpha"], "alpha") if with_alpha else None, states=states)
        for i, st in enumerate(states):
            out.update({f"k1_sum{i}": st.k1_sum, f"k1_count{i}": st.k1_count, f"k2_sum{i}": st.k2_sum, f"k2_count{i}": st.k2_count})
        return out
    both_fills(device, body)


@pytest.mark.parametrize("with_alpha", [False, True], ids=["mean", "alpha"])
@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
@pytest.mark.parametrize("kind", ["group", "group_ring"])
@pytest.mark.parametrize("n_v,cm,hw,grid", SHAPES)
def test_redzone_scene_groups(device, n_v, cm, hw, grid, kind, gated, with_alpha):
    """Two scenes of unequal view counts over shifted lattices: both take view 0, then scene 1 alone takes the other views (a grouped call brings the
    same number of views to every listed scene); the finishes list the scenes as [1, 0]."""
    from nerfdet_amd import ops
    d = _case(device, n_v, cm, hw, grid)
    n = grid[0] * grid[1] * grid[2]

    def views(rz, idx):
        pick = lambda t: t[idx].contiguous()
        feats = d["feats"][idx].contiguous(memory_format=torch.channels_last)
        mapped = d["mapped"].permute(0, 2, 3, 1)[idx].contiguous().permute(0, 3, 1, 2)
        p = dict(feats=rz.place(feats, "features"), mapped=rz.place(mapped, "mapped"), rgb=rz.place(pick(d["rgb"]), "images"),
                 proj=rz.place(pick(d["proj"]), "projection"), rgb_proj=rz.place(pick(d["rgb_proj"]), "rgb_projection"),
                 depth=rz.place(pick(d["depth"]), "depth"))
        return p, _gate(d, p, gated)

    def body(rz):
        points = [rz.place(d["points"], "points0"), rz.place(d["points"] + 0.25, "points1")]
        bias = rz.place(d["bias"], "bias")
        if kind == "group":
            group = ops.SceneGroupState(grid, d["c"], cm, points, device)
            add = lambda scenes, p, g: ops.scene_accumulate_group(group, scenes, p["feats"], p["mapped"], bias, p["rgb"], p["proj"], p["rgb_proj"], depth_gate=g)
        else:
            group = ops.SceneGroupRingState(grid, d["c"], cm, points, 2, device)
            add = lambda scenes, p, g: ops.scene_accumulate_group_ring(group, scenes, p["feats"], p["mapped"], bias, p["rgb"], p["proj"], p["rgb_proj"],
                                                                       depth_gate=g)
        p, g = views(rz, [0, 0])
        add([0, 1], p, g)
        p, g = views(rz, list(range(1, n_v)))
        add([1], p, g)
        assert group.n_views == [1, n_v]
        alpha = rz.place(torch.cat([d["alpha"], d["alpha"].flip(0)]), "alpha") if with_alpha else None
        out = _finishes(ops, kind, bias, alpha, group=group, scenes=[1, 0])
        states = group.states
        for i, st in enumerate(states):
            out.update({f"k1_sum{i}": st.k1_sum, f"k1_count{i}": st.k1_count, f"k2_sum{i}": st.k2_sum, f"k2_count{i}": st.k2_count})
        return out
    got = both_fills(device, body)
    assert got["rows"].shape == (2 * n, 2 * (3 + cm)) and got["count"].shape == (2, 1, *grid)
