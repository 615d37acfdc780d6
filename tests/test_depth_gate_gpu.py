"""GPU parity of the depth-gated backprojection (RGB-D scenes; mmdet3d/models/detectors/nerfdet.py:404-411): the resize kernel against
F.interpolate, the exact-API backproject, K1, both K2 kernels, the inference chain and its gradients against the real reference's fixtures
(tests/golden/make_golden_depth.py) and the gate restated on the CPU (tests/depth_gate_ref.py)."""
import copy
import importlib.util
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import golden_meta, load_golden, sub_state
from depth_gate_ref import gate_terms, oracle_extract_volume, plane_depth, resize_depth
from oracle import nerfdet_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _modules(g, device):
    from nerfdet_amd.radiance_field import VanillaNeRFRadianceField
    sd = sub_state(g, "nerf_mlp.")
    width = sd["mlp.base.hidden_layers.0.weight"].shape[0]
    fdim = sd["mlp.base.hidden_layers.0.weight"].shape[1] - 63
    mlp = VanillaNeRFRadianceField(4, width, 3, fdim, 1, width // 2)
    mlp.load_state_dict(sd)
    mapping = torch.nn.Sequential(torch.nn.Linear(g["mapping.0.weight"].shape[1], g["mapping.0.weight"].shape[0]))
    mapping.load_state_dict(sub_state(g, "mapping."))
    return mapping.to(device), mlp.to(device).eval()


def _edge_pairs(g, h, w, tol_rel=1e-6):
    """(voxel, view) pairs whose camera depth lies within tol_rel * d of a band edge: where the resize's last bits may decide."""
    vs = [float(v) for v in g["voxel_size"]]
    _, ungated, z, dv = gate_terms(g["points"], g["projection"], h, w, g["depth"], vs)
    tol = tol_rel * dv.abs().double().clamp(min=1.0)
    near = ((z.double() - (dv.double() - vs[-1])).abs() < tol) | ((z.double() - (dv.double() + vs[-1])).abs() < tol)
    return near & ungated


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_resize_matches_interpolate(device, dtype):
    from nerfdet_amd import ops
    torch.manual_seed(0)
    for src, fhw, ihw in [((240, 320), (60, 80), (240, 320)), ((480, 640), (120, 160), (480, 640)), ((60, 80), (15, 20), (60, 80))]:
        d = torch.rand(5, *src, dtype=dtype) * 6
        d[:, ::7, ::5] = 0
        got_f, got_r = ops.depth_resize(d.to(device), fhw, ihw)
        assert got_f.dtype == dtype and torch.equal(got_f.cpu(), resize_depth(d, fhw)), (src, fhw)
        assert torch.equal(got_r.cpu(), resize_depth(d, ihw)), (src, ihw)
    # non-integer ratios: a few ulp (PyTorch's CPU path forms the weights differently there)
    for src, fhw in [((237, 311), (60, 80)), ((47, 61), (15, 20)), ((968, 1296), (60, 80))]:
        d = torch.rand(3, *src, dtype=dtype) * 6
        got, _ = ops.depth_resize(d.to(device), fhw)
        ref = resize_depth(d, fhw)
        assert float((got.cpu() - ref).abs().max()) <= (4e-6 if dtype == torch.float32 else 1e-14) * 6


def test_backproject_with_depth_matches_reference_loader_scene(device):
    """float64 depth at img_shape (the loader's maps), integer ratio: validity and volume bit-exact."""
    from nerfdet_amd import ops
    g = load_golden("volume_depth_s0")
    meta = golden_meta(g)
    h, w = meta["img_shape"][0] // 4, meta["img_shape"][1] // 4
    vs = g["voxel_size"].tolist()
    for cl in (False, True):
        f = g["features"].to(device)
        if cl:
            f = f.contiguous(memory_format=torch.channels_last)
        vol, valid = ops.backproject(f[:, :, :h, :w], g["points"].to(device), g["projection"].to(device), g["depth"].to(device), vs)
        assert torch.equal(valid.cpu(), g["bp_valid"])
        assert torch.equal(vol[0].cpu(), g["bp_volume_v0"])
        torch.testing.assert_close(vol.sum(0).cpu(), g["bp_volume_sum"], rtol=0, atol=2e-5)   # the view sum's order is the device's
    _, rvalid = ops.backproject(g["denorm_images"].to(device), g["points"].to(device), g["rgb_projection"].to(device), g["depth"].to(device), vs)
    assert torch.equal(rvalid.cpu(), g["rgb_bp_valid"])
    # the ungated call differs: the gate is really applied
    _, valid0 = ops.backproject(g["features"].to(device)[:, :, :h, :w], g["points"].to(device), g["projection"].to(device))
    assert int(valid0.sum()) > 2 * int(valid.sum())


def test_backproject_with_depth_non_integer_ratio_float32(device):
    """float32 depth at 47x61 with holes: validity may differ only where z is within 1e-6 d of a band edge, under 0.1 % of the pairs."""
    from nerfdet_amd import ops
    g = load_golden("volume_depth_s1")
    meta = golden_meta(g)
    h, w = meta["img_shape"][0] // 4, meta["img_shape"][1] // 4
    _, valid = ops.backproject(g["features"].to(device)[:, :, :h, :w], g["points"].to(device), g["projection"].to(device),
                               g["depth"].to(device), g["voxel_size"].tolist())
    diff = (valid.cpu() != g["bp_valid"]).reshape(valid.shape[0], -1)
    near = _edge_pairs(g, h, w)
    n_diff, n_pairs = int(diff.sum()), diff.numel()
    print(f"non-integer ratio: {n_diff} of {n_pairs} (voxel, view) pairs differ, {int(near.sum())} within 1e-6 d of a band edge")
    assert not (diff & ~near).any()
    assert n_diff <= 0.001 * n_pairs


@pytest.mark.parametrize("name", ["volume_depth_s0", "volume_depth_s1"])
def test_k1_gated_counts_and_mean(device, name):
    from nerfdet_amd import ops
    g = load_golden(name)
    meta = golden_meta(g)
    h, w = meta["img_shape"][0] // 4, meta["img_shape"][1] // 4
    gate = ops.depth_gate(g["depth"].to(device), g["voxel_size"].tolist(), (h, w))
    f = g["features"].to(device).contiguous(memory_format=torch.channels_last)[:, :, :h, :w]
    for cl in (True, False):
        mean, cnt = ops.backproject_aggregate(f, g["points"].to(device), g["projection"].to(device), channels_last_out=cl, depth_gate=gate)
        ref_cnt = g["bp_valid"].sum(0)
        if name == "volume_depth_s0":
            assert torch.equal(cnt.cpu(), ref_cnt)
        else:   # non-integer ratio: only voxels with a pair at a band edge may differ
            near = _edge_pairs(g, h, w).any(0).view_as(ref_cnt)
            assert not ((cnt.cpu() != ref_cnt) & ~near).any()
        ref_mean = g["bp_volume_sum"] / (ref_cnt + 1e-8)
        ref_mean[:, ref_cnt[0] == 0] = 0
        same = (cnt.cpu() == ref_cnt)[0]
        err = (mean.cpu() - ref_mean)[:, same].abs().max()
        assert float(err) <= 1e-6 * max(1.0, float(ref_mean.abs().max()))


@pytest.mark.parametrize("packed", [True, False])
def test_k2_gated_vs_oracle(device, monkeypatch, packed):
    from nerfdet_amd import ops
    from nerfdet_amd.volume import map_features_2d
    g = load_golden("volume_depth_s0")
    meta = golden_meta(g)
    mapping, mlp = _modules(g, device)
    vs = g["voxel_size"].tolist()
    h, w = meta["img_shape"][0] // 4, meta["img_shape"][1] // 4
    with torch.no_grad():
        ov = oracle_extract_volume(monkeypatch, g["depth"], vs, g["features"], g["denorm_images"], meta, g["n_voxels"].tolist(), vs,
                                   mapping[0].weight.cpu(), mapping[0].bias.cpu(), {k: v.cpu() for k, v in mlp.state_dict().items()})
        f = g["features"].to(device)[:, :, :h, :w]
        mapped = map_features_2d(f, mapping[0].weight, mapping[0].bias)
        gate = ops.depth_gate(g["depth"].to(device), vs, (h, w), meta["img_shape"][:2])
        if not packed:
            monkeypatch.setattr(ops, "density_packed_ok", lambda *a, **k: False)
        glob = ops.density_features(mapped, mapping[0].bias, g["denorm_images"].to(device), g["points"].to(device), g["projection"].to(device),
                                    g["rgb_projection"].to(device), depth_gate=gate)
    seen = ov["valid"].reshape(-1) > 0
    assert int(seen.sum()) > 20
    err = float((glob.cpu() - ov["global_feat"])[seen].abs().max())
    assert err <= 1e-4 * max(1.0, float(ov["global_feat"][seen].abs().max())), err
    # unseen voxels: the reference's n_v*b/1e-8 "mean" and cov = exp(-1e6): same rule as the ungated K2 tests (relative)
    un = ~seen
    torch.testing.assert_close(glob.cpu()[un], ov["global_feat"][un], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("name", ["volume_depth_s0", "volume_depth_s1"])
def test_extract_volume_with_depth_matches_reference(device, name):
    """The whole inference chain with depth == the real reference's extract_feat(..., depth) output."""
    from nerfdet_amd.volume import extract_volume
    g = load_golden(name)
    meta = golden_meta(g)
    mapping, mlp = _modules(g, device)
    h, w = meta["img_shape"][0] // 4, meta["img_shape"][1] // 4
    with torch.no_grad():
        out = extract_volume(g["features"].to(device).contiguous(memory_format=torch.channels_last), g["denorm_images"].to(device), meta,
                             g["n_voxels"].tolist(), g["voxel_size"].tolist(), mapping, mlp, depth=g["depth"].to(device))
        plain = extract_volume(g["features"].to(device).contiguous(memory_format=torch.channels_last), g["denorm_images"].to(device), meta,
                               g["n_voxels"].tolist(), g["voxel_size"].tolist(), mapping, mlp)
    if name == "volume_depth_s0":
        assert torch.equal(out["valid"].cpu(), g["out_valid"])
        ok = torch.ones(g["out_valid"][0].shape, dtype=torch.bool)
    else:
        ok = (out["valid"].cpu() == g["out_valid"])[0] & ~_edge_pairs(g, h, w).any(0).view_as(g["out_valid"][0])
        assert float(ok.float().mean()) > 0.99
    err = float((out["volume"].cpu() - g["out_volume"])[:, ok].abs().max())
    assert err <= 1e-4 * max(1.0, float(g["out_volume"].abs().max())), err
    assert not torch.equal(out["valid"], plain["valid"])


def test_gradients_through_the_gate(device, monkeypatch):
    """Training: d(features) and d(mapping) of a random linear functional of extract_volume(..., depth) against autograd through the
    restated reference in float64; deterministic mode bitwise reproducible."""
    from nerfdet_amd import autograd as A
    from nerfdet_amd.volume import extract_volume
    g = load_golden("volume_depth_s0")
    meta = golden_meta(g)
    mapping, mlp = _modules(g, device)
    vs = g["voxel_size"].tolist()
    torch.manual_seed(3)
    probe = torch.randn(g["out_volume"].shape, dtype=torch.float64)

    def run():
        f = g["features"].to(device).contiguous(memory_format=torch.channels_last).requires_grad_(True)   # the FPN's layout
        mapping.zero_grad()
        out = extract_volume(f, g["denorm_images"].to(device), meta, g["n_voxels"].tolist(), vs, mapping, mlp, channels_last_out=False,
                             depth=g["depth"].to(device))
        (out["volume"].double() * probe.to(device)).sum().backward()
        return f.grad.cpu().clone(), mapping[0].weight.grad.cpu().clone(), mapping[0].bias.grad.cpu().clone(), out["valid"].cpu()

    gf, gw, gb, cnt = run()
    assert torch.equal(cnt, g["out_valid"])
    # reference side: float64 autograd through the oracle with the gated backproject (gate decisions from the float32 projection)
    fr = g["features"].double().clone().requires_grad_(True)
    wr = mapping[0].weight.detach().cpu().double().clone().requires_grad_(True)
    br = mapping[0].bias.detach().cpu().double().clone().requires_grad_(True)
    sd = {k: v.detach().cpu().double() for k, v in mlp.state_dict().items()}
    ov = oracle_extract_volume(monkeypatch, g["depth"], vs, fr, g["denorm_images"].double(), meta, g["n_voxels"].tolist(), vs, wr, br, sd)
    (ov["volume"] * probe).sum().backward()
    for got, ref, what in ((gf, fr.grad, "features"), (gw, wr.grad, "mapping.weight"), (gb, br.grad, "mapping.bias")):
        scale = max(1.0, float(ref.abs().max()))
        err = float((got.double() - ref).abs().max())
        assert err <= 1e-5 * scale, f"d{what}: {err} (scale {scale})"
    prev = A.set_deterministic(True)
    try:
        a, b = run(), run()
    finally:
        A.set_deterministic(prev)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_cfg2_full_size_with_depth(device, monkeypatch):
    """cfg2 shapes (50 views 240x320, 40x40x16), float64 depth of a plane at img_shape: view counts bit-exact against the restated gate,
    the gated volume against the oracle with the gated backproject, identical detections on identical head outputs, defer=True equal
    to the direct call, and different from the ungated result."""
    bench = _bench()
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    w = bench.WORKLOADS["cfg2"]
    det_cpu = bench.build_model(w)
    batch_cpu = bench.synth_batch(w, 0)
    meta = batch_cpu["img_metas"][0]
    depth = plane_depth(meta, w["img_hw"], 0.45, noise=0.03, seed=5).unsqueeze(0)
    det = copy.deepcopy(det_cpu).to(device)
    batch = bench.to_device(batch_cpu, device)
    import nerfdet_amd.volume as V
    tc = det_cpu.bbox_head.test_cfg
    with torch.no_grad():
        x, _, stride = det.extract_2d(batch["img"])
        out = V.extract_volume(x, batch["denorm_images"][0], meta, det.n_voxels, det.voxel_size, det.mapping, det.nerf_mlp, stride=stride,
                               channels_last_out=True, depth=depth[0].to(device))
        ctr, reg, cls = det.bbox_head(det.neck_3d(out["volume"].unsqueeze(0)))
        rb = det._ray_batch(batch)
        res = det.simple_test(batch["img"], batch["img_metas"], depth=depth.to(device), ray_batch=rb)[0]
        res_defer = det.simple_test(batch["img"], batch["img_metas"], depth=depth.to(device), ray_batch=rb, defer=True)()[0]
        res_plain = det.simple_test(batch["img"], batch["img_metas"], ray_batch=rb)[0]
    f_host = x.float().cpu().contiguous()
    hf, wf = w["img_hw"][0] // 4, w["img_hw"][1] // 4
    gated, ungated, _, _ = gate_terms(out["points"].cpu(), out["projection"].cpu(), hf, wf, depth[0], list(w["voxel_size"]))
    assert torch.equal(out["valid"].cpu().reshape(-1), gated.sum(0))
    assert int(gated.sum()) < int(ungated.sum()) and int((gated.sum(0) > 0).sum()) > 1000
    with torch.no_grad():
        ov = oracle_extract_volume(monkeypatch, depth[0], list(w["voxel_size"]), f_host, batch_cpu["denorm_images"][0], meta, w["n_voxels"],
                                   w["voxel_size"], det_cpu.mapping[0].weight, det_cpu.mapping[0].bias, det_cpu.nerf_mlp.state_dict())
    assert torch.equal(out["valid"].cpu(), ov["valid"])
    scale = max(1.0, float(ov["volume"].abs().max()))
    err = float((out["volume"].cpu() - ov["volume"]).abs().max())
    assert err <= 1e-4 * scale, f"gated voxel features differ from the oracle by {err}"
    same_in = O.head_get_bboxes([t.cpu() for t in ctr], [t.cpu() for t in reg], [t.cpu() for t in cls], out["valid"].cpu().unsqueeze(0).float(),
                                meta["lidar2img"]["origin"], w["voxel_size"], tc.nms_pre, tc.score_thr, tc.iou_thr)
    assert len(same_in["labels"]) > 0
    assert torch.equal(res["labels_3d"], same_in["labels"])
    got = res["boxes_3d"].tensor[:, :6].clone()
    got[:, 2] += got[:, 5] * 0.5
    torch.testing.assert_close(got, same_in["boxes"], rtol=1e-4, atol=1e-4)
    assert torch.equal(res_defer["labels_3d"], res["labels_3d"]) and torch.equal(res_defer["boxes_3d"].tensor, res["boxes_3d"].tensor)
    assert not (torch.equal(res_plain["labels_3d"], res["labels_3d"]) and torch.equal(res_plain["boxes_3d"].tensor, res["boxes_3d"].tensor))
