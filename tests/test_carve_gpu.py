"""GPU checks of space carving from depth frames (csrc/carve_kernels.hip, ops.carve_accumulate / carve_bits, rays.CarveStore,
``begin_scene(carve=)``, ``occupancy(source=)``, ``skip_empty=dict(source="depth")``): counters and bits against the numpy restatement
(tests/carve_ref.py) byte for byte, the store following streams, windows and groups, and renders through a carved fine grid against the
public pieces with the culled rows zeroed."""
import itertools

import numpy as np
import pytest
import torch

import carve_ref as C
import skip_empty_ref as R

pytestmark = pytest.mark.gpu

_CACHE = {}


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _gate(depth, band=C.BAND):
    from nerfdet_amd import ops
    return ops.DepthGate(depth, depth, band)


def _case(nv, refine, k, dtype):
    """Fine points, projections, depth maps and the restated words of one chunk over zeroed counters; made once (the projected
    coordinates once for both dtypes: the maps differ by their dtype alone)."""
    key = ("case", nv, refine, k, np.dtype(dtype).name)
    if key not in _CACHE:
        pts = C.fine_points(nv, refine)
        proj, depth = C.views_case(nv, k, dtype)
        pkey = ("projected", nv, refine, k)
        projected = _CACHE.pop(pkey, None)
        if projected is None:
            projected = _CACHE[pkey] = C.project(pts, proj)
        want = C.accumulate(np.zeros(pts[0].numel(), dtype=np.int32), pts, proj, depth, C.BAND, C.HW, projected)
        _CACHE[key] = (pts, proj, depth, want)
    return _CACHE[key]


# ---- counters ----
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("k", [1, 3, 65])
@pytest.mark.parametrize("refine", [1, 2, 4])
@pytest.mark.parametrize("nv", [(5, 3, 7), (8, 8, 40)])
def test_counters_equal_the_restatement(device, nv, refine, k, dtype):
    """Holes, a negative and a NaN depth, points outside the image and behind a camera, camera depths exactly on d - band and d + band
    (tests/test_carve_cpu.py checks that the shared inputs hold them all); a contiguous and a view-pitched map; a second call."""
    from nerfdet_amd import ops
    pts, proj, depth, want = _case(nv, refine, k, dtype)
    fine = tuple(refine * v for v in nv)
    n = fine[0] * fine[1] * fine[2]
    dev_pts = ops.get_points(fine, [v / refine for v in C.VS], C.ORIGIN, device)
    assert torch.equal(dev_pts.cpu(), pts)                                      # the lattice itself, bit for bit
    d = _dev(depth, device)
    pitched = torch.full((k, C.HW[0] + 3, C.HW[1] + 5), 7.0, dtype=d.dtype, device=device)
    pitched[:, :C.HW[0], :C.HW[1]] = d
    pitched = pitched[:, :C.HW[0], :C.HW[1]]
    assert not pitched.is_contiguous()
    for m in (d, pitched, d):
        counts = torch.zeros((n,), dtype=torch.int32, device=device)
        out = ops.carve_accumulate(counts, dev_pts, proj.to(device), _gate(m))
        assert out is counts
        assert np.array_equal(counts.cpu().numpy(), want), f"{nv} r{refine} k{k} {np.dtype(dtype).name}"
    free, hit = C.unpack(want)
    assert free.any() and (hit.any() or k == 1)
    print(f"{nv} r{refine} k{k} {np.dtype(dtype).name}: free in {int((free > 0).sum())}, hit in {int((hit > 0).sum())} of {n} voxels")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_counters_saturate(device, dtype):
    from nerfdet_amd import ops
    nv, refine = (5, 3, 7), 2
    pts, proj, depth, _ = _case(nv, refine, 3, dtype)
    n = pts[0].numel()
    rng = np.random.RandomState(2)
    start = C.pack(rng.choice([0, 65534, 65535], n), rng.choice([65533, 65534, 65535], n))
    want = C.accumulate(start, pts, proj, depth, C.BAND, C.HW)
    f0, h0 = C.unpack(start)
    f1, h1 = C.unpack(want)
    assert ((f0 == 65534) & (f1 == 65535)).any() and ((f0 + C.evidence(pts, proj, depth, C.BAND, C.HW)[0].sum(0)) > 65535).any()
    assert f1.max() == 65535 and h1.max() == 65535
    counts = _dev(start, device)
    ops.carve_accumulate(counts, pts.to(device), proj.to(device), _gate(_dev(depth, device)))
    assert np.array_equal(counts.cpu().numpy(), want)


def test_any_chunking_leaves_the_same_bytes(device):
    from nerfdet_amd import ops
    nv, refine = (8, 8, 40), 2
    pts = C.fine_points(nv, refine)
    proj, depth = C.views_case(nv, 6, np.float64)
    n = pts[0].numel()
    dp, dproj, dd = pts.to(device), proj.to(device), _dev(depth, device)
    got = []
    for sizes in ([6], [2, 4], [1] * 6):
        counts, v = torch.zeros((n,), dtype=torch.int32, device=device), 0
        for s in sizes:
            ops.carve_accumulate(counts, dp, dproj[v:v + s], _gate(dd[v:v + s]))
            v += s
        got.append(counts)
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])
    assert np.array_equal(got[0].cpu().numpy(), C.accumulate(np.zeros(n, dtype=np.int32), pts, proj, depth, C.BAND, C.HW))


# ---- bits ----
BITS_LATTICES = {   # name -> (fine n_voxels, refine of the coarse grid, segment counts)
    "ragged": ((5, 3, 7), 1, (1, 2, 64)),             # 105 voxels: a ragged last word
    "z_word": ((6, 4, 40), 2, (1, 2, 64)),            # Z crosses a word boundary
    "global": ((128, 128, 64), 4, (1, 2)),            # 128 KiB of bits: beyond the cull kernels' LDS staging
}


@pytest.mark.parametrize("name", list(BITS_LATTICES))
def test_bits_equal_the_restatement(device, name):
    from nerfdet_amd import ops
    nv, r, seg_counts = BITS_LATTICES[name]
    n = nv[0] * nv[1] * nv[2]
    assert (4 * ((n + 31) // 32) > 64 * 1024) == (name == "global")
    coarse = R.pack_bits(np.random.RandomState(9).rand(n // r ** 3) < 0.7)
    dev_coarse = _dev(coarse, device)
    knobs = list(itertools.product((1, 2, 3), (0, 1, 2), (False, True)))
    if name == "global":
        knobs = [(1, 0, False), (2, 1, True), (3, 2, False), (2, 2, True)]
    fracs = []
    for n_segs in seg_counts:
        segs = C.segments_case(n, n_segs, seed=n_segs)
        dev_segs = [_dev(s, device) for s in segs]
        for min_free, dilate, with_coarse in knobs:
            want = C.bits(segs, nv, min_free, dilate, coarse if with_coarse else None, r)
            args = (dev_segs, nv, min_free, dilate, dev_coarse if with_coarse else None, r)
            got = ops.carve_bits(*args)
            assert got.dtype == torch.int32 and tuple(got.shape) == ((n + 31) // 32,)
            assert np.array_equal(got.cpu().numpy(), want), f"{name} segs {n_segs} min_free {min_free} dilate {dilate} coarse {with_coarse}"
            assert torch.equal(ops.carve_bits(*args), got), "a second call gives other bytes"
            for two in (False, True):                                      # both forms of the kernel
                assert torch.equal(ops.carve_bits(*args, two_pass=two), got), f"two_pass={two}"
            fracs.append(np.unpackbits(want.view(np.uint8)).sum() / n)
    print(f"{name}: {min(fracs):.4f} .. {max(fracs):.4f} of the bits set")
    assert 0 < min(fracs) < 0.9


# ---- streams and groups ----
def _carved(device):
    """_small_detector, synth.train_scene(6, (64, 96)) and a float64 floor-plane depth map per view with 5 % holes; made once."""
    key = ("carved", str(device))
    if key not in _CACHE:
        from depth_gate_ref import plane_depth
        from test_stream_render_gpu import _det_and_scene
        det, img, dn, meta, rb = _det_and_scene(device)
        depth = plane_depth(meta, (64, 96), 0.0, noise=0.01, seed=3, missing=0.05).unsqueeze(0).to(device)
        _CACHE[key] = dict(det=det, img=img, dn=dn, meta=meta, depth=depth, ray_o=rb["ray_o"].view(-1, 3).contiguous(),
                           ray_d=rb["ray_d"].view(-1, 3).contiguous())
    return _CACHE[key]


def _feed(scene, c, splits, depth=True):
    from test_stream_render_gpu import _chunk_meta
    for v0, v1 in splits:
        scene.add_views(c["img"][:, v0:v1], c["dn"][:, v0:v1], _chunk_meta(c["meta"], v0, v1), depth=c["depth"][:, v0:v1] if depth else None)
    return scene


def _same_counts(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


KNOBS = dict(dilate=1, outside="cull", source="depth")


def test_scene_counts_equal_the_restatement(device):
    """The road from add_views to the store: the counts of an unwindowed scene fed [2, 1, 3] are the restatement's over the gate's own
    image-resolution map and the stride-1 projection, at refine 2 and the default band voxel_size[2]."""
    from nerfdet_amd import ops
    c = _carved(device)
    det = c["det"]
    scene = _feed(det.begin_scene(dict(c["meta"]), carve=True), c, [(0, 2), (2, 3), (3, 6)])
    assert scene.carve.refine == 2 and scene.carve.band == float(det.voxel_size[2]) and len(scene.carve.store.segments) == 1
    free, hit = scene.carve_counts()
    fine = tuple(2 * int(v) for v in det.n_voxels)
    assert tuple(free.shape) == fine and free.dtype == torch.int32 and hit.dtype == torch.int32
    gate = ops.depth_gate(c["depth"][0], det.voxel_size, (16, 24), (64, 96))
    pts = scene.carve.points.cpu()
    want = C.accumulate(np.zeros(pts[0].numel(), dtype=np.int32), pts, ops.compute_projection(c["meta"], 1), gate.depth_r.cpu().numpy(),
                        float(det.voxel_size[2]), (64, 96))
    wf, wh = C.unpack(want)
    assert np.array_equal(free.cpu().numpy().reshape(-1), wf) and np.array_equal(hit.cpu().numpy().reshape(-1), wh)
    print(f"free in {int((wf > 0).sum())}, hit in {int((wh > 0).sum())}, empty {(int(((wf >= 2) & (wh == 0)).sum()))} of {wf.size} fine voxels")
    assert (wf >= 2).any() and (wh > 0).any()
    occ = scene.occupancy(**KNOBS)
    assert occ.n_voxels == fine and scene.occupancy(**KNOBS) is occ and scene.occupancy(min_free=3, **KNOBS) is not occ
    assert np.array_equal(occ.bits.cpu().numpy(), C.bits([want], fine, 2, 1))
    assert occ.p0 == tuple(float(v) for v in pts[:, 0, 0, 0]) and occ.voxel_size == tuple(float(np.float32(v) / np.float32(2)) for v in det.voxel_size)
    # "both": carve-solid AND the parent's bit of the undilated alpha grid
    alpha, _, valid = scene._finish()
    thr = float(torch.quantile(alpha, 0.5, interpolation="lower"))
    coarse = R.occupancy_bits(alpha.cpu().numpy(), valid.cpu().numpy(), det.n_voxels, np.float32(thr), 0)
    both = scene.occupancy(thr, 1, "cull", source="both")
    assert np.array_equal(both.bits.cpu().numpy(), C.bits([want], fine, 2, 1, coarse, 2))
    assert not torch.equal(both.bits, occ.bits)


def test_a_window_follows_the_chunks(device):
    """S + 2 chunks through a window of S = 2 leave what a fresh stream fed the last S holds; drop_oldest and reset leave no trace; a chunk
    without depth adds a segment without evidence; a refused call changes nothing."""
    from test_stream_render_gpu import _chunk_meta
    c = _carved(device)
    det = c["det"]
    begin = lambda: det.begin_scene(dict(c["meta"]), window=2, carve=dict(refine=2))
    scene = _feed(begin(), c, [(0, 2), (2, 3), (3, 5), (5, 6)])
    fresh = _feed(begin(), c, [(3, 5), (5, 6)])
    assert len(scene.carve.store.segments) == 2 == scene.n_chunks
    assert _same_counts(scene.carve_counts(), fresh.carve_counts()) and int(scene.carve_counts()[0].sum()) > 0
    assert torch.equal(scene.occupancy(**KNOBS).bits, fresh.occupancy(**KNOBS).bits)
    owned = scene.carve.store.nbytes()
    before = scene.occupancy(**KNOBS)
    counts = scene.carve_counts()
    with pytest.raises(ValueError):
        scene.add_views(c["img"][:, 0:2], c["dn"][:, 0:2], _chunk_meta(c["meta"], 0, 3), depth=c["depth"][:, 0:2])     # 3 extrinsics for 2 views
    assert _same_counts(scene.carve_counts(), counts) and scene.occupancy(**KNOBS) is before and len(scene.carve.store.segments) == 2
    scene.drop_oldest(1)
    only = _feed(begin(), c, [(5, 6)])
    assert scene.occupancy(**KNOBS) is not before
    assert _same_counts(scene.carve_counts(), only.carve_counts()) and torch.equal(scene.occupancy(**KNOBS).bits, only.occupancy(**KNOBS).bits)
    _feed(scene, c, [(0, 2)], depth=False)                                      # no depth: a segment without evidence
    assert len(scene.carve.store.segments) == 2 and not scene.carve.store.segments[-1].any()
    assert _same_counts(scene.carve_counts(), only.carve_counts())
    _feed(scene, c, [(2, 3)])                                                   # evicts (5, 6)
    assert scene.carve.store.nbytes() == owned                                 # a window that has slid allocates nothing
    scene.reset()
    assert scene.carve.store.segments == [] and not scene.carve_counts()[0].any() and not scene.carve_counts()[1].any()
    _feed(scene, c, [(3, 5), (5, 6)])
    assert _same_counts(scene.carve_counts(), fresh.carve_counts())
    # an unwindowed scene: reset leaves no trace either
    plain = _feed(det.begin_scene(dict(c["meta"]), carve=True), c, [(0, 3)])
    plain.reset()
    _feed(plain, c, [(3, 5), (5, 6)])
    assert _same_counts(plain.carve_counts(), fresh.carve_counts())


def test_without_carve_nothing_changes(device):
    """carve=None: no k_carve_* launch and the scene state of a carved stream bit for bit; sources that need a carve are refused."""
    from nerfdet_amd import trace
    c = _carved(device)
    det = c["det"]
    trace.recorder = trace.Recorder()
    try:
        plain = _feed(det.begin_scene(dict(c["meta"])), c, [(0, 2), (2, 6)])
        names_plain = {s[0] for s in trace.recorder.spans}
        trace.recorder = trace.Recorder()
        carved = _feed(det.begin_scene(dict(c["meta"]), carve=True), c, [(0, 2), (2, 6)])
        spans = [s for s in trace.recorder.spans if s[0].startswith("k_carve")]
        names_carved = {s[0] for s in trace.recorder.spans}
        trace.recorder = trace.Recorder()
        carved.occupancy(**KNOBS)
        names_grid = [s[0] for s in trace.recorder.spans]
    finally:
        trace.recorder = None
    assert not any(n.startswith("k_carve") for n in names_plain) and plain.carve is None
    assert [s[0] for s in spans] == ["k_carve_accumulate"] * 2 and names_carved - {"k_carve_accumulate"} == names_plain
    assert names_grid == ["k_carve_bits"]                                       # source="depth" runs no finish and no MLP
    assert torch.equal(plain.state.k1_sum, carved.state.k1_sum) and torch.equal(plain.state.k2_sum, carved.state.k2_sum)
    assert torch.equal(plain.state.k1_count, carved.state.k1_count) and torch.equal(plain.state.k2_count, carved.state.k2_count)
    for source in ("depth", "both"):
        with pytest.raises(ValueError, match="carve"):
            plain.occupancy(source=source)
    with pytest.raises(ValueError, match="carve"):
        plain.carve_counts()
    for bad in (dict(refine=3), dict(band=0.0), 5):
        with pytest.raises(ValueError):
            det.begin_scene(dict(c["meta"]), carve=bad)
        with pytest.raises(ValueError):
            det.begin_scenes([dict(c["meta"])], carve=bad)


@pytest.mark.parametrize("window", [None, 2])
def test_a_group_of_one_scene_is_the_stream(device, window):
    from test_stream_render_gpu import _chunk_meta
    c = _carved(device)
    det = c["det"]
    splits = [(0, 2), (2, 3), (3, 5), (5, 6)]
    scene = _feed(det.begin_scene(dict(c["meta"]), window=window, carve=True), c, splits)
    group = det.begin_scenes([dict(c["meta"])], window=window, carve=True)
    for v0, v1 in splits:
        group.add_views(c["img"][:, v0:v1], c["dn"][:, v0:v1], [_chunk_meta(c["meta"], v0, v1)], depth=c["depth"][:, v0:v1])
    assert _same_counts(group.carve_counts()[0], scene.carve_counts()) and int(scene.carve_counts()[0].sum()) > 0
    assert len(group.carves[0].store.segments) == len(scene.carve.store.segments)
    for a, b in zip(group.carves[0].store.segments, scene.carve.store.segments):
        assert torch.equal(a, b)
    assert torch.equal(group.occupancy(**KNOBS)[0].bits, scene.occupancy(**KNOBS).bits)
    assert torch.equal(group.occupancy(0.01, 1, "cull", source="both")[0].bits, scene.occupancy(0.01, 1, "cull", source="both").bits)


def test_a_subset_call_touches_only_the_listed_scenes(device):
    from depth_gate_ref import plane_depth
    from test_group_render_gpu import _chunk_meta, _det_scenes
    det, scenes = _det_scenes(device)
    depth = [plane_depth(scenes[s]["meta"], (64, 96), 0.0, noise=0.01, seed=s, missing=0.05).unsqueeze(0).to(device) for s in (0, 1)]
    group = det.begin_scenes([dict(scenes[s]["meta"]) for s in (0, 1)], window=2, carve=True)

    def add(rows, a, b, with_depth=True):
        group.add_views(torch.cat([scenes[s]["img"][:, a:b] for s in rows]), torch.cat([scenes[s]["dn"][:, a:b] for s in rows]),
                        [_chunk_meta(scenes[s]["meta"], a, b) for s in rows], scenes=rows,
                        depth=torch.cat([depth[s][:, a:b] for s in rows]) if with_depth else None)

    add([0, 1], 0, 3)
    streams = []
    for s in (0, 1):
        st = det.begin_scene(dict(scenes[s]["meta"]), window=2, carve=True)
        st.add_views(scenes[s]["img"][:, 0:3], scenes[s]["dn"][:, 0:3], _chunk_meta(scenes[s]["meta"], 0, 3), depth=depth[s][:, 0:3])
        streams.append(st)
    for s in (0, 1):                       # the counters depend on the depth maps and cameras alone: each scene's are its stream's
        assert _same_counts(group.carve_counts()[s], streams[s].carve_counts())
    assert not _same_counts(group.carve_counts()[0], group.carve_counts()[1])
    grids = group.occupancy(**KNOBS)
    zero = group.carve_counts(scenes=[0])[0]
    add([1], 3, 6)
    assert _same_counts(group.carve_counts(scenes=[0])[0], zero) and len(group.carves[0].store.segments) == 1
    assert len(group.carves[1].store.segments) == 2
    after = group.occupancy(**KNOBS)
    assert after[0] is grids[0] and after[1] is not grids[1]
    streams[1].add_views(scenes[1]["img"][:, 3:6], scenes[1]["dn"][:, 3:6], _chunk_meta(scenes[1]["meta"], 3, 6), depth=depth[1][:, 3:6])
    assert _same_counts(group.carve_counts()[1], streams[1].carve_counts()) and torch.equal(after[1].bits, streams[1].occupancy(**KNOBS).bits)
    group.drop_oldest(1, scenes=[1])
    assert len(group.carves[1].store.segments) == 1 and len(group.carves[0].store.segments) == 1
    group.reset(scenes=[0])
    assert group.carves[0].store.segments == [] and len(group.carves[1].store.segments) == 1


# ---- renders through a carved fine grid ----
def test_renders_through_a_carved_grid(device):
    """An r = 2 carved grid: n_kept is the restated keep mask's count, the mask is the plain render's, rgb and depth are the plain pieces'
    with the culled rows zeroed, bit for bit; once more with early_stop=True on top.  One pass over the 6688 rays, which keeps 215 637 of
    428 032 rows.  Measured on an MI355X: every difference is 0.  The same rays in two passes of 4096 keep 132 292 and 83 345 rows, and
    then ``rgb`` differs from the plain pieces by 1.2e-7 (one unit in the last place, ``depth`` by 0) in the first pass: ``nerf_mlp``
    called on exactly 132 292 rows returns other last bits of ``rgb`` for the same rows than a call of 131 072, 147 456 or 262 144 rows
    does, whichever rows they are (the first 132 292 of the pass as well as the kept ones).  That is the radiance MLP's row-count
    dependence rays.mlp_rows_padded describes, at a size its measured range did not hold; it does not depend on where the grid comes
    from, and a culled pass pads nothing (streaming._culled_shade).  The test therefore fixes its pass and checks the count it relies
    on."""
    from nerfdet_amd import rays, streaming
    from test_early_stop_gpu import _expected as _expected_stopped
    from test_skip_empty_gpu import _close, _expected, _keep
    c = _carved(device)
    det = c["det"]
    assert c["ray_o"].shape[0] <= rays.RENDER_TESTING_RAYS
    scene = _feed(det.begin_scene(dict(c["meta"]), keep_views=True, carve=dict(refine=2)), c, [(0, 2), (2, 3), (3, 6)])
    occ = scene.occupancy(**KNOBS)
    assert occ.n_voxels == tuple(2 * int(v) for v in det.n_voxels)
    o, d = c["ray_o"], c["ray_d"]
    far = float(det.near_far_range[1])
    got = scene.render_rays(o, d, skip_empty=occ)
    want, kept = _expected(det, scene.bank, occ, o, d)
    plain = scene.render_rays(o, d)
    assert got["n_samples"] == o.shape[0] * det.N_samples and got["n_kept"] == kept
    print(f"kept {kept} of {got['n_samples']} samples ({kept / got['n_samples']:.4f}) through the carved grid")
    assert kept == 215637 < got["n_samples"], "another kept count: the nerf_mlp call's launches may be others (see above)"
    with torch.no_grad():
        keep = _keep(occ, rays.sample_along_camera_ray(o, d, det.near_far_range, det.N_samples, det=True)[0])
    assert int(keep.sum()) == kept
    print("kept rows per 4096 rays: " + ", ".join(str(int(k.sum())) for k in keep.view(-1, det.N_samples).split(4096)))
    assert torch.equal(got["mask"], plain["mask"]) and got["mask"].any()
    _close(got, want, far, "render through the carved grid")
    by_knobs = scene.render_rays(o, d, skip_empty=KNOBS)                          # the grid the scene makes itself
    for key in ("rgb", "depth", "mask"):
        assert torch.equal(by_knobs[key], got[key]), key
    assert by_knobs["n_kept"] == kept
    stop = dict(streaming.EARLY_STOP_DEFAULTS)
    got = scene.render_rays(o, d, skip_empty=occ, early_stop=True)
    want, _, _, kept_stopped = _expected_stopped(det, scene.bank, stop, occ, o, d)
    assert got["n_kept"] == kept_stopped <= kept and torch.equal(got["mask"], plain["mask"])
    _close(got, want, far, "stopped render through the carved grid")
    with pytest.raises(ValueError, match="carve"):
        _feed(det.begin_scene(dict(c["meta"]), keep_views=True), c, [(0, 2)]).render_rays(o[:64], d[:64], skip_empty=KNOBS)
