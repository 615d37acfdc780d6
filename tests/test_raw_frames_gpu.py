"""k_resize_normalize_views (csrc/frame_kernels.hip) and what stands on it -- pipeline.prepare_frames, MultiViewPipeline(img_scale=, pad_size=),
SceneStream.add_frames, SceneGroup.add_frames -- against the numpy oracle of tests/raw_frames_ref.py: the datasets chain
imresize_linear -> imnormalize -> zero pad -> imdenormalize_u8 / 255 from frames at capture resolution.

Kernel sizes (capture, img_scale (32, 24), resized, pad (24, 32)):
  37 x 53   -> 22 x 32   downscale, a pad row at the bottom
  100 x 129 -> 24 x 31   a pad column on the right
  19 x 23   -> 24 x 29   UPSCALE: the low and the high border clamp fire on both axes; pad columns
  24 x 32   -> 24 x 32   the copy
  97 x 131  -> 24 x 32   a non-integer reduction of about 4, no pad
and one pair of 968 x 1296 frames -> 239 x 320 in 240 x 320, the real tap table.  Frames are those of tests/test_pipeline_edges_gpu.py (random
bytes plus a ramp through every byte value per channel), 14 of them; the four mean / std sets are that test's.  Every byte and every float is
compared, after the outputs were pre-filled with NaN / 0xFF; tests/test_raw_frames_cpu.py shows that a floating-point interpolation differs
from the host function on every non-copy size, and the count is asserted again here."""
import os

import numpy as np
import pytest
import torch

import raw_frames_ref as R
from test_pipeline_edges_gpu import GOLDEN, MEAN_STD, _frames

pytestmark = pytest.mark.gpu

IDS = {"descending-with-repeats": [13, 13, 9, 9, 4, 2, 2, 0], "null": None}
_cache = {}


def _ref(size_key, norm, ids_key):
    """The oracle of one case, computed once (read-only afterwards)."""
    key = (size_key, norm, ids_key)
    if key not in _cache:
        size, scale, _, pad = R.SIZES[size_key]
        _cache[key] = R.prepare(_frames(size), scale, pad, *MEAN_STD[norm], ids=IDS[ids_key])
    return _cache[key]


def _launch(frames_d, ids, hr, wr, h, w, mean, std, with_u8=True):
    """ndet_resize_normalize_views on pre-filled outputs: NaN in the float planes, 0xFF in the bytes."""
    from ctypes import c_void_p
    from nerfdet_amd import _lib
    dev = frames_d.device
    n_sel = frames_d.shape[0] if ids is None else len(ids)
    ids_d = None if ids is None else torch.tensor(ids, dtype=torch.int32, device=dev)
    img = torch.full((n_sel, 3, h, w), float("nan"), device=dev)
    dn = torch.full_like(img, float("nan"))
    u8 = torch.full((n_sel, h, w, 3), 255, dtype=torch.uint8, device=dev) if with_u8 else None
    mean, std = np.asarray(mean, np.float64), np.asarray(std, np.float64)
    _lib.check(_lib.load().ndet_resize_normalize_views(_lib._ptr(frames_d), _lib._ptr(ids_d), n_sel, frames_d.shape[1], frames_d.shape[2], hr, wr,
                                                       h, w, mean.ctypes.data_as(c_void_p), std.ctypes.data_as(c_void_p), _lib._ptr(img),
                                                       _lib._ptr(dn), _lib._ptr(u8), c_void_p(_lib.raw_stream(dev))), "resize_normalize_views")
    torch.cuda.synchronize()
    return img, dn, u8


def _normalize_views(u8_d, mean, std):
    """The existing kernel on already resized bytes: what the content region must equal."""
    from ctypes import c_void_p
    from nerfdet_amd import _lib
    n, h, w, _ = u8_d.shape
    ids_d = torch.arange(n, dtype=torch.int32, device=u8_d.device)
    img = torch.empty((n, 3, h, w), device=u8_d.device)
    dn = torch.empty_like(img)
    mean, std = np.asarray(mean, np.float64), np.asarray(std, np.float64)
    _lib.check(_lib.load().ndet_normalize_views(_lib._ptr(u8_d), _lib._ptr(ids_d), n, h, w, mean.ctypes.data_as(c_void_p), std.ctypes.data_as(c_void_p),
                                                _lib._ptr(img), _lib._ptr(dn), c_void_p(_lib.raw_stream(u8_d.device))), "normalize_views")
    return img, dn


def _assert_case(got, ref, hr, wr, mean, std, what):
    img, dn, u8 = got
    assert torch.equal(u8.cpu(), torch.from_numpy(ref["u8"])), f"{what}: resized bytes differ from imresize_linear"
    assert torch.equal(img.cpu(), torch.from_numpy(ref["img"])), f"{what}: img"
    assert torch.equal(dn.cpu(), torch.from_numpy(ref["denorm"])), f"{what}: denorm"
    # content region: ndet_normalize_views on the resized bytes
    want_img, want_dn = _normalize_views(u8[:, :hr, :wr].contiguous(), mean, std)
    assert torch.equal(img[:, :, :hr, :wr], want_img) and torch.equal(dn[:, :, :hr, :wr], want_dn), f"{what}: content vs k_normalize_views"
    # pad region: exactly 0.0 and trunc(mean) / 255 per BGR plane, zero bytes
    pad = torch.ones(img.shape[2:], dtype=torch.bool, device=img.device)
    pad[:hr, :wr] = False
    if bool(pad.any()):
        assert bool((img[:, :, pad] == 0.0).all()) and not bool(torch.signbit(img[:, :, pad]).any()) and not bool(u8[:, pad].any())
        for plane, c in enumerate((2, 1, 0)):      # BGR plane <- RGB mean
            want = np.float32(np.float32(mean[c]).astype(np.uint8)) / np.float32(255.0)
            assert bool((dn[:, plane][:, pad] == float(want)).all()), (what, plane)


@pytest.mark.parametrize("ids_key", list(IDS))
@pytest.mark.parametrize("norm", list(MEAN_STD))
@pytest.mark.parametrize("size_key", list(R.SIZES))
def test_kernel_matches_the_host_chain_in_every_byte(device, size_key, norm, ids_key):
    from nerfdet_amd.datasets import imresize_linear
    size, scale, (hr, wr), (h, w) = R.SIZES[size_key]
    mean, std = MEAN_STD[norm]
    frames = _frames(size)
    # the test is not blind: a float64 bilinear resize with round-to-nearest differs from the host function on this size
    blind = int((R.float_bilinear(frames[0], (wr, hr)) != imresize_linear(frames[0], (wr, hr))).sum())
    assert (blind > 0) == ("copy" not in size_key), (size_key, blind)
    ref = _ref(size_key, norm, ids_key)
    assert ref["resized_hw"] == (hr, wr)
    if "upscale" in size_key:          # both clamps fire on both axes: the first and the last output rows / columns copy a border source line
        assert np.array_equal(ref["u8"][0, 0, :wr][[0, -1]], frames[(IDS[ids_key] or [0])[0], 0][[0, -1]])
        assert np.array_equal(ref["u8"][0, hr - 1, :wr][[0, -1]], frames[(IDS[ids_key] or [0])[0], -1][[0, -1]])
    got = _launch(torch.from_numpy(frames).to(device), IDS[ids_key], hr, wr, h, w, mean, std)
    _assert_case(got, ref, hr, wr, mean, std, f"{size_key} {norm} ids={ids_key}")


def test_capture_size_frames(device):
    """Two frames of 968 x 1296 -> 239 x 320 in 240 x 320 (cfg2's ScanNet case): the real tap table, 29 386 bytes of frame 0 where a float
    bilinear resize is one grey level off, the pad row, and without the byte output."""
    from nerfdet_amd import pipeline as P
    from nerfdet_amd.datasets import imresize_linear
    frames = np.random.RandomState(1).randint(0, 256, (2, 968, 1296, 3)).astype(np.uint8)
    assert P.rescale_size((968, 1296), (320, 240)) == (239, 320)
    assert int((R.float_bilinear(frames[0], (320, 239)) != imresize_linear(frames[0], (320, 239))).sum()) > 0
    mean, std = MEAN_STD["default"]
    ref = R.prepare(frames, (320, 240), (240, 320), mean, std)
    fd = torch.from_numpy(frames).to(device)
    _assert_case(_launch(fd, None, 239, 320, 240, 320, mean, std), ref, 239, 320, mean, std, "968x1296")
    img, dn, none = _launch(fd, [1, 0], 239, 320, 240, 320, mean, std, with_u8=False)
    assert none is None and torch.equal(img.cpu(), torch.from_numpy(ref["img"][::-1].copy())) and torch.equal(dn.cpu(), torch.from_numpy(ref["denorm"][::-1].copy()))
    # the public wrapper makes the same launch
    a, b, c = P.prepare_frames(fd, (320, 240), (240, 320), want_u8=True)
    assert torch.equal(a.cpu(), torch.from_numpy(ref["img"])) and torch.equal(b.cpu(), torch.from_numpy(ref["denorm"])) and torch.equal(c.cpu(), torch.from_numpy(ref["u8"]))
    a2, b2 = P.prepare_frames(fd, (320, 240), (240, 320), ids=[1, 1])
    assert torch.equal(a2[0], a[1]) and torch.equal(b2[1], b[1])
    with pytest.raises(ValueError, match="does not fit"):
        P.prepare_frames(fd.transpose(1, 2).contiguous(), (320, 240), (240, 320))


# ---- MultiViewPipeline(img_scale=, pad_size=) ----
@pytest.fixture(scope="module")
def g():
    z = np.load(os.path.join(GOLDEN, "pipeline_small.npz"))
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("margin", [0, 3])
@pytest.mark.parametrize("norm", ["default", "spread"])
def test_raw_pipeline_matches_the_datasets_chain(device, g, norm, margin):
    """37 x 53 raw frames -> 22 x 32 in 24 x 32.  With margin 0 the targets' rays reach the two pad rows, where gt_images is trunc(mean) / 255."""
    from nerfdet_amd import pipeline as P
    from oracle import pipeline_oracle as O
    mean, std = MEAN_STD[norm]
    size, scale, (hr, wr), (h, w) = R.SIZES["37x53-down-bottom-pad"]
    ids, tids = [13, 13, 9, 9, 4, 2, 2, 0], [7, 13, 2]
    frames = _frames(size)
    info = dict(extrinsics=list(g["poses"]), intrinsics=g["intrinsic"], annos=dict(axis_align_matrix=g["axis_align"]))
    ref = R.batch(frames, O.scene_cameras(info), ids, tids, scale, (h, w), mean, std, margin)
    pipe = P.MultiViewPipeline(len(ids), mean=mean, std=std, margin=margin, nerf_target_views=len(tids), img_scale=scale, pad_size=(h, w))
    batch = pipe(torch.from_numpy(frames).to(device), P.scene_cameras(info), None, ids=ids, target_ids=tids)
    torch.cuda.synchronize()
    meta = batch["img_metas"][0]
    assert (meta["ori_shape"], meta["img_shape"], meta["pad_shape"]) == ((37, 53, 3), (22, 32, 3), (24, 32, 3))
    rays = (h - 2 * margin) * (w - 2 * margin)
    assert batch["img"].shape == (1, len(ids), 3, h, w) and batch["raydirs"].shape == (1, len(tids), rays, 3)
    assert torch.equal(batch["img"][0].cpu(), torch.from_numpy(ref["img"]))
    assert torch.equal(batch["denorm_images"][0].cpu(), torch.from_numpy(ref["denorm_images"]))
    assert torch.equal(batch["lightpos"][0].cpu(), torch.from_numpy(ref["lightpos"]))
    assert np.array_equal(np.stack(meta["lidar2img"]["extrinsic"]), ref["extrinsic"])
    gt = batch["gt_images"][0].cpu().double().numpy()
    assert gt.shape == ref["gt_images"].shape and np.abs(gt - ref["gt_images"]).max() <= 1e-7          # the oracle keeps float64 here
    rd = batch["raydirs"][0].cpu().numpy()
    assert np.abs(rd - ref["raydirs"]).max() <= 2e-7 * max(1.0, np.abs(ref["raydirs"]).max())
    assert [tuple(s[0].tolist()) for s in batch["nerf_sizes"]] == [tuple(r) for r in ref["nerf_sizes"]] == [(h - 2 * margin, w - 2 * margin, 3)] * len(tids)
    if margin == 0:     # the last two grid rows are pad: trunc(mean) / 255 in BGR order
        want = np.float32(mean).astype(np.uint8)[::-1] / 255.0
        assert np.array_equal(ref["gt_images"][:, hr * w:], np.broadcast_to(want, (len(tids), (h - hr) * w, 3)))
    with pytest.raises(ValueError, match="ori_shape"):
        pipe(torch.from_numpy(frames).to(device), P.scene_cameras(info), (74, 106, 3), ids=ids, target_ids=tids)


# ---- streaming ----
RAW, SCALE, PAD = (128, 194), (96, 64), (64, 96)        # -> 63 x 96: a pad row, and a feature map cropped to 15 rows
STATE = ("k1_sum", "k1_count", "k2_sum", "k2_count")


def _raw_scene(device, seed, n_v=6, turn=0):
    """Raw frames (1, n_v, 128, 194, 3), the scene's meta (the ring cameras' overwritten with frame_meta) and the oracle's img / denorm."""
    from nerfdet_amd import pipeline as P
    from oracle import nerfdet_oracle as O
    frames = np.random.RandomState(seed).randint(0, 256, (n_v,) + RAW + (3,)).astype(np.uint8)
    ring = O.ring_scene_meta(n_v, PAD)["lidar2img"]
    ring["extrinsic"] = ring["extrinsic"][turn:] + ring["extrinsic"][:turn]
    ring["origin"] = np.asarray(ring["origin"], np.float32) + np.float32([0.2 * turn, -0.1 * turn, 0.0])
    meta = P.frame_meta(ring, RAW, SCALE, PAD)
    assert (meta["ori_shape"], meta["img_shape"], meta["pad_shape"]) == ((128, 194, 3), (63, 96, 3), (64, 96, 3))
    ref = R.prepare(frames, SCALE, PAD, P.IMG_MEAN, P.IMG_STD)
    return (torch.from_numpy(frames).to(device).unsqueeze(0), meta, torch.from_numpy(ref["img"]).to(device).unsqueeze(0),
            torch.from_numpy(ref["denorm"]).to(device).unsqueeze(0))


def _states_equal(a, b):
    return all(torch.equal(getattr(a, t), getattr(b, t)) for t in STATE)


def _rays64(device):
    gen = torch.Generator().manual_seed(11)
    ang = torch.rand(64, generator=gen) * 6.2831853
    ray_o = torch.stack([2.0 * torch.cos(ang), 2.0 * torch.sin(ang), 1.0 + 0.3 * torch.rand(64, generator=gen)], -1)
    ray_d = -ray_o / ray_o.norm(dim=-1, keepdim=True) + 0.35 * torch.randn(64, 3, generator=gen)
    return ray_o.to(device), ray_d.to(device)


@pytest.mark.parametrize("keep_views", [False, True])
def test_stream_add_frames_is_add_views_on_the_oracles_tensors(device, keep_views):
    from test_detector_gpu import _small_detector
    from test_streaming_gpu import _chunk_meta, _same
    det = _small_detector(device)
    frames, meta, img, dn = _raw_scene(device, 21)
    a, b = det.begin_scene(dict(meta), keep_views=keep_views), det.begin_scene(dict(meta), keep_views=keep_views)
    for v0, v1 in ((0, 4), (4, 6)):
        a.add_frames(frames[:, v0:v1], _chunk_meta(meta, v0, v1))
        b.add_views(img[:, v0:v1], dn[:, v0:v1], _chunk_meta(meta, v0, v1))
    assert a.n_views == b.n_views == 6 and _states_equal(a.state, b.state)
    assert int(a.state.k1_count.sum()) > 0
    _same(a.detect(), b.detect())
    if keep_views:
        ray_o, ray_d = _rays64(device)
        ra, rb = a.render_rays(ray_o, ray_d), b.render_rays(ray_o, ray_d)
        assert bool(ra["mask"].any()) and all(torch.equal(ra[k], rb[k]) for k in ("rgb", "depth", "mask"))
    # a refused call (frames one row short) changes nothing
    keep = [getattr(a.state, t).clone() for t in STATE]
    with pytest.raises(ValueError, match="ori_shape"):
        a.add_frames(frames[:, :2, :127].contiguous(), _chunk_meta(meta, 0, 2))
    assert a.n_views == 6 and all(torch.equal(getattr(a.state, t), k) for t, k in zip(STATE, keep))


def test_stream_add_frames_takes_the_scenes_mean_and_std(device):
    from nerfdet_amd import pipeline as P
    from test_detector_gpu import _small_detector
    from test_streaming_gpu import _chunk_meta
    det = _small_detector(device)
    frames, meta, _, _ = _raw_scene(device, 22, n_v=2)
    mean, std = MEAN_STD["spread"]
    ref = R.prepare(frames[0].cpu().numpy(), SCALE, PAD, mean, std)
    a, b = det.begin_scene(dict(meta), mean=mean, std=std), det.begin_scene(dict(meta))
    a.add_frames(frames, _chunk_meta(meta, 0, 2))
    b.add_views(torch.from_numpy(ref["img"]).to(device).unsqueeze(0), torch.from_numpy(ref["denorm"]).to(device).unsqueeze(0), _chunk_meta(meta, 0, 2))
    assert a.mean == tuple(mean) and b.mean == tuple(P.IMG_MEAN) and _states_equal(a.state, b.state)


@pytest.mark.parametrize("keep_views", [False, True])
def test_group_add_frames_is_add_views_on_the_oracles_tensors(device, keep_views):
    """Three scenes, one call for all of them (4 views each) and a subset call scenes=[2, 0] (2 views each).  The group fed raw frames holds
    the bits of a group fed the oracle's tensors by the same calls.  Against per-scene streams fed raw frames it holds what a group promises
    against streams (SceneGroup: the scenes of a call share the backbone's fp16-pair scales): the counts exactly, detections to 1e-4."""
    from test_detector_gpu import _small_detector
    from test_streaming_gpu import _chunk_meta, _close, _same
    det = _small_detector(device)
    sc = [_raw_scene(device, 30 + i, turn=i) for i in range(3)]
    metas = [dict(s[1]) for s in sc]
    a, b = det.begin_scenes(metas, keep_views=keep_views), det.begin_scenes(metas, keep_views=keep_views)
    streams = [det.begin_scene(dict(m), keep_views=keep_views) for m in metas]
    for rows, v0, v1 in (([0, 1, 2], 0, 4), ([2, 0], 4, 6)):
        chunk = [_chunk_meta(sc[s][1], v0, v1) for s in rows]
        a.add_frames(torch.cat([sc[s][0][:, v0:v1] for s in rows]), chunk, scenes=rows)
        b.add_views(torch.cat([sc[s][2][:, v0:v1] for s in rows]), torch.cat([sc[s][3][:, v0:v1] for s in rows]), chunk, scenes=rows)
        for s in rows:
            streams[s].add_frames(sc[s][0][:, v0:v1], _chunk_meta(sc[s][1], v0, v1))
    assert a.n_views == b.n_views == [6, 4, 6] == [s.n_views for s in streams]
    for sa, sb, st in zip(a.group.states, b.group.states, streams):
        assert _states_equal(sa, sb)
        assert torch.equal(sa.k1_count, st.state.k1_count) and torch.equal(sa.k2_count, st.state.k2_count)
    got, want = a.detect(), b.detect()
    for s in range(3):
        _same(got[s], want[s])
        _close(got[s], streams[s].detect())
    if keep_views:
        ray_o, ray_d = _rays64(device)
        ra, rb = a.render_rays([ray_o] * 3, [ray_d] * 3), b.render_rays([ray_o] * 3, [ray_d] * 3)
        for x, y in zip(ra, rb):
            assert all(torch.equal(x[k], y[k]) for k in ("rgb", "depth", "mask"))
    keep = [[getattr(st, t).clone() for t in STATE] for st in a.group.states]
    with pytest.raises(ValueError, match="ori_shape"):
        a.add_frames(torch.cat([sc[s][0][:, :2, :127] for s in (2, 0)]).contiguous(), [_chunk_meta(sc[s][1], 0, 2) for s in (2, 0)], scenes=[2, 0])
    assert a.n_views == [6, 4, 6]
    assert all(torch.equal(getattr(st, t), k) for st, ks in zip(a.group.states, keep) for t, k in zip(STATE, ks))
