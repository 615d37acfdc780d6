"""The NV12 kernels (csrc/nv12_frames_kernels.hip) and what stands on them -- pipeline.prepare_frames(format="nv12"), pipeline.nv12_to_bgr,
pipeline.bgr_to_nv12, MultiViewPipeline(frame_format="nv12"), SceneStream / SceneGroup.add_frames(format="nv12") and
score_frames(format="nv12") -- against the numpy oracle of tests/nv12_ref.py: the datasets chain of tests/raw_frames_ref.py on
datasets.nv12_to_bgr of each surface, and against the BGR entry points run on the uploaded host-converted frames.  Everything is compared bit
for bit.

Kernel sizes (capture, img_scale (32, 24), resized, pad (24, 32)), the even counterparts of tests/test_raw_frames_gpu.py's:
  38 x 54   -> 23 x 32   downscale, a pad row at the bottom
  100 x 130 -> 24 x 31   a pad column on the right
  20 x 24   -> 24 x 29   UPSCALE: the low and the high border clamp fire on both axes; pad columns
  24 x 32   -> 24 x 32   the copy
  98 x 132  -> 24 x 32   a non-integer reduction of about 4, no pad
each on full-range random bytes (the Y < 16 clamp and both saturations; about 40 % of the converted bytes saturated) and on video-range
bytes (about 10 %, so a wrong coefficient or rounding shows), in the tight layout and in a padded one (pitch = Ws + 10 rounded up to even,
uv_row = Hs + 2, every slack byte 0xA5), and one pair of 968 x 1296 surfaces -> 239 x 320 in 240 x 320, the real tap table.  Outputs are
pre-filled with NaN / 0xFF.  tests/test_nv12_frames_cpu.py shows that a floating-point conversion differs from the host definition on every
size and data set."""
from ctypes import c_void_p

import numpy as np
import pytest
import torch

import nv12_ref as N
import raw_frames_ref as R
from test_pipeline_edges_gpu import GOLDEN, MEAN_STD
from test_raw_frames_gpu import IDS, PAD, RAW, SCALE, STATE, _assert_case, _launch, _states_equal

pytestmark = pytest.mark.gpu

_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _planes(size_key, data):
    return _cached(("planes", size_key, data), lambda: N.planes(N.SIZES[size_key][0], data))


def _bgr(size_key, data):
    return _cached(("bgr", size_key, data), lambda: N.to_bgr(*_planes(size_key, data)))


def _ref(size_key, data, norm, ids_key):
    """The oracle of one case, computed once (read-only afterwards)."""
    _, scale, _, pad = N.SIZES[size_key]
    return _cached(("ref", size_key, data, norm, ids_key), lambda: R.prepare(_bgr(size_key, data), scale, pad, *MEAN_STD[norm], ids=IDS[ids_key]))


def _launch_nv12(surf_d, ids, size, uv_row, hr, wr, h, w, mean, std, with_u8=True):
    """ndet_resize_normalize_views_nv12 on pre-filled outputs: NaN in the float planes, 0xFF in the bytes."""
    from nerfdet_amd import _lib
    dev = surf_d.device
    n, rows, pitch = surf_d.shape
    n_sel = n if ids is None else len(ids)
    ids_d = None if ids is None else torch.tensor(ids, dtype=torch.int32, device=dev)
    img = torch.full((n_sel, 3, h, w), float("nan"), device=dev)
    dn = torch.full_like(img, float("nan"))
    u8 = torch.full((n_sel, h, w, 3), 255, dtype=torch.uint8, device=dev) if with_u8 else None
    mean, std = np.asarray(mean, np.float64), np.asarray(std, np.float64)
    _lib.check(_lib.load().ndet_resize_normalize_views_nv12(_lib._ptr(surf_d), _lib._ptr(ids_d), n_sel, size[0], size[1], pitch, uv_row, rows, hr, wr, h, w,
                                                            mean.ctypes.data_as(c_void_p), std.ctypes.data_as(c_void_p), _lib._ptr(img), _lib._ptr(dn),
                                                            _lib._ptr(u8), c_void_p(_lib.raw_stream(dev))), "resize_normalize_views_nv12")
    torch.cuda.synchronize()
    return img, dn, u8


def _all_equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ---- 1. the ingest kernel ----
@pytest.mark.parametrize("ids_key", list(IDS))
@pytest.mark.parametrize("norm", list(MEAN_STD))
@pytest.mark.parametrize("data", N.DATA)
@pytest.mark.parametrize("size_key", list(N.SIZES))
def test_ingest_kernel_matches_the_host_chain_in_every_byte(device, size_key, data, norm, ids_key):
    size, scale, (hr, wr), (h, w) = N.SIZES[size_key]
    mean, std = MEAN_STD[norm]
    y, uv = _planes(size_key, data)
    ref = _ref(size_key, data, norm, ids_key)
    assert ref["resized_hw"] == (hr, wr)
    what = f"{size_key} {data} {norm} ids={ids_key}"
    # tight layout: the oracle in every byte and float, the content against k_normalize_views, the pad region exactly
    tight = _launch_nv12(torch.from_numpy(N.pack(y, uv)).to(device), IDS[ids_key], size, size[0], hr, wr, h, w, mean, std)
    _assert_case(tight, ref, hr, wr, mean, std, what)
    # the BGR entry on the uploaded host-converted frames writes the same bits
    assert _all_equal(tight, _launch(torch.from_numpy(_bgr(size_key, data)).to(device), IDS[ids_key], hr, wr, h, w, mean, std)), f"{what}: BGR entry"
    # a padded layout gives the tight layout's bytes: no slack byte is read as a pixel
    pitch, uv_row, rows = N.padded_layout(size)
    surf = N.pack(y, uv, pitch, uv_row, rows)
    assert int((surf == N.SLACK).sum()) >= y.shape[0] * (rows * pitch - size[0] * size[1] * 3 // 2)
    assert _all_equal(tight, _launch_nv12(torch.from_numpy(surf).to(device), IDS[ids_key], size, uv_row, hr, wr, h, w, mean, std)), f"{what}: padded"


# ---- 2. capture size ----
def test_capture_size_surfaces(device):
    """Two surfaces of 968 x 1296 -> 239 x 320 in 240 x 320 (cfg2's ScanNet case), one per data set: the real tap table and the pad row,
    every byte against the oracle; the padded layout; without the byte output; the public wrapper."""
    from nerfdet_amd import pipeline as P
    size = (968, 1296)
    assert P.rescale_size(size, (320, 240)) == (239, 320)
    pl = [N.planes(size, d, n=1, seed=i) for i, d in enumerate(N.DATA)]
    y, uv = np.concatenate([p[0] for p in pl]), np.concatenate([p[1] for p in pl])
    mean, std = MEAN_STD["default"]
    ref = R.prepare(N.to_bgr(y, uv), (320, 240), (240, 320), mean, std)
    sd = torch.from_numpy(N.pack(y, uv)).to(device)
    got = _launch_nv12(sd, None, size, 968, 239, 320, 240, 320, mean, std)
    _assert_case(got, ref, 239, 320, mean, std, "968x1296")
    pitch, uv_row, rows = N.padded_layout(size)
    pd = torch.from_numpy(N.pack(y, uv, pitch, uv_row, rows)).to(device)
    assert _all_equal(got, _launch_nv12(pd, None, size, uv_row, 239, 320, 240, 320, mean, std))
    img, dn, none = _launch_nv12(sd, [1, 0], size, 968, 239, 320, 240, 320, mean, std, with_u8=False)
    assert none is None and torch.equal(img, got[0].flip(0)) and torch.equal(dn, got[1].flip(0))
    a, b, c = P.prepare_frames(pd, (320, 240), (240, 320), want_u8=True, format="nv12", size=size, uv_row=uv_row)
    assert _all_equal((a, b, c), got)
    a2, b2 = P.prepare_frames(sd, (320, 240), (240, 320), ids=[1, 1], format="nv12", size=size)
    assert torch.equal(a2[0], a[1]) and torch.equal(b2[1], b[1])
    with pytest.raises(ValueError, match="ids"):
        P.prepare_frames(sd, (320, 240), (240, 320), ids=[2], format="nv12", size=size)


# ---- 3. ndet_nv12_to_bgr ----
TO_BGR = list(N.SIZES) + ["2x2", "2x514-partial-last-workgroup"]


@pytest.mark.parametrize("layout", ["tight", "padded"])
@pytest.mark.parametrize("size_key", TO_BGR)
def test_nv12_to_bgr_matches_the_host_function_in_every_byte(device, size_key, layout):
    from nerfdet_amd import pipeline as P
    if size_key in N.SIZES:
        size, data, ids = N.SIZES[size_key][0], N.DATA[len(size_key) % 2], IDS["descending-with-repeats"]
        y, uv = _planes(size_key, data)
        want = _bgr(size_key, data)
    else:
        size, ids = tuple(int(v) for v in size_key.split("-")[0].split("x")), [2, 0, 2]
        rng = np.random.RandomState(size[1])
        y, uv = rng.randint(0, 256, (3,) + size).astype(np.uint8), rng.randint(0, 256, (3, size[0] // 2, size[1] // 2, 2)).astype(np.uint8)
        want = N.to_bgr(y, uv)
        assert (3 * (size[0] // 2) * (size[1] // 2)) % 256 != 0
    pitch, uv_row, rows = N.tight_layout(size) if layout == "tight" else N.padded_layout(size)
    sd = torch.from_numpy(N.pack(y, uv, pitch, uv_row, rows)).to(device)
    got = P.nv12_to_bgr(sd, size, uv_row=uv_row)
    assert got.shape == want.shape and got.dtype == torch.uint8 and torch.equal(got.cpu(), torch.from_numpy(want)), f"{size_key} {layout}"
    sel = P.nv12_to_bgr(sd, size, uv_row=uv_row, ids=ids)
    assert torch.equal(sel.cpu(), torch.from_numpy(want[ids])), f"{size_key} {layout} ids"
    with pytest.raises(ValueError, match="ids"):
        P.nv12_to_bgr(sd, size, uv_row=uv_row, ids=[len(y)])


# ---- 4. ndet_bgr_to_nv12 ----
@pytest.mark.parametrize("hw", [(24, 32), (23, 31), (24, 31), (23, 32), (1, 1), (239, 320)])
def test_bgr_to_nv12_matches_the_host_function_in_every_byte(device, hw):
    from nerfdet_amd import _lib
    from nerfdet_amd import pipeline as P
    h, w = hw
    n = 3
    frames = np.random.RandomState(h * 1000 + w).randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    frames[0, 0, 0] = (255, 255, 255)
    frames[-1, -1, -1] = (0, 0, 0)
    want = N.to_nv12(frames)
    he, we = h + h % 2, w + w % 2
    assert want.shape == (n, he * 3 // 2, we) and int(want.max()) < 255            # Y <= 235, U, V <= 240: 0xFF is never a result
    fd = torch.from_numpy(frames).to(device)
    out = torch.full((n, he * 3 // 2, we), 255, dtype=torch.uint8, device=device)
    _lib.check(_lib.load().ndet_bgr_to_nv12(_lib._ptr(fd), n, h, w, _lib._ptr(out), c_void_p(_lib.raw_stream(fd.device))), "bgr_to_nv12")
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.from_numpy(want)), hw
    a, size = P.bgr_to_nv12(fd)
    b, _ = P.bgr_to_nv12(fd)
    assert size == (he, we) and torch.equal(a, out) and torch.equal(b, out)
    # and back: the surfaces are what the ingest side takes
    back = P.nv12_to_bgr(a, size)
    y, uv = N.unpack(want, size)
    assert torch.equal(back.cpu(), torch.from_numpy(N.to_bgr(y, uv)))


# ---- 5. streams ----
def _nv12_scene(device, seed, layout="tight", n_v=6, turn=0):
    """A scene of NV12 surfaces (1, n_v, rows, pitch) at 128 x 194, the host-converted BGR frames (1, n_v, 128, 194, 3), its meta (the raw
    scene of tests/test_raw_frames_gpu.py) and the layout's uv_row."""
    from nerfdet_amd import pipeline as P
    from oracle import nerfdet_oracle as O
    y, uv = N.planes(RAW, N.DATA[seed % 2], n=n_v, seed=seed)
    pitch, uv_row, rows = N.tight_layout(RAW) if layout == "tight" else N.padded_layout(RAW)
    ring = O.ring_scene_meta(n_v, PAD)["lidar2img"]
    ring["extrinsic"] = ring["extrinsic"][turn:] + ring["extrinsic"][:turn]
    ring["origin"] = np.asarray(ring["origin"], np.float32) + np.float32([0.2 * turn, -0.1 * turn, 0.0])
    meta = P.frame_meta(ring, RAW, SCALE, PAD)
    assert (meta["ori_shape"], meta["img_shape"], meta["pad_shape"]) == ((128, 194, 3), (63, 96, 3), (64, 96, 3))
    return (torch.from_numpy(N.pack(y, uv, pitch, uv_row, rows)).to(device).unsqueeze(0), torch.from_numpy(N.to_bgr(y, uv)).to(device).unsqueeze(0),
            meta, uv_row)


def _depth_frames(device, n, k, seed):
    rs = np.random.RandomState(seed)
    d = (rs.randint(300, 6000, (n, k, 60, 80)) * (rs.rand(n, k, 60, 80) > 0.2)).astype(np.uint16)
    return torch.from_numpy(d).to(device)


def _banks_equal(a, b):
    same = lambda x, y: torch.equal(x, y) if isinstance(x, torch.Tensor) else np.array_equal(np.asarray(x), np.asarray(y))
    return len(a.segments) == len(b.segments) and all(same(getattr(p, t), getattr(q, t)) for p, q in zip(a.segments, b.segments)
                                                        for t in ("feat", "rgb4", "ke"))


@pytest.mark.parametrize("layout", ["tight", "padded"])
def test_stream_add_frames_nv12_is_add_frames_of_the_converted_frames(device, layout):
    from test_detector_gpu import _small_detector
    from test_streaming_gpu import _chunk_meta, _same
    det = _small_detector(device)
    surf, bgr, meta, uv_row = _nv12_scene(device, 21, layout)
    depth = _depth_frames(device, 1, 6, 3)
    a, b = det.begin_scene(dict(meta), keep_views=True), det.begin_scene(dict(meta), keep_views=True)
    for v0, v1, with_depth in ((0, 4, False), (4, 6, True)):
        d = depth[:, v0:v1].contiguous() if with_depth else None
        a.add_frames(surf[:, v0:v1], _chunk_meta(meta, v0, v1), depth_frames=d, format="nv12", uv_row=uv_row)
        b.add_frames(bgr[:, v0:v1], _chunk_meta(meta, v0, v1), depth_frames=d)
    assert a.n_views == b.n_views == 6 and _states_equal(a.state, b.state) and int(a.state.k1_count.sum()) > 0
    assert _banks_equal(a.bank, b.bank) and a.bank.n_views == 6
    _same(a.detect(), b.detect())
    # a refused call (a chunk meta with one extrinsic too many) changes nothing: state and bank
    keep = [getattr(a.state, t).clone() for t in STATE]
    with pytest.raises(ValueError, match="extrinsics"):
        a.add_frames(surf[:, :2], _chunk_meta(meta, 0, 3), format="nv12", uv_row=uv_row)
    with pytest.raises(ValueError, match="rows do not hold"):
        a.add_frames(surf[:, :2, :-2].contiguous(), _chunk_meta(meta, 0, 2), format="nv12", uv_row=uv_row)     # the padded layout has one spare row
    assert a.n_views == 6 and all(torch.equal(getattr(a.state, t), k) for t, k in zip(STATE, keep)) and _banks_equal(a.bank, b.bank)


def test_windowed_stream_add_frames_nv12_with_an_eviction(device):
    from test_detector_gpu import _small_detector
    from test_streaming_gpu import _chunk_meta, _same
    det = _small_detector(device)
    surf, bgr, meta, uv_row = _nv12_scene(device, 22, "padded")
    a, b = det.begin_scene(dict(meta), window=2), det.begin_scene(dict(meta), window=2)
    for v0, v1 in ((0, 2), (2, 4), (4, 6)):                    # the third chunk evicts the first
        a.add_frames(surf[:, v0:v1], _chunk_meta(meta, v0, v1), format="nv12", uv_row=uv_row)
        b.add_frames(bgr[:, v0:v1], _chunk_meta(meta, v0, v1))
    assert a.chunk_views == b.chunk_views == [2, 2]
    assert all(_states_equal(p, q) for p, q in zip(a._segs, b._segs))
    _same(a.detect(), b.detect())
    keep = [[getattr(st, t).clone() for t in STATE] for st in a._segs]
    with pytest.raises(ValueError, match="extrinsics"):
        a.add_frames(surf[:, :2], _chunk_meta(meta, 0, 3), format="nv12", uv_row=uv_row)
    assert a.chunk_views == [2, 2] and all(torch.equal(getattr(st, t), k) for st, ks in zip(a._segs, keep) for t, k in zip(STATE, ks))


@pytest.mark.parametrize("keep_views", [False, True])
def test_group_add_frames_nv12_is_add_frames_of_the_converted_frames(device, keep_views):
    """Three scenes, one call for all of them (4 views each) and a subset call scenes=[2, 0] (2 views each, with depth frames): the group fed
    surfaces holds the bits of a group fed the converted frames by the same calls."""
    from test_detector_gpu import _small_detector
    from test_streaming_gpu import _chunk_meta, _same
    det = _small_detector(device)
    sc = [_nv12_scene(device, 30 + i, "padded", turn=i) for i in range(3)]
    uv_row = sc[0][3]
    metas = [dict(s[2]) for s in sc]
    a, b = det.begin_scenes(metas, keep_views=keep_views), det.begin_scenes(metas, keep_views=keep_views)
    depth = _depth_frames(device, 2, 2, 4)
    for rows, v0, v1, d in (([0, 1, 2], 0, 4, None), ([2, 0], 4, 6, depth)):
        chunk = [_chunk_meta(sc[s][2], v0, v1) for s in rows]
        a.add_frames(torch.cat([sc[s][0][:, v0:v1] for s in rows]), chunk, scenes=rows, depth_frames=d, format="nv12", uv_row=uv_row)
        b.add_frames(torch.cat([sc[s][1][:, v0:v1] for s in rows]), chunk, scenes=rows, depth_frames=d)
    assert a.n_views == b.n_views == [6, 4, 6]
    assert all(_states_equal(sa, sb) for sa, sb in zip(a.group.states, b.group.states))
    if keep_views:
        assert all(_banks_equal(p, q) for p, q in zip(a.banks, b.banks)) and [bk.n_views for bk in a.banks] == [6, 4, 6]
    for got, want in zip(a.detect(), b.detect()):
        _same(got, want)
    keep = [[getattr(st, t).clone() for t in STATE] for st in a.group.states]
    with pytest.raises(ValueError, match="extrinsics"):
        a.add_frames(torch.cat([sc[s][0][:, :2] for s in (2, 0)]), [_chunk_meta(sc[2][2], 0, 2), _chunk_meta(sc[0][2], 0, 1)], scenes=[2, 0],
                     format="nv12", uv_row=uv_row)
    assert a.n_views == [6, 4, 6]
    assert all(torch.equal(getattr(st, t), k) for st, ks in zip(a.group.states, keep) for t, k in zip(STATE, ks))
    if keep_views:
        assert all(_banks_equal(p, q) for p, q in zip(a.banks, b.banks))


# ---- 6. score_frames ----
def _scores_equal(got, want):
    assert list(got) == list(want)
    for key in want:
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key].cpu().numpy(), want[key].cpu().numpy(), equal_nan=True), key


@pytest.mark.parametrize("ssim", [False, True])
def test_score_frames_nv12_scores_the_converted_frames(device, ssim):
    from test_detector_gpu import _small_detector
    from test_streaming_gpu import _chunk_meta
    det = _small_detector(device)
    sc = [_nv12_scene(device, 40 + i, "padded", turn=i) for i in range(2)]
    uv_row = sc[0][3]
    scene = det.begin_scene(dict(sc[0][2]), keep_views=True)
    scene.add_frames(sc[0][1][:, :4], _chunk_meta(sc[0][2], 0, 4))
    depth = _depth_frames(device, 2, 2, 5)
    chunk = _chunk_meta(sc[0][2], 4, 6)
    got = scene.score_frames(sc[0][0][:, 4:6], chunk, depth_frames=depth[:1], ssim=ssim, format="nv12", uv_row=uv_row)
    want = scene.score_frames(sc[0][1][:, 4:6], chunk, depth_frames=depth[:1], ssim=ssim)
    _scores_equal(got, want)
    assert all(k in got for k in ("sse", "n_px", "depth_sad_mm", "n_depth") + (("ssim", "n_windows") if ssim else ()))
    assert int(got["n_px"].sum()) > 0
    group = det.begin_scenes([dict(s[2]) for s in sc], keep_views=True)
    group.add_frames(torch.cat([s[1][:, :4] for s in sc]), [_chunk_meta(s[2], 0, 4) for s in sc])
    listed = [1, 0]
    metas = [_chunk_meta(sc[s][2], 4, 6) for s in listed]
    g = group.score_frames(torch.cat([sc[s][0][:, 4:6] for s in listed]), metas, scenes=listed, depth_frames=depth, ssim=ssim, format="nv12", uv_row=uv_row)
    w = group.score_frames(torch.cat([sc[s][1][:, 4:6] for s in listed]), metas, scenes=listed, depth_frames=depth, ssim=ssim)
    assert len(g) == len(w) == 2
    for x, y in zip(g, w):
        _scores_equal(x, y)


# ---- 7. MultiViewPipeline(frame_format="nv12") ----
def _batches_equal(a, b, path="batch"):
    if isinstance(a, torch.Tensor):
        assert isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), path
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b), path
    elif isinstance(a, dict):
        assert list(a) == list(b), path
        for k in a:
            _batches_equal(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _batches_equal(x, y, f"{path}[{i}]")
    else:
        assert a == b, path


@pytest.mark.parametrize("margin", [0, 3])
def test_raw_pipeline_nv12_is_the_bgr_raw_pipeline_on_converted_frames(device, margin):
    import os
    from nerfdet_amd import pipeline as P
    z = np.load(os.path.join(GOLDEN, "pipeline_small.npz"))
    info = dict(extrinsics=list(z["poses"]), intrinsics=z["intrinsic"], annos=dict(axis_align_matrix=z["axis_align"]))
    size_key = "38x54-down-bottom-pad"
    size, scale, (hr, wr), (h, w) = N.SIZES[size_key]
    mean, std = MEAN_STD["spread"]
    ids, tids = [13, 13, 9, 9, 4, 2, 2, 0], [7, 13, 2]
    y, uv = _planes(size_key, "video-range")
    pitch, uv_row, rows = N.padded_layout(size)
    kw = dict(mean=mean, std=std, margin=margin, nerf_target_views=len(tids), img_scale=scale, pad_size=(h, w))
    cams = P.scene_cameras(info)
    depth = torch.from_numpy(np.random.RandomState(2).randint(300, 6000, (14, 30, 40)).astype(np.uint16)).to(device)
    got = P.MultiViewPipeline(len(ids), frame_format="nv12", **kw)(torch.from_numpy(N.pack(y, uv, pitch, uv_row, rows)).to(device), cams, size + (3,),
                                                                  ids=ids, target_ids=tids, depth_frames=depth, uv_row=uv_row)
    want = P.MultiViewPipeline(len(ids), **kw)(torch.from_numpy(_bgr(size_key, "video-range")).to(device), cams, None, ids=ids, target_ids=tids,
                                              depth_frames=depth)
    torch.cuda.synchronize()
    assert got["img_metas"][0]["ori_shape"] == (38, 54, 3) and got["img_metas"][0]["img_shape"] == (hr, wr, 3)
    assert {"img", "denorm_images", "raydirs", "lightpos", "gt_images", "depth", "gt_depths", "depth_rays"} <= set(got)
    _batches_equal(got, want)
    ref = _ref(size_key, "video-range", "spread", "descending-with-repeats")
    assert torch.equal(got["img"][0].cpu(), torch.from_numpy(ref["img"]))
