"""The NV12 path without a GPU: the three entry points are exported and refuse what their header says before any device work, the two host
definitions (datasets.nv12_to_bgr, datasets.bgr_to_nv12) give the anchor values and stay inside int32, the every-byte GPU tests are not
blind to a floating-point conversion, and add_frames(format="nv12") refuses surfaces that its scene's meta does not describe before
anything touches a device."""
import ctypes

import numpy as np
import pytest
import torch

import nv12_ref as N

F = ctypes.c_void_p(0x1000)
MEAN_OK, STD_OK = (ctypes.c_double * 3)(123.675, 116.28, 103.53), (ctypes.c_double * 3)(58.395, 57.12, 57.375)


def test_the_library_exports_the_three_entry_points():
    from nerfdet_amd import _lib
    lib = _lib.load()
    for name, n_args in (("ndet_resize_normalize_views_nv12", 18), ("ndet_nv12_to_bgr", 10), ("ndet_bgr_to_nv12", 6)):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][0]) == n_args, name
    assert len(_lib.SIGNATURES["ndet_resize_normalize_views"][0]) == 15      # the BGR entry keeps its signature


def _ingest(surfaces=F, ids=F, n_sel=2, Hs=38, Ws=54, pitch=54, uv_row=38, rows=57, Hr=23, Wr=32, H=24, W=32, mean=MEAN_OK, std=STD_OK, img=F,
            denorm=F, u8=F):
    from nerfdet_amd import _lib
    return _lib.load().ndet_resize_normalize_views_nv12(surfaces, ids, n_sel, Hs, Ws, pitch, uv_row, rows, Hr, Wr, H, W, mean, std, img, denorm, u8, None)


def _to_bgr(surfaces=F, ids=F, n_sel=2, Hs=38, Ws=54, pitch=54, uv_row=38, rows=57, out=F):
    from nerfdet_amd import _lib
    return _lib.load().ndet_nv12_to_bgr(surfaces, ids, n_sel, Hs, Ws, pitch, uv_row, rows, out, None)


def _to_nv12(frames=F, n=2, H=23, W=31, out=F):
    from nerfdet_amd import _lib
    return _lib.load().ndet_bgr_to_nv12(frames, n, H, W, out, None)


def test_the_ingest_entry_refuses_bad_arguments_without_a_gpu():
    from nerfdet_amd import _lib
    err = _lib.load().ndet_last_error
    for null in ("surfaces", "mean", "std", "img", "denorm"):
        assert _ingest(**{null: None}) == -1 and b"null pointer" in err(), null
    for bad in ("n_sel", "Hs", "Ws", "pitch", "uv_row", "rows", "Hr", "Wr", "H", "W"):
        for v in (0, -3):
            assert _ingest(**{bad: v}) == -1 and b"sizes must be positive" in err(), (bad, v)
    for bad in ((58.395, 0.0, 57.375), (-1.0, 57.12, 57.375), (58.395, 57.12, float("nan"))):
        assert _ingest(std=(ctypes.c_double * 3)(*bad)) == -1 and b"std must be positive" in err(), bad
    assert _ingest(Hr=25) == -1 and b"does not fit the pad" in err()
    assert _ingest(Wr=33) == -1 and b"does not fit the pad" in err()
    assert _ingest(Hs=37) == -1 and b"even sizes" in err()
    assert _ingest(Ws=53) == -1 and b"even sizes" in err()
    assert _ingest(pitch=52) == -1 and b"pitch 52 is below the width 54" in err()
    assert _ingest(uv_row=36) == -1 and b"uv_row 36 lies inside the Y plane" in err()
    assert _ingest(rows=56) == -1 and b"56 rows do not hold a UV plane of 19 rows at row 38" in err()
    assert _ingest(uv_row=40, rows=58) == -1 and b"do not hold a UV plane" in err()
    # the 16-bit UV load: an odd pitch or an odd base address
    assert _ingest(pitch=55) == -2 and b"odd pitch" in err()
    assert _ingest(surfaces=ctypes.c_void_p(0x1001)) == -2 and b"base address" in err()
    # one surface of 2^31 bytes or more; one view's output planes of 2^31 elements or more; 2^31 workgroups or more
    assert 49152 * 43692 >= 1 << 31 > 49152 * 43690
    assert _ingest(Hs=32768, Ws=43692, pitch=43692, uv_row=32768, rows=49152) == -2 and b"surface" in err() and b"2^31" in err()
    assert _ingest(surfaces=ctypes.c_void_p(0x1001), Hs=32768, Ws=43690, pitch=43690, uv_row=32768, rows=49152) == -2 \
        and b"base address" in err()                                                                  # just below: the next refusal
    assert _ingest(Hr=32768, Wr=21846, H=32768, W=21846) == -2 and b"planes" in err() and b"2^31" in err()
    assert _ingest(n_sel=1 << 30, H=512, W=1024, Hr=23, Wr=32) == -2 and b"workgroups" in err()
    # ids and resized_bgr may be null: with them null the next refusal is still the one reported
    assert _ingest(ids=None, u8=None, Hr=25) == -1 and b"does not fit the pad" in err()


def test_the_conversion_entries_refuse_bad_arguments_without_a_gpu():
    from nerfdet_amd import _lib
    err = _lib.load().ndet_last_error
    for null in ("surfaces", "out"):
        assert _to_bgr(**{null: None}) == -1 and b"null pointer" in err(), null
    for bad in ("n_sel", "Hs", "Ws", "pitch", "uv_row", "rows"):
        assert _to_bgr(**{bad: 0}) == -1 and b"sizes must be positive" in err(), bad
    assert _to_bgr(Hs=37) == -1 and b"even sizes" in err()
    assert _to_bgr(pitch=52) == -1 and b"below the width" in err()
    assert _to_bgr(uv_row=37) == -1 and b"inside the Y plane" in err()
    assert _to_bgr(rows=56) == -1 and b"do not hold a UV plane" in err()
    assert _to_bgr(pitch=55) == -2 and b"odd pitch" in err()
    assert _to_bgr(surfaces=ctypes.c_void_p(0x1001)) == -2 and b"base address" in err()
    assert _to_bgr(Hs=32768, Ws=43692, pitch=43692, uv_row=32768, rows=49152) == -2 and b"2^31" in err()
    assert _to_bgr(Hs=32768, Ws=21846, pitch=21846, uv_row=32768, rows=49152) == -2 and b"frame" in err() and b"2^31" in err()
    assert _to_bgr(ids=None, rows=56) == -1 and b"do not hold a UV plane" in err()
    for null in ("frames", "out"):
        assert _to_nv12(**{null: None}) == -1 and b"null pointer" in err(), null
    for bad in ("n", "H", "W"):
        for v in (0, -1):
            assert _to_nv12(**{bad: v}) == -1 and b"sizes must be positive" in err(), (bad, v)
    assert _to_nv12(H=32768, W=21846) == -2 and b"frame" in err() and b"2^31" in err()


def test_the_codes_become_the_usual_exceptions():
    from nerfdet_amd import _lib
    with pytest.raises(AssertionError, match="even sizes"):
        _lib.check(_ingest(Hs=37), "resize_normalize_views_nv12")
    with pytest.raises(ValueError, match="odd pitch"):
        _lib.check(_ingest(pitch=55), "resize_normalize_views_nv12")
    with pytest.raises(AssertionError, match="below the width"):
        _lib.check(_to_bgr(pitch=52), "nv12_to_bgr")
    with pytest.raises(ValueError, match="2\\^31"):
        _lib.check(_to_nv12(H=32768, W=21846), "bgr_to_nv12")


# ---- the two host definitions ----
NV12_TO_BGR = [((16, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255)), ((0, 128, 128), (0, 0, 0)), ((81, 90, 240), (0, 0, 254)),
               ((41, 240, 110), (255, 0, 0))]
BGR_TO_NV12 = [((0, 0, 0), (16, 128, 128)), ((255, 255, 255), (235, 128, 128)), ((0, 0, 255), (82, 90, 240)), ((255, 0, 0), (41, 240, 110)),
               ((0, 255, 0), (145, 54, 34))]


@pytest.mark.parametrize("yuv,bgr", NV12_TO_BGR)
def test_nv12_to_bgr_anchor_values(yuv, bgr):
    from nerfdet_amd.datasets import nv12_to_bgr
    y = np.full((4, 6), yuv[0], np.uint8)
    uv = np.broadcast_to(np.uint8(yuv[1:]), (2, 3, 2)).copy()
    out = nv12_to_bgr(y, uv)
    assert out.shape == (4, 6, 3) and out.dtype == np.uint8 and (out == np.uint8(bgr)).all(), out[0, 0]


@pytest.mark.parametrize("bgr,yuv", BGR_TO_NV12)
def test_bgr_to_nv12_anchor_values(bgr, yuv):
    from nerfdet_amd.datasets import bgr_to_nv12
    y, uv = bgr_to_nv12(np.broadcast_to(np.uint8(bgr), (3, 5, 3)).copy())
    assert y.shape == (4, 6) and uv.shape == (2, 3, 2) and y.dtype == uv.dtype == np.uint8
    assert (y == yuv[0]).all() and (uv == np.uint8(yuv[1:])).all(), (y[0, 0], uv[0, 0])


def test_nv12_to_bgr_uses_the_nearest_chroma_and_refuses_odd_sizes():
    from nerfdet_amd.datasets import nv12_to_bgr
    y = np.full((4, 4), 128, np.uint8)
    uv = np.full((2, 2, 2), 128, np.uint8)
    uv[1, 0] = (90, 240)                                        # one chroma sample: rows 2-3, columns 0-1 and nothing else
    out = nv12_to_bgr(y, uv)
    tinted = (out != out[0, 0]).any(axis=-1)
    want = np.zeros((4, 4), bool)
    want[2:, :2] = True
    assert np.array_equal(tinted, want)
    with pytest.raises(ValueError, match="even"):
        nv12_to_bgr(np.zeros((3, 4), np.uint8), np.zeros((1, 2, 2), np.uint8))
    with pytest.raises(ValueError, match="even"):
        nv12_to_bgr(np.zeros((4, 4), np.uint8), np.zeros((2, 2), np.uint8))


def test_the_conversion_stays_inside_int32():
    """Every intermediate of nv12_to_bgr over all 2^24 inputs: the extremes are at the ends of each operand's range, and |.| < 5.7e8."""
    y = np.maximum(np.arange(256, dtype=np.int64) - 16, 0) * 1220542 + (1 << 19)
    c = np.arange(256, dtype=np.int64) - 128
    r = y[:, None] + 1673527 * c[None, :]
    b = y[:, None] + 2116026 * c[None, :]
    g = y[:, None, None] - 852492 * c[None, :, None] - 409993 * c[None, None, :]
    worst = max(int(np.abs(t).max()) for t in (r, g, b))
    assert worst == int(np.abs(b).max()) and worst < 5.7e8 < 2 ** 31
    # ... and of bgr_to_nv12: the coefficients of each row sum to below 2^20 in magnitude, times 255, plus the offsets
    for coef, off in (((269484, 528482, 102760), 16), ((-155188, -305135, 460324), 128), ((460324, -385875, -74448), 128)):
        assert sum(abs(k) for k in coef) * 255 + (off << 20) + (1 << 19) < 2 ** 31
    # the host function computes in int32 and agrees with int64 arithmetic at the corners
    from nerfdet_amd.datasets import nv12_to_bgr
    yy, uu, vv = np.meshgrid([0, 15, 16, 17, 235, 255], [0, 1, 128, 254, 255], [0, 1, 128, 254, 255], indexing="ij")
    ys = np.repeat(np.repeat(yy.reshape(-1, 1).astype(np.uint8), 2, 0), 2, 1)              # one 2 x 2 block per combination
    uvs = np.stack((uu.reshape(-1), vv.reshape(-1)), -1).astype(np.uint8)[:, None, :]
    got = nv12_to_bgr(ys, uvs)[::2, 0]
    y64 = np.maximum(yy.reshape(-1).astype(np.int64) - 16, 0) * 1220542 + (1 << 19)
    u64, v64 = uu.reshape(-1).astype(np.int64) - 128, vv.reshape(-1).astype(np.int64) - 128
    want = np.clip(np.stack(((y64 + 2116026 * u64) >> 20, (y64 - 852492 * v64 - 409993 * u64) >> 20, (y64 + 1673527 * v64) >> 20), -1), 0, 255)
    assert np.array_equal(got, want.astype(np.uint8))


@pytest.mark.parametrize("data", N.DATA)
@pytest.mark.parametrize("size_key", list(N.SIZES))
def test_the_host_conversion_is_not_a_float_conversion(size_key, data):
    """What the every-byte GPU tests rest on: on every test size and both data sets the host definition differs from a floating-point
    BT.601 conversion with round-to-nearest in some bytes, so a kernel that converted in floats could not pass them."""
    from nerfdet_amd.datasets import nv12_to_bgr
    y, uv = N.planes(N.SIZES[size_key][0], data, n=1)
    a, b = nv12_to_bgr(y[0], uv[0]), N.float_nv12_to_bgr(y[0], uv[0])
    assert a.shape == b.shape and int((a != b).sum()) > 0


def test_the_data_sets_reach_what_they_are_for():
    y, uv = N.planes((98, 132), "full-range", n=1)
    out = N.to_bgr(y, uv)
    assert (y < 16).any() and all((out[..., c] == 0).any() and (out[..., c] == 255).any() for c in range(3))
    sat = lambda o: float(((o == 0) | (o == 255)).mean())
    yv, uvv = N.planes((98, 132), "video-range", n=1)
    assert yv.min() >= 16 and yv.max() <= 235 and uvv.min() >= 96 and uvv.max() <= 160
    assert sat(out) > 0.25 and sat(N.to_bgr(yv, uvv)) < 0.2


@pytest.mark.parametrize("hw", [(23, 31), (24, 31), (23, 32), (1, 1)])
def test_bgr_to_nv12_on_an_odd_size_is_itself_on_the_edge_padded_frame(hw):
    from nerfdet_amd.datasets import bgr_to_nv12
    h, w = hw
    f = np.random.RandomState(h * 100 + w).randint(0, 256, (h, w, 3)).astype(np.uint8)
    padded = np.pad(f, ((0, h % 2), (0, w % 2), (0, 0)), mode="edge")
    (y, uv), (y2, uv2) = bgr_to_nv12(f), bgr_to_nv12(padded)
    assert y.shape == (h + h % 2, w + w % 2) and uv.shape == (y.shape[0] // 2, y.shape[1] // 2, 2)
    assert np.array_equal(y, y2) and np.array_equal(uv, uv2)


def test_pack_and_unpack_are_inverse_and_keep_the_slack():
    size = (38, 54)
    y, uv = N.planes(size, "full-range", n=3)
    pitch, uv_row, rows = N.padded_layout(size)
    assert (pitch, uv_row, rows) == (64, 40, 60)
    s = N.pack(y, uv, pitch, uv_row, rows)
    y2, uv2 = N.unpack(s, size, uv_row)
    assert np.array_equal(y, y2) and np.array_equal(uv, uv2)
    assert (s[:, :, 54:] == N.SLACK).all() and (s[:, 38:40] == N.SLACK).all() and (s[:, 59:] == N.SLACK).all()
    t = N.pack(y, uv)
    assert N.tight_layout(size) == (54, 38, 57) and t.shape == (3, 57, 54)
    assert np.array_equal(N.unpack(t, size)[1], uv)


def test_the_even_sizes_rescale_as_the_table_says():
    from nerfdet_amd import pipeline as P
    import raw_frames_ref as R
    for size, scale, want, pad in N.SIZES.values():
        assert P.rescale_size(size, scale) == want == R.resized_size(size, scale)
        assert want[0] <= pad[0] and want[1] <= pad[1] and size[0] % 2 == 0 and size[1] % 2 == 0


def test_the_wrappers_refuse_before_any_device_work():
    from nerfdet_amd import pipeline as P
    ok = torch.zeros(2, 57, 54, dtype=torch.uint8)
    kw = dict(format="nv12", size=(38, 54))
    with pytest.raises(ValueError, match="format="):
        P.prepare_frames(ok, (32, 24), (24, 32), format="i420", size=(38, 54))
    with pytest.raises(ValueError, match="size="):
        P.prepare_frames(ok, (32, 24), (24, 32), format="nv12")
    with pytest.raises(ValueError, match="NV12 surfaces"):
        P.prepare_frames(torch.zeros(2, 38, 54, 3, dtype=torch.uint8), (32, 24), (24, 32), **kw)
    with pytest.raises(ValueError, match="NV12 surfaces"):
        P.prepare_frames(ok.float(), (32, 24), (24, 32), **kw)
    with pytest.raises(ValueError, match="even sizes"):
        P.prepare_frames(ok, (32, 24), (24, 32), format="nv12", size=(37, 54))
    with pytest.raises(ValueError, match="pitch"):
        P.prepare_frames(ok, (32, 24), (24, 32), format="nv12", size=(38, 56))
    with pytest.raises(ValueError, match="uv_row"):
        P.prepare_frames(ok, (32, 24), (24, 32), uv_row=37, **kw)
    with pytest.raises(ValueError, match="57 rows do not hold"):
        P.prepare_frames(ok, (32, 24), (24, 32), uv_row=40, **kw)
    with pytest.raises(ValueError, match="odd pitch"):
        P.prepare_frames(torch.zeros(2, 57, 55, dtype=torch.uint8), (32, 24), (24, 32), **kw)
    with pytest.raises(ValueError, match="describe NV12 surfaces"):
        P.prepare_frames(torch.zeros(2, 38, 54, 3, dtype=torch.uint8), (32, 24), (24, 32), size=(38, 54))
    with pytest.raises(ValueError, match="does not fit"):
        P.prepare_frames(torch.zeros(1, 81, 38, dtype=torch.uint8), (32, 24), (24, 32), format="nv12", size=(54, 38))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        P.prepare_frames(ok, (32, 24), (24, 32), **kw)
    with pytest.raises(ValueError, match="NV12 surfaces"):
        P.nv12_to_bgr(ok[0], (38, 54))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        P.nv12_to_bgr(ok, (38, 54))
    with pytest.raises(ValueError, match="uint8 frames"):
        P.bgr_to_nv12(torch.zeros(2, 23, 31, 3))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        P.bgr_to_nv12(torch.zeros(2, 23, 31, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="format='yuv'"):
        P.MultiViewPipeline(4, img_scale=(32, 24), pad_size=(24, 32), frame_format="yuv")
    with pytest.raises(ValueError, match="capture resolution"):
        P.MultiViewPipeline(4, frame_format="nv12")
    pipe = P.MultiViewPipeline(2, img_scale=(32, 24), pad_size=(24, 32), frame_format="nv12")
    with pytest.raises(ValueError, match="ori_shape"):
        pipe(ok, {}, None, ids=[0, 1])
    with pytest.raises(ValueError, match="57 rows do not hold"):
        pipe(ok, {}, (40, 54, 3), ids=[0, 1])
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        pipe(ok, {}, (38, 54, 3), ids=[0, 1])


# ---- add_frames(format="nv12") refuses before any device work ----
class _Det:
    training = False


def _raw_meta(n_v=6, size=(128, 194)):
    from nerfdet_amd import pipeline as P
    from nerfdet_amd.synth import ring_scene_meta
    return P.frame_meta(ring_scene_meta(n_v, (64, 97))["lidar2img"], size, (96, 64), (64, 96))


def _chunk(meta, k):
    m = dict(meta)
    m["lidar2img"] = dict(meta["lidar2img"], extrinsic=meta["lidar2img"]["extrinsic"][:k])
    return m


def test_stream_add_frames_refuses_surfaces_its_meta_does_not_describe():
    from nerfdet_amd.streaming import SceneStream
    meta = _raw_meta()
    assert (meta["ori_shape"], meta["img_shape"], meta["pad_shape"]) == ((128, 194, 3), (63, 96, 3), (64, 96, 3))
    s = SceneStream.__new__(SceneStream)      # the checks below run before anything touches a device
    s.det, s.meta = _Det(), meta
    ok = torch.zeros(1, 2, 192, 194, dtype=torch.uint8)
    nv = dict(format="nv12")
    with pytest.raises(ValueError, match="format="):
        s.add_frames(ok, _chunk(meta, 2), format="p010")
    with pytest.raises(ValueError, match="NV12 surfaces"):                       # a wrong dtype; a wrong rank (BGR frames); another n
        s.add_frames(ok.float(), _chunk(meta, 2), **nv)
    with pytest.raises(ValueError, match="NV12 surfaces"):
        s.add_frames(torch.zeros(1, 2, 128, 194, 3, dtype=torch.uint8), _chunk(meta, 2), **nv)
    with pytest.raises(ValueError, match="NV12 surfaces"):
        s.add_frames(ok[0], _chunk(meta, 2), **nv)
    with pytest.raises(ValueError, match="NV12 surfaces"):
        s.add_frames(torch.zeros(2, 2, 192, 194, dtype=torch.uint8), _chunk(meta, 2), **nv)
    with pytest.raises(ValueError, match="pitch"):                               # pitch < Ws
        s.add_frames(torch.zeros(1, 2, 192, 192, dtype=torch.uint8), _chunk(meta, 2), **nv)
    with pytest.raises(ValueError, match="191 rows do not hold"):                # too few rows
        s.add_frames(torch.zeros(1, 2, 191, 194, dtype=torch.uint8), _chunk(meta, 2), **nv)
    with pytest.raises(ValueError, match="192 rows do not hold"):                # ... for this uv_row
        s.add_frames(ok, _chunk(meta, 2), uv_row=130, **nv)
    with pytest.raises(ValueError, match="uv_row=127"):                          # uv_row < Hs
        s.add_frames(ok, _chunk(meta, 2), uv_row=127, **nv)
    with pytest.raises(ValueError, match="odd pitch"):
        s.add_frames(torch.zeros(1, 2, 192, 195, dtype=torch.uint8), _chunk(meta, 2), **nv)
    with pytest.raises(ValueError, match="extrinsics"):
        s.add_frames(ok, _chunk(meta, 3), **nv)
    with pytest.raises(ValueError, match="depth"):
        s.add_frames(ok, _chunk(meta, 2), depth=torch.zeros(1, 3, 8, 8), **nv)
    # an odd ori_shape cannot be an NV12 surface
    odd = _raw_meta(size=(127, 193))
    s.meta = odd
    with pytest.raises(ValueError, match="even sizes"):
        s.add_frames(ok, _chunk(odd, 2), **nv)
    # the format is never inferred from the rank: BGR is the default, and says what it always said
    s.meta = meta
    with pytest.raises(ValueError, match="raw uint8 BGR frames"):
        s.add_frames(ok, _chunk(meta, 2))
    with pytest.raises(ValueError, match="raw uint8 BGR frames"):
        s.add_frames(ok, _chunk(meta, 2), format="bgr")
    with pytest.raises(ValueError, match="describes NV12 surfaces"):
        s.add_frames(torch.zeros(1, 2, 128, 194, 3, dtype=torch.uint8), _chunk(meta, 2), uv_row=128)
    # a described chunk passes every check and stops where the device work would begin: tight, and with a pitch and a uv_row
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        s.add_frames(ok, _chunk(meta, 2), **nv)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        s.add_frames(torch.zeros(1, 2, 200, 204, dtype=torch.uint8), _chunk(meta, 2), uv_row=130, **nv)


def test_group_add_frames_refuses_surfaces_its_meta_does_not_describe():
    from nerfdet_amd.streaming import SceneGroup
    meta = _raw_meta()
    g = SceneGroup.__new__(SceneGroup)
    g.det, g.metas = _Det(), [dict(meta) for _ in range(3)]
    ok = torch.zeros(2, 2, 192, 194, dtype=torch.uint8)
    chunks = [_chunk(meta, 2), _chunk(meta, 2)]
    nv = dict(format="nv12")
    with pytest.raises(ValueError, match="NV12 surfaces"):
        g.add_frames(ok, chunks, **nv)                              # three scenes listed, two rows
    with pytest.raises(ValueError, match="pitch"):
        g.add_frames(torch.zeros(2, 2, 192, 190, dtype=torch.uint8), chunks, scenes=[2, 0], **nv)
    with pytest.raises(ValueError, match="rows do not hold"):
        g.add_frames(torch.zeros(2, 2, 190, 194, dtype=torch.uint8), chunks, scenes=[2, 0], **nv)
    with pytest.raises(ValueError, match="uv_row=100"):
        g.add_frames(ok, chunks, scenes=[2, 0], uv_row=100, **nv)
    with pytest.raises(ValueError, match="chunk metas"):
        g.add_frames(ok, chunks[:1], scenes=[2, 0], **nv)
    with pytest.raises(ValueError, match="extrinsics"):
        g.add_frames(ok, [_chunk(meta, 2), _chunk(meta, 1)], scenes=[2, 0], **nv)
    with pytest.raises(ValueError, match="raw uint8 BGR frames"):
        g.add_frames(ok, chunks, scenes=[2, 0])
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        g.add_frames(ok, chunks, scenes=[2, 0], **nv)
