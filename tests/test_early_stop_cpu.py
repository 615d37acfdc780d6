"""Early ray termination without a GPU: the entry points exist and refuse bad arguments on the host before any HIP call
(csrc/early_stop_kernels.hip), the numpy restatement of the keep rule (tests/early_stop_ref.py) agrees with brute force, and the Python
layer refuses bad knobs before it touches a tensor."""
import ctypes

import numpy as np
import pytest

import early_stop_ref as E
import skip_empty_ref as SE

INVALID, UNSUPPORTED = -1, -2
FAKE = ctypes.c_void_p(0x1000)
ODD = ctypes.c_void_p(0x1001)
OFF4 = ctypes.c_void_p(0x1004)      # 4-byte aligned, not 16


def _lib():
    from nerfdet_amd import _lib
    return _lib, _lib.load()


def _i3(*v):
    return (ctypes.c_int * 3)(*v)


def test_entry_points_exist():
    L, lib = _lib()
    for name in ("ndet_ray_advance", "ndet_front_blocks", "ndet_front_count", "ndet_front_write"):
        assert name in L.SIGNATURES and hasattr(lib, name)
    assert lib.ndet_version() == 110          # an added entry point does not move the ABI version
    from nerfdet_amd import rays, streaming
    assert callable(rays.advance_transmittance) and callable(rays.front_segment)
    assert callable(streaming._front_shade) and callable(streaming._render_passes_stopped)
    assert streaming.EARLY_STOP_DEFAULTS["eps"] == 1e-3 and streaming.EARLY_STOP_DEFAULTS["segment"] in (4, 8, 16, 32)


@pytest.mark.parametrize("w", list(range(1, 33)))
def test_front_blocks(w):
    """A block of rays is 512 / nominal rays, nominal the least of 4, 8, 16, 32 that holds w."""
    _, lib = _lib()
    per = 512 // (4 if w <= 4 else 8 if w <= 8 else 16 if w <= 16 else 32)
    assert [lib.ndet_front_blocks(r, w) for r in (-1, 0, 1, per, per + 1)] == [0, 0, 1, 1, 2]
    assert [E.front_blocks(r, w) for r in (-1, 0, 1, per, per + 1, 1000)] == [lib.ndet_front_blocks(r, w) for r in (-1, 0, 1, per, per + 1, 1000)]


def test_front_blocks_of_a_bad_width():
    _, lib = _lib()
    assert [lib.ndet_front_blocks(100, w) for w in (-1, 0, 33)] == [0, 0, 0]


def test_advance_host_checks():
    _, lib = _lib()
    ok = dict(raw=FAKE, T=FAKE, R=100, S=64, s0=16, s1=32)

    def call(**bad):
        a = dict(ok, **bad)
        return lib.ndet_ray_advance(a["raw"], a["T"], a["R"], a["S"], a["s0"], a["s1"], None)

    for key in ("raw", "T"):
        assert call(**{key: None}) == INVALID and b"null" in lib.ndet_last_error()
    for key in ("R", "S"):
        assert call(**{key: 0}) == INVALID and call(**{key: -3}) == INVALID
    assert call(s0=-1) == INVALID and call(s1=65) == INVALID and call(s0=33, s1=32) == INVALID
    assert b"columns" in lib.ndet_last_error()
    assert call(R=1 << 20, S=1 << 11, s0=0, s1=4) == UNSUPPORTED and b"2^31" in lib.ndet_last_error()
    assert call(raw=ODD) == UNSUPPORTED and call(raw=OFF4) == UNSUPPORTED and b"16-byte" in lib.ndet_last_error()
    assert call(T=ODD) == UNSUPPORTED and b"misaligned" in lib.ndet_last_error()
    # s0 == s1 is a no-op that launches nothing: it returns NDET_OK on a machine without a device, fake pointers and all
    assert call(s0=32, s1=32) == 0 and call(s0=0, s1=0) == 0 and call(s0=64, s1=64) == 0
    # (2^24 workgroups of 256 rays lie beyond 2^31 samples, which are refused first: the bound guards the block size)


@pytest.mark.parametrize("write", [False, True])
@pytest.mark.parametrize("grid", [False, True])
def test_front_host_checks(write, grid):
    _, lib = _lib()
    from nerfdet_amd._lib import float3
    ok = dict(pts=FAKE, R=100, S=64, s0=16, s1=32, T=FAKE, eps=1e-3, bits=FAKE if grid else None, nv=_i3(4, 4, 4) if grid else None,
              p0=float3([0, 0, 0]) if grid else None, vs=float3([.1, .1, .1]) if grid else None, outside=0, a=FAKE, b=FAKE, c=FAKE)

    def call(**bad):
        a = dict(ok, **bad)
        head = (a["pts"], a["R"], a["S"], a["s0"], a["s1"], a["T"], a["eps"], a["bits"], a["nv"], a["p0"], a["vs"], a["outside"])
        if write:
            return lib.ndet_front_write(*head, a["a"], a["b"], a["c"], None)
        return lib.ndet_front_count(*head, a["a"], None)

    outs = ("a", "b", "c") if write else ("a",)
    for key in ("pts", "T") + outs:
        assert call(**{key: None}) == INVALID and b"null" in lib.ndet_last_error(), key
    for key in ("R", "S"):
        assert call(**{key: 0}) == INVALID and call(**{key: -3}) == INVALID
    assert call(s0=-1) == INVALID and call(s1=65) == INVALID and call(s0=33, s1=32) == INVALID
    assert call(s0=32, s1=32) == INVALID and b"columns" in lib.ndet_last_error()          # an empty segment
    for eps in (float("nan"), -1e-3, 1.0, float("inf"), -float("inf")):
        assert call(eps=eps) == INVALID and b"eps" in lib.ndet_last_error(), eps
    if grid:      # the lattice's knobs, as ndet_cull_count rejects them
        for key in ("nv", "p0", "vs"):
            assert call(**{key: None}) == INVALID and b"null" in lib.ndet_last_error(), key
        assert call(nv=_i3(4, 0, 4)) == INVALID
        for vs in ([.1, 0.0, .1], [.1, .1, -1.0], [float("nan"), .1, .1], [.1, float("inf"), .1]):
            assert call(vs=float3(vs)) == INVALID and b"voxel size" in lib.ndet_last_error()
        assert call(p0=float3([0, float("nan"), 0])) == INVALID
        for outside in (-1, 2):
            assert call(outside=outside) == INVALID and b"outside" in lib.ndet_last_error()
        assert call(nv=_i3(2048, 1024, 1024)) == UNSUPPORTED and b"2^31" in lib.ndet_last_error()
        assert call(bits=ODD) == UNSUPPORTED and b"misaligned" in lib.ndet_last_error()
    assert call(s0=16, s1=49) == UNSUPPORTED and b"32" in lib.ndet_last_error()          # w = 33
    assert call(R=1 << 20, S=1 << 11) == UNSUPPORTED and b"2^31" in lib.ndet_last_error()
    for key in ("pts", "T") + outs:
        assert call(**{key: ODD}) == UNSUPPORTED and b"misaligned" in lib.ndet_last_error(), key
    # (2^24 workgroups of at least 64 rays lie beyond 2^31 samples, which are refused first: the bound guards the block size)


# ---- the restatement against brute force ----
@pytest.mark.parametrize("with_grid", [False, True])
def test_restatement_against_brute_force(with_grid):
    nv, p0, vs = (5, 3, 7), np.float32([-0.4, 0.3, 1.0]), np.float32([0.16, 0.2, 0.1])
    alpha, count, thr = SE.grid_case(nv, 5)
    bits = SE.occupancy_bits(alpha, count, nv, thr, 0)
    rng = np.random.RandomState(3)
    r, s, eps = 7, 11, np.float32(1e-3)
    pts = ((rng.rand(r, s, 3).astype(np.float32) * 9 - 2) * vs + p0).astype(np.float32)
    pts[2, 5, 1] = np.nan
    T = np.float32([1.0, 1e-4, eps, np.nan, np.nextafter(eps, np.float32(0)), np.nextafter(eps, np.float32(1)), 0.0])
    for outside in ("keep", "cull"):
        grid = (bits, nv, p0, vs, outside) if with_grid else None
        n_kept = 0
        for s0, s1 in ((0, 4), (4, 8), (8, 11), (0, 11)):
            idx, kept = E.front(pts, T, s0, s1, eps, grid)
            want = []
            for ray in range(r):
                for col in range(s1 - s0):
                    f = ray * s + s0 + col
                    if T[ray] < eps:                     # False for the NaN
                        continue
                    if with_grid:
                        p = pts.reshape(-1, 3)[f]
                        with np.errstate(invalid="ignore"):
                            fl = [np.floor(np.float32(np.float32((p[k] - p0[k]) / vs[k]) + np.float32(0.5))) for k in range(3)]
                        inside = all(np.isfinite(p)) and all(0 <= fl[k] < nv[k] for k in range(3))
                        if inside:
                            n = (int(fl[0]) * nv[1] + int(fl[1])) * nv[2] + int(fl[2])
                            keep = bool((bits.view(np.uint32)[n >> 5] >> np.uint32(n & 31)) & 1)
                        else:
                            keep = outside == "keep"
                        if not keep:
                            continue
                    want.append(f)
            assert idx.dtype == np.int32 and np.array_equal(idx, np.int32(want)), (outside, s0, s1)
            assert np.array_equal(kept, pts.reshape(-1, 3)[want], equal_nan=True)
            assert len(want) < r * (s1 - s0)
            n_kept += len(want)
        assert n_kept > 0, outside
    # the live rays: below eps stops, eps itself and NaN do not
    assert E.live(T, eps).tolist() == [True, False, True, True, False, True, False]


# ---- the Python layer refuses before it touches a tensor ----
def test_knobs_are_checked_before_any_launch():
    import torch
    from nerfdet_amd import rays, streaming
    for eps in (-1e-3, 1, float("nan"), float("inf"), "x", True, None):
        with pytest.raises(ValueError, match="eps"):
            streaming._stop_knobs(dict(eps=eps), "render_rays")
    for segment in (0, 3, 64, 8.0, True, "8"):
        with pytest.raises(ValueError, match="segment"):
            streaming._stop_knobs(dict(segment=segment), "render_rays")
    for bad in (dict(epsilon=1e-3), dict(eps=1e-3, width=8), 3, "yes", 1e-3):
        with pytest.raises(ValueError):
            streaming._stop_knobs(bad, "render_rays")
    assert streaming._stop_knobs(None, "render_rays") is None and streaming._stop_knobs(False, "render_rays") is None
    assert streaming._stop_knobs(True, "render_rays") == streaming.EARLY_STOP_DEFAULTS
    assert streaming._stop_knobs(dict(eps=0, segment=np.int64(4)), "render_rays") == dict(eps=0.0, segment=4)
    assert streaming._stop_knobs(dict(segment=32), "render_rays") == dict(eps=1e-3, segment=32)
    import types
    det = types.SimpleNamespace(training=False)
    with pytest.raises(ValueError, match="batched"):
        streaming._stop_checked(det, True, "render_rays", batched=True)
    assert streaming._stop_checked(det, None, "render_rays", batched=True) is None
    with pytest.raises(RuntimeError, match=r"render_rays\(early_stop=\): the rays must live on the GPU"):
        streaming._stop_checked(det, True, "render_rays", torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match=r"render\(early_stop=\) is inference only"):
        streaming._stop_checked(types.SimpleNamespace(training=True), True, "render")
    with pytest.raises(RuntimeError, match="GPU"):
        rays.front_segment(torch.zeros(4, 8, 3), torch.ones(4), 0, 4, 1e-3)
    with pytest.raises(RuntimeError, match="GPU"):
        rays.advance_transmittance(torch.zeros(4, 8, 4), torch.ones(4), 0, 4)
