"""CPU side of the depth-frame path: the oracle of tests/depth_frames_ref.py is what the datasets chain produces, its inputs tell the
kernel's arithmetic from its near misses, and the new entry points exist and refuse bad arguments before any device work.

Outputs of frame 0 that differ from the oracle, of 704 - 768 a frame (printed by the test):
  multiply by 0.001                  71 - 100   (every case, the copy too)
  float32 interpolation              658 - 734
  contracted, non-integer sizes      171 - 181
  contracted, ratio 2 and the copy   0          (f is 0.5 or 0: the products are exact)

Condition of the inputs, asserted here: in every case 0 < K < number of rays (some resized pixels are exactly 0, most are not), so
``depth_rays`` is neither empty nor the identity."""
import ctypes

import numpy as np
import pytest
import torch

import depth_frames_ref as D


def _all_cases():
    for key, (size, out) in D.CASES.items():
        yield key, size, out
    (size, outs) = D.CAPTURE
    for h, w, _ in outs:
        yield f"480x640-to-{h}x{w}", size, (h, w)


def test_oracle_is_what_the_datasets_chain_produces(tmp_path):
    """A hand-made ``results`` dict whose depth PNGs hold the oracle's frames: ``MultiViewPipeline._depth`` per view (to ``img_shape``) and
    per target (to the padded image's shape, then the pixel grid), ``DefaultFormatBundle3D`` on top."""
    from PIL import Image
    from nerfdet_amd import datasets as DS
    size, (hr, wr) = D.CASES["30x41-noninteger"]
    h, w, m = 24, 32, 2
    fr = D.frames(size)
    ids, tids = [13, 13, 9, 4, 0], [7, 2]
    infos = []
    for i in range(len(fr)):
        name = str(tmp_path / f"{i}.png")
        Image.fromarray(np.array(fr[i])).save(name)
        assert np.array_equal(np.asarray(Image.open(name)), fr[i])
        infos.append(dict(filename=name))
    pipe = DS.MultiViewPipeline([], len(ids), margin=m, nerf_target_views=len(tids))
    px, py = np.meshgrid(np.arange(m, w - m).astype(np.float32), np.arange(m, h - m).astype(np.float32))   # multi_view.py:124-132
    iy, ix = py.astype(np.int32), px.astype(np.int32)
    rays = (h - 2 * m) * (w - 2 * m)
    results = dict(depth=[pipe._depth(infos[i], (hr, wr, 3)) for i in ids],
                   gt_depths=[pipe._depth(infos[i], (h, w, 3))[iy, ix] for i in tids], ray_info=True,
                   raydirs=[np.zeros((rays, 3), np.float32)] * len(tids), lightpos=[np.zeros(3, np.float32)] * len(tids),
                   gt_images=[np.zeros((rays, 3))] * len(tids), denorm_images=[np.zeros((h, w, 3))] * len(ids))
    out = DS.DefaultFormatBundle3D(class_names=())(results)
    ref = D.batch(fr, ids, tids, (hr, wr), (h, w), m)
    assert out["depth"].dtype == torch.float64 and torch.equal(out["depth"], torch.from_numpy(ref["depth"][0]))
    assert out["gt_depths"].dtype == torch.float64 and torch.equal(out["gt_depths"], torch.from_numpy(ref["gt_depths"][0]))
    assert out["depth_rays"].dtype == torch.int64 and torch.equal(out["depth_rays"], torch.from_numpy(ref["depth_rays"][0]))
    assert ref["gt_depths"].shape == (1, len(tids), h - 2 * m, w - 2 * m) and ref["depth_rays"].shape[0] == 1


@pytest.mark.parametrize("case", [c[0] for c in _all_cases()])
def test_inputs_tell_the_arithmetic_from_its_near_misses(case):
    """Frame 0 of each case: multiplying by 0.001 and interpolating in float32 differ from the oracle on every case but the copy; the
    contracted form differs on the non-integer sizes and is the oracle's on ratio 2 and the copy (f = 0.5 or 0: the products are exact)."""
    key, size, (h, w) = next(c for c in _all_cases() if c[0] == case)
    fr = D.frames(size, 2) if size == D.CAPTURE[0] else D.frames(size)
    ref = D.resize(fr[:1], (h, w))[0]
    k = int((ref > 0).sum())
    assert 0 < k < ref.size, (case, k)                      # condition of the inputs
    mul = int((D.variant_multiply(fr[0], (h, w)) != ref).sum())
    f32 = int((D.variant_float32(fr[0], (h, w)) != ref).sum())
    print(f"{case}: {ref.size} outputs, K = {k}; multiply-by-0.001 differs in {mul}, float32 in {f32}")
    if "copy" in case:
        assert np.array_equal(ref, fr[0] / 1000)
    else:
        assert mul > 0 and f32 > 0, (case, mul, f32)
    if size != D.CAPTURE[0]:                                # the rational emulation is per pixel: the small cases only
        con = int((D.variant_contracted(fr[0], (h, w)) != ref).sum())
        print(f"{case}: contracted differs in {con}")
        assert (con > 0) == (key in D.NONINTEGER), (case, con)


def test_margin_crop_keeps_some_zero_and_some_positive_rays():
    for key, (size, (h, w)) in D.CASES.items():
        for m in D.MARGINS:
            for ids in D.IDS.values():
                x = D.resize(D.frames(size), (h, w), ids, m)
                assert x.shape[1:] == (h - 2 * m, w - 2 * m) and 0 < int((x > 0).sum()) < x.size, (key, m)


def test_new_entry_points_refuse_bad_arguments_without_a_gpu():
    from nerfdet_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)
    df = lib.ndet_depth_frames
    assert df(fake, None, 2, 30, 41, 22, 32, 0, None, None) == -1 and b"null" in lib.ndet_last_error()
    assert df(None, None, 2, 30, 41, 22, 32, 0, fake, None) == -1
    for bad in ((0, 30, 41, 22, 32), (2, 0, 41, 22, 32), (2, 30, 0, 22, 32), (2, 30, 41, 0, 32), (2, 30, 41, 22, -1)):
        assert df(fake, None, *bad, 0, fake, None) == -1, bad
    assert df(fake, None, 2, 30, 41, 22, 32, 11, fake, None) == -1 and b"margin" in lib.ndet_last_error()      # 22 - 2 * 11 rows
    assert df(fake, None, 2, 30, 41, 22, 32, 16, fake, None) == -1
    assert df(fake, None, 2, 30, 41, 22, 32, -1, fake, None) == -1
    assert df(fake, None, 2, 1 << 16, 1 << 15, 22, 32, 0, fake, None) == -2                                       # a frame of 2^31 elements
    assert df(fake, None, 2, 30, 41, 1 << 16, 1 << 15, 0, fake, None) == -2                                       # a map of 2^31 elements
    pi, wsb = lib.ndet_positive_indices, lib.ndet_positive_indices_workspace_bytes
    for k in (0, 2, 3, 4):                  # x, indices, count, workspace
        args = [fake, 100, fake, fake, fake, None]
        args[k] = None
        assert pi(*args) == -1 and b"null" in lib.ndet_last_error(), k
    assert pi(fake, 0, fake, fake, fake, None) == -1 and pi(fake, -5, fake, fake, fake, None) == -1
    assert pi(fake, 100, fake, fake, ctypes.c_void_p(0x1008), None) == -1                                        # a misaligned workspace
    assert pi(fake, 1 << 31, fake, fake, fake, None) == -2 and pi(fake, 1 << 40, fake, fake, fake, None) == -2
    assert wsb(0) == 0 and wsb(1 << 31) == 0
    for n in (1, 255, 256, 257, 660000, (1 << 31) - 1):
        tiles = (n + 255) // 256
        assert wsb(n) % 16 == 0 and wsb(n) >= 8 * (2 + tiles), n


def test_python_wrappers_refuse_before_any_device_work():
    from nerfdet_amd import pipeline as P
    good = torch.zeros((3, 30, 41), dtype=torch.uint16)
    for bad in (good, good.to(torch.int32), torch.zeros((3, 30, 41), dtype=torch.float32), torch.zeros((30, 41), dtype=torch.uint16), None):
        with pytest.raises(ValueError, match="uint16"):
            P.prepare_depth_frames(bad, (22, 32))           # a CPU tensor, other dtypes, a 2-D tensor, not a tensor
