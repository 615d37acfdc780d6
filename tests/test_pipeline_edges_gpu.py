"""k_normalize_views and k_target_rays (csrc/pipeline_kernels.hip) through nerfdet_amd.pipeline.MultiViewPipeline against the numpy oracle
(oracle/pipeline_oracle.py, which tests/test_pipeline_cpu.py pins bit for bit to the reference's MultiViewPipeline + DefaultFormatBundle:
mmdet3d/datasets/pipelines/multi_view.py:46-196, formating.py:33-117) at the shapes and settings the one golden scene does not have:

* frames that hold every byte value in every channel: the reference's uint8 round trip (imdenormalize(...).astype(uint8), multi_view.py:107-110)
  TRUNCATES, which at the default mean / std returns 31 of the 768 (value, channel) pairs one below what went in; the kernel must give exactly those;
* four mean / std sets.  For each the oracle's de-normalised float stays inside (-1, 256) for every byte (asserted below), so numpy's astype(uint8)
  and the kernel's (unsigned char)(int) are both defined and truncate alike;
* pixel and ray counts that are no multiple of the 256-thread workgroup (14 frames of 37 x 53), and one that is (24 x 32);
* margins 0, the largest that leaves one column (2 margin == W - 1) and one that leaves a single row;
* ``ids`` in descending order with repeats (what select_views draws with replacement), a target that is not among ``ids``, one target, every
  frame as a target.

The assertions are those of tests/test_pipeline_gpu.py::test_pipeline_batch_matches_reference."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

MEAN_STD = {
    "default": ((123.675, 116.28, 103.53), (58.395, 57.12, 57.375)),
    "identity": ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
    "spread": ((127.5, 0.25, 254.9), (0.37, 255.0, 3.3)),
    "extreme": ((1e-3, 200.0, 77.7), (1e-2, 1e3, 19.19)),
}
GEOMETRY = {
    # (H, W), margin, ori_h, ids, target ids
    "37x53-margin0-every-frame-a-target": ((37, 53), 0, 74, [13, 13, 9, 9, 4, 2, 2, 0], list(range(14))),
    "53x37-one-column-target-not-in-ids": ((53, 37), 18, 100, [5, 3, 3, 1], [7]),
    "37x53-one-row": ((37, 53), 18, 74, [0, 6, 11, 12], [12, 2, 12]),
    "24x32-margin3": ((24, 32), 3, 48, [11, 10, 10, 8, 1, 0, 0], [13, 10]),
}


@pytest.fixture(scope="module")
def g():
    z = np.load(os.path.join(GOLDEN, "pipeline_small.npz"))
    return {k: z[k] for k in z.files}


def _frames(hw, n=14):
    """uint8 BGR frames of random bytes; the first 256 pixels of every frame are a ramp through every byte value, rotated differently per channel
    and per frame, so every (value, channel) pair occurs in every frame and the three channels of a pixel differ."""
    h, w = hw
    assert h * w >= 256
    rng = np.random.RandomState(h * 1000 + w)
    f = rng.randint(0, 256, (n, h * w, 3)).astype(np.uint8)
    for i in range(n):
        for c in range(3):
            f[i, :256, c] = (np.arange(256) + 85 * c + 19 * i) % 256
    return f.reshape(n, h, w, 3)


def _round_trip(mean, std):
    """The oracle's de-normalised float (before the uint8 cast) for every byte value in every RGB channel: (256, 3) float32."""
    from oracle import pipeline_oracle as O
    mean, std = np.asarray(mean, np.float64), np.asarray(std, np.float64)
    ramp_bgr = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)[None]          # (1, 256, 3)
    norm = O.imnormalize(ramp_bgr, mean, std)
    return (norm * std.astype(np.float32) + mean.astype(np.float32))[0]


def test_reference_round_trip_truncates_31_pairs_at_the_default():
    """What the byte-ramp rows below rest on, on the CPU side: at the default mean / std the reference's round trip is off by one, downwards, for 31
    (value, channel) pairs -- so a kernel that rounded instead of truncating cannot pass them."""
    back = _round_trip(*MEAN_STD["default"])
    q = back.astype(np.uint8).astype(np.int64)
    want = np.repeat(np.arange(256)[:, None], 3, axis=1)
    assert int((q != want).sum()) == 31 and set((q - want)[q != want].tolist()) == {-1}
    assert np.array_equal(np.floor(back + 0.5).astype(np.int64), want), "rounding would return every byte"


@pytest.mark.parametrize("geometry", list(GEOMETRY))
@pytest.mark.parametrize("norm", list(MEAN_STD))
def test_pipeline_matches_oracle(device, g, norm, geometry):
    from nerfdet_amd import pipeline as P
    from oracle import pipeline_oracle as O
    mean, std = MEAN_STD[norm]
    hw, margin, ori_h, ids, tids = GEOMETRY[geometry]
    h, w = hw
    assert (14 * h * w) % 256 != 0 or hw == (24, 32)
    assert 2 * margin < min(h, w) and (margin != 18 or min(h, w) - 2 * margin == 1)
    back = _round_trip(mean, std)
    assert -1.0 < float(back.min()) and float(back.max()) < 256.0, "the uint8 cast must be defined for every byte"
    frames = _frames(hw)
    assert all(len(np.unique(frames[i, ..., c])) == 256 for i in range(14) for c in range(3))
    info = dict(extrinsics=list(g["poses"]), intrinsics=g["intrinsic"], annos=dict(axis_align_matrix=g["axis_align"]))
    ref = O.multi_view_batch(frames, O.scene_cameras(info), ids, tids, ori_h, mean, std, margin=margin)
    pipe = P.MultiViewPipeline(len(ids), mean=mean, std=std, margin=margin, nerf_target_views=len(tids))
    batch = pipe(torch.from_numpy(frames).to(device), P.scene_cameras(info), (ori_h, ori_h * w // h, 3), ids=ids, target_ids=tids)
    torch.cuda.synchronize()
    rays = (h - 2 * margin) * (w - 2 * margin)
    assert batch["img"].shape == (1, len(ids), 3, h, w) and batch["raydirs"].shape == (1, len(tids), rays, 3)
    assert ref["img"].dtype == np.float32 and ref["denorm_images"].dtype == np.float32 and ref["lightpos"].dtype == np.float32
    # exact: the normalised views, the de-normalised uint8 round trip, camera centres, view selection
    assert torch.equal(batch["img"][0].cpu(), torch.from_numpy(ref["img"]))
    assert torch.equal(batch["denorm_images"][0].cpu(), torch.from_numpy(ref["denorm_images"]))
    assert torch.equal(batch["lightpos"][0].cpu(), torch.from_numpy(ref["lightpos"]))
    assert np.array_equal(np.stack(batch["img_metas"][0]["lidar2img"]["extrinsic"]), ref["extrinsic"])
    gt = batch["gt_images"][0].cpu().double().numpy()
    assert gt.shape == ref["gt_images"].shape and np.abs(gt - ref["gt_images"]).max() <= 1e-7          # the oracle keeps float64 here
    rd = batch["raydirs"][0].cpu().numpy()
    assert np.abs(rd - ref["raydirs"]).max() <= 2e-7 * max(1.0, np.abs(ref["raydirs"]).max())
    assert [tuple(s[0].tolist()) for s in batch["nerf_sizes"]] == [tuple(r) for r in ref["nerf_sizes"]] == [(h - 2 * margin, w - 2 * margin, 3)] * len(tids)
    if margin == 0:            # the targets see the ramp too: every byte value, through k_target_rays' own round trip
        assert len(np.unique(np.round(ref["gt_images"] * 255))) == 256
