"""The numpy oracle of the raw-frame path (ndet_resize_normalize_views, pipeline.prepare_frames, MultiViewPipeline(img_scale=, pad_size=),
add_frames): the configs' chain, link by link, from frames at capture resolution --

  1. datasets.imresize_linear                       Resize(keep_ratio=True): the project's definition of the resize
  2. oracle.pipeline_oracle.imnormalize             Normalize(to_rgb=True)
  3. a zero pad of the float image                  Pad(size=pad_size), after Normalize
  4. imdenormalize_u8(...) / 255                    the reference's de-normalised copy (multi_view.py:107-110)
  5. the ray part of oracle.pipeline_oracle.multi_view_batch with ratio = Hs / Hr over the padded grid (multi_view.py:113-155)

Test infrastructure only."""
import numpy as np

from oracle import pipeline_oracle as O

# capture size, img_scale (w, h), resized size, pad size: what each exercises is in tests/test_raw_frames_gpu.py
SIZES = {
    "37x53-down-bottom-pad": ((37, 53), (32, 24), (22, 32), (24, 32)),
    "100x129-right-pad": ((100, 129), (32, 24), (24, 31), (24, 32)),
    "19x23-upscale": ((19, 23), (32, 24), (24, 29), (24, 32)),
    "24x32-copy": ((24, 32), (32, 24), (24, 32), (24, 32)),
    "97x131-no-pad": ((97, 131), (32, 24), (24, 32), (24, 32)),
}


def resized_size(size_hw, img_scale):
    """(Hr, Wr) as datasets.Resize(keep_ratio=True) itself reports it (img_shape of a zero frame)."""
    from nerfdet_amd.datasets import Resize
    out = Resize(img_scale=img_scale, keep_ratio=True)(dict(img=np.zeros(tuple(size_hw) + (3,), np.uint8)))
    return tuple(out["img_shape"][:2])


def prepare(frames_u8_bgr, img_scale, pad_size, mean, std, ids=None):
    """Links 1-4 for frames (n, Hs, Ws, 3): ``u8 (n_sel, H, W, 3)`` resized bytes zero-padded, ``img`` and ``denorm`` (n_sel, 3, H, W)
    float32, and ``resized_hw``.  Each distinct frame is resized once."""
    from nerfdet_amd.datasets import imresize_linear
    mean, std = np.asarray(mean, np.float64), np.asarray(std, np.float64)
    hs, ws = frames_u8_bgr.shape[1:3]
    hr, wr = resized_size((hs, ws), img_scale)
    h, w = pad_size
    ids = list(range(len(frames_u8_bgr))) if ids is None else [int(i) for i in ids]
    one = {}
    for i in set(ids):
        r = imresize_linear(frames_u8_bgr[i], (wr, hr))
        norm = np.zeros((h, w, 3), np.float32)
        norm[:hr, :wr] = O.imnormalize(r, mean, std)
        u8 = np.zeros((h, w, 3), np.uint8)
        u8[:hr, :wr] = r
        bgr = O.imdenormalize_u8(norm, mean, std)
        one[i] = (u8, norm, bgr)
    return dict(u8=np.stack([one[i][0] for i in ids]), img=np.stack([one[i][1].transpose(2, 0, 1) for i in ids]),
                denorm=np.stack([(one[i][2] / 255.0).transpose(2, 0, 1) for i in ids]).astype(np.float32),
                bgr=np.stack([one[i][2] for i in ids]), resized_hw=(hr, wr))


def batch(frames_u8_bgr, cams, ids, target_ids, img_scale, pad_size, mean, std, margin):
    """What the datasets chain + MultiViewPipeline + DefaultFormatBundle make of raw frames: the keys of O.multi_view_batch."""
    hs = frames_u8_bgr.shape[1]
    h, w = pad_size
    src = prepare(frames_u8_bgr, img_scale, pad_size, mean, std, ids)
    out = dict(img=src["img"], denorm_images=src["denorm"], extrinsic=np.stack([cams["extrinsic"][int(i)] for i in ids]), resized_hw=src["resized_hw"])
    if len(target_ids):
        tgt = prepare(frames_u8_bgr, img_scale, pad_size, mean, std, target_ids)
        ratio = hs / src["resized_hw"][0]
        k = cams["intrinsic"].copy()
        k[:2] = k[:2] / ratio
        px, py = np.meshgrid(np.arange(margin, w - margin).astype(np.float32), np.arange(margin, h - margin).astype(np.float32))
        pix = np.stack((px, py), axis=-1).astype(np.float32)
        rays, lights, gts, sizes = [], [], [], []
        for j, t in enumerate(target_ids):
            rays.append(np.reshape(O.get_dtu_raydir(pix, k, cams["camrotc2w"][int(t)]).astype(np.float32), (-1, 3)))
            g = tgt["bgr"][j][py.astype(np.int32), px.astype(np.int32), :]
            sizes.append(np.array(g.shape))
            gts.append(np.reshape(g, (-1, 3)) / 255.0)
            lights.append(cams["lightpos"][int(t)])
        rays = np.stack(rays)
        out.update(raydirs=rays, gt_images=np.stack(gts), nerf_sizes=np.stack(sizes),
                   lightpos=np.repeat(np.stack(lights)[:, None, :], rays.shape[1], axis=1))
    return out


def float_bilinear(frame_u8, size_wh):
    """Exact bilinear interpolation with float64 taps and round-to-nearest: what a floating-point resize would give."""
    nw, nh = size_wh
    h, w = frame_u8.shape[:2]

    def taps(n_dst, n_src):
        f = (np.arange(n_dst, dtype=np.float64) + 0.5) * (n_src / n_dst) - 0.5
        s = np.floor(f).astype(np.int64)
        f = f - s
        f[s < 0], s[s < 0] = 0.0, 0
        hi = s >= n_src - 1
        f[hi], s[hi] = 0.0, n_src - 1
        return s, np.minimum(s + 1, n_src - 1), f
    x0, x1, fx = taps(nw, w)
    y0, y1, fy = taps(nh, h)
    rows = frame_u8.astype(np.float64)
    hor = rows[:, x0] * (1 - fx)[None, :, None] + rows[:, x1] * fx[None, :, None]
    out = hor[y0] * (1 - fy)[:, None, None] + hor[y1] * fy[:, None, None]
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)
