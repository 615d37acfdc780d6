"""Plain-torch CPU references of the projecting kernels, shared by the tests that hold K1 / K2 / K4 and their backward kernels to float64:
the oracle's nearest-pixel chain as one differentiable gather (with the depth gate), the bilinear sampler of the ray branch with its
float32 coordinate chain and float64 arithmetic, and the three gradient assertions of test_backward_shapes_gpu.py."""
import pytest
import torch

from oracle import nerfdet_oracle as O

HALF_ULP = 2.0 ** -41                             # deterministic scatter: rounding of one contribution
EPS32 = float(torch.finfo(torch.float32).eps)


def _check(got, ref, what, hits=None, tol=2e-5, etol=1e-4, atol=1e-6, floor=0.0):
    """The three assertions of the module docstring.  ``hits``: contributions per element (deterministic mode) or None; ``floor``: least
    scale (for a part of a gradient that may be zero)."""
    got, ref = got.detach().cpu().double(), ref.detach().double()
    assert got.shape == ref.shape, what
    scale = max(float(ref.abs().max()), floor)
    assert scale > 0, f"{what}: reference gradient is zero"
    slack = torch.zeros_like(ref) if hits is None else hits.double() * HALF_ULP
    err = (got - ref).abs()
    assert float(err.max()) <= tol * scale + float(slack.max()), f"{what}: max err {float(err.max()):.3e} vs scale {scale:.3e}"
    bound = etol * ref.abs() + atol * scale + slack
    bad = err > bound
    if bad.any():
        i = int(torch.argmax((err - bound).flatten()))
        pytest.fail(f"{what}: {int(bad.sum())} of {ref.numel()} elements out of bound; worst got {float(got.flatten()[i]):.6e} "
                    f"ref {float(ref.flatten()[i]):.6e}")
    # nonzero exactly where the reference is.  An entry below float32's resolution at the gradient's scale may come out 0 (1 - exp(-1e-12)
    # is 0 in float32, exp(-var) of a view far from the mean underflows), and the fixed point rounds an entry below its own slack to 0
    assert not (got[ref == 0] != 0).any(), f"{what}: {int((got[ref == 0] != 0).sum())} gradient entries where the reference has none"
    lost = (got == 0) & (ref.abs() > slack + EPS32 * scale)
    assert not lost.any(), f"{what}: {int(lost.sum())} entries the reference reaches are 0"


def _pixels(points, projection, h, w):
    """Pixel index (n_v, N) and validity of every voxel in every view, from the oracle's float32 projection chain."""
    fu, fv, z = O.project_voxels(points, projection)
    x, y = fu.round().long(), fv.round().long()
    valid = (x >= 0) & (y >= 0) & (x < w) & (y < h) & (z > 0)
    return x.clamp(0, w - 1), y.clamp(0, h - 1), z, valid


def _backproject64(feat, points, projection, dmap=None, band=None):
    """O.backproject as one differentiable gather; with ``dmap`` (n_v, h, w), the depth gate of nerfdet.py:404-411 against that
    already resized map (the resize itself is tested in test_depth_gate_gpu.py: here the kernel's own map is used so that both
    sides gate the same voxels).  Autograd through the oracle's per-view masked gather takes ~25 s at C = 320, 101 views on the
    CPU; the forward is checked equal to the oracle's instead."""
    n_v, c, h, w = feat.shape
    x, y, z, valid = _pixels(points, projection, h, w)
    if dmap is not None:
        dv = torch.gather(dmap.reshape(n_v, -1), 1, y * w + x)
        valid = valid & (z > dv - band) & (z < dv + band)
    idx = torch.arange(n_v).view(n_v, 1) * (h * w) + y * w + x
    rows = feat.permute(0, 2, 3, 1).reshape(n_v * h * w, c).index_select(0, idx.flatten()).view(n_v, -1, c)
    vol = torch.where(valid.unsqueeze(-1), rows, torch.zeros((), dtype=feat.dtype)).permute(0, 2, 1)
    vol, valid = vol.reshape(n_v, c, *points.shape[-3:]), valid.view(n_v, 1, *points.shape[-3:])
    if dmap is None:
        ov, ovalid = O.backproject(feat.detach(), points, projection)
        assert torch.equal(ovalid, valid) and torch.equal(ov, vol.detach())
    return vol, valid


def _hits(valid, points, projection, h, w):
    """Voxel-view pairs per feature pixel (n_v, h, w): the scatter contributions each gradient pixel of K1 / K2 receives."""
    x, y, _, _ = _pixels(points, projection, h, w)
    valid = valid.reshape(valid.shape[0], -1)
    out = torch.zeros(valid.shape[0], h * w, dtype=torch.int64)
    out.scatter_add_(1, (y * w + x), valid.long())
    return out.view(-1, h, w)


def _k4_ref(pts, ke, img_hw, feat):
    """projection.py:42-64 + 91-151 (bilinear sampling of the feature maps, zero padding, align_corners=True) and
    render_ray.py:71-93 (O.compute_mask_points).  The sample's source coordinate is the float32 chain of the kernels (KE rows as
    a k-ordered FMA chain: O.fma_chain_matmul); the bilinear weights and everything after are float64.  F.grid_sample itself
    cannot be used: it takes the grid in the map's dtype and would recompute the coordinate in float64.
    pts (n,3) float32, ke (n_v,3,4) float32, feat (n_v,d,hf,wf) float64 -> (mean (n,d), exp(-var) (n,d), mask (n,n_v), taps)."""
    n_v, d, hf, wf = feat.shape
    h, w = img_hw
    hom = torch.cat([pts.t(), torch.ones(1, pts.shape[0])]).numpy()[None]
    q = torch.from_numpy(O.fma_chain_matmul(ke.numpy(), hom))                    # (n_v, 3, n) float32
    den = q[:, 2].clamp(min=1e-8)
    px, py = (q[:, 0] / den).clamp(-1e6, 1e6), (q[:, 1] / den).clamp(-1e6, 1e6)
    mask = (px <= w - 1.0) & (px >= 0) & (py <= h - 1.0) & (py >= 0) & (q[:, 2] > 0)
    nx, ny = 2.0 * px / (w - 1.0) - 1.0, 2.0 * py / (h - 1.0) - 1.0
    ix = (((nx + 1) / 2) * (wf - 1)).double()                                    # grid_sample's source coordinate, float32
    iy = (((ny + 1) / 2) * (hf - 1)).double()
    x0, y0 = ix.floor(), iy.floor()
    flat = feat.permute(0, 2, 3, 1).reshape(-1, d)
    view = torch.arange(n_v).view(n_v, 1)
    val = torch.zeros(pts.shape[0], n_v, d, dtype=feat.dtype)
    taps = []
    for xt, yt, wt in ((x0, y0, (x0 + 1 - ix) * (y0 + 1 - iy)), (x0 + 1, y0, (ix - x0) * (y0 + 1 - iy)),
                       (x0, y0 + 1, (x0 + 1 - ix) * (iy - y0)), (x0 + 1, y0 + 1, (ix - x0) * (iy - y0))):
        inside = (xt >= 0) & (xt <= wf - 1) & (yt >= 0) & (yt <= hf - 1)
        # (a NaN coordinate -- a NaN or infinite point -- is inside no map: its tap is zero-padded like any other outside tap)
        idx = view * hf * wf + yt.clamp(0, hf - 1).nan_to_num(0.0).long() * wf + xt.clamp(0, wf - 1).nan_to_num(0.0).long()
        wt = torch.where(inside, wt, torch.zeros_like(wt))
        val = val + flat[idx.t()] * wt.t().unsqueeze(-1)
        taps.append((idx, wt))
    mk = mask.t().double().unsqueeze(-1)                                          # (n, n_v, 1)
    mean, ev = O.compute_mask_points(val.unsqueeze(1), mk.unsqueeze(1))
    return mean.view(-1, d), ev.view(-1, d), mask.t(), taps


def _k4_val(feat, taps):
    n_v, d, hf, wf = feat.shape
    flat = feat.permute(0, 2, 3, 1).reshape(-1, d)
    val = 0
    for idx, wt in taps:
        val = val + flat[idx.t()] * wt.t().unsqueeze(-1)
    return val
