"""Plain restatements of hierarchical sampling (mmdet3d/models/model_utils/render_ray.py:96-142) for the importance-sampling tests,
written from the algorithm, not from the reference's text: the inverse-CDF draw with the uniforms ``u`` GIVEN, in float64
(:func:`sample_pdf64`) and in float32 torch with the reference's operation order (:func:`sample_pdf32`), the piecewise-linear CDF
evaluated at a depth (:func:`cdf64`), the bound the tests hold a draw to in CDF space (:func:`cdf_bound`), and the shared input
patterns."""
import numpy as np
import torch

FLOOR = 1e-5          # added to every weight, and the threshold below which a cdf step is not divided by (render_ray.py:106, 137)


def _cdf64(weights):
    w = weights.double() + FLOOR
    pdf = w / w.sum(dim=-1, keepdim=True)
    cdf = torch.cat([torch.zeros_like(pdf[:, :1]), torch.cumsum(pdf, dim=-1)], dim=-1)
    return pdf, cdf


def _rows(u, r):
    return u.reshape(1, -1).expand(r, -1) if u.dim() == 1 else u


def sample_pdf64(bins, weights, u):
    """float64 draw: ``bins`` (R, M+1), ``weights`` (R, M), ``u`` (R, N) or (N,) -> ``(samples (R, N), slope (R, N))`` where slope is
    d sample / d u = (bins[above] - bins[below]) / denom of the bin each sample fell into."""
    r, m = weights.shape
    _, cdf = _cdf64(weights)
    b, u = bins.double(), _rows(u.double(), r)
    above = (u.unsqueeze(-1) >= cdf[:, None, :m]).sum(dim=-1)
    below = (above - 1).clamp(min=0)
    c0, c1 = torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)
    b0, b1 = torch.gather(b, 1, below), torch.gather(b, 1, above)
    denom = c1 - c0
    denom = torch.where(denom < FLOOR, torch.ones_like(denom), denom)
    return b0 + (u - c0) / denom * (b1 - b0), (b1 - b0) / denom


def sample_pdf32(bins, weights, u):
    """The same draw in float32 torch, one rounding per operation in the reference's order (sum, divide, cumsum, count, gather, divide,
    multiply, add): what the reference computes for these uniforms.  ``weights`` is not modified."""
    r, m = weights.shape
    w = weights.float() + FLOOR
    pdf = w / torch.sum(w, dim=-1, keepdim=True)
    cdf = torch.cumsum(pdf, dim=-1)
    cdf = torch.cat([torch.zeros_like(cdf[:, :1]), cdf], dim=-1)
    b, u = bins.float(), _rows(u.float(), r)
    above = (u.unsqueeze(-1) >= cdf[:, None, :m]).sum(dim=-1)        # an integer count: exact
    below = (above - 1).clamp(min=0)
    c0, c1 = torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)
    b0, b1 = torch.gather(b, 1, below), torch.gather(b, 1, above)
    denom = c1 - c0
    denom = torch.where(denom < FLOOR, torch.ones_like(denom), denom)
    t = (u - c0) / denom
    return b0 + t * (b1 - b0)


def cdf64(bins, weights, z):
    """The piecewise-linear CDF the weights give over the bins, evaluated at depths ``z`` (R, N) in float64; 0 below bins[0], cdf[M]
    above bins[M].  Bins strictly increasing."""
    r, m = weights.shape
    pdf, cdf = _cdf64(weights)
    b, z = bins.double().contiguous(), z.double().contiguous()
    k = (torch.searchsorted(b, z, right=True) - 1).clamp(0, m - 1)
    b0, b1 = torch.gather(b, 1, k), torch.gather(b, 1, k + 1)
    t = ((z - b0) / (b1 - b0)).clamp(0.0, 1.0)
    return torch.gather(cdf, 1, k) + t * torch.gather(pdf, 1, k)


def cdf_bound(m):
    """|cdf64(sample) - u| <= 1e-5 + (M + 4) * 2^-24.  First term: where a cdf step is below 1e-5 the reference does not divide, so the
    sample sits at cdf[below] + (u - cdf[below]) * step, within step < 1e-5 of u.  Second: the rounding of an M-term positive running
    sum (each partial sum <= 1, half an ulp of 1 = 2^-24 per add in any order) and of its normalisation."""
    return FLOOR + (m + 4) * 2.0 ** -24


# ---- inputs ----
SHAPES = [(3, 1), (5, 7), (40, 64), (64, 128), (256, 256)]      # (S, n_imp); M = S - 2
RAY_COUNTS = [1, 4, 5, 1003]
NEAR, FAR = 0.2, 8.0


def coarse_depths(r, s, seed, jitter=True):
    """(R, S) ascending depths in [NEAR, FAR]: the uniform lattice, with ``jitter`` moved by up to a quarter step so that the bins differ in width."""
    g = torch.Generator().manual_seed(seed)
    z = torch.linspace(NEAR, FAR, s).reshape(1, s).repeat(r, 1)
    if jitter:
        step = (FAR - NEAR) / (s - 1)
        z = z + (torch.rand(r, s, generator=g) - 0.5) * 0.5 * step
    return z.float().contiguous()


def mid_bins(z):
    return 0.5 * (z[:, 1:] + z[:, :-1])


WEIGHT_PATTERNS = ["uniform", "zero", "onehot_first", "onehot_mid", "onehot_last", "ramp", "plateau"]


def weights_of(pattern, r, m, seed):
    """(R, M) weights: uniform random, all zero (the floor alone), one-hot on the first / a middle / the last bin, a 1e-6 .. 1 ramp, and
    'plateau' = uniform in [0.2, 1] (well conditioned: used where depths are compared)."""
    g = torch.Generator().manual_seed(seed)
    if pattern == "uniform":
        return torch.rand(r, m, generator=g)
    if pattern == "zero":
        return torch.zeros(r, m)
    if pattern.startswith("onehot"):
        w = torch.zeros(r, m)
        w[:, onehot_bin(pattern, m)] = 1.0
        return w
    if pattern == "ramp":
        return torch.logspace(-6, 0, m).reshape(1, m).repeat(r, 1).contiguous() if m > 1 else torch.full((r, 1), 1e-6)
    if pattern == "plateau":
        return 0.2 + 0.8 * torch.rand(r, m, generator=g)
    raise KeyError(pattern)


def onehot_bin(pattern, m):
    return {"onehot_first": 0, "onehot_mid": m // 2, "onehot_last": m - 1}[pattern]


U_PATTERNS = ["det", "random", "ends"]


def uniforms_of(pattern, r, n, seed):
    """'det': torch.linspace(0, 1, n) as one shared row; 'random': (R, n) torch.rand; 'ends': random rows whose first entry is exactly
    0.0 and, from two entries on, whose last is exactly 1.0."""
    g = torch.Generator().manual_seed(seed)
    if pattern == "det":
        return torch.linspace(0., 1., n)
    u = torch.rand(r, n, generator=g)
    if pattern == "ends":
        u[:, 0] = 0.0
        if n > 1:
            u[:, -1] = 1.0
    return u


def as_np(**tensors):
    return {k: (v.numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in tensors.items()}
