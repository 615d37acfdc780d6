"""float64 references, seeded inputs and error bars for the forward kernels of the NeRF ray branch: the sampler (k_sample_rays), the
compositor (k_composite), the radiance MLP at inference (forward_rows_hip: k_point_mlp or k_posenc_concat + linear_rows + k_sigma_head)
and the small A6 kernels.  No GPU in here: tests/test_ray_forward_ref_cpu.py runs it against the recorded goldens and asserts the table
below; tests/test_ray_forward_gpu.py holds the kernels to it.

References.  The sampler and the compositor are ``oracle.sample_along_camera_ray`` / ``oracle.raw2outputs`` handed float64 tensors.
The encoders are NOT the oracle's in float64: the operation is defined with float32 arguments -- ``x * 2^k`` is exact and
``+ float32(pi / 2)`` is one float32 rounding (nerf_mlp.py:190-194, the same in k_posenc_concat and k_point_mlp) -- so
:func:`encode_f32args` rounds the arguments that way and takes the sine, and everything after it, in float64.  A pure-float64 encoder
differs from it by the rounding of that sum: up to 4.45e-6 for points in +-8, 30 times the encoder's bar below, which would hide or fake
errors of that size.  (Half an ulp of the argument at |x| = 8, k = 9 would be 2.4e-4; it is never reached, because pi / 2
lies 4.45e-6 below a multiple of 2^-12 and so rounds that little on every grid from 2^-17 up: the CPU test asserts the 4.45e-6.)

Inputs.  Every builder is seeded and is shared by the CPU and the GPU tests; none filters its result after the fact.
Compositing sigmas are one of 0, 1e-12, a value in [1e-3, 16], or 40, nothing else: between about 3e-8 and 1e-6 ``1 - exp(-sigma)`` is 0
in float32 and not in float64, so a ray made of such samples is clamped in one arithmetic and not in the other, and between 16 and 40 the
transmittance behind the sample differs by orders of magnitude for the same reason (tests/test_backward_shapes_gpu.py::
test_composite_backward_vs_fp64).  Those are properties of float32, not of the kernel, and are excluded by construction.

Bars.  Quantities the project already holds to a bar keep it: 2e-5 absolute on colours, depths and statistics (test_rays_gpu.ATOL), the
trunk output within 1e-5 of its row maximum, raw sigma within 2e-5 (1 + |sigma|), alpha within 1e-5 (test_fused_point_mlp_*).  For the
others the FLOAT32 CPU RESTATEMENT (the oracle function in float32) is measured against float64 on the very inputs of each case:
``floor`` below is the worst such error over the cases of a row, and the bar is ``max(4 * floor, 2^-23 * magnitude)``, magnitude = ``far``
for z and 1 for weights, alpha, transparency, rgb and sines.  4: a kernel may sum in another valid order and the device's expf / sinf
differ from the host's by ulps; a missing term or a shifted sample index shows at 1e-3 or more.  The rgb bar is capped at the 1e-4 of
BASELINE's north star.  The table holds the figures of the machine it was written on.  The float32 restatement's own error moves
between CPUs, because torch vectorises cumprod, sums, GEMMs and exp by the vector width (the transparency of (65, 64): 9.3e-8 on one
machine, 1.5e-7 on another), so the CPU test recomputes every floor and holds it to [floor / 4, bar]: on any machine the reference alone
passes, and no row of the table is more than four times what is measured.  It asserts each bar from its floor.

    quantity                                floor      bar
    --------------------------------------------------------
    sampler_z (0.2, 8.0)                  7.10e-07  2.84e-06
    sampler_z (0.05, 0.051)               4.80e-09  1.92e-08
    composite_weights (1, 1)              2.70e-08  1.19e-07
    composite_alpha (1, 1)                2.70e-08  1.19e-07
    composite_transparency (1, 1)         0.00e+00  1.19e-07
    composite_weights (63, 2)             4.30e-08  1.72e-07
    composite_alpha (63, 2)               4.30e-08  1.72e-07
    composite_transparency (63, 2)        4.30e-08  1.72e-07
    composite_weights (64, 9)             6.70e-08  2.68e-07
    composite_alpha (64, 9)               4.50e-08  1.80e-07
    composite_transparency (64, 9)        6.20e-08  2.48e-07
    composite_weights (65, 64)            4.50e-08  1.80e-07
    composite_alpha (65, 64)              4.60e-08  1.84e-07
    composite_transparency (65, 64)       9.30e-08  3.72e-07
    composite_weights (130, 80)           5.90e-08  2.36e-07
    composite_alpha (130, 80)             4.60e-08  1.84e-07
    composite_transparency (130, 80)      1.30e-07  5.20e-07
    composite_weights (7, 512)            3.00e-08  1.20e-07
    composite_alpha (7, 512)              4.50e-08  1.80e-07
    composite_transparency (7, 512)       2.20e-07  8.80e-07
    mlp_rgb w256_f22                      2.10e-06  8.40e-06
    mlp_rgb w256_f70                      3.00e-06  1.20e-05
    mlp_rgb w256_f102                     4.50e-06  1.80e-05
    mlp_rgb w128_f70                      3.50e-06  1.40e-05
    encoder_pos 10                        3.60e-08  1.44e-07
    encoder_view 4                        3.60e-08  1.44e-07
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import nerfdet_oracle as O

EPS32 = 2.0 ** -23
ATOL = 2e-5            # colours, depths, statistics (tests/test_rays_gpu.py)
SIGMA_REL = 2e-5       # raw sigma, of 1 + |sigma|                    (test_fused_point_mlp_*)
ALPHA_ATOL = 1e-5      # alpha                                        (test_fused_point_mlp_*)
RGB_CAP = 1e-4         # BASELINE north star
POS_DEG, VIEW_DEG = 10, 4

# the cases of tests/test_ray_forward_gpu.py
SAMPLER_SHAPES = [(1, 2), (5, 51), (4, 64), (257, 3), (33, 65), (2, 256)]
SAMPLER_RANGES = [(0.2, 8.0), (0.05, 0.051)]
JITTERS = ["zero", "below_one", "half", "random"]
COMPOSITE_SHAPES = [(1, 1), (63, 2), (64, 9), (65, 64), (130, 80), (7, 512)]
MLP_ARCHS = {"w256_f22": (256, 22), "w256_f70": (256, 70), "w256_f102": (256, 102), "w128_f70": (128, 70)}
MLP_SHAPES = [(1, 1), (1, 65), (7, 73), (96, 40)]
ROW_CLASSES = ["zero", "ordinary", "bright", "x1e-4"]

# measured floors: worst |float32 restatement - float64| over the cases of the row (see the module docstring)
FLOORS = {
    ('sampler_z', (0.2, 8.0)): 7.1e-07,
    ('sampler_z', (0.05, 0.051)): 4.8e-09,
    ('composite_weights', (1, 1)): 2.7e-08,
    ('composite_alpha', (1, 1)): 2.7e-08,
    ('composite_transparency', (1, 1)): 0.0e+00,
    ('composite_weights', (63, 2)): 4.3e-08,
    ('composite_alpha', (63, 2)): 4.3e-08,
    ('composite_transparency', (63, 2)): 4.3e-08,
    ('composite_weights', (64, 9)): 6.7e-08,
    ('composite_alpha', (64, 9)): 4.5e-08,
    ('composite_transparency', (64, 9)): 6.2e-08,
    ('composite_weights', (65, 64)): 4.5e-08,
    ('composite_alpha', (65, 64)): 4.6e-08,
    ('composite_transparency', (65, 64)): 9.3e-08,
    ('composite_weights', (130, 80)): 5.9e-08,
    ('composite_alpha', (130, 80)): 4.6e-08,
    ('composite_transparency', (130, 80)): 1.3e-07,
    ('composite_weights', (7, 512)): 3.0e-08,
    ('composite_alpha', (7, 512)): 4.5e-08,
    ('composite_transparency', (7, 512)): 2.2e-07,
    ('mlp_rgb', 'w256_f22'): 2.1e-06,
    ('mlp_rgb', 'w256_f70'): 3.0e-06,
    ('mlp_rgb', 'w256_f102'): 4.5e-06,
    ('mlp_rgb', 'w128_f70'): 3.5e-06,
    ('encoder_pos', 10): 3.6e-08,
    ('encoder_view', 4): 3.6e-08,
}


def bar(key):
    """max(4 * floor, 2^-23 * magnitude) of a table row; rgb capped at RGB_CAP."""
    kind = key[0]
    mag = float(np.float32(key[1][1])) if kind == "sampler_z" else 1.0
    b = max(4.0 * FLOORS[key], EPS32 * mag)
    return min(b, RGB_CAP) if kind == "mlp_rgb" else b


def render_table():
    """The table of the module docstring, from FLOORS (the CPU test asserts that the docstring holds exactly this)."""
    lines = ["    quantity                                floor      bar", "    " + "-" * 56]
    for key in FLOORS:
        name = f"{key[0]} {key[1]}"
        lines.append(f"    {name:<36} {FLOORS[key]:>9.2e} {bar(key):>9.2e}")
    return "\n".join(lines)


# ------------------------------------------------------------------------------------------------------
# encoders
# ------------------------------------------------------------------------------------------------------
def encode_f32args(x, n_deg):
    """``[x | sin(x 2^k) k < n | sin(x 2^k + pi/2) k < n]``, degree-major and xyz-minor, with the ARGUMENTS formed in float32 as the
    reference forms them and the sine in float64."""
    x32 = x.to(torch.float32)
    scales = torch.tensor([2.0 ** i for i in range(n_deg)], dtype=torch.float32)
    xb = (x32[..., None, :] * scales[:, None]).reshape(*x32.shape[:-1], n_deg * x32.shape[-1])      # exact: a power of two
    arg = torch.cat([xb, xb + torch.tensor(0.5 * math.pi, dtype=torch.float32)], dim=-1)              # one float32 rounding
    return torch.cat([x32.double(), torch.sin(arg.double())], dim=-1)


def encode_f64(x, n_deg):
    """The pure-float64 encoder (what :func:`encode_f32args` is NOT): the oracle's on float64 input."""
    return O.sinusoidal_encode(x.double(), n_deg)


# ------------------------------------------------------------------------------------------------------
# radiance MLP
# ------------------------------------------------------------------------------------------------------
def nerf_forward64(sd, xyz, ray_d, features):
    """nerf_mlp.py:146-161,229-234 on a reference-named state dict in float64 with the float32-argument encoders:
    ``(rgb (.., 3), relu(sigma) (.., 1), trunk output (.., W))``.  ``ray_d`` (R, 3), broadcast over the samples, or (R, S, 3)."""
    sd = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    h = O._mlp_trunk(sd, torch.cat([encode_f32args(xyz, POS_DEG), features.double()], dim=-1))
    sigma = F.linear(h, sd["mlp.sigma_layer.output_layer.weight"], sd["mlp.sigma_layer.output_layer.bias"])
    cond = encode_f32args(ray_d, VIEW_DEG)
    if cond.shape[:-1] != h.shape[:-1]:
        cond = cond.view([cond.shape[0]] + [1] * (h.dim() - cond.dim()) + [cond.shape[-1]]).expand(*h.shape[:-1], cond.shape[-1])
    b = F.linear(h, sd["mlp.bottleneck_layer.output_layer.weight"], sd["mlp.bottleneck_layer.output_layer.bias"])
    z = F.relu(F.linear(torch.cat([b, cond], dim=-1), sd["mlp.rgb_layer.hidden_layers.0.weight"], sd["mlp.rgb_layer.hidden_layers.0.bias"]))
    rgb = F.linear(z, sd["mlp.rgb_layer.output_layer.weight"], sd["mlp.rgb_layer.output_layer.bias"])
    width = sd["mlp.base.hidden_layers.3.weight"].shape[0]
    return torch.sigmoid(rgb), F.relu(sigma), h[..., :width]


def nerf_forward32(sd, xyz, ray_d, features):
    """The float32 CPU restatement: ``oracle.nerf_forward`` on float32 tensors."""
    sd = {k: v.float() for k, v in sd.items() if v.is_floating_point()}
    return O.nerf_forward(sd, xyz.float(), ray_d.float(), features.float())


def build_mlp(arch):
    """The module of ``MLP_ARCHS[arch]`` on the CPU: (net_depth 4, width, skip 3, condition 1 x width / 2), biases normal(0, 0.1)."""
    from nerfdet_amd.radiance_field import VanillaNeRFRadianceField
    width, fdim = MLP_ARCHS[arch]
    torch.manual_seed(1000 + width + fdim)
    mlp = VanillaNeRFRadianceField(4, width, 3, fdim, 1, width // 2)
    with torch.no_grad():
        for p in mlp.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)
    return mlp.eval()


# Scale of the bright rows.  The issue this module answers asked for x 1e3.  The absolute error of ANY float32 evaluation grows with the
# row's scale, the bars (2e-5 (1 + |sigma|), an rgb behind a sigmoid) do not: a few per cent of the x 1e3 rows have a sigma between 0 and
# ~10 summed from terms of 1e2 .. 1e3, and on those the float32 CPU restatement itself reached 4.2e-5 (1 + |sigma|) and 6.6e-5 in rgb.
# That is a property of float32, so the scale comes down: to the largest power of two at which the float32 restatement stays within a
# quarter of the sigma bar on every case (measured: 3.4e-6 at 32, 1.3e-5 at 64, 1.1e-5 at 128; tests/test_ray_forward_ref_cpu.py
# holds it to half the bar, for CPUs whose GEMM sums in another order).  Rows 2^5 apart in one tile still cost a shared scale five
# bits on the dimmer ones.
BRIGHT = 32.0


def row_class(n):
    """Class of each of n sample rows, an index into ROW_CLASSES: period 4, so every 64-row tile mixes all four."""
    return torch.arange(n) % 4


def mlp_inputs(arch, r, s):
    """``(pts (R, S, 3), dirs (R, 3), glob (R, S, F))``: points uniform in +-8 (the far end of the depth range), unit view directions,
    conditioning rows shaped like the sampler's ``[mean (3 + d) | exp(-var) (3 + d)]`` -- colours in [0, 1), features N(0, 1),
    exp(-var) in (0, 1] -- of which row i is all zero (a sample no view sees), ordinary, x BRIGHT or x 1e-4 by ``row_class``."""
    fdim = MLP_ARCHS[arch][1]
    d = fdim // 2 - 3
    gen = torch.Generator().manual_seed(7 * fdim + 131 * r + s)
    n = r * s
    pts = torch.rand(n, 3, generator=gen) * 16 - 8
    dirs = torch.randn(r, 3, generator=gen)
    dirs = dirs / dirs.norm(dim=-1, keepdim=True)
    glob = torch.cat([torch.rand(n, 3, generator=gen), torch.randn(n, d, generator=gen),
                      torch.exp(-3 * torch.rand(n, 3 + d, generator=gen))], dim=1)
    cls = row_class(n)
    glob[cls == 0] = 0.0
    glob[cls == 2] *= BRIGHT
    glob[cls == 3] *= 1.0e-4
    return pts.view(r, s, 3), dirs, glob.view(r, s, fdim)


def mlp_case_floor(arch, r, s):
    """Worst |float32 restatement - float64| of rgb on one case, and of relu(sigma) relative to 1 + |sigma|."""
    mlp = build_mlp(arch)
    pts, dirs, glob = mlp_inputs(arch, r, s)
    rgb64, sig64, _ = nerf_forward64(mlp.state_dict(), pts, dirs, glob)
    rgb32, sig32 = nerf_forward32(mlp.state_dict(), pts, dirs, glob)
    return (float((rgb32.double() - rgb64).abs().max()),
            float(((sig32.double() - sig64).abs() / (1 + sig64.abs())).max()))


# ------------------------------------------------------------------------------------------------------
# sampler
# ------------------------------------------------------------------------------------------------------
BELOW_ONE = float(np.nextafter(np.float32(1), np.float32(0)))


def sampler_inputs(r, s, jitter):
    """``(ray_o (R, 3), ray_d (R, 3), t_rand (R, S) or None)``; ``jitter`` is "det" or one of JITTERS."""
    gen = torch.Generator().manual_seed(17 * r + s)
    ray_o = torch.randn(r, 3, generator=gen) * 2
    ray_d = torch.randn(r, 3, generator=gen)
    t = {"det": None, "zero": torch.zeros(r, s), "below_one": torch.full((r, s), BELOW_ONE), "half": torch.full((r, s), 0.5),
         "random": torch.rand(r, s, generator=gen)}[jitter]
    return ray_o, ray_d, t


def f32_range(near_far):
    """The depth range as the float32 values the operation is handed (render_ray.py:163-164 multiplies float32 ones by them)."""
    return float(np.float32(near_far[0])), float(np.float32(near_far[1]))


def sample64(ray_o, ray_d, near_far, s, t_rand):
    return O.sample_along_camera_ray(ray_o.double(), ray_d.double(), f32_range(near_far), s, det=t_rand is None,
                                     t_rand=None if t_rand is None else t_rand.double())


def sample32(ray_o, ray_d, near_far, s, t_rand):
    return O.sample_along_camera_ray(ray_o.float(), ray_d.float(), near_far, s, det=t_rand is None, t_rand=t_rand)


def sampler_case_floor(near_far, r, s, jitter):
    ray_o, ray_d, t = sampler_inputs(r, s, jitter)
    return float((sample32(ray_o, ray_d, near_far, s, t)[1].double() - sample64(ray_o, ray_d, near_far, s, t)[1]).abs().max())


# ------------------------------------------------------------------------------------------------------
# compositor
# ------------------------------------------------------------------------------------------------------
ROW_KINDS = ["ordinary", "transparent", "one_opaque", "three_opaque", "opaque_first", "opaque_last", "thin"]
SIGMA_LO, SIGMA_HI, OPAQUE, TINY = 1e-3, 16.0, 40.0, 1e-12
MASK_COUNTS = (0, 8, 9)          # ... and S: the seen-sample counts planted in the first rows of a case's pixel mask


def row_kind(r):
    """Kind of each of r rays, an index into ROW_KINDS."""
    return torch.arange(r) % len(ROW_KINDS)


def planted_counts(r, s):
    """Seen-sample counts of the first rows of the pixel mask: 0, 8, 9 and S, those that S samples allow, as many as there are rays."""
    counts = []
    for c in MASK_COUNTS + (s,):
        if c <= s and c not in counts:
            counts.append(c)
    return counts[:r]


def composite_inputs(r, s, negate=False):
    """``(raw (R, S, 4), z (R, S), pixel_mask (R, S) bool)``.

    z: ascending in (0.2, 8) per ray, the call's minimum 0.2 and maximum 8.0 both planted in ray R // 2; the (130, 80) case repeats every
    fifth depth, as a merged fine pass does; ``negate`` flips the sign (descending, negative).  sigma by ``row_kind``: ordinary = 0 (10 %),
    1e-12 (10 %), 40 (2 %), else log-uniform in [1e-3, 16]; transparent = 1e-12 in a quarter of the samples, else 0; one / three opaque
    samples, an opaque first, an opaque last sample in an ordinary ray; thin = log-uniform in [t, 3 t], t = max(5e-3, 1 / S), so that a
    512-sample sum keeps transmittance to its end.  The first rows of the pixel mask see exactly ``planted_counts`` samples, the others
    a random fifth.

    No ray is faint without being transparent: every ordinary ray has one sample, at a random place, with sigma log-uniform in
    [0.5, 16], and a thin ray's sigmas sum to more than 1.  A first version had thin rays in [1e-3, 3e-2] at every S and no such sample,
    and the float32 restatement itself missed the 2e-5 of the depth on (63, 2) by 2.1e-5: ``1 - exp(-sigma)`` carries half an ulp of 1,
    3e-8, whatever sigma is, so a weight of 1e-3 is known to 3e-5 of itself, and the depth of a ray whose weights sum to 2e-3 -- a
    mean of depths up to 7.8 apart -- to 1e-4.  A property of float32, excluded here by construction."""
    gen = torch.Generator().manual_seed(29 * r + s)
    z = torch.sort(torch.rand(r, s, generator=gen) * 7.6 + 0.3, dim=1)[0]
    if (r, s) == (130, 80):
        z[:, 4::5] = z[:, 3::5]
    z[r // 2, 0] = 0.2
    z[r // 2, -1] = 8.0 if s > 1 else 0.2
    if r > 1 and s == 1:
        z[r // 2 - 1, 0] = 8.0
    if negate:
        z = -z

    def log_uniform(lo, hi):
        return torch.exp(torch.rand(r, s, generator=gen) * (math.log(hi) - math.log(lo)) + math.log(lo)).clamp(lo, hi)

    pick = torch.rand(r, s, generator=gen)
    sigma = log_uniform(SIGMA_LO, SIGMA_HI)
    sigma[pick < 0.22] = OPAQUE
    sigma[pick < 0.20] = TINY
    sigma[pick < 0.10] = 0.0
    kind = row_kind(r)
    anchor = torch.randint(0, s, (r,), generator=gen)
    strong = log_uniform(0.5, SIGMA_HI)[:, 0]
    rows = torch.nonzero(kind == 0).squeeze(1)
    sigma[rows, anchor[rows]] = strong[rows]
    t = max(5e-3, 1.0 / s)
    thin = log_uniform(t, 3 * t)
    sigma[kind == 6] = thin[kind == 6]
    quarter = torch.rand(r, s, generator=gen) < 0.25
    sigma[kind == 1] = torch.where(quarter, torch.tensor(TINY), torch.tensor(0.0))[kind == 1]
    mid = int(torch.randint(0, s, (1,), generator=gen))
    sigma[kind == 2, mid] = OPAQUE
    first3 = min(mid, max(s - 3, 0))
    sigma[kind == 3, first3:first3 + 3] = OPAQUE
    sigma[kind == 4, 0] = OPAQUE
    sigma[kind == 5, -1] = OPAQUE
    raw = torch.cat([torch.rand(r, s, 3, generator=gen), sigma.unsqueeze(-1)], dim=-1)
    pmask = torch.rand(r, s, generator=gen) < 0.2
    for i, c in enumerate(planted_counts(r, s)):
        pmask[i] = False
        pmask[i, torch.randperm(s, generator=gen)[:c]] = True
    return raw, z, pmask


def sigma_allowed(sigma):
    """True where a compositing sigma is one of 0, 1e-12, 40 or lies in [1e-3, 16] (as float32 values)."""
    s = sigma.float()
    return (s == 0) | (s == np.float32(TINY)) | (s == OPAQUE) | ((s >= np.float32(SIGMA_LO)) & (s <= SIGMA_HI))


COMPOSITE_KEYS = ("rgb", "depth", "weights", "alpha", "transparency")


def _raw2outputs(raw, z, pmask, white):
    """``oracle.raw2outputs``; a single-sample ray, for which the reference's ``ones_like(t[:, 0:1])`` of an empty cumprod is empty, is
    composited with an empty second sample behind it (sigma 0, the same depth, unseen), which changes no output, and cut back."""
    if raw.shape[1] > 1:
        return O.raw2outputs(raw, z, pmask, white_bkgd=white)
    out = O.raw2outputs(torch.cat([raw, torch.zeros_like(raw)], dim=1), torch.cat([z, z], dim=1),
                        None if pmask is None else torch.cat([pmask, torch.zeros_like(pmask)], dim=1), white_bkgd=white)
    for k in ("weights", "alpha", "transparency"):
        out[k] = out[k][:, :1]
    out["z_vals"] = z
    return out


def composite64(raw, z, pmask, white):
    return _raw2outputs(raw.double(), z.double(), pmask, white)


def composite32(raw, z, pmask, white):
    return _raw2outputs(raw.float(), z.float(), pmask, white)


def composite_case_floor(r, s, white, negate):
    """{quantity: worst |float32 restatement - float64|} on one case."""
    raw, z, pmask = composite_inputs(r, s, negate)
    a, b = composite32(raw, z, pmask, white), composite64(raw, z, pmask, white)
    return {k: float((a[k].double() - b[k]).abs().max()) for k in COMPOSITE_KEYS}


# ------------------------------------------------------------------------------------------------------
# the table's rows, recomputed
# ------------------------------------------------------------------------------------------------------
def encoder_points(n):
    """(3, n) points uniform in +-8 with the ends themselves in the first columns."""
    gen = torch.Generator().manual_seed(n)
    p = torch.rand(3, n, generator=gen) * 16 - 8
    p[:, 0] = torch.tensor([8.0, -8.0, 8.0])
    return p


def measure_floors():
    """Every row of FLOORS, measured now: {key: worst error over the row's cases}."""
    out = {}
    for nf in SAMPLER_RANGES:
        out[("sampler_z", nf)] = max(sampler_case_floor(nf, r, s, j) for r, s in SAMPLER_SHAPES for j in ["det"] + JITTERS)
    for r, s in COMPOSITE_SHAPES:
        worst = {}
        for white in (False, True):
            for negate in (False, True):
                for k, v in composite_case_floor(r, s, white, negate).items():
                    worst[k] = max(worst.get(k, 0.0), v)
        for k in ("weights", "alpha", "transparency"):
            out[("composite_" + k, (r, s))] = worst[k]
    for arch in MLP_ARCHS:
        out[("mlp_rgb", arch)] = max(mlp_case_floor(arch, r, s)[0] for r, s in MLP_SHAPES)
    for name, deg, x in (("encoder_pos", POS_DEG, encoder_points(257).t()), ("encoder_view", VIEW_DEG, mlp_inputs("w256_f70", 96, 40)[1])):
        out[(name, deg)] = float((O.sinusoidal_encode(x.float(), deg).double() - encode_f32args(x, deg)).abs().max())
    return out


if __name__ == "__main__":
    for key, v in measure_floors().items():
        print(f"    {key!r}: {v:.2e},")
