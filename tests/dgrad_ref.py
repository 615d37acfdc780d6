"""The convolution data gradients of the training step (nerfdet_amd/conv_train.py: _conv_grads, _dgrad_strided, ConvT2, ConvAffineAct) stated
plainly in torch, the data the tests feed them, and the case tables tests/test_dgrad_ref_cpu.py and tests/test_dgrad_shapes_gpu.py share.  Nothing
here calls nerfdet_amd; every function takes the dtype it computes in (fp64: the reference; fp32: the "e32" error figure of the bars) and runs on
the device of its arguments.

Layouts: channels-last throughout, (D, H, W, C) for a volume and (N, H, W, C) for a batch of maps; weights as torch holds them,
(Cout, Cin, *kernel) for Conv2d / Conv3d and (Cin, Cout, 2, 2, 2) for ConvTranspose3d."""
import itertools
import math

import torch

EXACT_BELOW = 1 << 24               # integers of smaller magnitude are exact in fp32


def _as3d(kernel, stride):
    """(k3, s3, p3) of an odd same-padded kernel: a 2D kernel takes the batch as a depth axis of extent-1 taps that is never strided or padded."""
    k = tuple(int(v) for v in kernel)
    assert len(k) in (2, 3) and all(v % 2 == 1 for v in k), k
    k3 = (1,) + k if len(k) == 2 else k
    s3 = (1, stride, stride) if len(k) == 2 else (stride,) * 3
    return k3, s3, tuple(v // 2 for v in k3)


def out_grid(dims_in, kernel, stride):
    """Output grid of the same-padded convolution over the input grid ``dims_in`` ((D, H, W) or (N, H, W))."""
    k3, s3, p3 = _as3d(kernel, stride)
    return tuple((n + 2 * p - k) // s + 1 for n, p, k, s in zip(dims_in, p3, k3, s3))


def dx_conv(dy, w, stride, dims_in, dtype=torch.float64):
    """dx[i][ci] = sum_t sum_co dy[(i + p - t) / s][co] w[co][ci][t] over the taps where the division is exact and in range: the data gradient of
    the odd same-padded convolution of uniform stride 1 or 2 with the torch-layout weight ``w``.  dy (OD, OH, OW, Cout) / (N, OH, OW, Cout);
    ``dims_in`` the input's grid, (D, H, W) / (N, H, W); returns (*dims_in, Cin).  Tap by tap: output position o adds dy[o] w[t] to input
    position s o + t - p, one matmul per tap into a strided slice of a buffer with the padding still on it."""
    assert stride in (1, 2)
    k3, s3, p3 = _as3d(w.shape[2:], stride)
    o3 = tuple(dy.shape[:3])
    assert o3 == out_grid(dims_in, w.shape[2:], stride), (o3, dims_in)
    cout, cin = int(w.shape[0]), int(w.shape[1])
    assert dy.shape[3] == cout
    g = dy.to(dtype).reshape(-1, cout)
    wt = w.to(dtype).reshape(cout, cin, -1)
    ext = tuple(max(k + s * (o - 1), p + n) for k, s, o, p, n in zip(k3, s3, o3, p3, dims_in))
    buf = torch.zeros(ext + (cin,), dtype=dtype, device=dy.device)
    for t, (a, b, c) in enumerate(itertools.product(*(range(k) for k in k3))):
        buf[a:a + s3[0] * (o3[0] - 1) + 1:s3[0], b:b + s3[1] * (o3[1] - 1) + 1:s3[1], c:c + s3[2] * (o3[2] - 1) + 1:s3[2]] += (g @ wt[:, :, t]).view(*o3, cin)
    return buf[p3[0]:p3[0] + dims_in[0], p3[1]:p3[1] + dims_in[1], p3[2]:p3[2] + dims_in[2]].contiguous()


def dx_convT2(dy, w, dtype=torch.float64):
    """Data gradient of ConvTranspose3d(k = 2, s = 2): dx[i][ci] = sum_t sum_co dy[2 i + t][co] w[ci][co][t] -- the unpadded stride-2 2x2x2
    convolution of dy (2D, 2H, 2W, Cout) with w (Cin, Cout, 2, 2, 2) read as a Conv3d weight, no flip.  Returns (D, H, W, Cin)."""
    cin, cout = int(w.shape[0]), int(w.shape[1])
    assert tuple(w.shape[2:]) == (2, 2, 2) and dy.shape[3] == cout and all(v % 2 == 0 for v in dy.shape[:3])
    d, h, wd = (v // 2 for v in dy.shape[:3])
    g, wt = dy.to(dtype), w.to(dtype)
    out = torch.zeros((d * h * wd, cin), dtype=dtype, device=dy.device)
    for a, b, c in itertools.product(range(2), repeat=3):
        out += g[a::2, b::2, c::2].reshape(-1, cout) @ wt[:, :, a, b, c].t()
    return out.view(d, h, wd, cin)


def affine_act_bwd(dy, y, scale, relu, dtype=torch.float64):
    """(g', d_identity) = (dy [y > 0] scale, dy [y > 0]): the elementwise pass of ConvAffineAct.backward for y = act(conv(x) scale + shift + residual)
    (without ReLU the mask is all ones).  ``scale`` per channel (last axis)."""
    d_id = dy.to(dtype) * (y > 0).to(dtype) if relu else dy.to(dtype).clone()
    return d_id * scale.to(dtype), d_id


def rel_max(got, ref):
    """max |got - ref| / max |ref|"""
    return float((got.double() - ref.double()).abs().max()) / float(ref.abs().max())


def rel_rms(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())


# ---- data ----
def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def integer_case(cin, cout, kernel, grid, seed=0, transposed=False):
    """(dy, w) of the exact ladder: dy in {-3 .. 3} over the output grid ``grid`` with a +3 and a -3 in it, weights in {-2 .. 2} with a +2 and a -2
    (so the per-tensor power-of-two scales of the fp16-pair scheme are those of 3 and 2, and no low half holds anything).  Every product and every
    partial sum of the data gradient is an integer of magnitude <= taps x padded Cout x 3 x 2 (integer_bound), exact in fp32 below 2^24 in any
    order.  ``transposed``: w in ConvTranspose3d's layout (Cin, Cout, *kernel)."""
    g = _gen(seed)
    dy = torch.randint(-3, 4, (*grid, cout), generator=g).float()
    w = torch.randint(-2, 3, ((cin, cout) if transposed else (cout, cin)) + tuple(kernel), generator=g).float()
    dy.view(-1)[0], dy.view(-1)[-1] = 3.0, -3.0
    w.view(-1)[0], w.view(-1)[-1] = 2.0, -2.0
    return dy, w


def integer_bound(cout, kernel):
    """The largest magnitude a partial sum of an integer case's data gradient can reach: taps x Cout padded to 32 x max|dy| x max|w|."""
    return math.prod(kernel) * ((cout + 31) // 32 * 32) * 3 * 2


def grid_weights(cout, cin, kernel, seed=0):
    """Weights k / 1024, |k| <= 1024 (a +-1 among them): times any power of two they are 11-bit integers -- exact as the high half of an fp16 pair,
    exact as the sum of three bf16 terms."""
    w = torch.randint(-1024, 1025, (cout, cin) + tuple(kernel), generator=_gen(seed)).float() / 1024.0
    w.view(-1)[0], w.view(-1)[-1] = 1.0, -1.0
    return w


def gradient_like(grid, channels, seed=0):
    """A loss gradient as the head hands it back: standard normal times a per-voxel magnitude exp(1.5 N(0, 1)), 80 % of the voxels exactly zero
    (a few positives, the rest nothing)."""
    g = _gen(seed)
    v = torch.randn(*grid, channels, generator=g) * torch.exp(1.5 * torch.randn(*grid, 1, generator=g))
    keep = torch.rand(*grid, 1, generator=g) >= 0.8
    keep.view(-1)[0] = True         # (never all zero, whatever the grid)
    return v * keep


def kaiming(cout, cin, kernel, seed=0, transposed=False):
    """N(0, 2 / fan_in) weights; ``transposed``: ConvTranspose3d's layout."""
    shape = ((cin, cout) if transposed else (cout, cin)) + tuple(kernel)
    return torch.randn(*shape, generator=_gen(seed)) * (2.0 / (cin * math.prod(kernel))) ** 0.5


# ---- the case tables (tests/test_dgrad_shapes_gpu.py runs them, tests/test_dgrad_ref_cpu.py proves what they stand on) ----
# (a) the exact ladder on the adjoint launch: name -> (layer Cin, layer Cout, kernel, grid); the grid is the layer's input AND output grid (stride 1)
LADDER = {
    "64to25": (64, 25, (3, 3, 3), (3, 4, 5)),           # 7 zero padding channels, one chunk
    "96to40": (96, 40, (3, 3, 3), (3, 4, 5)),           # second chunk 8 real + 24 padding channels; adjoint Cout 96 ragged on 64- and 128-column tiles
    "160to64": (160, 64, (3, 3, 3), (7, 6, 5)),         # M = 210 ragged; 160 of 256 columns on the 256-column tiles
    "288to96": (288, 96, (3, 3, 3), (5, 7, 9)),         # production shape class
    "128to64-2d": (128, 64, (3, 3), (2, 15, 20)),       # the batch axis must not be convolved over
}
LADDER_1X1 = {
    "64to32-1x1": (64, 32, (1, 1, 1), (6, 6, 4)),       # 1 K step in fp16 pairs
    "64to64-1x1": (64, 64, (1, 1, 1), (6, 6, 4)),       # 2 K steps
    "64to96-1x1": (64, 96, (1, 1, 1), (6, 6, 4)),       # 3 K steps
}
TILES_1X1 = (64, 100064, 128, 100128, 12864, 112864, 128256)
# the ConvT2 dx launch: name -> (ConvTranspose3d Cin, Cout, input grid of x); dy lives on twice the grid
LADDER_T2 = {"t2-128to32": (128, 32, (2, 3, 5)), "t2-128to64": (128, 64, (2, 3, 5))}
TILES_T2 = (64, 128, 128256)
MAX_SPLITS = 32


def padded(c):
    return (c + 31) // 32 * 32


def adjoint_ksteps(cout, kernel):
    """K steps of the adjoint launch: taps x (layer Cout padded to 32) / 32."""
    return math.prod(kernel) * padded(cout) // 32


def ladder_splits(cout, kernel, halo):
    """The split counts of a ladder row: 1, 2, 3 and the cap min(32, K steps) (halo tiles: min(32, padded Cout / 32), the channel chunks),
    none above the cap."""
    cap = min(MAX_SPLITS, padded(cout) // 32 if halo else adjoint_ksteps(cout, kernel))
    return sorted({min(s, cap) for s in (1, 2, 3, cap)})


# (c) through autograd: name -> (module, layer Cin, layer Cout, kernel, stride, input grid)
AUTOGRAD = {
    "s1-3d-96to25": ("ConvS1", 96, 25, (3, 3, 3), 1, (7, 9, 5)),
    "s1-2d-64to96": ("ConvS1", 64, 96, (3, 3), 1, (2, 11, 13)),
    "s2-3d-64to128": ("ConvS1", 64, 128, (3, 3, 3), 2, (7, 9, 5)),      # odd in every axis
    "s2-2d-64to64": ("ConvS1", 64, 64, (3, 3), 2, (2, 11, 13)),
    "affine-2d-128to64": ("ConvAffineAct", 128, 64, (3, 3), 1, (2, 11, 13)),
    "affine-2d-256to64-1x1": ("ConvAffineAct", 256, 64, (1, 1), 1, (2, 11, 13)),
    "head-128to25": ("shared", 128, 25, (3, 3, 3), 1, (6, 5, 4)),       # 1 + 6 + 18
    "t2-128to32": ("ConvT2", 128, 32, (2, 2, 2), 2, (3, 4, 5)),
}
HEAD_SPLIT = (1, 6, 18)
