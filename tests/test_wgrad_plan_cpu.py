"""conv_train.implicit_plan -- the tile, K splits and keep flag of the implicit weight-gradient launch -- pinned for every shape
tests/test_wgrad_shapes_gpu.py runs and for the training step's own layers: a retune of the heuristics has to move these numbers in the open, not
move the GPU tests off the branches they exist for.  No GPU, no library."""
import math

import pytest

from test_wgrad_shapes_gpu import ARITHS, CASES, STAGED, _library_tile, geometry, impulse_voxels, staged_tiling


@pytest.mark.parametrize("name", list(CASES))
def test_every_gpu_case_reaches_the_branch_it_is_named_for(name):
    from nerfdet_amd.conv_train import implicit_plan
    dims, cin, cout, kernel, stride, pads, plans = CASES[name]
    taps, lo = math.prod(kernel), math.prod(geometry(dims, kernel, stride, pads)[3])
    for arith in ARITHS:
        f16 = arith == "f16x2"
        bm, bn, splits = plans[arith]
        assert implicit_plan(taps, cin, cout, lo, f16) == (bm, bn, splits, f16 and splits > 1), (name, arith)
        assert _library_tile(taps, cin, cout, f16) == (bm, bn), (name, arith)


def test_the_cases_cover_what_they_were_written_for():
    """Output voxels and K steps of the split ladder as the cases' comments give them; 8, 16, 24 and 32 splits; both arithmetics get an 8- and a
    32-split case; the 128 x 256 tile with one and with two column tiles; only the 16 900-voxel case is one weight_grad takes the kernel for by itself."""
    from nerfdet_amd import conv_train
    lo = {n: math.prod(geometry(c[0], c[3], c[4], c[5])[3]) for n, c in CASES.items()}
    assert [lo[n] for n in ("ladder-8", "ladder-16", "ladder-24", "ladder-32", "auto-32")] == [1584, 2366, 4335, 6498, 16900]
    assert [(lo[n] + 31) // 32 for n in ("ladder-8", "ladder-16", "ladder-24", "ladder-32")] == [50, 74, 136, 204]
    assert 50 % 8 != 0
    for arith in ARITHS:
        assert {8, 16, 24, 32} <= {c[6][arith][2] for c in CASES.values()}
    assert CASES["tile-128x256"][6]["f16x2"][:2] == (128, 256) and CASES["tile-128x256"][2] // 256 == 1
    assert CASES["tile-128x256-2col"][6]["f16x2"][:2] == (128, 256) and CASES["tile-128x256-2col"][2] // 256 == 2
    assert {CASES[n][6]["f16x2"][:2] for n in CASES} == {(128, 256), (128, 64), (64, 128), (64, 64)}      # (128 x 128: the knob, and bf16x3)
    assert (128, 128) in {CASES[n][6]["bf16x3"][:2] for n in CASES}
    auto = [n for n, c in CASES.items() if math.prod(c[3]) >= conv_train.IMPLICIT_MIN_TAPS and lo[n] >= 16384]
    assert auto == ["auto-32"] and conv_train.IMPLICIT_WGRAD
    assert all(v == 1584 for n, v in lo.items() if n not in ("ladder-16", "ladder-24", "ladder-32", "auto-32"))
    assert geometry(*[CASES["ow-1"][i] for i in (0, 3, 4, 5)])[3][2] == 1 and geometry(*[CASES["ow-33"][i] for i in (0, 3, 4, 5)])[3][2] == 33


def test_plan_of_the_training_steps_layers():
    """The layers the heuristics were measured on (conv_train.implicit_plan's comment), and the two rows of
    test_implicit_weight_gradient_equals_the_staged_form that stay below the 128 x 256 tile's 32 row tiles."""
    from nerfdet_amd.conv_train import implicit_plan
    assert implicit_plan(27, 256, 256, 40 * 40 * 16, True) == (128, 256, 16, True)          # the neck's 54-tile layers
    assert implicit_plan(27, 256, 256, 40 * 40 * 16, False) == (128, 128, 16, False)
    assert implicit_plan(9, 256, 256, 40 * 60 * 80, True) == (128, 128, 32, True)            # the FPN's 36-tile layer: 18 row tiles, no wide tile
    assert implicit_plan(27, 128, 256, 7 * 6 * 5, True) == (128, 128, 1, False)              # 27 row tiles, 7 K steps
    assert implicit_plan(9, 256, 512, 3 * 9 * 10, True) == (128, 128, 1, False)              # 18 row tiles, 9 K steps
    assert implicit_plan(27, 128, 64, 12 * 10 * 6, True) == (128, 64, 2, True)               # 720 voxels: the most that test splits
    # rounding: 6 and 7 go to 8, 5 stays, and nothing passes 32
    assert [implicit_plan(27, 64, 64, 32 * 8 * s, True)[2] for s in (1, 2, 5, 6, 7, 8, 9, 17, 25, 40)] == [1, 2, 5, 8, 8, 8, 16, 24, 32, 32]
    # the K steps of a split are never empty: the library rejects splits > ksteps
    for lo in (1, 31, 33, 255, 256, 1584, 16900):
        for taps, cin, cout in ((27, 64, 64), (8, 64, 64), (27, 256, 512), (9, 128, 25)):
            for f16 in (False, True):
                assert 1 <= implicit_plan(taps, cin, cout, lo, f16)[2] <= (lo + 31) // 32


@pytest.mark.parametrize("name", list(STAGED))
def test_staged_cases_split_k(name):
    """The tiling tables split the staged form's GEMM at these sizes (8, 22 and 2 ways) on a tile that keeps split-K partials."""
    from nerfdet_amd import conv_tiles
    tile, splits = staged_tiling(name)
    assert splits == STAGED[name][6] and splits > 1
    assert conv_tiles.TILES[tile].family == "unified" and not conv_tiles.is_direct(tile)


def test_impulse_voxels_sit_on_the_split_boundaries():
    imp = impulse_voxels(6498, 32)
    ksteps = 204
    assert len(imp) == 65 and len(set(imp)) == 65
    by_channel = {}
    for k, j in imp:
        by_channel.setdefault(k, []).append(j)
    assert sorted(by_channel) == list(range(64))
    for z in range(32):
        begin = ksteps * z // 32
        assert by_channel[2 * z] == [32 * begin]
        if z:
            assert by_channel[2 * z - 1] == [32 * begin - 1] and begin > ksteps * (z - 1) // 32
    assert sorted(by_channel[63]) == [32 * 203 - 1, 6497]
