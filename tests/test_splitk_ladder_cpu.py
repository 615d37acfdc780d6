"""What tests/test_splitk_ladder_gpu.py stands on, checked without a GPU: the premise of its exact ladder (integer fixtures whose convolution is exact
in fp32 in any order and whose operands the fp16-pair and bf16 schemes of csrc/conv_split_kernels.hip hold without loss), its coverage of every
(tile, splits > 1) pair the tables of conv_tuning.py dispatch, and the K walks its cases give the kernels (restated from the kernels:
it_begin = n s / S, it_end = n (s + 1) / S; the wave-specialised tiles round a walk up to WS_DEPTH = 2; the halo tiles split the channel chunks)."""
import pytest
import torch

import test_splitk_ladder_gpu as G
from nerfdet_amd import conv_tiles, conv_tuning
from nerfdet_amd.conv3d import f16_weight_scale

CASES = [(name, volume) for name in G.LADDER for volume in ((0, 1) if name in {n for _, n in G.BATCHED.values()} else (0,))]


@pytest.mark.parametrize("name,volume", CASES)
def test_the_integer_fixtures_are_exact_in_fp32_and_in_both_operand_schemes(name, volume):
    case = G._int_case(name, volume)
    cin, cout, grid, k, relu, res = G.LADDER[name]
    # every partial sum, and the output through bias and residual, is an integer below 2^24
    w, x = case.conv.weight.detach(), case.x
    assert float(x.abs().max()) == 3.0 and float(w.abs().max()) == 2.0 and float(case.conv.bias.detach().abs().max()) <= 5.0
    assert all(torch.equal(t, t.round()) for t in (x, w, case.conv.bias.detach()) + (() if case.res is None else (case.res,)))
    assert (case.res is None) == (res == 0) and (case.res is None or float(case.res.abs().max()) <= 4.0)
    assert case.bound == k ** 3 * cin * 3 * 2 + 5 + (4 if res else 0) and case.bound < G.EXACT_BELOW == 2 ** 24
    assert float(case.ref.abs().max()) <= case.bound
    # ... so fp32 in PyTorch-CPU's order gives the fp64 result, and the fp32 copy the GPU file compares with is that result
    assert torch.equal(case.forward(torch.float32).double(), case.ref)
    assert torch.equal(case.ref.float().double(), case.ref)
    assert case.ref.dtype == torch.float64 and tuple(case.ref.shape) == (*grid, cout)
    # the fp16-pair scheme: operand times a power of two, rounded to fp16; nothing is left for the low half
    for t in (x, w):
        s = f16_weight_scale(float(t.abs().max()))
        assert s == 2.0 ** 13
        assert torch.equal((t * s).half().float(), t * s)
    # the bf16 planes: the leading one holds the operand
    assert torch.equal(x.bfloat16().float(), x) and torch.equal(w.bfloat16().float(), w)
    if volume:
        assert not torch.equal(case.x, G._int_case(name, 0).x) and torch.equal(w, G._int_case(name, 0).conv.weight.detach())


def _table_pairs():
    return {(tile, splits) for table in (conv_tuning.TUNED_SPLIT, conv_tuning.TUNED_F16, conv_tuning.TUNED_BF16)
            for tile, splits in table.values() if splits > 1}


def test_every_pair_the_tables_dispatch_is_covered():
    pairs = _table_pairs()
    assert pairs, "the tables hold split-K rows"
    assert G.COVERED == G.LADDER_PAIRS | G.ROW_PAIRS
    missing = sorted(pairs - G.COVERED)
    assert not missing, f"(tile, splits) pairs of conv_tuning.py without a ladder step or a row in tests/test_splitk_ladder_gpu.py: {missing}"
    # ... and each of them has its real-valued row, beside the ladder step
    missing = sorted(pairs - G.ROW_PAIRS)
    assert not missing, f"(tile, splits) pairs of conv_tuning.py without a row in PRODUCTION of tests/test_splitk_ladder_gpu.py: {missing}"
    assert G.ROW_PAIRS <= pairs, f"PRODUCTION names pairs no table dispatches: {sorted(G.ROW_PAIRS - pairs)}"
    # the rules outside the tables hand out up to MAX_SPLITS: the ladder reaches it on every tile
    assert G.TILE_IDS == conv_tiles.ids("unified", "ws", "wsp", "halo")
    for tile in G.TILE_IDS:
        assert {s for t, s in G.LADDER_PAIRS if t == tile} == set(range(1, G.MAX_SPLITS + 1)), tile
    assert {t for t, _ in G.LADDER_ROWS} == set(G.TILE_IDS)
    for tile, splits in sorted(G.ROW_PAIRS | set(G.BF16X3_ROWS) | set(G.BF16_ROWS)):
        units = G.production_units(tile, splits)
        assert units >= splits and units % splits, (tile, splits, units)
        assert len(set(G.walks(units, splits))) == 2, "an uneven cut: two walk lengths"
    bf16_pairs = {v for v in conv_tuning.TUNED_BF16.values() if v[1] > 1}
    assert set(G.BF16_ROWS) <= bf16_pairs and set(G.BF16X3_ROWS) <= G.ROW_PAIRS
    assert {conv_tiles.TILES[t].family for t, _ in G.BF16X3_ROWS} == {"unified", "ws", "wsp", "halo"}


def test_resolve_leaves_every_ladder_and_production_launch_alone():
    """conv_tiles.resolve on the shapes of the GPU file: the tile and split count asked are the ones that run (the GPU file asserts it per launch;
    here the whole set, so a rule change that re-routes a row shows without a GPU)."""
    for tile, name in G.LADDER_ROWS:
        cin, cout, grid, k, _, _ = G.LADDER[name]
        m = grid[0] * grid[1] * grid[2]
        for splits in range(1, G.ladder_cap(tile, name) + 1):
            got = conv_tiles.resolve(tile, splits, m=m, cout=cout, cin=cin, taps=k ** 3, transposed=False, halo_ok=k > 1, direct_epilogue=False)
            assert got == (tile, splits), (tile, name, splits, got)
    for tile, splits in G.PRODUCTION_ROWS:
        cin, cout, grid, k, _, _ = G.production_shape(tile, splits)
        got = conv_tiles.resolve(tile, splits, m=grid[0] * grid[1] * grid[2], cout=cout, cin=cin, taps=k ** 3, transposed=False, halo_ok=k > 1,
                                 direct_epilogue=False)
        assert got == (tile, splits), (tile, splits, got)
    for family, (tile, name) in G.BATCHED.items():
        cin, cout, grid, k, _, _ = G.LADDER[name]
        assert conv_tiles.TILES[tile].family == family and name in G.FAMILY_CASES[family]
        for splits in (2, 5, G.ladder_cap(tile, name)):
            got = conv_tiles.resolve(tile, splits, m=2 * grid[0] * grid[1] * grid[2], cout=cout, cin=cin, taps=k ** 3, transposed=False, halo_ok=k > 1,
                                     direct_epilogue=False, batch=2)
            assert got == (tile, splits)
    assert set(G.BATCHED) == {"unified", "ws", "halo"}, "the persistent tiles take one volume per launch"


def test_the_walks_the_ladder_gives_the_kernels():
    w = G.walks
    # the walks partition the K steps, in order, for every case and split count of the ladder
    for tile, name in G.LADDER_ROWS:
        n = G.ladder_units(tile, name)
        for splits in range(1, G.ladder_cap(tile, name) + 1):
            assert sum(w(n, splits)) == n and min(w(n, splits)) >= 1
            assert G.starts(n, splits) == [sum(w(n, splits)[:s]) for s in range(splits)]
    # the cases the shapes were chosen for
    assert G.ladder_ksteps("k27c96-cout40") == G.ladder_ksteps("k27c96-cout300") == G.ladder_ksteps("k27c96-cout304") == 81
    assert G.ladder_ksteps("k1c1024-cout64") == G.ladder_ksteps("k1c1024-cout256") == 32
    assert set(w(81, 32)) == {2, 3} and set(w(81, 24)) == {3, 4} and w(81, 16).count(5) == 15 and set(w(81, 16)) == {5, 6}
    assert w(32, 32) == [1] * 32 and set(w(32, 24)) == {1, 2} and set(w(32, 12)) == {2, 3}
    assert w(10, 4) == [2, 3, 2, 3] and w(10, 8) == [1, 1, 1, 2, 1, 1, 1, 2] and w(10, 3) == [3, 3, 4]
    assert w(32, 32) == [1] * 32 and set(w(32, 5)) == {6, 7}
    # production has such rows: head2 (TUNED_F16: 108 K steps over 16 splits), the 100-step weight-gradient GEMM over 3
    assert set(w(108, 16)) == {6, 7} and w(100, 3) == [33, 33, 34]
    # the ladder as a whole: walks of 1, 2 and 3 on every tile; on the wave-specialised tiles (walks rounded up to WS_DEPTH = 2) an odd walk from an
    # odd start, an odd walk from an even start, an even walk from an odd start, and walks shorter than the pipeline; on every halo tile a split of
    # one chunk and a chunk count the split count does not divide
    for tile in G.TILE_IDS:
        family = conv_tiles.TILES[tile].family
        seen = set()
        for t, name in G.LADDER_ROWS:
            if t != tile:
                continue
            n = G.ladder_units(tile, name)
            for splits in range(2, G.ladder_cap(tile, name) + 1):
                seen |= {(length, start % 2, n % splits != 0) for length, start in zip(w(n, splits), G.starts(n, splits))}
        lengths = {length for length, _, _ in seen}
        assert {1, 2, 3} <= lengths, (tile, lengths)
        assert any(uneven for _, _, uneven in seen)
        if family in ("ws", "wsp"):
            for length, odd_start in ((1, 1), (1, 0), (3, 1), (3, 0), (2, 1), (5, 1)):
                assert any(l == length and o == odd_start for l, o, _ in seen), (tile, length, odd_start)
        if family == "halo":
            assert G.ladder_units(tile, "k27c1024-cout72") == 32 and G.ladder_cap(tile, "k27c1024-cout72") == 32
            assert G.ladder_units(tile, "k27c320-cout300") == 10


def test_the_ladder_shapes_are_ragged_and_small():
    for name, (cin, cout, grid, k, relu, res) in G.LADDER.items():
        m = grid[0] * grid[1] * grid[2]
        assert m in (60, 120, 315) and m % 64 and cin % 32 == 0 and k in (1, 3) and relu in (0, 1, 2)
        assert 2 * m * cout * cin * k ** 3 <= 0.6e9, "the fp64 reference stays near half a GFLOP"
    couts = {family: {G.LADDER[n][1] for n in names} for family, names in G.FAMILY_CASES.items()}
    assert 40 in couts["unified"] and 300 in couts["ws"] and 304 in couts["wsp"] and 300 in couts["halo"]
    assert {G.LADDER[n][4] for names in G.FAMILY_CASES.values() for n in names} == {0, 1, 2}
