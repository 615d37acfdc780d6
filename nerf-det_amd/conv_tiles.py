"""The tile ids of the split-family convolution (NdetConvArgs::tile) as data: the host's copy of the table CONV_TILES of
csrc/conv_split_kernels.hip (tests/test_abi_cpu.py holds the two against each other through ndet_conv_tile_info), and the rules that turn a
chosen tile into one the layer can run.  Pure Python: no tensor, no GPU."""
from __future__ import annotations

from typing import NamedTuple, Optional

DIRECT, OWNS_ROWS, ORDER2 = 1, 2, 4     # NDET_TILE_* of include/nerfdet_hip.h


class Tile(NamedTuple):
    rows: int               # GEMM rows (voxels / pixels) x
    cols: int               # ... output channels of a workgroup's tile
    family: str             # "unified", "ws" (wave-specialised), "wsp" (its persistent form), "halo" (halo-stationary)
    flags: int              # DIRECT: the epilogue stores straight from the accumulators (final values only: no split-K); OWNS_ROWS: one tile holds all
                            # 256 channels of its rows (the chained projection is allowed); ORDER2: may take the activation-stationary workgroup order
    partner: Optional[int]  # the direct form of a staged unified tile and the other way round
    name: str               # the kernel, as bench.py keys its per-kernel rooflines


TILES = {
    64: Tile(64, 64, "unified", ORDER2, 100064, "k_conv_split<64,64,2,2>"),
    128: Tile(128, 128, "unified", ORDER2, 100128, "k_conv_split<128,128,2,2>"),
    12864: Tile(128, 64, "unified", ORDER2, 112864, "k_conv_split<128,64,2,2>"),
    128256: Tile(128, 256, "ws", ORDER2, None, "k_conv_split_ws"),
    129256: Tile(128, 256, "wsp", 0, None, "k_conv_split_wsp<128>"),
    129257: Tile(128, 256, "wsp", 0, None, "k_conv_split_wsp<128,8>"),       # eight consumer waves
    129064: Tile(64, 256, "wsp", 0, None, "k_conv_split_wsp<64>"),
    3128: Tile(128, 128, "halo", 0, None, "k_conv_split_halo<4,2>"),
    3256: Tile(128, 256, "halo", OWNS_ROWS, None, "k_conv_split_halo<8,2>"),
    3257: Tile(128, 256, "halo", OWNS_ROWS, None, "k_conv_split_halo<4,4>"),  # two consumer waves per SIMD
    3258: Tile(128, 256, "halo", OWNS_ROWS, None, "k_conv_split_halo<4,4,p8>"),   # ... and eight producer waves
    100064: Tile(64, 64, "unified", ORDER2 | DIRECT, 64, "k_conv_split<64,64,2,2>"),
    100128: Tile(128, 128, "unified", ORDER2 | DIRECT, 128, "k_conv_split<128,128,2,2>"),
    112864: Tile(128, 64, "unified", ORDER2 | DIRECT, 12864, "k_conv_split<128,64,2,2>"),
}
SPLIT_IDS = tuple(TILES)
F32_IDS = (64, 128)     # the fp32-MFMA family (csrc/conv3d_kernels.hip) has its own two tiles


def ids(*families: str, direct: bool = False):
    """The ids of the given families in table order; the direct forms (which resolve() promotes to by itself) only on request."""
    return tuple(t for t, row in TILES.items() if row.family in families and (direct or not row.flags & DIRECT))


def is_direct(tile: int) -> bool:
    return tile in TILES and bool(TILES[tile].flags & DIRECT)


def owns_rows(tile: int) -> bool:
    return tile in TILES and bool(TILES[tile].flags & OWNS_ROWS)


def resolve(tile: int, splits: int, *, m: int, cout: int, cin: int, taps: int, transposed: bool, halo_ok: bool, direct_epilogue: bool = True,
            batch: int = 1):
    """(tile, splits) the layer runs when the tables / the caller name ``tile``: what a family does not take goes to the nearest tile that does (the
    library itself rejects such a request: the NDET_REQUIREs of each split_launch_*).  ``halo_ok``: stride 1, odd same-padded kernel, more than one
    tap.  ``batch``: volumes in the launch (ndet_conv_split_batch; ``m`` counts the rows of all of them).  An id outside the table is left for the
    library to reject."""
    row = TILES.get(tile)
    if row is None:
        return tile, splits
    if row.family == "halo":        # stride-1 same-padded multi-tap convolutions only, K split over the channel chunks
        if not halo_ok:
            tile = 128256 if cout > 128 else 128
        else:
            splits = min(splits, cin // 32)
    elif row.family == "wsp" and (transposed or cout % 16 or taps > 32 or batch > 1):
        tile = 128256               # the persistent form takes plain convolutions with Cout % 16 == 0, one volume per launch
    row = TILES[tile]
    if row.family == "unified":
        # unified tiles that write final values: the epilogue straight from the MFMA's C layout (no LDS staging, no barriers)
        staged = row.partner if row.flags & DIRECT else tile
        direct_ok = splits == 1 and not transposed and cout % 32 == 0 and (m + 128) * cout * 4 < (1 << 32)
        tile = TILES[staged].partner if (direct_ok and direct_epilogue) else staged
    return tile, splits
