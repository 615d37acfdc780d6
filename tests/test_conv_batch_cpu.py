"""CPU-side checks of the batched split-family convolution's entry point, ndet_conv_split_batch (csrc/conv_split_kernels.hip; the layers of
mmdet3d/models/necks/imvoxelnet.py:36-67,233-260 and dense_heads/imvoxel_head_v2.py:45-49 for several scenes in one launch): the header, the
ctypes table and the library agree on the symbol, every refusal comes back with its error code before any HIP call (this file runs without a
GPU: a block that got past the checks would try to launch), and conv_tiles.resolve sends a batch away from the persistent tiles only."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERSISTENT = (129256, 129257, 129064)


def test_header_ctypes_table_and_library_agree_on_the_symbol():
    from nerfdet_amd import _lib
    lib = _lib.load()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nerfdet_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+ndet_conv_split_batch\s*\(\s*const\s+NdetConvArgs\s*\*\s*a\s*,\s*int\s+batch\s*,\s*void\s*\*\s*stream\s*\)\s*;", txt)
    argtypes, restype = _lib.SIGNATURES["ndet_conv_split_batch"]
    assert argtypes == [ctypes.POINTER(_lib.NdetConvArgs), ctypes.c_int, ctypes.c_void_p] and restype is ctypes.c_int
    assert hasattr(lib, "ndet_conv_split_batch")
    assert lib.ndet_version() == 110, "an added entry point does not move the ABI version"
    assert _lib.NdetConvArgs._fields_[-1][0] == "map_out", "the block is ndet_conv_split's, unchanged: the batch travels beside it"


def _call(batch, **fields):
    from nerfdet_amd import _lib
    block = dict(size=ctypes.sizeof(_lib.NdetConvArgs), in_=0x1000, w_planes=0x1000, out=0x1000, D=4, H=6, W=5, Cin=64, Cout=256, kernel=(3, 3, 3),
                 stride=(1, 1, 1), pad=(1, 1, 1), tile=128256)
    block.update(fields)
    lib = _lib.load()
    return lib.ndet_conv_split_batch(_lib.NdetConvArgs(**block), batch, None), lib.ndet_last_error().decode()


def test_refusals_come_before_any_hip_call():
    rc, msg = _call(0)
    assert rc == -1 and "batch=0" in msg
    assert _call(-3)[0] == -1
    # what a batch does not take (each of them is fine, or differently checked, with batch == 1)
    for bad in (dict(arith=1, in_amax=0x1000, w_amax=0x1000), dict(keep_partials=1), dict(residual=0x1000, residual_up2=1),
                dict(tile=3256, map_w=0x1000, map_b=0x1000, map_out=0x1000)):
        rc, msg = _call(2, **bad)
        assert rc == -2 and "a batch takes no" in msg, (bad, rc, msg)
    for tile in PERSISTENT:
        rc, msg = _call(2, tile=tile)
        assert rc == -2 and "persistent" in msg, (tile, rc, msg)
    # the rows of the whole batch: 2 x 1024^3 = 2^31
    rc, msg = _call(2, D=1024, H=1024, W=1024, Cin=32, Cout=32, tile=64)
    assert rc == -2 and "too large together" in msg, (rc, msg)
    rc, msg = _call(2, D=512, H=512, W=512, Cin=32, Cout=32, tile=64, transposed=1, kernel=(2, 2, 2), stride=(2, 2, 2), pad=(0, 0, 0))
    assert rc == -2 and "too large" in msg, (rc, msg)
    # the families' 2 GB per operand, over the whole batch: one 64^3 x 512-channel volume is 512 MB, four are 2 GB
    for tile, family in ((128256, "128x256"), (3128, "halo"), (3256, "halo"), (3258, "halo")):
        rc, msg = _call(4, D=64, H=64, W=64, Cin=512, tile=tile)
        assert rc == -2 and family in msg and "2 GB" in msg, (tile, rc, msg)
    # the direct epilogue's 4 GB output, over the whole batch: 16 x 64^3 rows x 256 channels x 4 bytes
    rc, msg = _call(16, D=64, H=64, W=64, Cin=32, tile=100128)
    assert rc == -2 and "direct epilogue" in msg, (rc, msg)
    # the block's own checks still come first, as in ndet_conv_split
    assert _call(2, size=8)[0] == -1
    assert _call(2, in_=None)[0] == -1
    assert _call(2, tile=77)[0] == -1
    assert _call(1, tile=77)[0] == -1


def test_resolve_sends_a_batch_away_from_the_persistent_tiles_only():
    from nerfdet_amd import conv_tiles
    shape = dict(m=3200, cout=256, cin=256, taps=27, transposed=False, halo_ok=True, direct_epilogue=True)
    for tile in conv_tiles.TILES:
        one = conv_tiles.resolve(tile, 2, **shape)
        assert conv_tiles.resolve(tile, 2, batch=1, **shape) == one
        got = conv_tiles.resolve(tile, 2, batch=2, **shape)
        assert got == ((128256, 2) if tile in PERSISTENT else one), (tile, got, one)
    assert all(conv_tiles.TILES[t].family == "wsp" for t in PERSISTENT)
    assert [t for t, row in conv_tiles.TILES.items() if row.family == "wsp"] == list(PERSISTENT)


def test_the_halo_rows_of_the_gpu_test_take_both_geometry_forms():
    """tests/test_conv_batch_gpu.py relies on its halo rows covering both forms of the launcher's halo_geometry; asked of the launcher's own rule
    (ndet_conv_halo_patch), so a change of the cost rule that moves a row to the other form fails here."""
    from nerfdet_amd import _lib
    lib = _lib.load()

    def form(tile, grid):
        patch, looped = (ctypes.c_int * 3)(), ctypes.c_int()
        assert lib.ndet_conv_halo_patch(tile, *grid, (ctypes.c_int * 3)(3, 3, 3), patch, ctypes.byref(looped)) == 0
        return tuple(patch), looped.value
    assert form(3128, (3, 6, 10)) == ((4, 8, 4), 0)                  # depth taps inside the image, 1 x 1 x 3 patches a volume
    for tile in (3256, 3257, 3258):
        assert form(tile, (3, 6, 10)) == ((1, 8, 16), 1)             # looped, 3 depth patches a volume
    assert form(3128, (1, 8, 16)) == ((1, 8, 16), 1)                 # looped, one patch a volume
    assert lib.ndet_conv_halo_patch(128256, 3, 6, 10, (ctypes.c_int * 3)(3, 3, 3), (ctypes.c_int * 3)(), ctypes.byref(ctypes.c_int())) == -1
