"""Host side of the three-taps-per-interval walk of tile 3128 (csrc/conv_split_kernels.hip: halo_tps, halo_walk_lds behind ndet_conv_halo_taps; the
launcher of the convolutions of mmdet3d/models/necks/imvoxelnet.py:36-67): which walk a launch takes, what LDS it asks for, and the test-support
switch that forces the one-tap walk.  No HIP call is made."""
import ctypes

import pytest

CU_LDS = 160 * 1024
BF16X3, F16X2, BF16 = 0, 1, 2


def _query(lib, mode, tile, arith, tin):
    taps, lds = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.ndet_conv_halo_taps(mode, tile, arith, tin, ctypes.byref(taps), ctypes.byref(lds))
    return rc, taps.value, lds.value


@pytest.fixture
def lib():
    from nerfdet_amd import _lib
    lib = _lib.load()
    yield lib
    assert lib.ndet_conv_halo_taps(0, 0, 0, 0, None, None) == 0     # automatic again, whatever the test did


def test_taps_rule_follows_the_taps_per_image(lib):
    # Tin: 3x3 = 9, 3x3x3 inside the image = 27, looped outside it = 9, 3x1x3 = 9, 1x5x1 = 5
    for arith in (F16X2, BF16):
        for tin, want in ((9, 3), (27, 3), (3, 3), (5, 1), (25, 1), (1, 1), (7, 1)):
            assert _query(lib, -1, 3128, arith, tin)[:2] == (0, want), (arith, tin)
    for tin in (9, 27, 5):
        assert _query(lib, -1, 3128, BF16X3, tin)[:2] == (0, 1)          # three planes: 224 KB at three taps
        for tile in (3256, 3257, 3258):                                  # the 256-column tiles' LDS is full
            for arith in (BF16X3, F16X2, BF16):
                assert _query(lib, -1, tile, arith, tin)[:2] == (0, 1)


def test_lds_request_fits_a_cu(lib):
    # image planes x 400 rows x 32 channels x 2 B + weight stages x taps x planes x 128 x 32 x 2 B
    assert _query(lib, -1, 3128, F16X2, 9) == (0, 3, 2 * 400 * 64 + 2 * 3 * 2 * 128 * 64) == (0, 3, 149504)
    assert _query(lib, -1, 3128, BF16, 27) == (0, 3, 400 * 64 + 2 * 3 * 128 * 64)
    assert _query(lib, -1, 3128, F16X2, 5) == (0, 1, 2 * 400 * 64 + 3 * 2 * 128 * 64)      # the one-tap walk: three one-tap stages, as before
    assert _query(lib, -1, 3128, BF16X3, 9) == (0, 1, 3 * 400 * 64 + 3 * 3 * 128 * 64)
    assert _query(lib, -1, 3256, F16X2, 9) == (0, 1, 2 * 224 * 64 + 2 * 2 * 256 * 64)
    for tile in (3128, 3256, 3257, 3258):
        for arith in (BF16X3, F16X2, BF16):
            for tin in (9, 27, 5):
                assert 0 < _query(lib, -1, tile, arith, tin)[2] <= CU_LDS


def test_switch_forces_one_tap_and_is_left_by_a_query(lib):
    assert _query(lib, 1, 3128, F16X2, 9)[:2] == (0, 1)
    assert _query(lib, -1, 3128, F16X2, 27)[:2] == (0, 1)        # -1 leaves the switch
    assert _query(lib, -1, 3128, BF16, 9) == (0, 1, 400 * 64 + 3 * 128 * 64)
    assert lib.ndet_conv_halo_taps(0, 0, 0, 0, None, None) == 0  # no query: tile / arith / taps are not looked at
    assert _query(lib, -1, 3128, F16X2, 27)[:2] == (0, 3)


def test_bad_arguments(lib):
    assert lib.ndet_conv_halo_taps(2, 0, 0, 0, None, None) == -1 and lib.ndet_conv_halo_taps(-2, 0, 0, 0, None, None) == -1
    assert _query(lib, -1, 128256, F16X2, 9)[0] == -1 and b"not a halo tile" in lib.ndet_last_error()
    assert _query(lib, -1, 3128, 3, 9)[0] == -1 and _query(lib, -1, 3128, F16X2, 0)[0] == -1
    assert _query(lib, 1, 3128, 7, 9)[0] == -1                   # a refused call leaves the switch
    assert _query(lib, -1, 3128, F16X2, 9)[:2] == (0, 3)
