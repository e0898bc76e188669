"""The host's rule for sample slices on brute-force scenes (csrc/rt_slices.h, through rt_debug_brute_slices): what
setup_slices offers a launch and what launch_pick makes of it, on the host alone.  Frames are bit-identical whether
or not slices are taken and whatever share of the pixels is sliced, so only this file notices a rule that turns
the headline's slices off, or one that slices every pixel of the frame."""
import pytest

from ensem3a_openclraytracer_amd import _native

LANES = 5 * 4 * 256 * 64          # MI355X: 5 waves x 4 SIMDs x 256 CUs x 64 lanes of the 96-VGPR kernel
C2 = 1024 * 1024
OFF = (False, 0, 0)


def rule(nloc, lanes=LANES, spp=64, option=-1, accum_base=-1):
    return _native.brute_slices(nloc, lanes, spp, option, accum_base)


def test_c2_and_its_row_tiles():
    assert LANES == 327680
    # the whole frame: 3.2 pixels per lane; the last two per lane are ceil(256 x 2 x 327680 / 1048576) = 160 / 256
    assert rule(C2) == (True, 4, 160)
    # rows 0::2, 1.6 pixels per lane: two per lane is more than the tile has, so every pixel
    assert rule(C2 // 2) == (True, 4, 256)
    # rows 0::3 (342 rows, 1.07 per lane), 0::4, 0::8 and C1's frame: measured slower with slices
    for nloc in (342 * 1024, C2 // 4, C2 // 8, 256 * 256):
        assert rule(nloc) == OFF, nloc


def test_threshold_is_one_and_a_half_pixels_per_lane():
    assert rule(3 * LANES // 2) == (True, 4, 256)
    assert rule(3 * LANES // 2 - 1) == OFF
    assert rule(3, lanes=2) == (True, 4, 256) and rule(2, lanes=2) == OFF
    assert rule(0) == OFF and rule(1, lanes=0)[0]


def test_tail_share_rounds_up_and_clamps():
    # two pixels per lane of nloc, in 1/256, rounded up, within 1..256
    for nloc in (2 * LANES, 2 * LANES + 1, 3 * LANES, C2, 1024 * 704, 5 * LANES, 512 * LANES, 513 * LANES, 10 ** 12):
        on, k, tail = rule(nloc)
        want = min(256, max(1, -(-512 * LANES // nloc)))
        assert (on, k, tail) == (True, 4, want), nloc
    assert rule(2 * LANES)[2] == 256 and rule(2 * LANES + 1)[2] == 256 and rule(2 * LANES + 2600)[2] == 255
    assert rule(1024 * 704)[2] == 233
    assert rule(512 * LANES)[2] == 1 and rule(10 ** 12)[2] == 1          # never 0: at least 1 / 256 of the pixels
    assert rule(5, lanes=0) == (True, 4, 1)


def test_every_slice_at_least_two_samples():
    assert rule(C2, spp=8)[1] == 4
    assert rule(C2, spp=7)[1] == 3
    assert rule(C2, spp=4) == (True, 2, 160)
    assert rule(C2, spp=3) == OFF and rule(C2, spp=1) == OFF and rule(C2, spp=0) == OFF
    assert rule(C2, spp=3, option=8) == OFF


def test_a_set_slice_count_slices_every_pixel_of_any_tile():
    for nloc in (C2, 32 * 32, 1):
        assert rule(nloc, option=8) == (True, 8, 256)
        assert rule(nloc, option=16, spp=13) == (True, 6, 256)
        assert rule(nloc, option=5, spp=13) == (True, 5, 256)
    assert rule(C2, option=1) == OFF       # one slice is no slice
    assert rule(C2, option=0) == OFF
    for bad in (-2, 17):
        with pytest.raises(_native.NativeError):
            rule(C2, option=bad)


def test_adds_of_a_progressive_accumulation():
    # auto: slices of at least kAccumSliceMin = 8 samples of the samples the add runs (spp - accum_base)
    assert rule(C2, spp=64, accum_base=0) == (True, 4, 160)
    assert rule(C2, spp=64, accum_base=32) == (True, 4, 160)      # 32 samples: 4 slices of 8
    assert rule(C2, spp=64, accum_base=40) == (True, 3, 160)      # 24: 3 of 8
    assert rule(C2, spp=64, accum_base=48) == (True, 2, 160)      # 16: 2 of 8
    assert rule(C2, spp=64, accum_base=49) == OFF                 # 15: one slice
    assert rule(C2, spp=64, accum_base=60) == OFF
    # a one-shot frame of 15 samples is not under that rule
    assert rule(C2, spp=15) == (True, 4, 160)
    # a set slice count: only the two-sample bound
    assert rule(C2, spp=64, option=8, accum_base=48) == (True, 8, 256)
    assert rule(C2, spp=64, option=8, accum_base=60) == (True, 2, 256)
    assert rule(C2, spp=64, option=8, accum_base=61) == OFF
