"""The host's rule for the refill threshold of the one-lane brute-force kernels (csrc/rt_internal.h
brute_refill_launch, through rt_debug_brute_refill): the R that launch_pick gives its kernel for option
"brute_refill".  Frames are bit-identical whatever R is (tests/test_gpu_brute_refill.py), so only this file
notices a rule that turns the headline's threshold off, or one that turns it on for the small tiles."""
import pytest

from ensem3a_openclraytracer_amd import _native

LANES = 5 * 4 * 256 * 64          # MI355X: 5 waves x 4 SIMDs x 256 CUs x 64 lanes of the 96-VGPR kernel
C2 = 1024 * 1024
R_AUTO = 4                        # kRefillBrute


def rule(nloc, lanes=LANES, option=-1):
    return _native.brute_refill(nloc, lanes, option)


def restated(nloc, lanes, option):
    """The rule again, in Python."""
    if option >= 0:
        return min(option, 64) if option >= 2 else 0
    return R_AUTO if 2 * nloc >= 3 * lanes else 0


def test_c2_and_its_row_tiles():
    assert LANES == 327680
    assert rule(C2) == R_AUTO                 # 3.2 pixels per lane
    assert rule(C2 // 2) == R_AUTO            # rows 0::2, 1.6 per lane
    # rows 0::3 (1.07 per lane), 0::4, 0::8 and C1's frame: every free lane refilled at once, as before
    for nloc in (342 * 1024, C2 // 4, C2 // 8, 256 * 256, 96 * 96, 1):
        assert rule(nloc) == 0, nloc


def test_boundary_is_one_and_a_half_pixels_per_lane():
    assert rule(3 * LANES // 2) == R_AUTO
    assert rule(3 * LANES // 2 - 1) == 0
    assert rule(3, lanes=2) == R_AUTO and rule(2, lanes=2) == 0
    assert rule(0) == 0
    # the boundary the sample slices use (tests/test_brute_slices_rule.py)
    for nloc in (3 * LANES // 2 - 1, 3 * LANES // 2, C2, C2 // 4):
        assert (rule(nloc) > 0) == _native.brute_slices(nloc, LANES, 64)[0], nloc


def test_forced_values_hold_on_any_tile():
    for nloc in (C2, C2 // 8, 32 * 32, 1, 0):
        for r in (2, 3, 4, 6, 63, 64):
            assert rule(nloc, option=r) == r, (nloc, r)


def test_zero_and_one_mean_off():
    for nloc in (C2, C2 // 8, 1):
        assert rule(nloc, option=0) == 0
        assert rule(nloc, option=1) == 0


def test_matches_the_restated_rule():
    for lanes in (LANES, 4 * 4 * 256 * 64, 64, 1):
        for nloc in (0, 1, 63, 64, 96, 97, 3 * lanes // 2 - 1, 3 * lanes // 2, 3 * lanes // 2 + 1, 2 * lanes, C2):
            for option in (-1, 0, 1, 2, 4, 64):
                assert rule(nloc, lanes, option) == restated(nloc, lanes, option), (nloc, lanes, option)


def test_bad_arguments():
    for bad in (-2, 65):
        with pytest.raises(_native.NativeError):
            rule(C2, option=bad)
    with pytest.raises(_native.NativeError):
        rule(-1)
