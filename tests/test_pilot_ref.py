"""tests/pilot_ref.py, the restatement of the two-pass scheduler's order and pick, against an independent
construction of the same definition (no GPU): Python's stable sort with the key the definition names.  The GPU
tests (tests/test_gpu_pilot_order.py) hold the device to the restatement; these hold the restatement to the
definition, so that the two cannot be wrong together without one of the files saying so."""
import os
import re

import numpy as np
import pytest

from ensem3a_openclraytracer_amd import _native
from tests import pilot_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, chunk, levels, pilot, max_bounce): sizes around the sort's 256-chunk segments, chunks that do not divide n,
# a chunk larger than n, few and many bins
SHAPES = [(1, 1, 2, 1, 0), (63, 7, 33, 2, 4), (63, 64, 256, 1, 4), (255, 1, 256, 1, 4), (256, 1, 2, 3, 1),
          (257, 1, 33, 1, 4), (257, 100, 256, 2, 4), (4099, 7, 33, 1, 8), (4099, 64, 256, 4, 4),
          (1792, 7, 256, 1, 4), (1799, 7, 2, 1, 4), (66000, 1, 256, 1, 4)]


def _costs(n, top, kind, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "zero":
        return np.zeros(n, np.uint32)
    if kind == "equal":
        return np.full(n, 3, np.uint32)
    if kind == "up":
        return np.arange(n, dtype=np.uint32)
    if kind == "down":
        return np.arange(n, 0, -1).astype(np.uint32)
    if kind == "random":
        return rng.integers(0, top + 1, n).astype(np.uint32)
    if kind == "saturate":
        return rng.integers(0, 4 * top + 1, n).astype(np.uint32)
    if kind == "huge":
        c = rng.integers(0, top + 1, n).astype(np.uint32)
        c[rng.random(n) < 0.3] = 0xFFFFFFFF
        return c
    raise KeyError(kind)


KINDS = ["zero", "equal", "up", "down", "random", "saturate", "huge"]


def _independent(cost, chunk, levels, pilot, max_bounce):
    """The definition, with Python ints and sorted(): chunk sums mod 2^32, the bin formula, the sort key."""
    cost = [int(v) for v in cost]
    n = len(cost)
    nfull = n // chunk
    top = chunk * pilot * 2 * (max(max_bounce, 0) + 1)
    scale = max(1, (levels << 16) // max(top, 1))
    csum = [sum(cost[c * chunk:(c + 1) * chunk]) % (1 << 32) for c in range(nfull)]
    b = [min(levels - 1, (v * scale) >> 16) for v in csum]
    chunks = sorted(range(nfull), key=lambda c: (-b[c], c))
    px = [c * chunk + k for c in chunks for k in range(chunk)] + list(range(nfull * chunk, n))
    return np.array(px, dtype=np.uint32), b


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_c%d_l%d_k%d_b%d" % s)
def test_order_is_the_sorted_definition(shape, kind):
    n, chunk, levels, pilot, mb = shape
    cost = _costs(n, P.top_of(chunk, pilot, mb) // chunk, kind, seed=n + chunk)
    got = P.order(cost, chunk, levels, pilot, mb)
    want, b = _independent(cost, chunk, levels, pilot, mb)
    assert got.dtype == np.uint32
    np.testing.assert_array_equal(got, want)
    # a permutation of the tile
    np.testing.assert_array_equal(np.sort(got), np.arange(n, dtype=np.uint32))
    # bins never rise along the order's whole chunks, and the tail is in place
    nfull = n // chunk
    np.testing.assert_array_equal(P.chunk_bins(cost, chunk, levels, pilot, mb), np.array(b, dtype=np.int64))
    if nfull:
        along = np.array(b)[got[: nfull * chunk:chunk] // chunk]
        assert np.all(np.diff(along) <= 0)
        assert along.max() <= levels - 1 and along.min() >= 0
    np.testing.assert_array_equal(got[nfull * chunk:], np.arange(nfull * chunk, n, dtype=np.uint32))
    # pixels of a chunk stay together, in tile order
    if nfull:
        block = got[: nfull * chunk].reshape(nfull, chunk).astype(np.int64)
        assert np.all(block[:, 0] % chunk == 0)
        np.testing.assert_array_equal(block - block[:, :1], np.tile(np.arange(chunk), (nfull, 1)))


def test_order_edges():
    # equal costs: the identity (stability); no whole chunk: the identity
    np.testing.assert_array_equal(P.order(np.full(1000, 5, np.uint32), 1, 256, 1, 4), np.arange(1000))
    np.testing.assert_array_equal(P.order(np.arange(63, dtype=np.uint32), 64, 256, 1, 4), np.arange(63))
    # descending costs, one pixel per chunk, a bin per cost: the identity; ascending: reversed
    top = P.top_of(1, 1, 4)   # 10
    assert top == 10 and P.scale_of(256, top) == (256 << 16) // 10
    down = np.arange(10, 0, -1).astype(np.uint32)
    np.testing.assert_array_equal(P.order(down, 1, 256, 1, 4), np.arange(10))
    np.testing.assert_array_equal(P.order(down[::-1].copy(), 1, 256, 1, 4), np.arange(9, -1, -1))
    # two bins (scale 13107: 5 * 13107 = 65535 is still bin 0, 6 is bin 1), each group in tile order, and a cost
    # past top saturates
    c = np.array([1, 9, 2, 6, 10, 0, 40, 5], np.uint32)
    np.testing.assert_array_equal(P.order(c, 1, 2, 1, 4), [1, 3, 4, 6, 0, 2, 5, 7])
    # sums wrap: 64 words of 2^26 + 1 are 2^32 + 64 -> 64
    w = np.full(64, (1 << 26) + 1, np.uint32)
    assert int(P.chunk_costs(w, 64)[0]) == 64
    # the 64-bit product: 0xFFFFFFFF * scale does not wrap into a low bin
    assert int(P.bins_of(np.array([0xFFFFFFFF], np.uint64), 256, P.scale_of(256, 2))[0]) == 255
    # maxBounce below zero counts as zero
    assert P.top_of(3, 2, -5) == 12


@pytest.mark.parametrize("args", [(0, 1, 256, 1, 4), (-3, 1, 256, 1, 4), (10, 0, 256, 1, 4), (10, -1, 256, 1, 4),
                                  (10, 1, 1, 1, 4), (10, 1, 257, 1, 4), (10, 1, 256, 0, 4), (10, 1, 256, -2, 4),
                                  (10, P.CHUNK_MAX + 1, 256, 1, 4), (10, 1, 256, P.PILOT_MAX + 1, 4),
                                  (10, 1, 256, 1, P.BOUNCE_MAX + 1)])
def test_order_rejects_what_the_entry_point_rejects(args):
    n, chunk, levels, pilot, mb = args
    with pytest.raises(ValueError):
        P.check_order_args(n, chunk, levels, pilot, mb)
    with pytest.raises(ValueError):
        P.order(np.zeros(max(n, 0), np.uint32), chunk, levels, pilot, mb)


def test_pick_rule():
    L = 1024
    # (left, spec 0, spec 1): every threshold on both sides
    table = [(0, 4, 18), (1, 4, 18), (L // 4, 4, 18), (L // 4 + 1, 4, 14), (L // 2, 4, 14), (L // 2 + 1, 2, 12),
             (L, 2, 12), (L + 1, 1, 1), (10 * L, 1, 1)]
    for left, k0, k1 in table:
        assert P.pick(left, L, 0) == k0, left
        assert P.pick(left, L, 1) == k1, left
    # an odd lane count: the comparisons are on 4 left, with no division
    assert P.pick(1, 3, 0) == 4 and P.pick(2, 3, 0) == 2 and P.pick(3, 3, 0) == 2 and P.pick(4, 3, 0) == 1
    assert P.pick(0, 3, 1) == P.SPEC_PICK + 8 and P.pick(1, 3, 1) == P.SPEC_PICK + 4
    assert P.left_of(np.array([0, 3, 0, 0xFFFFFFFF, 1], np.uint32)) == 3
    for bad in [(0, 1024, 0), (5, 0, 0), (5, -1, 1), (5, 1024, 2), (5, 1024, -1)]:
        with pytest.raises(ValueError):
            P.check_pick_args(*bad)
    P.check_pick_args(1, 1, 1)


def test_spec_pick_is_the_headers_constant():
    with open(os.path.join(ROOT, "ensem3a_openclraytracer_amd", "csrc", "rt_internal.h")) as f:
        k = int(re.search(r"constexpr int kSpecPick = (\d+);", f.read()).group(1))
    with open(os.path.join(ROOT, "include", "rt_debug.h")) as f:
        d = int(re.search(r"RT_SPEC_PICK = (\d+)", f.read()).group(1))
    assert k == d == P.SPEC_PICK == _native.SPEC_PICK
