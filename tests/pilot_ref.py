"""The two-pass scheduler's decisions, restated in plain integer arithmetic (include/rt_debug.h states the same
steps for rt_debug_pilot_order and rt_debug_pilot_pick; DESIGN.md, "Two passes ordered by a pilot").

The order of pass 2 over a tile of n pixels, from the rays each pixel traced in pass 1 (``cost``, 32-bit words):

  * chunks of ``chunk`` consecutive tile pixels, ``nfull = n // chunk`` of them whole; a chunk's cost is the sum of
    its pixels' costs modulo 2^32 (the device sums in 32-bit words);
  * ``top = chunk * pilot * 2 * (max(max_bounce, 0) + 1)``, ``scale = max(1, (levels << 16) // max(top, 1))``,
    ``bin(v) = min(levels - 1, (v * scale) >> 16)`` with the product in 64 bits;
  * the whole chunks by bin, descending; chunks of one bin keep their tile order (a stable sort);
  * a chunk's pixels in tile order; the pixels past ``nfull * chunk`` stay in place; ``nfull == 0``: the identity.

The pick of pass 2's kernel, from the pixels pass 1 left (``left``, the non-zero costs) and the resident lanes.

Python ints carry the 64-bit products; numpy carries the arrays.  Nothing here calls the native library.
"""
import numpy as np

SPEC_PICK = 10   # rt_internal.h kSpecPick (tests/test_pilot_ref.py checks it against the header)

# what the entry points accept (rt_debug.h): the ranges of the options and of a frame's maxBounce
CHUNK_MAX = 4096
PILOT_MAX = 1 << 20
BOUNCE_MAX = 4096


def check_order_args(n, chunk, levels, pilot, max_bounce):
    """ValueError for the arguments rt_debug_pilot_order rejects."""
    if n <= 0 or n > 0x7fffffff:
        raise ValueError(f"n {n}")
    if chunk < 1 or chunk > CHUNK_MAX:
        raise ValueError(f"chunk {chunk}")
    if levels < 2 or levels > 256:
        raise ValueError(f"levels {levels}")
    if pilot < 1 or pilot > PILOT_MAX:
        raise ValueError(f"pilot {pilot}")
    if max_bounce > BOUNCE_MAX:
        raise ValueError(f"max_bounce {max_bounce}")


def top_of(chunk, pilot, max_bounce):
    return int(chunk) * int(pilot) * 2 * (max(int(max_bounce), 0) + 1)


def scale_of(levels, top):
    return max(1, (int(levels) << 16) // max(int(top), 1))


def chunk_costs(cost, chunk):
    """The whole chunks' costs, modulo 2^32 (uint64 sums of at most 4096 32-bit words cannot overflow)."""
    c = np.asarray(cost, dtype=np.uint32).astype(np.uint64)
    nfull = c.size // chunk
    return (c[: nfull * chunk].reshape(nfull, chunk).sum(axis=1) & np.uint64(0xFFFFFFFF)).astype(np.uint64)


def bins_of(ccost, levels, scale):
    """bin(v) per chunk cost, with Python ints: v < 2^32 and scale <= 2^24, so the product needs up to 56 bits."""
    return np.array([min(levels - 1, (int(v) * scale) >> 16) for v in ccost], dtype=np.int64)


def chunk_bins(cost, chunk, levels, pilot, max_bounce):
    n = int(np.asarray(cost).size)
    check_order_args(n, chunk, levels, pilot, max_bounce)
    return bins_of(chunk_costs(cost, chunk), levels, scale_of(levels, top_of(chunk, pilot, max_bounce)))


def order(cost, chunk, levels, pilot, max_bounce):
    """The pass-2 pixel order, uint32[n]: order[q] is the tile pixel started q-th."""
    n = int(np.asarray(cost).size)
    b = chunk_bins(cost, chunk, levels, pilot, max_bounce)
    nfull = n // chunk
    out = np.arange(n, dtype=np.int64)
    if nfull == 0:
        return out.astype(np.uint32)
    # a counting sort, written as one: the bins from the top down, each bin's chunks as they come
    corder = np.concatenate([np.flatnonzero(b == v) for v in range(levels - 1, -1, -1)])
    out[: nfull * chunk] = (corder[:, None] * chunk + np.arange(chunk)[None, :]).reshape(-1)
    return out.astype(np.uint32)


def left_of(cost):
    return int(np.count_nonzero(np.asarray(cost, dtype=np.uint32)))


def check_pick_args(n, lanes, spec):
    """ValueError for the arguments rt_debug_pilot_pick rejects."""
    if n <= 0 or n > 0x7fffffff:
        raise ValueError(f"n {n}")
    if lanes < 1:
        raise ValueError(f"lanes {lanes}")
    if spec not in (0, 1):
        raise ValueError(f"spec {spec}")


def pick(left, lanes, spec):
    """The pick word: lanes per pixel 4 at <= 1/2 unfinished pixel per resident lane, 2 at <= 1, else 1; with trails
    available (spec) and a team to replace, SPEC_PICK + trails: 8 at <= 1/4 pixel per lane, else the team's size."""
    left, lanes = int(left), int(lanes)
    u4 = 4 * left
    k = 4 if u4 <= 2 * lanes else 2 if u4 <= 4 * lanes else 1
    if spec and k > 1:
        return SPEC_PICK + (8 if u4 <= lanes else k)
    return k
