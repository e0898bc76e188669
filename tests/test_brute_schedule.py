"""Which slots the lock-step walks of the brute-force kernels test (rt_device.h trace_brute_compact), restated in
numpy on the host tables: the clustered loop walks its single slots and a cluster's members in whole groups of 4
and then the last 1-3 alone, so it visits every real slot once and no padding slot; the unclustered loop walks
brute_box in whole groups, padding included.  A single table of singles and union slots walked together was built
and measured slower; it is not in the tree, and rt_debug_brute_clusters is what the kernels read."""
import numpy as np
import pytest

from ensem3a_openclraytracer_amd import _native
from tests.test_brute_clusters import GPU_SOUPS, MODES, SLOTS, _args, _row_ints
from tests.test_malformed_inputs import BRUTE_SCENES, _brute_scene

GROUP = 4            # rt_layout.h kBoxGroup
SCENES = BRUTE_SCENES + GPU_SOUPS + [(4, 40)]     # (4, 40), auto: three single slots


def _tables(which, mode):
    sc = _brute_scene(which)
    base, nbox, nbrute = _native.brute_layout(*_args(sc))
    slots, rows, nsingle = _native.brute_clusters(*_args(sc), MODES[mode])
    return base, nbox, slots, rows, nsingle


def _walk(gb, ge):
    """`lockstep`: the (first slot, width) pieces in which slots [gb, ge) are loaded and tested."""
    out, g0 = [], gb
    while g0 + GROUP <= ge:
        out.append((g0, GROUP))
        g0 += GROUP
    rem = ge - g0
    if rem & 2:
        out.append((g0 + (rem & ~3), 2))
    if rem & 1:
        out.append((g0 + (rem & ~1), 1))
    return out


def _walk_padded(gb, ge):
    """`lockstep_padded`: whole groups."""
    return [(g0, GROUP) for g0 in range(gb, ge, GROUP)]


def _visits(pieces, size):
    n = np.zeros(size, int)
    for g, w in pieces:
        assert w in (1, 2, GROUP) and 0 <= g and g + w <= size, (g, w, size)    # a load never leaves the array
        n[g:g + w] += 1
    return n


@pytest.mark.parametrize("n", range(0, 19))
def test_walk_pieces(n):
    for gb in (0, 4, 12):
        pieces = _walk(gb, gb + n)
        assert (_visits(pieces, gb + n + 3)[gb:gb + n] == 1).all() and sum(w for _, w in pieces) == n
        assert len(pieces) == n // GROUP + bin(n % GROUP).count("1")        # one scalar wait each
        assert [w for _, w in pieces] == sorted((w for _, w in pieces), reverse=True)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("which", SCENES, ids=str)
def test_walks_visit_each_real_slot_once(which, mode):
    base, nbox, slots, rows, nsingle = _tables(which, mode)
    # the unclustered loop: every slot of the padded array once
    assert (_visits(_walk_padded(0, nbox), len(base)) == 1).all()
    if len(rows) == 0:
        return
    first, count = _row_ints(rows)
    pad = (slots[:, :6] == np.float32(1e30)).all(1)
    # the clustered loop's singles, and each cluster's members where its wave takes the lock-step branch
    n = _visits(_walk(0, nsingle), len(slots))
    for f, c in zip(first, count):
        assert f % GROUP == 0 and 2 <= c <= SLOTS
        n += _visits(_walk(f, f + c), len(slots))
    assert (n[~pad] == 1).all() and (n[pad] == 0).all()
    assert n.sum() == nbox


def test_scenes_cover_every_tail_length():
    singles, members = {}, {}
    for which in SCENES:
        for mode in MODES:
            base, nbox, slots, rows, nsingle = _tables(which, mode)
            if len(rows):
                singles.setdefault(nsingle % GROUP, (which, mode))
                for c in _row_ints(rows)[1]:
                    members.setdefault(int(c) % GROUP, (which, mode))
    assert sorted(singles) == [0, 1, 2, 3], singles
    assert sorted(members) == [0, 1, 2, 3], members
    # the frames the GPU tests render: C2 by default (tests/test_gpu_parity.py; 6 singles, a group and a pair) ...
    base, nbox, slots, rows, nsingle = _tables("cornell", "auto")
    assert nsingle == 6 and _row_ints(rows)[1].tolist() == [8, 8] and nbox % GROUP == 2
    # ... and these four, forced (tests/test_gpu_brute_schedule.py): clusters of every tail length, a lone single,
    # and box counts of every remainder for the unclustered kernel
    seen, boxes = set(), set()
    for which in ["cornell", (11, 23), (2, 64), (9, 33)]:
        base, nbox, slots, rows, nsingle = _tables(which, "force")
        assert nsingle in (0, 1)
        seen |= set((_row_ints(rows)[1] % GROUP).tolist())
        boxes.add(nbox % GROUP)
    assert seen == {0, 1, 2, 3} and boxes == {0, 1, 2, 3}
