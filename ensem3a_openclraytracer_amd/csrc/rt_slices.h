// The host's rule for sample slices on brute-force scenes (option "slices"; the one-lane kernels of
// rt_kernels.hip render_kernel).  Plain C++: rt_api.hip (setup_slices) makes the offer, rt_kernels.hip
// (launch_pick) decides where it knows its kernel's resident lanes, and rt_debug_brute_slices evaluates both
// for tests/test_brute_slices_rule.py.  Frames do not depend on any of it; the frame time does.
#pragma once
#include <algorithm>
#include <cstdint>

namespace rt {

// K on auto.  C2 r09, the last two pixels per lane in K = 3 / 4 / 5 / 6 / 8 slices:
// 6.63 / 6.57 / 6.59 / 6.67 / 7.00 ms
constexpr int kSlicesBrute = 4;
// an add of a progressive accumulation on auto: slices of at least this many samples (below that the
// hand-offs cost more than the shorter tail gives back)
constexpr int kAccumSliceMin = 8;

// What setup_slices offers a launch that runs `todo` samples per pixel: K for a set slice count, -K for K on
// auto, 0 for none.  Every slice at least two samples; accum: an add, under the kAccumSliceMin rule on auto.
inline int brute_slice_offer(int option, int todo, bool accum) {
    if (option == 0) return 0;
    int k = option > 0 ? option : kSlicesBrute;
    k = std::min(k, todo / 2);
    if (accum && option < 0) k = std::min(k, todo / kAccumSliceMin);
    if (k <= 1) return 0;
    return option < 0 ? -k : k;
}

// Auto: tiles of at least 1.5 pixels per resident lane.  Measured on C2 row tiles 0::N (r09, DESIGN.md 5.2;
// ms, off / on): N=1 (3.2 pixels per lane) 7.03 / 6.57, N=2 (1.6) 4.27 / 3.81, N=3 (1.07) 3.15 / 3.50, N=4 (0.8)
// 2.78 / 3.09: near one pixel per lane slice k + 1 of a pixel is taken while its slice k still runs, and the
// job waits
inline bool brute_auto_slices(int64_t nloc, int64_t lanes) { return 2 * nloc >= 3 * lanes; }

// ... and the share of the tile's pixels they slice, in 1/256 (1..256, rounded up): the last two pixels per
// resident lane.  Every sliced pixel pays its hand-offs, but only the last ones shorten the frame's end; with
// too few of them the jobs wait for their predecessors again (C2, K = 4, pixels per lane sliced 1.5 / 1.75 /
// 2 / 2.25 / 2.5 / all 3.2: 6.82 / 6.65 / 6.57 / 6.61 / 6.61 / 6.75 ms)
inline int brute_slice_tail(int64_t nloc, int64_t lanes) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(256, (2 * 256 * lanes + nloc - 1) / std::max<int64_t>(nloc, 1)));
}

// What launch_pick makes of the offer on a tile of nloc pixels with `lanes` resident lanes: FrameParams::slices as
// the sliced kernels read it, K | tail << 8 (a set slice count slices every pixel: tail 256), or 0 for an
// unsliced launch
inline int brute_slice_launch(int offer, int64_t nloc, int64_t lanes) {
    const int k = offer < 0 ? -offer : offer;
    if (k <= 1 || (offer < 0 && !brute_auto_slices(nloc, lanes))) return 0;
    return k | ((offer < 0 ? brute_slice_tail(nloc, lanes) : 256) << 8);
}

}  // namespace rt
